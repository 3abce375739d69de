"""Host side of the inference harness (thermo_nerf_amd.render.Renderer, thermo_nerf_amd.colormaps): colour tables, the
frame-finishing semantics pinned by tests/golden/frame_finish.npz (tools/make_golden_frames.py: matplotlib + numpy), file names,
GIF, camera path — none of which needs a device [REF thermo_nerf/render/renderer.py; REF tests/test_renderer.py]."""
import os

import numpy as np
import pytest

from tests import frame_forms as FF
from tests import helpers
from thermo_nerf_amd import colormaps
from thermo_nerf_amd.render import Renderer
from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", colormaps.NAMES)
def test_tables_are_matplotlibs(name):
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps[name]
    want = np.asarray(cmap.colors) if hasattr(cmap, "colors") else np.asarray(cmap(np.arange(256)))[:, :3]
    assert np.array_equal(colormaps.table_f64(name), want.astype(np.float64))


@pytest.mark.parametrize("name", colormaps.NAMES)
def test_derived_tables(name):
    t = colormaps.table_f64(name)
    assert t.shape == (256, 3) and t.dtype == np.float64 and t.min() >= 0.0 and t.max() <= 1.0
    u8 = colormaps.table_u8(name)
    assert u8.dtype == np.uint8 and np.array_equal(u8, np.trunc(t * 255).astype(np.uint8))
    f32 = colormaps.table_f32(name)
    assert f32.dtype == np.float32 and np.array_equal(f32, t.astype(np.float32))
    with pytest.raises(KeyError):
        colormaps.table_f64("no-such-map")


def test_package_does_not_import_matplotlib():
    import subprocess
    import sys

    code = "import sys, thermo_nerf_amd.colormaps as c, thermo_nerf_amd.render; c.table_u8('magma'); print('matplotlib' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False"


def test_fixture_reproduces_under_the_index_forms():
    """the fixture was made by matplotlib; the documented index form gives the same bytes with the package's tables alone"""
    g = np.load(os.path.join(GOLDEN, "frame_finish.npz"))
    x = g["x"]
    assert x.dtype == np.float32 and x.shape[0] > 3000 and np.isnan(x).any() and np.isinf(x).any()
    assert np.array_equal(FF.scale_form(x), g["scale"])
    for name in ("magma", "turbo"):
        assert np.array_equal(FF.lut_form(x, colormaps.table_u8(name)), g["lut_" + name]), name
    # where the reference's expressions are defined they ARE the fixture
    unit = (x >= 0) & (x <= 1)
    assert np.array_equal((x[unit] * 255).astype(np.uint8), g["scale"][unit])


def _renderer_with_frames(frames):
    model, _, _ = helpers.build("scene", 48)
    r = Renderer(model)
    assert r.model is model
    r._rendered_images = {RM.RGB: frames}  # as REF tests/test_renderer.py:24-29 injects them
    return r


def _frames(count=3, h=24, w=32):
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def test_save_images_names(tmp_path):
    r = _renderer_with_frames(_frames(2))
    r.save_images([RM.RGB], tmp_path / "out")
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["img_00000.jpeg", "img_00001.jpeg"]
    from PIL import Image

    with Image.open(tmp_path / "out" / "img_00001.jpeg") as im:
        assert im.size == (32, 24) and im.mode == "RGB"


def test_save_gif_reads_back(tmp_path):
    frames = _frames(4)
    r = _renderer_with_frames(frames)
    r.save_gif([RM.RGB], 0.05, tmp_path)
    from PIL import Image

    with Image.open(tmp_path / "synthesized_video_img.gif") as im:
        assert im.n_frames == len(frames) and im.size == (32, 24)
        assert im.info["duration"] == 50


def test_missing_modality_raises(tmp_path):
    r = _renderer_with_frames(_frames(1))
    with pytest.raises(KeyError):
        r.save_images([RM.THERMAL], tmp_path)
    with pytest.raises(KeyError):
        r.save_gif([RM.THERMAL], 1, tmp_path)
    # a modality the model's outputs do not hold: the reference's message, before anything is queued on a device
    cams = Renderer.load_cameras(os.path.join(GOLDEN, "camera_path_facade_2.json"), 0.05)
    with pytest.raises(Exception, match="thermal_combined modality does not exist"):
        r.render([RM.THERMAL, RM.THERMAL_COMBINED], cams)


def test_load_cameras():
    cams = Renderer.load_cameras(os.path.join(GOLDEN, "camera_path_facade_2.json"))
    assert cams.size == 96 and cams.camera_to_worlds.shape == (96, 3, 4) and (cams.height, cams.width) == (1080, 1920)
    half = Renderer.load_cameras(os.path.join(GOLDEN, "camera_path_facade_2.json"), 0.5)
    assert (half.height, half.width) == (540, 960) and float(half.fx[0]) == pytest.approx(0.5 * float(cams.fx[0]))


def test_from_checkpoint_loads_the_newest(tmp_path):
    """[REF tests/test_renderer.py:31-44] the model a run directory holds, rebuilt from the config handed in"""
    import torch

    from thermo_nerf_amd import ThermalNerfModelConfig
    from thermo_nerf_amd.checkpoint import save_nerfstudio_checkpoint

    model, sd, _ = helpers.build("scene", 48)
    stale = {k: torch.zeros_like(v) for k, v in model.state_dict().items()}
    torch.save({"step": 10, "pipeline": {"_model." + k: v for k, v in stale.items()}}, tmp_path / "step-000000010.ckpt")
    save_nerfstudio_checkpoint(model, tmp_path / "nerfstudio_models", 2000)
    cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=48, **helpers.SMALL)
    r = Renderer.from_checkpoint(tmp_path, cfg, num_train_data=8, eval_num_rays_per_chunk=8192, device="cpu")
    assert not r.model.training and r.model.config.eval_num_rays_per_chunk == 8192
    assert cfg.eval_num_rays_per_chunk != 8192, "the caller's config is not edited"
    got = r.model.state_dict()
    for k, v in model.state_dict().items():
        assert torch.equal(got[k], v), k
    with pytest.raises(ValueError, match="num_train_data"):
        Renderer.from_checkpoint(tmp_path, cfg, num_train_data=9, device="cpu")
