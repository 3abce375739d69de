"""tn_frame_to_rgb8 and Renderer.render on the device [REF thermo_nerf/render/renderer.py:160-201].  Every comparison is on bytes,
without tolerance: each step of the frame-finishing arithmetic is one correctly rounded fp32 operation (DESIGN.md "Frame
finishing"), restated in numpy (tests/frame_forms.py), pinned by the matplotlib-made fixture tests/golden/frame_finish.npz, and
— DEPTH mode — in plain CPU torch below."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import frame_forms as FF
from tests import helpers
from thermo_nerf_amd import colormaps
from thermo_nerf_amd.cameras import Cameras
from thermo_nerf_amd.engine import RayRenderEngine
from thermo_nerf_amd.render import Renderer
from thermo_nerf_amd.render.renderer import DEPTH, LUT, SCALE, frame_to_rgb8
from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = (1, 3, 63, 64, 65, 1000)


def fixture():
    g = np.load(os.path.join(GOLDEN, "frame_finish.npz"))
    return {k: g[k] for k in g.files}


def finish(x: np.ndarray, mode: int, table=None, offset_pixels: int = 0) -> np.ndarray:
    """run the kernel on x [n, C]; dst starts ``offset_pixels`` pixels (3 bytes each) into its allocation, and the bytes around the
    view must come back untouched"""
    n = x.shape[0]
    src = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    buf = torch.full((3 * (n + offset_pixels) + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    view = buf[3 * offset_pixels: 3 * (offset_pixels + n)]
    frame_to_rgb8(src, mode, table=table, out=view)
    host = buf.cpu().numpy()
    assert (host[: 3 * offset_pixels] == 0xA5).all() and (host[3 * (offset_pixels + n):] == 0xA5).all(), "wrote outside dst"
    return host[3 * offset_pixels: 3 * (offset_pixels + n)].reshape(n, 3)


def windows(total: int, n: int):
    """three windows of n fixture inputs: the start, the special values at the end, and one in between"""
    return sorted({0, max(0, (total - n) // 2), max(0, total - n)})


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_scale_matches_fixture(n, offset):
    g = fixture()
    x, want = g["x"], g["scale"]
    for w0 in windows(x.shape[0], n):
        got = finish(x[w0: w0 + n, None], SCALE, offset_pixels=offset)
        np.testing.assert_array_equal(got, np.repeat(want[w0: w0 + n, None], 3, axis=1))
    # C = 3: consecutive inputs as one pixel's channels
    for w0 in windows(x.shape[0], 3 * n):
        got = finish(x[w0: w0 + 3 * n].reshape(n, 3), SCALE, offset_pixels=offset)
        np.testing.assert_array_equal(got, want[w0: w0 + 3 * n].reshape(n, 3))


@pytest.mark.parametrize("name", ["magma", "turbo"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_lut_matches_fixture(name, n, offset):
    g = fixture()
    x, want = g["x"], g["lut_" + name]
    table = colormaps.get_table(name, DEV)[1]
    for w0 in windows(x.shape[0], n):
        got = finish(x[w0: w0 + n, None], LUT, table=table, offset_pixels=offset)
        np.testing.assert_array_equal(got, want[w0: w0 + n])
    # C = 3: the reference looks channel 0 up [REF renderer.py:194]
    for w0 in windows(x.shape[0], 3 * n):
        got = finish(x[w0: w0 + 3 * n].reshape(n, 3), LUT, table=table, offset_pixels=offset)
        np.testing.assert_array_equal(got, want[w0: w0 + 3 * n: 3])


def test_whole_fixture_every_mode():
    """all ~3600 inputs in one launch per mode (boundaries k/256, k/255 and their neighbours, NaN, +-inf, -0.0, out of range)"""
    g = fixture()
    x = g["x"]
    np.testing.assert_array_equal(finish(x[:, None], SCALE), np.repeat(g["scale"][:, None], 3, axis=1))
    for name in ("magma", "turbo"):
        np.testing.assert_array_equal(finish(x[:, None], LUT, table=colormaps.get_table(name, DEV)[1]), g["lut_" + name])


def test_src_need_not_be_16_byte_aligned():
    """a piece of a frame: src and dst views that start at the same pixel of their allocations"""
    g = fixture()
    x = g["x"]
    for start in (1, 2, 3, 5):
        src = torch.from_numpy(x).to(DEV)[start: start + 1001, None]
        out = torch.zeros((x.shape[0], 3), dtype=torch.uint8, device=DEV)
        frame_to_rgb8(src, SCALE, out=out[start: start + 1001])
        np.testing.assert_array_equal(out[start: start + 1001].cpu().numpy(), np.repeat(g["scale"][start: start + 1001, None], 3, axis=1))
        assert int(out[:start].sum()) == 0 and int(out[start + 1001:].sum()) == 0


def test_1080p_frame_grid_stride():
    """2 073 600 pixels: more groups of 4 than the capped grid has threads"""
    n = 1920 * 1080
    rng = np.random.default_rng(1080)
    th = rng.random((n, 1), dtype=np.float32)
    th[rng.integers(0, n, 500)] = np.float32(1.0)
    th[rng.integers(0, n, 500)] = np.float32(0.0)
    rgb = rng.random((n, 3), dtype=np.float32)
    for name in ("magma", "turbo", "gray"):
        got = finish(th, LUT, table=colormaps.get_table(name, DEV)[1])
        np.testing.assert_array_equal(got, FF.lut_form(th[:, 0], colormaps.table_u8(name)))
    np.testing.assert_array_equal(finish(rgb, SCALE), FF.scale_frame(rgb))
    np.testing.assert_array_equal(finish(th, SCALE), FF.scale_frame(th))


def depth_form(d: torch.Tensor, acc: torch.Tensor, near_far: torch.Tensor, table: torch.Tensor) -> np.ndarray:
    """NS colormaps.apply_depth_colormap in CPU fp32 torch, one rounded operation per step, in the kernel's order:
    d, acc [n]; near_far [2]; table [256, 3] float32"""
    near, far = near_far[0], near_far[1]
    denom = (far - near) + torch.tensor(1e-10, dtype=torch.float32)
    t = (d - near) / denom
    t = torch.nan_to_num(torch.clip(t, 0, 1), 0)
    c = table[(t * 255).long()]
    a = acc[:, None]
    img = c * a + (1 - a)
    v = torch.clip(torch.nan_to_num(img * 255, nan=0.0, posinf=255.0, neginf=0.0), 0, 255)
    return v.to(torch.uint8).numpy()


@pytest.mark.parametrize("case", ["frame", "degenerate", "acc01", "odd"])
def test_depth_mode(case):
    g = torch.Generator().manual_seed(11)
    n = {"frame": 480 * 270, "degenerate": 4096, "acc01": 4099, "odd": 1003}[case]
    d = 0.05 + 5.0 * torch.rand(n, generator=g)
    acc = torch.rand(n, generator=g)
    if case == "degenerate":  # far == near: every pixel 0 / 1e-10
        d = torch.full((n,), 2.5)
    if case == "acc01":
        acc = (torch.rand(n, generator=g) < 0.5).float()
    if case == "odd":
        d[::7] = float("nan")
        d[1::7] = float("inf")
        acc[::5] = 0.0
        acc[1::5] = 1.0
    finite = d[torch.isfinite(d)]
    near_far = torch.stack((finite.min(), finite.max()))
    for name in ("turbo", "magma"):
        table = colormaps.get_table(name, DEV)[0]
        for offset in (0, 1):
            buf = torch.zeros(3 * (n + offset) + 4, dtype=torch.uint8, device=DEV)
            view = buf[3 * offset: 3 * (offset + n)]
            frame_to_rgb8(d[:, None].to(DEV), DEPTH, table=table, acc=acc.to(DEV), near_far=near_far.to(DEV), out=view)
            want = depth_form(d, acc, near_far, torch.from_numpy(colormaps.table_f32(name)))
            np.testing.assert_array_equal(view.cpu().numpy().reshape(n, 3), want)


def test_argument_checks():
    x = torch.rand(16, 1, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frame_to_rgb8(x.cpu())
    with pytest.raises(ValueError):
        frame_to_rgb8(x, LUT)  # no table
    with pytest.raises(ValueError):
        frame_to_rgb8(x, LUT, table=colormaps.get_table("magma", DEV)[0])  # the float table where bytes are wanted
    with pytest.raises(ValueError):
        frame_to_rgb8(x, SCALE, out=torch.empty(10, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="TN_ERR_SHAPE"):
        frame_to_rgb8(torch.rand(16, 2, device=DEV))
    assert frame_to_rgb8(torch.empty(0, 3, device=DEV)).shape == (0, 3)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def path_cameras(poses=(0, 40, 95), scale=0.1) -> Cameras:
    cams = Renderer.load_cameras(os.path.join(GOLDEN, "camera_path_facade_2.json"), scale)
    idx = torch.tensor(poses)
    c2w = cams.camera_to_worlds.clone()
    c2w[:, :3, 3] *= 0.45 / c2w[:, :3, 3].norm(dim=-1).max()  # the path was recorded around a real scene; the weights live in [-1,1]^3
    return Cameras(camera_to_worlds=c2w[idx], fx=cams.fx[idx], fy=cams.fy[idx], cx=cams.cx, cy=cams.cy, height=cams.height,
                   width=cams.width)


def host_route(model, cams: Cameras, modalities, cmap="magma"):
    """the reference's loop [REF renderer.py:180-199] with this project's model: float outputs to the host, numpy forms there"""
    frames = {m: [] for m in modalities}
    for i in range(cams.size):
        out = model.get_outputs_for_camera_ray_bundle(cams.generate_rays(i, device=DEV))
        for m in modalities:
            img = out["rgb" if m == RM.RGB else m.value].cpu().numpy()
            h, w, c = img.shape
            if m == RM.THERMAL:
                frames[m].append(FF.lut_form(img[:, :, 0].reshape(-1), colormaps.table_u8(cmap)).reshape(h, w, 3))
            else:
                frames[m].append(FF.scale_frame(img.reshape(-1, c)).reshape(h, w, 3))
    return frames


def test_renderer_end_to_end(monkeypatch):
    model, _, _ = helpers.build("scene", 48)
    gm = copy.deepcopy(model).to(DEV).eval()
    cams = path_cameras()
    modalities = [RM.THERMAL, RM.RGB, RM.ACCUMULATION]
    want = host_route(gm, cams, modalities)

    calls = []
    real = RayRenderEngine.render

    def counting(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(RayRenderEngine, "render", counting)
    r = Renderer(gm)
    r.render(modalities, cams)
    assert len(calls) == cams.size, "one render per pose, whatever the number of modalities"
    first = {m: [f.copy() for f in r._rendered_images[m]] for m in modalities}
    for m in modalities:
        assert len(first[m]) == cams.size
        for got, ref in zip(first[m], want[m]):
            assert got.dtype == np.uint8 and got.shape == (cams.height, cams.width, 3)
            np.testing.assert_array_equal(got, ref, err_msg=m.value)
    # the poses differ and the frames are not blank: a frame copied before its finish kernel ran would show up here
    assert not np.array_equal(first[RM.RGB][0], first[RM.RGB][1]) and first[RM.RGB][0].std() > 0
    # a second pass reuses the pinned double buffers: identical bytes
    r.render(modalities, cams)
    assert len(calls) == 2 * cams.size
    for m in modalities:
        for a, b in zip(first[m], r._rendered_images[m]):
            np.testing.assert_array_equal(a, b, err_msg=m.value)


def test_renderer_depth_colour_and_other_maps():
    """DEPTH: x 255 by default (the reference), nerfstudio's turbo colouring on request; THERMAL with another table"""
    model, _, _ = helpers.build("scene", 48)
    gm = copy.deepcopy(model).to(DEV).eval()
    cams = path_cameras(poses=(3, 60))
    r = Renderer(gm)
    r.render([RM.DEPTH, RM.THERMAL], cams, thermal_color_map="turbo", depth_color_map="turbo")
    coloured = r._rendered_images[RM.DEPTH]
    want_th = host_route(gm, cams, [RM.THERMAL], cmap="turbo")[RM.THERMAL]
    for i in range(cams.size):
        out = gm.get_outputs_for_camera_ray_bundle(cams.generate_rays(i, device=DEV))
        d, acc = out["depth"].reshape(-1).cpu(), out["accumulation"].reshape(-1).cpu()
        want = depth_form(d, acc, torch.stack((d.min(), d.max())), torch.from_numpy(colormaps.table_f32("turbo")))
        np.testing.assert_array_equal(coloured[i].reshape(-1, 3), want)
        np.testing.assert_array_equal(r._rendered_images[RM.THERMAL][i], want_th[i])
    r.render([RM.DEPTH], cams)
    for i in range(cams.size):
        out = gm.get_outputs_for_camera_ray_bundle(cams.generate_rays(i, device=DEV))
        np.testing.assert_array_equal(r._rendered_images[RM.DEPTH][i].reshape(-1, 3), FF.scale_frame(out["depth"].reshape(-1, 1).cpu().numpy()))


def test_render_video_tool(tmp_path):
    """tools/render_video.py: run directory + camera path JSON -> JPEG frames and GIFs on disk, equal to Renderer's own"""
    import importlib.util
    import json

    from PIL import Image

    from thermo_nerf_amd.checkpoint import save_nerfstudio_checkpoint

    model, _, _ = helpers.build("scene", 48)
    save_nerfstudio_checkpoint(model, tmp_path / "run" / "nerfstudio_models", 30000)
    cfg = dict(helpers.SMALL, num_nerf_samples_per_ray=48)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    path = json.load(open(os.path.join(GOLDEN, "camera_path_facade_2.json")))
    path["camera_path"] = [path["camera_path"][i] for i in (0, 40, 95)]
    centres = [[c["camera_to_world"][k] for k in (3, 7, 11)] for c in path["camera_path"]]
    shrink = 0.45 / max(sum(v * v for v in c) ** 0.5 for c in centres)  # into the unit box the weights live in: distinct frames
    for c in path["camera_path"]:
        for k in (3, 7, 11):
            c["camera_to_world"][k] *= shrink
    (tmp_path / "path.json").write_text(json.dumps(path))
    spec = importlib.util.spec_from_file_location("render_video", os.path.join(ROOT, "tools", "render_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "frames"
    assert tool.main([str(tmp_path / "run"), str(tmp_path / "path.json"), "--config-json", str(tmp_path / "config.json"),
                      "--downscale-factor", "10", "--save-images", "--seconds", "0.1", "--output-dir", str(out),
                      "--rendered-image-modalities", "rgb", "thermal", "accumulation"]) == 0
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted([f"{v}_{i:05d}.jpeg" for v in ("img", "thermal", "accumulation") for i in range(3)]
                           + [f"synthesized_video_{v}.gif" for v in ("img", "thermal", "accumulation")])
    with Image.open(out / "thermal_00002.jpeg") as im:
        assert im.size == (192, 108)
    with Image.open(out / "synthesized_video_img.gif") as im:
        assert im.n_frames == 3 and im.size == (192, 108)
    # (the synthetic weights' temperature is nearly uniform: the thermal frames are one colour, and PIL folds identical
    # consecutive GIF frames into one of the summed duration)
    with Image.open(out / "synthesized_video_thermal.gif") as im:
        assert im.size == (192, 108)
