"""CPU: the foreground threshold's host side (file listing, enum, command-line parsing, C-ABI declaration and argument checks)
and the test-side restatement of the Otsu recurrence on the fixture image.  No device arithmetic runs here."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import otsu_reference as R
from thermo_nerf_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_type_has_the_references_members():
    import thermo_nerf_amd as tna
    from thermo_nerf_amd.model_type import ModelType

    assert tna.ModelType is ModelType
    assert {m.name: m.value for m in ModelType} == {"THERMALNERFACTO": 1, "THERMONERF": 2, "CONCATNERF": 3, "NERFACTO": 4}
    assert ModelType(2) is ModelType.THERMONERF


def test_restatement_on_the_fixture_image(golden_dir):
    """tests/golden/thermal/IMG_3561.PNG (480 x 640, mode L): the recurrence and a brute-force class-variance maximisation both
    give 53; the two best sigmas differ by 4e-4 relative (no plateau decides this image); 53 / 255 = 0.20784..."""
    pil = Image.open(os.path.join(golden_dir, "thermal", "IMG_3561.PNG"))
    assert pil.mode == "L" and pil.size == (480, 640)
    hist = np.bincount(np.asarray(pil, dtype=np.uint8).reshape(-1), minlength=256)
    assert hist.sum() == 480 * 640
    assert R.otsu_restated(hist) == 53
    sigma = R.between_class_variance(hist)
    assert int(np.argmax(sigma)) == 53
    best, second = np.sort(sigma)[::-1][:2]
    assert 1e-4 < (best - second) / best < 1e-3
    assert 53 / 255.0 == pytest.approx(0.20784, abs=1e-5)


def test_restatement_edge_cases():
    const = np.zeros(256, dtype=np.int64)
    const[77] = 1000
    assert R.otsu_restated(const) == 0  # a constant image
    two = np.zeros(256, dtype=np.int64)
    two[10], two[200] = 300, 700
    t = R.otsu_restated(two)
    assert 10 <= t < 200  # anywhere on the plateau between the two values separates them
    assert R.between_class_variance(two)[t] == R.between_class_variance(two).max()
    assert R.smallest_class_fraction(two) == 0.3 and R.smallest_class_fraction(const) == 1.0


def _write_tree(root, n=5):
    (root / "images").mkdir()
    (root / "thermal").mkdir()
    rng = np.random.default_rng(3)
    frames = []
    for i in range(n):
        name = f"frame_{'eval' if i % 5 == 4 else 'train'}_{i:04d}.png"
        Image.fromarray(rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)).save(root / "images" / name)
        th = rng.integers(0, 256, (6, 8), dtype=np.uint8)
        Image.fromarray(th, mode="L").save(root / "thermal" / name)
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}",
                       "transform_matrix": np.eye(4).tolist()})
    (root / "transforms.json").write_text(json.dumps({"fl_x": 10.0, "fl_y": 10.0, "cx": 4, "cy": 3, "w": 8, "h": 6, "frames": frames}))
    return frames


def test_file_listing_uses_every_frame_and_the_model_types_key(tmp_path):
    from thermo_nerf_amd.model_type import ModelType
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import load_grey_image, thermal_image_paths

    frames = _write_tree(tmp_path, n=5)
    from_dir = thermal_image_paths(tmp_path)
    from_json = thermal_image_paths(tmp_path / "transforms.json")
    assert from_dir == from_json and len(from_dir) == 5  # train AND eval frames
    assert from_dir == [tmp_path / f["thermal_file_path"] for f in frames]
    assert sum("eval" in p.name for p in from_dir) == 1
    for mt in (ModelType.THERMONERF, ModelType.THERMALNERFACTO, ModelType.CONCATNERF):
        assert thermal_image_paths(tmp_path, mt) == from_dir
    assert thermal_image_paths(tmp_path, ModelType.NERFACTO) == [tmp_path / f["file_path"] for f in frames]
    # single-channel bytes as they are; anything else through PIL's convert("L"); always the file's full resolution
    grey = load_grey_image(from_dir[0])
    assert grey.dtype == np.uint8 and grey.shape == (6, 8)
    assert np.array_equal(grey, np.asarray(Image.open(from_dir[0])))
    rgb_path = tmp_path / frames[0]["file_path"]
    assert np.array_equal(load_grey_image(rgb_path), np.asarray(Image.open(rgb_path).convert("L")))
    with pytest.raises(FileNotFoundError):
        load_grey_image(tmp_path / "thermal" / "absent.png")


def test_calculate_threshold_has_no_cpu_fallback(tmp_path):
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import calculate_threshold, otsu_thresholds

    _write_tree(tmp_path, n=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        calculate_threshold(tmp_path, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        otsu_thresholds([torch.zeros(4, 4, dtype=torch.uint8)])


def test_train_eval_parse_defaults_and_refusals(capsys):
    from pathlib import Path

    from thermo_nerf_amd.model_type import ModelType

    tool = _tool("train_eval")
    a = tool.parse([])
    assert a.model_type is ModelType.THERMONERF and a.experiment_name == "nerfacto training"
    assert a.model_output_folder == Path("./outputs") and a.max_num_iterations == 30000 and a.data == Path("./inputs")
    assert a.metrics_output_folder == Path("./outputs/") and a.seed == 0 and a.temperature_bounds == [1.0, 0.0]
    assert a.cold is False and a.camera_optimizer_mode == "SO3xR3" and a.eval_mode == "filename" and a.config_json is None
    b = tool.parse(["--temperature-bounds", "33", "14", "--cold", "--eval-mode", "interval", "--camera-optimizer-mode", "off",
                    "--max-num-iterations", "30", "--seed", "7"])
    assert b.temperature_bounds == [33.0, 14.0] and b.cold is True and b.eval_mode == "interval"
    assert b.camera_optimizer_mode == "off" and b.max_num_iterations == 30 and b.seed == 7
    for name in ("thermalnerfacto", "concatnerf", "nerfacto"):
        with pytest.raises(SystemExit) as e:
            tool.parse(["--model-type", name])
        assert e.value.code == 2
        assert "baseline models" in capsys.readouterr().err


def test_evaluate_parse_defaults_and_threshold_forms(capsys):
    from pathlib import Path

    from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM

    tool = _tool("evaluate")
    a = tool.parse(["run", "data"])
    assert a.model_uri == Path("run") and a.dataset_path == Path("data") and a.output_folder == Path("./outputs")
    assert a.modalities == [RM.RGB] and a.threshold is None and a.config_json is None
    assert tool.parse(["run", "data", "--threshold", "none"]).threshold is None
    assert tool.parse(["run", "data", "--threshold", "auto"]).threshold == "auto"
    assert tool.parse(["run", "data", "--threshold", "0.3"]).threshold == 0.3
    b = tool.parse(["run", "data", "--modalities-to-save", "rgb", "thermal", "thermal_combined"])
    assert b.modalities == [RM.RGB, RM.THERMAL, RM.THERMAL_COMBINED]
    with pytest.raises(SystemExit) as e:
        tool.parse(["run", "data", "--threshold", "high"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        tool.parse(["run"])  # both positionals are required
    assert e.value.code == 2
    capsys.readouterr()


def test_run_config_round_trip(tmp_path):
    """config.json keeps the model fields that differ from the defaults and rebuilds the same configuration from them"""
    import dataclasses

    from tests import helpers
    from thermo_nerf_amd import ThermalNerfModelConfig, run_config

    cfg = ThermalNerfModelConfig(**helpers.SMALL, max_temperature=33.0, min_temperature=14.0, eval_num_rays_per_chunk=1 << 16,
                                 num_proposal_samples_per_ray=(64, 32))
    path = run_config.write_run_config(tmp_path, cfg, 8, [33.0, 14.0], False, "filename", tmp_path / "data", 0.25, seed=3)
    run = run_config.read_run_config(tmp_path)
    assert path.name == "config.json" and run["num_train_data"] == 8 and run["threshold"] == 0.25 and run["seed"] == 3
    assert run["temperature_bounds"] == [33.0, 14.0] and run["cold"] is False and run["eval_mode"] == "filename"
    assert set(run["model"]) == {"log2_hashmap_size", "proposal_net_args_list", "max_temperature", "min_temperature",
                                 "eval_num_rays_per_chunk", "num_proposal_samples_per_ray"}  # (SMALL's other two are defaults)
    again = run_config.model_config(run_config.load_overrides(path))
    for f in dataclasses.fields(cfg):
        if f.name not in ("_target", "camera_optimizer"):
            assert getattr(again, f.name) == getattr(cfg, f.name), f.name
    with pytest.raises(FileNotFoundError):
        run_config.read_run_config(tmp_path / "absent")


def test_entry_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bint tn_otsu_thresholds\(const uint8_t \*pixels, const int64_t \*offsets, int32_t num_images", header)
    assert "[REF thermo_nerf/thermal_nerf/calculate_threshold.py:29-38]" in header
    assert "tn_otsu_thresholds" in _hip.SIGNATURES
    fn = _hip.load().tn_otsu_thresholds
    offs = (ctypes.c_int64 * 2)(0, 16)
    dummy = 4096  # a non-null address: every case below is refused before anything is dereferenced or launched
    assert fn(None, offs, 1, dummy, dummy, None) == -1
    assert fn(dummy, None, 1, dummy, dummy, None) == -1
    assert fn(dummy, offs, 1, None, dummy, None) == -1
    assert fn(dummy, offs, 1, dummy, None, None) == -1
    assert fn(dummy, offs, 0, dummy, dummy, None) == -2
    assert fn(dummy, offs, -3, dummy, dummy, None) == -2
    assert fn(dummy, (ctypes.c_int64 * 2)(0, 0), 1, dummy, dummy, None) == -2          # an image without pixels
    assert fn(dummy, (ctypes.c_int64 * 3)(0, 16, 8), 2, dummy, dummy, None) == -2      # decreasing offsets
    assert fn(dummy, (ctypes.c_int64 * 2)(0, 1 << 32), 1, dummy, dummy, None) == -3    # TN_ERR_UNSUPPORTED: 2^32 pixels
