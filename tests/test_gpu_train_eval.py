"""GPU: the train-and-evaluate workflow as its two command lines run it — tools/train_eval.py on a small dataset tree, then
tools/evaluate.py on the run directory it left."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the keys of the reference's metrics.json [REF thermo_nerf/thermal_nerf/thermal_nerf_model.py get_image_metrics_and_images]
METRIC_KEYS = ("psnr", "ssim", "lpips", "psnr_thermal", "ssim_thermal", "lpips_thermal", "mae_thermal", "mae_thermal_foreground")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_tree(root):
    """10 frames of 32 x 32 from the analytic scene: 8 train, 2 eval (the tree of test_thermoscenes_style_tree_to_training_steps)"""
    from thermo_nerf_amd import synthetic

    res, n = 32, 10
    cams = synthetic.orbit_cameras(res, res, list(range(n)), num_views=n, elevation_deg=[(0.0, 25.0)[v % 2] for v in range(n)])
    (root / "images").mkdir(parents=True)
    (root / "thermal").mkdir()
    frames = []
    for i in range(n):
        rb = cams.generate_rays(i, device=DEV)
        rgb, th = synthetic.analytic_scene(rb.origins, rb.directions)
        name = f"frame_{'eval' if i % 5 == 4 else 'train'}_{i:04d}.png"
        Image.fromarray((rgb.cpu().numpy() * 255).round().astype(np.uint8)).save(root / "images" / name)
        Image.fromarray((th[..., 0].cpu().numpy() * 255).round().astype(np.uint8), mode="L").save(root / "thermal" / name)
        c2w = torch.cat([cams.camera_to_worlds[i], torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}", "transform_matrix": c2w})
    f = float(cams.fx[0])
    (root / "transforms.json").write_text(json.dumps(
        {"fl_x": f, "fl_y": f, "cx": res / 2, "cy": res / 2, "w": res, "h": res, "frames": frames}))


def _check_metrics(path, images: int):
    info = json.loads(path.read_text())
    assert info["method_name"] == "thermal-nerf"
    res = info["results"]
    assert set(res) == {k + s for k in METRIC_KEYS for s in ("", "_mean", "_std")}
    for k in METRIC_KEYS:
        assert len(res[k]) == images
    assert all(v is None for v in res["lpips"] + res["lpips_thermal"])  # no pretrained network offline: null
    return info


def test_train_eval_then_evaluate(tmp_path):
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import calculate_threshold

    data = tmp_path / "data"
    _write_tree(data)
    small = tmp_path / "small.json"
    small.write_text(json.dumps(helpers.SMALL))
    models, metrics = tmp_path / "models", tmp_path / "metrics"

    rc = _tool("train_eval").main(["--data", str(data), "--experiment-name", "unit run", "--model-output-folder", str(models),
                                   "--metrics-output-folder", str(metrics), "--max-num-iterations", "30", "--config-json", str(small),
                                   "--temperature-bounds", "33", "14", "--device", DEV])
    assert rc == 0
    runs = list((models / "unit run" / "thermal-nerf").iterdir())
    assert len(runs) == 1
    run_dir = runs[0]
    assert (run_dir / "nerfstudio_models" / "step-000000030.ckpt").is_file()
    run = json.loads((run_dir / "config.json").read_text())
    threshold = calculate_threshold(data, device=DEV)
    assert run["threshold"] == threshold and 0.0 < threshold < 1.0
    assert run["num_train_data"] == 8 and run["temperature_bounds"] == [33.0, 14.0] and run["cold"] is False
    assert run["eval_mode"] == "filename" and run["data"] == str(data)
    assert run["model"]["log2_hashmap_size"] == 15 and run["model"]["max_temperature"] == 33.0

    first = _check_metrics(metrics / "metrics.json", images=2)
    assert first["experiment_name"] == "unit run"
    for k in range(2):
        for stem in ("img", "thermal", "thermal_combined"):
            assert (metrics / f"{stem}_{k:05d}.jpg").is_file(), (stem, k)
    assert sorted(p.name for p in metrics.iterdir()) == sorted(
        ["metrics.json"] + [f"{s}_{k:05d}.jpg" for s in ("img", "thermal", "thermal_combined") for k in range(2)])
    res = first["results"]
    assert all(0.0 < v < 19.0 for v in res["mae_thermal"])  # degrees: normalised error x (33 - 14)

    # the same checkpoint through the evaluation command, deterministic eval kernels: the same numbers, exactly
    evaluate = _tool("evaluate")
    again_dir = tmp_path / "again"
    assert evaluate.main([str(run_dir), str(data), "--output-folder", str(again_dir), "--threshold", "auto",
                          "--modalities-to-save", "rgb", "thermal", "thermal_combined", "--device", DEV]) == 0
    again = _check_metrics(again_dir / "metrics.json", images=2)
    for key in res:
        print(key, res[key], again["results"][key])
    assert again["results"] == res
    for k in range(2):
        for stem in ("img", "thermal", "thermal_combined"):
            assert (again_dir / f"{stem}_{k:05d}.jpg").read_bytes() == (metrics / f"{stem}_{k:05d}.jpg").read_bytes()

    # without a threshold (the reference's eval script) the foreground is the whole image
    none_dir = tmp_path / "none"
    assert evaluate.main([str(run_dir), str(data), "--output-folder", str(none_dir), "--threshold", "none", "--device", DEV]) == 0
    none = _check_metrics(none_dir / "metrics.json", images=2)["results"]
    assert none["mae_thermal_foreground"] == none["mae_thermal"] == res["mae_thermal"]
    assert sorted(p.name for p in none_dir.iterdir()) == ["img_00000.jpg", "img_00001.jpg", "metrics.json"]
