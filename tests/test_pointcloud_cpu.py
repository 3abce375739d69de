"""CPU: the point-cloud export's host side — the PLY writer / reader, the numpy yardstick's own properties, the world
transform, the thinning rule and the command line's grammar (no kernel runs)."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import pointcloud_reference as R
from thermo_nerf_amd.export import ThermalPointCloud, read_ply, subsample, subsample_indices, world_transform, write_ply
from thermo_nerf_amd.export import ply as ply_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = """ply
format binary_little_endian 1.0
comment temperature_unit celsius
comment temperature_bounds 14.0 33.5
element vertex {m}
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property float temperature
end_header
"""


def _cloud(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ThermalPointCloud(positions=torch.randn((m, 3), generator=g) * 7.0,
                             colors=torch.randint(0, 256, (m, 3), generator=g, dtype=torch.uint8),
                             temperature=torch.rand((m,), generator=g) * 19.5 + 14.0,
                             thermal_colors=torch.randint(0, 256, (m, 3), generator=g, dtype=torch.uint8),
                             source=torch.arange(m, dtype=torch.int64), temperature_bounds=(14.0, 33.5))


@pytest.mark.parametrize("m", [0, 1, 1000])
def test_ply_round_trip(tmp_path, m):
    cloud = _cloud(m)
    path = write_ply(tmp_path / "sub" / "cloud.ply", cloud)
    blob = path.read_bytes()
    head = HEADER.format(m=m).encode("ascii")
    assert blob[:len(head)] == head
    assert len(blob) == len(head) + 19 * m
    back = read_ply(path)
    assert back["positions"].dtype == np.float32 and back["positions"].shape == (m, 3)
    assert back["colors"].dtype == np.uint8 and back["colors"].shape == (m, 3)
    assert back["temperature"].dtype == np.float32 and back["temperature"].shape == (m,)
    assert np.array_equal(back["positions"], cloud.positions.numpy())
    assert np.array_equal(back["colors"], cloud.colors.numpy())
    assert np.array_equal(back["temperature"], cloud.temperature.numpy())
    assert back["comments"] == ["temperature_unit celsius", "temperature_bounds 14.0 33.5"]
    # colors="thermal" swaps the colour columns and nothing else
    thermal = read_ply(write_ply(tmp_path / "thermal.ply", cloud, colors="thermal"))
    assert np.array_equal(thermal["colors"], cloud.thermal_colors.numpy())
    assert np.array_equal(thermal["positions"], back["positions"]) and np.array_equal(thermal["temperature"], back["temperature"])
    if m:
        assert not np.array_equal(thermal["colors"], back["colors"])
    # the same cloud, the same bytes
    assert write_ply(tmp_path / "again.ply", cloud).read_bytes() == blob


def test_ply_rejects_what_it_cannot_write_or_read(tmp_path):
    cloud = _cloud(3)
    with pytest.raises(ValueError):
        write_ply(tmp_path / "a.ply", cloud, colors="depth")
    cloud.thermal_colors = None
    with pytest.raises(ValueError):
        write_ply(tmp_path / "a.ply", cloud, colors="thermal")
    assert ply_module.header(2).splitlines()[3] == "comment temperature_bounds none none"
    bad = tmp_path / "bad.ply"
    bad.write_bytes(HEADER.format(m=2).encode("ascii") + b"\0" * 19)  # one vertex short
    with pytest.raises(ValueError):
        read_ply(bad)
    bad.write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        read_ply(bad)


def _random_rays(n, seed=1):
    rng = np.random.default_rng(seed)
    f = np.float32
    return dict(origins=rng.normal(0, 0.4, (n, 3)).astype(f), directions=rng.normal(0, 1, (n, 3)).astype(f),
                depth=rng.uniform(0, 1, n).astype(f), accumulation=rng.uniform(0, 1, n).astype(f),
                rgb=rng.uniform(0, 1, (n, 3)).astype(f), thermal=rng.uniform(0, 1, n).astype(f))


def test_reference_all_kept_identity_is_the_back_projection():
    r = _random_rays(500)
    q = R.params(min_accumulation=-1.0)
    out = R.export(**r, q=q, source_base=7)
    want = (r["origins"] + r["directions"] * r["depth"][:, None]).astype(np.float32)  # numpy's own o + d * depth in fp32
    assert out["keep"].all() and out["positions"].dtype == np.float32
    assert np.array_equal(out["positions"], want)
    assert np.array_equal(out["source"], np.arange(500) + 7)
    assert np.array_equal(out["temperature"], r["thermal"])  # span 1, min 0
    assert np.array_equal(out["colors"], (r["rgb"] * np.float32(255)).astype(np.uint8))  # in [0, 1): numpy's cast


def test_reference_drops_nan_and_values_on_a_bound():
    r = _random_rays(64, seed=2)
    r["origins"][:] = 0.0
    r["directions"][:] = np.float32(0.25)
    r["depth"][:] = 1.0      # p = (0.25, 0.25, 0.25)
    r["accumulation"][:] = 0.75
    r["thermal"][:] = 0.5
    q = R.params(min_accumulation=0.5, box_min=(-1, -1, -1), box_max=(1, 1, 1), thermal_lo=0.25, thermal_hi=0.875)
    assert R.export(**r, q=q)["keep"].all()
    nan = np.float32("nan")
    r["depth"][1] = nan
    r["accumulation"][2] = nan
    r["thermal"][3] = nan
    r["origins"][4, 1] = nan          # NaN in p through the origin
    r["directions"][5, 2] = nan       # ... and through the direction
    r["accumulation"][6] = 0.5        # == min_accumulation
    r["origins"][7, 0] = 0.75         # p_x = 1.0 exactly: on the upper face
    r["origins"][8, 2] = -1.25        # p_z = -1.0 exactly: on the lower face
    r["thermal"][9] = 0.25            # == thermal_lo
    r["thermal"][10] = 0.875          # == thermal_hi
    r["depth"][11] = np.float32("inf")
    out = R.export(**r, q=q)
    assert np.array_equal(np.nonzero(~out["keep"])[0], np.arange(1, 12))
    assert np.array_equal(out["source"], np.concatenate([[0], np.arange(12, 64)]))
    # infinite bounds switch a test off — but never let a NaN through
    free = R.params(min_accumulation=-np.inf)
    assert np.array_equal(np.nonzero(~R.export(**r, q=free)["keep"])[0], [1, 2, 3, 4, 5, 11])  # (11: p = inf is not < inf)


def test_reference_bytes_and_degrees():
    table = np.arange(768, dtype=np.int64).reshape(256, 3).astype(np.uint8)
    x = np.array([-0.5, 0.0, 0.00390625, 0.999, 1.0, 1.5, np.nan], dtype=np.float32)
    assert R.scale_bytes(x).tolist() == [0, 0, 0, 254, 255, 255, 0]
    assert R.lut_bytes(x, table)[:, 0].tolist() == [table[0, 0], table[0, 0], table[1, 0], table[255, 0], table[255, 0], table[255, 0], 0]
    q = R.params(min_accumulation=-1.0, max_temperature=33.0, min_temperature=14.0)
    assert q["temperature_span"] == np.float32(19.0)
    r = _random_rays(16, seed=3)
    out = R.export(**r, q=q, table_u8=table)
    assert np.array_equal(out["temperature"], r["thermal"] * np.float32(19.0) + np.float32(14.0))
    assert out["thermal_colors"].shape == (16, 3)


def test_world_transform_maps_normalised_origins_back_to_the_files_translations(tmp_path):
    """Tolerance, derived: the parser forms a normalised origin in fp32 as (T @ pose) * scale — per coordinate three products,
    three sums and the scaling, 7 roundings — and world_transform rounds its fp64 inverse to fp32 once: 8 roundings, each at
    most half an ulp (eps / 2) of a partial sum no larger than sqrt(3) L, L = the largest coordinate involved (a rotated
    vector's partial sums are bounded by its norm).  The inverse amplifies them by the condition of its 3 x 3 part."""
    from thermo_nerf_amd.data import ThermalDataParserConfig

    rng = np.random.default_rng(4)
    frames, want = [], {}
    for k in range(7):
        az = 2 * math.pi * k / 7
        c2w = np.eye(4)
        c2w[:3, 3] = [3 * math.cos(az) + 10.0, 3 * math.sin(az) - 4.0, 1.0 + 0.1 * k]
        c2w[:3, 1] = [0.0, 0.6, 0.8]
        c2w[:3, 2] = [0.0, -0.8, 0.6]
        name = f"frame_{'eval' if k == 3 else 'train'}_{k:04d}.png"
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}", "transform_matrix": c2w.tolist()})
        want[name] = c2w[:3, 3]
    order = rng.permutation(7)
    (tmp_path / "transforms.json").write_text(json.dumps(
        {"fl_x": 10.0, "fl_y": 10.0, "cx": 4, "cy": 3, "w": 8, "h": 6, "frames": [frames[k] for k in order]}))
    for split in ("train", "val"):
        out = ThermalDataParserConfig(data=tmp_path).setup().get_dataparser_outputs(split)
        m = world_transform(out)
        assert m.dtype == torch.float32 and tuple(m.shape) == (3, 4)
        m64 = m.double().numpy()
        origins = out.cameras.camera_to_worlds[:, :3, 3].double().numpy()
        back = origins @ m64[:, :3].T + m64[:, 3]
        files = np.stack([want[p.name] for p in out.image_filenames])
        largest = max(np.abs(files).max(), np.abs(m64[:, 3]).max())
        tol = 8 * (np.finfo(np.float32).eps / 2) * math.sqrt(3.0) * largest * np.linalg.cond(m64[:, :3])
        err = np.abs(back - files).max()
        print(split, "error", err, "tolerance", tol)
        assert err <= tol
        assert abs(out.dataparser_scale - 1.0) > 0.1  # the scene was rescaled: the transform is not a plain rigid motion


def test_subsample_index_rule():
    for m, n in ((5, 8), (8, 8), (3 * 8 + 1, 8), (0, 4), (7, 0)):
        idx = subsample_indices(m, n)
        assert idx.dtype == torch.int64
        want = list(range(m)) if m <= n else [j * m // n for j in range(n)]
        assert idx.tolist() == want, (m, n)
    assert subsample_indices(25, 8).tolist() == [0, 3, 6, 9, 12, 15, 18, 21]
    assert subsample_indices(1 << 40, 3).tolist() == [0, (1 << 40) // 3, 2 * (1 << 40) // 3]
    cloud = _cloud(25)
    assert subsample(cloud, 25) is cloud and subsample(cloud, 100) is cloud
    thin = subsample(cloud, 8)
    assert len(thin) == 8 and thin.source.tolist() == [0, 3, 6, 9, 12, 15, 18, 21]
    assert torch.equal(thin.positions, cloud.positions[thin.source]) and torch.equal(thin.thermal_colors, cloud.thermal_colors[thin.source])
    assert thin.temperature_bounds == cloud.temperature_bounds


def _tool():
    spec = importlib.util.spec_from_file_location("export_pointcloud", os.path.join(ROOT, "tools", "export_pointcloud.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_defaults_and_threshold_grammar(capsys):
    tool = _tool()
    a = tool.parse(["run", "data", "--output", "cloud.ply"])
    assert (str(a.model_uri), str(a.dataset_path), str(a.output)) == ("run", "data", "cloud.ply")
    assert a.split == "train" and a.num_points == 1000000 and a.resolution_scale == 1.0 and a.depth == "depth"
    assert a.min_accumulation == 0.5 and a.no_bounding_box is False and a.bounding_box_min is None and a.bounding_box_max is None
    assert a.threshold is None and a.colors == "rgb" and a.scene_frame is False and a.config_json is None and a.device == "cuda"
    assert tool.parse(["r", "d", "--output", "o", "--threshold", "none"]).threshold is None
    assert tool.parse(["r", "d", "--output", "o", "--threshold", "AUTO"]).threshold == "auto"
    assert tool.parse(["r", "d", "--output", "o", "--threshold", "0.25"]).threshold == 0.25
    b = tool.parse(["r", "d", "--output", "o", "--split", "val", "--num-points", "10", "--depth", "expected_depth", "--colors",
                    "thermal", "--scene-frame", "--bounding-box-min", "-1", "-2", "-3", "--bounding-box-max", "1", "2", "3"])
    assert b.split == "val" and b.num_points == 10 and b.depth == "expected_depth" and b.colors == "thermal" and b.scene_frame
    assert b.bounding_box_min == [-1.0, -2.0, -3.0] and b.bounding_box_max == [1.0, 2.0, 3.0]
    for bad in (["r", "d"], ["r", "d", "--output", "o", "--threshold", "warm"], ["r", "d", "--output", "o", "--depth", "median"],
                ["r", "d", "--output", "o", "--bounding-box-min", "0", "0", "0"],
                ["r", "d", "--output", "o", "--no-bounding-box", "--bounding-box-min", "0", "0", "0", "--bounding-box-max", "1", "1", "1"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    capsys.readouterr()
