"""CPU: the numpy restatement of the voxel down-sampling (tests/voxel_reference.py) against closed forms, the argument checks of
tn_sort_pairs and tn_voxel_downsample through the library (every refusal comes before the first HIP call), and the host side:
the command line's --voxel-size and the grid that voxel_downsample derives.  No device arithmetic runs here."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import voxel_reference as R
from thermo_nerf_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OK, NULL, SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3, -4


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_lattice_on_voxel_faces_gives_one_unchanged_point_per_voxel():
    """coordinates -0.5 + 0.25 i: every point lies exactly on a face of a 0.25 grid from -0.5, every step is exact"""
    p, colors, temperature, thermal, source = R.lattice(side=6, step=0.25)
    origin, dims = R.grid_of(p, 0.25)
    assert origin.tolist() == [-0.5] * 3 and dims.tolist() == [6, 6, 6]
    out = R.voxel_downsample(p, colors, temperature, thermal, source, origin, 0.25, dims)
    keys, total = R.voxel_keys(p, origin, 0.25, dims)
    assert total == 216 and sorted(keys.tolist()) == list(range(216))
    order = np.argsort(keys, kind="stable")
    assert out["members"] == 216 and (out["voxel_count"] == 1).all()
    assert out["positions"].tobytes() == p[order].tobytes() and out["temperature"].tobytes() == temperature[order].tobytes()
    assert np.array_equal(out["colors"], colors[order]) and np.array_equal(out["thermal_colors"], thermal[order])
    assert np.array_equal(out["source"], source[order])
    # x runs fastest in the key
    assert (np.diff(out["positions"][:6, 0]) == F(0.25)).all() and (out["positions"][:6, 1:] == F(-0.5)).all()


def test_lattice_at_twice_the_voxel_size_gives_the_centres_of_eight():
    p, colors, temperature, thermal, source = R.lattice(side=6, step=0.25)
    origin, dims = R.grid_of(p, 0.5)
    assert dims.tolist() == [3, 3, 3]
    out = R.voxel_downsample(p, colors, temperature, thermal, source, origin, 0.5, dims)
    assert (out["voxel_count"] == 8).all() and int(out["voxel_count"].sum()) == out["members"] == 216
    g = np.arange(3, dtype=np.float64) * 0.5 - 0.5 + 0.125  # the mean of -0.5 + 0.5 c and -0.25 + 0.5 c
    want = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1].astype(F)  # z slowest, x fastest
    assert out["positions"].tobytes() == np.ascontiguousarray(want).tobytes()
    # the first member's source, and a temperature mean within its members' range
    keys, _ = R.voxel_keys(p, origin, 0.5, dims)
    for v in (0, 13, 26):
        rows = np.nonzero(keys == v)[0]
        assert out["source"][v] == source[rows[0]] and temperature[rows].min() <= out["temperature"][v] <= temperature[rows].max()
        s = np.float64(0.0)
        for i in rows:
            s = s + np.float64(temperature[i])
        assert out["temperature"][v] == F(s / np.float64(8))


def test_points_outside_the_grid_and_non_finite_points_are_dropped():
    p, colors, temperature, thermal, source = R.lattice(side=4, step=0.25)
    p = p.copy()
    p[3, 1], p[9, 0], p[20, 2] = np.nan, np.inf, -np.inf
    origin, dims = np.array([-0.5, -0.5, -0.5], F), np.array([3, 4, 2], np.int32)  # x = 0.25 is ON the upper face u = 3: dropped
    keys, total = R.voxel_keys(p, origin, 0.25, dims)
    inside = np.isfinite(p).all(axis=1) & (p[:, 0] < 0.25) & (p[:, 2] < 0.0)
    assert total == 24 and np.array_equal(keys < 24, inside) and (keys[~inside] == 24).all()
    out = R.voxel_downsample(p, colors, temperature, None, None, origin, 0.25, dims)
    assert out["members"] == int(inside.sum()) == int(out["voxel_count"].sum()) and out["thermal_colors"] is None and out["source"] is None
    assert R.grid_of(np.full((3, 3), np.nan, F), 0.25) is None


def test_colours_round_half_up():
    two = np.array([[0, 1, 255], [1, 2, 254]], np.uint8)     # means 0.5, 1.5, 254.5
    assert R.rounded_mean(two, 2).tolist() == [1, 2, 255]
    four = np.array([[10, 0, 3]] * 3 + [[12, 1, 4]], np.uint8)  # means 10.5, 0.25, 3.25
    assert R.rounded_mean(four, 4).tolist() == [11, 0, 3]
    three = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1]], np.uint8)  # 1/3 twice
    assert R.rounded_mean(three, 3).tolist() == [0, 0, 0]
    p = np.zeros((2, 3), F)
    out = R.voxel_downsample(p, two, np.array([1.0, 2.0], F), two[::-1].copy(), None, np.zeros(3, F), 1.0, np.ones(3, np.int32))
    assert out["colors"].tolist() == [[1, 2, 255]] and out["thermal_colors"].tolist() == [[1, 2, 255]] and out["temperature"][0] == F(1.5)


def test_sort_reference_orders_by_the_low_bytes_only():
    keys = np.array([0x1FF, 0x2FE, 0x100, 0x3FF], np.uint64)
    k, v = R.sort_pairs(keys, None, 8)  # one pass: bits 8 and above travel
    assert k.tolist() == [0x100, 0x2FE, 0x1FF, 0x3FF] and v.tolist() == [2, 1, 0, 3]
    k, v = R.sort_pairs(keys, np.array([7, 8, 9, 10], np.int32), 9)  # two passes: 16 ordering bits
    assert k.tolist() == [0x100, 0x1FF, 0x2FE, 0x3FF] and v.tolist() == [9, 7, 8, 10]
    assert R.ordering_mask(64) == np.uint64(2 ** 64 - 1) and R.ordering_mask(1) == np.uint64(255)


def test_sort_entry_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bint tn_sort_pairs\(const uint64_t \*keys_in, const int32_t \*values_in, int64_t n, int key_bits", header)
    assert re.search(r"\bsize_t tn_sort_pairs_workspace_bytes\(int64_t n\);", header)
    assert "tn_sort_pairs" in _hip.SIGNATURES and "tn_sort_pairs_workspace_bytes" in _hip.SIGNATURES
    lib = _hip.load()
    n = 1000
    need = lib.tn_sort_pairs_workspace_bytes(n)
    tile = lib.tn_sort_tile()
    assert tile > 0 and tile % 256 == 0
    assert need == 8 * n + 4 * n + 8 * (256 * -(-n // tile) + 1)
    assert lib.tn_sort_pairs_workspace_bytes(-1) == 0 and lib.tn_sort_pairs_workspace_bytes(2 ** 31) == 0
    assert lib.tn_sort_pairs_workspace_bytes(0) == 8 and lib.tn_sort_pairs_workspace_bytes(2 ** 31 - 1) > 12 * (2 ** 31 - 1)
    dummy = 4096  # a non-null, aligned address: every case below is refused before anything is dereferenced or launched
    names = ("keys_in", "values_in", "n", "key_bits", "keys_out", "values_out", "workspace", "workspace_bytes", "stream")
    good = dict(keys_in=dummy, values_in=dummy, n=n, key_bits=64, keys_out=dummy, values_out=dummy, workspace=dummy,
                workspace_bytes=need, stream=None)

    def call(**change):
        args = dict(good, **change)
        return lib.tn_sort_pairs(*[args[k] for k in names])

    assert call(key_bits=0) == UNSUPPORTED and call(key_bits=65) == UNSUPPORTED and call(key_bits=-8) == UNSUPPORTED
    assert call(n=-1) == SHAPE and call(n=2 ** 31) == SHAPE
    assert call(n=0) == OK and call(n=0, keys_in=None, keys_out=None, values_out=None, workspace=None, workspace_bytes=0) == OK
    for name in ("keys_in", "keys_out", "values_out", "workspace"):
        assert call(**{name: None}) == NULL, name
    for name, off in (("keys_in", 4), ("keys_out", 4), ("workspace", 4), ("values_in", 2), ("values_out", 2)):
        assert call(**{name: dummy + off}) == SHAPE, name
    assert call(workspace_bytes=need - 1) == WORKSPACE and call(workspace_bytes=0) == WORKSPACE
    assert call(workspace_bytes=need - 1, values_in=None) == WORKSPACE  # values_in may be null: the next check is reached


def test_voxel_entry_is_declared_bound_and_checks_its_arguments():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bint tn_voxel_downsample\(const float \*positions, const uint8_t \*colors, const float \*temperature", header)
    assert re.search(r"\bsize_t tn_voxel_downsample_workspace_bytes\(int64_t num_points\);", header)
    assert "tn_voxel_downsample" in _hip.SIGNATURES
    lib = _hip.load()
    n = 1000
    need = lib.tn_voxel_downsample_workspace_bytes(n)
    assert need >= lib.tn_sort_pairs_workspace_bytes(n) + 2 * 8 * n + 2 * 4 * n
    assert lib.tn_voxel_downsample_workspace_bytes(-1) == 0 and lib.tn_voxel_downsample_workspace_bytes(2 ** 31) == 0
    dummy = 4096
    names = ("positions", "colors", "temperature", "thermal_colors", "source", "num_points", "params", "positions_out", "colors_out",
             "temperature_out", "thermal_colors_out", "source_out", "voxel_count", "capacity", "count", "workspace", "workspace_bytes",
             "stream")

    def params(size=0.25, dims=(4, 4, 4)):
        q = _hip.tn_voxel_params()
        q.voxel_size = size
        q.dims[:] = dims
        return ctypes.byref(q)

    good = dict({k: dummy for k in names}, num_points=n, params=params(), capacity=n, workspace_bytes=need, stream=None)

    def call(**change):
        args = dict(good, **change)
        return lib.tn_voxel_downsample(*[args[k] for k in names])

    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (2 ** 21 + 1, 4, 4), (4, 4, 2 ** 21 + 1), (-1, 4, 4)):
        assert call(params=params(dims=dims)) == UNSUPPORTED, dims
    for size in (0.0, -0.25, float("nan"), float("inf")):
        assert call(params=params(size=size)) == UNSUPPORTED, size
    assert call(num_points=-1) == SHAPE and call(num_points=2 ** 31) == SHAPE and call(capacity=-1) == SHAPE
    for name in ("params", "count", "positions", "colors", "temperature", "workspace", "positions_out", "colors_out", "temperature_out",
                 "voxel_count"):
        assert call(**{name: None}) == NULL, name
    assert call(thermal_colors=None) == NULL and call(source=None) == NULL  # an output without its input
    for name, off in (("positions", 2), ("temperature", 2), ("source", 4), ("positions_out", 2), ("temperature_out", 2),
                      ("source_out", 4), ("voxel_count", 2), ("count", 4), ("workspace", 4)):
        assert call(**{name: dummy + off}) == SHAPE, name
    assert call(workspace_bytes=need - 1) == WORKSPACE and call(workspace_bytes=0) == WORKSPACE
    # null on both sides, and the sizing call's null outputs, pass every check up to the workspace's
    assert call(thermal_colors=None, thermal_colors_out=None, source=None, source_out=None, workspace_bytes=need - 1) == WORKSPACE
    assert call(capacity=0, positions_out=None, colors_out=None, temperature_out=None, thermal_colors_out=None, source_out=None,
                voxel_count=None, workspace_bytes=need - 1) == WORKSPACE
    assert call(params=params(dims=(2 ** 21,) * 3), workspace_bytes=need - 1) == WORKSPACE  # the largest grid is accepted


def test_command_line_voxel_size(capsys):
    tool = _tool("export_pointcloud")
    base = ["run", "data", "--output", "c.ply"]
    assert tool.parse(base).voxel_size is None
    assert tool.parse(base + ["--voxel-size", "0.02"]).voxel_size == 0.02
    for bad in ("0", "-0.5", "nan", "inf", "small"):
        with pytest.raises(SystemExit) as e:
            tool.parse(base + ["--voxel-size", bad])
        assert e.value.code == 2, bad
    assert "--voxel-size" in capsys.readouterr().err


def test_the_grid_voxel_downsample_derives_and_its_limit():
    import torch

    from thermo_nerf_amd.export import ThermalPointCloud, voxel_downsample, voxel_grid

    p = R.lattice(side=6, step=0.25)[0]
    for size in (0.25, 0.5, 0.11, 0.01):
        origin, dims = voxel_grid(p.min(axis=0).tolist(), p.max(axis=0).tolist(), size)
        want = R.grid_of(p, size)
        assert np.array_equal(np.array(origin, F), want[0]) and list(dims) == want[1].tolist(), size
    assert voxel_grid((0.0,) * 3, (1.0,) * 3, 2.0 ** -20)[1] == (2 ** 20 + 1,) * 3
    assert voxel_grid((0.0,) * 3, (2.0 - 2.0 ** -22,) * 3, 2.0 ** -20)[1] == (2 ** 21,) * 3  # the last size that fits
    with pytest.raises(ValueError, match=r"voxel_size 9\.5\d*e-07 needs more than 2\^21 voxels"):
        voxel_grid((0.0,) * 3, (0.5, 2.0, 0.5), 2.0 ** -20)  # axis 1 alone needs 2^21 + 1
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-50):  # (1e-50 is 0 in fp32)
        with pytest.raises(ValueError, match="positive and finite"):
            voxel_grid((0.0,) * 3, (1.0,) * 3, bad)
    # the host function refuses before it touches a device: a bad size first, then a cloud that is not on one
    cloud = ThermalPointCloud(torch.from_numpy(p), torch.zeros((len(p), 3), dtype=torch.uint8), torch.zeros(len(p)))
    with pytest.raises(ValueError, match="positive and finite"):
        voxel_downsample(cloud, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voxel_downsample(cloud, 0.25)
