"""GPU: tn_sort_pairs against numpy's stable argsort of the masked keys and tn_voxel_downsample against its numpy restatement
(tests/voxel_reference.py), byte for byte — sizes around the wave, the sort's tile and the 1024-wide scan's carry, every pass
count, guarded buffers, every call made twice — then voxel_downsample and the command line's --voxel-size end to end on a small
trained run."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import helpers
from tests import voxel_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (ThermalPointCloud, read_ply, sort_pairs, sort_pairs_workspace_bytes, sort_tile, subsample,
                                    voxel_downsample, voxel_downsample_workspace_bytes, write_ply)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GUARD = 96  # rows behind every output buffer that must keep their pattern
KEY_PATTERN, VALUE_PATTERN = 0x7A7A7A7A7A7A7A7A, -7


def T():
    return sort_tile()


# ---- tn_sort_pairs ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def keys_of(kind, n):
    """uint64 [n]; callers do not modify it"""
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "random":
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.uint64)
    if kind == "sorted":
        return np.sort(rng.integers(0, 2 ** 64, n, dtype=np.uint64))
    if kind == "reversed":
        return np.sort(rng.integers(0, 2 ** 64, n, dtype=np.uint64))[::-1].copy()
    if kind == "three":
        return np.array([5, 2 ** 40 + 1, 2 ** 63 + 9], np.uint64)[rng.integers(0, 3, n)]
    assert kind == "top-byte"
    return (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00ABCDEF01234567)


def sort_raw(keys, values, key_bits):
    """tn_sort_pairs itself, twice, on guarded buffers: (keys_out, values_out) as numpy.  The GUARD rows behind each output keep
    their pattern, both calls give the same bytes, the inputs are unchanged."""
    n = len(keys)
    k_in = torch.from_numpy(keys.view(np.int64).copy()).to(DEV)
    v_in = None if values is None else torch.from_numpy(values.copy()).to(DEV)
    need = sort_pairs_workspace_bytes(n)
    results = []
    for _ in range(2):
        k_out = torch.full((n + GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
        v_out = torch.full((n + GUARD,), VALUE_PATTERN, dtype=torch.int32, device=DEV)
        ws = torch.full((need // 8 + GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
        code = _hip.load().tn_sort_pairs(k_in.data_ptr(), _hip.ptr(v_in), n, key_bits, k_out.data_ptr(), v_out.data_ptr(),
                                         ws.data_ptr(), need, _hip.current_stream())
        assert code == 0, code
        k, v, w = k_out.cpu().numpy(), v_out.cpu().numpy(), ws.cpu().numpy()
        assert (k[n:] == KEY_PATTERN).all() and (v[n:] == VALUE_PATTERN).all() and (w[need // 8:] == KEY_PATTERN).all(), "written behind a buffer"
        results.append((k[:n].view(np.uint64), v[:n]))
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes(), "two calls differ"
    assert k_in.cpu().numpy().tobytes() == keys.tobytes(), "keys_in was modified"
    assert values is None or v_in.cpu().numpy().tobytes() == values.tobytes(), "values_in was modified"
    return results[0]


def sorted_as_the_reference(keys, values, key_bits, what):
    got_k, got_v = sort_raw(keys, values, key_bits)
    want_k, want_v = R.sort_pairs(keys, values, key_bits)
    bad = np.nonzero((got_k != want_k) | (got_v != want_v))[0]
    assert got_k.tobytes() == want_k.tobytes() and got_v.tobytes() == want_v.tobytes(), f"{what}: first differences at {bad[:8]} of {len(keys)}"
    return got_k, got_v


SIZES = ("1", "63", "64", "65", "T-1", "T", "T+1", "5T+17", "300000")


def size_of(name):
    return {"T-1": T() - 1, "T": T(), "T+1": T() + 1, "5T+17": 5 * T() + 17}.get(name) or int(name)


@pytest.mark.parametrize("size", SIZES)
def test_sort_sizes(size):
    """5 tiles x 256 digits already crosses the 1024-wide scan's carry; 300 000 crosses it many times"""
    n = size_of(size)
    assert T() % 256 == 0 and (size != "5T+17" or 256 * -(-n // T()) > 1024)
    sorted_as_the_reference(keys_of("random", n), None, 64, f"n = {n}")


@pytest.mark.parametrize("kind", ["random", "equal", "sorted", "reversed", "three", "top-byte"])
def test_sort_key_patterns(kind):
    """all equal: stability alone decides, the values come back 0 .. n-1"""
    n = size_of("5T+17")
    _, v = sorted_as_the_reference(keys_of(kind, n), None, 64, kind)
    if kind == "equal":
        assert np.array_equal(v, np.arange(n, dtype=np.int32))


@pytest.mark.parametrize("key_bits,passes", [(1, 1), (8, 1), (9, 2), (30, 4), (33, 5), (64, 8)])
def test_sort_key_bits_odd_and_even_pass_counts(key_bits, passes):
    """the result is in the output buffers for odd and even pass counts; bits above the ordering bits travel and do not order"""
    assert (key_bits + 7) // 8 == passes
    for n in (size_of("T+1"), size_of("5T+17")):
        keys = keys_of("random", n)
        k, v = sorted_as_the_reference(keys, None, key_bits, f"key_bits {key_bits}, n = {n}")
        assert np.array_equal(k, keys[v]), "a key left its value"
        if key_bits in (9, 30):
            mask = R.ordering_mask(key_bits)
            assert (np.diff((k & mask).astype(np.float64)) >= 0).all() and (np.diff(k.astype(np.float64)) < 0).any(), \
                "the high bits are random: the full keys are not in order, the masked ones are"


def test_sort_values_null_iota_and_given():
    n = size_of("5T+17")
    keys = keys_of("three", n)
    iota = np.arange(n, dtype=np.int32)
    k0, v0 = sorted_as_the_reference(keys, None, 64, "null values")
    k1, v1 = sorted_as_the_reference(keys, iota, 64, "iota values")
    assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes()
    other = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    _, v2 = sorted_as_the_reference(keys, other, 64, "given values")
    assert np.array_equal(v2, other[v0])
    # the wrapper: int64 and uint64 keys, the dtype kept, the permutation as the second result
    dev_keys = torch.from_numpy(keys.view(np.int64).copy()).to(DEV)
    wk, wv = sort_pairs(dev_keys)
    assert wk.dtype == torch.int64 and wk.cpu().numpy().view(np.uint64).tobytes() == k0.tobytes() and wv.cpu().numpy().tobytes() == v0.tobytes()
    wk, wv = sort_pairs(dev_keys.view(torch.uint64), torch.from_numpy(other).to(DEV), key_bits=8)
    want = R.sort_pairs(keys, other, 8)
    assert wk.dtype == torch.uint64 and wk.view(torch.int64).cpu().numpy().view(np.uint64).tobytes() == want[0].tobytes()
    assert wv.cpu().numpy().tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        sort_pairs(dev_keys, key_bits=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sort_pairs(dev_keys.cpu())
    ek, ev = sort_pairs(dev_keys[:0])
    assert tuple(ek.shape) == (0,) and tuple(ev.shape) == (0,)


def test_sort_of_nothing_touches_nothing():
    k_out = torch.full((GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
    v_out = torch.full((GUARD,), VALUE_PATTERN, dtype=torch.int32, device=DEV)
    ws = torch.full((GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
    assert _hip.load().tn_sort_pairs(k_out.data_ptr(), None, 0, 64, k_out.data_ptr(), v_out.data_ptr(), ws.data_ptr(), 8 * GUARD,
                                     _hip.current_stream()) == 0
    torch.cuda.synchronize()
    assert (k_out == KEY_PATTERN).all() and (v_out == VALUE_PATTERN).all() and (ws == KEY_PATTERN).all()


# ---- tn_voxel_downsample ----------------------------------------------------------------------------------------------------

OUTPUTS = (("positions", torch.float32, 3, -777.0), ("colors", torch.uint8, 3, 0x5A), ("temperature", torch.float32, 1, -777.0),
           ("thermal_colors", torch.uint8, 3, 0x5A), ("source", torch.int64, 1, -7), ("voxel_count", torch.int32, 1, -7))


def voxel_raw(cloud, origin, voxel_size, dims, capacity=None):
    """tn_voxel_downsample itself, twice, on guarded buffers: (dict of numpy outputs cut to min(count, capacity), count).  Rows at
    or beyond the capacity and the GUARD rows behind keep their pattern; both calls give the same bytes.  ``capacity`` None: the
    number of points; 0: the sizing call with null outputs."""
    p, colors, temperature, thermal, source = cloud
    n = len(p)
    capacity = n if capacity is None else capacity
    dev_in = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (p, colors, temperature, thermal, source)]
    q = _hip.tn_voxel_params()
    q.origin[:], q.voxel_size, q.dims[:] = [float(v) for v in origin], float(voxel_size), [int(v) for v in dims]
    need = voxel_downsample_workspace_bytes(n)
    results = []
    for _ in range(2):
        outs = {}
        for name, dtype, width, pattern in OUTPUTS:
            absent = capacity == 0 or (name == "thermal_colors" and thermal is None) or (name == "source" and source is None)
            outs[name] = None if absent else torch.full((capacity + GUARD, width), pattern, dtype=dtype, device=DEV)
        count = torch.full((1 + GUARD,), -7, dtype=torch.int64, device=DEV)
        ws = torch.full((need // 8 + GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
        code = _hip.load().tn_voxel_downsample(
            *[(_hip.ptr(t) if n else None) for t in dev_in], n, q, *[_hip.ptr(outs[name]) for name, *_ in OUTPUTS[:5]],
            _hip.ptr(outs["voxel_count"]), capacity, count.data_ptr(), ws.data_ptr() if n else None, need, _hip.current_stream())
        assert code == 0, code
        count = count.cpu().numpy()
        assert (count[1:] == -7).all() and (ws.cpu().numpy()[need // 8:] == KEY_PATTERN).all(), "written behind count or the workspace"
        full = int(count[0])
        written = min(full, capacity)
        got = {}
        for name, dtype, width, pattern in OUTPUTS:
            if outs[name] is None:
                got[name] = None
                continue
            a = outs[name].cpu().numpy()
            assert (a[written:] == a.dtype.type(pattern)).all(), f"{name}: written at or beyond min(count, capacity)"
            got[name] = a[:written] if width == 3 else a[:written, 0]
        results.append((got, full))
    for name, *_ in OUTPUTS:
        a, b = results[0][0][name], results[1][0][name]
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), f"{name}: two calls differ"
    assert results[0][1] == results[1][1]
    for t, a in zip(dev_in, (p, colors, temperature, thermal, source)):
        assert t is None or t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input was modified"
    return results[0]


def as_the_reference(cloud, origin, voxel_size, dims, what):
    got, count = voxel_raw(cloud, origin, voxel_size, dims)
    want = R.voxel_downsample(*cloud, origin, voxel_size, dims)
    assert count == len(want["voxel_count"]), f"{what}: {count} voxels, the reference has {len(want['voxel_count'])}"
    for name, *_ in OUTPUTS:
        if want[name] is None:
            assert got[name] is None
        else:
            assert got[name].tobytes() == want[name].tobytes(), f"{what}: {name} differs"
    assert int(got["voxel_count"].sum()) == want["members"]
    return got, want


@functools.lru_cache(maxsize=None)
def random_cloud(n=20000, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (n, 3)).astype(F),) + R.attributes(n, rng)


def test_voxel_lattices():
    cloud = R.lattice(side=6, step=0.25)
    for size, members in ((0.25, 1), (0.5, 8)):
        origin, dims = R.grid_of(cloud[0], size)
        got, _ = as_the_reference(cloud, origin, size, dims, f"lattice at {size}")
        assert (got["voxel_count"] == members).all() and len(got["voxel_count"]) == 216 // members


@pytest.mark.parametrize("voxel_size", [0.01, 0.11, 0.5])
def test_voxel_random_points(voxel_size):
    """0.01: about one member per voxel and 24 key bits; 0.11 is no power of two (the fp64 coordinate rule at faces); 0.5: 64 voxels"""
    cloud = random_cloud()
    origin, dims = R.grid_of(cloud[0], voxel_size)
    got, _ = as_the_reference(cloud, origin, voxel_size, dims, f"voxel size {voxel_size}")
    voxels = len(got["voxel_count"])
    assert {0.01: voxels > 19000, 0.11: 4000 < voxels < 8000, 0.5: voxels == 64}[voxel_size], voxels


def test_voxel_one_long_walk_and_duplicates():
    rng = np.random.default_rng(3)
    p = rng.uniform(0.0, 1.0, (5000, 3)).astype(F)
    got, _ = as_the_reference((p,) + R.attributes(5000, rng), np.zeros(3, F), 1.0, np.ones(3, np.int32), "one voxel of 5000")
    assert got["voxel_count"].tolist() == [5000]
    d = np.concatenate([np.tile(np.array([[0.3, -0.2, 0.7]], F), (300, 1)), rng.uniform(-1.0, 1.0, (50, 3)).astype(F)])
    d = d[rng.permutation(len(d))]
    origin, dims = R.grid_of(d, 0.05)
    got, _ = as_the_reference((d,) + R.attributes(len(d), rng), origin, 0.05, dims, "300 duplicates")
    assert got["voxel_count"].max() >= 300 and int(got["voxel_count"].sum()) == 350


def test_voxel_non_finite_and_outside_points_are_dropped():
    p, colors, temperature, thermal, source = random_cloud()
    p = p[:3000].copy()
    for row, (c, v) in {0: (0, np.nan), 63: (1, np.inf), 64: (2, -np.inf), 257: (0, np.nan), 2999: (2, np.inf)}.items():
        p[row, c] = v
    cloud = (p, colors[:3000], temperature[:3000], thermal[:3000], source[:3000])
    origin, dims = R.grid_of(p, 0.11)
    got, want = as_the_reference(cloud, origin, 0.11, dims, "non-finite rows")
    assert want["members"] == 2995
    # a grid smaller than the cloud; one point exactly ON the upper face u = dims (dropped), one ON the lower face u = 0 (kept)
    origin, dims = np.array([-0.5, -0.25, -0.75], F), np.array([8, 3, 11], np.int32)
    p[5] = [-0.5 + 8 * 0.125, 0.0, 0.0]
    p[6] = [-0.5, -0.25, -0.75]
    keys, total = R.voxel_keys(p, origin, 0.125, dims)
    assert keys[5] == total and keys[6] == 0 and 0 < (keys == total).sum() < len(p) - 100
    as_the_reference(cloud, origin, 0.125, dims, "points outside the grid")
    # no point inside at all, and no finite point at all
    got, count = voxel_raw(cloud, np.array([5.0, 5.0, 5.0], F), 0.125, dims)
    assert count == 0 and len(got["positions"]) == 0
    got, count = voxel_raw((np.full((70, 3), np.nan, F),) + tuple(a[:70] for a in cloud[1:]), origin, 0.125, dims)
    assert count == 0


def test_voxel_null_attributes_sizing_call_small_capacity_and_nothing():
    p, colors, temperature, thermal, source = random_cloud()
    cloud = (p[:5000], colors[:5000], temperature[:5000], None, None)
    origin, dims = R.grid_of(cloud[0], 0.11)
    got, want = as_the_reference(cloud, origin, 0.11, dims, "thermal_colors and source null")
    assert got["thermal_colors"] is None and got["source"] is None
    full = len(want["voxel_count"])
    _, count = voxel_raw(cloud, origin, 0.11, dims, capacity=0)
    assert count == full, "the sizing call"
    part, count = voxel_raw(cloud, origin, 0.11, dims, capacity=full // 3)
    assert count == full and len(part["positions"]) == full // 3
    for name in ("positions", "colors", "temperature", "voxel_count"):
        assert part[name].tobytes() == want[name][:full // 3].tobytes(), name
    empty = tuple(a[:0] for a in random_cloud())
    got, count = voxel_raw(empty, origin, 0.11, dims, capacity=0)
    assert count == 0, "n = 0 overwrites the count with 0"
    got, count = voxel_raw(empty, origin, 0.11, dims, capacity=16)
    assert count == 0 and len(got["positions"]) == 0


def device_cloud(cloud, normals=False):
    p, colors, temperature, thermal, source = cloud
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in cloud]
    return ThermalPointCloud(*dev, temperature_bounds=(14.0, 33.0), normals=torch.ones((len(p), 3), device=DEV) if normals else None)


def test_voxel_downsample_host_function():
    p, colors, temperature, thermal, source = random_cloud()
    p = p[:6000].copy()
    p[17, 1], p[4000, 0] = np.nan, np.inf
    cloud = (p, colors[:6000], temperature[:6000], thermal[:6000], source[:6000])
    for size in (0.11, 0.5):
        origin, dims = R.grid_of(p, size)
        want = R.voxel_downsample(*cloud, origin, size, dims)
        out, counts = voxel_downsample(device_cloud(cloud, normals=True), size)
        assert len(out) == len(want["voxel_count"]) and counts.dtype == torch.int32
        for name in ("positions", "colors", "temperature", "thermal_colors", "source"):
            assert getattr(out, name).cpu().numpy().tobytes() == want[name].tobytes(), name
        assert counts.cpu().numpy().tobytes() == want["voxel_count"].tobytes() and int(counts.sum()) == 5998
        assert out.normals is None and out.temperature_bounds == (14.0, 33.0)
    bare, counts = voxel_downsample(device_cloud(cloud[:3] + (None, None)), 0.5)
    assert bare.thermal_colors is None and bare.source is None and len(bare) == len(counts) == len(want["voxel_count"])
    for none in (device_cloud(tuple(a[:0] for a in cloud)), device_cloud((np.full((9, 3), np.nan, F),) + tuple(a[:9] for a in cloud[1:]))):
        out, counts = voxel_downsample(none, 0.5)
        assert len(out) == 0 and tuple(counts.shape) == (0,) and out.temperature_bounds == (14.0, 33.0)
    with pytest.raises(ValueError, match="2\\^21 voxels"):
        voxel_downsample(device_cloud(cloud), 1e-7)


# ---- the command line ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trained_run(tmp_path_factory):
    """the small trained run of tests/test_gpu_neighbors.py's command-line test: (run directory, dataset, export tool)"""
    from tests.test_gpu_neighbors import _tool, _write_tree

    root = tmp_path_factory.mktemp("voxel_cli")
    data = root / "data"
    _write_tree(data)
    small = root / "small.json"
    small.write_text(json.dumps(helpers.SMALL))
    models = root / "models"
    assert _tool("train_eval").main(["--data", str(data), "--experiment-name", "cloud", "--model-output-folder", str(models),
                                     "--metrics-output-folder", str(root / "metrics"), "--max-num-iterations", "30",
                                     "--config-json", str(small), "--temperature-bounds", "33", "14", "--device", DEV]) == 0
    return next((models / "cloud" / "thermal-nerf").iterdir()), data, _tool("export_pointcloud")


def test_command_line_voxel_size(trained_run, tmp_path, capsys):
    from tests.test_gpu_neighbors import CLI_FILTER

    run_dir, data, tool = trained_run
    common = [str(run_dir), str(data), "--device", DEV] + CLI_FILTER
    args = tool.parse(common + ["--output", str(tmp_path / "unused.ply")])
    exporter, cameras, adjust = tool.build_exporter(args)
    full = exporter.export(cameras, apply_camera_optimizer=adjust)
    p = full.positions.cpu().numpy()
    size = float((p.max(axis=0) - p.min(axis=0)).max()) / 16.0  # at most 16^3 voxels: the filter must bite
    down, counts = voxel_downsample(full, size)
    print("exported", len(full), "voxel size", size, "voxels", len(down))
    assert 1 < len(down) < len(full) and int(counts.sum()) == len(full)
    keep = len(down) // 2

    # --voxel-size: export -> voxel_downsample -> subsample -> write_ply, byte for byte
    capsys.readouterr()
    voxel, plain = tmp_path / "voxel.ply", tmp_path / "plain.ply"
    assert tool.main(common + ["--num-points", str(keep), "--voxel-size", repr(size), "--output", str(voxel)]) == 0
    printed = capsys.readouterr().out
    want = write_ply(tmp_path / "want.ply", subsample(down, keep))
    assert voxel.read_bytes() == want.read_bytes()
    assert printed.splitlines()[0] == f"rays cast 8192, kept {len(full)}, voxels {len(down)} of {len(full)}, written {keep} -> {voxel}"

    # without the switch: the file and the line of before
    assert tool.main(common + ["--num-points", "500", "--output", str(plain)]) == 0
    printed = capsys.readouterr().out
    old = write_ply(tmp_path / "old.ply", subsample(full, 500))
    assert plain.read_bytes() == old.read_bytes() and plain.read_bytes() != voxel.read_bytes()
    assert printed.splitlines()[0] == f"rays cast 8192, kept {len(full)}, written 500 -> {plain}"

    # with outlier removal before and normals after: the count of the down-sampled cloud, every normal unit or zero
    from thermo_nerf_amd.export import remove_statistical_outliers

    rich = tmp_path / "rich.ply"
    assert tool.main(common + ["--num-points", "1000000", "--voxel-size", repr(size), "--remove-outliers", "--outlier-neighbors", "9",
                               "--outlier-std-ratio", "1.0", "--normals", "--normal-neighbors", "12", "--output", str(rich)]) == 0
    printed = capsys.readouterr().out
    cleaned, _ = remove_statistical_outliers(full, 9, 1.0)
    down_cleaned, _ = voxel_downsample(cleaned, size)
    got = read_ply(rich)
    assert len(got["positions"]) == len(down_cleaned) and got["positions"].tobytes() == down_cleaned.positions.cpu().numpy().tobytes()
    assert f"outliers removed {len(full) - len(cleaned)}, voxels {len(down_cleaned)} of {len(cleaned)}, written {len(down_cleaned)}" in printed
    norm = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert ((np.abs(norm - 1.0) < 1e-6) | (norm == 0.0)).all()
