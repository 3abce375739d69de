"""tn_mesh_simplify on the device against tests/mesh_simplify_reference.py, exactly (integers and float bit patterns), into guarded
buffers: the literal cases, sizes around the block, the sort's tile and a scan pass, random meshes with invalid and repeated
indices and non-member vertices, the finest and the coarsest grid, a long walk, a sparse mesh, both sides of the one-sort / two-sort
threshold, the sphere mesh, determinism, empty meshes, the sizing call, small capacities, the error codes, the Python layer, the
exporter and the command line."""
from __future__ import annotations

import copy
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import helpers, mesh_reference
from tests import mesh_simplify_reference as R
from tests import voxel_reference
from tests.mesh_components_reference import random_mesh
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (MeshExporter, PointCloudExporter, SimplifyInfo, ThermalMesh, ThermalPointCloud, mesh_scan_width,
                                    mesh_simplify_into, mesh_simplify_workspace_bytes, mesh_tile, read_mesh_ply,
                                    remove_small_components, simplify_mesh, smooth_mesh, sort_tile, voxel_downsample, voxel_grid,
                                    voxel_params)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILLS = {torch.int32: -5, torch.float32: -777.0, torch.uint8: 0xEE, torch.int64: -9}
NAMES = ("positions", "colors", "temperature", "thermal_colors", "triangles", "num_vertices", "num_triangles", "params",
         "positions_out", "colors_out", "temperature_out", "thermal_colors_out", "cluster_count", "capacity_vertices",
         "triangles_out", "triangle_source", "capacity_triangles", "vertex_map", "counts", "workspace", "workspace_bytes", "stream")
OUTPUTS = {"positions_out": (torch.float32, 3), "colors_out": (torch.uint8, 3), "temperature_out": (torch.float32, 1),
           "thermal_colors_out": (torch.uint8, 3), "cluster_count": (torch.int32, 1), "triangles_out": (torch.int32, 3),
           "triangle_source": (torch.int32, 1), "vertex_map": (torch.int32, 1)}
WANT_KEY = {"positions_out": "positions", "colors_out": "colors", "temperature_out": "temperature",
            "thermal_colors_out": "thermal_colors", "cluster_count": "cluster_count", "triangles_out": "triangles",
            "triangle_source": "triangle_source", "vertex_map": "vertex_map"}


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw(mesh, grid, cap_v=None, cap_t=None, absent=()):
    """tn_mesh_simplify into guarded buffers of ``cap_v`` / ``cap_t`` rows (default V and T; 0: the output is NULL), the outputs
    named in ``absent`` NULL: dict of the host arrays (every row below the capacity), the buffers and the counts"""
    pos, colors, temperature, thermal, tri = mesh
    v, t = len(pos), len(tri)
    cap_v, cap_t = v if cap_v is None else cap_v, t if cap_t is None else cap_t
    inputs = [_device(a) for a in (pos, colors, temperature, thermal, np.ascontiguousarray(tri, dtype=np.int32))]
    rows = {"triangles_out": cap_t, "triangle_source": cap_t, "vertex_map": v}
    buffers = {}
    for name, (dtype, width) in OUTPUTS.items():
        n = rows.get(name, cap_v)
        skip = name in absent or (name == "thermal_colors_out" and thermal is None) or (n == 0 and name != "vertex_map")
        buffers[name] = None if skip else _buffer(n * width, dtype)
    counts = _buffer(4, torch.int64)
    need = mesh_simplify_workspace_bytes(v, t)
    workspace = _buffer(need, torch.uint8)
    params = voxel_params(grid["origin"], grid["voxel_size"], grid["dims"])
    args = dict(zip(NAMES[:5], [_hip.ptr(a) if len(a) else None for a in inputs[:3]] + [_hip.ptr(inputs[3]) if v else None]
                    + [inputs[4].data_ptr() if t else None]))
    args.update(num_vertices=v, num_triangles=t, params=ctypes.byref(params), capacity_vertices=cap_v, capacity_triangles=cap_t,
                counts=counts.data_ptr(), workspace=workspace.data_ptr() if v else None, workspace_bytes=need,
                stream=_hip.current_stream(), **{k: _hip.ptr(b) for k, b in buffers.items()})
    _hip.check(_hip.load().tn_mesh_simplify(*[args[k] for k in NAMES]), "tn_mesh_simplify")
    torch.cuda.synchronize()
    _untouched(counts, 4, "counts")
    _untouched(workspace, need, "workspace")
    for name, buf in buffers.items():
        if buf is not None:
            _untouched(buf, buf.numel() - GUARD, name)
    for given, now in zip((pos, colors, temperature, thermal, tri), inputs):
        assert given is None or np.ascontiguousarray(given).tobytes() == now.cpu().numpy().tobytes(), "an input was written"
    return {"buffers": buffers, "counts": counts[:4].cpu().numpy(), "cap": (cap_v, cap_t)}


def check(mesh, grid, want=None, **kw):
    """one call compared with the yardstick (or ``want``) on every output it was given: the rows below min(count, capacity)"""
    want = R.simplify(*mesh, grid["origin"], grid["voxel_size"], grid["dims"]) if want is None else want
    got = raw(mesh, grid, **kw)
    assert got["counts"].tolist() == want["counts"].tolist(), "counts"
    assert int(got["counts"][1:].sum()) == len(mesh[4])
    cap_v, cap_t = got["cap"]
    for name, buf in got["buffers"].items():
        if buf is None:
            continue
        w = want[WANT_KEY[name]]
        rows = len(w) if name == "vertex_map" else min(len(w), cap_t if name in ("triangles_out", "triangle_source") else cap_v)
        w = np.ascontiguousarray(w[:rows])
        g = buf[:w.size].cpu().numpy()
        assert g.tobytes() == w.tobytes(), name
    return want, got


def random_case(seed, v, t, extent=8.0, thermal=True, bad=0.03):
    pos = R.random_positions(seed, v, extent, bad)
    colors, temperature, thermal_colors = R.random_attributes(seed, v, thermal)
    tri = random_mesh(seed, v, t, invalid=0.03) if t and v else np.zeros((0, 3), np.int32)
    return pos, colors, temperature, thermal_colors, tri


def grid_over(extent, voxel_size):
    return dict(origin=(0.0, 0.0, 0.0), voxel_size=voxel_size, dims=(int(extent / voxel_size) + 1,) * 3)


# ---- the literal cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_literal_cases_through_the_kernel(name):
    case = R.LITERAL[name]
    check(R.literal_arrays(case), R.GRID, want=R.literal_want(case))


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

def _sizes():
    tile, sort, scan = 256, 2048, 1024  # asserted against the library in the test
    return [n + d for n in (tile, sort, scan * tile) for d in (-1, 0, 1)]


@pytest.mark.parametrize("n", _sizes())
def test_vertex_and_triangle_counts_around_the_tile_the_sort_tile_and_a_scan_pass(n):
    assert (mesh_tile(), sort_tile(), mesh_scan_width()) == (256, 2048, 1024)
    small = min(n, 3000)
    # V at the size with a few thousand triangles, then T at the size over a few thousand vertices; cells of two to three vertices
    want, _ = check(random_case(n, n, small, extent=2.0 * round(n ** (1 / 3))), grid_over(2.0 * round(n ** (1 / 3)), 2.5))
    assert want["counts"][0] > 0
    extent = 2.0 * round(small ** (1 / 3))
    want, _ = check(random_case(n + 1, small, n, extent=extent, thermal=False), grid_over(extent, 2.5))
    assert want["counts"][1] > 0 and want["counts"][2] > 0


@pytest.mark.parametrize("seed, v, t, size", [(31, 3000, 400, 1.0), (32, 3000, 9000, 0.7), (33, 5000, 9000, 2.0), (34, 700, 9000, 1.3)])
def test_random_meshes_with_invalid_and_repeated_indices_and_non_members(seed, v, t, size):
    mesh = random_case(seed, v, t)
    want, _ = check(mesh, grid_over(8.0, size))
    m, k, dropped, duplicate = want["counts"]
    assert m > 0 and k > 0 and dropped > 0
    assert not np.isfinite(mesh[0]).all() and (mesh[0] >= 8.0).any() and (mesh[4] < 0).any() and (mesh[4][:, 0] == mesh[4][:, 1]).any()
    if seed == 34:
        assert duplicate > 0, "many triangles over few cells repeat"


# ---- the two ends of the cell size --------------------------------------------------------------------------------------------------------

def test_a_grid_so_fine_that_no_two_vertices_share_a_cell_only_re_indexes():
    v, t = 2500, 4000
    rng = np.random.default_rng(41)
    cells = rng.permutation(64 ** 3)[:v]  # one cell each
    pos = (np.stack([cells % 64, cells // 64 % 64, cells // 4096], axis=1) + rng.uniform(0.1, 0.9, (v, 3))).astype(F)
    colors, temperature, thermal = R.random_attributes(41, v)
    tri = random_mesh(41, v, t, invalid=0.0)
    mesh = (pos, colors, temperature, thermal, tri)
    want, got = check(mesh, dict(origin=(0.0, 0.0, 0.0), voxel_size=1.0, dims=(64, 64, 64)))
    m, k = int(want["counts"][0]), int(want["counts"][1])
    vertex_map = got["buffers"]["vertex_map"][:v].cpu().numpy()
    # a triangle goes only for a repeated index or as a copy of an earlier one; the others are the input's, re-indexed
    source = got["buffers"]["triangle_source"][:k].cpu().numpy()
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    assert want["counts"][2] == int((~distinct).sum()) and set(source.tolist()) <= set(np.flatnonzero(distinct).tolist())
    assert np.array_equal(got["buffers"]["triangles_out"][:3 * k].cpu().numpy().reshape(-1, 3), vertex_map[tri[source]])
    # every referenced vertex is kept with its own attributes, bit for bit
    referenced = np.zeros(v, bool)
    referenced[tri[source].reshape(-1)] = True
    assert np.array_equal(vertex_map >= 0, referenced) and m == int(referenced.sum())
    kept = np.flatnonzero(referenced)
    order = vertex_map[kept]
    assert sorted(order.tolist()) == list(range(m))
    b = got["buffers"]
    assert np.array_equal(R.bits(b["positions_out"][:3 * m].cpu().numpy().reshape(-1, 3)[order]), R.bits(pos[kept]))
    assert np.array_equal(R.bits(b["temperature_out"][:m].cpu().numpy()[order]), R.bits(temperature[kept]))
    assert np.array_equal(b["colors_out"][:3 * m].cpu().numpy().reshape(-1, 3)[order], colors[kept])
    assert np.array_equal(b["thermal_colors_out"][:3 * m].cpu().numpy().reshape(-1, 3)[order], thermal[kept])
    assert bool((b["cluster_count"][:m] == 1).all())


def test_a_grid_of_one_cell_leaves_nothing():
    mesh = random_case(42, 1500, 2600, bad=0.0)
    want, got = check(mesh, dict(origin=(0.0, 0.0, 0.0), voxel_size=8.0, dims=(1, 1, 1)))
    assert got["counts"].tolist() == [0, 0, 2600, 0] and bool((got["buffers"]["vertex_map"][:1500] == -1).all())


def test_one_cluster_of_ten_thousand_members_the_long_walk():
    v = 10000 + 600
    pos = R.random_positions(43, v, extent=1.0, bad=0.0)  # 10^4 vertices in cell 0 ...
    pos[10000:] += np.array([1.0, 0.0, 0.0], F) + np.random.default_rng(43).integers(0, 5, (600, 3)).astype(F)  # ... the others around it
    colors, temperature, thermal = R.random_attributes(43, v)
    tri = random_mesh(43, v, 3000, invalid=0.01)
    tri[::7, 0] = np.arange(len(tri[::7])) % 10000  # triangles between the big cluster and the rest
    tri[::7, 1] = 10000 + np.arange(len(tri[::7])) % 600
    want, _ = check((pos, colors, temperature, thermal, tri), dict(origin=(0.0, 0.0, 0.0), voxel_size=1.0, dims=(6, 5, 5)))
    assert int(want["cluster_count"][0]) == 10000 and want["counts"][1] > 0


def test_sparse_mesh_a_few_triangles_over_a_hundred_thousand_vertices():
    mesh = random_case(44, 100000, 40, extent=40.0)
    want, _ = check(mesh, grid_over(40.0, 1.0))
    assert 0 < want["counts"][0] <= 120 and int((want["vertex_map"] >= 0).sum()) < 1000


# ---- one sort of the triples below 2^21 vertices, two from there on ---------------------------------------------------------------------------

def _wide_mesh(v, seed):
    """v vertices on a 2048-wide lattice of unit cells, one per cell, with a few hundred triangles among forty of them — low and
    high indices — so that triples repeat, rotate, flip and share two of their three clusters"""
    i = np.arange(v)
    pos = (np.stack([i % 2048, i // 2048, np.zeros_like(i)], axis=1) + 0.5).astype(F)
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(0, v, 30), [0, 1, v - 1, v - 2, v - 3, 2 ** 20, 2 ** 20 + 1, 2047, 2048, v // 3]])
    tri = pool[rng.integers(0, len(pool), (300, 3))].astype(np.int32)
    tri[5, 2], tri[9, 0] = v, -1
    tri[10], tri[20], tri[21], tri[22] = (0, v - 1, 2 ** 20), (v - 1, 2 ** 20, 0), (0, 2 ** 20, v - 1), (0, v - 1, 2 ** 20 + 3)
    colors, temperature, _ = R.random_attributes(seed, v, thermal=False)
    return pos, colors, temperature, None, tri


@pytest.mark.parametrize("v, size", [(2 ** 21 - 1, 1.0), (2 ** 21, 2.0), (2 ** 21 + 5, 1.0)])
def test_both_sides_of_the_one_sort_two_sorts_threshold(v, size):
    lib = _hip.load()
    assert lib.tn_mesh_simplify_workspace_bytes(2 ** 21, 300) - lib.tn_mesh_simplify_workspace_bytes(2 ** 21 - 1, 300) >= 300 * 20
    mesh = _wide_mesh(v, v % 97)
    rows = (v + 2047) // 2048
    want, _ = check(mesh, dict(origin=(0.0, 0.0, 0.0), voxel_size=size, dims=(int(2048 / size), int(rows / size) + 1, 1)),
                    absent=("thermal_colors_out",))
    m, k, dropped, duplicate = want["counts"]
    assert k > 100 and dropped >= 2 and duplicate > 0 and m <= 45


# ---- the sphere mesh --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sphere():
    mesh = mesh_reference.sphere_mesh()[1]
    pos, tri = mesh["positions"], mesh["triangles"]
    colors, _, thermal = R.random_attributes(3, len(pos))
    return pos, colors, mesh["temperature"], thermal, tri


@pytest.mark.parametrize("steps", [1.5, 2.0, 4.0])
def test_sphere_mesh(steps):
    mesh = _sphere()
    pos, tri = mesh[0], mesh[4]
    size = steps / 23.0
    origin, dims = voxel_grid(pos.min(axis=0).tolist(), pos.max(axis=0).tolist(), size)
    want, got = check(mesh, dict(origin=origin, voxel_size=size, dims=dims))
    m, k, dropped, duplicate = (int(c) for c in got["counts"])
    assert k + dropped + duplicate == len(tri) and 0 < m < len(pos) and 0 < k < len(tri)
    out = got["buffers"]["triangles_out"][:3 * k].cpu().numpy().reshape(-1, 3)
    assert out.min() >= 0 and out.max() < m and all(len(set(row)) == 3 for row in out.tolist())
    assert set(out.reshape(-1).tolist()) == set(range(m)), "every output vertex is in a triangle"
    # the Python layer on the same mesh: the same arrays at their exact sizes
    device = ThermalMesh(*[_device(a) for a in mesh], temperature_bounds=(14.0, 33.0), normals=torch.ones((len(pos), 3), device=DEV))
    simple, info = simplify_mesh(device, size)
    assert isinstance(info, SimplifyInfo) and (info.vertices_before, info.triangles_before) == (len(pos), len(tri))
    assert (info.vertices_after, info.triangles_after, info.degenerate_triangles, info.duplicate_triangles) == (m, k, dropped, duplicate)
    assert len(simple) == m and simple.normals is None and simple.temperature_bounds == (14.0, 33.0) and device.normals is not None
    for key in ("positions", "colors", "temperature", "thermal_colors", "triangles"):
        assert getattr(simple, key).cpu().numpy().tobytes() == want[key].tobytes(), key
    assert info.cluster_count.cpu().numpy().tobytes() == want["cluster_count"].tobytes()


# ---- determinism, empty meshes, the sizing call, small capacities ------------------------------------------------------------------------

def test_the_same_call_twice_gives_identical_bytes():
    mesh, grid = random_case(51, 6000, 11000), grid_over(8.0, 0.9)
    first, second = raw(mesh, grid), raw(mesh, grid)
    assert first["counts"].tobytes() == second["counts"].tobytes()
    for name, buf in first["buffers"].items():
        assert torch.equal(buf, second["buffers"][name]), name


def test_no_vertices_and_no_triangles():
    none = random_case(52, 0, 0)
    for mesh in (none, none[:4] + (np.array([[0, 1, 2]], np.int32),)):
        # V == 0 is the one early exit that zeroes counts by a memset: the triangles, all invalid, are not looked at
        want = dict(R.simplify(*mesh, (0.0, 0.0, 0.0), 1.0, (9, 9, 9)), counts=np.zeros(4, np.int64))
        got = raw(mesh, grid_over(8.0, 1.0))
        assert got["counts"].tolist() == [0, 0, 0, 0] and len(want["triangles"]) == 0
        assert all(b is None for k, b in got["buffers"].items() if k not in ("triangles_out", "triangle_source", "vertex_map"))
        for name in ("triangles_out", "triangle_source", "vertex_map"):
            if got["buffers"][name] is not None:
                _untouched(got["buffers"][name], 0, name)
    mesh = random_case(53, 700, 0)
    want, got = check(mesh, grid_over(8.0, 1.0))
    assert got["counts"].tolist() == [0, 0, 0, 0] and bool((got["buffers"]["vertex_map"][:700] == -1).all())
    for name in ("positions_out", "cluster_count"):
        _untouched(got["buffers"][name], 0, name)
    check(mesh, grid_over(8.0, 1.0), absent=("vertex_map",))


def test_sizing_call_writes_nothing_but_the_counts():
    mesh, grid = random_case(54, 3000, 5000), grid_over(8.0, 1.1)
    want, got = check(mesh, grid, cap_v=0, cap_t=0, absent=("vertex_map",))
    assert all(b is None for b in got["buffers"].values()) and got["counts"][0] > 0
    # the Python layer's raw entry: counts alone, then exact allocation from them
    device = ThermalMesh(*[_device(a) for a in mesh])
    counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    params = voxel_params(grid["origin"], grid["voxel_size"], grid["dims"])
    mesh_simplify_into(device, params, counts=counts)
    assert counts.tolist() == want["counts"].tolist()
    m, k = int(counts[0]), int(counts[1])
    outs = dict(positions=torch.empty((m, 3), device=DEV), colors=torch.empty((m, 3), dtype=torch.uint8, device=DEV),
                temperature=torch.empty((m,), device=DEV), cluster_count=torch.empty((m,), dtype=torch.int32, device=DEV),
                thermal_colors=torch.empty((m, 3), dtype=torch.uint8, device=DEV), triangles=torch.empty((k, 3), dtype=torch.int32, device=DEV),
                triangle_source=torch.empty((k,), dtype=torch.int32, device=DEV), vertex_map=torch.empty((3000,), dtype=torch.int32, device=DEV))
    mesh_simplify_into(device, params, counts=counts, **outs)
    for key, out in outs.items():
        assert out.cpu().numpy().tobytes() == want[key].tobytes(), key
    with pytest.raises(ValueError):
        mesh_simplify_into(device, params, counts=counts, positions=outs["positions"])  # the other vertex outputs are missing
    with pytest.raises(ValueError):
        mesh_simplify_into(ThermalMesh(device.positions, device.colors, device.temperature, None, device.triangles), params,
                           counts=counts, thermal_colors=outs["thermal_colors"], capacity_vertices=0)
    with pytest.raises(ValueError):
        mesh_simplify_into(device, params, counts=counts, workspace=torch.empty((64,), dtype=torch.uint8, device=DEV))


def test_capacities_below_the_result_write_nothing_beyond_them_and_report_the_full_counts():
    mesh, grid = random_case(55, 3000, 5000), grid_over(8.0, 1.1)
    want = R.simplify(*mesh, grid["origin"], grid["voxel_size"], grid["dims"])
    m, k = int(want["counts"][0]), int(want["counts"][1])
    assert m > 300 and k > 300
    for cap_v, cap_t in ((m // 2, k // 2), (m - 1, k + 5), (257, 1), (m + 5, 0), (0, k)):
        check(mesh, grid, want=want, cap_v=cap_v, cap_t=cap_t)


def test_optional_outputs_absent():
    mesh, grid = random_case(56, 2000, 3000), grid_over(8.0, 1.2)
    for absent in (("vertex_map",), ("triangle_source",), ("vertex_map", "triangle_source", "thermal_colors_out")):
        check(mesh, grid, absent=absent)
    check(random_case(56, 2000, 3000, thermal=False), grid)


# ---- the error codes ------------------------------------------------------------------------------------------------------------------------

def test_error_codes_without_a_launch():
    lib = _hip.load()
    v, t = 700, 900
    mesh = random_case(57, v, t)
    inputs = [_device(a) for a in mesh]
    buffers = {name: _buffer((t if name in ("triangles_out", "triangle_source") else v) * width, dtype)
               for name, (dtype, width) in OUTPUTS.items()}
    counts = _buffer(4, torch.int64)
    need = mesh_simplify_workspace_bytes(v, t)
    ws = _buffer(need, torch.uint8)
    params = voxel_params((0.0, 0.0, 0.0), 1.0, (9, 9, 9))
    good = dict(zip(NAMES[:5], [a.data_ptr() for a in inputs]))
    good.update(num_vertices=v, num_triangles=t, params=params, capacity_vertices=v, capacity_triangles=t, counts=counts.data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=need, stream=_hip.current_stream(), **{k: b.data_ptr() for k, b in buffers.items()})

    def call(**change):
        args = dict(good, **change)
        args["params"] = None if args["params"] is None else ctypes.byref(args["params"])
        return lib.tn_mesh_simplify(*[args[k] for k in NAMES])

    for k in ("positions", "colors", "temperature", "triangles", "params", "positions_out", "colors_out", "temperature_out",
              "cluster_count", "triangles_out", "counts", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    assert call(thermal_colors=None) == -1, "thermal_colors_out without thermal_colors"
    limit = (2 ** 31 - 1) // 3
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2  # TN_ERR_SHAPE
    assert call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert call(capacity_vertices=-1) == -2 and call(capacity_triangles=-1) == -2
    for k in ("positions", "temperature", "triangles", "positions_out", "temperature_out", "cluster_count", "triangles_out",
              "triangle_source", "vertex_map"):
        assert call(**{k: good[k] + 2}) == -2, k
    assert call(counts=good["counts"] + 4) == -2 and call(workspace=good["workspace"] + 4) == -2
    for bad in (voxel_params((0, 0, 0), 0.0, (9, 9, 9)), voxel_params((0, 0, 0), -1.0, (9, 9, 9)),
                voxel_params((0, 0, 0), float("nan"), (9, 9, 9)), voxel_params((0, 0, 0), float("inf"), (9, 9, 9)),
                voxel_params((0, 0, 0), 1.0, (9, 0, 9)), voxel_params((0, 0, 0), 1.0, (2 ** 21 + 1, 9, 9))):
        assert call(params=bad) == -3  # TN_ERR_UNSUPPORTED
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    assert lib.tn_mesh_simplify_workspace_bytes(-1, 0) == 0 and lib.tn_mesh_simplify_workspace_bytes(0, limit + 1) == 0
    assert lib.tn_mesh_simplify_workspace_bytes(2 ** 31, 0) == 0 and lib.tn_mesh_simplify_workspace_bytes(2 ** 31 - 1, limit) > 0
    torch.cuda.synchronize()
    for name, buf in list(buffers.items()) + [("counts", counts), ("workspace", ws)]:
        _untouched(buf, 0, name)
    assert call() == 0
    torch.cuda.synchronize()
    assert counts[:4].tolist() == R.simplify(*mesh, (0.0, 0.0, 0.0), 1.0, (9, 9, 9))["counts"].tolist()
    device = ThermalMesh(*inputs)
    with pytest.raises(ValueError, match="cell_size"):
        simplify_mesh(device, -1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        simplify_mesh(device, 1e-7)
    with pytest.raises(ValueError, match="no triangles"):
        simplify_mesh(ThermalMesh(*inputs[:4]), 1.0)
    with pytest.raises(TypeError):
        simplify_mesh(ThermalMesh(inputs[0].double(), *inputs[1:]), 1.0)


def test_simplify_mesh_of_nothing_and_of_no_finite_vertex():
    mesh = random_case(58, 50, 80)
    for pos in (mesh[0][:0], np.full((50, 3), np.nan, F)):
        v = len(pos)
        device = ThermalMesh(_device(pos), *[_device(a[:v]) for a in mesh[1:4]], _device(mesh[4]), (14.0, 33.0))
        out, info = simplify_mesh(device, 0.5)
        assert len(out) == 0 and tuple(out.triangles.shape) == (0, 3) and out.triangles.dtype == torch.int32
        assert out.temperature_bounds == (14.0, 33.0) and tuple(out.thermal_colors.shape) == (0, 3)
        assert (info.vertices_before, info.triangles_before, info.vertices_after, info.triangles_after) == (v, 80, 0, 0)
        assert info.degenerate_triangles == 80 and info.duplicate_triangles == 0 and tuple(info.cluster_count.shape) == (0,)


# ---- tn_voxel_downsample shares the grid code: one call against its own yardstick -----------------------------------------------------------

def test_voxel_downsample_is_unchanged_by_the_shared_grid_code():
    rng = np.random.default_rng(59)
    p = R.random_positions(59, 5000, extent=3.0)
    cloud = (p,) + voxel_reference.attributes(len(p), rng)
    origin, dims = voxel_reference.grid_of(p, 0.37)
    want = voxel_reference.voxel_downsample(*cloud, origin, 0.37, dims)
    out, counts = voxel_downsample(ThermalPointCloud(*[_device(a) for a in cloud], temperature_bounds=(14.0, 33.0)), 0.37)
    for name in ("positions", "colors", "temperature", "thermal_colors", "source"):
        assert getattr(out, name).cpu().numpy().tobytes() == want[name].tobytes(), name
    assert counts.cpu().numpy().tobytes() == want["voxel_count"].tobytes()


# ---- the exporter ---------------------------------------------------------------------------------------------------------------------------

def _same(a, b, keys=("positions", "colors", "temperature", "thermal_colors", "triangles")):
    for key in keys:
        assert getattr(a, key).cpu().numpy().tobytes() == getattr(b, key).cpu().numpy().tobytes(), key


def test_exporter_simplifies_between_the_components_and_the_smoothing_and_is_unchanged_by_default():
    from thermo_nerf_amd import synthetic

    cpu_model, _, _ = helpers.build("scene", 48)
    model = copy.deepcopy(cpu_model).to(DEV).eval()
    cameras = synthetic.orbit_cameras(32, 32, [0, 1, 2, 3], num_views=4, elevation_deg=[0.0, 25.0, 0.0, 25.0])
    kw = dict(max_temperature=33.0, min_temperature=14.0, resolution=32)
    exporter = MeshExporter(model, **kw)
    plain = exporter.export(cameras)
    if plain.triangles.shape[0] == 0:  # no surface inside the scene box for these weights: the box of the cloud of the same cameras
        cloud = PointCloudExporter(model, max_temperature=33.0, min_temperature=14.0, bounding_box=None).export(cameras)
        box = [cloud.positions.min(dim=0).values.cpu().double().tolist(), cloud.positions.max(dim=0).values.cpu().double().tolist()]
        exporter = MeshExporter(model, bounding_box=box, **kw)
        plain = exporter.export(cameras)
    v, t = len(plain), int(plain.triangles.shape[0])
    assert v > 0 and t > 0 and exporter.last_simplify is None
    _same(plain, exporter.extract(exporter.fuse(cameras)))  # the default: today's extraction, bit for bit
    p = plain.positions.cpu().numpy()
    size = 2.5 * float((p.max(axis=0) - p.min(axis=0)).max()) / 31.0  # two and a half grid steps
    # simplification alone: the yardstick on the extracted mesh
    got = exporter.export(cameras, simplify_cell_size=size)
    info = exporter.last_simplify
    origin, dims = voxel_grid(p.min(axis=0).tolist(), p.max(axis=0).tolist(), size)
    want = R.simplify(p, plain.colors.cpu().numpy(), plain.temperature.cpu().numpy(), plain.thermal_colors.cpu().numpy(),
                      plain.triangles.cpu().numpy(), origin, size, dims)
    for key in ("positions", "colors", "temperature", "thermal_colors", "triangles"):
        assert getattr(got, key).cpu().numpy().tobytes() == want[key].tobytes(), key
    assert (info.vertices_before, info.triangles_before, info.vertices_after, info.triangles_after) == (v, t, len(got), len(want["triangles"]))
    assert 0 < len(got) < v and got.normals is None and got.temperature_bounds == plain.temperature_bounds
    # the chain: components, simplification, smoothing, normals — equal to the steps by hand in that order
    _, found = remove_small_components(plain, largest_only=True)
    n = max(2, found.largest_triangles // 2)
    got = exporter.export(cameras, min_component_triangles=n, simplify_cell_size=size, smooth_iterations=2, normals=True)
    kept, components = remove_small_components(plain, min_triangles=n)
    simple, by_hand = simplify_mesh(kept, size)
    hand = smooth_mesh(simple, 2, normals=True)
    assert exporter.last_components == components and 0 < len(simple) < len(kept)
    _same(got, hand, keys=("positions", "normals", "colors", "temperature", "thermal_colors", "triangles"))
    _same(got, simple, keys=("colors", "temperature", "thermal_colors", "triangles"))  # the smoothing moves only positions
    last = exporter.last_simplify
    assert torch.equal(last.cluster_count, by_hand.cluster_count)
    assert [getattr(last, f) for f in ("vertices_before", "triangles_before", "vertices_after", "triangles_after",
                                      "degenerate_triangles", "duplicate_triangles")] == \
        [getattr(by_hand, f) for f in ("vertices_before", "triangles_before", "vertices_after", "triangles_after",
                                       "degenerate_triangles", "duplicate_triangles")]
    assert last.vertices_before == len(kept), "the components went first"
    exporter.export(cameras)
    assert exporter.last_simplify is None
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            exporter.export(cameras, simplify_cell_size=bad)


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def test_command_line_writes_the_simplified_mesh(tmp_path, capsys):
    from tests.test_gpu_mesh_components import _write_tree
    from tests.test_gpu_mesh_smooth import _tool

    data = tmp_path / "data"
    _write_tree(data)
    small = tmp_path / "small.json"
    small.write_text(json.dumps(helpers.SMALL))
    models = tmp_path / "models"
    assert _tool("train_eval").main(["--data", str(data), "--experiment-name", "mesh", "--model-output-folder", str(models),
                                     "--metrics-output-folder", str(tmp_path / "metrics"), "--max-num-iterations", "30",
                                     "--config-json", str(small), "--temperature-bounds", "33", "14", "--device", DEV]) == 0
    run_dir = next((models / "mesh" / "thermal-nerf").iterdir())
    tool = _tool("export_mesh")
    common = [str(run_dir), str(data), "--min-accumulation", "0.02", "--resolution", "24", "--device", DEV]
    plain_file, simple_file = tmp_path / "plain.ply", tmp_path / "simple.ply"
    exporter, cameras, adjust = tool.build_exporter(tool.parse(common + ["--output", str(plain_file)]))
    plain = exporter.export(cameras, apply_camera_optimizer=adjust)
    assert len(plain) > 0 and plain.triangles.shape[0] > 0
    p = plain.positions.cpu().numpy()
    # the mesh of so short a training is a handful of triangles among vertices in none: the coarsest of these cells that leaves some
    for steps in (2.5, 1.5, 1.0, 0.5, 0.25):
        size = float(F(steps * float((p.max(axis=0) - p.min(axis=0)).max()) / 23.0))
        want = exporter.export(cameras, apply_camera_optimizer=adjust, simplify_cell_size=size, normals=True)
        info = exporter.last_simplify
        if len(want):
            break
    assert 0 < len(want) < len(plain) and info.triangles_after == want.triangles.shape[0] > 0
    capsys.readouterr()
    assert tool.main(common + ["--output", str(plain_file)]) == 0
    assert "simplified" not in capsys.readouterr().out
    assert tool.main(common + ["--output", str(simple_file), "--simplify-cell-size", repr(size), "--normals"]) == 0
    printed = capsys.readouterr().out
    print(printed)
    assert f"vertices {len(plain)} -> {len(want)}, triangles {int(plain.triangles.shape[0])} -> {int(want.triangles.shape[0])}" in printed
    assert f"(degenerate {info.degenerate_triangles}, duplicate {info.duplicate_triangles})" in printed
    assert f"vertices {len(want)}, triangles {int(want.triangles.shape[0])}" in printed
    got, old = read_mesh_ply(simple_file), read_mesh_ply(plain_file)
    for key in ("positions", "normals", "colors", "temperature", "triangles"):
        assert got[key].tobytes() == getattr(want, key).cpu().numpy().tobytes(), key
    assert old["positions"].tobytes() == p.tobytes() and 0 < len(got["positions"]) < len(old["positions"])
    assert got["triangles"].max() < len(got["positions"]) and "normals" not in old
