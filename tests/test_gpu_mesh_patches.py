"""tn_mesh_patches on the device against tests/mesh_patches_reference.py, exactly — every integer and every float bit pattern, no
tolerance anywhere — into guarded buffers: the literal meshes, faces that are not geometric, NaN temperatures, the threshold to the
bit, foreign twin tables, patches of 1 .. 65 537+ faces and more faces than one pass of the scan, a thousand single faces, the
union-find's worst chain, the tube's chaining, the capacities, the error codes, determinism, the Python layer and the command line."""
from __future__ import annotations

import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_patches_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (PATCH_BYTES, PATCH_DTYPE, MeshPatches, ThermalMesh, edge_components, mesh_components, mesh_half_edges,
                                    mesh_patches_into, mesh_patches_workspace_bytes, mesh_sections, mesh_thermogram, patch_view,
                                    planar_patches, read_mesh_ply, regions_mesh, write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F, D = np.float32, np.float64
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILLS = {torch.int32: -5, torch.float64: -777.0, torch.uint8: 0xEE, torch.int64: -9}
NAMES = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "twin", "min_cos", "patches", "capacity_patches",
         "face_patch", "counts", "totals", "workspace", "workspace_bytes", "stream")
COS10, COS3 = math.cos(math.radians(10.0)), math.cos(math.radians(3.0))


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _temperature(pos, seed=0):
    p = np.nan_to_num(np.asarray(pos, D), nan=0.0, posinf=0.0, neginf=0.0)
    return (21.0 + 4.0 * np.sin(p[:, 0] / 3.0) + 2.0 * np.cos(p[:, 1] / 5.0) + np.random.default_rng(seed + 99).uniform(-1, 1, len(p))).astype(F)


def raw(mesh, twin, min_cos, cap=None):
    """tn_mesh_patches into guarded buffers.  ``cap`` None: the sizing call with NULL patches first, then room for exactly Q rows."""
    lib = _hip.load()
    pos, temp, tri = (np.ascontiguousarray(a, dtype=k) for a, k in zip(mesh, (F, F, np.int32)))
    twin = np.ascontiguousarray(twin, dtype=np.int32)
    v, t = len(pos), len(tri)
    inputs = [_device(a) if a.size else None for a in (pos, temp, tri, twin)]
    need = mesh_patches_workspace_bytes(v, t) if v and t else 0
    ws = _buffer(need, torch.uint8)
    face_patch, counts, totals = _buffer(t, torch.int32), _buffer(3, torch.int64), _buffer(2, torch.float64)
    ptr = [None if a is None else a.data_ptr() for a in inputs]

    def call(rows, capacity):
        code = lib.tn_mesh_patches(ptr[0], ptr[1], ptr[2], v, t, ptr[3], float(min_cos), None if rows is None else rows.data_ptr(), capacity,
                                   face_patch.data_ptr() if t else None, counts.data_ptr(), totals.data_ptr(),
                                   ws.data_ptr() if need else None, need, _hip.current_stream())
        torch.cuda.synchronize()
        assert code == 0, code

    if cap is None:
        call(None, 0)
        cap = int(counts[0])
        sized = (counts[:3].cpu().numpy().copy(), totals[:2].cpu().numpy().copy(), face_patch[:t].cpu().numpy().copy())
    else:
        sized = None
    rows = _buffer(cap * PATCH_BYTES, torch.uint8)
    call(rows, cap)
    got_counts = counts[:3].cpu().numpy()
    written = min(int(got_counts[0]), cap)
    _untouched(rows, written * PATCH_BYTES, "patches")
    for name, buf, n in (("face_patch", face_patch, t), ("counts", counts, 3), ("totals", totals, 2), ("workspace", ws, need)):
        _untouched(buf, n, name)
    for given, now, what in zip((pos, temp, tri, twin), inputs, ("positions", "temperature", "triangles", "twin")):
        assert now is None or given.tobytes() == now.cpu().numpy().tobytes(), f"{what} was written"
    got = {"patches": np.frombuffer(rows[:written * PATCH_BYTES].cpu().numpy().tobytes(), dtype=PATCH_DTYPE), "counts": got_counts,
           "totals": totals[:2].cpu().numpy(), "face_patch": face_patch[:t].cpu().numpy(), "buffers": (rows, face_patch, counts, totals)}
    if sized is not None:  # the sizing call says the same, rows aside
        assert sized[0].tobytes() == got["counts"].tobytes() and sized[1].tobytes() == got["totals"].tobytes()
        assert sized[2].tobytes() == got["face_patch"].tobytes()
    return got


def compare(got, want, rows=None):
    assert got["counts"].tolist() == want["counts"].tolist()
    assert got["face_patch"].tobytes() == want["face_patch"].astype(np.int32).tobytes()
    assert R.bits(got["totals"]).tolist() == R.bits(want["totals"]).tolist()
    table = want["patches"] if rows is None else want["patches"][:rows]
    assert len(got["patches"]) == len(table)
    for name in PATCH_DTYPE.names:
        g, w = np.ascontiguousarray(got["patches"][name]), np.ascontiguousarray(table[name])
        if g.tobytes() != w.tobytes():
            q = int(np.flatnonzero((R.bits(g).reshape(len(g), -1) != R.bits(w).reshape(len(w), -1)).any(axis=1))[0])
            raise AssertionError(f"{name} of patch {q}: {g[q]!r} != {w[q]!r}")


def check(mesh, min_cos, twin=None, **kw):
    pos, temp, tri = mesh
    if twin is None:
        twin = R.half_edges(tri, len(pos))["twin"]
    want = R.patches(pos, temp, tri, twin, min_cos)
    got = raw(mesh, twin, min_cos, **kw)
    compare(got, want)
    return want, got


def _with_temperature(pos, tri, seed=0):
    return np.asarray(pos, F), _temperature(pos, seed), np.asarray(tri, np.int32)


# ---- the literal meshes -------------------------------------------------------------------------------------------------------------------

def test_literal_meshes():
    cube = _with_temperature(*R.cube())
    want, _ = check(cube, COS10)
    assert want["counts"].tolist() == [6, 12, 12] and want["patches"]["area"].tolist() == [1.0] * 6
    want, _ = check(cube, -1.0)
    assert want["counts"].tolist() == [1, 12, 36] and want["patches"]["flatness"].tolist() == [0.0]
    one = (np.array([(0, 0, 2), (1, 0, 2), (0, 1, 2)], F), np.array([18, 21, 24], F), np.array([(0, 1, 2)], np.int32))
    assert check(one, COS10)[0]["counts"].tolist() == [1, 1, 0]
    assert check(_with_temperature(*R.rectangle((0, 0, 0), (4, 0, 3), (0, 1, 0))), COS10)[0]["counts"].tolist() == [1, 2, 2]
    # the fan's edge has three faces: no twins, nothing joins, whatever the angle
    assert check(_with_temperature(*R.fan()), -1.0)[0]["counts"].tolist() == [3, 3, 0]
    # two coplanar faces that run the SAME way along their shared edge have no twin and stay two patches
    pos, tri = R.rectangle((0, 0, 0), (1, 0, 0), (0, 1, 0))
    same_way = tri.copy()
    same_way[1] = same_way[1][::-1]
    assert check(_with_temperature(pos, same_way), -1.0)[0]["counts"].tolist() == [2, 2, 0]
    # the ridge: two patches at 10 degrees, one of flatness 0.8 at 180
    ridge = R.weld(*R.join_meshes(R.rectangle((0, 0, 0), (4, 0, 3), (0, 1, 0)), R.rectangle((4, 0, 3), (4, 0, -3), (0, 1, 0))))
    assert check(_with_temperature(*ridge), COS10)[0]["counts"].tolist() == [2, 4, 4]
    want, _ = check(_with_temperature(*ridge), -1.0)
    assert want["patches"]["flatness"].tolist() == [F(0.8)] and want["patches"]["max_deviation"].tolist() == [1.5]


def test_faces_that_are_not_geometric_leave_their_neighbours_alone():
    pos, tri = R.flat_lattice(9, 9, 4, permute=False)
    pos, temp, tri = _with_temperature(pos, tri, 4)
    tri = tri.copy()
    tri[5, 1] = tri[5, 0]          # a repeated index
    tri[17, 2] = len(pos)          # an index outside [0, V)
    tri[30, 0] = -3                # a negative index
    tri[44] = (0, 9, 18)           # zero area after the next line: three vertices on one line
    pos[[0, 9, 18]] = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    bad_vertex = int(tri[70, 1])
    pos[bad_vertex, 2] = np.nan    # a NaN coordinate: every face around that vertex
    want, got = check((pos, temp, tri), COS10)
    out = want["face_patch"] < 0
    assert out[[5, 17, 30, 44, 70]].all() and out.sum() == len(tri) - want["counts"][1]
    assert ((tri == bad_vertex).any(axis=1) <= out).all() and want["counts"][0] >= 1
    check((pos, temp, tri), -1.0)
    # inf coordinates, and temperatures that are NaN or infinite at a few vertices: in the patch, out of the mean
    pos, temp, tri = _with_temperature(*R.flat_lattice(9, 9, 4, permute=False), 4)
    temp[[3, 40, 41]] = [np.nan, np.inf, -np.inf]
    pos[60, 0] = np.inf
    want, _ = check((pos, temp, tri), COS10)
    row = want["patches"][0]
    assert 0 < row["thermal_faces"] < row["faces"] and 0.0 < row["thermal_area"] < row["area"]
    # no thermal face at all: the NaN pattern
    temp[:] = np.nan
    want, _ = check((pos, temp, tri), COS10)
    assert R.bits(want["patches"]["mean_temperature"]).tolist() == [R.NAN_BITS] * len(want["patches"]) and want["totals"][1] == 0.0


def test_the_threshold_to_the_bit():
    ell = _with_temperature(*R.ell())
    assert check(ell, 0.0)[0]["counts"].tolist() == [1, 4, 6]
    assert check(ell, float(np.nextafter(0.0, 1.0)))[0]["counts"].tolist() == [2, 4, 4]
    roof = _with_temperature(*R.roof())
    _, _, _, _, _, _, u = R.face_quantities(*roof)
    dot = float((u[0, 0] * u[2, 0] + u[0, 1] * u[2, 1]) + u[0, 2] * u[2, 2])  # faces 0, 1 are the left half, 2, 3 the right
    assert check(roof, dot)[0]["counts"].tolist() == [1, 4, 6]
    assert check(roof, float(np.nextafter(dot, 2.0)))[0]["counts"].tolist() == [2, 4, 4]
    # (the two triangles of a half have the same normal up to the rounding of 1 / sqrt(2): at min_cos = 1 their dot product falls short)
    assert check(roof, 1.0)[0]["counts"].tolist() == [4, 4, 0] and check(roof, -1.0)[0]["counts"].tolist() == [1, 4, 6]


def test_foreign_twin_tables():
    pos, temp, tri = _with_temperature(*R.flat_lattice(7, 7, 2, permute=False), 2)
    t = len(tri)
    twin = R.half_edges(tri, len(pos))["twin"].copy()
    inner = np.flatnonzero(twin >= 0)
    twin[inner[:3]] = [3 * t, -7, 2 ** 31 - 1]   # values outside [0, 3T): no edge there
    check((pos, temp, tri), COS10, twin=twin)
    # an asymmetric pair: h points at a face that does not point back — by the definition it still joins
    lone = np.full(3 * t, -1, np.int32)
    lone[3 * 10 + 1] = 3 * 50 + 2
    want, _ = check((pos, temp, tri), COS10, twin=lone)
    assert want["counts"].tolist() == [t - 1, t, 1] and want["face_patch"][50] == want["face_patch"][10] == 10
    # a half-edge that names its own face joins nothing
    own = np.full(3 * t, -1, np.int32)
    own[0] = 2
    assert check((pos, temp, tri), -1.0, twin=own)[0]["counts"].tolist() == [t, t, 0]
    foreign = np.random.default_rng(5).integers(-9, 3 * t + 9, 3 * t).astype(np.int32)
    check((pos, temp, tri), -1.0, twin=foreign)


# ---- SUM2's boundaries --------------------------------------------------------------------------------------------------------------------

def _jittered_strip(faces, seed):
    pos, tri = R.lattice((faces + 1) // 2 + 1, 2, seed, jitter=0.1)
    pos[:, 2] = 0.0
    # (a cell's SECOND triangle shares the edge with the cell before: an odd strip ends with it)
    tri = tri[:faces] if faces % 2 == 0 else np.delete(tri[:faces + 1], faces - 1, axis=0)
    return pos[:int(tri.max()) + 1].copy(), tri.copy()


def test_patches_of_1_255_256_and_257_faces():
    parts = [_jittered_strip(n, n) for n in (1, 255, 256, 257, 513)]
    pos, tri = R.join_meshes(*[(p + F(k) * np.array([0, 10, 0], F), t) for k, (p, t) in enumerate(parts)])
    tri = tri[np.random.default_rng(3).permutation(len(tri))]
    want, _ = check(_with_temperature(pos, tri, 3), COS10)
    assert sorted(want["patches"]["faces"].tolist()) == [1, 255, 256, 257, 513]
    # every temperature -0.0: a sum is +0.0 whether the patch is walked by its row's thread (up to 256 faces) or has partials (257,
    # 513), while the extremes keep the sign
    want, got = check((np.asarray(pos, F), np.full(len(pos), -0.0, F), np.asarray(tri, np.int32)), COS10)
    rows = got["patches"][:5]
    assert sorted(rows["faces"].tolist()) == [1, 255, 256, 257, 513] and (rows["thermal_area"] > 0.0).all()
    assert R.bits(rows["mean_temperature"]).tolist() == [0x00000000] * 5
    assert R.bits(rows["min_temperature"]).tolist() == R.bits(rows["max_temperature"]).tolist() == [0x80000000] * 5


@functools.lru_cache(maxsize=None)
def _large():
    pos, tri = R.flat_lattice(183, 183, 6)
    return _with_temperature(pos, tri, 6)


def test_one_patch_of_more_than_65_536_faces_carries_both_levels_of_the_sum():
    want, _ = check(_large(), COS10)
    assert want["counts"][0] == 1 and want["patches"]["faces"][0] == 2 * 182 * 182 > 65536
    assert want["patches"]["flatness"][0] == 1.0 and want["patches"]["max_deviation"][0] == 0.0


def test_more_faces_than_one_pass_of_the_scan_folded_into_strips():
    pos, tri = R.strips_lattice(371, 371, 8, 37)
    mesh = _with_temperature(pos, tri, 8)
    assert len(tri) > 1024 * 256
    want, _ = check(mesh, math.cos(math.radians(30.0)))
    faces = want["patches"]["faces"]
    assert len(faces) >= 19 and faces.max() > 256 * 64 and faces.sum() == len(tri)


def test_more_than_a_thousand_single_face_patches():
    pos, tri = R.icosphere(4)
    want, _ = check(_with_temperature(pos, tri, 1), 1.0)
    assert want["counts"][0] == len(tri) == 5120 and want["counts"][2] == 0
    want, _ = check(_with_temperature(pos, tri, 1), -1.0)
    assert want["counts"].tolist() == [1, 5120, 3 * 5120] and want["patches"]["flatness"][0] < 1e-6


def test_a_strip_of_4096_faces_in_reverse_order():
    pos, tri = R.flat_strip(4096)
    want, _ = check(_with_temperature(pos, tri, 2), COS10)
    assert want["counts"].tolist() == [1, 4096, 2 * 4095]


def test_the_tube_pins_the_chaining():
    mesh = _with_temperature(*R.tube(64, 8))
    want, _ = check(mesh, COS10)  # neighbouring columns differ by 5.625 degrees: the whole side is ONE patch
    assert want["counts"][0] == 1 and want["patches"]["flatness"][0] < 1e-6 and want["patches"]["rms_deviation"][0] > 0.5
    want, _ = check(mesh, COS3)   # at 3 degrees every column is a strip of its own
    assert want["counts"][0] == 64 and set(want["patches"]["faces"].tolist()) == {14}


# ---- capacities, error codes, degenerate calls, determinism ----------------------------------------------------------------------------------

def test_capacities():
    mesh = _with_temperature(*R.cube())
    twin = R.half_edges(mesh[2], 8)["twin"]
    want = R.patches(*mesh, twin, COS10)
    for cap in (0, 1, 4, 6, 9):
        got = raw(mesh, twin, COS10, cap=cap)
        compare(got, want, rows=min(cap, 6))


def test_error_codes_with_nothing_written():
    lib = _hip.load()
    pos, temp, tri = _with_temperature(*R.cube())
    twin = R.half_edges(tri, 8)["twin"]
    v, t, cap = 8, 12, 12
    inputs = [_device(pos), _device(temp), _device(tri), _device(twin)]
    outs = {"patches": _buffer(cap * PATCH_BYTES, torch.uint8), "face_patch": _buffer(t, torch.int32), "counts": _buffer(3, torch.int64),
            "totals": _buffer(2, torch.float64)}
    need = mesh_patches_workspace_bytes(v, t)
    ws = _buffer(need, torch.uint8)
    good = dict(positions=inputs[0].data_ptr(), temperature=inputs[1].data_ptr(), triangles=inputs[2].data_ptr(), num_vertices=v,
                num_triangles=t, twin=inputs[3].data_ptr(), min_cos=0.5, capacity_patches=cap, workspace=ws.data_ptr(), workspace_bytes=need,
                stream=_hip.current_stream(), **{k: b.data_ptr() for k, b in outs.items()})

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_patches(*[args[k] for k in NAMES])

    for k in ("positions", "temperature", "triangles", "twin", "patches", "face_patch", "counts", "totals", "workspace"):
        assert call(**{k: None}) == -1, k                                                       # TN_ERR_NULL
    limit = (2 ** 31 - 1) // 3
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2  # TN_ERR_SHAPE
    assert call(num_triangles=limit + 1) == -2 and call(capacity_patches=-1) == -2
    for k in ("positions", "temperature", "triangles", "twin", "face_patch"):
        assert call(**{k: good[k] + 2}) == -2, k
    for k in ("patches", "counts", "totals", "workspace"):
        assert call(**{k: good[k] + 4}) == -2, k
    for bad in (math.nan, 1.0000000000000002, -1.0000000000000002, math.inf, -math.inf):        # TN_ERR_UNSUPPORTED
        assert call(min_cos=bad) == -3, bad
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4              # TN_ERR_WORKSPACE
    # the siblings' order: counts / totals, the shape, min_cos, the other pointers, the alignment, the workspace
    assert call(counts=None, num_vertices=-1) == -1 and call(num_vertices=-1, min_cos=math.nan) == -2
    assert call(min_cos=math.nan, positions=None) == -3 and call(positions=None, twin=good["twin"] + 2) == -1
    assert call(twin=good["twin"] + 2, workspace_bytes=0) == -2
    assert lib.tn_mesh_patches_workspace_bytes(-1, 0) == 0 and lib.tn_mesh_patches_workspace_bytes(0, limit + 1) == 0
    torch.cuda.synchronize()
    for name, buf in (("workspace", ws), *outs.items()):
        _untouched(buf, 0, name)
    assert call(min_cos=1.0) == 0 and call(min_cos=-1.0) == 0
    torch.cuda.synchronize()
    assert outs["counts"][:3].tolist() == [1, 12, 36]


def test_no_vertices_and_no_triangles():
    mesh = _with_temperature(*R.cube())
    twin = R.half_edges(mesh[2], 8)["twin"]
    for v, t in ((0, 0), (0, 12), (8, 0)):
        part = (mesh[0][:v], mesh[1][:v], mesh[2][:t])
        got = raw(part, twin[:3 * t], COS10, cap=4)
        assert got["counts"].tolist() == [0, 0, 0] and got["totals"].tolist() == [0.0, 0.0] and got["face_patch"].tolist() == [-1] * t
        compare(got, R.patches(*part, twin[:3 * t], COS10))
    # vertices and faces, but no geometric face: no patch, and the rows stay untouched
    nowhere = (np.full((8, 3), np.nan, F), mesh[1], mesh[2])
    got = raw(nowhere, twin, -1.0, cap=4)
    assert got["counts"].tolist() == [0, 0, 0] and got["totals"].tolist() == [0.0, 0.0] and got["face_patch"].tolist() == [-1] * 12
    compare(got, R.patches(*nowhere, twin, -1.0))


def test_the_same_call_twice_gives_identical_bytes():
    mesh = _large()
    twin = R.half_edges(mesh[2], len(mesh[0]))["twin"]
    first, second = raw(mesh, twin, COS10, cap=3), raw(mesh, twin, COS10, cap=3)
    for a, b in zip(first["buffers"], second["buffers"]):
        assert torch.equal(a, b)
    # the device's own table gives the same patches
    mine = mesh_half_edges(_device(mesh[2]), len(mesh[0])).twin.cpu().numpy()
    assert mine.tobytes() == twin.tobytes()


# ---- the Python layer and the command line ---------------------------------------------------------------------------------------------------

def _mesh(pos, temp, tri, bounds=(10.0, 35.0)):
    colors = np.random.default_rng(23).integers(0, 256, (len(pos), 3)).astype(np.uint8)
    return ThermalMesh(_device(np.asarray(pos, F)), _device(colors), _device(temp), None, _device(np.ascontiguousarray(tri, dtype=np.int32)), bounds)


def _box():
    pos, tri = R.cube()
    return (pos * np.array([1, 2, 3], F)).astype(F), tri


def test_planar_patches_order_min_area_top_and_refusals():
    pos, tri = _box()
    temp = _temperature(pos)
    mesh = _mesh(pos, temp, tri)
    want = R.patches(pos, temp, tri, R.half_edges(tri, 8)["twin"], COS10)
    found = planar_patches(mesh)
    assert isinstance(found, MeshPatches) and found.patches.dtype == PATCH_DTYPE and len(found) == 6
    # -x +x (2 x 3 = 6), -y +y (1 x 3 = 3), -z +z (1 x 2 = 2): largest first, ties by ascending label
    assert found.patch_index.tolist() == [0, 1, 2, 3, 4, 5] and found.patches["area"].tolist() == [6.0, 6.0, 3.0, 3.0, 2.0, 2.0]
    assert found.patches.tobytes() == want["patches"].tobytes() and found.face_patch.cpu().numpy().tobytes() == want["face_patch"].tobytes()
    assert (found.num_patches, found.geometric_faces, found.joined_half_edges) == tuple(want["counts"].tolist())
    assert (found.mesh_area, found.thermal_area) == (22.0, 22.0) and found.min_cos == COS10
    assert found.num_regions == 6 and found.region_index is found.patch_index and found.face_region is found.face_patch
    edges = mesh_half_edges(mesh.triangles, 8)
    assert planar_patches(mesh, 10.0, half_edges=edges, min_area=2.5).patches["area"].tolist() == [6.0, 6.0, 3.0, 3.0]
    top = planar_patches(mesh, 10.0, half_edges=edges, top=3)
    assert top.patch_index.tolist() == [0, 1, 2] and top.num_patches == 6
    assert len(planar_patches(mesh, 90.5)) == 1 and len(planar_patches(mesh, 180.0)) == 1 and len(planar_patches(mesh, 0.0)) == 6
    for bad in (dict(min_area=-1.0), dict(min_area=math.nan), dict(top=-1)):
        with pytest.raises(ValueError):
            planar_patches(mesh, 10.0, **bad)
    counts, totals = torch.empty(3, dtype=torch.int64, device=DEV), torch.empty(2, dtype=torch.float64, device=DEV)
    face_patch = torch.empty(12, dtype=torch.int32, device=DEV)
    ok = dict(counts=counts, totals=totals, face_patch=face_patch)
    mesh_patches_into(mesh, edges.twin, COS10, **ok)  # the sizing call
    assert counts.tolist() == [6, 12, 12]
    for twin in (edges.twin[:-1], edges.twin.long(), edges.twin.cpu(), None):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            mesh_patches_into(mesh, twin, COS10, **ok)
    for bad in (dict(ok, counts=counts.int()), dict(ok, totals=totals.float()), dict(ok, face_patch=face_patch[:5]), dict(ok, face_patch=None),
                dict(ok, patches=torch.empty(PATCH_BYTES, dtype=torch.int32, device=DEV)), dict(ok, capacity_patches=2),
                dict(ok, patches=torch.empty(PATCH_BYTES, dtype=torch.uint8, device=DEV), capacity_patches=2),
                dict(ok, workspace=torch.empty(8, dtype=torch.uint8, device=DEV)), dict(ok, capacity_patches=-1)):
        with pytest.raises(ValueError):
            mesh_patches_into(mesh, edges.twin, COS10, **bad)


def test_edge_components_where_they_differ_from_vertex_components():
    pos, tri = R.two_cubes_touching()
    assert len(pos) == 15
    mesh = _mesh(pos, _temperature(pos), tri)
    assert int(mesh_components(mesh.triangles, 15).summary[0]) == 1
    found = edge_components(mesh)
    assert found.num_patches == 2 == len(found) and found.patches["faces"].tolist() == [12, 12] and found.patches["area"].tolist() == [6.0, 6.0]
    assert found.face_patch.cpu().tolist() == [0] * 12 + [1] * 12 and found.min_cos == -1.0


def test_regions_mesh_region_map_patch_view_thermogram_and_sections():
    pos, tri = R.cube()
    temp = _temperature(pos)
    mesh = _mesh(pos, temp, tri)
    found = planar_patches(mesh)
    k = int(np.flatnonzero(found.patches["label"] == 2)[0])  # the side +x, faces 2 and 3
    one = found.only(k)
    side = regions_mesh(mesh, one)
    assert len(side) == 4 and side.triangles.shape[0] == 2 and bool((side.positions[:, 0] == 1.0).all())
    assert regions_mesh(mesh, found).triangles.shape[0] == 12
    size = 1.0 / 32.0
    view = patch_view(mesh, found, k, pixel_size=size)
    assert view.forward == (-1.0, 0.0, 0.0) and view.cull and view.width == view.height == 32 + 4
    whole = mesh_thermogram(mesh, view)  # the whole cube through the side's view: only the side faces the camera
    shown = whole.region_map(found)
    covered = whole.pixel_face >= 0
    assert bool((shown[covered] == int(found.patch_index[k])).all()) and bool((shown[~covered] == -1).all())
    alone = mesh_thermogram(side, view)
    assert abs(alone.covered_area - 1.0) <= 2.0 * size + size * size and alone.covered == whole.covered
    top = int(np.flatnonzero(found.patches["label"] == 10)[0])   # +z: up falls back to world y
    assert patch_view(mesh, found, top, width=40).forward == (0.0, 0.0, -1.0)
    with pytest.raises(IndexError):
        patch_view(mesh, found, 6, pixel_size=size)
    with pytest.raises(ValueError, match="no plane"):
        patch_view(mesh, planar_patches(mesh, 180.0), 0, pixel_size=size)
    # a row's plane as it is: the ridge at 180 degrees is one patch whose plane z = 3 / 2 cuts each ramp in a line of length 1
    pos, tri = R.weld(*R.join_meshes(R.rectangle((0, 0, 0), (4, 0, 3), (0, 1, 0)), R.rectangle((4, 0, 3), (4, 0, -3), (0, 1, 0))))
    ridge = _mesh(pos, _temperature(pos), tri)
    plane = edge_components(ridge).patches["plane"][0]
    cut = mesh_sections(ridge, plane[:3], [plane[3]])
    assert plane.tolist() == [0.0, 0.0, 1.0, 1.5] and cut.num_curves == 2 and cut.curves["length"].tolist() == [1.0, 1.0]


def test_command_line_end_to_end_on_a_written_ply(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("mesh_patches_tool", os.path.join(ROOT, "tools", "mesh_patches.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for bad in (["m.ply"], ["m.ply", "--report", "r.json", "--max-angle", "181"], ["m.ply", "--report", "r.json", "--thermograms", "d"],
                ["m.ply", "--report", "r.json", "--min-area", "-1"], ["m.ply", "--report", "r.json", "--length-scale", "0"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    pos, tri = _box()
    temp = _temperature(pos)
    source = tmp_path / "box.ply"
    write_mesh_ply(source, _mesh(pos, temp, tri))
    report_file, out, pictures = tmp_path / "out" / "patches.json", tmp_path / "out" / "patches.ply", tmp_path / "pictures"
    assert tool.main([str(source), "--max-angle", "10", "--top", "4", "--length-scale", "2", "--report", str(report_file), "--output", str(out),
                      "--thermograms", str(pictures), "--pixel-size", "0.125", "--device", DEV]) == 0
    printed = capsys.readouterr().out
    want = R.patches(pos, temp, tri, R.half_edges(tri, 8)["twin"], COS10)["patches"]
    report = json.loads(report_file.read_text())
    assert report["edges"] == {"edges": 18, "boundary": 0, "nonmanifold": 0, "inconsistent": 0, "closed_manifold": True, "joined_half_edges": 12}
    assert report["counts"] == {"vertices": 8, "faces": 12, "geometric_faces": 12, "patches": 6, "reported_patches": 4}
    assert report["mesh_area"] == 88.0 and report["reported_area"] == 72.0 and report["reported_share"] == 72.0 / 88.0
    assert report["max_angle_degrees"] == 10.0 and report["length_scale"] == 2.0
    for row, w in zip(report["patches"], want[:4]):
        assert (row["patch"], row["label"], row["faces"], row["area"]) == (int(w["label"]) // 2, int(w["label"]), 2, 4.0 * float(w["area"]))
        assert row["plane"] == {"normal": w["plane"][:3].tolist(), "offset": 2.0 * float(w["plane"][3])} and row["flatness"] == 1.0
        assert (row["rms_deviation"], row["max_deviation"]) == (0.0, 0.0) and row["centroid"] == (2.0 * w["centroid"]).tolist()
        assert (row["mean_temperature"], row["min_temperature"], row["max_temperature"]) == \
            (float(w["mean_temperature"]), float(w["min_temperature"]), float(w["max_temperature"]))
        assert row["bounds"] == {"min": (2.0 * w["bounds"][:3].astype(D)).tolist(), "max": (2.0 * w["bounds"][3:].astype(D)).tolist()}
    assert printed.count("\npatch ") == 4 and "6 patches" in printed
    written = read_mesh_ply(out)
    assert len(written["triangles"]) == 8 and len(written["positions"]) == 8
    from PIL import Image

    assert sorted(p.name for p in pictures.iterdir()) == [f"patch_{k}.png" for k in range(4)]
    assert Image.open(pictures / "patch_0.png").size == (2 * 8 + 4, 3 * 8 + 4)  # the side -x: 2 along y, 3 along z (up), two pixels around
