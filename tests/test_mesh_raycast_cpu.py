"""The yardstick of the ray caster (tests/mesh_raycast_reference.py) checked on its own — literal cases with hand-computed answers,
that the box clause rejects nothing on the scenes the device tests use, the monotonicity the traversal rests on, the reference tree —
and the host side of the feature: the declarations, the struct, the refusals of the two entries, the Python layer's refusals, the
command line and its report.  No GPU."""
from __future__ import annotations

import ctypes
import dataclasses
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_raycast_reference as R
from tests import test_gpu_mesh_arguments as mesh_arguments
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (CameraThermogram, CameraView, MeshBVH, ThermalMesh, build_mesh_bvh, camera_rays, mesh_bvh_bytes,
                                    mesh_bvh_depth_bound, mesh_bvh_workspace_bytes, mesh_camera_thermogram, mesh_raycast,
                                    mesh_raycast_into, visible_from)
from thermo_nerf_amd.export import raycast as raycast_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_camera_view_tool", os.path.join(ROOT, "tools", "mesh_camera_view.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the reference on literal cases -----------------------------------------------------------------------------------------------------

TRIANGLE = (np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F), np.array([10, 20, 30], F), np.array([(0, 0, 0), (200, 100, 0), (0, 100, 255)], np.uint8),
            np.array([(0, 1, 2)], np.int32))


def test_one_triangle_by_hand():
    o = np.array([(1, 1, 2), (1, 1, -3), (1, 2, 2), (3, 3, 2), (0, 0, 5), (2, 2, 1), (1, 1, 2), (1, 1, 2)], F)
    d = np.array([(0, 0, -1), (0, 0, 2), (0, 0, -4), (0, 0, -1), (0, 0, -1), (0, 0, -1), (0, 0, 1), (1, 0, 0)], F)
    got = R.raycast(*TRIANGLE, o, d)
    assert got["hit_face"].tolist() == [0, 0, 0, -1, 0, 0, -1, -1], "inside, from below, unnormalised, outside, a vertex, the hypotenuse, away, parallel"
    assert got["hit_t"][[0, 1, 2, 4, 5]].tolist() == [2.0, 1.5, 0.5, 5.0, 1.0]
    assert got["hit_uv"][:3].tolist() == [[0.25, 0.25], [0.25, 0.25], [0.25, 0.5]] and got["hit_uv"][4].tolist() == [0.0, 0.0]
    # (1, 1): 0.5 * 10 + 0.25 * 20 + 0.25 * 30; (1, 2): 0.25 * 10 + 0.25 * 20 + 0.5 * 30; the vertex: 10; (2, 2): 0.5 * 20 + 0.5 * 30
    assert got["hit_temperature"][[0, 1, 2, 4, 5]].tolist() == [17.5, 17.5, 22.5, 10.0, 25.0]
    assert got["hit_colors"][0].tolist() == [50, 50, 64], "0.25 * 200; 0.25 * 100 + 0.25 * 100; 0.25 * 255 = 63.75 rounds to 64"
    assert got["hit_colors"][3].tolist() == [0, 0, 0] and got["hit_any"].tolist() == [1, 1, 1, 0, 1, 1, 0, 0]
    assert R.bits(got["hit_t"][[3, 6, 7]]).tolist() == [R.NAN_BITS] * 3 and R.bits(got["hit_uv"][3]).tolist() == [R.NAN_BITS] * 2
    assert R.bits(got["hit_temperature"][[3, 6, 7]]).tolist() == [R.NAN_BITS] * 3
    assert got["counts"].tolist() == [5, 8, 1, 0] and got["stats"].tolist() == [17.5 + 17.5 + 22.5 + 10.0 + 25.0, 10.0, 25.0]
    assert got["hit_face"].dtype == np.int32 and got["hit_t"].dtype == F and got["counts"].dtype == np.int64 and got["stats"].dtype == D


def test_cull_follows_the_rasteriser_winding():
    """the normal (p1 - p0) x (p2 - p0) of TRIANGLE is +z: a ray going down meets its front (det > 0), a ray going up sees it from
    behind (det < 0), which is what tn_mesh_rasterize calls area2 > 0 for a view with forward = +z"""
    o, d = np.array([(1, 1, 2), (1, 1, -2)], F), np.array([(0, 0, -1), (0, 0, 1)], F)
    assert R.raycast(*TRIANGLE, o, d)["hit_face"].tolist() == [0, 0]
    assert R.raycast(*TRIANGLE, o, d, cull=1)["hit_face"].tolist() == [0, -1]
    flipped = TRIANGLE[:3] + (np.array([(0, 2, 1)], np.int32),)
    assert R.raycast(*flipped, o, d, cull=1)["hit_face"].tolist() == [-1, 0]
    from tests import mesh_raster_reference as Q

    view = Q.view(8, 8)  # forward = +z
    shifted = (TRIANGLE[0] + np.array([1, 1, 3], F),) + TRIANGLE[1:]
    assert Q.rasterize(*shifted, dict(view, cull=1))["counts"][1] == 0, "seen from behind by a view along +z: like the ray going up"


def test_windows_ties_and_unusable_things():
    pos = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 1), (4, 0, 1), (0, 4, 1)], F)
    temp = np.array([10, 20, 30, 40, 50, 60], F)
    tri = np.array([(3, 4, 5), (0, 1, 2), (0, 1, 2), (0, 0, 1), (0, 1, 9)], np.int32)  # the upper sheet, the lower one twice, two unusable
    o, d = np.array([(1, 1, 3)], F), np.array([(0, 0, -1)], F)
    assert R.usable_faces(pos, temp, tri).tolist() == [True, True, True, False, False]
    assert R.raycast(pos, temp, None, tri, o, d)["hit_face"].tolist() == [0] and R.raycast(pos, temp, None, tri, o, d)["hit_colors"] is None
    assert R.raycast(pos, temp, None, tri, o, d, t_min=2.5)["hit_face"].tolist() == [1], "equal t: the lowest index"
    assert R.raycast(pos, temp, None, tri, o, d, t_min=2.0, t_max=2.0)["hit_face"].tolist() == [0], "the window is closed on both sides"
    assert R.raycast(pos, temp, None, tri, o, d, t_max=1.5)["hit_face"].tolist() == [-1]
    assert R.raycast(pos, temp, None, tri, o, d, t_min=3.0, t_max=2.0)["hit_face"].tolist() == [-1]
    for end, want in ((1.5, -1), (2.0, 0), (np.nan, 0), (np.inf, 0), (-1.0, -1)):
        assert R.raycast(pos, temp, None, tri, o, d, ray_t_max=np.array([end], F))["hit_face"].tolist() == [want], end
    assert R.raycast(pos, temp, None, tri, o, d, ray_t_max=np.array([5.0], F), t_max=1.5)["hit_face"].tolist() == [-1], "the smaller end holds"
    hot = temp.copy()
    hot[4] = np.inf
    assert R.raycast(pos, hot, None, tri, o, d)["hit_face"].tolist() == [1], "a non-finite temperature spoils its faces"
    bad_o = np.array([(1, 1, 3), (np.nan, 1, 3), (1, 1, np.inf), (1, 1, 3), (1, 1, 3)], F)
    bad_d = np.array([(0, 0, 0), (0, 0, -1), (0, 0, -1), (0, np.nan, -1), (0, 0, -1)], F)
    got = R.raycast(pos, temp, None, tri, bad_o, bad_d)
    assert got["hit_face"].tolist() == [-1, -1, -1, -1, 0] and got["counts"].tolist() == [1, 1, 3, 0]
    empty = R.raycast(pos[:0], temp[:0], None, tri, o, d)
    assert empty["counts"].tolist() == [0, 1, 0, 0] and empty["stats"].tolist() == [0.0, math.inf, -math.inf]
    none = R.raycast(pos, temp, None, tri, o[:0], d[:0])
    assert none["counts"].tolist() == [0, 0, 3, 0] and none["hit_face"].shape == (0,) and none["hit_uv"].shape == (0, 2)


def test_sum2_and_the_orders():
    values = np.array([-math.inf, -1.0, -0.0, 0.0, 1e-40, 1.0, math.inf], F)
    assert (np.diff(R.ord32(values).astype(np.int64)) > 0).all()
    assert R.bits(R.min_ord(F(0.0), F(-0.0))).tolist() == [0x80000000] and R.bits(R.max_ord(F(-0.0), F(0.0))).tolist() == [0]
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, 257).tolist()
    assert R.sum2([]) == 0.0 and R.sum2(x[:256]) == sum(x[:256], 0.0) and R.sum2(x) == sum(x[:256], 0.0) + x[256]


# ---- the box clause hides nothing; the slack does real work ------------------------------------------------------------------------------

def test_box_clause_rejects_nothing_on_the_cube_lattice_and_the_slack_is_needed(monkeypatch):
    pos, tri = R.cube_lattice(4)
    temp, col = R.attributes(len(pos), 6)
    o, d = R.lattice_rays(4)
    got = R.raycast(pos, temp, col, tri, o, d)
    assert len(o) > 2000 and got["rejected"] == 0 and got["counts"][0] == len(o), "every ray aims at the cube's surface"
    monkeypatch.setattr(R, "SLACK", 1.0)
    bare = R.raycast(pos, temp, col, tri, o, d)
    print(f"{len(o)} rays at {len(tri)} faces: without the 2^-32 slack the box clause rejects {bare['rejected']} Moeller-Trumbore passes")
    assert bare["rejected"] > 0, "the scene cannot tell the slack from none: choose other rays"


def test_box_clause_rejects_nothing_on_a_soup():
    pos, tri = R.soup(300, 12)
    temp, col = R.attributes(len(pos), 7)
    o, d = R.soup_rays(1500, 13)
    for kw in (dict(), dict(cull=1, t_min=0.125), dict(t_max=1.0)):
        got = R.raycast(pos, temp, col, tri, o, d, **kw)
        assert got["rejected"] == 0 and 0.2 < got["counts"][0] / len(o) <= 1.0, kw


def test_slab_bounds_are_monotone_under_box_inclusion():
    """what the traversal rests on: the parent's enter is at most the child's, its exit at least the child's, and a parent of a box
    that passes passes — on random nested boxes, flat ones, rays with zero components and origins on box planes"""
    rng = np.random.default_rng(3)
    n = 20000
    lo = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    hi = (lo + rng.uniform(0.0, 1.0, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.2)).astype(F)  # one side in five is flat
    grow = rng.uniform(0.0, 0.5, (2, n, 3)) * (rng.uniform(0, 1, (2, n, 3)) > 0.3)
    plo, phi = (lo - grow[0]).astype(F), (hi + grow[1]).astype(F)
    assert (plo <= lo).all() and (phi >= hi).all()
    o = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    aim = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))  # most rays aim at the child box
    d = np.where(rng.uniform(0, 1, (n, 1)) < 0.7, aim - o, rng.uniform(-1.0, 1.0, (n, 3))).astype(F)
    d[rng.uniform(0, 1, (n, 3)) < 0.15] = 0.0
    d[d.any(axis=1) == 0] = 1.0
    on = rng.uniform(0, 1, (n, 3)) < 0.1
    o[on] = lo[on]  # an origin on a box plane
    with np.errstate(all="ignore"):
        cols = lambda a: [a[:, k].astype(D) for k in range(3)]
        inv = [1.0 / x for x in cols(d)]
        child = R.slab(np, cols(o), cols(d), inv, cols(lo), cols(hi), 0.0, math.inf)
        parent = R.slab(np, cols(o), cols(d), inv, cols(plo), cols(phi), 0.0, math.inf)
    assert (parent[1] <= child[1]).all() and (parent[2] >= child[2]).all(), "s and exit are monotone"
    assert (parent[0] | ~child[0]).all() and 0.05 < child[0].mean() < 0.95, "a box that passes has a parent that passes"


# ---- the reference tree ------------------------------------------------------------------------------------------------------------------

def test_reference_tree_on_small_cases_by_hand():
    # four faces along x at 0, 1/4, 1/2 and 1 of the extent: the codes' x bits are 0, 256, 512 and 1023
    def face(x):
        return [(x, 0.0, 0.0), (x + 0.001953125, 0.0, 0.0), (x, 0.001953125, 0.0)]

    pos = np.array(face(0.0) + face(0.5) + face(0.25) + face(1.0 - 0.001953125), F)
    tri = np.arange(12, dtype=np.int32).reshape(-1, 3)
    key, usable, lo, hi = R.keys(pos, np.zeros(12, F), tri)
    assert usable.all() and lo.tolist() == [0.0, 0.0, 0.0] and hi.tolist() == [1.0, 0.001953125, 0.0]
    # centre of face 0 along x: 0.0009765625 -> q = 1; along y: (0 + 2^-9) / 2 of an extent of 2^-9 -> q = 512; z: no extent -> 0
    assert key[0] == (int(R.spread3(1)) << 2 | int(R.spread3(512)) << 1) and int(R.spread3(0x3FF)) == 0x09249249
    tree = R.tree(pos, np.zeros(12, F), tri)
    assert tree["faces"].tolist() == [0, 2, 1, 3] and tree["root"] == 0 and tree["num_nodes"] == 3
    # the top x bit splits {0, 1/4} from {1/2, 1}
    assert tree["child"].tolist() == [[1, 2], [~0, ~1], [~2, ~3]] and tree["level"].tolist() == [2, 1, 1] and tree["depth"] == 2
    assert tree["box_lo"][0, 0].tolist() == [0.0, 0.0, 0.0] and tree["box_hi"][0, 0, 0] == F(0.25) + F(0.001953125)
    one = R.tree(pos[:3], np.zeros(3, F), tri[:1])
    assert (one["root"], one["depth"], one["num_nodes"], one["faces"].tolist()) == (-1, 0, 0, [0])
    none = R.tree(pos[:3], np.full(3, np.nan, F), tri[:1])
    assert (none["root"], none["num_usable"], none["lo"].tolist(), none["hi"].tolist()) == (R.NONE, 0, [math.inf] * 3, [-math.inf] * 3)
    same = R.tree(pos[:3], np.zeros(3, F), np.tile(tri[:1], (5, 1)))
    assert same["faces"].tolist() == [0, 1, 2, 3, 4] and same["depth"] == 3, "equal codes: the position in the leaf order splits 0 - 3 | 4"
    assert same["child"].tolist() == [[3, ~4], [~0, ~1], [~2, ~3], [1, 2]]


def test_reference_tree_invariants_and_depth_bound():
    pos, tri = R.soup(257, 4)
    tri = tri.copy()
    tri[5, 1] = tri[5, 0]
    tree = R.tree(pos, np.zeros(len(pos), F), tri)
    n = tree["num_nodes"]
    assert tree["num_usable"] == 256 and n == 255 and tree["faces"][-1] == 5 and tree["depth"] <= R.DEPTH_BOUND == 61
    child = tree["child"]
    assert np.sort(~child[child < 0]).tolist() == list(range(256)) and np.sort(child[child >= 0]).tolist() == list(range(1, n))
    key = R.keys(pos, np.zeros(len(pos), F), tri)[0]
    assert (np.diff(key[tree["faces"]].astype(np.int64)) >= 0).all() and key[5] == 1 << 30 and key[tree["faces"][:256]].max() < 1 << 30


# ---- the declarations --------------------------------------------------------------------------------------------------------------------

BUILD_NAMES = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "bvh", "bvh_bytes", "workspace", "workspace_bytes",
               "stream")
CAST_NAMES = ("positions", "temperature", "colors", "triangles", "num_vertices", "num_triangles", "bvh", "bvh_bytes", "origins", "directions",
              "ray_t_max", "num_rays", "params", "hit_face", "hit_t", "hit_uv", "hit_temperature", "hit_colors", "hit_any", "counts", "stats",
              "stream")


def test_entries_struct_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bsize_t tn_mesh_bvh_bytes\(int64_t num_triangles\);", header)
    assert re.search(r"\bsize_t tn_mesh_bvh_workspace_bytes\(int64_t num_triangles\);", header)
    assert re.search(r"\bint32_t tn_mesh_bvh_depth_bound\(void\);", header)
    for entry, names in (("tn_mesh_bvh_build", BUILD_NAMES), ("tn_mesh_raycast", CAST_NAMES)):
        declared = re.search(r"\bint %s\(([^;]*)\);" % entry, header).group(1)
        assert [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")] == list(names), entry
        assert len(_hip.SIGNATURES[entry][1]) == len(names) and _hip.SIGNATURES[entry][0] == ctypes.c_int
    assert _hip.SIGNATURES["tn_mesh_raycast"][1][12] == ctypes.POINTER(_hip.tn_raycast_params)
    assert _hip.SIGNATURES["tn_mesh_bvh_bytes"] == (ctypes.c_size_t, [ctypes.c_int64]) == _hip.SIGNATURES["tn_mesh_bvh_workspace_bytes"]
    assert "tn_mesh_bvh.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    offsets = {"t_min": 0, "t_max": 8, "cull": 16, "mode": 20}
    assert ctypes.sizeof(_hip.tn_raycast_params) == 24 and [f[0] for f in _hip.tn_raycast_params._fields_] == list(offsets)
    for name, offset in offsets.items():
        assert getattr(_hip.tn_raycast_params, name).offset == offset, name
    body = re.search(r"typedef struct tn_raycast_params \{([^}]*)\} tn_raycast_params;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == list(offsets)
    assert re.search(r"#define TN_RAYCAST_CLOSEST 0\b", header) and re.search(r"#define TN_RAYCAST_ANY 1\b", header)
    assert (_hip.TN_RAYCAST_CLOSEST, _hip.TN_RAYCAST_ANY) == (R.CLOSEST, R.ANY) == (0, 1)
    assert "30 + 31" in header and "0x56424e54" in header, "the depth bound's proof and the blob's magic are in the header"


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _hip.load()
    assert mesh_bvh_depth_bound() == lib.tn_mesh_bvh_depth_bound() == R.DEPTH_BOUND <= raycast_module.STACK_ENTRIES == 64
    limit = (2 ** 31 - 1) // 3
    assert [mesh_bvh_bytes(t) for t in (0, 1, 2, 16, 17)] == [64, 128, 192, 64 + 64 + 15 * 64, 64 + 128 + 16 * 64]
    assert mesh_bvh_bytes(-1) == mesh_bvh_bytes(limit + 1) == 0 == mesh_bvh_workspace_bytes(-1) == mesh_bvh_workspace_bytes(limit + 1)
    assert mesh_bvh_workspace_bytes(2000) >= 64 + 2 * 8 * 2000 and mesh_bvh_workspace_bytes(2000) % 8 == 0 and mesh_bvh_bytes(limit) > 64 * limit
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy, t = 4096, 2000
    blob, work = mesh_bvh_bytes(t), mesh_bvh_workspace_bytes(t)
    good = dict(zip(BUILD_NAMES, [dummy, dummy, dummy, 1000, t, dummy, blob - 1, dummy, work, None]))

    def build(**change):
        args = dict(good, **change)
        return lib.tn_mesh_bvh_build(*[args[k] for k in BUILD_NAMES])

    assert build() == -4 and build(bvh_bytes=blob, workspace_bytes=work - 1) == -4 and build(bvh_bytes=0) == -4  # TN_ERR_WORKSPACE
    for k in ("positions", "temperature", "triangles", "bvh", "workspace"):
        assert build(**{k: None}) == -1, k  # TN_ERR_NULL
    assert build(num_vertices=-1) == -2 and build(num_vertices=2 ** 31) == -2 and build(num_triangles=-1) == -2 and build(num_triangles=limit + 1) == -2
    for k in ("positions", "temperature", "triangles"):
        assert build(**{k: dummy + 2}) == -2, k
    assert build(bvh=dummy + 32) == -2 and build(workspace=dummy + 4) == -2
    assert build(bvh=None, num_vertices=-1) == -1 and build(num_vertices=-1, triangles=None) == -2 and build(triangles=None, bvh=dummy + 32) == -1, \
        "in the siblings' order"
    assert build(num_vertices=0, positions=None, temperature=None) == -4, "a mesh without vertices needs no vertex arrays"

    def params(t_min=0.0, t_max=math.inf, cull=0, mode=0):
        return _hip.tn_raycast_params(t_min, t_max, cull, mode)

    good = dict(zip(CAST_NAMES, [dummy, dummy, dummy, dummy, 1000, t, dummy, blob - 1, dummy, dummy, dummy, 500, params()] + [dummy] * 8 + [None]))

    def cast(**change):
        args = dict(good, **change)
        return lib.tn_mesh_raycast(*[args[k] for k in CAST_NAMES])

    assert cast() == -4 and cast(bvh_bytes=0) == -4
    for k in ("positions", "temperature", "colors", "triangles", "bvh", "origins", "directions", "params", "hit_temperature"):
        assert cast(**{k: None}) == -1, k
    for k in ("ray_t_max", "hit_face", "hit_t", "hit_uv", "hit_colors", "hit_any", "counts"):
        assert cast(**{k: None}) == -4, f"{k} may be absent"
    assert cast(stats=None, hit_temperature=None) == -4 and cast(colors=None, hit_colors=None) == -4
    assert cast(params=params(mode=1), colors=None, hit_temperature=None) == -4, "any-hit writes hit_any alone: nothing else is required"
    assert cast(num_vertices=-1) == -2 and cast(num_triangles=limit + 1) == -2 and cast(num_rays=-1) == -2 and cast(num_rays=limit + 1) == -2
    for change in (dict(t_min=math.nan), dict(t_max=math.nan), dict(t_min=-1.0), dict(t_min=-math.inf), dict(cull=2), dict(cull=-1), dict(mode=2),
                   dict(mode=-1)):
        assert cast(params=params(**change)) == -3, change  # TN_ERR_UNSUPPORTED
    assert cast(params=params(t_min=5.0, t_max=1.0)) == -4 and cast(params=params(t_min=math.inf)) == -4 and cast(params=params(cull=1, mode=1)) == -4
    for k in ("positions", "temperature", "triangles", "origins", "directions", "ray_t_max", "hit_face", "hit_t", "hit_uv", "hit_temperature"):
        assert cast(**{k: dummy + 2}) == -2, k
    assert cast(counts=dummy + 4) == -2 and cast(stats=dummy + 4) == -2 and cast(bvh=dummy + 32) == -2
    bad = params(cull=2)
    assert cast(params=bad, bvh=None) == -1 and cast(params=bad, num_rays=-1) == -2 and cast(params=bad, origins=None) == -3 and \
        cast(origins=None, hit_t=dummy + 2) == -1, "in the siblings' order"
    assert cast(num_rays=0, origins=None, directions=None, hit_temperature=None) == -4


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------

def test_python_layer_refuses_before_it_reaches_a_kernel():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    bvh = MeshBVH(torch.zeros(128, dtype=torch.uint8), 3, 1, mesh)
    rays = torch.zeros((4, 3))
    with pytest.raises(ValueError, match="no triangles"):
        build_mesh_bvh(ThermalMesh(pos, mesh.colors, mesh.temperature))
    for kw in (dict(t_min=-1.0), dict(t_min=math.nan), dict(t_max=math.nan)):
        with pytest.raises(ValueError, match="t_min"):
            mesh_raycast(bvh, rays, rays, **kw)
        with pytest.raises(ValueError, match="t_min"):
            mesh_raycast_into(bvh, rays, rays, **kw)
    for call in (lambda: build_mesh_bvh(mesh), lambda: mesh_raycast(bvh, rays, rays), lambda: mesh_raycast_into(bvh, rays, rays),
                 lambda: visible_from(bvh, rays, (0.0, 0.0, 1.0)), lambda: camera_rays(CameraView(np.eye(4)[:3], 10.0, 10.0, 4.0, 4.0, 8, 8), "cpu"),
                 lambda: mesh_camera_thermogram(bvh, CameraView(np.eye(4)[:3], 10.0, 10.0, 4.0, 4.0, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    good = dict(c2w=np.eye(4)[:3], fx=10.0, fy=10.0, cx=4.0, cy=4.0, width=8, height=8)
    for change in (dict(width=0), dict(height=16385), dict(fx=0.0), dict(fy=-1.0), dict(cx=math.nan), dict(c2w=np.eye(3)),
                   dict(c2w=np.full((3, 4), math.inf))):
        with pytest.raises(ValueError):
            mesh_camera_thermogram(bvh, CameraView(**dict(good, **change)))
    assert CameraView(**dict(good, c2w=np.eye(4))).matrix().shape == (3, 4)
    with pytest.raises(ValueError, match="eye"):
        visible_from(bvh, rays, (0.0, math.nan, 1.0))
    assert raycast_module.VISIBLE_FRACTION == 1.0 - 2.0 ** -10 and np.float32(raycast_module.VISIBLE_FRACTION) < 1.0
    with pytest.raises(ValueError, match="does not carry the header"):
        bvh.tree()


@pytest.mark.parametrize("entry", list(mesh_arguments.ENTRIES))
def test_every_mesh_entry_refuses_a_host_mesh_in_one_order(entry):
    """the CPU half of tests/test_gpu_mesh_arguments.py: "no triangles" comes before "no CPU fallback", whichever entry is asked"""
    mesh = mesh_arguments.quad("cpu")
    bvh = MeshBVH(torch.zeros(192, dtype=torch.uint8), 4, 2, mesh)
    call = mesh_arguments.ENTRIES[entry][0]
    with pytest.raises(ValueError, match="the mesh has no triangles"):
        call(dataclasses.replace(mesh, triangles=None), bvh, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(mesh, bvh, "cpu")


def _hand_made():
    """a 2 x 3 camera view on the host: one empty pixel; the camera at (1, 2, 3) looks along -z"""
    nan = math.nan
    camera = CameraView([[1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]], 2.0, 2.0, 1.5, 1.0, 3, 2)
    temperature = torch.tensor([[20.0, 21.5, nan], [30.0, 19.0, 30.0]])
    face = torch.tensor([[4, 4, -1], [7, 2, 9]], dtype=torch.int32)
    distance = torch.tensor([[2.0, 1.5, nan], [2.0, 0.5, 2.5]])
    colors = torch.zeros((2, 3, 3), dtype=torch.uint8)
    origins = torch.tensor([[1.0, 2.0, 3.0]]).repeat(6, 1)
    directions = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.6, -0.8], [0.6, 0.0, -0.8], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    return CameraThermogram(face, distance, temperature, colors, camera, origins, directions, 5, 24.1, 19.0, 30.0, 8, 0, (14.0, 33.0))


def test_camera_thermogram_methods_that_need_no_kernel():
    found = _hand_made()
    assert found.world_position(0, 0) == (1.0, 2.0, 1.0) and found.world_position(1, 1) == (1.5, 2.0, 3.0)
    assert all(math.isnan(c) for c in found.world_position(0, 2))
    assert found.to_rgb8("rgb") is found.pixel_colors
    with pytest.raises(ValueError):
        found.to_rgb8("grey")
    from thermo_nerf_amd.export import ThermalRegions
    from thermo_nerf_amd.export.regions import REGION_DTYPE

    face_region = torch.tensor([-1, -1, 5, -1, 0, -1, -1, 3, -1, -1], dtype=torch.int32)
    regions = ThermalRegions(np.zeros(0, REGION_DTYPE), np.zeros(0, np.int64), face_region, 1.0, 0.5, 6, 3, 10, (20.0, 30.0))
    assert found.region_map(regions).tolist() == [[0, 0, -1], [3, 5, -1]]
    with pytest.raises(ValueError, match="another mesh"):
        found.region_map(ThermalRegions(np.zeros(0, REGION_DTYPE), np.zeros(0, np.int64), face_region[:9], 1.0, 0.5, 6, 3, 9, (20.0, 30.0)))


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_command_line_refuses_bad_arguments(capsys):
    tool = _tool()
    base = ["mesh.ply", "--transforms", "transforms.json", "--frame", "7", "--output", "v.png"]
    args = tool.parse(base)
    assert (args.frame, args.scale, args.cull_back, args.colors, args.temperatures, args.report, args.probe) == ("7", 1.0, False, "thermal", None, None, [])
    args = tool.parse(base + ["--scale", "0.5", "--cull-back", "--colors", "rgb", "--temperatures", "t.npy", "--report", "v.json", "--probe", "3", "4",
                              "--probe", "0", "9"])
    assert args.scale == 0.5 and args.cull_back and args.colors == "rgb" and args.probe == [[3, 4], [0, 9]] and str(args.report) == "v.json"
    for bad, flag in ((["--scale", "0"], "--scale"), (["--scale", "inf"], "--scale"), (["--scale", "nan"], "--scale"), (["--colors", "x"], "--colors"),
                      (["--probe", "-1", "2"], "--probe"), (["--probe", "1"], "--probe")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    for missing in ("--transforms", "--frame", "--output"):
        k = base.index(missing)
        with pytest.raises(SystemExit):
            tool.parse(base[:k] + base[k + 2:])
        assert missing in capsys.readouterr().err
    for flag in ("--transforms", "--frame", "--scale", "--cull-back", "--colors", "--output", "--temperatures", "--report", "--probe"):
        assert flag in tool.__doc__, flag
    assert "original world frame" in " ".join(tool.__doc__.split())


def test_frames_and_cameras_are_read_like_the_dataparser_reads_them():
    tool = _tool()
    pose = [[1.0, 0.0, 0.0, 0.5], [0.0, 0.0, -1.0, 1.5], [0.0, 1.0, 0.0, 2.5], [0.0, 0.0, 0.0, 1.0]]
    meta = {"fl_x": 100.0, "fl_y": 110.0, "cx": 64.0, "cy": 48.0, "w": 128, "h": 96,
            "frames": [{"file_path": "images/frame_00002.png", "transform_matrix": np.eye(4).tolist()},
                       {"file_path": "images/frame_00001.png", "transform_matrix": pose, "fl_x": 5.0},
                       {"file_path": "other/frame_00001.png", "transform_matrix": pose}]}
    assert tool.find_frame(meta, "images/frame_00001.png") == 1 and tool.find_frame(meta, "frame_00002.png") == 0 and tool.find_frame(meta, "frame_00002") == 0
    assert tool.find_frame(meta, "2") == 2 and tool.find_frame(meta, "0") == 0
    for bad in ("frame_00001.png", "nothing.png", "3", "-1"):
        with pytest.raises(ValueError, match="--frame"):
            tool.find_frame(meta, bad)
    with pytest.raises(ValueError, match="no frames"):
        tool.find_frame({"frames": []}, "0")
    camera = tool.frame_camera(meta, 1)
    assert camera == {"c2w": pose[:3], "fx": 100.0, "fy": 110.0, "cx": 64.0, "cy": 48.0, "width": 128, "height": 96}, "the file's value wins"
    half = tool.frame_camera(meta, 1, 0.5)
    assert (half["fx"], half["fy"], half["cx"], half["cy"], half["width"], half["height"]) == (50.0, 55.0, 32.0, 24.0, 64, 48)
    per_frame = {"frames": [dict(meta["frames"][1], fl_x=90.0, fl_y=91.0, cx=10.0, cy=11.0, w=20, h=22)]}
    assert tool.frame_camera(per_frame, 0)["fx"] == 90.0 and tool.frame_camera(per_frame, 0)["height"] == 22
    with pytest.raises(ValueError, match="fl_y"):
        tool.frame_camera({"fl_x": 1.0, "frames": meta["frames"]}, 0)
    with pytest.raises(ValueError, match="perspective"):
        tool.frame_camera(dict(meta, camera_model="OPENCV_FISHEYE"), 0)
    with pytest.raises(ValueError, match="--scale"):
        tool.frame_camera(meta, 0, 0.001)
    # applied_transform (a 3 x 4 the poses were multiplied with) and applied_scale are undone: the PLY is in the frame before them
    applied = [[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]]
    moved = tool.frame_camera(dict(meta, applied_transform=applied, applied_scale=2.0), 1)
    want = np.linalg.inv(np.concatenate([applied, [[0, 0, 0, 1]]])) @ np.array(pose)
    want[:3, 3] /= 2.0
    assert np.allclose(moved["c2w"], want[:3], atol=1e-15)
    # export/_common.py and pointcloud.py: the exporters' to_world is the inverse of the dataparser's transform and scale
    from thermo_nerf_amd.export import world_transform

    assert "original world frame" in " ".join(world_transform.__doc__.split())


def test_report_schema_with_a_hand_made_result():
    tool = _tool()
    found = _hand_made()
    camera = {"c2w": found.camera.c2w, "fx": 2.0, "fy": 2.0, "cx": 1.5, "cy": 1.0, "width": 3, "height": 2}
    arrays = (found.origins.numpy(), found.directions.numpy(), found.pixel_temperature.numpy(), found.pixel_face.numpy(), found.pixel_distance.numpy())
    report = tool.build_report(camera, "images/a.png", 4, found, *arrays, 12, 10, True, "mesh.ply")
    assert json.loads(json.dumps(report)) == report, "plain JSON: no numpy scalars, no infinities"
    assert set(report) == {"mesh", "frame", "frame_index", "camera", "counts", "covered_share", "mean_temperature", "min_temperature", "max_temperature",
                           "hottest_pixel", "coldest_pixel"}
    assert report["camera"] == {"c2w": [[1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]], "fx": 2.0, "fy": 2.0, "cx": 1.5, "cy": 1.0,
                                "width": 3, "height": 2, "cull_back": True}
    assert report["counts"] == {"vertices": 12, "faces": 10, "usable_faces": 8, "pixels": 6, "covered_pixels": 5, "stack_limit_rays": 0}
    assert (report["covered_share"], report["mean_temperature"], report["min_temperature"], report["max_temperature"]) == (5 / 6, 24.1, 19.0, 30.0)
    assert report["hottest_pixel"] == {"row": 1, "column": 0, "temperature": 30.0, "distance": 2.0, "face": 7, "position": [1.0, 2.0, 1.0]}, \
        "the first of two equally hot pixels"
    assert report["coldest_pixel"] == {"row": 1, "column": 1, "temperature": 19.0, "distance": 0.5, "face": 2, "position": [1.5, 2.0, 3.0]}
    assert (report["frame"], report["frame_index"], report["mesh"]) == ("images/a.png", 4, "mesh.ply")
    line = tool.summary_line(report, "mesh.ply")
    assert "\n" not in line and line.startswith("mesh.ply from images/a.png: 3 x 2 pixels, 5 covered (83.3 %), mean 24.10 C")
    probe = tool.probe_line(tool.pixel_record(camera, *arrays, 0, 1))
    assert probe.startswith("probe (0, 1): 21.50 C at distance 1.5, face 4, position (1, 2.9, 1.8)")
    assert tool.probe_line(tool.pixel_record(camera, *arrays, 0, 2)) == "probe (0, 2): nothing there"
    import dataclasses

    nothing = dataclasses.replace(found, pixel_temperature=torch.full((2, 3), math.nan), covered=0, mean_temperature=math.nan,
                                  min_temperature=math.inf, max_temperature=-math.inf)
    empty = tool.build_report(camera, "a", 0, nothing, arrays[0], arrays[1], nothing.pixel_temperature.numpy(), arrays[3], arrays[4], 12, 10, False)
    assert json.loads(json.dumps(empty)) == empty and empty["hottest_pixel"] is None and empty["mean_temperature"] is None
    assert "nothing covered" in tool.summary_line(empty, "mesh.ply")
