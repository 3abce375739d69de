"""The yardstick of the registration (tests/mesh_register_reference.py) checked on its own — literal cases with hand-computed rows,
the order of its sums, the two refusals, the recovery of known similarities on the L-shaped boxes and of a plane grid's offset — and
the host side of the feature: the declaration, the struct, the refusals of the entry and of the Python layer, the closed-form start,
``transform_mesh``, the command line and its report.  No GPU."""
from __future__ import annotations

import ctypes
import dataclasses
import importlib.util
import json
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mesh_closest_reference as C
from tests import mesh_register_reference as G
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (MeshBVH, Registration, ThermalMesh, mesh_bvh_bytes, register_mesh, register_points, register_points_into,
                                    register_workspace_bytes, similarity_from_pairs, transform_mesh)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_register_tool", os.path.join(ROOT, "tools", "mesh_register.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the reference on literal cases -----------------------------------------------------------------------------------------------------

def test_one_point_on_a_face_gives_zero_sums_and_no_step():
    pos, temp, _, tri = C.TRIANGLE
    for metric in (G.PLANE, G.POINT):
        got = G.register(pos, temp, tri, np.array([(1, 1, 0)], F), center=(1.0, 1.0, 0.0), length=4.0, damping=1e-6, metric=metric)
        assert got["partials"].shape == (1, 40) and got["partials"][0, 28:36].tolist() == [0.0] * 8, "r = 0: no right-hand side, no error"
        assert got["partials"][0, 36:].tolist() == [1.0, 1.0, 0.0, 0.0] and [abs(d) for d in got["deltas"][0]] == [0.0] * 7
        assert got["transform"].tolist() == G.IDENTITY.tolist() and got["result"].tolist() == [G.CONVERGED, 1, 1, 1]
        assert got["history"].tolist() == [[1.0, 0.0, 0.0, 0.0]]
    off = G.register(pos, temp, tri, np.array([(1, 1, 0)], F), center=(1.0, 1.0, 0.0), length=4.0, damping=0.0, metric=G.POINT)
    assert off["result"].tolist() == [G.DEGENERATE, 1, 1, 1], "y = 0: the rotation's pivots are 0 without damping"


def test_a_point_above_a_plane_grid_gives_the_literal_row():
    pos, temp, tri = C.plane_grid(4, 0.0, 20.0)
    scene = C._scene(pos, temp, tri, None)
    center = (2.0, 2.0, 0.0)
    partials, seen = G.iteration_sums(scene, G.IDENTITY, np.array([(0.5, 1.0, 0.25)], F), math.inf, center, G.PLANE)
    # y = (-1.5, -1, 0.25), n = (0, 0, 1): y x n = (-1, 1.5, 0), n . y = 0.25; e = (0, 0, 0.25), r = 0.25
    g = [-1.0, 1.5, 0.0, 0.0, 0.0, 1.0, 0.25]
    assert seen["c"].tolist() == [[0.5, 1.0, 0.0]] and seen["matched"].tolist() == [True]
    assert partials[0, :28].tolist() == [g[i] * g[j] for i in range(7) for j in range(i, 7)]
    assert partials[0, 28:35].tolist() == [x * 0.25 for x in g] and partials[0, 35] == 0.0625 and partials[0, 36:].tolist() == [1.0, 1.0, 0.0, 0.0]
    rows, _ = G.iteration_sums(scene, G.IDENTITY, np.array([(0.5, 1.0, 0.25)], F), math.inf, center, G.POINT)
    # three rows n = ex, ey, ez: only the last has r != 0
    assert rows[0, 35] == 0.0625 and np.abs(rows[0, 28:35] - partials[0, 28:35]).max() == 0.0, "the same right-hand side as the one plane row"
    assert rows[0, [0, 7, 13]].tolist() == [1.0 + 0.0625, 2.25 + 0.0625, 2.25 + 1.0], "S[0][0], S[1][1], S[2][2]: sums of squares of y's other two"
    moved = G.transformed(np.array([2, 0, 0, 1, 0, 2, 0, 1, 0, 0, 2, 1], D), np.array([(1, 2, 3), (np.nan, 0, 0)], F))
    assert moved[0][0].tolist() == [3.0, 5.0, 7.0] and moved[1].tolist() == [True, False]


def test_the_wave_tree_and_the_runs_of_256_are_the_written_orders():
    rng = np.random.default_rng(2)
    sums = np.zeros((130, 36), D)
    sums[:, 0] = rng.uniform(-1.0, 1.0, 130) * 10.0 ** rng.integers(-8, 8, 130)
    flags = np.ones(130, bool)
    partials = G.wave_partials(sums, flags, flags, ~flags)

    def tree(x):
        return x[0] if len(x) == 1 else tree([x[k] + x[k + 1] for k in range(0, len(x), 2)])

    lanes = np.zeros(192, D)
    lanes[:130] = sums[:, 0]
    assert partials[:, 0].tolist() == [tree(lanes[64 * w: 64 * w + 64].tolist()) for w in range(3)] and partials[:, 36].tolist() == [64.0, 64.0, 2.0]
    assert partials[:, 0].tolist() != [sum(lanes[64 * w: 64 * w + 64].tolist()) for w in range(3)], "the inputs tell the tree from a running sum"
    many = np.zeros((600, 40), D)
    many[:, 5] = rng.uniform(-1.0, 1.0, 600) * 10.0 ** rng.integers(-8, 8, 600)
    runs = [sum(many[a:b, 5].tolist(), 0.0) for a, b in ((0, 256), (256, 512), (512, 600))]
    assert G.totals(many)[5] == (0.0 + runs[0] + runs[1]) + runs[2] and G.totals(many)[5] != sum(many[:, 5].tolist(), 0.0)
    assert G.totals(np.zeros((0, 40), D)).tolist() == [0.0] * 40


def test_too_few_pairs_and_a_bare_plane_are_refused_with_the_transform_unchanged():
    pos, temp, tri = C.plane_grid(4, 0.0, 20.0)
    above = np.array([(x, y, 0.25) for x in (0.5, 1.75, 3.0) for y in (0.25, 2.0, 3.5)], F)
    start = G.similarity((0.0, 0.0, 0.01), (0.01, 0.0, 0.0))[:3].reshape(12)
    kw = dict(center=(2.0, 2.0, 0.0), length=4.0, iterations=5, transform=start)
    few = G.register(pos, temp, tri, above, min_pairs=10, damping=1e-6, **kw)
    assert few["result"].tolist() == [G.TOO_FEW, 1, 9, 9] and few["transform"].tobytes() == start.tobytes()
    assert few["history"][0].tolist() == [9.0, 9 * 0.0625, G.NOT_RUN, G.NOT_RUN] and (few["history"][1:] == G.NOT_RUN).all()
    far = G.register(pos, temp, tri, above, max_distance=0.125, min_pairs=1, damping=1e-6, **kw)
    assert far["result"].tolist() == [G.TOO_FEW, 1, 0, 9]
    bare = G.register(pos, temp, tri, above, min_pairs=6, damping=0.0, **kw)
    assert bare["result"].tolist() == [G.DEGENERATE, 1, 9, 9] and bare["transform"].tobytes() == start.tobytes(), "a plane lets the cloud slide and spin"
    assert bare["history"][0, 2:].tolist() == [G.NOT_RUN, G.NOT_RUN]
    for metric in (G.PLANE, G.POINT):
        flat = G.register(*[x for x in C.degenerate_mesh() if x is not None], C.DEGENERATE_POINTS, metric=metric, damping=1e-6, min_pairs=1)
        assert flat["result"].tolist() == ([G.TOO_FEW, 1, 0, 10] if metric == G.PLANE else [G.ITERATIONS, 1, 10, 10]), "faces without area have no normal"
        assert flat["partials"][0, 38] == (10.0 if metric == G.PLANE else 0.0)


# ---- recovery ------------------------------------------------------------------------------------------------------------------------------

# Measured on the reference against the known truth, max |entry| of the recovered 3 x 4 minus the true one (the cloud is the exact
# pre-image rounded to fp32, which is what limits it; the point-to-point runs stop on the tolerance 1e-9 while still converging
# linearly): plane 1.15e-9 (5 iterations), plane with scale 3.13e-9 (6), point 1.49e-8 (72), point with scale 1.03e-8 (74), the plane
# grid 0 (3).  The bounds are 10 x these: the arithmetic is libm-free and BLAS-free, the same everywhere.
RECOVERY = {(G.PLANE, False): 1.15e-8, (G.PLANE, True): 3.13e-8, (G.POINT, False): 1.49e-7, (G.POINT, True): 1.03e-7}


@pytest.mark.parametrize("metric,with_scale", list(RECOVERY))
def test_reference_recovers_a_known_similarity_on_the_l_boxes(metric, with_scale):
    """600 points on the 240 faces of two boxes that form an L, moved by 0.08 rad and 0.15 units (and 7 % in size): every point is
    matched in every iteration, so nothing passes by being left out (200 points under the point metric, which needs over 70
    iterations where point to plane needs 5 - 6: its rate is linear).  Measured max |entry error| of the recovered matrix: 1.15e-9,
    3.13e-9 (with scale), 1.49e-8, 1.03e-8 (point, with scale); asserted: 10 x each."""
    pos, temp, tri = G.l_boxes()
    assert len(tri) == 240
    center, length = G.box_of(pos)
    truth = G.similarity((0.05, -0.04, 0.047), (0.1, -0.08, 0.07), 1.07 if with_scale else 1.0, center)
    cloud = G.moved_cloud(G.surface_points(pos, tri, 600 if metric == G.PLANE else 200, 1), truth)
    got = G.register(pos, temp, tri, cloud, max_distance=0.5, center=center, length=length, damping=1e-6, tolerance=1e-9,
                     iterations=30 if metric == G.PLANE else 120, metric=metric, with_scale=with_scale, min_pairs=6)
    ran = int(got["result"][1])
    assert got["result"].tolist() == [G.CONVERGED, ran, len(cloud), len(cloud)] and (got["history"][:ran, 0] == len(cloud)).all()
    assert (ran <= 7) == (metric == G.PLANE)
    error = float(np.abs(got["transform"].reshape(3, 4) - truth[:3]).max())
    print(f"metric {metric} scale {with_scale}: {ran} iterations, max |entry error| {error:.3g}")
    assert error < RECOVERY[(metric, with_scale)]
    assert (np.diff(got["history"][:ran, 1]) < 0).all() or metric == G.PLANE, "point to point: the error falls in every iteration"


def test_reference_recovers_the_plane_grids_offset_with_damping():
    pos, temp, tri = C.plane_grid(4, 0.25, 21.5)
    cloud = C.plane_grid(4, 0.0, 20.0)[0]
    center, length = G.box_of(pos)
    got = G.register(pos, temp, tri, cloud, max_distance=1.0, center=center, length=length, damping=1e-6, tolerance=1e-9, iterations=30,
                     min_pairs=6)
    assert got["result"].tolist() == [G.CONVERGED, 3, 25, 25] and got["history"][0, :2].tolist() == [25.0, 25 * 0.0625]
    want = G.IDENTITY.copy()
    want[11] = 0.25
    error = float(np.abs(got["transform"] - want).max())
    print(f"plane grid: max |entry error| {error:.3g}")
    assert error == 0.0, "measured 0: the sliding directions and the spin are left exactly alone, and 0.25 is found to the bit"
    assert got["transform"][[3, 7]].tolist() == [0.0, 0.0] and got["transform"][[1, 4]].tolist() == [0.0, 0.0]


# ---- the declarations and the refusals ---------------------------------------------------------------------------------------------------

NAMES = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "bvh", "bvh_bytes", "points", "num_points", "params",
         "transform", "history", "result", "workspace", "workspace_bytes", "stream")
FIELDS = ["max_distance", "center", "length", "damping", "tolerance", "iterations", "metric", "with_scale", "min_pairs", "reserved"]


def test_entry_struct_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = re.search(r"\bint tn_mesh_register\(([^;]*)\);", header).group(1)
    assert [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")] == list(NAMES)
    assert header.index("int tn_mesh_project(") < header.index("size_t tn_mesh_register_workspace_bytes(") < header.index("int tn_mesh_register("), \
        "behind the projection"
    result, arguments = _hip.SIGNATURES["tn_mesh_register"]
    assert result == ctypes.c_int and len(arguments) == len(NAMES) and arguments[9] == ctypes.POINTER(_hip.tn_register_params)
    assert arguments[3] == arguments[4] == arguments[8] == ctypes.c_int64 and arguments[6] == arguments[14] == ctypes.c_size_t
    assert _hip.SIGNATURES["tn_mesh_register_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64])
    params = _hip.tn_register_params
    assert ctypes.sizeof(params) == 80 and [f[0] for f in params._fields_] == FIELDS
    assert [getattr(params, f).offset for f in FIELDS] == [0, 8, 32, 40, 48, 56, 60, 64, 68, 72]
    body = re.search(r"typedef struct tn_register_params \{([^}]*)\} tn_register_params;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;\[])", body) == FIELDS
    for name, value in (("POINT", 0), ("PLANE", 1), ("CONVERGED", 0), ("ITERATIONS", 1), ("TOO_FEW", 2), ("DEGENERATE", 3)):
        assert re.search(rf"#define TN_REGISTER_{name} {value}\b", header), name
        assert getattr(G, name) == value
    assert _hip.TN_REGISTER_STATUS == G.STATUS and (_hip.TN_REGISTER_POINT, _hip.TN_REGISTER_PLANE) == (G.POINT, G.PLANE)
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert "tn_mesh_project.hip tn_mesh_register.hip" in makefile and "tn_mesh_bvh.h tn_mesh_closest.h " in makefile
    text = " ".join(header.split())
    assert "given there holds for this Q as it stands" in text and "the damping is ADDITIVE" in text
    shared = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_mesh_closest.h")).read()
    for source in ("tn_mesh_closest.hip", "tn_mesh_register.hip"):
        code = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", source)).read()
        assert '#include "tn_mesh_closest.h"' in code and "face_nearest(" in code and "double box_bound(" not in code, source
    assert "double box_bound(" in shared and "bool face_nearest(" in shared, "one definition of the bound and of the face's arithmetic"


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _hip.load()
    limit = (2 ** 31 - 1) // 3
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy, t, n = 4096, 2000, 500
    blob, need = mesh_bvh_bytes(t), register_workspace_bytes(n)
    assert need == G.workspace_bytes(n) == 64 + 320 * 8 and register_workspace_bytes(0) == 64 and register_workspace_bytes(16385) == 64 + 320 * 257

    def params(**change):
        values = dict(max_distance=math.inf, center=(0.0, 0.0, 0.0), length=1.0, damping=1e-6, tolerance=1e-9, iterations=30, metric=1,
                      with_scale=0, min_pairs=6)
        values.update(change)
        values["center"] = (ctypes.c_double * 3)(*values["center"])
        return _hip.tn_register_params(*[values[k] for k in FIELDS[:-1]])

    good = dict(zip(NAMES, [dummy, dummy, dummy, 1000, t, dummy, blob, dummy, n, params(), dummy, dummy, dummy, dummy, need - 1, None]))

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_register(*[args[k] for k in NAMES])

    assert call() == -4 and call(workspace_bytes=0) == -4 and call(workspace_bytes=need, bvh_bytes=blob - 1) == -4  # TN_ERR_WORKSPACE: the last refusal
    for k in ("positions", "temperature", "triangles", "bvh", "points", "params", "transform", "history", "result", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert call(num_points=-1) == -2 and call(num_points=limit + 1) == -2  # TN_ERR_SHAPE
    for bad in (dict(max_distance=math.nan), dict(max_distance=-1.0), dict(center=(math.nan, 0, 0)), dict(center=(0, math.inf, 0)), dict(length=0.0),
                dict(length=-1.0), dict(length=math.inf), dict(length=math.nan), dict(damping=-1e-9), dict(damping=math.inf), dict(damping=math.nan),
                dict(tolerance=-1.0), dict(tolerance=math.nan), dict(iterations=0), dict(iterations=1025), dict(metric=2), dict(metric=-1),
                dict(with_scale=2), dict(min_pairs=-1)):
        assert call(params=params(**bad)) == -3, bad  # TN_ERR_UNSUPPORTED
    for fine in (dict(max_distance=0.0), dict(max_distance=math.inf), dict(damping=0.0), dict(tolerance=0.0), dict(tolerance=math.inf),
                 dict(iterations=1), dict(iterations=1024), dict(metric=0), dict(with_scale=1), dict(min_pairs=0), dict(length=1e-300)):
        assert call(params=params(**fine)) == -4, fine
    for k in ("positions", "temperature", "triangles", "points"):
        assert call(**{k: dummy + 2}) == -2, k
    for k in ("transform", "history", "result", "workspace"):
        assert call(**{k: dummy + 4}) == -2, k
    assert call(bvh=dummy + 32) == -2
    bad = params(length=0.0)
    assert call(params=bad, bvh=None) == -1 and call(params=bad, num_points=-1) == -2 and call(params=bad, points=None) == -3 and \
        call(points=None, transform=dummy + 4) == -1 and call(transform=dummy + 4, workspace_bytes=0) == -2, "in the siblings' order"
    assert call(num_points=0, points=None, workspace_bytes=63) == -4 and call(num_points=0, points=None, workspace_bytes=64, bvh_bytes=0) == -4
    assert call(num_vertices=0, positions=None, temperature=None) == -4, "a mesh without vertices needs no arrays"
    assert call(num_triangles=0, triangles=None, positions=None, temperature=None, bvh_bytes=63) == -4


def _host_mesh():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    return mesh, MeshBVH(torch.zeros(128, dtype=torch.uint8), 3, 1, mesh)


def test_python_layer_refuses_before_it_reaches_a_kernel():
    mesh, bvh = _host_mesh()
    points = torch.zeros((4, 3))
    for bad, word in ((dict(max_distance=-1.0), "max_distance"), (dict(max_distance=math.nan), "max_distance"), (dict(metric="line"), "metric"),
                      (dict(iterations=0), "iterations"), (dict(iterations=2000), "iterations"), (dict(tolerance=-1.0), "tolerance"),
                      (dict(damping=-1.0), "damping"), (dict(damping=math.inf), "damping"), (dict(min_pairs=-1), "min_pairs"),
                      (dict(length=0.0), "length"), (dict(center=(0.0, math.nan, 0.0)), "center")):
        options = dict(dict(max_distance=1.0, center=(0.0, 0.0, 0.0), length=1.0), **bad)
        with pytest.raises(ValueError, match=word):
            register_points_into(bvh, points, torch.zeros(12, dtype=torch.float64), torch.zeros(120, dtype=torch.float64),
                                 torch.zeros(4, dtype=torch.int64), **options)
    for call in (lambda: register_points(bvh, points, max_distance=1.0), lambda: register_mesh(mesh, bvh, max_distance=[1.0, 0.5]),
                 lambda: register_points_into(bvh, points, torch.zeros(12, dtype=torch.float64), torch.zeros(120, dtype=torch.float64),
                                              torch.zeros(4, dtype=torch.int64), max_distance=1.0, center=(0.0, 0.0, 0.0), length=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        register_points(bvh, points)  # the radius is required: there is no distance that suits every pair of surveys
    with pytest.raises(ValueError, match="non-empty"):
        register_points(bvh, points, max_distance=[])
    with pytest.raises(ValueError, match="initial"):
        register_points(bvh, points, max_distance=1.0, initial=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="max_points"):
        register_mesh(mesh, bvh, max_distance=1.0, max_points=0)
    assert {"matrix", "scale", "status", "iterations", "matched", "matched_share", "usable_points", "rms", "stages"} == \
        {f.name for f in dataclasses.fields(Registration)}


# ---- the closed-form start and the transform of a mesh -------------------------------------------------------------------------------------

def test_similarity_from_exact_dyadic_pairs():
    source = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0.5)], D)
    turn = np.array([(0, -1, 0), (1, 0, 0), (0, 0, 1)], D)  # a quarter turn about z
    target = 2.0 * source @ turn.T + np.array([1.0, 2.0, 3.0])
    got = similarity_from_pairs(source, target)
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = 2.0 * turn, (1.0, 2.0, 3.0)
    assert np.abs(got - want).max() < 1e-14 and got[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    rigid = similarity_from_pairs(source, source @ turn.T + 0.5, with_scale=False)
    assert np.abs(rigid[:3, :3] - turn).max() < 1e-14 and np.abs(rigid[:3, 3] - 0.5).max() < 1e-14
    kept = similarity_from_pairs(torch.from_numpy(source), target, with_scale=False)
    assert abs(np.linalg.det(kept[:3, :3]) - 1.0) < 1e-14, "without scale: the best rigid motion, whatever the targets' size"
    mirrored = similarity_from_pairs(source, source * np.array([1.0, 1.0, -1.0]))
    assert np.linalg.det(mirrored[:3, :3]) > 0.0, "never a reflection"
    for bad in ((source[:2], target[:2]), (source, target[:4]), (np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2)], D),) * 2, (source * np.nan, target)):
        with pytest.raises(ValueError):
            similarity_from_pairs(*bad)


def test_transform_mesh_round_trip():
    rng = np.random.default_rng(8)
    pos = torch.from_numpy(rng.uniform(-2.0, 2.0, (50, 3)).astype(F))
    normals = torch.nn.functional.normalize(torch.from_numpy(rng.normal(0.0, 1.0, (50, 3)).astype(F)), dim=1)
    mesh = ThermalMesh(pos, torch.zeros((50, 3), dtype=torch.uint8), torch.arange(50.0), None, torch.zeros((1, 3), dtype=torch.int32),
                       (0.0, 49.0), normals)
    matrix = G.similarity((0.3, -0.2, 0.5), (1.0, -2.0, 0.25), 1.5, (0.5, 0.5, 0.5))
    there = transform_mesh(mesh, matrix)
    want = (pos.numpy().astype(D) @ matrix[:3, :3].T + matrix[:3, 3]).astype(F)
    assert there.positions.dtype == torch.float32 and np.abs(there.positions.numpy() - want).max() <= 2.0 ** -21, "fp64, rounded once"
    for name in ("colors", "temperature", "triangles", "thermal_colors", "temperature_bounds"):
        assert getattr(there, name) is getattr(mesh, name), name
    rotation = matrix[:3, :3] / 1.5
    assert np.abs(there.normals.numpy() - normals.numpy().astype(D) @ rotation.T).max() < 1e-6 and there.normals.dtype == torch.float32
    back = transform_mesh(there, np.linalg.inv(matrix)[:3])  # 3 x 4 is accepted as well
    assert float((back.positions - pos).abs().max()) < 1e-6 and float((back.normals - normals).abs().max()) < 1e-6
    same = transform_mesh(mesh, np.eye(4))
    assert same.positions.numpy().tobytes() == pos.numpy().tobytes()
    exact = transform_mesh(mesh, np.array([(2, 0, 0, 1), (0, 2, 0, -1), (0, 0, 2, 0.5), (0, 0, 0, 1)], D))
    assert exact.positions.numpy().tolist() == (2.0 * pos.numpy() + np.array([1, -1, 0.5], F)).tolist()
    with pytest.raises(ValueError, match="determinant"):
        transform_mesh(mesh, np.diag([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="initial|matrix"):
        transform_mesh(mesh, np.eye(3))


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_command_line_arguments(capsys, tmp_path):
    tool = _tool()
    base = ["moving.ply", "fixed.ply", "--max-distance", "0.5", "--output", "registered.ply", "--matrix", "out.txt", "--report", "register.json"]
    args = tool.parse(base)
    assert (str(args.moving), str(args.fixed), args.max_distance, args.metric, args.with_scale, args.iterations, args.initial, args.pairs,
            args.max_points) == ("moving.ply", "fixed.ply", [0.5], "plane", False, 30, None, None, None)
    args = tool.parse(base[:2] + ["--max-distance", "1.0", "0.25", "0.05", "--metric", "point", "--with-scale", "--iterations", "50", "--pairs", "p.txt",
                                  "--max-points", "1000"] + base[4:])
    assert args.max_distance == [1.0, 0.25, 0.05] and (args.metric, args.with_scale, args.iterations, str(args.pairs), args.max_points) == \
        ("point", True, 50, "p.txt", 1000)
    for bad, flag in ((["--max-distance", "-1"], "--max-distance"), (["--max-distance", "nan"], "--max-distance"), (["--iterations", "0"], "--iterations"),
                      (["--iterations", "5000"], "--iterations"), (["--metric", "line"], "--metric"), (["--max-points", "0"], "--max-points"),
                      (["--initial", "a.txt", "--pairs", "b.txt"], "--pairs")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    for missing in ("--max-distance", "--output", "--matrix", "--report"):
        k = base.index(missing)
        with pytest.raises(SystemExit):
            tool.parse(base[:k] + base[k + 2:])
        assert missing in capsys.readouterr().err
    for flag in ("--initial", "--pairs", "--max-distance", "--metric", "--with-scale", "--iterations", "--max-points", "--output", "--matrix", "--report"):
        assert flag in tool.__doc__, flag
    (tmp_path / "m.txt").write_text("1 0 0 0.5\n0 1 0 0\n0 0 1 0\n")
    (tmp_path / "p.txt").write_text("0 0 0 1 2 3\n1 0 0 1 4 3\n0 1 0 -1 2 3\n0 0 1 1 2 5\n")
    assert tool.starting_matrix(tmp_path / "m.txt", None, False).tolist() == [[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    start = tool.starting_matrix(None, tmp_path / "p.txt", True)
    assert np.abs(start - np.array([(0, -2, 0, 1), (2, 0, 0, 2), (0, 0, 2, 3), (0, 0, 0, 1)], D)).max() < 1e-14
    assert abs(np.linalg.det(tool.starting_matrix(None, tmp_path / "p.txt", False)[:3, :3]) - 1.0) < 1e-14 and tool.starting_matrix(None, None, True) is None


def test_report_schema_with_a_hand_made_result():
    tool = _tool()
    matrix = np.eye(4)
    matrix[2, 3] = 0.25
    stages = [{"max_distance": 1.0, "status": "iterations", "iterations": 30, "matched": 20, "matched_share": 0.8, "rms": 0.125},
              {"max_distance": math.inf, "status": "converged", "iterations": 4, "matched": 25, "matched_share": 1.0, "rms": math.nan}]
    found = SimpleNamespace(matrix=matrix, scale=1.0, status="converged", iterations=34, matched=25, matched_share=1.0, usable_points=25,
                            rms=[0.25, math.nan], stages=stages)
    report = tool.build_report(found, 100, 25, "now.ply", "before.ply", "plane", True, np.eye(4))
    assert json.loads(json.dumps(report)) == report, "plain JSON: no numpy scalars, no infinities"
    assert set(report) == {"moving", "fixed", "metric", "with_scale", "vertices", "points", "status", "iterations", "scale", "matrix", "start",
                           "matched", "matched_share", "usable_points", "rms", "stages"}
    assert report["matrix"][2] == [0.0, 0.0, 1.0, 0.25] and report["rms"] == [0.25, None] and report["stages"][1]["max_distance"] is None
    assert report["stages"][0] == stages[0] and report["start"][0] == [1.0, 0.0, 0.0, 0.0] and report["with_scale"] is True
    line = tool.summary_line(report)
    assert "\n" not in line and line == "now.ply onto before.ply: converged after 34 iterations in 2 stage(s), 25 of 25 matched (100.0 %), rms -, scale 1"
