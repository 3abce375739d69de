"""tn_mesh_register on the device against tests/mesh_register_reference.py, exactly — the transform, every history row, the result and
the per-wave partials the workspace holds, bit for bit, no tolerance anywhere — through the raw entry into guarded buffers with the
inputs unchanged afterwards: point counts around the wave and one past 256 waves (the finish's run boundary), face counts around the
tile, both metrics with and without scale, one iteration and a run to convergence on the L-shaped boxes, points beyond the radius
and points that are not numbers, nothing matched, a face without area, the identity on surface points, determinism, a zeroed blob,
the Python layer on two plane grids with a known shift followed by ``mesh_difference``, and the command line."""
from __future__ import annotations

import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_closest_reference as C
from tests import mesh_raycast_reference as R
from tests import mesh_register_reference as G
from tests.test_gpu_mesh_raycast import GUARD, Scene, _buffer, _device, _untouched
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (ThermalMesh, build_mesh_bvh, mesh_difference, read_mesh_ply, register_mesh, register_points,
                                    register_workspace_bytes, transform_mesh, write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
assert GUARD >= 64


def _params(max_distance=math.inf, center=(0.0, 0.0, 0.0), length=1.0, damping=0.0, tolerance=0.0, iterations=1, metric=G.PLANE,
            with_scale=False, min_pairs=1):
    return _hip.tn_register_params(float(max_distance), (_hip.C.c_double * 3)(*center), float(length), float(damping), float(tolerance),
                                   int(iterations), int(metric), 1 if with_scale else 0, int(min_pairs))


class Mesh(Scene):
    """the ray cast's scene — a mesh on the device with its tree, built through the raw entry into guarded buffers — and the run"""

    def register(self, points, transform=None, **kw):
        """tn_mesh_register into guarded buffers: host copies of what was written"""
        points = np.ascontiguousarray(points, F).reshape(-1, 3)
        n, iterations = len(points), kw.get("iterations", 1)
        cloud = _device(points)
        start = G.IDENTITY.copy() if transform is None else np.ascontiguousarray(transform, D).reshape(12)
        matrix, history, result = _buffer(12, torch.float64), _buffer(4 * iterations, torch.float64), _buffer(4, torch.int64)
        matrix[:12] = _device(start)
        need = register_workspace_bytes(n)
        assert need == G.workspace_bytes(n)
        workspace = _buffer(need, torch.uint8)
        p, t, tri = self.pointers()
        work = self.v > 0 and self.t > 0
        _hip.check(_hip.load().tn_mesh_register(
            p if work else None, t if work else None, tri, self.v, self.t, self.blob.data_ptr(), self.blob_bytes,
            cloud.data_ptr() if n else None, n, _params(**kw), matrix.data_ptr(), history.data_ptr(), result.data_ptr(),
            workspace.data_ptr(), need, _hip.current_stream()), "tn_mesh_register")
        torch.cuda.synchronize()
        for buf, size, name in ((matrix, 12, "transform"), (history, 4 * iterations, "history"), (result, 4, "result"),
                                (workspace, need, "workspace")):
            _untouched(buf, size, name)
        self.unchanged()
        assert points.tobytes() == cloud.cpu().numpy().tobytes(), "the cloud was written"
        return {"transform": matrix[:12].cpu().numpy(), "history": history[:4 * iterations].cpu().numpy().reshape(iterations, 4),
                "result": result[:4].cpu().numpy(), "partials": workspace[64:need].cpu().numpy().view(D).reshape(-1, G.WORDS)}

    def reference(self, points, transform=None, **kw):
        pos, temp, _, tri = self.host
        return G.register(pos, temp, tri, points, transform=transform, **kw)

    def check(self, points, transform=None, want=None, **kw):
        """one run compared with the yardstick, bit for bit"""
        want = self.reference(points, transform, **kw) if want is None else want
        got = self.register(points, transform, **kw)
        _same(got, want)
        return want, got


def _same(got, want):
    assert got["result"].tolist() == want["result"].tolist(), ("result", got["result"], want["result"])
    for name in ("history", "transform", "partials"):
        a, b = np.ascontiguousarray(got[name]).view(np.uint64), np.ascontiguousarray(want[name], D).view(np.uint64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        differ = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        assert len(differ) == 0, (name, len(differ), "first differing entry", int(differ[0]), got[name].reshape(-1)[differ[0]],
                                  np.asarray(want[name]).reshape(-1)[differ[0]])


@functools.lru_cache(maxsize=None)
def soup(faces):
    pos, temp, col, tri, points = C.scene(f"soup-{faces}")
    return Mesh(pos, temp, col, tri), points


@functools.lru_cache(maxsize=None)
def cube():
    pos, tri = R.box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1)
    return Mesh(pos, R.attributes(len(pos), 6)[0], None, tri)


@functools.lru_cache(maxsize=None)
def boxes():
    pos, temp, tri = G.l_boxes()
    return Mesh(pos, temp, None, tri), G.box_of(pos)


def _near(seed):
    """a start near the identity, so that an iteration moves something"""
    rng = np.random.default_rng(seed)
    return G.similarity(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.05, 0.05, 3), 1.0 + rng.uniform(-0.03, 0.03), (0.5, 0.5, 0.5))[:3].reshape(12)


OPTIONS = [(G.PLANE, False), (G.PLANE, True), (G.POINT, False), (G.POINT, True)]


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces", C.SIZES)
def test_point_counts_around_the_wave_against_face_counts_around_the_tile(faces):
    scene, points = soup(faces)
    for k, n in enumerate((0, 1, 63, 64, 65, 129)):
        metric, with_scale = OPTIONS[(k + faces) % 4]
        want, got = scene.check(points[:n], _near(n), center=(0.5, 0.5, 0.5), length=1.7, damping=1e-6, iterations=2, metric=metric,
                                with_scale=with_scale, min_pairs=1)
        assert got["partials"].shape == ((n + 63) // 64, 40)
        if faces == 0 or n == 0:
            assert got["result"].tolist() == [G.TOO_FEW, 1, 0, n if faces else n] and (got["history"][1] == G.NOT_RUN).all()
        else:
            assert got["result"][2] + got["partials"][:, 38].sum() == n, "every point has a face as soon as there is one"


@pytest.mark.parametrize("metric,with_scale", OPTIONS)
def test_both_metrics_with_and_without_scale_one_iteration_and_three(metric, with_scale):
    scene, points = soup(257)
    for iterations in (1, 3):
        want, got = scene.check(points, _near(7), center=(0.5, 0.5, 0.5), length=1.7, damping=1e-6, iterations=iterations, metric=metric,
                                with_scale=with_scale, min_pairs=6)
        assert got["result"].tolist()[:2] == [G.ITERATIONS, iterations] and got["result"][3] == len(points)
        assert (got["history"][:, 2] > 0).all() and not np.array_equal(got["transform"], _near(7))
    scale = np.cbrt(np.linalg.det(got["transform"].reshape(3, 4)[:, :3]) / np.linalg.det(_near(7).reshape(3, 4)[:, :3]))
    assert (abs(scale - 1.0) > 1e-6) == with_scale, "without scale the update is a rigid motion"


@pytest.mark.parametrize("which", ["cube", "soup-257"])
def test_one_point_past_256_waves_crosses_the_run_boundary(which):
    scene = cube() if which == "cube" else soup(257)[0]
    points = np.random.default_rng(41).uniform(-0.25, 1.25, (16385, 3)).astype(F)
    for n in (16385,) + ((1, 63, 64, 65, 129, 0) if which == "cube" else ()):
        want, got = scene.check(points[:n], _near(3), center=(0.5, 0.5, 0.5), length=1.7, damping=1e-6, iterations=2,
                                metric=G.PLANE if n % 2 else G.POINT, with_scale=True, min_pairs=1)
        assert len(got["partials"]) == (n + 63) // 64
        if n == 16385:
            assert got["result"].tolist() == [G.ITERATIONS, 2, 16385, 16385] and len(got["partials"]) == 257, "two runs of waves: 256 and 1"


# ---- a run to convergence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_scale", [False, True])
def test_run_to_convergence_on_the_l_boxes(with_scale):
    scene, (center, length) = boxes()
    pos, _, _, tri = scene.host
    truth = G.similarity((0.05, -0.04, 0.047), (0.1, -0.08, 0.07), 1.07 if with_scale else 1.0, center)
    cloud = G.moved_cloud(G.surface_points(pos, tri, 600, 1), truth)
    want, got = scene.check(cloud, None, max_distance=0.5, center=center, length=length, damping=1e-6, tolerance=1e-9, iterations=30,
                            metric=G.PLANE, with_scale=with_scale, min_pairs=6)
    ran = int(got["result"][1])
    assert got["result"].tolist() == [G.CONVERGED, ran, 600, 600] and 4 <= ran <= 8, "every point is matched: nothing passes by being left out"
    assert (got["history"][ran:] == G.NOT_RUN).all() and (got["history"][:ran, 0] == 600).all()
    assert np.abs(got["transform"].reshape(3, 4) - truth[:3]).max() < 1e-7
    few, got = scene.check(cloud, None, max_distance=0.5, center=center, length=length, damping=1e-6, tolerance=1e-9, iterations=5,
                           metric=G.POINT, with_scale=with_scale, min_pairs=6)
    assert got["result"].tolist() == [G.ITERATIONS, 5, 600, 600] and (np.diff(got["history"][:, 1]) < 0).all(), "point to point: slower, and still going"


# ---- points and faces that are left out ----------------------------------------------------------------------------------------------------

def test_points_beyond_the_radius_points_that_are_not_numbers_and_nothing_matched():
    scene, (center, length) = boxes()
    pos, _, _, tri = scene.host
    rng = np.random.default_rng(9)
    cloud = (G.surface_points(pos, tri, 200, 2) + rng.normal(0.0, 0.01, (200, 3))).astype(F)
    cloud[::7] += F(0.75)                       # beyond the radius
    cloud[[3, 64, 130]] = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)]
    for metric, with_scale in OPTIONS:
        want, got = scene.check(cloud, None, max_distance=0.125, center=center, length=length, damping=1e-6, iterations=3, metric=metric,
                                with_scale=with_scale, min_pairs=6)
        assert got["result"][3] == 197 and 100 < got["result"][2] < 180
    start = _near(5)
    huge = start.copy()
    huge[3] = 1e308
    huge[0] = 1e308                             # x overflows for some points: unusable, not a fault
    want, got = scene.check(cloud, huge, max_distance=0.125, center=center, length=length, iterations=1)
    assert got["result"][0] == G.TOO_FEW and got["result"][3] < 197
    lifted = cloud + F(10.0)
    want, got = scene.check(lifted, start, max_distance=0.5, center=center, length=length, damping=1e-6, iterations=4, min_pairs=6)
    assert got["result"].tolist() == [G.TOO_FEW, 1, 0, 197] and got["transform"].tobytes() == start.tobytes(), "the transform's bytes are unchanged"
    assert got["history"][0].tolist() == [0.0, 0.0, G.NOT_RUN, G.NOT_RUN] and (got["history"][1:] == G.NOT_RUN).all()
    want, got = scene.check(cloud, start, max_distance=0.125, center=center, length=length, damping=0.0, iterations=2, min_pairs=0,
                            metric=G.PLANE)
    pos, temp, tri = C.plane_grid(4, 0.0, 20.0)
    plane = Mesh(pos, temp, None, tri)
    above = np.array([(x, y, 0.25) for x in (0.5, 1.75, 3.0) for y in (0.25, 2.0, 3.5)], F)
    want, got = plane.check(above, None, center=(2.0, 2.0, 0.0), length=4.0, damping=0.0, iterations=2, min_pairs=6)
    assert got["result"].tolist() == [G.DEGENERATE, 1, 9, 9] and got["transform"].tobytes() == G.IDENTITY.tobytes(), "a bare plane lets the cloud slide"


def test_a_face_without_area_has_no_normal():
    pos, temp, tri = G.l_boxes()
    needle = np.array([(10, 0, 0), (10, 0, 0), (10, 4, 0)], F)
    scene = Mesh(np.concatenate([pos, needle]), np.concatenate([temp, np.array([1, 2, 3], F)]), None,
                 np.concatenate([tri, np.array([(len(pos), len(pos) + 1, len(pos) + 2)], np.int32)]))
    center, length = G.box_of(pos)
    near = G.surface_points(pos, tri, 100, 4) + np.random.default_rng(4).normal(0.0, 0.01, (100, 3))  # off the faces: something to move
    cloud = np.concatenate([near, [(10.5, 1, 0), (9, 2, 1), (10, 5, 0)]]).astype(F)
    want, got = scene.check(cloud, None, center=center, length=length, damping=1e-6, iterations=2, metric=G.PLANE, min_pairs=6)
    assert got["result"].tolist() == [G.ITERATIONS, 2, 100, 103] and got["partials"][:, 38].tolist() == [0.0, 3.0]
    want, got = scene.check(cloud, None, center=center, length=length, damping=1e-6, iterations=1, metric=G.POINT, min_pairs=6)
    assert got["result"].tolist() == [G.ITERATIONS, 1, 103, 103], "point to point needs no normal"


def test_identity_on_surface_points_converges_in_the_first_iteration():
    scene, (center, length) = boxes()
    pos, _, _, tri = scene.host
    corner = pos[tri.astype(np.int64)].astype(D)
    cloud = np.concatenate([pos, (corner[:, 0] + corner[:, 1]) / 2]).astype(F)   # vertices and edge midpoints: dyadic, exactly on faces
    for metric, with_scale in OPTIONS:
        want, got = scene.check(cloud, None, max_distance=0.0, center=center, length=length, damping=1e-6, tolerance=0.0, iterations=4,
                                metric=metric, with_scale=with_scale, min_pairs=6)
        assert got["result"].tolist() == [G.CONVERGED, 1, len(cloud), len(cloud)] and got["history"][0].tolist() == [len(cloud), 0.0, 0.0, 0.0]
        assert got["transform"].tolist() == G.IDENTITY.tolist()


def test_two_runs_are_byte_equal_and_a_zeroed_blob_matches_nothing():
    scene, points = soup(257)
    kw = dict(center=(0.5, 0.5, 0.5), length=1.7, damping=1e-6, iterations=3, metric=G.PLANE, with_scale=True, min_pairs=6)
    first, again = scene.register(points, _near(1), **kw), scene.register(points, _near(1), **kw)
    for name in ("transform", "history", "result", "partials"):
        assert first[name].tobytes() == again[name].tobytes(), ("two runs differ", name)
    good = scene.blob.clone()
    try:
        scene.blob.zero_()
        got = scene.register(points, _near(1), **kw)
        assert got["result"].tolist() == [G.TOO_FEW, 1, 0, len(points)] and got["transform"].tobytes() == _near(1).tobytes()
        scene.blob.copy_(good)
        nodes = scene.blob[64 + (4 * scene.t + 63) // 64 * 64: scene.blob_bytes].view(torch.int32).reshape(-1, 16)
        nodes[:, 12] = 2 ** 30      # child 0 of every node: beyond the tree
        nodes[:, 13] = 0            # child 1: the root again, a cycle
        assert scene.register(points, _near(1), **kw)["result"].tolist() == [G.TOO_FEW, 1, 0, len(points)]  # no fault, and it ends
    finally:
        scene.blob.copy_(good)
    _same(scene.register(points, _near(1), **kw), {k: first[k] for k in first})


# ---- the Python layer and the command line --------------------------------------------------------------------------------------------------

def _two_surveys():
    """A: a plane grid at z = 0 with T = 20 + 4 x; B: the same grid at z = 0.25 with T = 21.5 + 4 x: A registered onto B moves up by
    0.25 and is 1.5 degrees colder everywhere"""
    meshes = []
    for z, offset in ((0.0, 20.0), (0.25, 21.5)):
        pos, temp, tri = C.plane_grid(4, z, offset)
        meshes.append(ThermalMesh(_device(pos), _device(R.attributes(len(pos), 3)[1]), _device(temp), None, _device(tri), (20.0, 40.0)))
    return meshes


def test_python_layer_recovers_a_known_shift_and_feeds_mesh_difference():
    a, b = _two_surveys()
    tree = build_mesh_bvh(b)
    found = register_mesh(a, tree, max_distance=[1.0, 0.5])
    assert found.status == "converged" and found.converged and (found.matched, found.matched_share, found.usable_points) == (25, 1.0, 25)
    assert len(found.stages) == 2 and [s["max_distance"] for s in found.stages] == [1.0, 0.5] and found.iterations == len(found.rms) <= 8
    assert found.rms[0] == 0.25 and found.rms[-1] < 1e-9 and abs(found.scale - 1.0) < 1e-12
    want = np.eye(4)
    want[2, 3] = 0.25
    assert np.abs(found.matrix - want).max() < 1e-9, "the plane fixes z and two tilts; the damping leaves the sliding directions alone"
    pos, temp, tri = C.plane_grid(4, 0.25, 21.5)
    center, length = G.box_of(pos)
    ref = G.register(pos, temp, tri, a.positions.cpu().numpy(), max_distance=1.0, center=center, length=length, damping=1e-6, tolerance=1e-9,
                     iterations=30, metric=G.PLANE, min_pairs=6)
    assert found.stages[0]["iterations"] == int(ref["result"][1])
    moved = transform_mesh(a, found.matrix)
    assert moved.colors is a.colors and moved.temperature is a.temperature and moved.triangles is a.triangles
    assert moved.positions.dtype == torch.float32 and float((moved.positions - b.positions).abs().max()) < 1e-6
    delta = mesh_difference(moved, tree, max_distance=0.05)
    assert delta.matched == 25 and delta.max_distance < 1e-6 and abs(delta.mean_difference + 1.5) < 1e-5
    none = register_points(tree, a.positions, max_distance=0.125)
    assert none.status == "too_few" and none.matched == 0 and np.array_equal(none.matrix, np.eye(4)) and none.iterations == 1
    bare = register_points(tree, a.positions, max_distance=1.0, damping=0.0)
    assert bare.status == "degenerate" and np.array_equal(bare.matrix, np.eye(4))
    strided = register_mesh(a, tree, max_distance=1.0, max_points=9)
    assert strided.usable_points == 9 and strided.status == "converged"


def test_command_line_on_two_small_plys(tmp_path, capsys):
    a, b = _two_surveys()
    moving, fixed = tmp_path / "now.ply", tmp_path / "before.ply"
    write_mesh_ply(moving, a)
    write_mesh_ply(fixed, b)
    spec = importlib.util.spec_from_file_location("mesh_register_tool", os.path.join(ROOT, "tools", "mesh_register.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, matrix, report = tmp_path / "registered.ply", tmp_path / "matrix.txt", tmp_path / "register.json"
    assert tool.main([str(moving), str(fixed), "--max-distance", "1.0", "0.5", "--output", str(out), "--matrix", str(matrix), "--report",
                      str(report)]) == 0
    printed = capsys.readouterr().out
    found = json.loads(report.read_text())
    assert found["status"] == "converged" and found["matched_share"] == 1.0 and len(found["stages"]) == 2 and abs(found["scale"] - 1.0) < 1e-12
    got = np.loadtxt(matrix)
    assert got.shape == (4, 4) and np.array_equal(got, np.array(found["matrix"])) and abs(got[2, 3] - 0.25) < 1e-9
    assert "converged" in printed and "25 of 25 matched" in printed
    data = read_mesh_ply(out)
    assert np.abs(data["positions"] - b.positions.cpu().numpy()).max() < 1e-6 and data["temperature"].tolist() == a.temperature.cpu().tolist()
    assert data["triangles"].tolist() == a.triangles.cpu().tolist()
