"""tn_mesh_closest on the device against tests/mesh_closest_reference.py, exactly — every integer and every float bit pattern, no
tolerance anywhere — through the raw entry into guarded buffers with the inputs unchanged afterwards: sizes around the tile and the
wave, the literal triangle and the faces without area, ties (a shared edge, a shared vertex, 300 copies of one triangle, the centre of
a cube), unusable faces and points, the cut (0, a distance equal to it, +inf), geometry that stresses the pruning (a flat mesh, a chain
25 deep, a mesh 10^6 units away), a room and a soup of a few thousand faces, absent outputs, determinism, a zeroed blob, the Python
layer on two plane grids with a known difference, and the command line."""
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
from tests.test_gpu_mesh_raycast import DEV, FILLS, GUARD, Scene, _buffer, _device, _untouched
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (ThermalMesh, build_mesh_bvh, mesh_closest, mesh_difference, read_mesh_ply, thermal_regions,
                                    write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
OUT = {"closest_face": (torch.int32, 1), "closest_distance": (torch.float32, 1), "closest_point": (torch.float32, 3),
       "closest_uv": (torch.float32, 2), "closest_temperature": (torch.float32, 1), "closest_colors": (torch.uint8, 3),
       "difference": (torch.float32, 1)}
assert tuple(OUT) == C.OUTPUTS and GUARD >= 64 and len(FILLS) == 5


class Mesh(Scene):
    """the ray cast's scene — a mesh on the device with its tree, built through the raw entry into guarded buffers — and the query"""

    def closest(self, points, point_temperature=None, max_distance=math.inf, absent=()):
        """tn_mesh_closest into guarded buffers (``absent``: the outputs passed as NULL): host copies of what was written"""
        points = np.ascontiguousarray(points, F).reshape(-1, 3)
        n = len(points)
        given = [points] + ([np.ascontiguousarray(point_temperature, F).reshape(-1)] if point_temperature is not None else [])
        inputs = [_device(a) for a in given]
        no_colors = self.col is None or not self.v
        missing = set(absent) | ({"closest_colors"} if no_colors else set())
        if point_temperature is None or "closest_temperature" in missing:
            missing.add("difference")
        buffers = {k: None if k in missing else _buffer(n * width, dtype) for k, (dtype, width) in OUT.items()}
        counts = None if "counts" in absent else _buffer(4, torch.int64)
        stats = None if ("stats" in absent or buffers["closest_distance"] is None) else _buffer(8, torch.float64)
        params = _hip.tn_closest_params(max_distance)
        p, t, tri = self.pointers()
        work = self.v > 0 and self.t > 0
        _hip.check(_hip.load().tn_mesh_closest(
            p if work else None, t if work else None, _hip.ptr(self.col) if self.v else None, tri, self.v, self.t, self.blob.data_ptr(),
            self.blob_bytes, inputs[0].data_ptr() if n else None, inputs[1].data_ptr() if len(inputs) > 1 and n else None, n, params,
            *[_hip.ptr(buffers[k]) for k in OUT], _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()), "tn_mesh_closest")
        torch.cuda.synchronize()
        out = {}
        for name, buf in list(buffers.items()) + [("counts", counts), ("stats", stats)]:
            if buf is None:
                out[name] = None
                continue
            width = OUT[name][1] if name in OUT else 1
            size = {"counts": 4, "stats": 8}.get(name, n * width)
            _untouched(buf, size, name)
            host = buf[:size].cpu().numpy()
            out[name] = host.reshape(n, width) if width > 1 else host
        self.unchanged()
        for before, now in zip(given, inputs):
            assert before.tobytes() == now.cpu().numpy().tobytes(), "a query input was written"
        return out

    def reference(self, points, point_temperature=None, **kw):
        return C.closest(*self.host, points, point_temperature=point_temperature, **kw)

    def check(self, points, point_temperature=None, want=None, absent=(), **kw):
        """one call compared with the yardstick, bit for bit, on every output it was given"""
        want = self.reference(points, point_temperature, **kw) if want is None else want
        got = self.closest(points, point_temperature, absent=absent, **kw)
        _same(got, want)
        return want, got


def _same(got, want):
    if got["counts"] is not None:
        assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
        assert got["counts"][3] == 0, "a point reached the stack limit"
    for name in OUT:
        if got[name] is not None:
            assert want[name] is not None and got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            differ = np.flatnonzero(np.ascontiguousarray(got[name]).view(np.uint8).reshape(-1) != np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1))
            assert len(differ) == 0, (name, len(differ), "first differing byte", int(differ[0]))
    if got["stats"] is not None:
        stats = want["stats"].copy()
        if got["difference"] is None:
            stats[4:] = (0.0, 0.0, math.inf, -math.inf)
        assert got["stats"].view(np.uint64).tolist() == stats.view(np.uint64).tolist(), ("stats", got["stats"], stats)


@functools.lru_cache(maxsize=None)
def mesh(name):
    pos, temp, col, tri, points = C.scene(name)
    return Mesh(pos, temp, col, tri), points


def own_temperature(n, seed=0):
    return np.random.default_rng(seed).uniform(5.0, 40.0, n).astype(F)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces", C.SIZES)
def test_sizes_around_the_tile_and_the_wave(faces):
    scene, points = mesh(f"soup-{faces}")
    for n in (0, 1, 63, 64, 65, 129):
        want, _ = scene.check(points[:n], own_temperature(n, n))
        assert want["counts"].tolist() == [n if faces else 0, n, faces, 0], "every point has a face as soon as there is one"


def test_mesh_without_vertices():
    scene = Mesh(np.zeros((0, 3), F), np.zeros(0, F), None, np.array([(0, 1, 2), (0, 0, 0)], np.int32))
    want, got = scene.check(C.TRIANGLE_POINTS, own_temperature(12))
    assert got["counts"].tolist() == [0, 12, 0, 0] and (got["closest_face"] == -1).all() and got["closest_colors"] is None
    assert got["stats"].tolist() == [0.0, 0.0, math.inf, -math.inf, 0.0, 0.0, math.inf, -math.inf]


# ---- literal and degenerate cases, ties ---------------------------------------------------------------------------------------------------

def test_one_triangle_and_faces_without_area():
    scene, points = mesh("triangle")
    want, got = scene.check(points, np.full(12, 20.0, F))
    assert got["closest_distance"][[0, 1, 2, 6, 9]].tolist() == [0.0, 2.0, 3.0, 2.0, 0.0] and got["closest_temperature"][[0, 2, 8]].tolist() == [17.5, 22.5, 25.0]
    assert got["closest_uv"][[2, 4, 5, 8]].tolist() == [[0.25, 0.5], [1, 0], [0, 1], [0.5, 0.5]] and got["difference"][[2, 3]].tolist() == [-2.5, 10.0]
    scene, points = mesh("degenerate")
    want, got = scene.check(points, own_temperature(len(points)))
    assert got["closest_face"].tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 1] and got["closest_uv"][[0, 4, 6]].tolist() == [[0.5, 0], [0, 0.5], [0, 1]]
    for name in ("closest_distance", "closest_point", "closest_uv", "closest_temperature", "difference"):
        assert np.isfinite(got[name]).all(), name


def test_ties_go_to_the_lowest_face_index():
    scene = Mesh(*C.SHEETS)
    want, got = scene.check(C.SHEET_POINTS, own_temperature(6))
    assert got["closest_face"].tolist() == [0, 2, 1, 1, 1, 0] and got["closest_distance"].tolist() == [3.0, 2.0, 1.0, 0.0, 1.0, 2.0]
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F)
    copies = Mesh(pos, np.array([10, 20, 30], F), None, np.tile(np.array([(0, 1, 2)], np.int32), (300, 1)))
    points = np.array([(0.25, 0.25, 1), (0.25, 0.25, 0), (2, 2, 1), (0, 0, 0), (-1, -1, -1), (0.5, 0.5, 0)], F)
    want, got = copies.check(points)
    assert got["closest_face"].tolist() == [0] * 6 and got["counts"].tolist() == [6, 6, 300, 0], "equal d2 three hundred times: face 0"
    box = R.box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1)
    temp, col = R.attributes(len(box[0]), 6)
    cube = Mesh(box[0], temp, col, box[1])
    assert cube.t == 12
    points = np.array([(0.5, 0.5, 0.5), (0, 0, 0), (1, 1, 1), (1, 0.5, 0.5), (0.5, 0.5, 0.75)], F)
    want, got = cube.check(points, own_temperature(5))
    assert got["closest_face"][0] == 0 and got["closest_distance"].tolist() == [0.5, 0.0, 0.0, 0.0, 0.25], "the centre is 0.5 from all twelve"
    d2 = np.array([C.closest(box[0], temp, col, box[1][k:k + 1], points[:1])["d2"][0] for k in range(12)])
    assert (d2 == 0.25).all()
    assert got["closest_face"][1] == min(k for k in range(12) if (box[0][box[1][k]] == 0).all(axis=1).any()), "the lowest face at that corner"


# ---- unusable things ------------------------------------------------------------------------------------------------------------------------

def test_unusable_faces_never_win_and_unusable_points_find_nothing():
    scene, points = mesh("unusable")
    points = points.copy()
    points[[3, 70, 71, 199]] = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (np.nan, np.nan, np.nan)]
    own = own_temperature(len(points))
    own[[5, 6]] = [np.nan, np.inf]
    want, got = scene.check(points, own)
    assert got["counts"].tolist() == [196, 196, 1, 0] and set(got["closest_face"].tolist()) == {-1, 3}
    for name in ("closest_distance", "closest_temperature", "difference"):
        assert C.bits(got[name][[3, 70, 71, 199]]).tolist() == [C.NAN_BITS] * 4, name
    assert C.bits(got["closest_point"][3]).tolist() == [C.NAN_BITS] * 3 and got["closest_colors"][3].tolist() == [0, 0, 0]
    assert C.bits(got["difference"][5:6]).tolist() == [C.NAN_BITS] and got["difference"][6] == math.inf
    pos, temp, col, tri = scene.host
    none = Mesh(pos, temp, col, np.delete(tri, 3, axis=0))
    want, got = none.check(points, own)
    assert got["counts"].tolist() == [0, 196, 0, 0] and (got["closest_face"] == -1).all() and C.bits(got["closest_uv"]).reshape(-1).tolist() == [C.NAN_BITS] * 400


# ---- the cut ------------------------------------------------------------------------------------------------------------------------------------

def test_max_distance_zero_exact_and_infinite():
    pos, temp, tri = C.plane_grid(4, 0.0, 20.0)
    scene = Mesh(pos, temp, R.attributes(len(pos), 2)[1], tri)
    on = np.array([(1, 1, 0), (0.5, 2.5, 0), (4, 4, 0), (0, 3.25, 0), (1.5, 1.5, 0)], F)  # vertices, points on edges and diagonals
    off = np.array([(1, 1, 2.0 ** -20), (-(2.0 ** -20), 1, 0), (2, 2, -1), (5, 5, 0)], F)
    want, got = scene.check(np.concatenate([on, off]), max_distance=0.0)
    assert got["closest_face"][:5].min() >= 0 and got["closest_face"][5:].tolist() == [-1] * 4 and got["closest_distance"][:5].tolist() == [0.0] * 5
    above = np.array([(x, y, 3.0) for x in (0.0, 0.75, 2.0, 3.5) for y in (0.25, 1.0, 4.0)], F)
    want, got = scene.check(above, max_distance=3.0)
    assert got["counts"][0] == 12 and got["closest_distance"].tolist() == [3.0] * 12, "a distance equal to the cut is inside"
    want, got = scene.check(above, max_distance=float(np.nextafter(3.0, 0.0)))
    assert got["counts"][0] == 0
    want, got = scene.check(np.concatenate([above, off * F(1e6)]), own_temperature(16), max_distance=math.inf)
    assert got["counts"][0] == 16
    want, got = scene.check(np.concatenate([above, off]), max_distance=1e-300)  # R2 underflows to 0
    assert got["counts"][0] == 0


# ---- geometry that stresses the pruning ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat", "chain", "far"])
def test_flat_boxes_a_deep_chain_and_a_mesh_a_million_units_away(name):
    scene, points = mesh(name)
    if name == "chain":
        assert scene.bvh().tree()["depth"] >= 25
    want, got = scene.check(points, own_temperature(len(points), 3))
    assert got["counts"].tolist() == [len(points), len(points), scene.t, 0]
    if name == "far":
        assert got["closest_distance"].min() > 0.9e6 and len(np.unique(got["closest_face"])) > 20
    half = float(np.median(want["closest_distance"]))
    want, got = scene.check(points, max_distance=half)
    assert 0 < got["counts"][0] < len(points)


# ---- the larger scenes ------------------------------------------------------------------------------------------------------------------------------

def test_device_reference_is_the_numpy_reference():
    pos, temp, col, tri, points = C.scene("soup-257")
    own = own_temperature(len(points))
    host = C.closest(pos, temp, col, tri, points, own, max_distance=0.5)
    device = C.closest(pos, temp, col, tri, points, own, max_distance=0.5, torch_device=DEV, chunk=50)
    for name in C.OUTPUTS + ("counts", "stats", "d2"):
        assert host[name].tobytes() == device[name].tobytes(), name
    assert 0 < host["counts"][0] < len(points)


@pytest.mark.parametrize("name", ["room", "soup"])
def test_a_few_thousand_faces_against_a_few_thousand_points(name):
    scene, points = mesh(name)
    own = own_temperature(len(points), 4)
    want = C.closest(*scene.host, points, own, torch_device=DEV, chunk=1024)
    assert scene.t > 2000 and want["counts"].tolist() == [2400, 2400, scene.t, 0], "every point has a face: nothing is compared by leaving it out"
    assert len(np.unique(want["closest_face"])) > 500 and (want["closest_distance"][1600:] < 1e-6).all(), "the last third lies on faces"
    _, got = scene.check(points, own, want=want)
    again = scene.closest(points, own)
    for name_ in list(OUT) + ["counts", "stats"]:
        assert got[name_].tobytes() == again[name_].tobytes(), ("two calls differ", name_)
    cut = float(np.median(want["closest_distance"][:1600]))
    near = C.closest(*scene.host, points, own, max_distance=cut, torch_device=DEV, chunk=1024)
    assert 1600 <= near["counts"][0] < 2400
    scene.check(points, own, want=near, max_distance=cut)


# ---- call behaviour ------------------------------------------------------------------------------------------------------------------------------------

def test_absent_outputs_and_a_zeroed_blob():
    scene, points = mesh("soup-257")
    own = own_temperature(len(points))
    want = scene.reference(points, own)
    for absent in (("closest_face",), ("closest_distance",), ("closest_point", "closest_uv"), ("closest_temperature",), ("closest_colors",),
                   ("difference",), ("counts",), ("stats",), ("closest_face", "closest_point", "closest_uv", "closest_colors", "counts"),
                   ("closest_distance", "closest_temperature"), tuple(OUT) + ("counts", "stats")):
        got = scene.closest(points, own, absent=absent)
        assert all(got[k] is None for k in absent), absent
        _same(got, want)
    without = scene.closest(points)  # no point_temperature: no difference, and its statistics say so
    assert without["difference"] is None and without["stats"][4:].tolist() == [0.0, 0.0, math.inf, -math.inf]
    _same(without, want)
    good = scene.blob.clone()
    try:
        scene.blob.zero_()
        got = scene.closest(points, own)
        assert got["counts"].tolist() == [0, len(points), 0, 0] and (got["closest_face"] == -1).all()
        assert C.bits(got["closest_distance"]).tolist() == [C.NAN_BITS] * len(points) and not got["closest_colors"].any()
        scene.blob.copy_(good)
        nodes = scene.blob[64 + (4 * scene.t + 63) // 64 * 64: scene.blob_bytes].view(torch.int32).reshape(-1, 16)
        nodes[:, 12] = 2 ** 30      # child 0 of every node: beyond the tree
        nodes[:, 13] = 0            # child 1: the root again, a cycle
        assert (scene.closest(points, own)["closest_face"] == -1).all()  # other numbers, no fault, and it ends
        scene.blob.copy_(good)
        scene.blob[64: 64 + 4 * scene.t].view(torch.int32)[:] = 2 ** 30
        assert (scene.closest(points, own)["closest_face"] == -1).all()
    finally:
        scene.blob.copy_(good)
    _same(scene.closest(points, own), want)


# ---- the Python layer and the command line --------------------------------------------------------------------------------------------------------------

def _two_surveys():
    """A: a plane grid at z = 0 with T = 20 + 4 x; B: the same grid at z = 0.25 with T = 21.5 + 4 x.  Every vertex of A is 0.25 from B,
    at a vertex of B, and 1.5 degrees colder than B there: exactly"""
    meshes = []
    for z, offset in ((0.0, 20.0), (0.25, 21.5)):
        pos, temp, tri = C.plane_grid(4, z, offset)
        meshes.append(ThermalMesh(_device(pos), _device(R.attributes(len(pos), 3)[1]), _device(temp), None, _device(tri), (20.0, 40.0)))
    return meshes


def test_python_layer_difference_of_two_plane_grids():
    a, b = _two_surveys()
    tree = build_mesh_bvh(b)
    found = mesh_difference(a, tree, max_distance=1.0)
    assert (found.matched, found.matched_share, found.closest.found, found.closest.usable_points, found.closest.usable_faces) == (25, 1.0, 25, 25, 32)
    assert (found.mean_distance, found.rms_distance, found.max_distance, found.closest.min_distance) == (0.25, 0.25, 0.25, 0.25)
    assert (found.mean_difference, found.rms_difference, found.min_difference, found.max_difference) == (-1.5, 1.5, -1.5, -1.5)
    delta = found.mesh
    assert delta.temperature.cpu().tolist() == [-1.5] * 25 and delta.temperature_bounds == (-1.5, 1.5) and delta.thermal_colors is None
    assert delta.positions is a.positions and delta.colors is a.colors and delta.triangles is a.triangles
    assert found.closest.closest_point.cpu().numpy().tobytes() == b.positions.cpu().numpy().tobytes() and found.closest.stack_limit_points == 0
    assert found.closest.closest_temperature.cpu().tolist() == b.temperature.cpu().tolist()
    want = C.closest(*(x.cpu().numpy() for x in (b.positions, b.temperature, b.colors, b.triangles)), a.positions.cpu().numpy(),
                     a.temperature.cpu().numpy())
    assert found.closest.closest_face.cpu().numpy().tolist() == want["closest_face"].tolist()
    assert found.closest.closest_colors.cpu().numpy().tobytes() == want["closest_colors"].tobytes()
    cooled = thermal_regions(delta, max_temperature=-1.0)
    assert len(cooled) == 1 and cooled.regions[0]["faces"] == 32 and cooled.regions[0]["area"] == 16.0 and cooled.regions[0]["mean_temperature"] == -1.5
    assert len(thermal_regions(delta, min_temperature=1.0)) == 0
    beyond = mesh_difference(a, tree, max_distance=0.125)
    assert beyond.matched == 0 and beyond.matched_share == 0.0 and bool(torch.isnan(beyond.mesh.temperature).all()) and beyond.mesh.temperature_bounds is None
    assert math.isnan(beyond.mean_difference) and math.isnan(beyond.mean_distance) and beyond.closest.usable_points == 25
    assert thermal_regions(beyond.mesh, max_temperature=math.inf, min_temperature=-1e30).usable_faces == 0, "a NaN vertex makes its faces unusable"
    points = torch.cat([a.positions[:3], torch.full((1, 3), math.nan, device=DEV)])
    some = mesh_closest(tree, points, max_distance=0.25)
    assert (some.found, some.usable_points, some.mean_distance, some.difference, some.mean_difference) == (3, 3, 0.25, None, None)
    import dataclasses

    other = ThermalMesh(b.positions, b.colors, b.temperature, None, b.triangles[:-1].contiguous())
    with pytest.raises(ValueError, match="another mesh"):
        mesh_closest(dataclasses.replace(tree, mesh=other), points)
    with pytest.raises(ValueError, match="point_temperature must hold N values"):
        mesh_closest(tree, points, point_temperature=a.temperature)


def test_command_line_on_two_small_plys(tmp_path, capsys):
    a, b = _two_surveys()
    now, before = tmp_path / "now.ply", tmp_path / "before.ply"
    write_mesh_ply(now, a)
    write_mesh_ply(before, b)
    spec = importlib.util.spec_from_file_location("mesh_compare_tool", os.path.join(ROOT, "tools", "mesh_compare.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, report = tmp_path / "diff.ply", tmp_path / "diff.json"
    assert tool.main([str(now), str(before), "--max-distance", "0.5", "--output", str(out), "--report", str(report), "--min-change", "1.0",
                      "--length-scale", "2.0"]) == 0
    printed = capsys.readouterr().out
    found = json.loads(report.read_text())
    assert found["counts"] == {"vertices": 25, "faces": 32, "reference_vertices": 25, "reference_faces": 32, "reference_usable_faces": 32,
                               "matched_vertices": 25, "stack_limit_points": 0}
    assert found["matched_share"] == 1.0 and found["distance"] == {"mean": 0.5, "rms": 0.5, "max": 0.5}, "lengths times --length-scale"
    assert found["difference"] == {"mean": -1.5, "rms": 1.5, "min": -1.5, "max": -1.5} and found["min_change"] == 1.0
    assert found["warmed"] == {"regions": [], "area": 0.0, "share": 0.0} and found["cooled"]["area"] == 64.0 and found["cooled"]["share"] == 1.0
    assert found["cooled"]["regions"] == [{"region": 0, "faces": 32, "area": 64.0, "mean_difference": -1.5, "largest_change": -1.5, "centroid": [4.0, 4.0, 0.0]}]
    assert "25 matched (100.0 %)" in printed and "cooled 0: area 64, 32 faces, mean -1.50 C" in printed and "warmed" not in printed
    data = read_mesh_ply(out)
    assert data["temperature"].tolist() == [-1.5] * 25 and data["positions"].tobytes() == a.positions.cpu().numpy().tobytes()
    assert data["triangles"].tolist() == a.triangles.cpu().tolist() and "temperature_bounds -1.5 1.5" in data["comments"]
