"""The yardstick of the projection (tests/mesh_project_reference.py) checked on its own — literal cases with hand-computed answers: a
wall seen head-on through a 4 x 4 image, pixel centres and the points between them, the image's border to the ulp, cos == min_cos, a
point behind the camera and one at the eye, equal weights, a wall hidden behind another, unusable points and cameras, calls without a
camera, a point or a face, the statistics' block order, the conditions of the random scene of the device test — and the host side of
the feature: the declaration, the structs, the refusals of the entry and of the Python layer, the command line and its report.  No GPU."""
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

from tests import mesh_project_reference as P
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (CameraView, MeshBVH, MeshMeasurement, ProjectedTemperatures, ThermalMesh, camera_records, mesh_bvh_bytes,
                                    mesh_measurement, project_images, project_images_into)
from thermo_nerf_amd.export.regions import REGION_DTYPE, ThermalRegions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NAN = P.NAN_BITS
UP = np.array([0.0, 0.0, 1.0], F)


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_project_tool", os.path.join(ROOT, "tools", "mesh_project.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _wall(points, cameras=None, images=None, normals=UP, t_lo=10.0, t_hi=40.0, **kw):
    points = np.asarray(points, F).reshape(-1, 3)
    cameras = np.stack([P.down_camera()]) if cameras is None else np.asarray(cameras, F).reshape(-1, 16)
    images = np.stack([P.WALL_IMAGE] * len(cameras)) if images is None else images
    normals = None if normals is None else np.broadcast_to(np.asarray(normals, F), points.shape)
    pos, tri = P.WALL
    return P.project(pos, np.full(len(pos), 20.0, F), tri, points, normals, cameras, images, t_lo, t_hi, **kw)


def _degrees(s, t_lo=10.0, t_hi=40.0):
    return float(F(t_lo + (s / 255.0) * (t_hi - t_lo)))


# ---- the reference on literal cases -----------------------------------------------------------------------------------------------------

def test_wall_seen_head_on_pixel_centres_and_between_them():
    """the camera at (0, 0, 4) looks down at the wall z = 0 through a 4 x 4 image, fx = fy = 1, cx = cy = 2: (x, y, 0) lands at
    u = 2 + x / 4, v = 2 - y / 4, so the centre of pixel (row r, column c) is the point (4 c - 6, 6 - 4 r, 0)"""
    points = [(-2, 2, 0), (-6, -6, 0), (-6, 6, 0), (0, 0, 0), (1, 0, 0), (2, -2, 0)]
    got = _wall(points, point_temperature=np.full(6, 25.0, F))
    assert got["views"].tolist() == [1] * 6 and got["best_camera"].tolist() == [0] * 6 and got["spread"].tolist() == [0.0] * 6
    # pixel (1, 1) holds 50; (3, 0) holds 255: exactly t_hi; (0, 0) holds 0: exactly t_lo; between the centres of (1,1) (1,2) (2,1) (2,2):
    # top = 55, bottom = 95, s = 75; a quarter pixel further right: top = 57.5, bottom = 97.5, s = 77.5; pixel (2, 2) holds 100
    assert got["measured"].tolist() == [_degrees(50.0), 40.0, 10.0, _degrees(75.0), _degrees(77.5), _degrees(100.0)]
    assert got["difference"].tolist() == [float(F(25.0 - D(x))) for x in got["measured"]]
    assert got["counts"].tolist() == [6, 6, 1, 6, 6, 0] and got["pairs"] == 6
    assert got["measured"].dtype == F and got["views"].dtype == np.int32 and got["counts"].dtype == np.int64 and got["stats"].shape == (8,)
    g = P.pair_geometry(P.down_camera(), np.array(points, F), np.tile(UP, (6, 1)), 4, 4)
    assert g["u"].tolist() == [1.5, 0.5, 0.5, 2.0, 2.25, 2.5] and g["v"].tolist() == [1.5, 3.5, 0.5, 2.0, 2.0, 2.5]
    assert g["w"][3] == 1.0 / 16.0 and g["cos"][3] == 1.0 and g["dist2"][0] == 24.0


def test_border_of_the_image_to_the_ulp():
    right, left = np.nextafter(F(6), F(np.inf)), np.nextafter(F(-6), F(-np.inf))
    points = np.array([(6, 0, 0), (right, 0, 0), (-6, 0, 0), (left, 0, 0), (0, 6, 0), (0, np.nextafter(F(6), F(np.inf)), 0), (0, -6, 0),
                       (0, np.nextafter(F(-6), F(-np.inf)), 0)], F)
    got = _wall(points, normals=None)
    assert got["views"].tolist() == [1, 0, 1, 0, 1, 0, 1, 0], "u = 0.5 and u = W - 0.5 are inside, one ulp beyond is outside; the same for rows"
    # u = 3.5: x0 = min(3, 2) = 2, fa = 1: column 3; v = 2: rows 1 and 2 halfway: (70 + 110) / 2; u = 0.5: column 0: (40 + 80) / 2
    # v = 0.5: row 0 between columns 1 and 2: 15; v = 3.5: row 3 between columns 1 and 2: (0 + 51) / 2
    assert got["measured"][[0, 2, 4, 6]].tolist() == [_degrees(90.0), _degrees(60.0), _degrees(15.0), _degrees(25.5)]
    assert P.bits(got["measured"][[1, 3, 5, 7]]).tolist() == [NAN] * 4 and got["best_camera"][[1, 3]].tolist() == [-1, -1]
    assert got["outside"] == 4 and got["behind"] == 0 and got["facing"] == 0 and got["hidden"] == 0


def test_cos_equal_to_min_cos_is_inside():
    # (3, 0, 0) from (0, 0, 4): d = (3, 0, -4), dist = 5, cos = 4 / 5, and div(4, 5) is the double 0.8
    point = [(3, 0, 0)]
    assert _wall(point, min_cos=0.8)["views"].tolist() == [1]
    assert _wall(point, min_cos=float(np.nextafter(0.8, 1.0)))["views"].tolist() == [0]
    assert _wall(point, normals=-UP, min_cos=0.8)["views"].tolist() == [0] and _wall(point, normals=-UP, min_cos=0.8)["facing"] == 1
    assert _wall(point, normals=-UP, min_cos=0.8, two_sided=True)["views"].tolist() == [1]
    assert _wall(point, normals=2.0 * UP, min_cos=0.8)["views"].tolist() == [1], "the normal's length divides out: 4 * 2 / (5 * 2)"


def test_behind_the_camera_at_the_eye_and_near():
    got = _wall([(0, 0, 5), (0, 0, 4), (0, 0, 3), (0, 0, 0)], normals=None)
    assert got["views"].tolist() == [0, 0, 1, 1] and got["behind"] == 2, "z = -1 and z = 0 are not in front"
    assert got["counts"].tolist() == [2, 4, 1, 2, 2, 0]
    got = _wall([(0, 0, 3), (0, 0, 2), (0, 0, 0)], normals=None, near=2.0)
    assert got["views"].tolist() == [0, 1, 1], "z = 1 is nearer than near; z = near is inside"


def test_equal_weights_keep_the_lower_camera_and_spread_is_the_disagreement():
    other = (255 - P.WALL_IMAGE.astype(np.int64)).astype(np.uint8)
    two = [P.down_camera(), P.down_camera()]
    got = _wall([(-2, 2, 0), (0, 0, 0)], cameras=two, images=np.stack([P.WALL_IMAGE, other]))
    assert got["views"].tolist() == [2, 2] and got["best_camera"].tolist() == [0, 0]
    t0, t1 = 10.0 + (50.0 / 255.0) * 30.0, 10.0 + (205.0 / 255.0) * 30.0
    w = (4.0 / math.sqrt(24.0)) / 24.0
    assert got["measured"][0] == F((w * t0 + w * t1) / (w + w)) and got["spread"][0] == F(t1 - t0)
    # a camera twice as far: a quarter of the weight; whichever comes first, the nearer one is the best
    far = P.down_camera(z=8.0, fx=2.0, fy=2.0)
    for order, best in (([far, P.down_camera()], 1), ([P.down_camera(), far], 0)):
        got = _wall([(0, 0, 0)], cameras=order, images=np.stack([P.WALL_IMAGE, P.WALL_IMAGE]))
        assert got["best_camera"].tolist() == [best] and got["views"].tolist() == [2] and got["spread"].tolist() == [0.0]
        assert got["measured"].tolist() == [_degrees(75.0)], "both see s = 75: u = 2 + 2 * 0 / 8"


def test_back_wall_hidden_from_one_camera_and_seen_from_the_other():
    pos, temp, tri = P.two_walls()
    cameras = np.stack([P.down_camera(), P.down_camera(x=5.0)])
    images = np.stack([np.full((4, 4), 100, np.uint8), np.full((4, 4), 200, np.uint8)])
    points = np.array([(0, 0, -2), (0, 0, 0), (3, 0, -2)], F)
    got = P.project(pos, temp, tri, points, np.tile(UP, (3, 1)), cameras, images, 0.0, 51.0)
    # (0, 0, -2): camera 0 looks through the front wall (t = 4 / 6), camera 1 past its edge (x = 5 / 3 at z = 0)
    assert got["views"].tolist() == [1, 2, 2] and got["best_camera"].tolist() == [1, 0, 1]
    assert got["measured"][0] == F(40.0) and got["spread"][0] == 0.0 and got["hidden"] == 1 and got["counts"].tolist() == [3, 3, 2, 6, 5, 0]
    assert got["spread"][1] == F(20.0)
    nothing = P.project(pos[:0], temp[:0], tri, points, None, cameras, images, 0.0, 51.0)
    assert nothing["views"].tolist() == [2, 2, 2] and nothing["hidden"] == 0, "without a usable face nothing hides anything"
    assert P.project(pos, temp, tri[:0], points, None, cameras, images, 0.0, 51.0)["views"].tolist() == [2, 2, 2]


def test_unusable_points_and_cameras_and_calls_without_either():
    points = np.array([(0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0)], F)
    normals = np.tile(UP, (6, 1))
    normals[3], normals[4, 0] = 0.0, np.nan
    bad_fx, bad_pose, negative = P.down_camera(fx=0.0), P.down_camera(x=np.inf), P.down_camera(fy=-1.0)
    cameras = np.stack([bad_fx, P.down_camera(), bad_pose, negative])
    pos, tri = P.WALL
    temp = np.full(4, 20.0, F)
    images = np.stack([P.WALL_IMAGE] * 4)
    got = P.project(pos, temp, tri, points, normals, cameras, images, 10.0, 40.0, point_temperature=np.full(6, 30.0, F))
    assert P.usable_cameras(cameras).tolist() == [False, True, False, False] and P.usable_points(points, normals).tolist() == [True, False, False, False, False, True]
    assert got["views"].tolist() == [1, 0, 0, 0, 0, 1] and got["best_camera"].tolist() == [1, -1, -1, -1, -1, 1]
    assert got["counts"].tolist() == [2, 2, 1, 2, 2, 0] and got["pairs"] == 2
    for name in ("measured", "spread", "difference"):
        assert P.bits(got[name][1:5]).tolist() == [NAN] * 4, name
    assert P.project(pos, temp, tri, points, None, cameras, images, 10.0, 40.0)["views"].tolist() == [1, 0, 0, 1, 1, 1], "without normals only positions count"
    none = P.project(pos, temp, tri, points, normals, cameras[:0], images[:0], 10.0, 40.0, point_temperature=np.full(6, 30.0, F))
    assert none["counts"].tolist() == [0, 2, 0, 0, 0, 0] and none["views"].tolist() == [0] * 6 and P.bits(none["difference"]).tolist() == [NAN] * 6
    assert none["stats"].tolist() == [0.0, 0.0, math.inf, -math.inf, 0.0, -math.inf, 0.0, 0.0]
    empty = P.project(pos, temp, tri, points[:0], normals[:0], cameras, images, 10.0, 40.0)
    assert empty["counts"].tolist() == [0, 0, 1, 0, 0, 0] and empty["measured"].shape == (0,) and empty["difference"] is None
    own = P.project(pos, temp, tri, points[[0, 5]], None, cameras, images, 10.0, 40.0, point_temperature=np.array([np.nan, 30.0], F))
    assert P.bits(own["difference"][:1]).tolist() == [NAN] and own["difference"][1] == F(30.0 - D(own["measured"][1]))


def test_statistics_are_the_ordered_sums_in_blocks_of_256():
    rng = np.random.default_rng(5)
    points = np.concatenate([rng.uniform(-5.0, 5.0, (600, 2)), np.zeros((600, 1))], axis=1).astype(F)
    points[[3, 300, 599], 0] = 50.0  # outside the image: unseen
    cameras = np.stack([P.down_camera(), P.down_camera(x=0.5, z=5.0)])
    images = rng.integers(0, 256, (2, 4, 4)).astype(np.uint8)
    got = _wall(points, cameras=cameras, images=images, point_temperature=rng.uniform(10.0, 40.0, 600).astype(F))
    assert got["views"][[3, 300, 599]].tolist() == [0, 0, 0] and int(got["counts"][0]) == 597 and (got["views"][:3] == 2).all()

    def blocks(x):
        x = np.where(np.isnan(x), 0.0, x.astype(D))
        return sum((sum(b.tolist(), 0.0) for b in (x[:256], x[256:512], x[512:])), 0.0)

    d, s, m = got["difference"], got["spread"], got["measured"]
    assert got["stats"].tolist() == [blocks(d), blocks((np.where(np.isnan(d), 0, d).astype(D) ** 2).astype(D)), float(np.nanmin(d)), float(np.nanmax(d)),
                                     blocks(s), float(np.nanmax(s)), blocks(m), 0.0]
    assert P.stats_of(None, None, None).tolist() == [0.0, 0.0, math.inf, -math.inf, 0.0, -math.inf, 0.0, 0.0]


def test_random_scene_meets_its_conditions():
    """what the device test relies on: the reference alone shows that every clause works on the scene"""
    scene, out = P.random_reference()
    P.conditions(out)
    count = len(scene["points"])
    assert count % 64 == 37 and count > 512 and len(scene["cameras"]) == 6 and scene["images"].shape == (6, 24, 32)
    assert 1000 <= len(scene["triangles"]) <= 3000 and out["counts"][1] == count - 4 and out["counts"][2] == 6
    assert (out["views"] >= 3).sum() > 20 and (out["views"] == 0).sum() > 20 and len(set(out["best_camera"].tolist())) == 7
    assert (out["spread"][out["views"] > 1] > 0).all(), "random bytes: two views never agree"


# ---- the declarations and the refusals ---------------------------------------------------------------------------------------------------

NAMES = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "bvh", "bvh_bytes", "points", "normals", "point_temperature",
         "num_points", "cameras", "images", "num_cameras", "params", "measured", "views", "best_camera", "spread", "difference", "counts",
         "stats", "stream")


def test_entry_structs_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = re.search(r"\bint tn_mesh_project\(([^;]*)\);", header).group(1)
    assert [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")] == list(NAMES)
    assert header.index("int tn_mesh_closest(") < header.index("int tn_mesh_project("), "behind the closest-point query"
    result, arguments = _hip.SIGNATURES["tn_mesh_project"]
    assert result == ctypes.c_int and len(arguments) == len(NAMES) and arguments[14] == ctypes.POINTER(_hip.tn_project_params)
    assert arguments[3] == arguments[4] == arguments[10] == arguments[13] == ctypes.c_int64 and arguments[6] == ctypes.c_size_t
    camera, params = _hip.tn_project_camera, _hip.tn_project_params
    assert ctypes.sizeof(camera) == 64 and [f[0] for f in camera._fields_] == ["c2w", "fx", "fy", "cx", "cy"]
    assert [getattr(camera, k).offset for k in ("c2w", "fx", "fy", "cx", "cy")] == [0, 48, 52, 56, 60]
    assert ctypes.sizeof(params) == 48 and [f[0] for f in params._fields_] == ["t_lo", "t_hi", "min_cos", "near", "width", "height", "two_sided", "reserved"]
    assert [getattr(params, f[0]).offset for f in params._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    body = re.search(r"typedef struct tn_project_params \{([^}]*)\} tn_project_params;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;\[])", body) == [f[0] for f in params._fields_]
    body = re.search(r"typedef struct tn_project_camera \{([^}]*)\} tn_project_camera;", header).group(1)
    assert re.findall(r"\b([a-z_0-9]+)(?=[,;\[])", body) == ["c2w", "fx", "fy", "cx", "cy"]
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert "tn_mesh_closest.hip tn_mesh_project.hip" in makefile and "tn_mesh_bvh.h " in makefile
    text = " ".join(header.split())
    for phrase in ("Why the order is fixed", "the lower index wins a tie", "the hull of the pixel centres", "equality is inside",
                   "w = div(cos, dist2)", "0 <= t <= 1 - 2^-10"):
        assert phrase in text, phrase
    assert camera_records([CameraView(np.arange(12).reshape(3, 4), 13.0, 14.0, 15.0, 16.0, 8, 6)])[0].tolist() == [list(map(float, range(12))) + [13.0, 14.0, 15.0, 16.0]]


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _hip.load()
    limit = (2 ** 31 - 1) // 3
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy, t = 4096, 2000
    blob = mesh_bvh_bytes(t)

    def params(t_lo=10.0, t_hi=40.0, min_cos=0.2, near=0.0, width=32, height=24, two_sided=0):
        return _hip.tn_project_params(t_lo, t_hi, min_cos, near, width, height, two_sided, 0)

    good = dict(zip(NAMES, [dummy, dummy, dummy, 1000, t, dummy, blob - 1, dummy, dummy, dummy, 500, dummy, dummy, 6, params()] + [dummy] * 7 + [None]))

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_project(*[args[k] for k in NAMES])

    assert call() == -4 and call(bvh_bytes=0) == -4  # TN_ERR_WORKSPACE: the last refusal, so everything before it passed
    for k in ("positions", "temperature", "triangles", "bvh", "points", "point_temperature", "cameras", "images", "params"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    for k in ("normals", "measured", "views", "best_camera", "spread", "difference", "counts", "stats"):
        assert call(**{k: None}) == -4, f"{k} may be absent"
    assert call(point_temperature=None, difference=None) == -4 and call(**{k: None for k in NAMES[15:22]}) == -4, "every output absent"
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert call(num_points=-1) == -2 and call(num_points=limit + 1) == -2 and call(num_cameras=-1) == -2 and call(num_cameras=2 ** 31) == -2
    for side in (-1, 0, 1, 16385):
        assert call(params=params(width=side)) == -2 and call(params=params(height=side)) == -2, side  # TN_ERR_SHAPE
    assert call(params=params(width=2, height=2)) == -4 and call(params=params(width=16384, height=16384)) == -4
    for bad in (dict(min_cos=0.0), dict(min_cos=-0.5), dict(min_cos=float(np.nextafter(1.0, 2.0))), dict(min_cos=math.nan), dict(near=-1e-300),
                dict(near=math.nan), dict(t_lo=math.nan), dict(t_lo=math.inf), dict(t_hi=-math.inf), dict(t_hi=math.nan)):
        assert call(params=params(**bad)) == -3, bad  # TN_ERR_UNSUPPORTED
    for fine in (dict(min_cos=1.0), dict(min_cos=1e-300), dict(near=math.inf), dict(t_lo=40.0, t_hi=10.0), dict(t_lo=5.0, t_hi=5.0), dict(two_sided=7)):
        assert call(params=params(**fine)) == -4, fine
    for k in ("positions", "temperature", "triangles", "points", "normals", "point_temperature", "cameras", "measured", "views", "best_camera",
              "spread", "difference"):
        assert call(**{k: dummy + 2}) == -2, k
    assert call(counts=dummy + 4) == -2 and call(stats=dummy + 4) == -2 and call(bvh=dummy + 32) == -2
    assert call(images=dummy + 1) == -4, "bytes need no alignment"
    bad = params(min_cos=0.0)
    assert call(params=bad, bvh=None) == -1 and call(params=bad, num_points=-1) == -2 and call(params=bad, points=None) == -3 and \
        call(points=None, views=dummy + 2) == -1 and call(views=dummy + 2, bvh_bytes=0) == -2, "in the siblings' order"
    assert call(num_points=0, points=None, normals=None, point_temperature=None) == -4, "without a point the three input arrays may be absent"
    assert call(num_cameras=0, cameras=None, images=None) == -4, "without a camera neither records nor photos are needed"
    assert call(num_vertices=0, positions=None, temperature=None) == -4, "a mesh without vertices needs no arrays"
    assert call(num_triangles=0, triangles=None, positions=None, temperature=None, bvh_bytes=63) == -4 and mesh_bvh_bytes(0) == 64


def _host_mesh():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    return mesh, MeshBVH(torch.zeros(128, dtype=torch.uint8), 3, 1, mesh)


def test_python_layer_refuses_before_it_reaches_a_kernel():
    mesh, bvh = _host_mesh()
    points, images = torch.zeros((4, 3)), torch.zeros((2, 6, 8), dtype=torch.uint8)
    view = CameraView(np.eye(4)[:3], 10.0, 10.0, 4.0, 3.0, 8, 6)
    views = [view, view]
    table = torch.zeros((2, 16))
    for kw, words in ((dict(min_cos=0.0), "min_cos"), (dict(min_cos=1.5), "min_cos"), (dict(min_cos=math.nan), "min_cos"), (dict(near=-1.0), "near"),
                      (dict(near=math.nan), "near")):
        for call in (lambda: project_images(bvh, points, None, views, images, (10.0, 40.0), **kw),
                     lambda: project_images_into(bvh, points, None, table, images, (10.0, 40.0), **kw),
                     lambda: mesh_measurement(mesh, bvh, views, images, (10.0, 40.0), **kw)):
            with pytest.raises(ValueError, match=words):
                call()
    for bounds in ((10.0, math.inf), (math.nan, 40.0), (10.0,), None, "ab"):
        with pytest.raises(ValueError, match="temperature_bounds"):
            project_images(bvh, points, None, views, images, bounds)
    for call in (lambda: project_images(bvh, points, None, views, images, (10.0, 40.0)),
                 lambda: project_images_into(bvh, points, None, table, images, (10.0, 40.0)),
                 lambda: mesh_measurement(mesh, bvh, views, images, (10.0, 40.0))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="share one image size"):
        project_images(bvh, points, None, [view, dataclasses.replace(view, width=9)], images, (10.0, 40.0))
    with pytest.raises(ValueError, match="2 .. 16384 pixels"):
        camera_records([dataclasses.replace(view, width=1)])
    with pytest.raises(ValueError, match="fx and fy must be positive"):
        camera_records([dataclasses.replace(view, fx=0.0)])
    with pytest.raises(ValueError, match="no triangles"):
        mesh_measurement(ThermalMesh(mesh.positions, mesh.colors, mesh.temperature), bvh, views, images, (10.0, 40.0))
    records, width, height = camera_records([])
    assert records.shape == (0, 16) and (width, height) == (0, 0)
    fields = {f.name for f in dataclasses.fields(ProjectedTemperatures)}
    assert {"measured", "views", "best_camera", "spread", "difference", "seen", "usable_points", "usable_cameras", "tested_pairs", "accepted_pairs",
            "stack_limit_pairs", "seen_share", "mean_views", "mean_spread", "max_spread", "mean_difference", "rms_difference", "min_difference",
            "max_difference"} <= fields
    assert {"projected", "measured", "residual", "seen", "seen_share", "mean_difference", "rms_difference", "min_difference", "max_difference",
            "mean_spread", "max_spread"} <= {f.name for f in dataclasses.fields(MeshMeasurement)}
    assert "unusable for ``thermal_regions`` and the rasteriser" in " ".join(mesh_measurement.__doc__.split())


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_command_line_arguments(capsys):
    tool = _tool()
    base = ["mesh.ply", "--transforms", "data/transforms.json", "--output", "measured.ply"]
    args = tool.parse(base)
    assert (str(args.mesh), str(args.transforms), args.frames, str(args.output), args.residual, args.report, args.temperature_bounds, args.min_cos,
            args.two_sided, args.min_change, args.length_scale) == ("mesh.ply", "data/transforms.json", "all", "measured.ply", None, None, None, 0.2,
                                                                    False, None, 1.0)
    args = tool.parse(base + ["--frames", "eval", "--residual", "r.ply", "--report", "p.json", "--temperature-bounds", "41.5", "12", "--min-cos", "0.5",
                              "--two-sided", "--min-change", "2.0", "--length-scale", "0.37"])
    assert (args.frames, str(args.residual), str(args.report), args.temperature_bounds, args.min_cos, args.two_sided, args.min_change, args.length_scale) == \
        ("eval", "r.ply", "p.json", [41.5, 12.0], 0.5, True, 2.0, 0.37)
    for bad, flag in ((["--min-cos", "0"], "--min-cos"), (["--min-cos", "1.5"], "--min-cos"), (["--min-cos", "nan"], "--min-cos"),
                      (["--temperature-bounds", "12", "41.5"], "--temperature-bounds"), (["--temperature-bounds", "inf", "0"], "--temperature-bounds"),
                      (["--min-change", "0"], "--min-change"), (["--min-change", "inf"], "--min-change"), (["--length-scale", "0"], "--length-scale"),
                      (["--frames", "some"], "--frames")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    for missing in ("--transforms", "--output"):
        k = base.index(missing)
        with pytest.raises(SystemExit):
            tool.parse(base[:k] + base[k + 2:])
        assert missing in capsys.readouterr().err
    for flag in ("--transforms", "--frames", "--output", "--residual", "--report", "--temperature-bounds", "--min-cos", "--two-sided", "--min-change",
                 "--length-scale"):
        assert flag in tool.__doc__, flag
    assert "Lens distortion is ignored" in tool.__doc__
    meta = {"frames": [{"file_path": "images/frame_train_00001.jpg", "thermal_file_path": "thermal/frame_train_00001.PNG"},
                       {"file_path": "images/frame_eval_00002.jpg", "thermal_file_path": "thermal/frame_eval_00002.PNG"},
                       {"file_path": "images/frame_train_00003.jpg", "thermal_file_path": "thermal/frame_train_00003.PNG"}]}
    assert tool.select_frames(meta, "all") == [0, 1, 2] and tool.select_frames(meta, "train") == [0, 2] and tool.select_frames(meta, "eval") == [1]
    del meta["frames"][2]["thermal_file_path"]
    with pytest.raises(ValueError, match="thermal_file_path"):
        tool.select_frames(meta, "train")
    with pytest.raises(ValueError, match="no frames"):
        tool.select_frames({}, "all")
    with pytest.raises(ValueError, match="none of the 1 frames"):
        tool.select_frames({"frames": meta["frames"][:1]}, "eval")


def _hand_made(seen=3):
    projected = SimpleNamespace(usable_points=4, usable_cameras=2, tested_pairs=7, accepted_pairs=5 if seen else 0, stack_limit_pairs=0)
    if not seen:
        return SimpleNamespace(projected=projected, seen=0, seen_share=0.0, mean_views=0.0, mean_difference=math.nan, rms_difference=math.nan,
                               min_difference=math.inf, max_difference=-math.inf, mean_spread=math.nan, max_spread=-math.inf)
    return SimpleNamespace(projected=projected, seen=3, seen_share=0.75, mean_views=1.25, mean_difference=-1.5, rms_difference=2.0,
                           min_difference=-3.0, max_difference=0.5, mean_spread=0.25, max_spread=1.0)


def test_report_schema_with_a_hand_made_result():
    tool = _tool()
    report = tool.build_report(_hand_made(), 4, 2, 2, 32, 24, (12.0, 41.5), 0.2, False, source="mesh.ply", transforms="t.json")
    assert json.loads(json.dumps(report)) == report, "plain JSON: no numpy scalars, no infinities"
    assert set(report) == {"mesh", "transforms", "frames", "length_scale", "temperature_bounds", "min_cos", "two_sided", "image", "counts",
                           "seen_share", "mean_views", "residual", "spread"}
    assert report["counts"] == {"vertices": 4, "faces": 2, "frames": 2, "usable_vertices": 4, "usable_cameras": 2, "seen_vertices": 3,
                                "tested_pairs": 7, "accepted_pairs": 5, "stack_limit_pairs": 0}
    assert report["residual"] == {"mean": -1.5, "rms": 2.0, "min": -3.0, "max": 0.5} and report["spread"] == {"mean": 0.25, "max": 1.0}
    assert report["seen_share"] == 0.75 and report["mean_views"] == 1.25 and report["temperature_bounds"] == [12.0, 41.5]
    assert report["image"] == {"width": 32, "height": 24} and report["frames"] == "all"
    line = tool.summary_line(report)
    assert "\n" not in line and line == ("mesh.ply under 2 photos: 4 vertices, 3 seen (75.0 %), 1.25 views each, model - photos mean -1.50 C rms 2.00 "
                                         "min -3.00 max +0.50, spread mean 0.25 max 1.00")
    table = np.zeros(2, REGION_DTYPE)
    table["area"], table["faces"], table["mean_temperature"] = [2.0, 0.5], [5, 1], [3.0, 2.5]
    table["min_temperature"], table["max_temperature"], table["centroid"] = [2.25, 2.5], [4.0, 2.5], [[1, 2, 3], [4, 5, 6]]
    above = ThermalRegions(table, np.array([1, 0]), torch.zeros(2, dtype=torch.int32), 10.0, 2.5, 2, 6, 8, (2.0, math.inf))
    below = ThermalRegions(table[:0], np.zeros(0, np.int64), torch.zeros(2, dtype=torch.int32), 10.0, 0.0, 0, 0, 8, (-math.inf, -2.0))
    report = tool.build_report(_hand_made(), 4, 2, 2, 32, 24, (12.0, 41.5), 0.2, True, 2.0, above, below, 2.0, "mesh.ply", "t.json", "train")
    assert json.loads(json.dumps(report)) == report and report["min_change"] == 2.0 and report["two_sided"] is True and report["frames"] == "train"
    assert report["compared_area"] == 40.0 and report["model_below"] == {"area": 0.0, "share": 0.0, "regions": []}
    assert report["model_above"] == {"area": 10.0, "share": 0.25, "regions": [
        {"region": 1, "faces": 5, "area": 8.0, "mean_difference": 3.0, "largest_change": 4.0, "centroid": [2.0, 4.0, 6.0]},
        {"region": 0, "faces": 1, "area": 2.0, "mean_difference": 2.5, "largest_change": 2.5, "centroid": [8.0, 10.0, 12.0]}]}
    assert tool.region_lines(report) == ["model_above 0: area 8, 5 faces, mean +3.00 C, largest +4.00 C, centroid (2, 4, 6)",
                                         "model_above 1: area 2, 1 faces, mean +2.50 C, largest +2.50 C, centroid (8, 10, 12)"]
    empty = tool.build_report(_hand_made(0), 4, 2, 2, 32, 24, (12.0, 41.5), 0.2, False, source="mesh.ply", transforms="t.json")
    assert json.loads(json.dumps(empty)) == empty and empty["residual"] == {"mean": None, "rms": None, "min": None, "max": None}
    assert empty["spread"] == {"mean": None, "max": None} and "none seen" in tool.summary_line(empty)
