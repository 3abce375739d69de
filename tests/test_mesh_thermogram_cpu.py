"""The yardstick of the mesh rasteriser (tests/mesh_raster_reference.py) checked on its own — the literal cases, watertightness, the
winner's independence of the face order, that its ordered sum is told apart from the other two on the scene the device tests use —
and the host side of the feature: the declarations, the struct, the refusals of the entry, the arithmetic of ``fit_view``, the command
line and its report.  No GPU."""
from __future__ import annotations

import ctypes
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_raster_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (RasterView, ThermalMesh, Thermogram, fit_view, mesh_raster_small_box, mesh_rasterize_into,
                                    mesh_rasterize_workspace_bytes, mesh_thermogram, place_view, view_axes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_thermogram_tool", os.path.join(ROOT, "tools", "mesh_thermogram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the reference against its literal cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_yardstick_on_the_literal_cases(name):
    case = R.LITERAL[name]
    got = R.rasterize(*R.literal_arrays(case), case["view"])
    assert R.literal_mismatch(got, case["want"]) is None, R.literal_mismatch(got, case["want"])
    assert got["pixel_face"].dtype == np.int32 and got["pixel_depth"].dtype == F and got["pixel_temperature"].dtype == F
    assert got["counts"].dtype == np.int64 and got["stats"].dtype == D
    empty = got["pixel_face"] < 0
    assert (R.bits(got["pixel_depth"])[empty] == R.NAN_BITS).all() and (R.bits(got["pixel_temperature"])[empty] == R.NAN_BITS).all()


def test_literal_cases_are_the_ones_the_feature_is_defined_by():
    w = {k: R.LITERAL[k]["want"] for k in R.LITERAL}
    assert w["top_left_rule"]["pixel_face"][0] == [0, 0, 0, 0, -1] and w["top_left_rule"]["counts"] == [10, 1, 1]
    assert w["top_left_rule_other_winding"]["pixel_face"] == w["top_left_rule"]["pixel_face"]
    assert w["seen_from_behind_and_culled"]["counts"] == [0, 0, 1] and w["seen_from_behind_and_culled"]["stats"][1:] == [math.inf, -math.inf]
    assert [row[k] for k, row in enumerate(w["shared_diagonal"]["pixel_face"])] == [0, 0, 0, 0], "the diagonal goes to the lower face"
    assert w["nearer_face_and_equal_depth"]["pixel_face"] == [[1, 1], [1, 1]]
    assert w["slab_cuts_a_tilted_face"]["counts"][0] == 8


def test_orders_and_sums_of_the_yardstick():
    values = np.array([-math.inf, -1.0, -0.0, 0.0, 1e-40, 1.0, math.inf], F)
    assert (np.diff(R.ord32(values).astype(np.int64)) > 0).all(), "the numbers' order, -0.0 below +0.0"
    assert R.sum2([]) == 0.0 and math.copysign(1.0, R.sum2([-0.0])) == 1.0
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, 257).tolist()
    assert R.sum2(x[:256]) == sum(x[:256], 0.0) and R.sum2(x) == sum(x[:256], 0.0) + x[256]
    # rint rounds half to even; a vertex exactly on the fixed-point limit is rasterable, one beyond is not
    X, Y, z, ok = R.vertices(np.array([(0.001953125, 0.005859375, 1), (2.0 ** 21, -(2.0 ** 21), 0), (2.0 ** 21 + 0.25, 0, 0), (np.nan, 0, 0),
                                       (0, 0, np.inf)], F), R.view(4, 4))
    assert X[:2].tolist() == [0, 2 ** 29] and Y[:2].tolist() == [2, -(2 ** 29)] and ok.tolist() == [True, True, False, False, False]


# ---- the reference's own invariants -----------------------------------------------------------------------------------------------------

def test_a_lattice_of_quads_is_watertight():
    mesh = R.quad_lattice(12, 1.3125, 2.171875, 7, jitter=0.5)
    got = R.rasterize(*mesh, R.view(30, 30))
    assert int(got["samples"].sum()) == int(got["counts"][0]), "no pixel is covered by two faces of one sheet"
    x0, x1 = 1.3125, 1.3125 + 12 * 2.171875
    j, i = np.mgrid[0:30, 0:30]
    inner = (i + 0.5 > x0) & (i + 0.5 < x1) & (j + 0.5 > x0) & (j + 0.5 < x1)
    assert ((got["pixel_face"] >= 0) == inner).all() and inner.sum() == 26 * 26
    assert (np.bincount(got["pixel_face"][inner], minlength=288) == got["samples"]).all() and got["ties"] == 0
    # either winding of any of its faces: the same coverage
    pos, temp, col, tri = mesh
    flipped = tri.copy()
    flipped[::3] = flipped[::3][:, [0, 2, 1]]
    again = R.rasterize(pos, temp, col, flipped, R.view(30, 30))
    for name in ("pixel_face", "pixel_depth", "pixel_temperature", "pixel_colors"):
        assert again[name].tobytes() == got[name].tobytes(), name
    culled = R.rasterize(pos, temp, col, flipped, R.view(30, 30, cull=1))
    assert culled["counts"][1] == 96 and 0 < culled["counts"][0] < got["counts"][0]


def test_the_big_scene_has_no_ties_and_does_not_depend_on_the_order_of_its_faces():
    pos, temp, col, tri = R.big_scene()
    view = R.view(R.BIG_SIDE, R.BIG_SIDE)
    got = R.rasterize(pos, temp, col, tri, view)
    assert len(tri) == 2 * 182 * 182 + 338 >= 65537 and got["ties"] == 0 and got["counts"].tolist() == [90000, len(tri), len(tri)]
    back = R.rasterize(pos, temp, col, tri[::-1].copy(), view)
    for name in ("pixel_depth", "pixel_temperature", "pixel_colors"):
        assert back[name].tobytes() == got[name].tobytes(), name
    assert (back["pixel_face"] == len(tri) - 1 - got["pixel_face"]).all() and back["stats"].tobytes() == got["stats"].tobytes()
    # the coarse faces are spread through the list, have boxes beyond the small / large threshold and both win and lose pixels
    coarse = np.flatnonzero(np.arange(len(tri)) % 191 == 190)[:338]
    X, Y = R.faces(pos, temp, tri, view)[3:5]
    spans = np.maximum(X.max(axis=1) - X.min(axis=1), Y.max(axis=1) - Y.min(axis=1)) / 256.0
    assert (spans[coarse] > 12).all() and (np.delete(spans, coarse) < 4).all() and len(coarse) > 256
    shown = np.isin(got["pixel_face"], coarse).mean()
    assert 0.1 < shown < 0.9, shown
    # SUM2 is told apart from the sequential and from numpy's pairwise sum
    t = got["pixel_temperature"].astype(D).reshape(-1)
    sequential = 0.0
    for x in t.tolist():
        sequential += x
    print(f"300 x 300 pixels: SUM2 {got['stats'][0].hex()}, sequential {sequential.hex()}, numpy.sum {float(np.sum(t)).hex()}")
    assert got["stats"][0] not in (sequential, float(np.sum(t))), "the scene cannot tell SUM2 from another order: choose another seed"


def test_slab_cull_and_unusable_faces_in_the_yardstick():
    mesh = R.tetrahedron()
    both, front = R.rasterize(*mesh, R.view(16, 16)), R.rasterize(*mesh, R.view(16, 16, cull=1))
    assert both["counts"].tolist()[1:] == [4, 4] and 0 < front["counts"][1] < 4 and (both["pixel_face"] == front["pixel_face"]).all()
    assert R.rasterize(*mesh, R.view(16, 16, near=3.0, far=2.0))["counts"].tolist() == [0, 4, 4], "near > far keeps nothing"
    pos, temp, col, tri = mesh
    bad = np.array([(0, 1, 4), (0, -1, 2), (1, 1, 2), (0, 1, 2)], np.int32)
    got = R.rasterize(pos, temp, col, bad, R.view(16, 16))
    assert got["counts"].tolist()[1:] == [1, 1] and set(np.unique(got["pixel_face"]).tolist()) == {-1, 3}
    hot = temp.copy()
    hot[2] = np.nan
    assert R.rasterize(pos, hot, col, tri, R.view(16, 16))["counts"].tolist()[1:] == [1, 1], "a NaN temperature spoils its three faces"
    assert R.rasterize(pos[:0], temp[:0], None, tri, R.view(3, 2))["counts"].tolist() == [0, 0, 0]


# ---- the declarations ------------------------------------------------------------------------------------------------------------------

NAMES = ("positions", "temperature", "colors", "triangles", "num_vertices", "num_triangles", "view", "pixel_face", "pixel_depth",
         "pixel_temperature", "pixel_colors", "counts", "stats", "workspace", "workspace_bytes", "stream")


def test_entry_struct_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bsize_t tn_mesh_rasterize_workspace_bytes\(int64_t num_triangles, int32_t width, int32_t height\);", header)
    assert re.search(r"\bint32_t tn_mesh_raster_small_box\(void\);", header)
    declared = re.search(r"\bint tn_mesh_rasterize\(([^;]*)\);", header).group(1)
    assert [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")] == list(NAMES)
    assert len(_hip.SIGNATURES["tn_mesh_rasterize"][1]) == len(NAMES) == 16
    assert _hip.SIGNATURES["tn_mesh_rasterize"][1][6] == ctypes.POINTER(_hip.tn_raster_view)
    assert _hip.SIGNATURES["tn_mesh_rasterize_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32])
    assert _hip.SIGNATURES["tn_mesh_raster_small_box"] == (ctypes.c_int32, [])
    assert "tn_mesh_raster.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    offsets = {"origin": 0, "right": 24, "down": 48, "forward": 72, "pixel_size": 96, "near": 104, "far": 112, "width": 120, "height": 124,
               "cull": 128, "reserved": 132}
    assert ctypes.sizeof(_hip.tn_raster_view) == 136
    for name, offset in offsets.items():
        assert getattr(_hip.tn_raster_view, name).offset == offset, name
    assert [f[0] for f in _hip.tn_raster_view._fields_] == list(offsets)
    body = re.search(r"typedef struct tn_raster_view \{([^}]*)\} tn_raster_view;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?:\[\d\])?(?=[,;])", body) == list(offsets)
    fields = {f.name for f in RasterView.__dataclass_fields__.values()}
    assert fields == set(offsets) - {"reserved"}


def _view(**change):
    """the struct of an 11 x 6 view along +z with some fields changed (``cull`` and ``reserved`` as raw numbers)"""
    reserved, cull = change.pop("reserved", 0), change.pop("cull", 0)
    fields = dict(origin=(0.0, 0.0, 0.0), right=(1.0, 0.0, 0.0), down=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0), pixel_size=1.0, width=11,
                  height=6, near=-math.inf, far=math.inf)
    fields.update(change)
    struct = RasterView(**fields).struct(reserved)
    struct.cull = cull
    return struct


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _hip.load()
    assert mesh_raster_small_box() == lib.tn_mesh_raster_small_box() >= 1
    t = 2000
    need = mesh_rasterize_workspace_bytes(t, 11, 6)
    limit = (2 ** 31 - 1) // 3
    assert need >= 8 * 66 and need % 8 == 0 and mesh_rasterize_workspace_bytes(limit, 16384, 16384) > 8 * 16384 ** 2
    for bad in ((-1, 11, 6), (limit + 1, 11, 6), (t, 0, 6), (t, 11, 0), (t, 16385, 6), (t, 11, 16385), (t, -3, 6)):
        assert mesh_rasterize_workspace_bytes(*bad) == 0, bad
    assert mesh_rasterize_workspace_bytes(t, 16384, 1) > 0 and mesh_rasterize_workspace_bytes(0, 1, 1) > 0
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy = 4096
    good = dict(zip(NAMES, [dummy, dummy, dummy, dummy, 1000, t, _view(), dummy, dummy, dummy, dummy, dummy, dummy, dummy, need, None]))

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_rasterize(*[args[k] for k in NAMES])

    for k in ("positions", "temperature", "colors", "triangles", "view", "counts", "stats", "workspace"):
        assert call(**{k: None}, workspace_bytes=0) == -1, k  # TN_ERR_NULL
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2  # TN_ERR_SHAPE
    assert call(num_triangles=limit + 1, workspace_bytes=2 ** 60) == -2
    for change in (dict(width=0), dict(width=16385), dict(height=-1), dict(height=16385), dict(pixel_size=0.0), dict(pixel_size=-2.0),
                   dict(pixel_size=math.inf), dict(pixel_size=math.nan), dict(origin=(math.nan, 0.0, 0.0)), dict(right=(1.0, math.inf, 0.0)),
                   dict(down=(0.0, 1.0, math.nan)), dict(forward=(-math.inf, 0.0, 1.0))):
        assert call(view=_view(**change)) == -2, change
    for k in ("positions", "temperature", "triangles", "pixel_face", "pixel_depth", "pixel_temperature"):
        assert call(**{k: dummy + 2}) == -2, k
    for k in ("counts", "stats", "workspace"):
        assert call(**{k: dummy + 4}) == -2, k
    for change in (dict(near=math.nan), dict(far=math.nan), dict(cull=2), dict(cull=-1), dict(reserved=-1), dict(reserved=16385)):
        assert call(view=_view(**change)) == -3, change  # TN_ERR_UNSUPPORTED
    nan_view = _view(near=math.nan)
    assert call(view=nan_view, counts=None) == -1 and call(view=nan_view, num_vertices=-1) == -2 and call(view=nan_view, colors=None) == -3, \
        "in the siblings' order"
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    # what may be absent or unusual, checked up to the workspace's size: every pixel array, infinite bounds, near > far, a threshold
    assert call(pixel_face=None, pixel_depth=None, pixel_temperature=None, pixel_colors=None, colors=None, workspace_bytes=0) == -4
    assert call(view=_view(near=3.0, far=2.0), workspace_bytes=0) == -4 and call(view=_view(reserved=16384, cull=1), workspace_bytes=0) == -4
    assert call(view=_view(width=16384, height=16384), workspace_bytes=need) == -4


# ---- fit_view's host arithmetic ---------------------------------------------------------------------------------------------------------------

def test_view_axes_are_orthonormal_and_right_handed():
    for forward, up in (((0, -1, 0), (0, 0, 1)), ((0, 0, -1), (0, 1, 0)), ((0.3, -0.5, 0.81), (0.1, 0.2, 1.0)), ((5, 0, 0), (0, 1, 3))):
        r, d, f = view_axes(forward, up)
        m = np.stack([r, d, f])
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-15 and np.abs(np.cross(r, d) - f).max() < 1e-15
        assert np.dot(d, np.asarray(up, D)) < 0, "up points up in the image"
        assert np.abs(f - np.asarray(forward, D) / np.linalg.norm(forward)).max() < 1e-16
    r, d, f = view_axes((0, -1, 0), (0, 0, 1))  # looking south with z up: west is to the right
    assert r.tolist() == [-1.0, 0.0, 0.0] and d.tolist() == [0.0, 0.0, -1.0]
    for bad in (((0, 0, 0), (0, 0, 1)), ((0, 0, 1), (0, 0, 0)), ((0, 0, 1), (0, 0, -2)), ((math.nan, 0, 1), (0, 1, 0)), ((0, 1), (0, 1, 0))):
        with pytest.raises(ValueError):
            view_axes(*bad)


def test_place_view_frames_the_extent_with_its_margin_and_refuses_what_does_not_fit():
    axes = view_axes((0, 0, 1), (0, -1, 0))  # right = +x, down = +y
    assert axes[0].tolist() == [1.0, 0.0, 0.0] and axes[1].tolist() == [0.0, 1.0, 0.0]
    v = place_view(axes, (1.0, 2.0, 5.0), (11.0, 6.5, 9.0), pixel_size=0.5)
    assert (v.width, v.height, v.pixel_size) == (20 + 4, 9 + 4, 0.5) and v.origin == (0.0, 1.0, 5.0)
    assert (v.near, v.far, v.cull) == (-math.inf, math.inf, False) and v.forward == (0.0, 0.0, 1.0)
    v = place_view(axes, (1.0, 2.0, 5.0), (11.0, 6.5, 9.0), width=104, margin_pixels=2, near=0.5, far=2.0, cull=True)
    assert (v.width, v.height, v.pixel_size) == (104, 45 + 4, 0.1) and (v.near, v.far, v.cull) == (0.5, 2.0, True)
    assert np.allclose(v.origin, (0.8, 1.8, 5.0), atol=1e-12)
    v = place_view(axes, (1.0, 2.0, 5.0), (1.0, 2.0, 5.0), pixel_size=1.0, margin_pixels=0)
    assert (v.width, v.height) == (1, 1), "a mesh without extent still gets a pixel"
    with pytest.raises(ValueError, match=r"pixel size of 0\.000610501 or more fits"):
        place_view(axes, (1.0, 2.0, 5.0), (11.0, 6.5, 9.0), pixel_size=0.0005)  # 10 / (16384 - 4)
    assert place_view(axes, (1.0, 2.0, 5.0), (11.0, 6.5, 9.0), pixel_size=0.000610501 * 1.0001).width <= 16384
    for bad in (dict(), dict(pixel_size=1.0, width=10), dict(pixel_size=0.0), dict(pixel_size=math.inf), dict(width=4), dict(width=16385),
                dict(pixel_size=1.0, margin_pixels=-1)):
        with pytest.raises(ValueError):
            place_view(axes, (1.0, 2.0, 5.0), (11.0, 6.5, 9.0), **bad)
    with pytest.raises(ValueError, match="no finite vertex"):
        place_view(axes, (math.inf,) * 3, (-math.inf,) * 3, pixel_size=1.0)
    with pytest.raises(ValueError, match="no extent"):
        place_view(axes, (1.0, 2.0, 5.0), (1.0, 6.0, 5.0), width=20)


def test_python_layer_refuses_before_it_reaches_a_kernel():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    view = RasterView((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 1.0, 8, 8)
    import dataclasses

    with pytest.raises(ValueError, match="no triangles"):
        mesh_rasterize_into(ThermalMesh(pos, mesh.colors, mesh.temperature), view, counts=None, stats=None)
    for change in (dict(width=0), dict(height=16385), dict(pixel_size=0.0), dict(pixel_size=math.nan), dict(near=math.nan),
                   dict(origin=(0.0, math.inf, 0.0))):
        with pytest.raises(ValueError):
            mesh_thermogram(mesh, dataclasses.replace(view, **change))
    for call in (lambda: mesh_thermogram(mesh, view), lambda: fit_view(pos, (0, 0, 1), (0, 1, 0), pixel_size=1.0),
                 lambda: mesh_rasterize_into(mesh, view, counts=torch.zeros(3, dtype=torch.int64), stats=torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        fit_view(pos, (0, 0, 1), (0, 0, 1), pixel_size=1.0)
    with pytest.raises(ValueError):
        fit_view(pos, (0, 0, 1), (0, 1, 0))


def _hand_made():
    """a 2 x 3 thermogram on the host: one empty pixel"""
    nan = math.nan
    view = RasterView((10.0, 20.0, 30.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.5, 3, 2, 0.25, math.inf, True)
    temperature = torch.tensor([[20.0, 21.5, nan], [30.0, 19.0, 30.0]])
    face = torch.tensor([[4, 4, -1], [7, 2, 9]], dtype=torch.int32)
    depth = torch.tensor([[1.0, 1.5, nan], [2.0, 0.5, 2.5]])
    colors = torch.zeros((2, 3, 3), dtype=torch.uint8)
    return Thermogram(face, depth, temperature, colors, view, 5, 5 * 0.25, 24.1, 19.0, 30.0, 6, 8, (14.0, 33.0))


def test_thermogram_methods_that_need_no_kernel():
    found = _hand_made()
    assert found.world_position(1, 0) == (10.25, 22.0, 30.0 - 0.75) and all(math.isnan(c) for c in found.world_position(0, 2))
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


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def test_command_line_refuses_bad_arguments(capsys):
    tool = _tool()
    base = ["mesh.ply", "--output", "t.png"]
    args = tool.parse(base + ["--view", "-y", "--pixel-size", "0.01"])
    assert (args.forward, args.up, args.pixel_size, args.width) == ((0, -1, 0), (0, 0, 1), 0.01, None)
    assert (args.near, args.far, args.cull_back, args.colors, args.length_scale) == (-math.inf, math.inf, False, "thermal", 1.0)
    assert args.temperatures is None and args.report is None
    args = tool.parse(base + ["--forward", "1", "2", "3", "--up", "0", "0", "1", "--width", "800", "--near", "0.5", "--far", "2", "--cull-back",
                              "--colors", "rgb", "--length-scale", "2.5", "--temperatures", "t.npy", "--report", "t.json"])
    assert (args.forward, args.up, args.width, args.near, args.far) == ((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), 800, 0.5, 2.0)
    assert args.cull_back and args.colors == "rgb" and args.length_scale == 2.5 and str(args.report) == "t.json"
    for view in tool.VIEWS:
        view_axes(*tool.VIEWS[view])  # every named view has a usable up
    size = ["--pixel-size", "1"]
    for bad, flag in (([] + size, "--view"), (["--view", "+x", "--forward", "1", "0", "0", "--up", "0", "0", "1"] + size, "--view"),
                      (["--view", "+x", "--up", "0", "0", "1"] + size, "--up"), (["--forward", "1", "0", "0"] + size, "--up"),
                      (["--view", "up"] + size, "--view"), (["--view", "+x"], "--pixel-size"), (["--view", "+x", "--width", "100"] + size, "--width"),
                      (["--view", "+x", "--pixel-size", "0"], "--pixel-size"), (["--view", "+x", "--pixel-size", "inf"], "--pixel-size"),
                      (["--view", "+x", "--width", "4"], "--width"), (["--view", "+x", "--width", "16385"], "--width"),
                      (["--view", "+x", "--near=nan"] + size, "--near"), (["--view", "+x", "--length-scale", "0"] + size, "--length-scale"),
                      (["--view", "+x", "--colors", "x"] + size, "--colors")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        tool.parse(["mesh.ply", "--view", "+x"] + size)  # no --output
    assert "--output" in capsys.readouterr().err
    for flag in ("--view", "--forward", "--up", "--pixel-size", "--width", "--near", "--far", "--cull-back", "--colors", "--length-scale",
                 "--output", "--temperatures", "--report"):
        assert flag in tool.__doc__, flag


def test_report_schema_and_length_scale_with_a_hand_made_result():
    tool = _tool()
    found = _hand_made()
    arrays = (found.pixel_temperature.numpy(), found.pixel_face.numpy(), found.pixel_depth.numpy())
    plain = tool.build_report(found, *arrays, 12, 10, 1.0, "mesh.ply")
    assert json.loads(json.dumps(plain)) == plain, "plain JSON: no numpy scalars, no infinities"
    assert set(plain) == {"mesh", "length_scale", "view", "counts", "covered_area", "mean_temperature", "min_temperature", "max_temperature",
                          "hottest_pixel", "coldest_pixel"}
    assert plain["view"] == {"origin": [10.0, 20.0, 30.0], "right": [1.0, 0.0, 0.0], "down": [0.0, 0.0, -1.0], "forward": [0.0, 1.0, 0.0],
                             "pixel_size": 0.5, "width": 3, "height": 2, "near": 0.25, "far": None, "cull_back": True}
    assert plain["counts"] == {"vertices": 12, "faces": 10, "usable_faces": 8, "drawn_faces": 6, "pixels": 6, "covered_pixels": 5}
    assert (plain["covered_area"], plain["mean_temperature"], plain["min_temperature"], plain["max_temperature"]) == (1.25, 24.1, 19.0, 30.0)
    assert plain["hottest_pixel"] == {"row": 1, "column": 0, "temperature": 30.0, "face": 7, "position": [10.25, 22.0, 29.25]}, \
        "the first of two equally hot pixels"
    assert plain["coldest_pixel"] == {"row": 1, "column": 1, "temperature": 19.0, "face": 2, "position": [10.75, 20.5, 29.25]}
    scaled = tool.build_report(found, *arrays, 12, 10, 2.0, "mesh.ply")
    assert scaled["length_scale"] == 2.0 and scaled["covered_area"] == 5.0 and scaled["view"]["pixel_size"] == 1.0
    assert scaled["view"]["origin"] == [20.0, 40.0, 60.0] and scaled["view"]["near"] == 0.5 and scaled["view"]["right"] == [1.0, 0.0, 0.0]
    assert scaled["hottest_pixel"]["position"] == [20.5, 44.0, 58.5] and scaled["hottest_pixel"]["temperature"] == 30.0, "degrees are not lengths"
    assert scaled["counts"] == plain["counts"] and scaled["mean_temperature"] == 24.1
    line = tool.summary_line(plain, "mesh.ply")
    assert "\n" not in line and line.startswith("mesh.ply: 3 x 2 pixels of 0.5, 5 covered (area 1.25), 6 of 10 faces drawn, mean 24.10 C")
    import dataclasses

    nothing = dataclasses.replace(found, pixel_temperature=torch.full((2, 3), math.nan), covered=0, covered_area=0.0, mean_temperature=math.nan,
                                  min_temperature=math.inf, max_temperature=-math.inf)
    empty = tool.build_report(nothing, nothing.pixel_temperature.numpy(), arrays[1], arrays[2], 12, 10)
    assert json.loads(json.dumps(empty)) == empty and empty["hottest_pixel"] is None and empty["mean_temperature"] is None
    assert "nothing covered" in tool.summary_line(empty, "mesh.ply")
