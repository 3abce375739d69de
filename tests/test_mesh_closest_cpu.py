"""The yardstick of the closest-point query (tests/mesh_closest_reference.py) checked on its own — literal cases with hand-computed
answers, faces without area, the tie rules, d2 >= b of the face's own box on every scene the device test uses, the monotonicity of b
that the traversal rests on — and the host side of the feature: the declaration, the struct, the refusals of the entry and of the
Python layer, the command line and its report.  No GPU."""
from __future__ import annotations

import ctypes
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
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (ClosestPoints, MeshBVH, MeshDifference, ThermalMesh, mesh_bvh_bytes, mesh_closest, mesh_closest_into,
                                    mesh_difference)
from thermo_nerf_amd.export.regions import REGION_DTYPE, ThermalRegions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
NAN = C.NAN_BITS


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_compare_tool", os.path.join(ROOT, "tools", "mesh_compare.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the reference on literal cases -----------------------------------------------------------------------------------------------------

def test_one_triangle_by_hand():
    """(0,0,0) (4,0,0) (0,4,0) with 10, 20, 30 degrees: a point in each of the seven regions of its plane, on the plane inside, above
    and below it, on a corner, on an edge, on the hypotenuse"""
    got = C.closest(*C.TRIANGLE, C.TRIANGLE_POINTS, point_temperature=np.full(12, 20.0, F))
    assert got["closest_face"].tolist() == [0] * 12
    root2, root3 = float(F(math.sqrt(2.0))), float(F(math.sqrt(3.0)))
    assert got["closest_distance"].tolist() == [0.0, 2.0, 3.0, root2, root2, root3, 2.0, 2.0, root2, 0.0, 0.0, 0.0]
    assert got["closest_point"].tolist() == [[1, 1, 0], [1, 1, 0], [1, 2, 0], [0, 0, 0], [4, 0, 0], [0, 4, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0],
                                            [0, 0, 0], [2, 0, 0], [2, 2, 0]]
    assert got["closest_uv"].tolist() == [[0.25, 0.25], [0.25, 0.25], [0.25, 0.5], [0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5],
                                         [0, 0], [0.5, 0], [0.5, 0.5]]
    # (1, 1): 0.5 * 10 + 0.25 * 20 + 0.25 * 30; (1, 2): 0.25 * 10 + 0.25 * 20 + 0.5 * 30; corners; edge midpoints
    assert got["closest_temperature"].tolist() == [17.5, 17.5, 22.5, 10.0, 20.0, 30.0, 15.0, 20.0, 25.0, 10.0, 15.0, 25.0]
    assert got["difference"].tolist() == [2.5, 2.5, -2.5, 10.0, 0.0, -10.0, 5.0, 0.0, -5.0, 10.0, 5.0, -5.0]
    assert got["closest_colors"][[0, 2, 4, 8]].tolist() == [[50, 50, 64], [50, 75, 128], [200, 100, 0], [100, 100, 128]], "63.75 and 127.5 round up"
    assert got["counts"].tolist() == [12, 12, 1, 0]
    distances = [0.0, 2.0, 3.0, root2, root2, root3, 2.0, 2.0, root2, 0.0, 0.0, 0.0]
    assert got["stats"].tolist() == [sum(distances, 0.0), sum((x * x for x in distances), 0.0), 0.0, 3.0, 12.5, 3 * 6.25 + 3 * 100.0 + 4 * 25.0, -10.0,
                                     10.0]
    assert got["closest_face"].dtype == np.int32 and got["closest_distance"].dtype == F and got["counts"].dtype == np.int64 and got["stats"].dtype == D
    assert got["closest_point"].shape == (12, 3) and got["closest_uv"].shape == (12, 2) and got["stats"].shape == (8,)


def test_faces_without_area_are_the_segment_or_the_point_they_are():
    pos, temp, col, tri = C.degenerate_mesh()
    assert C.usable_faces(pos, temp, tri).all(), "distinct indices: usable, whatever the positions"
    got = C.closest(pos, temp, col, tri, C.DEGENERATE_POINTS)
    assert got["closest_face"].tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 1]
    # the collinear face (0,0,0) (2,0,0) (1,0,0): the segment 0 .. 2 on the x axis; (1,1,0) is nearest to (1,0,0), which the first edge
    # names (s = 0.5) before the other two do (s = 1): the first candidate holds on the tie
    assert got["closest_point"][:4].tolist() == [[1, 0, 0], [0, 0, 0], [2, 0, 0], [0.5, 0, 0]]
    assert got["closest_uv"][:4].tolist() == [[0.5, 0], [0, 0], [1, 0], [0.25, 0]] and got["closest_temperature"][:4].tolist() == [15.0, 10.0, 20.0, 12.5]
    assert got["closest_distance"][:4].tolist() == [1.0, 1.0, float(F(math.sqrt(5.0))), 0.0]
    # the needle (10,0,0) (10,0,0) (10,4,0): its first edge has no length (s = 0 without a division), the other two are the segment
    assert got["closest_point"][4:7].tolist() == [[10, 2, 0], [10, 0, 0], [10, 4, 0]] and got["closest_uv"][4:7].tolist() == [[0, 0.5], [0, 0], [0, 1]]
    assert got["closest_distance"][4:7].tolist() == [3.0, 1.0, float(F(math.sqrt(2.0)))] and got["closest_temperature"][4:7].tolist() == [50.0, 40.0, 60.0]
    # three equal positions: the point
    assert got["closest_point"][7:9].tolist() == [[20, 1, 1]] * 2 and got["closest_distance"][7:9].tolist() == [0.0, 5.0]
    assert got["closest_uv"][7:9].tolist() == [[0, 0]] * 2 and got["closest_temperature"][7:9].tolist() == [70.0, 70.0]
    assert got["closest_distance"][9] == 5.0 and got["closest_point"][9].tolist() == [10, 0, 0], "(15,0,0): 13 from the first, sqrt(27) from the last"
    for name in ("closest_distance", "closest_point", "closest_uv", "closest_temperature"):
        assert np.isfinite(got[name]).all(), name


def test_ties_the_cut_and_unusable_things():
    pos, temp, _, tri = C.SHEETS
    assert C.usable_faces(pos, temp, tri).tolist() == [True, True, True, True, False, False]
    points = C.SHEET_POINTS
    got = C.closest(pos, temp, None, tri, points)
    assert got["closest_face"].tolist() == [0, 2, 1, 1, 1, 0], \
        "3 from both sheets: the lower index; two copies: the lower index; on the shared edge and on a shared vertex: the lower index"
    assert got["closest_distance"].tolist() == [3.0, 2.0, 1.0, 0.0, 1.0, 2.0] and got["closest_colors"] is None and got["difference"] is None
    assert got["closest_uv"][2].tolist() == [0.0, 0.5], "face (1,3,2) at (2,2,0): halfway along its edge from corner 0 to corner 2"
    for cut, want in ((math.inf, [0, 2, 1, 1, 1, 0]), (3.0, [0, 2, 1, 1, 1, 0]), (2.0, [-1, 2, 1, 1, 1, 0]), (1.0, [-1, -1, 1, 1, 1, -1]),
                      (0.5, [-1, -1, -1, 1, -1, -1]), (0.0, [-1, -1, -1, 1, -1, -1])):
        cutoff = C.closest(pos, temp, None, tri, points, max_distance=cut)
        assert cutoff["closest_face"].tolist() == want, ("a distance equal to the cut is inside", cut)
        assert cutoff["counts"].tolist() == [sum(f >= 0 for f in want), 6, 4, 0]
    nothing = C.closest(pos, temp, None, tri, points, max_distance=0.5, point_temperature=np.zeros(6, F))
    gone = [0, 1, 2, 4, 5]
    for name in ("closest_distance", "closest_temperature", "difference"):
        assert C.bits(nothing[name][gone]).tolist() == [NAN] * 5, name
    assert C.bits(nothing["closest_point"][gone]).reshape(-1).tolist() == [NAN] * 15 and C.bits(nothing["closest_uv"][gone]).reshape(-1).tolist() == [NAN] * 10
    assert nothing["stats"].tolist() == [0.0, 0.0, 0.0, 0.0, -32.5, 32.5 * 32.5, -32.5, -32.5], "(3,3,0) on face (1,3,2): 0.25 * 20 + 0.5 * 40 + 0.25 * 30"
    hot = temp.copy()
    hot[5] = np.inf
    assert C.closest(pos, hot, None, tri, points)["closest_face"].tolist() == [2, 2, 1, 1, 1, 2], "a non-finite temperature spoils its faces"
    bad = np.array([(1, 1, 3), (np.nan, 1, 3), (1, np.inf, 3), (1, 1, -np.inf)], F)
    got = C.closest(pos, temp, None, tri, bad, point_temperature=np.array([1, 2, np.nan, 4], F))
    assert got["closest_face"].tolist() == [0, -1, -1, -1] and got["counts"].tolist() == [1, 1, 4, 0]
    assert C.bits(got["difference"][1:]).tolist() == [NAN] * 3 and got["stats"][4:].tolist() == [-56.5, 56.5 * 56.5, -56.5, -56.5]
    own = C.closest(pos, temp, None, tri, points[:2], point_temperature=np.array([np.nan, 25.0], F))
    assert C.bits(own["difference"][:1]).tolist() == [NAN] and own["difference"][1] == 25.0 - 17.5 and own["stats"][4] == 7.5
    empty = C.closest(pos[:0], temp[:0], None, tri, points)
    assert empty["counts"].tolist() == [0, 6, 0, 0] and empty["stats"].tolist() == [0.0, 0.0, math.inf, -math.inf, 0.0, 0.0, math.inf, -math.inf]
    none = C.closest(pos, temp, None, tri, points[:0])
    assert none["counts"].tolist() == [0, 0, 4, 0] and none["closest_face"].shape == (0,) and none["closest_point"].shape == (0, 3)


def test_statistics_are_the_ordered_sums_in_blocks_of_256():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, 600).astype(F)
    x[[3, 300, 599]] = np.nan
    x[7] = -0.0
    x[8] = 0.0
    kept = np.where(np.isnan(x), 0.0, x.astype(D))
    total, squares, low, high = C.stats_of(x)
    blocks = [kept[:256], kept[256:512], kept[512:]]
    assert total == sum((sum(b.tolist(), 0.0) for b in blocks), 0.0) and squares == sum((sum((b * b).tolist(), 0.0) for b in blocks), 0.0)
    assert math.copysign(1.0, low) == -1.0 and low == 0.0 and high == float(np.nanmax(x)), "-0.0 is below +0.0"
    assert C.stats_of(np.full(5, np.nan, F)) == [0.0, 0.0, math.inf, -math.inf] == C.stats_of(np.zeros(0, F))


# ---- what the traversal rests on ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.SCENES)
def test_no_face_is_nearer_than_the_bound_of_its_own_box(name):
    """d2 >= b of the face's own box for every (point, usable face) pair of every scene the device test uses — the first link of the
    header's proof; and no NaN arises anywhere on them (``bound_slack`` asserts it)"""
    pos, temp, _, tri, points = C.scene(name)
    slack, pairs = C.bound_slack(pos, temp, tri, points)
    usable = int(C.usable_faces(pos, temp, tri).sum())
    assert pairs == usable * len(points) and (slack >= 0.0 or pairs == 0), (name, slack)
    if name == "far":
        b = C.box_bound(points[:, None, :].astype(D), *[x[None] for x in C.face_boxes(pos, tri, C.usable_faces(pos, temp, tri))])
        assert b.min() > 0.9e12, "every box is about 10^6 units away: b and d2 differ in their last bits, if at all"


def test_bound_by_hand_and_monotone_under_box_growth():
    lo, hi = np.array([1, 2, 3], F), np.array([2, 4, 3], F)
    assert C.box_bound(np.array([(1.5, 3, 3), (0, 3, 3), (4, 0, 5), (1, 2, 3), (2, 4, -1)], D), lo, hi).tolist() == [0.0, 1.0, 12.0, 0.0, 16.0]
    rng = np.random.default_rng(3)
    n = 20000
    lo = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    hi = (lo + rng.uniform(0.0, 1.0, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.2)).astype(F)  # one side in five is flat
    grow = rng.uniform(0.0, 0.5, (2, n, 3)) * (rng.uniform(0, 1, (2, n, 3)) > 0.3)
    plo, phi = (lo - grow[0]).astype(F), (hi + grow[1]).astype(F)
    assert (plo <= lo).all() and (phi >= hi).all()
    q = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    on = rng.uniform(0, 1, (n, 3)) < 0.1
    q[on] = lo[on]  # a point on a box plane
    q[:2000] *= F(1e6)
    q[2000:6000] = (lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3)))[2000:6000]  # inside the box: b = 0
    child, parent = C.box_bound(q, lo, hi), C.box_bound(q, plo, phi)
    assert (parent <= child).all() and 0.05 < (child == 0.0).mean() < 0.95 and (parent < child).mean() > 0.3


# ---- the declarations and the refusals ---------------------------------------------------------------------------------------------------

NAMES = ("positions", "temperature", "colors", "triangles", "num_vertices", "num_triangles", "bvh", "bvh_bytes", "points", "point_temperature",
         "num_points", "params", "closest_face", "closest_distance", "closest_point", "closest_uv", "closest_temperature", "closest_colors",
         "difference", "counts", "stats", "stream")


def test_entry_struct_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = re.search(r"\bint tn_mesh_closest\(([^;]*)\);", header).group(1)
    assert [re.split(r"[\s\*]+", a.strip())[-1] for a in declared.split(",")] == list(NAMES)
    assert header.index("int tn_mesh_raycast(") < header.index("int tn_mesh_closest("), "behind the ray cast"
    result, arguments = _hip.SIGNATURES["tn_mesh_closest"]
    assert result == ctypes.c_int and len(arguments) == len(NAMES) and arguments[11] == ctypes.POINTER(_hip.tn_closest_params)
    assert arguments[4] == arguments[5] == arguments[10] == ctypes.c_int64 and arguments[7] == ctypes.c_size_t
    assert ctypes.sizeof(_hip.tn_closest_params) == 16 and [f[0] for f in _hip.tn_closest_params._fields_] == ["max_distance", "reserved"]
    assert _hip.tn_closest_params.max_distance.offset == 0 and _hip.tn_closest_params.reserved.offset == 8
    body = re.search(r"typedef struct tn_closest_params \{([^}]*)\} tn_closest_params;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;\[])", body) == ["max_distance", "reserved"]
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert "tn_mesh_closest.hip" in makefile and "tn_mesh_bvh.h " in makefile
    text = " ".join(header.split())
    assert "Why the tree cannot change the output: after the clamp" in text and "d2 >= b of the face's own box" in text, "the proof is in the header"


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _hip.load()
    limit = (2 ** 31 - 1) // 3
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy, t = 4096, 2000
    blob = mesh_bvh_bytes(t)

    def params(max_distance=math.inf):
        return _hip.tn_closest_params(max_distance)

    good = dict(zip(NAMES, [dummy, dummy, dummy, dummy, 1000, t, dummy, blob - 1, dummy, dummy, 500, params()] + [dummy] * 9 + [None]))

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_closest(*[args[k] for k in NAMES])

    assert call() == -4 and call(bvh_bytes=0) == -4  # TN_ERR_WORKSPACE: the last refusal, so everything before it passed
    for k in ("positions", "temperature", "colors", "triangles", "bvh", "points", "point_temperature", "params", "closest_temperature",
              "closest_distance"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    for k in ("closest_face", "closest_point", "closest_uv", "closest_colors", "difference", "counts", "stats"):
        assert call(**{k: None}) == -4, f"{k} may be absent"
    assert call(colors=None, closest_colors=None) == -4 and call(point_temperature=None, difference=None) == -4
    assert call(closest_temperature=None, difference=None) == -4 and call(closest_distance=None, stats=None) == -4
    assert call(**{k: None for k in NAMES[12:21]}) == -4, "every output absent"
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert call(num_points=-1) == -2 and call(num_points=limit + 1) == -2  # TN_ERR_SHAPE
    for bad in (math.nan, -1.0, -math.inf, -1e-300):
        assert call(params=params(bad)) == -3, bad  # TN_ERR_UNSUPPORTED
    for fine in (0.0, -0.0, 1e-300, 1e300, math.inf):
        assert call(params=params(fine)) == -4, fine
    for k in ("positions", "temperature", "triangles", "points", "point_temperature", "closest_face", "closest_distance", "closest_point",
              "closest_uv", "closest_temperature", "difference"):
        assert call(**{k: dummy + 2}) == -2, k
    assert call(counts=dummy + 4) == -2 and call(stats=dummy + 4) == -2 and call(bvh=dummy + 32) == -2
    assert call(colors=dummy + 1, closest_colors=dummy + 1) == -4, "bytes need no alignment"
    bad = params(-1.0)
    assert call(params=bad, bvh=None) == -1 and call(params=bad, num_points=-1) == -2 and call(params=bad, points=None) == -3 and \
        call(points=None, closest_uv=dummy + 2) == -1 and call(closest_uv=dummy + 2, bvh_bytes=0) == -2, "in the siblings' order"
    assert call(num_points=0, points=None, point_temperature=None) == -4, "without a point the two input arrays may be absent"
    assert call(num_points=0, closest_temperature=None) == -1
    assert call(num_vertices=0, positions=None, temperature=None, colors=None, closest_colors=None) == -4, "a mesh without vertices needs no arrays"
    assert call(num_triangles=0, triangles=None, positions=None, temperature=None, bvh_bytes=63) == -4 and mesh_bvh_bytes(0) == 64


def _host_mesh():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    return mesh, MeshBVH(torch.zeros(128, dtype=torch.uint8), 3, 1, mesh)


def test_python_layer_refuses_before_it_reaches_a_kernel():
    mesh, bvh = _host_mesh()
    points = torch.zeros((4, 3))
    for bad in (-1.0, math.nan, -math.inf):
        for call in (lambda: mesh_closest(bvh, points, max_distance=bad), lambda: mesh_closest_into(bvh, points, max_distance=bad),
                     lambda: mesh_difference(mesh, bvh, max_distance=bad)):
            with pytest.raises(ValueError, match="max_distance"):
                call()
    for call in (lambda: mesh_closest(bvh, points), lambda: mesh_closest_into(bvh, points), lambda: mesh_difference(mesh, bvh, max_distance=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="no triangles"):
        mesh_difference(ThermalMesh(mesh.positions, mesh.colors, mesh.temperature), bvh, max_distance=1.0)
    with pytest.raises(TypeError):
        mesh_difference(mesh, bvh)  # the radius is required: there is no distance that suits every pair of surveys
    fields = {f.name for f in __import__("dataclasses").fields(ClosestPoints)}
    assert {"closest_face", "closest_distance", "closest_point", "closest_uv", "closest_temperature", "closest_colors", "difference", "found",
            "usable_points", "usable_faces", "stack_limit_points", "mean_distance", "rms_distance", "min_distance", "max_distance",
            "mean_difference", "rms_difference", "min_difference", "max_difference"} <= fields
    assert {"closest", "mesh", "matched_share", "mean_distance", "rms_distance", "max_distance", "mean_difference", "rms_difference",
            "min_difference", "max_difference"} <= {f.name for f in __import__("dataclasses").fields(MeshDifference)}
    assert "unusable for ``thermal_regions`` and the rasteriser" in " ".join(mesh_difference.__doc__.split())


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_command_line_arguments(capsys):
    tool = _tool()
    base = ["now.ply", "before.ply", "--max-distance", "0.05", "--output", "diff.ply", "--report", "diff.json"]
    args = tool.parse(base)
    assert (str(args.mesh), str(args.reference), args.max_distance, str(args.output), str(args.report), args.min_change, args.length_scale) == \
        ("now.ply", "before.ply", 0.05, "diff.ply", "diff.json", None, 1.0)
    args = tool.parse(base + ["--min-change", "2.0", "--length-scale", "0.37"])
    assert args.min_change == 2.0 and args.length_scale == 0.37
    assert tool.parse(base[:2] + ["--max-distance", "inf"] + base[4:]).max_distance == math.inf
    for bad, flag in ((["--max-distance", "-1"], "--max-distance"), (["--max-distance", "nan"], "--max-distance"), (["--min-change", "0"], "--min-change"),
                      (["--min-change", "-2"], "--min-change"), (["--min-change", "inf"], "--min-change"), (["--length-scale", "0"], "--length-scale"),
                      (["--length-scale", "nan"], "--length-scale")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    for missing in ("--max-distance", "--output", "--report"):
        k = base.index(missing)
        with pytest.raises(SystemExit):
            tool.parse(base[:k] + base[k + 2:])
        assert missing in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tool.parse(base[1:])
    for flag in ("--max-distance", "--output", "--report", "--min-change", "--length-scale"):
        assert flag in tool.__doc__, flag


def _hand_made(matched=3):
    closest = SimpleNamespace(usable_faces=7, stack_limit_points=0)
    if not matched:
        return SimpleNamespace(closest=closest, matched=0, matched_share=0.0, mean_distance=math.nan, rms_distance=math.nan, max_distance=-math.inf,
                               mean_difference=math.nan, rms_difference=math.nan, min_difference=math.inf, max_difference=-math.inf)
    return SimpleNamespace(closest=closest, matched=3, matched_share=0.75, mean_distance=0.25, rms_distance=0.5, max_distance=1.0,
                           mean_difference=-1.5, rms_difference=2.0, min_difference=-3.0, max_difference=0.5)


def test_report_schema_with_a_hand_made_result():
    tool = _tool()
    report = tool.build_report(_hand_made(), 4, 2, 9, 8, 0.05, source="now.ply", reference="before.ply")
    assert json.loads(json.dumps(report)) == report, "plain JSON: no numpy scalars, no infinities"
    assert set(report) == {"mesh", "reference", "length_scale", "max_distance", "counts", "matched_share", "distance", "difference"}
    assert report["counts"] == {"vertices": 4, "faces": 2, "reference_vertices": 9, "reference_faces": 8, "reference_usable_faces": 7,
                                "matched_vertices": 3, "stack_limit_points": 0}
    assert report["distance"] == {"mean": 0.25, "rms": 0.5, "max": 1.0} and report["matched_share"] == 0.75 and report["max_distance"] == 0.05
    assert report["difference"] == {"mean": -1.5, "rms": 2.0, "min": -3.0, "max": 0.5}
    line = tool.summary_line(report)
    assert "\n" not in line and line.startswith("now.ply against before.ply: 4 vertices, 3 matched (75.0 %), distance mean 0.25 rms 0.5 max 1, "
                                                "difference mean -1.50 C rms 2.00 min -3.00 max +0.50")
    table = np.zeros(2, REGION_DTYPE)
    table["area"], table["faces"], table["mean_temperature"] = [2.0, 0.5], [5, 1], [3.0, 2.5]
    table["min_temperature"], table["max_temperature"], table["centroid"] = [2.25, 2.5], [4.0, 2.5], [[1, 2, 3], [4, 5, 6]]
    warmed = ThermalRegions(table, np.array([1, 0]), torch.zeros(2, dtype=torch.int32), 10.0, 2.5, 2, 6, 8, (2.0, math.inf))
    cooled = ThermalRegions(table[:0], np.zeros(0, np.int64), torch.zeros(2, dtype=torch.int32), 10.0, 0.0, 0, 0, 8, (-math.inf, -2.0))
    report = tool.build_report(_hand_made(), 4, 2, 9, 8, math.inf, 2.0, warmed, cooled, 2.0, "now.ply", "before.ply")
    assert json.loads(json.dumps(report)) == report and report["max_distance"] is None and report["min_change"] == 2.0
    assert set(report) >= {"warmed", "cooled", "compared_area", "min_change"} and report["compared_area"] == 40.0
    assert report["distance"] == {"mean": 0.5, "rms": 1.0, "max": 2.0}, "lengths times the scale"
    assert report["warmed"] == {"area": 10.0, "share": 0.25, "regions": [
        {"region": 1, "faces": 5, "area": 8.0, "mean_difference": 3.0, "largest_change": 4.0, "centroid": [2.0, 4.0, 6.0]},
        {"region": 0, "faces": 1, "area": 2.0, "mean_difference": 2.5, "largest_change": 2.5, "centroid": [8.0, 10.0, 12.0]}]}
    assert report["cooled"] == {"area": 0.0, "share": 0.0, "regions": []}
    assert tool.region_rows(warmed, False)[0]["largest_change"] == 2.25, "of a region that cooled: its coldest face"
    lines = tool.region_lines(report)
    assert lines == ["warmed 0: area 8, 5 faces, mean +3.00 C, largest +4.00 C, centroid (2, 4, 6)",
                     "warmed 1: area 2, 1 faces, mean +2.50 C, largest +2.50 C, centroid (8, 10, 12)"]
    empty = tool.build_report(_hand_made(0), 4, 2, 9, 8, 0.05, source="now.ply", reference="before.ply")
    assert json.loads(json.dumps(empty)) == empty and empty["distance"] == {"mean": None, "rms": None, "max": None}
    assert empty["difference"] == {"mean": None, "rms": None, "min": None, "max": None} and "none within 0.05" in tool.summary_line(empty)
