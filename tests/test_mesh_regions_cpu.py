"""The yardstick of the thermal-regions kernel (tests/mesh_regions_reference.py) checked on its own — the literal cases, a sphere's
area, that its ordered sum is told apart from the other two on the meshes the device tests use — and the host side of the feature:
the declarations, the struct, the ordering and filtering of the region table, the command line and its report.  No GPU."""
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

from tests import mesh_regions_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (REGION_DTYPE, ThermalMesh, ThermalRegions, mesh_regions_into, mesh_regions_workspace_bytes,
                                    order_regions, regions_mesh, thermal_regions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_regions_tool", os.path.join(ROOT, "tools", "mesh_regions.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the reference against its literal cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_yardstick_on_the_literal_cases(name):
    case = R.LITERAL[name]
    got = R.regions(*R.literal_arrays(case), *case["window"])
    assert R.literal_mismatch(got, case["want"]) is None, R.literal_mismatch(got, case["want"])
    assert got["regions"].dtype == R.REGION_DTYPE and got["face_region"].dtype == np.int32 and got["face_area"].dtype == D
    assert got["counts"].dtype == np.int64 and got["totals"].dtype == D


def test_literal_cases_are_the_ones_the_feature_is_defined_by():
    w = {k: R.LITERAL[k]["want"] for k in R.LITERAL}
    assert w["unit_square_window_open"]["area"] == [1.0] and w["unit_square_window_open"]["centroid"] == [(0.5, 0.5, 0.0)]
    assert w["unit_square_window_open"]["mean_temperature"] == [24.0]
    assert w["unit_square_one_face_outside"]["face_region"] == [-1, 0] and w["unit_square_one_face_outside"]["totals"] == [1.0, 0.5]
    assert w["two_patches_touching_in_one_vertex"]["counts"][0] == 1
    assert w["two_patches_joined_only_through_a_cold_face"]["counts"][0] == 2
    assert w["hottest_vertex_tie"]["hottest_vertex"] == [1] and w["hottest_vertex_tie"]["coldest_vertex"] == [0]


def test_degenerate_faces_in_the_yardstick():
    pos = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (np.nan, 0, 0), (0, np.inf, 0), (5, 5, 5)], F)
    temp = np.array([20, 20, 20, 20, 20, 20, np.nan], F)
    tri = np.array([(0, 1, 2), (0, 1, 3), (0, 0, 1), (0, 1, 7), (-1, 0, 1), (0, 1, 4), (0, 1, 5), (0, 1, 6)], np.int32)
    got = R.regions(pos, temp, tri)
    # the collinear face is usable and selected with area +0.0; a repeated, foreign, NaN or inf corner makes a face unusable
    assert got["counts"].tolist() == [1, 2, 2] and got["face_region"].tolist() == [0, 0, -1, -1, -1, -1, -1, -1]
    assert R.bits(got["face_area"]).tolist() == R.bits(np.array([0.0, 0.5, 0, 0, 0, 0, 0, 0], D)).tolist()
    flat = R.regions(pos, temp, tri[:1])  # a region of no area: the NaN of the header
    assert flat["counts"].tolist() == [1, 1, 1] and flat["regions"]["area"][0] == 0.0
    assert R.bits(flat["regions"]["mean_temperature"]).tolist() == [0x7fc00000]
    assert R.bits(flat["regions"]["centroid"]).tolist() == [[0x7fc00000] * 3]
    assert R.regions(pos, temp, tri, 30.0, 10.0)["counts"].tolist() == [0, 0, 2]  # min > max selects nothing
    # the extremes order -0.0 below +0.0, whoever comes first
    assert R.bits(np.array([R.lowest([F(0.0), F(-0.0)]), R.lowest([F(-0.0), F(0.0)])], F)).tolist() == [0x80000000] * 2
    assert R.bits(np.array([R.highest([F(0.0), F(-0.0)]), R.highest([F(-0.0), F(0.0)])], F)).tolist() == [0] * 2


# ---- a sphere's area ------------------------------------------------------------------------------------------------------------------

def test_icosphere_area_within_its_own_tessellation_error():
    radius = 0.75
    pos, tri = R.icosphere(3, radius)
    assert len(tri) == 20 * 4 ** 3 and len(pos) == 10 * 4 ** 3 + 2
    got = R.regions(pos.astype(F), np.full(len(pos), 21.5, F), tri)
    assert got["counts"].tolist() == [1, len(tri), len(tri)] and got["regions"]["faces"][0] == len(tri)
    # A face lies in a plane at distance d = sqrt(r^2 - rho^2) from the centre, rho the circumradius of its three chords
    # (rho = a b c / (4 area)).  Projected from the centre onto the sphere an area element of that plane grows by r^2 d / s^3 with
    # d <= s <= r the distance of the element, i.e. by at most (r / d)^2 and at least d / r > 0; the projections tile the sphere.
    # So 4 pi r^2 (d_min / r)^2 <= polyhedron area <= 4 pi r^2.  The fp32 vertices are off the sphere by 2^-24 relative: 1e-6 covers it.
    p = pos[tri]
    a, b, c = (np.linalg.norm(p[:, i] - p[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0)))
    flat_area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    rho = a * b * c / (4.0 * flat_area)
    d_min = float(np.sqrt(radius ** 2 - rho ** 2).min())
    sphere = 4.0 * math.pi * radius ** 2
    total = float(got["totals"][0])
    print(f"icosphere level 3: area {total:.9f}, sphere {sphere:.9f}, lower bound {sphere * (d_min / radius) ** 2:.9f}")
    assert sphere * (d_min / radius) ** 2 * (1 - 1e-6) <= total <= sphere * (1 + 1e-6)
    assert (d_min / radius) ** 2 > 0.98, "a level-3 icosphere is within 2 % of its sphere"
    assert got["totals"][1] == got["totals"][0] == got["regions"]["area"][0]
    centroid = got["regions"]["centroid"][0]
    assert np.abs(centroid).max() < 1e-6 * radius and got["regions"]["mean_temperature"][0] == F(21.5)


# ---- the ordered sum is told apart ------------------------------------------------------------------------------------------------------

def test_sum2_differs_from_the_sequential_and_the_pairwise_sum_on_the_test_meshes():
    pos, tri = R.lattice(40, 40, R.LATTICE_SEED)
    temp = R.lattice_temperature(pos, R.LATTICE_SEED)
    area = R.face_quantities(pos, temp, tri, -math.inf, math.inf)[3]
    assert len(area) == 2 * 39 * 39
    a, b, c = R.sum2(area.tolist()), R.sequential_sum(area.tolist()), float(np.sum(area))
    print(f"40 x 40 lattice: SUM2 {a.hex()}, sequential {b.hex()}, numpy.sum {c.hex()}")
    assert a != b and a != c, "the lattice cannot tell SUM2 from another order of summation: choose another seed"
    for faces in (513, 65537):
        p, t = R.strip(faces, R.STRIP_SEED)
        area = R.face_quantities(p, np.zeros(len(p), F), t, -math.inf, math.inf)[3]
        assert len(area) == faces and R.sum2(area.tolist()) not in (R.sequential_sum(area.tolist()), float(np.sum(area))), faces
    # by construction: up to 257 entries SUM2 is the sequential sum (one block, or one block and one more entry)
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257):
        x = rng.uniform(0.0, 1.0, n).tolist()
        assert R.sum2(x) == R.sequential_sum(x)
    assert R.sum2([]) == 0.0 and math.copysign(1.0, R.sum2([-0.0])) == 1.0, "a sum starts from +0.0"


def test_the_lattice_window_gives_more_than_a_hundred_regions_of_mixed_size():
    pos, tri = R.lattice(40, 40, R.LATTICE_SEED)
    temp = R.lattice_temperature(pos, R.LATTICE_SEED)
    got = R.regions(pos, temp, tri, *R.LATTICE_WINDOW)
    faces = got["regions"]["faces"]
    assert len(faces) > 100 and faces.max() > 256 and (faces == 1).sum() > 10 and ((faces > 5) & (faces < 100)).sum() > 10
    assert int(faces.sum()) == int(got["counts"][1]) == int((got["face_region"] >= 0).sum())
    assert np.array_equal(np.unique(got["face_region"][got["face_region"] >= 0]), np.arange(len(faces)))
    assert (np.diff(got["regions"]["label"]) > 0).all(), "regions are numbered in ascending label"
    whole = R.regions(pos, temp, tri)
    assert whole["counts"].tolist() == [1, len(tri), len(tri)] and whole["totals"][0] == whole["totals"][1] == whole["regions"]["area"][0]


# ---- the declarations ------------------------------------------------------------------------------------------------------------------

NAMES = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "min_temperature", "max_temperature", "regions",
         "capacity_regions", "face_region", "face_area", "counts", "totals", "workspace", "workspace_bytes", "stream")


def test_entry_struct_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bsize_t tn_mesh_regions_workspace_bytes\(int64_t num_vertices, int64_t num_triangles\);", header)
    assert re.search(r"\bint tn_mesh_regions\(const float \*positions, const float \*temperature, const int32_t \*triangles", header)
    assert re.search(r"typedef struct tn_mesh_region \{[^}]*\} tn_mesh_region;", header)
    assert len(_hip.SIGNATURES["tn_mesh_regions"][1]) == len(NAMES) == 16 and len(_hip.SIGNATURES["tn_mesh_regions_workspace_bytes"][1]) == 2
    assert _hip.SIGNATURES["tn_mesh_regions"][1][5:7] == [ctypes.c_float, ctypes.c_float]
    assert "tn_mesh_regions.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    offsets = {"area": 0, "label": 8, "faces": 12, "mean_temperature": 16, "min_temperature": 20, "max_temperature": 24,
               "centroid": 28, "bounds": 40, "coldest_vertex": 64, "hottest_vertex": 68}
    assert ctypes.sizeof(_hip.tn_mesh_region) == 72 == REGION_DTYPE.itemsize == R.REGION_DTYPE.itemsize
    for name, offset in offsets.items():
        assert getattr(_hip.tn_mesh_region, name).offset == offset == REGION_DTYPE.fields[name][1] == R.REGION_DTYPE.fields[name][1], name
    assert [f[0] for f in _hip.tn_mesh_region._fields_] == list(REGION_DTYPE.names) == list(offsets)
    # the header's struct lists the same fields in the same order
    body = re.search(r"typedef struct tn_mesh_region \{([^}]*)\}", header).group(1)
    declared = re.findall(r"\b([a-z_]+)(?:\[\d\])?(?=[,;])", body)
    assert declared == list(offsets), declared


def test_entry_refuses_bad_arguments_before_any_launch():
    lib = _hip.load()
    v, t = 1000, 2000
    need = mesh_regions_workspace_bytes(v, t)
    limit = (2 ** 31 - 1) // 3
    assert need > 0 and need % 8 == 0 and mesh_regions_workspace_bytes(2 ** 31 - 1, limit) > 0
    for bad in ((-1, t), (v, -1), (2 ** 31, t), (v, limit + 1)):
        assert mesh_regions_workspace_bytes(*bad) == 0, bad
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy = 4096
    good = dict(zip(NAMES, [dummy, dummy, dummy, v, t, 20.0, 30.0, dummy, 10, dummy, dummy, dummy, dummy, dummy, need, None]))

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_regions(*[args[k] for k in NAMES])

    for k in ("positions", "temperature", "triangles", "regions", "face_region", "counts", "totals", "workspace"):
        assert call(**{k: None}, workspace_bytes=0) == -1, k  # TN_ERR_NULL
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2  # TN_ERR_SHAPE
    assert call(num_triangles=limit + 1, workspace_bytes=2 ** 60) == -2 and call(capacity_regions=-1) == -2
    for k in ("positions", "temperature", "triangles", "face_region"):
        assert call(**{k: dummy + 2}) == -2, k
    for k in ("regions", "face_area", "counts", "totals", "workspace"):
        assert call(**{k: dummy + 4}) == -2, k
    nan = float("nan")
    assert call(min_temperature=nan) == -3 and call(max_temperature=nan) == -3 and call(min_temperature=nan, counts=dummy + 4) == -3
    assert call(min_temperature=nan, counts=None) == -1 and call(min_temperature=nan, num_vertices=-1) == -2, "in the neighbours' order"
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    # what may be absent, checked up to the workspace's size: face_area, and regions with a capacity of 0; infinite bounds, min > max
    assert call(face_area=None, regions=None, capacity_regions=0, workspace_bytes=0) == -4
    assert call(min_temperature=-math.inf, max_temperature=math.inf, workspace_bytes=0) == -4
    assert call(min_temperature=30.0, max_temperature=20.0, workspace_bytes=0) == -4


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def _table(rows):
    table = np.zeros(len(rows), REGION_DTYPE)
    for k, (area, label) in enumerate(rows):
        table[k]["area"], table[k]["label"], table[k]["faces"] = area, label, 1
    return table


def test_order_regions_on_a_hand_made_table():
    table = _table([(2.0, 0), (0.0, 3), (5.0, 7), (2.0, 9), (0.25, 12), (5.0, 20), (1e-300, 31)])
    assert order_regions(table).tolist() == [2, 5, 0, 3, 4, 6], "area descending, ties by ascending label, zero area dropped"
    assert order_regions(table, min_area=2.0).tolist() == [2, 5, 0, 3] and order_regions(table, min_area=2.5).tolist() == [2, 5]
    assert order_regions(table, top=3).tolist() == [2, 5, 0] and order_regions(table, top=0).tolist() == []
    assert order_regions(table, min_area=0.2, top=100).tolist() == [2, 5, 0, 3, 4] and order_regions(table, min_area=9.0).tolist() == []
    assert order_regions(table[::-1].copy()).tolist() == [4, 1, 6, 3, 2, 0], "ties go by the label, not by the row"
    assert order_regions(_table([])).tolist() == [] and order_regions(table).dtype == np.int64
    for bad in (dict(min_area=-1.0), dict(min_area=float("nan")), dict(top=-1)):
        with pytest.raises(ValueError):
            order_regions(table, **bad)


def test_python_layer_refuses_before_it_reaches_a_kernel():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    bare = ThermalMesh(pos, mesh.colors, mesh.temperature)
    with pytest.raises(ValueError, match="no triangles"):
        thermal_regions(bare, 20.0)
    with pytest.raises(ValueError, match="no triangles"):
        mesh_regions_into(bare, 20.0, 30.0, counts=None, totals=None)
    for bad in (dict(min_temperature=float("nan")), dict(max_temperature=float("nan")), dict(min_area=-1.0), dict(top=-2)):
        with pytest.raises(ValueError):
            thermal_regions(mesh, **bad)
    for call in (lambda: thermal_regions(mesh, 20.0),
                 lambda: mesh_regions_into(mesh, 20.0, 30.0, counts=torch.zeros(3, dtype=torch.int64), totals=torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    found = ThermalRegions(_table([]), np.zeros(0, np.int64), torch.full((2,), -1, dtype=torch.int32), 1.0, 0.0, 0, 0, 1, (20.0, 30.0))
    with pytest.raises(ValueError, match="another mesh"):
        regions_mesh(mesh, found)


def test_regions_mesh_keeps_the_faces_of_the_kept_regions_and_compacts_the_vertices():
    # host tensors: regions_mesh is torch indexing, the same on any device
    v = 8
    pos = torch.arange(3 * v, dtype=torch.float32).reshape(v, 3)
    colors = torch.arange(3 * v, dtype=torch.uint8).reshape(v, 3)
    temp = torch.arange(v, dtype=torch.float32) + 20
    normals = -pos
    tri = torch.tensor([[5, 6, 7], [0, 1, 2], [2, 3, 4], [1, 2, 7]], dtype=torch.int32)
    mesh = ThermalMesh(pos, colors, temp, colors + 1, tri, (14.0, 33.0), normals)
    face_region = torch.tensor([1, 0, -1, 2], dtype=torch.int32)
    found = ThermalRegions(_table([(1.0, 5), (2.0, 1)]), np.array([1, 2], np.int64), face_region, 4.0, 3.0, 3, 3, 4, (20.0, 30.0))
    out = regions_mesh(mesh, found)
    keep = [1, 2, 5, 6, 7]
    assert out.triangles.tolist() == [[2, 3, 4], [0, 1, 4]] and out.triangles.dtype == torch.int32
    for name in ("positions", "colors", "temperature", "thermal_colors", "normals"):
        assert torch.equal(getattr(out, name), getattr(mesh, name)[keep]), name
    assert out.temperature_bounds == (14.0, 33.0)
    none = regions_mesh(mesh, ThermalRegions(_table([]), np.zeros(0, np.int64), face_region, 4.0, 3.0, 3, 3, 4, (20.0, 30.0)))
    assert len(none) == 0 and tuple(none.triangles.shape) == (0, 3)


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def test_command_line_refuses_bad_arguments(capsys):
    tool = _tool()
    base = ["mesh.ply", "--report", "r.json"]
    args = tool.parse(base + ["--min-temperature", "28"])
    assert (args.min_temperature, args.max_temperature, args.min_area, args.top, args.length_scale) == (28.0, math.inf, 0.0, None, 1.0)
    assert args.output is None and args.colors == "rgb"
    args = tool.parse(base + ["--max-temperature", "5", "--min-area", "0.5", "--top", "3", "--length-scale", "2.5", "--output", "o.ply",
                              "--colors", "thermal"])
    assert (args.min_temperature, args.max_temperature, args.min_area, args.top, args.length_scale) == (-math.inf, 5.0, 0.5, 3, 2.5)
    for bad, flag in ((["--min-temperature=nan"], "--min-temperature"), ([], "--min-temperature"), (["--min-temperature", "1", "--min-area=-1"], "--min-area"),
                      (["--min-temperature", "1", "--top=-1"], "--top"), (["--min-temperature", "1", "--length-scale", "0"], "--length-scale"),
                      (["--min-temperature", "1", "--length-scale", "inf"], "--length-scale"), (["--min-temperature", "1", "--colors", "x"], "--colors")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        tool.parse(["mesh.ply", "--min-temperature", "28"])  # no --report
    assert "--report" in capsys.readouterr().err
    for flag in ("--min-temperature", "--max-temperature", "--min-area", "--top", "--length-scale", "--report", "--output", "--colors"):
        assert flag in tool.__doc__, flag


def test_report_schema_and_length_scale_with_a_fake_result():
    tool = _tool()
    positions = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (9, 9, 9)], F)
    temperature = np.array([20, 23, 26, 29, 0], F)
    table = np.zeros(2, REGION_DTYPE)
    table[0] = (1.0, 0, 2, 24.0, 23.0, 25.0, (0.5, 0.5, 0.0), (0, 0, 0, 1, 1, 0), 0, 3)
    table[1] = (0.25, 1, 1, 26.0, 26.0, 26.0, (0.75, 0.5, 0.0), (1, 0, 0, 1, 1, 0), 1, 2)
    found = ThermalRegions(table, np.array([4, 6], np.int64), torch.zeros(3, dtype=torch.int32), 8.0, 2.0, 7, 3, 5, (23.0, math.inf))
    plain = tool.build_report(found, positions, temperature, 6, 1.0, "mesh.ply")
    assert json.loads(json.dumps(plain)) == plain, "plain JSON: no numpy scalars, no infinities"
    assert set(plain) == {"mesh", "length_scale", "window", "counts", "mesh_area", "selected_area", "selected_share", "regions"}
    assert plain["window"] == {"min_temperature": 23.0, "max_temperature": None}
    assert plain["counts"] == {"vertices": 5, "faces": 6, "usable_faces": 5, "selected_faces": 3, "regions": 7, "reported_regions": 2}
    assert (plain["mesh_area"], plain["selected_area"], plain["selected_share"]) == (8.0, 2.0, 0.25)
    first = plain["regions"][0]
    assert set(first) == {"region", "label", "faces", "area", "mean_temperature", "min_temperature", "max_temperature", "centroid",
                          "bounds", "hottest_vertex", "coldest_vertex"}
    assert first == {"region": 4, "label": 0, "faces": 2, "area": 1.0, "mean_temperature": 24.0, "min_temperature": 23.0,
                     "max_temperature": 25.0, "centroid": [0.5, 0.5, 0.0], "bounds": {"min": [0.0, 0.0, 0.0], "max": [1.0, 1.0, 0.0]},
                     "hottest_vertex": {"index": 3, "position": [0.0, 1.0, 0.0], "temperature": 29.0},
                     "coldest_vertex": {"index": 0, "position": [0.0, 0.0, 0.0], "temperature": 20.0}}
    assert plain["regions"][1]["region"] == 6 and plain["regions"][1]["hottest_vertex"]["position"] == [1.0, 1.0, 0.0]
    scaled = tool.build_report(found, positions, temperature, 6, 2.0, "mesh.ply")
    assert (scaled["length_scale"], scaled["mesh_area"], scaled["selected_area"], scaled["selected_share"]) == (2.0, 32.0, 8.0, 0.25)
    s = scaled["regions"][0]
    assert s["area"] == 4.0 and s["centroid"] == [1.0, 1.0, 0.0] and s["bounds"]["max"] == [2.0, 2.0, 0.0]
    assert s["hottest_vertex"] == {"index": 3, "position": [0.0, 2.0, 0.0], "temperature": 29.0}
    assert (s["mean_temperature"], s["min_temperature"], s["max_temperature"], s["faces"]) == (24.0, 23.0, 25.0, 2), "degrees are not lengths"
    lines = tool.region_lines(plain)
    assert len(lines) == 2 and lines[0].startswith("region 0: area 1, 2 faces, mean 24.00 C") and "label 0" in lines[0]
    assert tool.file_bounds(["temperature_unit celsius", "temperature_bounds 14.0 33.0"]) == (14.0, 33.0)
    assert tool.file_bounds(["temperature_bounds none none"]) is None
    colours = tool.thermal_bytes(np.array([14.0, 33.0, 100.0, -5.0, 23.5], F), (14.0, 33.0))
    from thermo_nerf_amd import colormaps
    magma = colormaps.table_u8("magma")
    assert colours.dtype == np.uint8 and colours.tolist() == magma[[0, 255, 255, 0, 128]].tolist()
