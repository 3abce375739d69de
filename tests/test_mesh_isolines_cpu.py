"""The yardstick of the level-set curves (tests/mesh_isolines_reference.py) against closed forms, the new entries in header, ctypes
table and library, and the curve PLY writer.  No GPU."""
from __future__ import annotations

import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import mesh_isolines_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import CURVE_DTYPE, write_curves_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
Z = (0.0, 0.0, 1.0)


def _cube(levels, normal=Z, tri=None, temp=None):
    pos, faces = R.cube()
    tri = faces if tri is None else tri
    temp = np.linspace(18.0, 25.0, 8).astype(F) if temp is None else temp
    return R.isolines(pos, temp, tri, R.half_edges(tri, 8)["twin"], levels, normal=normal)


def test_the_cube_is_closed_manifold_and_its_middle_cut_is_one_loop_of_length_four():
    edges = R.half_edges(R.cube()[1], 8)
    assert edges["counts"].tolist() == [18, 0, 0, 0] and sorted(edges["twin"].tolist()) == list(range(36))
    assert (edges["twin"][edges["twin"]] == np.arange(36)).all()
    got = _cube([0.5])
    assert got["counts"].tolist() == [8, 1, 9, 1, 12]
    row = got["curves"][0]
    assert (row["length"], row["level"], row["first_point"], row["points"], row["closed"]) == (4.0, 0, 0, 9, 1)
    assert got["positions"][0].tobytes() == got["positions"][8].tobytes() and (got["positions"][:, 2] == 0.5).all()
    assert got["arc"].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    assert row["min_temperature"] == got["temperature"].min() and row["max_temperature"] == got["temperature"].max()
    # the segment that starts at a point lies in that point's face; consecutive faces differ
    assert (got["face"][:-1] != np.roll(got["face"][:-1], 1)).all() and got["face"][-1] == got["face"][-2]


def test_a_vertex_on_the_level_is_high_so_the_bottom_has_no_curve_and_the_top_has_one():
    got = _cube([0.0, 1.0])
    assert got["counts"].tolist() == [8, 1, 9, 1, 12] and got["curves"]["level"].tolist() == [1]
    assert got["curves"]["length"].tolist() == [4.0] and (got["positions"][:, 2] == 1.0).all()


def test_three_levels_along_x_give_three_closed_loops_of_length_four():
    got = _cube([0.25, 0.5, 0.75], normal=(1.0, 0.0, 0.0))
    assert got["counts"][:4].tolist() == [24, 3, 27, 3]
    assert got["curves"]["length"].tolist() == [4.0, 4.0, 4.0] and sorted(got["curves"]["level"].tolist()) == [0, 1, 2]
    assert got["curves"]["first_point"].tolist() == [0, 9, 18]
    for q, row in enumerate(got["curves"]):
        assert (got["positions"][9 * q:9 * q + 9, 0] == [0.25, 0.5, 0.75][row["level"]]).all()


def test_one_flipped_face_breaks_the_loop_into_two_open_curves_that_sum_to_four():
    tri = R.cube()[1].copy()
    tri[4] = tri[4][::-1]
    assert R.half_edges(tri, 8)["counts"].tolist() == [18, 0, 0, 3]
    got = _cube([0.5], tri=tri)
    assert got["counts"][:4].tolist() == [8, 2, 10, 0] and got["curves"]["closed"].tolist() == [0, 0]
    assert float(got["curves"]["length"].sum()) == 4.0 and sorted(got["curves"]["points"].tolist()) == [2, 8]


def test_a_vertex_with_nan_degrees_opens_the_curve_around_it():
    temp = np.linspace(18.0, 25.0, 8).astype(F)
    temp[0] = np.nan
    got = _cube([0.5], temp=temp)
    usable = int(got["counts"][4])
    assert usable == 12 - int((R.cube()[1] == 0).any(axis=1).sum())
    assert got["counts"][3] == 0 and got["counts"][1] >= 1 and got["counts"][0] < 8
    assert np.isfinite(got["temperature"]).all() and float(got["curves"]["length"].sum()) < 4.0


def test_header_ctypes_table_and_library_agree_on_the_new_entries():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_hip.lib_path())
    for name in ("tn_mesh_half_edges", "tn_mesh_half_edges_workspace_bytes", "tn_mesh_isolines", "tn_mesh_isolines_workspace_bytes"):
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert len(_hip.SIGNATURES["tn_mesh_half_edges"][1]) == 8 and len(_hip.SIGNATURES["tn_mesh_isolines"][1]) == 18
    assert ctypes.sizeof(_hip.tn_mesh_curve) == 40 == CURVE_DTYPE.itemsize == R.CURVE_DTYPE.itemsize
    assert ctypes.sizeof(_hip.tn_isoline_params) == 24 + 8 + 256 * 8
    assert [n for n, _ in _hip.tn_mesh_curve._fields_] == list(CURVE_DTYPE.names) == list(R.CURVE_DTYPE.names)
    for (name, kind), (_, (dtype, offset)) in zip(_hip.tn_mesh_curve._fields_, sorted(CURVE_DTYPE.fields.items(), key=lambda f: f[1][1])):
        assert getattr(_hip.tn_mesh_curve, name).offset == offset and ctypes.sizeof(kind) == dtype.itemsize
    # the size functions run without a device; the error codes that come before any launch too
    assert lib.tn_mesh_half_edges_workspace_bytes(-1, 0) == 0 and _hip.load().tn_mesh_half_edges_workspace_bytes(8, 12) > 0
    load = _hip.load()
    assert load.tn_mesh_isolines_workspace_bytes(8, 12, 0) > 0 and load.tn_mesh_isolines_workspace_bytes(8, 12, 2 ** 30 + 1) == 0
    assert load.tn_mesh_isolines_workspace_bytes(8, 12, 64) > load.tn_mesh_isolines_workspace_bytes(8, 12, 0)
    assert load.tn_mesh_isolines(*([None] * 3), 8, 12, None, None, None, *([None] * 5), 0, None, None, 0, None) == -1


def test_write_curves_ply_round_trips(tmp_path):
    got = _cube([0.25, 0.75])
    curves = types.SimpleNamespace(curves=got["curves"], positions=got["positions"], temperature=got["temperature"])
    path = write_curves_ply(tmp_path / "sub" / "curves.ply", curves, (12.0, 30.5))
    blob = path.read_bytes()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    assert blob[:end].decode("ascii").split("\n") == [
        "ply", "format binary_little_endian 1.0", "comment temperature_unit celsius", "comment temperature_bounds 12.0 30.5",
        "element vertex 18", "property float x", "property float y", "property float z", "property float temperature",
        "element edge 16", "property int vertex1", "property int vertex2", "end_header", ""]
    vertex = np.frombuffer(blob, dtype=np.dtype([("p", "<f4", (3,)), ("t", "<f4")]), count=18, offset=end)
    assert vertex["p"].tobytes() == got["positions"].tobytes() and vertex["t"].tobytes() == got["temperature"].tobytes()
    edge = np.frombuffer(blob, dtype="<i4", offset=end + 18 * 16).reshape(16, 2)
    assert edge[:, 0].tolist() == list(range(8)) + list(range(9, 17)) and (edge[:, 1] == edge[:, 0] + 1).all()
    assert len(blob) == end + 18 * 16 + 16 * 8
    assert write_curves_ply(tmp_path / "again.ply", curves, (12.0, 30.5)).read_bytes() == blob
    empty = types.SimpleNamespace(curves=got["curves"][:0], positions=got["positions"][:0], temperature=got["temperature"][:0])
    assert b"element vertex 0\n" in write_curves_ply(tmp_path / "empty.ply", empty).read_bytes()
    with pytest.raises(ValueError):
        write_curves_ply(tmp_path / "bad.ply", types.SimpleNamespace(curves=got["curves"], positions=got["positions"][:5],
                                                                     temperature=got["temperature"][:5]))


def _tool():
    import importlib.util

    spec = importlib.util.spec_from_file_location("mesh_isolines_tool", os.path.join(ROOT, "tools", "mesh_isolines.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_tools_arguments_levels_report_and_profile(tmp_path):
    import torch

    tool = _tool()
    for bad in (["m.ply"], ["m.ply", "--plane", "0", "0", "1"], ["m.ply", "--offsets", "1"], ["m.ply", "--plane", "0", "0", "0", "--offsets", "1"],
                ["m.ply", "--isotherms", "18", "--isotherm-step", "1"], ["m.ply", "--isotherm-step", "0"], ["m.ply", "--isotherms", "nan"],
                ["m.ply", "--isotherms", "18", "--length-scale", "-1"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    assert tool.parse(["m.ply", "--isotherms", "22", "18", "22"]).isotherms == [18.0, 22.0]
    assert tool.step_levels(np.array([17.2, np.nan, 20.0], F), 1.0) == [18.0, 19.0, 20.0] and tool.step_levels(np.array([np.nan], F), 1.0) == []
    got = _cube([0.25, 0.75])
    found = types.SimpleNamespace(curves=got["curves"], levels=(0.25, 0.75), positions=torch.from_numpy(got["positions"]),
                                  temperature=torch.from_numpy(got["temperature"]), arc=torch.from_numpy(got["arc"]),
                                  num_segments=16, num_curves=2, num_points=18, closed_curves=2, usable_faces=12)
    edges = types.SimpleNamespace(edges=18, boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, closed_manifold=True)
    report = tool.build_report(found, edges, 2.0, "cube.ply", {"plane": [0.0, 0.0, 1.0], "offsets": [0.25, 0.75]})
    assert report["edges"] == {"edges": 18, "boundary": 0, "nonmanifold": 0, "inconsistent": 0, "closed_manifold": True}
    assert [(r["level"], r["value"], r["closed"], r["points"], r["length"]) for r in report["curves"]] == \
        [(int(w["level"]), (0.25, 0.75)[w["level"]], True, 9, 8.0) for w in got["curves"]]
    assert [(r["curves"], r["closed_curves"], r["length"]) for r in report["levels"]] == [(1, 1, 8.0), (1, 1, 8.0)]
    by_level = {int(w["level"]): float(w["mean_temperature"]) for w in got["curves"]}
    assert [r["mean_temperature"] for r in report["levels"]] == [4.0 * by_level[0] / 4.0, 4.0 * by_level[1] / 4.0]
    assert len(tool.curve_lines(report)) == 2 and all("closed" in line and "length 8" in line for line in tool.curve_lines(report))
    tool.write_profile(tmp_path / "out" / "cut.csv", found, 2.0)
    rows = (tmp_path / "out" / "cut.csv").read_text().splitlines()
    assert rows[0] == "curve,level,arc,x,y,z,temperature" and len(rows) == 19
    first = rows[1].split(",")
    assert first[0] == "0" and float(first[2]) == 0.0 and float(first[6]) == float(got["temperature"][0])
    assert [float(r.split(",")[2]) for r in rows[1:]] == (2.0 * got["arc"]).tolist()
