"""The yardstick of the planar patches (tests/mesh_patches_reference.py) against closed forms, the row's layout against the header as
a C++ compiler lays it out, the new entries in header, ctypes table and library, and the refusals that need no device.  No GPU."""
from __future__ import annotations

import ctypes
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import mesh_patches_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import PATCH_BYTES, PATCH_DTYPE, mesh_patches_into, order_regions, planar_patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
COS10 = math.cos(math.radians(10.0))


def _patches(pos, tri, min_cos, temp=None):
    temp = np.linspace(18.0, 25.0, len(pos)).astype(F) if temp is None else temp
    return R.patches(pos, temp, tri, R.half_edges(tri, len(pos))["twin"], min_cos)


def test_sum2_fast_is_sum2():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 255, 256, 257, 513, 70000):
        x = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
        assert R.bits(np.array([R.sum2_fast(x)])) == R.bits(np.array([R.sum2(x)])), n
    assert math.copysign(1.0, R.sum2_fast([-0.0])) == 1.0 == math.copysign(1.0, R.sum2([-0.0]))


def test_the_unit_cube_at_ten_degrees_is_six_sides_of_area_one():
    pos, tri = R.cube()
    got = _patches(pos, tri, COS10)
    table = got["patches"]
    assert got["counts"].tolist() == [6, 12, 12] and got["totals"].tolist() == [6.0, 6.0]
    assert got["face_patch"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and table["label"].tolist() == [0, 2, 4, 6, 8, 10]
    assert table["area"].tolist() == [1.0] * 6 and table["flatness"].tolist() == [1.0] * 6 and table["faces"].tolist() == [2] * 6
    assert table["rms_deviation"].tolist() == [0.0] * 6 and table["max_deviation"].tolist() == [0.0] * 6
    # -x +x -y +y -z +z, outward: the plane passes through the side
    assert table["plane"].tolist() == [[-1, 0, 0, 0], [1, 0, 0, 1], [0, -1, 0, 0], [0, 1, 0, 1], [0, 0, -1, 0], [0, 0, 1, 1]]
    assert table["centroid"][1].tolist() == [1.0, 0.5, 0.5] and table["bounds"][1].tolist() == [1, 0, 0, 1, 1, 1]
    assert table["thermal_area"].tolist() == [1.0] * 6 and table["thermal_faces"].tolist() == [2] * 6 and not table["reserved"].any()


def test_the_cube_at_180_degrees_is_one_closed_patch_of_flatness_zero():
    pos, tri = R.cube()
    got = _patches(pos, tri, -1.0)
    row = got["patches"][0]
    assert got["counts"].tolist() == [1, 12, 36] and (got["face_patch"] == 0).all()
    assert row["area"] == 6.0 and row["flatness"] == 0.0 and row["plane"].tolist() == [0.0] * 4 and row["faces"] == 12
    assert R.bits(np.array([row["rms_deviation"], row["max_deviation"]], F)).tolist() == [R.NAN_BITS] * 2
    assert row["centroid"].tolist() == [0.5, 0.5, 0.5]


def test_one_triangle_lies_in_its_own_plane_exactly():
    pos, tri = np.array([(0, 0, 2), (1, 0, 2), (0, 1, 2)], F), np.array([(0, 1, 2)], np.int32)
    got = _patches(pos, tri, COS10, temp=np.array([18, 21, 24], F))
    row = got["patches"][0]
    assert got["counts"].tolist() == [1, 1, 0] and got["totals"].tolist() == [0.5, 0.5]
    assert row["area"] == 0.5 and row["flatness"] == 1.0 and row["plane"].tolist() == [0.0, 0.0, 1.0, 2.0]
    assert row["rms_deviation"] == 0.0 and row["max_deviation"] == 0.0
    assert (row["mean_temperature"], row["min_temperature"], row["max_temperature"]) == (21.0, 21.0, 21.0)


def test_a_tilted_rectangle_and_a_ridge_of_two_about_hand_computed_planes():
    # the rectangle spanned by (4, 0, 3) and (0, 1, 0): area 5, normal (-3, 0, 4) / 5, through the origin
    pos, tri = R.rectangle((0, 0, 0), (4, 0, 3), (0, 1, 0))
    row = _patches(pos, tri, COS10)["patches"][0]
    assert row["area"] == 5.0 and row["flatness"] == 1.0 and row["faces"] == 2
    assert np.allclose(row["plane"], [-0.6, 0.0, 0.8, 0.0], rtol=0, atol=1e-15) and row["rms_deviation"] < 1e-15 and row["max_deviation"] < 1e-15
    # up that rectangle and down its mirror image: at 10 degrees two patches; at 180 one of area 10 whose vector area is (0, 0, 8) —
    # the plane z = 3 / 2, flatness 8 / 10, every corner 3 / 2 from it, and the mean squared distance of a ramp of height 3 is 9 / 12
    pos, tri = R.weld(*R.join_meshes(R.rectangle((0, 0, 0), (4, 0, 3), (0, 1, 0)), R.rectangle((4, 0, 3), (4, 0, -3), (0, 1, 0))))
    assert len(pos) == 6 and _patches(pos, tri, COS10)["counts"].tolist() == [2, 4, 4]
    got = _patches(pos, tri, -1.0)
    row = got["patches"][0]
    assert got["counts"].tolist() == [1, 4, 6] and row["area"] == 10.0 and row["plane"].tolist() == [0.0, 0.0, 1.0, 1.5]
    assert row["flatness"] == F(0.8) and row["max_deviation"] == 1.5 and row["rms_deviation"] == F(math.sqrt(0.75))
    assert row["centroid"].tolist() == [4.0, 0.5, 1.5]


def test_a_nan_temperature_stays_in_the_wall_and_out_of_the_mean():
    pos, tri = R.rectangle((0, 0, 0), (1, 0, 0), (0, 1, 0))
    got = _patches(pos, tri, COS10, temp=np.array([20, np.nan, 26, 29], F))  # face 0 names vertex 1, face 1 does not
    row = got["patches"][0]
    assert got["counts"].tolist() == [1, 2, 2] and got["totals"].tolist() == [1.0, 0.5]
    assert (row["area"], row["thermal_area"], row["faces"], row["thermal_faces"]) == (1.0, 0.5, 2, 1)
    assert (row["mean_temperature"], row["min_temperature"], row["max_temperature"]) == (25.0, 25.0, 25.0)
    cold = _patches(pos, tri, COS10, temp=np.full(4, np.nan, F))["patches"][0]
    assert R.bits(np.array([cold[n] for n in ("mean_temperature", "min_temperature", "max_temperature")], F)).tolist() == [R.NAN_BITS] * 3


def test_the_threshold_is_the_dot_product_itself():
    pos, tri = R.ell()
    assert _patches(pos, tri, 0.0)["counts"].tolist() == [1, 4, 6]
    assert _patches(pos, tri, float(np.nextafter(0.0, 1.0)))["counts"].tolist() == [2, 4, 4]


def test_order_regions_takes_the_patch_table():
    table = np.zeros(5, PATCH_DTYPE)
    table["area"], table["label"] = [2.0, 5.0, 2.0, 0.0, 0.5], [9, 4, 1, 0, 7]
    assert order_regions(table).tolist() == [1, 2, 0, 4] and order_regions(table, min_area=1.0, top=2).tolist() == [1, 2]
    assert order_regions(table[:0]).tolist() == []


def test_refusals_before_anything_runs():
    mesh = types.SimpleNamespace(triangles=object())
    for angle in (-0.001, 180.001, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_angle_degrees"):
            planar_patches(mesh, angle)
    with pytest.raises(ValueError, match="no triangles"):
        planar_patches(types.SimpleNamespace(triangles=None))
    for min_cos in (math.nan, 1.0000001, -1.5):
        with pytest.raises(ValueError, match="min_cos"):
            mesh_patches_into(mesh, None, min_cos, counts=None, totals=None)
    # the type and the length of twin, against a mesh of 12 faces, before any check that needs a device
    import torch

    mesh = types.SimpleNamespace(triangles=torch.zeros((12, 3), dtype=torch.int32))
    for twin in (None, np.zeros(36, np.int32), torch.zeros(36, dtype=torch.int64), torch.zeros(36, dtype=torch.float32)):
        with pytest.raises(TypeError, match="twin"):
            mesh_patches_into(mesh, twin, 0.5, counts=None, totals=None)
    for length in (0, 35, 37, 12):
        with pytest.raises(ValueError, match="3 T"):
            mesh_patches_into(mesh, torch.zeros(length, dtype=torch.int32), 0.5, counts=None, totals=None)


def test_the_row_is_136_bytes_laid_out_as_the_header_says(tmp_path):
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "a C++ compiler is needed for the layout probe"
    names = list(PATCH_DTYPE.names)
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include <cstddef>\n#include <cstdio>\n#include "thermonerf_hip.h"\nint main() {\n'
                     '    std::printf("%zu", sizeof(tn_mesh_patch));\n' +
                     "".join(f'    std::printf(" %zu", offsetof(tn_mesh_patch, {n}));\n' for n in names) + "    return 0;\n}\n")
    subprocess.run([compiler, "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(tmp_path / "probe")], check=True)
    size, *offsets = (int(x) for x in subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout.split())
    assert size == 136 == PATCH_DTYPE.itemsize == PATCH_BYTES == R.PATCH_DTYPE.itemsize == ctypes.sizeof(_hip.tn_mesh_patch)
    assert offsets == [PATCH_DTYPE.fields[n][1] for n in names] == [getattr(_hip.tn_mesh_patch, n).offset for n in names]
    assert names == [n for n, _ in _hip.tn_mesh_patch._fields_] == list(R.PATCH_DTYPE.names)
    assert PATCH_DTYPE == R.PATCH_DTYPE


def test_header_makefile_ctypes_table_and_library_agree_on_the_new_entries():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_hip.lib_path())
    for name in ("tn_mesh_patches", "tn_mesh_patches_workspace_bytes"):
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert len(_hip.SIGNATURES["tn_mesh_patches"][1]) == 15
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert " tn_mesh_patches.hip " in makefile and " tn_union_find.h " in makefile
    shared = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_union_find.h")).read()
    for source in ("tn_mesh_components.hip", "tn_mesh_patches.hip"):
        code = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", source)).read()
        assert '#include "tn_union_find.h"' in code and "unite(" in code and "int find_root(" not in code, source
    assert "int find_root(" in shared and "void unite(" in shared and "int load_parent(" in shared
    # the size function runs without a device; the error codes that come before any launch too
    load = _hip.load()
    assert lib.tn_mesh_patches_workspace_bytes(-1, 0) == 0 and load.tn_mesh_patches_workspace_bytes(8, 2 ** 30) == 0
    assert load.tn_mesh_patches_workspace_bytes(8, 12) > 0
    assert load.tn_mesh_patches(None, None, None, 8, 12, None, 0.5, None, 0, None, None, None, None, 0, None) == -1
