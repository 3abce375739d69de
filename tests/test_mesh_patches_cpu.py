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
    # the grouped sums, the two lists and the face loader of regions and patches are tn_group_sum.h's, and the small host helpers
    # tn_device.h's: no source carries a copy
    assert " tn_group_sum.h " in makefile
    for source in ("tn_mesh_regions.hip", "tn_mesh_patches.hip"):
        code = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", source)).read()
        assert '#include "tn_group_sum.h"' in code and "group_sum(" in code, source
        assert "total_blocks_kernel(" not in code and "block_sums_kernel(" not in code, source
    shared = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_group_sum.h")).read()
    assert "total_blocks_kernel(" in shared and "block_sums_kernel(" in shared and "Face load_face(" in shared
    csrc = os.path.join(ROOT, "thermo_nerf_amd", "csrc")
    holders = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".h")) and "ints_bytes(long long" in open(os.path.join(csrc, n)).read())
    assert holders == ["tn_device.h"]
    # the size function runs without a device; the error codes that come before any launch too
    load = _hip.load()
    assert lib.tn_mesh_patches_workspace_bytes(-1, 0) == 0 and load.tn_mesh_patches_workspace_bytes(8, 2 ** 30) == 0
    assert load.tn_mesh_patches_workspace_bytes(8, 12) > 0
    assert load.tn_mesh_patches(None, None, None, 8, 12, None, 0.5, None, 0, None, None, None, None, 0, None) == -1


def test_workspace_sizes_against_those_of_the_separate_implementations():
    """(V, T) -> the bytes the two entries asked for while each carried its own grouped sum: patches asks for exactly as much, regions
    (which lost its three arrays of vertex-tile counts and keeps its T / 256 + min(V / 3, T) partials) for no more"""
    before = {(8, 12): (5080, 4408), (300, 257): (60312, 56304), (110162, 220320): (49841528, 39268464),
              (1048576, 2097152): (474415136, 373773688)}
    load = _hip.load()
    for (v, t), (patches, regions) in before.items():
        assert load.tn_mesh_patches_workspace_bytes(v, t) == patches, (v, t)
        assert 0 < load.tn_mesh_regions_workspace_bytes(v, t) <= regions, (v, t)
    # many more faces than vertices: the bound on the partials falls back on the regions the vertices allow
    assert 0 < load.tn_mesh_regions_workspace_bytes(8, 2 ** 20) <= 160973200


def test_the_bench_tool_finds_every_kernel_of_the_call_under_the_name_a_trace_gives_it():
    """tools/mesh_patches_bench.py matches traced kernel names whole: the kernels of tn_mesh_patches.hip and of tn_group_sum.h, as a
    trace demangles them, are the tool's groups without the sort's three"""
    import importlib.util
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        spec = importlib.util.spec_from_file_location("mesh_patches_bench_tool", os.path.join(ROOT, "tools", "mesh_patches_bench.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    traced = ["(anonymous namespace)::scan_faces_kernel(tn::FaceLists, long long)",
              "(anonymous namespace)::total_blocks_kernel(tn::FaceLists, long long, char const*, long long, long long, double*)",
              "(anonymous namespace)::count_heads_kernel(tn::Groups, long long*)",
              "(anonymous namespace)::rows_kernel(tn::Groups, (anonymous namespace)::Acc const*, (anonymous namespace)::Acc const*, long long, tn_mesh_patch*)",
              "void (anonymous namespace)::block_sums_kernel<(anonymous namespace)::Acc>(tn::Groups, long long, (anonymous namespace)::Acc const*, (anonymous namespace)::Acc*)",
              "void (anonymous namespace)::block_sums_kernel<(anonymous namespace)::Dev>(tn::Groups, long long, (anonymous namespace)::Dev const*, (anonymous namespace)::Dev*)"]
    assert [tool.short_name(n) for n in traced] == ["scan_faces_kernel", "total_blocks_kernel", "count_heads_kernel", "rows_kernel",
                                                    "block_sums_kernel<Acc>", "block_sums_kernel<Dev>"]
    assert all(tool.short_name(n) in tool.GROUP_OF for n in traced)
    # every kernel the two files define, under the name the tool lists; a kernel in a named namespace or a template over the record
    # where the tool lists a plain name would drop out of the shares without an error
    csrc = os.path.join(ROOT, "thermo_nerf_amd", "csrc")
    shared, own = open(os.path.join(csrc, "tn_group_sum.h")).read(), open(os.path.join(csrc, "tn_mesh_patches.hip")).read()
    kernels = re.compile(r"(template <typename R>\n)?__global__ void (?:__launch_bounds__\(\w+\)\s+)?(\w+)\(")
    assert "static __global__" not in shared and shared.index("\nnamespace {\n") < shared.index("__global__ void") < shared.index("\n}  // namespace\n")
    named = set()
    for template, name in kernels.findall(shared) + kernels.findall(own):
        named |= {name + "<Acc>", name + "<Dev>"} if template else {name}
    assert named == set(tool.GROUP_OF) - {"histogram_kernel", "scatter_kernel", "scan_kernel"}, named ^ set(tool.GROUP_OF)
