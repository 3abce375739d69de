"""The yardstick of the mesh simplification kernel (tests/mesh_simplify_reference.py) checked on its own — the literal cases, a
brute-force cross-check on random meshes, what clustering does to the sphere mesh — and the host side of the feature: the command
line, the refusals of the Python layer, the declarations and the error codes that need no device.  No GPU."""
from __future__ import annotations

import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_reference
from tests import mesh_simplify_reference as R
from tests.mesh_components_reference import random_mesh
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (SimplifyInfo, ThermalMesh, mesh_simplify_into, mesh_simplify_workspace_bytes, simplify_mesh,
                                    voxel_grid, voxel_params)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference against its literal cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_yardstick_on_the_literal_cases(name):
    case = R.LITERAL[name]
    got = R.simplify(*R.literal_arrays(case), **R.GRID)
    want = R.literal_want(case)
    assert R.same(got, want) is None, R.same(got, want)
    for key, w in want.items():
        assert w is None or got[key].dtype == w.dtype, key
    assert int(got["counts"][1:].sum()) == len(case["triangles"])


def test_literal_cases_are_the_ones_the_feature_is_defined_by():
    c = {k: R.LITERAL[k]["want"] for k in R.LITERAL}
    assert c["four_cells"]["counts"] == [4, 2, 0, 0] and c["four_cells"]["cluster_count"] == [1, 1, 1, 1]
    assert c["quad_strip"]["counts"][2] == 1 and 2 in c["quad_strip"]["cluster_count"]
    assert c["rotated_and_opposite"]["counts"] == [3, 2, 0, 1] and c["rotated_and_opposite"]["triangle_source"] == [0, 2]
    assert c["island_in_one_cell"]["vertex_map"][:4] == [-1] * 4 and c["island_in_one_cell"]["counts"][2] == 4
    assert c["unreferenced_member"]["cluster_count"][0] == 2 and c["unreferenced_member"]["colors"][0] == [128, 128, 128]


def test_canonical_rotation_keeps_the_orientation():
    assert R.canonical(5, 7, 2) == R.canonical(7, 2, 5) == R.canonical(2, 5, 7) == (2, 5, 7)
    assert R.canonical(7, 5, 2) == R.canonical(2, 7, 5) == (2, 7, 5) != R.canonical(5, 7, 2)


# ---- the brute-force cross-check -------------------------------------------------------------------------------------------------------

def test_yardstick_equals_a_brute_force_search_on_random_meshes():
    rng = np.random.default_rng(11)
    duplicates = dropped = unused = multi = 0
    for seed in range(150):
        v = int(rng.integers(1, 80))
        t = int(rng.integers(0, 3 * v + 2))
        pos = R.random_positions(seed, v, extent=4.0, bad=0.08)
        tri = random_mesh(seed, v, t, invalid=0.1) if t else np.zeros((0, 3), np.int32)
        colors, temperature, thermal = R.random_attributes(seed, v, thermal=bool(seed % 2))
        size = float(rng.choice([0.5, 1.0, 1.7]))
        dims = (int(4.0 / size) + 1,) * 3
        got = R.simplify(pos, colors, temperature, thermal, tri, (0.0, 0.0, 0.0), size, dims)
        source, vertex_map, cluster_count, counts = R.brute_force(pos, tri, (0.0, 0.0, 0.0), size, dims)
        assert np.array_equal(got["triangle_source"], source) and np.array_equal(got["vertex_map"], vertex_map), seed
        assert np.array_equal(got["cluster_count"], cluster_count) and np.array_equal(got["counts"], counts), seed
        assert int(counts[1:].sum()) == t
        # every output triangle has three different vertices in range, every output vertex is in a triangle
        out = got["triangles"]
        assert out.shape == (counts[1], 3) and (len(out) == 0 or (0 <= out.min() and out.max() < counts[0]))
        assert all(len(set(row)) == 3 for row in out.tolist()) and set(out.reshape(-1).tolist()) == set(range(int(counts[0])))
        # the corners are the input's, mapped
        assert np.array_equal(out, vertex_map[tri[source]].reshape(-1, 3))
        # a mean lies within its members' range
        for k in range(int(counts[0])):
            rows = np.flatnonzero(vertex_map == k)
            assert len(rows) == cluster_count[k]
            assert (pos[rows].min(axis=0) <= got["positions"][k]).all() and (got["positions"][k] <= pos[rows].max(axis=0)).all()
            assert temperature[rows].min() <= got["temperature"][k] <= temperature[rows].max()
        duplicates, dropped = duplicates + int(counts[3]), dropped + int(counts[2])
        unused += int(((vertex_map < 0) & np.array([k is not None for k in R.cell_keys(pos, (0.0, 0.0, 0.0), size, dims)])).sum())
        multi += int((cluster_count > 1).sum())
    assert duplicates > 50 and dropped > 500 and unused > 100 and multi > 300, (duplicates, dropped, unused, multi)


def test_sphere_mesh_clustered_at_two_grid_steps():
    mesh = mesh_reference.sphere_mesh()[1]
    pos, tri = mesh["positions"], mesh["triangles"]
    colors, temperature, thermal = R.random_attributes(3, len(pos))
    step = 1.0 / 23.0
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    origin, dims = voxel_grid(lo.tolist(), hi.tolist(), 2 * step)
    got = R.simplify(pos, colors, mesh["temperature"], thermal, tri, origin, 2 * step, dims)
    m, k, dropped, duplicate = (int(c) for c in got["counts"])
    print(f"sphere mesh at two grid steps: vertices {len(pos)} -> {m}, triangles {len(tri)} -> {k} (degenerate {dropped}, duplicate {duplicate})")
    assert k + dropped + duplicate == len(tri) and 0 < m < len(pos) // 2 and 0 < k < len(tri) // 2
    radius = np.linalg.norm(got["positions"].astype(np.float64), axis=1)
    assert 0.2 < radius.min() and radius.max() < 0.35, "the clustered vertices still lie on the sphere of radius 0.3"
    assert int(got["cluster_count"].sum()) == len(pos), "the sphere has no unreferenced vertex and no unused cell"


# ---- the Python layer's refusals (nothing here reaches a kernel) ----------------------------------------------------------------------

def test_python_layer_refuses_bad_cell_sizes_missing_triangles_and_host_tensors():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="cell_size"):
            simplify_mesh(mesh, bad)
    with pytest.raises(ValueError, match="no triangles"):
        simplify_mesh(ThermalMesh(pos, mesh.colors, mesh.temperature), 1.0)
    with pytest.raises(ValueError, match="no triangles"):
        mesh_simplify_into(ThermalMesh(pos, mesh.colors, mesh.temperature), voxel_params((0, 0, 0), 1.0, (1, 1, 1)), counts=None)
    for call in (lambda: simplify_mesh(mesh, 1.0),
                 lambda: mesh_simplify_into(mesh, voxel_params((0, 0, 0), 1.0, (1, 1, 1)), counts=torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="2\\^21"):
        voxel_grid((0.0, 0.0, 0.0), (1.0, 1.0, 3.0), 1e-6)
    assert [f.name for f in __import__("dataclasses").fields(SimplifyInfo)] == [
        "vertices_before", "triangles_before", "vertices_after", "triangles_after", "degenerate_triangles", "duplicate_triangles",
        "cluster_count"]


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_export_mesh_parses_the_simplify_flag_and_it_defaults_to_off(capsys):
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(ROOT, "tools", "export_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["run", "data", "--output", "mesh.ply"]
    assert tool.parse(base).simplify_cell_size == 0.0
    assert tool.parse(base + ["--simplify-cell-size", "0.05"]).simplify_cell_size == 0.05
    assert tool.parse(base + ["--simplify-cell-size", "0"]).simplify_cell_size == 0.0
    for bad in ("-0.1", "nan", "inf", "-inf"):
        with pytest.raises(SystemExit):
            tool.parse(base + [f"--simplify-cell-size={bad}"])
        assert "--simplify-cell-size" in capsys.readouterr().err, bad
    assert "--simplify-cell-size" in tool.__doc__


# ---- the declarations ------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_and_refuse_bad_arguments_before_any_launch():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bsize_t tn_mesh_simplify_workspace_bytes\(int64_t num_vertices, int64_t num_triangles\);", header)
    assert re.search(r"\bint tn_mesh_simplify\(const float \*positions, const uint8_t \*colors, const float \*temperature", header)
    assert len(_hip.SIGNATURES["tn_mesh_simplify"][1]) == 22 and len(_hip.SIGNATURES["tn_mesh_simplify_workspace_bytes"][1]) == 2
    assert "tn_mesh_simplify.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    lib = _hip.load()
    v, t = 1000, 2000
    need = mesh_simplify_workspace_bytes(v, t)
    limit = (2 ** 31 - 1) // 3
    assert need > 0 and need % 8 == 0 and mesh_simplify_workspace_bytes(0, 0) >= 0
    assert mesh_simplify_workspace_bytes(2 ** 31 - 1, limit) > 0
    for bad in ((-1, t), (v, -1), (2 ** 31, t), (v, limit + 1)):
        assert mesh_simplify_workspace_bytes(*bad) == 0, bad
    # one sort of the triples below 2^21 vertices, two from there on: two more key arrays and one more index array per triangle
    below, above = mesh_simplify_workspace_bytes(2 ** 21 - 1, t), mesh_simplify_workspace_bytes(2 ** 21, t)
    # (and what one more vertex costs: under 4 KiB, a tile of the sort's counts included)
    assert 0 <= above - below - (2 * 8 * t + 4 * t) < 4096, (below, above)
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy = 4096
    names = ("positions", "colors", "temperature", "thermal_colors", "triangles", "num_vertices", "num_triangles", "params",
             "positions_out", "colors_out", "temperature_out", "thermal_colors_out", "cluster_count", "capacity_vertices",
             "triangles_out", "triangle_source", "capacity_triangles", "vertex_map", "counts", "workspace", "workspace_bytes", "stream")
    params = voxel_params((0.0, 0.0, 0.0), 1.0, (4, 4, 4))
    good = dict(zip(names, [dummy] * 5 + [v, t, params] + [dummy] * 5 + [v, dummy, dummy, t, dummy, dummy, dummy, need, None]))

    def call(**change):
        args = dict(good, **change)
        p = args["params"]
        return lib.tn_mesh_simplify(*[(None if p is None else __import__("ctypes").byref(p)) if k == "params" else args[k] for k in names])

    for k in ("positions", "colors", "temperature", "triangles", "params", "positions_out", "colors_out", "temperature_out",
              "cluster_count", "triangles_out", "counts", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    assert call(thermal_colors=None) == -1  # thermal_colors_out without thermal_colors
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2
    assert call(num_triangles=limit + 1, workspace_bytes=2 ** 60) == -2
    assert call(capacity_vertices=-1) == -2 and call(capacity_triangles=-1) == -2
    for k in ("positions", "temperature", "triangles", "positions_out", "temperature_out", "cluster_count", "triangles_out",
              "triangle_source", "vertex_map"):
        assert call(**{k: dummy + 2}) == -2, k  # TN_ERR_SHAPE
    assert call(counts=dummy + 4) == -2 and call(workspace=dummy + 4) == -2
    assert call(colors=dummy + 1, colors_out=dummy + 3, thermal_colors=dummy + 1, thermal_colors_out=dummy + 1, workspace_bytes=0) == -4
    for bad in (voxel_params((0, 0, 0), 0.0, (4, 4, 4)), voxel_params((0, 0, 0), float("nan"), (4, 4, 4)),
                voxel_params((0, 0, 0), float("inf"), (4, 4, 4)), voxel_params((0, 0, 0), 1.0, (0, 4, 4)),
                voxel_params((0, 0, 0), 1.0, (4, 4, 2 ** 21 + 1))):
        assert call(params=bad) == -3  # TN_ERR_UNSUPPORTED
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    # what may be absent: the optional outputs, and outputs with a capacity of 0 (checked up to the workspace's size)
    assert call(thermal_colors_out=None, triangle_source=None, vertex_map=None, workspace_bytes=0) == -4
    assert call(positions_out=None, colors_out=None, temperature_out=None, cluster_count=None, thermal_colors_out=None,
                capacity_vertices=0, triangles_out=None, capacity_triangles=0, workspace_bytes=0) == -4
