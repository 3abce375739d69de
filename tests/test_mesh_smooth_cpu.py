"""The yardstick of the mesh normals / smoothing kernels (tests/mesh_smooth_reference.py) checked on its own — literal cases, the
incidence index against a brute-force search, what Taubin smoothing does to the analytic sphere — and the host side of the feature:
PLY layouts, ``ThermalMesh``, the command line, the declarations.  No GPU."""
from __future__ import annotations

import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_reference
from tests import mesh_smooth_reference as R
from tests.mesh_components_reference import random_mesh
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (MeshIncidence, ThermalMesh, mesh_incidence, mesh_incidence_workspace_bytes, read_mesh_ply,
                                    smooth_mesh, smooth_positions, vertex_normals, write_mesh_ply)
from thermo_nerf_amd.export import ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference against its literal cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_yardstick_on_the_literal_cases(name):
    case = R.LITERAL[name]
    pos, tri = R.literal_arrays(case)
    index = R.incidence(tri, len(pos))
    assert index["offsets"].dtype == np.int32 and index["offsets"].tolist() == case["offsets"]
    assert index["corners"].dtype == np.int32 and index["corners"].tolist() == case["corners"]
    assert R.bits(R.vertex_normals(pos, tri, index)).tolist() == case["normals"]
    assert R.bits(R.smooth_pass(pos, tri, index, 0.5)).tolist() == case["pass_half"]
    assert R.bits(R.smooth(pos, tri, index, 0, 0.5, -0.53)).tolist() == R.bits(pos).tolist()
    # an iteration is a pass with lambda, then a pass with mu
    want = R.smooth_pass(R.smooth_pass(pos, tri, index, 0.5), tri, index, -0.53)
    assert np.array_equal(R.bits(R.smooth(pos, tri, index, 1, 0.5, -0.53)), R.bits(want))


def test_the_tetrahedron_normal_is_minus_one_over_root_three_rounded_as_defined():
    n = R.vertex_normals(*R.literal_arrays(R.LITERAL["tetrahedron"]), R.incidence(R.LITERAL["tetrahedron"]["triangles"], 4))
    want = F(-1.0) / np.sqrt(F(3.0))
    assert n[0].tolist() == [want] * 3 and abs(float(want) + 1.0 / np.sqrt(3.0)) < 3e-8


def test_empty_meshes():
    for v, tri in ((0, np.zeros((0, 3), np.int32)), (5, np.zeros((0, 3), np.int32)), (0, np.array([[0, 1, 2]], np.int32))):
        index = R.incidence(tri, v)
        assert index["offsets"].tolist() == [0] * (v + 1) and index["corners"] is None
        pos = R.random_positions(1, v)
        assert not R.vertex_normals(pos, tri, index).any()
        assert np.array_equal(R.smooth(pos, tri, index, 3, 0.5, -0.53), pos)


def test_incidence_equals_a_brute_force_search_on_random_sparse_meshes():
    rng = np.random.default_rng(9)
    longest, invalid_rows = 0, 0
    for seed in range(200):
        v = int(rng.integers(1, 90))
        t = int(rng.integers(1, 2 * v + 2))
        tri = random_mesh(seed, v, t, invalid=0.1)
        index = R.incidence(tri, v)
        offsets, corners = index["offsets"], index["corners"]
        lists = R.brute_force_lists(tri, v)
        assert [corners[offsets[k]:offsets[k + 1]].tolist() for k in range(v)] == lists, seed
        keys = R.corner_keys(tri, v)
        assert corners[offsets[v]:].tolist() == [c for c in range(3 * t) if keys[c] == v], seed  # the invalid ones, ascending
        assert sorted(corners.tolist()) == list(range(3 * t))
        longest, invalid_rows = max(longest, max(len(x) for x in lists)), invalid_rows + 3 * t - int(offsets[v])
    assert longest >= 8 and invalid_rows > 100, "the random meshes have long lists and invalid triangles"


# ---- the analytic sphere ---------------------------------------------------------------------------------------------------------------

def _sphere():
    mesh = mesh_reference.sphere_mesh()[1]
    pos, tri = mesh["positions"], mesh["triangles"]
    assert pos.shape == (910, 3) and tri.shape == (1816, 3)
    return pos, tri, R.incidence(tri, len(pos))


def test_taubin_smoothing_on_the_sphere_mesh():
    """Measured with this reference (printed below; DESIGN.md 5.5e quotes them): mean / max angle between normal and radius 5.372 /
    32.25 degrees unsmoothed, 3.785 / 15.35 after 10 default iterations (ratio 0.704); mean radius 0.29682 -> 0.29741 (+0.200 %);
    20 passes of lambda = 0.5 alone shrink it to 0.27125 (-8.6 %).  The asserted margins sit on the reference's side of these."""
    pos, tri, index = _sphere()
    normals = R.vertex_normals(pos, tri, index)
    assert ((pos * normals).sum(axis=1) > 0).all(), "every normal points outward"
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0, atol=1e-6)
    smoothed = R.smooth(pos, tri, index, 10, 0.5, -0.53)
    smoothed_normals = R.vertex_normals(smoothed, tri, index)
    assert ((smoothed * smoothed_normals).sum(axis=1) > 0).all()
    before, after = R.radial_angles_deg(pos, normals), R.radial_angles_deg(smoothed, smoothed_normals)
    radius = lambda p: float(np.linalg.norm(p.astype(np.float64), axis=1).mean())  # noqa: E731
    r0, r1 = radius(pos), radius(smoothed)
    laplacian = R.smooth(pos, tri, index, 10, 0.5, 0.5)  # through the raw interface: 20 passes of lambda alone
    r2 = radius(laplacian)
    print(f"sphere mesh: angle mean / max {before.mean():.3f} / {before.max():.2f} deg -> {after.mean():.3f} / {after.max():.2f} deg "
          f"(ratio {after.mean() / before.mean():.3f}); mean radius {r0:.5f} -> {r1:.5f} ({(r1 / r0 - 1) * 100:+.3f} %); "
          f"20 lambda passes -> {r2:.5f} ({(r2 / r0 - 1) * 100:+.3f} %)")
    assert after.mean() < 0.75 * before.mean()
    assert abs(r1 / r0 - 1.0) < 0.005
    assert r2 < 0.97 * r0, "plain Laplacian smoothing shrinks the sphere: the mu pass is what keeps the radius"
    # the topology is unchanged: the same triangles, still closed and consistently wound
    topo = mesh_reference.mesh_topology(tri, len(pos))
    assert topo["bad_edges"] == 0 and topo["inconsistent"] == 0 and topo["euler"] == 2 and topo["unused"] == 0
    assert np.isfinite(smoothed).all() and not np.array_equal(smoothed, pos)


# ---- PLY -------------------------------------------------------------------------------------------------------------------------------

def _host_mesh(normals: bool):
    rng = np.random.default_rng(4)
    v, t = 7, 5
    mesh = ThermalMesh(torch.from_numpy(rng.normal(size=(v, 3)).astype(F)), torch.from_numpy(rng.integers(0, 256, (v, 3)).astype(np.uint8)),
                       torch.from_numpy(rng.uniform(14, 33, v).astype(F)), torch.from_numpy(rng.integers(0, 256, (v, 3)).astype(np.uint8)),
                       torch.from_numpy(rng.integers(0, v, (t, 3)).astype(np.int32)), (14.0, 33.0))
    if normals:
        mesh.normals = torch.from_numpy(rng.normal(size=(v, 3)).astype(F))
    return mesh


def test_ply_round_trip_with_normals_is_the_31_byte_vertex(tmp_path):
    mesh = _host_mesh(True)
    path = write_mesh_ply(tmp_path / "n.ply", mesh)
    blob = path.read_bytes()
    head = blob[:blob.index(b"end_header\n")].decode("ascii").split("\n")
    props = [ln for ln in head if ln.startswith("property ")]
    assert props == ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                     "property float nz", "property uchar red", "property uchar green", "property uchar blue", "property float temperature",
                     "property list uchar int vertex_indices"]
    assert len(blob) == blob.index(b"end_header\n") + len(b"end_header\n") + 7 * 31 + 5 * 13
    got = read_mesh_ply(path)
    for key in ("positions", "normals", "colors", "temperature", "triangles"):
        assert got[key].tobytes() == getattr(mesh, key).numpy().tobytes(), key
    record = np.frombuffer(blob, dtype=ply.NORMAL_VERTEX_DTYPE, count=7, offset=blob.index(b"end_header\n") + 11)
    assert np.array_equal(record["ny"], mesh.normals.numpy()[:, 1])
    thermal = read_mesh_ply(write_mesh_ply(tmp_path / "t.ply", mesh, colors="thermal"))
    assert np.array_equal(thermal["colors"], mesh.thermal_colors.numpy()) and np.array_equal(thermal["normals"], got["normals"])
    mesh.normals = mesh.normals[:-1]
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "bad.ply", mesh)


def test_ply_without_normals_is_the_old_file_byte_for_byte(tmp_path):
    mesh = _host_mesh(False)
    blob = write_mesh_ply(tmp_path / "m.ply", mesh).read_bytes()
    vertex = np.empty(7, dtype=ply.VERTEX_DTYPE)
    pos, col = mesh.positions.numpy(), mesh.colors.numpy()
    vertex["x"], vertex["y"], vertex["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    vertex["red"], vertex["green"], vertex["blue"] = col[:, 0], col[:, 1], col[:, 2]
    vertex["temperature"] = mesh.temperature.numpy()
    face = np.empty(5, dtype=ply.FACE_DTYPE)
    face["n"], face["v"] = 3, mesh.triangles.numpy()
    head = ("ply\nformat binary_little_endian 1.0\ncomment temperature_unit celsius\ncomment temperature_bounds 14.0 33.0\n"
            "element vertex 7\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nproperty float temperature\nelement face 5\nproperty list uchar int vertex_indices\nend_header\n")
    assert blob == head.encode("ascii") + vertex.tobytes() + face.tobytes()
    got = read_mesh_ply(tmp_path / "m.ply")
    assert "normals" not in got and got["positions"].tobytes() == pos.tobytes()
    assert ply.mesh_header(7, 5, (14.0, 33.0)) == head


def test_thermal_mesh_positional_construction_is_unchanged():
    a, b, c, d, e = (torch.zeros(1) for _ in range(5))
    mesh = ThermalMesh(a, b, c, d, e, (1.0, 2.0))
    assert (mesh.positions, mesh.colors, mesh.temperature, mesh.thermal_colors, mesh.triangles) == (a, b, c, d, e)
    assert mesh.temperature_bounds == (1.0, 2.0) and mesh.normals is None
    assert ThermalMesh(a, b, c).normals is None and ThermalMesh(a, b, c, d, e, None, a).normals is a
    import dataclasses

    assert [f.name for f in dataclasses.fields(ThermalMesh)][-1] == "normals"


# ---- the Python layer's refusals (nothing here reaches a kernel) ----------------------------------------------------------------------

def test_python_layer_refuses_bad_factors_and_host_tensors():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for kw in (dict(iterations=-1), dict(iterations=1, lambda_=0.0), dict(iterations=1, lambda_=-0.5), dict(iterations=1, mu=-0.5),
               dict(iterations=1, mu=0.5), dict(iterations=1, lambda_=float("nan")), dict(iterations=1, mu=float("-inf"))):
        with pytest.raises(ValueError):
            smooth_positions(pos, tri, **kw)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    with pytest.raises(ValueError):
        smooth_mesh(mesh, iterations=2, mu=0.1)
    with pytest.raises(ValueError):
        smooth_mesh(ThermalMesh(pos, mesh.colors, mesh.temperature))  # no triangles
    for call in (lambda: mesh_incidence(tri, 3), lambda: vertex_normals(pos, tri), lambda: smooth_positions(pos, tri, 1),
                 lambda: smooth_mesh(mesh)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert MeshIncidence._fields == ("offsets", "corners")


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_export_mesh_parses_the_smoothing_flags_and_they_default_to_off(capsys):
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(ROOT, "tools", "export_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["run", "data", "--output", "mesh.ply"]
    a = tool.parse(base)
    assert a.smooth_iterations == 0 and a.smooth_lambda == 0.5 and a.smooth_mu == -0.53 and a.normals is False
    b = tool.parse(base + ["--smooth-iterations", "10", "--smooth-lambda", "0.33", "--smooth-mu", "-0.34", "--normals"])
    assert b.smooth_iterations == 10 and b.smooth_lambda == 0.33 and b.smooth_mu == -0.34 and b.normals is True
    for bad, word in ((["--smooth-iterations", "-1"], "--smooth-iterations"), (["--smooth-lambda", "0"], "--smooth-lambda"),
                      (["--smooth-mu", "-0.5"], "--smooth-mu"), (["--smooth-lambda", "0.6"], "--smooth-mu"),
                      (["--smooth-mu", "nan"], "--smooth-mu"), (["--smooth-iterations", "1.5"], "--smooth-iterations")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert word in capsys.readouterr().err, bad


# ---- the declarations ------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_in_the_header_and_the_ctypes_table():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    assert re.search(r"\bsize_t tn_mesh_incidence_workspace_bytes\(int64_t num_vertices, int64_t num_triangles\);", header)
    assert re.search(r"\bint tn_mesh_incidence\(const int32_t \*triangles, int64_t num_triangles, int64_t num_vertices, int32_t \*offsets", header)
    assert re.search(r"\bint tn_mesh_vertex_normals\(const float \*positions, const int32_t \*triangles, int64_t num_triangles", header)
    assert re.search(r"\bint tn_mesh_smooth\(const float \*positions_in, const int32_t \*triangles, int64_t num_triangles", header)
    for name, args in (("tn_mesh_incidence_workspace_bytes", 2), ("tn_mesh_incidence", 8), ("tn_mesh_vertex_normals", 8),
                       ("tn_mesh_smooth", 12)):
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == args, name
    assert "tn_mesh_smooth.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    lib = _hip.load()
    v, t = 1000, 2000
    need = mesh_incidence_workspace_bytes(v, t)
    assert need == 2 * 8 * 3 * t + lib.tn_sort_pairs_workspace_bytes(3 * t) and need % 8 == 0
    limit = (2 ** 31 - 1) // 3
    assert mesh_incidence_workspace_bytes(v, limit) > 0
    for bad in ((-1, t), (v, -1), (2 ** 31, t), (v, limit + 1)):
        assert mesh_incidence_workspace_bytes(*bad) == 0, bad
    # every code below is returned from the arguments alone: nothing is dereferenced, allocated or launched (4096: a non-null address)
    dummy = 4096
    assert lib.tn_mesh_incidence(dummy, t, v, None, dummy, dummy, need, None) == -1
    assert lib.tn_mesh_incidence(dummy, limit + 1, v, dummy, dummy, dummy, 2 ** 40, None) == -2
    assert lib.tn_mesh_incidence(dummy, t, 2 ** 31, dummy, dummy, dummy, need, None) == -2
    assert lib.tn_mesh_incidence(dummy, t, v, dummy + 2, dummy, dummy, need, None) == -2
    assert lib.tn_mesh_incidence(dummy, t, v, dummy, dummy, dummy + 4, need, None) == -2
    assert lib.tn_mesh_incidence(None, t, v, dummy, dummy, dummy, need, None) == -1
    assert lib.tn_mesh_incidence(dummy, t, v, dummy, dummy, dummy, need - 1, None) == -4
    assert lib.tn_mesh_vertex_normals(None, dummy, t, v, dummy, dummy, dummy, None) == -1
    assert lib.tn_mesh_vertex_normals(dummy, dummy, limit + 1, v, dummy, dummy, dummy, None) == -2
    assert lib.tn_mesh_vertex_normals(dummy, dummy, t, 0, dummy, dummy, dummy, None) == 0  # V == 0: nothing to do
    good = [dummy, dummy, t, v, dummy, dummy, 2, 0.5, -0.53, 2 ** 20, 2 ** 21, None]

    def smooth(**change):
        names = ("positions_in", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "iterations", "lambda_", "mu",
                 "positions_out", "scratch", "stream")
        return lib.tn_mesh_smooth(*[change.get(k, g) for k, g in zip(names, good)])

    assert smooth(scratch=None) == -1 and smooth(positions_out=None) == -1 and smooth(corners=None) == -1
    assert smooth(iterations=-1) == -2 and smooth(scratch=2 ** 21 + 2) == -2
    assert smooth(lambda_=float("nan")) == -3 and smooth(mu=float("inf")) == -3 and smooth(lambda_=float("-inf")) == -3
    assert smooth(scratch=dummy + 12) == -2 and smooth(scratch=2 ** 20 + 12 * (v - 1)) == -2  # scratch overlaps an end of in / out
    assert smooth(positions_out=dummy + 12) == -2  # out overlaps in without being in
    assert smooth(num_vertices=0) == 0
