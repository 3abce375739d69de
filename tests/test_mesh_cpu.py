"""CPU: the mesh export's definitions and host side — the numpy yardstick on an analytic sphere scene (watertight, outward, within
half a voxel, temperature within a voxel's worth of gradient), the 3 x 3 x 3 patterns, the mesh PLY, the parameter block's
rounding, the grid sizing and the command line's grammar (no kernel runs)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as R
from thermo_nerf_amd.export import (ThermalMesh, grid_dims, mesh_params, read_mesh_ply, read_ply, world_to_camera, write_mesh_ply)
from thermo_nerf_amd.export import ply as ply_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _normals_and_centroids(mesh):
    p = mesh["positions"].astype(np.float64)
    t = mesh["triangles"]
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3


def test_sphere_scene_is_watertight_outward_and_within_half_a_voxel():
    """Bounds as the definitions promise them: the surface within 0.5 step of the sphere, the temperature within the thermal change
    over one step (thermal = (z / 0.3 + 1) / 2: step / 0.6).  Measured with this fp32 reference: 910 vertices, 1816 triangles,
    0.310 step, 0.0445 against 0.0725."""
    s = R.SPHERE
    volume, mesh = R.sphere_mesh()
    step = 2 * s["half"] / (s["grid"] - 1)
    v, t = len(mesh["positions"]), len(mesh["triangles"])
    topo = R.mesh_topology(mesh["triangles"], v)
    radial = np.abs(np.linalg.norm(mesh["positions"].astype(np.float64), axis=1) - s["radius"]).max()
    truth = (mesh["positions"][:, 2].astype(np.float64) / s["radius"] + 1) / 2
    thermal_error = np.abs(mesh["temperature"] - truth).max()
    print("vertices", v, "triangles", t, topo, "radial error / step", radial / step, "thermal error", thermal_error, "bound", step / 0.6)
    assert v > 0 and t > 0
    assert topo["bad_edges"] == 0, "every mesh edge is shared by exactly two triangles"
    assert topo["inconsistent"] == 0 and topo["euler"] == 2 and topo["unused"] == 0
    normal, centroid = _normals_and_centroids(mesh)
    assert ((normal * centroid).sum(axis=1) > 0).all(), "every triangle normal points away from the centre"
    assert radial <= 0.5 * step
    assert thermal_error <= step / 0.6
    assert mesh["triangles"].dtype == np.int32 and mesh["triangles"].min() >= 0 and mesh["triangles"].max() < v
    # the colour weight of an active cell is positive: an inside corner was fused with -truncation <= sdf < 0
    assert np.isfinite(mesh["temperature"]).all()
    assert int((mesh["cell_index"] >= 0).sum()) == v and np.array_equal(mesh["cell_index"][mesh["cell_index"] >= 0], np.arange(v))


Q3 = R.params((-1.0,) * 3, (1.0,) * 3, (3, 3, 3), 1.0, max_temperature=30.0, min_temperature=10.0)


def test_one_inside_point_gives_a_closed_outward_cube():
    mesh = R.extract(R.volume3(), Q3)
    assert mesh["positions"].shape == (8, 3) and mesh["triangles"].shape == (12, 3)
    topo = R.mesh_topology(mesh["triangles"], 8)
    assert topo == dict(edges=18, bad_edges=0, inconsistent=0, euler=2, unused=0)
    normal, centroid = _normals_and_centroids(mesh)
    assert ((normal * centroid).sum(axis=1) > 0).all()
    # every cell has three crossing edges, each halfway along its axis and at offset 1 (a low cell) or 0 (a high cell) on the other
    # two: local = (0.5 + 1 + 1) / 3 in a low cell, (0.5 + 0 + 0) / 3 in a high one, on every axis
    lo, hi = F(-1.0) + F(F(2.5) / F(3.0)), F(-1.0) + (F(1.0) + F(F(0.5) / F(3.0)))
    assert sorted(set(mesh["positions"].reshape(-1).tolist())) == sorted({float(lo), float(hi)})
    assert np.array_equal(mesh["cell_index"], np.arange(8))
    assert (mesh["temperature"] == F(0.25) * F(20.0) + F(10.0)).all()
    assert (mesh["colors"] == np.array([31, 127, 191], np.uint8)).all()


def test_nothing_observed_all_inside_and_one_unobserved_corner():
    empty = R.extract(np.zeros((R.PLANES, 3, 3, 3), F), Q3)
    assert len(empty["positions"]) == 0 and len(empty["triangles"]) == 0 and (empty["cell_index"] == -1).all()
    full = R.extract(R.volume3(inside=[(i, j, k) for i in range(3) for j in range(3) for k in range(3)]), Q3)
    assert len(full["positions"]) == 0 and len(full["triangles"]) == 0
    # an unobserved grid corner (0,0,0) removes exactly cell (0,0,0); an unobserved face centre (1,1,0) the four cells of k = 0
    one = R.extract(R.volume3(unobserved=[(0, 0, 0)]), Q3)
    assert one["cell_index"].tolist() == [-1, 0, 1, 2, 3, 4, 5, 6]
    assert len(one["triangles"]) == 12 - 2 * 3  # the three quads around the removed cell's vertex
    four = R.extract(R.volume3(unobserved=[(1, 1, 0)]), Q3)
    assert four["cell_index"].tolist() == [-1, -1, -1, -1, 0, 1, 2, 3]
    assert len(four["triangles"]) == 2  # only the quad of the edge (1,1,1) -> (1,1,2) keeps its four cells


def _mesh(v, t, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ThermalMesh(positions=torch.randn((v, 3), generator=g) * 7.0, colors=torch.randint(0, 256, (v, 3), generator=g, dtype=torch.uint8),
                       temperature=torch.rand((v,), generator=g) * 19.5 + 14.0,
                       thermal_colors=torch.randint(0, 256, (v, 3), generator=g, dtype=torch.uint8),
                       triangles=torch.randint(0, max(v, 1), (t, 3), generator=g, dtype=torch.int32), temperature_bounds=(14.0, 33.5))


MESH_HEADER = """ply
format binary_little_endian 1.0
comment temperature_unit celsius
comment temperature_bounds 14.0 33.5
element vertex {v}
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property float temperature
element face {t}
property list uchar int vertex_indices
end_header
"""


@pytest.mark.parametrize("v,t", [(0, 0), (5, 0), (4, 2), (300, 777)])
def test_mesh_ply_round_trip(tmp_path, v, t):
    mesh = _mesh(v, t)
    path = write_mesh_ply(tmp_path / "sub" / "mesh.ply", mesh)
    blob = path.read_bytes()
    head = MESH_HEADER.format(v=v, t=t).encode("ascii")
    assert blob[:len(head)] == head and len(blob) == len(head) + 19 * v + 13 * t
    if t:
        face0 = blob[len(head) + 19 * v:][:13]
        assert face0[0] == 3 and np.frombuffer(face0[1:], "<i4").tolist() == mesh.triangles[0].tolist()
    back = read_mesh_ply(path)
    assert back["triangles"].dtype == np.int32 and back["triangles"].shape == (t, 3)
    assert np.array_equal(back["triangles"], mesh.triangles.numpy())
    assert np.array_equal(back["positions"], mesh.positions.numpy()) and np.array_equal(back["colors"], mesh.colors.numpy())
    assert np.array_equal(back["temperature"], mesh.temperature.numpy())
    assert back["comments"] == ["temperature_unit celsius", "temperature_bounds 14.0 33.5"]
    thermal = read_mesh_ply(write_mesh_ply(tmp_path / "thermal.ply", mesh, colors="thermal"))
    assert np.array_equal(thermal["colors"], mesh.thermal_colors.numpy()) and np.array_equal(thermal["triangles"], back["triangles"])
    assert write_mesh_ply(tmp_path / "again.ply", mesh).read_bytes() == blob  # the same mesh, the same bytes
    with pytest.raises(ValueError):
        read_ply(path)  # the cloud reader takes one element only


def test_mesh_ply_rejects_what_it_cannot_write_or_read(tmp_path):
    mesh = _mesh(4, 2)
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "a.ply", mesh, colors="depth")
    mesh.triangles[1, 2] = 4  # names a vertex that is not there
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "a.ply", mesh)
    bad = tmp_path / "bad.ply"
    bad.write_bytes(MESH_HEADER.format(v=1, t=1).encode("ascii") + b"\0" * 19 + b"\3" + b"\0" * 11)  # one byte short
    with pytest.raises(ValueError):
        read_mesh_ply(bad)
    assert ply_module.mesh_header(0, 0).splitlines()[3] == "comment temperature_bounds none none"


def test_mesh_params_round_once_from_double():
    lo, hi, dims = (-0.7, 0.1, -1.3), (0.9, 1.2, 0.35), (24, 7, 11)
    a, b = 0.7, -0.4
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    c2w = np.concatenate([rz @ rx, np.array([[0.3], [-1.7], [0.45]])], axis=1)
    q = mesh_params(lo, hi, dims, 0.13, 0.25, 33.0, 14.0, to_world=c2w * 3.0, camera=(41.3, 40.9, 15.5, 16.25, c2w))
    for c in range(3):
        assert F(q.step[c]) == F((hi[c] - lo[c]) / (dims[c] - 1)) and F(q.lo[c]) == F(lo[c]) and q.dims[c] == dims[c]
    fp32_steps = [F(F(hi[c]) - F(lo[c])) / F(dims[c] - 1) for c in range(3)]
    assert any(F(q.step[c]) != fp32_steps[c] for c in range(3)), "the case must tell double-then-once from fp32 arithmetic"
    assert F(q.inv_truncation) == F(1.0 / 0.13) and F(q.inv_truncation) != F(1.0) / F(0.13)
    assert F(q.truncation) == F(0.13) and F(q.min_accumulation) == F(0.25)
    assert F(q.temperature_span) == F(19.0) and F(q.temperature_min) == F(14.0)
    want = np.concatenate([c2w[:, :3].T, -(c2w[:, :3].T @ c2w[:, 3:])], axis=1)
    assert np.array_equal(np.array(list(q.w2c), F), want.astype(F).reshape(-1))
    assert np.array_equal(world_to_camera(c2w), want)
    fp32_route = -(c2w[:, :3].T.astype(F) @ c2w[:, 3:].astype(F)).astype(F).reshape(-1)
    assert not np.array_equal(np.array(list(q.w2c), F).reshape(3, 4)[:, 3], fp32_route)
    assert np.array_equal(np.array(list(q.to_world), F), (c2w * 3.0).astype(F).reshape(-1))
    assert (F(q.fx), F(q.fy), F(q.cx), F(q.cy)) == (F(41.3), F(40.9), F(15.5), F(16.25))
    # the reference's block holds the same numbers
    r = R.params(lo, hi, dims, 0.13, 0.25, 33.0, 14.0, to_world=c2w * 3.0, camera=(41.3, 40.9, 15.5, 16.25, c2w))
    assert np.array_equal(r["step"], np.array(list(q.step), F)) and r["inv_truncation"] == F(q.inv_truncation)
    assert np.array_equal(r["w2c"].reshape(-1), np.array(list(q.w2c), F))
    for bad in (dict(dims=(1, 4, 4)), dict(dims=(4, 4)), dict(truncation=0.0), dict(to_world=np.eye(4))):
        with pytest.raises(ValueError):
            mesh_params(**dict(dict(lo=lo, hi=hi, dims=dims, truncation=0.13), **bad))


def test_resolution_to_dims():
    assert grid_dims((-1, -1, -1), (1, 1, 1), 256) == (256, 256, 256)
    assert grid_dims((0, 0, 0), (2.0, 1.0, 0.5), 41) == (41, 21, 11)          # step 0.05
    assert grid_dims((0, 0, 0), (1.0, 0.26, 0.01), 11) == (11, 4, 2)          # round(2.6) + 1; a thin side still gets 2
    assert grid_dims((0, 0, 0), (1.0, 2.0, 3.0), (5, 6, 7)) == (5, 6, 7)
    assert grid_dims((0, 0, 0), (1.0, 2.0, 3.0), np.int64(4)) == (2, 3, 4)
    for lo, hi, res in (((0, 0, 0), (1, 1, 1), 1), ((0, 0, 0), (1, 0, 1), 8), ((0, 0, 0), (1, 1, 1), (4, 4)),
                        ((0, 0, 0), (1, 1, 1), (4, 1, 4)), ((0, 0, 0), (1, float("inf"), 1), 8)):
        with pytest.raises(ValueError):
            grid_dims(lo, hi, res)


class _Stub:
    """what MeshExporter's constructor touches of a model"""
    class scene_box:
        aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])

    def _fusable(self):
        return True


def test_exporter_refuses_a_missing_box_and_a_short_truncation():
    from thermo_nerf_amd.export import MeshExporter

    kw = dict(max_temperature=33.0, min_temperature=14.0, resolution=21)
    ex = MeshExporter(_Stub(), **kw)
    assert ex.dims == (21, 21, 21) and ex.truncation == pytest.approx(0.4) and F(ex.params.step[0]) == F(0.1)
    with pytest.raises(ValueError, match="bounding box"):
        MeshExporter(_Stub(), bounding_box=None, **kw)
    with pytest.raises(ValueError, match="sqrt"):
        MeshExporter(_Stub(), truncation=1.7 * 0.1, **kw)
    assert MeshExporter(_Stub(), truncation=1.74 * 0.1, **kw).truncation == pytest.approx(0.174)
    # the largest step decides: a box of sides 2, 2, 0.3 at resolution 21 has steps 0.1, 0.1 and 0.3 / 3 = 0.1
    ex = MeshExporter(_Stub(), bounding_box=[[-1, -1, 0], [1, 1, 0.3]], **kw)
    assert ex.dims == (21, 21, 4) and ex.truncation == pytest.approx(4 * 0.1)
    with pytest.raises(ValueError):
        MeshExporter(_Stub(), depth_output_name="median", **kw)

    class Staged(_Stub):
        def _fusable(self):
            return False

    with pytest.raises(RuntimeError, match="not fusable"):
        MeshExporter(Staged(), **kw)


def _tool():
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(ROOT, "tools", "export_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_defaults_and_grammar(capsys):
    tool = _tool()
    a = tool.parse(["run", "data", "--output", "mesh.ply"])
    assert (str(a.model_uri), str(a.dataset_path), str(a.output)) == ("run", "data", "mesh.ply")
    assert a.split == "train" and a.resolution == [256] and a.truncation is None and a.resolution_scale == 1.0 and a.depth == "depth"
    assert a.min_accumulation == 0.5 and a.bounding_box_min is None and a.bounding_box_max is None
    assert a.colors == "rgb" and a.scene_frame is False and a.config_json is None and a.device == "cuda"
    b = tool.parse(["r", "d", "--output", "o", "--split", "val", "--resolution", "32", "16", "8", "--truncation", "0.25", "--depth",
                    "expected_depth", "--colors", "thermal", "--scene-frame", "--bounding-box-min", "-1", "-2", "-3",
                    "--bounding-box-max", "1", "2", "3", "--min-accumulation", "0.1", "--resolution-scale", "0.5"])
    assert b.split == "val" and b.resolution == [32, 16, 8] and b.truncation == 0.25 and b.depth == "expected_depth"
    assert b.colors == "thermal" and b.scene_frame and b.bounding_box_min == [-1.0, -2.0, -3.0] and b.bounding_box_max == [1.0, 2.0, 3.0]
    assert b.min_accumulation == 0.1 and b.resolution_scale == 0.5
    for bad in (["r", "d"], ["r", "d", "--output", "o", "--resolution", "32", "16"], ["r", "d", "--output", "o", "--depth", "median"],
                ["r", "d", "--output", "o", "--bounding-box-min", "0", "0", "0"], ["r", "d", "--output", "o", "--resolution", "1"]):
        with pytest.raises(SystemExit):
            tool.parse(bad)
    capsys.readouterr()
