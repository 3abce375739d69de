"""tn_mesh_incidence / tn_mesh_vertex_normals / tn_mesh_smooth on the device against tests/mesh_smooth_reference.py, exactly (int32
and float bit patterns), into guarded buffers: the literal cases, sizes around the block and the sort's tile, a sparse index over
many vertices, the long list of a fan, a strip, random meshes with invalid and repeated indices, the sphere mesh, empty meshes, the
error codes, the exporter and the command line."""
from __future__ import annotations

import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import helpers, mesh_reference
from tests import mesh_smooth_reference as R
from tests.mesh_components_reference import random_mesh
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (MeshExporter, MeshIncidence, PointCloudExporter, ThermalMesh, mesh_incidence,
                                    mesh_incidence_workspace_bytes, read_mesh_ply, remove_small_components, smooth_mesh,
                                    smooth_positions, sort_tile, vertex_normals)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILL, FLOAT_FILL, BYTE_FILL = -5, -777.0, 0xEE


def _ints(n):
    return torch.full((n + GUARD,), FILL, dtype=torch.int32, device=DEV)


def _floats(rows):
    return torch.full((rows + GUARD, 3), FLOAT_FILL, dtype=torch.float32, device=DEV)


def _guard_kept(buf, used, name):
    tail = buf.reshape(-1)[used:]
    assert bool((tail == (FILL if buf.dtype == torch.int32 else FLOAT_FILL)).all()), f"{name} was written beyond element {used}"


def run_incidence(tri, v):
    """tn_mesh_incidence into guarded buffers, compared to the yardstick: (device triangles, MeshIncidence of exact size, yardstick)"""
    want = R.incidence(tri, v)
    t = len(tri)
    dev_tri = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)).to(DEV)
    offsets, corners = _ints(v + 1), _ints(3 * t)
    need = mesh_incidence_workspace_bytes(v, t)
    workspace = torch.full((need + 64,), BYTE_FILL, dtype=torch.uint8, device=DEV)
    _hip.check(_hip.load().tn_mesh_incidence(dev_tri.data_ptr() if t else None, t, v, offsets.data_ptr(), corners.data_ptr(),
                                             workspace.data_ptr(), need, _hip.current_stream()), "tn_mesh_incidence")
    assert np.array_equal(offsets[:v + 1].cpu().numpy(), want["offsets"]), "offsets"
    _guard_kept(offsets, v + 1, "offsets")
    if want["corners"] is None:
        _guard_kept(corners, 0, "corners")  # untouched
    else:
        assert np.array_equal(corners[:3 * t].cpu().numpy(), want["corners"]), "corners"
        _guard_kept(corners, 3 * t, "corners")
    assert bool((workspace[need:] == BYTE_FILL).all()), "written beyond the workspace"
    return dev_tri, MeshIncidence(offsets[:v + 1], corners[:3 * t]), want


def run_normals(pos, dev_tri, index, want_index, tri):
    v, t = len(pos), len(tri)
    dev_pos = torch.from_numpy(pos).to(DEV)
    normals = _floats(v)
    _hip.check(_hip.load().tn_mesh_vertex_normals(dev_pos.data_ptr() if v else None, dev_tri.data_ptr() if t else None, t, v,
                                                  index.offsets.data_ptr(), index.corners.data_ptr() if t else None,
                                                  normals.data_ptr(), _hip.current_stream()), "tn_mesh_vertex_normals")
    want = R.vertex_normals(pos, tri, want_index)
    assert np.array_equal(R.bits(normals[:v].cpu().numpy()), R.bits(want)), "normals"
    _guard_kept(normals, 3 * v, "normals")
    return want


def run_smooth(pos, dev_tri, index, want_index, tri, iterations, lambda_=0.5, mu=-0.53, in_place=False, want=None):
    v, t = len(pos), len(tri)
    out, scratch = _floats(v), _floats(v)
    if in_place:
        out[:v] = torch.from_numpy(pos).to(DEV)
        dev_pos = out
    else:
        dev_pos = torch.from_numpy(pos).to(DEV)
    _hip.check(_hip.load().tn_mesh_smooth(dev_pos.data_ptr() if v else None, dev_tri.data_ptr() if t else None, t, v,
                                          index.offsets.data_ptr(), index.corners.data_ptr() if t else None, iterations, lambda_, mu,
                                          out.data_ptr(), scratch.data_ptr(), _hip.current_stream()), "tn_mesh_smooth")
    want = R.smooth(pos, tri, want_index, iterations, lambda_, mu) if want is None else want
    assert np.array_equal(R.bits(out[:v].cpu().numpy()), R.bits(want)), f"positions after {iterations} iterations"
    _guard_kept(out, 3 * v, "positions_out")
    _guard_kept(scratch, 3 * v, "scratch")
    if not in_place and v:
        assert np.array_equal(R.bits(dev_pos.cpu().numpy()), R.bits(pos)), "positions_in was written"
    return want


def check_mesh(pos, tri, iterations=(1,)):
    """the index, the normals and ``iterations`` smoothing runs of one mesh, each exact"""
    dev_tri, index, want_index = run_incidence(tri, len(pos))
    run_normals(pos, dev_tri, index, want_index, tri)
    for k in iterations:
        run_smooth(pos, dev_tri, index, want_index, tri, k)
    return dev_tri, index, want_index


# ---- the literal cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_literal_cases_through_the_kernels(name):
    case = R.LITERAL[name]
    pos, tri = R.literal_arrays(case)
    dev_tri, index, want_index = run_incidence(tri, len(pos))
    assert index.offsets.tolist() == case["offsets"] and index.corners.tolist() == case["corners"]
    assert R.bits(run_normals(pos, dev_tri, index, want_index, tri)).tolist() == case["normals"]
    # one pass with 0.5, then a pass with 0, which moves nothing (p + 0 (m - p) = p for these non-negative finite values)
    literal = np.array(case["pass_half"], dtype=np.uint32).view(F)
    run_smooth(pos, dev_tri, index, want_index, tri, 1, 0.5, 0.0, want=literal)
    run_smooth(pos, dev_tri, index, want_index, tri, 2)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v, t", [(n, 2 * n) for n in (255, 256, 257)] + [(2 * n, n) for n in (255, 256, 257)])
def test_vertex_and_triangle_counts_around_the_block(v, t):
    check_mesh(R.random_positions(v, v), random_mesh(v + t, v, t))


def _sort_tile_cases():
    tile = 2048  # asserted against tn_sort_tile() in the test
    return [tile // 3, tile // 3 + 1, 2 * tile // 3, 2 * tile // 3 + 1]


@pytest.mark.parametrize("t", _sort_tile_cases())
def test_corner_counts_around_the_sort_tile_and_one_tile_more(t):
    tile = sort_tile()
    assert tile == 2048 and 3 * t in (tile - 2, tile + 1, 2 * tile - 1, 2 * tile + 2)
    v = 600
    check_mesh(R.random_positions(t, v), random_mesh(t, v, t))


def test_seventy_thousand_vertices_three_sort_passes_mostly_unreferenced():
    v, t = 70000, 3000
    assert v.bit_length() == 17  # three 8-bit passes
    tri = random_mesh(7, v, t)
    _, _, want_index = check_mesh(R.random_positions(7, v), tri)
    assert int((np.diff(want_index["offsets"]) == 0).sum()) > 60000


def test_fan_of_two_thousand_triangles_the_long_list():
    t = 2000
    tri = R.fan(t)
    pos = R.random_positions(2, t + 2)
    _, _, want_index = check_mesh(pos, tri, iterations=(1, 2))
    assert int(want_index["offsets"][1]) == t, "vertex 0 lists a corner of every triangle"


def test_triangle_strip():
    v = 3001
    pos = R.random_positions(3, v)
    pos[:, 2] *= F(0.01)  # nearly flat: the alternating winding keeps every face vector on one side
    check_mesh(pos, R.strip(v), iterations=(1, 3))


@pytest.mark.parametrize("seed, t", [(21, 400), (22, 2500), (23, 9000)])
def test_random_sparse_meshes_with_invalid_and_repeated_indices(seed, t):
    v = 3000
    tri = random_mesh(seed, v, t, invalid=0.05)
    _, _, want_index = check_mesh(R.random_positions(seed, v), tri, iterations=(1, 2))
    assert int(want_index["offsets"][v]) < 3 * t, "some triangles are invalid"
    assert bool((tri[:, 0] == tri[:, 1]).any())


# ---- the sphere mesh --------------------------------------------------------------------------------------------------------------------

def test_sphere_mesh_index_normals_iterations_in_place_and_zero_iterations():
    mesh = mesh_reference.sphere_mesh()[1]
    pos, tri = mesh["positions"], mesh["triangles"]
    dev_tri, index, want_index = run_incidence(tri, len(pos))
    run_normals(pos, dev_tri, index, want_index, tri)
    five = None
    for k in (1, 2, 5):
        five = run_smooth(pos, dev_tri, index, want_index, tri, k)
    run_smooth(pos, dev_tri, index, want_index, tri, 5, in_place=True, want=five)
    run_smooth(pos, dev_tri, index, want_index, tri, 0, want=pos)
    run_smooth(pos, dev_tri, index, want_index, tri, 0, in_place=True, want=pos)
    # the Python layer gives the same arrays, twice the same bytes, and leaves its input alone
    dev_pos = torch.from_numpy(pos).to(DEV)
    built = mesh_incidence(dev_tri, len(pos))
    assert torch.equal(built.offsets, index.offsets) and torch.equal(built.corners, index.corners)
    first, second = smooth_positions(dev_pos, dev_tri, 5, incidence=built), smooth_positions(dev_pos, dev_tri, 5)
    assert np.array_equal(R.bits(first.cpu().numpy()), R.bits(five)) and torch.equal(first, second)
    assert np.array_equal(R.bits(dev_pos.cpu().numpy()), R.bits(pos))
    normals = vertex_normals(first, dev_tri, built)
    assert torch.equal(normals, vertex_normals(first, dev_tri))
    assert np.array_equal(R.bits(normals.cpu().numpy()), R.bits(R.vertex_normals(five, tri, want_index)))
    # smooth_mesh: the index once, the attribute tensors shared
    colors = torch.zeros((len(pos), 3), dtype=torch.uint8, device=DEV)
    temperature = torch.from_numpy(mesh["temperature"]).to(DEV)
    source = ThermalMesh(dev_pos, colors, temperature, None, dev_tri, (14.0, 33.0))
    got = smooth_mesh(source, 5, normals=True)
    assert torch.equal(got.positions, first) and torch.equal(got.normals, normals)
    assert got.colors is colors and got.temperature is temperature and got.triangles is dev_tri and got.temperature_bounds == (14.0, 33.0)
    assert smooth_mesh(source, 5).normals is None and source.normals is None
    only_normals = smooth_mesh(source, 0, normals=True)
    assert torch.equal(only_normals.positions, dev_pos)
    assert np.array_equal(R.bits(only_normals.normals.cpu().numpy()), R.bits(R.vertex_normals(pos, tri, want_index)))


# ---- empty meshes and the error codes ---------------------------------------------------------------------------------------------------

def test_no_vertices_or_no_triangles():
    none = np.zeros((0, 3), np.int32)
    for v, tri in ((0, none), (300, none), (0, np.array([[0, 1, 2], [3, 4, 5]], np.int32))):
        pos = R.random_positions(5, v)
        check_mesh(pos, tri, iterations=(0, 2))
        if v:
            dev = torch.from_numpy(pos).to(DEV)
            empty = torch.empty((0, 3), dtype=torch.int32, device=DEV)
            assert torch.equal(smooth_positions(dev, empty, 2), dev) and not vertex_normals(dev, empty).any()


def test_error_codes_without_a_launch():
    lib = _hip.load()
    v, t = 700, 900
    tri_host = random_mesh(3, v, t)
    pos_host = R.random_positions(3, v)
    dev_tri, index, _ = run_incidence(tri_host, v)
    pos = torch.from_numpy(pos_host).to(DEV)
    offsets, corners = _ints(v + 1), _ints(3 * t)
    need = mesh_incidence_workspace_bytes(v, t)
    ws = torch.full((need,), BYTE_FILL, dtype=torch.uint8, device=DEV)
    stream = _hip.current_stream()
    names = ("triangles", "num_triangles", "num_vertices", "offsets", "corners", "workspace", "workspace_bytes", "stream")
    good = dict(triangles=dev_tri.data_ptr(), num_triangles=t, num_vertices=v, offsets=offsets.data_ptr(), corners=corners.data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=need, stream=stream)

    def incidence(**change):
        args = dict(good, **change)
        return lib.tn_mesh_incidence(*[args[k] for k in names])

    for k in ("triangles", "offsets", "corners", "workspace"):
        assert incidence(**{k: None}) == -1, k  # TN_ERR_NULL
    limit = (2 ** 31 - 1) // 3
    assert incidence(num_vertices=-1) == -2 and incidence(num_vertices=2 ** 31) == -2  # TN_ERR_SHAPE
    assert incidence(num_triangles=-1) == -2 and incidence(num_triangles=limit + 1) == -2  # by the arguments alone
    for k in ("triangles", "offsets", "corners"):
        assert incidence(**{k: good[k] + 2}) == -2, k
    assert incidence(workspace=good["workspace"] + 4) == -2
    assert incidence(workspace_bytes=need - 1) == -4 and incidence(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    assert lib.tn_mesh_incidence_workspace_bytes(-1, 0) == 0 and lib.tn_mesh_incidence_workspace_bytes(0, limit + 1) == 0
    assert lib.tn_mesh_incidence_workspace_bytes(2 ** 31, 0) == 0 and lib.tn_mesh_incidence_workspace_bytes(2 ** 31 - 1, limit) > 0

    out, scratch = _floats(v), _floats(v)
    mesh_names = ("positions", "triangles", "num_triangles", "num_vertices", "offsets", "corners")
    mesh_good = dict(positions=pos.data_ptr(), triangles=dev_tri.data_ptr(), num_triangles=t, num_vertices=v,
                     offsets=index.offsets.data_ptr(), corners=index.corners.data_ptr())

    def normals(**change):
        args = {**mesh_good, "normals": out.data_ptr(), **change}
        return lib.tn_mesh_vertex_normals(*[args[k] for k in mesh_names + ("normals",)], stream)

    def smooth(**change):
        args = {**mesh_good, "iterations": 2, "lambda_": 0.5, "mu": -0.53, "positions_out": out.data_ptr(), "scratch": scratch.data_ptr(),
                **change}
        return lib.tn_mesh_smooth(*[args[k] for k in mesh_names + ("iterations", "lambda_", "mu", "positions_out", "scratch")], stream)

    for call, output in ((normals, "normals"), (smooth, "positions_out")):
        for k in ("positions", "triangles", "offsets", "corners", output):
            assert call(**{k: None}) == -1, (output, k)
        for k in ("positions", "triangles", "offsets", "corners", output):
            assert call(**{k: dict(mesh_good, normals=out.data_ptr(), positions_out=out.data_ptr())[k] + 2}) == -2, (output, k)
        assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2
        assert call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert smooth(scratch=None) == -1 and smooth(scratch=scratch.data_ptr() + 2) == -2 and smooth(iterations=-1) == -2
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert smooth(lambda_=bad) == -3 and smooth(mu=bad) == -3  # TN_ERR_UNSUPPORTED
    assert smooth(scratch=out.data_ptr()) == -2 and smooth(scratch=pos.data_ptr()) == -2  # scratch overlaps an end of the chain
    assert smooth(scratch=out.data_ptr() + 12 * (v - 1)) == -2 and smooth(positions_out=pos.data_ptr() + 12) == -2
    torch.cuda.synchronize()
    assert bool((offsets == FILL).all()) and bool((corners == FILL).all()) and bool((ws == BYTE_FILL).all())
    assert bool((out == FLOAT_FILL).all()) and bool((scratch == FLOAT_FILL).all()), "a refused call launched something"
    assert smooth(lambda_=-0.5, mu=0.5) == 0  # the entry takes any finite pair; the Python layer is the one that asks for Taubin's
    with pytest.raises(ValueError):
        smooth_positions(pos, dev_tri, 1, incidence=MeshIncidence(index.offsets[:-1], index.corners))
    with pytest.raises(ValueError):
        mesh_incidence(dev_tri, v, workspace=ws[:-8])
    with pytest.raises(TypeError):
        vertex_normals(pos.double(), dev_tri)
    with pytest.raises(ValueError):
        vertex_normals(pos.reshape(-1), dev_tri)


# ---- the exporter -------------------------------------------------------------------------------------------------------------------------

def _same(a, b, keys=("positions", "colors", "temperature", "thermal_colors", "triangles")):
    for key in keys:
        assert getattr(a, key).cpu().numpy().tobytes() == getattr(b, key).cpu().numpy().tobytes(), key


def test_exporter_smooths_and_adds_normals_as_the_steps_by_hand_and_is_unchanged_by_default():
    from thermo_nerf_amd import synthetic

    cpu_model, _, _ = helpers.build("scene", 48)
    model = copy.deepcopy(cpu_model).to(DEV).eval()
    cameras = synthetic.orbit_cameras(32, 32, [0, 1, 2, 3], num_views=4, elevation_deg=[0.0, 25.0, 0.0, 25.0])
    kw = dict(max_temperature=33.0, min_temperature=14.0, resolution=32)
    exporter = MeshExporter(model, **kw)
    plain = exporter.export(cameras)
    if plain.triangles.shape[0] == 0:  # no surface inside the scene box for these weights: the box of the cloud of the same cameras
        cloud = PointCloudExporter(model, max_temperature=33.0, min_temperature=14.0, bounding_box=None).export(cameras)
        box = [cloud.positions.min(dim=0).values.cpu().double().tolist(), cloud.positions.max(dim=0).values.cpu().double().tolist()]
        exporter = MeshExporter(model, bounding_box=box, **kw)
        plain = exporter.export(cameras)
    v, t = len(plain), int(plain.triangles.shape[0])
    assert v > 0 and t > 0
    # the defaults: today's extraction, bit for bit, and no normals
    _same(plain, exporter.extract(exporter.fuse(cameras)))
    assert plain.normals is None
    # all three steps: components, smoothing, normals — in that order, equal to the steps by hand and to the yardstick
    _, found = remove_small_components(plain, largest_only=True)
    n = max(2, found.largest_triangles // 2)
    got = exporter.export(cameras, min_component_triangles=n, smooth_iterations=3, normals=True)
    kept, info = remove_small_components(plain, min_triangles=n)
    assert exporter.last_components == info and 0 < len(kept) == len(got)
    hand = smooth_mesh(kept, 3, normals=True)
    _same(got, hand, keys=("positions", "normals", "colors", "temperature", "thermal_colors", "triangles"))
    _same(got, kept, keys=("colors", "temperature", "thermal_colors", "triangles"))  # only positions move
    pos, tri = kept.positions.cpu().numpy(), kept.triangles.cpu().numpy()
    index = R.incidence(tri, len(pos))
    want = R.smooth(pos, tri, index, 3, 0.5, -0.53)
    assert np.array_equal(R.bits(got.positions.cpu().numpy()), R.bits(want))
    assert np.array_equal(R.bits(got.normals.cpu().numpy()), R.bits(R.vertex_normals(want, tri, index)))
    # normals alone are those of the unsmoothed positions; other factors reach the kernel
    only = exporter.export(cameras, normals=True)
    _same(only, plain)
    full = R.incidence(plain.triangles.cpu().numpy(), v)
    assert np.array_equal(R.bits(only.normals.cpu().numpy()),
                          R.bits(R.vertex_normals(plain.positions.cpu().numpy(), plain.triangles.cpu().numpy(), full)))
    other = exporter.export(cameras, smooth_iterations=1, smooth_lambda=0.33, smooth_mu=-0.34)
    assert np.array_equal(R.bits(other.positions.cpu().numpy()),
                          R.bits(R.smooth(plain.positions.cpu().numpy(), plain.triangles.cpu().numpy(), full, 1, 0.33, -0.34)))
    with pytest.raises(ValueError):
        exporter.export(cameras, smooth_iterations=-1)
    with pytest.raises(ValueError):
        exporter.export(cameras, smooth_iterations=1, smooth_mu=0.5)


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_writes_the_smoothed_mesh_with_normals(tmp_path, capsys):
    from tests.test_gpu_mesh_components import _write_tree

    data = tmp_path / "data"
    _write_tree(data)
    small = tmp_path / "small.json"
    small.write_text(json.dumps(helpers.SMALL))
    models = tmp_path / "models"
    assert _tool("train_eval").main(["--data", str(data), "--experiment-name", "mesh", "--model-output-folder", str(models),
                                     "--metrics-output-folder", str(tmp_path / "metrics"), "--max-num-iterations", "30",
                                     "--config-json", str(small), "--temperature-bounds", "33", "14", "--device", DEV]) == 0
    run_dir = next((models / "mesh" / "thermal-nerf").iterdir())
    tool = _tool("export_mesh")
    common = [str(run_dir), str(data), "--min-accumulation", "0.02", "--resolution", "24", "--device", DEV]
    plain_file, smooth_file = tmp_path / "plain.ply", tmp_path / "smooth.ply"
    exporter, cameras, adjust = tool.build_exporter(tool.parse(common + ["--output", str(plain_file)]))
    plain = exporter.export(cameras, apply_camera_optimizer=adjust)
    want = exporter.export(cameras, apply_camera_optimizer=adjust, smooth_iterations=4, normals=True)
    assert len(plain) > 0 and plain.triangles.shape[0] > 0
    capsys.readouterr()
    assert tool.main(common + ["--output", str(plain_file)]) == 0
    printed = capsys.readouterr().out
    assert "smoothing iterations 0, normals no" in printed
    old = read_mesh_ply(plain_file)
    assert "normals" not in old and old["positions"].tobytes() == plain.positions.cpu().numpy().tobytes()
    assert b"property float nx" not in plain_file.read_bytes()
    assert tool.main(common + ["--output", str(smooth_file), "--smooth-iterations", "4", "--normals"]) == 0
    printed = capsys.readouterr().out
    print(printed)
    assert "smoothing iterations 4, normals yes" in printed and f"vertices {len(want)}, triangles {int(want.triangles.shape[0])}" in printed
    got = read_mesh_ply(smooth_file)
    for key in ("positions", "normals", "colors", "temperature", "triangles"):
        assert got[key].tobytes() == getattr(want, key).cpu().numpy().tobytes(), key
    assert got["temperature"].tobytes() == old["temperature"].tobytes() and got["positions"].tobytes() != old["positions"].tobytes()
    lengths = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert bool(((np.abs(lengths - 1.0) < 1e-6) | (lengths == 0.0)).all())
