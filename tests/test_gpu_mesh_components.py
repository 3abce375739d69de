"""tn_mesh_components / tn_mesh_filter_components on the device against tests/mesh_components_reference.py, exactly: the literal
cases, sizes around the tile and the scan, contention (stars), depth (strips), random sparse meshes with every filter setting,
the error codes, two spheres through the extraction (independent of the yardstick) and the command line."""
from __future__ import annotations

import importlib.util
import json
import os
import time

import numpy as np
import pytest
import torch
from PIL import Image

from tests import helpers
from tests import mesh_components_reference as R
from thermo_nerf_amd import _hip, colormaps
from thermo_nerf_amd.export import (ComponentsInfo, MeshComponents, ThermalMesh, filter_components, mesh_components,
                                    mesh_components_workspace_bytes, mesh_extract, mesh_params, mesh_scan_width, mesh_tile,
                                    mesh_workspace_bytes, read_mesh_ply, remove_small_components, write_mesh_ply)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 96  # rows behind every output buffer that must keep their pattern
FILL = -5


def upload(tri):
    return torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)).to(DEV)


def check_components(tri, v, want=None):
    """run tn_mesh_components and compare its three outputs to the yardstick's (or to ``want``); returns (device, expected)"""
    want = R.components(tri, v) if want is None else want
    comp = mesh_components(upload(tri), v)
    assert isinstance(comp, MeshComponents)
    assert comp.summary.tolist() == want["summary"].tolist(), "summary"
    assert np.array_equal(comp.labels.cpu().numpy(), want["labels"]), "labels"
    assert np.array_equal(comp.component_triangles.cpu().numpy(), want["component_triangles"]), "component_triangles"
    return comp, want


def check_filter(tri, v, comp, want_comp, min_triangles, largest_only, cap_v=None, cap_t=None, want=None):
    """run tn_mesh_filter_components into guarded buffers: the counts, every row below the capacities, the pattern everywhere
    else, the complete vertex_map and the bytes behind the workspace"""
    want = R.filter_components(tri, v, want_comp, min_triangles, largest_only) if want is None else want
    kv, kt = (int(c) for c in want["counts"])
    cap_v, cap_t = kv if cap_v is None else cap_v, kt if cap_t is None else cap_t
    source = torch.full((cap_v + GUARD,), FILL, dtype=torch.int32, device=DEV)
    out = torch.full((cap_t + GUARD, 3), FILL, dtype=torch.int32, device=DEV)
    counts = torch.tensor([-7, -9], dtype=torch.int64, device=DEV)
    need = mesh_components_workspace_bytes(v, len(tri))
    workspace = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    filter_components(upload(tri), v, comp, counts=counts, min_triangles=min_triangles, largest_only=largest_only,
                      vertex_source=source if cap_v else None, triangles_out=out if cap_t else None, capacity_vertices=cap_v,
                      capacity_triangles=cap_t, workspace=workspace)
    assert counts.tolist() == [kv, kt], (counts.tolist(), kv, kt)
    got_source, got_out = source.cpu().numpy(), out.cpu().numpy()
    ev, et = min(kv, cap_v), min(kt, cap_t)
    assert np.array_equal(got_source[:ev], want["vertex_source"][:ev]), "vertex_source"
    assert (got_source[ev:] == FILL).all(), f"vertex_source was written at or beyond row {ev}"
    assert np.array_equal(got_out[:et], want["triangles"][:et]), "triangles_out"
    assert (got_out[et:] == FILL).all(), f"triangles_out was written at or beyond row {et}"
    ws = workspace.cpu().numpy()
    if v:
        assert np.array_equal(ws[:4 * v].view(np.int32), want["vertex_map"]), "vertex_map is incomplete"
    assert (ws[need:] == 0xEE).all(), "written beyond the workspace"
    return want


# ---- the literal cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_literal_cases_through_the_kernels(name):
    case = R.LITERAL[name]
    tri, v = R.literal_triangles(case), case["num_vertices"]
    literal = dict(labels=np.array(case["labels"], np.int32), component_triangles=np.array(case["component_triangles"], np.int32),
                   summary=np.array(case["summary"], np.int64))
    comp, want_comp = check_components(tri, v, want=literal)
    for (min_triangles, largest_only), want in case["filters"].items():
        got = check_filter(tri, v, comp, want_comp, min_triangles, largest_only)
        assert got["vertex_source"].tolist() == want["vertex_source"] and got["triangles"].tolist() == want["triangles"]
        check_filter(tri, v, comp, want_comp, min_triangles, largest_only, cap_v=0, cap_t=0)  # the sizing call


# ---- around the tile and the scan -----------------------------------------------------------------------------------------------------

def islands(v, t, seed):
    """three-vertex islands of alternately 1 and 3 triangles (so min_triangles = 2 drops about half the components), as many as
    ``t`` triangles and ``v`` vertices allow, the rest of the vertices isolated; vertex numbers and triangle order shuffled, so
    that kept and dropped ones alternate across every tile border"""
    rng = np.random.default_rng(seed)
    tri, base, k = [], 0, 0
    while base + 3 <= v and len(tri) < t:
        a, b, c = base, base + 1, base + 2
        tri += [(a, b, c), (b, c, a), (c, a, b)][:min(3 if k % 2 else 1, t - len(tri))]
        base, k = base + 3, k + 1
    tri = np.array(tri, dtype=np.int64).reshape(-1, 3)
    return rng.permutation(v)[tri[rng.permutation(len(tri))]].astype(np.int32).reshape(-1, 3)


def _tile_cases():
    tile = 256
    return [(n, 2 * n, "V") for n in (tile - 1, tile, tile + 1)] + [(2 * n, n, "T") for n in (tile - 1, tile, tile + 1)]


@pytest.mark.parametrize("v, t, which", _tile_cases())
def test_vertex_and_triangle_counts_around_the_tile(v, t, which):
    assert mesh_tile() == 256
    tri = islands(v, t, seed=v + t)
    assert which == "V" or len(tri) == t, "the triangle count sits at the tile border"
    comp, want_comp = check_components(tri, v)
    want = check_filter(tri, v, comp, want_comp, 2, False)
    dropped = int((want_comp["component_triangles"] == 1).sum())
    assert dropped > 20 and int((want_comp["component_triangles"] >= 2).sum()) > 20, "both kinds of components are there"
    assert 0 < want["counts"][0] < v and 0 < want["counts"][1] < len(tri)
    check_filter(tri, v, comp, want_comp, 1, False)
    check_filter(tri, v, comp, want_comp, 2, True)


def test_more_vertices_than_one_pass_of_the_scan_block():
    tile, width = mesh_tile(), mesh_scan_width()
    v, t = tile * width + 300, 60000  # 1026 vertex tiles: the scan block makes two passes
    tri = islands(v, t, seed=1)
    assert len(tri) == t
    comp, want_comp = check_components(tri, v)
    want = check_filter(tri, v, comp, want_comp, 2, False)
    assert want["vertex_source"][-1] > tile * width, "kept vertices lie in the second pass"
    assert 0 < want["counts"][0] < v and 0 < want["counts"][1] < t


# ---- contention and depth -------------------------------------------------------------------------------------------------------------

def _one_component(tri, v):
    """every vertex in triangle-connected reach of vertex 0: the expected outputs without the yardstick's loop"""
    t = len(tri)
    count = np.zeros(v, np.int32)
    count[0] = t
    return (dict(labels=np.zeros(v, np.int32), component_triangles=count, summary=np.array([1, t, 0], np.int64)),
            dict(vertex_source=np.arange(v, dtype=np.int32), triangles=tri, counts=np.array([v, t], np.int64),
                 vertex_map=np.arange(v, dtype=np.int32)))


@pytest.mark.parametrize("hub", ["first", "last"])
def test_star_every_triangle_contains_one_vertex(hub):
    t = 100000
    v = t + 2
    i = np.arange(t, dtype=np.int32)
    # hub 0: rims 1 .. V-1; hub V-1: rims 0 .. V-2 — every hook then has to move a root downward
    tri = np.stack([np.zeros(t, np.int32), i + 1, i + 2], axis=1) if hub == "first" else np.stack([np.full(t, v - 1, np.int32), i, i + 1], axis=1)
    want_comp, want = _one_component(tri, v)
    comp, _ = check_components(tri, v, want=want_comp)
    check_filter(tri, v, comp, want_comp, t, True, want=want)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_strip_of_two_hundred_thousand_vertices(order):
    """the case a find without path shortening turns quadratic.  No threshold on the time; it is printed for the record (on an
    MI355X: 0.26 ms ascending, 0.77 ms descending)."""
    v = 200000
    i = np.arange(v - 2, dtype=np.int32)
    tri = np.stack([i, i + 1, i + 2], axis=1)
    if order == "descending":
        tri = np.ascontiguousarray(tri[::-1])
    want_comp, want = _one_component(tri, v)
    dev_tri = upload(tri)
    mesh_components(dev_tri[:256], 258)  # the code objects are loaded before the clock starts
    torch.cuda.synchronize()
    start = time.perf_counter()
    mesh_components(dev_tri, v)
    torch.cuda.synchronize()
    print(f"strip {order}: V = {v}, T = {len(tri)}, tn_mesh_components wall time {(time.perf_counter() - start) * 1e3:.3f} ms")
    comp, _ = check_components(tri, v, want=want_comp)
    check_filter(tri, v, comp, want_comp, 1, False, want=want)


# ---- random sparse meshes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed, t", [(seed, t) for seed in (11, 12, 13) for t in (500, 2500, 10000)])
def test_random_sparse_meshes_every_filter_setting(seed, t):
    v = 5000
    tri = R.random_mesh(seed, v, t)
    comp, want_comp = check_components(tri, v)
    sizes = want_comp["component_triangles"]
    assert len(np.unique(sizes[sizes > 0])) >= 4 and want_comp["summary"][0] > 50, "many components of many sizes"
    for min_triangles in (1, 2, 7):
        for largest_only in (False, True):
            want = check_filter(tri, v, comp, want_comp, min_triangles, largest_only)
    want = check_filter(tri, v, comp, want_comp, 2, False, cap_v=0, cap_t=0)  # the sizing call
    kv, kt = (int(c) for c in want["counts"])
    assert kv > 200 and kt > 100
    check_filter(tri, v, comp, want_comp, 2, False, cap_v=kv // 2, cap_t=kt - 1)
    check_filter(tri, v, comp, want_comp, 2, False, cap_v=1, cap_t=kt // 2)


# ---- the error codes ------------------------------------------------------------------------------------------------------------------

def _setup_calls():
    v, t = 700, 900
    tri = upload(R.random_mesh(3, v, t))
    comp = mesh_components(tri, v)
    lib = _hip.load()
    return v, t, tri, comp, lib


def test_components_error_codes_without_a_launch():
    v, t, tri, _, lib = _setup_calls()
    labels = torch.full((v,), FILL, dtype=torch.int32, device=DEV)
    count = torch.full((v,), FILL, dtype=torch.int32, device=DEV)
    summary = torch.tensor([-7, -8, -9], dtype=torch.int64, device=DEV)
    names = ("triangles", "num_triangles", "num_vertices", "labels", "component_triangles", "summary", "stream")
    good = dict(triangles=tri.data_ptr(), num_triangles=t, num_vertices=v, labels=labels.data_ptr(),
                component_triangles=count.data_ptr(), summary=summary.data_ptr(), stream=_hip.current_stream())

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_components(*[args[k] for k in names])

    for k in ("triangles", "labels", "component_triangles", "summary"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    for k in ("num_vertices", "num_triangles"):
        assert call(**{k: -1}) == -2 and call(**{k: 2 ** 31}) == -2, k  # TN_ERR_SHAPE
    for k in ("triangles", "labels", "component_triangles"):
        assert call(**{k: good[k] + 2}) == -2, k
    assert call(summary=good["summary"] + 4) == -2
    torch.cuda.synchronize()
    assert summary.tolist() == [-7, -8, -9] and (labels == FILL).all() and (count == FILL).all(), "a refused call launched something"
    # V == 0: the summary is zeroed, nothing else happens
    assert call(num_vertices=0, num_triangles=0, triangles=None, labels=None, component_triangles=None) == 0
    assert summary.tolist() == [0, 0, 0] and (labels == FILL).all()
    # T == 0: every vertex is its own label
    comp = mesh_components(torch.empty((0, 3), dtype=torch.int32, device=DEV), 300)
    assert comp.labels.tolist() == list(range(300)) and not comp.component_triangles.any() and comp.summary.tolist() == [300, 0, 0]
    counts = torch.tensor([-7, -9], dtype=torch.int64, device=DEV)
    filter_components(torch.empty((0, 3), dtype=torch.int32, device=DEV), 300, comp, counts=counts)
    assert counts.tolist() == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_components(tri.cpu(), v)
    with pytest.raises(ValueError):
        mesh_components(tri.reshape(-1), v)
    with pytest.raises(TypeError):
        mesh_components(tri.long(), v)


def test_filter_error_codes_without_a_launch():
    v, t, tri, comp, lib = _setup_calls()
    source = torch.full((v,), FILL, dtype=torch.int32, device=DEV)
    out = torch.full((t, 3), FILL, dtype=torch.int32, device=DEV)
    counts = torch.tensor([-7, -9], dtype=torch.int64, device=DEV)
    ws = torch.full((mesh_components_workspace_bytes(v, t),), 0xEE, dtype=torch.uint8, device=DEV)
    names = ("triangles", "num_triangles", "num_vertices", "labels", "component_triangles", "summary", "min_triangles", "largest_only",
             "vertex_source", "capacity_vertices", "triangles_out", "capacity_triangles", "counts", "workspace", "workspace_bytes",
             "stream")
    good = dict(triangles=tri.data_ptr(), num_triangles=t, num_vertices=v, labels=comp.labels.data_ptr(),
                component_triangles=comp.component_triangles.data_ptr(), summary=comp.summary.data_ptr(), min_triangles=2,
                largest_only=1, vertex_source=source.data_ptr(), capacity_vertices=v, triangles_out=out.data_ptr(),
                capacity_triangles=t, counts=counts.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                stream=_hip.current_stream())

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_filter_components(*[args[k] for k in names])

    for k in ("triangles", "labels", "component_triangles", "summary", "vertex_source", "triangles_out", "counts", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL (the summary: because largest_only is set)
    for k in ("num_vertices", "num_triangles"):
        assert call(**{k: -1}) == -2 and call(**{k: 2 ** 31}) == -2, k  # TN_ERR_SHAPE
    assert call(capacity_vertices=-1) == -2 and call(capacity_triangles=-1) == -2 and call(min_triangles=-1) == -2
    for k in ("triangles", "labels", "component_triangles", "vertex_source", "triangles_out"):
        assert call(**{k: good[k] + 2}) == -2, k
    for k in ("summary", "counts", "workspace"):
        assert call(**{k: good[k] + 4}) == -2, k
    assert call(workspace_bytes=ws.numel() - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    assert lib.tn_mesh_components_workspace_bytes(-1, 0) == 0 and lib.tn_mesh_components_workspace_bytes(0, 2 ** 31) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [-7, -9] and (source == FILL).all() and (out == FILL).all() and (ws == 0xEE).all(), \
        "a refused call launched something"
    # V == 0: the counts are zeroed, nothing else happens
    assert call(num_vertices=0, num_triangles=0, triangles=None, labels=None, component_triangles=None, workspace=None,
                workspace_bytes=0) == 0
    assert counts.tolist() == [0, 0] and (source == FILL).all()
    # a NULL summary is fine without largest_only
    assert call(summary=None, largest_only=0) == 0
    assert counts[0] > 0
    with pytest.raises(ValueError):
        filter_components(tri, v, comp, counts=counts, min_triangles=-1)
    with pytest.raises(ValueError):
        filter_components(tri, v + 1, comp, counts=counts)
    with pytest.raises(ValueError):
        filter_components(tri, v, comp, counts=counts, capacity_vertices=5)  # no vertex_source
    with pytest.raises(ValueError):
        filter_components(tri, v, comp, counts=counts, vertex_source=source, triangles_out=out, workspace=ws[:-8])


# ---- two spheres, independent of the yardstick ----------------------------------------------------------------------------------------

DIMS = (44, 24, 24)
BOX = ((-1.1, -0.6, -0.6), (1.1, 0.6, 0.6))
TRUNCATION = 0.2
LARGE, SMALL = ((-0.45, 0.0, 0.02), 0.43), ((0.72, 0.05, 0.0), 0.14)  # 9 cells of empty space between them


def sphere_volume(spheres):
    """a TSDF volume written directly: every grid point observed once, tsdf = min(1, sdf / truncation) of the union of the
    spheres; colour and temperature sums that depend on the grid point only, so that two volumes agree wherever their tsdf does"""
    nx, ny, nz = DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = [(BOX[0][c] + idx * ((BOX[1][c] - BOX[0][c]) / (DIMS[c] - 1))).astype(F) for c, idx in enumerate((i, j, k))]
    sdf = None
    for centre, radius in spheres:
        d = (np.sqrt(sum((p[c] - F(centre[c])) ** 2 for c in range(3))).astype(F) - F(radius)).astype(F)
        sdf = d if sdf is None else np.minimum(sdf, d)
    vol = np.zeros((7, nz, ny, nx), F)
    vol[0] = np.minimum(F(1.0), sdf / F(TRUNCATION)).astype(F)
    vol[1] = 1.0
    vol[6] = 1.0
    vol[2] = (0.5 + 0.4 * np.sin(0.3 * i + 0.2 * j)).astype(F)
    for ch in range(3):
        vol[3 + ch] = (0.5 + 0.4 * np.cos(0.25 * k + 0.1 * i + ch)).astype(F)
    return vol


def extract(vol):
    """the mesh of ``vol`` as MeshExporter.extract forms it: sizing call, one read, emitting call"""
    q = mesh_params(BOX[0], BOX[1], DIMS, TRUNCATION, max_temperature=33.0, min_temperature=14.0)
    volume = torch.from_numpy(vol).to(DEV)
    counts = torch.zeros((2,), dtype=torch.int64, device=DEV)
    workspace = torch.empty((mesh_workspace_bytes(DIMS),), dtype=torch.uint8, device=DEV)
    mesh_extract(volume, q, counts=counts, workspace=workspace)
    v, t = counts.tolist()
    mesh = ThermalMesh(torch.empty((v, 3), dtype=torch.float32, device=DEV), torch.empty((v, 3), dtype=torch.uint8, device=DEV),
                       torch.empty((v,), dtype=torch.float32, device=DEV), torch.empty((v, 3), dtype=torch.uint8, device=DEV),
                       torch.empty((t, 3), dtype=torch.int32, device=DEV), (14.0, 33.0))
    mesh_extract(volume, q, counts=counts, positions=mesh.positions, colors=mesh.colors, temperature=mesh.temperature,
                 thermal_colors=mesh.thermal_colors, thermal_table=colormaps.get_table("magma", torch.device(DEV))[1],
                 triangles=mesh.triangles, workspace=workspace)
    return mesh


def same_mesh(a, b):
    for key in ("positions", "colors", "temperature", "thermal_colors", "triangles"):
        assert getattr(a, key).cpu().numpy().tobytes() == getattr(b, key).cpu().numpy().tobytes(), key
    assert a.temperature_bounds == b.temperature_bounds


def test_two_spheres_without_the_small_one_equal_the_large_one_alone():
    both, alone = extract(sphere_volume([LARGE, SMALL])), extract(sphere_volume([LARGE]))
    v, t = len(both), int(both.triangles.shape[0])
    large_t = int(alone.triangles.shape[0])
    small_t = t - large_t
    assert 0 < small_t < large_t and len(alone) < v
    comp = mesh_components(both.triangles, v)
    assert comp.summary.tolist()[:2] == [2, large_t], "exactly two components before the filter"
    assert sorted(comp.component_triangles[comp.component_triangles > 0].tolist()) == [small_t, large_t]
    assert mesh_components(alone.triangles, len(alone)).summary.tolist() == [1, large_t, 0]
    min_triangles = (small_t + large_t) // 2
    assert small_t < min_triangles <= large_t
    got, info = remove_small_components(both, min_triangles=min_triangles)
    same_mesh(got, alone)
    assert info == ComponentsInfo(components=2, largest_triangles=large_t, vertices_removed=v - len(alone), triangles_removed=small_t)
    got, info = remove_small_components(both, largest_only=True)  # --largest-component
    same_mesh(got, alone)
    assert info.components == 2 and info.triangles_removed == small_t
    got, info = remove_small_components(both, min_triangles=1)  # nothing is small enough: the mesh itself
    same_mesh(got, both)
    assert info.vertices_removed == 0 and info.triangles_removed == 0
    got, info = remove_small_components(both, min_triangles=large_t + 1)  # everything goes
    assert len(got) == 0 and got.triangles.shape == (0, 3) and info.triangles_removed == t


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_tree(root):
    """10 frames of 32 x 32 from the analytic scene: 8 train, 2 eval (a copy of the tree of tests/test_gpu_mesh.py)"""
    from thermo_nerf_amd import synthetic

    res, n = 32, 10
    cams = synthetic.orbit_cameras(res, res, list(range(n)), num_views=n, elevation_deg=[(0.0, 25.0)[v % 2] for v in range(n)])
    (root / "images").mkdir(parents=True)
    (root / "thermal").mkdir()
    frames = []
    for i in range(n):
        rb = cams.generate_rays(i, device=DEV)
        rgb, th = synthetic.analytic_scene(rb.origins, rb.directions)
        name = f"frame_{'eval' if i % 5 == 4 else 'train'}_{i:04d}.png"
        Image.fromarray((rgb.cpu().numpy() * 255).round().astype(np.uint8)).save(root / "images" / name)
        Image.fromarray((th[..., 0].cpu().numpy() * 255).round().astype(np.uint8), mode="L").save(root / "thermal" / name)
        c2w = torch.cat([cams.camera_to_worlds[i], torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}", "transform_matrix": c2w})
    f = float(cams.fx[0])
    (root / "transforms.json").write_text(json.dumps(
        {"fl_x": f, "fl_y": f, "cx": res / 2, "cy": res / 2, "w": res, "h": res, "frames": frames}))


def test_command_line_removes_the_components_the_exporter_removes(tmp_path, capsys):
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
    plain, filtered, want_file = tmp_path / "plain.ply", tmp_path / "filtered.ply", tmp_path / "want.ply"

    # without the flags: the bytes of the exporter's unfiltered mesh, and no new line
    exporter, cameras, adjust = tool.build_exporter(tool.parse(common + ["--output", str(plain)]))
    mesh = exporter.export(cameras, apply_camera_optimizer=adjust)
    assert exporter.last_components is None
    capsys.readouterr()
    assert tool.main(common + ["--output", str(plain)]) == 0
    printed = capsys.readouterr().out
    assert "components found" not in printed and f"vertices {len(mesh)}, triangles {int(mesh.triangles.shape[0])}" in printed
    write_mesh_ply(want_file, mesh)
    assert plain.read_bytes() == want_file.read_bytes()

    # with --min-component-triangles: the exporter's filtered mesh, and the new line
    _, found = remove_small_components(mesh, largest_only=True)
    n = max(2, found.largest_triangles // 2)
    kept = exporter.export(cameras, apply_camera_optimizer=adjust, min_component_triangles=n)
    info = exporter.last_components
    assert info is not None and info.components == found.components and info.largest_triangles == found.largest_triangles
    assert len(kept) == len(mesh) - info.vertices_removed and int(kept.triangles.shape[0]) == int(mesh.triangles.shape[0]) - info.triangles_removed
    assert tool.main(common + ["--output", str(filtered), "--min-component-triangles", str(n)]) == 0
    printed = capsys.readouterr().out
    print(printed)
    assert (f"components found {info.components}, largest {info.largest_triangles} triangles, removed vertices {info.vertices_removed}, "
            f"triangles {info.triangles_removed}") in printed
    assert f"vertices {len(kept)}, triangles {int(kept.triangles.shape[0])}" in printed
    got = read_mesh_ply(filtered)
    for key in ("positions", "colors", "temperature", "triangles"):
        assert got[key].tobytes() == getattr(kept, key).cpu().numpy().tobytes(), key
    t = int(kept.triangles.shape[0])
    assert t == 0 or (got["triangles"].min() >= 0 and got["triangles"].max() < len(kept))
