"""GPU: tn_tsdf_integrate and tn_mesh_extract against their numpy restatement (tests/mesh_reference.py), bit for bit — grid extents
around the wave and the tile, the five classes of a voxel, edge values, unaligned views; cell counts around the tile and the scan
block's pass, the 3 x 3 x 3 patterns, capacities below the counts, the sizing call, the optional output, the world transform, the
error codes; the analytic sphere scene; camera_pose against the adjusted rays; then MeshExporter end to end and the command line
on a small trained run."""
import copy
import importlib.util
import json
import math
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests import helpers
from tests import mesh_reference as R
from thermo_nerf_amd import _hip, colormaps
from thermo_nerf_amd.export import (MeshExporter, PointCloudExporter, camera_pose, mesh_extract, mesh_params, mesh_scan_width,
                                    mesh_tile, mesh_workspace_bytes, read_mesh_ply, set_camera, tsdf_integrate, world_transform)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 96  # rows behind every output buffer that must keep their pattern
PATTERN = dict(positions=-777.0, colors=0xAB, temperature=-777.0, thermal_colors=0xCD, triangles=-5)
TABLE = colormaps.table_u8("magma")
BOX = ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8))
TRUNCATION = 0.3


# ---- fusion -------------------------------------------------------------------------------------------------------------------------

def _cameras():
    """two poses inside the box that see a common part of it: voxels behind each, outside its 16 x 16 image, and at every distance"""
    a = R.look_at((0.15, -0.1, 0.35), target=(0.0, 0.1, -1.0), up=(0.0, 1.0, 0.0))
    b = R.look_at((-0.7, -0.5, 0.1), target=(0.4, 0.3, -0.8), up=(0.0, 0.0, 1.0))
    return [(9.3, 8.9, 8.25, 7.75, a), (6.1, 6.4, 7.5, 8.5, b)]


def random_pose(seed, size=16):
    rng = np.random.default_rng(seed)
    n = size * size
    return dict(depth=rng.uniform(0.3, 1.9, n).astype(F), accumulation=rng.uniform(0.3, 1.0, n).astype(F),
                thermal=rng.uniform(-0.05, 1.05, n).astype(F), rgb=rng.uniform(-0.05, 1.05, (n, 3)).astype(F), height=size, width=size)


def aimed_pose(seed, dims, camera, size=16):
    """a random pose whose depth is set where the grid's voxels land: the in-image voxels in turn get a surface 2 truncations in
    front of them (beyond -truncation), 0.4 behind (near) and 3 behind (far, clamped to 1), so that a grid of a few voxels still
    meets every class; three pixels in four of those are opaque"""
    pose = random_pose(seed, size)
    q = R.params(BOX[0], BOX[1], dims, TRUNCATION, camera=camera)
    front, u, v, c = R.project(q, R.grid_points(q))
    ok = np.nonzero(front & (u >= 0) & (u < size) & (v >= 0) & (v < size))[0]
    pix = v[ok].astype(np.int64) * size + u[ok].astype(np.int64)
    dist = np.sqrt(sum(x[ok].astype(np.float64) ** 2 for x in c))
    turn = np.arange(len(ok))
    pose["depth"][pix] = (dist + TRUNCATION * np.array([-2.0, 0.4, 3.0])[turn % 3]).astype(F)
    pose["accumulation"][pix] = np.where(turn % 4 == 3, pose["accumulation"][pix], F(0.9))
    return pose


def upload_pose(pose, lead=0):
    """device tensors of the pose's arrays; ``lead`` > 0: as views that start at element ``lead`` (per row) of a larger allocation"""
    out = {}
    for k in ("depth", "accumulation", "thermal", "rgb"):
        v = pose[k]
        big = torch.full((v.shape[0] + lead + 1,) + v.shape[1:], float("nan"), dtype=torch.float32, device=DEV)
        big[lead:lead + v.shape[0]] = torch.from_numpy(v).to(DEV)
        out[k] = big[lead:lead + v.shape[0]]
    return out


def fuse_both(dims, poses, cameras, lead=0, min_accumulation=0.5):
    """(device volume, reference volume, the reference's class masks per pose) after fusing ``poses`` in sequence"""
    kw = dict(lo=BOX[0], hi=BOX[1], dims=dims, truncation=TRUNCATION, min_accumulation=min_accumulation)
    q, qr = mesh_params(**kw), R.params(**kw)
    nx, ny, nz = dims
    n = nx * ny * nz
    # the volume sits between two guard stretches of a larger allocation
    big = torch.zeros((7 * n + 2 * GUARD,), dtype=torch.float32, device=DEV)
    big[:GUARD] = -777.0
    big[GUARD + 7 * n:] = -777.0
    volume = big[GUARD:GUARD + 7 * n].view(7, nz, ny, nx)
    want = np.zeros((7, nz, ny, nx), F)
    classes = []
    for pose, camera in zip(poses, cameras):
        set_camera(q, *camera)
        t = upload_pose(pose, lead)
        tsdf_integrate(t["depth"], t["accumulation"], t["thermal"], t["rgb"], pose["height"], pose["width"], q, volume)
        classes.append(R.integrate(want, pose, dict(qr, **R.camera_params(*camera))))
    got = big.cpu().numpy()
    assert (got[:GUARD] == F(-777.0)).all() and (got[GUARD + 7 * n:] == F(-777.0)).all(), "written outside the volume"
    return got[GUARD:GUARD + 7 * n].reshape(7, nz, ny, nx), want, classes


@pytest.mark.parametrize("dims", [(2, 2, 2), (63, 3, 2), (64, 3, 2), (65, 5, 3), (257, 2, 2)])
def test_integrate_two_poses_in_sequence(dims):
    cameras = _cameras()
    poses = [aimed_pose(10 + dims[0], dims, cameras[0]), aimed_pose(20 + dims[0], dims, cameras[1])]
    got, want, classes = fuse_both(dims, poses, cameras)
    for name in ("behind", "outside", "beyond", "far", "near"):
        assert any(c[name].any() for c in classes), f"no voxel of class {name!r}: the case does not cover it"
    assert (want[1] == 2).any() and (want[6] == 2).any(), "some voxel is fused by both poses, with colour"
    for plane in range(7):
        assert got[plane].tobytes() == want[plane].tobytes(), f"plane {plane} differs from the reference"


def test_integrate_edge_values_and_unaligned_views():
    dims = (65, 5, 3)
    cameras = _cameras()
    poses = [random_pose(31), random_pose(32)]
    for pose in poses:
        pix = np.arange(256)
        pose["accumulation"][pix % 4 == 1] = F(0.5)      # == min_accumulation: skipped
        pose["depth"][pix % 8 == 2] = F("nan")            # skipped
        pose["depth"][pix % 8 == 6] = F("inf")            # sdf = +inf: skipped
        pose["accumulation"][pix % 16 == 3] = F("inf")    # fused: +inf > 0.5
        pose["accumulation"][pix % 16 == 11] = F("nan")   # skipped
    qr = R.params(BOX[0], BOX[1], dims, TRUNCATION)
    hit = set()
    for pose, camera in zip(poses, cameras):  # the reference's own projection: which pixels do voxels land on?
        front, u, v, _ = R.project(dict(qr, **R.camera_params(*camera)), R.grid_points(qr))
        ok = front & (u >= 0) & (u < 16) & (v >= 0) & (v < 16)
        hit |= set((v[ok].astype(np.int64) * 16 + u[ok].astype(np.int64)).tolist())
    for name, sel in (("accumulation == min", lambda p: p % 4 == 1), ("NaN depth", lambda p: p % 8 == 2),
                      ("+inf depth", lambda p: p % 8 == 6), ("+inf accumulation", lambda p: p % 16 == 3),
                      ("NaN accumulation", lambda p: p % 16 == 11)):
        assert any(sel(p) for p in hit), f"no voxel lands on a pixel with {name}"
    for lead in (0, 1, 3):
        t = upload_pose(poses[0], lead)
        assert lead == 0 or (t["depth"].data_ptr() % 16 != 0 and t["rgb"].data_ptr() % 16 != 0)
        got, want, classes = fuse_both(dims, poses, cameras, lead=lead)
        assert all(c["transparent"].any() and c["beyond"].any() and c["near"].any() for c in classes)
        for plane in range(7):
            assert got[plane].tobytes() == want[plane].tobytes(), (lead, plane)


# ---- extraction ---------------------------------------------------------------------------------------------------------------------

def random_volume(dims, seed, observed=0.9):
    """written directly: tsdf_sum of either sign, fp32 counts as weights (0 = unobserved), positive colour weights"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    shape = (nz, ny, nx)
    vol = np.zeros((7,) + shape, F)
    vol[1] = np.where(rng.uniform(size=shape) < observed, rng.integers(1, 4, shape), 0).astype(F)
    vol[0] = (rng.uniform(-1, 1, shape) * vol[1]).astype(F)
    vol[6] = rng.integers(1, 4, shape).astype(F)
    vol[2] = (rng.uniform(-0.05, 1.05, shape) * vol[6]).astype(F)
    for ch in range(3):
        vol[3 + ch] = (rng.uniform(-0.05, 1.05, shape) * vol[6]).astype(F)
    return vol


def smooth_volume(dims, seed):
    """a blobby field: many quads (random signs give active cells everywhere but few edges whose four cells are all active)"""
    nx, ny, nz = dims
    vol = random_volume(dims, seed, observed=0.995)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    field = np.sin(0.9 * i + 0.3) * np.cos(0.7 * j) + np.sin(0.8 * k + 0.5 * i) * 0.7 + 0.1
    vol[0] = (field * vol[1]).astype(F)
    return vol


def buffers(cap_v, cap_t):
    return dict(positions=torch.full((cap_v + GUARD, 3), PATTERN["positions"], dtype=torch.float32, device=DEV),
                colors=torch.full((cap_v + GUARD, 3), PATTERN["colors"], dtype=torch.uint8, device=DEV),
                temperature=torch.full((cap_v + GUARD,), PATTERN["temperature"], dtype=torch.float32, device=DEV),
                thermal_colors=torch.full((cap_v + GUARD, 3), PATTERN["thermal_colors"], dtype=torch.uint8, device=DEV),
                triangles=torch.full((cap_t + GUARD, 3), PATTERN["triangles"], dtype=torch.int32, device=DEV),
                counts=torch.tensor([-7, -9], dtype=torch.int64, device=DEV))


def extract_both(vol, dims, cap_v=None, cap_t=None, thermal_colors=True, **kw):
    """run the kernel and the reference on ``vol``; check the counts, every row below the capacities, the pattern everywhere
    else (the guard rows included) and the complete cell_index; returns the reference's mesh"""
    kw = dict(dict(lo=BOX[0], hi=BOX[1], dims=dims, truncation=TRUNCATION, max_temperature=33.0, min_temperature=14.0), **kw)
    q, qr = mesh_params(**kw), R.params(**kw)
    want = R.extract(vol, qr, TABLE)
    v, t = len(want["positions"]), len(want["triangles"])
    cap_v, cap_t = v if cap_v is None else cap_v, t if cap_t is None else cap_t
    b = buffers(cap_v, cap_t)
    need = mesh_workspace_bytes(dims)
    workspace = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    mesh_extract(torch.from_numpy(vol).to(DEV), q, counts=b["counts"], positions=b["positions"], colors=b["colors"],
                 temperature=b["temperature"], thermal_colors=b["thermal_colors"] if thermal_colors else None,
                 thermal_table=torch.from_numpy(TABLE).to(DEV) if thermal_colors else None, triangles=b["triangles"],
                 capacity_vertices=cap_v, capacity_triangles=cap_t, workspace=workspace)
    assert b["counts"].tolist() == [v, t], (b["counts"].tolist(), v, t)
    for k, fill in PATTERN.items():
        got = b[k].cpu().numpy()
        if k == "thermal_colors" and not thermal_colors:
            assert (got == got.dtype.type(fill)).all(), "thermal_colors was not passed and must be untouched"
            continue
        end = min(t, cap_t) if k == "triangles" else min(v, cap_v)
        assert got[:end].tobytes() == want[k][:end].tobytes(), f"{k} differs from the reference"
        assert (got[end:] == got.dtype.type(fill)).all(), f"{k} was written at or beyond row {end}"
    ws = workspace.cpu().numpy()
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    assert ws[:4 * cells].view(np.int32).tobytes() == want["cell_index"].tobytes(), "cell_index is incomplete"
    assert (ws[need:] == 0xEE).all(), "written beyond the workspace"
    return want


def test_extract_cell_counts_around_the_tile():
    tile = mesh_tile()
    assert tile == 256
    for nx in (2, tile, tile + 1, tile + 2):  # 1, 255, 256, 257 cells
        want = extract_both(random_volume((nx, 2, 2), seed=nx), (nx, 2, 2))
        assert nx == 2 or 0.2 * (nx - 1) < len(want["positions"]) < 0.8 * (nx - 1)
    want = extract_both(smooth_volume((9, 70, 6), seed=3), (9, 70, 6))  # several tiles of cells and of points, with quads
    assert len(want["positions"]) > 500 and len(want["triangles"]) > 500


def test_extract_two_scan_passes_for_cells_and_points():
    tile, width = mesh_tile(), mesh_scan_width()
    dims = (65, 65, 66)
    cells, points = 64 * 64 * 65, 65 * 65 * 66
    assert cells >= tile * width + tile + 5 and points > cells  # a second pass: one whole tile and a partial one, at least
    assert mesh_workspace_bytes(dims) == 4 * cells + 8 * (-(-cells // tile) + -(-points // tile))
    want = extract_both(smooth_volume(dims, seed=4), dims)
    last = np.nonzero(want["cell_index"] >= 0)[0][-1]
    assert last >= tile * width, "an active cell lies in the scan's second pass"
    assert len(want["triangles"]) > 10000 and want["triangles"].max() > tile * width // 8


def test_extract_the_three_cubed_patterns():
    cube = extract_both(R.volume3(), (3, 3, 3))
    assert cube["positions"].shape == (8, 3) and cube["triangles"].shape == (12, 3)
    assert R.mesh_topology(cube["triangles"], 8) == dict(edges=18, bad_edges=0, inconsistent=0, euler=2, unused=0)
    empty = extract_both(np.zeros((7, 3, 3, 3), F), (3, 3, 3))
    assert len(empty["positions"]) == 0 and len(empty["triangles"]) == 0
    full = extract_both(R.volume3(inside=[(i, j, k) for i in range(3) for j in range(3) for k in range(3)]), (3, 3, 3))
    assert len(full["positions"]) == 0 and len(full["triangles"]) == 0
    one = extract_both(R.volume3(unobserved=[(0, 0, 0)]), (3, 3, 3))
    assert one["cell_index"].tolist() == [-1, 0, 1, 2, 3, 4, 5, 6] and len(one["triangles"]) == 6


def test_extract_capacities_below_the_counts_sizing_call_and_optional_output():
    dims = (9, 70, 6)
    vol = smooth_volume(dims, seed=5)
    full = extract_both(vol, dims)
    v, t = len(full["positions"]), len(full["triangles"])
    for cap_v, cap_t in ((v // 2, t // 2 | 1), (v - 1, t - 1), (1, 1), (0, 0), (v, 0), (0, t)):
        extract_both(vol, dims, cap_v=cap_v, cap_t=cap_t)  # the counts stay full, nothing lands beyond, cell_index is complete
    extract_both(vol, dims, thermal_colors=False)
    # the sizing call: null outputs, both capacities 0
    q = mesh_params(BOX[0], BOX[1], dims, TRUNCATION)
    counts = torch.tensor([-7, -9], dtype=torch.int64, device=DEV)
    mesh_extract(torch.from_numpy(vol).to(DEV), q, counts=counts)
    assert counts.tolist() == [v, t]


def test_extract_world_transform_rotation_scale_offset():
    a, b = 0.7, -0.4
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    m = np.concatenate([3.7 * (rz @ rx), np.array([[10.5], [-4.25], [0.3]])], axis=1)
    dims = (9, 70, 6)
    vol = smooth_volume(dims, seed=6)
    moved = extract_both(vol, dims, to_world=m)
    plain = extract_both(vol, dims)
    assert np.abs(moved["positions"]).max() > 3.0 and np.abs(plain["positions"]).max() <= 1.0
    assert np.array_equal(moved["triangles"], plain["triangles"]) and np.array_equal(moved["temperature"], plain["temperature"])


def test_error_codes_without_a_launch():
    dims = (9, 7, 6)
    vol = smooth_volume(dims, seed=7)
    q = mesh_params(BOX[0], BOX[1], dims, TRUNCATION, camera=_cameras()[0])
    b = buffers(400, 800)
    table = torch.from_numpy(TABLE).to(DEV)
    volume = torch.from_numpy(vol).to(DEV)
    ws = torch.empty(mesh_workspace_bytes(dims), dtype=torch.uint8, device=DEV)
    lib = _hip.load()
    names = ("volume", "params", "thermal_table", "positions", "colors", "temperature", "thermal_colors", "capacity_vertices",
             "triangles", "capacity_triangles", "counts", "workspace", "workspace_bytes", "stream")
    good = dict(volume=volume.data_ptr(), params=q, thermal_table=table.data_ptr(), positions=b["positions"].data_ptr(),
                colors=b["colors"].data_ptr(), temperature=b["temperature"].data_ptr(), thermal_colors=b["thermal_colors"].data_ptr(),
                capacity_vertices=400, triangles=b["triangles"].data_ptr(), capacity_triangles=800, counts=b["counts"].data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=ws.numel(), stream=_hip.current_stream())

    def call(**change):
        args = dict(good, **change)
        return lib.tn_mesh_extract(*[args[k] for k in names])

    def with_dims(*d):
        bad = mesh_params(BOX[0], BOX[1], (2, 2, 2), TRUNCATION)
        bad.dims[0], bad.dims[1], bad.dims[2] = d
        return bad

    for k in ("volume", "params", "thermal_table", "positions", "colors", "temperature", "triangles", "counts", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL (the table: because thermal_colors is asked for)
    assert call(capacity_vertices=-1) == -2 and call(capacity_triangles=-1) == -2  # TN_ERR_SHAPE
    assert call(params=with_dims(1, 7, 6)) == -2 and call(params=with_dims(9, 7, 0)) == -2
    assert call(params=with_dims(2048, 2048, 512)) == -3  # 2^31 grid points: TN_ERR_UNSUPPORTED
    for k in ("volume", "positions", "temperature", "triangles"):
        assert call(**{k: good[k] + 2}) == -2, k
    for k in ("counts", "workspace"):
        assert call(**{k: good[k] + 4}) == -2, k
    assert call(workspace_bytes=ws.numel() - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    assert lib.tn_mesh_workspace_bytes(1, 7, 6) == 0 and lib.tn_mesh_workspace_bytes(2048, 2048, 512) == 0

    pose = upload_pose(random_pose(8))
    target = torch.full((7, 6, 7, 9), -777.0, dtype=torch.float32, device=DEV)
    inames = ("depth", "accumulation", "thermal", "rgb", "height", "width", "params", "volume", "stream")
    igood = dict(depth=pose["depth"].data_ptr(), accumulation=pose["accumulation"].data_ptr(), thermal=pose["thermal"].data_ptr(),
                 rgb=pose["rgb"].data_ptr(), height=16, width=16, params=q, volume=target.data_ptr(), stream=_hip.current_stream())

    def icall(**change):
        args = dict(igood, **change)
        return lib.tn_tsdf_integrate(*[args[k] for k in inames])

    for k in ("depth", "accumulation", "thermal", "rgb", "params", "volume"):
        assert icall(**{k: None}) == -1, k
    for k in ("depth", "accumulation", "thermal", "rgb", "volume"):
        assert icall(**{k: igood[k] + 2}) == -2, k
    assert icall(height=0) == -2 and icall(width=-1) == -2 and icall(height=1 << 16, width=1 << 15) == -2
    assert icall(params=with_dims(9, 1, 6)) == -2 and icall(params=with_dims(2048, 2048, 512)) == -3
    torch.cuda.synchronize()
    assert b["counts"].tolist() == [-7, -9], "a refused call launched something"
    for k, fill in PATTERN.items():
        got = b[k].cpu().numpy()
        assert (got == got.dtype.type(fill)).all(), k
    assert (target == -777.0).all()
    # the Python wrappers refuse before the library is reached
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_extract(torch.from_numpy(vol), q, counts=b["counts"])
    with pytest.raises(ValueError):
        mesh_extract(volume[:6], q, counts=b["counts"])
    with pytest.raises(ValueError):
        mesh_extract(volume, q, counts=b["counts"], positions=b["positions"])  # no colours / temperature
    with pytest.raises(ValueError):
        mesh_extract(volume, q, counts=b["counts"], positions=b["positions"], colors=b["colors"], temperature=b["temperature"],
                     thermal_colors=b["thermal_colors"])  # no table
    with pytest.raises(ValueError):
        tsdf_integrate(pose["depth"][:4], pose["accumulation"], pose["thermal"], pose["rgb"], 16, 16, q, target)
    with pytest.raises(ValueError):
        tsdf_integrate(pose["depth"], pose["accumulation"], pose["thermal"], pose["rgb"], 16, 16, q, target[:, :, :, :8])


# ---- the sphere scene ---------------------------------------------------------------------------------------------------------------

def test_sphere_scene_through_the_kernels_equals_the_reference():
    """bit-equal to the mesh tests/test_mesh_cpu.py proves watertight, outward and within half a voxel"""
    qr, poses = R.sphere_scene()
    want_volume, want = R.sphere_mesh()
    s = R.SPHERE
    step = 2 * s["half"] / (s["grid"] - 1)
    q = mesh_params((-s["half"],) * 3, (s["half"],) * 3, (s["grid"],) * 3, s["truncation_steps"] * step)
    volume = torch.zeros((7,) + (s["grid"],) * 3, dtype=torch.float32, device=DEV)
    for camera, pose in poses:
        set_camera(q, *camera)
        t = upload_pose(pose)
        tsdf_integrate(t["depth"], t["accumulation"], t["thermal"], t["rgb"], pose["height"], pose["width"], q, volume)
    got = volume.cpu().numpy()
    for plane in range(7):
        assert got[plane].tobytes() == want_volume[plane].tobytes(), f"plane {plane} differs from the reference"
    mesh = extract_both(np.ascontiguousarray(want_volume), (s["grid"],) * 3, lo=(-s["half"],) * 3, hi=(s["half"],) * 3,
                        truncation=s["truncation_steps"] * step, max_temperature=1.0, min_temperature=0.0)
    for k in ("positions", "colors", "temperature", "thermal_colors", "triangles"):
        assert mesh[k].tobytes() == want[k].tobytes(), k
    assert R.mesh_topology(mesh["triangles"], len(mesh["positions"]))["bad_edges"] == 0


# ---- camera_pose --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_camera_pose_is_the_pose_the_adjusted_rays_are_cast_from(mode):
    from thermo_nerf_amd import synthetic
    from thermo_nerf_amd.camera_optimizer import CameraOptimizerConfig

    size = 32
    cameras = synthetic.orbit_cameras(size, size, [0, 1, 2, 3], num_views=4, elevation_deg=[0.0, 25.0, -10.0, 40.0])
    opt = CameraOptimizerConfig(mode=mode).setup(4, device=DEV)
    rows = np.random.default_rng(9).uniform(-0.15, 0.15, (4, 6))
    rows[3, 3:] = 1e-3  # |w|^2 below the clamp
    with torch.no_grad():
        opt.pose_adjustment.copy_(torch.from_numpy(rows).float())
    model = types.SimpleNamespace(camera_optimizer=opt)
    row, col = np.divmod(np.arange(size * size), size)
    for k in range(4):
        rb = cameras.generate_rays(k, device=DEV, flat=True)
        plain = rb.origins.clone()
        with torch.no_grad():
            opt.apply_to_raybundle(rb)
        assert not torch.equal(plain, rb.origins), "the adjustment moves the camera"
        p = (rb.origins.double() + 0.7 * rb.directions.double()).cpu().numpy().astype(F)
        pose = camera_pose(model, cameras, k, True)
        assert pose.dtype == np.float64 and pose.shape == (3, 4)
        q = R.camera_params(float(cameras.fx[k]), float(cameras.fy[k]), cameras.cx, cameras.cy, pose)
        front, u, v, _ = R.project(q, [p[:, 0], p[:, 1], p[:, 2]])
        assert front.all()
        assert np.array_equal(v.astype(np.int64), row) and np.array_equal(u.astype(np.int64), col), (mode, k)
        # pixel centres sit half a pixel from any boundary: the projection lands near them
        assert np.abs(u - (col + 0.5)).max() < 0.01 and np.abs(v - (row + 0.5)).max() < 0.01
        assert np.array_equal(camera_pose(model, cameras, k, False), cameras.camera_to_worlds[k].double().numpy())


# ---- the exporter -------------------------------------------------------------------------------------------------------------------

def _pose_outputs(model, cameras, k, engine, adjust=True):
    rb = cameras.generate_rays(k, device=DEV, flat=True)
    if adjust:
        model.camera_optimizer.apply_to_raybundle(rb)
    out = engine.render(rb.origins, rb.directions)
    return {key: v.clone() for key, v in out.items()}


def _reference_mesh(model, cameras, exporter, engine, adjust=True, box=None, to_world=None, min_accumulation=0.5):
    """the reference run on the engine's own outputs of every camera"""
    lo, hi = box
    qr = R.params(lo, hi, exporter.dims, exporter.truncation, min_accumulation, exporter.temperature_bounds[1],
                  exporter.temperature_bounds[0], to_world=to_world)
    volume = np.zeros((7,) + exporter.dims[::-1], F)
    for k in range(cameras.size):
        with torch.no_grad():
            out = _pose_outputs(model, cameras, k, engine, adjust)
        pose = dict(depth=out["depth"].cpu().numpy(), accumulation=out["accumulation"].cpu().numpy(),
                    thermal=out["thermal"].cpu().numpy(), rgb=out["rgb"].cpu().numpy(), height=cameras.height, width=cameras.width)
        camera = (float(cameras.fx[k]), float(cameras.fy[k]), cameras.cx, cameras.cy, camera_pose(model, cameras, k, adjust))
        R.integrate(volume, pose, dict(qr, **R.camera_params(*camera)))
    return volume, R.extract(volume, qr, TABLE)


def test_exporter_end_to_end_equals_the_reference_on_the_engines_outputs():
    from thermo_nerf_amd import synthetic
    from thermo_nerf_amd.engine import RayRenderEngine

    cpu_model, _, _ = helpers.build("scene", 48)
    model = copy.deepcopy(cpu_model).to(DEV).eval()
    cameras = synthetic.orbit_cameras(32, 32, [0, 1, 2, 3], num_views=4, elevation_deg=[0.0, 25.0, 0.0, 25.0])
    engine = RayRenderEngine(model, chunk=int(model.config.eval_num_rays_per_chunk))
    kw = dict(max_temperature=33.0, min_temperature=14.0, resolution=32)
    box = model.scene_box.aabb.cpu().double().tolist()
    exporter = MeshExporter(model, **kw)
    mesh = exporter.export(cameras)
    print("scene box", box, "dims", exporter.dims, "vertices", len(mesh), "triangles", int(mesh.triangles.shape[0]))
    if mesh.triangles.shape[0] == 0:  # no surface inside the scene box for these weights: the box of the cloud of the same cameras
        cloud = PointCloudExporter(model, max_temperature=33.0, min_temperature=14.0, bounding_box=None).export(cameras)
        box = [cloud.positions.min(dim=0).values.cpu().double().tolist(), cloud.positions.max(dim=0).values.cpu().double().tolist()]
        exporter = MeshExporter(model, bounding_box=box, **kw)
        mesh = exporter.export(cameras)
        print("cloud box", box, "dims", exporter.dims, "vertices", len(mesh), "triangles", int(mesh.triangles.shape[0]))
    assert mesh.triangles.shape[0] > 0 and len(mesh) > 0
    volume, want = _reference_mesh(model, cameras, exporter, engine, box=box)
    assert exporter.fuse(cameras).cpu().numpy().tobytes() == volume.tobytes()
    for key in ("positions", "colors", "temperature", "thermal_colors", "triangles"):
        assert getattr(mesh, key).cpu().numpy().tobytes() == want[key].tobytes(), key
    assert exporter.last_poses == 4 and mesh.temperature_bounds == (14.0, 33.0) and mesh.triangles.dtype == torch.int32
    # a subset of the cameras, in the order given
    two = exporter.export(cameras, camera_indices=[2, 0])
    assert exporter.last_poses == 2 and len(two) > 0
    # refusals
    with pytest.raises(ValueError, match="bounding box"):
        MeshExporter(model, bounding_box=None, **kw)
    with pytest.raises(ValueError, match="sqrt"):
        MeshExporter(model, bounding_box=box, truncation=1.5 * max(exporter.params.step), **kw)
    with pytest.raises(IndexError):
        exporter.export(cameras, camera_indices=[4])
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        exporter.export(cameras)
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshExporter(cpu_model, **kw).export(cameras)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_tree(root):
    """10 frames of 32 x 32 from the analytic scene: 8 train, 2 eval (a copy of the tree of tests/test_gpu_pointcloud.py)"""
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


def test_command_line_writes_the_mesh_the_exporter_computes(tmp_path, capsys):
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
    world, again, scene = tmp_path / "world.ply", tmp_path / "again.ply", tmp_path / "scene.ply"
    capsys.readouterr()
    assert tool.main(common + ["--output", str(world)]) == 0
    printed = capsys.readouterr().out
    print(printed)
    assert "poses fused 8" in printed and "vertices" in printed and "triangles" in printed and "temperature min" in printed
    assert tool.main(common + ["--output", str(again)]) == 0
    assert again.read_bytes() == world.read_bytes()  # a second run: the same bytes
    assert tool.main(common + ["--output", str(scene), "--scene-frame", "--colors", "thermal"]) == 0

    # the same mesh in-process
    exporter, cameras, adjust = tool.build_exporter(tool.parse(common + ["--output", str(world)]))
    assert adjust and cameras.size == 8 and max(exporter.dims) == 24
    mesh = exporter.export(cameras, apply_camera_optimizer=adjust)
    got = read_mesh_ply(world)
    v, t = len(mesh), int(mesh.triangles.shape[0])
    assert f"vertices {v}, triangles {t}" in printed
    for key in ("positions", "colors", "temperature", "triangles"):
        assert got[key].tobytes() == getattr(mesh, key).cpu().numpy().tobytes(), key
    assert got["comments"] == ["temperature_unit celsius", "temperature_bounds 14.0 33.0"]
    assert np.isfinite(got["positions"]).all() and np.isfinite(got["temperature"]).all()
    assert ((got["temperature"] >= 14.0) & (got["temperature"] <= 33.0)).all(), "degrees lie within the bounds"
    assert got["triangles"].shape == (t, 3) and (t == 0 or (got["triangles"].min() >= 0 and got["triangles"].max() < v))

    # --scene-frame: the normalised frame; the world frame is world_transform of it; the faces and degrees are the same
    from thermo_nerf_amd.data import ThermalDataParserConfig

    got_scene = read_mesh_ply(scene)
    assert got_scene["colors"].tobytes() == mesh.thermal_colors.cpu().numpy().tobytes()
    assert got_scene["triangles"].tobytes() == got["triangles"].tobytes() and got_scene["temperature"].tobytes() == got["temperature"].tobytes()
    parsed = ThermalDataParserConfig(data=data).setup().get_dataparser_outputs("train")
    m = world_transform(parsed).numpy()
    p = got_scene["positions"]
    moved = np.stack([(((m[c, 0] * p[:, 0]).astype(F) + (m[c, 1] * p[:, 1]).astype(F)).astype(F) + (m[c, 2] * p[:, 2]).astype(F)).astype(F)
                      + m[c, 3] for c in range(3)], axis=1).astype(F)
    assert moved.tobytes() == got["positions"].tobytes()
    box = parsed.scene_box.aabb.double()
    assert v == 0 or ((torch.from_numpy(p).double() >= box[0]) & (torch.from_numpy(p).double() <= box[1])).all()
