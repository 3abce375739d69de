"""Test-side yardstick of the mesh export (tn_tsdf_integrate, tn_mesh_extract): a numpy restatement of the definitions in
include/thermonerf_hip.h with explicit float32 steps in the stated order — the fusion of a pose into the volume, the active
cells and their surface-net vertices, the quads in (grid point, axis) order, degrees, and the SCALE / LUT bytes.  numpy's float32
`/` and sqrt are correctly rounded.  Test code, not product."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests.pointcloud_reference import lut_bytes, scale_bytes

F = np.float32
IDENTITY = np.eye(3, 4, dtype=np.float32)
PLANES = 7


def world_to_camera(c2w) -> np.ndarray:
    """fp64 [3,4]: [R^T | -R^T t]"""
    m = np.asarray(c2w, dtype=np.float64).reshape(3, 4)
    rt = m[:, :3].T
    return np.concatenate([rt, -(rt @ m[:, 3:])], axis=1)


def params(lo, hi, dims, truncation, min_accumulation=0.5, max_temperature=1.0, min_temperature=0.0, to_world=None,
           camera=None) -> dict:
    """the parameter block as fp32 values, each formed in double and rounded once.  camera = (fx, fy, cx, cy, c2w [3,4])"""
    lo64, hi64 = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    dims = tuple(int(v) for v in dims)
    q = dict(lo=lo64.astype(F), step=((hi64 - lo64) / (np.asarray(dims, dtype=np.float64) - 1.0)).astype(F), dims=dims,
             truncation=F(truncation), inv_truncation=F(1.0 / float(truncation)), min_accumulation=F(min_accumulation),
             temperature_span=F(float(max_temperature) - float(min_temperature)), temperature_min=F(min_temperature),
             to_world=IDENTITY.copy() if to_world is None else np.asarray(to_world, dtype=np.float64).reshape(3, 4).astype(F))
    if camera is not None:
        q.update(camera_params(*camera))
    return q


def camera_params(fx, fy, cx, cy, c2w) -> dict:
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), w2c=world_to_camera(c2w).astype(F))


def _affine(m, p):
    """((m0 p0 + m1 p1) + m2 p2) + m3 per row, one rounding per operation; p = three arrays"""
    rows = []
    for r in range(3):
        s = ((m[r, 0] * p[0]).astype(F) + (m[r, 1] * p[1]).astype(F)).astype(F)
        s = (s + (m[r, 2] * p[2]).astype(F)).astype(F)
        rows.append((s + m[r, 3]).astype(F))
    return rows


def grid_points(q):
    """the three coordinate arrays of every grid point, flat, x fastest"""
    nx, ny, nz = q["dims"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return [(q["lo"][c] + (idx.reshape(-1).astype(F) * q["step"][c]).astype(F)).astype(F) for c, idx in enumerate((i, j, k))]


def project(q, p):
    """the fusion kernel's projection of points p (three arrays): (valid, row, col, camera-frame coordinates)"""
    with np.errstate(all="ignore"):
        c = _affine(q["w2c"], p)
        zc = -c[2]
        front = zc > 0
        u = (((q["fx"] * c[0]).astype(F) / zc).astype(F) + q["cx"]).astype(F)
        v = (((q["fy"] * -c[1]).astype(F) / zc).astype(F) + q["cy"]).astype(F)
    return front, u, v, c


def integrate(volume, pose, q) -> dict:
    """Fuse one pose (dict: depth, accumulation, thermal [H*W], rgb [H*W,3], height, width) into ``volume`` [7,Nz,Ny,Nx] IN PLACE.
    Returns the class of every voxel as boolean masks: behind, outside (the image), transparent, beyond (-truncation, NaN and
    +inf depth included), far (fused, clamped band in front: no colour), near (fused with colour)."""
    h, w = int(pose["height"]), int(pose["width"])
    depth, acc, th = (np.asarray(pose[k], dtype=F).reshape(-1) for k in ("depth", "accumulation", "thermal"))
    rgb = np.asarray(pose["rgb"], dtype=F).reshape(-1, 3)
    nx, ny, nz = q["dims"]
    n = nx * ny * nz
    assert volume.dtype == F and volume.flags.c_contiguous
    flat = volume.reshape(PLANES, n)  # a view: updates land in the caller's array
    front, u, v, c = project(q, grid_points(q))
    with np.errstate(all="ignore"):
        in_image = front & (u >= 0) & (u < F(w)) & (v >= 0) & (v < F(h))
        col, row = np.where(in_image, u, 0).astype(np.int64), np.where(in_image, v, 0).astype(np.int64)
        pix = row * w + col
        opaque = in_image & (acc[pix] > q["min_accumulation"])
        dist = np.sqrt((((c[0] * c[0]).astype(F) + (c[1] * c[1]).astype(F)).astype(F) + (c[2] * c[2]).astype(F)).astype(F)).astype(F)
        sdf = (depth[pix] - dist).astype(F)
        fused = opaque & (sdf >= -q["truncation"]) & (sdf < F(np.inf))
        near = fused & (sdf <= q["truncation"])
        value = np.minimum(F(1.0), (sdf * q["inv_truncation"]).astype(F))
    flat[0][fused] = (flat[0][fused] + value[fused]).astype(F)
    flat[1][fused] = (flat[1][fused] + F(1.0)).astype(F)
    flat[2][near] = (flat[2][near] + th[pix[near]]).astype(F)
    for ch in range(3):
        flat[3 + ch][near] = (flat[3 + ch][near] + rgb[pix[near], ch]).astype(F)
    flat[6][near] = (flat[6][near] + F(1.0)).astype(F)
    return dict(behind=~front, outside=front & ~in_image, transparent=in_image & ~opaque, beyond=opaque & ~fused,
                far=fused & ~near, near=near)


def _corner(a, dx, dy, dz):
    """[Nz,Ny,Nx] -> the (dx,dy,dz) corner of every cell, [Nz-1,Ny-1,Nx-1]"""
    nz, ny, nx = a.shape
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def extract(volume, q, table_u8=None) -> dict:
    """positions, colors, temperature, thermal_colors (with a table), triangles and cell_index, in the defined order"""
    nx, ny, nz = q["dims"]
    vol = np.asarray(volume, dtype=F).reshape(PLANES, nz, ny, nx)
    observed = vol[1] > 0
    with np.errstate(all="ignore"):
        f = np.where(observed, (vol[0] / vol[1]).astype(F), F(0.0))
    inside = observed & (f < 0)
    corners = [(e & 1, e >> 1 & 1, e >> 2) for e in range(8)]  # x fastest
    all_obs = np.ones((nz - 1, ny - 1, nx - 1), bool)
    n_in = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for d in corners:
        all_obs &= _corner(observed, *d)
        n_in += _corner(inside, *d)
    active = (all_obs & (n_in > 0) & (n_in < 8)).reshape(-1)
    cells = np.nonzero(active)[0]
    cell_index = np.full(active.shape[0], -1, np.int32)
    cell_index[cells] = np.arange(len(cells), dtype=np.int32)
    ci, cj, ck = cells % (nx - 1), cells // (nx - 1) % (ny - 1), cells // ((nx - 1) * (ny - 1))
    fc = {d: _corner(f, *d).reshape(-1)[cells] for d in corners}
    s = [np.zeros(len(cells), F) for _ in range(3)]
    n = np.zeros(len(cells), F)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, c = [x for x in range(3) if x != a]  # the other two axes, ascending
            for ob, oc in ((0, 0), (1, 0), (0, 1), (1, 1)):
                lo_corner, hi_corner = [0, 0, 0], [0, 0, 0]
                lo_corner[b] = hi_corner[b] = ob
                lo_corner[c] = hi_corner[c] = oc
                hi_corner[a] = 1
                fa, fb = fc[tuple(lo_corner)], fc[tuple(hi_corner)]
                cross = (fa < 0) != (fb < 0)
                t = (fa / (fa - fb).astype(F)).astype(F)
                s[a] = np.where(cross, (s[a] + t).astype(F), s[a])
                s[b] = np.where(cross, (s[b] + F(ob)).astype(F), s[b])
                s[c] = np.where(cross, (s[c] + F(oc)).astype(F), s[c])
                n = np.where(cross, (n + F(1.0)).astype(F), n)
        p = [(q["lo"][a] + ((idx.astype(F) + (s[a] / n).astype(F)).astype(F) * q["step"][a]).astype(F)).astype(F)
             for a, idx in enumerate((ci, cj, ck))]
        world = _affine(q["to_world"], p)
        sums = []
        for plane in range(2, 7):
            acc = np.zeros(len(cells), F)
            for d in corners:
                acc = (acc + _corner(vol[plane], *d).reshape(-1)[cells]).astype(F)
            sums.append(acc)
        mean_thermal = (sums[0] / sums[4]).astype(F)
        mean_rgb = np.stack([(sums[1 + ch] / sums[4]).astype(F) for ch in range(3)], axis=1)
        temperature = ((mean_thermal * q["temperature_span"]).astype(F) + q["temperature_min"]).astype(F)
    out = dict(positions=np.stack(world, axis=1).astype(F) if len(cells) else np.zeros((0, 3), F),
               colors=scale_bytes(mean_rgb) if len(cells) else np.zeros((0, 3), np.uint8), temperature=temperature,
               cell_index=cell_index)
    if table_u8 is not None:
        out["thermal_colors"] = lut_bytes(mean_thermal, table_u8) if len(cells) else np.zeros((0, 3), np.uint8)

    # quads: per grid point, per axis
    grid_cells = cell_index.reshape(nz - 1, ny - 1, nx - 1)
    padded = np.full((nz + 1, ny + 1, nx + 1), -1, np.int32)  # cell (i,j,k) at [k+1, j+1, i+1]; -1 where no cell exists
    padded[1:nz, 1:ny, 1:nx] = grid_cells
    dims = (nx, ny, nz)
    per_axis = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        sl_p = [slice(None)] * 3   # numpy axes are (z, y, x) = (2 - axis)
        sl_n = [slice(None)] * 3
        sl_p[2 - a], sl_n[2 - a] = slice(0, dims[a] - 1), slice(1, dims[a])
        crossing = np.zeros((nz, ny, nx), bool)
        crossing[tuple(sl_p)] = observed[tuple(sl_p)] & observed[tuple(sl_n)] & (inside[tuple(sl_p)] != inside[tuple(sl_n)])
        flip = np.zeros((nz, ny, nx), bool)
        flip[tuple(sl_p)] = inside[tuple(sl_n)]

        def cell_at(db, dc):
            """cell_index of the cell at offsets (db, dc) in (b, c) from every grid point's own cell coordinates"""
            start = [1, 1, 1]  # padded index of the point's own cell, per axis x, y, z
            start[b] += db
            start[c] += dc
            return padded[start[2]:start[2] + nz, start[1]:start[1] + ny, start[0]:start[0] + nx]

        v = [cell_at(-1, -1), cell_at(0, -1), cell_at(0, 0), cell_at(-1, 0)]
        on = crossing & (v[0] >= 0) & (v[1] >= 0) & (v[2] >= 0) & (v[3] >= 0)
        v1 = np.where(flip, v[3], v[1])
        v3 = np.where(flip, v[1], v[3])
        tri = np.stack([v[0], v1, v[2], v[0], v[2], v3], axis=-1).reshape(-1, 6)
        per_axis.append((on.reshape(-1), tri))
    on = np.stack([x[0] for x in per_axis], axis=1).reshape(-1)           # [points * 3], (point, axis) order
    tri = np.stack([x[1] for x in per_axis], axis=1).reshape(-1, 6)
    out["triangles"] = tri[on].reshape(-1, 3).astype(np.int32)
    return out


def mesh_topology(triangles, num_vertices) -> dict:
    """edge-use statistics of an indexed triangle list: bad_edges (undirected edges not shared by exactly two triangles),
    inconsistent (directed edges used twice: two neighbours wound against each other), euler = V - E + T, unused vertices"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = np.sort(directed, axis=1)
    _, counts = np.unique(key, axis=0, return_counts=True)
    _, dcounts = np.unique(directed, axis=0, return_counts=True)
    used = np.zeros(num_vertices, bool)
    used[t.reshape(-1)] = True
    return dict(edges=len(counts), bad_edges=int((counts != 2).sum()), inconsistent=int((dcounts != 1).sum()),
                euler=num_vertices - len(counts) + len(t), unused=int((~used).sum()))


def volume3(inside=((1, 1, 1),), unobserved=()):
    """a 3 x 3 x 3 volume written directly: weight 1 and tsdf +0.5 everywhere but -0.5 at the grid points ``inside`` (i, j, k) and
    weight 0 at ``unobserved``; constant colour planes"""
    vol = np.zeros((PLANES, 3, 3, 3), F)
    vol[0], vol[1], vol[2], vol[6] = 0.5, 1.0, 0.25, 1.0
    vol[3], vol[4], vol[5] = 0.125, 0.5, 0.75
    for i, j, k in inside:
        vol[0, k, j, i] = -0.5
    for i, j, k in unobserved:
        vol[1, k, j, i] = 0.0
    return vol


# ---- the analytic sphere scene of the watertightness tests -------------------------------------------------------------------------
SPHERE = dict(radius=0.3, enclosure=2.0, grid=24, half=0.5, truncation_steps=3.0, cameras=12, image=48, fov_deg=50.0, orbit=0.8)


def look_at(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """fp64 [3,4] camera-to-world of a camera at ``position`` that looks along its -z at ``target``"""
    position = np.asarray(position, dtype=np.float64)
    z = position - np.asarray(target, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z, position], axis=1)


def pinhole_rays(c2w, f, size):
    """origins [3], unit directions [size*size, 3] (fp64) of a size x size pinhole, pixel centres at +0.5, principal point in the
    middle — the convention of Cameras.generate_rays"""
    px = np.arange(size, dtype=np.float64) + 0.5
    v, u = np.meshgrid(px, px, indexing="ij")
    d = np.stack([(u - size / 2) / f, -(v - size / 2) / f, -np.ones_like(u)], axis=-1).reshape(-1, 3) @ c2w[:, :3].T
    return c2w[:, 3], d / np.linalg.norm(d, axis=1, keepdims=True)


def _sphere_hit(o, d, radius):
    """distance along unit d from o to the NEAREST intersection with the origin-centred sphere (inf on a miss); from inside: the exit"""
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    root = np.sqrt(np.where(disc >= 0, disc, np.nan))
    near = -b - root
    return np.where(disc >= 0, np.where(near > 0, near, -b + root), np.inf)


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """(params without a camera, list of (camera tuple, pose outputs)) of the sphere scene: a 24^3 grid over [-0.5, 0.5]^3,
    truncation 3 steps, 12 cameras of 48 x 48 with a 50 degree field of view on a Fibonacci sphere of radius 0.8 that look at the
    origin; depth = the ray's hit on a sphere of radius 0.3 or, when it misses, on an enclosing sphere of radius 2; accumulation 1;
    thermal (z / 0.3 + 1) / 2 on the sphere and 0 on the enclosure; rgb = the hit point's normal mapped into [0, 1] (0 outside)."""
    s = SPHERE
    step = 2 * s["half"] / (s["grid"] - 1)
    q = params((-s["half"],) * 3, (s["half"],) * 3, (s["grid"],) * 3, s["truncation_steps"] * step)
    f = (s["image"] / 2) / math.tan(math.radians(s["fov_deg"]) / 2)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    poses = []
    for k in range(s["cameras"]):
        z = 1.0 - (2 * k + 1) / s["cameras"]
        r = math.sqrt(1.0 - z * z)
        c2w = look_at(s["orbit"] * np.array([r * math.cos(golden * k), r * math.sin(golden * k), z]))
        o, d = pinhole_rays(c2w, f, s["image"])
        t = _sphere_hit(o, d, s["radius"])
        hit = np.isfinite(t)
        depth = np.where(hit, t, _sphere_hit(o, d, s["enclosure"]))
        p = o[None, :] + d * depth[:, None]
        thermal = np.where(hit, (p[:, 2] / s["radius"] + 1) / 2, 0.0)
        rgb = np.where(hit[:, None], (p / s["radius"] + 1) / 2, 0.0)
        pose = dict(depth=depth.astype(F), accumulation=np.ones(len(depth), F), thermal=thermal.astype(F), rgb=rgb.astype(F),
                    height=s["image"], width=s["image"])
        poses.append(((f, f, s["image"] / 2, s["image"] / 2, c2w), pose))
    return q, poses


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """(the fused volume, the extracted mesh) of ``sphere_scene`` through this reference; computed once, left unchanged"""
    from thermo_nerf_amd import colormaps

    q, poses = sphere_scene()
    nx, ny, nz = q["dims"]
    volume = np.zeros((PLANES, nz, ny, nx), F)
    for camera, pose in poses:
        integrate(volume, pose, dict(q, **camera_params(*camera)))
    mesh = extract(volume, q, colormaps.table_u8("magma"))
    volume.setflags(write=False)
    return volume, mesh
