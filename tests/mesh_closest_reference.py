"""The yardstick of the closest-point query: include/thermonerf_hip.h's definition of ``tn_mesh_closest`` as brute force in fp64, every
point against every face, with no tree.

``closest`` is written once over an array namespace, like ``mesh_raycast_reference.raycast``: numpy on the host, or torch with fp64
tensors where the caller has a device.  Every step is one add, sub, mul, div or sqrt of fp64 arrays, which both round correctly and
neither contracts; the device tests compare the two on a small scene first.  ``box_bound`` is b of a box, ``bound_slack`` the
smallest d2 - b over all (point, usable face) pairs: what the proof in the header says is never negative."""
from __future__ import annotations

import math

import numpy as np

from tests.mesh_raycast_reference import NAN_BITS, bits, face_boxes, ord32, sum2, usable_faces  # noqa: F401

F, D = np.float32, np.float64
OUTPUTS = ("closest_face", "closest_distance", "closest_point", "closest_uv", "closest_temperature", "closest_colors", "difference")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def box_bound(q, lo, hi):
    """b of the boxes lo .. hi (fp32 [..., 3]) against the points q (fp32 or fp64 [..., 3]), broadcasting: fp64 [...]"""
    q, lo, hi = np.asarray(q, D), np.asarray(lo, F).astype(D), np.asarray(hi, F).astype(D)
    g = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


class _Best:
    def __init__(self):
        self.some = self.d2 = self.u = self.v = self.c = None

    def consider(self, xp, q, lo, hi, c, u, v, valid):
        """a candidate per (point, face): clamped into the face's box, kept where it is valid and strictly nearer"""
        x = [xp.where(c[k] < lo[k], lo[k], xp.where(c[k] > hi[k], hi[k], c[k])) for k in range(3)]
        r = [q[k] - x[k] for k in range(3)]
        d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        if self.some is None:
            self.some, self.d2, self.u, self.v, self.c = valid, d2, u, v, x
            return
        take = valid & (~self.some | (d2 < self.d2))
        self.d2, self.u, self.v = xp.where(take, d2, self.d2), xp.where(take, u, self.u), xp.where(take, v, self.v)
        self.c = [xp.where(take, x[k], self.c[k]) for k in range(3)]
        self.some = self.some | valid


def _edge(xp, qa, ab):
    den = _dot(ab, ab)
    s = _dot(qa, ab) / den
    s = xp.where(den == 0.0, xp.zeros_like(s), s)  # (0 / 0 of a segment without length is replaced before it is looked at)
    return xp.where(s > 0.0, xp.where(s > 1.0, xp.ones_like(s), s), xp.zeros_like(s))


def _pairs(xp, q, p0, p1, p2, lo, hi):
    """every point (lists of three [R, 1] arrays) against every face ([1, F] arrays): a ``_Best`` of [R, F] arrays"""
    e1, e2, e3 = [p1[k] - p0[k] for k in range(3)], [p2[k] - p0[k] for k in range(3)], [p2[k] - p1[k] for k in range(3)]
    w, w1 = [q[k] - p0[k] for k in range(3)], [q[k] - p1[k] for k in range(3)]
    best = _Best()
    n = _cross(e1, e2)
    nn = _dot(n, n)
    u = _dot(_cross(w, e2), n) / nn
    v = _dot(_cross(e1, w), n) / nn
    inside = (nn != 0.0) & (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0)
    best.consider(xp, q, lo, hi, [(p0[k] + u * e1[k]) + v * e2[k] for k in range(3)], u, v, inside)
    always = xp.ones_like(u) > 0.0
    s = _edge(xp, w, e1)
    best.consider(xp, q, lo, hi, [p0[k] + s * e1[k] for k in range(3)], s, xp.zeros_like(s), always)
    s = _edge(xp, w, e2)
    best.consider(xp, q, lo, hi, [p0[k] + s * e2[k] for k in range(3)], xp.zeros_like(s), s, always)
    s = _edge(xp, w1, e3)
    best.consider(xp, q, lo, hi, [p1[k] + s * e3[k] for k in range(3)], 1.0 - s, s, always)
    return best


def _scene(positions, temperature, triangles, torch_device):
    positions, temperature = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    usable = usable_faces(positions, temperature, tri)
    lo32, hi32 = face_boxes(positions, tri, usable)
    safe = np.where(usable[:, None], tri.astype(np.int64), 0)
    corner = positions[safe].astype(D) if len(positions) else np.zeros((len(tri), 3, 3), D)
    if torch_device is not None:
        import torch

        xp = torch

        def arr(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(torch_device)
    else:
        xp, arr = np, (lambda x: x)
    p = [[arr(corner[None, :, c, k]) for k in range(3)] for c in range(3)]
    lo, hi = [arr(lo32[None, :, k].astype(D)) for k in range(3)], [arr(hi32[None, :, k].astype(D)) for k in range(3)]
    return positions, temperature, tri, usable, (lo32, hi32), xp, arr, p, lo, hi


def closest(positions, temperature, colors, triangles, points, point_temperature=None, max_distance=math.inf, chunk=256,
            torch_device=None):
    """The definition.  A dict of ``closest_face`` int32 [N], ``closest_distance``, ``closest_temperature`` float32 [N],
    ``closest_point`` float32 [N, 3], ``closest_uv`` float32 [N, 2], ``closest_colors`` uint8 [N, 3] (None without colors),
    ``difference`` float32 [N] (None without point_temperature), ``counts`` int64 [4], ``stats`` float64 [8], and ``d2`` float64 [N]
    (the winner's, +inf without one)."""
    positions, temperature, tri, usable, _, xp, arr, p, lo, hi = _scene(positions, temperature, triangles, torch_device)
    points = np.asarray(points, F).reshape(-1, 3)
    n, faces = len(points), len(tri)
    good = np.isfinite(points).all(axis=1)
    r2 = float(D(max_distance) * D(max_distance))
    use = arr(usable[None, :])
    face = np.full(n, -1, np.int32)
    best = np.zeros((n, 6), D)  # d2, u, v, C
    with np.errstate(all="ignore"):
        for first in range(0, n if faces else 0, chunk):
            rows = slice(first, min(first + chunk, n))
            safe_q = np.where(good[rows, None], points[rows], 0).astype(D)
            q = [arr(safe_q[:, k:k + 1]) for k in range(3)]
            found = _pairs(xp, q, p[0], p[1], p[2], lo, hi)
            ok = use & arr(good[rows, None]) & (found.d2 <= r2)
            if xp is np:
                masked = np.where(ok, found.d2, np.inf)
                nearest = masked.min(axis=1, keepdims=True)
                first_of = np.argmax(ok & (masked == nearest), axis=1)
                some = ok.any(axis=1)
                pick = (np.arange(len(first_of)), first_of)
                values = np.stack([x[pick] for x in (found.d2, found.u, found.v, *found.c)], axis=1)
            else:
                import torch

                masked = torch.where(ok, found.d2, torch.full_like(found.d2, math.inf))
                nearest = masked.amin(dim=1, keepdim=True)
                first_of = torch.argmax((ok & (masked == nearest)).to(torch.int8), dim=1)
                some = ok.any(dim=1).cpu().numpy()
                at = first_of[:, None]
                values = torch.cat([x.expand_as(found.d2).gather(1, at) for x in (found.d2, found.u, found.v, *found.c)], dim=1).cpu().numpy()
                first_of = first_of.cpu().numpy()
            face[rows] = np.where(some, first_of, -1)
            best[rows] = np.where(some[:, None], values, 0.0)
    return finish(positions, temperature, colors, tri, usable, good, face, best, point_temperature)


def stats_of(values):
    """SUM2 of the values and of their squares over ALL entries (a NaN counts +0.0), the minimum and the maximum over the others in
    the numbers' order with -0.0 below +0.0 (+inf and -inf without one): four float64"""
    values = np.asarray(values, F)
    has = ~np.isnan(values)
    x = np.where(has, values.astype(D), 0.0)
    shown = values[has]
    low = D(shown[np.argmin(ord32(shown))]) if has.any() else math.inf
    high = D(shown[np.argmax(ord32(shown))]) if has.any() else -math.inf
    return [sum2(x), sum2(x * x), low, high]


def finish(positions, temperature, colors, tri, usable, good, face, best, point_temperature):
    n = len(face)
    found = face >= 0
    d2, u, v, c = best[:, 0], best[:, 1], best[:, 2], best[:, 3:6]
    nan = np.uint32(NAN_BITS).view(F)
    corner = np.where(found[:, None], tri[np.where(found, face, 0)] if len(tri) else np.zeros((n, 3), np.int32), 0).astype(np.int64)
    out = {"closest_face": face.astype(np.int32), "d2": np.where(found, d2, math.inf)}
    out["closest_distance"] = np.where(found, np.sqrt(d2).astype(F), nan).astype(F)
    out["closest_point"] = np.where(found[:, None], c.astype(F), nan).astype(F)
    out["closest_uv"] = np.where(found[:, None], np.stack([u, v], axis=1).astype(F), nan).astype(F)
    w = (1.0 - u) - v
    if len(positions):
        temp = temperature.astype(D)[corner]
        blend = (w * temp[:, 0] + u * temp[:, 1]) + v * temp[:, 2]
    else:
        blend = np.zeros(n, D)
    with np.errstate(all="ignore"):
        out["closest_temperature"] = np.where(found, blend.astype(F), nan).astype(F)
    out["closest_colors"] = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).reshape(-1, 3).astype(D)[corner] if len(positions) else np.zeros((n, 3, 3), D)
        mixed = (w[:, None] * col[:, 0] + u[:, None] * col[:, 1]) + v[:, None] * col[:, 2]
        out["closest_colors"] = np.where(found[:, None], np.clip(np.floor(mixed + 0.5), 0.0, 255.0), 0.0).astype(np.uint8)
    out["difference"] = None
    if point_temperature is not None:
        with np.errstate(all="ignore"):
            delta = (np.asarray(point_temperature, F).reshape(-1).astype(D) - out["closest_temperature"].astype(D)).astype(F)
        out["difference"] = np.where(np.isnan(delta), nan, delta).astype(F)
    out["counts"] = np.array([int(found.sum()), int(good.sum()), int(usable.sum()), 0], np.int64)
    out["stats"] = np.array(stats_of(out["closest_distance"]) + (stats_of(out["difference"]) if out["difference"] is not None
                                                                   else [0.0, 0.0, math.inf, -math.inf]), D)
    return out


def bound_slack(positions, temperature, triangles, points, chunk=256):
    """(the smallest d2 - b over every usable point against every usable face, b of the face's own box; the number of pairs): the
    header's proof says the first is never negative"""
    positions, temperature, tri, usable, (lo32, hi32), xp, arr, p, lo, hi = _scene(positions, temperature, triangles, None)
    points = np.asarray(points, F).reshape(-1, 3)
    points = points[np.isfinite(points).all(axis=1)]
    worst, pairs = math.inf, 0
    if not usable.any():
        return worst, pairs
    with np.errstate(all="ignore"):
        for first in range(0, len(points), chunk):
            rows = points[first:first + chunk].astype(D)
            found = _pairs(np, [rows[:, k:k + 1] for k in range(3)], p[0], p[1], p[2], lo, hi)
            b = box_bound(rows[:, None, :], lo32[None], hi32[None])
            gap = (found.d2 - b)[:, usable]
            assert not np.isnan(found.d2[:, usable]).any() and not np.isnan(found.u[:, usable]).any() and not np.isnan(found.v[:, usable]).any()
            worst, pairs = min(worst, float(gap.min())), pairs + gap.size
    return worst, pairs


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------

def face_normals(positions, triangles):
    """unit normals float64 [T, 3] (zeros for a face without area)"""
    p = np.asarray(positions, D)[np.asarray(triangles, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)


def query_points(positions, triangles, count, seed):
    """a third each: the mesh's own vertices (cycled) pushed along +- a normal of a face they belong to, uniform points in twice the
    extent, and points exactly on faces (a corner, an edge midpoint or a random interior point, rounded to fp32)"""
    positions, tri = np.asarray(positions, F), np.asarray(triangles, np.int64)
    rng = np.random.default_rng(seed)
    lo, hi = positions.min(axis=0).astype(D), positions.max(axis=0).astype(D)
    span = np.maximum(hi - lo, 1e-3)
    k = count // 3
    normal_of = np.zeros((len(positions), 3), D)
    normal_of[tri.reshape(-1)] = np.repeat(face_normals(positions, tri), 3, axis=0)
    vertex = np.arange(k) % len(positions)
    pushed = positions[vertex].astype(D) + normal_of[vertex] * (rng.choice([-1.0, 1.0], (k, 1)) * rng.uniform(0.0, 0.05, (k, 1)) * span.max())
    uniform = rng.uniform(lo - span / 2, hi + span / 2, (k, 3))
    f = rng.integers(0, len(tri), count - 2 * k)
    weights = rng.dirichlet((1.0, 1.0, 1.0), count - 2 * k)
    kind = rng.integers(0, 3, count - 2 * k)
    weights[kind == 0] = (1.0, 0.0, 0.0)
    weights[kind == 1] = (0.5, 0.5, 0.0)
    on = (positions[tri[f]].astype(D) * weights[:, :, None]).sum(axis=1)
    return np.concatenate([pushed, uniform, on]).astype(F)


def plane_grid(cells, z, offset, size=4.0):
    """a ``cells`` x ``cells`` grid of two-triangle quads over [0, size]^2 at height z with T = offset + 4 x: (positions,
    temperature, triangles); cells a power of two keeps every number exact"""
    g = np.linspace(0.0, size, cells + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    positions = np.stack([x, y, np.full_like(x, z)], axis=-1).reshape(-1, 3).astype(F)
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    v00 = i * (cells + 1) + j
    v10, v01, v11 = v00 + cells + 1, v00 + 1, v00 + cells + 2
    tri = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], -2).reshape(-1, 3).astype(np.int32)
    return positions, (offset + 4.0 * positions[:, 0].astype(D)).astype(F), tri


TRIANGLE = (np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0)], F), np.array([10, 20, 30], F), np.array([(0, 0, 0), (200, 100, 0), (0, 100, 255)], np.uint8),
            np.array([(0, 1, 2)], np.int32))
# inside on the plane, above, below; beyond each corner; beyond each edge; on a corner, on an edge, on the hypotenuse
TRIANGLE_POINTS = np.array([(1, 1, 0), (1, 1, 2), (1, 2, -3), (-1, -1, 0), (5, -1, 0), (-1, 5, 1), (2, -2, 0), (-2, 2, 0), (3, 3, 0),
                            (0, 0, 0), (2, 0, 0), (2, 2, 0)], F)


def degenerate_mesh():
    """faces without area under distinct indices: collinear corners (the third between the other two), a needle with two equal
    positions, three equal positions — each far from the others"""
    positions = np.array([(0, 0, 0), (2, 0, 0), (1, 0, 0), (10, 0, 0), (10, 0, 0), (10, 4, 0), (20, 1, 1), (20, 1, 1), (20, 1, 1)], F)
    return positions, np.array([10, 20, 30, 40, 50, 60, 70, 80, 90], F), None, np.arange(9, dtype=np.int32).reshape(-1, 3)


DEGENERATE_POINTS = np.array([(1, 1, 0), (-1, 0, 0), (3, 0, 2), (0.5, 0, 0), (10, 2, 3), (10, -1, 0), (11, 5, 0), (20, 1, 1), (20, 4, 5),
                              (15, 0, 0)], F)


# an upper sheet at z = 6; the lower sheet's second half; its first half twice; two unusable faces
SHEETS = (np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 0), (0, 0, 6), (4, 0, 6), (0, 4, 6)], F), np.array([10, 20, 30, 40, 50, 60, 70], F), None,
          np.array([(4, 5, 6), (1, 3, 2), (0, 1, 2), (0, 1, 2), (0, 0, 1), (0, 1, 9)], np.int32))
# 3 from both sheets; 2 from the copies; 1 above the edge two faces share; inside a face; 1 above a vertex three faces share; 2 below the top
SHEET_POINTS = np.array([(1, 1, 3), (1, 1, 2), (2, 2, 1), (3, 3, 0), (4, 0, 1), (1, 1, 4)], F)


def unusable_mix():
    """a soup of 40 faces of which one is usable: the others repeat an index, leave [0, V), or carry a NaN / inf coordinate or a NaN
    temperature (the ray cast's test mesh)"""
    from tests.mesh_raycast_reference import attributes, soup

    pos, tri = soup(40, 4)
    temp, col = attributes(len(pos), 2)
    tri, pos, temp = tri.copy(), pos.copy(), temp.copy()
    tri[:, 1] = tri[:, 0]
    tri[3] = (9, 10, 11)
    tri[5] = (0, 1, len(pos))
    tri[6] = (-1, 1, 2)
    tri[7], tri[8], tri[9] = (21, 22, 23), (24, 25, 26), (27, 28, 29)
    pos[22, 1] = np.inf
    temp[25] = np.nan
    pos[28, 0] = np.nan
    return pos, temp, col, tri


def scene(name):
    """(positions, temperature, colors, triangles, points) of a named scene of the device test"""
    from tests import mesh_raycast_reference as R

    if name == "triangle":
        return (*TRIANGLE, TRIANGLE_POINTS)
    if name == "degenerate":
        return (*degenerate_mesh(), DEGENERATE_POINTS)
    if name.startswith("soup-"):  # sizes around the tile
        faces = int(name[5:])
        pos, tri = R.soup(faces, 10 + faces)
        temp, col = R.attributes(len(pos), 1)
        return pos, temp, col, tri, np.random.default_rng(faces).uniform(-0.5, 1.5, (129, 3)).astype(F)
    if name == "unusable":
        pos, temp, col, tri = unusable_mix()
        return pos, temp, col, tri, np.random.default_rng(3).uniform(-0.5, 1.5, (200, 3)).astype(F)
    if name == "flat":  # every box of the tree has no thickness along z
        pos, tri = R.soup(90, 8)
        pos = pos.copy()
        pos[:, 2] = 0.625
        temp, col = R.attributes(len(pos), 3)
        points = np.random.default_rng(5).uniform(-0.5, 1.5, (300, 3)).astype(F)
        points[:120, 2] = 0.625
        return pos, temp, col, tri, points
    if name == "chain":
        from tests.test_gpu_mesh_raycast import deep_chain

        pos, tri = deep_chain()
        temp, col = R.attributes(len(pos), 4)
        rng = np.random.default_rng(6)
        near = pos[rng.integers(0, len(pos), 150)].astype(D) + rng.normal(0.0, 2.0 ** -12, (150, 3))
        return pos, temp, col, tri, np.concatenate([near, rng.uniform(-0.25, 1.25, (150, 3))]).astype(F)
    if name == "far":  # a small mesh seen from 10^6 units away: b and d2 agree to the last bits
        pos, tri = R.soup(200, 31, size=0.05)
        temp, col = R.attributes(len(pos), 5)
        rng = np.random.default_rng(7)
        direction = rng.normal(0.0, 1.0, (400, 3))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        points = 0.5 + direction * 1e6
        points[:60] = 0.5 + np.eye(3)[rng.integers(0, 3, 60)] * rng.choice([-1e6, 1e6], (60, 1))  # along the axes
        return pos, temp, col, tri, points.astype(F)
    if name == "room":
        pos, tri = R.room(cells=12, boxes=2, box_cells=4, seed=5)
        temp, col = R.attributes(len(pos), 8)
        return pos, temp, col, tri, query_points(pos, tri, 2400, 11)
    if name == "soup":
        pos, tri = R.soup(2400, 21, size=0.04)
        temp, col = R.attributes(len(pos), 9)
        return pos, temp, col, tri, query_points(pos, tri, 2400, 12)
    raise KeyError(name)


SIZES = (0, 1, 2, 3, 255, 256, 257)
SCENES = ("triangle", "degenerate", "unusable", "flat", "chain", "far", "room", "soup") + tuple(f"soup-{t}" for t in SIZES)
