"""The yardstick of tn_mesh_scalar_smooth / tn_mesh_scalar_gradient: the definitions of include/thermonerf_hip.h restated in numpy
float64 and plain Python, operation by operation in the stated order.  Every numpy operation used on floats is one correctly rounded
IEEE operation per element (add, subtract, multiply, divide, sqrt, the float32 conversion).  The per-vertex loops run as ROUNDS —
round k handles the k-th corner of every list that has one — which is the same sequence of operations per vertex.  The lists are
``tests.mesh_smooth_reference.incidence``'s; a foreign index is clipped and checked as the header says.  Test code, not product."""
from __future__ import annotations

import numpy as np

from tests.mesh_components_reference import valid_mask
from tests.mesh_smooth_reference import incidence  # noqa: F401  (the lists every function below takes as ``index``)

F, D = np.float32, np.float64
BLOCK = 256
NAN32_BITS, NAN64_BITS = 0x7fc00000, 0x7ff8000000000000
NAN32 = np.array([NAN32_BITS], np.uint32).view(F)[0]
NAN64 = np.array([NAN64_BITS], np.uint64).view(D)[0]


def bits(a) -> np.ndarray:
    """the bit patterns of a float32 or float64 array"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rounds(index: dict, num_corners: int):
    """yields (vertices, their k-th corners) for k = 0, 1, ...: every list clipped to [0, 3T] and walked in its own order, a corner
    outside [0, 3T) left out"""
    if index["corners"] is None or num_corners == 0:
        return
    offsets, corners = np.asarray(index["offsets"], np.int64), np.asarray(index["corners"], np.int64)
    begin, end = np.maximum(offsets[:-1], 0), np.minimum(offsets[1:], num_corners)
    length = np.maximum(end - begin, 0)
    for k in range(int(length.max()) if len(length) else 0):
        vs = np.flatnonzero(length > k)
        cs = corners[begin[vs] + k]
        ok = (cs >= 0) & (cs < num_corners)
        yield vs[ok], cs[ok]


# ---- the scalar passes --------------------------------------------------------------------------------------------------------------------

def smooth_pass(src, triangles, index: dict, k, fill: bool) -> np.ndarray:
    """one Jacobi pass with factor k: a new float32 array"""
    src = np.asarray(src, F).reshape(-1)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    v = len(src)
    valid = valid_mask(tri, v)
    s, n = np.zeros(v, D), np.zeros(v, np.int64)
    for vs, cs in rounds(index, 3 * len(tri)):
        t, j = cs // 3, cs % 3
        ok = valid[t]
        vs, t, j = vs[ok], t[ok], j[ok]
        for partner in (src[tri[t, (j + 1) % 3]], src[tri[t, (j + 2) % 3]]):  # q, then r
            has = np.isfinite(partner)
            s[vs[has]] = s[vs[has]] + partner[has].astype(D)
            n[vs[has]] += 1
    out = src.copy()  # the same bits where nothing below applies
    some, own = n > 0, np.isfinite(src)
    with np.errstate(all="ignore"):
        m = s / np.where(some, n, 1).astype(D)
        p = src.astype(D)
        moved = (p + D(F(k)) * (m - p)).astype(F)
        filled = m.astype(F)
    out[some & own] = moved[some & own]
    if fill:
        out[some & ~own] = filled[some & ~own]
    return out


def smooth(values, triangles, index: dict, iterations: int, lambda_, mu, fill: bool = False) -> np.ndarray:
    """tn_mesh_scalar_smooth: per iteration a pass with ``lambda_`` and, unless ``mu`` is zero, a pass with ``mu``"""
    x = np.asarray(values, F).reshape(-1).copy()
    for _ in range(int(iterations)):
        x = smooth_pass(x, triangles, index, lambda_, fill)
        if F(mu) != 0:
            x = smooth_pass(x, triangles, index, mu, fill)
    return x


# ---- the gradient -------------------------------------------------------------------------------------------------------------------------

def cross(a, b):
    """per row (sub(mul(ay, bz), mul(az, by)), sub(mul(az, bx), mul(ax, bz)), sub(mul(ax, by), mul(ay, bx)))"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def length(x):
    """per row sqrt(add(add(mul(xx, xx), mul(xy, xy)), mul(xz, xz)))"""
    return np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])


def face_gradients(positions, values, triangles) -> dict:
    """usable bool [T]; g float64 [T, 3], the NaN row of every face that is not usable; w float64 [T] = sqrt(n2) and steep float64 [T]
    = |g|, +0.0 of every face that is not usable; e1, e2, n float64 [T, 3] of the usable faces (zero rows elsewhere)"""
    pos, val = np.asarray(positions, F).reshape(-1, 3), np.asarray(values, F).reshape(-1)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    v, t = len(pos), len(tri)
    usable = np.zeros(t, bool)
    g, w, steep = np.full((t, 3), NAN64, D), np.zeros(t, D), np.zeros(t, D)
    e1, e2, n = np.zeros((t, 3), D), np.zeros((t, 3), D), np.zeros((t, 3), D)
    if v and t:
        valid = valid_mask(tri, v)
        distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
        safe = np.where(valid[:, None], tri, 0)
        rows = np.flatnonzero(valid & distinct & np.isfinite(pos[safe]).all(axis=(1, 2)) & np.isfinite(val[safe]).all(axis=1))
        i = tri[rows]
        p0, p1, p2 = (pos[i[:, k]].astype(D) for k in range(3))
        u0, u1, u2 = (val[i[:, k]].astype(D) for k in range(3))
        with np.errstate(all="ignore"):
            f1, f2 = p1 - p0, p2 - p0
            c = cross(f1, f2)
            n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
            keep = (n2 > 0.0) & (n2 < np.inf)
            rows, f1, f2, c, n2 = rows[keep], f1[keep], f2[keep], c[keep], n2[keep]
            a, b = (u1 - u0)[keep], (u2 - u0)[keep]
            big_a, big_b = cross(f2, c), cross(c, f1)
            grad = (a[:, None] * big_a + b[:, None] * big_b) / n2[:, None]
            usable[rows] = True
            g[rows], w[rows], steep[rows] = grad, np.sqrt(n2), length(grad)
            e1[rows], e2[rows], n[rows] = f1, f2, c
    return dict(usable=usable, g=g, w=w, steep=steep, e1=e1, e2=e2, n=n)


def sum2(values) -> float:
    """blocks of 256 from the start of the list, each from +0.0 in list order; then the block sums from +0.0 in block order.  (The
    last block is padded with +0.0, which changes no sum of numbers >= +0.0 and no bit of any sum that started from +0.0.)"""
    x = np.asarray(values, D).reshape(-1)
    blocks = -(-len(x) // BLOCK)
    padded = np.zeros(blocks * BLOCK, D)
    padded[:len(x)] = x
    padded = padded.reshape(blocks, BLOCK)
    partial = np.zeros(blocks, D)
    for k in range(BLOCK):
        partial = partial + padded[:, k]
    total = D(0.0)
    for s in partial:
        total = total + s
    return float(total)


def gradient(positions, values, triangles, index: dict) -> dict:
    """tn_mesh_scalar_gradient: face_gradient float64 [T, 3], vertex_gradient float32 [V, 3], vertex_magnitude float32 [V], totals
    float64 [4], and ``faces`` = what ``face_gradients`` gave"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    v, t = len(pos), len(tri)
    faces = face_gradients(pos, values, tri)
    big_s, big_w, some = np.zeros((v, 3), D), np.zeros(v, D), np.zeros(v, bool)
    with np.errstate(all="ignore"):
        for vs, cs in rounds(index, 3 * t):
            f = cs // 3
            ok = faces["usable"][f]
            vs, f = vs[ok], f[ok]
            big_s[vs] = big_s[vs] + faces["w"][f][:, None] * faces["g"][f]
            big_w[vs] = big_w[vs] + faces["w"][f]
            some[vs] = True
        big_g = big_s / np.where(some, big_w, 1.0)[:, None]
        vertex_gradient = np.where(some[:, None], big_g.astype(F), NAN32).astype(F)
        vertex_magnitude = np.where(some, length(big_g).astype(F), NAN32).astype(F)
        totals = np.array([float(faces["usable"].sum()), sum2(faces["w"]), sum2(faces["w"] * faces["steep"]),
                           float(faces["steep"].max()) if t else 0.0], D)
    return dict(face_gradient=faces["g"], vertex_gradient=vertex_gradient, vertex_magnitude=vertex_magnitude, totals=totals, faces=faces)


# ---- shapes the tests share ---------------------------------------------------------------------------------------------------------------

RIGHT_TRIANGLE = (np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F), np.array([(0, 1, 2)], np.int32))


def lattice(nx: int, ny: int):
    """(positions float32 [nx ny, 3], triangles int32 [2 (nx - 1)(ny - 1), 3]): the integer points (x, y, 0), vertex y nx + x, every
    unit cell cut along the diagonal from (x, y) to (x + 1, y + 1), wound towards +z: every face has n = (0, 0, 1)"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny))
    pos = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(nx * ny)], axis=1).astype(F)
    a = (y[:-1, :-1] * nx + x[:-1, :-1]).reshape(-1)
    tri = np.concatenate([np.stack([a, a + 1, a + nx + 1], axis=1), np.stack([a, a + nx + 1, a + nx], axis=1)], axis=1).reshape(-1, 3)
    return pos, tri.astype(np.int32)


def hole(nx: int, ny: int, x0: int, y0: int, side: int) -> np.ndarray:
    """bool [nx ny]: the vertices of the lattice inside the side x side block at (x0, y0)"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny))
    return ((x >= x0) & (x < x0 + side) & (y >= y0) & (y < y0 + side)).reshape(-1)


def random_values(seed: int, n: int) -> np.ndarray:
    """float32 [n]: degrees around 20"""
    return np.random.default_rng(seed).uniform(14.0, 33.0, int(n)).astype(F)
