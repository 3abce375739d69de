"""The yardstick of tn_mesh_half_edges and tn_mesh_isolines: the definitions of include/thermonerf_hip.h restated in numpy float64 and
plain Python — a dictionary of edge classes, a plain walk along the successors — and the meshes of the tests.  It knows nothing of
sorts, scans or pointer jumping.  Every numpy operation used on floats is one correctly rounded IEEE operation per element (add,
subtract, multiply, divide, sqrt, the float32 conversion), which is what the header asks of the kernels; the per-face counting and
the crossing points are vectorised over the faces and the segments, the curves are walked one segment at a time."""
from __future__ import annotations

import numpy as np

F, D = np.float32, np.float64
CURVE_DTYPE = np.dtype([("length", "<f8"), ("level", "<i4"), ("first_point", "<i4"), ("points", "<i4"), ("closed", "<i4"),
                        ("mean_temperature", "<f4"), ("min_temperature", "<f4"), ("max_temperature", "<f4"), ("first_face", "<i4")])
NAN = np.array([0x7fc00000], np.uint32).view(F)[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def order_keys(x):
    """the numbers' order with -0.0 below +0.0, as unsigned keys"""
    b = bits(np.asarray(x, F)).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xffffffff, b | 0x80000000)


def structural_faces(triangles, num_vertices):
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    inside = ((tri >= 0) & (tri < num_vertices)).all(axis=1)
    return inside & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])


# ---- half-edges -------------------------------------------------------------------------------------------------------------------------

def half_edges(triangles, num_vertices):
    """{"twin": int32 [3T], "counts": int64 [4]}"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = structural_faces(tri, num_vertices)
    classes = {}
    for f in np.flatnonzero(ok).tolist():
        a, b, c = tri[f].tolist()
        for j, (u, v) in enumerate(((a, b), (b, c), (c, a))):
            classes.setdefault((u, v) if u < v else (v, u), []).append((3 * f + j, u < v))
    twin = np.full(3 * len(tri), -1, np.int32)
    counts = np.zeros(4, np.int64)
    counts[0] = len(classes)
    for members in classes.values():
        if len(members) == 1:
            counts[1] += 1
        elif len(members) >= 3:
            counts[2] += 1
        elif members[0][1] == members[1][1]:
            counts[3] += 1
        else:
            twin[members[0][0]], twin[members[1][0]] = members[1][0], members[0][0]
    return {"twin": twin, "counts": counts}


# ---- isolines ---------------------------------------------------------------------------------------------------------------------------

def vertex_scalar(positions, scalar=None, normal=None):
    if scalar is not None:
        return np.asarray(scalar, F).astype(D)
    p = np.asarray(positions, F).astype(D).reshape(-1, 3)
    n = np.asarray(normal, D)
    return (n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]


def _crossing(s, p, t, a, b, level):
    """the crossing points of the edges between vertices a and b at `level` (arrays over the segments): xyz float32 [n, 3], float32 [n]"""
    a_high = s[a] >= level
    lo, hi = np.where(a_high, b, a), np.where(a_high, a, b)
    w = (level - s[lo]) / (s[hi] - s[lo])
    xyz = (p[lo] + w[:, None] * (p[hi] - p[lo])).astype(F)
    return xyz, (t[lo] + w * (t[hi] - t[lo])).astype(F)


def isolines(positions, temperature, triangles, twin, levels, scalar=None, normal=None):
    """tn_mesh_isolines with room for everything: counts int64 [5], curves CURVE_DTYPE [Q], positions float32 [P, 3], temperature
    float32 [P], arc float64 [P], face int32 [P]"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    temp = np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    twin = np.asarray(twin, np.int64).reshape(-1)
    levels = np.asarray(levels, D).reshape(-1)
    v, t = len(pos), len(tri)
    empty = {"counts": np.zeros(5, np.int64), "curves": np.zeros(0, CURVE_DTYPE), "positions": np.zeros((0, 3), F),
             "temperature": np.zeros(0, F), "arc": np.zeros(0, D), "face": np.zeros(0, np.int32)}
    if v == 0 or t == 0:
        return empty
    with np.errstate(all="ignore"):
        s = vertex_scalar(pos, scalar, normal)
        p, c = pos.astype(D), temp.astype(D)
        usable = structural_faces(tri, v)
        safe = np.where(usable[:, None], tri, 0)
        usable &= np.isfinite(pos[safe]).all(axis=(1, 2)) & np.isfinite(temp[safe]).all(axis=1) & np.isfinite(s[safe]).all(axis=1)
        safe = np.where(usable[:, None], tri, 0)
        first = np.searchsorted(levels, s[safe].min(axis=1), side="right")   # #{L <= m}
        last = np.searchsorted(levels, s[safe].max(axis=1), side="right")    # #{L <= M}
        first, last = np.where(usable, first, 0), np.where(usable, last, 0)
        number = last - first
        base = np.cumsum(number) - number
        total = int(number.sum())
        counts = np.array([total, 0, 0, 0, int(usable.sum())], np.int64)
        if total == 0:
            return dict(empty, counts=counts)
        face = np.repeat(np.arange(t), number)                    # face-major
        k = np.arange(total) - base[face] + first[face]
        level = levels[k]
        corners = tri[face]
        high = s[corners] >= level[:, None]
        j0 = np.where((high[:, 0] != high[:, 1]) & (high[:, 0] != high[:, 2]), 0, np.where(high[:, 1] != high[:, 0], 1, 2))
        rows = np.arange(total)
        c0, c1, c2 = corners[rows, j0], corners[rows, (j0 + 1) % 3], corners[rows, (j0 + 2) % 3]
        on_a, t_a = _crossing(s, p, c, c0, c1, level)             # hA = c0 -> c1 = 3 f + j0
        on_b, t_b = _crossing(s, p, c, c2, c0, level)             # hB = c2 -> c0 = 3 f + (j0 + 2) % 3
        from_a = high[rows, j0]
        start = np.where(from_a[:, None], on_a, on_b)
        end = np.where(from_a[:, None], on_b, on_a)
        t_start, t_end = np.where(from_a, t_a, t_b), np.where(from_a, t_b, t_a)
        g = twin[3 * face + np.where(from_a, (j0 + 2) % 3, j0)]
        linked = (g >= 0) & (g < 3 * t)
        gf = np.where(linked, g, 0) // 3
        linked &= usable[gf] & (k >= first[gf]) & (k < last[gf])
        succ = np.where(linked, base[gf] + (k - first[gf]), -1)
        d = end.astype(D) - start.astype(D)
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    pred = np.full(total, -1, np.int64)
    pred[succ[succ >= 0]] = np.flatnonzero(succ >= 0)
    succ_l, pred_l = succ.tolist(), pred.tolist()
    # the walk: heads first come out in ascending number anyway, because curves are numbered by their first segment
    owner = [-1] * total
    chains = []   # (first segment, its segments in order, closed)
    for head in range(total):
        if pred_l[head] >= 0:
            continue
        chain, at = [], head
        while at >= 0:
            owner[at] = head
            chain.append(at)
            at = succ_l[at]
        chains.append((head, chain, 0))
    for seed in range(total):          # what is left lies on cycles: ascending, so a cycle is met at its lowest member
        if owner[seed] >= 0:
            continue
        chain, at = [], seed
        while owner[at] < 0:
            owner[at] = seed
            chain.append(at)
            at = succ_l[at]
        chains.append((seed, chain, 1))
    chains.sort(key=lambda item: item[0])
    q_total = len(chains)
    points = total + q_total
    out_pos, out_temp = np.zeros((points, 3), F), np.zeros(points, F)
    out_arc, out_face = np.zeros(points, D), np.zeros(points, np.int32)
    curves = np.zeros(q_total, CURVE_DTYPE)
    at = 0
    for q, (head, chain, closed) in enumerate(chains):
        n = len(chain)
        idx = np.asarray(chain)
        out_pos[at], out_temp[at] = start[head], t_start[head]
        out_pos[at + 1:at + n + 1], out_temp[at + 1:at + n + 1] = end[idx], t_end[idx]
        out_face[at:at + n], out_face[at + n] = face[idx], face[idx[-1]]
        arc = np.add.accumulate(np.concatenate([[0.0], length[idx]]))        # sequential, from +0.0
        out_arc[at:at + n + 1] = arc
        tp = out_temp[at:at + n + 1].astype(D)
        w = np.add.accumulate(np.concatenate([[0.0], length[idx] * (0.5 * (tp[:-1] + tp[1:]))]))[-1]
        keys = order_keys(out_temp[at:at + n + 1])
        with np.errstate(all="ignore"):
            mean = NAN if arc[-1] == 0.0 else F(w / arc[-1])
        curves[q] = (arc[-1], int(k[head]), at, n + 1, closed, mean, out_temp[at + int(np.argmin(keys))],
                     out_temp[at + int(np.argmax(keys))], int(face[head]))
        at += n + 1
    counts[1], counts[2], counts[3] = q_total, points, sum(item[2] for item in chains)
    return {"counts": counts, "curves": curves, "positions": out_pos, "temperature": out_temp, "arc": out_arc, "face": out_face}


# ---- the test meshes ----------------------------------------------------------------------------------------------------------------------

def cube():
    """the unit cube, 12 outward faces: positions, triangles"""
    pos = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], F)   # vertex 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z, outward
    tri = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return pos, tri


def octahedron():
    """the six unit points, eight outward faces; its equator z = 0 passes through four vertices"""
    pos = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)
    tri = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (1, 0, 5), (2, 1, 5), (3, 2, 5), (0, 3, 5)], np.int32)
    return pos, tri


def tube(columns, rings, radius=1.0, wrap=True):
    """`rings` rings of `columns` vertices around the z axis at z = 0, 1, ..: an open tube (a boundary at both ends) of
    2 * columns faces per band, outward; without `wrap` the seam stays open: a band of 2 * (columns - 1) faces"""
    angle = 2.0 * np.pi * np.arange(columns) / columns
    ring = np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1)
    pos = np.concatenate([np.concatenate([ring, np.full((columns, 1), float(z))], axis=1) for z in range(rings)]).astype(F)
    tri = []
    for z in range(rings - 1):
        for c in range(columns if wrap else columns - 1):
            a, b = z * columns + c, z * columns + (c + 1) % columns
            tri += [(a, b, b + columns), (a, b + columns, a + columns)]
    return pos, np.array(tri, np.int32).reshape(-1, 3)


def band(faces):
    """the first `faces` triangles of an open two-ring band and the vertices they name: a plane through its middle cuts every face"""
    pos, tri = tube(faces // 2 + 2, 2, radius=3.0, wrap=False)
    # the cut visits a cell's second triangle before its first: an odd band ends with the second triangle of its last cell
    return pos, (tri[:faces] if faces % 2 == 0 else np.delete(tri[:faces + 1], faces - 1, axis=0)).copy()


def fan():
    """three faces on the edge 0 - 1: a non-manifold edge"""
    pos = np.array([(0, 0, 0), (0, 0, 1), (1, 0, 0.5), (-0.5, 1, 0.5), (-0.5, -1, 0.5)], F)
    return pos, np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], np.int32)


def lattice(nx, ny, seed, jitter=0.3):
    """an nx x ny vertex lattice with seeded fp32 jitter (in all three axes), two triangles per cell: positions, triangles"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pos = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3).astype(D) + rng.uniform(-jitter, jitter, (nx * ny, 3))
    i = (x * ny + y)[:-1, :-1].reshape(-1)
    tri = np.stack([np.stack([i, i + ny, i + ny + 1], axis=1), np.stack([i, i + ny + 1, i + 1], axis=1)], axis=1).reshape(-1, 3)
    return pos.astype(F), tri.astype(np.int32)


def bumps(nx, ny, period=6.0, height=1.0):
    """a lattice whose height is a field of bumps, sin x sin: every bump is ringed by closed contour lines"""
    pos, tri = lattice(nx, ny, 0, jitter=0.0)
    p = pos.astype(D)
    p[:, 2] = height * np.sin(2.0 * np.pi * p[:, 0] / period) * np.sin(2.0 * np.pi * p[:, 1] / period)
    return p.astype(F), tri


def wave_temperature(positions, seed):
    """a seeded smooth field with per-vertex noise, about 14 .. 30 degrees"""
    rng = np.random.default_rng(seed + 1000)
    p = np.nan_to_num(np.asarray(positions, D), nan=0.0, posinf=0.0, neginf=0.0)
    return (22.0 + 5.0 * np.sin(p[:, 0] / 4.0 + 0.3) * np.cos(p[:, 1] / 5.0) + 1.5 * np.sin(p[:, 2] * 2.0) +
            rng.uniform(-1.0, 1.0, len(p))).astype(F)
