"""The yardstick of tn_mesh_geodesic and tn_mesh_distance_bands: the definition of include/thermonerf_hip.h restated in numpy float64,
twice — ``solve_scalar`` follows the header line by line, vertex by vertex and corner by corner, in plain Python; ``solve`` does the
same operations on whole arrays, for the larger cases — and the bands with their SUM2 order.  Both forms evaluate EVERY vertex in every
round, as the kernel does.  Every numpy operation used on floats is one
correctly rounded IEEE operation per element (add, subtract, multiply, divide, sqrt), which is what the header asks of the kernels.
The mesh makers of the tests are here too.  Test code, not product."""
from __future__ import annotations

import math

import numpy as np

from tests import mesh_regions_reference as R

F, D = np.float32, np.float64
INF = math.inf
BAND_DTYPE = np.dtype([("area", "<f8"), ("warm_area", "<f8"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                       ("max_temperature", "<f4"), ("faces", "<i4"), ("warm_faces", "<i4"), ("reserved", "<i4")])


# ---- the lists and the seeds ------------------------------------------------------------------------------------------------------------

def incidence(triangles, v):
    """tn_mesh_incidence's offsets and corners: the corners of the valid triangles, stable by the vertex they name"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    valid = ((tri >= 0) & (tri < v)).all(axis=1) if len(tri) else np.zeros(0, bool)
    keys = np.where(np.repeat(valid, 3), tri.reshape(-1), v)
    corners = np.argsort(keys, kind="stable").astype(np.int32)
    offsets = np.searchsorted(keys[corners], np.arange(v + 1), side="left").astype(np.int32)
    return offsets, corners


def initial(v, seed_vertex, seed_offset):
    """RESTART: (D, L) from the seeds in ascending i"""
    dist, label = np.full(v, INF, D), np.full(v, -1, np.int32)
    for i, (s, o) in enumerate(zip(np.asarray(seed_vertex, np.int64).reshape(-1), np.asarray(seed_offset, D).reshape(-1))):
        if s < 0 or s >= v or not math.isfinite(o) or o < 0.0:
            continue
        o = D(o) + D(0.0)
        if o < dist[s]:
            dist[s], label[s] = o, i
    return dist, label


# ---- the scalar form: the header, line by line ----------------------------------------------------------------------------------------------

def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _norm(x):
    return np.sqrt(_dot(x, x))


def candidates(pc, pa, pb, da, db):
    """the up to three candidates of triangle (c, a, b) as (value, which) with which = 0: a's label, 1: b's"""
    ac, bc, ab = pc - pa, pc - pb, pb - pa
    out = [(da + _norm(ac), 0), (db + _norm(bc), 1)]
    if not (math.isfinite(da) and math.isfinite(db)):
        return out
    u = _norm(ab)
    if not u > 0.0:
        return out
    cr = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]], D)
    cx, cy = _dot(ab, ac) / u, _norm(cr) / u
    if not cy > 0.0:
        return out
    a2 = da * da
    sx = ((u * u + a2) - db * db) / (D(2.0) * u)
    sy2 = a2 - sx * sx
    if not sy2 >= 0.0:
        return out
    sy = np.sqrt(sy2)
    dx, h = cx - sx, cy + sy
    xs = sx + (dx * sy) / h
    if not (xs > 0.0 and xs < u):
        return out
    out.append((np.sqrt(dx * dx + h * h), 0 if da <= db else 1))
    return out


def round_scalar(dist, label, pos, tri, offsets, corners, limit):
    """one ROUND: (D_k+1, L_k+1, the number of vertices that changed)"""
    v, nc = len(dist), 3 * len(tri)
    new_d, new_l, changed = dist.copy(), label.copy(), 0
    with np.errstate(all="ignore"):
        for c in range(v):
            best, lab = dist[c], label[c]
            if np.isfinite(pos[c]).all():
                for i in range(max(int(offsets[c]), 0), min(int(offsets[c + 1]), nc)):
                    k = int(corners[i])
                    if k < 0 or k >= nc:
                        continue
                    t, j = divmod(k, 3)
                    ids = [int(x) for x in tri[t]]
                    if any(x < 0 or x >= v for x in ids) or ids[j] != c:
                        continue
                    a, b = ids[(j + 1) % 3], ids[(j + 2) % 3]
                    if a == b or a == c or b == c or not (np.isfinite(pos[a]).all() and np.isfinite(pos[b]).all()):
                        continue
                    for cand, which in candidates(pos[c].astype(D), pos[a].astype(D), pos[b].astype(D), dist[a], dist[b]):
                        if cand < best and cand <= limit:
                            best, lab = cand, label[a] if which == 0 else label[b]
            new_d[c], new_l[c] = best, lab
            changed += int(best < dist[c])
    return new_d, new_l, changed


# ---- the array form ---------------------------------------------------------------------------------------------------------------------

class Entries:
    """every (vertex, corner of its list) that gives candidates, in list order, with what does not depend on the distances"""

    def __init__(self, pos, tri, offsets, corners):
        v, nc = len(pos), 3 * len(tri)
        begin = np.clip(np.asarray(offsets, np.int64)[:-1], 0, None)
        end = np.clip(np.asarray(offsets, np.int64)[1:], None, nc)
        length = np.clip(end - begin, 0, None)
        owner = np.repeat(np.arange(v, dtype=np.int64), length)
        at = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(np.cumsum(length) - length, length) + np.repeat(begin, length)
        k = np.asarray(corners, np.int64)[at] if len(at) else np.zeros(0, np.int64)
        ok = (k >= 0) & (k < nc)
        k = np.where(ok, k, 0)
        t, j = k // 3, k % 3
        ids = np.asarray(tri, np.int64).reshape(-1, 3)[t] if len(at) else np.zeros((0, 3), np.int64)
        ok &= ((ids >= 0) & (ids < v)).all(axis=1)
        ids = np.where(ok[:, None], ids, 0)
        rows = np.arange(len(at))
        ok &= ids[rows, j] == owner
        a, b = ids[rows, (j + 1) % 3], ids[rows, (j + 2) % 3]
        ok &= (a != b) & (a != owner) & (b != owner)
        fin = np.isfinite(pos).all(axis=1)
        ok &= fin[owner] & fin[a] & fin[b]
        self.c, self.a, self.b = owner[ok], a[ok], b[ok]
        p = pos.astype(D)
        pc, pa, pb = p[self.c], p[self.a], p[self.b]
        with np.errstate(all="ignore"):
            ac, bc, ab = pc - pa, pc - pb, pb - pa
            dot = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]  # noqa: E731
            self.la, self.lb, self.u = np.sqrt(dot(ac, ac)), np.sqrt(dot(bc, bc)), np.sqrt(dot(ab, ab))
            cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                           ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
            self.cx, self.cy = dot(ab, ac) / self.u, np.sqrt(dot(cr, cr)) / self.u
        self.plane = (self.u > 0.0) & (self.cy > 0.0)
        # the segments of the vertices that have an entry, for reduceat over the 3 candidates of every entry
        self.vertices, first = np.unique(self.c, return_index=True)
        self.starts = 3 * first
        self.segment = np.repeat(np.searchsorted(self.vertices, self.c), 3)


def round_arrays(dist, label, e: Entries, limit):
    new_d, new_l = dist.copy(), label.copy()
    if len(e.c) == 0:
        return new_d, new_l, 0
    with np.errstate(all="ignore"):
        da, db = dist[e.a], dist[e.b]
        c3 = np.full(len(e.c), INF, D)
        face = e.plane & np.isfinite(da) & np.isfinite(db)
        u, a, b = e.u[face], da[face], db[face]
        a2 = a * a
        sx = ((u * u + a2) - b * b) / (D(2.0) * u)
        sy2 = a2 - sx * sx
        sy = np.sqrt(np.where(sy2 >= 0.0, sy2, 0.0))
        dx, h = e.cx[face] - sx, e.cy[face] + sy
        xs = sx + (dx * sy) / h
        good = (sy2 >= 0.0) & (xs > 0.0) & (xs < u)
        c3[np.flatnonzero(face)[good]] = np.sqrt(dx * dx + h * h)[good]
        cand = np.stack([da + e.la, db + e.lb, c3], axis=1).reshape(-1)
        lab = np.stack([label[e.a], label[e.b], np.where(da <= db, label[e.a], label[e.b])], axis=1).reshape(-1)
    cand = np.where(cand <= limit, cand, INF)  # (a NaN fails)
    low = np.minimum.reduceat(cand, e.starts)
    index = np.where(cand == low[e.segment], np.arange(len(cand)), len(cand))
    first = np.minimum.reduceat(index, e.starts)
    wins = low < dist[e.vertices]
    vs = e.vertices[wins]
    new_d[vs], new_l[vs] = low[wins], lab[first[wins]]
    return new_d, new_l, int(wins.sum())


def solve(positions, triangles, seed_vertex, seed_offset=None, max_distance=INF, max_rounds=None, lists=None, scalar=False, start=None):
    """the solve by the plain definition: distance, nearest_seed, rounds (those that changed a vertex), converged (a round changed
    nothing); ``max_rounds``: the rounds run at most; ``start``: (D, L) to continue from instead of the seeds"""
    pos = np.asarray(positions, F).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    v = len(pos)
    seed_vertex = np.asarray(seed_vertex, np.int64).reshape(-1)
    seed_offset = np.zeros(len(seed_vertex), D) if seed_offset is None else np.asarray(seed_offset, D).reshape(-1)
    offsets, corners = incidence(tri, v) if lists is None else lists
    dist, label = initial(v, seed_vertex, seed_offset) if start is None else (np.array(start[0], D), np.array(start[1], np.int32))
    entries = None if scalar else Entries(pos, tri, offsets, corners)
    rounds, converged = 0, False
    while not converged and (max_rounds is None or rounds < max_rounds):
        if scalar:
            dist, label, changed = round_scalar(dist, label, pos, tri, offsets, corners, max_distance)
        else:
            dist, label, changed = round_arrays(dist, label, entries, max_distance)
        if changed:
            rounds += 1
        else:
            converged = True
    return dict(distance=dist, nearest_seed=label, rounds=rounds, converged=converged)


# ---- the bands --------------------------------------------------------------------------------------------------------------------------

def bands(positions, temperature, triangles, distance, nearest_seed, width, k, cell=-1):
    """rows (BAND_DTYPE [K]), counts [3], face_band (int64 [T]: the band of a face that takes part, -1 of every other)"""
    pos, temp = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    dist, seed = np.asarray(distance, D), np.asarray(nearest_seed, np.int32)
    v, t = len(pos), len(tri)
    rows = np.zeros(k, BAND_DTYPE)
    for name in ("mean_temperature", "min_temperature", "max_temperature"):
        rows[name] = R.NAN
    face_band = np.full(t, -1, np.int64)
    counts = np.zeros(3, np.int64)
    if v == 0 or t == 0:
        return rows, counts, face_band
    valid = ((tri >= 0) & (tri < v)).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    safe = np.where(valid[:, None], tri, 0)
    placed = valid & distinct & np.isfinite(pos[safe]).all(axis=(1, 2))
    warm = valid & distinct & np.isfinite(temp[safe]).all(axis=1)
    d = dist[safe]
    measured = placed & np.isfinite(d).all(axis=1)
    if cell >= 0:
        measured &= (seed[safe] == cell).all(axis=1)
    with np.errstate(all="ignore"):
        q = (((d[:, 0] + d[:, 1]) + d[:, 2]) / D(3.0)) / D(width)
        p0, p1, p2 = (pos[safe[:, i]].astype(D) for i in range(3))
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = D(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
        c = temp[safe].astype(D)
        tf = (((c[:, 0] + c[:, 1]) + c[:, 2]) / D(3.0)).astype(F)
    inside = measured & (q >= 0.0) & (q < float(k))
    face_band[inside] = np.floor(q[inside]).astype(np.int64)
    counts[:] = (len(np.unique(face_band[inside])), int(inside.sum()), int(measured.sum()))
    for band in np.unique(face_band[inside]):
        faces = np.flatnonzero(face_band == band)  # ascending face index
        hot = warm[faces]
        row = rows[band]
        row["area"] = R.sum2(area[faces])
        row["warm_area"] = R.sum2(np.where(hot, area[faces], 0.0))
        row["faces"], row["warm_faces"] = len(faces), int(hot.sum())
        if row["warm_area"] > 0.0:
            row["mean_temperature"] = F(D(R.sum2(np.where(hot, area[faces] * tf[faces].astype(D), 0.0))) / row["warm_area"])
        if hot.any():
            row["min_temperature"], row["max_temperature"] = R.lowest(tf[faces][hot]), R.highest(tf[faces][hot])
    return rows, counts, face_band


# ---- the test meshes --------------------------------------------------------------------------------------------------------------------

def lattice(nx, ny, pattern="same", jitter=0.0, seed=0):
    """an nx x ny vertex lattice in the plane z = 0, vertex (x, y) at index x * ny + y, every cell split by one diagonal: "same" — always
    from (x, y) to (x + 1, y + 1) — or "alternating" — the other one in every cell with x + y odd; ``jitter``: the inner vertices moved
    by up to that share of a cell"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pos = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3).astype(D)
    if jitter:
        rng = np.random.default_rng(seed)
        inner = ((x > 0) & (x < nx - 1) & (y > 0) & (y < ny - 1)).reshape(-1)
        pos[inner, :2] += rng.uniform(-jitter, jitter, size=(int(inner.sum()), 2))
    i = (x * ny + y)[:-1, :-1].reshape(-1)
    a, b, c, d = i, i + ny, i + ny + 1, i + 1  # (x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)
    main = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1)
    other = np.stack([np.stack([a, b, d], axis=1), np.stack([b, c, d], axis=1)], axis=1)
    odd = (((x + y) % 2 == 1)[:-1, :-1].reshape(-1) if pattern == "alternating" else np.zeros(len(i), bool))
    tri = np.where(odd[:, None, None], other, main).reshape(-1, 3)
    return pos.astype(F), tri.astype(np.int32)


def slit_lattice(n=65, row=32, upto=48):
    """the n x n lattice with the faces of the cells (x, row), x < upto, removed: a slit between the vertex rows y = row and
    y = row + 1 that a path has to go around, at x = upto"""
    pos, tri = lattice(n, n)
    cell = np.repeat(np.arange((n - 1) * (n - 1)), 2)
    cx, cy = cell // (n - 1), cell % (n - 1)
    return pos, np.ascontiguousarray(tri[~((cy == row) & (cx < upto))])


def hub(spokes):
    """a fan of ``spokes`` triangles around vertex 0 on the unit circle: a list of ``spokes`` corners"""
    angle = 2.0 * np.pi * np.arange(spokes) / spokes
    pos = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(angle), np.sin(angle), np.zeros(spokes)], axis=1)]).astype(F)
    k = np.arange(spokes)
    tri = np.stack([np.zeros(spokes, np.int64), 1 + k, 1 + (k + 1) % spokes], axis=1).astype(np.int32)
    return pos, tri


def soup(seed, lo=30, hi=50):
    """a random triangle soup on integer positions (heavy ties) with, now and then, a repeated index, a NaN position and a foreign
    index; two seeds (sometimes the same vertex, sometimes outside [0, V)) with offsets, and a finite max_distance every other time"""
    rng = np.random.default_rng(seed)
    v = int(rng.integers(lo, hi + 1))
    t = int(rng.integers(v, 3 * v))
    pos = rng.integers(0, 6, size=(v, 3)).astype(F)
    if seed % 3 == 0:
        pos += rng.uniform(-0.2, 0.2, size=(v, 3)).astype(F)
    tri = rng.integers(0, v, size=(t, 3)).astype(np.int32)
    pos[int(rng.integers(0, v)), int(rng.integers(0, 3))] = np.nan
    tri[int(rng.integers(0, t)), int(rng.integers(0, 3))] = [v, -1, 2 ** 31 - 1][seed % 3]
    seeds = rng.integers(0, v, size=2).astype(np.int32)
    if seed % 5 == 0:
        seeds[1] = seeds[0]
    if seed % 7 == 0:
        seeds[1] = v + 3
    offsets = rng.integers(0, 3, size=2).astype(D) * 0.5
    limit = float(rng.integers(3, 9)) if seed % 2 else INF
    return pos, tri, seeds, offsets, limit
