"""The yardstick of tn_mesh_peaks, tn_basin_persistence and tn_mesh_spots: the definitions of include/thermonerf_hip.h restated by
another route — ranks from numpy's stable argsort, neighbours from a brute-force pass over the triangles, basins from walking ``up``
vertex by vertex, persistence from the classical VERTEX sweep (the saddle table plays no part in it), rows from the functions of
tests/mesh_regions_reference.py — in plain Python and numpy float64, every float operation one correctly rounded IEEE operation."""
from __future__ import annotations

import math

import numpy as np

from tests import mesh_regions_reference as R

F, D = np.float32, np.float64
SADDLE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("pass_vertex", "<i4"), ("pass_rank", "<i4")])
SPOT_DTYPE = np.dtype(R.REGION_DTYPE.descr + [("vertices", "<i4"), ("reserved", "<i4")])
NEVER = 2 ** 31 - 1


def ranks(temperature, coldest=False):
    """(rank int32 [V], by_rank int64 [V], finite bool [V])"""
    temp = np.asarray(temperature, F).reshape(-1)
    finite = np.isfinite(temp)
    value = temp.astype(D)
    key = np.where(finite, value if coldest else -value, np.inf)  # -0.0 == +0.0 for the sort; no finite key is infinite
    by_rank = np.argsort(key, kind="stable")
    rank = np.empty(len(temp), np.int32)
    rank[by_rank] = np.arange(len(temp), dtype=np.int32)
    return rank, by_rank, finite


def valid_triangles(triangles, v):
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    return tri, ((tri >= 0) & (tri < v)).all(axis=1)


def neighbours(triangles, v, finite, lists=None):
    """per vertex the set of its finite neighbours, from all valid triangles — or, with ``lists`` = (offsets, corners), from the
    corners of its clipped list alone, as the kernel reads a foreign index"""
    tri, valid = valid_triangles(triangles, v)
    if lists is None:  # the corner (t, j) of every valid triangle belongs to the vertex it names
        owned = [(int(tri[t, j]), int(t), j) for t in np.flatnonzero(valid) for j in range(3)]
    else:  # ... or to the vertex whose list holds it
        offsets, corners = (np.asarray(a, np.int64) for a in lists)
        owned = []
        for x in range(v):
            begin, end = max(int(offsets[x]), 0), min(int(offsets[x + 1]), 3 * len(tri))
            listed = [int(corners[i]) for i in range(begin, end)]  # (a range, not a slice: an end below zero is an empty list)
            owned += [(x, c // 3, c % 3) for c in listed if 0 <= c < 3 * len(tri) and valid[c // 3]]
    out = [set() for _ in range(v)]
    for x, t, j in owned:
        for n in (int(tri[t, (j + 1) % 3]), int(tri[t, (j + 2) % 3])):
            if n != x and finite[x] and finite[n]:
                out[x].add(n)
    return out


def peaks(temperature, triangles, coldest=False, lists=None):
    """everything tn_mesh_peaks writes: rank, vertex_basin (int32 [V]), basin_peak (int32 [B]), saddles (SADDLE_DTYPE [S]), counts"""
    temp = np.asarray(temperature, F).reshape(-1)
    v = len(temp)
    rank, by_rank, finite = ranks(temp, coldest)
    near = neighbours(triangles, v, finite, lists)
    up = np.arange(v)
    for x in range(v):
        if finite[x] and near[x]:
            best = min(near[x], key=lambda n: rank[n])
            if rank[best] < rank[x]:
                up[x] = best
    peak = np.full(v, -1, np.int64)
    for x in range(v):
        if finite[x]:
            y, path = x, []
            while up[y] != y and peak[y] < 0:  # walk until a peak, or a vertex whose walk is already known
                path.append(y)
                y = up[y]
            top = y if peak[y] < 0 else peak[y]
            peak[y] = top
            for z in path:
                peak[z] = top
    basin_peak = np.array(sorted(set(peak[finite].tolist())), np.int32)
    number = {int(p): b for b, p in enumerate(basin_peak)}
    vertex_basin = np.array([number[int(p)] if p >= 0 else -1 for p in peak], np.int32)
    tri, valid = valid_triangles(triangles, v)
    best = {}
    for t in np.flatnonzero(valid):
        for j in range(3):
            u, w = int(tri[t, j]), int(tri[t, (j + 1) % 3])
            if not (finite[u] and finite[w]):
                continue
            a, b = int(vertex_basin[u]), int(vertex_basin[w])
            if a == b:
                continue
            pair, edge_pass = (min(a, b), max(a, b)), int(max(rank[u], rank[w]))
            best[pair] = min(best.get(pair, edge_pass), edge_pass)
    saddles = np.zeros(len(best), SADDLE_DTYPE)
    for s, pair in enumerate(sorted(best)):
        saddles[s] = (pair[0], pair[1], int(by_rank[best[pair]]), best[pair])
    counts = np.array([len(basin_peak), len(saddles), int(finite.sum())], np.int64)
    return {"rank": rank, "vertex_basin": vertex_basin, "basin_peak": basin_peak, "saddles": saddles, "counts": counts,
            "by_rank": by_rank, "finite": finite, "near": near}


def sweep(found):
    """(death_vertex, parent), int32 [B]: the classical vertex sweep over ``found`` = peaks(...).  Vertices are taken in rank order;
    each joins the components of its higher neighbours; all but the eldest of those die at that vertex, with the eldest as parent"""
    rank, by_rank, finite, near = found["rank"], found["by_rank"], found["finite"], found["near"]
    vertex_basin, basin_peak = found["vertex_basin"], found["basin_peak"]
    b = len(basin_peak)
    death_vertex, parent = np.full(b, -1, np.int32), np.full(b, -1, np.int32)
    root_of, eldest = {}, {}  # union-find over the vertices swept so far; per root the eldest basin of the component

    def find(x):
        while root_of[x] != x:
            root_of[x] = root_of[root_of[x]]
            x = root_of[x]
        return x

    for x in by_rank.tolist():
        if not finite[x]:
            break
        roots = sorted({find(n) for n in near[x] if rank[n] < rank[x]}, key=lambda r: rank[basin_peak[eldest[r]]])
        root_of[x] = x
        if not roots:
            eldest[x] = int(vertex_basin[x])
            continue
        first = roots[0]
        root_of[x] = first
        for r in roots[1:]:
            death_vertex[eldest[r]], parent[eldest[r]] = x, eldest[first]
            root_of[r] = first
    return death_vertex, parent


def merge(basin_rank, saddles):
    """(death_saddle, parent): the batches over the basin graph, as the header defines tn_basin_persistence — dicts and lists"""
    b = len(basin_rank)
    rep = list(range(b))

    def find(x):
        while rep[x] != x:
            x = rep[x]
        return x

    death, parent = np.full(b, -1, np.int32), np.full(b, -1, np.int32)
    rows = sorted(range(len(saddles)), key=lambda s: (int(saddles["pass_rank"][s]), s))
    at = 0
    while at < len(rows):
        end, died = at, []
        while end < len(rows) and saddles["pass_rank"][rows[end]] == saddles["pass_rank"][rows[at]]:
            s = rows[end]
            ra, rb = find(int(saddles["a"][s])), find(int(saddles["b"][s]))
            if ra != rb:
                young, old = (rb, ra) if basin_rank[ra] < basin_rank[rb] else (ra, rb)
                rep[young] = old
                death[young] = s
                died.append(young)
            end += 1
        for d in died:
            parent[d] = find(d)
        at = end
    return death, parent


def prominence(temperature, basin_peak, saddles, death_saddle, coldest=False):
    temp = np.asarray(temperature, F).reshape(-1)
    out = np.full(len(basin_peak), np.inf, F)
    for b, s in enumerate(death_saddle):
        if s >= 0:
            top, low = D(temp[basin_peak[b]]), D(temp[saddles["pass_vertex"][s]])
            out[b] = F(low - top) if coldest else F(top - low)
    return out


def hotspots(positions, temperature, triangles, min_prominence, coldest=False, extent_drop=math.inf):
    """the whole chain: peaks, the merge, the spots, vertex_spot, face_spot, the rows (SPOT_DTYPE [K]) and counts of tn_mesh_spots"""
    pos, temp = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    found = peaks(temp, triangles, coldest)
    rank, vertex_basin, basin_peak, saddles = found["rank"], found["vertex_basin"], found["basin_peak"], found["saddles"]
    basin_rank = rank[basin_peak] if len(basin_peak) else np.zeros(0, np.int32)
    death, parent = merge(basin_rank, saddles)
    prom = prominence(temp, basin_peak, saddles, death, coldest)
    survive = [float(p) > float(min_prominence) for p in prom]
    chosen = sorted((b for b in range(len(prom)) if survive[b]), key=lambda b: (-float(prom[b]), int(basin_rank[b])))
    number = {b: k for k, b in enumerate(chosen)}
    basin_spot = np.full(len(prom), -1, np.int32)
    for b in range(len(prom)):
        x = b
        while x >= 0 and not survive[x]:
            x = int(parent[x])
        basin_spot[b] = number[x] if x >= 0 else -1
    k = len(chosen)
    limit = np.array([int(saddles["pass_rank"][death[b]]) if death[b] >= 0 else NEVER for b in chosen], np.int32)
    with np.errstate(over="ignore"):
        bound = np.array([F(D(temp[basin_peak[b]]) + D(extent_drop)) if coldest else F(D(temp[basin_peak[b]]) - D(extent_drop))
                          for b in chosen], F)
    vertex_spot = np.full(len(temp), -1, np.int32)
    for x in range(len(temp)):
        if vertex_basin[x] >= 0:
            s = int(basin_spot[vertex_basin[x]])
            if s >= 0 and rank[x] < limit[s] and (temp[x] <= bound[s] if coldest else temp[x] >= bound[s]):
                vertex_spot[x] = s
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    usable, _, tf, area, centroid = R.face_quantities(pos, temp, tri, -math.inf, math.inf)
    face_spot = np.full(len(tri), -1, np.int32)
    for t in np.flatnonzero(usable):
        s = vertex_spot[tri[t]]
        if s[0] >= 0 and s[0] == s[1] == s[2]:
            face_spot[t] = s[0]
    table = np.zeros(k, SPOT_DTYPE)
    for s in range(k):
        faces = np.flatnonzero(face_spot == s).tolist()
        row = table[s]
        row["label"], row["faces"], row["vertices"] = basin_peak[chosen[s]], len(faces), int((vertex_spot == s).sum())
        a = area[faces].tolist()
        total = R.sum2(a)
        row["area"] = total
        for name in ("mean_temperature", "min_temperature", "max_temperature", "centroid", "bounds"):
            row[name] = R.NAN
        row["hottest_vertex"] = row["coldest_vertex"] = -1
        if not faces:
            continue
        vertices = sorted(set(tri[faces].reshape(-1).tolist()))
        if total != 0.0:
            with np.errstate(over="ignore"):
                row["mean_temperature"] = F(D(R.sum2(x * float(c) for x, c in zip(a, tf[faces].astype(D).tolist()))) / D(total))
                for c in range(3):
                    row["centroid"][c] = F(D(R.sum2(x * y for x, y in zip(a, centroid[faces, c].tolist()))) / D(total))
        row["min_temperature"], row["max_temperature"] = R.lowest(tf[faces]), R.highest(tf[faces])
        for c in range(3):
            row["bounds"][c], row["bounds"][3 + c] = R.lowest(pos[vertices, c]), R.highest(pos[vertices, c])
        hot = cold = vertices[0]
        for x in vertices[1:]:
            if float(temp[x]) > float(temp[hot]):
                hot = x
            if float(temp[x]) < float(temp[cold]):
                cold = x
        row["hottest_vertex"], row["coldest_vertex"] = hot, cold
    for name in ("mean_temperature", "min_temperature", "max_temperature", "centroid", "bounds"):  # the one NaN: 0x7fc00000
        view = table[name].view(np.uint32)
        view[np.isnan(table[name])] = 0x7fc00000
    counts = np.array([len(set(face_spot[face_spot >= 0].tolist())), int((face_spot >= 0).sum()), int(usable.sum())], np.int64)
    return {"peaks": found, "basin_rank": basin_rank, "death_saddle": death, "parent": parent, "prominence": prom,
            "spot_basin": np.array(chosen, np.int64), "basin_spot": basin_spot, "spot_limit": limit, "spot_bound": bound,
            "vertex_spot": vertex_spot, "face_spot": face_spot, "spots": table, "counts": counts}


# ---- the test meshes ----------------------------------------------------------------------------------------------------------------------

def grid(nx, ny):
    """an nx x ny vertex lattice without jitter, vertex (x, y) at index x * ny + y, two triangles per cell"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pos = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3).astype(F)
    i = (x * ny + y)[:-1, :-1].reshape(-1)
    tri = np.stack([np.stack([i, i + ny, i + ny + 1], axis=1), np.stack([i, i + ny + 1, i + 1], axis=1)], axis=1).reshape(-1, 3)
    return pos, tri.astype(np.int32)


def two_bumps():
    """the 5 x 5 lattice by hand: bumps of 9 degrees at (1, 1) and 7 degrees at (3, 3) on a floor of 1 degree, the cell between them,
    (2, 2), at 4 degrees.  Two peaks; the floor's vertices climb to one or the other.  The bumps' basins meet along many edges; the
    highest lower end of any of them is (2, 2): the saddle, 4 degrees, so the second bump's prominence is 7 - 4 = 3 degrees"""
    pos, tri = grid(5, 5)
    temp = np.ones(25, F)
    temp[1 * 5 + 1], temp[3 * 5 + 3], temp[2 * 5 + 2] = 9.0, 7.0, 4.0
    return pos, temp, tri


def incidence(triangles, v):
    """tn_mesh_incidence's offsets and corners (include/thermonerf_hip.h), for the raw calls of the tests"""
    tri, valid = valid_triangles(triangles, v)
    keys = np.where(np.repeat(valid, 3), tri.reshape(-1), v)
    corners = np.argsort(keys, kind="stable").astype(np.int32)
    offsets = np.searchsorted(keys[corners], np.arange(v + 1), side="left").astype(np.int32)
    return offsets, corners


def soup(seed):
    """a random triangle soup of 3 - 60 vertices, temperatures from 1 - 7 distinct values (heavy ties) and 10 % NaN"""
    rng = np.random.default_rng(seed)
    v = int(rng.integers(3, 61))
    t = int(rng.integers(1, 2 * v + 1))
    tri = rng.integers(0, v, size=(t, 3)).astype(np.int32)
    temp = rng.integers(0, int(rng.integers(1, 8)), size=v).astype(F)
    temp[rng.uniform(size=v) < 0.1] = np.nan
    return temp, tri
