"""The yardstick of tn_mesh_patches: the definition of include/thermonerf_hip.h restated in numpy float64 and plain Python — a
sequential union-find over the faces, a loop per patch, the ordered sum SUM2 — and pinned by the closed forms of
test_mesh_patches_cpu.py.  Every numpy operation used on floats is one correctly rounded IEEE operation per element (add, subtract,
multiply, divide, sqrt, the float32 conversion), which is what the header asks of the kernels; ``np.cumsum`` along a row adds one
element after the other."""
from __future__ import annotations

import numpy as np

from tests.mesh_isolines_reference import cube, fan, half_edges, tube  # noqa: F401
from tests.mesh_regions_reference import bits, icosphere, lattice, order_key, sum2  # noqa: F401

F, D = np.float32, np.float64
BLOCK = 256
PATCH_DTYPE = np.dtype([("area", "<f8"), ("thermal_area", "<f8"), ("plane", "<f8", (4,)), ("centroid", "<f8", (3,)), ("flatness", "<f4"),
                        ("rms_deviation", "<f4"), ("max_deviation", "<f4"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                        ("max_temperature", "<f4"), ("bounds", "<f4", (6,)), ("label", "<i4"), ("faces", "<i4"),
                        ("thermal_faces", "<i4"), ("reserved", "<i4")])
NAN_BITS = 0x7fc00000


def sum2_fast(values) -> float:
    """``sum2`` for long lists: the blocks as rows behind a leading +0.0, padded with +0.0 (adding +0.0 to a sum that started from +0.0
    changes nothing), ``cumsum`` along each row; then the same over the block sums"""
    x = np.asarray(values, D).reshape(-1)
    if len(x) == 0:
        return 0.0
    blocks = -(-len(x) // BLOCK)
    rows = np.zeros((blocks, BLOCK + 1), D)
    padded = np.zeros(blocks * BLOCK, D)
    padded[:len(x)] = x
    rows[:, 1:] = padded.reshape(blocks, BLOCK)
    partial = np.cumsum(rows, axis=1)[:, -1]
    return float(np.cumsum(np.concatenate([[0.0], partial]))[-1])


def _keys(x):
    """the numbers' order with -0.0 below +0.0, as unsigned keys (``order_key`` on an array)"""
    b = bits(np.asarray(x, F)).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xffffffff, b | 0x80000000)


def lowest(x):
    x = np.asarray(x, F).reshape(-1)
    return x[int(np.argmin(_keys(x)))]


def highest(x):
    x = np.asarray(x, F).reshape(-1)
    return x[int(np.argmax(_keys(x)))]


def face_quantities(positions, temperature, triangles):
    """per face: geometric, thermal (bool), tf (float32), area, c [T, 3], m [T, 3], u [T, 3] (float64, zero unless geometric)"""
    pos, temp, tri = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1), np.asarray(triangles, np.int64).reshape(-1, 3)
    v, t = len(pos), len(tri)
    geometric, thermal = np.zeros(t, bool), np.zeros(t, bool)
    tf, area, c, m, u = np.zeros(t, F), np.zeros(t, D), np.zeros((t, 3), D), np.zeros((t, 3), D), np.zeros((t, 3), D)
    if v == 0 or t == 0:
        return geometric, thermal, tf, area, c, m, u
    inside = ((tri >= 0) & (tri < v)).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    safe = np.where(inside[:, None], tri, 0)
    candidate = inside & distinct & np.isfinite(pos[safe]).all(axis=(1, 2))
    p0, p1, p2 = (pos[safe[:, k]].astype(D) for k in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n2 = (cx * cx + cy * cy) + cz * cz
        geometric = candidate & (n2 > 0.0)
        length = np.sqrt(np.where(geometric, n2, 1.0))
        cross = np.stack([cx, cy, cz], axis=1)
        g = geometric[:, None]
        c = np.where(g, cross, 0.0)
        area = np.where(geometric, 0.5 * length, 0.0)
        m = np.where(g, ((p0 + p1) + p2) / 3.0, 0.0)
        u = np.where(g, cross / length[:, None], 0.0)
        t0, t1, t2 = (temp[safe[:, k]] for k in range(3))
        thermal = geometric & np.isfinite(t0) & np.isfinite(t1) & np.isfinite(t2)
        tf = np.where(thermal, (((t0.astype(D) + t1.astype(D)) + t2.astype(D)) / 3.0).astype(F), F(0))
    return geometric, thermal, tf, area, c, m, u


def joined_half_edges(twin, geometric, u, min_cos):
    """bool [3T]: the half-edges h whose face is JOINED with the face of twin[h]"""
    t = len(geometric)
    tw = np.asarray(twin, np.int64).reshape(-1)
    h = np.arange(3 * t)
    f = h // 3
    inside = (tw >= 0) & (tw < 3 * t)
    g = np.where(inside, tw, 0) // 3
    dot = (u[f, 0] * u[g, 0] + u[f, 1] * u[g, 1]) + u[f, 2] * u[g, 2]
    return inside & (g != f) & geometric[f] & geometric[g] & (dot >= D(min_cos)), g


def patches(positions, temperature, triangles, twin, min_cos):
    """everything tn_mesh_patches writes: patches (PATCH_DTYPE [Q]), face_patch (int32 [T]), counts (int64 [3]), totals (float64 [2])"""
    pos, temp, tri = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1), np.asarray(triangles, np.int64).reshape(-1, 3)
    t = len(tri)
    if len(pos) == 0 or t == 0:
        return {"patches": np.zeros(0, PATCH_DTYPE), "face_patch": np.full(t, -1, np.int32), "counts": np.zeros(3, np.int64),
                "totals": np.zeros(2, D)}
    geometric, thermal, tf, area, c, m, u = face_quantities(pos, temp, tri)
    joined, other = joined_half_edges(twin, geometric, u, min_cos)
    parent = list(range(t))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for h in np.flatnonzero(joined).tolist():
        a, b = find(h // 3), find(int(other[h]))
        if a != b:
            parent[max(a, b)] = min(a, b)  # the root is the smallest face of its class
    faces_of = {}
    for f in np.flatnonzero(geometric).tolist():  # ascending face index
        faces_of.setdefault(find(f), []).append(f)
    labels = sorted(faces_of)
    face_patch = np.full(t, -1, np.int32)
    table = np.zeros(len(labels), PATCH_DTYPE)
    nan = np.array([NAN_BITS], np.uint32).view(F)[0]
    safe = np.clip(tri, 0, len(pos) - 1)
    for q, label in enumerate(labels):
        faces = np.array(faces_of[label], np.int64)
        face_patch[faces] = q
        row = table[q]
        a, warm = area[faces], thermal[faces]
        total = sum2_fast(a)
        thermal_area = sum2_fast(np.where(warm, a, 0.0))
        normal = [sum2_fast(0.5 * c[faces, k]) for k in range(3)]
        centroid = [D(sum2_fast(a * m[faces, k])) / D(total) for k in range(3)]
        row["area"], row["thermal_area"], row["centroid"] = total, thermal_area, centroid
        row["label"], row["faces"], row["thermal_faces"] = label, len(faces), int(warm.sum())
        if thermal_area == 0.0:
            row["mean_temperature"] = row["min_temperature"] = row["max_temperature"] = nan
        else:
            weighted = sum2_fast(np.where(warm, a * tf[faces].astype(D), 0.0))
            row["mean_temperature"] = F(D(weighted) / D(thermal_area))
            row["min_temperature"], row["max_temperature"] = lowest(tf[faces][warm]), highest(tf[faces][warm])
        corners = pos[safe[faces].reshape(-1)]
        for k in range(3):
            row["bounds"][k], row["bounds"][3 + k] = lowest(corners[:, k]), highest(corners[:, k])
        nn = (D(normal[0]) * D(normal[0]) + D(normal[1]) * D(normal[1])) + D(normal[2]) * D(normal[2])
        if nn > 0.0:
            length = np.sqrt(D(nn))
            n = [D(normal[k]) / length for k in range(3)]
            row["plane"][:3] = n
            row["plane"][3] = (n[0] * centroid[0] + n[1] * centroid[1]) + n[2] * centroid[2]
            row["flatness"] = F(length / D(total))
            p = pos[safe[faces]].astype(D)  # [n, 3 corners, 3 axes]
            e = (n[0] * (p[:, :, 0] - centroid[0]) + n[1] * (p[:, :, 1] - centroid[1])) + n[2] * (p[:, :, 2] - centroid[2])
            s = (e[:, 0] + e[:, 1]) + e[:, 2]
            term = (a / 12.0) * (((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + s * s)
            row["rms_deviation"] = F(np.sqrt(D(sum2_fast(term)) / D(total)))
            row["max_deviation"] = F(np.abs(e).max())
        else:
            row["plane"], row["flatness"] = 0.0, 0.0
            row["rms_deviation"] = row["max_deviation"] = nan
    for name in ("rms_deviation", "max_deviation", "mean_temperature", "min_temperature", "max_temperature"):
        column = table[name]  # the one NaN, whatever the assignment above made of its bits
        column.view(np.uint32)[np.isnan(column)] = NAN_BITS
    totals = np.array([sum2_fast(area[geometric]), sum2_fast(area[thermal])], D)
    counts = np.array([len(labels), int(geometric.sum()), int(joined.sum())], np.int64)
    return {"patches": table, "face_patch": face_patch, "counts": counts, "totals": totals}


# ---- the test meshes ----------------------------------------------------------------------------------------------------------------------

def rectangle(origin, a, b):
    """the two triangles (0, 1, 2), (0, 2, 3) of the parallelogram origin, origin + a, origin + a + b, origin + b: normal a x b"""
    o, a, b = (np.asarray(x, D) for x in (origin, a, b))
    return np.array([o, o + a, o + a + b, o + b], F), np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def join_meshes(*meshes):
    """several (positions, triangles) as one mesh, nothing shared"""
    pos, tri, first = [], [], 0
    for p, t in meshes:
        pos.append(np.asarray(p, F))
        tri.append(np.asarray(t, np.int32) + first)
        first += len(p)
    return np.concatenate(pos), np.concatenate(tri)


def weld(positions, triangles):
    """vertices at the same position become one (the lowest index survives in order of first appearance)"""
    pos = np.asarray(positions, F)
    _, first, inverse = np.unique(pos, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return pos[first[order]], rank[inverse.reshape(-1)][np.asarray(triangles, np.int64)].astype(np.int32)


def ell():
    """two unit squares along the edge x = 1, y in [0, 1]: the floor z = 0 (normal +z) and the wall x = 1 (normal -x), welded; the two
    unit normals are exact and their dot product is exactly 0"""
    floor = rectangle((0, 0, 0), (1, 0, 0), (0, 1, 0))
    wall = rectangle((1, 0, 0), (0, 0, 1), (0, 1, 0))
    return weld(*join_meshes(floor, wall))


def roof():
    """two rectangles meeting in a ridge along y, 45 degrees to the ground each; the unit normals carry the rounding of 1 / sqrt(2), so
    the yardstick's own dot product is the threshold"""
    left = rectangle((0, 0, 0), (1, 0, 1), (0, 1, 0))
    right = rectangle((1, 0, 1), (1, 0, -1), (0, 1, 0))
    return weld(*join_meshes(left, right))


def two_cubes_touching():
    """two unit cubes that share the one vertex (1, 1, 1): one vertex component, two edge components"""
    p, t = cube()
    return weld(*join_meshes((p, t), (p + F(1), t)))


def flat_strip(faces):
    """a flat strip of ``faces`` triangles in the plane z = 0, given in REVERSE order: the union-find's worst chain"""
    pos, tri = lattice((faces + 1) // 2 + 1, 2, 0, jitter=0.0)
    return pos[:int(tri[:faces].max()) + 1].copy(), tri[:faces][::-1].copy()


def flat_lattice(nx, ny, seed, permute=True):
    """a flat nx x ny lattice (z = 0 exactly, seeded jitter in x and y of a tenth of a cell so that no face flips), its faces permuted"""
    pos, tri = lattice(nx, ny, seed, jitter=0.1)
    pos[:, 2] = 0.0
    if permute:
        tri = tri[np.random.default_rng(seed + 7).permutation(len(tri))]
    return pos, np.ascontiguousarray(tri)


def strips_lattice(nx, ny, seed, rows_per_strip):
    """``flat_lattice`` folded into strips: every ``rows_per_strip`` rows of cells along x the next strip is lifted by one unit in z, and
    the cells between two strips become vertical steps — patches of many sizes in one mesh"""
    pos, tri = flat_lattice(nx, ny, seed)
    pos[:, 2] = (np.rint(pos[:, 0].astype(D)) // rows_per_strip).astype(F)
    return pos, tri
