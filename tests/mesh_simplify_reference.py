"""Vertex-clustering simplification restated in numpy and plain Python — what tn_mesh_simplify (include/thermonerf_hip.h) must give,
byte for byte — written another way than the kernel: the clusters are lists in a dict keyed by the cell's number, the duplicates
are found with a dict from the canonical triple to the first triangle that has it, and the ordered fp64 sums are explicit loops.

inv = 1.0 / float64(float32(voxel_size)); u_a = (float64(p_a) - float64(origin_a)) * inv; a vertex is a member iff its coordinates
are finite and 0 <= u_a < float64(dims_a) on every axis; c_a = int64(u_a); key = (c_z dims_y + c_y) dims_x + c_x.  A triangle is
valid iff its indices are in [0, V) and its vertices are members, degenerate iff two of its clusters are equal; its canonical triple
is the rotation with the smallest cluster first; the first triangle of a canonical triple is kept.  A cluster is used iff a kept
triangle names it; the used clusters in ascending key are the output vertices: the float64 sum over ALL members in ascending index
divided by float64(n) and rounded once to float32, colours (2 S + n) // (2 n)."""
import numpy as np

F32, F64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def cell_keys(positions, origin, voxel_size, dims):
    """list, per vertex: the number of its cell (a Python int) or None for a non-member"""
    p = np.asarray(positions, dtype=F32).reshape(-1, 3)
    inv = F64(1.0) / F64(F32(voxel_size))
    d = [int(v) for v in dims]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (p.astype(F64) - np.asarray(origin, dtype=F32).astype(F64)[None, :]) * inv
        member = np.isfinite(p).all(axis=1) & (u >= 0.0).all(axis=1) & (u < np.asarray(d, dtype=F64)[None, :]).all(axis=1)
    c = np.where(member[:, None], u, 0.0).astype(np.int64)
    key = (c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0]  # below 2^63
    return [k if m else None for k, m in zip(key.tolist(), member.tolist())]


def canonical(a, b, c):
    """the rotation of three different numbers with the smallest first"""
    if a < b and a < c:
        return (a, b, c)
    return (b, c, a) if b < c else (c, a, b)


def rounded_mean(rows, n):
    s = [sum(int(r[ch]) for r in rows) for ch in range(3)]
    return [(2 * x + n) // (2 * n) for x in s]


def simplify(positions, colors, temperature, thermal_colors, triangles, origin, voxel_size, dims):
    """dict of positions float32 [V',3], colors uint8 [V',3], temperature float32 [V'], thermal_colors uint8 [V',3] or None,
    cluster_count int32 [V'], triangles int32 [T',3], triangle_source int32 [T'], vertex_map int32 [V], counts int64 [4]"""
    p = np.asarray(positions, dtype=F32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist()
    v = len(p)
    cluster_of = cell_keys(p, origin, voxel_size, dims)
    first_with, kept, used = {}, [], set()
    dropped = duplicates = 0
    for t, corner in enumerate(tri):
        if not all(0 <= i < v and cluster_of[i] is not None for i in corner):
            dropped += 1
            continue
        a, b, c = (cluster_of[i] for i in corner)
        if a == b or b == c or a == c:
            dropped += 1
            continue
        if first_with.setdefault(canonical(a, b, c), t) != t:
            duplicates += 1
            continue
        kept.append(t)
        used.update((a, b, c))
    vertex_of = {key: k for k, key in enumerate(sorted(used))}
    m = len(vertex_of)
    clusters = {key: [] for key in vertex_of}  # the members of the used cells: ALL of them, referenced or not
    for i, key in enumerate(cluster_of):  # ascending vertex index
        if key in clusters:
            clusters[key].append(i)
    out = {"positions": np.zeros((m, 3), F32), "colors": np.zeros((m, 3), np.uint8), "temperature": np.zeros(m, F32),
           "thermal_colors": None if thermal_colors is None else np.zeros((m, 3), np.uint8), "cluster_count": np.zeros(m, np.int32)}
    for key, k in vertex_of.items():
        rows = clusters[key]
        n = len(rows)
        s = [F64(0.0)] * 4
        for i in rows:
            for c in range(3):
                s[c] = s[c] + F64(p[i, c])
            s[3] = s[3] + F64(temperature[i])
        with np.errstate(over="ignore"):
            out["positions"][k] = [F32(s[c] / F64(n)) for c in range(3)]
            out["temperature"][k] = F32(s[3] / F64(n))
        out["colors"][k] = rounded_mean([colors[i] for i in rows], n)
        if thermal_colors is not None:
            out["thermal_colors"][k] = rounded_mean([thermal_colors[i] for i in rows], n)
        out["cluster_count"][k] = n
    out["triangles"] = np.array([[vertex_of[cluster_of[i]] for i in tri[t]] for t in kept], dtype=np.int32).reshape(-1, 3)
    out["triangle_source"] = np.array(kept, dtype=np.int32)
    out["vertex_map"] = np.array([vertex_of.get(key, -1) for key in cluster_of], dtype=np.int32)
    out["counts"] = np.array([m, len(kept), dropped, duplicates], dtype=np.int64)
    return out


def brute_force(positions, triangles, origin, voxel_size, dims):
    """The integers of ``simplify`` again without a dict, for small meshes: a triangle is a duplicate iff an EARLIER valid,
    non-degenerate triangle equals one of its three rotations (a quadratic scan); a vertex's cluster is found by comparing its cell
    with every other vertex's.  Returns (triangle_source, vertex_map, cluster_count, counts)."""
    p = np.asarray(positions, dtype=F32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist()
    v = len(p)
    cell = cell_keys(p, origin, voxel_size, dims)
    triples = []
    for corner in tri:
        ok = all(0 <= i < v and cell[i] is not None for i in corner)
        abc = tuple(cell[i] for i in corner) if ok else None
        triples.append(abc if ok and len(set(abc)) == 3 else None)
    kept, duplicates = [], 0
    for t, abc in enumerate(triples):
        if abc is None:
            continue
        rotations = (abc, abc[1:] + abc[:1], abc[2:] + abc[:2])
        if any(earlier in rotations for earlier in triples[:t] if earlier is not None):
            duplicates += 1
        else:
            kept.append(t)
    named = sorted({c for t in kept for c in triples[t]})
    vertex_map = [named.index(c) if c in named else -1 for c in cell]
    cluster_count = [sum(1 for c in cell if c == key) for key in named]
    counts = [len(named), len(kept), len(tri) - len(kept) - duplicates, duplicates]
    return (np.array(kept, np.int32), np.array(vertex_map, np.int32), np.array(cluster_count, np.int32), np.array(counts, np.int64))


def random_attributes(seed, n, thermal=True):
    """(colors uint8 [n,3], temperature float32 [n], thermal_colors uint8 [n,3] or None)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.uniform(14.0, 33.0, n).astype(F32),
            rng.integers(0, 256, (n, 3), dtype=np.uint8) if thermal else None)


def random_positions(seed, n, extent=8.0, bad=0.03):
    """float32 [n,3] in [0, extent)^3, a few of them NaN, +inf, -inf, below 0 or at / beyond ``extent`` (outside a grid over
    [0, extent)^3)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, extent, (n, 3)).astype(F32)
    p = np.minimum(p, np.nextafter(F32(extent), F32(0.0)))
    rows = np.flatnonzero(rng.uniform(size=n) < bad)
    p[rows, rng.integers(0, 3, len(rows))] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.25, extent, 2 * extent], F32), len(rows))
    return p


# ---- the hand-written cases: a grid of 4 x 4 x 4 unit cells at the origin (key = (cz 4 + cy) 4 + cx), every expected value a literal.
# Floats are written as fp32 bit patterns: 0.5 3F000000, 1.5 3FC00000, 2.5 40200000, 12.5 41480000, 14 41600000, 15 41700000,
# 20 41A00000, 21 41A80000, 22 41B00000, 22.5 41B40000, 24 41C00000, 25 41C80000, 27 41D80000, 30 41F00000, 33 42040000 ---------------

GRID = dict(origin=(0.0, 0.0, 0.0), voxel_size=1.0, dims=(4, 4, 4))
H, O, T = 0x3F000000, 0x3FC00000, 0x40200000  # 0.5, 1.5, 2.5
NAN = float("nan")

LITERAL = {
    # two triangles sharing an edge, four vertices in four cells: the output is the input
    "four_cells": dict(
        positions=[[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]],
        colors=[[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]], temperature=[20.0, 22.0, 24.0, 30.0],
        thermal_colors=[[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], triangles=[[0, 1, 2], [1, 3, 2]],
        want=dict(positions=[[H, H, H], [O, H, H], [H, O, H], [O, O, H]], temperature=[0x41A00000, 0x41B00000, 0x41C00000, 0x41F00000],
                  colors=[[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]],
                  thermal_colors=[[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], cluster_count=[1, 1, 1, 1],
                  triangles=[[0, 1, 2], [1, 3, 2]], triangle_source=[0, 1], vertex_map=[0, 1, 2, 3], counts=[4, 2, 0, 0])),
    # a strip of two quads; vertices 2 and 4 share cell 1: triangle 2 collapses, the cell's vertex is their mean (x (1.25 + 1.75) / 2,
    # 22.5 degrees) and its colour sums 21, 25, 510 and 1, 2, 5 round half up to 11, 13, 255 and 1, 1, 3
    "quad_strip": dict(
        positions=[[0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.25, 0.5, 0.5], [1.5, 1.5, 0.5], [1.75, 0.5, 0.5], [2.5, 1.5, 0.5]],
        colors=[[1, 2, 3], [4, 5, 6], [10, 11, 255], [7, 8, 9], [11, 14, 255], [12, 13, 14]],
        temperature=[14.0, 15.0, 20.0, 30.0, 25.0, 33.0],
        thermal_colors=[[20, 21, 22], [30, 31, 32], [0, 1, 2], [40, 41, 42], [1, 1, 3], [50, 51, 52]],
        triangles=[[0, 2, 1], [2, 3, 1], [2, 4, 3], [4, 5, 3]],
        want=dict(positions=[[H, H, H], [O, H, H], [H, O, H], [O, O, H], [T, O, H]],
                  temperature=[0x41600000, 0x41B40000, 0x41700000, 0x41F00000, 0x42040000],
                  colors=[[1, 2, 3], [11, 13, 255], [4, 5, 6], [7, 8, 9], [12, 13, 14]],
                  thermal_colors=[[20, 21, 22], [1, 1, 3], [30, 31, 32], [40, 41, 42], [50, 51, 52]], cluster_count=[1, 2, 1, 1, 1],
                  triangles=[[0, 1, 2], [1, 3, 2], [1, 4, 3]], triangle_source=[0, 1, 3], vertex_map=[0, 2, 1, 3, 1, 4],
                  counts=[5, 3, 1, 0])),
    # cells 0, 1, 4 with two vertices each: triangle 1 is triangle 0's triple rotated (a duplicate), triangle 2 is wound the other way
    # (stays); no thermal colours
    "rotated_and_opposite": dict(
        positions=[[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.25, 0.5, 0.5], [1.75, 0.5, 0.5], [0.5, 1.25, 0.5], [0.5, 1.75, 0.5]],
        colors=[[0, 1, 2], [10, 11, 12], [20, 21, 22], [30, 31, 32], [40, 41, 42], [50, 51, 52]],
        temperature=[20.0, 22.0, 24.0, 30.0, 10.0, 15.0], thermal_colors=None, triangles=[[0, 2, 4], [3, 5, 1], [1, 5, 3]],
        want=dict(positions=[[H, H, H], [O, H, H], [H, O, H]], temperature=[0x41A80000, 0x41D80000, 0x41480000],
                  colors=[[5, 6, 7], [25, 26, 27], [45, 46, 47]], thermal_colors=None, cluster_count=[2, 2, 2],
                  triangles=[[0, 1, 2], [0, 2, 1]], triangle_source=[0, 2], vertex_map=[0, 0, 1, 1, 2, 2], counts=[3, 2, 0, 1])),
    # a tetrahedron inside cell 5 around a real triangle over cells 0, 2, 8: the island vanishes, its cluster is unused
    "island_in_one_cell": dict(
        positions=[[1.25, 1.25, 0.25], [1.75, 1.25, 0.25], [1.25, 1.75, 0.25], [1.25, 1.25, 0.75], [0.5, 0.5, 0.5], [2.5, 0.5, 0.5],
                   [0.5, 2.5, 0.5]],
        colors=[[9, 9, 9]] * 4 + [[1, 2, 3], [4, 5, 6], [7, 8, 9]], temperature=[33.0] * 4 + [20.0, 22.0, 24.0],
        thermal_colors=[[8, 8, 8]] * 4 + [[3, 2, 1], [6, 5, 4], [9, 8, 7]],
        triangles=[[0, 2, 1], [0, 1, 3], [4, 5, 6], [1, 2, 3], [2, 0, 3]],
        want=dict(positions=[[H, H, H], [T, H, H], [H, T, H]], temperature=[0x41A00000, 0x41B00000, 0x41C00000],
                  colors=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], thermal_colors=[[3, 2, 1], [6, 5, 4], [9, 8, 7]], cluster_count=[1, 1, 1],
                  triangles=[[0, 1, 2]], triangle_source=[2], vertex_map=[-1, -1, -1, -1, 0, 1, 2], counts=[3, 1, 4, 0])),
    # vertex 1 is in no triangle but shares cell 0 with vertex 0: it counts in the mean (25 degrees, colour (0 + 255) / 2 -> 128);
    # vertex 4 is alone in cell 63 and unreferenced, 5 has a NaN, 6 lies outside the grid; index 7 does not exist
    "unreferenced_member": dict(
        positions=[[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [3.5, 3.5, 3.5], [NAN, 0.5, 0.5], [4.5, 0.5, 0.5]],
        colors=[[0, 0, 0], [255, 255, 255], [1, 2, 3], [4, 5, 6], [7, 7, 7], [8, 8, 8], [9, 9, 9]],
        temperature=[20.0, 30.0, 22.0, 24.0, 33.0, 33.0, 33.0], thermal_colors=None,
        triangles=[[0, 2, 7], [0, 2, 3], [0, 2, 5], [2, 3, 6]],
        want=dict(positions=[[H, H, H], [O, H, H], [H, O, H]], temperature=[0x41C80000, 0x41B00000, 0x41C00000],
                  colors=[[128, 128, 128], [1, 2, 3], [4, 5, 6]], thermal_colors=None, cluster_count=[2, 1, 1],
                  triangles=[[0, 1, 2]], triangle_source=[1], vertex_map=[0, 0, 1, 2, -1, -1, -1], counts=[3, 1, 3, 0])),
}


def literal_arrays(case):
    """(positions, colors, temperature, thermal_colors or None, triangles) of a literal case as arrays"""
    thermal = case["thermal_colors"]
    return (np.array(case["positions"], F32), np.array(case["colors"], np.uint8), np.array(case["temperature"], F32),
            None if thermal is None else np.array(thermal, np.uint8), np.array(case["triangles"], np.int32).reshape(-1, 3))


def literal_want(case):
    """the expected outputs of a literal case in the form ``simplify`` returns them"""
    w = case["want"]
    return {"positions": np.array(w["positions"], np.uint32).view(F32).reshape(-1, 3),
            "temperature": np.array(w["temperature"], np.uint32).view(F32), "colors": np.array(w["colors"], np.uint8).reshape(-1, 3),
            "thermal_colors": None if w["thermal_colors"] is None else np.array(w["thermal_colors"], np.uint8).reshape(-1, 3),
            "cluster_count": np.array(w["cluster_count"], np.int32), "triangles": np.array(w["triangles"], np.int32).reshape(-1, 3),
            "triangle_source": np.array(w["triangle_source"], np.int32), "vertex_map": np.array(w["vertex_map"], np.int32),
            "counts": np.array(w["counts"], np.int64)}


def same(got, want):
    """the first key at which two result dicts differ (integers exactly, floats by bit pattern), or None"""
    for key, w in want.items():
        g = got[key]
        if (w is None) != (g is None):
            return key
        if w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or not np.array_equal(bits(g) if w.dtype == F32 else g, bits(w) if w.dtype == F32 else w):
            return key
    return None
