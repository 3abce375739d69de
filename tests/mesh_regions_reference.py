"""The yardstick of tn_mesh_regions: the definition of include/thermonerf_hip.h restated in numpy float64 and plain Python — a
union-find on dicts, explicit loops for the ordered sum SUM2 — and pinned by the hand-worked literal cases below.  Every numpy
operation used on floats is one correctly rounded IEEE operation per element (add, subtract, multiply, divide, sqrt, the float32
conversion), which is what the header asks of the kernels."""
from __future__ import annotations

import math

import numpy as np

F, D = np.float32, np.float64
BLOCK = 256
REGION_DTYPE = np.dtype([("area", "<f8"), ("label", "<i4"), ("faces", "<i4"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                         ("max_temperature", "<f4"), ("centroid", "<f4", (3,)), ("bounds", "<f4", (6,)), ("coldest_vertex", "<i4"),
                         ("hottest_vertex", "<i4")])
NAN = np.array([0x7fc00000], np.uint32).view(F)[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the ordered sums -------------------------------------------------------------------------------------------------------------------

def sequential_sum(values) -> float:
    s = 0.0
    for x in values:
        s = s + x
    return s


def sum2(values) -> float:
    """blocks of 256 from the start of the list, each from +0.0 in list order; then the block sums from +0.0 in block order"""
    values = [float(x) for x in values]
    return sequential_sum(sequential_sum(values[k:k + BLOCK]) for k in range(0, len(values), BLOCK))


# ---- the extremes' order: the numbers' order with -0.0 below +0.0 ------------------------------------------------------------------------

def order_key(x) -> int:
    b = int(np.array([x], F).view(np.uint32)[0])
    return (~b & 0xffffffff) if b & 0x80000000 else b | 0x80000000


def lowest(values):
    return min(values, key=order_key)


def highest(values):
    return max(values, key=order_key)


# ---- the faces --------------------------------------------------------------------------------------------------------------------------

def face_quantities(positions, temperature, triangles, lo, hi):
    """per face: usable, selected (bool), tf (float32), area (float64, +0.0 unless usable), centroid (float64 [T, 3])"""
    pos, temp, tri = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1), np.asarray(triangles, np.int64).reshape(-1, 3)
    v, t = len(pos), len(tri)
    usable = np.zeros(t, bool)
    if v:
        valid = ((tri >= 0) & (tri < v)).all(axis=1)
        distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
        safe = np.where(valid[:, None], tri, 0)
        finite = np.isfinite(pos[safe]).all(axis=(1, 2)) & np.isfinite(temp[safe]).all(axis=1)
        usable = valid & distinct & finite
    tf, area, centroid = np.zeros(t, F), np.zeros(t, D), np.zeros((t, 3), D)
    rows = np.flatnonzero(usable)
    if len(rows):
        i = tri[rows]
        p0, p1, p2 = (pos[i[:, k]].astype(D) for k in range(3))
        c0, c1, c2 = (temp[i[:, k]].astype(D) for k in range(3))
        with np.errstate(over="ignore"):
            tf[rows] = (((c0 + c1) + c2) / 3.0).astype(F)
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n2 = (cx * cx + cy * cy) + cz * cz
        area[rows] = 0.5 * np.sqrt(n2)
        centroid[rows] = ((p0 + p1) + p2) / 3.0
    selected = usable & (F(lo) <= tf) & (tf <= F(hi))
    return usable, selected, tf, area, centroid


def components_of(triangles, selected):
    """label per vertex over the selected faces (the smallest vertex index of the component), by a union-find on a dict"""
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for t in np.flatnonzero(selected).tolist():
        a, b, c = (int(i) for i in triangles[t])
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return {x: find(x) for x in list(parent)}


def regions(positions, temperature, triangles, lo=-math.inf, hi=math.inf):
    """everything tn_mesh_regions writes: regions (REGION_DTYPE [R]), face_region (int32 [T]), face_area (float64 [T]), counts
    (int64 [3]), totals (float64 [2])"""
    pos, temp, tri = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1), np.asarray(triangles, np.int64).reshape(-1, 3)
    usable, selected, tf, area, centroid = face_quantities(pos, temp, tri, lo, hi)
    label_of = components_of(tri, selected)
    labels = sorted(set(label_of.values()))
    number = {label: r for r, label in enumerate(labels)}
    face_region = np.full(len(tri), -1, np.int32)
    faces_of = {label: [] for label in labels}
    for t in np.flatnonzero(selected).tolist():  # ascending face index
        label = label_of[int(tri[t, 0])]
        face_region[t] = number[label]
        faces_of[label].append(t)
    vertices_of = {label: [] for label in labels}
    for vertex in sorted(label_of):  # ascending vertex index
        vertices_of[label_of[vertex]].append(vertex)
    table = np.zeros(len(labels), REGION_DTYPE)
    for r, label in enumerate(labels):
        faces, vertices = faces_of[label], vertices_of[label]
        a = area[faces].tolist()
        total = sum2(a)
        row = table[r]
        row["area"], row["label"], row["faces"] = total, label, len(faces)
        weighted = sum2(x * float(c) for x, c in zip(a, tf[faces].astype(D).tolist()))
        with np.errstate(over="ignore"):
            row["mean_temperature"] = NAN if total == 0.0 else F(D(weighted) / D(total))
            for k in range(3):
                s = sum2(x * c for x, c in zip(a, centroid[faces, k].tolist()))
                row["centroid"][k] = NAN if total == 0.0 else F(D(s) / D(total))
        row["min_temperature"], row["max_temperature"] = lowest(tf[faces]), highest(tf[faces])
        for k in range(3):
            row["bounds"][k], row["bounds"][3 + k] = lowest(pos[vertices, k]), highest(pos[vertices, k])
        hot = cold = vertices[0]
        for vertex in vertices[1:]:  # compared as numbers; a later vertex must be strictly hotter / colder
            if float(temp[vertex]) > float(temp[hot]):
                hot = vertex
            if float(temp[vertex]) < float(temp[cold]):
                cold = vertex
        row["hottest_vertex"], row["coldest_vertex"] = hot, cold
    flat = table["area"] == 0.0  # the one NaN, whatever the assignment above made of its bits: 0x7fc00000
    table["mean_temperature"].view(np.uint32)[flat] = 0x7fc00000
    table["centroid"].view(np.uint32)[flat] = 0x7fc00000
    totals = np.array([sum2(area[usable].tolist()), sum2(area[selected].tolist())], D)
    counts = np.array([len(labels), int(selected.sum()), int(usable.sum())], np.int64)
    return {"regions": table, "face_region": face_region, "face_area": np.where(usable, area, 0.0).astype(D), "counts": counts,
            "totals": totals}


# ---- the literal cases, worked by hand ----------------------------------------------------------------------------------------------------

SQUARE = dict(positions=[(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], temperature=[20, 23, 26, 29], triangles=[(0, 1, 2), (0, 2, 3)])
LITERAL = {
    # two faces of area 1/2 at (20 + 23 + 26) / 3 = 23 and (20 + 26 + 29) / 3 = 25 degrees: mean 24, centroid the square's centre
    "unit_square_window_open": dict(SQUARE, window=(-math.inf, math.inf), want=dict(
        counts=[1, 2, 2], totals=[1.0, 1.0], face_region=[0, 0], face_area=[0.5, 0.5], area=[1.0], label=[0], faces=[2],
        mean_temperature=[24.0], min_temperature=[23.0], max_temperature=[25.0], centroid=[(0.5, 0.5, 0.0)],
        bounds=[(0, 0, 0, 1, 1, 0)], hottest_vertex=[3], coldest_vertex=[0])),
    # from 24 degrees up only the second face is left: its own mean, its own centroid (1/3, 2/3, 0); the mesh's area stays 1
    "unit_square_one_face_outside": dict(SQUARE, window=(24.0, math.inf), want=dict(
        counts=[1, 1, 2], totals=[1.0, 0.5], face_region=[-1, 0], face_area=[0.5, 0.5], area=[0.5], label=[0], faces=[1],
        mean_temperature=[25.0], min_temperature=[25.0], max_temperature=[25.0], centroid=[(float(F(1 / 3)), float(F(2 / 3)), 0.0)],
        bounds=[(0, 0, 0, 1, 1, 0)], hottest_vertex=[3], coldest_vertex=[0])),
    # a bow tie: the two faces share vertex 2 and nothing else
    "two_patches_touching_in_one_vertex": dict(
        positions=[(0, 0, 0), (0, 2, 0), (1, 1, 0), (2, 0, 0), (2, 2, 0)], temperature=[30, 30, 30, 30, 30],
        triangles=[(0, 2, 1), (2, 3, 4)], window=(25.0, 35.0), want=dict(
            counts=[1, 2, 2], totals=[2.0, 2.0], face_region=[0, 0], area=[2.0], label=[0], faces=[2], mean_temperature=[30.0],
            centroid=[(1.0, 1.0, 0.0)], bounds=[(0, 0, 0, 2, 2, 0)], hottest_vertex=[0], coldest_vertex=[0])),
    # faces 0 and 2 are hot, face 1 between them (vertex 6 is at -30 degrees: (30 + 30 - 30) / 3 = 10) is not: two regions, and the
    # cold face's vertices 2 and 3 belong to one each
    "two_patches_joined_only_through_a_cold_face": dict(
        positions=[(0, 0, 0), (1, 0, 0), (0, 1, 0), (4, 0, 0), (5, 0, 0), (4, 1, 0), (2, 3, 0)], temperature=[30, 30, 30, 30, 30, 30, -30],
        triangles=[(0, 1, 2), (2, 3, 6), (3, 4, 5)], window=(25.0, math.inf), want=dict(
            counts=[2, 2, 3], face_region=[0, -1, 1], area=[0.5, 0.5], label=[0, 3], faces=[1, 1], mean_temperature=[30.0, 30.0],
            bounds=[(0, 0, 0, 1, 1, 0), (4, 0, 0, 5, 1, 0)], hottest_vertex=[0, 3], coldest_vertex=[0, 3])),
    # vertices 1 and 3 are both the hottest, 0 and 2 both the coldest: the lower index each time
    "hottest_vertex_tie": dict(
        positions=SQUARE["positions"], temperature=[10, 40, 10, 40], triangles=SQUARE["triangles"], window=(-math.inf, math.inf),
        want=dict(counts=[1, 2, 2], label=[0], faces=[2], hottest_vertex=[1], coldest_vertex=[0], min_temperature=[20.0],
                  max_temperature=[20.0], mean_temperature=[20.0])),
}


def literal_arrays(case):
    return (np.array(case["positions"], F), np.array(case["temperature"], F), np.array(case["triangles"], np.int32))


def literal_mismatch(got, want):
    """None, or the first field of ``got`` (what ``regions`` returns, or the kernel's outputs in the same shape) that differs"""
    for key, w in want.items():
        g = got[key] if key in got else got["regions"][key]
        if np.asarray(g, D).tolist() != np.asarray(w, D).tolist():
            return f"{key}: {np.asarray(g).tolist()} != {w}"
    return None


# ---- the test meshes ----------------------------------------------------------------------------------------------------------------------

def lattice(nx, ny, seed, jitter=0.3):
    """an nx x ny vertex lattice with seeded fp32 jitter (in all three axes), two triangles per cell: positions, triangles"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pos = np.stack([x, y, np.zeros_like(x)], axis=-1).reshape(-1, 3).astype(D) + rng.uniform(-jitter, jitter, (nx * ny, 3))
    i = (x * ny + y)[:-1, :-1].reshape(-1)
    tri = np.stack([np.stack([i, i + ny, i + ny + 1], axis=1), np.stack([i, i + ny + 1, i + 1], axis=1)], axis=1).reshape(-1, 3)
    return pos.astype(F), tri.astype(np.int32)


def strip(faces, seed):
    """the first ``faces`` triangles of an n x 2 lattice and the vertices they name: one region"""
    pos, tri = lattice((faces + 1) // 2 + 1, 2, seed)
    tri = tri[:faces].copy()
    return pos[:int(tri.max()) + 1].copy(), tri


def lattice_temperature(positions, seed):
    """a seeded field over the lattice: two slow waves and per-vertex noise, about 8 .. 36 degrees, and a calm plateau at 24 degrees
    over the 13 x 13 vertices of one corner (one region of more than 256 faces in a window around 24 degrees)"""
    rng = np.random.default_rng(seed + 1000)
    p = np.asarray(positions, D)
    field = 22.0 + 5.0 * np.sin(p[:, 0] / 4.0) * np.cos(p[:, 1] / 5.0) + rng.uniform(-9.0, 9.0, len(p))
    plateau = (np.rint(p[:, 0]) < 13) & (np.rint(p[:, 1]) < 13)
    return np.where(plateau, 24.0 + rng.uniform(-0.5, 0.5, len(p)), field).astype(F)


# the 40 x 40 lattice of the tests: with this seed and window more than 100 regions, from single faces to the plateau's 300, and areas
# whose SUM2 differs from the sequential sum and from numpy's pairwise sum (test_mesh_regions_cpu.py asserts all of it)
LATTICE_SEED, LATTICE_WINDOW = 3, (23.0, 24.7)
STRIP_SEED = 1  # the strips of 513 and of 65 537 faces tell the three sums apart too


def icosphere(level, radius=1.0):
    """an icosahedron subdivided ``level`` times, every vertex pushed out to the sphere (float64 positions, int32 triangles)"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
             (-g, 0, -1), (-g, 0, 1)]
    verts = [tuple(np.array(p, D) / math.sqrt(1.0 + g * g)) for p in verts]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        middle, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                m = (np.array(verts[a]) + np.array(verts[b])) / 2.0
                verts.append(tuple(m / np.linalg.norm(m)))
                middle[key] = len(verts) - 1
            return middle[key]

        for a, b, c in tris:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    return np.array(verts, D) * radius, np.array(tris, np.int32)
