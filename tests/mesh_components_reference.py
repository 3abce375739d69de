"""The yardstick of tn_mesh_components / tn_mesh_filter_components: a plain numpy / Python restatement of the definitions in
include/thermonerf_hip.h.  Sequential union-find, nothing clever; test code, not product."""
from __future__ import annotations

import numpy as np


def valid_mask(triangles: np.ndarray, num_vertices: int) -> np.ndarray:
    """bool [T]: all three indices in [0, V)"""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((tri >= 0) & (tri < int(num_vertices))).all(axis=1)


def components(triangles, num_vertices: int) -> dict:
    """labels int32 [V], component_triangles int32 [V], summary int64 [3]"""
    v = int(num_vertices)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    valid = valid_mask(tri, v)
    parent = list(range(v))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in tri[valid].tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)  # the lower index stays the root: a root is its tree's smallest index
    labels = np.array([find(x) for x in range(v)], dtype=np.int32).reshape(v)
    count = np.zeros(v, dtype=np.int32)
    if valid.any():
        np.add.at(count, labels[tri[valid][:, 0]], 1)
    summary = np.zeros(3, dtype=np.int64)
    if v:
        summary[0] = int((labels == np.arange(v)).sum())
        summary[1] = int(count.max())
        summary[2] = int(np.argmax(count))  # the first maximum: the lowest label on a tie, 0 when every count is 0
    return dict(labels=labels, component_triangles=count, summary=summary)


def filter_components(triangles, num_vertices: int, comp: dict, min_triangles: int = 1, largest_only: bool = False) -> dict:
    """vertex_source int32 [V'], triangles int32 [T', 3], counts int64 [2], vertex_map int32 [V]"""
    v = int(num_vertices)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    labels, count = comp["labels"].astype(np.int64), comp["component_triangles"]
    kept_label = count >= max(int(min_triangles), 1)
    if largest_only:
        kept_label &= np.arange(v) == int(comp["summary"][2])
    keep_vertex = kept_label[labels] if v else np.zeros(0, dtype=bool)
    source = np.flatnonzero(keep_vertex).astype(np.int32)
    vertex_map = np.full(v, -1, dtype=np.int32)
    vertex_map[source] = np.arange(len(source), dtype=np.int32)
    valid = valid_mask(tri, v)
    keep_tri = valid.copy()
    keep_tri[valid] = keep_vertex[tri[valid][:, 0]]
    out = vertex_map[tri[keep_tri]].astype(np.int32).reshape(-1, 3)
    return dict(vertex_source=source, triangles=out, counts=np.array([len(source), len(out)], dtype=np.int64), vertex_map=vertex_map)


def bfs_labels(triangles, num_vertices: int) -> np.ndarray:
    """the labels again, by a breadth-first search over an adjacency list: an independent check of ``components``"""
    v = int(num_vertices)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    adjacent = [[] for _ in range(v)]
    for a, b, c in tri[valid_mask(tri, v)].tolist():
        adjacent[a] += [b, c]
        adjacent[b] += [a, c]
        adjacent[c] += [a, b]
    labels = np.full(v, -1, dtype=np.int32)
    for start in range(v):  # ascending: the first vertex to reach a component is its smallest
        if labels[start] >= 0:
            continue
        labels[start] = start
        frontier = [start]
        while frontier:
            nxt = []
            for x in frontier:
                for y in adjacent[x]:
                    if labels[y] < 0:
                        labels[y] = start
                        nxt.append(y)
            frontier = nxt
    return labels


# ---- the hand-written cases: (triangles, V) and every expected array written out -----------------------------------------------------

LITERAL = {
    "empty": dict(
        triangles=[], num_vertices=0, labels=[], component_triangles=[], summary=[0, 0, 0],
        filters={(1, False): dict(vertex_source=[], triangles=[])}),
    "one_triangle_among_five_vertices": dict(
        triangles=[[1, 3, 2]], num_vertices=5, labels=[0, 1, 1, 1, 4], component_triangles=[0, 1, 0, 0, 0], summary=[3, 1, 1],
        filters={(1, False): dict(vertex_source=[1, 2, 3], triangles=[[0, 2, 1]]),
                 (0, True): dict(vertex_source=[1, 2, 3], triangles=[[0, 2, 1]]),
                 (2, False): dict(vertex_source=[], triangles=[])}),
    "two_triangles_sharing_one_vertex": dict(
        triangles=[[4, 5, 6], [0, 1, 4]], num_vertices=7, labels=[0, 0, 2, 3, 0, 0, 0], component_triangles=[2, 0, 0, 0, 0, 0, 0],
        summary=[3, 2, 0],
        filters={(2, False): dict(vertex_source=[0, 1, 4, 5, 6], triangles=[[2, 3, 4], [0, 1, 2]]),
                 (3, False): dict(vertex_source=[], triangles=[])}),
    "two_separate_triangles_tie": dict(
        triangles=[[3, 4, 5], [2, 1, 0]], num_vertices=6, labels=[0, 0, 0, 3, 3, 3], component_triangles=[1, 0, 0, 1, 0, 0],
        summary=[2, 1, 0],
        filters={(1, False): dict(vertex_source=[0, 1, 2, 3, 4, 5], triangles=[[3, 4, 5], [2, 1, 0]]),
                 (1, True): dict(vertex_source=[0, 1, 2], triangles=[[2, 1, 0]])}),
    "invalid_triangles": dict(
        triangles=[[0, 1, -1], [1, 2, 3], [2, 3, 4], [0, 4, 2]], num_vertices=4, labels=[0, 1, 1, 1],
        component_triangles=[0, 1, 0, 0], summary=[2, 1, 1],
        filters={(1, False): dict(vertex_source=[1, 2, 3], triangles=[[0, 1, 2]])}),
    "repeated_index": dict(
        triangles=[[2, 2, 0], [3, 3, 3]], num_vertices=5, labels=[0, 1, 0, 3, 4], component_triangles=[1, 0, 0, 1, 0],
        summary=[4, 1, 0],
        filters={(1, False): dict(vertex_source=[0, 2, 3], triangles=[[1, 1, 0], [2, 2, 2]]),
                 (1, True): dict(vertex_source=[0, 2], triangles=[[1, 1, 0]])}),
}


def literal_triangles(case: dict) -> np.ndarray:
    return np.asarray(case["triangles"], dtype=np.int32).reshape(-1, 3)


def random_mesh(seed: int, num_vertices: int, num_triangles: int, invalid: float = 0.02) -> np.ndarray:
    """int32 [T, 3]: sparse random triangles — local ones (indices close together, so that components stay many and of many
    sizes), a few long-range ones, a few with an index outside [0, V) and a few with a repeated index"""
    rng = np.random.default_rng(seed)
    v, t = int(num_vertices), int(num_triangles)
    base = rng.integers(0, v, size=(t, 1))
    tri = (base + rng.integers(0, 4, size=(t, 3))) % v
    far = rng.uniform(size=t) < 0.03
    tri[far, 2] = rng.integers(0, v, size=int(far.sum()))
    rep = rng.uniform(size=t) < 0.05
    tri[rep, 1] = tri[rep, 0]
    bad = np.flatnonzero(rng.uniform(size=t) < invalid)
    tri[bad, rng.integers(0, 3, size=len(bad))] = rng.choice([-1, v, v + 7, -2 ** 31], size=len(bad))
    return tri.astype(np.int32)
