"""Test-side yardstick of tn_mesh_incidence / tn_mesh_vertex_normals / tn_mesh_smooth: a numpy restatement of the definitions in
include/thermonerf_hip.h in float32, one rounding per operation, every vertex's loop in the order of its list.  The loops run as
ROUNDS — round k handles the k-th corner of every list that has one, all those vertices at once — which is the same sequence of
operations per vertex.  numpy's float32 `/` and sqrt are correctly rounded.  Test code, not product."""
from __future__ import annotations

import numpy as np

from tests.mesh_components_reference import valid_mask

F = np.float32


def corner_keys(triangles, num_vertices: int) -> np.ndarray:
    """int64 [3T]: the vertex corner c names if its triangle is valid, else V"""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return np.where(valid_mask(tri, num_vertices)[:, None], tri, int(num_vertices)).reshape(-1)


def incidence(triangles, num_vertices: int) -> dict:
    """offsets int32 [V + 1], corners int32 [3T] (None with V == 0 or T == 0: the entry leaves them untouched)"""
    v = int(num_vertices)
    keys = corner_keys(triangles, v)
    if v == 0 or len(keys) == 0:
        return dict(offsets=np.zeros(v + 1, np.int32), corners=None)
    order = np.argsort(keys, kind="stable")
    return dict(offsets=np.searchsorted(keys[order], np.arange(v + 1), side="left").astype(np.int32), corners=order.astype(np.int32))


def brute_force_lists(triangles, num_vertices: int) -> list:
    """the list of every vertex straight from the definition: the corners that name it, ascending, of valid triangles only"""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    valid, flat = valid_mask(tri, num_vertices), tri.reshape(-1)
    return [[c for c in range(len(flat)) if valid[c // 3] and flat[c] == v] for v in range(int(num_vertices))]


def _rounds(offsets, corners):
    """yields (vertices, their k-th corners) for k = 0, 1, ...: every list walked in its own order"""
    offsets = np.asarray(offsets, dtype=np.int64)
    begin, length = offsets[:-1], np.diff(offsets)
    for k in range(int(length.max()) if len(length) else 0):
        vs = np.flatnonzero(length > k)
        yield vs, np.asarray(corners, dtype=np.int64)[begin[vs] + k]


def face_vectors(positions, triangles) -> np.ndarray:
    """float32 [T,3]: e1 x e2 per triangle in the header's operation order (rows of invalid triangles are zero and never used)"""
    pos = np.asarray(positions, dtype=F).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = valid_mask(tri, len(pos))
    t = np.where(ok[:, None], tri, 0)
    p0, p1, p2 = pos[t[:, 0]], pos[t[:, 1]], pos[t[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = (p1 - p0).astype(F), (p2 - p0).astype(F)
        f = np.stack([((e1[:, 1] * e2[:, 2]).astype(F) - (e1[:, 2] * e2[:, 1]).astype(F)).astype(F),
                      ((e1[:, 2] * e2[:, 0]).astype(F) - (e1[:, 0] * e2[:, 2]).astype(F)).astype(F),
                      ((e1[:, 0] * e2[:, 1]).astype(F) - (e1[:, 1] * e2[:, 0]).astype(F)).astype(F)], axis=1)
    return np.where(ok[:, None], f, F(0.0)).astype(F)


def vertex_normals(positions, triangles, index: dict) -> np.ndarray:
    pos = np.asarray(positions, dtype=F).reshape(-1, 3)
    v = len(pos)
    s = np.zeros((v, 3), F)
    if index["corners"] is not None:
        f = face_vectors(pos, triangles)
        with np.errstate(all="ignore"):
            for vs, cs in _rounds(index["offsets"], index["corners"]):
                s[vs] = (s[vs] + f[cs // 3]).astype(F)
    with np.errstate(all="ignore"):
        length = np.sqrt((((s[:, 0] * s[:, 0]).astype(F) + (s[:, 1] * s[:, 1]).astype(F)).astype(F) + (s[:, 2] * s[:, 2]).astype(F)).astype(F))
        unit = (length > 0) & (length < F(np.inf))
        n = (s / np.where(unit, length, F(1.0))[:, None]).astype(F)
    return np.where(unit[:, None], n, F(0.0)).astype(F)


def smooth_pass(src, triangles, index: dict, k) -> np.ndarray:
    """one Jacobi pass with factor k: a new array"""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    v = len(src)
    s, n = np.zeros((v, 3), F), np.zeros(v, np.int64)
    with np.errstate(all="ignore"):
        if index["corners"] is not None:
            for vs, cs in _rounds(index["offsets"], index["corners"]):
                t, j = cs // 3, cs % 3
                q, r = src[tri[t, (j + 1) % 3]], src[tri[t, (j + 2) % 3]]
                s[vs] = ((s[vs] + q).astype(F) + r).astype(F)
                n[vs] += 2
        moved = n > 0
        m = (s / np.where(moved, n, 1).astype(F)[:, None]).astype(F)
        dst = (src + (F(k) * (m - src).astype(F)).astype(F)).astype(F)
    return np.where(moved[:, None], dst, src).astype(F)


def smooth(positions, triangles, index: dict, iterations: int, lambda_, mu) -> np.ndarray:
    """the raw interface of tn_mesh_smooth: any pair of factors, a pass with ``lambda_`` then a pass with ``mu`` per iteration"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3).copy()
    for _ in range(int(iterations)):
        p = smooth_pass(smooth_pass(p, triangles, index, lambda_), triangles, index, mu)
    return p


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- literal cases, every array written out by hand ------------------------------------------------------------------------------
# floats as bit patterns: 0x3F800000 = 1, 0xBF800000 = -1, 0x3F000000 = 0.5, 0x3FC00000 = 1.5, 0x40000000 = 2, 0xBF13CD3A = -1 / fp32(sqrt 3)
# (div(-1, 0x3FDDB3D7) = -0.5773502588...), 0x3E2AAAAB = 0.5 * fp32(1 / 3) = 0.5 * div(2, 6).  `pass_half`: one pass with k = 0.5.
_Z, _ONE, _MONE, _HALF, _THIRD_HALF, _N3 = 0, 0x3F800000, 0xBF800000, 0x3F000000, 0x3E2AAAAB, 0xBF13CD3A
LITERAL = {
    # the unit tetrahedron wound outward: face vectors (0,0,-1), (0,-1,0), (-1,0,0), (1,1,1)
    "tetrahedron": dict(
        positions=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], triangles=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]],
        offsets=[0, 3, 6, 9, 12], corners=[0, 3, 6, 2, 4, 9, 1, 8, 10, 5, 7, 11],
        normals=[[_N3, _N3, _N3], [_ONE, _Z, _Z], [_Z, _ONE, _Z], [_Z, _Z, _ONE]],
        pass_half=[[_THIRD_HALF] * 3, [_HALF, _THIRD_HALF, _THIRD_HALF], [_THIRD_HALF, _HALF, _THIRD_HALF],
                   [_THIRD_HALF, _THIRD_HALF, _HALF]]),
    # face vector (0,0,4); a corner's partners are the other two vertices, n = 2
    "single_triangle": dict(
        positions=[[0, 0, 0], [2, 0, 0], [0, 2, 0]], triangles=[[0, 1, 2]], offsets=[0, 1, 2, 3], corners=[0, 1, 2],
        normals=[[_Z, _Z, _ONE]] * 3, pass_half=[[_HALF, _HALF, _Z], [_ONE, _HALF, _Z], [_HALF, _ONE, _Z]]),
    # (0,1,1) is valid and listed once per corner: vertex 1 has two corners, n = 4; its face vector is exactly 0; vertex 2 is in no
    # triangle and stays where it is
    "repeated_index": dict(
        positions=[[0, 0, 0], [2, 0, 0], [0, 2, 0]], triangles=[[0, 1, 1]], offsets=[0, 1, 3, 3], corners=[0, 1, 2],
        normals=[[_Z, _Z, _Z]] * 3, pass_half=[[_ONE, _Z, _Z], [0x3FC00000, _Z, _Z], [_Z, 0x40000000, _Z]]),
    # the first triangle names vertex 3 of three: its corners 0 1 2 get the key V and sort behind every list
    "index_beyond_the_vertices": dict(
        positions=[[0, 0, 0], [2, 0, 0], [0, 2, 0]], triangles=[[0, 3, 1], [0, 1, 2]], offsets=[0, 1, 2, 3], corners=[3, 4, 5, 0, 1, 2],
        normals=[[_Z, _Z, _ONE]] * 3, pass_half=[[_HALF, _HALF, _Z], [_ONE, _HALF, _Z], [_HALF, _ONE, _Z]]),
}


def literal_arrays(case: dict):
    """(positions float32 [V,3], triangles int32 [T,3])"""
    return np.asarray(case["positions"], dtype=F).reshape(-1, 3), np.asarray(case["triangles"], dtype=np.int32).reshape(-1, 3)


# ---- shapes the GPU tests share ---------------------------------------------------------------------------------------------------
def random_positions(seed: int, num_vertices: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(int(num_vertices), 3)).astype(F)


def fan(num_triangles: int) -> np.ndarray:
    """``num_triangles`` triangles around vertex 0 (an open fan over T + 2 vertices): the long list"""
    i = np.arange(int(num_triangles), dtype=np.int32)
    return np.stack([np.zeros_like(i), i + 1, i + 2], axis=1)


def strip(num_vertices: int) -> np.ndarray:
    """a triangle strip, wound alternately so that every face vector points the same way"""
    i = np.arange(int(num_vertices) - 2, dtype=np.int32)
    return np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], axis=1), np.stack([i + 1, i, i + 2], axis=1)).astype(np.int32)


def radial_angles_deg(positions, normals) -> np.ndarray:
    """the angle between each normal and the direction from the origin to its vertex, in degrees (fp64)"""
    p, n = np.asarray(positions, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    cos = (p * n).sum(axis=1) / (np.linalg.norm(p, axis=1) * np.linalg.norm(n, axis=1))
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
