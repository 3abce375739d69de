"""Test-side yardstick of the neighbour search and what is built on it (tn_knn, tn_pointcloud_normals,
remove_statistical_outliers): a numpy restatement of the definitions in include/thermonerf_hip.h — brute force over all pairs
with explicit float32 steps, ``lexsort`` on (index, d2), the outlier rule in fp64, a 3 x 3 ``eigh`` in fp64 for the normals — and
the analytic clouds the tests share.  Test code, not product."""
from __future__ import annotations

import numpy as np

F = np.float32
INF = float("inf")


def finite_rows(positions) -> np.ndarray:
    return np.isfinite(np.asarray(positions, dtype=F)).all(axis=1)


def knn(positions, k: int) -> dict:
    """index int32 [N,k], d2 float32 [N,k], mean_distance float64 [N] of the definition: O(N^2), one row at a time"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    index = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), INF, dtype=F)
    mean = np.full((n,), INF, dtype=np.float64)
    finite = finite_rows(p)
    others = np.nonzero(finite)[0]
    q = p[others]
    for i in others:
        with np.errstate(over="ignore", under="ignore"):
            dx, dy, dz = (p[i, 0] - q[:, 0]).astype(F), (p[i, 1] - q[:, 1]).astype(F), (p[i, 2] - q[:, 2]).astype(F)
            d = (((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
        rest = others != i
        cand, dist = others[rest], d[rest]
        order = np.lexsort((cand, dist))[:k]  # by d2, then by index
        m = len(order)
        index[i, :m], d2[i, :m] = cand[order], dist[order]
        if m == k:
            s = np.float64(0.0)
            for v in d2[i]:  # in row order, from 0
                s = s + np.sqrt(np.float64(v))
            mean[i] = s / np.float64(k)
    return dict(index=index, d2=d2, mean_distance=mean)


def outlier_threshold(mean_distance, std_ratio: float):
    """(mu, sigma, tau) over the finite entries, fp64, the n - 1 form"""
    m = np.asarray(mean_distance, dtype=np.float64)
    m = m[np.isfinite(m)]
    mu = m.mean()
    sigma = np.sqrt(((m - mu) ** 2).sum() / (len(m) - 1)) if len(m) > 1 else 0.0
    return mu, sigma, mu + float(std_ratio) * sigma


def outlier_keep(positions, nb_neighbors: int = 20, std_ratio: float = 10.0, mean_distance=None) -> np.ndarray:
    """bool [N]: the keep mask of remove_statistical_outliers"""
    finite = finite_rows(positions)
    if finite.sum() < nb_neighbors:
        return finite
    m = knn(positions, nb_neighbors - 1)["mean_distance"] if mean_distance is None else np.asarray(mean_distance)
    return m < outlier_threshold(m, std_ratio)[2]


def covariance(positions, row, i):
    """(centroid, 3 x 3 covariance sum) of point i and the valid entries of its row: fp64, summed from 0 in that order"""
    p = np.asarray(positions, dtype=F)
    members = [i] + [int(j) for j in row if 0 <= j < p.shape[0]]
    q = p[members].astype(np.float64)
    s = np.zeros(3)
    for v in q:
        s = s + v
    c = s / np.float64(len(members))
    cov = np.zeros((3, 3))
    for v in q:
        d = v - c
        cov = cov + np.outer(d, d)
    return c, cov, len(members) - 1


def normals(positions, index, viewpoints=None) -> dict:
    """normals float32 [N,3] of the definition, with gap [N] = (l1 - l0) / l2 of the covariance's ascending eigenvalues (inf
    where no normal is defined) and s [N] = the orientation sum (0 without a usable viewpoint)"""
    p = np.asarray(positions, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    out = np.zeros((n, 3), dtype=F)
    gap, sign = np.full(n, INF), np.zeros(n)
    finite = finite_rows(p)
    for i in range(n):
        if not finite[i]:
            continue
        _, cov, valid = covariance(p, index[i], i)
        if valid < 2:
            continue
        w, v = np.linalg.eigh(cov)
        nv = v[:, 0] / np.linalg.norm(v[:, 0])
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        s = 0.0
        if viewpoints is not None and np.isfinite(viewpoints[i]).all():
            s = float(np.dot(nv, np.asarray(viewpoints[i], dtype=np.float64) - p[i].astype(np.float64)))
        if s < 0 or (s == 0 and nv[int(np.argmax(np.abs(nv)))] < 0):  # argmax: the lowest index on a tie
            nv = -nv
        sign[i] = abs(s)
        out[i] = nv.astype(F)
    return dict(normals=out, gap=gap, s=sign)


# ---- the clouds ------------------------------------------------------------------------------------------------------------------
def sphere_cloud(num_surface: int = 1500, num_outliers: int = 9, seed: int = 7, radius: float = 0.3, noise: float = 0.004) -> dict:
    """``num_surface`` points on a sphere with relative radial noise and ``num_outliers`` points uniform in +-1 at least 0.15 from
    the sphere, inserted at random rows.  positions float32 [N,3], outlier bool [N]."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(num_surface, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    surface = d * (radius * (1.0 + noise * rng.normal(size=(num_surface, 1))))
    far = []
    while len(far) < num_outliers:
        c = rng.uniform(-1.0, 1.0, 3)
        if abs(np.linalg.norm(c) - radius) >= 0.15:
            far.append(c)
    n = num_surface + num_outliers
    rows = np.sort(rng.choice(n, num_outliers, replace=False))
    outlier = np.zeros(n, dtype=bool)
    outlier[rows] = True
    positions = np.empty((n, 3), dtype=F)
    positions[outlier] = np.asarray(far, dtype=F).reshape(-1, 3)
    positions[~outlier] = surface.astype(F)
    return dict(positions=positions, outlier=outlier)


def lattice_cloud(side: int = 6, spacing: float = 0.25, duplicates: int = 0, seed: int = 3) -> np.ndarray:
    """a ``side``^3 lattice (every row of its neighbour lists has tied distances), optionally with exact duplicates appended"""
    g = np.arange(side, dtype=F) * F(spacing)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F)
    if duplicates:
        rng = np.random.default_rng(seed)
        p = np.concatenate([p, p[rng.choice(len(p), duplicates, replace=False)]])
    return p


def two_clusters(big: int = 40, small: int = 5, separation: float = 1.9, spread: float = 0.01, seed: int = 5) -> np.ndarray:
    """two tight clusters ``separation`` apart along x: a point of the small one finds most of its neighbours across empty space"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, spread, (big, 3))
    b = rng.normal(0.0, spread, (small, 3)) + np.array([separation, 0.0, 0.0])
    return np.concatenate([a, b]).astype(F)


def angle_to_radial_deg(positions, normal_vectors) -> np.ndarray:
    p = np.asarray(positions, dtype=np.float64)
    r = p / np.linalg.norm(p, axis=1, keepdims=True)
    c = np.abs((r * np.asarray(normal_vectors, dtype=np.float64)).sum(axis=1))
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))
