"""The yardstick of the registration: include/thermonerf_hip.h's definition of ``tn_mesh_register`` in plain numpy fp64 — every point
against every face with no tree (``mesh_closest_reference._pairs`` from the TRANSFORMED fp64 point), one add, sub, mul, div or sqrt
per step; the wave's tree as six rounds of ``x[..., 0::2] + x[..., 1::2]``, the runs of 256 as sequential loops, the solve and the
update scalar by scalar in Python floats (IEEE doubles, one rounding per operation, nothing fused)."""
from __future__ import annotations

import math

import numpy as np

from tests.mesh_closest_reference import _cross, _dot, _pairs, _scene, plane_grid  # noqa: F401
from tests.mesh_raycast_reference import box_mesh

F, D = np.float32, np.float64
POINT, PLANE = 0, 1
CONVERGED, ITERATIONS, TOO_FEW, DEGENERATE = 0, 1, 2, 3
STATUS = ("converged", "iterations", "too_few", "degenerate")
NOT_RUN = -1.0
WORDS, RUN, LANES = 40, 256, 64
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], D)


def workspace_bytes(n):
    return 64 + 8 * WORDS * ((n + LANES - 1) // LANES)


def transformed(transform, points):
    """x [N, 3] fp64 and which points are usable"""
    m = np.asarray(transform, D).reshape(3, 4)
    p = np.asarray(points, F).reshape(-1, 3).astype(D)
    with np.errstate(all="ignore"):
        x = np.stack([((m[k, 0] * p[:, 0] + m[k, 1] * p[:, 1]) + m[k, 2] * p[:, 2]) + m[k, 3] for k in range(3)], axis=1)
    good = np.isfinite(np.asarray(points, F).reshape(-1, 3)).all(axis=1) & np.isfinite(x).all(axis=1)
    return x, good


def correspond(scene, x, good, r2, chunk=256):
    """the winner of every usable point among the usable faces with d2 <= r2: (face int32 [N], -1 without one; C fp64 [N, 3])"""
    positions, temperature, tri, usable, _, xp, arr, p, lo, hi = scene
    n = len(x)
    face, c = np.full(n, -1, np.int32), np.zeros((n, 3), D)
    with np.errstate(all="ignore"):
        for first in range(0, n if len(tri) else 0, chunk):
            rows = slice(first, min(first + chunk, n))
            safe = np.where(good[rows, None], x[rows], 0.0)
            found = _pairs(np, [safe[:, k:k + 1] for k in range(3)], p[0], p[1], p[2], lo, hi)
            ok = usable[None, :] & good[rows, None] & (found.d2 <= r2)
            masked = np.where(ok, found.d2, np.inf)
            first_of = np.argmax(ok & (masked == masked.min(axis=1, keepdims=True)), axis=1)
            some = ok.any(axis=1)
            pick = (np.arange(len(first_of)), first_of)
            face[rows] = np.where(some, first_of, -1)
            c[rows] = np.where(some[:, None], np.stack([np.broadcast_to(v, found.d2.shape)[pick] for v in found.c], axis=1), 0.0)
    return face, c


def point_sums(scene, x, face, c, center, metric):
    """the 36 numbers of every point [N, 36], which points are matched, which have a winner without a normal"""
    positions, tri = scene[0], scene[2]
    n = len(x)
    found = face >= 0
    y = [x[:, k] - center[k] for k in range(3)]
    e = [x[:, k] - c[:, k] for k in range(3)]
    flat = np.zeros(n, bool)
    if metric == PLANE:
        corner = positions[tri[np.where(found, face, 0)].astype(np.int64)].astype(D) if len(tri) and len(positions) else np.zeros((n, 3, 3), D)
        e1, e2 = [corner[:, 1, k] - corner[:, 0, k] for k in range(3)], [corner[:, 2, k] - corner[:, 0, k] for k in range(3)]
        w = _cross(e1, e2)
        nn = _dot(w, w)
        flat = found & (nn == 0.0)
        length = np.sqrt(np.where(nn == 0.0, 1.0, nn))
        normals = [[w[k] / length for k in range(3)]]
    else:
        one, zero = np.ones(n, D), np.zeros(n, D)
        normals = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    matched = found & ~flat
    sums = np.zeros((n, 36), D)
    with np.errstate(all="ignore"):
        for normal in normals:
            g = _cross(y, normal) + list(normal) + [_dot(normal, y)]
            r = _dot(normal, e)
            at = 0
            for i in range(7):
                for j in range(i, 7):
                    sums[:, at] = sums[:, at] + g[i] * g[j]
                    at += 1
            for i in range(7):
                sums[:, 28 + i] = sums[:, 28 + i] + g[i] * r
            sums[:, 35] = sums[:, 35] + r * r
    sums[~matched] = 0.0
    return sums, matched, flat


def wave_partials(sums, matched, good, flat):
    """[W, 40]: the adjacent-pair tree over each wave's 64 lanes, then the three counts and +0.0"""
    n = len(sums)
    waves = (n + LANES - 1) // LANES
    padded = np.zeros((waves * LANES, 36), D)
    padded[:n] = sums
    x = padded.reshape(waves, LANES, 36).transpose(0, 2, 1)
    with np.errstate(all="ignore"):
        for _ in range(6):
            x = x[..., 0::2] + x[..., 1::2]
    out = np.zeros((waves, WORDS), D)
    out[:, :36] = x[..., 0]
    for k, flags in ((36, matched), (37, good), (38, flat)):
        lanes = np.zeros(waves * LANES, D)
        lanes[:n] = flags
        out[:, k] = lanes.reshape(waves, LANES).sum(axis=1)
    return out


def totals(partials):
    """SUM2 with runs of 256 waves: sequential within a run, then over the runs"""
    with np.errstate(all="ignore"):
        runs = [np.cumsum(np.concatenate([np.zeros((1, WORDS), D), partials[first:first + RUN]]), axis=0)[-1]
                for first in range(0, len(partials), RUN)]
        total = np.zeros(WORDS, D)
        for run in runs:
            total = total + run
    return total


def solve(total, k, damping, length):
    """delta (7 floats) of the damped system, or None: DEGENERATE"""
    s = [[0.0] * 7 for _ in range(7)]
    at = 0
    for i in range(7):
        for j in range(i, 7):
            s[i][j] = s[j][i] = float(total[at])
            at += 1
    b = [float(v) for v in total[28:35]]
    m = float(total[36])
    lam, l2 = damping * m, length * length
    diag = [s[i][i] + lam * (1.0 if 3 <= i < 6 else l2) for i in range(7)]
    low = [[0.0] * 7 for _ in range(7)]
    d = [0.0] * 7
    for j in range(k):
        dj = diag[j]
        for p in range(j):
            dj = dj - low[j][p] * (low[j][p] * d[p])
        if not dj > 0.0 or not math.isfinite(dj):
            return None
        d[j] = dj
        for i in range(j + 1, k):
            v = s[j][i]
            for p in range(j):
                v = v - low[i][p] * (low[j][p] * d[p])
            low[i][j] = v / dj
    z = [0.0] * 7
    for i in range(k):
        v = -b[i]
        for p in range(i):
            v = v - low[i][p] * z[p]
        z[i] = v
    for i in range(k):
        z[i] = z[i] / d[i]
    delta = [0.0] * 7
    bad = False
    for i in range(k - 1, -1, -1):
        v = z[i]
        for p in range(i + 1, k):
            v = v - low[p][i] * delta[p]
        delta[i] = v
        bad = bad or not math.isfinite(v)
    return None if bad else delta


def update(transform, delta, center):
    """the Cayley update: the new 12 numbers"""
    m = [float(v) for v in transform]
    a = [0.5 * delta[0], 0.5 * delta[1], 0.5 * delta[2]]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    f = 2.0 / (1.0 + aa)
    scale = 1.0 + delta[6]
    skew = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    u = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            k2 = a[i] * a[i] - aa if i == j else a[i] * a[j]
            u[i][j] = scale * ((1.0 if i == j else 0.0) + f * (skew[i][j] + k2))
    t = [m[4 * j + 3] - center[j] for j in range(3)]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (u[i][0] * m[j] + u[i][1] * m[4 + j]) + u[i][2] * m[8 + j]
        out[4 * i + 3] = (center[i] + ((u[i][0] * t[0] + u[i][1] * t[1]) + u[i][2] * t[2])) + delta[3 + i]
    return np.array(out, D)


def iteration_sums(scene, transform, points, max_distance, center, metric):
    """one iteration up to the wave partials: (partials [W, 40], per-point dict for the tests)"""
    x, good = transformed(transform, points)
    r2 = float(D(max_distance) * D(max_distance))
    face, c = correspond(scene, x, good, r2)
    sums, matched, flat = point_sums(scene, x, face, c, center, metric)
    return wave_partials(sums, matched, good, flat), {"x": x, "good": good, "face": face, "c": c, "sums": sums, "matched": matched, "flat": flat}


def register(positions, temperature, triangles, points, *, max_distance=math.inf, center=(0.0, 0.0, 0.0), length=1.0, damping=0.0,
             tolerance=0.0, iterations=1, metric=PLANE, with_scale=False, min_pairs=1, transform=None):
    """The definition.  A dict of ``transform`` float64 [12], ``history`` float64 [iterations, 4], ``result`` int64 [4], ``partials``
    float64 [W, 40] of the last iteration that ran, and ``deltas``: the accepted steps."""
    scene = _scene(positions, temperature, triangles, None)
    points = np.asarray(points, F).reshape(-1, 3)
    transform = IDENTITY.copy() if transform is None else np.array(transform, D).reshape(12).copy()
    center = [float(v) for v in center]
    history = np.full((iterations, 4), NOT_RUN, D)
    result = np.zeros(4, np.int64)
    partials, deltas = None, []
    k = 7 if with_scale else 6
    for it in range(iterations):
        partials, _ = iteration_sums(scene, transform, points, max_distance, center, metric)
        total = totals(partials)
        m = float(total[36])
        status, delta = ITERATIONS, None
        if m < min_pairs:
            status = TOO_FEW
        else:
            with np.errstate(all="ignore"):
                delta = solve(total, k, float(damping), float(length))
            if delta is None:
                status = DEGENERATE
        history[it, :2] = (m, total[35])
        if delta is not None:
            transform = update(transform, delta, center)
            deltas.append(delta)
            turn = max(abs(delta[0]), abs(delta[1]), abs(delta[2]), abs(delta[6]))
            shift = max(abs(delta[3]), abs(delta[4]), abs(delta[5])) / float(length)
            history[it, 2:] = (turn, shift)
            if turn <= tolerance and shift <= tolerance:
                status = CONVERGED
        result[:] = (status, it + 1, int(m), int(total[37]))
        if status != ITERATIONS:
            break
    return {"transform": transform, "history": history, "result": result, "partials": partials, "deltas": deltas}


# ---- scenes and known transforms ----------------------------------------------------------------------------------------------------------

def l_boxes():
    """two boxes that form an L, 192 + 48 = 240 faces: no direction slides, no axis turns freely: (positions, temperature, triangles)"""
    a_pos, a_tri = box_mesh((0.0, 0.0, 0.0), (2.0, 1.0, 0.75), 4)
    b_pos, b_tri = box_mesh((0.0, 1.0, 0.0), (0.5, 2.5, 1.25), 2)
    positions = np.concatenate([a_pos, b_pos]).astype(F)
    triangles = np.concatenate([a_tri, b_tri + len(a_pos)]).astype(np.int32)
    return positions, (20.0 + positions[:, 0].astype(D)).astype(F), triangles


def surface_points(positions, triangles, count, seed):
    """``count`` points on the faces (uniform barycentrics, area-blind), fp64"""
    rng = np.random.default_rng(seed)
    tri = np.asarray(triangles, np.int64)
    f = rng.integers(0, len(tri), count)
    w = rng.dirichlet((1.0, 1.0, 1.0), count)
    return (np.asarray(positions, D)[tri[f]] * w[:, :, None]).sum(axis=1)


def similarity(rotation_vector, translation, scale=1.0, center=(0.0, 0.0, 0.0)):
    """the 4 x 4 of x -> center + scale R (x - center) + translation, R from the rotation vector (Rodrigues, host libm: a test input)"""
    w = np.asarray(rotation_vector, D)
    angle = float(np.linalg.norm(w))
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], D) / (angle if angle else 1.0)
    r = np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)
    c = np.asarray(center, D)
    out = np.eye(4)
    out[:3, :3] = scale * r
    out[:3, 3] = c - scale * r @ c + np.asarray(translation, D)
    return out


def moved_cloud(points, matrix):
    """the cloud whose registration is ``matrix``: the inverse applied in fp64, rounded to fp32 — with the exact pre-images, so the
    recovered matrix is compared with ``matrix`` up to that rounding"""
    inverse = np.linalg.inv(matrix)
    return (np.asarray(points, D) @ inverse[:3, :3].T + inverse[:3, 3]).astype(F)


def box_of(positions):
    """centre and diagonal of the finite positions' box, as the Python layer's default"""
    p = np.asarray(positions, D).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return tuple(float(v) for v in (lo + hi) / 2), float(np.linalg.norm(hi - lo))
