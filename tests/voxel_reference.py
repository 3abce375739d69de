"""The device sort and the voxel down-sampling restated in plain numpy with explicit dtypes — what tn_sort_pairs and
tn_voxel_downsample (include/thermonerf_hip.h) must give, byte for byte.

Sort: the pairs in ascending order of the keys' low 8 * ceil(key_bits / 8) bits, equal ones in input order — numpy's stable argsort
of the masked keys.

Voxels: inv = 1.0 / float64(float32(voxel_size)); u_a = (float64(p_a) - float64(origin_a)) * inv; a point is a member iff its
coordinates are finite and 0 <= u_a < float64(dims_a) on every axis; c_a = int64(u_a); key = (c_z dims_y + c_y) dims_x + c_x; a
voxel = the members with one key in ascending point index; voxels in ascending key.  Position and temperature: the float64 sum
from 0 in that order, divided by float64(n), rounded once to float32.  Colours: per channel the integer sum S, then
(2 S + n) // (2 n).  source: the first member's.  voxel_count: n."""
import numpy as np

F32, F64 = np.float32, np.float64


def ordering_mask(key_bits):
    bits = 8 * ((int(key_bits) + 7) // 8)
    return np.uint64((1 << bits) - 1)


def sort_pairs(keys, values, key_bits):
    """(keys, values) as tn_sort_pairs leaves them; values None stands for 0 .. n-1"""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.argsort(keys & ordering_mask(key_bits), kind="stable")
    vals = order.astype(np.int32) if values is None else np.asarray(values, dtype=np.int32)[order]
    return keys[order], vals


def grid_of(positions, voxel_size):
    """(origin float32 [3], dims int32 [3]) as voxel_downsample derives them: the minimum of the finite points, and the voxel of
    their maximum as the last one.  None without a finite point."""
    p = np.asarray(positions, dtype=F32)
    finite = np.isfinite(p).all(axis=1)
    if not finite.any():
        return None
    lo, hi = p[finite].min(axis=0), p[finite].max(axis=0)
    inv = F64(1.0) / F64(F32(voxel_size))
    u = (hi.astype(F64) - lo.astype(F64)) * inv
    return lo.astype(F32), (u.astype(np.int64) + 1).astype(np.int32)


def voxel_keys(positions, origin, voxel_size, dims):
    """(uint64 key per point — `total` for a dropped point —, total as a Python int)"""
    p = np.asarray(positions, dtype=F32)
    inv = F64(1.0) / F64(F32(voxel_size))
    d = [int(v) for v in dims]
    total = d[0] * d[1] * d[2]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (p.astype(F64) - np.asarray(origin, dtype=F32).astype(F64)[None, :]) * inv
        member = np.isfinite(p).all(axis=1) & (u >= 0.0).all(axis=1) & (u < np.asarray(d, dtype=F64)[None, :]).all(axis=1)
    c = np.where(member[:, None], u, 0.0).astype(np.int64)
    keys = np.full(len(p), total, dtype=object)
    for i in np.nonzero(member)[0]:
        keys[i] = (int(c[i, 2]) * d[1] + int(c[i, 1])) * d[0] + int(c[i, 0])
    return keys.astype(np.uint64), total


def voxel_downsample(positions, colors, temperature, thermal_colors, source, origin, voxel_size, dims):
    """dict of positions float32 [V,3], colors uint8 [V,3], temperature float32 [V], thermal_colors uint8 [V,3] or None, source
    int64 [V] or None, voxel_count int32 [V], members (the number of points that fell in the grid)"""
    p = np.asarray(positions, dtype=F32)
    keys, total = voxel_keys(p, origin, voxel_size, dims)
    order = np.argsort(keys, kind="stable")
    order = order[keys[order] < np.uint64(total)]  # (total <= 2^63)
    sorted_keys = keys[order]
    starts = np.nonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))[0] if len(order) else np.zeros(0, dtype=np.int64)
    ends = np.concatenate([starts[1:], [len(order)]]) if len(order) else starts
    v = len(starts)
    out = {"positions": np.zeros((v, 3), F32), "colors": np.zeros((v, 3), np.uint8), "temperature": np.zeros(v, F32),
           "thermal_colors": None if thermal_colors is None else np.zeros((v, 3), np.uint8),
           "source": None if source is None else np.zeros(v, np.int64), "voxel_count": np.zeros(v, np.int32),
           "members": int(len(order))}
    for k, (a, b) in enumerate(zip(starts, ends)):
        rows = order[a:b]  # ascending point index
        n = len(rows)
        s = [F64(0.0)] * 4
        for i in rows:
            for c in range(3):
                s[c] = s[c] + F64(p[i, c])
            s[3] = s[3] + F64(temperature[i])
        with np.errstate(over="ignore"):
            out["positions"][k] = [F32(s[c] / F64(n)) for c in range(3)]
            out["temperature"][k] = F32(s[3] / F64(n))
        out["colors"][k] = rounded_mean(colors[rows], n)
        if thermal_colors is not None:
            out["thermal_colors"][k] = rounded_mean(thermal_colors[rows], n)
        if source is not None:
            out["source"][k] = source[rows[0]]
        out["voxel_count"][k] = n
    return out


def rounded_mean(rows, n):
    """uint8 [3]: per channel (2 S + n) // (2 n) of the exact integer sum S — round half up"""
    s = np.asarray(rows, dtype=np.uint8).astype(np.int64).sum(axis=0)
    return ((2 * s + n) // (2 * n)).astype(np.uint8)


def lattice(side=6, step=0.25, seed=5):
    """side^3 points at integer multiples of ``step`` (a power of two: every coordinate step is exact), shuffled, with random
    colours, temperatures and sources: (positions, colors, temperature, thermal_colors, source)"""
    rng = np.random.default_rng(seed)
    g = np.arange(side, dtype=F64) * step - 0.5
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    p = p[rng.permutation(len(p))]
    return (p,) + attributes(len(p), rng)


def attributes(n, rng):
    return (rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.uniform(14.0, 33.0, n).astype(F32),
            rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.permutation(n).astype(np.int64) * 3)
