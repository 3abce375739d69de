"""fp64 reference of the position gradient (d loss / d sample position through the hash encoding and the position
normalisation), of the encoding's forward features and of the per-ray adjoint of the sample positions — numpy / torch, no device.

Why "frozen cell".  The kernels form the scaled coordinate ``sx = fl32(p * s)`` in fp32 and take the cell (floor, ceil) and the
interpolation offset ``sx - floor(sx)`` (exact in fp32) from it.  A plain fp64 run of the oracle forms ``p * s`` exactly: a few
samples in 1e4 land in another cell, and where they do not, the offset — the INPUT of the trilinear polynomial — differs by up to
half an ulp of ``sx``, which moves the gradient by ~1e-4 of its scale.  The reference therefore freezes the cell and the offsets at
their fp32 values and evaluates the polynomial's derivative in fp64: what is left between it and a kernel is the kernel's own
rounding.

The corner convention is torch's (NS HashEncoding.pytorch_fwd): ceil and floor of ``sx``.  On a grid plane they coincide, both
corners of the axis read the same entry, and the slope along that axis is exactly 0.

What scales the tolerance.  Every function returns, next to its value ``g``, a bound ``B``: the same expression with every table
entry, every ``d_enc`` entry and every factor of the chain replaced by its absolute value.  A rounding error of an fp32 evaluation
is proportional to B, not to |g|: the gradient is a sum over 16 levels of feature DIFFERENCES times scales up to 2047, and it
cancels (median B / |g| is about 8, the worst samples reach 1e4).  A test that compared against |g| would fail on the
cancellation, not on an error; the tests compare ``|got - want| <= K * 2^-24 * B`` with K the number of roundings on the longest
path of the form under test.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import hotpath as H

EPS32 = 2.0 ** -24
_P1, _P2 = 2654435761, 805459861
# corners in the f0 .. f7 order of NS HashEncoding.pytorch_fwd: (x, y, z) each the ceil (1) or the floor (0) coordinate
_CORNERS = ((1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0))


class Space(NamedTuple):
    """Position normalisation: the L-inf scene contraction followed by (c + 2) / 4, or the AABB ``[2, 3]`` normalisation."""
    contraction: bool
    aabb: Optional[np.ndarray] = None

    def oracle_args(self):
        aabb = None if self.aabb is None else torch.tensor(np.asarray(self.aabb, dtype=np.float32))
        return H.OracleConfig(disable_scene_contraction=not self.contraction), aabb


UNIT_BOX = Space(False, np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], dtype=np.float32))
CONTRACTION = Space(True, None)


def normalized(x32: np.ndarray, space: Space) -> Tuple[np.ndarray, np.ndarray]:
    """(p32 [n,3] with the selector applied, selector [n] bool) of the fp32 oracle — the values the kernels reproduce bit for bit."""
    cfg, aabb = space.oracle_args()
    p, sel = H.normalized_positions(torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)), cfg, aabb)
    return p.numpy(), sel.numpy()


# ----------------------------------------------------------------------------------------------------------------------
# K: fp32 roundings on the longest path from the inputs to a stored value, counted from the kernels' code.  First order: a
# product of two inexact operands carries the sum of their counts + 1, a sum the larger count + 1; exact operations (x 0.25,
# / 2, x selector, x sign, adding to a zero accumulator, sx - floor(sx)) count 0.
# ----------------------------------------------------------------------------------------------------------------------
# encode_level_grad, one level, the d/d ox path (the longest; q = 1 - o is one rounding where sx < 1):
#   (f1 - f2) 1, qy 1, their product 3, + (f0 - f3) oy 4, x oz 5; the qz half: sum 4, qz 1, product 6; both halves 7;
#   ge x 8, x s 9; the second channel's "gx +=" 10
K_LEVEL = 10
# position_grad_finish, contraction, the tie path: mag^3 2, 2 / it 3, + (-2 / mag^2) 4 = dsm; dot: products 1, two adds 3;
#   dsm x dot 5, / ties 6, "r +=" 7.  (The diagonal path: mag^2 1, 1 / it 2, 2 / mag - it 3, sm x g 4, "r +=" 5.)
#   AABB: mx - mn 1, g / it 2.
K_FINISH = 7
# tn_hash_encode_bwd_input: one lane per level, then log2(LP) shuffle adds (4 for the <16> kernel, 3 for <8>)
K_BWD_INPUT = K_LEVEL + 4 + K_FINISH
# tn_field_bwd_fused recomputing: four levels accumulate in one lane (the first level's value passes 3 more levels x 2 channel
#   adds = 6 more than K_LEVEL counts), then the two shuffle adds over the sample's four lanes
K_FUSED_RECOMPUTE = K_LEVEL + 6 + 2 + K_FINISH
# tn_field_bwd_fused from the forward's Jacobian: hash_blend_jac's slopes interpolate as fmaf(o, a, fmaf(-o, b, b)), two roundings
#   a stage: d / d ox: d03 1, y stage 3, z stage 5; d / d oy: x stage 2, difference 3, z stage 5; d / d oz: x stage 2, y stage 4,
#   difference 5; x s in the forward 6; the backward's fmaf chain of one axis is 4 levels x 2 channels = 8 deep; two shuffle adds
K_FUSED_JACOBIAN = 6 + 8 + 2 + K_FINISH
K_JACOBIAN_TENSOR = 6
# tn_hash_encode_fwd (torch's three-rounding lerp a o + b (1 - o), nested three times): per stage the b side is operand + q 1 +
#   product 1, + the sum 1 = 3 more: 3, 6, 9
K_FEATURES = 9


def frustum_roundings(n: int) -> Tuple[int, int]:
    """(K of d_o, K of d_d) for n samples per ray: s + e 1 and g x t 2 (d_d only); a lane sums ceil(n / 64) terms (the first
    into a zero accumulator), the wave scan adds 6 times, and the result is added to what d_o / d_d held"""
    per_lane = (n + 63) // 64 - 1
    return per_lane + 6 + 1, 2 + per_lane + 6 + 1


# ----------------------------------------------------------------------------------------------------------------------
# the encoding: one level, cell and offsets frozen at their fp32 values
# ----------------------------------------------------------------------------------------------------------------------
def frozen_cell(p32: np.ndarray, scale: float):
    """(floor [n,3] int64, ceil [n,3] int64, offset [n,3] fp64) of ``sx = fl32(p32 * scale)``; the offset is exact."""
    p32 = np.asarray(p32, dtype=np.float32)
    sx = (p32 * np.float32(scale)).astype(np.float32)
    fl, ce = np.floor(sx), np.ceil(sx)
    off = sx.astype(np.float64) - fl.astype(np.float64)
    return fl.astype(np.int64), ce.astype(np.int64), off


def _corner_values(fl, ce, table, level, log2T):
    """the 8 corner entries [8][n, 2] fp64 of one level; ``table`` is the whole [L * T, 2] array"""
    T = 1 << log2T
    tl = np.asarray(table[level * T:(level + 1) * T], dtype=np.float64)
    out = []
    for bx, by, bz in _CORNERS:
        x = (ce if bx else fl)[:, 0]
        y = (ce if by else fl)[:, 1] * _P1
        z = (ce if bz else fl)[:, 2] * _P2
        out.append(tl[(x ^ y ^ z) % T])
    return out


def _pairs(f):
    """the x pairs (ceil, floor) at (y, z) = (c, c), (f, c), (f, f), (c, f):  f0/f3, f1/f2, f5/f6, f4/f7"""
    return (f[0], f[3]), (f[1], f[2]), (f[5], f[6]), (f[4], f[7])


def frozen_features(p32, table, scale, level, log2T):
    """(enc_l [n, 2], B [n, 2]) fp64: the level's trilinear features on the frozen cell and their absolute evaluation."""
    fl, ce, off = frozen_cell(p32, scale)
    f = _corner_values(fl, ce, table, level, log2T)
    ox, oy, oz = (off[:, c:c + 1] for c in range(3))
    out = []
    for g in (f, [np.abs(v) for v in f]):
        (a03, b03), (a12, b12), (a56, b56), (a47, b47) = _pairs(g)
        f03, f12 = a03 * ox + b03 * (1 - ox), a12 * ox + b12 * (1 - ox)
        f56, f47 = a56 * ox + b56 * (1 - ox), a47 * ox + b47 * (1 - ox)
        out.append((f03 * oy + f12 * (1 - oy)) * oz + (f47 * oy + f56 * (1 - oy)) * (1 - oz))
    return out[0], out[1]


def frozen_level_gradient(p32, d_enc_l, table, scale, level, log2T):
    """(g [n, 3], B [n, 3]) fp64: g = d (d_enc_l . enc_l) / d p of one level with the cell and the offsets frozen from the fp32
    product ``fl32(p32 * scale)``; corners = ceil / floor of it (they coincide on a plane: slope exactly 0 along that axis).
    B: every table and d_enc entry replaced by its absolute value (differences become sums), times the scale."""
    fl, ce, off = frozen_cell(p32, scale)
    f = _corner_values(fl, ce, table, level, log2T)
    ox, oy, oz = (off[:, c:c + 1] for c in range(3))
    qx, qy, qz = 1 - ox, 1 - oy, 1 - oz
    d_enc_l = np.asarray(d_enc_l, dtype=np.float64).reshape(-1, 2)

    def slopes(diff):
        # diff(a, b): a - b for the value, |a| + |b| for the bound; on a plane a and b are the SAME entry: a - b == 0 exactly
        (a03, b03), (a12, b12), (a56, b56), (a47, b47) = _pairs(f)
        dox = (diff(a03, b03) * oy + diff(a12, b12) * qy) * oz + (diff(a47, b47) * oy + diff(a56, b56) * qy) * qz
        v = (lambda t: t) if diff is _sub else np.abs
        f03, f12 = v(a03) * ox + v(b03) * qx, v(a12) * ox + v(b12) * qx
        f47, f56 = v(a47) * ox + v(b47) * qx, v(a56) * ox + v(b56) * qx
        doy = diff(f03, f12) * oz + diff(f47, f56) * qz
        doz = diff(f03 * oy + f12 * qy, f47 * oy + f56 * qy)
        return dox, doy, doz

    g = np.stack([(d_enc_l * s).sum(axis=1) for s in slopes(_sub)], axis=1) * float(scale)
    B = np.stack([(np.abs(d_enc_l) * s).sum(axis=1) for s in slopes(_abs_sum)], axis=1) * float(scale)
    # an axis whose ceil and floor corners coincide carries no slope: exactly 0, whatever the summation above left
    flat = fl == ce
    g[flat] = 0.0
    return g, B


def _sub(a, b):
    return a - b


def _abs_sum(a, b):
    return np.abs(a) + np.abs(b)


def frozen_gradient(p32, d_enc, table, scalings: Sequence[float], log2T):
    """sum of frozen_level_gradient over the levels; d_enc [n, 2 L]"""
    d_enc = np.asarray(d_enc, dtype=np.float64)
    g = np.zeros((len(p32), 3))
    B = np.zeros((len(p32), 3))
    for l, s in enumerate(scalings):
        gl, Bl = frozen_level_gradient(p32, d_enc[:, 2 * l:2 * l + 2], table, s, l, log2T)
        g += gl
        B += Bl
    return g, B


# ----------------------------------------------------------------------------------------------------------------------
# from the normalised position back to the world position
# ----------------------------------------------------------------------------------------------------------------------
def position_chain_gradient(x32, g_p, B_p, space: Space):
    """(g_x [n, 3], B_x [n, 3]) fp64: ``g_p`` = d loss / d p pushed back through ``p * selector``, then (c + 2) / 4 and the L-inf
    contraction, or the AABB normalisation; the selector is the fp32 oracle's.  ``B_x`` is ``B_p`` pushed through the elementwise
    absolute Jacobian.  A sample with selector 0 has g_x == 0 exactly (and B_x == 0).

    Contraction, closed form: c = s(m) x with m = max_k |x_k| and s(m) = 2/m - 1/m^2 for m >= 1, the identity for m < 1, so
    d c_i / d x_j = s delta_ij + s'(m) x_i t_j,  s'(m) = -2/m^2 + 2/m^3,  t_j = d m / d x_j.
    Tie rule (torch's inf-norm backward, and the kernels'): t_j = sign(x_j) / (number of axes with |x_k| == m) on those axes,
    0 elsewhere — the subgradient is split evenly among the tied maxima.

    The origin.  torch (and the reference implementation, which uses the same ``torch.where(mag < 1, x, (2 - 1/mag) * (x/mag))``)
    returns NaN for a sample exactly at the origin: autograd differentiates BOTH branches of the where and multiplies the
    unselected one's gradient by 0, and there d (x / mag) is 0/0.  The kernels branch on ``mag < 1`` and return the identity
    branch's finite value; this function defines the origin the same way."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    _, sel = normalized(x32, space)
    sel = sel.astype(np.float64)[:, None]
    g = np.asarray(g_p, dtype=np.float64) * sel
    B = np.abs(np.asarray(B_p, dtype=np.float64)) * sel
    if not space.contraction:
        a = np.asarray(space.aabb, dtype=np.float32).astype(np.float64)
        ext = a[1] - a[0]
        return g / ext, B / np.abs(ext)
    g, B = g / 4.0, B / 4.0
    ax = np.abs(x)
    m = ax.max(axis=1, keepdims=True)
    out = m[:, 0] >= 1.0
    mo = np.where(out[:, None], m, 1.0)  # (no division by a small m on the identity branch)
    s = 2.0 / mo - 1.0 / mo ** 2
    ds = -2.0 / mo ** 2 + 2.0 / mo ** 3
    tied = ax == m
    t = np.sign(x) * tied / tied.sum(axis=1, keepdims=True)
    g_out = s * g + ds * (g * x).sum(axis=1, keepdims=True) * t
    B_out = s * B + np.abs(ds) * (B * ax).sum(axis=1, keepdims=True) * np.abs(t)
    return np.where(out[:, None], g_out, g), np.where(out[:, None], B_out, B)


def frustum_positions_adjoint(d_pos, starts, ends):
    """Frustums.get_positions backward, fp64: pos = o + d (s + e) / 2, so d_o = sum_i g_i and d_d = sum_i g_i (s_i + e_i) / 2.
    ``d_pos`` [R, n, 3], ``starts`` / ``ends`` [R, n].  Returns (d_o, d_d, B_o, B_d) [R, 3]: the sums and their absolute sums."""
    g = np.asarray(d_pos, dtype=np.float64)
    t = ((np.asarray(starts, dtype=np.float64) + np.asarray(ends, dtype=np.float64)) / 2.0)[..., None]
    return g.sum(axis=1), (g * t).sum(axis=1), np.abs(g).sum(axis=1), (np.abs(g) * np.abs(t)).sum(axis=1)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the kernels' arithmetic (numpy float32, one rounding per operation): the condition that the REFERENCE and
# the counted K fit together without a device — a restatement that left K * eps * B would mean a miscounted K or a wrong B
# ----------------------------------------------------------------------------------------------------------------------
def kernel_level_gradient_fp32(p32, d_enc_l, table, scale, level, log2T):
    """encode_level_grad in numpy float32, operation by operation; returns the level's contribution [n, 3] float32"""
    f32 = np.float32
    fl, ce, _ = frozen_cell(p32, scale)
    s = f32(scale)
    sx = (np.asarray(p32, dtype=f32) * s).astype(f32)
    o = (sx - np.floor(sx)).astype(f32)
    q = (f32(1.0) - o).astype(f32)
    f = [v.astype(f32) for v in _corner_values(fl, ce, table, level, log2T)]
    ox, oy, oz = (o[:, c:c + 1] for c in range(3))
    qx, qy, qz = (q[:, c:c + 1] for c in range(3))
    ge = np.asarray(d_enc_l, dtype=f32).reshape(-1, 2)
    (a03, b03), (a12, b12), (a56, b56), (a47, b47) = _pairs(f)
    f03, f12 = a03 * ox + b03 * qx, a12 * ox + b12 * qx
    f47, f56 = a47 * ox + b47 * qx, a56 * ox + b56 * qx
    dox = ((a03 - b03) * oy + (a12 - b12) * qy) * oz + ((a47 - b47) * oy + (a56 - b56) * qy) * qz
    doy = (f03 - f12) * oz + (f47 - f56) * qz
    doz = (f03 * oy + f12 * qy) - (f47 * oy + f56 * qy)
    out = np.zeros((len(sx), 3), dtype=f32)
    for c, d in enumerate((dox, doy, doz)):
        assert d.dtype == f32
        for ch in range(2):
            out[:, c] += ge[:, ch] * d[:, ch] * s
    return out


def _fma32(a, b, c):
    """fmaf: the fp32 product is exact in fp64, so only the sum is rounded before the final rounding to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lerp_w32(a, b, o):
    """lerp_w of tn_device.h: fmaf(o, a, fmaf(-o, b, b))"""
    return _fma32(o, a, _fma32(-o, b, b))


def kernel_level_jacobian_fp32(p32, table, scale, level, log2T):
    """the slopes of hash_blend_jac (floor / floor + 1 corners, two-fmaf interpolation o a + (1 - o) b, slope zeroed where the
    offset is 0) times the level scale, as tn_field_fwd_train stores them: [n, 3 axes, 2 features] float32"""
    f32 = np.float32
    s = f32(scale)
    sx = (np.asarray(p32, dtype=f32) * s).astype(f32)
    fl = np.floor(sx).astype(np.int64)
    o = (sx - np.floor(sx)).astype(f32)
    f = [v.astype(f32) for v in _corner_values(fl, fl + 1, table, level, log2T)]
    ox, oy, oz = (o[:, c:c + 1] for c in range(3))
    d03, d12, d56, d47 = f[0] - f[3], f[1] - f[2], f[5] - f[6], f[4] - f[7]
    c03, c12 = _lerp_w32(f[0], f[3], ox), _lerp_w32(f[1], f[2], ox)
    c56, c47 = _lerp_w32(f[5], f[6], ox), _lerp_w32(f[4], f[7], ox)
    jac = np.stack([_lerp_w32(_lerp_w32(d03, d12, oy), _lerp_w32(d47, d56, oy), oz),
                    _lerp_w32(c03 - c12, c47 - c56, oz),
                    _lerp_w32(c03, c12, oy) - _lerp_w32(c47, c56, oy)], axis=1)
    jac[o == 0] = 0.0
    assert jac.dtype == f32
    return jac * s


def kernel_level_jacobian_shared_differences_fp32(p32, table, scale, level, log2T):
    """the form hash_blend_jac had before: the slopes from the differences the feature lerp fmaf(o, a - b, b) forms anyway.  Kept
    as a restatement only, to show what the bound separates (tests/test_position_gradient_cpu.py)."""
    f32 = np.float32
    s = f32(scale)
    sx = (np.asarray(p32, dtype=f32) * s).astype(f32)
    fl = np.floor(sx).astype(np.int64)
    o = (sx - np.floor(sx)).astype(f32)
    f = [v.astype(f32) for v in _corner_values(fl, fl + 1, table, level, log2T)]
    ox, oy, oz = (o[:, c:c + 1] for c in range(3))
    d03, d12, d56, d47 = f[0] - f[3], f[1] - f[2], f[5] - f[6], f[4] - f[7]
    f03, f12, f56, f47 = _fma32(ox, d03, f[3]), _fma32(ox, d12, f[2]), _fma32(ox, d56, f[6]), _fma32(ox, d47, f[7])
    e0312, e4756 = f03 - f12, f47 - f56
    f0312, f4756 = _fma32(oy, e0312, f12), _fma32(oy, e4756, f56)
    dx_hi, dx_lo = _fma32(oy, d03 - d12, d12), _fma32(oy, d47 - d56, d56)
    jac = np.stack([_fma32(oz, dx_hi - dx_lo, dx_lo), _fma32(oz, e0312 - e4756, e4756), f0312 - f4756], axis=1)
    jac[o == 0] = 0.0
    return jac * s


def kernel_chain_fp32(x32, g_p32, space: Space):
    """position_grad_finish in numpy float32"""
    f32 = np.float32
    x = np.asarray(x32, dtype=f32)
    _, sel = normalized(x32, space)
    g = np.asarray(g_p32, dtype=f32) * sel.astype(f32)[:, None]
    if not space.contraction:
        a = np.asarray(space.aabb, dtype=f32)
        return g / (a[1] - a[0])
    g = g * f32(0.25)
    ax = np.abs(x)
    mag = ax.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sm = f32(2.0) / mag - f32(1.0) / (mag * mag)
        dsm = f32(-2.0) / (mag * mag) + f32(2.0) / (mag * mag * mag)
        dot = (g[:, 0:1] * x[:, 0:1] + g[:, 1:2] * x[:, 1:2]) + g[:, 2:3] * x[:, 2:3]
        tied = ax == mag
        share = dsm * dot / tied.sum(axis=1, keepdims=True).astype(f32)
        r = sm * g + np.where(tied, share * np.where(x > 0, f32(1.0), f32(-1.0)), f32(0.0))
    assert r.dtype == f32
    return np.where(mag < 1.0, g, r)


# ----------------------------------------------------------------------------------------------------------------------
# case builders: fp32 world positions [n, 3] and one label per sample
# ----------------------------------------------------------------------------------------------------------------------
class Cases(NamedTuple):
    positions: np.ndarray  # [n, 3] float32, world space
    labels: List[str]

    def __len__(self):
        return len(self.labels)

    def where(self, prefix: str) -> np.ndarray:
        return np.array([i for i, l in enumerate(self.labels) if l.startswith(prefix)], dtype=np.int64)


def concat(*cases: Cases) -> Cases:
    return Cases(np.concatenate([c.positions for c in cases]).astype(np.float32), [l for c in cases for l in c.labels])


def shuffled(cases: Cases, seed: int, n: Optional[int] = None) -> Cases:
    """the cases in a seeded random order; ``n``: that many of them (the first n of the permutation, cycled if there are fewer)"""
    perm = np.random.default_rng(seed).permutation(len(cases))
    if n is not None:
        perm = np.resize(perm, n)
    return Cases(cases.positions[perm], [cases.labels[i] for i in perm])


def plane_values(scale: float, count: int, lo: float = 0.0, hi: float = 1.0) -> List[Tuple[int, np.float32]]:
    """(k, p) pairs of one level with p = fl32(k / s) inside (lo, hi) and fl32(p * s) == k (85 - 100 % of all k on the 16 -> 2048
    grid), whose fp32 neighbours fall into the two adjacent cells: fl32(p- * s) < k and fl32(p+ * s) > k (the product of a
    neighbour rounds back onto the plane where an ulp of p times s is less than half an ulp of k).  All checked here; ``count``
    of the k that pass, spread over the level."""
    s = np.float32(scale)
    k_lo, k_hi = int(np.floor(lo * scale)) + 1, int(np.ceil(hi * scale)) - 1
    out = []
    for k in range(k_lo, k_hi + 1):
        p = np.float32(np.float32(k) / s)
        below, above = np.nextafter(p, np.float32(-1.0)), np.nextafter(p, np.float32(2.0))
        if lo < below and above < hi and np.float32(p * s) == np.float32(k) and np.float32(below * s) < k < np.float32(above * s):
            out.append((k, p))
    assert len(out) >= count, (scale, len(out))
    return [out[i] for i in np.linspace(0, len(out) - 1, count).round().astype(int)]


def on_planes(scalings: Sequence[float], levels: Sequence[int], contraction: bool = False, per_level: int = 4, seed: int = 1) -> Cases:
    """For every level, values on its grid planes (p = fl32(k / s) with fl32(p * s) == k) on one, two and all three axes, each with
    its two neighbours one ulp of p on either side (all plane axes moved together); the other axes hold seeded random values.
    Labels: ``plane:l<level>:<axes>:<on|below|above>``.  World positions: p itself (the unit box) or, with ``contraction``, the
    point 4 p - 2 of the identity branch — exact for p in [0.25, 0.75], where the values are taken from then."""
    rng = np.random.default_rng(seed)
    lo, hi = (0.25, 0.75) if contraction else (0.0, 1.0)
    pos, labels = [], []
    for l in levels:
        for k, p in plane_values(float(scalings[l]), per_level, lo, hi):
            for axes in ((0,), (1, 2), (0, 1, 2)):
                base = (lo + (hi - lo) * (0.05 + 0.9 * rng.random(3))).astype(np.float32)
                for name, v in (("on", p), ("below", np.nextafter(p, np.float32(-1.0))), ("above", np.nextafter(p, np.float32(2.0)))):
                    q = base.copy()
                    q[list(axes)] = v
                    pos.append(q)
                    labels.append(f"plane:l{l}:{''.join('xyz'[a] for a in axes)}:{name}")
    pos = np.array(pos, dtype=np.float32)
    if contraction:
        world = (np.float32(4.0) * pos - np.float32(2.0)).astype(np.float32)
        assert np.array_equal(world.astype(np.float64), 4.0 * pos.astype(np.float64) - 2.0)  # exact
        assert np.array_equal(normalized(world, CONTRACTION)[0], pos)
        pos = world
    return Cases(pos, labels)


def dyadic(n: int, bits: int = 12, seed: int = 2) -> Cases:
    """positions j / 2^bits, 0 < j < 2^bits, in the unit box: ``p * s`` is exact in fp32 and in fp64 (12 + 11 bits)"""
    j = np.random.default_rng(seed).integers(1, 1 << bits, size=(n, 3))
    return Cases((j / float(1 << bits)).astype(np.float32), ["dyadic"] * n)


def contraction_kinks() -> Cases:
    """the contraction's kinks: the switch of branches at mag == 1, single / two-way / three-way maxima with mixed signs, far
    samples, a sample so far that 2 - 1/m rounds to 2 (selector 0), and the origin"""
    below, above = float(np.nextafter(np.float32(1.0), np.float32(0.0))), float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    rows = [
        ("kink:below1", (below, 0.3, -0.2)), ("kink:below1", (-0.1, -below, 0.4)), ("kink:below1:tie", (below, -below, 0.25)),
        ("kink:at1", (1.0, 0.3, -0.2)), ("kink:at1", (0.5, -0.25, -1.0)), ("kink:at1:tie2", (1.0, -1.0, 0.5)),
        ("kink:at1:tie3", (-1.0, 1.0, 1.0)),
        ("kink:above1", (above, 0.3, -0.2)), ("kink:above1", (0.7, -above, 0.1)), ("kink:above1:tie2", (0.6, above, -above)),
        ("kink:single", (1.7, 0.4, -0.9)), ("kink:single", (-0.3, -2.5, 1.1)), ("kink:single", (0.2, 1.3, 3.75)),
        ("kink:tie2", (1.5, 1.5, 0.2)), ("kink:tie2", (-1.0, -1.0, 0.5)), ("kink:tie2", (0.3, -1.25, 1.25)),
        ("kink:tie2", (2.5, 0.7, -2.5)),
        ("kink:tie3", (2.0, -2.0, 2.0)), ("kink:tie3", (-1.5, -1.5, -1.5)), ("kink:tie3", (1.25, 1.25, -1.25)),
        ("kink:far", (1e3, -300.0, 20.0)), ("kink:far", (-5.0, 40.0, -1e3)), ("kink:far:tie2", (1e3, 1e3, -7.0)),
        ("kink:sel0:2^25", (2.0 ** 25, 3.0, -4.0)), ("kink:sel0:2^25", (1.0, -2.0 ** 25, 2.0 ** 25)),
        ("kink:origin", (0.0, 0.0, 0.0)),
    ]
    return Cases(np.array([r[1] for r in rows], dtype=np.float32), [r[0] for r in rows])


def box_faces(aabb, seed: int = 3) -> Cases:
    """without contraction: for each of the six faces a position on it, one ulp inside and one ulp outside (the ulp of the
    larger of the face's coordinate and the box's extent, so the normalised coordinate moves by an ulp of 1 and not into the
    denormals); the other two axes are interior.  On a face p is exactly 0 or 1: selector 0.
    Labels ``face:<axis><min|max>:<on|inside|outside>``."""
    a = np.asarray(aabb, dtype=np.float32)
    rng = np.random.default_rng(seed)
    pos, labels = [], []
    for axis in range(3):
        for side, name in ((0, "min"), (1, "max")):
            face = a[side, axis]
            ulp = np.spacing(np.float32(max(abs(face), abs(a[1, axis] - a[0, axis]))))
            inward = ulp if side == 0 else -ulp
            base = (a[0] + (a[1] - a[0]) * (0.1 + 0.8 * rng.random(3)).astype(np.float32)).astype(np.float32)
            for where, v in (("on", face), ("inside", np.float32(face + inward)), ("outside", np.float32(face - inward))):
                q = base.copy()
                q[axis] = v
                pos.append(q)
                labels.append(f"face:{'xyz'[axis]}{name}:{where}")
    return Cases(np.array(pos, dtype=np.float32), labels)


def mixed_cases(scalings: Sequence[float], contraction: bool, seed: int = 0) -> Cases:
    """every builder's cases for one grid and one space (the unit box, or the contraction), shuffled: what the device tests run.
    Cases made for the other space ride along (the kinks lie mostly outside the unit box: selector 0; the faces of the
    [-1, 1] box are the contraction's mag == 1)."""
    levels = range(len(scalings))
    if contraction:
        parts = (on_planes(scalings, levels, contraction=True), contraction_kinks(), dyadic(300), uniform(1500, 8, 3.0),
                 uniform(500, 9, 1.0), box_faces([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]))
    else:
        parts = (on_planes(scalings, levels), dyadic(1000), box_faces(UNIT_BOX.aabb), uniform(1500, 10, 0.6, center=0.5),
                 contraction_kinks())
    return shuffled(concat(*parts), seed)


def uniform(n: int, seed: int, extent: float, center: float = 0.0) -> Cases:
    """uniformly random positions in [center - extent, center + extent]^3"""
    x = center + (np.random.default_rng(seed).random((n, 3)) * 2.0 - 1.0) * extent
    return Cases(x.astype(np.float32), ["uniform"] * n)
