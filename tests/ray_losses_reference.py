"""fp64 references of the per-ray kernels of a training step's backward chain and of its losses, element by element, with the
bounds they are held to and builders of inputs on which they are EXACT in fp32 — numpy, no device.  The sibling of
tests/position_gradient_reference.py and tests/table_gradient_reference.py, one stage further up the chain:

* ``render_adjoint``  tn_ray_render_bwd (get_weights + both compositors + accumulation + distance-squared gradient scaling) in
                      closed form; with the compositor inputs absent it is tn_weights_bwd.  ``composite_adjoint``: tn_composite_bwd.
* ``distortion``      tn_distortion_loss[_term], O(n^2) form of oracle.training.lossfun_distortion
* ``interlevel``      tn_interlevel_loss[_levels], np.searchsorted(side="right") and the clamps of oracle.training.outer
* ``image_losses``    tn_image_losses

All references take the fp32 inputs as given and widen them.  Where a kernel forms ONE correctly rounded fp32 value from inputs the
reference forms it in fp32 too and widens it (a_i = fl32(delta_i sigma_i), the mid-points fl32((t_i + t_i+1) / 2), den =
fl32(w_i + 1e-7f), k = fl32(2 / fl32(count))), so that it carries no error of its own there.  The library is built with
-ffp-contract=off: no fused multiply-adds to model, except the explicit fmaf of image_losses_kernel (one rounding, counted as one).

Bounds.  u = 2^-24.  Every K below counts fp32 roundings on the longest dependency path of the kernel as written (first order in u,
as the K_* of the siblings); none was tuned against device output.  A wave scan (wave_incl_scan, wave_incl_scan_rev, wave_sum) is
6 adds deep; a carry over c chunks of 64 adds c roundings.  A sum whose terms each pass through at most D roundings is off by at most
D u (sum of |terms|); m values added in ANY order (atomics) pass through at most m - 1 adds each.

render adjoint (n <= 1024, 16 chunks).  E_i = sum_{j<i} a_j: wave_sum of a chunk (6) + `before` over up to 15 chunk sums (15) +
  the add onto the chunk's own scan (1): K_E = 22 relative to E_i (the a_j are >= 0 in every case here; |a_j| is summed anyway).
  T_i = expf(-E_i) is then off by (K_E E_i + K_EXP) u relative: the error of the argument is absolute in the exponent.  The bound
  carries E_i per term, not a flat factor.  ea = expf(-a): K_EXP.  w = (1 - ea) T: the subtraction loses what ea lost,
  ABSOLUTELY: |dw_i| <= u (w_i (K_E E_i + K_EXP + 2) + K_EXP ea_i T_i) =: u werr_i (2 = the subtraction's and the product's roundings).
  d_w_i = (ext + d_acc) + (r0 + r1 + r2) + th, r_c = d_rgb_c (v_c - last_c): a colour term passes sub, mul, two adds, the add onto
  d_w, the thermal add: K_DW = 6, relative to Bdw_i = |ext| + |d_acc| + sum_c |d_rgb_c| |v_c - last_c| + |d_th| |th - last|.
  first = (d_w ea) T: |err| <= u ea T (K_DW Bdw + |d_w| (2 K_EXP + K_E E_i + 2)).
  behind_i = (rincl - p_i) + suffix, p_k = d_w_k w_k: |err p_k| <= u (w_k K_DW Bdw_k + |d_w_k| werr_k + |d_w_k| w_k); the terms
  pass the reverse scan (6), the subtraction of p_i (1), up to 15 adds in `suffix` and the add of it (1): K_SUFFIX = 23, relative to
  sum_{k >= i} |p_k| (p_i is added and taken out again).
  tail: first - behind (1), delta * (1), * scale (1), scale = clamp(dist^2) with dist = (s + e) / 2 (1) squared (1): K_TAIL = 5
  relative to |first| + sum_{k >= i} |p_k|.
  d_v_i = (d_out (w_i + [last] bg)) scale, bg = 1 - acc (1): u |d_out| scale (werr_i + [last] (2 |bg| + w_i) + K_TAIL (w_i + [last] |bg|)).
  Underflow: a product whose T_i is denormal, or that is itself, may be flushed: one smallest normal (2^-126) per term, times the
  factors it is multiplied by afterwards.
  K_EXP: the device library's expf has no documented ulp bound among the files of the ROCm installation this was written
  against (searched; the OpenCL header there bounds only the half_ / native_ forms).  tools/micro/libm_accuracy.hip measured the
  LIBRARY FUNCTION (not the kernels) against fp64 exp on an MI355X over t in [0, 104], 10^7 points: worst 1.3863 u relative for
  normal results, denormal results correctly rounded (profiles/micro/libm_accuracy.txt).  Margin 2x, rounded up: K_EXP = 3.
  log10f over [2^-24, 2^40]: worst 2.8206 u relative; margin 2x, rounded up: K_LOG10 = 6.

composite adjoint.  d_v = g (w + [last] (1 - acc)): K_COMPOSITE_V = 3.  d_w += sum_c g_c (v_c - last_c): sub, mul, C - 1 adds
  (the first is onto 0: exact), the add onto what the buffer held: K_COMPOSITE_W = 5 relative to |held| + sum_c |g_c| |v_c - last_c|.

distortion.  c = ceil(n / 64) - 1 carries.  X_lt (X = W or WU) = carry + scan - own: product (1, WU only) + 6 + c + 2 =: D_lt = 9 + c;
  X = all: D_all = 7 + c;  X_gt = (X - X_lt) - own: D_all + D_lt + 1 + 4 (two subtractions of values up to twice the absolute sum);
  X_lt - X_gt: 2 D_lt + D_all + 7;  S_i = u_i (..) - (..): + 3  ->  K_S(n) = 2 D_lt + D_all + 10 = 35 + 3 c.  Gradient
  gscale (2 S_i + 2 w_i d_i / 3), gscale = scale mult: + 3  ->  K_DISTORTION(n) = 38 + 3 c, relative to |gscale| 2 B_i with
  B_i = sum_j |w_j| (|u_i| + |u_j|) + |w_i| d_i / 3 (2 S_i: exact doubling of both).  The intra term (d_i, the product, / 3, tail: 6)
  is below that.  Loss: w_i S_i + w_i^2 d_i / 3 per lane over the chunks, the rays of a wave, a wave_sum, the block's 2 adds, scale,
  one atomic per block and the add onto what loss_sum held: K_S + 3 + (c + 1) + rays_per_wave + 6 + 2 + 1 + blocks.

interlevel.  w_outer = max(cum[hi + 1] - cum[lo], 0): the envelope of weights is >= 0 (see covered_interlevel_case for what the
  kernel did without the max).  On the bounded and exact inputs of this module (weights on a dyadic grid) cum, w_outer and d are exact; den is formed in fp32 by the
  reference as well, so coef_i = fl32(-2 d_i / den_i) carries ONE rounding (the division is correctly rounded).  dhi / dlo take m
  coefficients by LDS atomics in any order (m - 1 adds); the reverse scans 6 + up to 16 carries + the add of the carry (1); the
  difference (1); the scale (1): K_INTERLEVEL = 1 + 6 + 16 + 1 + 1 + 1 = 26, and |got - want| <= (K_INTERLEVEL + m_k) u B_k with
  B_k = |scale| sum_i |coef_i| over ALL i with coef != 0 (each of the two suffix sums may hold every coefficient) and m_k their
  number.  With weights off the grid d_i = w_i - (cum[hi + 1] - cum[lo]) cancels and no bound in |coef| holds; such inputs belong to
  the rel-L2 tests of tests/test_gpu_training.py.  Loss: d d (exact here) / den (1) per lane over ceil(n / 64) intervals, then as
  the distortion loss.

image losses.  e = a - b (1: 2 on e^2), one fmaf per element of a thread (ceil(count / 1024)), wave_sum (6), 15 adds over the 16
  waves, the division (1): K_MSE(count) = 2 + ceil(count / 1024) + 22.  PSNR = 10 log10f(1 / mse): the argument is off by
  (K_MSE + 1) u relative, i.e. 10 / ln 10 times that absolutely in the result; log10f (K_LOG10) and the product (1) relative to it.
  Gradients: fl32(k fl32(a - b)), k = fl32(2 / fl32(count)): two roundings, modelled — bit-equal.

Exact families.
* dyadic distortion: edges multiples of 3 * 2^-10 in [0, 1] (d_i / 3 and u_i are multiples of 2^-11 and 3 * 2^-11), weights multiples
  of 2^-6 summing to at most 4 per ray: W, WU, every prefix, S_i and 2 S_i + 2 w_i d_i / 3 are multiples of
  2^-17 below 2^5 — fp32 numbers in any summation order; with scale and mult powers of two the device gradient equals the fp64
  reference bit for bit.  The loss terms w_i S_i + w_i^2 d_i / 3 are multiples of 2^-23: with the light weights of
  ``loss_exact`` the terms of a whole launch sum below 2 and the loss is bit-exact as well, whatever the order of the atomics.
* single-active-interval interlevel: exactly one d_i > 0 per ray, so dhi and dlo receive one value each and the gradient is
  fl32(scale fl32(coef)) on lo .. hi and 0 elsewhere whatever the order of the adds.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

f32, f64 = np.float32, np.float64
EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126

K_EXP = 3
K_LOG10 = 6
K_E = 22
K_DW = 6
K_SUFFIX = 23
K_TAIL = 5
K_COMPOSITE_V = 3
K_COMPOSITE_W = 5
K_INTERLEVEL = 26
MAX_SAMPLES = 1024
LOSS_GRID_CAP = 512      # blocks of the two loss launchers
WAVES_PER_BLOCK = 4


def _c(x, dt=f32):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dt))


def k_distortion(n: int) -> int:
    return 38 + 3 * ((n + 63) // 64 - 1)


def k_distortion_s(n: int) -> int:
    return 35 + 3 * ((n + 63) // 64 - 1)


def loss_blocks(R: int) -> int:
    return max(1, min((R + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, LOSS_GRID_CAP))


def _k_loss_tail(R: int, n: int, launches: int = 1) -> int:
    blocks = loss_blocks(R)
    rays_per_wave = -(-R // (blocks * WAVES_PER_BLOCK))
    return (n + 63) // 64 + rays_per_wave + 6 + 2 + 1 + blocks * launches


def k_distortion_loss(R: int, n: int) -> int:
    return k_distortion_s(n) + 3 + _k_loss_tail(R, n)


def k_interlevel_loss(R: int, n: int, levels: int = 1) -> int:
    return 1 + _k_loss_tail(R, n, levels)


def k_mse(count: int) -> int:
    return 2 + -(-count // 1024) + 22


# ----------------------------------------------------------------------------------------------------------------------
# render adjoint
# ----------------------------------------------------------------------------------------------------------------------
class RenderAdjoint(NamedTuple):
    d_rgb_samples: Optional[np.ndarray]      # [R, n, 3] fp64, None without d_rgb
    d_thermal_samples: Optional[np.ndarray]  # [R, n]
    d_densities: np.ndarray                  # [R, n]
    weights: np.ndarray                      # [R, n] fp64 w_i
    mag: Dict[str, np.ndarray]               # what tolerance_render_*() read


def render_adjoint(deltas, densities, d_weights=None, rgb=None, thermal=None, accumulation=None, d_rgb=None, d_thermal=None,
                   d_accumulation=None, starts=None, ends=None) -> RenderAdjoint:
    """closed form of tn_ray_render_bwd; every optional input may be None.  With rgb .. d_accumulation None: tn_weights_bwd."""
    dl32, dn32 = _c(deltas), _c(densities)
    R, n = dl32.shape
    a = (dl32 * dn32).astype(f32).astype(f64)          # the one rounded product the kernel forms as well
    dl = dl32.astype(f64)
    E = np.concatenate([np.zeros((R, 1)), np.cumsum(a, axis=1)[:, :-1]], axis=1)
    Eabs = np.concatenate([np.zeros((R, 1)), np.cumsum(np.abs(a), axis=1)[:, :-1]], axis=1)
    T, ea = np.exp(-E), np.exp(-a)
    w = -np.expm1(-a) * T
    last = np.zeros((R, n))
    last[:, -1] = 1.0
    dw = np.zeros((R, n))
    Bdw = np.zeros((R, n))
    if d_weights is not None:
        dw += _c(d_weights, f64)
        Bdw += np.abs(_c(d_weights, f64))
    if d_accumulation is not None:
        dw += _c(d_accumulation, f64).reshape(R, 1)
        Bdw += np.abs(_c(d_accumulation, f64)).reshape(R, 1)
    bg = None
    if d_rgb is not None or d_thermal is not None:
        bg = 1.0 - _c(accumulation, f64).reshape(R, 1)
    if d_rgb is not None:
        v, g = _c(rgb, f64).reshape(R, n, 3), _c(d_rgb, f64).reshape(R, 1, 3)
        diff = v - v[:, -1:, :]
        dw += (g * diff).sum(-1)
        Bdw += (np.abs(g) * np.abs(diff)).sum(-1)
    if d_thermal is not None:
        th, gt = _c(thermal, f64).reshape(R, n), _c(d_thermal, f64).reshape(R, 1)
        dw += gt * (th - th[:, -1:])
        Bdw += np.abs(gt) * np.abs(th - th[:, -1:])
    scale = np.ones((R, n))
    if starts is not None:
        mid = (_c(starts, f64).reshape(R, n) + _c(ends, f64).reshape(R, n)) / 2
        scale = np.clip(mid * mid, 0.0, 1.0)
    p = dw * w
    rev = lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1]  # noqa: E731  inclusive suffix sums
    behind = rev(p) - p
    first = dw * ea * T
    d_dens = dl * (first - behind) * scale
    werr = np.abs(w) * (K_E * Eabs + K_EXP + 2) + K_EXP * ea * T
    perr = np.abs(w) * K_DW * Bdw + np.abs(dw) * werr + np.abs(p)
    pabs_incl = rev(np.abs(p))
    mag = dict(E=Eabs, T=T, ea=ea, werr=werr, dw=dw, Bdw=Bdw, scale=scale, delta=np.abs(dl), last=last,
               first_err=ea * T * (K_DW * Bdw + np.abs(dw) * (2 * K_EXP + K_E * Eabs + 2)),
               behind_err=(rev(perr) - perr) + K_SUFFIX * pabs_incl,
               tail=np.abs(first) + pabs_incl,
               floor_terms=rev(1.0 + np.abs(dw)), bg=np.zeros((R, 1)) if bg is None else bg)
    d_rgb_s = d_th_s = None
    if d_rgb is not None:
        d_rgb_s = _c(d_rgb, f64).reshape(R, 1, 3) * ((w + last * bg) * scale)[..., None]
    if d_thermal is not None:
        d_th_s = _c(d_thermal, f64).reshape(R, 1) * (w + last * bg) * scale
    return RenderAdjoint(d_rgb_s, d_th_s, d_dens, w, mag)


def tolerance_render_densities(ref: RenderAdjoint) -> np.ndarray:
    m = ref.mag
    first_order = m["first_err"] + m["behind_err"] + K_TAIL * m["tail"]
    return m["delta"] * m["scale"] * (EPS32 * first_order + TINY32 * m["floor_terms"]) + TINY32


def tolerance_render_values(ref: RenderAdjoint, d_out) -> np.ndarray:
    """bound of d_rgb_samples ([R, n, 3] for d_out [R, 3]) or d_thermal_samples ([R, n] for d_out [R])"""
    m = ref.mag
    R, n = ref.weights.shape
    w, bgl = np.abs(ref.weights), m["last"] * np.abs(m["bg"])
    per = m["scale"] * (EPS32 * (m["werr"] + 2 * bgl + m["last"] * w + K_TAIL * (w + bgl)) + TINY32)
    g = np.abs(_c(d_out, f64))
    if g.shape == (R, 3):
        return g[:, None, :] * per[..., None] + TINY32
    return g.reshape(R, 1) * per + TINY32


def composite_adjoint(values, weights, accumulation, d_out, held) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """tn_composite_bwd for C in {1, 3}: (d_values [R, n, C], d_weights [R, n] = held + ..., tol_values, tol_weights)"""
    v, w, acc, g, held = _c(values, f64), _c(weights, f64), _c(accumulation, f64), _c(d_out, f64), _c(held, f64)
    R, n, C = v.shape
    last = np.zeros((1, n, 1))
    last[0, -1, 0] = 1.0
    bg = (1.0 - acc).reshape(R, 1, 1)
    g = g.reshape(R, 1, C)
    d_v = g * (w[..., None] + last * bg)
    diff = v - v[:, -1:, :]
    d_w = held + (g * diff).sum(-1)
    tol_v = K_COMPOSITE_V * EPS32 * np.abs(g) * (np.abs(w[..., None]) + last * np.abs(bg)) + TINY32
    tol_w = K_COMPOSITE_W * EPS32 * (np.abs(held) + (np.abs(g) * np.abs(diff)).sum(-1)) + TINY32
    return d_v, d_w, tol_v, tol_w


def render_adjoint_fp32(deltas, densities, d_weights=None, rgb=None, thermal=None, accumulation=None, d_rgb=None, d_thermal=None,
                        d_accumulation=None, starts=None, ends=None, pairwise=False, fault=None):
    """ray_render_bwd_kernel's formula in numpy float32, the sums sequential or pairwise, libm's exp rounded to fp32 for expf;
    ``fault``: "drop_suffix_term" | "no_background" | "scale_two_of_three" plants one.  Returns (d_rgb_s, d_th_s, d_dens)."""
    dl, dn = _c(deltas), _c(densities)
    R, n = dl.shape
    a = (dl * dn).astype(f32)
    E = np.zeros((R, n), f32)
    E[:, 1:] = _prefix32(a, pairwise)[:, :-1]
    T, ea = np.exp(-E.astype(f64)).astype(f32), np.exp(-a.astype(f64)).astype(f32)
    w = ((f32(1) - ea) * T).astype(f32)
    dwi = np.zeros((R, n), f32)
    if d_weights is not None:
        dwi = _c(d_weights).reshape(R, n).copy()
    if d_accumulation is not None:
        dwi = (dwi + _c(d_accumulation).reshape(R, 1)).astype(f32)
    scale = np.ones((R, n), f32)
    if starts is not None:
        dist = ((_c(starts).reshape(R, n) + _c(ends).reshape(R, n)).astype(f32) / f32(2)).astype(f32)
        scale = np.clip((dist * dist).astype(f32), f32(0), f32(1))
    wv = w.copy()
    if (d_rgb is not None or d_thermal is not None) and fault != "no_background":
        wv[:, -1] = (w[:, -1] + (f32(1) - _c(accumulation).reshape(R))).astype(f32)
    out_rgb = out_th = None
    if d_rgb is not None:
        v, g = _c(rgb).reshape(R, n, 3), _c(d_rgb).reshape(R, 1, 3)
        t = (g * (v - v[:, -1:, :]).astype(f32)).astype(f32)
        dwi = (dwi + ((t[..., 0] + t[..., 1]).astype(f32) + t[..., 2]).astype(f32)).astype(f32)
        out_rgb = ((g * wv[..., None]).astype(f32) * scale[..., None]).astype(f32)
    if d_thermal is not None:
        th, gt = _c(thermal).reshape(R, n), _c(d_thermal).reshape(R, 1)
        dwi = (dwi + (gt * (th - th[:, -1:]).astype(f32)).astype(f32)).astype(f32)
        out_th = (gt * wv).astype(f32)
        if fault != "scale_two_of_three":
            out_th = (out_th * scale).astype(f32)
    p = (dwi * w).astype(f32)
    if fault == "drop_suffix_term":
        p = p.copy()
        p[:, n // 2 + (n > 2)] = 0
    incl = _prefix32(p[:, ::-1], pairwise)[:, ::-1]
    behind = (incl - p).astype(f32)
    d_dens = ((dl * (((dwi * ea).astype(f32) * T).astype(f32) - behind).astype(f32)).astype(f32) * scale).astype(f32)
    return out_rgb, out_th, d_dens


def _prefix32(x: np.ndarray, pairwise: bool) -> np.ndarray:
    """inclusive prefix sums along axis 1 in float32: sequential, or a Hillis-Steele scan (the adds of a wave scan)"""
    x = np.ascontiguousarray(x, dtype=f32)
    if not pairwise:
        return np.cumsum(x, axis=1, dtype=f32)
    out, o = x.copy(), 1
    while o < out.shape[1]:
        nxt = out.copy()
        nxt[:, o:] = (out[:, o:] + out[:, :-o]).astype(f32)
        out, o = nxt, o * 2
    return out


def _sum32(x: np.ndarray, pairwise: bool) -> np.ndarray:
    return _prefix32(x, pairwise)[:, -1]


# ----------------------------------------------------------------------------------------------------------------------
# distortion
# ----------------------------------------------------------------------------------------------------------------------
class Distortion(NamedTuple):
    loss: np.ndarray   # [R] per-ray loss (unscaled)
    grad: np.ndarray   # [R, n] d loss_ray / d w (unscaled)
    B: np.ndarray      # [R, n] sum_j |w_j| (|u_i| + |u_j|) + |w_i| d_i / 3
    loss_abs: np.ndarray  # [R] sum_i |w_i| B_i


def distortion(bins, w) -> Distortion:
    t32, w = _c(bins), _c(w, f64)
    u = ((t32[:, 1:] + t32[:, :-1]).astype(f32) / f32(2)).astype(f32).astype(f64)  # the kernel's mid-points
    d = t32[:, 1:].astype(f64) - t32[:, :-1].astype(f64)
    dut = np.abs(u[:, :, None] - u[:, None, :])
    S = (w[:, None, :] * dut).sum(-1)
    loss = (w * S).sum(-1) + (w * w * d).sum(-1) / 3
    grad = 2 * S + 2 * w * d / 3
    aw = np.abs(w)
    B = np.abs(u) * aw.sum(-1, keepdims=True) + (aw * np.abs(u)).sum(-1, keepdims=True) + aw * d / 3
    return Distortion(loss, grad, B, (aw * B).sum(-1))


def tolerance_distortion(ref: Distortion, gscale: float) -> np.ndarray:
    n = ref.grad.shape[1]
    return k_distortion(n) * EPS32 * abs(gscale) * 2 * ref.B + TINY32


def tolerance_distortion_loss(ref: Distortion, scale: float, start: float = 0.0) -> float:
    R, n = ref.grad.shape
    return k_distortion_loss(R, n) * EPS32 * (abs(scale) * float(ref.loss_abs.sum()) + abs(start)) + TINY32


def distortion_fp32(bins, w, pairwise=False, fault=None):
    """distortion_kernel's formula in numpy float32 (unscaled gradient [R, n], per-ray loss [R]); fault: "gt_keeps_own" forms
    W_>i without the - w_i"""
    t, w = _c(bins), _c(w)
    u = ((t[:, 1:] + t[:, :-1]).astype(f32) / f32(2)).astype(f32)
    d = (t[:, 1:] - t[:, :-1]).astype(f32)
    wu = (w * u).astype(f32)
    W, WU = _sum32(w, pairwise)[:, None], _sum32(wu, pairwise)[:, None]
    Wlt, WUlt = (_prefix32(w, pairwise) - w).astype(f32), (_prefix32(wu, pairwise) - wu).astype(f32)
    Wgt, WUgt = (W - Wlt).astype(f32), ((WU - WUlt).astype(f32) - wu).astype(f32)
    if fault != "gt_keeps_own":
        Wgt = (Wgt - w).astype(f32)
    S = ((u * (Wlt - Wgt).astype(f32)).astype(f32) - (WUlt - WUgt).astype(f32)).astype(f32)
    intra = ((w * d).astype(f32) / f32(3)).astype(f32)
    grad = ((f32(2) * S).astype(f32) + (f32(2) * intra).astype(f32)).astype(f32)
    terms = ((w * S).astype(f32) + (w * intra).astype(f32)).astype(f32)
    return grad, _sum32(terms, pairwise)


# ----------------------------------------------------------------------------------------------------------------------
# interlevel
# ----------------------------------------------------------------------------------------------------------------------
class Interlevel(NamedTuple):
    lo: np.ndarray       # [R, n] int
    hi: np.ndarray       # [R, n] int
    w_outer: np.ndarray  # [R, n]
    d: np.ndarray        # [R, n]
    coef: np.ndarray     # [R, n] -2 d / den
    loss: np.ndarray     # [R] sum_i d_i^2 / den_i (unscaled)
    grad: np.ndarray     # [R, p] sum of coef over lo_i <= k <= hi_i (unscaled)
    B: np.ndarray        # [R, 1] sum_i |coef_i|
    m: np.ndarray        # [R, 1] number of nonzero coef_i


def interlevel(c, w, cp, wp, shift_lo: int = 0, shift_hi: int = 0) -> Interlevel:
    """``shift_lo`` / ``shift_hi`` move the indices by one before the clamp: the planted tie-rule faults of the CPU tests"""
    c, w32, cp, wp = _c(c), _c(w), _c(cp), _c(wp, f64)
    R, n = w32.shape
    p = wp.shape[1]
    lo, hi = np.zeros((R, n), np.int64), np.zeros((R, n), np.int64)
    for r in range(R):
        lo[r] = np.searchsorted(cp[r, :-1], c[r, :-1], side="right") - 1 + shift_lo
        hi[r] = np.searchsorted(cp[r, 1:], c[r, 1:], side="right") + shift_hi
    lo, hi = np.clip(lo, 0, p - 1), np.clip(hi, 0, p - 1)
    cum = np.concatenate([np.zeros((R, 1)), np.cumsum(wp, axis=1)], axis=1)
    w_outer = np.take_along_axis(cum[:, 1:], hi, 1) - np.take_along_axis(cum[:, :-1], lo, 1)
    wd = w32.astype(f64)
    d = np.maximum(wd - w_outer, 0.0)
    den = (w32 + f32(1.0e-7)).astype(f32).astype(f64)
    coef = -2.0 * d / den
    grad = np.zeros((R, p))
    k = np.arange(p)[None, None, :]
    for r0 in range(0, R, 64):  # [rays, n, p] masks in slabs
        s = slice(r0, r0 + 64)
        inside = (lo[s, :, None] <= k) & (k <= hi[s, :, None])
        grad[s] = (coef[s, :, None] * inside).sum(1)
    return Interlevel(lo, hi, w_outer, d, coef, (d * d / den).sum(-1), grad, np.abs(coef).sum(-1, keepdims=True),
                      (coef != 0).sum(-1, keepdims=True))


def tolerance_interlevel(ref: Interlevel, scale: float) -> np.ndarray:
    """[R, 1] (broadcasts over k); 0 for a ray without a nonzero coefficient: its gradient must be exactly 0"""
    return (K_INTERLEVEL + ref.m) * EPS32 * abs(scale) * ref.B


def tolerance_interlevel_loss(refs: Sequence[Interlevel], scale: float, n: int, start: float = 0.0) -> float:
    R = refs[0].loss.shape[0]
    return k_interlevel_loss(R, n, len(refs)) * EPS32 * (abs(scale) * sum(float(r.loss.sum()) for r in refs) + abs(start)) + TINY32


def interlevel_exact_gradient(ref: Interlevel, scale: float) -> np.ndarray:
    """[R, p] float32 gradient of rays with AT MOST one nonzero coefficient: fl32(scale fl32(coef)) on lo .. hi, 0 elsewhere"""
    assert int(ref.m.max()) <= 1
    R, p = ref.grad.shape
    out = np.zeros((R, p), f32)
    k = np.arange(p)
    for r in range(R):
        for i in np.nonzero(ref.coef[r])[0]:
            out[r, (ref.lo[r, i] <= k) & (k <= ref.hi[r, i])] = f32(scale) * f32(ref.coef[r, i])
    return out


def wave_scan_fp32(x: np.ndarray) -> np.ndarray:
    """wave_incl_scan of tn_device.h on rows of 64 in numpy float32, add by add: shifts by 1, 2, 4, 8 inside the rows of 16, lane 15
    of rows 0 and 2 into rows 1 and 3, lane 31 into rows 2 and 3"""
    v = np.ascontiguousarray(x, dtype=f32).copy()
    assert v.shape[-1] == 64
    lane = np.arange(64)
    for o in (1, 2, 4, 8):
        src = np.where(lane % 16 >= o, lane - o, lane)
        v = np.where(lane % 16 >= o, (v + v[..., src]).astype(f32), v)
    v = np.where((lane // 16) % 2 == 1, (v + v[..., (lane // 16) * 16 - 1]).astype(f32), v)
    return np.where(lane >= 32, (v + v[..., [31] * 64]).astype(f32), v)


def envelope_cum_fp32(wp) -> np.ndarray:
    """interlevel_kernel's cum [R, p + 1]: chunks of 64, cum[k] = carry + incl - v, carry += the chunk's total"""
    wp = _c(wp)
    R, p = wp.shape
    chunks = p // 64 + 1
    v = np.zeros((R, chunks * 64), f32)
    v[:, :p] = wp
    cum, carry = np.zeros((R, chunks * 64), f32), np.zeros((R, 1), f32)
    for b in range(chunks):
        blk = v[:, 64 * b:64 * b + 64]
        incl = wave_scan_fp32(blk)
        cum[:, 64 * b:64 * b + 64] = ((carry + incl).astype(f32) - blk).astype(f32)
        carry = (carry + incl[:, 63:]).astype(f32)
    return cum[:, :p + 1]


def interlevel_fp32(c, w, cp, wp, pairwise=False, shift_lo=0, shift_hi=0, drop=False, wave=False, clamp=True):
    """interlevel_kernel's formula in numpy float32: difference arrays, two reverse sums, their difference (unscaled [R, p]).
    ``drop``: the last nonzero entry of dhi is left out of its suffix sum.  ``wave``: cum as the kernel's wave scan forms it.
    ``clamp=False``: w_outer without its max(.., 0), as the kernel had it."""
    ref = interlevel(c, w, cp, wp, shift_lo, shift_hi)
    w32, wp32 = _c(w), _c(wp)
    R, n = w32.shape
    p = wp32.shape[1]
    cum = envelope_cum_fp32(wp32) if wave else np.concatenate([np.zeros((R, 1), f32), _prefix32(wp32, pairwise)], axis=1)
    w_outer = (np.take_along_axis(cum[:, 1:], ref.hi, 1) - np.take_along_axis(cum[:, :-1], ref.lo, 1)).astype(f32)
    if clamp:
        w_outer = np.maximum(w_outer, f32(0))
    d = np.maximum((w32 - w_outer).astype(f32), f32(0))
    den = (w32 + f32(1.0e-7)).astype(f32)
    coef = ((f32(-2) * d).astype(f32) / den).astype(f32)
    dhi, dlo = np.zeros((R, p + 1), f32), np.zeros((R, p + 1), f32)
    order = range(n) if not pairwise else range(n - 1, -1, -1)
    for i in order:
        np.add.at(dhi, (np.arange(R), ref.hi[:, i]), coef[:, i])
        np.add.at(dlo, (np.arange(R), ref.lo[:, i]), coef[:, i])
    if drop:
        for r in range(R):
            nz = np.nonzero(dhi[r])[0]
            if len(nz):
                dhi[r, nz[-1]] = 0
    rh = _prefix32(dhi[:, :p][:, ::-1], pairwise)[:, ::-1]
    rl = _prefix32(dlo[:, 1:][:, ::-1], pairwise)[:, ::-1]
    return (rh - rl).astype(f32)


# ----------------------------------------------------------------------------------------------------------------------
# image losses
# ----------------------------------------------------------------------------------------------------------------------
class ImageLosses(NamedTuple):
    mse_rgb: float
    mse_thermal: Optional[float]
    psnr: float
    d_rgb: np.ndarray                # float32, the two-rounding expectation
    d_thermal: Optional[np.ndarray]


def _two_rounding_gradient(a32, b32):
    k = f32(2) / f32(a32.size)
    return (k * (a32 - b32).astype(f32)).astype(f32)


def image_losses(rgb, gt_rgb, thermal=None, gt_thermal=None) -> ImageLosses:
    a, b = _c(rgb), _c(gt_rgb)
    mse = float(np.mean((a.astype(f64) - b.astype(f64)) ** 2))
    psnr = math.inf if mse == 0.0 else 10.0 * math.log10(1.0 / mse)
    mt = dt = None
    if thermal is not None:
        t, g = _c(thermal), _c(gt_thermal)
        mt, dt = float(np.mean((t.astype(f64) - g.astype(f64)) ** 2)), _two_rounding_gradient(t, g)
    return ImageLosses(mse, mt, psnr, _two_rounding_gradient(a, b), dt)


def tolerance_mse(mse: float, count: int) -> float:
    return k_mse(count) * EPS32 * mse + TINY32


def tolerance_psnr(psnr: float, count: int) -> float:
    return EPS32 * (10.0 / math.log(10.0) * (k_mse(count) + 1) + (K_LOG10 + 1) * abs(psnr))


# ----------------------------------------------------------------------------------------------------------------------
# case builders
# ----------------------------------------------------------------------------------------------------------------------
def dyadic_distortion_case(R: int, n: int, seed: int, loss_exact: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(bins [R, n + 1], w [R, n]) float32: edges sorted multiples of 3 * 2^-10 in [0, 1] (repeats = zero-width bins), weights
    multiples of 2^-6 that sum to at most 4 per ray.  Ray r mod 5: 0 mixed with zeros, 1 one heavy sample (the rest 0), 2 sum
    above 1, 3 all edges on three values (many zero-width bins), 4 sparse.  The gradient of every such ray is exact in fp32.
    ``loss_exact``: the weights are kept light (one heavy ray and one ray above 1 per launch) so that the loss terms of the WHOLE
    launch, all >= 0 and multiples of 2^-23, sum below 2: every partial sum in any order and grouping is an fp32 number."""
    rng = np.random.default_rng(seed)
    steps = 341  # 341 * 3 / 1024 < 1
    bins = np.sort(rng.integers(0, steps + 1, size=(R, n + 1)), axis=1)
    w = np.zeros((R, n), np.int64)  # in units of 2^-6
    for r in range(R):
        kind = r % 5
        if kind == 3:
            bins[r] = np.sort(rng.choice(rng.integers(0, steps + 1, size=3), size=n + 1))
        if kind == 1:
            w[r, rng.integers(0, n)] = (32 if r == 1 else 1) if loss_exact else 256
            continue
        if loss_exact:
            budget = 72 if r == 2 else 2
        else:
            budget = {0: 64, 2: 256, 3: 64, 4: 5}[kind]
        np.add.at(w[r], rng.integers(0, n, size=budget), 1)
        if kind == 0 and n > 1:
            w[r, rng.random(n) < 0.5] = 0
    assert int(w.sum(1).max()) <= 256
    bins32, w32 = (bins * 3 / 1024).astype(f32), (w / 64).astype(f32)
    if loss_exact:
        assert float(distortion(bins32, w32).loss.sum()) < 2.0  # the terms are >= 0: this IS their absolute sum
    return bins32, w32


def general_distortion_case(R: int, n: int, seed: int, peaked: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(seed)
    bins = np.sort(rng.random((R, n + 1)), axis=1)
    bins[:, 0], bins[:, -1] = 0.0, 1.0
    w = rng.random((R, n)) ** (8 if peaked else 1)
    w = w / w.sum(1, keepdims=True) * rng.random((R, 1))
    return bins.astype(f32), w.astype(f32)


G = 2.0 ** -13  # the grid of the interlevel edges: proposal edge k sits at (4 k + 4) G, three grid points inside every bin

INTERVAL_KINDS = ("start_on_edge", "end_on_edge", "both_on_edges", "inside_one_bin", "spans_all", "starts_at_cp0", "ends_at_cpp",
                  "left_of_cp0", "right_of_cpp", "after_duplicates", "before_duplicates", "zero_width", "zero_width_on_edge")
_MIN_P = {"start_on_edge": 2, "end_on_edge": 2, "both_on_edges": 2, "after_duplicates": 3, "before_duplicates": 3,
          "zero_width_on_edge": 2}


def interval_kinds(p: int) -> List[str]:
    """the kinds that exist with p proposal bins (an interior edge needs p >= 2, a run of duplicates with a neighbour p >= 3)"""
    return [k for k in INTERVAL_KINDS if p >= _MIN_P.get(k, 1)]


def single_interval_case(kinds: Sequence[str], R: int, n: int, p: int, seed: int):
    """(c [R, n + 1], w [R, n], cp [R, p + 1], wp [R, p], active [R]) float32 / int: ray r is of kind kinds[r % len(kinds)] and has
    d_i > 0 for i = active[r] alone.  The inactive intervals carry w = 0 or w = w_outer exactly (d = 0 either way); wp are
    multiples of 2^-8 (some 0), the active weight exceeds its envelope by a multiple of 2^-6."""
    rng = np.random.default_rng(seed)
    c = np.zeros((R, n + 1))
    cp = np.tile((4 * np.arange(p + 1) + 4) * G, (R, 1))
    wp = rng.integers(0, 4, size=(R, p)) / 256.0
    active = rng.integers(0, n, size=R)
    top = 4 * p + 4  # cp[p] in grid units
    for r in range(R):
        kind = kinds[r % len(kinds)]
        a = int(rng.integers(1, p)) if p >= 2 else 0          # an interior edge
        b = int(rng.integers(a, p)) if p >= 2 else 0          # an interior edge at or after it (b = a possible)
        inside = lambda k: 4 * k + 4 + int(rng.integers(1, 4))  # noqa: E731  a grid point strictly inside bin k
        if kind == "start_on_edge":
            s, e = 4 * a + 4, inside(b)
        elif kind == "end_on_edge":
            s, e = inside(int(rng.integers(0, a))), 4 * b + 4
        elif kind == "both_on_edges":
            s, e = 4 * a + 4, 4 * b + 4
            if p >= 3 and s == e:
                a, b = 1, 2
                s, e = 4 * a + 4, 4 * b + 4
        elif kind == "inside_one_bin":
            k = int(rng.integers(0, p))
            s, e = 4 * k + 5, 4 * k + 7
        elif kind == "spans_all":
            s, e = 5, top - 1
        elif kind == "starts_at_cp0":
            s, e = 4, inside(int(rng.integers(0, p)))
        elif kind == "ends_at_cpp":
            s, e = inside(int(rng.integers(0, p))), top
        elif kind == "left_of_cp0":
            s, e = 0, 2
        elif kind == "right_of_cpp":
            s, e = top + 1, top + 3
        elif kind in ("after_duplicates", "before_duplicates"):
            a = int(rng.integers(1, p - 1))                    # edges a and a + 1 coincide: bin a has zero width
            run = 1 + int(rng.integers(0, min(3, p - 1 - a)))  # ... and up to two more behind it
            cp[r, a:a + run + 1] = cp[r, a]
            v = int(round(cp[r, a] / G))
            if kind == "after_duplicates":
                s, e = v, inside(int(rng.integers(a + run, p)))
            else:
                s, e = inside(int(rng.integers(0, a))), v
        elif kind == "zero_width":
            s = e = inside(int(rng.integers(0, p)))
        elif kind == "zero_width_on_edge":
            s = e = 4 * a + 4
        else:
            raise ValueError(kind)
        i = int(active[r])
        before = np.sort(rng.integers(0, s + 1, size=i))
        after = np.sort(rng.integers(e, top + 9, size=n - 1 - i))
        c[r] = np.concatenate([before, [s, e], after]) * G
    c32, cp32, wp32 = c.astype(f32), cp.astype(f32), wp.astype(f32)
    w = np.zeros((R, n), f32)
    env = interlevel(c32, w, cp32, wp32).w_outer
    keep = rng.random((R, n)) < 0.5
    w[keep] = env[keep].astype(f32)
    rows = np.arange(R)
    w[rows, active] = (env[rows, active] + rng.integers(1, 65, size=R) / 64.0).astype(f32)
    return c32, w, cp32, wp32, active


def general_interlevel_case(R: int, n: int, p: int, seed: int):
    """(c, w, cp, wp) float32 for the bounded check: proposal edges sorted fp32 numbers in [0, 1] with a few repeats; final edges
    a sorted mix of proposal edges copied exactly and points strictly between two of them (the PDF resampler interpolates final
    edges from proposal edges); weights multiples of 2^-12 (see the module docstring), some w_i and wp_k zero; every third ray is
    covered by its envelope (every d_i = 0: the gradient must be exactly 0)."""
    rng = np.random.default_rng(seed)
    cp = np.sort(rng.random((R, p + 1)).astype(f32), axis=1)
    cp[:, 0], cp[:, -1] = 0.0, 1.0
    if p >= 4:
        for r in range(0, R, 2):
            k = int(rng.integers(1, p - 1))
            cp[r, k + 1] = cp[r, k]
    c = np.zeros((R, n + 1), f32)
    for r in range(R):
        k = rng.integers(0, p, size=n + 1)
        between = (cp[r, k].astype(f64) + (cp[r, k + 1].astype(f64) - cp[r, k]) * rng.random(n + 1)).astype(f32)
        copied = cp[r, rng.integers(0, p + 1, size=n + 1)]
        c[r] = np.sort(np.where(rng.random(n + 1) < 0.4, copied, between))
    wp = rng.integers(0, 64, size=(R, p)) * (rng.random((R, p)) < 0.8) / 4096.0
    w = rng.integers(0, 256, size=(R, n)) * (rng.random((R, n)) < 0.8) / 4096.0
    wp32 = wp.astype(f32)
    env = interlevel(c, np.zeros((R, n), f32), cp, wp32).w_outer
    w[::3] = np.minimum(w[::3], env[::3])
    return c, w.astype(f32), cp, wp32


def covered_interlevel_case(R: int, n: int, p: int, seed: int):
    """(c, w, cp, wp) float32 with w = 0 everywhere and proposal weights that are NOT on a grid (a peaked profile summing to
    0.3 .. 1, runs of exact zeros, a tail of exact zeros — what a saturated ray leaves behind its surface): the envelope of
    nonnegative weights is >= 0, so every d_i = max(0 - w_outer, 0) is 0, the loss adds nothing and the gradient is exactly 0.
    A cumulative sum that is not monotone in fp32 (a parallel scan groups the same addends differently from lane to lane) gives
    w_outer = -1 ulp of the total over a run of zeros, which den = 1e-7 turns into a coefficient of order 1."""
    rng = np.random.default_rng(seed)
    c, _, cp, _ = general_interlevel_case(R, n, p, seed)
    wp = rng.random((R, p)) ** 4
    wp = wp / wp.sum(1, keepdims=True) * (0.3 + 0.7 * rng.random((R, 1)))
    for r in range(R):
        if p >= 2:
            wp[r, int(rng.integers(max(1, p // 8), max(2, 7 * p // 8))):] = 0
        if p >= 16:
            k = int(rng.integers(0, p // 2))
            wp[r, k:k + int(rng.integers(1, 9))] = 0
    return c, np.zeros((R, n), f32), cp, wp.astype(f32)


class RenderCase(NamedTuple):
    deltas: np.ndarray
    densities: np.ndarray
    rgb: np.ndarray
    thermal: np.ndarray
    accumulation: np.ndarray
    d_rgb: np.ndarray
    d_thermal: np.ndarray
    d_accumulation: np.ndarray
    d_weights: np.ndarray
    starts: np.ndarray
    ends: np.ndarray


def render_case(R: int, n: int, seed: int) -> RenderCase:
    """ray r mod 9: 0 generic, 1 empty (all density 0), 2 saturates in the first samples (E in the hundreds, T underflows behind),
    3 / 4 / 5 / 6 one dense sample at index 0 / 63 / 64 / n - 1 (clamped into the ray), 7 density only in the last chunk, 8 generic
    with delta = 0 samples and a large delta on the last sample.  starts / ends: mid-points above 1, below 1 and (sample 1 of the even rays) exactly 0."""
    rng = np.random.default_rng(seed)
    deltas = (rng.random((R, n)) * 0.2).astype(f32)
    dens = (rng.random((R, n)) * 4).astype(f32)
    for r in range(R):
        kind = r % 9
        if kind == 1:
            dens[r] = 0
        elif kind == 2:
            dens[r, :min(n, 6)] *= 400
        elif kind in (3, 4, 5, 6):
            dens[r] = 0
            dens[r, min({3: 0, 4: 63, 5: 64, 6: n - 1}[kind], n - 1)] = 50.0
        elif kind == 7:
            dens[r, :((n - 1) // 64) * 64] = 0
        elif kind == 8:
            deltas[r, rng.random(n) < 0.3] = 0
            deltas[r, -1] = 1000.0
    starts = (rng.random((R, n)) * 1.6).astype(f32)
    ends = (starts + deltas).astype(f32)
    starts[::2, min(1, n - 1)] = 0
    ends[::2, min(1, n - 1)] = 0
    w = render_adjoint(deltas, dens).weights
    return RenderCase(deltas, dens, rng.random((R, n, 3)).astype(f32), rng.random((R, n)).astype(f32), w.sum(1).astype(f32),
                      rng.standard_normal((R, 3)).astype(f32), rng.standard_normal(R).astype(f32),
                      rng.standard_normal(R).astype(f32), rng.standard_normal((R, n)).astype(f32), starts, ends)
