"""fp64 reference of the eval field pass (tn_field_render_fwd / tn_field_render_chunked_fwd) ray by ray, with a running error bound
beside every value, a family of inputs on which every kernel form must be EXACT, fp32 emulations of the two associations the
kernels composite in, and the faults tests/test_field_eval_reference_cpu.py plants — numpy, no device.  The sibling of
tests/mlp_reference.py and tests/ray_forward_reference.py for the path bench.py reports.

Frozen inputs.  The reference starts from the DEVICE's fp32 spacing edges of the final level (tn_proposal_sample_fwd's
spacing_bins[2]).  Euclidean edges, mid-points (step = fl32(st + en) / 2), deltas, sample positions and the normalised position p
are formed in fp32 exactly as the torch-order kernels form them (spacing_fn_fp32, spacing_to_eucl_fp32, frustum_positions_fp32 of
tests/ray_forward_reference.py, normalized() of tests/position_gradient_reference.py); the hash cell and the interpolation offsets
are frozen at fl32(p s) as in tests/position_gradient_reference.py.  Everything behind that is fp64.

FAST geometry.  The FAST kernels (every matrix-pipe form) replace two divisions of that geometry by v_rcp_f32: spacing_fn_inv for
u >= 0.5 under the piecewise sampler, and x / mag in the contraction for |x|_inf >= 1.  v_rcp_f32 is not correctly rounded, so those
bits cannot be frozen on the CPU.  ``Geo.fast_exact`` says, ray by ray, whether neither division is reached (uniform sampler or
far < 1, and contraction off or every sample inside the unit cube): there the FAST kernels form the bits above.  Elsewhere
``geometry(fast=True)`` BOUNDS what they may form instead: K_RCP (measured like the other fast operations) gives an error of every
such edge, hence of step (``Geo.e_step``), delta (``e_delta``) and the sample position; the contraction (3-Lipschitz in the largest
norm) and its own v_rcp pass it on to p (``e_p``).  A position off by e_p moves a level's features by at most
(scale x e_p + 2 u |p scale|, the second term for the product's own rounding) x (the largest difference of two entries of that level's table): the features are continuous and piecewise trilinear, and
that slope holds in every cell, so a sample the FAST kernel puts in the neighbouring cell is covered.  At scale 2047 this term is
about 1e-3 of a feature: such rays' bounds are about 1e-2 under the FAST flavours, and the median depth and the clip's mid-points
are compared within e_step instead of bit for bit.  The torch-order kernel (main_valu_kernel) keeps the frozen geometry everywhere.

Bounds.  u = 2^-24; gamma(D) as in tests/mlp_reference.py.  Counted on the code as written:
  features.     frozen cell, exact offsets.  torch order: a o + b (1 - o), three roundings a stage; FAST: fmaf(o, a - b, b), two a
                stage (the dense x stage: the stored difference rounds once, the fmaf once).  With M = the largest |corner entry|
                of the cell, a stage's result is at most M, a difference at most 2 M: each stage adds at most 3 u M and passes what
                it carries through a convex combination: 9 u M after three stages, in either flavour.
  layers.       pre = b + sum x W: an fmaf / fp32-MFMA chain onto the bias, one rounding per NON-ZERO weight of the row (a zero
                product rounds nothing): gamma(nnz) B, B the absolute-value sum, plus what x carries through |W|.  mlp_head.0: the
                SH, geo and appearance columns are one chain in the torch-order kernel; the matrix forms fold the appearance
                product into the bias at prepare time and the SH product once per tile: the same steps in another order.  Output
                rows of the matrix forms: two half chains from zero, combine_halves, the bias: nnz + 2 is used for every form.
                The thermal hidden layer of main_mfma_rays_kernel is staged times -log2(e): one more rounding per term:
                nnz + 1.  ReLU is 1-Lipschitz, the sigmoid 1/4-Lipschitz.
                f16x3 / bf16x6: a per-product error of 2^-22 / 2^-23 relative (include/thermonerf_hip.h) and three / six partial
                products per step, each taken as one accumulation rounding (the assumption of tests/mlp_reference.py).
  exp.          expf: K_EXP u relative (tests/ray_losses_reference.py).  __expf, fast_sigmoid, fast_sigmoid_prescaled: ROCm states
                no bound; K_FEXP_A + K_FEXP_B |x| (relative), K_FSIG and K_FSIG_PRE (absolute) are MEASUREMENTS — the worst of 10^7
                arguments a range against host fp64 (tools/micro/libm_accuracy.hip, profiles/micro/libm_accuracy.txt) times two,
                rounded up.  An argument's own bound e passes through exp as v (e^e - 1).
  density.      (avg exp(raw)) sel: two products.
  weights.      dd = delta density: one rounding.  The optical depth before sample i: at most i + K additions (K segments).
                w = (1 - E1) E2: the subtraction, the product; sample-split: w = T_j w_local, one more product, and T_j's exponent is
                the sum of the segments' depths.
  sums.         S + K + 2 additions at the most (accumulation, colours, thermal, sum w step), a product each.
  background.   c_last (1 - sum w): the subtraction, the product, the addition.  Clamps and the clip are 1-Lipschitz.
  expected.     (sum w step) / (sum w + 1e-10): the addition, the division; where the denominator is not above its own bound the
                quotient is bounded by the clip interval alone.
  median.       decided by the fp64 cumulative weight where it is further than its bound from 0.5 at EVERY sample; ``med_ok`` marks
                the rays for which that holds, and the builders of the GPU tests redraw the others.  No ray is excused.

Exact family (first hit).  contraction off with a small box, mlp_base.1's density row zero with bias 60, mlp_head.2 zero with zero
bias, the thermal head's weight zero with a dyadic bias b: a sample's density is avg exp(60) inside the box and exactly 0 outside,
its colour fast_sigmoid(0) = 1/2 and its thermal b.  The first in-box sample then has weight exactly 1 and every other sample
exactly 0, in every association; ``first_hit_rays`` builds rays whose first in-box sample is a GIVEN index, from per-ray edges,
and asserts its premises on the fp32 geometry.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from tests import mlp_reference as M
from tests import position_gradient_reference as PG
from tests import ray_forward_reference as RF
from tests.ray_losses_reference import K_EXP

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY32 = 2.0 ** -126
FLT_MAX = float(np.finfo(f32).max)
GF, APP, LEVELS = 15, 32, 16
IN0 = 16 + GF + APP
SENTINEL = 7.0

# MEASURED (profiles/micro/libm_accuracy.txt, an MI355X): worst of 10^7 arguments a range against host fp64, times 2, rounded up
K_FEXP_A, K_FEXP_B = 5.0, 3.0   # __expf(x), x in [-87, 30]: relative error <= (A + B |x|) u; measured a = 2.02, b = 1.19
K_FEXP_TINY = 2.0               # __expf(x), x in [-104, -87): absolute, in 2^-126; measured 1.0
K_FSIG = 4.0                    # v_rcp(1 + __expf(-x)): absolute, in u; measured 1.81
K_FSIG_PRE = 4.0                # v_rcp(1 + v_exp(a)): absolute, in u; measured 1.83
K_RCP = 4.0                     # v_rcp_f32(x), x in [2^-20, 2^20]: relative, in u; measured 1.53
FEXP_MAX_ARG = 30.0             # the largest argument the __expf measurement covers


class Flavour(NamedTuple):
    name: str
    fast: bool        # FAST geometry and interpolation, __expf in the density and the weights
    sig_rgb: str      # "libm" | "fast"
    sig_th: str       # "libm" | "fast" | "prescaled"
    product: float    # per-product relative error of a matrix product, in u
    chain: int        # accumulation roundings per product


VALU = Flavour("valu", False, "libm", "libm", 0.0, 1)       # main_valu_kernel
MFMA = Flavour("mfma", True, "libm", "libm", 0.0, 1)        # main_mfma_kernel (one ray per wave)
RAYS = Flavour("rays", True, "fast", "prescaled", 0.0, 1)   # main_mfma_rays_kernel, field_records_kernel
F16X3 = Flavour("f16x3", True, "fast", "fast", 4.0, 3)      # main_split_rays_kernel
BF16X6 = Flavour("bf16x6", True, "fast", "fast", 2.0, 6)
WIDEST = Flavour("widest", True, "fast", "prescaled", 4.0, 6)   # no kernel: the largest of every count, for the median redraw

PARAMS = ("base0_w", "base0_b", "base1_w", "base1_b", "head0_w", "head0_b", "head1_w", "head1_b", "head2_w", "head2_b",
          "th0_w", "th0_b", "th1_w", "th1_b", "thead_w", "thead_b")
SHAPES = dict(base0_w=(64, 32), base0_b=(64,), base1_w=(16, 64), base1_b=(16,), head0_w=(64, IN0), head0_b=(64,), head1_w=(64, 64),
              head1_b=(64,), head2_w=(3, 64), head2_b=(3,), th0_w=(64, GF), th0_b=(64,), th1_w=(64, 64), th1_b=(64,),
              thead_w=(1, 64), thead_b=(1,))


class Field(NamedTuple):
    table: np.ndarray       # [16 T, 2] fp32
    scalings: np.ndarray    # [16] fp32
    log2T: int
    w: Dict[str, np.ndarray]
    emb: np.ndarray         # [num_images, 32] fp32
    contraction: bool
    aabb: np.ndarray        # [2, 3] fp32
    avg: float
    sh_shifted: bool
    use_avg: bool


def _w(x):
    return np.asarray(x, dtype=f64)


def scalings16(base: int = 16, top: int = 2048) -> np.ndarray:
    """NS HashEncoding's per-level scalings, floor(base growth^l), as fp32"""
    growth = np.exp((np.log(top) - np.log(base)) / (LEVELS - 1))
    return np.floor(base * growth ** np.arange(LEVELS)).astype(f32)


def random_field(seed: int, log2T: int = 11, contraction: bool = True, aabb=None, sh_shifted: bool = True, use_avg: bool = True,
                 num_images: int = 5, avg: float = 1.0) -> Field:
    """sparse Gaussian weights: a row keeps max(4, fan / 8) entries, sized so that its absolute sum is about 2.  A bound carried
    through a layer grows by that sum, so dense O(1) rows would make the last layer's bound ten thousand times its first's; the
    pre-activations stay O(1) and |raw density| far below FEXP_MAX_ARG"""
    r = np.random.default_rng(seed)
    w = {}
    for k in PARAMS:
        shape = SHAPES[k]
        if len(shape) == 1:
            w[k] = (r.standard_normal(shape) * 0.3).astype(f32)
            continue
        nnz = max(4, shape[1] // 8)
        m = np.zeros(shape)
        for row in range(shape[0]):
            cols = r.choice(shape[1], nnz, replace=False)
            m[row, cols] = r.standard_normal(nnz) * (2.0 / (0.8 * nnz))
        w[k] = m.astype(f32)
    w["base0_w"] = (w["base0_w"] * 2.0).astype(f32)   # the features are O(0.3)
    w["base1_w"][0] *= f32(5.0)                        # raw densities over a few e-folds: opaque and empty rays both occur
    w["thead_w"] = (w["thead_w"] * 0.25).astype(f32)   # thermal = 1/2 + O(0.2): the eval clamp to [0, 1] stays out of the way
    w["thead_b"] = np.array([0.5], f32)
    table = (r.uniform(-1.0, 1.0, (LEVELS << log2T, 2)) * 0.6).astype(f32)
    emb = r.standard_normal((num_images, APP)).astype(f32)
    box = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], f32) if aabb is None else np.asarray(aabb, f32)
    return Field(table, scalings16(), log2T, w, emb, contraction, box, avg, sh_shifted, use_avg)


# ----------------------------------------------------------------------------------------------------------------------
# geometry, fp32 as the torch-order kernels form it
# ----------------------------------------------------------------------------------------------------------------------
class Geo(NamedTuple):
    st: np.ndarray      # [R, S] fp32
    en: np.ndarray
    step: np.ndarray    # mid-points
    delta: np.ndarray   # fl(en - st)
    pos: np.ndarray     # [R, S, 3] fp32
    p32: np.ndarray     # [R S, 3] fp32 normalised, times the selector
    sel: np.ndarray     # [R S] bool
    fast_exact: np.ndarray   # [R] bool: the FAST kernels form the same bits (see the module's docstring)
    # how far a FAST kernel's fp32 values may lie from the ones above (None = nowhere: the torch-order kernel, or fast_exact rays)
    e_step: Optional[np.ndarray] = None    # [R, S]
    e_delta: Optional[np.ndarray] = None   # [R, S]
    e_p: Optional[np.ndarray] = None       # [R S, 3]


def geometry(field: Field, origins, directions, nears, fars, spacing, lin: bool, fast: bool = False) -> Geo:
    """fast: also bound what the FAST kernels' two v_rcp_f32 divisions move (module docstring, "FAST geometry")"""
    spacing = np.asarray(spacing, f32)
    sn, sf = RF.spacing_fn_fp32(nears, lin), RF.spacing_fn_fp32(fars, lin)
    eucl = RF.spacing_to_eucl_fp32(spacing, sn, sf, lin)
    pos, st, en, delta = RF.frustum_from_edges_fp32(origins, directions, eucl)
    step = RF.midpoints_fp32(st, en)
    p32, sel = PG.normalized(pos.reshape(-1, 3), PG.Space(field.contraction, field.aabb))
    u = ((spacing * sf.reshape(-1, 1)).astype(f32) + ((f32(1) - spacing).astype(f32) * sn.reshape(-1, 1)).astype(f32)).astype(f32)
    ok = np.ones(spacing.shape[0], bool) if lin else np.all(u < f32(0.5), axis=1)
    if field.contraction:
        ok &= np.all(np.abs(pos).max(-1) < f32(1), axis=1)
    g = Geo(st, en, step, delta, pos, p32, np.asarray(sel, bool), ok)
    if not fast or ok.all():
        return g
    # an edge with u >= 0.5 is v_rcp(2 - 2 u) against the correctly rounded quotient: (K_RCP + 1/2) u relative, rounded up
    e_edge = np.zeros(eucl.shape) if lin else np.where(u >= f32(0.5), (K_RCP + 1.0) * U * np.abs(_w(eucl)), 0.0)
    e_st, e_en = e_edge[:, :-1], e_edge[:, 1:]
    e_step = (e_st + e_en) / 2 + U * np.abs(_w(step))               # the sum rounds elsewhere
    e_delta = e_st + e_en + U * np.abs(_w(delta))
    d = np.abs(_w(directions))[:, None, :]
    e_pos = d * (e_st + e_en)[..., None] / 2 + 2 * U * d * np.abs(_w(step))[..., None] + U * np.abs(_w(pos))
    e_pos = np.where(((e_st + e_en) > 0)[..., None], e_pos, 0.0)    # (an exact edge pair gives the same position bits)
    if field.contraction:
        # c = (2 - 1 / m) x / m, m = |x|_inf >= 1: own-axis slope (2 - 1/m) / m <= 1, through m at most 2 |x| / m^2 <= 2: 3 in the
        # largest norm; v_rcp(m) in 2 - rinv ((K_RCP + 1) u, rinv <= 1 <= k), x rinv against x / m ((K_RCP + 2) u), the product: u
        c = 4.0 * _w(p32).reshape(pos.shape) - 2.0
        beyond = (np.abs(_w(pos)).max(-1) + e_pos.max(-1) >= 1.0)[..., None]
        e_c = 3.0 * e_pos.max(-1, keepdims=True) + np.where(beyond, (2 * K_RCP + 4.0) * U * np.abs(c), 0.0)
        e_p = e_c / 4 + np.where(e_c > 0, U * np.abs(_w(p32).reshape(pos.shape)), 0.0)
    else:
        e_p = e_pos / np.abs(_w(field.aabb[1]) - _w(field.aabb[0])) + np.where(e_pos > 0, 2 * U * np.abs(_w(p32).reshape(pos.shape)), 0.0)
    return g._replace(e_step=e_step, e_delta=e_delta, e_p=e_p.reshape(-1, 3))


# ----------------------------------------------------------------------------------------------------------------------
# the field in fp64
# ----------------------------------------------------------------------------------------------------------------------
def encode(field, p32: np.ndarray, fault: Optional[str] = None, e_p=None) -> Tuple[np.ndarray, np.ndarray]:
    """(enc [N, 32], e_enc [N, 32]): the sixteen levels on the frozen cells; fault "level_offset": level 3 reads level 4's table"""
    N, levels = p32.shape[0], len(field.scalings)
    enc, err = np.zeros((N, 2 * levels)), np.zeros((N, 2 * levels))
    for l in range(levels):
        fl, ce, off = PG.frozen_cell(p32, field.scalings[l])
        f = PG._corner_values(fl, ce, field.table, l + 1 if (fault == "level_offset" and l == 3) else l, field.log2T)
        ox, oy, oz = (off[:, c:c + 1] for c in range(3))
        (a03, b03), (a12, b12), (a56, b56), (a47, b47) = PG._pairs(f)
        f03, f12 = a03 * ox + b03 * (1 - ox), a12 * ox + b12 * (1 - ox)
        f56, f47 = a56 * ox + b56 * (1 - ox), a47 * ox + b47 * (1 - ox)
        enc[:, 2 * l:2 * l + 2] = (f03 * oy + f12 * (1 - oy)) * oz + (f47 * oy + f56 * (1 - oy)) * (1 - oz)
        err[:, 2 * l:2 * l + 2] = 9 * U * np.max(np.abs(np.stack(f)), axis=0)
        if e_p is not None:   # a position off by e_p: the features are continuous and piecewise trilinear, and no cell's slope along
            T = 1 << field.log2T   # an axis exceeds scale x (the largest difference of two entries of the level's table)
            tl = _w(field.table[l * T:(l + 1) * T])
            sc = f64(field.scalings[l])   # the moved position's own product p s rounds elsewhere: 2 u |p s| more on a moved axis
            e_off = (sc * e_p + np.where(e_p > 0, 2 * U * sc * np.abs(_w(p32)), 0.0)).sum(1, keepdims=True)
            err[:, 2 * l:2 * l + 2] += e_off * (tl.max(0) - tl.min(0))[None, :]
    return enc, err


def _layer(x, e_x, W, b, extra: int, fl: Flavour):
    """pre-activation and its bound: one chain step per NON-ZERO weight of the row (a zero product rounds nothing) onto the bias,
    ``extra`` further roundings"""
    W, b = _w(W), _w(b)
    pre = x @ W.T + b
    prod = np.abs(x) @ np.abs(W).T
    d = ((W != 0).sum(1) * fl.chain + extra) * U
    e = e_x @ np.abs(W).T + d / (1.0 - d) * (prod * (1.0 + (2.0 ** -6 if fl.chain > 1 else 0.0)) + np.abs(b)) + fl.product * U * prod
    return pre, e


def _exp(x, e_x, fast: bool):
    """exp(x) for an fp32 argument the kernel holds within e_x of x, and its bound"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = np.exp(x)
        k = (K_FEXP_A + K_FEXP_B * np.abs(x)) if fast else K_EXP
        grow = np.expm1(np.minimum(e_x, 700.0))   # (the exact family's densities: its bounds are not used)
        return v, v * (grow + k * U * (1.0 + grow)) + (K_FEXP_TINY if fast else 1.0) * TINY32


def _sigmoid(pre, e_pre, kind: str):
    s = 1.0 / (1.0 + np.exp(-pre))
    if kind == "libm":   # 1 / (1 + expf(-x)): tests/mlp_reference.py's count, the carried part through the Lipschitz constant
        return s, 0.25 * e_pre + s * ((1.0 - s) * K_EXP * U + 2 * U) + TINY32
    return s, 0.25 * e_pre + (K_FSIG_PRE if kind == "prescaled" else K_FSIG) * U


def appearance_fp32(field: Field, fault: Optional[str] = None) -> np.ndarray:
    """the eval appearance vector exactly as stage_heads / field_prepare_kernel form it: a sequential fp32 sum over the images and
    one division, or zeros"""
    if not field.use_avg or fault == "appearance_zeros":
        return np.zeros(APP, f32)
    m = np.zeros(APP, f32)
    for im in range(field.emb.shape[0]):
        m = (m + field.emb[im]).astype(f32)
    return (m / f32(field.emb.shape[0])).astype(f32)


def sh16(directions, shifted: bool, fp64: bool = False) -> np.ndarray:
    if not fp64:
        return M.sh16_fp32(directions, shifted).astype(f64)
    d = _w(directions)
    d = (d + 1.0) / 2.0 if shifted else d
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    c = np.empty((d.shape[0], 16))
    c[:, 0] = 0.28209479177387814
    c[:, 1], c[:, 2], c[:, 3] = 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x
    c[:, 4], c[:, 5], c[:, 7] = 1.0925484305920792 * x * y, 1.0925484305920792 * y * z, 1.0925484305920792 * x * z
    c[:, 6] = 0.9461746957575601 * zz - 0.31539156525251999
    c[:, 8] = 0.5462742152960396 * (xx - yy)
    c[:, 9] = 0.5900435899266435 * y * (3 * xx - yy)
    c[:, 10] = 2.890611442640554 * x * y * z
    c[:, 11] = 0.4570457994644658 * y * (5 * zz - 1)
    c[:, 12] = 0.3731763325901154 * z * (5 * zz - 3)
    c[:, 13] = 0.4570457994644658 * x * (5 * zz - 1)
    c[:, 14] = 1.445305721320277 * z * (xx - yy)
    c[:, 15] = 0.5900435899266435 * x * (xx - 3 * yy)
    return c


class Samples(NamedTuple):
    density: np.ndarray     # [N]
    rgb: np.ndarray         # [N, 3]
    thermal: np.ndarray     # [N]
    e_density: np.ndarray
    e_rgb: np.ndarray
    e_thermal: np.ndarray
    raw: np.ndarray         # [N] the density row of mlp_base.1
    e_raw: np.ndarray
    geo: np.ndarray         # [N, 15]
    e_geo: np.ndarray


FIELD_FAULTS = ("sh_shifted_ignored", "appearance_zeros", "level_offset", "no_selector")


def nan_to_num(x):
    return np.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)


class Heads(NamedTuple):
    rgb: np.ndarray        # [N, 3]
    thermal: np.ndarray    # [N]
    e_rgb: np.ndarray
    e_thermal: np.ndarray


def field_heads(field: Field, geo, e_geo, sh, app, fl: Flavour = VALU) -> Heads:
    """mlp_head and the thermal branch on given geo features [N, 15] (bound e_geo), SH components [N, 16] and appearance vectors
    [N, 32] (both exact fp32 inputs); before the renderers' nan_to_num"""
    w = field.w
    x0 = np.concatenate([sh, geo, app], axis=1)
    e_x0 = np.concatenate([np.zeros_like(sh), e_geo, np.zeros_like(app)], axis=1)
    c1, e_c1 = _layer(x0, e_x0, w["head0_w"], w["head0_b"], 0, fl)
    c2, e_c2 = _layer(np.maximum(c1, 0.0), e_c1, w["head1_w"], w["head1_b"], 0, fl)
    c3, e_c3 = _layer(np.maximum(c2, 0.0), e_c2, w["head2_w"], w["head2_b"], 2, fl._replace(product=0.0, chain=1))
    rgb, e_rgb = _sigmoid(c3, e_c3, fl.sig_rgb)
    t1, e_t1 = _layer(geo, e_geo, w["th0_w"], w["th0_b"], 0, fl)
    t2, e_t2 = _layer(np.maximum(t1, 0.0), e_t1, w["th1_w"], w["th1_b"], 1 if fl.sig_th == "prescaled" else 0, fl)
    s2, e_s2 = _sigmoid(t2, e_t2, fl.sig_th)
    th, e_th = _layer(s2, e_s2, w["thead_w"], w["thead_b"], 2, fl._replace(product=0.0, chain=1))
    return Heads(rgb, th[:, 0], e_rgb, e_th[:, 0])


def field_samples(field: Field, p32, sel, directions, ray_of, fl: Flavour = VALU, fault: Optional[str] = None,
                  sh_fp64: bool = False, e_p=None) -> Samples:
    """the four sample values of N samples: p32 [N, 3] normalised positions (times the selector), sel [N], directions [R, 3],
    ray_of [N] the ray of each sample"""
    w = field.w
    enc, e_enc = encode(field, np.asarray(p32, f32), fault, e_p if fl.fast else None)
    a0, e_a0 = _layer(enc, e_enc, w["base0_w"], w["base0_b"], 0, fl)
    o, e_o = _layer(np.maximum(a0, 0.0), e_a0, w["base1_w"], w["base1_b"], 0, fl)
    raw, e_raw = o[:, 0], e_o[:, 0]
    ex, e_ex = _exp(raw, e_raw, fl.fast)
    selv = np.ones(len(raw)) if fault == "no_selector" else _w(sel)
    density = f64(field.avg) * ex * selv
    e_density = (abs(field.avg) * e_ex + 2 * U * np.abs(f64(field.avg) * ex)) * selv
    geo, e_geo = o[:, 1:], e_o[:, 1:]
    sh = sh16(directions, field.sh_shifted and fault != "sh_shifted_ignored", sh_fp64)[ray_of]
    app = np.broadcast_to(appearance_fp32(field, fault).astype(f64), (len(raw), APP))
    h = field_heads(field, geo, e_geo, sh, app, fl)
    return Samples(density, nan_to_num(h.rgb), nan_to_num(h.thermal), e_density, h.e_rgb, h.e_thermal, raw, e_raw, geo, e_geo)


class GridRef(NamedTuple):
    table: np.ndarray
    scalings: np.ndarray
    log2T: int


def proposal_density(grid: GridRef, w0, b0, w1, b1, avg: float, p32, sel):
    """tn_density_fwd (hidden 16 or 64): (density [N], bound): expf, two products"""
    enc, e_enc = encode(grid, np.asarray(p32, f32))
    a0, e_a0 = _layer(enc, e_enc, w0, b0, 0, VALU)
    o, e_o = _layer(np.maximum(a0, 0.0), e_a0, w1, b1, 0, VALU)
    ex, e_ex = _exp(o[:, 0], e_o[:, 0], False)
    return f64(avg) * ex * _w(sel), (abs(avg) * e_ex + 2 * U * np.abs(f64(avg) * ex)) * _w(sel)


# ----------------------------------------------------------------------------------------------------------------------
# the eval renderers in fp64
# ----------------------------------------------------------------------------------------------------------------------
class Rendered(NamedTuple):
    rgb: np.ndarray           # [R, 3]
    thermal: np.ndarray       # [R]
    accumulation: np.ndarray
    depth: np.ndarray         # median
    expected_depth: np.ndarray       # clipped
    expected_unclipped: np.ndarray
    weights: np.ndarray       # [R, S]
    tol: Dict[str, np.ndarray]       # by output name
    med_index: np.ndarray     # [R]
    med_ok: np.ndarray        # [R] bool: the fp64 cumulative weight is further than its bound from 0.5 at every sample
    bounds: np.ndarray        # [slots, 2] fp32 (min, max) of the mid-points of the call / of each chunk
    slot_of: np.ndarray       # [R]


def segment_len(S: int, k: int) -> int:
    return -(-S // max(k, 1))


def depth_bounds(step, first_ray: int = 0, chunk_rays: int = 0, fault: Optional[str] = None, live=None):
    """([slots, 2] fp32, slot of every ray); chunk_rays 0: one pair for the call.  Faults: "chunk_slot" (ray -> chunk off by one
    ray), "minmax_live" (over the samples with a non-zero weight only)"""
    step = np.asarray(step, f32)
    R = step.shape[0]
    r = np.arange(R)
    if chunk_rays:
        slot = (first_ray + r + (1 if fault == "chunk_slot" else 0)) // chunk_rays - first_ray // chunk_rays
        slot = np.minimum(slot, (first_ray + R - 1) // chunk_rays - first_ray // chunk_rays)
    else:
        slot = np.zeros(R, np.int64)
    out = np.empty((int(slot.max()) + 1, 2), f32)
    for s in range(out.shape[0]):
        rows = step[slot == s]
        if fault == "minmax_live" and live is not None and live[slot == s].any():
            rows = rows[live[slot == s]]
        out[s] = rows.min(), rows.max()
    true_slot = (first_ray + r) // chunk_rays - first_ray // chunk_rays if chunk_rays else slot
    return out, true_slot


def render(s: Samples, g: Geo, fl: Flavour = VALU, split: int = 1, first_ray: int = 0, chunk_rays: int = 0) -> Rendered:
    """split: the number of sample segments of the sample-split form (segments of segment_len(S, split) samples); 1 = serial"""
    R, S = g.step.shape
    K = 1
    seg = S
    if split > 1:
        seg = segment_len(S, split)
        K = -(-S // seg)
    delta, step = _w(g.delta), _w(g.step)
    dens, e_dens = s.density.reshape(R, S), s.e_density.reshape(R, S)
    c, e_c = s.rgb.reshape(R, S, 3), s.e_rgb.reshape(R, S, 3)
    th, e_th = s.thermal.reshape(R, S), s.e_thermal.reshape(R, S)
    moved = fl.fast and g.e_step is not None
    e_step = g.e_step if moved else np.zeros((R, S))
    e_delta = g.e_delta if moved else np.zeros((R, S))
    dd = delta * dens
    e_dd = np.abs(delta) * e_dens + e_delta * (np.abs(dens) + e_dens) + U * np.abs(dd)
    idx = np.arange(S)
    seg_of = idx // seg
    E1, e_E1 = _exp(-dd, e_dd, fl.fast)
    om, e_om = 1.0 - E1, e_E1 + U * np.abs(1.0 - E1)
    before = np.cumsum(dd, axis=1) - dd
    e_before = np.cumsum(e_dd, axis=1) - e_dd + M.gamma(S + K) * np.abs(before)
    if K == 1:
        E2, e_E2 = _exp(-before, e_before, fl.fast)
        w = om * E2
        e_w = e_om * E2 + om * e_E2 + e_om * e_E2 + U * np.abs(w)
    else:
        start = before[:, seg_of * seg]                      # the optical depth in front of the sample's segment
        e_start = e_before[:, seg_of * seg]
        local, e_local = before - start, e_before + e_start   # (the local sum has no more roundings than the whole one)
        E2, e_E2 = _exp(-local, e_local, fl.fast)
        T, e_T = _exp(-start, e_start, fl.fast)
        wl = om * E2
        e_wl = e_om * E2 + om * e_E2 + e_om * e_E2 + U * np.abs(wl)
        w = T * wl
        e_w = e_T * wl + T * e_wl + e_T * e_wl + U * np.abs(w)
    w, e_w = nan_to_num(w), np.where(np.isfinite(e_w), e_w, 0.0)
    gs = M.gamma(S + K + 2)
    acc = w.sum(1)
    e_acc = e_w.sum(1) + gs * acc
    bg, e_bg = 1.0 - acc, e_acc + U * np.abs(1.0 - acc)

    def composite(v, e_v):
        tot = (w * v).sum(1)
        e_tot = (e_w * np.abs(v) + w * e_v + e_w * e_v).sum(1) + gs * (w * np.abs(v)).sum(1)
        last, e_last = v[:, -1], e_v[:, -1]
        term = last * bg
        e_term = e_last * np.abs(bg) + np.abs(last) * e_bg + e_last * e_bg + U * np.abs(term)
        out = tot + term
        return np.clip(out, 0.0, 1.0), e_tot + e_term + U * np.abs(out)

    rgb, e_rgb = np.empty((R, 3)), np.empty((R, 3))
    for k in range(3):
        rgb[:, k], e_rgb[:, k] = composite(c[:, :, k], e_c[:, :, k])
    thermal, e_thermal = composite(th, e_th)
    cum = np.cumsum(w, axis=1)
    e_cum = np.cumsum(e_w, axis=1) + gs * cum
    med_ok = np.all(np.abs(cum - 0.5) > e_cum, axis=1)
    hit = cum >= 0.5
    med_index = np.where(hit.any(1), hit.argmax(1), S - 1)
    depth = step[np.arange(R), med_index]
    num = (w * step).sum(1)
    e_num = (e_w * step + (w + e_w) * e_step).sum(1) + gs * num
    den = f64(f32(1e-10)) + acc
    e_den = e_acc + U * den
    q = num / den
    with np.errstate(divide="ignore", invalid="ignore"):
        e_q = np.where(den > 2 * e_den, (e_num + np.abs(q) * e_den) / (den - e_den) + U * np.abs(q), np.inf)
    bounds, slot_of = depth_bounds(g.step, first_ray, chunk_rays)
    lo, hi = _w(bounds[slot_of, 0]), _w(bounds[slot_of, 1])
    expected = np.clip(q, lo, hi)
    e_clip = e_step.max(1)   # (what the clip's own two mid-points may have moved by: zero unless the FAST geometry differs)
    e_expected = np.minimum(e_q, hi - lo) + e_clip
    tol = dict(rgb=e_rgb, thermal=e_thermal, accumulation=e_acc, depth=e_step[np.arange(R), med_index], expected_depth=e_expected,
               expected_unclipped=e_q, weights=e_w)
    return Rendered(rgb, thermal, acc, depth, expected, q, w, tol, med_index, med_ok, bounds, slot_of)


OUTPUTS = ("rgb", "thermal", "accumulation", "depth", "expected_depth")


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(np.asarray(want, f64).astype(f32))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~((got == 0) & (want == 0))
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def judge(name: str, ref: Rendered, got: Dict[str, np.ndarray], outputs: Sequence[str] = OUTPUTS, exact: bool = False) -> Dict[str, float]:
    """every ray of every output inside its bound (the median depth: the same bits, for EVERY ray — the builders redraw the rays
    with ``med_ok`` False beforehand and assert that none is left); returns the worst ratio to the bound by output"""
    worst = {}
    if "depth" in outputs and not exact:
        assert ref.med_ok.all(), (name, "a ray within its bound of the median split was not redrawn", np.flatnonzero(~ref.med_ok)[:8])
    for k in outputs:
        want = getattr(ref, k)
        have = np.asarray(got[k], f32)
        assert have.shape == want.shape, (name, k, have.shape, want.shape)
        if exact or (k == "depth" and not np.any(ref.tol["depth"])):
            same_bits(f"{name} {k}", have, want)
            worst[k] = 0.0
            continue
        assert np.all(np.isfinite(have)), (name, k)
        err = np.abs(have.astype(f64) - want)
        tol = ref.tol[k] + U * np.abs(want)   # the store's own rounding of the fp64 value
        ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
        worst[k] = float(ratio.max()) if ratio.size else 0.0
        assert np.all(err <= tol), (name, k, worst[k], np.unravel_index(int(ratio.argmax()), ratio.shape))
    print(f"{name}: worst |device - fp64| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    return worst


def fails(fn, *args, **kw) -> bool:
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the two associations (the serial march and the sample-split records + combine), with planted faults
# ----------------------------------------------------------------------------------------------------------------------
MARCH_FAULTS = ("seam_sample_dropped", "T_not_applied_to_thermal", "no_thermal_background", "median_off_by_one", "minmax_live",
                "chunk_slot")


def _e32(x):
    return RF.exp32(x)


def march_fp32(delta, density, rgb, thermal, step, split: int = 1, fault: Optional[str] = None, first_ray: int = 0,
               chunk_rays: int = 0) -> Dict[str, np.ndarray]:
    """the statements of main_mfma_rays_kernel (split 1) or of its SPLIT form + segments_combine_kernel in fp32, exp correctly
    rounded; all inputs fp32 [R, S] ([R, S, 3])"""
    delta, density, th, step = (np.asarray(a, f32) for a in (delta, density, thermal, step))
    rgb = np.asarray(rgb, f32)
    R, S = delta.shape
    seg = segment_len(S, split) if split > 1 else S
    K = -(-S // seg)
    vals = np.concatenate([rgb, th[..., None], step[..., None]], axis=2)    # r g b th step
    one = f32(1)
    wsum_g = np.zeros(R, f32)
    sums_g = np.zeros((R, 5), f32)
    depth_so_far = np.zeros(R, f32)
    med = np.zeros(R, f32)
    med_found = np.zeros(R, bool)
    weights = np.zeros((R, S), f32)
    for j in range(K):
        s0, s1 = j * seg, min(j * seg + seg, S)
        accum, cum_w, wsum = np.zeros(R, f32), np.zeros(R, f32), np.zeros(R, f32)
        sums = np.zeros((R, 5), f32)
        cums = np.zeros((R, s1 - s0), f32)
        with np.errstate(over="ignore", invalid="ignore"):
            T = _e32(-depth_so_far) if K > 1 else np.ones(R, f32)
            T = np.where(np.isnan(T), f32(0), T).astype(f32)
            for i in range(s0, s1):
                dd = (delta[:, i] * density[:, i]).astype(f32)
                wi = RF.nan_to_num32(((one - _e32(-dd)).astype(f32) * _e32(-accum)).astype(f32))
                if fault == "seam_sample_dropped" and i == seg and S > seg:
                    wi = np.zeros(R, f32)
                accum = (accum + dd).astype(f32)
                cum_w = (cum_w + wi).astype(f32)
                cums[:, i - s0] = cum_w
                wsum = (wsum + wi).astype(f32)
                sums = (sums + (wi[:, None] * vals[:, i]).astype(f32)).astype(f32)
                weights[:, i] = (T * wi).astype(f32) if K > 1 else wi
            total = (wsum_g + (T * wsum).astype(f32)).astype(f32) if K > 1 else wsum
            glob = (wsum_g[:, None] + (T[:, None] * cums).astype(f32)).astype(f32) if K > 1 else cums
            crossing = glob >= f32(0.5)
            if K > 1:   # the combine pass searches only a segment whose TOTAL reaches 0.5, and stops at its last sample
                crossing[:, -1] |= total >= f32(0.5)
                crossing &= (total >= f32(0.5))[:, None]
            first = crossing.argmax(1)
            if fault == "median_off_by_one":
                first = np.minimum(first + 1, s1 - s0 - 1)
            found = crossing.any(1) & ~med_found
            med = np.where(found, step[np.arange(R), s0 + first], med).astype(f32)
            med_found |= found
            Tv = np.repeat(T[:, None], 5, axis=1)
            if fault == "T_not_applied_to_thermal" and j > 0:
                Tv[:, 3] = one
            sums_g = (sums_g + (Tv * sums).astype(f32)).astype(f32) if K > 1 else sums
            wsum_g = total
            depth_so_far = (depth_so_far + accum).astype(f32)
    last = vals[:, S - 1]
    bg = (one - wsum_g).astype(f32)
    back = (last[:, :4] * bg[:, None]).astype(f32)
    if fault == "no_thermal_background":
        back[:, 3] = 0
    comp = np.clip((sums_g[:, :4] + back).astype(f32), f32(0), f32(1)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = (sums_g[:, 4] / (wsum_g + f32(1e-10)).astype(f32)).astype(f32)
    bounds, slot_of = depth_bounds(step, first_ray, chunk_rays, fault, live=weights > 0)
    clipped = np.minimum(np.maximum(expected, bounds[slot_of, 0]), bounds[slot_of, 1]).astype(f32)
    return dict(rgb=comp[:, :3], thermal=comp[:, 3], accumulation=wsum_g, depth=np.where(med_found, med, step[:, S - 1]).astype(f32),
                expected_depth=clipped, expected_unclipped=expected, weights=weights, bounds=bounds)


# ----------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------
class Rays(NamedTuple):
    origins: np.ndarray
    directions: np.ndarray
    nears: np.ndarray
    fars: np.ndarray


def random_rays(R: int, seed: int, inside: bool, near: float = 0.05, far: Optional[float] = None) -> Rays:
    """inside: origins within 0.25 of the centre and far = 0.6, so that every sample stays inside the unit cube and below the
    piecewise sampler's u = 0.5; else origins up to 1.5 out, far = 6: samples at and beyond |x|_inf = 1"""
    r = np.random.default_rng(seed)
    d = r.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    o = (r.uniform(-0.25, 0.25, (R, 3)) if inside else r.uniform(-1.5, 1.5, (R, 3))).astype(f32)
    far = (0.6 if inside else 6.0) if far is None else far
    return Rays(o, d, np.full(R, near, f32), np.full(R, far, f32))


def redraw(rays: Rays, which: np.ndarray, seed: int, inside: bool) -> Rays:
    fresh = random_rays(int(which.sum()), seed, inside, float(rays.nears[0]), float(rays.fars[0]))
    o, d = rays.origins.copy(), rays.directions.copy()
    o[which], d[which] = fresh.origins, fresh.directions
    return Rays(o, d, rays.nears, rays.fars)


# ----------------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------------
EXACT_THERMAL = 0.375
EXACT_RAW = 60.0
OVERFLOW_RAW = 100.0   # exp(100) is +inf in fp32: the density is inf inside the box and inf x 0 = NaN outside it
BOX = np.array([[0.25, -0.125, -0.125], [0.5, 0.125, 0.125]], f32)
FACE_MARGIN = 1e-5


def exact_field(seed: int, log2T: int = 10, sh_shifted: bool = True, use_avg: bool = True, raw: float = EXACT_RAW) -> Field:
    f = random_field(seed, log2T, contraction=False, aabb=BOX, sh_shifted=sh_shifted, use_avg=use_avg)
    w = dict(f.w)
    w["base1_w"] = w["base1_w"].copy()
    w["base1_w"][0] = 0
    w["base1_b"] = w["base1_b"].copy()
    w["base1_b"][0] = raw
    w["head2_w"], w["head2_b"] = np.zeros((3, 64), f32), np.zeros(3, f32)
    w["thead_w"], w["thead_b"] = np.zeros((1, 64), f32), np.array([EXACT_THERMAL], f32)
    return f._replace(w=w)


LOG2E32 = f32(1.4426950408889634)   # __expf(x) is v_exp_f32(fl32(x * 0x3fb8aa3b))


def tie_field(seed: int, avg: float) -> Field:
    """the exact field with raw density 0: a sample's density is exactly ``avg`` inside the box"""
    f = exact_field(seed)
    w = dict(f.w)
    w["base1_b"] = w["base1_b"].copy()
    w["base1_b"][0] = 0
    return f._replace(w=w, avg=float(f32(avg)))


def tie_density(delta0) -> Optional[float]:
    """an fp32 density a with fl32(fl32(delta0 a) log2(e)) = 1 exactly, so that __expf(-delta0 a) = v_exp_f32(-1) = 1/2 and the first
    sample's weight is 1/2 to the last bit (None if the few fp32 neighbours of 1 / (delta0 log2 e) hold none)"""
    delta0 = f32(delta0)
    a0 = f32(1.0) / (delta0 * LOG2E32)
    lo = a0
    for _ in range(16):
        lo = np.nextafter(lo, f32(0))
    a = lo
    for _ in range(33):
        if f32(f32(delta0 * a) * LOG2E32) == f32(1):
            return float(a)
        a = np.nextafter(a, f32(np.inf))
    return None


class FirstHit(NamedTuple):
    rays: Rays
    geo: Geo
    index: np.ndarray      # [R] the first in-box sample, -1 for a miss
    want: Dict[str, np.ndarray]
    bounds: np.ndarray
    weights: np.ndarray    # [R, S] exactly 0 / 1


def first_hit_rays(field: Field, spacing, nears, fars, lin: bool, targets: Sequence[int], seed: int, first_ray: int = 0,
                   chunk_rays: int = 0, overflow: bool = False) -> FirstHit:
    """rays whose first sample inside the box is targets[r] (-1: no sample inside), for the per-ray spacing edges [R, S + 1] the
    device made for these near / far planes (the edges must not depend on origin and direction: a uniform proposal density).
    overflow (a field of raw density OVERFLOW_RAW): every sample OUTSIDE the box has the density inf x 0 = NaN, so a ray whose
    sample 0 lies outside has a NaN optical depth from its first sample on and get_weights' nan_to_num zeroes every weight behind
    it — the box it enters later included; a ray whose sample 0 lies inside gives that sample the weight (1 - exp(-inf))
    exp(-0) = 1 and everything behind it 0 (exp(-inf) inside the box, NaN outside).  ``index`` is then 0 or -1 by that rule.
    Asserts: the fp32 geometry names that index; no sample position within FACE_MARGIN of a face; delta > 0 at the hit and
    delta density large enough that 1 - exp(-delta density) = 1 and exp(-delta density) = 0 in fp32"""
    assert not field.contraction
    spacing = np.asarray(spacing, f32)
    R, S = spacing.shape[0], spacing.shape[1] - 1
    assert len(targets) == R
    r = np.random.default_rng(seed)
    lo, hi = _w(field.aabb[0]), _w(field.aabb[1])
    size = hi - lo
    o, d = np.zeros((R, 3), f32), np.zeros((R, 3), f32)
    todo = np.ones(R, bool)
    index = np.asarray(targets, np.int64)
    sn, sf = RF.spacing_fn_fp32(nears, lin), RF.spacing_fn_fp32(fars, lin)
    eucl = RF.spacing_to_eucl_fp32(spacing, sn, sf, lin)
    step = _w(RF.midpoints_fp32(eucl[:, :-1], eucl[:, 1:]))
    for attempt in range(200):
        n = int(todo.sum())
        if n == 0:
            break
        rows = np.flatnonzero(todo)
        dd = r.standard_normal((n, 3)) * np.array([1.0, 0.15, 0.15])
        dd[:, 0] = np.abs(dd[:, 0]) + 0.5
        dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        face = np.stack([np.full(n, lo[0]), lo[1] + size[1] * r.uniform(0.3, 0.7, n), lo[2] + size[2] * r.uniform(0.3, 0.7, n)], 1)
        k = index[rows]
        kk = np.maximum(k, 0)
        t_in = np.where(kk > 0, 0.5 * (step[rows, np.maximum(kk - 1, 0)] + step[rows, kk]), 0.5 * step[rows, 0])
        oo = face - dd * t_in[:, None]
        oo[k < 0, 1] += 5.0 * size[1]
        dd[k < 0, 1] = np.abs(dd[k < 0, 1])
        o[rows], d[rows] = oo.astype(f32), dd.astype(f32)
        g = geometry(field, o[rows], d[rows], np.asarray(nears, f32)[rows], np.asarray(fars, f32)[rows], spacing[rows], lin)
        sel = g.sel.reshape(n, S)
        first = np.where(sel.any(1), sel.argmax(1), -1)
        pn = (_w(g.pos) - lo) / size
        near_face = np.any((np.abs(pn) < FACE_MARGIN) | (np.abs(pn - 1.0) < FACE_MARGIN), axis=(1, 2))
        good = (first == k) & ~near_face
        todo[rows[good]] = False
    assert not todo.any(), ("no ray found for", index[todo][:8])
    rays = Rays(o, d, np.asarray(nears, f32), np.asarray(fars, f32))
    g = geometry(field, o, d, rays.nears, rays.fars, spacing, lin)
    assert g.fast_exact.all()
    sel = g.sel.reshape(R, S)
    first = np.where(sel.any(1), sel.argmax(1), -1)
    assert np.array_equal(first, index)
    raw = float(field.w["base1_b"][0])
    assert raw == (OVERFLOW_RAW if overflow else EXACT_RAW) and np.all(_w(g.delta) >= 0)
    if overflow:
        assert np.isinf(RF.exp32(f32(raw))) and np.all(_w(g.delta)[sel] > 0)
        index = np.where(index == 0, 0, -1)
    hitr = np.flatnonzero(index >= 0)
    if not overflow:
        dd_hit = _w(g.delta)[hitr, index[hitr]] * f64(f32(field.avg) * RF.exp32(f32(raw)))
        assert np.all(dd_hit > 1000.0) and np.all(dd_hit * S < 1e37)
    weights = np.zeros((R, S))
    weights[hitr, index[hitr]] = 1.0
    bounds, slot_of = depth_bounds(g.step, first_ray, chunk_rays)
    hit = index >= 0
    want = dict(rgb=np.full((R, 3), 0.5), thermal=np.full(R, EXACT_THERMAL), accumulation=hit.astype(f64),
                depth=np.where(hit, _w(g.step)[np.arange(R), np.maximum(index, 0)], _w(g.step)[:, S - 1]),
                expected_depth=np.where(hit, _w(g.step)[np.arange(R), np.maximum(index, 0)], _w(bounds[slot_of, 0])))
    return FirstHit(rays, g, index, want, bounds, weights)


def seam_targets(S: int, ks: Sequence[int]) -> List[int]:
    """sample 0, S - 1, both sides of every segment seam of ks segments per tile, and a miss"""
    t = {0, S - 1}
    for k in ks:
        if k > 1:
            seg = segment_len(S, k)
            for j in range(1, -(-S // seg)):
                t.update((j * seg - 1, j * seg))
    return sorted(x for x in t if 0 <= x < S) + [-1]
