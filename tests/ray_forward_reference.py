"""fp64 references of the per-ray FORWARD kernels of the sampler / renderer chain, element by element, with the bounds they are
held to, fp32 op-by-op models with a selectable summation order and plantable faults, and builders of inputs on which the result
is EXACT in fp32 — numpy, no device.  The forward sibling of tests/ray_losses_reference.py, whose conventions and constants
(K_EXP, EPS32, TINY32, wave_scan_fp32) it imports.

* ``sample_pdf``       tn_sample_pdf (sample_pdf_kernel, tn_samplers.hip)
* ``weights``          tn_weights_fwd (weights_kernel) and the weights of tn_ray_render[_depth]_fwd (tn_train.hip)
* ``composite``        tn_composite_fwd, C = 1, 3, 4, training and eval
* ``depth``            tn_depth_fwd: accumulation, median, expected
* ``sample_initial_fp32``, ``frustum_positions_fp32``, ``frustum_from_edges_fp32``: a handful of correctly rounded operations each;
  the fp32 model IS the expectation, bit for bit.

All references take the fp32 inputs as given and widen them.  Where a kernel forms ONE correctly rounded fp32 value from inputs the
reference forms it in fp32 too and widens it: a_i = fl32(delta_i sigma_i), fl32(w_i + 0.01f), the mid-points fl32((s + e) / 2),
the draws fl32(u_j + fl32(rand / nb)).  The library is built with -ffp-contract=off: there is no fused multiply-add to model.

Bounds.  u = 2^-24.  Every K counts fp32 roundings on the longest dependency path of the kernel as written, first order in u; none
was tuned against device output.  c = ceil(n / 64) chunks.  A wave scan (wave_incl_scan, wave_sum) is 6 adds deep.  A lane's own
partial sum over its c elements is c - 1 adds (the first is onto 0: exact).

weights.  E_i = carry + excl_i.  excl_i: the chunk's scan (6).  carry is ACCUMULATED (carry += lane 63 of the scan), not summed
  from stored chunk totals as in the adjoint kernel: before chunk b it holds b totals and b - 1 roundings (the first add is onto 0).
  The add carry + excl (1; exact in chunk 0).  K_E(n) = 6 for n <= 64, else 6 + (c - 2) + 1 = c + 5 (21 at n = 1024, against the
  22 of the adjoint's form), relative to sum_{j<i} |a_j|.  weights_kernel and ray_render[_depth]_fwd_kernel are the same
  expressions (carry + excl against excl + carry: the same add).  Then, as the sibling derives it: T_i = expf(-E_i) is off by
  (K_E E_i + K_EXP) u relative, ea = expf(-a): K_EXP, w = (1 - ea) T:
  |dw_i| <= u (w_i (K_E E_i + K_EXP + 2) + K_EXP ea_i T_i) + 2^-126 (a flushed or denormal product).
  Pinned exactly (tolerance 0): a_i = 0 -> expf(-0) = 1, 1 - 1 = 0, w_i = 0; E_i = inf (behind a sample with a = inf, or NaN) ->
  expf = 0 or NaN, nan_to_num -> 0; a_i = NaN -> 0.  a_i = +inf with E_i finite: alpha = 1 exactly and w_i = T_i.

composite.  sum_i w_i v_i: product (1), lane partial (c - 1), wave_sum (6), the final add (1): c + 7 relative to sum |w v|.
  acc = sum w: c + 5 relative to sum |w|.  bg = 1 - acc (1), last * bg (1), the final add (1): 3 relative to |last| |bg|.
  |err| <= u ((c + 7) sum |w v| + |last| ((c + 5) sum |w| + 3 |1 - acc|)) + 2^-126.  The eval clamp is a contraction.

depth.  accumulation: c + 5 relative to sum |w|.  expected = num / den, num = sum w m (c + 6 relative to sum |w m|), den =
  acc + 1e-10f (c + 5 relative to sum |w|, + 1 of the add), the division (1):
  |err| <= u ((c + 6) sum |w m| / |den| + |num / den| ((c + 5) sum |w| / |den| + 2)) + 2^-126; the clip to the call's [min, max]
  mid-point (exact bounds: the mid-points are fp32 values of the reference as well) is a contraction.
  median: an index; its value is the fp32 mid-point of that sample, so a right index gives the right bits.  A device prefix is
  off by at most (6 + c - 1 + ...) < (7 + c) u prefix; ``depth_general_case`` walks seeds until no ray has an fp64 prefix within
  that of 0.5 at the reference index or its predecessor, so that no ray is excused.

sample_pdf.  The inverse CDF is continuous and piecewise linear in (cdf_k, bins_k).  A device CDF whose knots are off by at most d
  is off by at most d EVERYWHERE (linear interpolation of the knot errors), so the device sample b~ has F(b~) in [uu - d, uu + d]
  and |b~ - b| <= d times the steepest slope (b_k+1 - b_k) / (c_k+1 - c_k) among the bins whose CDF interval meets that range —
  a bin flip next to an edge is inside this or it is a failure.  d = K_CDF(n_in) u (the CDF is <= 1).  K_CDF: the two adds and the
  division of a pdf term (3); the relative error of ws: lane partial (c - 1), wave_sum (6), the padding add (1); the scan (6); the
  chunk carries (incl = scan + carry, c - 1):  K_CDF(n_in) = 3 + (c + 6) + 6 + (c - 1) = 2 c + 14  (16 up to 64, 46 at 1024).
  On top: t = fl(fl(uu - c0) / fl(c1 - c0)) (3 relative to t <= 1), b1 - b0 (1), the product (1): 5 |b1 - b0|; the add: 1 |b|.
  The clamp of t to [0, 1] cannot be observed on a sorted CDF: side="right" gives c0 <= uu < c1, rounding is monotone, so
  0 <= fl(uu - c0) <= fl(c1 - c0); outside the CDF both indices clamp to the same entry, t is NaN -> 0 or +-inf -> +-FLT_MAX and
  multiplies b1 - b0 = 0.  The CPU tests assert that the model without the clamp gives the same bits on every family.
  The clamp of the CDF to 1 is a rounding-level matter for weights >= 0 (the pdf sums to 1); the exact family carries one ray with
  a negative weight whose cumulative sum passes 1.5 before it returns to 1: only the clamp keeps that CDF sorted.
  Euclidean bins: spacing_to_eucl is x s_far + (1 - x) s_near in four correctly rounded operations and, for the piecewise map,
  2 u or 1.0f / (2 - 2 u) (t_rcp<false> is the IEEE quotient 1.0f / x: modelled, not counted).  The 1 / (2 - 2 s) map amplifies a
  spacing error by its derivative, so the euclidean bins are not bounded against fp64: they are held bit for bit to
  ``spacing_to_eucl_fp32`` of the SPACING BINS THE DEVICE RETURNED, which are themselves held to the bound above.

Exact families.
* PDF: every weight != 0 is m_i 2^40, m_i a (signed) power of two, sum m_i = M <= 1024 a power of two: fl32(w + 0.01f) = w, the
  padded sum is M 2^40 in any order, pdf_i = m_i / M, every CDF value a multiple of 1 / M.  The first weight is never 0 (leading
  zeros would make the CDF k fl32(0.01f / ws), which depends on the order); zero weights behind a non-zero one add about
  1e-14 / M each and are absorbed: the fp32 CDF is FLAT across them in any order.  The fp64 reference is asked for the same
  thing (``cdf_fp32=True``: every CDF entry rounded once to the kernel's storage format).  Existing bins are multiples of 2^-12,
  draws multiples of 2^-12 (u_j multiples of 2^-12, rand = nb q 2^-12 so that fl32(rand / nb) = q 2^-12), t = a 2^-12 / 2^-e a
  multiple of 2^-12, t (b1 - b0) a multiple of 2^-24 below 1: exact.  Contains draws equal to a CDF value at the start of a flat
  run (side="right": the edge behind the run; "left": the edge before it — the only place the two differ), draws equal to 1 and
  above 1, a draw of exactly 0, a flat run across the 64-entry chunk boundary.
* composite: weights multiples of 2^-10, values multiples of 2^-8 in [0, 1]: products multiples of 2^-18, sums below 2.
* depth: weights multiples of 2^-10 (a few negative), edges multiples of 2^-7 in [1, 17): every prefix, sum w m and 1 - acc exact;
  expected = fl32(num / fl32(acc + 1e-10f)) is two correctly rounded operations, modelled.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np

from tests.ray_losses_reference import EPS32, K_EXP, TINY32, render_case, wave_scan_fp32

f32, f64 = np.float32, np.float64
FLT_MAX = float(np.finfo(f32).max)
ORDERS = ("sequential", "pairwise", "wave")
N_EDGES = [1, 2, 63, 64, 65, 128, 129, 1024]   # sample counts n, n_in
R_EDGES = [1, 3, 4, 5, 37]                     # ray counts around the four rays of a block
N_OUT_EDGES = [1, 63, 64, 127, 300]            # n_out + 1 crosses 64 at 63
RAYS_PER_BLOCK = 4
DEPTH_GRID_CAP = 512                           # blocks of depth_kernel's ray loop
SENTINEL = 7.0                                 # what the GPU tests pre-fill every output with
MAX_PDF_IN = 1024


def _c(x, dt=f32):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dt))


def chunks(n: int) -> int:
    return (n + 63) // 64


def k_e_fwd(n: int) -> int:
    return 6 if n <= 64 else chunks(n) + 5


def k_composite(n: int) -> int:
    return chunks(n) + 7


def k_acc(n: int) -> int:
    return chunks(n) + 5


def k_cdf(n_in: int) -> int:
    return 2 * chunks(n_in) + 14


def k_prefix(n: int) -> int:
    return 7 + chunks(n)


# ----------------------------------------------------------------------------------------------------------------------
# the two checks of the GPU tests (tests/test_gpu_ray_losses.py defines the same two)
# ----------------------------------------------------------------------------------------------------------------------
def within(name, got, want, tol):
    """every element inside its bound; prints the worst ratio first.  A NaN of the reference must be a NaN of the device (and
    only there): such elements are compared as that and take no part in the ratio."""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    tol = np.broadcast_to(np.asarray(tol, f64), want.shape)
    assert got.shape == want.shape, name
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.all(np.isfinite(got[~nan])), (name, "NaN / inf pattern")
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want)))
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f"{name}: worst |device - fp64| / bound = {float(ratio.max()) if ratio.size else 0.0:.4f}")
    assert np.all(err <= np.where(nan, 0.0, tol)), (name, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, name
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~((got == 0) & (want == 0))  # the sign of a zero is not part of the contract
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def fails(check, *args) -> bool:
    """True where ``check`` (within / same_bits) raises: what a planted fault must do"""
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# fp32 sums in three orders
# ----------------------------------------------------------------------------------------------------------------------
def _scan(x: np.ndarray, order: str) -> np.ndarray:
    """inclusive prefix sums along axis 1 in float32, one pass without chunking"""
    x = np.ascontiguousarray(x, dtype=f32)
    if order == "sequential":
        return np.cumsum(x, axis=1, dtype=f32)
    out, o = x.copy(), 1
    while o < out.shape[1]:  # Hillis-Steele
        nxt = out.copy()
        nxt[:, o:] = (out[:, o:] + out[:, :-o]).astype(f32)
        out, o = nxt, o * 2
    return out


def prefix32(x, order: str, carry: str = "running", drop_carry: bool = False) -> np.ndarray:
    """inclusive prefix sums along axis 1 in float32.  "wave": chunks of 64 through wave_scan_fp32 with the chunk carry either
    "running" (incl = scan + carry; carry = lane 63 of incl: sample_pdf_kernel, depth_kernel) or "accumulated" (value = carry +
    scan; carry += lane 63 of the scan: weights_kernel).  ``drop_carry``: every chunk of 64 starts from 0, in any order."""
    x = np.ascontiguousarray(x, dtype=f32)
    R, n = x.shape
    if order != "wave" and not drop_carry:
        return _scan(x, order)
    c = chunks(n)
    v = np.zeros((R, c * 64), f32)
    v[:, :n] = x
    out, cr = np.zeros((R, c * 64), f32), np.zeros((R, 1), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(c):
            blk = v[:, 64 * b:64 * b + 64]
            scan = wave_scan_fp32(blk) if order == "wave" else _scan(blk, order)
            incl = (scan + cr).astype(f32)
            out[:, 64 * b:64 * b + 64] = incl
            if not drop_carry:
                cr = incl[:, 63:] if carry == "running" else (cr + scan[:, 63:]).astype(f32)
    return out[:, :n]


def sum32(x, order: str) -> np.ndarray:
    """sum along axis 1 in float32; "wave": lane l adds its elements l, l + 64, ... in turn, then wave_sum"""
    x = np.ascontiguousarray(x, dtype=f32)
    R, n = x.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if order != "wave":
            return _scan(x, order)[:, -1]
        c = chunks(n)
        v = np.zeros((R, c * 64), f32)
        v[:, :n] = x
        part = np.zeros((R, 64), f32)
        for b in range(c):
            part = (part + v[:, 64 * b:64 * b + 64]).astype(f32)
        return wave_scan_fp32(part)[:, 63]


def exp32(x) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, f64)).astype(f32)


def nan_to_num32(x) -> np.ndarray:
    return np.nan_to_num(np.asarray(x, f32), nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX).astype(f32)


# ----------------------------------------------------------------------------------------------------------------------
# spacing functions, sample_initial, frustums: fp32 op by op (numpy rounds every float32 operation correctly)
# ----------------------------------------------------------------------------------------------------------------------
def spacing_fn_fp32(x, lin: bool) -> np.ndarray:
    x = _c(x)
    if lin:
        return x
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x < f32(1), x / f32(2), f32(1) - f32(1) / (f32(2) * x)).astype(f32)


def spacing_to_eucl_fp32(b, s_near, s_far, lin: bool) -> np.ndarray:
    """b [R, k], s_near / s_far [R]: add_rn(mul_rn(x, sf), mul_rn(sub_rn(1, x), sn)), then the inverse spacing function"""
    b = _c(b)
    sn, sf = _c(s_near).reshape(-1, 1), _c(s_far).reshape(-1, 1)
    u = ((b * sf).astype(f32) + ((f32(1) - b).astype(f32) * sn).astype(f32)).astype(f32)
    if lin:
        return u
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u < f32(0.5), f32(2) * u, f32(1) / (f32(2) - (f32(2) * u).astype(f32)).astype(f32)).astype(f32)


def sample_initial_fp32(lin_bins, t_rand, nears, fars, lin: bool, per_sample: bool) -> Tuple[np.ndarray, np.ndarray]:
    """sample_initial_kernel: (spacing [R, n + 1], eucl [R, n + 1]); t_rand None | [R] | [R, n + 1]"""
    lb = _c(lin_bins)
    R = _c(nears).shape[0]
    b = np.broadcast_to(lb, (R, lb.shape[0])).copy()
    if t_rand is not None:
        centres = ((lb[1:] + lb[:-1]).astype(f32) / f32(2)).astype(f32)
        lo, hi = np.concatenate([lb[:1], centres]), np.concatenate([centres, lb[-1:]])
        t = _c(t_rand).reshape(R, -1 if per_sample else 1)
        b = (lo + ((hi - lo).astype(f32) * t).astype(f32)).astype(f32)
    return b, spacing_to_eucl_fp32(b, spacing_fn_fp32(nears, lin), spacing_fn_fp32(fars, lin), lin)


def frustum_positions_fp32(origins, directions, starts, ends) -> np.ndarray:
    """o + fl(fl(d fl(s + e)) / 2): [R, n, 3]"""
    o, d = _c(origins)[:, None, :], _c(directions)[:, None, :]
    se = (_c(starts) + _c(ends)).astype(f32)[..., None]
    return (o + ((d * se).astype(f32) / f32(2)).astype(f32)).astype(f32)


def frustum_from_edges_fp32(origins, directions, eucl):
    """-> (positions [R, n, 3], starts, ends, deltas = e - s)"""
    e = _c(eucl)
    s, t = e[:, :-1].copy(), e[:, 1:].copy()
    return frustum_positions_fp32(origins, directions, s, t), s, t, (t - s).astype(f32)


# ----------------------------------------------------------------------------------------------------------------------
# sample_pdf
# ----------------------------------------------------------------------------------------------------------------------
class PdfRef(NamedTuple):
    spacing: np.ndarray  # [R, n_out + 1] fp64
    tol: np.ndarray      # [R, n_out + 1]
    cdf: np.ndarray      # [R, n_in + 1] fp64
    uu: np.ndarray       # [R, n_out + 1] the draws (fp32 values, widened)
    index: np.ndarray    # [R, n_out + 1] searchsorted(cdf, uu, side="right") before the clamps


def draws_fp32(u, u_rand, R: int, n_out: int, per_sample: bool, fault: Optional[str] = None) -> np.ndarray:
    """[R, n_out + 1] float32: u_j, or add_rn(u_j, rand / nb) with one draw per ray or per edge"""
    nb = n_out + 1
    u = _c(u).reshape(nb)
    if u_rand is None:
        return np.broadcast_to(u, (R, nb)).copy()
    div = f32(n_out if fault == "jitter_div_n_out" else nb)
    ur = _c(u_rand).reshape(-1)
    if per_sample:
        stride = n_out if fault == "jitter_row_stride" else nb
        idx = np.arange(R)[:, None] * stride + np.arange(nb)[None, :]
        jit = (ur[idx] / div).astype(f32)
    else:
        jit = (ur.reshape(R, 1) / div).astype(f32)
    return (u[None, :] + jit).astype(f32)


def sample_pdf(weights, existing_bins, u, u_rand, nears, fars, n_out: int, lin: bool, per_sample: bool,
               cdf_fp32: bool = False, k: Optional[float] = None, k_t: float = 5.0) -> PdfRef:
    """spacing bins of tn_sample_pdf in fp64 (nears / fars / lin only enter the euclidean map, see the module docstring).
    k, k_t: the CDF count and the count of t and its product of ANOTHER kernel that resamples the same way (the fused proposal
    pass, tests/proposal_eval_reference.py); by default those of sample_pdf_kernel, k_cdf(n_in) and 5"""
    w, ex = _c(weights), _c(existing_bins).astype(f64)
    R, n_in = w.shape
    wpad = (w + f32(0.01)).astype(f32).astype(f64)
    ws = wpad.sum(1, keepdims=True)
    padding = np.maximum(float(f32(1e-5)) - ws, 0.0)
    pdf = (wpad + padding / n_in) / (ws + padding)
    cdf = np.concatenate([np.zeros((R, 1)), np.minimum(1.0, np.cumsum(pdf, axis=1))], axis=1)
    if cdf_fp32:
        cdf = cdf.astype(f32).astype(f64)
    uu = draws_fp32(u, u_rand, R, n_out, per_sample).astype(f64)
    idx = np.stack([np.searchsorted(cdf[r], uu[r], side="right") for r in range(R)])
    below, above = np.clip(idx - 1, 0, n_in), np.clip(idx, 0, n_in)
    c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    b0, b1 = np.take_along_axis(ex, below, 1), np.take_along_axis(ex, above, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip(np.nan_to_num((uu - c0) / (c1 - c0), nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX), 0.0, 1.0)
        b = b0 + t * (b1 - b0)
        dc, db = np.diff(cdf, axis=1), np.abs(np.diff(ex, axis=1))
        slope = np.where(dc > 0, db / np.where(dc > 0, dc, 1.0), np.where(db > 0, np.inf, 0.0))
    d = (k_cdf(n_in) if k is None else k) * EPS32
    tol = np.zeros_like(b)
    for r in range(R):
        klo = np.clip(np.searchsorted(cdf[r, 1:], uu[r] - d, side="left"), 0, n_in - 1)
        khi = np.maximum(np.clip(np.searchsorted(cdf[r, :-1], uu[r] + d, side="right") - 1, 0, n_in - 1), klo)
        for j in range(uu.shape[1]):
            lo, hi = int(klo[j]), int(khi[j]) + 1
            tol[r, j] = d * slope[r, lo:hi].max() + EPS32 * (k_t * db[r, lo:hi].max() + np.abs(ex[r, lo:hi + 1]).max())
    return PdfRef(b, tol + TINY32, cdf, uu, idx)


def _bisect(cdf: np.ndarray, uu: np.ndarray, left: bool = False) -> np.ndarray:
    """sample_pdf_kernel's binary search over the n_in + 1 CDF entries of each ray: the first index with cdf > uu
    (``left``: >= uu, the planted fault)"""
    R, m = cdf.shape
    lo, hi = np.zeros(uu.shape, np.int64), np.full(uu.shape, m, np.int64)
    for _ in range(12):
        active = lo < hi
        mid = (lo + hi) >> 1
        cm = np.take_along_axis(cdf, np.minimum(mid, m - 1), 1)
        go = active & ((cm < uu) if left else (cm <= uu))
        lo = np.where(go, mid + 1, lo)
        hi = np.where(active & ~go, mid, hi)
    return lo


PDF_FAULTS = ("side_left", "carry_dropped", "no_cdf_clamp", "jitter_row_stride", "jitter_div_n_out")


def sample_pdf_fp32(weights, existing_bins, u, u_rand, nears, fars, n_out: int, lin: bool, per_sample: bool,
                    order: str = "wave", fault: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
    """sample_pdf_kernel in numpy float32, op by op -> (spacing, eucl) [R, n_out + 1].  fault: one of PDF_FAULTS, or "t_unclamped"
    (which changes nothing, see the module docstring)."""
    w, ex = _c(weights), _c(existing_bins)
    R, n_in = w.shape
    wpad = (w + f32(0.01)).astype(f32)
    ws = sum32(wpad, order)[:, None]
    padding = np.maximum((f32(1e-5) - ws).astype(f32), f32(0))
    pad_each = (padding / f32(n_in)).astype(f32)
    ws = (ws + padding).astype(f32)
    pdf = ((wpad + pad_each).astype(f32) / ws).astype(f32)
    cum = prefix32(pdf, order, "running", drop_carry=(fault == "carry_dropped"))
    if fault != "no_cdf_clamp":
        cum = np.minimum(f32(1), cum)
    cdf = np.concatenate([np.zeros((R, 1), f32), cum], axis=1)
    uu = draws_fp32(u, u_rand, R, n_out, per_sample, fault)
    idx = _bisect(cdf, uu, left=(fault == "side_left"))
    below, above = np.clip(idx - 1, 0, n_in), np.clip(idx, 0, n_in)
    c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    b0, b1 = np.take_along_axis(ex, below, 1), np.take_along_axis(ex, above, 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = nan_to_num32(((uu - c0).astype(f32) / (c1 - c0).astype(f32)).astype(f32))
        if fault != "t_unclamped":
            t = np.clip(t, f32(0), f32(1))
        b = (b0 + (t * (b1 - b0).astype(f32)).astype(f32)).astype(f32)
    return b, spacing_to_eucl_fp32(b, spacing_fn_fp32(nears, lin), spacing_fn_fp32(fars, lin), lin)


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
class WeightsRef(NamedTuple):
    weights: np.ndarray  # [R, n] fp64
    tol: np.ndarray      # [R, n]; 0 where the value is pinned
    pinned: np.ndarray   # [R, n] bool


def weights(deltas, densities) -> WeightsRef:
    dl, dn = _c(deltas), _c(densities)
    R, n = dl.shape
    with np.errstate(invalid="ignore", over="ignore"):
        a = (dl * dn).astype(f32).astype(f64)
        excl = lambda x: np.concatenate([np.zeros((R, 1)), np.cumsum(x, axis=1)[:, :-1]], axis=1)  # noqa: E731
        E, Eabs = excl(a), excl(np.abs(a))
        T, ea = np.exp(-E), np.exp(-a)
        w = np.nan_to_num(-np.expm1(-a) * T, nan=0.0)
        werr = np.abs(w) * (k_e_fwd(n) * Eabs + K_EXP + 2) + K_EXP * ea * T
    pinned = (a == 0) | np.isnan(a) | ~np.isfinite(E)
    tol = np.where(pinned, 0.0, EPS32 * np.where(pinned, 0.0, werr) + TINY32)
    return WeightsRef(w, tol, pinned)


WEIGHTS_FAULTS = ("carry_dropped", "inclusive", "no_nan_to_num")


def weights_fp32(deltas, densities, order: str = "wave", fault: Optional[str] = None) -> np.ndarray:
    """weights_kernel (and the first half of ray_render[_depth]_fwd_kernel) in numpy float32"""
    dl, dn = _c(deltas), _c(densities)
    R, n = dl.shape
    with np.errstate(invalid="ignore", over="ignore"):
        a = (dl * dn).astype(f32)
        incl = prefix32(a, order, "accumulated", drop_carry=(fault == "carry_dropped"))
        E = incl if fault == "inclusive" else np.concatenate([np.zeros((R, 1), f32), incl[:, :-1]], axis=1)
        if fault == "carry_dropped":  # lane 0 of a chunk has nothing before it
            E = E.copy()
            E[:, 64::64] = 0
        w = ((f32(1) - exp32(-a.astype(f64))).astype(f32) * exp32(-E.astype(f64))).astype(f32)
    return w if fault == "no_nan_to_num" else nan_to_num32(w)


# ----------------------------------------------------------------------------------------------------------------------
# composite
# ----------------------------------------------------------------------------------------------------------------------
class CompositeRef(NamedTuple):
    out: np.ndarray  # [R, C] fp64; NaN where a NaN sample comes through (training)
    tol: np.ndarray


def composite(values, weights, training: bool) -> CompositeRef:
    v, w = _c(values).astype(f64), _c(weights).astype(f64)
    R, n, C = v.shape
    if not training:
        v = np.nan_to_num(v, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)
    with np.errstate(invalid="ignore"):
        acc = w.sum(1)[:, None]
        out = (w[..., None] * v).sum(1) + v[:, -1, :] * (1.0 - acc)
        mag = (k_composite(n) * (np.abs(w)[..., None] * np.abs(v)).sum(1)
               + np.abs(v[:, -1, :]) * (k_acc(n) * np.abs(w).sum(1)[:, None] + 3 * np.abs(1.0 - acc)))
    if not training:
        out = np.clip(out, 0.0, 1.0)
    return CompositeRef(out, np.where(np.isnan(out), 0.0, EPS32 * np.where(np.isnan(mag), 0.0, mag) + TINY32))


COMPOSITE_FAULTS = ("no_background", "no_eval_clamp", "nan_to_num_in_training")


def composite_fp32(values, weights, training: bool, order: str = "wave", fault: Optional[str] = None) -> np.ndarray:
    v, w = _c(values), _c(weights)
    R, n, C = v.shape
    if not training or fault == "nan_to_num_in_training":
        v = nan_to_num32(v)
    out = np.zeros((R, C), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = sum32(w, order)
        for ch in range(C):
            comp = sum32((w * v[:, :, ch]).astype(f32), order)
            if fault != "no_background":
                comp = (comp + (v[:, -1, ch] * (f32(1) - acc).astype(f32)).astype(f32)).astype(f32)
            out[:, ch] = comp
    if not training and fault != "no_eval_clamp":
        out = np.minimum(np.maximum(out, f32(0)), f32(1))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# depth
# ----------------------------------------------------------------------------------------------------------------------
class DepthRef(NamedTuple):
    accumulation: np.ndarray  # [R] fp64
    median: np.ndarray        # [R] float32: the mid-point of sample ``index``
    expected: np.ndarray      # [R] fp64, clipped
    tol_accumulation: np.ndarray
    tol_expected: np.ndarray
    index: np.ndarray         # [R] first i with cumsum >= 0.5, else n - 1
    lo: float                 # the call's smallest and largest mid-point
    hi: float
    near_tie: np.ndarray      # [R] bool: an fp64 prefix within k_prefix(n) u prefix of 0.5 at ``index`` or before it


def midpoints_fp32(starts, ends) -> np.ndarray:
    return ((_c(starts) + _c(ends)).astype(f32) / f32(2)).astype(f32)


def depth(weights, starts, ends) -> DepthRef:
    w = _c(weights).astype(f64)
    R, n = w.shape
    mid32 = midpoints_fp32(starts, ends)
    mid = mid32.astype(f64)
    cum = np.cumsum(w, axis=1)
    hit = cum >= 0.5
    idx = np.where(hit.any(1), hit.argmax(1), n - 1)
    rows = np.arange(R)
    at, before = cum[rows, idx], cum[rows, np.maximum(idx - 1, 0)]
    near = lambda p: np.abs(p - 0.5) <= k_prefix(n) * EPS32 * np.abs(p)  # noqa: E731
    near_tie = near(at) | ((idx > 0) & near(before))
    acc, aabs = w.sum(1), np.abs(w).sum(1)
    num, nabs = (w * mid).sum(1), (np.abs(w) * np.abs(mid)).sum(1)
    den = acc + float(f32(1e-10))
    lo, hi = float(mid32.min()), float(mid32.max())
    q = num / den
    tol_e = EPS32 * ((chunks(n) + 6) * nabs / np.abs(den) + np.abs(q) * (k_acc(n) * aabs / np.abs(den) + 2)) + TINY32
    return DepthRef(acc, mid32[rows, idx], np.clip(q, lo, hi), k_acc(n) * EPS32 * aabs + TINY32, tol_e, idx, lo, hi, near_tie)


DEPTH_FAULTS = ("gt_for_ge", "prefix_restart", "no_index_clamp", "block_bounds", "first_trip_only")


def depth_fp32(weights, starts, ends, order: str = "wave", fault: Optional[str] = None):
    """depth_kernel + depth_clip_kernel in numpy float32 -> (accumulation, median, expected) [R], rays a faulty kernel never
    reaches left at SENTINEL"""
    w = _c(weights)
    R, n = w.shape
    mid = midpoints_fp32(starts, ends)
    cum = prefix32(w, order, "running", drop_carry=(fault == "prefix_restart"))
    hit = (cum > f32(0.5)) if fault == "gt_for_ge" else (cum >= f32(0.5))
    idx = np.where(hit.any(1), hit.argmax(1), n)
    if fault != "no_index_clamp":
        idx = np.minimum(idx, n - 1)
    flat = np.concatenate([mid.reshape(-1), np.full(1, np.nan, f32)])  # what lies behind a ray is the next ray
    median = flat[np.arange(R) * n + idx]
    acc = sum32(w, order)
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = (sum32((w * mid).astype(f32), order) / (acc + f32(1e-10)).astype(f32)).astype(f32)
    grid = min((R + RAYS_PER_BLOCK - 1) // RAYS_PER_BLOCK, DEPTH_GRID_CAP)
    seen = np.arange(R) < (grid * RAYS_PER_BLOCK if fault == "first_trip_only" else R)
    if fault == "block_bounds":
        block = (np.arange(R) // RAYS_PER_BLOCK) % grid
        lo, hi = np.full(grid, np.inf, f32), np.full(grid, -np.inf, f32)
        np.minimum.at(lo, block, mid.min(1))
        np.maximum.at(hi, block, mid.max(1))
        lo, hi = lo[block], hi[block]
    else:
        lo, hi = mid[seen].min(), mid[seen].max()
    expected = np.minimum(np.maximum(expected, lo), hi).astype(f32)
    keep = lambda x: np.where(seen, x, f32(SENTINEL)).astype(f32)  # noqa: E731
    return keep(acc), keep(median), keep(expected)


def depth_exact_fp32(weights, starts, ends):
    """the exact family's expectation: every sum from fp64 (exact there), the two rounded operations of `expected` in fp32"""
    ref = depth(weights, starts, ends)
    mid = midpoints_fp32(starts, ends).astype(f64)
    num = (_c(weights).astype(f64) * mid).sum(1)
    assert np.array_equal(num, num.astype(f32)) and np.array_equal(ref.accumulation, ref.accumulation.astype(f32))
    den = (ref.accumulation.astype(f32) + f32(1e-10)).astype(f32)
    expected = (num / den.astype(f64)).astype(f32)  # 53 bits >= 2 * 24 + 2: one rounding
    return ref.accumulation.astype(f32), ref.median, np.clip(expected, f32(ref.lo), f32(ref.hi)).astype(f32)


# ----------------------------------------------------------------------------------------------------------------------
# case builders
# ----------------------------------------------------------------------------------------------------------------------
PdfCase = Dict[str, object]  # weights, existing_bins, u, u_rand, nears, fars, n_out, lin, per_sample: sample_pdf's arguments
JITTERS = (None, "ray", "edge")


def pdf_positions_fp32(nb: int, jitter) -> np.ndarray:
    """NS PDFSampler's u: linspace(0, 1 - 1 / nb, nb), plus 1 / (2 nb) where there is no jitter"""
    u = np.linspace(0.0, 1.0 - 1.0 / nb, nb).astype(f32)
    return u if jitter else (u + f32(1.0 / (2 * nb))).astype(f32)


def pdf_general_case(R: int, n_in: int, n_out: int, seed: int, jitter=None, lin: bool = False) -> PdfCase:
    """weights rand^6 (ray 0 all zero: a uniform resample through the histogram padding; ray 1 one spike), existing bins sorted
    fp32 numbers from 0 to 1, the sampler's own u, jitter None | one draw per "ray" | one per "edge\""""
    rng = np.random.default_rng(seed)
    nb = n_out + 1
    w = rng.random((R, n_in)) ** 6
    w[0] = 0
    if R > 1:
        w[1] = 0
        w[1, n_in // 2] = 1
    ex = np.sort(rng.random((R, n_in + 1)), axis=1)
    ex[:, 0], ex[:, -1] = 0.0, 1.0
    u_rand = None if jitter is None else rng.random(R if jitter == "ray" else (R, nb)).astype(f32)
    nears = np.where(np.arange(R) % 2 == 0, 0.05, 0.0).astype(f32)
    fars = np.where(np.arange(R) % 3 == 0, 6.0, 1000.0).astype(f32)
    return dict(weights=w.astype(f32), existing_bins=ex.astype(f32), u=pdf_positions_fp32(nb, jitter), u_rand=u_rand, nears=nears,
                fars=fars, n_out=n_out, lin=lin, per_sample=(jitter == "edge"))


GRID = 4096  # the exact PDF family's draws and bins are multiples of 1 / GRID


def _split_power_of_two(rng, M: int, q: int):
    parts = [M]
    while len(parts) < q:
        big = [i for i, p in enumerate(parts) if p > 1]
        i = big[int(rng.integers(0, len(big)))]
        parts[i] //= 2
        parts.insert(i, parts[i])
    return parts


def pdf_exact_case(R: int, n_in: int, n_out: int, seed: int, jitter=None, lin: bool = False) -> PdfCase:
    """see the module docstring.  Ray r mod 4: 0 up to 40 weights with zeros between them (for n_in >= 68 weights 61 .. 66 are
    zero: a flat run over CDF entries 61 .. 67, across the chunk boundary), 1 a single weight at index 0 (the CDF is 1 from entry
    1 on), 2 every weight non-zero where M allows, 3 (n_in >= 4) + M/2 + M/2 + M/2 - M/2: the cumulative sum passes 1.5.
    The draws of ray r visit, in turn: 0, the CDF values at the start of its flat runs, 1, 1 + 2^-12, 1.25, its other CDF values,
    then random multiples of 2^-12; without jitter and with one draw per ray only ray 0's list can be hit on purpose."""
    rng = np.random.default_rng(seed)
    nb = n_out + 1
    m = np.zeros((R, n_in))
    for r in range(R):
        kind = r % 4
        if kind == 3 and n_in >= 4:
            pos = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n_in), 3, replace=False))])
            m[r, pos] = [0.5, 0.5, 0.5, -0.5]
            continue
        q = {0: 1 + int(rng.integers(0, min(n_in, 40))), 1: 1, 2: min(n_in, 1024), 3: 1}[kind]
        free, fixed = np.arange(1, n_in), [0]
        if kind == 0 and n_in >= 68:
            free, fixed = free[(free < 60) | (free > 67)], [0, 60, 67]
            q = max(q, 3)
        extra = rng.choice(free, q - len(fixed), replace=False) if q > len(fixed) else []
        pos = np.concatenate([fixed, extra]).astype(np.int64)
        M = 1024 if q > 1 else 1
        m[r, np.sort(pos)] = np.asarray(_split_power_of_two(rng, M, q), f64) / M
    w = (m * 2.0 ** 40).astype(f32)
    ex = np.zeros((R, n_in + 1))
    for r in range(R):
        ex[r, 1:-1] = np.sort(rng.choice(np.arange(1, GRID), n_in - 1, replace=False))
    ex[:, -1] = GRID
    cdf = np.concatenate([np.zeros((R, 1)), np.minimum(1.0, np.cumsum(m, axis=1))], axis=1)
    targets = np.zeros((R, nb))
    for r in range(R):
        c = cdf[r]
        flat_start = [c[k] for k in range(1, n_in) if c[k] == c[k + 1] and c[k - 1] < c[k]]
        other = [c[k] for k in range(1, n_in + 1) if c[k] not in flat_start][:8]
        special = [0.0] + flat_start[:6] + [1.0, 1.0 + 1.0 / GRID, 1.25] + other
        rnd = rng.integers(0, GRID + 1, size=nb) / GRID
        targets[r] = (special + list(rnd))[:nb]
    if jitter is None:
        u, u_rand = targets[0], None
    elif jitter == "ray":
        q = rng.integers(0, GRID // 4 + 1, size=R)
        q[min(1, R - 1)] = 0
        u = np.where(targets[0] * GRID >= q[0], targets[0] - q[0] / GRID, targets[0])
        u_rand = nb * q / GRID
    else:
        u = (np.arange(nb) % 8) / GRID
        targets = np.maximum(targets, u[None, :])
        u_rand = nb * (targets - u[None, :])
    near = np.asarray([0.0, 0.0625, 0.5, 2.0])[np.arange(R) % 4]
    far = np.asarray([1024.0, 4.0, 8.0])[np.arange(R) % 3]
    return dict(weights=w, existing_bins=(ex / GRID).astype(f32), u=u.astype(f32), u_rand=None if u_rand is None else u_rand.astype(f32),
                nears=near.astype(f32), fars=far.astype(f32), n_out=n_out, lin=lin, per_sample=(jitter == "edge"))


def weights_general_case(R: int, n: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """the sibling's render_case: generic, empty, saturating, single dense sample, last chunk only, delta = 0 samples"""
    c = render_case(R, n, seed)
    return c.deltas, c.densities


def weights_special_case(n: int, seed: int):
    """(deltas, densities, kinds): ray 0 all density 0; then for k in {0, n // 2, 63, 64, n - 1} (inside the ray) three rays:
    "inf" sigma_k = inf with delta_k > 0, "nan" sigma_k = inf with delta_k = 0, "single" sigma = 0 except at k"""
    rng = np.random.default_rng(seed)
    ks = sorted({0, n // 2, min(63, n - 1), min(64, n - 1), n - 1})
    kinds = [("zero", 0)] + [(kind, k) for k in ks for kind in ("inf", "nan", "single")]
    R = len(kinds)
    deltas = (0.01 + rng.random((R, n)) * 0.2).astype(f32)
    dens = (rng.random((R, n)) * 4).astype(f32)
    for r, (kind, k) in enumerate(kinds):
        if kind == "zero":
            dens[r] = 0
        elif kind == "inf":
            dens[r, k] = np.inf
        elif kind == "nan":
            dens[r, k], deltas[r, k] = np.inf, 0
        else:
            dens[r] = 0
            dens[r, k] = 3.0
    return deltas, dens, kinds


def composite_general_case(R: int, n: int, C: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """values in [0, 1.3] with one NaN sample (ray 2 mod R, sample 1 mod n, channel 0), weights summing to 0 .. 1.2; ray 0 has none"""
    rng = np.random.default_rng(seed)
    v = (rng.random((R, n, C)) * 1.3).astype(f32)
    v[2 % R, 1 % n, 0] = np.nan
    w = rng.random((R, n))
    w = w / w.sum(1, keepdims=True) * rng.random((R, 1)) * 1.2
    w[0] = 0
    return v, w.astype(f32)


def composite_exact_case(R: int, n: int, C: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """ray r mod 4: 0 no weight (output = the last sample), 1 weights summing to 1 + 3 * 2^-10 on values 0 with a last sample of
    1 (a negative background term: below 0 before the eval clamp), 2 weights summing to at most 1, 3 sparse"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 257, size=(R, n, C)) / 256.0
    w = np.zeros((R, n), np.int64)
    for r in range(R):
        kind = r % 4
        if kind == 1:
            np.add.at(w[r], rng.integers(0, max(n - 1, 1), size=1027), 1)  # none on the last sample where there is another
            v[r], v[r, -1] = 0.0, 1.0
        elif kind == 2:
            np.add.at(w[r], rng.integers(0, n, size=int(rng.integers(1, 1025))), 1)
        elif kind == 3:
            np.add.at(w[r], rng.integers(0, n, size=5), 37)
    return v.astype(f32), (w / 1024.0).astype(f32)


def _distinct_edges(rng, R: int, n: int) -> np.ndarray:
    """[R, n + 1] strictly increasing multiples of 2^-7 in [1, 17): the mid-points are distinct multiples of 2^-8"""
    e = np.stack([np.sort(rng.choice(np.arange(128, 17 * 128), n + 1, replace=False)) for _ in range(R)])
    return e / 128.0


def depth_tie_indices(n: int):
    ks = {0, 62, 63, 64, 65, n - 1} | ({64 * c + 17 for c in range(16)} if n == 1024 else set())
    return sorted(k for k in ks if k < n)


def depth_exact_case(n: int, seed: int):
    """(weights, starts, ends, kinds).  One ray per k in depth_tie_indices(n) whose cumulative weight is 0.5 EXACTLY at k and
    below it before (k = n - 1: a total of exactly 0.5, reached only at the last sample), then "below" (a total below 0.5),
    "jump" (the prefix passes 0.5 without touching it), "zero" (no weight: expected = 0 clipped up to the call's smallest
    mid-point) and "overshoot" (n >= 2: weights -1/4 first and 1/2 last on the call's largest mid-point, expected =
    2 m_last - m_first, clipped down to that mid-point)."""
    rng = np.random.default_rng(seed)
    kinds = [("tie", k) for k in depth_tie_indices(n)] + [("below", 0), ("jump", 0), ("zero", 0)] + ([("overshoot", 0)] if n >= 2 else [])
    R = len(kinds)
    w = np.zeros((R, n), np.int64)  # units of 2^-10
    for r, (kind, k) in enumerate(kinds):
        if kind == "tie":
            w[r, k] = 1
            np.add.at(w[r], rng.integers(0, k + 1, size=511), 1)
            if k + 1 < n:
                np.add.at(w[r], rng.integers(k + 1, n, size=int(rng.integers(1, 600))), 1)
        elif kind == "below":
            np.add.at(w[r], rng.integers(0, n, size=500), 1)
        elif kind == "jump":  # 250 units before n // 2, 300 on it: from below 0.5 to above it in one step
            np.add.at(w[r], rng.integers(0, max(n // 2, 1), size=250), 1)
            w[r, n // 2] += 300
            np.add.at(w[r], rng.integers(n // 2, n, size=150), 1)
        elif kind == "overshoot":
            w[r, 0], w[r, -1] = -256, 512
    edges = _distinct_edges(rng, R, n)
    if n >= 2:
        edges[-1, -1] = 17.5  # the overshoot ray ends on the call's largest mid-point
    return (w / 1024.0).astype(f32), edges[:, :-1].astype(f32), edges[:, 1:].astype(f32), kinds


def depth_general_case(R: int, n: int, seed: int):
    """(weights, starts, ends, seed used): weights summing to 0 .. 1.2 (ray 0 none), edges sorted in [0, 5).  Walks seeds from
    ``seed`` until no ray has a near tie (DepthRef.near_tie), so that every median index is determinate in fp32."""
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        w = rng.random((R, n))
        w = w / w.sum(1, keepdims=True) * rng.random((R, 1)) * 1.2
        w[0] = 0
        edges = np.sort(rng.random((R, n + 1)) * 5, axis=1).astype(f32)
        w = w.astype(f32)
        if not depth(w, edges[:, :-1], edges[:, 1:]).near_tie.any():
            return w, edges[:, :-1].copy(), edges[:, 1:].copy(), s
    raise AssertionError("no seed without a near tie")


SECOND_TRIP_R = 2053  # > 512 blocks x 4 rays: rays 2048 .. 2052 are the second trip of blocks 0 and 1


def depth_second_trip_case(seed: int):
    """R = 2053, n = 3, exact weights.  The call's smallest mid-point lies in ray 2048 (block 0) and its largest in ray 2052
    (block 1), both on the second trip of the ray loop; rays 5 mod 16 carry no weight (expected = the call's smallest mid-point)
    and rays 9 mod 16 the overshoot weights of depth_exact_case (expected = the call's largest)."""
    rng = np.random.default_rng(seed)
    R, n = SECOND_TRIP_R, 3
    w = rng.integers(0, 400, size=(R, n))
    w[5::16] = 0
    w[9::16] = [-256, 0, 512]
    edges = np.stack([np.sort(rng.choice(np.arange(4 * 128, 12 * 128), n + 1, replace=False)) for _ in range(R)]) / 128.0
    edges[9::16] = [4.0, 4.5, 11.0, 11.5]  # mid-points 4.25 and 11.25: 2 * 11.25 - 4.25 = 18.25, above every mid-point
    edges[2048] = [1.0, 1.25, 5.0, 6.0]
    edges[2052] = [5.0, 6.0, 16.0, 16.5]
    return (w / 1024.0).astype(f32), edges[:, :-1].astype(f32), edges[:, 1:].astype(f32)


def sample_initial_case(R: int, n: int, seed: int, jitter=None):
    """(lin_bins [n + 1], t_rand None | [R] | [R, n + 1], nears, fars): nears below and above 1 (both branches of spacing_fn)"""
    rng = np.random.default_rng(seed)
    t = None if jitter is None else rng.random(R if jitter == "ray" else (R, n + 1)).astype(f32)
    nears = np.where(np.arange(R) % 3 == 0, 0.0, np.where(np.arange(R) % 3 == 1, 0.05, 1.5)).astype(f32)
    fars = np.where(np.arange(R) % 2 == 0, 1000.0, 6.0).astype(f32)
    return np.linspace(0.0, 1.0, n + 1).astype(f32), t, nears, fars


def frustum_case(R: int, n: int, seed: int):
    """(origins [R, 3], directions [R, 3], eucl edges [R, n + 1])"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((R, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rng.standard_normal((R, 3)).astype(f32), d.astype(f32), np.sort(rng.random((R, n + 1)) * 6, axis=1).astype(f32)


# the (n_in, n_out) pairs of the GPU tests: every n_in of N_EDGES, every n_out of N_OUT_EDGES
PDF_SHAPES = [(1, 63), (2, 1), (63, 64), (64, 127), (65, 63), (128, 300), (129, 64), (1024, 127), (129, 1), (129, 300)]
