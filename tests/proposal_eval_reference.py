"""fp64 reference of the eval proposal pass (tn_proposal_sample_fwd), ONE LEVEL AT A TIME, with the counted bound beside every value,
fp32 op-by-op models of its two kernel families with plantable faults, and the case builders of tests/test_gpu_proposal_eval.py and
tests/test_proposal_eval_reference_cpu.py — numpy, no device.  The sibling of tests/field_eval_reference.py (whose ``geometry``,
``GridRef``, ``encode`` / ``_layer`` / ``_exp`` behind ``proposal_density`` and measured K_FEXP_* / K_RCP it uses) and of
tests/ray_forward_reference.py (``sample_pdf``, ``sample_initial_fp32``, ``spacing_to_eucl_fp32``, ``k_cdf``, ``k_e_fwd``, ``within``,
``same_bits``, ``fails``).  Their conventions hold: fp32 inputs are widened, a single correctly rounded fp32 operation is formed in fp32.

The pass runs in two FAMILIES (thermo_nerf_amd/csrc/tn_render.hip):
  "wave"    proposal_kernel: one ray per wave; prop_level (wave scans) and pdf_resample (CDF in LDS, binary search)
  "serial"  lane = ray: proposal_rays_kernel<ND0, ND1, LEAN> and its split form proposal_density_segments_kernel +
            proposal_resample_kernel; per-lane running sums and the pdf_walk merge walk
Only the general forms write per-level outputs; the LEAN and the split forms leave the final edges and the two medians, and are held
bit for bit to the general form of the same grids by the GPU tests (the kernels' comments promise the same arithmetic).

Every stage is judged from the DEVICE's own output of the stage before it (``judge``), so no bound compounds across levels:

level-0 spacing edges.  lin_bins0 as given, or the four-operation stratified jitter lo + (hi - lo) t of sample_initial_fp32, one draw
  per ray or per edge: the fp32 model IS the expectation, bit for bit.
Euclidean edges from the device's spacing edges.  spacing_to_eucl<true> is four correctly rounded operations and then the identity
  (lin), 2 u (u < 0.5) or v_rcp_f32(2 - 2 u): bit for bit where no v_rcp_f32 is reached, (K_RCP + 1) u relative elsewhere (the
  same count as geometry(..., fast=True): K_RCP against the exact quotient, 1/2 for the correctly rounded one it is compared with,
  rounded up).
level weights from the device's Euclidean edges of that level.  delta = fl32(en - st) and the sample position are the kernel's own
  correctly rounded operations (formed in fp32); the contraction's v_rcp_f32 is BOUNDED as geometry(fast=True) bounds it (the
  edges enter geometry as an exact linear spacing from 0 to 1).  density: the counted bound of proposal_density — 9 u M a level,
  one rounding per non-zero weight of a row — with __expf in place of expf (K_FEXP_A + K_FEXP_B |x|, the fused kernels are FAST)
  and the position's bound carried through the features.  a_i = fl32(delta_i density_i): 1.  The optical depth before sample i:
  the lane = ray forms add ``accum`` serially, i terms, i - 1 roundings (the first add is onto 0): K_E = max(i - 1, 0) relative to
  sum_{j<i} |a_j|; the ray-per-wave form is k_e_fwd(n).  w = (1 - __expf(-a)) __expf(-E): both exponentials by K_FEXP_A, K_FEXP_B,
  K_FEXP_TINY, the subtraction 1, the product 1.
  Pinned (tolerance 0): a_i = 0 exactly (delta = 0 or density = 0 with no bound on either) -> __expf(-0) = 1, w = 0; everything
  behind an infinite or NaN optical depth -> 0; a NaN a_i -> 0.  A density whose fp64 value exceeds FLT_MAX by more than its bound is
  +inf, as in fp32.
resampled edges from the device's own weights and edges of the level.  The CDF-perturbation argument of ray_forward_reference:
  knots off by at most d move a sample by at most d times the steepest slope among the bins met.  d = K_CDF u.
    pdf_walk (serial):  a term fl(fl(fl(w + 0.01) + pad_each) rws): 3 roundings; rws = v_rcp_f32(ws): K_RCP; ``total`` is n_in
      serial adds, n_in - 1 roundings, + 1 for the padding add; the running sum at knot i: i adds, at most n_in:
      K_CDF_WALK(n_in) = 3 + K_RCP + n_in + n_in = 2 n_in + 3 + K_RCP  (267 at n_in = 130).
    pdf_resample (wave): k_cdf(n_in) of sample_pdf_kernel with the division as t_div<true>, a product + v_rcp_f32: + K_RCP.
  On top, t = fl(fl(uu - c0) v_rcp(fl(c1 - c0))): 3 + K_RCP relative to t <= 1, b1 - b0 (1), the product (1): (5 + K_RCP) |b1 - b0|;
  the add: 1 |b|.  anneal != 1: powf(w, anneal) is K_POW u relative (measured, below) on every term and on the total: + 2 (K_POW + 1)
  (the reference forms fl32(pow(w, anneal)) itself: 1/2 more a term, rounded up).
median depth.  An INDEX: the first i whose fp64 prefix of the DEVICE's weights of the level reaches 0.5, else n - 1 in every form; its
  value is fl32(fl32(st + en) / 2) of the device's own Euclidean edges at that index, bit for bit.  A device prefix is off by at most
  K_PREFIX u prefix: n serial adds (serial), 7 + c (wave, k_prefix).  A ray whose fp64 prefix lies within that of 0.5 at the
  index or before it is a near tie: ``general_case`` walks seeds until a case has none, then redraws single rays, at most 2 % of them.

K_POW.  powf(w, a), w in [0, 1], a in {0.5, 0.75}: MEASURED like the other library functions (tools/micro/libm_accuracy.hip,
  profiles/micro/libm_accuracy.txt): the worst value times 2, rounded up.

Every K is counted on the code as written, first order in u = 2^-24; none was tuned against device output."""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import field_eval_reference as F
from tests import ray_forward_reference as RF
from tests.field_eval_reference import K_RCP, TINY32, U, GridRef, geometry
from tests.ray_forward_reference import fails, k_cdf, k_e_fwd, same_bits, sample_initial_fp32, sample_pdf, spacing_to_eucl_fp32, within  # noqa: F401

f32, f64 = np.float32, np.float64
FLT_MAX = float(np.finfo(f32).max)
SENTINEL = 7.0
SERIAL, WAVE = "serial", "wave"
K_POW = 5.0              # MEASURED: worst of powf(w, 0.5) and powf(w, 0.75) over w in [0, 1]: 2.32 u (profiles/micro/libm_accuracy.txt), times 2, rounded up
WALK_BLOCK = 8           # TN_PDF_WALK_BLOCK of proposal_rays_kernel
RESAMPLE_BLOCK = 16      # TN_RESAMPLE_BLOCK of proposal_resample_kernel
REDRAW_CAP = 0.02

R_EDGES = [1, 63, 64, 65, 129]
SHAPES = [(1, 1, 1), (7, 5, 3), (63, 31, 12), (64, 32, 25), (70, 37, 48), (65, 130, 64)]   # (P0, P1, S)
TRAIN_SHAPE = (70, 37, 48)


def k_cdf_walk(n_in: int) -> float:
    return 2 * n_in + 3 + K_RCP


def k_cdf_family(family: str, n_in: int, anneal: float = 1.0) -> float:
    k = k_cdf_walk(n_in) if family == SERIAL else k_cdf(n_in) + K_RCP
    return k + (2 * (K_POW + 1) if anneal != 1.0 else 0)


K_T = 5 + K_RCP


def k_e(family: str, n: int) -> np.ndarray:
    """[n]: roundings in the optical depth in front of sample i"""
    return np.maximum(np.arange(n) - 1, 0).astype(f64) if family == SERIAL else np.full(n, float(k_e_fwd(n)))


def k_prefix(family: str, n: int) -> int:
    return n if family == SERIAL else RF.k_prefix(n)


# ----------------------------------------------------------------------------------------------------------------------
# networks, rays, cases
# ----------------------------------------------------------------------------------------------------------------------
class Net(NamedTuple):
    grid: GridRef
    w0: np.ndarray   # [16, 10]
    b0: np.ndarray   # [16]
    w1: np.ndarray   # [1, 16]
    b1: np.ndarray   # [1]
    avg: float


class Space(NamedTuple):   # what geometry() reads of a field
    contraction: bool
    aabb: np.ndarray


SPACE = Space(True, np.array([[-1, -1, -1], [1, 1, 1]], f32))
LOG2T = 10
OVERFLOW_BIAS = 200.0   # exp overflows whatever the hidden layer adds (|w1 . hidden| stays below 50)


def random_nets(seed: int, avg: float = 1.0, bias: float = 0.0) -> List[Net]:
    """the two proposal networks as tests/test_gpu_field_eval.py's DevProposal draws them: 5 levels, 16 hidden, contraction on"""
    r = np.random.default_rng(seed)
    nets = []
    for level in range(2):
        table = (r.uniform(-1, 1, (5 << LOG2T, 2)) * 0.6).astype(f32)
        scal = np.array((16.0, 26.0, 45.0, 76.0, 127.0 + 128 * level), f32)
        w0, b0 = (r.standard_normal((16, 10)) * 0.6).astype(f32), (r.standard_normal(16) * 0.2).astype(f32)
        w1 = (r.standard_normal((1, 16)) * 0.6).astype(f32)
        nets.append(Net(GridRef(table, scal, LOG2T), w0, b0, w1, np.array([bias], f32), float(f32(avg))))
    return nets


def mixed_rays(R: int, seed: int) -> F.Rays:
    """rays inside the unit cube (far 0.6: every sample below the piecewise map's u = 1/2), across it (origins up to 1.5 out, far 6)
    and beyond it (origins 2 .. 3 out, far 6: every sample under the contraction's v_rcp_f32), in turn; ray 1 has near = far = 0.5
    (every edge of every level is exactly 0.5 under both maps: delta = 0)"""
    r = np.random.default_rng(seed)
    d = r.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    kind = np.arange(R) % 3 if R > 1 else np.array([1])
    o = np.where((kind == 0)[:, None], r.uniform(-0.25, 0.25, (R, 3)),
                 np.where((kind == 1)[:, None], r.uniform(-1.5, 1.5, (R, 3)), r.uniform(2.0, 3.0, (R, 3)) * np.sign(r.standard_normal((R, 3))))).astype(f32)
    nears, fars = np.full(R, 0.05, f32), np.where(kind == 0, 0.6, 6.0).astype(f32)
    if R > 2:
        nears[1] = fars[1] = 0.5
    return F.Rays(o, d, nears, fars)


class Case(NamedTuple):
    nets: List[Net]
    rays: F.Rays
    P0: int
    P1: int
    S: int
    lin: bool
    lin0: np.ndarray          # [P0 + 1]
    u1: np.ndarray            # [P1 + 1]
    u2: np.ndarray            # [S + 1]
    jitter: Optional[np.ndarray] = None   # the device layout: [3, R] (one draw a ray and level) or [R, P0+1] | [R, P1+1] | [R, S+1], flat
    jper: bool = False
    anneal: float = 1.0

    @property
    def R(self) -> int:
        return len(self.rays.nears)

    @property
    def counts(self) -> Tuple[int, int, int]:
        return self.P0, self.P1, self.S

    def draws(self, level: int) -> Optional[np.ndarray]:
        """the level's stratified draws: [R] or [R, n + 1]"""
        if self.jitter is None:
            return None
        R, nb = self.R, [c + 1 for c in self.counts]
        if not self.jper:
            return self.jitter[level * R:(level + 1) * R]
        lo = R * sum(nb[:level])
        return self.jitter[lo:lo + R * nb[level]].reshape(R, nb[level])


def make_case(nets, rays, shape, lin: bool, jitter: Optional[str] = None, anneal: float = 1.0, seed: int = 0, u1=None, u2=None) -> Case:
    P0, P1, S = shape
    R = len(rays.nears)
    jit = None
    if jitter is not None:   # draws in [0, 1): below 1 after the cast to fp32 as well
        n = 3 * R if jitter == "ray" else R * (P0 + P1 + S + 3)
        jit = np.minimum(np.random.default_rng(seed + 5).random(n), 1.0 - 2.0 ** -24).astype(f32)
    u1 = RF.pdf_positions_fp32(P1 + 1, jitter) if u1 is None else np.asarray(u1, f32)
    u2 = RF.pdf_positions_fp32(S + 1, jitter) if u2 is None else np.asarray(u2, f32)
    return Case(nets, rays, P0, P1, S, lin, np.linspace(0.0, 1.0, P0 + 1).astype(f32), u1, u2, jit, jitter == "edge", anneal)


def planes(case: Case):
    return RF.spacing_fn_fp32(case.rays.nears, case.lin), RF.spacing_fn_fp32(case.rays.fars, case.lin)


# ----------------------------------------------------------------------------------------------------------------------
# the stages in fp64
# ----------------------------------------------------------------------------------------------------------------------
def level0_spacing(case: Case) -> np.ndarray:
    return sample_initial_fp32(case.lin0, case.draws(0), case.rays.nears, case.rays.fars, case.lin, case.jper)[0]


class Eucl(NamedTuple):
    value: np.ndarray   # [R, k] fp32: the torch-order model
    exact: np.ndarray   # [R, k] bool: no v_rcp_f32 on the way
    tol: np.ndarray     # [R, k]


def eucl_edges(case: Case, spacing) -> Eucl:
    b = np.asarray(spacing, f32)
    sn, sf = planes(case)
    e = spacing_to_eucl_fp32(b, sn, sf, case.lin)
    u = ((b * sf.reshape(-1, 1)).astype(f32) + ((f32(1) - b).astype(f32) * sn.reshape(-1, 1)).astype(f32)).astype(f32)
    exact = np.ones(b.shape, bool) if case.lin else (u < f32(0.5))
    return Eucl(e, exact, np.where(exact, 0.0, (K_RCP + 1.0) * U * np.abs(e.astype(f64))))


def check_eucl(name: str, case: Case, spacing, got) -> float:
    ref = eucl_edges(case, spacing)
    got = np.asarray(got, f32)
    same_bits(name + " (no v_rcp_f32)", np.where(ref.exact, got, f32(0)), np.where(ref.exact, ref.value, f32(0)))
    assert np.all(np.isfinite(got)), name
    err = np.abs(got.astype(f64) - ref.value.astype(f64))
    ratio = np.where(err > 0, err / np.maximum(ref.tol, 1e-300), 0.0)
    assert np.all(err <= ref.tol), (name, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))
    return float(ratio.max()) if ratio.size else 0.0


def density(net: Net, rays: F.Rays, eucl):
    """(density [R, n] fp64, bound, delta [R, n] fp32) of the samples between the given Euclidean edges: proposal_density's
    statements and counts, with __expf and the FAST contraction's bound carried through the features"""
    eucl = np.asarray(eucl, f32)
    R, n = eucl.shape[0], eucl.shape[1] - 1
    g = geometry(SPACE, rays.origins, rays.directions, np.zeros(R, f32), np.ones(R, f32), eucl, True, fast=True)
    assert np.array_equal(g.st, eucl[:, :-1]) and np.array_equal(g.en, eucl[:, 1:])   # the edges passed through unchanged
    enc, e_enc = F.encode(net.grid, g.p32, None, g.e_p)
    a0, e_a0 = F._layer(enc, e_enc, net.w0, net.b0, 0, F.MFMA)
    o, e_o = F._layer(np.maximum(a0, 0.0), e_a0, net.w1, net.b1, 0, F.MFMA)
    with np.errstate(over="ignore", invalid="ignore"):
        ex, e_ex = F._exp(o[:, 0], e_o[:, 0], True)
        sel = g.sel.astype(f64)
        dens = f64(net.avg) * ex * sel
        e_dens = (abs(net.avg) * e_ex + 2 * U * np.abs(f64(net.avg) * ex)) * sel
    over = dens - e_dens > FLT_MAX
    assert not np.any((dens + e_dens > FLT_MAX) & ~over), "a density within its bound of FLT_MAX"
    dens, e_dens = np.where(over, np.inf, dens), np.where(over, 0.0, e_dens)
    return dens.reshape(R, n), e_dens.reshape(R, n), g.delta


class WeightsRef(NamedTuple):
    weights: np.ndarray
    tol: np.ndarray
    pinned: np.ndarray


def level_weights(delta, dens, e_dens, family: str) -> WeightsRef:
    delta = np.asarray(delta, f32).astype(f64)
    R, n = delta.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = delta * dens
        fin = np.isfinite(a)
        e_a = np.where(fin, np.abs(delta) * e_dens + U * np.abs(a), 0.0)
        excl = lambda x: np.concatenate([np.zeros((R, 1)), np.cumsum(x, axis=1)[:, :-1]], axis=1)  # noqa: E731
        E, Eabs, e_sum = excl(a), excl(np.abs(a)), excl(e_a)
        e_E = np.where(np.isfinite(E), e_sum + k_e(family, n)[None, :] * U * Eabs, 0.0)
        E1, e_E1 = F._exp(-a, e_a, True)
        om = -np.expm1(-a)
        e_om = e_E1 + U * np.abs(om)
        E2, e_E2 = F._exp(-E, e_E, True)
        w = om * E2
        e_w = e_om * E2 + np.abs(om) * e_E2 + e_om * e_E2 + U * np.abs(w)
        e_w = np.where(a == np.inf, e_E2, e_w)   # alpha = 1 exactly: w = T
    pinned = ((a == 0) & (e_a == 0)) | np.isnan(a) | ~np.isfinite(E)
    w = np.where(pinned, 0.0, np.nan_to_num(w, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX))
    tol = np.where(pinned, 0.0, np.where(np.isfinite(e_w), e_w, 0.0) + U * np.abs(w) + TINY32)
    return WeightsRef(w, tol, pinned)


class Median(NamedTuple):
    value: np.ndarray      # [R] fp32
    index: np.ndarray
    near_tie: np.ndarray   # [R] bool


def median(weights, eucl, family: str) -> Median:
    w = np.asarray(weights, f32).astype(f64)
    R, n = w.shape
    e = np.asarray(eucl, f32)
    mid = RF.midpoints_fp32(e[:, :-1], e[:, 1:])
    cum = np.cumsum(w, axis=1)
    hit = cum >= 0.5
    idx = np.where(hit.any(1), hit.argmax(1), n - 1)
    rows = np.arange(R)
    near = lambda p: np.abs(p - 0.5) <= k_prefix(family, n) * U * np.abs(p)  # noqa: E731
    tie = near(cum[rows, idx]) | ((idx > 0) & near(cum[rows, np.maximum(idx - 1, 0)]))
    return Median(mid[rows, idx], idx, tie)


def annealed_fp32(weights, anneal: float) -> np.ndarray:
    w = np.asarray(weights, f32)
    if anneal == 1.0:
        return w
    with np.errstate(invalid="ignore"):
        return np.power(w.astype(f64), anneal).astype(f32)


def resample(case: Case, level: int, weights, spacing, family: str) -> RF.PdfRef:
    """the edges of level + 1 from the weights and spacing edges of ``level``"""
    n_out = case.counts[level + 1]
    u = case.u1 if level == 0 else case.u2
    n_in = np.asarray(weights).shape[1]
    return sample_pdf(annealed_fp32(weights, case.anneal), spacing, u, case.draws(level + 1), case.rays.nears, case.rays.fars, n_out, case.lin,
                      case.jper, k=k_cdf_family(family, n_in, case.anneal), k_t=K_T)


def sorted_within(name: str, edges, first, last):
    e = np.asarray(edges, f32)
    assert np.all(np.diff(e, axis=1) >= 0), (name, "edges decrease", np.argwhere(np.diff(e, axis=1) < 0)[:4].tolist())
    assert np.all(e >= np.asarray(first, f32).reshape(-1, 1)) and np.all(e <= np.asarray(last, f32).reshape(-1, 1)), (name, "edges outside the level")


OUTPUTS = ("spacing0", "spacing1", "spacing2", "eucl0", "eucl1", "eucl2", "weights0", "weights1", "depth0", "depth1", "ws")


def near_ties(case: Case, out: Dict[str, np.ndarray], family: str) -> np.ndarray:
    return median(out["weights0"], out["eucl0"], family).near_tie | median(out["weights1"], out["eucl1"], family).near_tie


def judge(name: str, case: Case, out: Dict[str, np.ndarray], family: str) -> Dict[str, float]:
    """every output of a general-form call, stage by stage from the outputs before it; returns the worst ratio to the bound by
    output (0 for what is held bit for bit)"""
    worst: Dict[str, float] = {}
    same_bits(f"{name} spacing0", out["spacing0"], level0_spacing(case))
    worst["spacing0"] = 0.0
    assert not near_ties(case, out, family).any(), (name, "a near tie of a median was not redrawn")
    for L in range(3):
        worst[f"eucl{L}"] = check_eucl(f"{name} eucl{L}", case, out[f"spacing{L}"], out[f"eucl{L}"])
    for L in range(2):
        sp, eu, w = out[f"spacing{L}"], out[f"eucl{L}"], out[f"weights{L}"]
        dens, e_dens, delta = density(case.nets[L], case.rays, eu)
        ref = level_weights(delta, dens, e_dens, family)
        within(f"{name} weights{L}", w, ref.weights, ref.tol)
        err = np.abs(np.asarray(w, f64) - ref.weights)
        worst[f"weights{L}"] = float(np.where(err > 0, err / np.maximum(ref.tol, 1e-300), 0.0).max())
        same_bits(f"{name} prop_depth_{L}", out[f"depth{L}"], median(w, eu, family).value)
        worst[f"depth{L}"] = 0.0
        pdf = resample(case, L, w, sp, family)
        nxt = out[f"spacing{L + 1}"]
        within(f"{name} spacing{L + 1}", nxt, pdf.spacing, pdf.tol)
        err = np.abs(np.asarray(nxt, f64) - pdf.spacing)
        worst[f"spacing{L + 1}"] = float(np.where(err > 0, err / np.maximum(pdf.tol, 1e-300), 0.0).max())
        sorted_within(f"{name} spacing{L + 1}", nxt, np.asarray(sp)[:, 0], np.asarray(sp)[:, -1])
    if case.jitter is None:
        sorted_within(f"{name} spacing0", out["spacing0"], case.lin0[:1], case.lin0[-1:])
    same_bits(f"{name} workspace edges", out["ws"], out["spacing2"])
    worst["ws"] = 0.0
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# fp32 op-by-op models of the two families (exp and the reciprocal correctly rounded), with plantable faults
# ----------------------------------------------------------------------------------------------------------------------
FAULTS = ("side_left", "no_padding", "own_a_in_transmittance", "seam_restart", "walk_block_no_break", "median_plus_one", "tail_other_edge",
          "idle_lane_store", "rcp_of_total")


def weights_model(a, family: str, fault: Optional[str] = None, seg: int = 0) -> np.ndarray:
    """a [R, n] fp32 = fl32(delta density).  Faults: own_a_in_transmittance (the sample's own a added first), seam_restart (the
    optical depth starts again at every ``seg``-th sample; the wave family: at every chunk of 64)"""
    a = np.asarray(a, f32)
    R, n = a.shape
    if family == WAVE:
        wf = {"own_a_in_transmittance": "inclusive", "seam_restart": "carry_dropped"}.get(fault)
        return RF.weights_fp32(a, np.ones_like(a), "wave", wf)
    w, accum = np.zeros((R, n), f32), np.zeros(R, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            if fault == "seam_restart" and seg and i and i % seg == 0:
                accum = np.zeros(R, f32)
            if fault == "own_a_in_transmittance":
                accum = (accum + a[:, i]).astype(f32)
            w[:, i] = RF.nan_to_num32(((f32(1) - RF.exp32(-a[:, i].astype(f64))).astype(f32) * RF.exp32(-accum.astype(f64))).astype(f32))
            if fault != "own_a_in_transmittance":
                accum = (accum + a[:, i]).astype(f32)
    return w


def median_model(w, family: str, fault: Optional[str] = None, block: int = 0) -> np.ndarray:
    w = np.asarray(w, f32)
    n = w.shape[1]
    cum = RF.prefix32(w, "wave" if family == WAVE else "sequential", "running")
    if fault == "walk_block_no_break" and block and n % block:   # the padded rounds count sample n - 1 again
        cum = cum.copy()
        cum[:, -1] = (cum[:, -1] + f32(block - n % block) * w[:, -1]).astype(f32)
    hit = cum >= f32(0.5)
    idx = np.where(hit.any(1), hit.argmax(1), n - 1)
    return np.minimum(idx + 1, n - 1) if fault == "median_plus_one" else idx


def resample_model(w, edges, uu, family: str, fault: Optional[str] = None, block: int = 0) -> np.ndarray:
    """pdf_walk (serial: the merge walk over a sorted CDF and sorted draws lands where searchsorted(side = right) does) or
    pdf_resample (wave) in fp32: w [R, n_in] (annealed), edges [R, n_in + 1], uu [R, n_out + 1] the draws -> [R, n_out + 1]"""
    w, ex, uu = np.asarray(w, f32), np.asarray(edges, f32), np.asarray(uu, f32)
    R, n_in = w.shape
    wpad = w if fault == "no_padding" else (w + f32(0.01)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        total = RF.sum32(wpad, "wave" if family == WAVE else "sequential")
        if fault == "walk_block_no_break" and block and n_in % block:
            for _ in range(block - n_in % block):
                total = (total + wpad[:, -1]).astype(f32)
        total = total[:, None]
        padding = np.maximum((f32(1e-5) - total).astype(f32), f32(0))
        pad_each = (padding / f32(n_in)).astype(f32)
        ws = (total + padding).astype(f32)
        rws = (f32(1) / (total if fault == "rcp_of_total" else ws)).astype(f32)
        pdf = ((wpad + pad_each).astype(f32) * rws).astype(f32)
        cum = RF.prefix32(pdf, "wave" if family == WAVE else "sequential", "running")
        cdf = np.concatenate([np.zeros((R, 1), f32), np.minimum(f32(1), cum)], axis=1)
        idx = RF._bisect(cdf, uu, left=(fault == "side_left"))
        below, above = np.clip(idx - 1, 0, n_in), np.clip(idx, 0, n_in)
        c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
        b0, b1 = np.take_along_axis(ex, below, 1), np.take_along_axis(ex, above, 1)
        if fault == "tail_other_edge":   # the draws at and behind the last knot get the last bin's OTHER edge
            b0 = np.where(idx > n_in, ex[:, n_in - 1:n_in], b0)
            b1 = np.where(idx > n_in, b0, b1)
        t = RF.nan_to_num32(((uu - c0).astype(f32) * (f32(1) / (c1 - c0).astype(f32)).astype(f32)).astype(f32))
        t = np.clip(t, f32(0), f32(1))
        return (b0 + (t * (b1 - b0).astype(f32)).astype(f32)).astype(f32)


def emulate(case: Case, family: str, fault: Optional[str] = None, split: bool = False) -> Dict[str, np.ndarray]:
    """an fp32 'device': every output of a general-form call.  The densities are the reference's, rounded to fp32.  split: the
    blocks and segment seams of the split form (RESAMPLE_BLOCK, segments of ceil(n / 8) and ceil(n / 4) samples)"""
    R = case.R
    sn, sf = planes(case)
    out: Dict[str, np.ndarray] = {}
    sp = level0_spacing(case)
    block = RESAMPLE_BLOCK if split else WALK_BLOCK
    for L in range(2):
        n = case.counts[L]
        eu = spacing_to_eucl_fp32(sp, sn, sf, case.lin)
        dens, _, delta = density(case.nets[L], case.rays, eu)
        with np.errstate(invalid="ignore", over="ignore"):
            a = (delta * dens.astype(f32)).astype(f32)
        w = weights_model(a, family, fault, -(-n // (8, 4)[L]))
        idx = median_model(w, family, fault, block if split else 0)
        out[f"spacing{L}"], out[f"eucl{L}"], out[f"weights{L}"] = sp, eu, w
        out[f"depth{L}"] = RF.midpoints_fp32(eu[:, :-1], eu[:, 1:])[np.arange(R), idx]
        n_out = case.counts[L + 1]
        uu = RF.draws_fp32(case.u1 if L == 0 else case.u2, case.draws(L + 1), R, n_out, case.jper)
        sp = resample_model(annealed_fp32(w, case.anneal), sp, uu, family, fault, block)
    out["spacing2"], out["eucl2"], out["ws"] = sp, spacing_to_eucl_fp32(sp, sn, sf, case.lin), sp.copy()
    if fault == "idle_lane_store" and R % 64:
        # a ragged tile's idle lanes load nothing (zeros) and store to the clamped ray index R - 1, after the live lane did.
        # This shows that ``judge`` sees a foreign row in ray R - 1, NOT that the kernels as written could be caught at it: their
        # idle lanes load ray R - 1's own inputs through the clamped index, so a stray store of theirs would write the same bits.
        # On the device only the ``live`` predicates and the guard rows behind every output stand against such a store.
        z = np.zeros((1, 3), f32)
        idle = emulate(case._replace(rays=F.Rays(z, z, np.zeros(1, f32), np.zeros(1, f32)),
                                     jitter=None if case.jitter is None else np.zeros_like(case.jitter)), family)
        for k in out:
            out[k] = out[k].copy()
            out[k][R - 1] = idle[k][0]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------------------------
Run = Callable[[Case], Dict[str, np.ndarray]]


def general_case(run: Run, family: str, nets, R: int, shape, lin: bool, seed: int, jitter=None, anneal: float = 1.0):
    """(case, outputs, redrawn share).  Walks four seeds until ``run`` (the device, or ``emulate``) leaves no ray with a near tie of
    either median; then redraws such rays one by one.  More than REDRAW_CAP of the rays redrawn is a failure."""
    for s in range(seed, seed + 4):
        case = make_case(nets, mixed_rays(R, s), shape, lin, jitter, anneal, s)
        out = run(case)
        bad = near_ties(case, out, family)
        if not bad.any():
            return case, out, 0.0
    redrawn = np.zeros(R, bool)
    for attempt in range(8):
        redrawn |= bad
        fresh = mixed_rays(R, seed + 100 + attempt)
        o, d = case.rays.origins.copy(), case.rays.directions.copy()
        o[bad], d[bad] = fresh.origins[bad], fresh.directions[bad]   # (a ray keeps its kind and planes: mixed_rays gives them by index)
        case = case._replace(rays=case.rays._replace(origins=o, directions=d))
        out = run(case)
        bad = near_ties(case, out, family)
        if not bad.any():
            break
    share = float(redrawn.mean())
    assert not bad.any() and share <= REDRAW_CAP, (share, "of the rays had to be redrawn")
    return case, out, share


def pinned_u(n_out: int) -> np.ndarray:
    """sorted caller-chosen draws: 0.0, a repeated value, 1.0 and a value above 1 among an even spread"""
    nb = n_out + 1
    u = np.sort(np.linspace(0.0, 0.95, nb)).astype(f32)
    if nb >= 6:
        u[nb // 2] = u[nb // 2 - 1]
        u[-2], u[-1] = 1.0, 1.25
    elif nb >= 2:
        u[-1] = 1.0
    u[0] = 0.0
    return u
