"""The per-ray kernels of a training step's backward chain and its losses on the device, element by element against the fp64
references of tests/ray_losses_reference.py: tn_ray_render_bwd, tn_weights_bwd, tn_composite_bwd, tn_distortion_loss[_term],
tn_interlevel_loss[_levels] and tn_image_losses.

Bit for bit: the dyadic distortion cases (gradient, and the loss of the light-weight ones), the single-active-interval interlevel
cases, tn_ray_render_bwd without heads against tn_weights_bwd, several interlevel levels in one launch against one at a time, the
image-loss gradients, every output a NULL head must leave alone.  Bounded per element by the counted constants of the reference
module (none tuned against what the device gives; run with -s for the worst ratio to the bound of every check): the rest.
Inputs are built on the CPU by the builders of the reference module and copied over; no element is skipped or masked."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from tests import ray_losses_reference as Q
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
TN_ERR_SHAPE = -2
N_EDGES = [1, 2, 63, 64, 65, 128, 129, 1024]


def dev(x, dtype=f32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def within(name, got, want, tol):
    """every element inside its bound; prints the worst ratio first"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    tol = np.broadcast_to(np.asarray(tol, f64), want.shape)
    assert got.shape == want.shape and np.all(np.isfinite(got)), name
    err = np.abs(got - want)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f"{name}: worst |device - fp64| / bound = {float(ratio.max()) if ratio.size else 0.0:.4f}")
    assert np.all(err <= tol), (name, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, name
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~((got == 0) & (want == 0))  # the sign of a zero is not part of the contract
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ----------------------------------------------------------------------------------------------------------------------
# tn_ray_render_bwd / tn_weights_bwd / tn_composite_bwd
# ----------------------------------------------------------------------------------------------------------------------
FILL = 7.0


def run_render_bwd(c: Q.RenderCase, rgb=True, th=True, acc=True, ext=True, scaled=True, n=None, expect=0):
    """-> (d_rgb_samples, d_thermal_samples, d_densities) as numpy, every output pre-filled with FILL"""
    R, nn = c.deltas.shape
    t = dict(dl=dev(c.deltas), dn=dev(c.densities), v=dev(c.rgb), th=dev(c.thermal), acc=dev(c.accumulation), g_rgb=dev(c.d_rgb),
             g_th=dev(c.d_thermal), g_acc=dev(c.d_accumulation), g_w=dev(c.d_weights), s=dev(c.starts), e=dev(c.ends))
    out_rgb = torch.full((R, nn, 3), FILL, device=DEV)
    out_th = torch.full((R, nn), FILL, device=DEV)
    out_d = torch.full((R, nn), FILL, device=DEV)
    code = _hip.load().tn_ray_render_bwd(
        ptr(t["dl"]), ptr(t["dn"]), ptr(t["v"]), ptr(t["th"]), ptr(t["acc"]), ptr(t["g_rgb"]) if rgb else None,
        ptr(t["g_th"]) if th else None, ptr(t["g_acc"]) if acc else None, ptr(t["g_w"]) if ext else None,
        ptr(t["s"]) if scaled else None, ptr(t["e"]) if scaled else None, R, nn if n is None else n, ptr(out_rgb), ptr(out_th),
        ptr(out_d), _hip.current_stream())
    assert code == expect, code
    res = host(out_rgb), host(out_th), host(out_d)
    del t
    return res


def render_reference(c, rgb=True, th=True, acc=True, ext=True, scaled=True):
    return Q.render_adjoint(c.deltas, c.densities, c.d_weights if ext else None, c.rgb if rgb else None, c.thermal if th else None,
                            c.accumulation, c.d_rgb if rgb else None, c.d_thermal if th else None,
                            c.d_accumulation if acc else None, c.starts if scaled else None, c.ends if scaled else None)


def check_render(name, c, got, rgb, th, acc, ext, scaled):
    ref = render_reference(c, rgb, th, acc, ext, scaled)
    within(f"{name} d_densities", got[2], ref.d_densities, Q.tolerance_render_densities(ref))
    if rgb:
        within(f"{name} d_rgb_samples", got[0], ref.d_rgb_samples, Q.tolerance_render_values(ref, c.d_rgb))
    else:
        assert np.all(got[0] == f32(FILL)), "d_rgb_samples written without d_rgb"
    if th:
        within(f"{name} d_thermal_samples", got[1], ref.d_thermal_samples, Q.tolerance_render_values(ref, c.d_thermal))
    else:
        assert np.all(got[1] == f32(FILL)), "d_thermal_samples written without d_thermal"


@pytest.mark.parametrize("R", [1, 3, 4, 5, 37])
@pytest.mark.parametrize("n", N_EDGES)
def test_ray_render_bwd_per_element(n, R):
    """all heads, with and without the distance-squared scaling: sample counts around the chunk of 64 and the 16-chunk limit, ray
    counts around the four rays of a block (the ragged last block is where ray >= R returns)"""
    c = Q.render_case(R, n, 1000 * n + R)
    for scaled in (True, False):
        got = run_render_bwd(c, scaled=scaled)
        check_render(f"render_bwd n={n} R={R} scaled={scaled}", c, got, True, True, True, True, scaled)


@pytest.mark.parametrize("rgb,th,acc,ext", list(itertools.product([True, False], repeat=4)))
def test_ray_render_bwd_every_null_branch(rgb, th, acc, ext):
    c = Q.render_case(5, 65, 17)
    for scaled in (True, False):
        got = run_render_bwd(c, rgb, th, acc, ext, scaled)
        check_render(f"render_bwd heads={int(rgb)}{int(th)}{int(acc)}{int(ext)} scaled={scaled}", c, got, rgb, th, acc, ext, scaled)


def test_ray_render_bwd_refuses_more_than_1024_samples():
    c = Q.render_case(3, 1025, 5)
    got = run_render_bwd(c, expect=TN_ERR_SHAPE)
    assert all(np.all(g == f32(FILL)) for g in got), "a refused call wrote"


def run_weights_bwd(deltas, dens, gw):
    R, n = deltas.shape
    a, b, g = dev(deltas), dev(dens), dev(gw)
    out = torch.full((R, n), FILL, device=DEV)
    _hip.check(_hip.load().tn_weights_bwd(ptr(a), ptr(b), ptr(g), R, n, ptr(out), _hip.current_stream()), "tn_weights_bwd")
    return host(out)


@pytest.mark.parametrize("n", N_EDGES)
def test_weights_bwd_per_element_and_ray_render_bwd_without_heads_is_the_same_kernel(n):
    R = 37
    c = Q.render_case(R, n, 77 + n)
    got = run_weights_bwd(c.deltas, c.densities, c.d_weights)
    ref = Q.render_adjoint(c.deltas, c.densities, c.d_weights)
    within(f"weights_bwd n={n}", got, ref.d_densities, Q.tolerance_render_densities(ref))
    # the two kernels run the same operations on d_w = ext + 0: bit for bit, from the code
    fused = run_render_bwd(c, rgb=False, th=False, acc=False, ext=True, scaled=False)
    same_bits(f"ray_render_bwd without heads == weights_bwd n={n}", fused[2], got)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 1024])
@pytest.mark.parametrize("C", [1, 3])
def test_composite_bwd_per_element(C, n):
    R = 41 if n <= 129 else 5
    rng = np.random.default_rng(100 * C + n)
    v, w = rng.random((R, n, C)).astype(f32), (rng.random((R, n)) / n).astype(f32)
    acc = w.astype(f64).sum(1).astype(f32)
    g, held = rng.standard_normal((R, C)).astype(f32), rng.standard_normal((R, n)).astype(f32)
    vd, wd, ad, gd = dev(v), dev(w), dev(acc), dev(g)
    gv, gw = torch.full((R, n, C), FILL, device=DEV), dev(held)
    _hip.check(_hip.load().tn_composite_bwd(ptr(vd), ptr(wd), ptr(ad), ptr(gd), R, n, C, ptr(gv), ptr(gw), _hip.current_stream()),
               "tn_composite_bwd")
    d_v, d_w, tol_v, tol_w = Q.composite_adjoint(v, w, acc, g, held)
    within(f"composite_bwd C={C} n={n} d_values", host(gv), d_v, tol_v)
    within(f"composite_bwd C={C} n={n} d_weights (+=)", host(gw), d_w, tol_w)


# ----------------------------------------------------------------------------------------------------------------------
# tn_distortion_loss / tn_distortion_loss_term
# ----------------------------------------------------------------------------------------------------------------------
def run_distortion(bins, w, scale, mult=None, start=(0.0, 0.0)):
    """-> (loss values [2] float32, gradient [R, n] float32); mult None: tn_distortion_loss (loss[1] must keep its start)"""
    R, n = w.shape
    b, wd = dev(bins), dev(w)
    loss = dev(np.asarray(start, f32))
    gw = torch.full((R, n), FILL, device=DEV)
    lib = _hip.load()
    if mult is None:
        _hip.check(lib.tn_distortion_loss(ptr(b), ptr(wd), R, n, scale, ptr(loss), ptr(gw), _hip.current_stream()), "tn_distortion_loss")
    else:
        _hip.check(lib.tn_distortion_loss_term(ptr(b), ptr(wd), R, n, scale, mult, ptr(loss), ptr(gw), _hip.current_stream()),
                   "tn_distortion_loss_term")
    return host(loss), host(gw)


@pytest.mark.parametrize("n,R", [(n, R) for n in (1, 2, 63, 64, 65, 200) for R in (1, 4, 64)] + [(5, 4096)])
def test_distortion_dyadic_cases_bit_for_bit(n, R):
    """R = 4096 with n = 5: every wave walks two rays and every block sum runs over eight"""
    scale = 1.0 / R
    bins, w = Q.dyadic_distortion_case(R, n, 3 * n + R, loss_exact=True)
    ref = Q.distortion(bins, w)
    loss, g = run_distortion(bins, w, scale)
    same_bits(f"distortion gradient n={n} R={R}", g, (scale * ref.grad).astype(f32))
    assert float(loss[0]) == scale * ref.loss.sum(), (loss[0], scale * ref.loss.sum())
    assert loss[1] == 0.0
    # the pair form at a power-of-two mult: metric, term and the TERM's gradient from one launch, still exact
    mult = 2.0 ** -9
    pair, g2 = run_distortion(bins, w, scale, mult)
    same_bits(f"distortion term gradient n={n} R={R}", g2, (scale * mult * ref.grad).astype(f32))
    assert float(pair[0]) == scale * ref.loss.sum() and float(pair[1]) == scale * mult * ref.loss.sum()
    # weights up to a sum of 4 per ray: the gradient is still exact, the loss bounded
    bins, w = Q.dyadic_distortion_case(R, n, 5 * n + R, loss_exact=False)
    ref = Q.distortion(bins, w)
    loss, g = run_distortion(bins, w, scale)
    same_bits(f"distortion gradient, heavy weights n={n} R={R}", g, (scale * ref.grad).astype(f32))
    within(f"distortion loss, heavy weights n={n} R={R}", loss[:1], [scale * ref.loss.sum()], Q.tolerance_distortion_loss(ref, scale))


@pytest.mark.parametrize("R,n,peaked", [(29, 48, False), (29, 65, False), (5, 200, False), (9, 1024, True), (2053, 5, False)])
def test_distortion_general_cases_per_element(R, n, peaked):
    bins, w = Q.general_distortion_case(R, n, R + n, peaked)
    ref = Q.distortion(bins, w)
    scale = float(f32(1.0 / R))
    loss, g = run_distortion(bins, w, scale)
    within(f"distortion gradient n={n} R={R}", g, scale * ref.grad, Q.tolerance_distortion(ref, scale))
    within(f"distortion loss n={n} R={R}", loss[:1], [scale * ref.loss.sum()], Q.tolerance_distortion_loss(ref, scale))
    # (+=) onto what loss_sum held; the pair form at the model's mult
    start, mult = (3.25, -1.5), float(f32(0.002))
    gscale = float(f32(scale) * f32(mult))
    pair, g2 = run_distortion(bins, w, scale, mult, start)
    within(f"distortion term gradient n={n} R={R}", g2, gscale * ref.grad, Q.tolerance_distortion(ref, gscale))
    within(f"distortion metric += n={n} R={R}", pair[:1], [start[0] + scale * ref.loss.sum()], Q.tolerance_distortion_loss(ref, scale, start[0]))
    within(f"distortion term += n={n} R={R}", pair[1:], [start[1] + gscale * ref.loss.sum()], Q.tolerance_distortion_loss(ref, gscale, start[1]))
    only, _ = run_distortion(bins, w, scale, None, start)
    assert only[1] == f32(start[1])
    within(f"distortion loss += n={n} R={R}", only[:1], [start[0] + scale * ref.loss.sum()], Q.tolerance_distortion_loss(ref, scale, start[0]))


# ----------------------------------------------------------------------------------------------------------------------
# tn_interlevel_loss / tn_interlevel_loss_levels
# ----------------------------------------------------------------------------------------------------------------------
def run_interlevel(c, w, levels, scale, start=0.0, single_entry=False, expect=0, p_override=None):
    """levels: [(cp, wp)] -> (loss float32, [gradient [R, p] float32 per level]), gradients pre-filled with FILL"""
    R, n = w.shape
    cd, wd = dev(c), dev(w)
    cps, wps = [dev(cp) for cp, _ in levels], [dev(wp) for _, wp in levels]
    ps = [wp.shape[1] for _, wp in levels] if p_override is None else list(p_override)
    outs = [torch.full(wp.shape, FILL, device=DEV) for _, wp in levels]
    loss = dev(np.asarray([start], f32))
    lib = _hip.load()
    if single_entry:
        code = lib.tn_interlevel_loss(ptr(cd), ptr(wd), ptr(cps[0]), ptr(wps[0]), R, n, ps[0], scale, ptr(loss), ptr(outs[0]),
                                      _hip.current_stream())
    else:
        L = len(levels)
        vp = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])  # noqa: E731
        code = lib.tn_interlevel_loss_levels(ptr(cd), ptr(wd), R, n, L, vp(cps), vp(wps), (C.c_int32 * L)(*ps), scale, ptr(loss),
                                             vp(outs), _hip.current_stream())
    assert code == expect, code
    res = host(loss)[0], [host(o) for o in outs]
    del cd, wd, cps, wps
    return res


INTERVAL_PARAMS = [(kind, p, n) for p in (1, 2, 63, 64, 65, 129, 1024) for n in (1, 48, 65) for kind in Q.interval_kinds(p)]


@pytest.mark.parametrize("kind,p,n", INTERVAL_PARAMS)
def test_interlevel_single_active_interval_exact(kind, p, n):
    """one d_i > 0 per ray: the gradient is fl32(scale fl32(coef)) on lo .. hi and 0 elsewhere in any order of the adds; a tie
    rule off by one moves the support by an element.  p = 1024 is the LDS opt-in size."""
    R = 6
    c, w, cp, wp, _ = Q.single_interval_case([kind], R, n, p, 131 * p + 7 * n + len(kind))
    ref = Q.interlevel(c, w, cp, wp)
    scale = float(f32(1.0 / (R * n)))
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], scale, single_entry=(n == 48))
    same_bits(f"interlevel {kind} p={p} n={n}", g, Q.interlevel_exact_gradient(ref, scale))
    within(f"interlevel loss {kind} p={p} n={n}", [loss], [scale * ref.loss.sum()], Q.tolerance_interlevel_loss([ref], scale, n))


@pytest.mark.parametrize("n,p", [(1, 1), (5, 7), (48, 64), (65, 129), (48, 1024), (1024, 63)])
def test_interlevel_general_cases_per_element(n, p):
    R = 24
    c, w, cp, wp = Q.general_interlevel_case(R, n, p, 11 * n + p)
    ref = Q.interlevel(c, w, cp, wp)
    scale = float(f32(1.0 / (R * n)))
    start = 0.75
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], scale, start)
    tol = Q.tolerance_interlevel(ref, scale)
    within(f"interlevel gradient n={n} p={p}", g, scale * ref.grad, tol)
    covered = (ref.m == 0)[:, 0]
    assert covered.any() and np.all(g[covered] == 0), "a ray under its envelope has a gradient"
    within(f"interlevel loss += n={n} p={p}", [loss], [start + scale * ref.loss.sum()], Q.tolerance_interlevel_loss([ref], scale, n, start))


@pytest.mark.parametrize("n,p", [(5, 7), (48, 64), (65, 129), (48, 1024)])
def test_interlevel_envelope_sum_over_zero_weights_is_not_negative(n, p):
    """rays under their envelope with weights off any grid: w = 0 and wp >= 0 give d = 0 for every interval, so the gradient is
    exactly 0 and the loss keeps its start, however the cumulative sum of wp is rounded.  Regression: the kernel took
    cum[hi + 1] - cum[lo] as it came; the wave scan's cum is not monotone over a run of zero weights, and 9 of 64 such rays had
    a gradient (up to 2.4 at scale 1) until w_outer was clamped at 0."""
    R = 64
    c, w, cp, wp = Q.covered_interlevel_case(R, n, p, 5 * n + p)
    ref = Q.interlevel(c, w, cp, wp)
    assert np.all(ref.m == 0) and np.all(ref.w_outer >= 0)
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], 1.0, start=0.5)
    print(f"interlevel covered rays n={n} p={p}: {int((g != 0).any(1).sum())} of {R} rays with a gradient, largest {np.abs(g).max():.3g}, "
          f"loss - start = {float(loss) - 0.5:.3g}")
    assert np.all(g == 0) and loss == 0.5


@pytest.mark.parametrize("n,p", [(5, 7), (65, 129)])
def test_interlevel_second_ray_of_a_wave(n, p):
    """R = 2053 > 512 blocks x 4 waves: rays r and r + 2048 share a wave and its LDS arrays; their supports differ, so a dhi / dlo
    value left over from the first would show in the second.  Exact, then the general cases bounded."""
    R = 2053
    kinds = Q.interval_kinds(p)
    c, w, cp, wp, _ = Q.single_interval_case(kinds, R, n, p, n + p)
    ref = Q.interlevel(c, w, cp, wp)
    want = Q.interlevel_exact_gradient(ref, 0.5)
    for r in range(R - 2048):
        assert not np.array_equal(want[r] != 0, want[r + 2048] != 0)
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], 0.5)
    same_bits(f"interlevel two rays per wave n={n} p={p}", g, want)
    within(f"interlevel loss two rays per wave n={n} p={p}", [loss], [0.5 * ref.loss.sum()], Q.tolerance_interlevel_loss([ref], 0.5, n))
    c, w, cp, wp = Q.general_interlevel_case(R, n, p, n * p)
    ref = Q.interlevel(c, w, cp, wp)
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], 0.5)
    within(f"interlevel general two rays per wave n={n} p={p}", g, 0.5 * ref.grad, Q.tolerance_interlevel(ref, 0.5))
    assert np.all(g[(ref.m == 0)[:, 0]] == 0)


@pytest.mark.parametrize("ps", [(7, 129), (64, 1024, 5, 65)])
def test_interlevel_levels_in_one_launch_equal_one_at_a_time(ps):
    R, n = 24, 48
    c, w, _, _ = Q.general_interlevel_case(R, n, ps[0], 3)
    levels = []
    for k, p in enumerate(ps):  # proposal levels of their own under the same final level
        _, _, cp, wp = Q.general_interlevel_case(R, n, p, 50 + k)
        levels.append((cp, wp))
    scale = float(f32(1.0 / (R * n)))
    loss, gs = run_interlevel(c, w, levels, scale)
    refs = []
    for (cp, wp), g, p in zip(levels, gs, ps):
        ref = Q.interlevel(c, w, cp, wp)
        refs.append(ref)
        _, (alone,) = run_interlevel(c, w, [(cp, wp)], scale)
        same_bits(f"interlevel level p={p} of {ps}", g, alone)
        within(f"interlevel level p={p} of {ps}", g, scale * ref.grad, Q.tolerance_interlevel(ref, scale))
    within(f"interlevel loss of {ps}", [loss], [scale * sum(r.loss.sum() for r in refs)], Q.tolerance_interlevel_loss(refs, scale, n))


def test_interlevel_refuses_p_1025_and_five_levels():
    R, n = 4, 5
    c, w, cp, wp = Q.general_interlevel_case(R, n, 7, 1)
    loss, (g,) = run_interlevel(c, w, [(cp, wp)], 1.0, start=2.0, expect=TN_ERR_SHAPE, p_override=[1025])
    assert loss == 2.0 and np.all(g == f32(FILL))
    loss, gs = run_interlevel(c, w, [(cp, wp)] * 5, 1.0, start=2.0, expect=TN_ERR_SHAPE)
    assert loss == 2.0 and all(np.all(g == f32(FILL)) for g in gs)


# ----------------------------------------------------------------------------------------------------------------------
# tn_image_losses
# ----------------------------------------------------------------------------------------------------------------------
def run_image_losses(rgb, gt, th=None, gt_th=None):
    R = rgb.shape[0]
    a, b, t, g = dev(rgb), dev(gt), dev(th), dev(gt_th)
    out = torch.zeros(3, device=DEV)
    d_rgb = torch.full((R, 3), FILL, device=DEV)
    d_th = torch.full((R, 1), FILL, device=DEV)
    _hip.check(_hip.load().tn_image_losses(ptr(a), ptr(b), ptr(t), ptr(g), R, ptr(out), ptr(d_rgb), ptr(d_th) if th is not None else None,
                                           _hip.current_stream()), "tn_image_losses")
    return host(out), host(d_rgb), host(d_th)


@pytest.mark.parametrize("R", [1, 341, 342, 1024, 1025, 4096])
def test_image_losses(R):
    """3 x 341 = 1023 and 3 x 342 = 1026 straddle the one block of 1024 threads"""
    rng = np.random.default_rng(R)
    rgb, gt = rng.random((R, 3)).astype(f32), rng.random((R, 3)).astype(f32)
    th, gt_th = rng.random((R, 1)).astype(f32), rng.random((R, 1)).astype(f32)
    ref = Q.image_losses(rgb, gt, th, gt_th)
    out, d_rgb, d_th = run_image_losses(rgb, gt, th, gt_th)
    same_bits(f"image_losses d_rgb R={R}", d_rgb, ref.d_rgb)
    same_bits(f"image_losses d_thermal R={R}", d_th, ref.d_thermal)
    within(f"image_losses mse rgb R={R}", out[:1], [ref.mse_rgb], Q.tolerance_mse(ref.mse_rgb, 3 * R))
    within(f"image_losses mse thermal R={R}", out[1:2], [ref.mse_thermal], Q.tolerance_mse(ref.mse_thermal, R))
    within(f"image_losses psnr R={R}", out[2:], [ref.psnr], Q.tolerance_psnr(ref.psnr, 3 * R))
    # thermal = NULL: out[1] stays 0, d_thermal is not touched
    out, d_rgb, d_th = run_image_losses(rgb, gt)
    same_bits(f"image_losses d_rgb without thermal R={R}", d_rgb, ref.d_rgb)
    assert out[1] == 0.0 and np.all(d_th == f32(FILL))
    within(f"image_losses mse rgb without thermal R={R}", out[:1], [ref.mse_rgb], Q.tolerance_mse(ref.mse_rgb, 3 * R))
    # identical images: MSE 0 and PSNR +inf, as oracle.hotpath.psnr gives
    out, d_rgb, d_th = run_image_losses(rgb, rgb, th, th)
    assert out[0] == 0.0 and out[1] == 0.0 and out[2] == math.inf and np.all(d_rgb == 0) and np.all(d_th == 0)
