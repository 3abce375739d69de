"""tests/ray_losses_reference.py against fp64 torch autograd over the CPU oracle and against cases worked by hand; its exact
families are exact; its counted bounds hold an fp32 emulation of each kernel's formula in two summation orders and do NOT hold
the planted faults (a bound that is too loose would let them in).  No device.  The device side: tests/test_gpu_ray_losses.py."""
import math

import numpy as np
import pytest
import torch

from oracle import hotpath as H
from oracle import training as T
from tests import ray_losses_reference as Q

f32, f64 = np.float32, np.float64


@pytest.fixture
def fp64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(prev)


def _t(x, grad=False):
    return torch.tensor(np.asarray(x, dtype=f64), requires_grad=grad)


def _close(got, want, mag, rel=1e-12):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    excess = np.abs(got - want) - rel * (np.abs(want) + mag)
    assert np.all(excess <= 0), float(excess.max())


HEADS = [(True, True, True, True, True), (False, False, False, True, False), (True, False, False, False, True),
         (False, True, True, False, False), (False, False, True, False, True), (True, True, False, True, False)]


def _render_args(c: Q.RenderCase, rgb, th, acc, ext, scaled, accumulation=None):
    return dict(d_weights=c.d_weights if ext else None, rgb=c.rgb if rgb else None, thermal=c.thermal if th else None,
                accumulation=c.accumulation if accumulation is None else accumulation, d_rgb=c.d_rgb if rgb else None,
                d_thermal=c.d_thermal if th else None, d_accumulation=c.d_accumulation if acc else None,
                starts=c.starts if scaled else None, ends=c.ends if scaled else None)


# ----------------------------------------------------------------------------------------------------------------------
# the references against fp64 autograd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb,th,acc,ext,scaled", HEADS)
@pytest.mark.parametrize("n", [1, 2, 65])
def test_render_adjoint_is_autograd_of_the_oracle(fp64_default, n, rgb, th, acc, ext, scaled):
    R = 19
    c = Q.render_case(R, n, 100 + n)
    a32 = (c.deltas * c.densities).astype(f32)
    # the oracle multiplies delta and density itself: hand it delta = 1 and density = the rounded product, and chain delta back in
    a = _t(a32, True)
    v, t = _t(c.rgb, True), _t(c.thermal, True)
    outs = {"a": a[..., None], "rgb": v, "thermal": t[..., None]}
    if scaled:
        outs = H.scale_gradients_by_distance_squared(outs, _t(c.starts)[..., None], _t(c.ends)[..., None])
    w = H.get_weights(torch.ones(R, n, 1), outs["a"])
    total = torch.zeros(())
    if rgb:
        total = total + (H.render_rgb(outs["rgb"], w, True) * _t(c.d_rgb)).sum()
    if th:
        total = total + (H.render_thermal(outs["thermal"], w, True)[..., 0] * _t(c.d_thermal)).sum()
    if acc:
        total = total + (H.render_accumulation(w)[..., 0] * _t(c.d_accumulation)).sum()
    if ext:
        total = total + (w[..., 0] * _t(c.d_weights)).sum()
    if not (rgb or th or acc or ext):
        pytest.fail("no head")
    total.backward()
    acc64 = w.detach().numpy()[..., 0].sum(1)
    ref = Q.render_adjoint(c.deltas, c.densities, **_render_args(c, rgb, th, acc, ext, scaled, accumulation=acc64))
    m = ref.mag
    np.testing.assert_allclose(ref.weights, w.detach().numpy()[..., 0], rtol=1e-12, atol=1e-300)
    _close(ref.d_densities, a.grad.numpy() * c.deltas.astype(f64), m["delta"] * m["scale"] * m["tail"])
    if rgb:
        _close(ref.d_rgb_samples, v.grad.numpy(), np.abs(c.d_rgb.astype(f64))[:, None, :])  # the last sample's 1 - acc cancels
    if th:
        _close(ref.d_thermal_samples, t.grad.numpy(), np.abs(c.d_thermal.astype(f64))[:, None])


@pytest.mark.parametrize("C", [1, 3])
def test_composite_adjoint_is_autograd_of_the_oracle(fp64_default, C):
    rng = np.random.default_rng(C)
    R, n = 7, 5
    v32, w32 = rng.random((R, n, C)).astype(f32), (rng.random((R, n)) / n).astype(f32)
    g32, held = rng.standard_normal((R, C)).astype(f32), rng.standard_normal((R, n)).astype(f32)
    v, w = _t(v32, True), _t(w32, True)
    out = (H.render_rgb if C == 3 else H.render_thermal)(v, w[..., None], True)
    (out * _t(g32)).sum().backward()
    d_v, d_w, tol_v, tol_w = Q.composite_adjoint(v32, w32, w32.astype(f64).sum(1), g32, held)
    _close(d_v, v.grad.numpy(), np.abs(g32.astype(f64))[:, None, :])
    _close(d_w - held, w.grad.numpy(), np.abs(held))
    assert np.all(tol_v > 0) and np.all(tol_w > 0)


@pytest.mark.parametrize("n", [1, 3, 65])
def test_distortion_is_the_oracle_and_its_autograd(fp64_default, n):
    bins, w32 = Q.general_distortion_case(11, n, n)
    # the reference keeps the kernel's fp32 mid-points: give the oracle edges that reproduce them (t_i' = u_i -+ d_i / 2 would
    # not be fp32; so compare on dyadic edges, where fl32((t0 + t1) / 2) is exact) and on the general ones to fp32's accuracy
    for b, rel in ((Q.dyadic_distortion_case(11, n, n)[0], 1e-12), (bins, 1e-6)):
        w = _t(w32, True)
        per_ray = T.lossfun_distortion(_t(b), w)
        per_ray.sum().backward()
        ref = Q.distortion(b, w32)
        _close(ref.loss, per_ray.detach().numpy(), ref.loss_abs, rel)
        _close(ref.grad, w.grad.numpy(), 2 * ref.B, rel)


@pytest.mark.parametrize("n,p", [(1, 1), (5, 7), (65, 129), (48, 2)])
def test_interlevel_is_the_oracle_and_its_autograd(fp64_default, n, p):
    for builder in ("general", "single"):
        if builder == "general":
            c, w32, cp, wp32 = Q.general_interlevel_case(13, n, p, n + p)
        else:
            c, w32, cp, wp32, _ = Q.single_interval_case(Q.interval_kinds(p), 13, n, p, n + p)
        wp = _t(wp32, True)
        # the oracle's den is w + 1e-7 in fp64, the kernel's (and the reference's) is fl32(w + 1e-7f): the oracle's envelope
        # (searches, clamps, cumulative sums) with the fp32 den first, then its own loss to the difference of the two dens
        ct, cpt = _t(c), _t(cp)
        w_outer = T.outer(ct[:, :-1], ct[:, 1:], cpt[:, :-1], cpt[:, 1:], wp)
        ref = Q.interlevel(c, w32, cp, wp32)
        _close(ref.w_outer, w_outer.detach().numpy(), 0.0)
        den = _t((w32 + f32(1.0e-7)).astype(f32))
        per = torch.clip(_t(w32) - w_outer, min=0) ** 2 / den
        per.sum().backward()
        _close(ref.loss, per.sum(-1).detach().numpy(), 0.0)
        _close(ref.grad, wp.grad.numpy(), ref.B)
        own = T.lossfun_outer(ct, _t(w32), cpt, wp.detach()).sum(-1).numpy()
        assert np.all(np.abs(own - ref.loss) <= 2 * Q.EPS32 * ref.loss)  # den: one fp32 rounding, 1e-7f against 1e-7


@pytest.mark.parametrize("R", [1, 342])
def test_image_losses_are_the_oracle_and_its_autograd(fp64_default, R):
    rng = np.random.default_rng(R)
    a, b = rng.random((R, 3)).astype(f32), rng.random((R, 3)).astype(f32)
    t, g = rng.random((R, 1)).astype(f32), rng.random((R, 1)).astype(f32)
    at, tt = _t(a, True), _t(t, True)
    l3, l1 = torch.nn.functional.mse_loss(_t(b), at), torch.nn.functional.mse_loss(tt, _t(g))
    (l3 + l1).backward()
    ref = Q.image_losses(a, b, t, g)
    assert abs(ref.mse_rgb - l3.item()) <= 1e-12 * l3.item() and abs(ref.mse_thermal - l1.item()) <= 1e-12 * l1.item()
    assert abs(ref.psnr - H.psnr(at.detach(), _t(b)).item()) <= 1e-10
    # the two-rounding fp32 gradients are within two roundings of the fp64 ones
    assert np.all(np.abs(ref.d_rgb - at.grad.numpy()) <= 3 * Q.EPS32 * np.abs(at.grad.numpy()) + 1e-45)
    assert np.all(np.abs(ref.d_thermal - tt.grad.numpy()) <= 3 * Q.EPS32 * np.abs(tt.grad.numpy()) + 1e-45)
    same = Q.image_losses(a, a)
    assert same.mse_rgb == 0.0 and same.psnr == math.inf and same.mse_thermal is None and same.d_thermal is None
    assert np.all(same.d_rgb == 0) and torch.isposinf(H.psnr(_t(a), _t(a)))


# ----------------------------------------------------------------------------------------------------------------------
# worked by hand
# ----------------------------------------------------------------------------------------------------------------------
def test_render_adjoint_two_sample_ray_by_hand():
    d0, d1, s0, s1 = 0.5, 2.0, 1.0, 0.25         # a = (0.5, 0.5), both products exact
    v = [[0.25, 0.5, 0.75], [1.0, 0.0, 0.5]]
    th, g_rgb, g_th, g_acc, g_ext = [0.125, 0.625], [1.0, -2.0, 0.5], 3.0, -1.0, [0.5, -0.25]
    e = math.exp(-0.5)
    w0, w1 = 1 - e, (1 - e) * e
    acc = f32(w0 + w1)
    dw0 = g_ext[0] + g_acc + sum(g * (a - b) for g, a, b in zip(g_rgb, v[0], v[1])) + g_th * (th[0] - th[1])
    dw1 = g_ext[1] + g_acc                        # the last sample's own colour terms vanish
    want_dens = [d0 * (dw0 * e * 1.0 - dw1 * w1), d1 * (dw1 * e * e - 0.0)]
    bg = 1.0 - float(acc)
    want_rgb = [[g * w0 for g in g_rgb], [g * (w1 + bg) for g in g_rgb]]
    want_th = [g_th * w0, g_th * (w1 + bg)]
    starts, ends = [[0.5, 1.5]], [[1.0, 3.5]]     # mid-points 0.75 and 2.5: scales 0.5625 and 1
    for scaled, sc in ((False, (1.0, 1.0)), (True, (0.5625, 1.0))):
        ref = Q.render_adjoint([[d0, d1]], [[s0, s1]], [g_ext], [v], [th], [acc], [g_rgb], [g_th], [g_acc],
                               starts if scaled else None, ends if scaled else None)
        np.testing.assert_allclose(ref.d_densities[0], [want_dens[0] * sc[0], want_dens[1] * sc[1]], rtol=1e-14)
        np.testing.assert_allclose(ref.d_rgb_samples[0], [[x * sc[0] for x in want_rgb[0]], [x * sc[1] for x in want_rgb[1]]], rtol=1e-14)
        np.testing.assert_allclose(ref.d_thermal_samples[0], [want_th[0] * sc[0], want_th[1] * sc[1]], rtol=1e-14)


def test_distortion_three_bins_by_hand():
    ref = Q.distortion([[0.0, 0.25, 0.5, 1.0]], [[0.5, 0.25, 0.25]])  # u = 0.125, 0.375, 0.75; d = 0.25, 0.25, 0.5
    S = [0.25 * 0.25 + 0.25 * 0.625, 0.5 * 0.25 + 0.25 * 0.375, 0.5 * 0.625 + 0.25 * 0.375]
    assert S == [0.21875, 0.21875, 0.40625]
    np.testing.assert_allclose(ref.loss, [0.265625 + 0.109375 / 3], rtol=1e-15)
    np.testing.assert_allclose(ref.grad[0], [0.4375 + 0.25 / 3, 0.4375 + 0.125 / 3, 0.8125 + 0.25 / 3], rtol=1e-15)
    np.testing.assert_allclose(ref.B[0, 0], 1.0 * 0.125 + (0.0625 + 0.09375 + 0.1875) + 0.5 * 0.25 / 3, rtol=1e-15)


def test_interlevel_two_in_three_by_hand_with_and_without_a_tie():
    cp, wp, w = [[0.0, 0.25, 0.5, 1.0]], [[0.125, 0.25, 0.125]], [[0.5, 0.5]]
    den = float(f32(0.5) + f32(1.0e-7))
    tie = Q.interlevel([[0.125, 0.25, 0.75]], w, cp, wp)          # the shared edge 0.25 IS a proposal edge
    assert tie.lo.tolist() == [[0, 1]] and tie.hi.tolist() == [[1, 2]]  # side="right": [0.125, 0.25] reaches into bin 1,
    np.testing.assert_array_equal(tie.w_outer, [[0.375, 0.375]])        # [0.25, 0.75] starts in bin 1
    np.testing.assert_allclose(tie.grad, [[-0.25 / den, -0.5 / den, -0.25 / den]], rtol=1e-15)
    np.testing.assert_allclose(tie.loss, [2 * 0.125 ** 2 / den], rtol=1e-15)
    below = float(np.nextafter(f32(0.25), f32(0)))
    off = Q.interlevel([[0.125, below, 0.75]], w, cp, wp)          # one ulp below it
    assert off.lo.tolist() == [[0, 0]] and off.hi.tolist() == [[0, 2]]
    np.testing.assert_array_equal(off.w_outer, [[0.125, 0.5]])
    np.testing.assert_allclose(off.grad, [[-0.75 / den, 0.0, 0.0]], rtol=1e-15)
    assert off.m.tolist() == [[1]] and off.B[0, 0] == 0.75 / den
    np.testing.assert_array_equal(Q.interlevel_exact_gradient(off, 0.5)[0], [f32(0.5) * f32(-0.75 / den), 0, 0])


# ----------------------------------------------------------------------------------------------------------------------
# the exact families
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n,loss_exact", [(64, 48, True), (64, 200, True), (4, 1, True), (1, 2, True), (4096, 5, True),
                                            (64, 200, False), (4, 65, False), (64, 63, False)])
def test_dyadic_distortion_cases_are_exact_in_fp32(R, n, loss_exact):
    bins, w = Q.dyadic_distortion_case(R, n, 7 * n + R, loss_exact)
    assert np.all(np.diff(bins, axis=1) >= 0) and bins.min() >= 0 and bins.max() <= 1
    assert np.all(bins * 1024 / 3 == np.round(bins * 1024 / 3)) and np.all(w * 64 == np.round(w * 64)) and w.sum(1).max() <= 4
    if R >= 5 and n > 2:
        assert (w.sum(1) > 1).any() and (w == 0).any() and ((w > 0).sum(1) == 1).any() and (np.diff(bins, axis=1) == 0).any()
    ref = Q.distortion(bins, w)
    b64, w64 = bins.astype(f64), w.astype(f64)
    u, d = (b64[:, 1:] + b64[:, :-1]) / 2, b64[:, 1:] - b64[:, :-1]
    exact = lambda x: np.array_equal(np.asarray(x, f64), np.asarray(x, f64).astype(f32).astype(f64))  # noqa: E731
    # every intermediate of the kernel's form, from fp64 values: mid-points, d / 3, the products, every prefix and suffix sum
    pre = lambda x: np.cumsum(x, axis=1) - x  # noqa: E731
    Wlt, WUlt = pre(w64), pre(w64 * u)
    Wgt, WUgt = w64.sum(1, keepdims=True) - Wlt - w64, (w64 * u).sum(1, keepdims=True) - WUlt - w64 * u
    S = u * (Wlt - Wgt) - (WUlt - WUgt)
    np.testing.assert_array_equal(2 * S + 2 * w64 * d / 3, ref.grad)  # the O(n) form IS the O(n^2) form on these inputs
    for x in (u, d / 3, w64 * u, Wlt, WUlt, Wgt, WUgt, Wlt - Wgt, u * (Wlt - Wgt), WUlt - WUgt, S, 2 * w64 * d, 2 * w64 * d / 3,
              ref.grad, ref.grad / 64):
        assert exact(x)
    # every term is a multiple of 2^-17 and a ray's absolute sums stay below 2^7 = 2^24 2^-17: exact in ANY order
    for x in (w64, w64 * u, ref.grad):
        assert np.all(x * 2 ** 17 == np.round(x * 2 ** 17))
    assert 2 * ref.B.max() < 2 ** 7
    for pairwise in (False, True):
        g, loss = Q.distortion_fp32(bins, w, pairwise)
        np.testing.assert_array_equal(g.astype(f64), ref.grad)
        if loss_exact:
            np.testing.assert_array_equal(loss.astype(f64), ref.loss)
    if loss_exact:
        terms = w64 * S + w64 * w64 * d / 3
        for x in (w64 * S, w64 * w64, w64 * w64 * d, w64 * w64 * d / 3, terms, ref.loss):
            assert exact(x)
        assert np.all(terms >= 0) and np.all(terms * 2 ** 23 == np.round(terms * 2 ** 23)) and terms.sum() < 2.0
        np.testing.assert_array_equal(terms.sum(1), ref.loss)


@pytest.mark.parametrize("p", [1, 2, 3, 64, 65, 1024])
@pytest.mark.parametrize("n", [1, 48, 65])
def test_single_interval_cases_have_one_active_interval_where_they_say(n, p):
    kinds = Q.interval_kinds(p)
    assert set(kinds) >= {"inside_one_bin", "spans_all", "starts_at_cp0", "ends_at_cpp", "left_of_cp0", "right_of_cpp", "zero_width"}
    assert p < 3 or kinds == list(Q.INTERVAL_KINDS)
    R = 2 * len(kinds)
    c, w, cp, wp, active = Q.single_interval_case(kinds, R, n, p, 31 * n + p)
    assert np.all(np.diff(c, axis=1) >= 0) and np.all(np.diff(cp, axis=1) >= 0)
    ref = Q.interlevel(c, w, cp, wp)
    rows = np.arange(R)
    assert np.all(ref.m == 1) and np.all(ref.d[rows, active] > 0)
    lo, hi, s, e = ref.lo[rows, active], ref.hi[rows, active], c[rows, active], c[rows, active + 1]
    interior = cp[:, 1:-1]
    for r in range(R):
        kind = kinds[r % len(kinds)]
        on = lambda x: bool((interior[r] == x).any())  # noqa: E731
        dup = np.nonzero(np.diff(cp[r]) == 0)[0]
        want = {"start_on_edge": on(s[r]) and not on(e[r]), "end_on_edge": on(e[r]) and not on(s[r]),
                "both_on_edges": on(s[r]) and on(e[r]), "inside_one_bin": lo[r] == hi[r] and cp[r, lo[r]] < s[r] < e[r] < cp[r, lo[r] + 1],
                "spans_all": lo[r] == 0 and hi[r] == p - 1 and s[r] > cp[r, 0] and e[r] < cp[r, -1],
                "starts_at_cp0": s[r] == cp[r, 0] and lo[r] == 0, "ends_at_cpp": e[r] == cp[r, -1] and hi[r] == p - 1,
                "left_of_cp0": e[r] < cp[r, 0] and lo[r] == 0 and hi[r] == 0,
                "right_of_cpp": s[r] > cp[r, -1] and lo[r] == p - 1 and hi[r] == p - 1,
                "after_duplicates": len(dup) > 0 and s[r] == cp[r, dup[0]] and lo[r] == dup[-1] + 1,  # right: past the whole run
                "before_duplicates": len(dup) > 0 and e[r] == cp[r, dup[0]] and hi[r] == dup[-1] + 1,
                "zero_width": s[r] == e[r] and not on(s[r]), "zero_width_on_edge": s[r] == e[r] and on(s[r])}[kind]
        assert want, (kind, r, s[r], e[r], lo[r], hi[r])
    # cum, w_outer and d are exact in fp32; the emulation gives the expected bits in both orders; a moved tie rule does not
    assert np.array_equal(ref.d, ref.d.astype(f32)) and np.array_equal(ref.w_outer, ref.w_outer.astype(f32))
    want = Q.interlevel_exact_gradient(ref, 0.375)
    assert np.all((want != 0).sum(1) == hi - lo + 1)
    for pairwise in (False, True):
        np.testing.assert_array_equal((f32(0.375) * Q.interlevel_fp32(c, w, cp, wp, pairwise)).astype(f32), want)
    if p >= 3:
        for shift in ((1, 0), (0, -1), (-1, 0), (0, 1)):
            moved = (f32(0.375) * Q.interlevel_fp32(c, w, cp, wp, False, *shift)).astype(f32)
            assert not np.array_equal(moved, want), shift


# ----------------------------------------------------------------------------------------------------------------------
# the counted constants: the emulations inside, the planted faults outside
# ----------------------------------------------------------------------------------------------------------------------
def _render_excess(c, args, **kw):
    ref = Q.render_adjoint(c.deltas, c.densities, **args)
    rgb, th, dens = Q.render_adjoint_fp32(c.deltas, c.densities, **args, **kw)
    out = {"dens": (np.abs(dens - ref.d_densities) / Q.tolerance_render_densities(ref)).max()}
    if rgb is not None:
        out["rgb"] = (np.abs(rgb - ref.d_rgb_samples) / Q.tolerance_render_values(ref, c.d_rgb)).max()
    if th is not None:
        out["th"] = (np.abs(th - ref.d_thermal_samples) / Q.tolerance_render_values(ref, c.d_thermal)).max()
    return out


@pytest.mark.parametrize("n", [2, 65, 129, 1024])
def test_render_bound_holds_the_emulation_and_not_the_faults(n):
    c = Q.render_case(19, n, n)
    for heads in HEADS:
        args = _render_args(c, *heads)
        for pairwise in (False, True):
            worst = _render_excess(c, args, pairwise=pairwise)
            assert max(worst.values()) <= 1.0, (heads, pairwise, worst)
    full = _render_args(c, True, True, True, True, True)
    assert _render_excess(c, full, fault="drop_suffix_term")["dens"] > 1.0
    no_bg = _render_excess(c, full, fault="no_background")
    assert no_bg["rgb"] > 1.0 and no_bg["th"] > 1.0
    two = _render_excess(c, full, fault="scale_two_of_three")
    assert two["th"] > 1.0 and two["rgb"] <= 1.0 and two["dens"] <= 1.0


@pytest.mark.parametrize("n,peaked", [(3, False), (65, False), (200, False), (1024, True)])
def test_distortion_bound_holds_the_emulation_and_not_the_fault(n, peaked):
    bins, w = Q.general_distortion_case(9, n, n, peaked)
    ref = Q.distortion(bins, w)
    tol = Q.tolerance_distortion(ref, 1.0)
    for pairwise in (False, True):
        g, loss = Q.distortion_fp32(bins, w, pairwise)
        assert (np.abs(g - ref.grad) / tol).max() <= 1.0
        assert np.all(np.abs(loss - ref.loss) <= Q.k_distortion_loss(1, n) * Q.EPS32 * ref.loss_abs)
    g, _ = Q.distortion_fp32(bins, w, fault="gt_keeps_own")
    assert (np.abs(g - ref.grad) / tol).max() > 1.0


@pytest.mark.parametrize("n,p", [(5, 7), (65, 129), (48, 1024), (65, 64)])
def test_interlevel_bound_holds_the_emulation_and_not_the_faults(n, p):
    c, w, cp, wp = Q.general_interlevel_case(24, n, p, n * p)
    ref = Q.interlevel(c, w, cp, wp)
    assert (ref.m == 0).any() and (ref.m > 1).any() and (w == 0).any() and (wp == 0).any()
    assert (np.diff(c, axis=1) == 0).any() or n < 5
    assert np.array_equal(ref.d, ref.d.astype(f32)) and np.array_equal(ref.w_outer, ref.w_outer.astype(f32))
    tol = Q.tolerance_interlevel(ref, 1.0)
    assert np.all(tol[ref.m == 0] == 0)
    for pairwise in (False, True):
        g = Q.interlevel_fp32(c, w, cp, wp, pairwise)
        assert np.all(np.abs(g - ref.grad) <= tol)
    for kw in (dict(shift_lo=1), dict(shift_hi=-1), dict(drop=True)):
        g = Q.interlevel_fp32(c, w, cp, wp, **kw)
        assert np.any(np.abs(g - ref.grad) > tol), kw


def test_wave_scan_emulation_sums_prefixes():
    x = np.random.default_rng(0).integers(-8, 9, size=(5, 64)).astype(f32)  # integers: exact in any grouping
    np.testing.assert_array_equal(Q.wave_scan_fp32(x), np.cumsum(x, axis=1))
    wp = np.random.default_rng(1).integers(0, 9, size=(3, 200)).astype(f32)
    np.testing.assert_array_equal(Q.envelope_cum_fp32(wp)[:, 1:], np.cumsum(wp, axis=1))
    assert np.all(Q.envelope_cum_fp32(wp)[:, 0] == 0)


@pytest.mark.parametrize("n,p", [(48, 64), (65, 129)])
def test_envelope_over_zero_weights_needs_its_clamp(n, p):
    """the regression behind test_interlevel_envelope_sum_over_zero_weights_is_not_negative: the wave scan's cum is not monotone over
    a run of zero weights; without max(w_outer, 0) rays with w = 0 under a nonnegative envelope get coefficients of order 1"""
    c, w, cp, wp = Q.covered_interlevel_case(64, n, p, 5 * n + p)
    ref = Q.interlevel(c, w, cp, wp)
    assert np.all(ref.m == 0) and np.all(ref.grad == 0) and np.all(ref.loss == 0)
    cum = Q.envelope_cum_fp32(wp)
    assert (np.diff(cum, axis=1) < 0).any(), "this case does not show the wobble"
    assert np.all(Q.interlevel_fp32(c, w, cp, wp, wave=True) == 0)
    bad = Q.interlevel_fp32(c, w, cp, wp, wave=True, clamp=False)
    assert np.abs(bad).max() > 0.05


def test_counted_constants_are_what_the_docstring_counts():
    assert (Q.K_EXP, Q.K_LOG10, Q.K_E, Q.K_DW, Q.K_SUFFIX, Q.K_TAIL) == (3, 6, 6 + 15 + 1, 6, 6 + 1 + 15 + 1, 5)
    assert Q.K_EXP >= 2 * 1.3863 and Q.K_LOG10 >= 2 * 2.8206      # profiles/micro/libm_accuracy.txt, margin 2x
    assert (Q.k_distortion(64), Q.k_distortion(65), Q.k_distortion(1024)) == (38, 41, 83)
    assert Q.K_INTERLEVEL == 26 and Q.k_mse(3) == 25 and Q.k_mse(3 * 4096) == 36
    assert Q.loss_blocks(1) == 1 and Q.loss_blocks(2053) == 512 and Q.loss_blocks(4096) == 512
