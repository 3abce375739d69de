"""tests/ray_forward_reference.py against the CPU oracle on the inputs of the parity tests; its exact families are what they
promise; its counted bounds hold the fp32 model of each kernel in its summation orders and do NOT hold the planted faults: for
every fault the very check the GPU test applies (within / same_bits of the reference module) fails on a shape the GPU test uses.
No device.  The device side: tests/test_gpu_ray_forward.py.

Summation orders.  On the exact families all three orders (sequential, pairwise, the 64-lane wave scan with chunk carry) must give
the reference's bits at every size.  On the general families the counts are those of the kernels' trees (a 6-deep scan, a carry
per chunk, a lane partial over the chunks): the wave order is that tree, and a pairwise (Hillis-Steele) prefix is ceil(log2 n)
adds deep, which is inside every count here, so both are asserted at every size.  A SEQUENTIAL sum has n - 1 roundings on its
longest path; no count of a 6-deep scan can hold it beyond n = 7, so on the general families it is asserted for n <= 7 only."""
import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import ray_forward_reference as F

f32, f64 = np.float32, np.float64


def orders_for(n):
    return F.ORDERS if n <= 7 else ("pairwise", "wave")


def ratio(got, ref, tol):
    return float((np.abs(np.asarray(got, f64) - ref) / tol).max())


def test_counted_constants_are_what_the_docstring_counts():
    assert [F.k_e_fwd(n) for n in (1, 64, 65, 128, 129, 1024)] == [6, 6, 7, 7, 8, 21]
    assert [F.k_cdf(n) for n in (1, 64, 65, 1024)] == [16, 16, 18, 46]
    assert [F.k_composite(n) for n in (64, 65, 1024)] == [8, 9, 23] and [F.k_acc(n) for n in (64, 1024)] == [6, 21]
    assert [F.k_prefix(n) for n in (64, 1024)] == [8, 23]
    assert F.K_EXP == 3 and F.EPS32 == 2.0 ** -24
    assert sorted({s[0] for s in F.PDF_SHAPES}) == F.N_EDGES and sorted({s[1] for s in F.PDF_SHAPES}) == F.N_OUT_EDGES


def test_wave_orders_sum_what_they_say():
    x = np.random.default_rng(0).integers(-8, 9, size=(5, 200)).astype(f32)  # integers: exact in any grouping
    for order in F.ORDERS:
        for carry in ("running", "accumulated"):
            np.testing.assert_array_equal(F.prefix32(x, order, carry), np.cumsum(x, axis=1))
        np.testing.assert_array_equal(F.sum32(x, order), x.sum(1))
        restarted = F.prefix32(x, order, drop_carry=True)
        np.testing.assert_array_equal(restarted[:, 64:128], np.cumsum(x[:, 64:128], axis=1))


# ----------------------------------------------------------------------------------------------------------------------
# the references against oracle/hotpath.py, on the inputs of tests/test_gpu_parity.py, to the oracle's fp32 accuracy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,n_out", [(256, 96), (96, 48), (96, 64), (96, 192), (64, 300)])
def test_sample_pdf_is_the_oracle(n_in, n_out):
    g = torch.Generator().manual_seed(n_in * 1000 + n_out)
    R = 29
    nears, fars = torch.zeros(R, 1), torch.full((R, 1), 1000.0)
    prev = H.sample_initial(nears, fars, n_in, None)
    w = torch.rand(R, n_in, 1, generator=g) ** 6
    w[0] = 0.0
    w[1] = 0.0
    w[1, n_in // 2] = 1.0
    existing = torch.cat([prev.spacing_starts[..., 0], prev.spacing_ends[..., -1:, 0]], dim=-1).numpy()
    want = H.sample_pdf(prev, w, n_out, None)
    ref = F.sample_pdf(w[..., 0].numpy(), existing, H.pdf_u(n_out + 1).numpy(), None, nears[:, 0].numpy(), fars[:, 0].numpy(), n_out, False, False)
    sp = torch.cat([want.spacing_starts[..., 0], want.spacing_ends[..., -1:, 0]], dim=-1).numpy()
    assert np.abs(ref.spacing - sp).max() <= 5e-6
    eucl = F.spacing_to_eucl_fp32(sp, F.spacing_fn_fp32(nears[:, 0].numpy(), False), F.spacing_fn_fp32(fars[:, 0].numpy(), False), False)
    x = torch.cat([want.starts[..., 0], want.ends[..., -1:, 0]], dim=-1).numpy().astype(f64)
    assert np.all(np.abs(eucl - x) <= 5e-7 * np.maximum(x, 1.0) ** 2)
    u = torch.rand(R, 1, generator=g)
    want = H.sample_pdf(prev, w, n_out, u)
    lin = torch.linspace(0.0, 1.0 - (1.0 / (n_out + 1)), steps=n_out + 1).numpy()
    ref = F.sample_pdf(w[..., 0].numpy(), existing, lin, u[:, 0].numpy(), nears[:, 0].numpy(), fars[:, 0].numpy(), n_out, False, False)
    sp = torch.cat([want.spacing_starts[..., 0], want.spacing_ends[..., -1:, 0]], dim=-1).numpy()
    assert np.abs(ref.spacing - sp).max() <= 5e-6


@pytest.mark.parametrize("n", [48, 64, 192, 256, 5])
def test_weights_are_the_oracle(n):
    g = torch.Generator().manual_seed(n)
    R = 33
    deltas = torch.rand(R, n, 1, generator=g) * 0.1
    dens = torch.exp(torch.randn(R, n, 1, generator=g) * 3)
    dens[0] = 0.0
    dens[1] = float("inf")
    want = H.get_weights(deltas, dens)[..., 0].numpy()
    ref = F.weights(deltas[..., 0].numpy(), dens[..., 0].numpy())
    assert np.all(np.abs(ref.weights - want) <= 2e-6 + 1e-5 * np.abs(want))
    assert np.all(ref.weights[0] == 0) and ref.weights[1, 0] == 1.0 and np.all(ref.weights[1, 1:] == 0)


@pytest.mark.parametrize("n", [48, 64, 192, 3])
def test_renderers_are_the_oracle(n):
    g = torch.Generator().manual_seed(77 + n)
    R = 41
    rgb = torch.rand(R, n, 3, generator=g)
    rgb[2, 1, 0] = float("nan")
    w = torch.rand(R, n, 1, generator=g)
    w = w / w.sum(1, keepdim=True) * torch.rand(R, 1, 1, generator=g) * 1.2
    w[0] = 0.0
    edges = torch.sort(torch.rand(R, n + 1, generator=g) * 5, dim=-1).values
    starts, ends = edges[:, :-1, None], edges[:, 1:, None]
    for training in (False, True):
        want = H.render_rgb(rgb, w, training).numpy()
        ref = F.composite(rgb.numpy(), w[..., 0].numpy(), training)
        np.testing.assert_array_equal(np.isnan(ref.out), np.isnan(want))
        m = ~np.isnan(want)
        assert np.abs(ref.out[m] - want[m]).max() <= 2e-6
    ref = F.depth(w[..., 0].numpy(), starts[..., 0].numpy(), ends[..., 0].numpy())
    assert np.abs(ref.accumulation - H.render_accumulation(w)[:, 0].numpy()).max() <= 2e-6
    want = H.render_depth_expected(w, starts, ends)[:, 0].numpy()
    assert np.all(np.abs(ref.expected - want) <= 1e-6 + 1e-5 * np.abs(want))
    want = H.render_depth_median(w, starts, ends)[:, 0].numpy()
    ties = H.median_depth_ties(w, starts, ends)
    clear = (torch.minimum(ties["margin_above"], ties["margin_below"])[:, 0] > 1e-6).numpy()
    assert clear.sum() >= R - 2
    np.testing.assert_array_equal(ref.median[clear], want[clear])


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("jitter", F.JITTERS)
def test_sample_initial_model_is_the_oracle(jitter, uniform):
    R, n = 7, 96
    lin_bins, t, nears, fars = F.sample_initial_case(R, n, 3, jitter)
    tt = None if t is None else torch.from_numpy(t).reshape(R, -1)
    want = H.sample_initial(torch.from_numpy(nears)[:, None], torch.from_numpy(fars)[:, None], n, tt, uniform)
    spacing, eucl = F.sample_initial_fp32(lin_bins, t, nears, fars, uniform, jitter == "edge")
    sp = torch.cat([want.spacing_starts[..., 0], want.spacing_ends[..., -1:, 0]], dim=-1).expand(R, n + 1).numpy()
    x = torch.cat([want.starts[..., 0], want.ends[..., -1:, 0]], dim=-1).numpy()
    assert np.abs(spacing - sp).max() <= 2e-7
    assert np.all(np.abs(eucl - x) <= 5e-7 * np.maximum(np.abs(x), 1.0) ** 2)
    o, d, edges = F.frustum_case(R, n, 4)
    pos, s, e, dl = F.frustum_from_edges_fp32(o, d, edges)
    want = o[:, None, :].astype(f64) + d[:, None, :].astype(f64) * ((s.astype(f64) + e) / 2)[..., None]
    assert np.abs(pos - want).max() <= 4 * F.EPS32 * 10 and np.array_equal(dl, e - s)
    np.testing.assert_array_equal(F.frustum_positions_fp32(o, d, s, e), pos)


# ----------------------------------------------------------------------------------------------------------------------
# sample_pdf: the exact family, the bound, the faults
# ----------------------------------------------------------------------------------------------------------------------
def _is_grid(x, g):
    x = np.asarray(x, f64)
    return bool(np.all(x * g == np.round(x * g)))


@pytest.mark.parametrize("jitter", F.JITTERS)
@pytest.mark.parametrize("n_in,n_out", F.PDF_SHAPES)
def test_pdf_exact_family_is_exact_in_every_order(n_in, n_out, jitter):
    for R in (5, 37):
        c = F.pdf_exact_case(R, n_in, n_out, 7 * n_in + n_out + R, jitter)
        w, ex = c["weights"], c["existing_bins"]
        assert np.all(w[:, 0] != 0) and _is_grid(ex, F.GRID) and np.all(np.diff(ex, axis=1) > 0) and ex.min() == 0 and ex.max() == 1
        nz = np.abs(w[w != 0]).astype(f64) / 2.0 ** 40
        assert np.all(np.log2(nz) == np.round(np.log2(nz))) and np.all((w.astype(f64).sum(1) / 2.0 ** 40) == 1.0)
        assert np.array_equal((w + f32(0.01)).astype(f32)[w != 0], w[w != 0])
        ref = F.sample_pdf(**c, cdf_fp32=True)
        assert _is_grid(ref.cdf, 1024) and _is_grid(ref.uu, F.GRID) and ref.cdf[:, -1].min() == 1.0
        want = ref.spacing.astype(f32)
        assert np.array_equal(want.astype(f64), ref.spacing)
        for order in F.ORDERS:
            got, eucl = F.sample_pdf_fp32(**c, order=order)
            F.same_bits(f"exact pdf {order}", got, want)
            F.same_bits(f"t clamp is not observable {order}", F.sample_pdf_fp32(**c, order=order, fault="t_unclamped")[0], want)


def _pdf_events(c):
    """which of the promised draws a case holds: ties at the start of a flat run, draws of 0, of 1, above 1, a flat run over the
    chunk boundary"""
    ref = F.sample_pdf(**c, cdf_fp32=True)
    cdf, uu = ref.cdf, ref.uu
    R, n1 = cdf.shape
    ev = dict(flat_tie=0, zero=int((uu == 0).sum()), one=int((uu == 1).sum()), above=int((uu > 1).sum()), straddle=0, overshoot=0)
    for r in range(R):
        flat = np.diff(cdf[r]) == 0
        if n1 > 66 and flat[63] and flat[64]:  # entries 63 = 64 = 65: the run crosses from chunk 0 (weights 0 .. 63) into chunk 1
            ev["straddle"] += 1
        ev["overshoot"] += int((c["weights"][r] < 0).any())
        for k in range(1, n1 - 1):
            if flat[k] and not flat[k - 1] and cdf[r, k] < 1:
                ev["flat_tie"] += int((uu[r] == cdf[r, k]).sum())
    return ev


def test_pdf_exact_family_holds_the_ties_it_promises():
    total = {}
    for jitter in F.JITTERS:
        ev = _pdf_events(F.pdf_exact_case(5, 129, 64, 3, jitter))
        assert ev["flat_tie"] > 0 and ev["one"] > 0 and ev["above"] > 0 and ev["straddle"] > 0 and ev["overshoot"] > 0, (jitter, ev)
        total = {k: total.get(k, 0) + v for k, v in ev.items()}
    assert total["zero"] > 0
    ev = _pdf_events(F.pdf_exact_case(37, 1024, 127, 3, "edge"))
    assert ev["flat_tie"] >= 37 and ev["zero"] >= 9 and ev["straddle"] >= 9


@pytest.mark.parametrize("jitter", F.JITTERS)
@pytest.mark.parametrize("n_in,n_out", F.PDF_SHAPES)
def test_pdf_bound_holds_the_model(n_in, n_out, jitter):
    c = F.pdf_general_case(5, n_in, n_out, n_in + n_out, jitter, lin=(n_in % 2 == 0))
    ref = F.sample_pdf(**c)
    assert np.all(np.isfinite(ref.tol)) and np.all(np.diff(ref.cdf, axis=1) > 0)
    for order in orders_for(n_in):
        got, eucl = F.sample_pdf_fp32(**c, order=order)
        assert ratio(got, ref.spacing, ref.tol) <= 1.0, order
        F.same_bits("eucl", eucl, F.spacing_to_eucl_fp32(got, F.spacing_fn_fp32(c["nears"], c["lin"]), F.spacing_fn_fp32(c["fars"], c["lin"]), c["lin"]))


def test_pdf_faults_fail_the_checks_of_the_gpu_test():
    n_in, n_out, R = 129, 64, 5
    for jitter in F.JITTERS:
        exact, general = F.pdf_exact_case(R, n_in, n_out, 3, jitter), F.pdf_general_case(R, n_in, n_out, 3, jitter)
        want = F.sample_pdf(**exact, cdf_fp32=True).spacing.astype(f32)
        ref = F.sample_pdf(**general)
        faults = ["side_left", "carry_dropped", "no_cdf_clamp"] + (["jitter_div_n_out"] if jitter else []) + (["jitter_row_stride"] if jitter == "edge" else [])
        for fault in faults:
            bad = F.sample_pdf_fp32(**exact, fault=fault)[0]
            assert F.fails(F.same_bits, fault, bad, want), (fault, jitter)
            if fault not in ("side_left", "no_cdf_clamp"):  # these two show on ties and on the overshoot ray alone
                bad = F.sample_pdf_fp32(**general, fault=fault)[0]
                assert F.fails(F.within, fault, bad, ref.spacing, ref.tol), (fault, jitter)
    # the carry between two chunks of 64 at n_in = 65: one bin's mass
    general = F.pdf_general_case(5, 65, 63, 1)
    ref = F.sample_pdf(**general)
    assert F.fails(F.within, "carry", F.sample_pdf_fp32(**general, fault="carry_dropped")[0], ref.spacing, ref.tol)


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.N_EDGES)
def test_weights_bound_holds_the_model_and_not_the_faults(n):
    dl, dn = F.weights_general_case(37, n, 1000 * n + 37)
    ref = F.weights(dl, dn)
    for order in orders_for(n):
        got = F.weights_fp32(dl, dn, order)
        assert np.all(np.abs(got - ref.weights) <= ref.tol), order
    if n > 1:
        assert F.fails(F.within, "inclusive", F.weights_fp32(dl, dn, fault="inclusive"), ref.weights, ref.tol)
    if n > 64:
        assert F.fails(F.within, "carry", F.weights_fp32(dl, dn, fault="carry_dropped"), ref.weights, ref.tol)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_weights_special_values_are_pinned(n):
    dl, dn, kinds = F.weights_special_case(n, n)
    ref = F.weights(dl, dn)
    for r, (kind, k) in enumerate(kinds):
        w, tol = ref.weights[r], ref.tol[r]
        if kind == "zero":
            assert np.all(w == 0) and np.all(tol == 0)
        elif kind == "inf":
            E = (dl[r, :k].astype(f32) * dn[r, :k]).astype(f32).astype(f64).sum()
            assert abs(w[k] - np.exp(-E)) <= 1e-15 and np.all(w[k + 1:] == 0) and np.all(tol[k + 1:] == 0)
        elif kind == "nan":
            assert np.all(w[k:] == 0) and np.all(tol[k:] == 0) and (k == 0 or w[:k].max() > 0)
        else:
            assert w[k] > 0 and np.all(np.delete(w, k) == 0) and np.all(np.delete(tol, k) == 0)
    for order in F.ORDERS:
        got = F.weights_fp32(dl, dn, order)
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref.weights) <= ref.tol), order
    assert F.fails(F.within, "nan", F.weights_fp32(dl, dn, fault="no_nan_to_num"), ref.weights, ref.tol)


# ----------------------------------------------------------------------------------------------------------------------
# composite
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("n", F.N_EDGES)
def test_composite_exact_family_bound_and_faults(n, C):
    R = 37
    v, w = F.composite_exact_case(R, n, C, 10 * n + C)
    assert _is_grid(w, 1024) and _is_grid(v, 256) and w.sum(1).max() > 1 and (w.sum(1) == 0).any() and w.sum(1).max() < 1.01
    for training in (True, False):
        ref = F.composite(v, w, training)
        assert np.array_equal(ref.out, ref.out.astype(f32).astype(f64))
        for order in F.ORDERS:
            F.same_bits(f"composite exact {order}", F.composite_fp32(v, w, training, order), ref.out.astype(f32))
        np.testing.assert_array_equal(ref.out[0], v[0, -1])  # no weight: the last sample
        assert F.fails(F.same_bits, "bg", F.composite_fp32(v, w, training, fault="no_background"), ref.out.astype(f32))
    if n > 1:  # a single sample is its own background: w v + v (1 - w) = v
        assert F.composite(v, w, True).out.min() < 0 and F.composite(v, w, False).out.min() == 0
        assert F.fails(F.same_bits, "clamp", F.composite_fp32(v, w, False, fault="no_eval_clamp"), F.composite(v, w, False).out.astype(f32))
    v, w = F.composite_general_case(R, n, C, 10 * n + C)
    for training in (True, False):
        ref = F.composite(v, w, training)
        assert np.isnan(ref.out).sum() == (1 if training else 0)
        for order in orders_for(n):
            F.within(f"composite general {order}", F.composite_fp32(v, w, training, order), ref.out, ref.tol)
        assert F.fails(F.within, "bg", F.composite_fp32(v, w, training, fault="no_background"), ref.out, ref.tol)
    ref = F.composite(v, w, True)
    assert F.fails(F.within, "nan", F.composite_fp32(v, w, True, fault="nan_to_num_in_training"), ref.out, ref.tol)


# ----------------------------------------------------------------------------------------------------------------------
# depth
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.N_EDGES)
def test_depth_exact_family_holds_its_ties_and_the_faults_fail(n):
    w, s, e, kinds = F.depth_exact_case(n, n)
    assert _is_grid(w, 1024) and _is_grid(s, 128) and np.all(e > s)
    ref = F.depth(w, s, e)
    cum = np.cumsum(w.astype(f64), axis=1)
    ties = [k for kind, k in kinds if kind == "tie"]
    assert ties == F.depth_tie_indices(n) and (n < 66 or {0, 62, 63, 64, 65, n - 1} <= set(ties))
    assert n != 1024 or {k // 64 for k in ties} == set(range(16))
    for r, (kind, k) in enumerate(kinds):
        if kind == "tie":
            assert cum[r, k] == 0.5 and (k == 0 or cum[r, k - 1] < 0.5) and ref.index[r] == k
        elif kind in ("below", "zero"):
            assert cum[r, -1] < 0.5 and ref.index[r] == n - 1
        elif kind == "jump":
            assert not (cum[r] == 0.5).any() and cum[r, ref.index[r]] > 0.5
    acc, med, exp = F.depth_exact_fp32(w, s, e)
    zero, over = [r for r, k in enumerate(kinds) if k[0] == "zero"], [r for r, k in enumerate(kinds) if k[0] == "overshoot"]
    assert exp[zero[0]] == f32(ref.lo) and ref.lo > 0 and (not over or exp[over[0]] == f32(ref.hi))
    for order in F.ORDERS:
        got = F.depth_fp32(w, s, e, order)
        for name, a, b in zip(("accumulation", "median", "expected"), got, (acc, med, exp)):
            F.same_bits(f"depth exact {name} {order}", a, b)
    if n > 1:
        assert F.fails(F.same_bits, "gt", F.depth_fp32(w, s, e, fault="gt_for_ge")[1], med)
    assert F.fails(F.same_bits, "clamp", F.depth_fp32(w, s, e, fault="no_index_clamp")[1], med)
    if n > 65:  # at n = 65 the second chunk is the last sample alone, which is also what the clamp answers
        assert F.fails(F.same_bits, "restart", F.depth_fp32(w, s, e, fault="prefix_restart")[1], med)


@pytest.mark.parametrize("R", F.R_EDGES)
@pytest.mark.parametrize("n", F.N_EDGES)
def test_depth_general_seeds_have_no_near_tie_and_the_bound_holds_the_model(n, R):
    w, s, e, seed = F.depth_general_case(R, n, 100 * n + R)
    ref = F.depth(w, s, e)
    assert not ref.near_tie.any() and seed < 100 * n + R + 8
    for order in orders_for(n):
        acc, med, exp = F.depth_fp32(w, s, e, order)
        F.within("acc", acc, ref.accumulation, ref.tol_accumulation)
        F.within("expected", exp, ref.expected, ref.tol_expected)
        F.same_bits("median", med, ref.median)


def test_depth_second_trip_case_and_its_faults():
    w, s, e = F.depth_second_trip_case(1)
    R = w.shape[0]
    assert R == F.SECOND_TRIP_R > F.DEPTH_GRID_CAP * F.RAYS_PER_BLOCK
    mid = F.midpoints_fp32(s, e)
    lo_ray, hi_ray = int(mid.min(1).argmin()), int(mid.max(1).argmax())
    assert (lo_ray, hi_ray) == (2048, 2052) and (lo_ray // 4) % 512 != (hi_ray // 4) % 512
    assert mid[:2048].min() > mid.min() and mid[:2048].max() < mid.max()
    acc, med, exp = F.depth_exact_fp32(w, s, e)
    assert np.all(exp[5::16] == mid.min()) and np.all(exp[9::16] == mid.max())
    for order in F.ORDERS:
        for a, b in zip(F.depth_fp32(w, s, e, order), (acc, med, exp)):
            F.same_bits(f"second trip {order}", a, b)
    assert F.fails(F.same_bits, "block", F.depth_fp32(w, s, e, fault="block_bounds")[2], exp)
    skipped = F.depth_fp32(w, s, e, fault="first_trip_only")
    assert all(F.fails(F.same_bits, "trip", a, b) for a, b in zip(skipped, (acc, med, exp)))
