"""The per-ray FORWARD kernels of the sampler / renderer chain on the device, element by element against the fp64 references of
tests/ray_forward_reference.py: tn_sample_pdf, tn_weights_fwd, tn_composite_fwd, tn_depth_fwd, tn_sample_initial,
tn_frustum_positions, tn_frustum_from_edges, and the training step's own forward tn_ray_render_fwd / tn_ray_render_depth_fwd
against the modular calls it replaced.

Bit for bit: the exact families of the reference module (PDF with ties on flat runs of the CDF, compositor, depth with the
cumulative weight on 0.5), every median depth (an index), the euclidean bins against spacing_to_eucl_fp32 of the device's own
spacing bins, tn_sample_initial and both frustum kernels against their fp32 models, the fused forward against the modular calls.
Bounded per element by the counted constants of the reference module (none tuned against what the device gives; run with -s for
the worst ratio to the bound of every check; profiles/micro/ray_forward_bounds.txt keeps those of one run): the general families.
Inputs are built on the CPU by the builders of the reference module and copied over; every output is pre-filled with a sentinel and
allocated PAD rows longer than the call writes: those rows must still hold it.  No element is skipped or masked."""
import numpy as np
import pytest
import torch

from tests import ray_forward_reference as F
from tests import ray_losses_reference as Q
from tests.ray_forward_reference import same_bits, within
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
TN_ERR_NULL, TN_ERR_SHAPE, TN_ERR_UNSUPPORTED = -1, -2, -3
FILL = F.SENTINEL
PAD = 2  # rows behind the last ray


def dev(x, dtype=f32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(DEV).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def out(R, *shape):
    return torch.full((R + PAD, *shape), FILL, device=DEV)


def host(t, R):
    """the first R rows; the PAD rows behind them must be untouched"""
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert np.all(a[R:] == f32(FILL)), "wrote behind the last ray"
    return a[:R]


def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == FILL).all()) for t in ts)


# ----------------------------------------------------------------------------------------------------------------------
# tn_sample_pdf
# ----------------------------------------------------------------------------------------------------------------------
def run_sample_pdf(c, expect=0, n_in=None, n_out=None):
    w = c["weights"]
    R, nb = w.shape[0], c["n_out"] + 1
    t = [dev(c[k]) for k in ("weights", "existing_bins", "u", "u_rand", "nears", "fars")]
    spacing, eucl = out(R, nb), out(R, nb)
    flags = (1 if c["lin"] else 0) | (2 if c["per_sample"] else 0)
    code = _hip.load().tn_sample_pdf(*[ptr(x) for x in t], R, w.shape[1] if n_in is None else n_in, c["n_out"] if n_out is None else n_out,
                                     flags, ptr(spacing), ptr(eucl), _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(spacing, eucl), "a refused call wrote"
        return None
    return host(spacing, R), host(eucl, R)


def eucl_of(c, spacing):
    return F.spacing_to_eucl_fp32(spacing, F.spacing_fn_fp32(c["nears"], c["lin"]), F.spacing_fn_fp32(c["fars"], c["lin"]), c["lin"])


@pytest.mark.parametrize("jitter", F.JITTERS, ids=["nojitter", "ray", "edge"])
@pytest.mark.parametrize("n_in,n_out", F.PDF_SHAPES)
def test_sample_pdf_per_element(n_in, n_out, jitter):
    for R in F.R_EDGES:
        tag = f"n_in={n_in} n_out={n_out} R={R} jitter={jitter}"
        c = F.pdf_exact_case(R, n_in, n_out, 7 * n_in + n_out + R, jitter, lin=(R % 2 == 0))
        spacing, eucl = run_sample_pdf(c)
        same_bits(f"sample_pdf exact spacing {tag}", spacing, F.sample_pdf(**c, cdf_fp32=True).spacing.astype(f32))
        same_bits(f"sample_pdf exact eucl {tag}", eucl, eucl_of(c, spacing))
        c = F.pdf_general_case(R, n_in, n_out, n_in + n_out + R, jitter, lin=(R % 2 == 1))
        ref = F.sample_pdf(**c)
        spacing, eucl = run_sample_pdf(c)
        within(f"sample_pdf spacing {tag}", spacing, ref.spacing, ref.tol)
        same_bits(f"sample_pdf eucl {tag}", eucl, eucl_of(c, spacing))


def test_sample_pdf_refuses_n_in_1025_and_0_and_n_out_0():
    c = F.pdf_general_case(3, 5, 7, 1, "edge")
    run_sample_pdf(c, expect=TN_ERR_SHAPE, n_in=1025)
    run_sample_pdf(c, expect=TN_ERR_SHAPE, n_in=0)
    run_sample_pdf(c, expect=TN_ERR_SHAPE, n_out=0)


# ----------------------------------------------------------------------------------------------------------------------
# tn_weights_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_weights(deltas, dens, n=None, expect=0):
    R, nn = deltas.shape
    a, b = dev(deltas), dev(dens)
    w = out(R, nn)
    code = _hip.load().tn_weights_fwd(ptr(a), ptr(b), R, nn if n is None else n, ptr(w), _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(w), "a refused call wrote"
        return None
    return host(w, R)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_weights_fwd_per_element(n):
    for R in F.R_EDGES:
        dl, dn = F.weights_general_case(R, n, 1000 * n + R)
        ref = F.weights(dl, dn)
        within(f"weights_fwd n={n} R={R}", run_weights(dl, dn), ref.weights, ref.tol)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_weights_fwd_special_values_are_pinned(n):
    """all-zero density, sigma = inf behind delta > 0 (the weight is the transmittance, every later one 0), delta = 0 with
    sigma = inf (a NaN product: that weight and every later one 0), one non-zero sample (exact zeros everywhere else)"""
    dl, dn, kinds = F.weights_special_case(n, n)
    ref = F.weights(dl, dn)
    got = run_weights(dl, dn)
    within(f"weights_fwd special n={n}", got, ref.weights, ref.tol)
    assert np.all(got[ref.pinned] == 0) and ref.pinned.sum() > 0


# ----------------------------------------------------------------------------------------------------------------------
# tn_composite_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_composite(v, w, training, C=None, n=None, expect=0):
    R, nn, CC = v.shape
    vd, wd = dev(v), dev(w)
    o = out(R, CC)
    code = _hip.load().tn_composite_fwd(ptr(vd), ptr(wd), R, nn if n is None else n, CC if C is None else C, int(training), ptr(o),
                                        _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(o), "a refused call wrote"
        return None
    return host(o, R)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("n", F.N_EDGES)
def test_composite_fwd_per_element(n, C):
    for R in F.R_EDGES:
        for training in (True, False):
            tag = f"C={C} n={n} R={R} training={training}"
            v, w = F.composite_exact_case(R, n, C, 10 * n + C + R)
            same_bits(f"composite_fwd exact {tag}", run_composite(v, w, training), F.composite(v, w, training).out.astype(f32))
            v, w = F.composite_general_case(R, n, C, 10 * n + C + R)
            ref = F.composite(v, w, training)
            assert np.isnan(ref.out).sum() == (1 if training else 0)  # a NaN sample comes through in training alone
            within(f"composite_fwd {tag}", run_composite(v, w, training), ref.out, ref.tol)


# ----------------------------------------------------------------------------------------------------------------------
# tn_depth_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_depth(w, s, e, acc=True, med=True, exp=True, scratch=True, n=None, expect=0):
    """-> (accumulation, median, expected), each None where it was passed as NULL"""
    R, nn = w.shape
    wd, sd, ed = dev(w), dev(s), dev(e)
    a, m, x = out(R), out(R), out(R)
    sc = torch.zeros(2, device=DEV)
    code = _hip.load().tn_depth_fwd(ptr(wd), ptr(sd), ptr(ed), R, nn if n is None else n, ptr(a) if acc else None, ptr(m) if med else None,
                                    ptr(x) if exp else None, ptr(sc) if scratch else None, _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(a, m, x), "a refused call wrote"
        return None
    res = []
    for on, t in ((acc, a), (med, m), (exp, x)):
        if on:
            res.append(host(t, R))
        else:
            assert untouched(t), "an output passed as NULL was written"
            res.append(None)
    return res


@pytest.mark.parametrize("n", F.N_EDGES)
def test_depth_fwd_exact_cases_bit_for_bit(n):
    """the cumulative weight EXACTLY 0.5 at index 0, 62, 63, 64, 65, n - 1 and in every chunk of 1024, a total below 0.5, no
    weight at all (expected clipped up to the call's smallest mid-point), an expected depth above the call's largest"""
    w, s, e, kinds = F.depth_exact_case(n, n)
    want = F.depth_exact_fp32(w, s, e)
    for name, got, ref in zip(("accumulation", "median", "expected"), run_depth(w, s, e), want):
        same_bits(f"depth_fwd exact {name} n={n}", got, ref)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_depth_fwd_general_cases_per_element(n):
    for R in F.R_EDGES:
        w, s, e, _ = F.depth_general_case(R, n, 100 * n + R)
        ref = F.depth(w, s, e)
        assert not ref.near_tie.any()
        acc, med, exp = run_depth(w, s, e)
        within(f"depth_fwd accumulation n={n} R={R}", acc, ref.accumulation, ref.tol_accumulation)
        within(f"depth_fwd expected n={n} R={R}", exp, ref.expected, ref.tol_expected)
        same_bits(f"depth_fwd median n={n} R={R}", med, ref.median)


def test_depth_fwd_second_trip_of_the_ray_loop():
    """R = 2053 > 512 blocks x 4 rays: rays 2048 .. 2052 are walked by the first two blocks on their second trip, and they hold the
    call's smallest and largest mid-point (in different blocks): the clip bounds of EVERY ray depend on them"""
    w, s, e = F.depth_second_trip_case(1)
    want = F.depth_exact_fp32(w, s, e)
    for name, got, ref in zip(("accumulation", "median", "expected"), run_depth(w, s, e), want):
        same_bits(f"depth_fwd second trip {name}", got, ref)


@pytest.mark.parametrize("acc,med,exp", [(False, True, True), (True, False, True), (True, True, False), (False, False, True),
                                         (False, True, False), (True, False, False)])
def test_depth_fwd_every_null_output(acc, med, exp):
    w, s, e, _ = F.depth_exact_case(65, 3)
    want = F.depth_exact_fp32(w, s, e)
    got = run_depth(w, s, e, acc, med, exp, scratch=exp)
    for name, on, g, ref in zip(("accumulation", "median", "expected"), (acc, med, exp), got, want):
        if on:
            same_bits(f"depth_fwd {name} with NULLs {int(acc)}{int(med)}{int(exp)}", g, ref)


def test_depth_fwd_refuses_expected_without_scratch():
    w, s, e, _ = F.depth_exact_case(5, 3)
    run_depth(w, s, e, scratch=False, expect=TN_ERR_NULL)


# ----------------------------------------------------------------------------------------------------------------------
# tn_sample_initial, tn_frustum_positions, tn_frustum_from_edges: fp32 models, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def run_sample_initial(lin_bins, t, nears, fars, lin, per_sample, n=None, expect=0):
    R, nn = nears.shape[0], lin_bins.shape[0] - 1
    lb, td, nd, fd = dev(lin_bins), dev(t), dev(nears), dev(fars)
    spacing, eucl = out(R, nn + 1), out(R, nn + 1)
    code = _hip.load().tn_sample_initial(ptr(lb), ptr(td), ptr(nd), ptr(fd), R, nn if n is None else n, (1 if lin else 0) | (2 if per_sample else 0),
                                         ptr(spacing), ptr(eucl), _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(spacing, eucl), "a refused call wrote"
        return None
    return host(spacing, R), host(eucl, R)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_sample_initial_bit_for_bit(n):
    for R in F.R_EDGES:
        for jitter in F.JITTERS:
            for lin in (False, True):
                lin_bins, t, nears, fars = F.sample_initial_case(R, n, n + R, jitter)
                spacing, eucl = run_sample_initial(lin_bins, t, nears, fars, lin, jitter == "edge")
                want = F.sample_initial_fp32(lin_bins, t, nears, fars, lin, jitter == "edge")
                same_bits(f"sample_initial spacing n={n} R={R} {jitter} lin={lin}", spacing, want[0])
                same_bits(f"sample_initial eucl n={n} R={R} {jitter} lin={lin}", eucl, want[1])


def run_frustums(o, d, edges, n=None, expect=0):
    """-> tn_frustum_from_edges' (positions, starts, ends, deltas) and tn_frustum_positions' positions on those starts / ends"""
    R, nn = edges.shape[0], edges.shape[1] - 1
    od, dd, ed = dev(o), dev(d), dev(edges)
    pos, s, e, dl, pos2 = out(R, nn, 3), out(R, nn), out(R, nn), out(R, nn), out(R, nn, 3)
    lib = _hip.load()
    code = lib.tn_frustum_from_edges(ptr(od), ptr(dd), ptr(ed), R, nn if n is None else n, ptr(pos), ptr(s), ptr(e), ptr(dl), _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(pos, s, e, dl), "a refused call wrote"
        sd = dev(edges[:, :-1])
        assert lib.tn_frustum_positions(ptr(od), ptr(dd), ptr(sd), ptr(sd), R, n, ptr(pos2), _hip.current_stream()) == expect
        assert untouched(pos2), "a refused call wrote"
        return None
    sd, e2 = dev(edges[:, :-1]), dev(edges[:, 1:])
    _hip.check(lib.tn_frustum_positions(ptr(od), ptr(dd), ptr(sd), ptr(e2), R, nn, ptr(pos2), _hip.current_stream()), "tn_frustum_positions")
    return host(pos, R), host(s, R), host(e, R), host(dl, R), host(pos2, R)


@pytest.mark.parametrize("n", F.N_EDGES)
def test_frustum_kernels_bit_for_bit(n):
    for R in F.R_EDGES:
        o, d, edges = F.frustum_case(R, n, 3 * n + R)
        pos, s, e, dl, pos2 = run_frustums(o, d, edges)
        want = F.frustum_from_edges_fp32(o, d, edges)
        for name, got, ref in zip(("positions", "starts", "ends", "deltas"), (pos, s, e, dl), want):
            same_bits(f"frustum_from_edges {name} n={n} R={R}", got, ref)
        same_bits(f"frustum_positions n={n} R={R}", pos2, want[0])


def test_every_entry_refuses_n_0_and_the_compositor_two_channels():
    R = 3
    dl, dn = F.weights_general_case(R, 5, 1)
    run_weights(dl, dn, n=0, expect=TN_ERR_SHAPE)
    v, w = F.composite_exact_case(R, 5, 3, 1)
    run_composite(v, w, True, n=0, expect=TN_ERR_SHAPE)
    run_composite(v, w, True, C=2, expect=TN_ERR_UNSUPPORTED)
    run_composite(v, w, False, C=2, expect=TN_ERR_UNSUPPORTED)
    ws, s, e, _ = F.depth_exact_case(5, 1)
    run_depth(ws, s, e, n=0, expect=TN_ERR_SHAPE)
    lin_bins, t, nears, fars = F.sample_initial_case(R, 5, 1, "edge")
    run_sample_initial(lin_bins, t, nears, fars, False, True, n=0, expect=TN_ERR_SHAPE)
    run_frustums(*F.frustum_case(R, 5, 1), n=0, expect=TN_ERR_SHAPE)
    c = Q.render_case(R, 5, 1)
    run_ray_render(c, depth=False, n=0, expect=TN_ERR_SHAPE)
    run_ray_render(c, depth=True, n=0, expect=TN_ERR_SHAPE)


# ----------------------------------------------------------------------------------------------------------------------
# tn_ray_render_fwd / tn_ray_render_depth_fwd against the modular calls
# ----------------------------------------------------------------------------------------------------------------------
def run_ray_render(c: Q.RenderCase, depth, n=None, expect=0):
    """-> dict of weights, rgb, thermal, accumulation (+ median, expected with ``depth``)"""
    R, nn = c.deltas.shape
    t = [dev(x) for x in (c.deltas, c.densities, c.rgb, c.thermal)]
    o = dict(weights=out(R, nn), rgb=out(R, 3), thermal=out(R), accumulation=out(R))
    lib, n_arg = _hip.load(), nn if n is None else n
    if depth:
        sd, ed = dev(c.starts), dev(c.ends)
        o.update(median=out(R), expected=out(R))
        scratch = torch.zeros(2 * ((R + 3) // 4), device=DEV)
        code = lib.tn_ray_render_depth_fwd(*[ptr(x) for x in t], ptr(sd), ptr(ed), R, n_arg, ptr(o["weights"]), ptr(o["rgb"]), ptr(o["thermal"]),
                                           ptr(o["accumulation"]), ptr(o["median"]), ptr(o["expected"]), ptr(scratch), _hip.current_stream())
    else:
        code = lib.tn_ray_render_fwd(*[ptr(x) for x in t], R, n_arg, ptr(o["weights"]), ptr(o["rgb"]), ptr(o["thermal"]), ptr(o["accumulation"]),
                                     _hip.current_stream())
    assert code == expect, code
    if expect != 0:
        assert untouched(*o.values()), "a refused call wrote"
        return None
    return {k: host(v, R) for k, v in o.items()}


def modular(c: Q.RenderCase):
    """tn_weights_fwd, tn_composite_fwd(training) on rgb and on thermal, tn_depth_fwd on those weights"""
    R, n = c.deltas.shape
    w = run_weights(c.deltas, c.densities)
    acc, med, exp = run_depth(w, c.starts, c.ends)
    return dict(weights=w, rgb=run_composite(c.rgb, w, True), thermal=run_composite(c.thermal.reshape(R, n, 1), w, True)[:, 0],
                accumulation=acc, median=med, expected=exp)


@pytest.mark.parametrize("n,rays", [(n, F.R_EDGES) for n in F.N_EDGES] + [(3, [F.SECOND_TRIP_R])])
def test_ray_render_forward_is_the_modular_calls_bit_for_bit(n, rays):
    """the training step's own forward runs the same operations in the same order as the kernels it replaced (read from the code;
    carry + excl against excl + carry is the same add).  R = 2053: 514 blocks, so ray_depth_clip_kernel's loop over the
    per-block bounds makes more than one trip per thread."""
    for R in rays:
        c = Q.render_case(R, n, 31 * n + R)
        want = modular(c)
        ref = F.weights(c.deltas, c.densities)
        for depth in (False, True):
            got = run_ray_render(c, depth)
            for k, v in got.items():
                same_bits(f"ray_render{'_depth' if depth else ''}_fwd {k} n={n} R={R}", v, want[k])
            within(f"ray_render{'_depth' if depth else ''}_fwd weights n={n} R={R}", got["weights"], ref.weights, ref.tol)
