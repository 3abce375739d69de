"""tests/proposal_eval_reference.py against the oracle and against itself, no device: its stages equal oracle/hotpath.py's proposal
sampler in fp64 on inputs the oracle can take exactly; the fp32 models of both kernel families stay inside the counted bounds on every
shape of the GPU tests; every planted fault fails the very check (``proposal_eval_reference.judge``, or a pinned value) the GPU tests
apply; and no case of the GPU tests needs more than 2 % of its rays redrawn for a median near a tie (the shares are printed)."""
import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import proposal_eval_reference as P
from tests import ray_forward_reference as RF

f32, f64 = np.float32, np.float64
FAMILIES = (P.SERIAL, P.WAVE)


@pytest.fixture(scope="module")
def nets():
    return P.random_nets(11)


@pytest.fixture()
def fp64_default():
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(before)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, f64)))


# ----------------------------------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------------------------------
def test_the_stages_equal_the_oracle_in_fp64(fp64_default, nets):
    """Level by level on inputs the oracle's fp64 takes exactly: dyadic sample positions inside an AABB (p s is exact: the frozen cell
    is the oracle's), the optical depths handed over as delta = 1, density = fl32(delta density), the padded weights as
    fl32(w + 0.01f) - 0.01, a power-of-two number of draws (u_j = (j + 1/2) / nb is the same number in fp32 and fp64)."""
    r = np.random.default_rng(3)
    R, n, n_out = 9, 21, 31
    # density
    net = nets[1]
    pos = (r.integers(0, 65, (R * n, 3)) / 64.0).astype(f32)
    sel = np.all((pos > 0) & (pos < 1), axis=1)
    assert 0 < sel.sum() < len(sel)
    dens, _ = P.F.proposal_density(net.grid, net.w0, net.b0, net.w1, net.b1, net.avg, (pos * sel[:, None]).astype(f32), sel)
    pre = "proposal_networks.1"
    sd = {f"{pre}.mlp_base.encoder.hash_table": _t(net.grid.table), f"{pre}.mlp_base.encoder.scalings": _t(net.grid.scalings),
          f"{pre}.aabb": _t([[0, 0, 0], [1, 1, 1]]), f"{pre}.mlp_base.mlp.layers.0.weight": _t(net.w0), f"{pre}.mlp_base.mlp.layers.0.bias": _t(net.b0),
          f"{pre}.mlp_base.mlp.layers.1.weight": _t(net.w1), f"{pre}.mlp_base.mlp.layers.1.bias": _t(net.b1)}
    args = {"hidden_dim": 16, "log2_hashmap_size": P.LOG2T, "num_levels": 5, "max_res": 256, "base_res": 16}
    cfg = H.OracleConfig(disable_scene_contraction=True, proposal_net_args_list=[args, args])
    want = H.proposal_density(sd, 1, _t(pos).view(R, n, 3), cfg)
    assert np.abs(want.numpy().reshape(-1) - dens).max() < 1e-12
    # weights and the median
    a32 = (r.random((R, n)) ** 4 * 2).astype(f32)
    a32[0], a32[1, 3] = 0, np.inf
    for family in FAMILIES:
        ref = P.level_weights(np.ones((R, n), f32), a32.astype(f64), np.zeros((R, n)), family)
        w = H.get_weights(torch.ones(R, n, 1), _t(a32)[..., None])[..., 0].numpy()
        assert np.abs(ref.weights - w).max() < 1e-12
        assert np.all(ref.weights[0] == 0) and ref.pinned[0].all() and np.all(ref.weights[1, 4:] == 0) and ref.pinned[1, 4:].all()
    w32 = np.asarray(w, f32)
    edges = np.cumsum(r.integers(1, 5, (R, n + 1)), axis=1).astype(f32) / 128
    med = P.median(w32, edges, P.SERIAL)
    want = H.render_depth_median(_t(w32)[..., None], _t(edges[:, :-1])[..., None], _t(edges[:, 1:])[..., None])[:, 0].numpy()
    assert np.array_equal(med.value.astype(f64), want)   # dyadic edges: the fp32 mid-point is the fp64 one
    # resampling, eval draws, anneal 1
    nears, fars = np.full(R, 0.05, f32), np.full(R, 6.0, f32)
    sp = np.sort(r.random((R, n + 1)), axis=1).astype(f32)
    case = P.make_case(nets, P.F.Rays(np.zeros((R, 3), f32), np.zeros((R, 3), f32), nears, fars), (n, n_out, n_out), False)
    ref = P.resample(case, 0, w32, sp, P.SERIAL)
    prev = H.Samples(None, None, _t(sp[:, :-1])[..., None], _t(sp[:, 1:])[..., None], H.spacing_fn(_t(nears)[:, None]),
                     H.spacing_fn(_t(fars)[:, None]))
    trick = (w32 + f32(0.01)).astype(f32).astype(f64) - 0.01
    got = H.sample_pdf(prev, _t(trick)[..., None], n_out, None)
    got = torch.cat([got.spacing_starts[..., 0], got.spacing_ends[..., -1:, 0]], dim=-1).numpy()
    assert np.abs(ref.spacing - got).max() < 1e-12
    # level 0: eval edges are lin_bins0, and their Euclidean map is the oracle's to fp32 accuracy
    s0 = H.sample_initial(_t(nears)[:, None], _t(fars)[:, None], n, None)
    e = P.eucl_edges(case, np.broadcast_to(case.lin0, (R, n + 1)))
    x = torch.cat([s0.starts[..., 0], s0.ends[..., -1:, 0]], dim=-1).numpy()
    assert np.all(np.abs(e.value - x) <= 5e-7 * np.maximum(x, 1.0) ** 2)


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 models inside the bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lin", [False, True])
@pytest.mark.parametrize("shape", P.SHAPES)
def test_the_models_stay_inside_the_bounds(nets, family, lin, shape):
    R = 129 if shape[0] <= 7 else 65
    for split in ((False, True) if family == P.SERIAL else (False,)):
        run = lambda c: P.emulate(c, family, split=split)  # noqa: E731
        case, out, share = P.general_case(run, family, nets, R, shape, lin, 1000 * shape[2] + R)
        worst = P.judge(f"{family} {shape} lin={lin}", case, out, family)
        assert all(v <= 1.0 for v in worst.values()), worst
        print(family, shape, lin, "split" if split else "", {k: round(v, 4) for k, v in worst.items()}, "redrawn", share)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("jitter,anneal", [("ray", 1.0), ("edge", 1.0), ("ray", 0.75), ("edge", 0.5)])
def test_the_training_models_stay_inside_the_bounds(nets, family, jitter, anneal):
    run = lambda c: P.emulate(c, family)  # noqa: E731
    case, out, share = P.general_case(run, family, nets, 65, P.TRAIN_SHAPE, False, 31, jitter, anneal)
    assert case.jitter is not None and case.jper == (jitter == "edge")
    P.judge(f"{family} training {jitter} anneal {anneal}", case, out, family)


def test_pinned_families_of_the_models(nets):
    """average_init_density 0 and an overflowing bias through the models and the reference: the values the GPU tests pin"""
    for family in FAMILIES:
        zero = [n._replace(avg=0.0) for n in nets]
        case = P.make_case(zero, P.mixed_rays(65, 1), (70, 37, 48), False)
        out = P.emulate(case, family)
        assert np.all(out["weights0"] == 0) and np.all(out["weights1"] == 0)
        P.judge("zero density", case, out, family)
        over = [n._replace(b1=np.array([P.OVERFLOW_BIAS], f32)) for n in nets]
        case = P.make_case(over, P.mixed_rays(65, 1), (70, 37, 48), False)
        out = P.emulate(case, family)
        for L in range(2):
            w = out[f"weights{L}"]
            live = np.arange(65) != 1
            assert np.all(w[live, 0] == 1) and np.all(w[live, 1:] == 0) and np.all(w[1] == 0)
        P.judge("overflow", case, out, family)


# ----------------------------------------------------------------------------------------------------------------------
# the planted faults
# ----------------------------------------------------------------------------------------------------------------------
CHAIN_FAULTS = ("no_padding", "own_a_in_transmittance", "seam_restart", "walk_block_no_break", "median_plus_one", "idle_lane_store", "tail_other_edge")


@pytest.mark.parametrize("fault", CHAIN_FAULTS)
def test_a_planted_fault_of_the_chain_fails_the_judge(nets, fault):
    caught = []
    for family in FAMILIES:
        if family == P.WAVE and fault in ("walk_block_no_break", "idle_lane_store"):
            continue   # the ray-per-wave form has neither walk blocks nor idle rays
        case, out, _ = P.general_case(lambda c: P.emulate(c, family, split=True), family, nets, 65, (70, 37, 48), False, 77)
        if fault == "tail_other_edge":   # seen only by draws at or behind the last knot: the caller-chosen draws of the GPU tests
            case = case._replace(u1=P.pinned_u(case.P1), u2=P.pinned_u(case.S))
            out = P.emulate(case, family, split=True)
        P.judge(f"{family} sound", case, out, family)
        bad = P.emulate(case, family, fault, split=True)
        assert P.fails(P.judge, f"{family} {fault}", case, bad, family), (family, fault)
        caught.append(family)
    assert caught


def test_side_left_fails_on_a_flat_run():
    """the only place side = left differs: a draw equal to the CDF value at the start of a flat run (the exact family of
    tests/ray_forward_reference.py, whose weights 2^40 absorb the histogram padding)"""
    for family in FAMILIES:
        for n_in, n_out in [(70, 37), (129, 64)]:
            c = RF.pdf_exact_case(8, n_in, n_out, n_in)
            ref = RF.sample_pdf(**c, cdf_fp32=True, k=P.k_cdf_family(family, n_in), k_t=P.K_T)
            uu = RF.draws_fp32(c["u"], c["u_rand"], 8, n_out, c["per_sample"])
            RF.same_bits("exact", P.resample_model(c["weights"], c["existing_bins"], uu, family), ref.spacing.astype(f32))
            got = P.resample_model(c["weights"], c["existing_bins"], uu, family, "side_left")
            assert RF.fails(RF.same_bits, "side_left", got, ref.spacing.astype(f32))   # (inside a flat run no slope bounds a sample)


def test_the_tail_and_the_padding_faults_break_pinned_values(nets):
    for family in FAMILIES:
        # draws at and above 1 must return the last edge's bits
        r = np.random.default_rng(5)
        R, n_in, n_out = 65, 37, 48
        w = (r.random((R, n_in)) ** 4).astype(f32)
        ex = np.sort(r.random((R, n_in + 1)), axis=1).astype(f32)
        u = P.pinned_u(n_out)
        assert u[0] == 0 and (u >= 1).sum() == 2 and (np.diff(u) == 0).sum() == 1
        uu = np.broadcast_to(u, (R, n_out + 1))
        good = P.resample_model(w, ex, uu, family)
        RF.same_bits("u >= 1", good[:, u >= 1], np.repeat(ex[:, -1:], 2, axis=1))
        RF.same_bits("u = 0", good[:, 0], ex[:, 0])
        bad = P.resample_model(w, ex, uu, family, "tail_other_edge")
        assert RF.fails(RF.same_bits, "u >= 1", bad[:, u >= 1], np.repeat(ex[:, -1:], 2, axis=1))
        # a total below 1e-5 (weights of -0.01f: every padded weight is 0): only the eps padding keeps the PDF uniform
        w = np.full((R, n_in), -0.01, f32)
        uu = np.broadcast_to(RF.pdf_positions_fp32(n_out + 1, None), (R, n_out + 1))
        ref = RF.sample_pdf(w, ex, uu[0], None, None, None, n_out, False, False, k=P.k_cdf_family(family, n_in), k_t=P.K_T)
        RF.within("eps padding", P.resample_model(w, ex, uu, family), ref.spacing, ref.tol)
        assert RF.fails(RF.within, "rcp_of_total", P.resample_model(w, ex, uu, family, "rcp_of_total"), ref.spacing, ref.tol)


def test_every_fault_is_planted_somewhere():
    assert set(P.FAULTS) == set(CHAIN_FAULTS) | {"side_left", "rcp_of_total"}


# ----------------------------------------------------------------------------------------------------------------------
# the redraw shares of every case of the GPU tests, from the reference alone
# ----------------------------------------------------------------------------------------------------------------------
def test_no_case_needs_more_than_the_cap_redrawn(nets):
    worst = 0.0
    for family in FAMILIES:
        for shape in P.SHAPES:
            for lin in (False, True):
                for R in P.R_EDGES:
                    _, _, share = P.general_case(lambda c: P.emulate(c, family), family, nets, R, shape, lin, 1000 * shape[2] + R)
                    worst = max(worst, share)
                    if share:
                        print(f"{family} {shape} lin={lin} R={R}: {share:.4f} of the rays redrawn")
        # the training cases: the seeds, draws and anneal of tests/test_gpu_proposal_eval.py::test_training_level_by_level
        for jitter, anneal in [("ray", 1.0), ("edge", 1.0), ("ray", 0.75)]:
            for R in P.R_EDGES:
                _, _, share = P.general_case(lambda c: P.emulate(c, family), family, nets, R, P.TRAIN_SHAPE, False, 31 + R, jitter, anneal)
                worst = max(worst, share)
                print(f"{family} training {P.TRAIN_SHAPE} jitter={jitter} anneal={anneal} R={R}: {share:.4f} of the rays redrawn")
    print(f"the largest share of rays redrawn for a median near a tie: {worst:.4f} (cap {P.REDRAW_CAP})")
    assert worst <= P.REDRAW_CAP
