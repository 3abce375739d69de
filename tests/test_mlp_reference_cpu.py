"""tests/mlp_reference.py without a device: the fp64 references against fp64 torch autograd over the same layers, the exact families
against fp32 emulations in two summation orders (bit for bit), every bound against those emulations on general inputs, every bound
against planted faults (it must NOT hold), and the builder conditions (redraw share, exactness) of every case that
tests/test_gpu_mlp.py runs on the device."""
import numpy as np
import pytest
import torch

from tests import mlp_reference as M

f32, f64 = np.float32, np.float64
ACTS = {0: lambda t: t, 1: torch.relu, 2: torch.sigmoid}


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, f64).copy()).requires_grad_(grad)


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= tol * (1 + np.abs(b))), float(np.abs(a - b).max())


def inside(got, want, tol):
    return bool(np.all(np.abs(np.asarray(got, f64) - want) <= tol))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(np.asarray(want, f64).astype(f32))
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))


# ----------------------------------------------------------------------------------------------------------------------
# the references are the derivatives
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("IN,OUT,n,act", [(15, 64, 65, 1), (64, 3, 7, 2), (1, 1, 3, 0), (130, 130, 5, 2)])
def test_linear_reference_is_fp64_autograd(IN, OUT, n, act):
    c = M.linear_case(IN, OUT, n, act, 1)
    x, W, b = t64(c.x, True), t64(c.W, True), t64(c.b, True)
    y = ACTS[act](torch.nn.functional.linear(x, W, b))
    close(M.linear_forward(c.x, c.W, c.b, act).y, y.detach().numpy())
    y.backward(t64(c.dy))
    # the derivative through the exact output (the builder's y is that output rounded to fp32: the adjoint takes what it is given)
    a = M.linear_adjoint(c.x, y.detach().numpy(), c.dy, c.W, act, dx_held=c.dx_held, accumulate_dx=True, dW_held=c.dW_held,
                         db_held=c.db_held)
    close(a.dx, x.grad.numpy() + c.dx_held)
    close(a.dW, W.grad.numpy() + c.dW_held)
    close(a.db, b.grad.numpy() + c.db_held)
    a = M.linear_adjoint(c.x, y.detach().numpy(), c.dy, c.W, act, want_w=False, want_b=False)
    close(a.dx, x.grad.numpy())
    assert a.dW is None and a.db is None and a.tol_dW is None


@pytest.mark.parametrize("name", list(M.CHAINS))
@pytest.mark.parametrize("act_top", [0, 2])
def test_chain_reference_is_fp64_autograd(name, act_top):
    spec = [list(s) for s in M.CHAINS[name][0]]
    spec[-1][2] = act_top
    n = 9
    r = np.random.default_rng(3)
    h = t64(r.standard_normal((n, spec[0][0])), True)
    x0, Ws, bs, tape = h, [], [], []
    for IN, OUT, act in spec:
        W, b = t64(r.standard_normal((OUT, IN)) / IN ** 0.5, True), t64(r.standard_normal(OUT), True)
        tape.append(h)
        h = ACTS[act](torch.nn.functional.linear(h, W, b))
        Ws.append(W)
        bs.append(b)
    dy = r.standard_normal((n, spec[-1][1]))
    h.backward(t64(dy))
    layers = [M.ChainLayer(Ws[k].detach().numpy(), tape[k].detach().numpy(), spec[k - 1][2] if k else 0) for k in range(len(spec) - 1, -1, -1)]
    res = M.chain_adjoint(layers, h.detach().numpy(), act_top, dy)
    for j, a in enumerate(res):
        k = len(spec) - 1 - j
        close(a.dW, Ws[k].grad.numpy(), 1e-10)
        close(a.db, bs[k].grad.numpy(), 1e-10)
        assert (a.dx is not None) == (k == 0)
    close(res[-1].dx, x0.grad.numpy(), 1e-10)


@pytest.mark.parametrize("clamp_min", [-15.0, -np.inf])
def test_density_reference_is_fp64_autograd_with_the_trunc_exp_clamps(clamp_min):
    c = M.density_case(257, 5, avg=0.75)
    enc, w0, b0, w1, b1 = t64(c.enc, True), t64(c.w0, True), t64(c.b0, True), t64(c.w1, True), t64(c.b1, True)
    raw = torch.relu(enc @ w0.T + b0) @ w1.reshape(-1) + b1
    fwd = M.density_train_forward(c.enc, c.selector, c.w0, c.b0, c.w1, c.b1, c.avg)
    close(fwd.raw, raw.detach().numpy())
    close(fwd.density, c.avg * np.exp(raw.detach().numpy()) * c.selector)
    # trunc_exp's backward is g exp(clamp(raw)) of the GIVEN raw: seed d_raw with it and let autograd do the layers
    g_raw = c.d_density.astype(f64) * c.selector * c.avg * np.exp(np.clip(c.raw.astype(f64), clamp_min, 15.0))
    raw.backward(t64(g_raw))
    a = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, clamp_min, c.held)
    close(a.d_enc, enc.grad.numpy(), 1e-10)
    close(a.d_w0, w0.grad.numpy() + c.held["d_w0"], 1e-10)
    close(a.d_b0, b0.grad.numpy() + c.held["d_b0"], 1e-10)
    close(a.d_w1, w1.grad.numpy().reshape(-1) + c.held["d_w1"], 1e-10)
    close(a.d_b1, b1.grad.numpy()[0] + c.held["d_b1"][0], 1e-10)
    rows = (c.raw < -15) & (c.selector > 0)
    assert rows.any() and (c.raw > 15).any() and (c.selector == 0).any()
    if clamp_min == -15.0:  # the lower clamp is felt: the unclamped gradient of those rows is smaller
        un = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -np.inf)
        assert np.all(np.abs(un.d_enc[rows]).sum(1) < np.abs(a.d_enc[rows]).sum(1))


# ----------------------------------------------------------------------------------------------------------------------
# exact families: two orders of fp32 arithmetic give the reference's bits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("IN,OUT,n,act", [(1, 1, 65, 0), (15, 64, 129, 1), (64, 64, 257, 1), (130, 130, 65, 0), (200, 1, 65, 1)])
def test_exact_linear_family_is_exact(IN, OUT, n, act):
    c = M.exact_linear_case(IN, OUT, n, act, 7)
    fwd = M.linear_forward(c.x, c.W, c.b, act)
    ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, act, dx_held=c.dx_held, accumulate_dx=True, dW_held=c.dW_held, db_held=c.db_held)
    for order in (0, 1):
        assert same_bits(M.linear_forward_fp32(c.x, c.W, c.b, act, order), fwd.y)
        dx, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, act, order, None, c.dx_held, True, c.dW_held, c.db_held)
        assert same_bits(dx, ref.dx) and same_bits(dW, ref.dW) and same_bits(db, ref.db)
    for fault in ("drop_last_row", "drop_col"):  # and a fault is a bit difference
        dx, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, act, 0, fault, c.dx_held, True, c.dW_held, c.db_held)
        assert not (same_bits(dx, ref.dx) and same_bits(dW, ref.dW) and same_bits(db, ref.db)), fault


@pytest.mark.parametrize("name", list(M.CHAINS))
@pytest.mark.parametrize("act_top", [0, 2])
def test_exact_chain_family_is_exact(name, act_top):
    c = M.exact_chain_case(M.CHAINS[name][0], 129, 11, act_top)
    ref = M.chain_adjoint(c.layers, c.y_top, c.act_top, c.dy, dx_held=c.dx_held, accumulate_dx=True)
    for order in (0, 1):
        got, dx = M.chain_adjoint_fp32(c.layers, c.y_top, c.act_top, c.dy, order, dx_held=c.dx_held, accumulate_dx=True)
        assert same_bits(dx, ref[-1].dx)
        for (dW, db), a in zip(got, ref):
            assert same_bits(dW, a.dW) and same_bits(db, a.db)
    assert np.abs(ref[-1].dx - c.dx_held).max() > 0 and all(np.abs(a.dW).max() > 0 for a in ref), "a trivial case"


def test_exact_density_family_is_exact():
    c = M.exact_density_case(769, 13)
    ref = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, 1.0, -15.0, c.held)
    for order in (0, 1):
        got = M.density_train_adjoint_fp32(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, 1.0, -15.0, c.held, order)
        for k in ("d_enc", "d_w0", "d_b0", "d_w1", "d_b1"):
            assert same_bits(got[k].reshape(-1), np.asarray(getattr(ref, k)).reshape(-1)), k
    assert np.abs(ref.d_enc).max() > 0 and np.abs(ref.d_w0 - c.held["d_w0"]).max() > 0


# ----------------------------------------------------------------------------------------------------------------------
# the exact cases of the device tests at their second-round sizes: the builders' own assertions (every |sum| below 2^24) must pass,
# and losing the second round is a bit difference there although no counted bound of 50 000 terms would see 65 rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("IN,OUT", [(64, 64), (15, 64)])
def test_exact_linear_second_round_case_builds_and_sees_a_lost_round(IN, OUT):
    n = M.LINEAR_SECOND_ROUND
    c = M.exact_linear_case(IN, OUT, n, 1, 100 + IN)
    ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, 1, dW_held=c.dW_held, db_held=c.db_held)
    _, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, 1, 0, None, dW_held=c.dW_held, db_held=c.db_held)
    assert same_bits(dW, ref.dW) and same_bits(db, ref.db)
    _, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, 1, 0, "lose_second_round", dW_held=c.dW_held, db_held=c.db_held)
    assert not same_bits(dW, ref.dW) and not same_bits(db, ref.db)


@pytest.mark.parametrize("name", list(M.CHAINS))
@pytest.mark.parametrize("act_top", [0, 2])
def test_exact_chain_cases_of_the_device_tests_build(name, act_top):
    for n in M.CHAIN_N:
        M.exact_chain_case(M.CHAINS[name][0], n, 17 + n, act_top)


def test_exact_density_cases_of_the_device_tests_build():
    for n in M.DENSITY_N:
        M.exact_density_case(n, M.density_seed(n))


@pytest.mark.parametrize("n", M.DENSITY_N)
def test_redraw_share_of_every_density_case_of_the_device_tests(n):
    c = M.density_case(n, M.density_seed(n))
    print(f"density_case n={n}: redrawn {c.redrawn:.5%}")
    assert c.redrawn <= M.REDRAW_CAP
    ref = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -15.0, c.held)
    assert ref.margin.min() > M.GATE_MARGIN


# ----------------------------------------------------------------------------------------------------------------------
# bounds: hold for two orders of fp32 arithmetic, do not hold for the planted faults
# ----------------------------------------------------------------------------------------------------------------------
LIN_BOUND_CASES = [(1, 1, 65, 0), (15, 64, 65, 1), (63, 64, 129, 2), (64, 3, 63, 2), (130, 130, 65, 2), (200, 1, 65, 0), (64, 64, 257, 1)]


@pytest.mark.parametrize("IN,OUT,n,act", LIN_BOUND_CASES)
def test_linear_bounds_hold_for_fp32_arithmetic_in_two_orders(IN, OUT, n, act):
    c = M.linear_case(IN, OUT, n, act, 21)
    fwd = M.linear_forward(c.x, c.W, c.b, act)
    for acc in (False, True):
        ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, act, dx_held=c.dx_held, accumulate_dx=acc, dW_held=c.dW_held, db_held=c.db_held)
        for order in (0, 1):
            assert inside(M.linear_forward_fp32(c.x, c.W, c.b, act, order), fwd.y, fwd.tol)
            dx, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, act, order, None, c.dx_held, acc, c.dW_held, c.db_held)
            assert inside(dx, ref.dx, ref.tol_dx) and inside(dW, ref.dW, ref.tol_dW) and inside(db, ref.db, ref.tol_db)


@pytest.mark.parametrize("IN,OUT,n,act", [(15, 64, 65, 1), (63, 64, 129, 2), (130, 130, 65, 2), (64, 64, 257, 0)])
@pytest.mark.parametrize("fault", ["drop_last_row", "drop_col", "swap_in_block", "double_bias_partial"])
def test_linear_bounds_do_not_hold_for_planted_faults(IN, OUT, n, act, fault):
    c = M.linear_case(IN, OUT, n, act, 22)
    ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, act, dW_held=c.dW_held, db_held=c.db_held)
    dx, dW, db, _ = M.linear_adjoint_fp32(c.x, c.y, c.dy, c.W, act, 0, fault, dW_held=c.dW_held, db_held=c.db_held)
    ok = dict(dx=inside(dx, ref.dx, ref.tol_dx), dW=inside(dW, ref.dW, ref.tol_dW), db=inside(db, ref.db, ref.tol_db))
    must_fail = {"drop_last_row": ("dx", "dW", "db"), "drop_col": ("dx", "dW"), "swap_in_block": ("dx", "dW", "db"),
                 "double_bias_partial": ("db",)}[fault]
    assert not any(ok[k] for k in must_fail), (fault, ok)
    if fault == "drop_col":
        fwd = M.linear_forward(c.x, c.W, c.b, act)
        assert not inside(M.linear_forward_fp32(c.x, c.W, c.b, act, 0, fault), fwd.y, fwd.tol)


def test_a_lost_second_round_of_rows_is_outside_the_dx_bound():
    """dx is per row: the rows of the second round are simply missing.  (dW over 50 000 rows: see the exact case above.)"""
    n = M.LINEAR_SECOND_ROUND
    c = M.linear_case(15, 64, n, 1, 23)
    ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, 1, want_w=False, want_b=False)
    g = (c.dy * (c.y > 0)).astype(f32)
    dx = (g.astype(f64) @ c.W.astype(f64)).astype(f32)  # one rounding: inside
    assert inside(dx, ref.dx, ref.tol_dx)
    dx[M.LIN_BWD_BLOCKS * 64:] = 0
    assert not inside(dx, ref.dx, ref.tol_dx)


@pytest.mark.parametrize("name", list(M.CHAINS))
@pytest.mark.parametrize("act_top", [0, 2])
def test_chain_bounds_hold_and_see_faults_in_every_layer(name, act_top):
    c = M.chain_case(M.CHAINS[name][0], 65, 31, act_top)
    ref = M.chain_adjoint(c.layers, c.y_top, c.act_top, c.dy, dx_held=c.dx_held, accumulate_dx=True)

    def verdict(got, dx):
        v = [inside(dx, ref[-1].dx, ref[-1].tol_dx)]
        for (dW, db), a in zip(got, ref):
            v += [inside(dW, a.dW, a.tol_dW), inside(db, a.db, a.tol_db)]
        return v

    for order in (0, 1):
        assert all(verdict(*M.chain_adjoint_fp32(c.layers, c.y_top, c.act_top, c.dy, order, dx_held=c.dx_held, accumulate_dx=True)))
    for j in range(len(c.layers)):
        for fault in ("drop_last_row", "drop_col", "swap_in_block", "double_bias_partial"):
            v = verdict(*M.chain_adjoint_fp32(c.layers, c.y_top, c.act_top, c.dy, 0, fault, j, c.dx_held, True))
            if fault == "double_bias_partial":
                assert not v[2 + 2 * j], (j, fault)
            elif fault == "swap_in_block" and min(c.layers[j].W.shape) == 1 and max(c.layers[j].W.shape) == 1:
                continue
            else:
                assert not v[1 + 2 * j], (j, fault, v)  # that layer's dW


@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_density_bounds_hold_and_see_faults(n):
    c = M.density_case(n, 41)
    ref = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -15.0, c.held)
    names = ("d_enc", "d_w0", "d_b0", "d_w1", "d_b1")
    tols = dict(d_enc=ref.tol_enc, d_w0=ref.tol_w0, d_b0=ref.tol_b0, d_w1=ref.tol_w1, d_b1=ref.tol_b1)

    def verdict(got):
        return {k: inside(got[k].reshape(np.shape(getattr(ref, k))), getattr(ref, k), tols[k]) for k in names}

    for order in (0, 1):
        assert all(verdict(M.density_train_adjoint_fp32(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -15.0, c.held,
                                                        order)).values())
    fwd = M.density_train_forward(c.enc, c.selector, c.w0, c.b0, c.w1, c.b1, c.avg)
    hid = M.linear_forward_fp32(c.enc, c.w0, c.b0, 1, 0)
    raw32 = M.linear_forward_fp32(hid, c.w1, c.b1, 0, 0)[:, 0]
    assert inside(raw32, fwd.raw, fwd.tol_raw)
    dens32 = ((f32(c.avg) * np.exp(raw32.astype(f64)).astype(f32)).astype(f32) * c.selector).astype(f32)
    assert inside(dens32, fwd.density, fwd.tol_density)
    if n < 255:
        return
    for fault, must in (("drop_last_row", ("d_enc",)), ("drop_col", ("d_w0",)), ("swap_in_block", ("d_w0", "d_enc")),
                        ("double_bias_partial", ("d_b0", "d_b1"))):
        v = verdict(M.density_train_adjoint_fp32(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -15.0, c.held, 0, fault))
        assert not any(v[k] for k in must), (fault, v)
    # the clamp rows matter: an adjoint without the lower clamp is outside the bound of d_enc
    un = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, -np.inf)
    assert not inside(un.d_enc, ref.d_enc, ref.tol_enc)


# ----------------------------------------------------------------------------------------------------------------------
# mlp_head.0's ray-constant part
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
def test_ray_head_reference_is_fp64_autograd(shifted):
    c = M.ray_head_case(65, 51, bad_cams=True)
    x, ok = M.ray_inputs(c.directions, c.cams, c.emb, shifted)
    assert (~ok).any() and ok.any()
    W, b, emb = t64(c.W0, True), t64(c.b0, True), t64(c.emb, True)
    sh = t64(x[:, :16], True)
    cam = torch.from_numpy(np.where(ok, c.cams, 0).astype(np.int64))
    v = b + sh @ W[:, :16].T + emb[cam] @ W[:, 16 + M.GF:].T
    ref_v, tol, _ = M.ray_head_forward(c.W0, c.b0, c.emb, c.directions, c.cams, shifted)
    close(ref_v[ok], v.detach().numpy()[ok])
    assert np.all(np.isnan(ref_v[~ok]))
    (v * t64(np.where(ok[:, None], c.g, 0.0))).sum().backward()
    a = M.ray_head_adjoint(c.W0, c.emb, c.directions, c.cams, c.g, shifted, c.held_w, c.held_b, c.held_emb)
    close(a.d_w, W.grad.numpy() + c.held_w, 1e-10)
    assert np.array_equal(a.d_w[:, 16:16 + M.GF], c.held_w[:, 16:16 + M.GF].astype(f64)) and np.all(a.tol_w[:, 16:16 + M.GF] == 0)
    close(a.d_b, b.grad.numpy() + c.held_b, 1e-10)
    close(a.d_emb, emb.grad.numpy() + c.held_emb, 1e-10)
    close(a.d_x, sh.grad.numpy(), 1e-10)
    # the SH components are nerfstudio's: degree-4 real harmonics of the direction (spot values)
    s = M.sh16_fp32(np.array([[0.0, 0.0, 1.0]], f32), False)[0]
    assert abs(s[0] - 0.28209479) < 1e-7 and abs(s[2] - 0.48860251) < 1e-7 and abs(s[6] - (0.94617470 - 0.31539157)) < 1e-6


@pytest.mark.parametrize("R", [1, 65, 321])
def test_ray_head_bounds_hold_and_see_faults(R):
    c = M.ray_head_case(R, 52, bad_cams=R > 1)
    a = M.ray_head_adjoint(c.W0, c.emb, c.directions, c.cams, c.g, False, c.held_w, c.held_b, c.held_emb)
    tols = dict(d_w=a.tol_w, d_b=a.tol_b, d_emb=a.tol_emb, d_x=a.tol_x)

    def verdict(got):
        return {k: inside(got[k][a.ok] if k == "d_x" else got[k], getattr(a, k)[a.ok] if k == "d_x" else getattr(a, k),
                          tols[k][a.ok] if k == "d_x" else tols[k]) for k in tols}

    for order in (0, 1):
        assert all(verdict(M.ray_head_adjoint_fp32(c, False, order)).values())
    if R < 65:
        return
    for fault, must in (("drop_last_row", ("d_w", "d_b")), ("double_bias_partial", ("d_b",)), ("shift_columns", ("d_w",)),
                        ("swap_in_block", ("d_w", "d_x", "d_emb"))):
        v = verdict(M.ray_head_adjoint_fp32(c, False, 0, fault))
        assert not any(v[k] for k in must), (fault, v)


@pytest.mark.parametrize("R", [65, M.RAY_HEAD_BWD_BLOCKS * 64 + 65])
def test_exact_ray_head_family_is_exact_and_sees_a_lost_round(R):
    c = M.ray_head_case(R, 53, bad_cams=True, exact=True)
    a = M.ray_head_adjoint(c.W0, c.emb, c.directions, c.cams, c.g, False, c.held_w, c.held_b, c.held_emb)
    app = slice(16 + M.GF, M.IN0)
    for order in (0, 1):
        got = M.ray_head_adjoint_fp32(c, False, order)
        assert same_bits(got["d_w"][:, app], a.d_w[:, app]) and same_bits(got["d_b"], a.d_b) and same_bits(got["d_emb"], a.d_emb)
        assert same_bits(got["d_x"][a.ok], a.d_x[a.ok])
    if R > M.RAY_HEAD_BWD_BLOCKS * 64:
        bad = M.ray_head_adjoint_fp32(c, False, 0, "lose_second_round")
        assert not same_bits(bad["d_w"][:, app], a.d_w[:, app]) and not same_bits(bad["d_b"], a.d_b) and not same_bits(bad["d_emb"], a.d_emb)


def test_a_lost_second_round_of_the_proposal_backward_is_a_bit_difference_in_the_exact_case():
    n = M.DENSITY_N[-1]
    c = M.exact_density_case(n, M.density_seed(n))
    ref = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, 1.0, -15.0, c.held)
    got = M.density_train_adjoint_fp32(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, 1.0, -15.0, c.held, 0)
    assert same_bits(got["d_w0"], ref.d_w0) and same_bits(got["d_b1"].reshape(-1), ref.d_b1.reshape(-1))
    bad = M.density_train_adjoint_fp32(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, 1.0, -15.0, c.held, 0, "lose_second_round")
    assert not same_bits(bad["d_w0"], ref.d_w0) and not same_bits(bad["d_enc"], ref.d_enc)


# ----------------------------------------------------------------------------------------------------------------------
# the fused field backward
# ----------------------------------------------------------------------------------------------------------------------
class _TruncExp(torch.autograd.Function):
    """exp forward; backward g exp(clamp(x, lo, 15)) (nerfstudio's trunc_exp)"""

    @staticmethod
    def forward(ctx, x, lo):
        ctx.save_for_backward(x)
        ctx.lo = lo
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, ctx.lo, 15.0)), None


def _field_autograd(c, pass_thermal, clamp_min, want_rgb, want_thermal):
    """fp64 autograd over the field's layers from the given enc -> (stored rgb of that forward, gradients by name, d_enc, d ray_bias)"""
    W = {k: t64(v, True) for k, v in c.w.items()}
    enc, rb = t64(c.enc, True), t64(c.ray_bias, True)
    N = c.enc.shape[0]
    ray = torch.arange(N) // c.S
    h1 = torch.relu(enc @ W["base0_w"].T + W["base0_b"])
    bo = h1 @ W["base1_w"].T + W["base1_b"]
    geo = bo[:, 1:]
    dens = c.avg * _TruncExp.apply(bo[:, 0], clamp_min) * t64(c.selector)
    c1 = torch.relu(rb[ray] + geo @ W["head0_w"][:, 16:16 + M.GF].T)
    c2 = torch.relu(c1 @ W["head1_w"].T + W["head1_b"])
    rgb = torch.sigmoid(c2 @ W["head2_w"].T + W["head2_b"])
    gt = geo if pass_thermal else geo.detach()
    t1 = torch.relu(gt @ W["th0_w"].T + W["th0_b"])
    t2 = torch.sigmoid(t1 @ W["th1_w"].T + W["th1_b"])
    th = t2 @ W["thead_w"].reshape(-1) + W["thead_b"]
    loss = (dens * t64(c.d_density)).sum()
    if want_rgb:
        loss = loss + (rgb * t64(c.d_rgb)).sum()
    if want_thermal:
        loss = loss + (th * t64(c.d_thermal)).sum()
    loss.backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return rgb.detach().numpy(), {k: z(v) for k, v in W.items()}, z(enc), z(rb)


@pytest.mark.parametrize("pass_thermal,clamp_min,want_rgb,want_thermal", [(1, -15.0, True, True), (0, -15.0, True, True),
                                                                          (1, -np.inf, False, True), (1, -15.0, True, False)])
def test_field_reference_is_fp64_autograd(pass_thermal, clamp_min, want_rgb, want_thermal):
    c = M.field_case(7, 23, 723, avg=0.75)
    rgb, g, d_enc, d_rb = _field_autograd(c, pass_thermal, clamp_min, want_rgb, want_thermal)
    c = c._replace(rgb=rgb)   # the derivative is taken through the STORED output: hand the reference that forward's
    for split, stored in ((0, False), (1, False), (2, False)):   # (without stored rows the forms differ in their bounds only)
        a = M.field_adjoint(c, split, stored, pass_thermal, clamp_min, want_rgb, want_thermal)
        close(a.d_enc, d_enc, 1e-9)
        close(a.d_ray_sum, d_rb + c.held_ray_sum, 1e-9)
        for k in M.FIELD_PARAMS:
            want = g[k].reshape(M.FIELD_SHAPES[k]) + c.held[k].reshape(M.FIELD_SHAPES[k])
            if k == "head0_w":   # the geo columns only
                want = c.held[k].astype(f64).copy()
                want[:, 16:16 + M.GF] += g[k][:, 16:16 + M.GF]
            close(a.grads[k], want, 1e-9)
    raw = c.base_out[:, 0]
    assert (raw < -15).any() and (raw > 15).any() and (c.selector == 0).any()
    # the stored rows are the recomputed ones rounded to fp32: the reference over them is the same derivative to that rounding
    a1, a2 = M.field_adjoint(c, 1, True, pass_thermal, clamp_min, want_rgb, want_thermal), M.field_adjoint(c, 1, False, pass_thermal, clamp_min, want_rgb, want_thermal)
    assert np.abs(a1.d_enc - a2.d_enc).max() <= 1e-4 * np.abs(a2.d_enc).max()


def _field_verdict(c, got, a):
    d_enc, ray_sum, grads = got
    v = dict(d_enc=inside(d_enc, a.d_enc, a.tol_enc), d_ray_sum=inside(ray_sum, a.d_ray_sum, a.tol_ray_sum))
    for k in M.FIELD_PARAMS:
        v[k] = inside(grads[k], a.grads[k], a.tols[k])
    return v


@pytest.mark.parametrize("split,stored", [(1, False), (1, True), (2, False), (2, True)])
def test_field_bounds_hold_for_fp32_arithmetic_in_two_orders_and_see_faults(split, stored):
    c = M.field_case(7, 23, 723)
    a = M.field_adjoint(c, split, stored)
    for order in (0, 1):
        v = _field_verdict(c, M.field_adjoint_fp32(c, split, stored, order), a)
        assert all(v.values()), (order, [k for k, ok in v.items() if not ok])
    for fault, must in (("shift_geo", ("head0_w",)), ("drop_last_row", ("d_enc", "base0_w", "head1_w", "thead_b")),
                        ("double_bias_partial", ("head1_b", "base0_b")), ("swap_in_block", ("d_enc", "head1_w", "th1_w", "base0_w", "head0_w"))):
        v = _field_verdict(c, M.field_adjoint_fp32(c, split, stored, 0, fault), a)
        assert not any(v[k] for k in must), (fault, {k: v[k] for k in must})
    if split == 2 and stored:
        # a piece product of the heads' second layer left out.  The leading product (5) and the two first-order cross terms (3, 4:
        # 2^-8 relative) are outside the bounds.  The three second-order products (0, 1, 2: 2^-16 relative) are NOT: the counted
        # bound of the pieces form assumes a chain of 6 nnz roundings (see _product) and is some 20 times the error of this
        # emulation; nothing in this module sees such a term dropped (the exact family's integers are single pieces).
        seen = {}
        for j in range(6):
            v = _field_verdict(c, M.field_adjoint_fp32(c, split, stored, 0, f"omit_piece_{j}"), a)
            seen[j] = [k for k, ok in v.items() if not ok]
            print(f"piece product {M.PIECE_ORDER[j]} omitted: outside the bound of", seen[j])
        assert all(seen[j] for j in (3, 4, 5)), seen
        assert "d_enc" in seen[3] and "head1_w" in seen[3] and "th1_w" in seen[3]


def test_bf16_pieces_are_an_exact_split_and_small_integers_are_one_piece():
    x = np.random.default_rng(1).standard_normal(4096).astype(f32)
    p1, p2, p3 = M.bf16_pieces(x)
    assert np.all(p1.astype(f64) + p2.astype(f64) + p3.astype(f64) == x.astype(f64))
    assert np.all(np.abs(p2) <= 2.0 ** -8 * np.abs(x)) and np.all(np.abs(p3) <= 2.0 ** -16 * np.abs(x))
    k = np.arange(-256, 257).astype(f32)
    p1, p2, p3 = M.bf16_pieces(k)
    assert np.all(p1 == k) and not p2.any() and not p3.any()
    dropped = np.abs(p2[:, None] * p3[None, :]).max()  # (trivially zero here; the general statement is PIECE_DROPPED)
    assert dropped == 0 and M.PIECE_DROPPED == 2 + 2.0 ** -8


@pytest.mark.parametrize("split,stored", [(1, False), (2, True)])
def test_exact_field_family_is_exact(split, stored):
    c = M.exact_field_case(7, 23, 723)
    a = M.field_adjoint(c, split, stored, want_thermal=False)
    for order in (0, 1):
        d_enc, ray_sum, grads = M.field_adjoint_fp32(c, split, stored, order, want_thermal=False)
        assert same_bits(d_enc, a.d_enc) and same_bits(ray_sum, a.d_ray_sum)
        for k in M.FIELD_PARAMS:
            assert same_bits(grads[k], a.grads[k]), k
    assert np.abs(a.d_enc).max() > 0 and np.abs(a.d_ray_sum - c.held_ray_sum).max() > 0 and np.abs(a.grads["head0_w"] - c.held["head0_w"]).max() > 0
    d_enc, ray_sum, grads = M.field_adjoint_fp32(c, split, stored, 0, "drop_last_row", want_thermal=False)
    assert not same_bits(grads["base1_b"], a.grads["base1_b"])


@pytest.mark.parametrize("R,S,seed", M.FIELD_CASES)
def test_redraw_share_of_every_field_case_of_the_device_tests(R, S, seed):
    c = M.field_case(R, S, seed)
    print(f"field_case R={R} S={S}: redrawn {c.redrawn:.5%}")
    assert c.redrawn <= M.REDRAW_CAP
    for split, stored in ((0, False), (1, True), (2, False), (2, True)):
        assert M.field_gate_margin(c, split, stored).min() > M.GATE_MARGIN


@pytest.mark.parametrize("R,S,seed", M.EXACT_FIELD_CASES)
def test_exact_field_cases_of_the_device_tests_build(R, S, seed):
    M.exact_field_case(R, S, seed)


def test_field_and_ray_head_references_are_fp64_autograd_over_the_oracle_s_field():
    """oracle/hotpath.py's field (mlp_base's layers, trunc_exp, field_outputs: the whole of mlp_head.0 with its SH and appearance
    columns) given the same hash features, in float64: the fused reference supplies d_enc, the per-ray sums and the geo columns
    of head0_w, the ray-head reference turns the per-ray sums into the layer's other columns, its bias and the embedding rows"""
    from oracle import hotpath as H

    R, S = 7, 23
    c = M.field_case(R, S, 723)
    rh = M.ray_head_case(R, 5)
    N = R * S
    r = np.random.default_rng(2)
    W0 = c.w["head0_w"].copy()
    W0[:, :16], W0[:, 16 + M.GF:] = rh.W0[:, :16], rh.W0[:, 16 + M.GF:]
    names = {"base0": "field.mlp_base.mlp.layers.0", "base1": "field.mlp_base.mlp.layers.1", "head1": "field.mlp_head.layers.1",
             "head2": "field.mlp_head.layers.2", "th0": "field.mlp_thermal.layers.0", "th1": "field.mlp_thermal.layers.1",
             "thead": "field.field_head_thermal.net"}
    sd = {}
    for k, nme in names.items():
        sd[nme + ".weight"], sd[nme + ".bias"] = t64(c.w[k + "_w"], True), t64(c.w[k + "_b"], True)
    sd["field.mlp_head.layers.0.weight"], sd["field.mlp_head.layers.0.bias"] = t64(W0, True), t64(rh.b0, True)
    sd["field.embedding_appearance.embedding.weight"] = t64(rh.emb, True)
    cfg = H.OracleConfig(sh_input="shifted", average_init_density=0.75)
    enc = t64(c.enc, True)
    h = H.mlp(enc, H._layers(sd, "field.mlp_base.mlp", 2), None)
    raw, geo = torch.split(h, [1, 15], dim=-1)
    dens = cfg.average_init_density * H.trunc_exp(raw, -15.0)[:, 0] * t64(c.selector)
    dirs = torch.from_numpy(rh.directions.astype(f64))[:, None, :].expand(R, S, 3).reshape(N, 3)
    cams = torch.from_numpy(rh.cams.astype(np.int64))[:, None].expand(R, S).reshape(N)
    rgb, th = H.field_outputs(sd, dirs, geo, cams, cfg, True)
    ((dens * t64(c.d_density)).sum() + (rgb * t64(c.d_rgb)).sum() + (th[:, 0] * t64(c.d_thermal)).sum()).backward()
    # the references: the ray's bias from the ray head, the stored rgb from that forward
    # (ray_head_forward forms the SH components in fp32, as the kernel does; the oracle in float64: the field reference gets the
    # float64 ones, and the ray head's SH columns are compared to fp32's rounding of the components below)
    ray_bias, _, _ = M.ray_head_forward(W0, rh.b0, rh.emb, rh.directions, rh.cams, True)
    sh = H.sh4((torch.from_numpy(rh.directions.astype(f64)) + 1.0) / 2.0).numpy()
    exact_bias = rh.b0.astype(f64) + sh @ W0[:, :16].astype(f64).T + rh.emb.astype(f64)[rh.cams] @ W0[:, 16 + M.GF:].astype(f64).T
    assert np.abs(ray_bias - exact_bias).max() <= 16 * 2.0 ** -23 * np.abs(W0[:, :16]).sum(1).max()
    ray_bias = exact_bias
    c = c._replace(w=dict(c.w, head0_w=W0), ray_bias=ray_bias, rgb=rgb.detach().numpy(), avg=0.75)
    a = M.field_adjoint(c, 1, False)

    def close(x, y, B):   # fp64 against fp64: to the rounding of sums whose terms add up to B in absolute value
        assert np.shape(x) == np.shape(y) and np.all(np.abs(np.asarray(x) - np.asarray(y)) <= 1e-12 * (1 + np.max(B)))

    close(a.d_enc, enc.grad.numpy(), a.B["d_enc"])
    for k, nme in names.items():
        close(a.grads[k + "_w"], sd[nme + ".weight"].grad.numpy() + c.held[k + "_w"], a.B[k + "_w"])
        close(a.grads[k + "_b"], sd[nme + ".bias"].grad.numpy().reshape(M.FIELD_SHAPES[k + "_b"]) + c.held[k + "_b"], a.B[k + "_b"])
    g0 = sd["field.mlp_head.layers.0.weight"].grad.numpy()
    close(a.grads["head0_w"][:, 16:31], g0[:, 16:31] + c.held["head0_w"][:, 16:31], a.B["head0_w"])
    b = M.ray_head_adjoint(W0, rh.emb, rh.directions, rh.cams, a.d_ray_sum - c.held_ray_sum, True, rh.held_w, rh.held_b, rh.held_emb)
    assert np.all(np.abs(b.d_w[:, :16] - (g0[:, :16] + rh.held_w[:, :16])) <= 8 * 2.0 ** -24 * b.B["d_w"][:, :16])
    close(b.d_w[:, 31:], g0[:, 31:] + rh.held_w[:, 31:], b.B["d_w"])
    close(b.d_b, sd["field.mlp_head.layers.0.bias"].grad.numpy() + rh.held_b, b.B["d_b"])
    close(b.d_emb, sd["field.embedding_appearance.embedding.weight"].grad.numpy() + rh.held_emb, b.B["d_emb"])
