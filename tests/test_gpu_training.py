"""GPU parity of the TRAINING step: every taped stage and its adjoint against torch autograd over the
CPU oracle (oracle/hotpath.py + oracle/training.py), then the whole step (outputs, losses, every parameter gradient).

Tolerances (written per test): the kernels are fp32 with a different summation order than torch's (tiled dots, atomics),
so gradients are compared in relative L2 norm per tensor; values pointwise.

The two halves of the hash encoding's adjoint are also held to fp64 references of their own, element by element: the position
gradient sample by sample (tests/position_gradient_reference.py, tests/test_gpu_position_gradient.py) and the table gradient
entry by entry, with inputs whose sums are exact in fp32 (tests/table_gradient_reference.py, tests/test_gpu_table_gradient.py)
— a whole-table L2 norm is dominated by the crowded coarse entries and would not see a lost record at a fine level.  The per-ray
kernels above them (tn_ray_render_bwd, tn_weights_bwd, tn_composite_bwd, the distortion and interlevel losses, tn_image_losses) are
held element by element to tests/ray_losses_reference.py by tests/test_gpu_ray_losses.py: exact on dyadic and single-interval
inputs, bounded by counted roundings elsewhere.  The forward half of that chain (tn_sample_pdf, tn_weights_fwd, tn_composite_fwd,
tn_depth_fwd, tn_sample_initial, the frustum kernels, tn_ray_render_fwd / tn_ray_render_depth_fwd against the modular calls) is held
the same way to tests/ray_forward_reference.py by tests/test_gpu_ray_forward.py.  The MLP stage between them (tn_linear_fwd / _bwd /
_chain_bwd, tn_field_bwd_fused in its three forms, tn_ray_head_fwd / _bwd, tn_density_fwd_train / _bwd_train) is held entry by entry to
tests/mlp_reference.py by tests/test_gpu_mlp.py, second rounds of the persistent blocks and the VALU backward included."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hotpath as H
from oracle import training as T
from tests import helpers
from thermo_nerf_amd import _hip
from thermo_nerf_amd import training as TR
from thermo_nerf_amd.rays import RayBundle

from thermo_nerf_amd import _hip as _hip_mod

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def lin_struct(w: torch.Tensor, b: torch.Tensor) -> _hip.tn_linear:
    return _hip.tn_linear(w.data_ptr(), b.data_ptr(), w.shape[1], w.shape[0])


# --------------------------------------------------------------------------------------------------
# stages
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("IN,OUT,ldx,off,act", [
    (32, 64, 32, 0, 1), (64, 16, 64, 0, 0), (63, 64, 64, 0, 1), (15, 64, 16, 1, 1), (64, 64, 64, 0, 2),
    (64, 3, 64, 0, 2), (64, 1, 64, 0, 0), (10, 16, 10, 0, 1), (16, 1, 16, 0, 0),
    # layers wider than 64 (hidden_dim* up to 256): the LDS-tiled forward, the backward one 64 x 64 weight block at a time
    (32, 128, 32, 0, 1), (128, 128, 128, 0, 1), (128, 16, 128, 0, 0), (63, 130, 64, 0, 1), (130, 130, 132, 2, 2), (130, 3, 130, 0, 2),
    (256, 256, 256, 0, 1), (200, 1, 200, 0, 0), (15, 100, 16, 1, 1), (100, 66, 100, 0, 2)])
@pytest.mark.parametrize("n", [1000, 64, 1])
def test_linear_fwd_bwd(IN, OUT, ldx, off, act, n):
    g = torch.Generator().manual_seed(IN * 100 + OUT + n)
    xfull = torch.randn(n, ldx, generator=g)
    w = (torch.randn(OUT, IN, generator=g) / IN**0.5).requires_grad_(True)
    b = torch.randn(OUT, generator=g).requires_grad_(True)
    x = xfull[:, off:off + IN].clone().requires_grad_(True)
    y = torch.nn.functional.linear(x, w, b)
    y = torch.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y
    dy = torch.randn(n, OUT, generator=g)
    y.backward(dy)

    xd, wd, bd, dyd = xfull.to(DEV), w.detach().to(DEV), b.detach().to(DEV), dy.to(DEV)
    lin = lin_struct(wd, bd)
    yd = TR.linear_fwd(xd, off, ldx, lin, act, n)
    assert (yd.cpu() - y.detach()).abs().max().item() <= 2e-5
    dx = torch.full((n, ldx), 7.0, device=DEV)
    dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
    TR.linear_bwd(xd, off, ldx, yd, dyd, OUT, lin, act, n, dx, off, ldx, False, dw, db)
    assert rel(dx[:, off:off + IN], x.grad) <= 1e-5
    if off:
        assert torch.all(dx[:, :off] == 7.0), "columns outside the layer's input were touched"
    assert rel(dw, w.grad) <= 1e-5 and rel(db, b.grad) <= 1e-5
    # accumulate_dx adds on top; weight/bias gradients accumulate (+=)
    TR.linear_bwd(xd, off, ldx, yd, dyd, OUT, lin, act, n, dx, off, ldx, True, dw, db)
    assert rel(dx[:, off:off + IN], 2 * x.grad) <= 1e-5 and rel(dw, 2 * w.grad) <= 1e-5


# (in, out, activation) bottom-up, x row stride / column offset of the bottom input, top dy width
CHAINS = {
    "mlp_head": ([(63, 64, 1), (64, 64, 1), (64, 3, 2)], 64, 0),           # REF thermal_field.py:160-168 (cin is 64 wide, 63 used)
    "mlp_thermal+head": ([(15, 64, 1), (64, 64, 2), (64, 1, 0)], 16, 1),   # REF :90-102,170-179 (input = columns 1..15 of bo)
    "mlp_base": ([(32, 64, 1), (64, 16, 0)], 32, 0),
    "proposal": ([(10, 16, 1), (16, 1, 0)], 10, 0),
    "single": ([(64, 64, 1)], 64, 0),
}


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("n", [1000, 64, 1, 4097])
def test_linear_chain_bwd(name, n):
    """tn_linear_chain_bwd (each MLP's backward in one launch) against torch autograd over the same layers."""
    spec, ldx, off = CHAINS[name]
    g = torch.Generator().manual_seed(n + len(name))
    act_fn = {0: lambda t: t, 1: torch.relu, 2: torch.sigmoid}
    xfull = torch.randn(n, ldx, generator=g)
    x0 = xfull[:, off:off + spec[0][0]].clone().requires_grad_(True)
    ws, bs, acts = [], [], []
    h = x0
    for IN, OUT, act in spec:
        w = (torch.randn(OUT, IN, generator=g) / IN**0.5).requires_grad_(True)
        b = torch.randn(OUT, generator=g).requires_grad_(True)
        h = act_fn[act](torch.nn.functional.linear(h, w, b))
        ws.append(w); bs.append(b); acts.append(h)
    dy = torch.randn(n, spec[-1][1], generator=g)
    h.backward(dy)
    # device side: the tape = activated outputs; layers listed top first, each with ITS input and the activation that made it
    xd = xfull.to(DEV)
    tape = [a.detach().to(DEV).contiguous() for a in acts]
    dws = [torch.zeros_like(w.detach()).to(DEV) for w in ws]
    dbs = [torch.zeros_like(b.detach()).to(DEV) for b in bs]
    lins = [lin_struct(w.detach().to(DEV), b.detach().to(DEV)) for w, b in zip(ws, bs)]
    keep = [l for l in lins]  # (the structs hold raw pointers of tensors created above: keep them alive)
    wkeep = [(w.detach().to(DEV), b.detach().to(DEV)) for w, b in zip(ws, bs)]
    lins = [lin_struct(w, b) for w, b in wkeep]
    layers = []
    for k in range(len(spec) - 1, -1, -1):
        if k == 0:
            layers.append((lins[0], xd, off, ldx, 0, dws[0], dbs[0]))
        else:
            layers.append((lins[k], tape[k - 1], 0, spec[k][0], spec[k - 1][2], dws[k], dbs[k]))
    top_act = spec[-1][2]
    dx = torch.full((n, ldx), 7.0, device=DEV)
    TR.linear_chain_bwd(layers, tape[-1] if top_act else None, top_act, dy.to(DEV), spec[-1][1], n, dx, off, ldx, False)
    IN0 = spec[0][0]
    assert rel(dx[:, off:off + IN0], x0.grad) <= 2e-5, rel(dx[:, off:off + IN0], x0.grad)
    if off:
        assert torch.all(dx[:, :off] == 7.0), "columns outside the chain's input were touched"
    for k in range(len(spec)):
        assert rel(dws[k], ws[k].grad) <= 2e-5, (k, rel(dws[k], ws[k].grad))
        assert rel(dbs[k], bs[k].grad) <= 2e-5, (k, rel(dbs[k], bs[k].grad))
    # accumulate_dx adds on top; weight/bias gradients accumulate (+=); dx may be NULL
    TR.linear_chain_bwd(layers, tape[-1] if top_act else None, top_act, dy.to(DEV), spec[-1][1], n, dx, off, ldx, True)
    assert rel(dx[:, off:off + IN0], 2 * x0.grad) <= 2e-5 and rel(dws[0], 2 * ws[0].grad) <= 2e-5
    TR.linear_chain_bwd(layers, tape[-1] if top_act else None, top_act, dy.to(DEV), spec[-1][1], n, None, 0, ldx, False)
    assert rel(dws[-1], 3 * ws[-1].grad) <= 2e-5
    del keep


@pytest.mark.parametrize("contraction", [True, False])
def test_hash_encode_fwd_bwd(contraction):
    L, log2T = 16, 15
    g = torch.Generator().manual_seed(3)
    table = (torch.rand(L << log2T, 2, generator=g) * 2 - 1).requires_grad_(True)
    scal = H.hash_scalings(L, 16, 2048)
    pos = (torch.rand(3000, 3, generator=g) * 2 - 1) * (3.0 if contraction else 1.3)
    cfg = H.OracleConfig(disable_scene_contraction=not contraction)
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    p, sel = H.normalized_positions(pos, cfg, aabb)
    enc = H.hash_encode(p, table, scal, log2T)
    d_enc = torch.randn(enc.shape, generator=g)
    enc.backward(d_enc)

    grid = _hip.tn_hashgrid()
    td = table.detach().to(DEV)
    grid.table, grid.num_levels, grid.log2_hashmap_size = td.data_ptr(), L, log2T
    for i, s in enumerate(scal.tolist()):
        grid.scalings[i] = s
    space = _hip.make_space(contraction, aabb)
    e, s = TR.hash_encode_fwd(grid, space, pos.to(DEV))
    assert torch.equal(s.cpu(), sel.float())
    assert (e.cpu() - enc.detach()).abs().max().item() <= 1e-6
    # records bucketed by owning slice + LDS sums | global atomics; the coarsest levels through private dense copies or not
    for bucketed, spread in ((0, True), (5, True), (5, False), (False, True), (False, False)):
        d_table = torch.zeros_like(td)
        for _ in range(2):  # twice: the spread workspace is cleared by every call
            d_table.zero_()
            TR.hash_encode_bwd(grid, space, pos.to(DEV), d_enc.to(DEV), d_table, bucketed=bucketed, spread=spread)
        assert rel(d_table, table.grad) <= 1e-5, (bucketed, spread)
        # untouched entries stay exactly zero
        assert torch.all(d_table.cpu()[table.grad == 0] == 0)


@pytest.mark.parametrize("L,log2T,max_res,n", [(16, 19, 2048, 4096 * 48), (5, 17, 256, 4097), (16, 15, 2048, 1000), (5, 13, 128, 1),
                                               (16, 12, 2048, 777), (16, 19, 2048, 3)])
def test_bucketed_table_scatter_matches_the_atomic_one(L, log2T, max_res, n):
    """tn_hash_encode_bwd_sorted (count -> scan -> emit -> one LDS-owning block per table slice) against tn_hash_encode_bwd
    (global atomics): 32 / 8 / 2 / 1 slices per level, tables smaller than a slice, ragged and tiny sample counts, samples
    without gradient (no record), rays of neighbouring samples (many records per entry at the coarse levels) and a d_table
    that already holds values (+=).  Both sum the same products in a different order: 1e-5 relative."""
    g = torch.Generator().manual_seed(L * 1000 + log2T + n)
    scal = H.hash_scalings(L, 16, max_res)
    rays = max(1, n // 48)
    o = (torch.rand(rays, 1, 3, generator=g) - 0.5) * 1.5
    d = torch.nn.functional.normalize(torch.randn(rays, 1, 3, generator=g), dim=-1)
    t = torch.sort(torch.rand(rays, 48, 1, generator=g), dim=1).values * 4.0
    pos = (o + d * t).reshape(-1, 3)[:n].contiguous()
    if pos.shape[0] < n:
        pos = torch.cat([pos, (torch.rand(n - pos.shape[0], 3, generator=g) * 2 - 1) * 2.0])
    d_enc = torch.randn(n, 2 * L, generator=g)
    d_enc[torch.rand(n, generator=g) < 0.3] = 0.0          # whole samples without gradient
    d_enc[:, 2::6] = 0.0                                   # and single features
    d_enc[0, 1::2] = 1.0                                   # (the first sample always carries some)
    grid = _hip.tn_hashgrid()
    grid.table, grid.num_levels, grid.log2_hashmap_size = 0, L, log2T
    table = torch.zeros(L << log2T, 2, device=DEV)
    grid.table = table.data_ptr()
    for i, s in enumerate(scal.tolist()):
        grid.scalings[i] = s
    space = _hip.make_space(True, torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]))
    assert _hip.load().tn_hash_encode_bwd_sorted_workspace_bytes(grid, n, 0) > 0
    # the library's advice (bucketed=True follows it; explicit levels here): from the first level with a scaling >= 200, if
    # that leaves at least 128 (level, slice) bins
    fine = [i for i, sc in enumerate(scal.tolist()) if sc >= 200]
    advised = fine[0] if fine and ((L - fine[0]) << max(0, log2T - 14)) >= 128 else -1
    assert _hip.load().tn_hash_encode_bwd_sorted_first_level(grid, n) == advised
    a, b = torch.zeros(L << log2T, 2, device=DEV), torch.zeros(L << log2T, 2, device=DEV)
    TR.hash_encode_bwd(grid, space, pos.to(DEV), d_enc.to(DEV), a, bucketed=0)
    TR.hash_encode_bwd(grid, space, pos.to(DEV), d_enc.to(DEV), b, bucketed=False)
    assert float(b.abs().sum()) > 0
    assert rel(a, b) <= 1e-5
    assert torch.equal(a == 0, b == 0)                      # the same entries are touched
    # (+=): on top of what the table gradient already holds
    start = torch.randn(L << log2T, 2, generator=g).to(DEV)
    c = start.clone()
    TR.hash_encode_bwd(grid, space, pos.to(DEV), d_enc.to(DEV), c, bucketed=min(2, L - 1))
    assert rel(c, start + b) <= 1e-6
    assert torch.equal(c[b == 0], start[b == 0])            # untouched entries keep their value bit for bit


@pytest.mark.parametrize("n", [48, 64, 96, 256, 300])
def test_weights_bwd(n):
    g = torch.Generator().manual_seed(n)
    R = 37
    deltas = torch.rand(R, n, generator=g) * 0.2
    dens = (torch.rand(R, n, generator=g) * 4).requires_grad_(True)
    dens.data[3, : n // 2] = 0.0
    dens.data[5] *= 40.0  # saturates early: tiny transmittance behind
    w = H.get_weights(deltas[..., None], dens[..., None])[..., 0]
    gw = torch.randn(R, n, generator=g)
    w.backward(gw)
    got = TR.weights_bwd(deltas.to(DEV), dens.detach().to(DEV), gw.to(DEV))
    assert rel(got, dens.grad) <= 1e-5


@pytest.mark.parametrize("C", [3, 1])
def test_composite_bwd(C):
    g = torch.Generator().manual_seed(C)
    R, n = 41, 48
    v = torch.rand(R, n, C, generator=g).requires_grad_(True)
    w = (torch.rand(R, n, 1, generator=g) / n).requires_grad_(True)
    out = H.render_rgb(v, w, True) if C == 3 else H.render_thermal(v, w, True)
    go = torch.randn(R, C, generator=g)
    out.backward(go)
    lib = _hip.load()
    vd, wd, god = v.detach().to(DEV), w.detach().reshape(R, n).to(DEV), go.to(DEV)
    acc = wd.sum(dim=1).contiguous()
    gv = torch.empty(R, n, C, device=DEV)
    gw = torch.full((R, n), 0.5, device=DEV)  # (+=) on top of what is there
    _hip.check(lib.tn_composite_bwd(vd.data_ptr(), wd.data_ptr(), acc.data_ptr(), god.data_ptr(), R, n, C, gv.data_ptr(),
                                    gw.data_ptr(), _hip.current_stream()), "tn_composite_bwd")
    assert rel(gv, v.grad) <= 1e-6
    assert rel(gw - 0.5, w.grad[..., 0]) <= 1e-5


def _levels(R, ns, seed):
    """monotone spacing bins + positive weights per level, CPU"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in ns:
        edges = torch.sort(torch.rand(R, n + 1, generator=g), dim=1).values
        edges[:, 0], edges[:, -1] = 0.0, 1.0
        w = torch.rand(R, n, generator=g)
        w = w / w.sum(dim=1, keepdim=True) * torch.rand(R, 1, generator=g)
        s = H.Samples(None, None, edges[:, :-1, None], edges[:, 1:, None], None, None)
        out.append((s, w[..., None]))
    return out


@pytest.mark.parametrize("n", [48, 64, 192])
def test_distortion_loss_and_gradient(n):
    (s, w), = _levels(29, [n], n)
    w = w.clone().requires_grad_(True)
    want = T.distortion_loss([w], [s])
    want.backward()

    class RS:  # what training.distortion_loss reads from a RaySamples
        spacing_bins = torch.cat([s.spacing_starts[..., 0], s.spacing_ends[:, -1:, 0]], dim=1).to(DEV)

    wd = w.detach().to(DEV).requires_grad_(True)
    got = TR.distortion_loss([wd], [RS])
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-8
    assert rel(wd.grad, w.grad) <= 2e-5

    # the model's form: the metric plus distortion_loss_mult * metric from the same launch [REF thermal_nerf_model.py:301-304]
    mult = 0.002
    w2 = w.detach().to(DEV).requires_grad_(True)
    metric = TR.distortion_loss([w2], [RS], mult=mult)
    m, term = metric.scaled_term
    assert m == mult and abs(metric.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-8
    assert abs(term.item() - mult * want.item()) <= 1e-5 * abs(mult * want.item()) + 1e-10
    (term + 3.0 * metric).backward()  # both outputs differentiate: (mult + 3) * d metric / d w
    assert rel(w2.grad, (mult + 3.0) * w.grad) <= 2e-5


@pytest.mark.parametrize("ns", [(256, 96, 48), (64, 300, 192), (5, 7, 3), (1024, 1000, 1024)])
def test_interlevel_loss_and_gradient(ns):
    lv = _levels(23, ns, sum(ns))
    ws = [w.clone().requires_grad_(True) for _, w in lv]
    want = T.interlevel_loss(ws, [s for s, _ in lv])
    want.backward()

    def rs(s):
        class RS:
            spacing_bins = torch.cat([s.spacing_starts[..., 0], s.spacing_ends[:, -1:, 0]], dim=1).to(DEV)
        return RS

    wd = [w.detach().to(DEV).requires_grad_(True) for w in ws]
    got = TR.interlevel_loss(wd, [rs(s) for s, _ in lv])
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-9
    tol = 2e-5 if max(ns) <= 512 else 1e-4  # reverse prefix sums over up to 1024 fp32 terms
    for a, b in zip(wd[:-1], ws[:-1]):
        assert rel(a.grad, b.grad) <= tol
    assert wd[-1].grad is None and ws[-1].grad is None  # the final level is detached in this loss
    w5 = [w.detach().to(DEV).requires_grad_(True) for w in ws]
    got5 = TR.interlevel_loss(w5, [rs(s) for s, _ in lv], mult=0.5)  # interlevel_loss_mult folded into the kernels' scale
    got5.backward()
    assert abs(got5.item() - 0.5 * want.item()) <= 1e-5 * abs(want.item()) + 1e-9
    for a, b in zip(w5[:-1], ws[:-1]):
        assert rel(a.grad, 0.5 * b.grad) <= tol


# --------------------------------------------------------------------------------------------------
# the whole step
# --------------------------------------------------------------------------------------------------
def _train_setup(kind, S, R_hw=(12, 12), seed=11, **over):
    over.setdefault("camera_optimizer_mode", "off")
    cm, sd, ocfg = helpers.build(kind, S, **over)
    gm = copy.deepcopy(cm).to(DEV)
    gm.train()
    o, d = helpers.rays(*R_hw, view=3)
    R = o.shape[0]
    g = torch.Generator().manual_seed(seed)
    jit = [torch.rand(R, 1, generator=g) for _ in range(3)]
    cam = torch.randint(0, 8, (R, 1), generator=g)
    batch = {"image": torch.rand(R, 3, generator=g), "thermal": torch.rand(R, 1, generator=g)}
    return gm, sd, ocfg, o, d, jit, cam, batch


def _gpu_step(gm, o, d, jit, cam, batch):
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV))
    rb = gm.collider(rb)
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    b = {k: v.to(DEV) for k, v in batch.items()}
    metrics = gm.get_metrics_dict(out, b)
    loss_dict = gm.get_loss_dict(out, b, metrics)
    gm.zero_grad(set_to_none=True)
    sum(loss_dict.values()).backward()
    return out, loss_dict


@pytest.mark.parametrize("kind", ["stress", "scene"])
def test_total_loss_with_the_unit_seed_equals_sum_and_backward(kind):
    """training.total_loss + backward_total (one summing node; a cached ones tensor as the seed, which the loss Functions recognise
    and pass their stored gradients through without the `seed * gradient` launches) against the plain `sum(loss_dict.values())
    .backward()` of NS Trainer.train_iteration: the same loss and bit-identical gradients of everything but the atomically
    accumulated tables; a NON-unit seed through the same node scales every gradient."""
    grads, losses = {}, {}
    for mode in ("sum", "total", "total_x3"):
        gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, 48)
        rb = gm.collider(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
        out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
        b = {k: v.to(DEV) for k, v in batch.items()}
        loss_dict = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
        gm.zero_grad(set_to_none=True)
        if mode == "sum":
            loss = sum(loss_dict.values())
            loss.backward()
        elif mode == "total":
            loss = TR.total_loss(loss_dict)
            TR.backward_total(loss)
        else:
            loss = TR.total_loss(loss_dict)
            loss.backward(torch.full((), 3.0, device=DEV))
        losses[mode] = float(loss.detach())
        grads[mode] = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
    assert abs(losses["total"] - losses["sum"]) <= 1e-6 * abs(losses["sum"]) and losses["total_x3"] == losses["total"]
    assert set(grads["total"]) == set(grads["sum"]) == set(grads["total_x3"])
    for n, g in grads["sum"].items():
        if n.endswith("hash_table") or "camera_optimizer" in n:  # atomics: the summation order is not reproducible
            assert rel(grads["total"][n], g) <= 1e-5, n
        else:
            assert rel(grads["total"][n], g) <= 1e-6, (n, rel(grads["total"][n], g))
        if g.norm().item() > 1e-10:
            assert rel(grads["total_x3"][n], 3.0 * g) <= 1e-5, n


ONE_NET = {"one_proposal_network": True}  # helpers.build: use_same_proposal_network + a one-entry proposal_net_args_list


@pytest.mark.parametrize("variant", ["default", "taped", "stage_forward", "gradient_scaling", "same_proposal_network",
                                     "uniform_initial_sampler", "trunc_exp_one_sided"])
@pytest.mark.parametrize("kind", ["stress", "scene"])
@pytest.mark.parametrize("S", [48, 64, 192])  # 192 = BASELINE config 3 (multi-chunk scans in every per-ray kernel)
def test_training_step_matches_autograd_oracle(kind, S, variant):
    """variant: the reference's config switches on this path — use_gradient_scaling [REF thermal_nerf_model.py:228-231],
    use_same_proposal_network [REF :122-139] and proposal_initial_sampler="uniform" [REF :164-170] — next to the default
    configuration."""
    if variant not in ("default", "taped", "stage_forward") and S != 48:
        pytest.skip("config variants are checked at the reference's default sample count")
    # default = the tape-free final level (tn_field_fwd_train + tn_field_bwd_fused: the hidden layers recomputed in the backward);
    # taped = the final level's forward as one MFMA kernel writing the tape (tn_field_fwd_taped) and each MLP's backward as one
    # launch (tn_linear_chain_bwd); stage_forward = one launch per nerfstudio module / layer in both directions
    over = {"gradient_scaling": {"use_gradient_scaling": True}, "same_proposal_network": ONE_NET,
            "taped": {"tape_free_training": False, "fused_proposal_training": False},
            "stage_forward": {"tape_free_training": False, "fused_train_forward": False, "fused_train_backward": False,
                              "fused_proposal_training": False},
            "trunc_exp_one_sided": {"trunc_exp_clamp_min": float("-inf")},
            "uniform_initial_sampler": {"proposal_initial_sampler": "uniform", "far_plane": 6.0}}.get(variant, {})
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, S, **over)
    if variant == "same_proposal_network":
        assert len(gm.proposal_networks) == 1
    out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    # forward values: same tolerances as the forward parity tests
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu() - want_out[k].detach()).abs().max().item() <= 2e-5, k
    for i in range(3):
        assert (out["weights_list"][i].detach().cpu() - want_out["weights_list"][i].detach()).abs().max().item() <= 2e-5
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    # every parameter gradient, relative L2 per tensor (fp32, different summation order, atomics)
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__"):
            continue
        gg = named[name].grad
        if gw.norm().item() == 0.0:
            assert gg is None or gg.abs().max().item() == 0.0, name
            continue
        assert gg is not None, f"{name}: no gradient"
        if gw.norm().item() < 1e-10:
            # an interlevel loss that is zero up to rounding (the proposal envelope already covers the final weights)
            # leaves gradients made of a few max(w - w_outer, 0) terms at the 1e-14 level: only their size is comparable
            assert gg.norm().item() < 1e-9, name
            continue
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e} (|g| {gw.norm().item():.2e})"
        checked += 1
    assert checked >= (13 if variant == "same_proposal_network" else 18)


def test_transient_embedding_flag_leaves_the_step_unchanged():
    """use_transient_embedding=True [REF thermal_nerf_model.py:111]: the reference's model never reads the transient heads (G10,
    tests/golden/transient_embedding.json) — eval outputs, training outputs, losses and every gradient equal the flag-off model's on
    the same weights; the transient parameters receive no gradient (as in the reference)."""
    res = {}
    for flag in (False, True):
        gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 48, use_transient_embedding=flag)
        if flag:  # the SAME weights (the counter-hash fill numbers its streams by parameter position: more parameters, other values)
            missing = gm.load_state_dict(res[False][4], strict=False)
            assert all("transient" in k for k in missing.missing_keys) and not missing.unexpected_keys
        state = {k: v.clone() for k, v in gm.state_dict().items()}
        out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
        assert not any("transient" in n for n in grads)
        gm.eval()
        with torch.no_grad():
            ev = gm(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
        res[flag] = (out, loss_dict, grads, ev, state)
    (o0, l0, g0, e0, _), (o1, l1, g1, e1, _) = res[False], res[True]
    for k in ("rgb", "thermal", "accumulation", "depth", "expected_depth"):
        assert torch.equal(o0[k], o1[k]) and torch.equal(e0[k], e1[k]), k
    assert set(g0) == set(g1)
    for n in g0:
        assert rel(g1[n], g0[n]) <= 2e-5, n
    for k in l0:
        assert abs(float(l0[k].detach()) - float(l1[k].detach())) <= 1e-6 * abs(float(l0[k].detach())), k


@pytest.mark.parametrize("widths", [(32, 16, 48), (16, 64, 8), (128, 128, 128), (100, 130, 66), (256, 72, 200)])
@pytest.mark.parametrize("kind", ["stress", "scene"])
def test_training_step_with_other_mlp_widths(kind, widths):
    """hidden_dim / hidden_dim_color / hidden_dim_transient other than 64 (field.staged): the training step takes the stage-by-stage
    forward and one tn_linear_bwd per layer (a layer above 64 wide: one pass of the 64-wide kernel per 64 x 64 block of its weight
    matrix); outputs, losses and every parameter gradient against torch autograd over the oracle."""
    hd, hc, ht = widths
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, 48, hidden_dim=hd, hidden_dim_color=hc, hidden_dim_transient=ht)
    assert gm.field.staged
    out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu() - want_out[k].detach()).abs().max().item() <= 2e-5, k
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__") or gw.norm().item() < 1e-10:
            continue
        gg = named[name].grad
        assert gg is not None and gg.shape == gw.shape, name
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e}"
        checked += 1
    assert checked >= 18


@pytest.mark.parametrize("widths", [(32, 16, 48), (128, 128, 128)])
@pytest.mark.parametrize("variant", ["pose", "pose_sh", "gradient_scaling"])
def test_training_step_with_other_mlp_widths_and_step_variants(widths, variant):
    """field.staged (widths other than 64) under the step's other switches: camera-pose optimisation (the ray gradients through the
    staged field's positions), the SH-basis term of the direction gradient, gradient scaling — every parameter gradient against the
    autograd oracle."""
    over = {"pose": {"camera_optimizer_mode": "SO3xR3"}, "pose_sh": {"camera_optimizer_mode": "SO3xR3", "sh_direction_gradient": True},
            "gradient_scaling": {"use_gradient_scaling": True}}[variant]
    hd, hc, ht = widths
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 48, hidden_dim=hd, hidden_dim_color=hc, hidden_dim_transient=ht, **over)
    assert gm.field.staged
    od, dd = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)  # what a camera optimizer differentiates
    rb = gm.collider(RayBundle(origins=od, directions=dd, camera_indices=cam.to(DEV)))
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    b = {k: v.to(DEV) for k, v in batch.items()}
    loss_dict = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
    gm.zero_grad(set_to_none=True)
    sum(loss_dict.values()).backward()
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__") or gw.norm().item() < 1e-10:
            continue
        gg = named[name].grad
        assert gg is not None and gg.shape == gw.shape, name
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e}"
        checked += 1
    assert checked >= 18
    # (the fine levels' position gradients cancel: the fp32 oracle itself is 3e-3 ... 1e-2 from its fp64 run, see the 64-wide test)
    assert rel(od.grad, want_grads["__origins__"]) <= 2e-2 and rel(dd.grad, want_grads["__directions__"]) <= 2e-2


@pytest.mark.parametrize("R_hw,P,S", [((1, 1), (7, 5), 3), ((3, 21), (33, 17), 13), ((5, 13), (256, 96), 1), ((13, 5), (2, 3), 70),
                                      ((1, 2), (130, 300), 200)])
@pytest.mark.parametrize("pose", [False, True])
def test_training_step_on_odd_shapes(R_hw, P, S, pose):
    """The training step on shapes that are multiples of nothing — one ray, 63 and 65 rays, one field sample per ray, a second proposal
    level larger than the first — with and without camera-pose optimisation, on an update step (the proposal networks take gradient):
    outputs, losses and every parameter gradient against torch autograd over the oracle."""
    over = {"camera_optimizer_mode": "SO3xR3"} if pose else {}
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", S, R_hw=R_hw, num_proposal_samples_per_ray=P, **over)
    out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu() - want_out[k].detach()).abs().max().item() <= 2e-5, k
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__") or gw.norm().item() < 1e-10:
            continue
        gg = named[name].grad
        assert gg is not None and gg.shape == gw.shape, name
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e}"
        checked += 1
    assert checked >= 12


@pytest.mark.parametrize("variant", ["default", "pose", "pose_sh", "gradient_scaling", "no_thermal_gradients", "deferred"])
@pytest.mark.parametrize("S", [48, 192])
def test_step_calls_equal_the_per_call_path(S, variant):
    """config.fused_step_calls (round 6): on a step whose proposal networks take no gradient the forward's launch chain
    and the backward's are ONE C-ABI call each (tn_train_step_fwd / tn_train_step_bwd) — the same entry points, in the same order, on
    the same streams as the per-call host path.  Every forward output is BIT-EQUAL between the two; the gradients agree to the
    per-call path's own run-to-run noise (its partial sums meet in atomics: two runs of ONE path differ by 1e-7 relative per
    tensor; asserted: 1e-6, 2e-5 for the table / embedding / pose gradients).  With camera-pose optimisation, the SH-basis term, gradient scaling, a detached thermal branch, and the deferred table
    update (both scatter halves left on the side streams)."""
    over = {"pose": {"camera_optimizer_mode": "SO3xR3"}, "pose_sh": {"camera_optimizer_mode": "SO3xR3", "sh_direction_gradient": True},
            "gradient_scaling": {"use_gradient_scaling": True}, "no_thermal_gradients": {"pass_thermal_gradients": False}}.get(variant, {})
    res = {}
    for fused in (True, False):
        gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", S, R_hw=(16, 12), small=(S == 48), **over)
        gm.config.fused_step_calls = fused
        gm.config.deferred_table_update = variant == "deferred"
        gm.set_step(5000)
        gm.proposal_sampler._steps_since_update = 0  # a frozen step: the sampler's schedule asks for an update every 6th
        bundle = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV))
        torch.manual_seed(5)
        out = gm(bundle)
        assert out["weights_list"][0].requires_grad is False
        b = {k: v.to(DEV) for k, v in batch.items()}
        loss_dict = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
        gm.zero_grad(set_to_none=True)
        TR.backward_total(TR.total_loss(loss_dict))
        _hip_mod.join_pending()
        torch.cuda.synchronize()
        res[fused] = ({k: v.detach().clone() for k, v in out.items() if isinstance(v, torch.Tensor)},
                      [w.detach().clone() for w in out["weights_list"]], {k: v.detach().clone() for k, v in loss_dict.items()},
                      {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None})
    (o1, w1, l1, g1), (o0, w0, l0, g0) = res[True], res[False]
    for k in o0:
        assert torch.equal(o1[k], o0[k]), k
    for a, b_ in zip(w1, w0):
        assert torch.equal(a, b_)
    for k in l0:  # (the regularisers' loss kernels sum per-ray terms with one atomic per wave: the last bit is not reproducible)
        assert torch.equal(l1[k], l0[k]) or (k in ("interlevel_loss", "distortion_loss") and abs(float(l1[k]) - float(l0[k])) <= 1e-6 * abs(float(l0[k]))), k
    assert set(g1) == set(g0) and "field.mlp_base.encoder.hash_table" in g0 and len(g0) >= (12 if variant == "no_thermal_gradients" else 15)
    for n, g in g0.items():
        atomic = n.endswith("hash_table") or "embedding" in n or n.startswith("camera_optimizer") or n.endswith("mlp_head.layers.0.weight") \
            or n.endswith("mlp_head.layers.0.bias")
        assert rel(g1[n], g) <= (2e-5 if atomic else 1e-6), (n, rel(g1[n], g))


@pytest.mark.parametrize("pieces", [True, False])
@pytest.mark.parametrize("S", [48, 192])
@pytest.mark.parametrize("kind", ["stress", "scene"])
def test_training_step_gradients_against_the_fp64_oracle(kind, S, pieces):
    """The whole step's parameter gradients with the oracle's FP64 run as the yardstick (SURVEY §8f-2 "gradcheck vs
    restatement (fp64 ...)"): a fixed 2e-3 per tensor would let a dropped small term through, and the default backward runs its
    K >= 32 products as bf16 pieces.  Per tensor: rel(HIP, fp64) <= 2 x rel(fp32 oracle, fp64) + 1e-5 — the HIP step may be at most
    twice as far from the exact gradient as torch's own fp32 evaluation of the same graph is — with backward_bf16_pieces on (the
    default: six-product splits of three exact bf16 pieces per operand) AND off (every product on the fp32 MFMA)."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, S, backward_bf16_pieces=pieces)
    assert gm.config.tape_free_training and gm.config.backward_bf16_pieces is pieces
    _gpu_step(gm, o, d, jit, cam, batch)
    _, _, g32 = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    _, _, g64 = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit, dtype=torch.float64)
    named = dict(gm.named_parameters())
    rows, bad = [], []
    for name, gw in g64.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__") or gw.norm().item() < 1e-10:
            continue
        gg = named[name].grad
        assert gg is not None, name
        r_hip = float((gg.detach().cpu().double() - gw).norm() / gw.norm())
        r_32 = float((g32[name].double() - gw).norm() / gw.norm())
        rows.append((name, r_hip, r_32))
        if r_hip > 2.0 * r_32 + 1e-5:
            bad.append((name, r_hip, r_32))
    print("\n".join(f"{n:58s} hip {a:.2e}  fp32 oracle {b:.2e}  ratio {a / max(b, 1e-30):.2f}" for n, a, b in rows))
    assert len(rows) >= 18 and not bad, bad


@pytest.mark.parametrize("update_step", [True, False])
@pytest.mark.parametrize("S,hw", [(48, (12, 12)), (192, (7, 5))])
@pytest.mark.parametrize("kind", ["stress", "scene"])
def test_training_step_with_one_jitter_draw_per_bin_edge(kind, S, hw, update_step):
    """use_single_jitter=False [REF thermal_nerf_model.py:176, nerfacto_config/thermal_nerfacto.py]: every bin edge of every level
    gets its own stratified draw ([R,n+1] per level).  Update steps sample level by level (tn_sample_initial / tn_sample_pdf with
    bit 1 set); the other steps run the proposal levels as one kernel reading tn_render_inputs.jitter in the per-edge layout
    (tn_render_config.per_sample_jitter).  Both against torch autograd over the oracle with the same draws."""
    gm, sd, ocfg, o, d, _, cam, batch = _train_setup(kind, S, R_hw=hw, use_single_jitter=False)
    assert gm.config.use_single_jitter is False
    R = o.shape[0]
    counts = (*gm.config.num_proposal_samples_per_ray, S)
    g = torch.Generator().manual_seed(S + R)
    jit = [torch.rand(R, n + 1, generator=g) for n in counts]
    if not update_step:
        gm.set_step(5000)
        gm.proposal_sampler._steps_since_update = 0
    rb = gm.collider(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
    out = TR.get_outputs_train(gm, rb, jitter=[j.to(DEV) for j in jit])
    assert out["weights_list"][0].requires_grad is update_step
    b = {k: v.to(DEV) for k, v in batch.items()}
    loss_dict = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
    gm.zero_grad(set_to_none=True)
    sum(loss_dict.values()).backward()
    anneal = float(gm.proposal_sampler._anneal)
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit, anneal=anneal,
                                                       proposal_requires_grad=update_step)
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu() - want_out[k].detach()).abs().max().item() <= 2e-5, k
    for i in range(3):
        assert (out["weights_list"][i].detach().cpu() - want_out["weights_list"][i].detach()).abs().max().item() <= 2e-5, i
        want_sp = torch.cat([want_out["ray_samples_list"][i].spacing_starts[..., 0],
                             want_out["ray_samples_list"][i].spacing_ends[:, -1:, 0]], -1)
        got_sp = out["ray_samples_list"][i].spacing_bins
        assert (got_sp.detach().cpu() - want_sp.detach()).abs().max().item() <= 1e-5, i
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw is None or gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__"):
            continue
        gg = named[name].grad
        if gw.norm().item() < 1e-10:
            assert gg is None or gg.norm().item() < 1e-9, name
            continue
        assert gg is not None, f"{name}: no gradient"
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e}"
        checked += 1
    assert checked >= (18 if update_step else 8)
    # the model's own draws: the per-edge layout, different per call, and a [3,R] tensor is refused by size
    a = TR.get_outputs_train(gm, rb)["rgb"].detach().clone()
    c = TR.get_outputs_train(gm, rb)["rgb"].detach()
    assert torch.isfinite(a).all() and not torch.equal(a, c)
    with pytest.raises(ValueError, match="draws"):
        TR.get_outputs_train(gm, rb, jitter=torch.rand(3, R, device=DEV))


def test_training_step_at_config3_sizes_matches_autograd_oracle():
    """BASELINE config 3's step held against the ORACLE at its real sizes (VERDICT r4 Weak #5: the full-size step was only held
    against other forms of the HIP step): S = 192 samples per ray on the FULL-SIZE tables (16 x 2^19 field entries, 5 x 2^17 per
    proposal grid), the default tape-free step with the bucketed scatter, 256 rays (what torch autograd over the CPU oracle does in
    seconds) — outputs, every loss term and every parameter gradient, the 64 MB table gradient included."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 192, R_hw=(16, 16), small=False)
    assert gm.field.mlp_base.encoder.hash_table.shape[0] == 16 << 19 and gm.config.bucketed_table_scatter and gm.config.tape_free_training
    out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
    want_out, want_loss, want_grads = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu() - want_out[k].detach()).abs().max().item() <= 2e-5, k
    for k, v in want_loss.items():
        assert abs(loss_dict[k].item() - v.item()) <= 2e-5 * abs(v.item()) + 1e-8, (k, loss_dict[k].item(), v.item())
    named = dict(gm.named_parameters())
    checked = 0
    for name, gw in want_grads.items():
        if gw.numel() == 0 or name.startswith("camera_optimizer") or name.startswith("__") or gw.norm().item() < 1e-10:
            continue
        gg = named[name].grad
        assert gg is not None, f"{name}: no gradient"
        assert rel(gg, gw) <= 2e-3, f"{name}: rel {rel(gg, gw):.2e} (|g| {gw.norm().item():.2e})"
        if name.endswith("hash_table"):  # the same entries touched: 256 rays reach a small part of a full-size table
            touched = gw != 0
            assert 0 < int(touched.sum()) < gw.numel() // 4
            # (entries where the oracle's contributions cancel to an exact zero may hold rounding residue here: 1e-12 against 1e-5)
            assert float(gg.cpu()[~touched].abs().max()) <= 1e-6 * float(gw.abs().max()), name
            assert int((gg.cpu()[~touched] != 0).sum()) <= max(64, int(touched.sum()) // 1000), name  # (measured: 102 of 1.6e7)
        checked += 1
    assert checked >= 18


@pytest.mark.parametrize("hw", [(12, 12), (7, 5), (1, 1)])  # 6912 (a multiple of 64), 1680 and 48 samples
def test_fused_field_forward_writes_the_stage_chain_tape(hw):
    """tn_field_fwd_taped against the chain of stage entry points it replaces, tape tensor by tape tensor."""
    from thermo_nerf_amd import _hip

    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48, R_hw=hw)
    lib = _hip.load()
    R, S = o.shape[0], 48
    N = R * S
    dd, cc = d.to(DEV), cam.to(DEV).reshape(-1).to(torch.int32)
    pos = (torch.rand(N, 3, generator=torch.Generator().manual_seed(3)) * 3 - 1.5).to(DEV)  # inside and outside the unit box
    fld = gm.field.c_struct(prepare=True, dense=False)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    enc, sel, dens, h1, bo = f32(N, 32), f32(N), f32(N), f32(N, 64), f32(N, 16)
    c1, c2, rgb, t1, t2, th = f32(N, 64), f32(N, 64), f32(N, 3), f32(N, 64), f32(N, 64), f32(N, 1)
    _hip.check(lib.tn_field_fwd_taped(fld, pos.data_ptr(), dd.data_ptr(), cc.data_ptr(), R, S, enc.data_ptr(), sel.data_ptr(),
                                      h1.data_ptr(), bo.data_ptr(), dens.data_ptr(), c1.data_ptr(), c2.data_ptr(), rgb.data_ptr(),
                                      t1.data_ptr(), t2.data_ptr(), th.data_ptr(), _hip.current_stream()), "tn_field_fwd_taped")
    # the chain it replaces
    enc_s, sel_s = TR.hash_encode_fwd(fld.grid, fld.space, pos)
    h1_s = TR.linear_fwd(enc_s, 0, 32, fld.base0, TR.ACT_RELU, N)
    bo_s = TR.linear_fwd(h1_s, 0, 64, fld.base1, TR.ACT_NONE, N)
    dens_s = f32(N)
    _hip.check(lib.tn_density_act_fwd(bo_s.data_ptr(), 16, sel_s.data_ptr(), fld.average_init_density, N, dens_s.data_ptr(),
                                      _hip.current_stream()), "tn_density_act_fwd")
    cin = f32(N, 64)
    _hip.check(lib.tn_color_input_fwd(fld, dd.data_ptr(), bo_s.data_ptr() + 4, 16, cc.data_ptr(), 1, R, S, cin.data_ptr(),
                                      _hip.current_stream()), "tn_color_input_fwd")
    c1_s = TR.linear_fwd(cin, 0, 64, fld.head0, TR.ACT_RELU, N)
    c2_s = TR.linear_fwd(c1_s, 0, 64, fld.head1, TR.ACT_RELU, N)
    rgb_s = TR.linear_fwd(c2_s, 0, 64, fld.head2, TR.ACT_SIGMOID, N)
    t1_s = TR.linear_fwd(bo_s, 1, 16, fld.th0, TR.ACT_RELU, N)
    t2_s = TR.linear_fwd(t1_s, 0, 64, fld.th1, TR.ACT_SIGMOID, N)
    th_s = TR.linear_fwd(t2_s, 0, 64, fld.thead, TR.ACT_NONE, N)
    torch.cuda.synchronize()
    assert torch.equal(sel, sel_s)
    for name, got, want, tol in (("enc", enc, enc_s, 2e-6), ("h1", h1, h1_s, 1e-5), ("bo", bo, bo_s, 2e-5), ("c1", c1, c1_s, 2e-5),
                                 ("c2", c2, c2_s, 3e-5), ("rgb", rgb, rgb_s, 1e-5), ("t1", t1, t1_s, 2e-5), ("t2", t2, t2_s, 1e-5),
                                 ("thermal", th, th_s, 2e-5)):
        err = (got - want).abs().max().item()
        assert err <= tol * max(1.0, want.abs().max().item()), f"{name}: {err:.3e}"
    assert rel(dens, dens_s) <= 1e-5


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("hw", [(12, 12), (7, 5), (1, 1), (1, 3)])  # (7,5) x 5 = 175 samples: a ragged last 16-sample tile
@pytest.mark.parametrize("S", [48, 192, 5])
@pytest.mark.parametrize("kind", ["stress", "scene"])
def test_tape_free_step_equals_the_taped_step(kind, S, hw, split):
    """tn_field_fwd_train + tn_field_bwd_fused (nothing but 38 floats per sample kept, the hidden layers recomputed in the
    backward; split: three launches colour head | thermal head | mlp_base, or the whole field in one) against the taped forward + chained backward on the same batch: same outputs, losses and parameter gradients up
    to fp32 summation order (the oracle comparison of both is test_training_step_matches_autograd_oracle)."""
    got = {}
    for tape_free in (True, False):
        gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, S, R_hw=hw, tape_free_training=tape_free, fused_backward_split=split)
        out, loss = _gpu_step(gm, o, d, jit, cam, batch)
        got[tape_free] = (out, loss, {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None})
    (o1, l1, g1), (o0, l0, g0) = got[True], got[False]
    for k in ("rgb", "thermal", "accumulation", "depth", "expected_depth"):
        assert (o1[k] - o0[k]).abs().max().item() <= 1e-5, k
    for k in l0:
        assert abs(l1[k].item() - l0[k].item()) <= 1e-5 * abs(l0[k].item()) + 1e-9, k
    assert set(g1) == set(g0)
    for n, g in g0.items():
        if g.norm().item() < 1e-10:
            assert g1[n].norm().item() < 1e-9, n
            continue
        assert rel(g1[n], g) <= 2e-4, f"{n}: rel {rel(g1[n], g):.2e} (|g| {g.norm().item():.2e})"


FIELD_TRAIN_FORMS = ((True, 1), (False, 1), (True, 2), (True, "jac"))


def field_train_forms(S, hw, pos=None, forms=FIELD_TRAIN_FORMS):
    """The call plumbing around tn_field_fwd_train / tn_field_bwd_fused on the "stress" model with R = hw rays x S samples:
    tn_field_fwd_taped (the tape to compare with), tn_field_fwd_train three times (base rows kept | nothing optional | base rows
    and the position Jacobian kept, each into buffers with a guard row behind them) and one tn_field_bwd_fused per entry of
    ``forms`` = (head launches read the kept base rows?, form 1 | 2 | "jac": form 2 with the position gradient from the
    forward's Jacobian).  ``pos`` [R * S, 3] device positions (default: uniformly random inside and outside the unit box).
    Returns a namespace of everything written; ``res[(stored, form)]`` holds the gradients of one backward call."""
    from types import SimpleNamespace

    from thermo_nerf_amd import _hip

    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", S, R_hw=hw)
    lib = _hip.load()
    R = o.shape[0]
    N = R * S
    dd, cc = d.to(DEV), cam.to(DEV).reshape(-1).to(torch.int32)
    if pos is None:
        pos = (torch.rand(N, 3, generator=torch.Generator().manual_seed(5)) * 3 - 1.5).to(DEV)
    assert pos.shape == (N, 3) and pos.is_contiguous()
    fld = gm.field.c_struct(prepare=True, dense=False)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    st = _hip.current_stream()
    enc, sel, dens, h1, bo = f32(N, 32), f32(N), f32(N), f32(N, 64), f32(N, 16)
    c1, c2, rgb, t1, t2, th = f32(N, 64), f32(N, 64), f32(N, 3), f32(N, 64), f32(N, 64), f32(N, 1)
    _hip.check(lib.tn_field_fwd_taped(fld, pos.data_ptr(), dd.data_ptr(), cc.data_ptr(), R, S, enc.data_ptr(), sel.data_ptr(),
                                      h1.data_ptr(), bo.data_ptr(), dens.data_ptr(), c1.data_ptr(), c2.data_ptr(), rgb.data_ptr(),
                                      t1.data_ptr(), t2.data_ptr(), th.data_ptr(), st), "tn_field_fwd_taped")
    ray_bias = f32(R, 64)
    _hip.check(lib.tn_ray_head_fwd(fld, dd.data_ptr(), cc.data_ptr(), R, ray_bias.data_ptr(), st), "tn_ray_head_fwd")
    enc_t, sel_t, dens_t, rgb_t, th_t = f32((N + 63) // 64 * 64, 32), f32(N), f32(N), f32(N, 3), f32(N, 1)
    base = torch.full((N + 1, 16), 7.0, device=DEV)  # one guard row behind the last sample
    _hip.check(lib.tn_field_fwd_train(fld, pos.data_ptr(), ray_bias.data_ptr(), R, S, enc_t.data_ptr(), sel_t.data_ptr(),
                                      dens_t.data_ptr(), rgb_t.data_ptr(), th_t.data_ptr(), base.data_ptr(), None, st), "tn_field_fwd_train")
    torch.cuda.synchronize()
    # without the optional store
    rgb_n, th_n = f32(N, 3), f32(N, 1)
    _hip.check(lib.tn_field_fwd_train(fld, pos.data_ptr(), ray_bias.data_ptr(), R, S, enc_t.data_ptr(), sel_t.data_ptr(),
                                      dens_t.data_ptr(), rgb_n.data_ptr(), th_n.data_ptr(), None, None, st), "tn_field_fwd_train")
    # with the optional position Jacobian (config.store_position_jacobian), another instantiation of the kernel
    jac = torch.full(((N + 63) // 64 * 64 + 1, 96), 7.0, device=DEV)
    enc_j, base_j, rgb_j, th_j = torch.empty_like(enc_t), torch.empty_like(base), f32(N, 3), f32(N, 1)
    _hip.check(lib.tn_field_fwd_train(fld, pos.data_ptr(), ray_bias.data_ptr(), R, S, enc_j.data_ptr(), sel_t.data_ptr(),
                                      dens_t.data_ptr(), rgb_j.data_ptr(), th_j.data_ptr(), base_j.data_ptr(), jac.data_ptr(), st),
               "tn_field_fwd_train")
    torch.cuda.synchronize()

    g = torch.Generator().manual_seed(9)
    g_rgb, g_th, g_dens = (torch.randn(N, 3, generator=g) * 1e-3).to(DEV), (torch.randn(N, generator=g) * 1e-3).to(DEV), \
        (torch.randn(N, generator=g) * 1e-3).to(DEV)
    names = {"base0": "field.mlp_base.mlp.layers.0", "base1": "field.mlp_base.mlp.layers.1", "head0": "field.mlp_head.layers.0",
             "head1": "field.mlp_head.layers.1", "head2": "field.mlp_head.layers.2", "th0": "field.mlp_thermal.layers.0",
             "th1": "field.mlp_thermal.layers.1", "thead": "field.field_head_thermal.net"}
    ws = torch.empty(lib.tn_field_bwd_fused_workspace_bytes(R, S), dtype=torch.uint8, device=DEV)
    res = {}
    # form 2: the heads' 64 x 64 products as six bf16-piece products; "jac": the position gradient from the forward's Jacobian
    for stored, form in forms:
        from_jac, form = (form == "jac"), (2 if form == "jac" else form)
        grads = {n: torch.zeros_like(p) for n, p in gm.named_parameters()}
        gr = _hip.tn_field_grads()
        for k, nme in names.items():
            setattr(gr, k + "_w", grads[nme + ".weight"].data_ptr())
            if k != "head0":
                setattr(gr, k + "_b", grads[nme + ".bias"].data_ptr())
        g_enc, g_ray, g_pos = f32(N, 32), torch.zeros(R, 64, device=DEV), f32(N, 3)
        _hip.check(lib.tn_field_bwd_fused(fld, R, S, enc_t.data_ptr(), sel_t.data_ptr(), base.data_ptr() if stored else None,
                                          ray_bias.data_ptr(), rgb_t.data_ptr(), g_rgb.data_ptr(), g_th.data_ptr(), g_dens.data_ptr(),
                                          1, -15.0, form, g_enc.data_ptr(), g_ray.data_ptr(), pos.data_ptr(), jac.data_ptr() if from_jac else None, g_pos.data_ptr(),
                                          C.byref(gr), ws.data_ptr(), ws.numel(), st), "tn_field_bwd_fused")
        torch.cuda.synchronize()
        res[(stored, "jac" if from_jac else form)] = dict({nme + sfx: grads[nme + sfx] for nme in names.values() for sfx in (".weight", ".bias") if nme + sfx in grads},
                           g_enc=g_enc, g_ray=g_ray, g_pos=g_pos)
    return SimpleNamespace(gm=gm, fld=fld, R=R, S=S, N=N, pos=pos, bo=bo, base=base, sel=sel_t, rgb_t=rgb_t, th_t=th_t, rgb_n=rgb_n,
                           th_n=th_n, rgb_j=rgb_j, th_j=th_j, enc_t=enc_t, enc_j=enc_j, base_j=base_j, jac=jac, res=res)


@pytest.mark.parametrize("hw", [(12, 12), (7, 5), (1, 3)])  # 64-sample multiples, a ragged last tile, fewer samples than a tile
@pytest.mark.parametrize("S", [48, 192, 5])
def test_kept_base_output_equals_the_tape_and_the_recomputing_backward(S, hw):
    """config.backward_bf16_pieces (round 5): tn_field_bwd_fused's split form 2 — the heads' 64 x 64 products as six products of
    exact bf16 pieces — against form 1 (fp32 MFMA) on the same inputs, and
    config.store_base_output (round 5): tn_field_fwd_train's optional base_out [N,16] holds the rows tn_field_fwd_taped writes
    as `bo` (same MFMA chain: bit for bit), and tn_field_bwd_fused's head launches reading them give the gradients of the launches
    that recompute mlp_base from the hash features (fp32 summation order of mlp_base's products differs between the two).
    (The position gradient of these forms against an fp64 reference, sample by sample: tests/test_gpu_position_gradient.py.)"""
    f = field_train_forms(S, hw)
    N, bo, base, jac, res = f.N, f.bo, f.base, f.jac, f.res
    assert torch.equal(base[:N], bo) and bool((base[N] == 7.0).all())
    assert torch.equal(f.rgb_n, f.rgb_t) and torch.equal(f.th_n, f.th_t)  # the optional store changes nothing else
    # ... nor does the optional position Jacobian (config.store_position_jacobian), another instantiation of the kernel
    assert torch.equal(f.rgb_j, f.rgb_t) and torch.equal(f.th_j, f.th_t) and torch.equal(f.base_j[:N], bo) and bool((jac[-1] == 7.0).all())
    assert torch.equal(f.enc_j.view(-1, 16, 64, 2)[: N // 64], f.enc_t.view(-1, 16, 64, 2)[: N // 64])

    for k, want in res[(False, 1)].items():
        for other in ((True, 1), (True, 2), (True, "jac")):
            if want.norm().item() == 0.0:
                assert res[other][k].norm().item() == 0.0, k
                continue
            assert rel(res[other][k], want) <= 2e-5, f"{k} {other}: rel {rel(res[other][k], want):.2e}"
    # the bf16-piece products are fp32 products up to the rounding of a product: the two stored-base forms differ by summation order only
    assert any(not torch.equal(res[(True, 1)][k], res[(True, 2)][k]) for k in res[(True, 1)])  # (form 2 really is another kernel)
    assert not torch.equal(res[(True, 2)]["g_pos"], res[(True, "jac")]["g_pos"])  # (and so is the Jacobian's position gradient)
    # the position gradient sample by sample, not only in norm: positions inside and outside the unit box, every level
    a, b = res[(True, "jac")]["g_pos"], res[(False, 1)]["g_pos"]
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-12

    # the whole step with and without the kept rows
    got = {}
    for keep, pieces in ((True, True), (True, False), (False, False)):
        gm2, _, _, o2, d2, jit2, cam2, batch2 = _train_setup("scene", S, R_hw=hw, store_base_output=keep, backward_bf16_pieces=pieces,
                                                             store_position_jacobian=keep)
        assert gm2.config.store_base_output is keep and gm2.config.backward_bf16_pieces is pieces
        out, loss = _gpu_step(gm2, o2, d2, jit2, cam2, batch2)
        got[(keep, pieces)] = (out, loss, {n: p.grad.clone() for n, p in gm2.named_parameters() if p.grad is not None})
    want = got[(False, False)]
    for other in ((True, True), (True, False)):
        for k in ("rgb", "thermal", "accumulation"):
            assert torch.equal(got[other][0][k], want[0][k]), k
        assert set(got[other][2]) == set(want[2])
        for n, gw in want[2].items():
            if gw.norm().item() < 1e-10:
                continue
            assert rel(got[other][2][n], gw) <= 2e-5, f"{n} {other}: rel {rel(got[other][2][n], gw):.2e}"


def test_trunc_exp_backward_clamp():
    """NS activations.trunc_exp backward = g * exp(clamp(x, -15, 15)) (two-sided, from torch-ngp; SURVEY A.3 [UNSURE]) against
    the upper-clamp-only form, with a raw-density bias that puts the samples below -15, where the two differ: the raw-density
    row of mlp_base.1 (which only the density gradient reaches) of the product — tape-free and taped — against torch autograd
    over the oracle in the same setting."""
    rows = {}
    for clamp_min in (-15.0, float("-inf")):
        for tape_free in (True, False):
            gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48, trunc_exp_clamp_min=clamp_min, tape_free_training=tape_free)
            assert ocfg.trunc_exp_clamp_min == clamp_min
            sd = {k: v.clone() for k, v in sd.items()}
            with torch.no_grad():
                gm.field.mlp_base.mlp.layers[1].bias[0] -= 30.0
                sd["field.mlp_base.mlp.layers.1.bias"][0] -= 30.0
            _gpu_step(gm, o, d, jit, cam, batch)
            _, _, want = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
            named = dict(gm.named_parameters())
            gw, gb = named["field.mlp_base.mlp.layers.1.weight"].grad[0], named["field.mlp_base.mlp.layers.1.bias"].grad[0]
            ww, wb = want["field.mlp_base.mlp.layers.1.weight"][0], want["field.mlp_base.mlp.layers.1.bias"][0]
            assert ww.norm().item() > 0
            assert rel(gw, ww) <= 2e-3 and rel(gb, wb) <= 2e-3, (clamp_min, tape_free, rel(gw, ww), rel(gb, wb))
            assert rel(named["field.mlp_base.encoder.hash_table"].grad, want["field.mlp_base.encoder.hash_table"]) <= 2e-3
            rows[(clamp_min, tape_free)] = gw.detach().cpu()
    assert rel(rows[(-15.0, True)], rows[(float("-inf"), True)]) > 0.1, "the bias did not move the samples below the clamp"


def test_proposal_networks_frozen_between_updates():
    """NS ProposalNetworkSampler: off the update schedule the proposal densities are evaluated under no_grad."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48)
    gm.set_step(2000)          # update_sched(2000) = 2 > steps_since_update = 1, step >= 10 -> not updated
    assert gm.proposal_sampler._steps_since_update == 1
    _gpu_step(gm, o, d, jit, cam, batch)
    for n, p in gm.named_parameters():
        if n.startswith("proposal_networks"):
            assert p.grad is None or p.grad.abs().max().item() == 0.0, n
    assert gm.field.mlp_base.encoder.hash_table.grad.abs().max().item() > 0
    _, _, want = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit, anneal=gm.proposal_sampler._anneal,
                                  proposal_requires_grad=False)
    assert rel(gm.field.mlp_head.layers[1].weight.grad, want["field.mlp_head.layers.1.weight"]) <= 2e-3


def test_pass_thermal_gradients_false_detaches_geo():
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48)
    _gpu_step(gm, o, d, jit, cam, batch)
    g_on = gm.field.mlp_base.mlp.layers[1].weight.grad.clone()
    gm.field.pass_thermal_gradients = False  # REF thermal_field.py:171-172 detaches; REF model :319 drops the loss too
    _, ld = _gpu_step(gm, o, d, jit, cam, batch)
    assert "thermal" not in ld
    assert not torch.equal(g_on, gm.field.mlp_base.mlp.layers[1].weight.grad)
    assert gm.field.mlp_thermal.layers[0].weight.grad is None


def test_adam_steps_reduce_the_loss_and_eval_follows():
    """A few optimizer steps on one batch lower the loss; the eval path then renders with the UPDATED weights
    (prepared MFMA blobs are rebuilt when parameter versions change)."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("init", 48)
    batch = {"image": torch.full_like(batch["image"], 0.85), "thermal": torch.full_like(batch["thermal"], 0.2)}
    groups = gm.get_param_groups()
    opt = torch.optim.Adam([{"params": groups["fields"]}, {"params": groups["proposal_networks"]}], lr=1e-2, eps=1e-15)
    losses = []
    for step in range(20):
        gm.set_step(step)
        _, ld = _gpu_step(gm, o, d, jit, cam, batch)
        losses.append(sum(v.item() for v in ld.values()))
        opt.step()
    assert losses[-1] < 0.5 * losses[0], losses
    gm.eval()
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=torch.zeros_like(cam).to(DEV))
    with torch.no_grad():
        got = gm(rb)
    sd_new = {k: v.detach().cpu() for k, v in gm.state_dict().items()}
    # nerfstudio's sampler applies its current proposal-weight anneal in eval renders too: the oracle gets the
    # value set_step(19) left behind.  Stale weights would be off by ~0.1.
    want = H.get_outputs(sd_new, o, d, None, ocfg, anneal=float(gm.proposal_sampler._anneal))
    assert (got["rgb"].cpu() - want["rgb"]).abs().max().item() <= 2e-3
    assert (got["thermal"].cpu() - want["thermal"]).abs().max().item() <= 2e-3
    assert (got["rgb"].cpu() - want["rgb"]).abs().mean().item() <= 1e-4


def test_loss_curve_follows_the_autograd_oracle():
    """SURVEY §8f row 2 "loss-curve parity": the same 12 Adam steps (lr 1e-2, eps 1e-15, REF config_thermal_nerf.py:32-45) on
    the HIP step and on torch autograd over the CPU oracle — same rays, targets, jitter draws and anneal schedule — give the
    same loss at every step (1e-3 relative; fp32 rounding compounds over the steps) and parameters that stay together."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("init", 48, R_hw=(10, 10))
    batch = {"image": torch.full_like(batch["image"], 0.85), "thermal": torch.full_like(batch["thermal"], 0.2)}  # fittable
    steps = 12
    g = torch.Generator().manual_seed(21)
    R = o.shape[0]
    jits = [[torch.rand(R, 1, generator=g) for _ in range(3)] for _ in range(steps)]
    # --- oracle trajectory: plain torch Adam over the leaves of the state dict
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith((".aabb", ".scalings")) and not k.startswith("camera_optimizer")}
    frozen = {k: v for k, v in sd.items() if k not in leaves}
    opt_cpu = torch.optim.Adam(list(leaves.values()), lr=1e-2, eps=1e-15)
    want = []
    for i in range(steps):
        anneal = T.proposal_anneal(i)
        out = H.get_outputs({**frozen, **leaves}, o, d, cam, ocfg, training=True, jitter=jits[i], anneal=anneal,
                            proposal_requires_grad=True)  # steps < 10 and the warm-up schedule: the sampler updates every step
        loss = sum(T.get_loss_dict(out, batch, T.get_metrics_dict(out, batch, True), True).values())
        opt_cpu.zero_grad(set_to_none=True)
        loss.backward()
        opt_cpu.step()
        want.append(loss.item())
    # --- the HIP step
    params = [p for n, p in gm.named_parameters() if not n.startswith("camera_optimizer")]
    opt = torch.optim.Adam(params, lr=1e-2, eps=1e-15, fused=True)
    b = {k: v.to(DEV) for k, v in batch.items()}
    got = []
    for i in range(steps):
        gm.set_step(i)
        assert abs(gm.proposal_sampler._anneal - T.proposal_anneal(i)) < 1e-7
        rb = gm.collider(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
        out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jits[i], dim=1).T.contiguous().to(DEV))
        loss = sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        got.append(loss.item())
    assert want[-1] < want[0]  # it is a descent, not a flat line
    for i, (a, w) in enumerate(zip(got, want)):
        assert abs(a - w) <= 1e-3 * abs(w), (i, a, w)
    named = dict(gm.named_parameters())
    # parameters: Adam with eps 1e-15 moves an entry by ~lr whatever the size of its gradient, so table entries whose gradient
    # is rounding noise (1e-12) step in a direction the two implementations need not share; the MLP weights (dense gradients)
    # must agree closely, the tables in the large
    drift = {name: rel(named[name], leaves[name]) for name in leaves}
    for name, v in drift.items():
        if name.startswith("proposal_networks"):
            continue  # driven by the interlevel loss alone, which is ~0 here: their gradients are rounding noise throughout
        assert v <= (0.25 if name.endswith("hash_table") else 5e-2), (name, v)


def test_bucketed_table_scatter_in_the_training_step():
    """config.bucketed_table_scatter (on by default) on the reference's full-size field grid: levels 8-15 (scaling >= 200,
    7 x 32 table slices) go through the bucketed records, levels 0-8 and the proposal grids (40 bins) keep the atomic scatter;
    the step's gradients equal those of the all-atomic step."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 48, small=False)
    assert gm.config.bucketed_table_scatter is True
    fld = gm.field.c_struct(prepare=False, dense=False)
    assert _hip.load().tn_hash_encode_bwd_sorted_first_level(fld.grid, o.shape[0] * 48) == 8
    assert _hip.load().tn_hash_encode_bwd_sorted_first_level(gm.proposal_networks[0].c_struct(dense=False).grid, 4096 * 256) == -1
    _gpu_step(gm, o, d, jit, cam, batch)
    got = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
    gm.config.bucketed_table_scatter = False
    _gpu_step(gm, o, d, jit, cam, batch)
    want = {n: p.grad for n, p in gm.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    name = "field.mlp_base.encoder.hash_table"
    assert float(want[name].abs().sum()) > 0 and rel(got[name], want[name]) <= 1e-5
    assert torch.equal(got[name] == 0, want[name] == 0)
    for n in want:
        if n != name:
            assert rel(got[n], want[n]) <= 1e-5, n  # (atomic orders differ from run to run)


@pytest.mark.parametrize("update_step", [True, False])
def test_step_streams_do_not_change_the_step(update_step):
    """config.overlap_table_scatter: the bucketed half of the field's table scatter on the step's second stream, the proposal
    levels' backward of an update step on its third (own ray-gradient buffers, added at the join) — against the same step queued
    on one stream, on the full-size grids with ray gradients asked for (what the camera optimizer backpropagates, from all three
    levels): same parameter and ray gradients up to the order of the atomics, same table entries touched."""
    got = {}
    for overlap in (True, False):
        gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 48, small=False, overlap_table_scatter=overlap)
        assert gm.config.overlap_table_scatter is overlap
        if not update_step:
            gm.set_step(5000)  # past the warm-up: the sampler skips the proposal networks' update on this step
        b = {k: v.to(DEV) for k, v in batch.items()}
        for _ in range(2):  # twice: the second step reuses the streams, workspaces and cached structs of the first
            gm.proposal_sampler._steps_since_update = 0
            od, dd = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
            rb = gm.collider(RayBundle(origins=od, directions=dd, camera_indices=cam.to(DEV)))
            out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
            gm.zero_grad(set_to_none=True)
            sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values()).backward()
        assert out["weights_list"][0].requires_grad is update_step
        torch.cuda.synchronize()
        got[overlap] = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
        got[overlap]["__origins__"], got[overlap]["__directions__"] = od.grad.clone(), dd.grad.clone()
    on, off = got[True], got[False]
    assert set(on) == set(off)
    assert ("proposal_networks.0.mlp_base.encoder.hash_table" in on) is update_step
    assert float(off["__origins__"].abs().sum()) > 0 and float(off["__directions__"].abs().sum()) > 0
    for n, g in off.items():
        assert rel(on[n], g) <= (1e-4 if n.startswith("__") else 1e-5), (n, rel(on[n], g))
        if n.endswith("hash_table"):
            assert torch.equal(on[n] == 0, g == 0), n


def test_bucketed_proposal_grid_on_the_third_stream():
    """A proposal grid large enough for the bucketed scatter (2^21 entries per level, max_res 256: level 4 = 128 table slices;
    the reference's 2^17-entry grids never qualify) on an update step: its backward is queued on the step's third stream, where
    the record workspace is a main-stream allocation that must outlive the call (it is handed to the caller's
    ``keep`` list until the join).  Same gradients as the one-stream step, same table entries touched."""
    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic

    nets = [{"hidden_dim": 16, "log2_hashmap_size": 21, "num_levels": 5, "max_res": 128, "use_linear": False},
            {"hidden_dim": 16, "log2_hashmap_size": 21, "num_levels": 5, "max_res": 256, "use_linear": False}]
    o, d = helpers.rays(16, 16, view=3)
    R = o.shape[0]
    g = torch.Generator().manual_seed(3)
    jit = [torch.rand(R, 1, generator=g) for _ in range(3)]
    cam = torch.randint(0, 8, (R, 1), generator=g)
    batch = {"image": torch.rand(R, 3, generator=g), "thermal": torch.rand(R, 1, generator=g)}
    got = {}
    for overlap in (True, False):
        cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=48, log2_hashmap_size=15, proposal_net_args_list=[dict(a) for a in nets],
                                     camera_optimizer_mode="off", overlap_table_scatter=overlap)
        gm = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=8)
        synthetic.fill_model_(gm, "scene")
        gm = gm.to(DEV).train()
        lib = _hip.load()
        assert lib.tn_hash_encode_bwd_sorted_first_level(gm.proposal_networks[1].c_struct(dense=False).grid, R * 96) == 4
        assert lib.tn_hash_encode_bwd_sorted_first_level(gm.proposal_networks[0].c_struct(dense=False).grid, R * 256) == -1
        for _ in range(2):
            gm.proposal_sampler._steps_since_update = 0
            out, _ = _gpu_step(gm, o, d, jit, cam, batch)
        assert out["weights_list"][1].requires_grad
        torch.cuda.synchronize()
        got[overlap] = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
        del gm
        torch.cuda.empty_cache()
    on, off = got[True], got[False]
    assert set(on) == set(off) and "proposal_networks.1.mlp_base.encoder.hash_table" in on
    for n, gr in off.items():
        assert rel(on[n], gr) <= 1e-5, (n, rel(on[n], gr))
        if n.endswith("hash_table"):
            assert float(gr.abs().sum()) > 0 and torch.equal(on[n] == 0, gr == 0), n


def test_config1_one_thousand_iterations_follow_the_cpu_reference_path(golden_dir):
    """BASELINE config 1 / SURVEY §8f row 2 "loss-curve parity over 1 k its on the analytic scene": the 1000 Adam steps of the
    CPU reference path (torch autograd over the oracle; tests/test_config1_cpu.py runs them live, tools/make_config1_golden.py
    recorded them in tests/golden/config1_oracle.npz — the GPU box's shared host cores can be 40x slower under load) and the
    same 1000 steps on the HIP path: same batches, jitter draws, anneal and proposal-update schedule.

    A 1000-step Adam run at eps = 1e-15 on 64-ray batches is a chaotic system: two valid fp32 runs of the CPU path agree step for
    step over the first tens of steps, to 2-9 % in the 100-step means of windows 2-3, and then wander — the fixture's NINE CPU runs
    (1 / 2 / 4 / 8 intra-op threads, five orders of the batches' rays) spread by 1.4x in windows 4-6 and by up to 5x in the plateau
    behind them, with bumps at other steps in every run; a float64 run of the same optimisation is recorded beside them.  One HIP
    run cannot be told from a biased step in that noise, so the test runs the HIP path SEVEN times (1.6 s each) and asks:
      * every run: step for step over the first 20 steps (2e-3 relative); windows 1-4 inside the CPU set's [min, max] x 1.25; a
        monotone descent over windows 1-5; windows 5-10 inside the band the CPU set's plateau covers (x 1.5) and below window 2;
      * the MEDIAN over the seven runs of each window 1-6 inside the CPU set's [min, max] x 1.10 — a systematic bias of the step moves
        the median, a bump moves one run;
      * while the trajectories still agree (windows 1-3) the HIP median is no further from the float64 run than the furthest CPU run
        x 1.5 (measured: fp32 runs of either path descend 0.3-2 % faster than float64 in window 2 — 0.01163 against 0.01136-0.01160
        CPU and 0.01133-0.01156 HIP);
      * the same final quality on held-out pixels (1.5 dB, 0.03 of the normalised thermal range, both improving on the initial
        thermal MAE by 2.5x) and the HIP eval render of the HIP-trained weights against the oracle on those weights."""
    import os

    import numpy as np

    prob = helpers.config1_problem()
    steps = helpers.CONFIG1["steps"]
    gold = np.load(os.path.join(golden_dir, "config1_oracle.npz"))
    want, p_cpu, m_cpu = gold["losses"], float(gold["psnr"]), float(gold["mae"])
    assert want.shape == (steps,)
    ws = gold["losses_set"].reshape(-1, 10, 100).mean(axis=2)
    assert ws.shape[0] >= 9
    lo, hi = ws.min(axis=0), ws.max(axis=0)
    w64 = gold["losses_fp64"].reshape(10, 100).mean(axis=1)
    plateau_lo, plateau_hi = ws[:, 4:].min() / 1.5, ws[:, 4:].max() * 1.5
    o, d, cam = prob["o"].to(DEV), prob["d"].to(DEV), prob["cam"].to(DEV)
    img, th, idx = prob["image"].to(DEV), prob["thermal"].to(DEV), prob["idx"].to(DEV)
    jitter = prob["jitter"].squeeze(-1).to(DEV)
    upd = helpers.proposal_updates(steps)
    windows, gm = [], None
    for run in range(7):
        gm = copy.deepcopy(prob["model"]).to(DEV)
        gm.train()
        params = [p for n, p in gm.named_parameters() if not n.startswith("camera_optimizer")]
        opt = torch.optim.Adam(params, lr=1e-2, eps=1e-15, fused=True)
        got = []
        for i in range(steps):
            gm.set_step(i)
            ix = idx[i]
            rb = gm.collider(RayBundle(origins=o[ix], directions=d[ix], camera_indices=cam[ix]))
            out = TR.get_outputs_train(gm, rb, jitter=jitter[i].contiguous())
            assert (gm.proposal_sampler._steps_since_update == 0) == upd[i], i  # same update steps as the CPU run
            b = {"image": img[ix], "thermal": th[ix]}
            loss = sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            got.append(loss.detach())
        got = torch.stack(got).cpu().numpy()
        assert np.isfinite(got).all()
        for i in range(20):
            assert abs(got[i] - want[i]) <= 2e-3 * abs(want[i]), (run, i, got[i], want[i])
        gw = got.reshape(10, 100).mean(axis=1)
        # the first 100 steps: every valid run — nine CPU, 400 HIP — has the same mean to 2e-4.  (Before round 6's fix of the gradient
        # arena's clear, which could overtake an earlier step's optimizer on a small problem, 1 run in 60 sat 2-25 % above it.)
        assert abs(gw[0] - lo[0]) <= 1e-3 * lo[0], (run, gw[0], lo[0])
        assert (gw[:4] <= 1.25 * hi[:4]).all() and (gw[:4] >= lo[:4] / 1.25).all(), (run, gw, lo, hi)
        assert (np.diff(gw[:5]) < 0).all(), (run, gw)
        assert (gw[4:] <= plateau_hi).all() and (gw[4:] >= plateau_lo).all() and (gw[4:] < gw[1]).all(), (run, gw, plateau_lo, plateau_hi)
        windows.append(gw)
        if run >= 2:
            continue
        # final quality on the held-out pixels of a training view (helpers.config1_problem says why a held-out VIEW checks nothing at this
        # size; novel-view quality is config 3's held-out PSNR / MAE in bench.py), both through the oracle's eval render: the HIP-trained weights
        # go back to the CPU
        sd_hip = {**prob["sd"], **{k: v.detach().cpu() for k, v in gm.state_dict().items() if k in prob["sd"]}}
        p_hip, m_hip, hit_hip = helpers.held_out_quality(prob, sd_hip)
        # held-out pixels of a training view (helpers.config1_problem): the CPU runs end at 15.7 ... 16.8 dB, thermal MAE 0.018 ... 0.044
        # from 12.8 dB / 0.255 / 0.227 (quality_set in the fixture); the late stage of a 64-ray-batch run wanders, hence bands
        # (twelve HIP runs, tools/config1_spread.py: psnr 15.7 ... 17.0 dB, thermal MAE 0.017 ... 0.054, on the sphere's rays 0.015 ... 0.070)
        assert p_hip >= p_cpu - 1.5, (p_cpu, p_hip)
        assert m_hip <= m_cpu + 0.03 and hit_hip <= float(gold["mae_hit"]) + 0.04, (m_cpu, m_hip, hit_hip)
        assert m_hip < 0.4 * float(gold["mae_initial"]) and hit_hip < 0.4 * float(gold["mae_hit_initial"])
    med = np.median(np.stack(windows), axis=0)
    assert (med[:6] <= 1.10 * hi[:6]).all() and (med[:6] >= lo[:6] / 1.10).all(), (med, lo, hi)
    far = np.abs(ws[:, :3] - w64[:3]).max(axis=0)
    assert (np.abs(med[:3] - w64[:3]) <= 1.5 * far + 1e-6).all(), (med[:3], w64[:3], far)
    # and the HIP eval render of the (last) HIP-trained model agrees with the oracle on the same weights (eval after 1000 fused steps)
    sd_hip = {**prob["sd"], **{k: v.detach().cpu() for k, v in gm.state_dict().items() if k in prob["sd"]}}
    gm.eval()
    h = prob["held_out"]
    with torch.no_grad():
        out = gm(RayBundle(origins=h["o"].to(DEV), directions=h["d"].to(DEV)))
    # (nerfstudio's sampler applies its current proposal-weight anneal in eval renders too: 0.9999 after set_step(999))
    ref = H.get_outputs(sd_hip, h["o"], h["d"], None, prob["ocfg"], anneal=float(gm.proposal_sampler._anneal))
    assert (out["rgb"].cpu() - ref["rgb"]).abs().mean() <= 1e-4
    assert (out["thermal"].cpu() - ref["thermal"]).abs().mean() <= 1e-4


def test_config1_at_its_stated_step_size_follows_the_cpu_path_step_for_step(golden_dir):
    """BASELINE config 1 at the step size it states [BASELINE.md §5; REF config_thermal_nerf.py:27]: 4096 rays per step, P = (256, 96),
    S = 48, full-size tables — 30 Adam steps from nerfstudio's initialisation on the HIP path against the same 30 on the CPU
    reference path (recorded by tools/make_config1_golden.py --batch4096: same batches, jitter, anneal, update schedule).  A
    4096-ray mean is smooth enough that the two trajectories stay together while rounding differences grow step by step (measured:
    exactly equal or 1e-7 over the first ten steps, 3e-5 at step 10, 3e-4 at step 20, 7e-4 ... 8e-3 at steps 28-29 over three runs — the
    table scatter's atomics make the HIP run itself vary in the last digit, and Adam at eps = 1e-15 amplifies it step by step): every
    loss of the first 20 steps within 1e-3 relative, the last ten within 2e-2."""
    import os

    import numpy as np

    prob = helpers.config1_problem(helpers.CONFIG1_FULL)
    gold = np.load(os.path.join(golden_dir, "config1_batch4096.npz"))
    want = gold["losses"]
    steps = helpers.CONFIG1_FULL["steps"]
    assert want.shape == (steps,) and int(gold["rays_per_batch"]) == 4096 and tuple(gold["proposal"]) == (256, 96) and int(gold["S"]) == 48
    gm = copy.deepcopy(prob["model"]).to(DEV)
    gm.train()
    assert gm.field.mlp_base.encoder.hash_table.shape[0] == 16 << 19
    params = [p for n, p in gm.named_parameters() if not n.startswith("camera_optimizer")]
    opt = torch.optim.Adam(params, lr=1e-2, eps=1e-15, fused=True)
    o, d, cam = prob["o"].to(DEV), prob["d"].to(DEV), prob["cam"].to(DEV)
    img, th, idx = prob["image"].to(DEV), prob["thermal"].to(DEV), prob["idx"].to(DEV)
    jitter = prob["jitter"].squeeze(-1).to(DEV)
    upd = helpers.proposal_updates(steps)
    got = []
    for i in range(steps):
        gm.set_step(i)
        ix = idx[i]
        rb = gm.collider(RayBundle(origins=o[ix], directions=d[ix], camera_indices=cam[ix]))
        out = TR.get_outputs_train(gm, rb, jitter=jitter[i].contiguous())
        assert (gm.proposal_sampler._steps_since_update == 0) == upd[i], i
        b = {"image": img[ix], "thermal": th[ix]}
        loss = sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        got.append(loss.detach())
    got = torch.stack(got).cpu().numpy()
    worst = np.abs(got - want) / np.abs(want)
    print("relative loss difference per step:", " ".join(f"{x:.1e}" for x in worst))
    assert np.isfinite(got).all() and worst[:20].max() <= 1e-3 and worst.max() <= 2e-2, (worst.argmax(), worst.max(), got, want)
    assert got[-1] < 0.5 * got[0]  # and it descends


@pytest.mark.parametrize("sh_grad", [False, True])
@pytest.mark.parametrize("kind,contraction", [("stress", True), ("scene", True), ("stress", False)])
def test_ray_gradients_match_autograd_oracle(kind, contraction, sh_grad):
    """d loss / d (origins, directions) — what a camera optimizer backpropagates — through the sample positions of all
    three levels (trilinear offsets, selector, contraction / AABB) and, with sh_direction_gradient=True, the SH basis
    (default False: nerfstudio's torch-fallback SHEncoding.pytorch_fwd runs under no_grad)."""
    over = {} if contraction else {"disable_scene_contraction": True}
    over["sh_direction_gradient"] = sh_grad
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup(kind, 48, **over)
    if not contraction:
        o = o * 0.6
    od, dd = o.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    rb = gm.collider(RayBundle(origins=od, directions=dd, camera_indices=cam.to(DEV)))
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    b = {k: v.to(DEV) for k, v in batch.items()}
    sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values()).backward()
    _, _, want = T.loss_and_grads(sd, o, d, cam, batch, ocfg, jit)
    # the position gradient is a sum over 16 levels of (feature differences x level scale up to 2047): the fine levels
    # dominate and cancel.  Yardstick: the fp32 oracle itself is 3e-3 .. 1e-2 away from its fp64 run on these cases.
    # (The tight check, kernel by kernel and sample by sample against a cell-exact fp64 reference, at a counted number of
    # roundings: tests/test_gpu_position_gradient.py.)
    assert rel(od.grad, want["__origins__"]) <= 2e-2, rel(od.grad, want["__origins__"])
    assert rel(dd.grad, want["__directions__"]) <= 2e-2, rel(dd.grad, want["__directions__"])
    # and the parameter gradients are unchanged by asking for ray gradients
    assert rel(gm.field.mlp_head.layers[0].weight.grad, want["field.mlp_head.layers.0.weight"]) <= 2e-3


@pytest.mark.parametrize("scale", [0.0, 0.004, 0.02, 0.5])  # |w|^2 below / around / above the 1e-4 clamp; large angles
@pytest.mark.parametrize("n,cams", [(1000, 8), (64, 1), (4097, 200), (1, 3)])
def test_camera_opt_apply_and_its_adjoint(n, cams, scale):
    """tn_camera_opt_fwd / tn_camera_opt_bwd against torch autograd over the oracle's restatement of NS exp_map_SO3xR3 +
    CameraOptimizer.apply_to_raybundle [REF thermal_nerf_model.py:218-219]."""
    from thermo_nerf_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig

    g = torch.Generator().manual_seed(n + cams)
    pose = scale * torch.randn(cams, 6, generator=g)
    pose[0, 3:] = 0.0  # an untouched camera: theta sits on the clamp
    o = torch.randn(n, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    cam = torch.randint(0, cams, (n, 1), generator=g)
    go, gd = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    pose_cpu, d_cpu = pose.clone().requires_grad_(True), d.clone().requires_grad_(True)
    wo, wd = T.apply_pose_adjustment(pose_cpu, cam, o, d_cpu)
    ((wo * go).sum() + (wd * gd).sum()).backward()

    copt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), cams, device=DEV)
    with torch.no_grad():
        copt.pose_adjustment.copy_(pose.to(DEV))
    d_dev = d.to(DEV).requires_grad_(True)
    rb = RayBundle(origins=o.to(DEV), directions=d_dev, camera_indices=cam.to(DEV))
    copt.apply_to_raybundle(rb)
    assert (rb.origins.detach().cpu() - wo.detach()).abs().max().item() <= 1e-6
    assert (rb.directions.detach().cpu() - wd.detach()).abs().max().item() <= 2e-6
    ((rb.origins * go.to(DEV)).sum() + (rb.directions * gd.to(DEV)).sum()).backward()
    assert rel(copt.pose_adjustment.grad, pose_cpu.grad) <= 2e-5, rel(copt.pose_adjustment.grad, pose_cpu.grad)
    assert rel(d_dev.grad, d_cpu.grad) <= 2e-6
    # the [N,3,4] matrices of forward(indices) are the same map
    m = copt(cam.reshape(-1).to(DEV)).detach().cpu()
    assert (m - T.exp_map_SO3xR3(pose[cam.reshape(-1)])).abs().max().item() <= 1e-6


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_camera_optimizer_receives_the_pose_gradient(mode):
    """camera_optimizer_mode [REF nerfacto_config/thermal_nerfacto.py:24: "off" | "SO3xR3" (the default) | "SE3"]:
    pose_adjustment gets its gradient through apply_to_raybundle from the HIP ray gradients (SE3: exp_map_SE3's translation
    V(w) u on the camera table, then the same per-ray kernels)."""
    cm, sd, ocfg = helpers.build("stress", 48, camera_optimizer_mode=mode)
    assert cm.config.camera_optimizer.mode == mode
    gm = copy.deepcopy(cm).to(DEV).train()
    o, d = helpers.rays(12, 12, view=3)
    R = o.shape[0]
    g = torch.Generator().manual_seed(5)
    cam = torch.randint(0, 8, (R, 1), generator=g)
    batch = {"image": torch.rand(R, 3, generator=g), "thermal": torch.rand(R, 1, generator=g)}
    pose = 0.02 * torch.randn(8, 6, generator=g)
    pose[3, 3:] *= 30.0  # one camera with a large rotation: the closed forms, not their small-angle limits
    pose[5, 3:] = 0.0    # and one inside the theta^2 clamp
    with torch.no_grad():
        gm.camera_optimizer.pose_adjustment.copy_(pose)
    jit = [torch.rand(R, 1, generator=g) for _ in range(3)]
    # the model draws its own jitter inside forward: fix it by seeding the device generator the same way twice
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV))
    rb = gm.collider(rb)
    gm.camera_optimizer.apply_to_raybundle(rb)
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    b = {k: v.to(DEV) for k, v in batch.items()}
    gm.zero_grad(set_to_none=True)
    sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values()).backward()
    got = gm.camera_optimizer.pose_adjustment.grad
    assert got is not None and torch.isfinite(got).all() and got.abs().max().item() > 0

    # expected: the same chain on the CPU — the oracle's camera optimizer in front of the autograd oracle
    pose_cpu = pose.clone().requires_grad_(True)
    o_adj, d_adj = T.apply_pose_adjustment(pose_cpu, cam, o, d, mode=mode)
    assert (rb.origins.detach().cpu() - o_adj.detach()).abs().max().item() <= 1e-6
    assert (rb.directions.detach().cpu() - d_adj.detach()).abs().max().item() <= 1e-6
    _, _, want = T.loss_and_grads(sd, o_adj.detach(), d_adj.detach(), cam, batch, ocfg, jit)
    ((o_adj * want["__origins__"]).sum() + (d_adj * want["__directions__"]).sum()).backward()
    assert rel(got, pose_cpu.grad) <= 2e-2, rel(got, pose_cpu.grad)
    # CameraOptimizer.forward: the [N,3,4] correction matrices of the mode
    idx = torch.tensor([3, 5, 0])
    want_m = (T.exp_map_SE3 if mode == "SE3" else T.exp_map_SO3xR3)(pose[idx])
    assert (gm.camera_optimizer(idx.to(DEV)).detach().cpu() - want_m).abs().max().item() <= 1e-6
    # used cameras only
    used = torch.zeros(8, dtype=torch.bool)
    used[cam.reshape(-1)] = True
    assert torch.all(got.cpu()[~used] == 0)


# --------------------------------------------------------------------------------------------------
# the loop: fit a closed-form RGB + thermal scene, check HELD-OUT views; checkpoint round trip
# --------------------------------------------------------------------------------------------------
def test_trainer_fits_analytic_scene_and_resumes(tmp_path):
    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic
    from thermo_nerf_amd.cameras import psnr
    from thermo_nerf_amd.trainer import RayDataset, Trainer, TrainerConfig, render_view

    res, n_views = 64, 72
    views = list(range(n_views))
    train_cams = synthetic.orbit_cameras(res, res, views, num_views=n_views,
                                         elevation_deg=[(-10.0, 20.0, 50.0)[v % 3] for v in views])
    test_cams = synthetic.orbit_cameras(res, res, [0.5, n_views / 2 + 0.5], num_views=n_views, elevation_deg=[5.0, 35.0])

    def truth(cams, i):
        rb = cams.generate_rays(i, device=DEV)
        return synthetic.analytic_scene(rb.origins, rb.directions)

    imgs, ths = zip(*[truth(train_cams, i) for i in range(n_views)])
    held_out = [truth(test_cams, i) for i in range(2)]
    ds = RayDataset.from_images(train_cams, imgs, ths, DEV)
    assert len(ds) == n_views * res * res

    def fresh():
        cfg = ThermalNerfModelConfig(camera_optimizer_mode="off", eval_num_rays_per_chunk=1 << 16, **helpers.SMALL)
        m = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=n_views)
        synthetic.fill_model_(m, "init")
        return m.to(DEV)

    def evaluate(m):
        ps, ma = [], []
        for i in range(2):
            o = render_view(m, test_cams, i, DEV)
            ps.append(psnr(o["rgb"], held_out[i][0]).item())
            ma.append((o["thermal"] - held_out[i][1]).abs().mean().item())
        return sum(ps) / 2, sum(ma) / 2

    model = fresh()
    tr = Trainer(model, ds, TrainerConfig(train_num_rays_per_batch=4096, steps_per_save=125))
    p0, m0 = evaluate(model)
    tr.train(250, checkpoint_dir=tmp_path)
    p1, m1 = evaluate(model)
    # measured on MI355X at 64x64: 12.5 dB / 0.26 before, ~20 dB / ~0.03 after 200-300 steps (the early PSNR wobbles by
    # a few dB from step to step: per-camera appearance codes are swapped for their mean at eval)
    print(f"held-out psnr {p0:.2f} -> {p1:.2f} dB, thermal mae {m0:.4f} -> {m1:.4f}")
    assert p1 >= p0 + 2.0, (p0, p1)
    assert m1 <= 0.12 and m1 <= 0.5 * m0, (m0, m1)
    assert sorted(p.name for p in tmp_path.glob("*.ckpt")) == ["step-000000125.ckpt", "step-000000250.ckpt"]

    # matched quality: the CPU oracle renders the TRAINED weights to the same PSNR / thermal MAE as the HIP path
    # (BASELINE: "at matched RGB PSNR and thermal MAE")
    rb = test_cams.generate_rays(0, device=DEV, flat=True)
    sd_trained = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = helpers.oracle_config(model.config)
    want = H.get_outputs(sd_trained, rb.origins.cpu(), rb.directions.cpu(), None, ocfg, anneal=model.proposal_sampler._anneal)
    got = render_view(model, test_cams, 0, DEV)
    gt_rgb, gt_th = held_out[0][0].reshape(-1, 3).cpu(), held_out[0][1].reshape(-1, 1).cpu()
    psnr_cpu, psnr_gpu = psnr(want["rgb"], gt_rgb).item(), psnr(got["rgb"].reshape(-1, 3).cpu(), gt_rgb).item()
    mae_cpu = (want["thermal"] - gt_th).abs().mean().item()
    mae_gpu = (got["thermal"].reshape(-1, 1).cpu() - gt_th).abs().mean().item()
    print(f"held-out view 0: psnr cpu {psnr_cpu:.3f} / gpu {psnr_gpu:.3f} dB, thermal mae cpu {mae_cpu:.5f} / gpu {mae_gpu:.5f}")
    assert abs(psnr_cpu - psnr_gpu) <= 0.05 and abs(mae_cpu - mae_gpu) <= 5e-4

    # resume into a fresh model/trainer: same step, same weights, same optimizer moments, same learning rate
    other = fresh()
    tr2 = Trainer(other, ds, TrainerConfig(train_num_rays_per_batch=4096))
    assert tr2.load_checkpoint(tmp_path) == 250
    for (k, a), (_, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    s1 = tr.optimizers["fields"].state_dict()["state"]
    s2 = tr2.optimizers["fields"].state_dict()["state"]
    assert s1.keys() == s2.keys()
    for k in s1:
        assert torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"].to(s1[k]["exp_avg"].device))
    assert abs(tr.optimizers["fields"].param_groups[0]["lr"] - tr2.optimizers["fields"].param_groups[0]["lr"]) < 1e-12
    # the proposal-weight anneal is callback state (set from the step by set_step), not checkpoint content
    other.proposal_sampler.set_anneal(model.proposal_sampler._anneal)
    p2, m2 = evaluate(other)
    assert abs(p2 - p1) < 1e-3 and abs(m2 - m1) < 1e-5


def test_config3_step_size_fresh_batches_against_the_atomic_single_stream_taped_step():
    """BASELINE config 3 at its REAL step size [REF config_thermal_nerf.py:17-48]: 4096 rays x S=192 x the full-size tables
    (2^19-entry field grid), SO3xR3 camera optimizer, a FRESH batch of random pixels of the analytic scene per step through
    trainer.Trainer.  At this size every default-on mechanism of the step is live together — tape-free field, bucketed scatter
    with 786 k x 8 records, spread copies of the coarse levels, three streams, regularisers launched by the forward — so the
    gradients of step 0 and of the step after 50 consecutive Trainer iterations are checked against the plain form of the same
    step: taped forward + chained backward, global atomics on every level, one stream, regularisers on demand."""
    from thermo_nerf_amd import synthetic
    from thermo_nerf_amd.trainer import RayDataset, Trainer, TrainerConfig

    S, R, V, res = 192, 4096, 12, 160
    cm, _, _ = helpers.build("init", S, small=False, num_images=V, camera_optimizer_mode="SO3xR3")
    views = list(range(V))
    cams = synthetic.orbit_cameras(res, res, views, num_views=V, elevation_deg=[(-10.0, 20.0, 50.0)[v % 3] for v in views])
    imgs, ths = [], []
    for i in range(V):
        rb = cams.generate_rays(i, device=DEV)
        im, th = synthetic.analytic_scene(rb.origins, rb.directions)
        imgs.append(im)
        ths.append(th)
    ds = RayDataset.from_images(cams, imgs, ths, DEV)
    model = copy.deepcopy(cm).to(DEV)
    cfg = model.config
    assert cfg.tape_free_training and cfg.bucketed_table_scatter and cfg.spread_coarse_scatter and cfg.overlap_table_scatter
    assert cfg.overlap_regularisers == "auto" and R * S >= 4096 * 96  # "auto" switches the side-stream regularisers on here
    plain = copy.deepcopy(cm)
    for k, v in dict(tape_free_training=False, bucketed_table_scatter=False, spread_coarse_scatter=False,
                     overlap_table_scatter=False, overlap_regularisers=False).items():
        setattr(plain.config, k, v)
    plain = plain.to(DEV)
    tr = Trainer(model, ds, TrainerConfig(train_num_rays_per_batch=R))

    def step_grads(m, step, rb, batch, sampler_state):
        m.train()
        m.set_step(step)
        m.proposal_sampler._steps_since_update = sampler_state
        torch.manual_seed(1234 + step)  # the jitter draw of get_outputs_train
        out = m(RayBundle(origins=rb.origins.clone(), directions=rb.directions.clone(), camera_indices=rb.camera_indices))
        loss = m.get_loss_dict(out, batch, m.get_metrics_dict(out, batch))
        m.zero_grad(set_to_none=True)
        sum(loss.values()).backward()
        torch.cuda.synchronize()
        return ({k: v.item() for k, v in loss.items()}, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None},
                out["weights_list"][0].requires_grad)

    def compare(step):
        plain.load_state_dict(model.state_dict())
        rb, batch = ds.sample(R, tr.generator)
        state = model.proposal_sampler._steps_since_update + 1  # what the sampler's step callback makes of it, for both models
        l1, g1, upd1 = step_grads(model, step, rb, batch, state)
        l0, g0, upd0 = step_grads(plain, step, rb, batch, state)
        assert upd1 == upd0
        for k in l0:
            assert abs(l1[k] - l0[k]) <= 2e-5 * abs(l0[k]) + 1e-9, (step, k, l1[k], l0[k])
        assert set(g1) == set(g0)
        assert "camera_optimizer.pose_adjustment" in g0 and "field.mlp_base.encoder.hash_table" in g0
        worst = {}
        for n, g in g0.items():
            if g.norm().item() < 1e-10:
                assert g1[n].norm().item() < 1e-9, n
                continue
            worst[n] = rel(g1[n], g)
            if n.endswith("hash_table"):
                # the same table entries touched.  (Up to a handful of entries whose contributions cancel to exactly 0 in one
                # summation order and to a denormal-sized rest in the other: 786 k samples x 8 corners meet in few coarse entries.)
                differ = (g1[n] == 0) != (g == 0)
                assert int(differ.sum()) <= max(64, int((g != 0).sum()) // 1000), (n, int(differ.sum()))
                if differ.any():
                    # such a rest is a rounding residue of its own level's sums, so it is held to one fp32 epsilon of that level's
                    # largest entry (the coarse levels carry the table's largest gradients, up to 2.5e-4 after 50 steps; measured
                    # at step 0: denormals and at most 1.2e-16 in a level whose largest entry is 1.1e-7)
                    T = model.field.mlp_base.encoder.hash_table_size
                    both = torch.maximum(g1[n].abs(), g.abs())
                    level_max = both.view(-1, T, both.shape[-1]).amax(dim=(1, 2))
                    level = differ.nonzero()[:, 0] // T
                    over = both[differ] > torch.finfo(torch.float32).eps * level_max[level]
                    assert not bool(over.any()), (n, both[differ][over].tolist(), level[over].tolist(), level_max.tolist())
        print(f"step {step}: worst relative gradient difference " + ", ".join(f"{n.split('.')[-3:]}: {v:.1e}" for n, v in
              sorted(worst.items(), key=lambda kv: -kv[1])[:4]))
        for n, v in worst.items():
            # pose gradients pass through the position gradient (two different kernels: fused into the mlp_base launch / the
            # standalone tn_hash_encode_bwd_input) and 786 k atomics: the ray-gradient tolerance of this file
            assert v <= (2e-3 if n.startswith("camera_optimizer") else 2e-4), (step, n, v)
        return upd1

    assert compare(0) is True  # steps < 10 update the proposal networks
    losses = [float(tr.train_iteration(i)[0]) for i in range(50)]
    tr.step = 50
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-10:]) < 0.7 * np.mean(losses[:5]), (losses[:5], losses[-10:])
    seen = {compare(50), compare(51)}  # update_schedule(50) = 1: every second step updates the proposal networks
    assert seen == {True, False}, seen


def test_thermoscenes_style_tree_to_training_steps(tmp_path):
    """Dataset boundary end to end: write a transforms.json tree (images/ + thermal/ PNGs, frame_train_* / frame_eval_*),
    parse it with the Thermal dataparser, build the HBM ray table and take optimisation steps on it."""
    import json

    import numpy as np
    from PIL import Image

    from thermo_nerf_amd import ThermalNerfModel, ThermalNerfModelConfig, synthetic
    from thermo_nerf_amd.data import ThermalDataParserConfig, ThermalDataset
    from thermo_nerf_amd.trainer import Trainer, TrainerConfig

    res, n = 32, 10
    cams = synthetic.orbit_cameras(res, res, list(range(n)), num_views=n, elevation_deg=[(0.0, 25.0)[v % 2] for v in range(n)])
    (tmp_path / "images").mkdir()
    (tmp_path / "thermal").mkdir()
    frames = []
    for i in range(n):
        rb = cams.generate_rays(i, device=DEV)
        rgb, th = synthetic.analytic_scene(rb.origins, rb.directions)
        name = f"frame_{'eval' if i % 5 == 4 else 'train'}_{i:04d}.png"
        Image.fromarray((rgb.cpu().numpy() * 255).round().astype(np.uint8)).save(tmp_path / "images" / name)
        Image.fromarray((th[..., 0].cpu().numpy() * 255).round().astype(np.uint8), mode="L").save(tmp_path / "thermal" / name)
        c2w = torch.cat([cams.camera_to_worlds[i], torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}", "transform_matrix": c2w})
    f = float(cams.fx[0])
    (tmp_path / "transforms.json").write_text(json.dumps(
        {"fl_x": f, "fl_y": f, "cx": res / 2, "cy": res / 2, "w": res, "h": res, "frames": frames}))

    parser = ThermalDataParserConfig(data=tmp_path).setup()
    train_out, eval_out = parser.get_dataparser_outputs("train"), parser.get_dataparser_outputs("val")
    assert len(train_out.cameras) == 8 and len(eval_out.cameras) == 2
    ds = ThermalDataset(train_out)
    table = ds.to_ray_table(DEV)
    assert len(table) == 8 * res * res and table.thermal.shape == (8 * res * res, 1)
    assert table.camera_indices.max().item() == 7
    # quantised to 8 bits on disk: within half a grey level of the analytic value
    rb0 = train_out.cameras.generate_rays(0, device=DEV, flat=True)
    assert torch.equal(rb0.origins, table.origins[: res * res])

    cfg = ThermalNerfModelConfig(**helpers.SMALL)  # camera optimizer SO3xR3, as in the reference
    model = ThermalNerfModel(cfg, metadata=train_out.metadata, scene_box=train_out.scene_box, num_train_data=len(ds)).to(DEV)
    synthetic.fill_model_(model, "init")
    tr = Trainer(model, table, TrainerConfig(train_num_rays_per_batch=2048))
    first = None
    for step in range(30):
        loss, loss_dict, metrics = tr.train_iteration(step)
        tr.step += 1
        first = loss.item() if first is None else first
    assert set(loss_dict) == {"rgb_loss", "interlevel_loss", "distortion_loss", "thermal"}
    assert torch.isfinite(loss) and loss.item() < 0.6 * first
    assert model.camera_optimizer.pose_adjustment.grad is not None
    with pytest.raises(ValueError, match="Thermal images not found"):
        ThermalNerfModel(cfg, metadata={}, scene_box=train_out.scene_box, num_train_data=8)  # REF thermal_nerf_model.py:75-76

    # evaluation harness on the eval split [REF evaluator/evaluator.py:47-133]
    from thermo_nerf_amd.evaluator import Evaluator
    from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as M

    model.max_temperature, model.min_temperature = 33.0, 14.0
    ev = Evaluator(model, ThermalDataset(eval_out), experiment_name="unit", job_param_identifier="t",
                   modalities_to_save=[M.RGB, M.THERMAL, M.THERMAL_COMBINED], threshold=0.5, device=DEV)
    res = ev.metrics
    for key in ("psnr", "psnr_thermal", "mae_thermal", "mae_thermal_foreground"):
        assert len(res[key]) == 2 and res[f"{key}_mean"] == pytest.approx(sum(res[key]) / 2, rel=1e-6)
        assert res[f"{key}_std"] >= 0
    assert 0 < res["mae_thermal_mean"] < 19.0  # degrees: normalised error x (33 - 14)
    for key in ("ssim", "ssim_thermal"):  # torchmetrics' SSIM of each frame (tn_ssim_fwd)
        assert len(res[key]) == 2 and all(-1.0 <= v <= 1.0 for v in res[key])
    assert all(v != v for v in res["lpips"]) and all(v != v for v in res["lpips_thermal"])  # NaN: no pretrained network offline
    ev.save_metrics(tmp_path / "eval")
    text = (tmp_path / "eval" / "metrics.json").read_text()
    assert "NaN" not in text  # strict JSON: the LPIPS entries are null
    saved = json.loads(text)
    assert saved["results"]["lpips_mean"] is None
    assert saved["method_name"] == "thermal-nerf" and saved["job_param_identifier"] == "t" and "psnr_mean" in saved["results"]
    ev.save_images([M.RGB, M.THERMAL_COMBINED], tmp_path / "eval" / "images")
    names = sorted(p.name for p in (tmp_path / "eval" / "images").glob("*.jpg"))
    assert names == ["img_00000.jpg", "img_00001.jpg", "thermal_combined_00000.jpg", "thermal_combined_00001.jpg"]
    assert Image.open(tmp_path / "eval" / "images" / "img_00000.jpg").size == (64, 32)  # ground truth | prediction


@pytest.mark.parametrize("dense_mb", [0, 8])
def test_eval_follows_fused_optimizer_updates(dense_mb):
    """torch.optim.Adam(fused=True) changes parameters without bumping their version counters; the prepared MFMA blobs
    (and, with a dense-grid budget, the dense re-layout of the coarse hash levels) must still be rebuilt before the next
    eval render."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48)
    for mod in [gm.field] + list(gm.proposal_networks):
        mod.dense_budget_bytes = dense_mb << 20
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=torch.zeros_like(cam).to(DEV))
    gm.eval()
    with torch.no_grad():
        before = gm(rb)["rgb"].clone()
    gm.train()
    opt = torch.optim.Adam(gm.get_param_groups()["fields"], lr=5e-2, eps=1e-15, fused=True)
    b = {k: v.to(DEV) for k, v in batch.items()}
    for step in range(3):
        out = gm(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
        loss = sum(gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b)).values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    gm.eval()
    with torch.no_grad():
        after = gm(rb)
    want = H.get_outputs({k: v.detach().cpu() for k, v in gm.state_dict().items()}, o, d, None, ocfg)
    assert (after["rgb"] - before).abs().max().item() > 1e-2, "the render did not move: stale prepared weights"
    assert (after["rgb"].cpu() - want["rgb"]).abs().max().item() <= 2e-3
    assert (after["thermal"].cpu() - want["thermal"]).abs().max().item() <= 2e-3


# --------------------------------------------------------------------------------------------------
# G7: the reference's own get_outputs / get_loss_dict (run over oracle-built components) against the HIP model
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["eval", "train", "train_scaled", "train_no_thermal"])
def test_model_wiring_golden_g7(golden_dir, monkeypatch, tag):
    """tests/golden/model_wiring.npz holds what the REAL ThermalNerfModel.get_outputs / get_loss_dict
    [REF thermal_nerf_model.py:210-326] returned (tools/make_golden.py G7): the HIP model's forward, loss dictionary and
    gradients reproduce the keys, their order, the values and the gates (camera optimizer in training only, pass_thermal_gradients,
    use_gradient_scaling, the never-applied thermal_loss_weight)."""
    from tests.test_oracle_golden import G7_CASES, G7_GRADS, g7_problem

    g, cm, sd, ocfg, o, d, cam, jit, batch = g7_problem(golden_dir)
    kw = G7_CASES[tag]
    training = kw["training"]
    gm = copy.deepcopy(cm).to(DEV)
    gm.config = copy.deepcopy(gm.config)
    with torch.no_grad():
        gm.camera_optimizer.pose_adjustment.copy_(sd["camera_optimizer.pose_adjustment"].to(DEV))
    gm.config.use_gradient_scaling = bool(kw.get("gradient_scaling", False))
    gm.field.pass_thermal_gradients = bool(kw.get("pass_thermal", True))
    gm.config.thermal_loss_weight = 123.0  # never applied [REF :319-323]
    gm.train(training)
    if training:
        orig = TR.get_outputs_train
        J = torch.cat(jit, dim=1).T.contiguous().to(DEV)
        monkeypatch.setattr(TR, "get_outputs_train", lambda m, rb: orig(m, rb, jitter=J))
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV))
    out = gm(rb) if training else gm(RayBundle(origins=o.to(DEV), directions=d.to(DEV)))
    assert list(out.keys()) == g[f"{tag}.output_keys"].tolist()
    for k in ("rgb", "thermal", "accumulation"):
        assert (out[k].detach().cpu().numpy() - g[f"{tag}.out.{k}"]).__abs__().max() <= 2e-5, k
    want_e = g[f"{tag}.out.expected_depth"]
    assert (np.abs(out["expected_depth"].detach().cpu().numpy() - want_e) <= 1e-4 * np.abs(want_e) + 1e-6).all()
    for k in ("depth", "prop_depth_0", "prop_depth_1"):  # medians: at most one ray may sit on a 0.5 tie
        bad = np.abs(out[k].detach().cpu().numpy() - g[f"{tag}.out.{k}"]) > 1e-4 * np.abs(g[f"{tag}.out.{k}"]) + 1e-6
        assert bad.sum() <= 1, k
    if training:
        for i in range(3):
            assert np.abs(out["weights_list"][i].detach().cpu().numpy() - g[f"{tag}.out.weights_list.{i}"]).max() <= 2e-5
            assert np.abs(out["ray_samples_list"][i].spacing_bins.cpu().numpy() - g[f"{tag}.out.spacing_bins.{i}"]).max() <= 2e-5
    b = {k: v.to(DEV) for k, v in batch.items()}
    loss = gm.get_loss_dict(out, b, gm.get_metrics_dict(out, b))
    assert list(loss.keys()) == g[f"{tag}.loss_keys"].tolist()
    for k, v in loss.items():
        want = float(g[f"{tag}.loss.{k}"])
        assert abs(v.item() - want) <= 5e-5 * abs(want) + 1e-8, (k, v.item(), want)
    if training:
        gm.zero_grad(set_to_none=True)
        sum(loss.values()).backward()
        named = dict(gm.named_parameters())
        for name in G7_GRADS:
            want = torch.from_numpy(g[f"{tag}.grad.{name}"])
            got = named[name].grad
            if want.abs().max().item() == 0.0:
                assert got is None or got.abs().max().item() == 0.0, name
                continue
            tol = 2e-2 if name.startswith("camera_optimizer") else 2e-3
            assert rel(got, want) <= tol, f"{name}: {rel(got, want):.2e}"


def test_out_of_range_camera_index_poisons_the_ray_instead_of_reading_elsewhere():
    """the camera-optimizer and appearance-embedding look-ups index tables with the batch's camera ids; torch's
    index_select / nn.Embedding would raise on a stale or eval-split id.  The kernels never read outside the tables: such a ray
    comes out NaN (the step's loss turns NaN — loud), and the backward skips it."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("stress", 48, camera_optimizer_mode="SO3xR3")
    cam = cam.clone()
    cam[5] = 8      # num_train_data = 8: one past the tables
    cam[9] = -1
    out, loss = _gpu_step(gm, o, d, jit, cam, batch)
    rgb = out["rgb"].detach().cpu()
    bad = torch.isnan(rgb).any(dim=-1)
    assert bad[5] and bad[9] and int(bad.sum()) == 2
    assert torch.isnan(loss["rgb_loss"]).item()


def test_cached_training_structs_follow_the_parameter_storage():
    """train_struct() keeps the C structs of a network while its parameters keep their storage (an optimizer updates in place);
    moving a parameter to new storage (what .to(), .float() or a manual `p.data = ...` do) must rebuild them — the step then
    reads the NEW memory: same gradients as before when the values are the same, different ones when they are not."""
    gm, sd, ocfg, o, d, jit, cam, batch = _train_setup("scene", 48)
    _gpu_step(gm, o, d, jit, cam, batch)
    before = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
    s0 = gm.field.train_struct()
    assert gm.field.train_struct() is s0  # cached
    old = {}
    for n, p in gm.named_parameters():
        old[n] = p.data
        p.data = p.data.clone()  # same values, new storage
    assert gm.field.train_struct() is not s0
    _gpu_step(gm, o, d, jit, cam, batch)
    for n, p in gm.named_parameters():
        if n in before:
            assert rel(p.grad, before[n]) <= 1e-5, n
    for t in old.values():
        t.fill_(float("nan"))  # the old storage is dead: a stale pointer would now read NaN
    with torch.no_grad():
        gm.field.mlp_head.layers[2].bias += 0.25
    _gpu_step(gm, o, d, jit, cam, batch)
    g = dict(gm.named_parameters())["field.mlp_head.layers.2.bias"].grad
    assert torch.isfinite(g).all() and rel(g, before["field.mlp_head.layers.2.bias"]) > 1e-3


def test_fresh_zeros_are_zero_disjoint_and_survive_a_block_rollover():
    """_hip.fresh_zeros: the small zero-initialised accumulators of a step (loss scalars, pose gradient) are successive slices of
    a pre-cleared block — never handed out twice, zero on arrival, also across the change to a new block."""
    from thermo_nerf_amd import _hip as H

    seen = []
    n = H._ZERO_BLOCK_FLOATS // 16  # the largest request a block serves
    for k in range(40):  # 40 x 1/16 of a block: at least two rollovers
        t = H.fresh_zeros((n,), DEV)
        assert t.shape == (n,) and float(t.abs().sum()) == 0.0
        t.fill_(float(k + 1))
        seen.append(t)
    for k, t in enumerate(seen):
        assert float(t.min()) == float(t.max()) == float(k + 1)  # nobody else got the same memory
    big = H.fresh_zeros((H._ZERO_BLOCK_FLOATS,), DEV)  # larger than a block serves: a plain zeros tensor
    assert big.numel() == H._ZERO_BLOCK_FLOATS and float(big.abs().sum()) == 0.0
    s = H.fresh_zeros((3, 6), DEV)
    assert s.shape == (3, 6) and s.is_contiguous() and s.data_ptr() % 256 == 0


@pytest.mark.parametrize("S", [48, 192])
def test_regularisers_launched_by_the_forward_equal_the_ones_launched_on_demand(S):
    """config.overlap_regularisers: the training forward launches distortion + interlevel on the step's side streams;
    get_metrics_dict / get_loss_dict must pick exactly those results up (entry consumed), every loss and every gradient must
    equal the on-demand launches (same kernels, same inputs; their block sums meet in fp32 atomics, so to rounding), and a call
    with OTHER tensors or another multiplier must not be served from the forward's launch."""
    gm, _, _, o, d, jit, cam, batch = _train_setup("scene", S)

    def run(flag):
        gm.config.overlap_regularisers = flag
        out, loss_dict = _gpu_step(gm, o, d, jit, cam, batch)
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in gm.named_parameters() if p.grad is not None}
        return {k: v.detach().clone() for k, v in loss_dict.items()}, grads

    l0, g0 = run(False)
    assert not TR._REG_PRE
    l1, g1 = run(True)
    assert not TR._REG_PRE  # both results were taken
    assert set(l0) == set(l1) and set(g0) == set(g1)
    for k in l0:
        assert torch.allclose(l0[k], l1[k], rtol=2e-6, atol=0), (k, l0[k].item(), l1[k].item())
    for n in g0:
        if "hash_table" in n:  # fp32 atomics: order-dependent
            assert torch.allclose(g0[n], g1[n], rtol=1e-4, atol=1e-9), n
        else:
            assert torch.allclose(g0[n], g1[n], rtol=2e-5, atol=1e-9), n

    # a forward whose regularisers are asked for with a different multiplier / different tensors: computed afresh, same
    # numbers, and the forward's launch stays for a caller it does match
    gm.config.overlap_regularisers = True
    rb = gm.collider(RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=cam.to(DEV)))
    out = TR.get_outputs_train(gm, rb, jitter=torch.cat(jit, dim=1).T.contiguous().to(DEV))
    assert TR._REG_PRE
    entry = next(iter(TR._REG_PRE.values()))
    other = TR.distortion_loss(out["weights_list"], out["ray_samples_list"], mult=0.5 * gm.config.distortion_loss_mult)
    assert "dist" in entry  # another multiplier: not served, not dropped
    clone = [w.clone() for w in out["weights_list"]]
    a = TR.interlevel_loss(clone, out["ray_samples_list"], mult=gm.config.interlevel_loss_mult)
    assert "inter" in entry  # other tensors: the same
    b = TR.interlevel_loss(out["weights_list"], out["ray_samples_list"], mult=gm.config.interlevel_loss_mult)
    assert "inter" not in entry  # the forward's own tensors: served
    assert torch.allclose(a, b, rtol=2e-6, atol=0)
    # an in-place edit between the forward and the losses.  The weights are views returned by the step's
    # autograd Function: torch itself refuses to use them after an in-place edit.  The bins are plain outputs: their version
    # counter is part of the key, so the distortion term is computed from the edited values, not served from the forward's launch
    with torch.no_grad():
        out["ray_samples_list"][-1].spacing_bins.mul_(0.5)
    edited = TR.distortion_loss(out["weights_list"], out["ray_samples_list"], mult=gm.config.distortion_loss_mult)
    assert "dist" in entry
    gm.config.overlap_regularisers = False
    want = TR.distortion_loss([w.clone() for w in out["weights_list"]], out["ray_samples_list"], mult=gm.config.distortion_loss_mult)
    assert torch.allclose(edited, want, rtol=2e-6, atol=0)
    fresh = TR.distortion_loss(out["weights_list"], out["ray_samples_list"], mult=0.5 * gm.config.distortion_loss_mult)
    assert not torch.allclose(fresh, other, rtol=1e-3, atol=0)  # (the halved bins do change the term)
    # what nobody collected is dropped (its side stream joined) by the backward of that forward, or by the next forward
    assert TR._REG_PRE
    (out["rgb"].sum() + out["thermal"].sum()).backward()
    assert not TR._REG_PRE
