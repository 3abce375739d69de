"""The position gradient's device forms (tn_hash_encode_bwd_input, tn_field_bwd_fused recomputing the corners, tn_field_bwd_fused
from tn_field_fwd_train's Jacobian), the Jacobian tensor itself, tn_hash_encode_fwd and tn_frustum_positions_bwd, sample by
sample against the cell-exact fp64 reference of tests/position_gradient_reference.py — on grid planes and their ulp neighbours,
at the contraction's kinks and ties, on box faces, in ragged waves and in the grid-stride pass.

Tolerance, everywhere: |got - want| <= K * 2^-24 * B (+ 1e-30 for all-zero rows), B the reference's absolute evaluation and K
the number of fp32 roundings on the longest path of the form under test, counted from the kernels' code (the counts and their
derivations stand next to the K_* constants of the reference module and are repeated at each form below).  K is never tuned
against device output.  Every check prints ``position-gradient bound | form | grid | K | worst err / (eps B)``;
profiles/micro/position_gradient_bounds.txt records one run's lines."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import position_gradient_reference as R
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25  # prefill of every output buffer and its guard rows
GUARD = 5

# (num_levels, log2_hashmap_size, max_res): the field's grid; a proposal grid; either side of the LP = 8 / 16 switch of
# hash_encode_bwd_input_kernel; 13 levels (three idle lanes per sample in the <16> form); one level
GRIDS = [(16, 15, 2048), (5, 13, 128), (8, 12, 512), (9, 12, 512), (13, 10, 1024), (1, 4, 16)]
# 4 and 8 samples fill one wave of the <16> and <8> forms; 4097: more than one block, a ragged last wave
COUNTS = [1, 3, 4, 5, 8, 9, 63, 64, 65, 4097]
BOX = np.array([[-1.5, -0.5, 0.25], [1.0, 2.0, 0.75]], dtype=np.float32)


def _report(form, grid, K, got, want, B):
    """assert |got - want| <= K eps32 B + 1e-30 entry by entry, after printing the worst ratio"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == B.shape and np.isfinite(got).all(), form
    err = np.abs(got - want)
    pos = B > 0
    worst = float((err[pos] / (R.EPS32 * B[pos])).max()) if pos.any() else 0.0
    print(f"position-gradient bound | {form} | {grid} | K {K} | worst {worst:.3f}")
    bad = err > K * R.EPS32 * B + 1e-30
    assert not bad.any(), f"{form} {grid}: {int(bad.sum())} entries outside K = {K}, worst {worst:.2f} eps B at {np.argwhere(bad)[:5].tolist()}"
    return worst


class Grid:
    """a hash grid with a seeded random table on the device and its host copy"""
    _cache: dict = {}

    def __init__(self, L, log2T, max_res):
        self.L, self.log2T, self.max_res = L, log2T, max_res
        self.scal = H.hash_scalings(L, 16, max_res)
        self.scalings = [float(s) for s in self.scal.tolist()]
        t = torch.rand(L << log2T, 2, generator=torch.Generator().manual_seed(100 * L + log2T)) * 2 - 1
        self.table, self.table_dev = t.numpy(), t.to(DEV)
        self.c = _hip.tn_hashgrid()
        self.c.table, self.c.num_levels, self.c.log2_hashmap_size = self.table_dev.data_ptr(), L, log2T
        for i, s in enumerate(self.scalings):
            self.c.scalings[i] = s
        self.name = f"L{L} T2^{log2T} res{max_res}"

    @classmethod
    def get(cls, L, log2T, max_res):
        key = (L, log2T, max_res)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def cases(self, contraction):
        key = ("cases", self.L, self.log2T, self.max_res, contraction)
        if key not in self._cache:
            cases = R.mixed_cases(self.scalings, contraction)
            space = R.CONTRACTION if contraction else R.UNIT_BOX
            self._cache[key] = (cases, space, *R.normalized(cases.positions, space))
        return self._cache[key]


def c_space(space: R.Space):
    return _hip.make_space(space.contraction, None if space.aabb is None else torch.tensor(np.asarray(space.aabb)))


def guarded(n, width):
    """an [n, width] output inside a sentinel-filled buffer with GUARD rows on either side"""
    buf = torch.full((n + 2 * GUARD, width), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def bwd_input(grid: Grid, space: R.Space, pos32: np.ndarray, d_enc32: np.ndarray):
    """tn_hash_encode_bwd_input into a guarded buffer, twice: the call overwrites (same bits again), the guards stay"""
    n = len(pos32)
    pos, d_enc = torch.from_numpy(pos32).to(DEV), torch.from_numpy(d_enc32).to(DEV)
    buf, out = guarded(n, 3)
    sp = c_space(space)
    for rep in range(2):
        _hip.check(_hip.load().tn_hash_encode_bwd_input(grid.c, sp, pos.data_ptr(), d_enc.data_ptr(), n, out.data_ptr(), _hip.current_stream()),
                   "tn_hash_encode_bwd_input")
        torch.cuda.synchronize()
        if rep == 0:
            first = out.clone()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32)) and guards_intact(buf, n)
    return out.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# tn_hash_encode_bwd_input.  K = R.K_BWD_INPUT = 21: encode_level_grad 10 (difference, 1 - o, three nested products and sums,
# x d_enc, x scale, the second channel's add) + 4 shuffle adds (<16>; the <8> kernel has 3: counted as 4) + position_grad_finish 7
# (dsm from mag^3, the dot product, dsm x dot / ties, the final add).
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contraction", [False, True], ids=["box", "contraction"])
@pytest.mark.parametrize("L,log2T,max_res", GRIDS)
def test_bwd_input_against_the_frozen_cell_reference(L, log2T, max_res, contraction):
    """d_enc random normal with whole zero rows; every sample count of COUNTS (the first n of the shuffled cases; 4097 cycles
    through all of them); the unit box isolates the levels, the contraction adds the chain"""
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32, sel = grid.cases(contraction)
    rng = np.random.default_rng(L + 7 * contraction)
    for n in COUNTS:
        idx = np.resize(np.arange(len(cases)), n)
        d_enc = rng.standard_normal((n, 2 * L)).astype(np.float32)
        d_enc[rng.random(n) < 0.2] = 0.0
        got = bwd_input(grid, space, cases.positions[idx], d_enc)
        g, B = R.frozen_gradient(p32[idx], d_enc, grid.table, grid.scalings, log2T)
        g_x, B_x = R.position_chain_gradient(cases.positions[idx], g, B, space)
        _report("tn_hash_encode_bwd_input", f"{grid.name} {'contraction' if contraction else 'unit box'} n={n}", R.K_BWD_INPUT, got, g_x, B_x)
        # selector 0: +0.0 bit for bit
        assert not got[~sel[idx]].view(np.int32).any()
        assert not got[(d_enc == 0).all(axis=1)].any()


@pytest.mark.parametrize("L,log2T,max_res", GRIDS)
def test_bwd_input_one_level_at_a_time(L, log2T, max_res):
    """one call per level with d_enc zero outside that level: a level on the wrong lane, or with another level's scale or table,
    shows here.  In the unit box the chain is the identity, so an axis on a plane of the level carries exactly 0.0."""
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32, sel = grid.cases(False)
    n = len(cases)
    rng = np.random.default_rng(L)
    worst, planes = 0.0, 0
    for l in range(L):
        d_enc = np.zeros((n, 2 * L), dtype=np.float32)
        d_enc[:, 2 * l:2 * l + 2] = rng.standard_normal((n, 2))
        got = bwd_input(grid, space, cases.positions, d_enc)
        g, B = R.frozen_level_gradient(p32, d_enc[:, 2 * l:2 * l + 2], grid.table, grid.scalings[l], l, log2T)
        g_x, B_x = R.position_chain_gradient(cases.positions, g, B, space)
        worst = max(worst, _report("tn_hash_encode_bwd_input one-hot", f"{grid.name} unit box level {l}", R.K_BWD_INPUT, got, g_x, B_x))
        fl, ce, _ = R.frozen_cell(p32, grid.scalings[l])
        flat = (fl == ce) & sel[:, None]
        planes += int(flat.sum())
        assert not got[flat].any()                       # exactly 0.0 along an on-plane axis
        assert np.abs(g_x[sel]).max() > 0 and np.abs(got[sel]).max() > 0
        for tag in ("x", "yz", "xyz"):                   # the crafted plane samples of this level are among them
            rows = cases.where(f"plane:l{l}:{tag}:on")
            assert len(rows) == 4 and flat[rows][:, ["xyz".index(a) for a in tag]].all()
    assert planes >= 24 * L


def test_bwd_input_in_a_box_that_is_not_the_unit_box():
    """the AABB branch of the chain with three different extents, and its faces (p exactly 0 or 1: selector 0)"""
    grid = Grid.get(16, 15, 2048)
    space = R.Space(False, BOX)
    lo, hi = BOX.astype(np.float64)
    inside = (lo + (hi - lo) * np.random.default_rng(21).random((700, 3))).astype(np.float32)
    cases = R.concat(R.box_faces(BOX), R.Cases(inside, ["inside"] * len(inside)), R.uniform(300, 22, 2.5))
    p32, sel = R.normalized(cases.positions, space)
    d_enc = np.random.default_rng(23).standard_normal((len(cases), 32)).astype(np.float32)
    got = bwd_input(grid, space, cases.positions, d_enc)
    g, B = R.frozen_gradient(p32, d_enc, grid.table, grid.scalings, 15)
    g_x, B_x = R.position_chain_gradient(cases.positions, g, B, space)
    _report("tn_hash_encode_bwd_input", f"{grid.name} box {BOX.tolist()}", R.K_BWD_INPUT, got, g_x, B_x)
    assert sel.sum() >= 700 and (~sel).sum() >= 12 + 100
    assert not got[~sel].view(np.int32).any()
    for i, label in enumerate(cases.labels[:18]):
        assert bool(sel[i]) == label.endswith(":inside"), label


@pytest.mark.parametrize("L,log2T,max_res,n", [(1, 4, 16, (1 << 21) + 9), (9, 12, 512, (1 << 20) + 7)], ids=["LP8", "LP16"])
def test_bwd_input_grid_stride_pass(L, log2T, max_res, n):
    """more (sample, level) lanes than the 2^16-block launch holds (2^21 samples of the <8> kernel, 2^20 of the <16> kernel): the
    samples behind them are the grid-stride loop's second pass.  Checked: every sample of the second pass and every 97th before."""
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32_all, sel_all = grid.cases(True)
    first_pass = (1 << 16) * 256 // (8 if L <= 8 else 16)
    assert n > first_pass
    pick = torch.randint(0, len(cases), (n,), generator=torch.Generator().manual_seed(n))
    pos = torch.from_numpy(cases.positions)[pick].to(DEV)
    d_enc = torch.randn(n, 2 * L, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    buf, out = guarded(n, 3)
    rows = torch.cat([torch.arange(0, first_pass, 97), torch.arange(first_pass, n)])
    for rep in range(2):
        _hip.check(_hip.load().tn_hash_encode_bwd_input(grid.c, c_space(space), pos.data_ptr(), d_enc.data_ptr(), n, out.data_ptr(),
                                                        _hip.current_stream()), "tn_hash_encode_bwd_input")
        torch.cuda.synchronize()
        if rep == 0:  # (a checksum of all bits and the checked rows themselves, not a second copy of the output)
            first = (int(out.view(torch.int32).sum(dtype=torch.int64)), out[rows.to(DEV)].clone())
    assert first[0] == int(out.view(torch.int32).sum(dtype=torch.int64)) and torch.equal(first[1].view(torch.int32), out[rows.to(DEV)].view(torch.int32))
    assert guards_intact(buf, n)
    assert int((out == SENTINEL).sum()) == 0  # every row was written
    idx = pick[rows].numpy()
    de = d_enc[rows.to(DEV)].cpu().numpy()
    g, B = R.frozen_gradient(p32_all[idx], de, grid.table, grid.scalings, log2T)
    g_x, B_x = R.position_chain_gradient(cases.positions[idx], g, B, space)
    _report("tn_hash_encode_bwd_input grid-stride", f"{grid.name} contraction n={n}", R.K_BWD_INPUT, out[rows.to(DEV)].cpu().numpy(), g_x, B_x)


# ----------------------------------------------------------------------------------------------------------------------
# tn_hash_encode_fwd.  K = R.K_FEATURES = 9: torch's lerp a o + b (1 - o) is three roundings on its b side (1 - o, the product,
# the sum), nested three times.
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contraction", [False, True], ids=["box", "contraction"])
@pytest.mark.parametrize("L,log2T,max_res", [(16, 15, 2048), (5, 13, 128), (1, 4, 16)])
def test_hash_encode_fwd_on_the_crafted_positions(L, log2T, max_res, contraction):
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32, sel = grid.cases(contraction)
    n = len(cases)
    pos = torch.from_numpy(cases.positions).to(DEV)
    ebuf, enc = guarded(n, 2 * L)
    sbuf, s = guarded(n, 1)
    _hip.check(_hip.load().tn_hash_encode_fwd(grid.c, c_space(space), pos.data_ptr(), n, enc.data_ptr(), s.data_ptr(), _hip.current_stream()),
               "tn_hash_encode_fwd")
    torch.cuda.synchronize()
    assert guards_intact(ebuf, n) and guards_intact(sbuf, n)
    assert np.array_equal(s.cpu().numpy()[:, 0], sel.astype(np.float32))
    got = enc.cpu().numpy()
    want, B = np.zeros((n, 2 * L)), np.zeros((n, 2 * L))
    for l in range(L):
        want[:, 2 * l:2 * l + 2], B[:, 2 * l:2 * l + 2] = R.frozen_features(p32, grid.table, grid.scalings[l], l, log2T)
    _report("tn_hash_encode_fwd", f"{grid.name} {'contraction' if contraction else 'unit box'}", R.K_FEATURES, got, want, B)


# ----------------------------------------------------------------------------------------------------------------------
# tn_field_fwd_train / tn_field_bwd_fused on the builders' cases
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = {15: (5, (1, 3)), 175: (5, (7, 5)), 6912: (48, (12, 12))}  # N = R * S: fewer than a 16-sample tile | a ragged last tile | full
_fused_cache: dict = {}


def fused(N):
    """the forward with its Jacobian and the two backward forms under test, once per N, on the shuffled cases of every builder"""
    if N not in _fused_cache:
        from tests.test_gpu_training import field_train_forms

        S, hw = SHAPES[N]
        scal = [float(s) for s in H.hash_scalings(16, 16, 2048).tolist()]
        cases = R.mixed_cases(scal, True, seed=N)
        idx = np.resize(np.arange(len(cases)), N)
        pos32 = cases.positions[idx]
        f = field_train_forms(S, hw, pos=torch.from_numpy(pos32).to(DEV), forms=((True, 1), (True, "jac")))
        assert f.N == N
        enc = f.gm.field.mlp_base.encoder
        assert [float(s) for s in enc.scalings.tolist()] == scal and enc.num_levels == 16
        p32, sel = R.normalized(pos32, R.CONTRACTION)
        _fused_cache[N] = dict(f=f, cases=cases, idx=idx, pos32=pos32, p32=p32, sel=sel, scal=scal, log2T=enc.log2_hashmap_size,
                               table=enc.hash_table.detach().cpu().numpy())
    return _fused_cache[N]


# K = R.K_FUSED_RECOMPUTE = 25: encode_level_grad 10, three more levels x two channel adds in the same lane 6, two shuffle adds,
#   position_grad_finish 7
# K = R.K_FUSED_JACOBIAN = 23: hash_blend_jac 5 (corner difference, two stages of fmaf(o, a, fmaf(-o, b, b))),
#   x scale in the forward 1, the backward's fmaf chain of one axis 8 (4 levels x 2 channels), two shuffle adds,
#   position_grad_finish 7
@pytest.mark.parametrize("form,K", [(1, R.K_FUSED_RECOMPUTE), ("jac", R.K_FUSED_JACOBIAN)], ids=["recompute", "jacobian"])
@pytest.mark.parametrize("N", list(SHAPES))
def test_fused_backward_position_gradient(N, form, K):
    """g_enc as the kernel wrote it is the reference's d_enc; g_pos sample by sample"""
    c = fused(N)
    res = c["f"].res[(True, form)]
    d_enc = res["g_enc"].cpu().numpy()
    assert np.isfinite(d_enc).all() and np.abs(d_enc).max() > 0
    g, B = R.frozen_gradient(c["p32"], d_enc, c["table"], c["scal"], c["log2T"])
    g_x, B_x = R.position_chain_gradient(c["pos32"], g, B, R.CONTRACTION)
    got = res["g_pos"].cpu().numpy()
    _report(f"tn_field_bwd_fused {'from the Jacobian' if form == 'jac' else 'recomputing'}", f"L16 T2^{c['log2T']} res2048 contraction N={N}", K, got, g_x, B_x)
    assert not got[~c["sel"]].view(np.int32).any()     # selector 0: +0.0 bit for bit
    assert np.array_equal(c["f"].sel.cpu().numpy(), c["sel"].astype(np.float32))


def _jacobian(N):
    """(got [N, 16, 3, 2], want, B) of the stored Jacobian J[l][c] = s_l d enc_l / d o_c, and the raw tensor"""
    c = fused(N)
    jac = c["f"].jac
    passes = (N + 63) // 64
    tiles = jac[:-1].reshape(passes, 16, 3, 64, 2).cpu().numpy()
    got = tiles.transpose(0, 3, 1, 2, 4).reshape(passes * 64, 16, 3, 2)
    want, B = np.zeros((N, 16, 3, 2)), np.zeros((N, 16, 3, 2))
    for l in range(16):
        for ch in range(2):
            one = np.zeros((N, 2))
            one[:, ch] = 1.0
            want[:, l, :, ch], B[:, l, :, ch] = R.frozen_level_gradient(c["p32"], one, c["table"], c["scal"][l], l, c["log2T"])
    return c, jac, got, want, B


@pytest.mark.parametrize("N", list(SHAPES))
def test_forward_jacobian_structure(N):
    """the padding samples of the last pass are finite (or untouched), the guard row behind the tensor is untouched, an axis on a
    plane of a level (and every axis of a sample with selector 0) holds exactly 0"""
    c, jac, got, want, B = _jacobian(N)
    assert bool((jac[-1] == 7.0).all())
    assert np.isfinite(got).all()
    flat = np.zeros((N, 16, 3), dtype=bool)
    for l in range(16):
        fl, ce, _ = R.frozen_cell(c["p32"], c["scal"][l])
        flat[:, l] = fl == ce
    assert flat[~c["sel"]].all()
    assert not got[:N][flat].any() and (N < 100 or flat[c["sel"]].sum() >= 30)


# K = R.K_JACOBIAN_TENSOR = 6: hash_blend_jac's slopes interpolate as fmaf(o, a, fmaf(-o, b, b)), two roundings a stage:
#   d / d ox: corner difference 1, y stage 3, z stage 5; d / d oy: x stage 2, difference 3, z stage 5; d / d oz: x stage 2,
#   y stage 4, difference 5; x scale 6
@pytest.mark.parametrize("N", list(SHAPES))
def test_forward_jacobian_entries(N):
    """every entry of every case against frozen_level_gradient with a one-hot d_enc.  (Slopes taken from the differences of the
    feature lerp fmaf(o, a - b, b), as hash_blend_jac first had them, fail this at N = 6912: 8 of 663 552 entries left K = 6, the
    worst at 7.94 eps B one ulp below a plane, where that form weighs the floor corner's rounding with o and B with 1 - o.)"""
    c, jac, got, want, B = _jacobian(N)
    _report("tn_field_fwd_train Jacobian", f"L16 T2^{c['log2T']} res2048 contraction N={N}", R.K_JACOBIAN_TENSOR, got[:N], want, B)


# ----------------------------------------------------------------------------------------------------------------------
# tn_frustum_positions_bwd.  K = R.frustum_roundings(n): s + e and g x t (d_d only), ceil(n / 64) - 1 adds in a lane, 6 in the
# wave scan, 1 onto what the output held.
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_frustum_positions_bwd(n):
    rng = np.random.default_rng(n)
    for rays in (1, 3, 4, 5, 257):  # four rays per block: a partial last block, one ray more than 64 blocks
        g = rng.standard_normal((rays, n, 3)).astype(np.float32)
        g[rng.random((rays, n)) < 0.1] = 0.0
        starts = (rng.random((rays, n)) * 6).astype(np.float32)
        ends = (starts + rng.random((rays, n)).astype(np.float32)).astype(np.float32)
        pre_o, pre_d = rng.standard_normal((rays, 3)).astype(np.float32), rng.standard_normal((rays, 3)).astype(np.float32)
        obuf, d_o = guarded(rays, 3)
        dbuf, d_d = guarded(rays, 3)
        d_o.copy_(torch.from_numpy(pre_o))
        d_d.copy_(torch.from_numpy(pre_d))
        dev = [torch.from_numpy(a).to(DEV) for a in (g, starts, ends)]
        _hip.check(_hip.load().tn_frustum_positions_bwd(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), rays, n, d_o.data_ptr(),
                                                        d_d.data_ptr(), _hip.current_stream()), "tn_frustum_positions_bwd")
        torch.cuda.synchronize()
        assert guards_intact(obuf, rays) and guards_intact(dbuf, rays)
        w_o, w_d, B_o, B_d = R.frustum_positions_adjoint(g, starts, ends)
        K_o, K_d = R.frustum_roundings(n)
        _report("tn_frustum_positions_bwd d_origins", f"R={rays} n={n}", K_o, d_o.cpu().numpy(), pre_o + w_o, np.abs(pre_o) + B_o)
        _report("tn_frustum_positions_bwd d_directions", f"R={rays} n={n}", K_d, d_d.cpu().numpy(), pre_d + w_d, np.abs(pre_d) + B_d)
