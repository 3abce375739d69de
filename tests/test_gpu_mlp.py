"""The MLP kernels of a training step on the device, entry by entry against the fp64 references of tests/mlp_reference.py, through
the C entry points: tn_linear_fwd (rows form, wide form, the second grid-stride round), tn_linear_bwd (matrix-pipe form with the
workspace, 64 x 64 blocks of a wide layer, the VALU form without a workspace), tn_linear_chain_bwd, tn_density_fwd_train,
tn_density_bwd_train, tn_ray_head_fwd / tn_ray_head_bwd and tn_field_bwd_fused (one launch, split, split with bf16 pieces, each with
and without stored base rows) — each also at a size where a persistent block takes a SECOND tile, which no other stage test reaches.

Bit for bit: every exact family of the reference module through every form and at both the small and the second-round sizes.
Bounded per entry by the counted bounds of the reference module (none tuned against what the device gives; run with -s for the worst
ratio to the bound of every check; profiles/micro/mlp_bounds.txt holds one such run): the rest.  Inputs are built on the CPU by the
builders of the reference module and copied over; no element is skipped or masked.  Every matrix lives in a buffer with its row
stride, a column offset, two guard rows and, for the unaligned forms, a one-float shift of the pointer: whatever lies outside the
[n, width] block the contract names must keep its fill, outputs are pre-filled with a sentinel where the contract is `=`.

tn_field_bwd_fused is called on a hand-built tn_thermal_field over the builder's weights with the builder's hash features written in
the tiled layout the header documents, so that the reference and the kernel start from the same numbers; its position gradient
(d_positions, the Jacobian variant) has its own module, tests/test_gpu_position_gradient.py, and is not asked for here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mlp_reference as M
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
SENT = f32(7.0)      # outputs
PAD = f32(1.0e30)    # what surrounds an input: a kernel that takes it for data is off by far more than any bound
TN_ERR_WORKSPACE = -4


class Mat:
    """an [n, w] matrix inside a device buffer of rows ``ld`` floats apart, at column ``off``, the pointer ``shift`` floats behind an
    allocation boundary, two guard rows behind it; everything around the matrix holds ``fill``"""

    def __init__(self, a, ld=None, off=0, shift=0, fill=PAD):
        a = np.asarray(a, f32)
        self.n, self.w = a.shape
        self.ld = self.w if ld is None else ld
        assert off + self.w <= self.ld
        self.off, self.shift, self.fill, self.rows = off, shift, f32(fill), self.n + 2
        flat = np.full(shift + self.rows * self.ld, fill, f32)
        flat[shift:].reshape(self.rows, self.ld)[:self.n, off:off + self.w] = a
        self.t = torch.from_numpy(flat).to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * (self.shift + self.off)

    def read(self, name):
        """the matrix; asserts that nothing around it was written"""
        torch.cuda.synchronize()
        flat = self.t.cpu().numpy()
        v = flat[self.shift:].reshape(self.rows, self.ld)
        out = v[:self.n, self.off:self.off + self.w].copy()
        around = np.ones(v.shape, bool)
        around[:self.n, self.off:self.off + self.w] = False
        assert np.all(v[around] == self.fill) and np.all(flat[:self.shift] == self.fill), f"{name}: written outside its block"
        return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, f32))).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def within(entry, family, what, got, want, tol, m):
    """every entry inside its bound; prints the worst ratio first"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    tol = np.broadcast_to(np.asarray(tol, f64), want.shape)
    assert got.shape == want.shape and np.all(np.isfinite(got)), (entry, family, what)
    err = np.abs(got - want)
    ratio = np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0)
    print(f"{entry} | {family} | {what}: worst |device - fp64| / bound = {float(ratio.max()) if ratio.size else 0.0:.4f} (m = {m})")
    assert np.all(err <= tol), (entry, family, what, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(np.asarray(want, f64).astype(f32))
    assert got.shape == want.shape, name
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~((got == 0) & (want == 0))  # the sign of a zero is not part of the contract
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def judge(exact, entry, family, what, got, want, tol, m):
    if exact:
        same_bits(f"{entry} {family} {what}", got, want)
    else:
        within(entry, family, what, got, want, tol, m)


_WS = {}


def workspace(kind):
    """the partial-sum slabs, filled with NaN once: a slab entry read before it was written would show"""
    if kind not in _WS:
        lib = _hip.load()
        nbytes = lib.tn_linear_bwd_workspace_bytes() if kind == "linear" else lib.tn_linear_chain_bwd_workspace_bytes()
        _WS[kind] = (torch.full((nbytes // 4,), float("nan"), device=DEV), nbytes)
    return _WS[kind]


# ----------------------------------------------------------------------------------------------------------------------
# tn_linear_fwd
# ----------------------------------------------------------------------------------------------------------------------
def run_fwd(c: M.LinearCase, ldx, off, ldy=None, shift=0, bias=True):
    n, IN = c.x.shape
    OUT = c.W.shape[0]
    x = Mat(c.x, ldx, off, shift)
    y = Mat(np.full((n, OUT), SENT), ldy, 0, shift, fill=SENT)
    w, b = dev(c.W), dev(c.b)
    lin = _hip.tn_linear(w.data_ptr(), b.data_ptr() if bias else None, IN, OUT)
    _hip.check(_hip.load().tn_linear_fwd(x.ptr, x.ld, C.byref(lin), c.act, n, y.ptr, y.ld, _hip.current_stream()), "tn_linear_fwd")
    return y.read("y")


def check_fwd(family, IN, OUT, n, act, ldx, off, exact, seed, **kw):
    c = (M.exact_linear_case if exact else M.linear_case)(IN, OUT, n, act, seed)
    ref = M.linear_forward(c.x, c.W, c.b if kw.get("bias", True) else None, act)
    got = run_fwd(c, ldx, off, **kw)
    judge(exact, "tn_linear_fwd", family, f"({IN},{OUT}) n={n} act={act} {kw or ''}", got, ref.y, ref.tol, ref.m)


ROWS_SHAPES = [(1, 1, 1, 0), (15, 64, 16, 1), (32, 64, 32, 0), (63, 64, 64, 0), (64, 3, 64, 0), (64, 1, 64, 0), (64, 64, 64, 0)]
N_FWD = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("IN,OUT,ldx,off", ROWS_SHAPES)
def test_linear_fwd_rows_form(IN, OUT, ldx, off):
    """INP 16 / 32 / 64; (15,64) at offset 1 and every shifted call are unaligned (vec_in = 0); (63,64) at ldx 64 reads the padded
    column and must zero it"""
    for n in N_FWD:
        for act in (0, 1, 2):
            check_fwd("rows", IN, OUT, n, act, ldx, off, False, 10 * n + act)
            if act != 2:
                check_fwd("rows exact", IN, OUT, n, act, ldx, off, True, 10 * n + act)
        check_fwd("rows", IN, OUT, n, 2, ldx, off, False, n, shift=1)
        check_fwd("rows exact", IN, OUT, n, 1, ldx, off, True, n, shift=1)
    check_fwd("rows", IN, OUT, 65, 1, ldx, off, False, 5, ldy=OUT + 4)   # ldy > OUT, still 16-byte rows
    check_fwd("rows", IN, OUT, 65, 1, ldx, off, False, 6, ldy=OUT + 3)
    check_fwd("rows", IN, OUT, 65, 2, ldx, off, False, 7, bias=False)
    check_fwd("rows exact", IN, OUT, 65, 1, ldx, off, True, 8, bias=False, ldy=OUT + 1)


@pytest.mark.parametrize("IN,OUT,ldx,off", [(65, 5, 65, 0), (130, 130, 132, 2), (256, 256, 256, 0)])
def test_linear_fwd_wide_form(IN, OUT, ldx, off):
    for n in (1, 65):
        for act in (0, 1, 2):
            check_fwd("wide", IN, OUT, n, act, ldx, off, False, 20 * n + act)
            if act != 2:
                check_fwd("wide exact", IN, OUT, n, act, ldx, off, True, 20 * n + act)
    check_fwd("wide", IN, OUT, 65, 2, ldx, off, False, 9, bias=False, ldy=OUT + 3, shift=1)


def test_linear_fwd_wide_form_second_tile_of_a_block():
    """1024 persistent tiles: at 1024 x 64 + 65 rows blocks 0 and 1 take a second tile and the last tile is ragged"""
    n = M.FWD_WIDE_TILES * 64 + 65
    check_fwd("wide second round", 65, 5, n, 2, 65, 0, False, 31)
    check_fwd("wide second round exact", 65, 5, n, 1, 65, 0, True, 32)


def test_linear_fwd_rows_form_second_grid_stride_round_bit_for_bit():
    """65536 blocks of 256 rows: row 65536 x 256 is block 0's second round.  Exact integers: y = relu(2 x + 1)"""
    n = M.FWD_ROWS_BLOCKS * 256 + 1
    x = (torch.arange(n, device=DEV, dtype=torch.int32) % 7 - 3).to(torch.float32).reshape(n, 1).contiguous()
    y = torch.full((n + 2, 1), float(SENT), device=DEV)
    w, b = dev([[2.0]]), dev([1.0])
    lin = _hip.tn_linear(w.data_ptr(), b.data_ptr(), 1, 1)
    _hip.check(_hip.load().tn_linear_fwd(x.data_ptr(), 1, C.byref(lin), M.ACT_RELU, n, y.data_ptr(), 1, _hip.current_stream()), "tn_linear_fwd")
    got, xs = host(y)[:, 0], host(x)[:, 0]
    same_bits("rows second round", got[:n], np.maximum(2.0 * xs.astype(f64) + 1.0, 0.0))
    assert np.all(got[n:] == SENT), "guard rows written"


# ----------------------------------------------------------------------------------------------------------------------
# tn_linear_bwd
# ----------------------------------------------------------------------------------------------------------------------
def run_bwd(c: M.LinearCase, ldx, off, shift=0, accumulate=False, want_dx=True, want_w=True, want_b=True, ws=True, expect=0):
    """-> (dx, dW, db) as numpy (None where not asked for); x is NULL when no weight gradient is asked for"""
    n, IN = c.x.shape
    OUT = c.W.shape[0]
    x = Mat(c.x, ldx, off, shift)
    y, dy = Mat(c.y, None, 0, shift), Mat(c.dy, None, 0, shift)
    dx = Mat(c.dx_held if accumulate else np.full((n, IN), SENT), ldx, off, shift, fill=SENT)
    w, b, dW, db = dev(c.W), dev(c.b), dev(c.dW_held), dev(c.db_held)
    lin = _hip.tn_linear(w.data_ptr(), b.data_ptr(), IN, OUT)
    wst, wsb = workspace("linear") if ws else (None, 0)
    code = _hip.load().tn_linear_bwd(x.ptr if (want_w or want_b) else None, x.ld, y.ptr, dy.ptr, y.ld, C.byref(lin), c.act, n,
                                     dx.ptr if want_dx else None, dx.ld, 1 if accumulate else 0, dW.data_ptr() if want_w else None,
                                     db.data_ptr() if want_b else None, wst.data_ptr() if ws else None, wsb, _hip.current_stream())
    assert code == expect, code
    return dx.read("dx"), host(dW), host(db)


def check_bwd(family, IN, OUT, n, act, ldx, off, exact, seed, **kw):
    c = (M.exact_linear_case if exact else M.linear_case)(IN, OUT, n, act, seed)
    acc, want_dx = kw.get("accumulate", False), kw.get("want_dx", True)
    want_w, want_b = kw.get("want_w", True), kw.get("want_b", True)
    ref = M.linear_adjoint(c.x, c.y, c.dy, c.W, act, want_dx, c.dx_held, acc, want_w, c.dW_held, want_b, c.db_held)
    dx, dW, db = run_bwd(c, ldx, off, **kw)
    tag = f"({IN},{OUT}) n={n} act={act} {kw or ''}"
    if want_dx:
        judge(exact, "tn_linear_bwd", family, f"dx {tag}", dx, ref.dx, ref.tol_dx, OUT + int(acc))
    else:
        assert np.all(dx == (c.dx_held if acc else SENT)), "dx written although NULL was passed"
    if want_w:
        judge(exact, "tn_linear_bwd", family, f"dW {tag}", dW, ref.dW, ref.tol_dW, n + 1)
    else:
        assert np.array_equal(dW, c.dW_held)
    if want_b:
        judge(exact, "tn_linear_bwd", family, f"db {tag}", db, ref.db, ref.tol_db, n + 1)
    else:
        assert np.array_equal(db, c.db_held)


BWD_VARIANTS = [dict(), dict(accumulate=True), dict(shift=1), dict(shift=1, accumulate=True), dict(want_dx=False),
                dict(want_w=False, want_b=False), dict(want_b=False), dict(want_w=False)]


@pytest.mark.parametrize("IN,OUT,ldx,off", ROWS_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_bwd_matrix_pipe_form(IN, OUT, ldx, off, act):
    """with the workspace.  (32,64) and (64,64) at shift 0 take the 16-byte loads (vec) and, without accumulate_dx, the 16-byte dx
    stores (vec_dx); with accumulate_dx the same aligned call must take the read-modify-write path; shift 1 takes neither"""
    for n in (1, 63, 64, 65, 129):
        for k, kw in enumerate(BWD_VARIANTS):
            check_bwd("mfma", IN, OUT, n, act, ldx, off, False, 100 * n + k, **kw)
            if act != 2:
                check_bwd("mfma exact", IN, OUT, n, act, ldx, off, True, 100 * n + k, **kw)


@pytest.mark.parametrize("IN,OUT,ldx,off", [(130, 130, 132, 2), (200, 1, 200, 0), (65, 5, 65, 0), (256, 256, 256, 0)])
def test_linear_bwd_wide_layer_by_64_blocks(IN, OUT, ldx, off):
    """dx of the second output block accumulates onto the first's; d_bias once per output block"""
    for n in (1, 65):
        for act in (0, 1, 2):
            for k, kw in enumerate([dict(), dict(accumulate=True), dict(want_w=False, want_b=False), dict(want_dx=False, shift=1)]):
                check_bwd("mfma wide", IN, OUT, n, act, ldx, off, False, 200 * n + k, **kw)
                if act != 2:
                    check_bwd("mfma wide exact", IN, OUT, n, act, ldx, off, True, 200 * n + k, **kw)


@pytest.mark.parametrize("IN,OUT,ldx,off", [(64, 64, 64, 0), (15, 64, 16, 1)])
def test_linear_bwd_matrix_pipe_form_second_tile_of_a_block(IN, OUT, ldx, off):
    """768 persistent blocks: at 768 x 64 + 65 rows blocks 0 and 1 carry accw / accb over to a second tile, the last one ragged"""
    n = M.LINEAR_SECOND_ROUND
    check_bwd("mfma second round", IN, OUT, n, 2, ldx, off, False, 41)
    check_bwd("mfma second round", IN, OUT, n, 1, ldx, off, False, 42, accumulate=True)
    check_bwd("mfma second round exact", IN, OUT, n, 1, ldx, off, True, 43)
    check_bwd("mfma second round exact", IN, OUT, n, 0, ldx, off, True, 44, accumulate=True, shift=1)


@pytest.mark.parametrize("IN", [10, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("OUT", [1, 16, 64])
def test_linear_bwd_valu_form_without_a_workspace(IN, OUT):
    """linear_bwd_kernel<4 | 8 | 16>: one atomic per block and weight entry"""
    for n in (1, 65):
        for act in (0, 1, 2):
            for k, kw in enumerate([dict(), dict(accumulate=True, shift=1), dict(want_b=False), dict(want_w=False), dict(want_dx=False)]):
                check_bwd("valu", IN, OUT, n, act, IN, 0, False, 300 * n + k, ws=False, **kw)
                if act != 2:
                    check_bwd("valu exact", IN, OUT, n, act, IN, 0, True, 300 * n + k, ws=False, **kw)


@pytest.mark.parametrize("IN,OUT", [(10, 16), (33, 64)])
def test_linear_bwd_valu_form_second_tile_of_a_block(IN, OUT):
    n = M.LINEAR_SECOND_ROUND
    check_bwd("valu second round", IN, OUT, n, 2, IN, 0, False, 51, ws=False)
    check_bwd("valu second round exact", IN, OUT, n, 1, IN, 0, True, 52, ws=False, accumulate=True)


def test_linear_bwd_wide_layer_without_a_workspace_is_refused_and_writes_nothing():
    c = M.linear_case(130, 16, 65, 1, 61)
    dx, dW, db = run_bwd(c, 130, 0, ws=False, expect=TN_ERR_WORKSPACE)
    assert np.all(dx == SENT) and np.array_equal(dW, c.dW_held) and np.array_equal(db, c.db_held)
    # without weight gradients it needs none
    check_bwd("mfma wide", 130, 16, 65, 1, 130, 0, False, 62, ws=False, want_w=False, want_b=False)


# ----------------------------------------------------------------------------------------------------------------------
# tn_linear_chain_bwd
# ----------------------------------------------------------------------------------------------------------------------
def run_chain(c: M.ChainCase, ldx, off, shift=0, accumulate=False, want_dx=True, skip_layer=None):
    """-> (dx, [(dW, db)]); skip_layer: that layer's two gradients are NULL"""
    nl = len(c.layers)
    n = c.dy.shape[0]
    keep, arr = [], (_hip.tn_chain_layer * nl)()
    grads = []
    for j, L in enumerate(c.layers):
        last = j == nl - 1
        x = Mat(L.x, ldx if last else None, off if last else 0, shift)
        w, b, dW, db = dev(L.W), dev(c.biases[j]), dev(L.dW_held), dev(L.db_held)
        keep += [x, w, b]
        grads.append((dW, db))
        OUT, IN = L.W.shape
        on = j != skip_layer
        arr[j] = _hip.tn_chain_layer(_hip.tn_linear(w.data_ptr(), b.data_ptr(), IN, OUT), x.ptr, x.ld, L.act_x,
                                     dW.data_ptr() if on else None, db.data_ptr() if on else None)
    IN_last = c.layers[-1].W.shape[1]
    dx = Mat(c.dx_held if accumulate else np.full((n, IN_last), SENT), ldx, off, shift, fill=SENT)
    dy = Mat(c.dy, None, 0, shift)
    yt = Mat(c.y_top, None, 0, shift) if c.y_top is not None else None
    wst, wsb = workspace("chain")
    _hip.check(_hip.load().tn_linear_chain_bwd(arr, nl, yt.ptr if yt else None, c.act_top, dy.ptr, dy.ld, n,
                                               dx.ptr if want_dx else None, dx.ld, 1 if accumulate else 0, wst.data_ptr(), wsb,
                                               _hip.current_stream()), "tn_linear_chain_bwd")
    out = dx.read("dx"), [(host(a), host(b)) for a, b in grads]
    del keep
    return out


def check_chain(family, name, n, act_top, exact, seed, **kw):
    spec, ldx, off = M.CHAINS[name]
    c = (M.exact_chain_case if exact else M.chain_case)(spec, n, seed, act_top)
    acc, want_dx, skip = kw.get("accumulate", False), kw.get("want_dx", True), kw.get("skip_layer")
    layers = [L._replace(want_w=j != skip, want_b=j != skip) for j, L in enumerate(c.layers)]
    ref = M.chain_adjoint(layers, c.y_top, c.act_top, c.dy, want_dx, c.dx_held, acc)
    dx, grads = run_chain(c, ldx, off, **kw)
    tag = f"{name} n={n} top={act_top} {kw or ''}"
    if want_dx:
        judge(exact, "tn_linear_chain_bwd", family, f"dx {tag}", dx, ref[-1].dx, ref[-1].tol_dx, layers[-1].W.shape[0] + int(acc))
    else:
        assert np.all(dx == (c.dx_held if acc else SENT)), "dx written although NULL was passed"
    for j, ((dW, db), a) in enumerate(zip(grads, ref)):
        if j == skip:
            assert np.array_equal(dW, c.layers[j].dW_held) and np.array_equal(db, c.layers[j].db_held), "a NULL layer's gradients written"
            continue
        judge(exact, "tn_linear_chain_bwd", family, f"dW[{j}] {tag}", dW, a.dW, a.tol_dW, n + 1)
        judge(exact, "tn_linear_chain_bwd", family, f"db[{j}] {tag}", db, a.db, a.tol_db, n + 1)


@pytest.mark.parametrize("name", list(M.CHAINS))
@pytest.mark.parametrize("act_top", [0, 2])
def test_linear_chain_bwd(name, act_top):
    nl = len(M.CHAINS[name][0])
    for n in M.CHAIN_N[:3]:
        for k, kw in enumerate([dict(), dict(accumulate=True), dict(shift=1), dict(want_dx=False), dict(skip_layer=0),
                                dict(skip_layer=nl - 1, accumulate=True, shift=1)]):
            check_chain("chain", name, n, act_top, False, 400 * n + k, **kw)
            check_chain("chain exact", name, n, act_top, True, 400 * n + k, **kw)


@pytest.mark.parametrize("name", list(M.CHAINS))
def test_linear_chain_bwd_second_tile_of_a_block(name):
    """512 persistent blocks: at 512 x 64 + 65 rows blocks 0 and 1 prefetch and run a second tile, the last one ragged"""
    n = M.CHAIN_N[3]
    check_chain("chain second round", name, n, 2, False, 71)
    check_chain("chain second round exact", name, n, 0, True, 17 + n)
    check_chain("chain second round exact", name, n, 2, True, 17 + n, accumulate=True)


# ----------------------------------------------------------------------------------------------------------------------
# the proposal network in one launch each way
# ----------------------------------------------------------------------------------------------------------------------
class Proposal:
    """a tn_density_field over a small hash grid (5 levels) holding the case's weights"""

    def __init__(self, c: M.DensityCase, table_scale=1.0):
        r = np.random.default_rng(99)
        self.table = dev(table_scale * r.uniform(-1, 1, (5 * 2 ** 12, 2)))
        self.w0, self.b0, self.w1, self.b1 = dev(c.w0), dev(c.b0), dev(c.w1), dev(c.b1)
        f = _hip.tn_density_field()
        f.grid.table = self.table.data_ptr()
        for i, s in enumerate((16.0, 26.0, 45.0, 76.0, 128.0)):
            f.grid.scalings[i] = s
        f.grid.num_levels, f.grid.log2_hashmap_size = 5, 12
        f.grid.dense = None
        f.l0 = _hip.tn_linear(self.w0.data_ptr(), self.b0.data_ptr(), M.PE, M.PH)
        f.l1 = _hip.tn_linear(self.w1.data_ptr(), self.b1.data_ptr(), M.PH, 1)
        f.space.contraction = 0
        for i in range(3):
            f.space.aabb_min[i], f.space.aabb_max[i] = -1.0, 1.0
        f.average_init_density = c.avg
        self.f = f


def run_density_bwd(c: M.DensityCase, clamp_min=-15.0):
    n = c.enc.shape[0]
    p = Proposal(c)
    enc, raw, sel, g = dev(c.enc), dev(c.raw), dev(c.selector), dev(c.d_density)
    d_enc = torch.full((n + 2, M.PE), float(SENT), device=DEV)
    held = {k: dev(v) for k, v in c.held.items()}
    _hip.check(_hip.load().tn_density_bwd_train(C.byref(p.f), enc.data_ptr(), raw.data_ptr(), sel.data_ptr(), g.data_ptr(), n, clamp_min,
                                                d_enc.data_ptr(), held["d_w0"].data_ptr(), held["d_b0"].data_ptr(),
                                                held["d_w1"].data_ptr(), held["d_b1"].data_ptr(), _hip.current_stream()),
               "tn_density_bwd_train")
    out = host(d_enc)
    assert np.all(out[n:] == SENT), "guard rows of d_enc written"
    return out[:n], {k: host(v) for k, v in held.items()}


@pytest.mark.parametrize("n", M.DENSITY_N)
def test_density_bwd_train(n):
    """512 blocks of 256 samples: the last size gives every block a second round and block 0 a third; rows with raw below -15 and
    above 15 (both clamps, and the one-sided form), rows with selector 0, the four parameter buffers already holding values"""
    for exact in (False, True):
        c = (M.exact_density_case if exact else M.density_case)(n, M.density_seed(n))
        for clamp_min in ((-15.0,) if exact else (-15.0, -np.inf)):
            ref = M.density_train_adjoint(c.enc, c.raw, c.selector, c.d_density, c.w0, c.b0, c.w1, c.avg, clamp_min, c.held)
            if not exact:
                assert ref.margin.min() > M.GATE_MARGIN
            d_enc, grads = run_density_bwd(c, clamp_min)
            fam = ("exact" if exact else "general") + (" second round" if n > M.DENSITY_BWD_BLOCKS * 256 else "")
            tag = f"n={n} clamp_min={clamp_min}"
            judge(exact, "tn_density_bwd_train", fam, f"d_enc {tag}", d_enc, ref.d_enc, ref.tol_enc, M.PH)
            for k, tol in (("d_w0", ref.tol_w0), ("d_b0", ref.tol_b0), ("d_w1", ref.tol_w1), ("d_b1", ref.tol_b1)):
                want = np.asarray(getattr(ref, k))
                judge(exact, "tn_density_bwd_train", fam, f"{k} {tag}", grads[k].reshape(want.shape), want, tol, n + 1)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 257])
def test_density_fwd_train_from_the_device_s_own_enc(n):
    """raw and density against the fp64 network over the enc and selector the SAME launch wrote (the encoding has its own tests);
    4096 blocks of 256: the last size is a second grid-stride round.  Positions beyond the box: selector 0 rows."""
    c = M.density_case(8, 3, avg=0.75)  # for its weights
    p = Proposal(c)
    r = np.random.default_rng(n)
    pos = dev(r.uniform(-1.25, 1.25, (n, 3)))
    enc = torch.full((n + 2, M.PE), float(SENT), device=DEV)
    sel, raw, den = (torch.full((n + 2,), float(SENT), device=DEV) for _ in range(3))
    _hip.check(_hip.load().tn_density_fwd_train(C.byref(p.f), pos.data_ptr(), n, enc.data_ptr(), sel.data_ptr(), raw.data_ptr(),
                                                den.data_ptr(), _hip.current_stream()), "tn_density_fwd_train")
    enc, sel, raw, den = host(enc), host(sel), host(raw), host(den)
    for a in (enc, sel, raw, den):
        assert np.all(a[n:] == SENT), "guard rows written"
    enc, sel, raw, den = enc[:n], sel[:n], raw[:n], den[:n]
    assert np.all((sel == 0) | (sel == 1))
    ref = M.density_train_forward(enc, sel, c.w0, c.b0, c.w1, c.b1, c.avg)
    fam = "second round" if n > 4096 * 256 else "general"
    within("tn_density_fwd_train", fam, f"raw n={n}", raw, ref.raw, ref.tol_raw, M.PH + 1)
    within("tn_density_fwd_train", fam, f"density n={n}", den, ref.density, ref.tol_density, M.PH + 1)
    if n > 4096:
        assert (sel == 0).any() and (sel == 1).any() and np.abs(enc).max() > 0.1 and np.ptp(ref.raw) > 0.1


# ----------------------------------------------------------------------------------------------------------------------
# mlp_head.0's ray-constant part
# ----------------------------------------------------------------------------------------------------------------------
class FieldStruct:
    """a tn_thermal_field of the reference geometry over given weights (name -> (weight, bias)); what is not given is zeros"""
    SHAPES = dict(base0=(64, 32), base1=(16, 64), head0=(64, M.IN0), head1=(64, 64), head2=(3, 64), th0=(64, M.GF), th1=(64, 64),
                  thead=(1, 64))

    def __init__(self, weights, emb, sh_shifted=0, avg=1.0):
        self.keep = {}
        f = _hip.tn_thermal_field()
        self.table = torch.zeros((16 * 2 ** 4, 2), device=DEV)
        f.grid.table = self.table.data_ptr()
        f.grid.num_levels, f.grid.log2_hashmap_size = 16, 4
        for i in range(16):
            f.grid.scalings[i] = 16.0 + i
        for name, (o, i) in self.SHAPES.items():
            w, b = weights.get(name, (np.zeros((o, i), f32), np.zeros(o, f32)))
            wd, bd = dev(np.asarray(w, f32).reshape(o, i)), dev(np.asarray(b, f32).reshape(o))
            self.keep[name] = (wd, bd)
            setattr(f, name, _hip.tn_linear(wd.data_ptr(), bd.data_ptr(), i, o))
        self.emb = dev(emb)
        f.appearance = self.emb.data_ptr()
        f.num_images, f.app_dim, f.geo_feat_dim, f.sh_shifted = emb.shape[0], M.APP, M.GF, sh_shifted
        f.space.contraction = 1
        f.average_init_density = avg
        self.f = f


@pytest.mark.parametrize("R", [1, 5, 2049])
@pytest.mark.parametrize("shifted", [0, 1])
def test_ray_head_fwd(R, shifted):
    """512 blocks of 4 rays: 2049 gives block 0 a second round; a camera index without an embedding row poisons its ray"""
    c = M.ray_head_case(R, 80 + R, bad_cams=R > 1)
    fs = FieldStruct(dict(head0=(c.W0, c.b0)), c.emb, shifted)
    d, cams = dev(c.directions), torch.from_numpy(c.cams).to(DEV)
    out = torch.full((R + 2, 64), float(SENT), device=DEV)
    _hip.check(_hip.load().tn_ray_head_fwd(C.byref(fs.f), d.data_ptr(), cams.data_ptr(), R, out.data_ptr(), _hip.current_stream()),
               "tn_ray_head_fwd")
    got = host(out)
    assert np.all(got[R:] == SENT), "guard rows written"
    ref, tol, _ = M.ray_head_forward(c.W0, c.b0, c.emb, c.directions, c.cams, bool(shifted))
    ok = ~np.isnan(ref[:, 0])
    assert np.all(np.isnan(got[:R][~ok])), "a ray without an embedding row must be poisoned"
    within("tn_ray_head_fwd", "general", f"ray_bias R={R} shifted={shifted}", got[:R][ok], ref[ok], tol[ok], M.RH_IN + 1)


def run_ray_head_bwd(c: M.RayHeadCase, shifted=0, want_b=True, want_emb=True, want_x=True):
    R = c.g.shape[0]
    fs = FieldStruct(dict(head0=(c.W0, c.b0)), c.emb, shifted)
    d, cams, g = dev(c.directions), torch.from_numpy(c.cams).to(DEV), dev(c.g)
    d_w, d_b, d_emb = dev(c.held_w), dev(c.held_b), dev(c.held_emb)
    d_x = torch.full((R + 2, 64), float(SENT), device=DEV)
    _hip.check(_hip.load().tn_ray_head_bwd(C.byref(fs.f), d.data_ptr(), cams.data_ptr(), R, g.data_ptr(), d_w.data_ptr(),
                                           d_b.data_ptr() if want_b else None, d_emb.data_ptr() if want_emb else None,
                                           d_x.data_ptr() if want_x else None, _hip.current_stream()), "tn_ray_head_bwd")
    return dict(d_w=host(d_w), d_b=host(d_b), d_emb=host(d_emb), d_x=host(d_x))


def check_ray_head_bwd(R, seed, exact, shifted=0, **kw):
    c = M.ray_head_case(R, seed, bad_cams=R > 1, exact=exact)
    a = M.ray_head_adjoint(c.W0, c.emb, c.directions, c.cams, c.g, bool(shifted), c.held_w, c.held_b, c.held_emb)
    got = run_ray_head_bwd(c, shifted, **kw)
    fam = ("exact" if exact else "general") + (" second round" if R > M.RAY_HEAD_BWD_BLOCKS * 64 else "")
    tag = f"R={R} shifted={shifted} {kw or ''}"
    geo, app = slice(16, 16 + M.GF), slice(16 + M.GF, M.IN0)
    assert np.array_equal(got["d_w"][:, geo], c.held_w[:, geo]), "the geo columns of d_head0_weight belong to tn_field_bwd_fused"
    within("tn_ray_head_bwd", fam, f"d_w SH columns {tag}", got["d_w"][:, :16], a.d_w[:, :16], a.tol_w[:, :16], R + 1)
    judge(exact, "tn_ray_head_bwd", fam, f"d_w appearance columns {tag}", got["d_w"][:, app], a.d_w[:, app], a.tol_w[:, app], R + 1)
    if kw.get("want_b", True):
        judge(exact, "tn_ray_head_bwd", fam, f"d_b {tag}", got["d_b"], a.d_b, a.tol_b, R + 1)
    else:
        assert np.array_equal(got["d_b"], c.held_b)
    if kw.get("want_emb", True):
        judge(exact, "tn_ray_head_bwd", fam, f"d_emb {tag}", got["d_emb"], a.d_emb, a.tol_emb, int(a.ok.sum()) + 1)
    else:
        assert np.array_equal(got["d_emb"], c.held_emb)
    dx = got["d_x"]
    assert np.all(dx[R:] == SENT) and np.all(dx[:R, 16:] == SENT) and np.all(dx[:R][~a.ok] == SENT), "d_ray_inputs written outside the SH columns of the live rays"
    if kw.get("want_x", True):
        judge(exact, "tn_ray_head_bwd", fam, f"d_x {tag}", dx[:R, :16][a.ok], a.d_x[a.ok], a.tol_x[a.ok], 64)
    else:
        assert np.all(dx == SENT)


@pytest.mark.parametrize("R", [1, 65, M.RAY_HEAD_BWD_BLOCKS * 64 + 65])
def test_ray_head_bwd(R):
    """256 persistent blocks of 64 rays: the last size gives blocks 0 and 1 a second batch, the last one ragged.  Rays whose camera
    index is out of range are skipped, as the kernel documents: no gradient from them, no row of d_ray_inputs"""
    for exact in (False, True):
        check_ray_head_bwd(R, 90 + R, exact)
        check_ray_head_bwd(R, 91 + R, exact, shifted=1)
    if R == 65:
        check_ray_head_bwd(R, 92, False, want_b=False)
        check_ray_head_bwd(R, 93, True, want_emb=False, want_x=False)


# ----------------------------------------------------------------------------------------------------------------------
# tn_field_bwd_fused
# ----------------------------------------------------------------------------------------------------------------------
def run_field_bwd(c: M.FieldCase, split, stored, pass_thermal=1, clamp_min=-15.0, want_rgb=True, want_thermal=True):
    """-> (d_enc [N, 32], d_ray_sum [R, 64], {name: gradient}); d_enc pre-filled with the sentinel, guard rows behind N and R"""
    N, S = c.enc.shape[0], c.S
    R = N // S
    w = c.w
    pairs = {k: (w[k + "_w"], w.get(k + "_b", np.zeros(M.FIELD_SHAPES[k + "_w"][0], f32)))
             for k in ("base0", "base1", "head0", "head1", "head2", "th0", "th1", "thead")}
    fs = FieldStruct(pairs, np.zeros((1, M.APP), f32), 0, c.avg)
    lib = _hip.load()
    enc, sel, bo, rb, rgb = dev(M.enc_tiles(c.enc)), dev(c.selector), dev(c.base_out), dev(c.ray_bias), dev(c.rgb)
    g_rgb, g_th, g_d = dev(c.d_rgb), dev(c.d_thermal), dev(c.d_density)
    d_enc = torch.full((N + 2, 32), float(SENT), device=DEV)
    d_ray = torch.full((R + 2, 64), float(SENT), device=DEV)
    d_ray[:R] = dev(c.held_ray_sum)
    held = {k: dev(c.held[k]) for k in M.FIELD_PARAMS}
    gr = _hip.tn_field_grads()
    for k in M.FIELD_PARAMS:
        setattr(gr, k, held[k].data_ptr())
    nbytes = lib.tn_field_bwd_fused_workspace_bytes(R, S)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)  # NaN bit patterns: a slab entry read before it was written shows
    _hip.check(lib.tn_field_bwd_fused(C.byref(fs.f), R, S, enc.data_ptr(), sel.data_ptr(), bo.data_ptr() if stored else None, rb.data_ptr(),
                                      rgb.data_ptr(), g_rgb.data_ptr() if want_rgb else None, g_th.data_ptr() if want_thermal else None,
                                      g_d.data_ptr(), pass_thermal, clamp_min, split, d_enc.data_ptr(), d_ray.data_ptr(), None, None, None,
                                      C.byref(gr), ws.data_ptr(), nbytes, _hip.current_stream()), "tn_field_bwd_fused")
    de, dr = host(d_enc), host(d_ray)
    assert np.all(de[N:] == SENT) and np.all(dr[R:] == SENT), "guard rows written"
    return de[:N], dr[:R], {k: host(v) for k, v in held.items()}


FIELD_FORMS = [(0, False), (1, False), (1, True), (2, False), (2, True), (0, True)]


def check_field(c, exact, split, stored, tag, **kw):
    a = M.field_adjoint(c, split, stored, **kw)
    d_enc, d_ray, grads = run_field_bwd(c, split, stored, **kw)
    N = c.enc.shape[0]
    fam = f"split={split} stored={int(stored)}" + (" exact" if exact else "") + (" second round" if N > 32768 else "")
    judge(exact, "tn_field_bwd_fused", fam, f"d_enc {tag}", d_enc, a.d_enc, a.tol_enc, 64)
    judge(exact, "tn_field_bwd_fused", fam, f"d_ray_sum {tag}", d_ray, a.d_ray_sum, a.tol_ray_sum, c.S + 1)
    for k in M.FIELD_PARAMS:
        judge(exact, "tn_field_bwd_fused", fam, f"{k} {tag}", grads[k].reshape(M.FIELD_SHAPES[k]), a.grads[k], a.tols[k], N + 1)
    if not kw.get("want_rgb", True):
        assert np.array_equal(d_ray, c.held_ray_sum) and all(np.array_equal(grads[k], c.held[k]) for k in ("head0_w", "head1_w", "head1_b", "head2_w", "head2_b"))
    if not kw.get("want_thermal", True):
        assert all(np.array_equal(grads[k], c.held[k]) for k in ("th0_w", "th0_b", "th1_w", "th1_b", "thead_w", "thead_b"))
    geo = np.ones(M.IN0, bool)
    geo[16:16 + M.GF] = False
    assert np.array_equal(grads["head0_w"][:, geo], c.held["head0_w"][:, geo]), "head0_w: only the geo columns 16..30 belong to this kernel"


FIELD_RS = [(1, 1), (1, 15), (1, 17), (3, 5), (7, 23)]


@pytest.mark.parametrize("split,stored", FIELD_FORMS)
def test_field_bwd_fused_small_shapes(split, stored):
    """ragged tiles of 16 samples, rays that cross tile boundaries (their per-ray sums meet by atomics); rows with the raw density
    beyond both clamps and rows with selector 0 are in the (7, 23) case"""
    for R, S in FIELD_RS:
        c = M.field_case(R, S, 100 * R + S)
        check_field(c, False, split, stored, f"R={R} S={S}")
        e = M.exact_field_case(R, S, 100 * R + S)
        check_field(e, True, split, stored, f"R={R} S={S}", want_thermal=False)
    c = M.field_case(7, 23, 723)
    check_field(c, False, split, stored, "R=7 S=23 pass_thermal=0", pass_thermal=0)
    check_field(c, False, split, stored, "R=7 S=23 d_rgb NULL", want_rgb=False)
    check_field(c, False, split, stored, "R=7 S=23 d_thermal NULL", want_thermal=False)
    check_field(c, False, split, stored, "R=7 S=23 one-sided clamp", clamp_min=-np.inf)


@pytest.mark.parametrize("split,stored", FIELD_FORMS)
def test_field_bwd_fused_beyond_one_round(split, stored):
    """(1929, 17) = 32 793 samples: the split form's 256 blocks x 8 waves x 16 samples = 32 768 leave a second round of one full tile
    and one of 9 samples; in the one-launch form (4 waves) it is a third round"""
    c = M.field_case(1929, 17, 1929)
    check_field(c, False, split, stored, "R=1929 S=17")
    e = M.exact_field_case(1929, 17, 1930)
    check_field(e, True, split, stored, "R=1929 S=17", want_thermal=False)
