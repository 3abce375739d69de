"""tests/position_gradient_reference.py against torch's fp64 autograd, its case builders against what they claim, and the fp32
restatements of the kernels' arithmetic against the tolerance tests/test_gpu_position_gradient.py uses (no device)."""
from __future__ import annotations

import collections

import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import position_gradient_reference as R

L, LOG2T = 16, 15
SCAL = H.hash_scalings(L, 16, 2048)
SCALINGS = [float(s) for s in SCAL.tolist()]
BOX = np.array([[-1.5, -0.5, 0.25], [1.0, 2.0, 0.75]], dtype=np.float32)


@pytest.fixture(scope="module")
def table():
    return (torch.rand(L << LOG2T, 2, generator=torch.Generator().manual_seed(3)) * 2 - 1).numpy()


def _ratio(got, want, B):
    """worst |got - want| / (eps32 B) over the entries with B > 0; entries with B == 0 must agree to 1e-30"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert np.all(err[B == 0] <= 1e-30)
    return float((err[B > 0] / (R.EPS32 * B[B > 0])).max()) if (B > 0).any() else 0.0


def test_frozen_gradient_equals_fp64_autograd_on_dyadic_positions(table):
    """positions j / 4096: p * s is exact in both precisions, so the frozen cell IS the fp64 cell and the reference must equal
    torch's autograd through H.hash_encode.  Measured worst 4e-9 eps32 B; bound: one order above."""
    cases = R.dyadic(20000)
    rng = np.random.default_rng(5)
    d_enc = rng.standard_normal((len(cases), 2 * L))
    p = torch.from_numpy(cases.positions).double().requires_grad_(True)
    enc = H.hash_encode(p, torch.from_numpy(table).double(), SCAL.double(), LOG2T)
    enc.backward(torch.from_numpy(d_enc))
    g, B = R.frozen_gradient(cases.positions, d_enc, table, SCALINGS, LOG2T)
    on_plane = sum(int((fl == ce).sum()) for fl, ce, _ in (R.frozen_cell(cases.positions, s) for s in SCALINGS))
    worst = _ratio(p.grad.numpy(), g, B)
    print(f"frozen-cell reference vs fp64 autograd: worst {worst:.2e} eps32 B, scale {np.abs(g).max():.3g}, {on_plane} on-plane triples")
    assert on_plane >= 300
    assert worst <= 4e-8
    # the features too
    for l in (0, 7, 15):
        f, Bf = R.frozen_features(cases.positions, table, SCALINGS[l], l, LOG2T)
        assert _ratio(enc.detach().numpy()[:, 2 * l:2 * l + 2], f, Bf) <= 4e-8


def _autograd_chain(x32, g_p, space):
    cfg, aabb = space.oracle_args()
    x = torch.from_numpy(x32).double().requires_grad_(True)
    p, sel = H.normalized_positions(x, cfg, None if aabb is None else aabb.double())
    p.backward(torch.from_numpy(g_p))
    return x.grad.numpy(), sel.numpy()


def test_chain_equals_fp64_autograd_at_the_kinks_and_pins_the_tie_rule():
    cases = R.contraction_kinks()
    rng = np.random.default_rng(6)
    g_p = rng.standard_normal((len(cases), 3))
    B_p = np.abs(g_p)
    want, sel64 = _autograd_chain(cases.positions, g_p, R.CONTRACTION)
    got, B = R.position_chain_gradient(cases.positions, g_p, B_p, R.CONTRACTION)
    # the selector is the fp32 oracle's: at 2^25 fp32 rounds 2 - 1/m to 2 (p == 1 or 0: outside), fp64 does not — the only kinks
    # on which the two precisions select differently, and there the reference is zero (asserted below)
    s0 = cases.where("kink:sel0")
    differ = np.nonzero(sel64 != R.normalized(cases.positions, R.CONTRACTION)[1])[0]
    assert np.array_equal(differ, s0)
    want[s0] = 0.0
    origin = cases.where("kink:origin")
    assert len(origin) == 1
    # the origin: torch differentiates the unselected branch too, 0 x d (x / 0) = NaN; the reference (like the kernels) takes the
    # identity branch
    assert np.isnan(want[origin]).all()
    assert np.array_equal(got[origin], g_p[origin] / 4.0)
    rest = np.setdiff1d(np.arange(len(cases)), origin)
    worst = _ratio(want[rest], got[rest], B[rest])
    print(f"chain reference vs fp64 autograd at the kinks: worst {worst:.2e} eps32 B")
    assert worst <= 1e-6  # fp64 against fp64: 2^-53 / 2^-24 = 2e-9 per rounding
    # the tie rule itself, spelled out on one case: (2, -2, 2) with g = (1, 0, 0) / 4: s = 3/4, s' = -1/4, dot = 2 / 4
    x = np.array([[2.0, -2.0, 2.0]], dtype=np.float32)
    got1, _ = R.position_chain_gradient(x, np.array([[1.0, 0.0, 0.0]]), np.ones((1, 3)), R.CONTRACTION)
    share = -0.25 * 0.5 / 3.0
    assert np.allclose(got1, [[0.75 / 4 + share, -share, share]], rtol=0, atol=1e-15)
    # selector 0: exactly zero, and zero bound
    # (s0 from above)
    assert len(s0) == 2 and np.all(got[s0] == 0.0) and np.all(B[s0] == 0.0)


@pytest.mark.parametrize("aabb", [R.UNIT_BOX.aabb, BOX])
def test_chain_equals_fp64_autograd_on_the_box_faces(aabb):
    space = R.Space(False, aabb)
    cases = R.box_faces(aabb)
    g_p = np.random.default_rng(7).standard_normal((len(cases), 3))
    got, B = R.position_chain_gradient(cases.positions, g_p, np.abs(g_p), space)
    p32, sel32 = R.normalized(cases.positions, space)
    # fp64 autograd with the fp32 oracle's selector (one ulp inside a face is inside in both; on it and outside are out in both)
    want, sel64 = _autograd_chain(cases.positions, g_p, space)
    assert np.array_equal(sel64, sel32)
    assert _ratio(want, got, B) <= 1e-6
    for i, label in enumerate(cases.labels):
        assert bool(sel32[i]) == label.endswith(":inside"), label
        if label.endswith(":on"):
            axis, side = "xyz".index(label[5]), label[6:9]
            # p is exactly 0 or 1 on a face (then multiplied by the selector: 0)
            raw = (cases.positions[i, axis] - aabb[0][axis]) / (aabb[1][axis] - aabb[0][axis])
            assert raw == (0.0 if side == "min" else 1.0)
        if not sel32[i]:
            assert np.all(got[i] == 0.0)


def test_builders_produce_what_they_claim():
    for contraction in (False, True):
        space = R.CONTRACTION if contraction else R.UNIT_BOX
        cases = R.on_planes(SCALINGS, range(L), contraction=contraction)
        count = collections.Counter(l.rsplit(":", 1)[1] for l in cases.labels)
        assert count == {"on": L * 4 * 3, "below": L * 4 * 3, "above": L * 4 * 3}, count  # 16 levels x 4 planes x 3 axis sets
        p32, sel = R.normalized(cases.positions, space)
        assert sel.all()
        for i in range(0, len(cases), 3):
            _, lvl, axes, name = cases.labels[i].split(":")
            assert name == "on" and cases.labels[i + 1].endswith("below") and cases.labels[i + 2].endswith("above")
            s = np.float32(SCALINGS[int(lvl[1:])])
            ax = ["xyz".index(a) for a in axes]
            sx = (p32[i:i + 3, ax] * s).astype(np.float32)
            k = sx[0]
            assert np.all(k == np.round(k)) and np.all(k >= 1)                      # fl32(p s) == k: on the plane
            assert np.all(sx[1] < k) and np.all(np.floor(sx[1]) == k - 1)             # one ulp below: the cell under it
            assert np.all(sx[2] > k) and np.all(np.floor(sx[2]) == k)                 # one ulp above: the cell over it
            assert np.all(p32[i + 1, ax] == np.nextafter(p32[i, ax], np.float32(-1))) and np.all(p32[i + 2, ax] == np.nextafter(p32[i, ax], np.float32(2)))
            fl, ce, off = R.frozen_cell(p32[i:i + 1], s)
            assert np.all(fl[0, ax] == ce[0, ax]) and np.all(off[0, ax] == 0.0)
    kinks = collections.Counter(l.split(":")[1] for l in R.contraction_kinks().labels)
    assert kinks == {"below1": 3, "at1": 4, "above1": 3, "single": 3, "tie2": 4, "tie3": 3, "far": 3, "sel0": 2, "origin": 1}, kinks
    k = R.contraction_kinks()
    mag = np.abs(k.positions).max(axis=1)
    for i, label in enumerate(k.labels):
        ties = int((np.abs(k.positions[i]) == mag[i]).sum())
        if "tie2" in label or "tie3" in label:
            assert ties == int(label[label.index("tie") + 3]), label
        elif label != "kink:origin" and not label.endswith(":tie"):
            assert ties == 1 or "2^25" in label, label
    assert np.all(mag[k.where("kink:below1")] < 1) and np.all(mag[k.where("kink:at1")] == 1) and np.all(mag[k.where("kink:above1")] > 1)
    assert not R.normalized(k.positions, R.CONTRACTION)[1][k.where("kink:sel0")].any()
    assert len(R.box_faces(BOX)) == 18 and collections.Counter(l.rsplit(":", 1)[1] for l in R.box_faces(BOX).labels) == {"on": 6, "inside": 6, "outside": 6}
    d = R.dyadic(1000)
    assert np.array_equal(d.positions * 4096, np.round(d.positions * 4096)) and d.positions.min() > 0 and d.positions.max() < 1
    u = R.uniform(1000, 4, 3.0)
    assert u.positions.dtype == np.float32 and np.abs(u.positions).max() <= 3.0 and np.abs(u.positions).max() > 2.5
    mixed = R.shuffled(R.concat(k, d), seed=1, n=175)
    assert len(mixed) == 175 and mixed.positions.shape == (175, 3)


@pytest.mark.parametrize("contraction", [False, True])
def test_fp32_restatement_of_the_kernels_stays_inside_the_device_tolerance(table, contraction):
    """the condition the reference passes alone: numpy float32 restatements of encode_level_grad, hash_blend_jac and
    position_grad_finish against the fp64 reference under the counted K of the device test, on every builder's cases"""
    space = R.CONTRACTION if contraction else R.UNIT_BOX
    cases = R.mixed_cases(SCALINGS, contraction)
    p32, sel = R.normalized(cases.positions, space)
    d_enc = np.random.default_rng(11).standard_normal((len(cases), 2 * L)).astype(np.float32)
    d_enc[::7] = 0.0
    g32 = np.zeros((len(cases), 3), dtype=np.float32)
    gj32 = np.zeros((len(cases), 3), dtype=np.float32)
    worst_level = worst_jac = worst_jac_shared = 0.0
    for l, s in enumerate(SCALINGS):
        gl, Bl = R.frozen_level_gradient(p32, d_enc[:, 2 * l:2 * l + 2], table, s, l, LOG2T)
        k32 = R.kernel_level_gradient_fp32(p32, d_enc[:, 2 * l:2 * l + 2], table, s, l, LOG2T)
        worst_level = max(worst_level, _ratio(k32, gl, Bl))
        g32 += k32
        jac = R.kernel_level_jacobian_fp32(p32, table, s, l, LOG2T)
        shared = R.kernel_level_jacobian_shared_differences_fp32(p32, table, s, l, LOG2T)
        for ch in range(2):
            one = np.zeros((len(cases), 2))
            one[:, ch] = 1.0
            gj, Bj = R.frozen_level_gradient(p32, one, table, s, l, LOG2T)
            worst_jac = max(worst_jac, _ratio(jac[:, :, ch], gj, Bj))
            worst_jac_shared = max(worst_jac_shared, _ratio(shared[:, :, ch], gj, Bj))
            for c in range(3):
                gj32[:, c] = R._fma32(d_enc[:, 2 * l + ch], jac[:, c, ch], gj32[:, c])
    g, B = R.frozen_gradient(p32, d_enc, table, SCALINGS, LOG2T)
    g_x, B_x = R.position_chain_gradient(cases.positions, g, B, space)
    worst_sum = _ratio(R.kernel_chain_fp32(cases.positions, g32, space), g_x, B_x)
    worst_sum_jac = _ratio(R.kernel_chain_fp32(cases.positions, gj32, space), g_x, B_x)
    print(f"fp32 restatement, contraction={contraction}: per level {worst_level:.2f} (K {R.K_LEVEL}), Jacobian entries {worst_jac:.2f} "
          f"(K {R.K_JACOBIAN_TENSOR}; from the feature lerp's differences: {worst_jac_shared:.2f}), world gradient {worst_sum:.2f} "
          f"(K {R.K_BWD_INPUT}), from the Jacobian {worst_sum_jac:.2f} (K {R.K_FUSED_JACOBIAN}) eps32 B")
    assert worst_level <= R.K_LEVEL
    assert worst_jac <= R.K_JACOBIAN_TENSOR
    # what the bound separates: slopes taken from the differences of the feature lerp b + o (a - b) round (a - b) with weight o on
    # BOTH corners, while B weighs the floor corner b with 1 - o; towards o = 1 (one ulp below a plane above all) single entries
    # leave K eps B (10.6 and 6.3 on these cases).  hash_blend_jac had that form; its slopes now interpolate as o a + (1 - o) b.
    assert worst_jac_shared > R.K_JACOBIAN_TENSOR
    assert worst_sum <= R.K_BWD_INPUT - 1 and worst_sum_jac <= R.K_FUSED_JACOBIAN
    # the restatement really is another evaluation, and B is no loose bound: some sample sits within two orders of it
    assert worst_level > 0.05


def test_frustum_adjoint():
    rng = np.random.default_rng(12)
    g, s = rng.standard_normal((3, 5, 3)), rng.random((3, 5))
    e = s + 0.1
    d_o, d_d, B_o, B_d = R.frustum_positions_adjoint(g, s, e)
    o = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    d = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    pos = o[:, None, :] + d[:, None, :] * ((torch.from_numpy(s) + torch.from_numpy(e)) / 2)[..., None]
    pos.backward(torch.from_numpy(g))
    assert np.allclose(o.grad.numpy(), d_o, rtol=0, atol=1e-14) and np.allclose(d.grad.numpy(), d_d, rtol=0, atol=1e-14)
    assert np.all(B_o >= np.abs(d_o)) and np.all(B_d >= np.abs(d_d))
    assert R.frustum_roundings(1) == (7, 9) and R.frustum_roundings(65) == (8, 10) and R.frustum_roundings(1024) == (22, 24)
