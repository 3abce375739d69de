"""tests/table_gradient_reference.py against torch's fp64 autograd and against hand-computed samples, and its exact-sum builders
against what they claim: every case meets its own exactness condition, and a sequential fp32 sum of its contributions gives the
bits of the fp64 sum in whatever order (no device)."""
import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import position_gradient_reference as P
from tests import table_gradient_reference as R

GRIDS = [(16, 15, 2048), (5, 13, 128), (8, 12, 512), (1, 4, 16)]


def _hash(x, y, z, T):
    return (x ^ (y * 2654435761) ^ (z * 805459861)) % T


@pytest.mark.parametrize("L,log2T,max_res", GRIDS)
def test_reference_against_fp64_autograd_on_dyadic_positions(L, log2T, max_res):
    """on dyadic positions the fp32 and the fp64 cell agree (p * s is exact in both): autograd through the oracle's encoding in
    fp64 is the same sum; 1e-12 relative to B"""
    scal = H.hash_scalings(L, 16, max_res)
    cases = P.dyadic(400, bits=10, seed=L)
    p32, sel = P.normalized(cases.positions, P.UNIT_BOX)
    assert sel.all()
    rng = np.random.default_rng(L)
    d_enc = rng.standard_normal((len(cases), 2 * L))
    d_enc[rng.random(len(cases)) < 0.2] = 0.0
    table = torch.zeros(L << log2T, 2, dtype=torch.float64, requires_grad=True)
    enc = H.hash_encode(torch.from_numpy(p32).double(), table, scal.double(), log2T)
    enc.backward(torch.from_numpy(d_enc))
    g, B, m = R.frozen_table_gradient(p32, d_enc, [float(s) for s in scal.tolist()], log2T)
    assert g.shape == B.shape == m.shape == (L << log2T, 2) and m.dtype == np.int64
    assert (np.abs(g - table.grad.numpy()) <= 1e-12 * B).all() and np.abs(g).max() > 0
    # m and B are consistent with g
    assert (np.abs(g) <= B * (1 + 1e-15)).all()
    assert ((m == 0) == (B == 0)).all() and not g[m == 0].any()
    one = (m == 1)
    assert (one.any() or log2T == 4) and np.array_equal(np.abs(g[one]), B[one])  # (16 entries: every one is crowded)
    # a level range: the same rows, zero elsewhere
    if L >= 5:
        T = 1 << log2T
        g2, B2, m2 = R.frozen_table_gradient(p32, d_enc, [float(s) for s in scal.tolist()], log2T, 1, 3)
        assert np.array_equal(g2[T:3 * T], g[T:3 * T]) and np.array_equal(m2[T:3 * T], m[T:3 * T])
        assert not g2[:T].any() and not g2[3 * T:].any() and not m2[:T].any() and not B2[3 * T:].any()


def _one(p, d, scale, log2T):
    """(g, B, m) [T, 2] of one sample on a one-level grid"""
    return R.frozen_table_gradient(np.array([p], dtype=np.float32), np.array([d], dtype=np.float32), [scale], log2T)


def test_hand_computed_interior_sample():
    """s = 16, p = (2.25, 5.5, 9.75) / 16: floor (2, 5, 9), offsets (1/4, 1/2, 3/4); eight different entries at T = 2^15"""
    T = 1 << 15
    g, B, m = _one((2.25 / 16, 5.5 / 16, 9.75 / 16), (2.0, -3.0), 16.0, 15)
    ox, oy, oz = 0.25, 0.5, 0.75
    want = np.zeros((T, 2))
    for bx, wx in ((1, ox), (0, 1 - ox)):
        for by, wy in ((1, oy), (0, 1 - oy)):
            for bz, wz in ((1, oz), (0, 1 - oz)):
                want[_hash(2 + bx, 5 + by, 9 + bz, T)] += wx * wy * wz * np.array([2.0, -3.0])
    assert np.array_equal(g, want) and np.array_equal(B, np.abs(want))
    assert int(m.sum()) == 16 and m.max() == 1
    assert np.allclose(g.sum(axis=0), [2.0, -3.0], rtol=0, atol=1e-15)  # the weights sum to 1
    assert g[_hash(3, 6, 10, T), 0] == 2.0 * 0.25 * 0.5 * 0.75           # the ceil corner carries ox oy oz


@pytest.mark.parametrize("axes", [(0,), (1, 2), (0, 1, 2)], ids=["x", "yz", "xyz"])
def test_hand_computed_sample_on_planes(axes):
    """on a plane ceil == floor: both corners of the axis are ONE entry, with the weights 0 (ceil side: o = 0) and 1"""
    T = 1 << 15
    s = [2.25, 5.5, 9.75]
    for a in axes:
        s[a] = float(int(s[a]))
    g, B, m = _one(tuple(v / 16 for v in s), (1.0, 4.0), 16.0, 15)
    want = np.zeros((T, 2))
    ranges = [((int(v), 1.0),) if v == int(v) else ((int(v) + 1, v - int(v)), (int(v), 1 - (v - int(v)))) for v in s]
    for x, wx in ranges[0]:
        for y, wy in ranges[1]:
            for z, wz in ranges[2]:
                want[_hash(x, y, z, T)] += wx * wy * wz * np.array([1.0, 4.0])
    assert np.array_equal(g, want)
    assert int((m > 0).sum()) == 2 * 2 ** (3 - len(axes)) and m.max() == 1  # zero-weight terms are not counted
    if len(axes) == 3:
        assert np.array_equal(g[_hash(2, 5, 9, T)], [1.0, 4.0])


def test_hand_computed_selector_zero_sample():
    """outside the box the selector zeroes p: the whole d_enc lands on entry hash(0, 0, 0) = 0 of every level"""
    scal = [16.0, 32.0, 64.0]
    for space, x in ((P.UNIT_BOX, (1.5, 0.5, 0.5)), (P.UNIT_BOX, (0.5, 0.0, 0.5)), (P.CONTRACTION, (2.0 ** 25, 3.0, -4.0))):
        p32, sel = R.normalized(np.array([x], dtype=np.float32), space)
        assert not sel.any() and not p32.any()
        d = np.arange(1.0, 7.0)[None, :]
        g, B, m = R.frozen_table_gradient(p32, d, scal, 6)
        want = np.zeros((3 << 6, 2))
        for l in range(3):
            want[l << 6] = d[0, 2 * l:2 * l + 2]
        assert np.array_equal(g, want) and np.array_equal(B, want) and np.array_equal(m, (want != 0).astype(np.int64))


def test_hand_computed_colliding_corners():
    """T = 16: the eight corners of cell (4, 8, 12) fall on fewer than eight entries; every corner still adds"""
    T = 16
    corners = [(4 + bx, 8 + by, 12 + bz) for bx in (0, 1) for by in (0, 1) for bz in (0, 1)]
    entries = [_hash(*c, T) for c in corners]
    assert len(set(entries)) < 8
    g, B, m = _one((4.5 / 16, 8.5 / 16, 12.5 / 16), (8.0, -8.0), 16.0, 4)
    want = np.zeros((T, 2))
    for e in entries:
        want[e] += np.array([1.0, -1.0])  # every weight is 1/8
    assert np.array_equal(g, want) and np.array_equal(B, np.abs(want))
    assert np.array_equal(m[:, 0], np.bincount(entries, minlength=T)) and int(m.sum()) == 16 and m.max() >= 2


def test_contribution_roundings_fit_the_counted_K():
    """the kernel's fp32 contribution (restated operation by operation) stays within K_CONTRIBUTION * 2^-24 of the fp64 term on
    every builder's positions: a miscounted K or a wrong weight association would show without a device"""
    scal = R.integer_scalings(16, 2048)
    cases = R.mixed_cases(scal, False)
    p32, _ = R.normalized(cases.positions, R.UNIT_BOX)
    d = np.random.default_rng(0).standard_normal((len(cases), 2)).astype(np.float32)
    worst = 0.0
    for s in scal:
        _, term = R.level_terms(p32, d, s, 15)
        got = R.kernel_level_terms_fp32(p32, d, s).astype(np.float64)
        nz = term != 0
        worst = max(worst, float((np.abs(got - term)[nz] / (R.EPS32 * np.abs(term[nz]))).max()))
        assert (np.abs(got - term) <= R.K_CONTRIBUTION * R.EPS32 * np.abs(term) + 1e-45).all()
    assert 1.0 < worst <= R.K_CONTRIBUTION


def _sequential_fp32(case, scalings, log2T, order_seed):
    """the case's contributions added one by one in fp32, into a table of fp32 zeros, in a seeded order"""
    L = len(scalings)
    p32, _ = R.normalized(case.positions, case.space)
    slots, terms = [], []
    for l, s in enumerate(scalings):
        d_l = case.d_enc[:, 2 * l:2 * l + 2]
        if d_l.any():
            slot, _ = R.level_terms(p32, d_l, s, log2T)
            slots.append(slot + (2 * l << log2T))
            terms.append(R.kernel_level_terms_fp32(p32, d_l, s))
    slots, terms = np.concatenate(slots), np.concatenate(terms)
    assert terms.dtype == np.float32
    order = np.arange(len(slots)) if order_seed is None else np.random.default_rng(order_seed).permutation(len(slots))
    acc = np.zeros(2 * L << log2T, dtype=np.float32)
    np.add.at(acc, slots[order], terms[order])  # unbuffered: one fp32 add per term, in this order
    return acc


@pytest.mark.parametrize("contraction", [False, True], ids=["box", "contraction"])
@pytest.mark.parametrize("L,log2T,max_res", GRIDS)
def test_exact_sum_cases_are_exact(L, log2T, max_res, contraction):
    scal = R.integer_scalings(L, max_res)
    cases = R.exact_sum_cases(scal, log2T, contraction)
    labels = [c.label for c in cases]
    assert len(set(labels)) == len(labels)
    for prefix in ("one:4097", "cell:", "cells:", "runs:63+1", "emit:", "channels:minus0", "selector0"):
        assert any(l.startswith(prefix) for l in labels), prefix
    zero = np.zeros((L << log2T, 2), dtype=np.float32)
    for case in cases:
        assert case.q <= 12 and 0 < case.fill < 1, case.label
        assert np.array_equal(case.d_enc, np.round(case.d_enc)) and np.abs(case.d_enc).max() <= 2
        p32, _ = R.normalized(case.positions, case.space)
        g, B, m = R.frozen_table_gradient(p32, case.d_enc, scal, log2T)
        scaled = g * 2.0 ** case.q
        assert np.array_equal(scaled, np.round(scaled))
        T = 1 << log2T
        for l, s in enumerate(scal):  # the condition itself, level by level
            if case.d_enc[:, 2 * l:2 * l + 2].any():
                assert (B[l * T:(l + 1) * T].max() + R.START_MAX) * 2.0 ** R.level_q(p32, s) < 2.0 ** 24
        want = case.expected(zero)
        assert np.array_equal(want.astype(np.float64), g), case.label
        assert np.array_equal(np.flatnonzero(m.reshape(-1)), case.slots) and np.array_equal(m.reshape(-1)[case.slots], case.counts)
        for order in (None, 1):
            got = _sequential_fp32(case, scal, log2T, order)
            assert np.array_equal(got.view(np.int32), want.reshape(-1).view(np.int32)), (case.label, order)
        # (+=) on integers: still exact, other levels' rows untouched
        start = np.random.default_rng(3).integers(-R.START_MAX, R.START_MAX + 1, size=zero.shape).astype(np.float32)
        part = case.expected(start, L - 1, L)
        T = 1 << log2T
        assert np.array_equal(part[:(L - 1) * T], start[:(L - 1) * T])
        assert np.array_equal(part[(L - 1) * T:].astype(np.float64), start[(L - 1) * T:].astype(np.float64) + g[(L - 1) * T:])


def test_crafted_level_positions_hit_their_targets():
    """per level of the 16 -> 2048 and 16 -> 128 grids at least 80 % of the targets cell + k / 4 are attained by an fp32 p"""
    rng = np.random.default_rng(4)
    for L, max_res in ((16, 2048), (5, 128)):
        for s in R.integer_scalings(L, max_res):
            cells = rng.integers(1, int(s) - 1, size=(500, 3))
            ks = rng.integers(0, 4, size=(500, 3))
            p, ok = R.crafted_level_positions(s, cells, ks)
            assert ok.mean() >= 0.8, (s, ok.mean())
            fl, ce, off = R.frozen_cell(p, s)
            assert np.array_equal(fl[ok], cells[ok]) and np.array_equal(off[ok], ks[ok] / 4.0)


def test_exact_sum_large():
    """the 2^20-sample case of the atomic kernel's grid-stride pass: exact, with thousands of terms per entry"""
    scal = R.integer_scalings(16, 2048)
    case = R.exact_sum_large(scal, 15, (1 << 20) + 7)
    assert case.counts.max() >= 2000 and 0 < case.fill < 1
