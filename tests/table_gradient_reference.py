"""fp64 reference of the table gradient (d loss / d hash table: the scatter that turns ``d_enc`` into ``d_table``), entry by entry,
and builders of inputs whose scatter is EXACT in fp32 — numpy, no device.  The sibling of tests/position_gradient_reference.py
(the other half of the encoding's adjoint), whose frozen cell, corner order, hash primes, spaces and case builders it reuses.

What the reference is.  Sample i adds ``w_corner(i) * d_enc[i, 2 l + c]`` to entry ``hash(corner) mod T`` of level l, for each of
its eight corners; the weights are products of the offsets ``o`` (corner = ceil) or ``1 - o`` (corner = floor) of the frozen fp32
cell ``sx = fl32(p * s)``.  On a grid plane ceil and floor are the same vertex: both corners of the axis are the same entry, with
the weights 0 and 1.  Two corners of one sample that hash to the same entry both add (small T).  A sample with selector 0 has
p = 0: it adds its whole ``d_enc`` to entry hash(0, 0, 0) = 0 of every level, as the reference implementation does.

Two kinds of check stand on it (tests/test_gpu_table_gradient.py):

* bounded: ``|got - want| <= (K_CONTRIBUTION + m) * 2^-24 * B`` per entry, B the sum of the absolute terms (and of what the table
  held before) and m the number of nonzero terms of the entry.  The bound loosens as m grows: a crowded coarse entry could lose a
  term and stay inside it.
* exact: inputs whose every contribution is a multiple of 2^-q and whose absolute sums stay below 2^(24 - q) per entry.  Every
  partial sum of such terms, in any order and any grouping, is an fp32 number: the device result is ``fl32(reference)`` bit for
  bit whatever the order of the adds, and any dropped, doubled or misplaced contribution changes bits.  This is what holds the
  crowded entries to account.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from oracle import hotpath as H
from tests.position_gradient_reference import (CONTRACTION, EPS32, UNIT_BOX, Space, _CORNERS, _P1, _P2, frozen_cell,  # noqa: F401
                                               mixed_cases, normalized)

# fp32 roundings on the longest path from the inputs to ONE contribution, counted from hash_encode_bwd_kernel and sort_records
# (both form the weights as (a * b) * c and multiply by d_enc last; first order, as the K_* of the sibling module):
#   o = sx - floor(sx) is exact: 0;  q = 1 - o: 1;  q * q: 1 + 1 + 1 = 3;  (q * q) * q: 3 + 1 + 1 = 5;  x d_enc (exact input): 6.
# An entry that receives m nonzero terms, in any order and grouping (run sums, private copies, an LDS slice, the final add onto
# what the table held), carries at most m further roundings: a sum of k terms that starts from zero takes k - 1, merging j partial
# sums j - 1, the add onto the table 1.
K_CONTRIBUTION = 6
START_MAX = 8           # exact cases start from a table of integers in [-START_MAX, START_MAX]


def tolerance(B: np.ndarray, m: np.ndarray) -> np.ndarray:
    """the per-entry bound of the bounded checks; derived from the code, never tuned against device output"""
    return (K_CONTRIBUTION + m) * EPS32 * B + 1e-30


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
def level_terms(p32: np.ndarray, d_enc_l: np.ndarray, scale: float, log2T: int) -> Tuple[np.ndarray, np.ndarray]:
    """every contribution of one level: (slot [8 * n * 2] int64 = 2 * entry + channel, term [8 * n * 2] fp64), corner-major in
    the f0 .. f7 order, then sample, then channel.  The fp64 products of fp32 offsets are exact to fp64's 53 bits."""
    T = 1 << log2T
    fl, ce, off = frozen_cell(p32, scale)
    d = np.asarray(d_enc_l, dtype=np.float64).reshape(-1, 2)
    slots, terms = [], []
    for bx, by, bz in _CORNERS:
        w = np.ones(len(d))
        for axis, b in enumerate((bx, by, bz)):
            w = w * (off[:, axis] if b else 1.0 - off[:, axis])
        x = (ce if bx else fl)[:, 0]
        y = (ce if by else fl)[:, 1] * _P1
        z = (ce if bz else fl)[:, 2] * _P2
        idx = (x ^ y ^ z) % T
        slots.append((2 * idx[:, None] + np.arange(2)[None, :]).reshape(-1))
        terms.append((w[:, None] * d).reshape(-1))
    return np.concatenate(slots), np.concatenate(terms)


def _level_sparse(p32, d_enc_l, scale, log2T):
    """(slot, g, B, m) of the slots (2 * entry + channel, ascending) that receive a term, zero terms included"""
    slot, term = level_terms(p32, d_enc_l, scale, log2T)
    hit, inv = np.unique(slot, return_inverse=True)
    return (hit, np.bincount(inv, weights=term, minlength=len(hit)), np.bincount(inv, weights=np.abs(term), minlength=len(hit)),
            np.bincount(inv[term != 0], minlength=len(hit)).astype(np.int64))


def _level_sums(p32, d_enc_l, scale, log2T):
    """(g, B, m) [T, 2] of one level: one np.bincount per (corner, channel) and quantity — or, with fewer terms than the level has
    slots, over the touched slots alone"""
    T = 1 << log2T
    if 16 * len(p32) < 2 * T:
        g, B, m = np.zeros(2 * T), np.zeros(2 * T), np.zeros(2 * T, dtype=np.int64)
        hit, g[hit], B[hit], m[hit] = _level_sparse(p32, d_enc_l, scale, log2T)
        return g.reshape(T, 2), B.reshape(T, 2), m.reshape(T, 2)
    fl, ce, off = frozen_cell(p32, scale)
    d = np.asarray(d_enc_l, dtype=np.float64).reshape(-1, 2)
    g, B, m = np.zeros((T, 2)), np.zeros((T, 2)), np.zeros((T, 2), dtype=np.int64)
    for bx, by, bz in _CORNERS:
        w = (off[:, 0] if bx else 1.0 - off[:, 0]) * (off[:, 1] if by else 1.0 - off[:, 1]) * (off[:, 2] if bz else 1.0 - off[:, 2])
        idx = ((ce if bx else fl)[:, 0] ^ ((ce if by else fl)[:, 1] * _P1) ^ ((ce if bz else fl)[:, 2] * _P2)) % T
        for c in range(2):
            term = w * d[:, c]
            g[:, c] += np.bincount(idx, weights=term, minlength=T)
            B[:, c] += np.bincount(idx, weights=np.abs(term), minlength=T)
            m[:, c] += np.bincount(idx[term != 0], minlength=T)
    return g, B, m


def frozen_table_gradient(p32, d_enc, scalings: Sequence[float], log2T: int, level_begin: int = 0, level_end: Optional[int] = None):
    """(g, B, m), each [L * T, 2]: the fp64 sum over the samples and the eight corners of ``w_corner * d_enc[:, 2 l + c]`` at row
    ``l * T + hash(corner) mod T``; the same sum of absolute values; the integer count of nonzero terms.  ``p32``: normalised
    positions with the selector applied (``normalized()``).  Rows of levels outside [level_begin, level_end) are zero."""
    L, T = len(scalings), 1 << log2T
    level_end = L if level_end is None else level_end
    d_enc = np.asarray(d_enc)
    assert d_enc.shape == (len(p32), 2 * L) and 0 <= level_begin <= level_end <= L
    g, B, m = np.zeros((L * T, 2)), np.zeros((L * T, 2)), np.zeros((L * T, 2), dtype=np.int64)
    for l in range(level_begin, level_end):
        g[l * T:(l + 1) * T], B[l * T:(l + 1) * T], m[l * T:(l + 1) * T] = _level_sums(p32, d_enc[:, 2 * l:2 * l + 2], scalings[l], log2T)
    return g, B, m


def kernel_level_terms_fp32(p32, d_enc_l, scale):
    """the contributions as hash_encode_bwd_kernel and sort_records form them, in numpy float32 operation by operation:
    q = 1 - o, the weight (a * b) * c, then x d_enc.  Same order as level_terms."""
    f32 = np.float32
    sx = (np.asarray(p32, dtype=f32) * f32(scale)).astype(f32)
    o = (sx - np.floor(sx)).astype(f32)
    q = (f32(1.0) - o).astype(f32)
    d = np.asarray(d_enc_l, dtype=f32).reshape(-1, 2)
    out = []
    for bx, by, bz in _CORNERS:
        w = ((o if bx else q)[:, 0] * (o if by else q)[:, 1]).astype(f32) * (o if bz else q)[:, 2]
        out.append((w.astype(f32)[:, None] * d).astype(f32).reshape(-1))
    return np.concatenate(out)


# ----------------------------------------------------------------------------------------------------------------------
# inputs whose scatter is exact in fp32
# ----------------------------------------------------------------------------------------------------------------------
def integer_scalings(L: int, max_res: int) -> List[float]:
    """the oracle's scalings (floor of a geometric progression): integers, which is what makes ``p * s`` of a dyadic p exact"""
    s = [float(v) for v in H.hash_scalings(L, 16, max_res).tolist()]
    assert all(v == np.floor(v) and 1 <= v < 2 ** 12 for v in s), s
    return s


def dyadic_pool(b: int, contraction: bool) -> np.ndarray:
    """all points (j / 2^b)^3 inside the unit box, or inside (0.25, 0.75)^3 — the image of the contraction's identity branch"""
    j = np.arange(1, 1 << b)
    v = (j / float(1 << b)).astype(np.float32)
    if contraction:
        v = v[(v > 0.25) & (v < 0.75)]
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)


def to_world(p32: np.ndarray, contraction: bool) -> Tuple[np.ndarray, Space]:
    """world positions that normalise back to ``p32`` bit for bit: p itself (unit box) or 4 p - 2 (identity branch; exact)"""
    p32 = np.ascontiguousarray(p32, dtype=np.float32)
    if not contraction:
        space, world = UNIT_BOX, p32
    else:
        space, world = CONTRACTION, (np.float32(4.0) * p32 - np.float32(2.0)).astype(np.float32)
        assert np.array_equal(world.astype(np.float64), 4.0 * p32.astype(np.float64) - 2.0)
    back, sel = normalized(world, space)
    assert sel.all() and np.array_equal(back, p32)
    return world, space


def crafted_level_positions(scale: float, cells: np.ndarray, ks: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(p32 [n, 3], attained [n, 3]) with ``fl32(p * scale) == cell + k / 4`` where attained: the few fp32 values around
    ``(cell + k / 4) / scale`` are searched for one whose fp32 product lands on the target (83 - 100 % of the coordinates do on the
    16 -> 2048 and 16 -> 128 grids).  Offsets k / 4 make every weight a multiple of 2^-6 at that level, whatever the scale."""
    s = np.float32(scale)
    target = (np.asarray(cells, dtype=np.float64) + np.asarray(ks, dtype=np.float64) / 4.0).astype(np.float32)
    p = (target / s).astype(np.float32)
    best, hit = p.copy(), (p * s).astype(np.float32) == target
    lo, hi = p.copy(), p.copy()
    for _ in range(3):
        lo, hi = np.nextafter(lo, np.float32(-1.0)), np.nextafter(hi, np.float32(2.0))
        for cand in (lo, hi):
            ok = ~hit & ((cand * s).astype(np.float32) == target)
            best[ok], hit = cand[ok], hit | ok
    return best, hit


class ExactCase(NamedTuple):
    """inputs whose scatter is exact, and its result in sparse form: d_table.reshape(-1)[slots] += sums, everything else untouched"""
    label: str
    positions: np.ndarray   # [n, 3] float32, world space
    d_enc: np.ndarray       # [n, 2 L] float32, small integers
    space: Space
    q: int                  # every contribution is a multiple of 2^-q
    slots: np.ndarray       # flat indices into [L * T * 2] with at least one nonzero term
    sums: np.ndarray        # float64, exactly representable in fp32
    counts: np.ndarray      # m of those slots
    largest_B: float
    fill: float             # the largest (B + START_MAX) 2^q_level / 2^24 over the levels: below 1

    def expected_sparse(self, start: np.ndarray, level_begin: int = 0, level_end: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(slots, fl32(start + reference) at those slots) of a call over the levels [level_begin, level_end); every other slot keeps
        what ``start`` ([L * T, 2] float32, integers up to START_MAX) holds"""
        L = self.d_enc.shape[1] // 2
        per_level = start.size // L
        lo, hi = level_begin * per_level, (L if level_end is None else level_end) * per_level
        slots = self.slots[(self.slots >= lo) & (self.slots < hi)]
        sums = self.sums[(self.slots >= lo) & (self.slots < hi)]
        before = start.reshape(-1)[slots]
        want = before.astype(np.float64) + sums
        assert np.abs(before).max(initial=0.0) <= START_MAX and np.array_equal(want.astype(np.float32).astype(np.float64), want)
        return slots, want.astype(np.float32)

    def expected(self, start: np.ndarray, level_begin: int = 0, level_end: Optional[int] = None) -> np.ndarray:
        out = np.array(start, dtype=np.float32).reshape(-1)
        slots, values = self.expected_sparse(start, level_begin, level_end)
        out[slots] = values
        return out.reshape(start.shape)


def level_q(p32, scale) -> int:
    """q of one level: the weights are products of three offsets"""
    return 3 * _offset_bits(p32, scale)


def _offset_bits(p32, scale) -> int:
    """smallest k with every offset of the level a multiple of 2^-k"""
    off = frozen_cell(p32, scale)[2]
    for k in range(0, 25):
        if np.array_equal(np.round(off * (1 << k)), off * (1 << k)):
            return k
    raise AssertionError("offsets are not dyadic")


def check_exact(label, world, space: Space, d_enc, scalings, log2T) -> Optional[ExactCase]:
    """the exactness condition, level by level: every term a multiple of 2^-q, (B + START_MAX) 2^q < 2^24 for every entry, and the
    kernel's own fp32 arithmetic (kernel_level_terms_fp32) forms every term without rounding.  None if it does not hold."""
    L, T = len(scalings), 1 << log2T
    world = np.ascontiguousarray(world, dtype=np.float32)
    p32 = normalized(world, space)[0]
    d_enc = np.asarray(d_enc, dtype=np.float32)
    assert d_enc.shape == (len(p32), 2 * L) and np.array_equal(d_enc, np.round(d_enc))
    slots, sums, counts, q, largest, fill = [], [], [], 0, 0.0, 0.0
    distinct = np.unique(p32, axis=0)
    ones = np.ones((len(distinct), 2), dtype=np.float32)
    for l, s in enumerate(scalings):
        d_l = d_enc[:, 2 * l:2 * l + 2]
        if not d_l.any():
            continue
        # the weights of every distinct position: multiples of 2^-q that the kernel's fp32 products form without rounding; with the
        # bound on B below, w * d is then exact for every integer d
        ql = level_q(distinct, s)
        _, w = level_terms(distinct, ones, s, log2T)
        scaled = w * 2.0 ** ql
        if ql > 24 or not np.array_equal(scaled, np.round(scaled)):
            return None
        if not np.array_equal(kernel_level_terms_fp32(distinct, ones, s).astype(np.float64), w):
            return None
        if 16 * len(p32) < 2 * T:
            hit, g, B, m = _level_sparse(p32, d_l, s, log2T)
        else:
            g, B, m = (a.reshape(-1) for a in _level_sums(p32, d_l, s, log2T))
            hit = np.arange(2 * T)
        if (B.max() + START_MAX) * 2.0 ** ql >= 2.0 ** 24:
            return None
        slots.append(hit[m > 0] + 2 * l * T)
        sums.append(g[m > 0])
        counts.append(m[m > 0])
        q, largest, fill = max(q, ql), max(largest, float(B.max())), max(fill, float(B.max() + START_MAX) * 2.0 ** (ql - 24))
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    return ExactCase(label, world, d_enc, space, q, cat(slots, np.int64), cat(sums, np.float64), cat(counts, np.int64), largest, fill)


def integer_d_enc(rng, n: int, L: int, dmax: int, nonzero: bool = False) -> np.ndarray:
    """integers in [-dmax, dmax] ([-dmax, dmax] without 0 with ``nonzero``)"""
    d = rng.integers(-dmax, dmax + 1, size=(n, 2 * L))
    if nonzero:
        d = np.where(d == 0, dmax, d)
    return d.astype(np.float32)


# (bits of the dyadic positions, largest |d_enc|) from the most varied to the most room per entry: b = 3 with |d_enc| <= 2 leaves
# room for 2^24 / 2^9 / 2 = 16 384 contributions per entry
_CHOICES = ((4, 2), (3, 2), (3, 1), (2, 1), (1, 1))


def exact_case(label: str, scalings, log2T: int, contraction: bool, pattern: Sequence[int], seed: int, edit=None,
               nonzero: bool = False, choices=_CHOICES) -> ExactCase:
    """sample i sits on distinct point ``pattern[i]`` of a dyadic pool (different points lie in different cells at every level:
    their scaled coordinates differ by at least 1 on some axis); b and the range of d_enc are the first of ``choices`` that meet
    the exactness condition.  ``edit(d_enc)``: changes d_enc in place before the check (zero rows, channels ...)."""
    pattern = np.asarray(pattern, dtype=np.int64)
    L = len(scalings)
    for b, dmax in choices:
        pool = dyadic_pool(b, contraction)
        if len(pool) <= pattern.max() or (1 << b) > min(scalings):
            continue
        rng = np.random.default_rng(seed)
        points = pool[rng.permutation(len(pool))[:pattern.max() + 1]]
        d_enc = integer_d_enc(rng, len(pattern), L, dmax, nonzero)
        if edit is not None:
            edit(d_enc)
        case = check_exact(f"{label} b={b} |d|<={dmax}", *to_world(points[pattern], contraction), d_enc, scalings, log2T)
        if case is not None:
            return case
    raise AssertionError(f"{label}: no choice of b and d_enc range is exact")


def crafted_case(label: str, scalings, log2T: int, contraction: bool, level: int, cells: np.ndarray, ks: np.ndarray, seed: int,
                 dmax: int = 2, take: Optional[int] = None) -> ExactCase:
    """one crafted level: sample i aims at ``cells[i] + ks[i] / 4`` of ``level``; d_enc is zero outside that level.  At least 80 %
    of the coordinates must be attained; the samples with all three are kept, in order; ``take``: the first that many of them."""
    L = len(scalings)
    p32, hit = crafted_level_positions(scalings[level], cells, ks)
    assert hit.mean() >= 0.8, (label, float(hit.mean()))
    ok = hit.all(axis=1)
    if contraction:
        ok &= ((p32 > 0.25) & (p32 < 0.75)).all(axis=1)
    else:
        ok &= ((p32 > 0.0) & (p32 < 1.0)).all(axis=1)
    p32 = p32[ok]
    assert len(p32) > 0, label
    if take is not None:
        assert len(p32) >= take, (label, len(p32))
        p32 = p32[:take]
    rng = np.random.default_rng(seed)
    d_enc = np.zeros((len(p32), 2 * L), dtype=np.float32)
    d_enc[:, 2 * level:2 * level + 2] = integer_d_enc(rng, len(p32), 1, dmax)
    case = check_exact(f"{label} level {level}", *to_world(p32, contraction), d_enc, scalings, log2T)
    assert case is not None and case.q <= 6, label
    return case


def runs(lengths: Sequence[int], points: int) -> np.ndarray:
    """a pattern of runs of the given lengths; consecutive runs sit on different points (0, 1, ... cycling through ``points``)"""
    return np.concatenate([np.full(n, i % points, dtype=np.int64) for i, n in enumerate(lengths)])


ONE_CELL_COUNTS = (1, 63, 64, 65, 255, 256, 257, 4097)


def exact_sum_cases(scalings, log2T: int, contraction: bool = False) -> List[ExactCase]:
    """the exact family of one grid (every case meets check_exact; the builders assert it):

    one:<n>          all samples on one point = one cell at every level: a run that fills a wave and crosses waves, blocks, chunks
    cell:<n>         one cell of the finest level with the offsets k / 4, k = 1 .. 3, on every axis (crafted level)
    cells:<l>        crafted level l: random cells and offsets k / 4, k = 0 .. 3 (k = 0: on a plane), in short runs
    runs:*           run patterns inside a wave: ABAB, lengths 2 and 3, 63 + 1, a run that ends at lane 63 and goes on in the next
                     wave, a ragged last wave whose dead lanes repeat the final sample's cell, random lengths
    emit:<n>         256 * 8 + 1 and 256 * 9 + 5 samples: chunk counts of the bucketed emit pass that are no multiple of 8
    channels:*       d_enc with channel 0 zero, with -0.0, with whole zero rows, with rows zero from the middle level up
    selector0        every sample outside the box: p = 0, the whole d_enc lands on entry 0 of every level
    top-vertex:<l>   every sample in the last cell of level l (ceil = the scaling: the highest vertex of a dense copy)
    """
    L = len(scalings)
    assert all(float(s) == np.floor(s) for s in scalings)
    args = (scalings, log2T, contraction)
    out = [exact_case(f"one:{n}", *args, np.zeros(n, dtype=np.int64), seed=n, nonzero=True) for n in ONE_CELL_COUNTS]
    rng = np.random.default_rng(17 * L + log2T)
    lo, hi = (0.25, 0.75) if contraction else (0.0, 1.0)

    def cell_range(l):  # cells whose vertices stay inside (lo, hi) of the space
        return int(np.floor(lo * scalings[l])) + 1, int(np.ceil(hi * scalings[l])) - 2

    fine = L - 1
    a, b = cell_range(fine)
    for n in (65, 257, 4097):
        cell = rng.integers(a, b + 1, size=(1, 3))
        out.append(crafted_case(f"cell:{n}", *args, fine, np.repeat(cell, 2 * n, axis=0), rng.integers(1, 4, size=(2 * n, 3)), seed=n, take=n))
    for l in sorted({0, L // 2, fine}):
        a, b = cell_range(l)
        lengths = rng.integers(1, 6, size=200)
        cells = rng.integers(a, b + 1, size=(len(lengths), 3))
        ks = rng.integers(0, 4, size=(len(lengths), 3))
        rep = np.repeat(np.arange(len(lengths)), lengths)
        out.append(crafted_case(f"cells:{l}", *args, l, cells[rep], ks[rep], seed=l))
    patterns = {
        "abab": runs([1] * 128, 2), "len2": runs([2] * 70, 5), "len3": runs([3] * 50, 7), "63+1": runs([63, 1, 63, 1], 2),
        "ends-at-63": runs([10, 54, 30, 34, 64, 7], 3), "ragged": runs([5, 9, 50, 3, 2], 4), "ragged-1": runs([64, 1], 2),
        "random": runs(rng.integers(1, 40, size=60), 11),
    }
    for i, (name, pat) in enumerate(patterns.items()):
        out.append(exact_case(f"runs:{name}", *args, pat, seed=100 + i))
    for n in (256 * 8 + 1, 256 * 9 + 5):
        out.append(exact_case(f"emit:{n}", *args, runs(rng.integers(1, 30, size=n // 8), 23)[:n], seed=n))
    mid = L // 2

    def channel0(d): d[:, 0::2] = 0.0
    def minus0(d): d[d == 0] = -0.0; d[::3] = -0.0
    def zero_rows(d): d[rng.random(len(d)) < 0.3] = 0.0
    def zero_fine(d): d[::2, 2 * mid:] = 0.0
    for i, (name, edit) in enumerate((("channel0", channel0), ("minus0", minus0), ("zero-rows", zero_rows), ("zero-fine-levels", zero_fine))):
        out.append(exact_case(f"channels:{name}", *args, runs(rng.integers(1, 9, size=120), 9), seed=200 + i, edit=edit))
    # selector 0: outside the box (or, with the contraction, so far that 2 - 1 / mag rounds to 2)
    n = 300
    far = np.full((n, 3), 2.0 ** 25 if contraction else 1.5, dtype=np.float32)
    far[:, 1:] = rng.integers(-3, 4, size=(n, 2))
    space = CONTRACTION if contraction else UNIT_BOX
    p0, sel = normalized(far, space)
    assert not sel.any() and not p0.any()
    out.append(check_exact("selector0", far, space, integer_d_enc(rng, n, L, 2), scalings, log2T))
    assert out[-1] is not None and np.array_equal(out[-1].slots // 2 % (1 << log2T), np.zeros_like(out[-1].slots))
    if not contraction:  # (the last cell of a level lies outside the contraction's identity branch)
        for l in sorted({0, min(2, L - 1)}):
            top = int(scalings[l]) - 1
            out.append(crafted_case(f"top-vertex:{l}", *args, l, np.full((130, 3), top), rng.integers(1, 4, size=(130, 3)), seed=300 + l))
    return out


def exact_sum_large(scalings, log2T: int, n: int, seed: int = 5) -> ExactCase:
    """n samples drawn from the few hundred points of a dyadic pool (m reaches ~1e4 per entry at n = 2^20: b = 3, |d_enc| <= 1)"""
    rng = np.random.default_rng(seed)
    pool = len(dyadic_pool(3, False))
    return exact_case(f"large:{n}", scalings, log2T, False, rng.integers(0, pool, size=n), seed, choices=((3, 1), (2, 1)))
