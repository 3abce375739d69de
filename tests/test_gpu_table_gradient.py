"""The table gradient's device forms — the atomic kernel (tn_hash_encode_bwd, tn_hash_encode_bwd_levels), the spread form
(tn_hash_encode_bwd_spread), the bucketed form (tn_hash_encode_bwd_sorted) and the split form the training step uses
(training.hash_encode_bwd: atomic below the first bucketed level, bucketed from it, optionally on side streams) — entry by entry
against the fp64 reference of tests/table_gradient_reference.py.

A. Exact-sum cases.  Inputs whose every contribution is a multiple of 2^-q and whose absolute sums stay below 2^(24 - q) per
   entry: whatever the order and the grouping of the adds, d_table must equal fl32(reference) BIT FOR BIT, for every form and
   therefore across forms.  A dropped, doubled or misplaced contribution changes bits.
B. Bounded cases.  Every builder's positions (grid planes and their ulp neighbours, kinks, faces, dyadic, uniform) with a normal
   d_enc: |got - want| <= (K_CONTRIBUTION + m) * 2^-24 * B per entry, m the number of nonzero terms of the entry and B their
   absolute sum (plus what the entry held); K_CONTRIBUTION = 6 is counted from the kernels' code next to the constant and never
   tuned against device output.  The bound loosens as m grows — a crowded coarse entry could lose one of thousands of terms and
   stay inside it: family A is what holds the crowded entries to account, family B the weights at arbitrary offsets.
   Every check prints ``table-gradient bound | form | grid | worst err/(eps B) | largest m``; profiles/micro/table_gradient_bounds.txt
   records one run's lines.
C. Refusals and no-ops, none of which may touch d_table.

Every call writes into a d_table that sits between sentinel rows and starts from small random integers (+=): untouched entries,
the rows of levels outside the call's range and the guard rows must keep their bits.  The comparisons run on the device (a table
of 2^19 entries x 16 levels is 64 MB); the host sees the result only to describe a mismatch."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import pytest
import torch

from tests import table_gradient_reference as R
from tests.test_gpu_position_gradient import COUNTS, c_space
from thermo_nerf_amd import _hip
from thermo_nerf_amd import training as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25  # prefill of the guard rows
GUARD = 8         # rows on either side (64 bytes: d_table keeps the 16-byte alignment the owner pass's float4 accesses need)
TN_ERR_SHAPE, TN_ERR_UNSUPPORTED, TN_ERR_WORKSPACE = -2, -3, -4

# (num_levels, log2_hashmap_size, max_res): 2 slices per level | 32 slices, the field's grid | tables smaller than a slice (two) |
# a proposal grid, 8 slices | collisions
GRIDS = [(16, 15, 2048), (16, 19, 2048), (5, 13, 128), (8, 12, 512), (5, 17, 256), (1, 4, 16)]
GRID_IDS = [f"L{L}-T{t}-res{r}" for L, t, r in GRIDS]


class Grid:
    """a hash grid, its start table of small integers (host and device) and its cached cases"""
    _cache: dict = {}

    def __init__(self, L, log2T, max_res, scalings=None):
        self.L, self.log2T, self.T, self.rows = L, log2T, 1 << log2T, L << log2T
        self.scalings = R.integer_scalings(L, max_res) if scalings is None else scalings
        rng = np.random.default_rng(1000 * L + log2T)
        self.start = rng.integers(-R.START_MAX, R.START_MAX + 1, size=(self.rows, 2)).astype(np.float32)
        self.start_dev = torch.from_numpy(self.start).to(DEV)
        self.c = _hip.tn_hashgrid()
        # (the scatter never reads the table; the pointer only has to be a table's)
        self.c.table, self.c.num_levels, self.c.log2_hashmap_size = self.start_dev.data_ptr(), L, log2T
        for i, s in enumerate(self.scalings):
            self.c.scalings[i] = s
        self.name = f"L{L} T2^{log2T} res{max_res}"
        self._cases: dict = {}

    @classmethod
    def get(cls, L, log2T, max_res):
        key = (L, log2T, max_res)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def exact(self, contraction):
        key = ("exact", contraction)
        if key not in self._cases:
            self._cases[key] = R.exact_sum_cases(self.scalings, self.log2T, contraction)
        return self._cases[key]

    def mixed(self, contraction):
        key = ("mixed", contraction)
        if key not in self._cases:
            cases = R.mixed_cases(self.scalings, contraction)
            space = R.CONTRACTION if contraction else R.UNIT_BOX
            self._cases[key] = (cases, space, *R.normalized(cases.positions, space))
        return self._cases[key]


# ----------------------------------------------------------------------------------------------------------------------
# the forms
# ----------------------------------------------------------------------------------------------------------------------
class Call(NamedTuple):
    grid: Grid
    space: object       # tn_space
    pos: torch.Tensor
    d_enc: torch.Tensor
    n: int
    out: torch.Tensor   # d_table

    def args(self):
        return (self.grid.c, self.space, self.pos.data_ptr(), self.d_enc.data_ptr(), self.n, self.out.data_ptr())


class Form(NamedTuple):
    name: str
    levels: Callable[[int], Optional[Tuple[int, int]]]  # L -> the levels [lo, hi) the form covers, or None: not on this grid
    run: Callable[[Call], None]


_WS: dict = {}


def _workspace(kind, nbytes):
    """one buffer per kind and size, filled with junk when made and kept between calls: a form must clear what it relies on"""
    key = (kind, nbytes)
    if key not in _WS:
        _WS[key] = torch.full((max(nbytes, 16),), 0x5b, dtype=torch.uint8, device=DEV)
    return _WS[key]


def _lib():
    return _hip.load()


def _atomic(c: Call):
    _hip.check(_lib().tn_hash_encode_bwd(*c.args(), _hip.current_stream()), "tn_hash_encode_bwd")


def _levels(lo_of, hi_of):
    def run(c: Call):
        L = c.grid.L
        _hip.check(_lib().tn_hash_encode_bwd_levels(*c.args(), lo_of(L), hi_of(L), _hip.current_stream()), "tn_hash_encode_bwd_levels")
    return run


def _spread(lo: int):
    def run(c: Call):
        need = _lib().tn_hash_encode_bwd_spread_workspace_bytes(c.grid.c)
        assert need > 0  # every grid here starts at a scaling of 16: a dense copy of 18^3 vertices
        ws = _workspace("spread", need)
        _hip.check(_lib().tn_hash_encode_bwd_spread(*c.args(), lo, c.grid.L, ws.data_ptr(), need, _hip.current_stream()), "tn_hash_encode_bwd_spread")
    return run


def _sorted(first_of):
    def run(c: Call):
        first = first_of(c.grid.L)
        need = _lib().tn_hash_encode_bwd_sorted_workspace_bytes(c.grid.c, c.n, first)
        assert need > 0
        ws = _workspace("sorted", need)
        _hip.check(_lib().tn_hash_encode_bwd_sorted(*c.args(), first, ws.data_ptr(), need, _hip.current_stream()), "tn_hash_encode_bwd_sorted")
    return run


def _split(bucketed_of, **kw):
    def run(c: Call):
        deferred = TR.hash_encode_bwd(c.grid.c, c.space, c.pos, c.d_enc, c.out, bucketed=bucketed_of(c.grid.L), **kw)
        assert deferred == bool(kw.get("defer") and c.grid.L > 1)
        _hip.join_pending()  # join before reading
    return run


def _whole(L):
    return 0, L


def _middle(L):
    return L // 2


def _side(L):  # the first bucketed level of the calls that put the two parts on different streams: it must leave an atomic part
    return max(1, L // 2) if L > 1 else 0


FORMS = [
    Form("tn_hash_encode_bwd", _whole, _atomic),
    Form("tn_hash_encode_bwd_levels [0,1)", lambda L: (0, 1), _levels(lambda L: 0, lambda L: 1)),
    Form("tn_hash_encode_bwd_levels [3,7)", lambda L: (3, 7) if L >= 7 else None, _levels(lambda L: 3, lambda L: 7)),
    Form("tn_hash_encode_bwd_levels [L-1,L)", lambda L: (L - 1, L), _levels(lambda L: L - 1, lambda L: L)),
    Form("tn_hash_encode_bwd_spread", _whole, _spread(0)),
    Form("tn_hash_encode_bwd_spread from level 1", lambda L: (1, L) if L > 1 else None, _spread(1)),  # falls back to no spread
    Form("tn_hash_encode_bwd_sorted from level 0", _whole, _sorted(lambda L: 0)),
    Form("tn_hash_encode_bwd_sorted from the middle", lambda L: (L // 2, L) if L > 2 else None, _sorted(_middle)),
    Form("tn_hash_encode_bwd_sorted from the last level", lambda L: (L - 1, L) if L > 1 else None, _sorted(lambda L: L - 1)),
    Form("hash_encode_bwd bucketed=True", _whole, _split(lambda L: True)),
    Form("hash_encode_bwd bucketed=int", _whole, _split(_middle)),
    Form("hash_encode_bwd bucketed=int no spread", _whole, _split(_middle, spread=False)),
    Form("hash_encode_bwd overlap", _whole, _split(_side, overlap=True)),
    Form("hash_encode_bwd overlap defer", _whole, _split(_side, overlap=True, defer=True)),
]
BY_NAME = {f.name: f for f in FORMS}


def guarded(grid: Grid):
    """a d_table inside a sentinel-filled buffer with GUARD rows on either side"""
    buf = torch.full((grid.rows + 2 * GUARD, 2), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + grid.rows]


def guards_intact(buf, rows):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + rows:] == SENTINEL).all())


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def scatter(form: Form, grid: Grid, space: R.Space, pos32: np.ndarray, d_enc32: np.ndarray, same_bits: bool, reps: int = 2):
    """one form into a guarded d_table that starts from grid.start, ``reps`` times from the same start (the second call finds the
    workspaces as the first left them).  Returns the results of the last and of the first call, on the device.  ``same_bits``
    (exact inputs): both calls give the same bits."""
    n = len(pos32)
    pos = torch.from_numpy(np.ascontiguousarray(pos32, dtype=np.float32)).to(DEV)
    d_enc = torch.from_numpy(np.ascontiguousarray(d_enc32, dtype=np.float32)).to(DEV)
    assert d_enc.shape == (n, 2 * grid.L)
    buf, out = guarded(grid)
    call = Call(grid, c_space(space), pos, d_enc, n, out)
    first = None
    for rep in range(reps):
        out.copy_(grid.start_dev)
        form.run(call)
        torch.cuda.synchronize()
        if rep == 0:
            first = out.clone()
    assert guards_intact(buf, grid.rows), form.name
    if same_bits:
        assert torch.equal(bits(first), bits(out)), f"{form.name}: the second call gives other bits than the first"
    return out, first


def _describe(grid: Grid, got: torch.Tensor, want: torch.Tensor, limit=6):
    bad = (bits(got) != bits(want)).reshape(-1).nonzero().reshape(-1)
    rows = []
    for s in bad[:limit].tolist():
        rows.append(f"level {s // (2 * grid.T)} entry {s // 2 % grid.T} ch {s % 2}: got {float(got.reshape(-1)[s])!r} want {float(want.reshape(-1)[s])!r}"
                    f" start {float(grid.start.reshape(-1)[s])!r}")
    return f"{int(bad.numel())} slots differ; " + "; ".join(rows)


def assert_exact(form: Form, grid: Grid, case: R.ExactCase, reps: int = 2):
    """d_table == fl32(start + reference) bit for bit over the form's levels, == start everywhere else"""
    lo, hi = form.levels(grid.L)
    slots, values = case.expected_sparse(grid.start, lo, hi)
    want = grid.start_dev.clone()
    want.view(-1)[torch.from_numpy(slots).to(DEV)] = torch.from_numpy(values).to(DEV)
    # (both calls against the reference: equal to it, they are equal to each other)
    for got in scatter(form, grid, case.space, case.positions, case.d_enc, False, reps)[:reps]:
        if not torch.equal(bits(got), bits(want)):
            raise AssertionError(f"{form.name} | {grid.name} | {case.label} (n={len(case.positions)}): {_describe(grid, got, want)}")
    return want


# ----------------------------------------------------------------------------------------------------------------------
# A. exact-sum cases
# ----------------------------------------------------------------------------------------------------------------------
def _forms_on(L):
    return [f for f in FORMS if f.levels(L) is not None]


@pytest.mark.parametrize("L,log2T,max_res", GRIDS, ids=GRID_IDS)
def test_exact_sum_cases_every_form(L, log2T, max_res):
    """every case of R.exact_sum_cases (one cell at 1 .. 4097 samples, run patterns inside a wave, ragged waves, emit chunk counts
    that are no multiple of 8, zero channels / -0.0 / zero rows / rows zero at the bucketed levels, selector 0, the highest
    vertex of a dense copy, crafted cells on and off planes), in the unit box, through every form: bit for bit"""
    grid = Grid.get(L, log2T, max_res)
    cases = grid.exact(False)
    for form in _forms_on(L):
        for case in cases:
            assert_exact(form, grid, case)
    assert len(cases) >= 25 and len(_forms_on(L)) >= (14 if L >= 7 else 8)


@pytest.mark.parametrize("L,log2T,max_res", [(16, 15, 2048), (5, 13, 128), (1, 4, 16)], ids=["L16-T15", "L5-T13", "L1-T4"])
def test_exact_sum_cases_through_the_contraction(L, log2T, max_res):
    """the same family placed in the contraction's identity branch (world = 4 p - 2)"""
    grid = Grid.get(L, log2T, max_res)
    for form in _forms_on(L):
        for case in grid.exact(True):
            assert_exact(form, grid, case)


def _capacity(n: int, owners: int) -> int:
    """a bin's region (sort_layout): its share of an even spread of the level's 4 n records, + 25 % + 1024, in multiples of 64"""
    share = (4 * n + owners - 1) // owners
    return (share + share // 4 + 1024 + 63) & ~63


def test_overflow_of_a_bins_region():
    """4097 samples in one cell of the 2-slice grid: the 4097 records of each (y, z) combination go to ONE slice, and where three
    or four combinations share a slice its region (11 328 records) is full: the rest goes straight into the table with atomics.
    The seam must lose or double nothing: equal to the reference bit for bit, hence equal to the atomic form."""
    L, log2T, n = 16, 15, 4097
    grid = Grid.get(L, log2T, 2048)
    owners = 1 << (log2T - 14)
    capacity = _capacity(n, owners)
    assert (owners, capacity) == (2, 11328)
    case = next(c for c in grid.exact(False) if c.label.startswith("one:4097"))
    assert len(case.positions) == n and (case.d_enc != 0).all()  # every (sample, level) writes its four records
    p32, _ = R.normalized(case.positions[:1], case.space)
    fullest = []
    for s in grid.scalings:
        fl, ce, _ = R.frozen_cell(p32, s)
        per_slice = np.zeros(owners, dtype=np.int64)
        for y in (ce[0, 1], fl[0, 1]):
            for z in (ce[0, 2], fl[0, 2]):
                hyz = (y * R._P1) ^ (z * R._P2)
                a, b = ((ce[0, 0] ^ hyz) % grid.T) >> 14, ((fl[0, 0] ^ hyz) % grid.T) >> 14
                assert a == b  # both x-neighbours of a record lie in one slice
                per_slice[a] += n
        fullest.append(int(per_slice.max()))
    assert max(fullest) == 4 * n == 16388 > capacity and max(fullest[8:]) > capacity > min(fullest)  # overflowing and fitting bins
    wants = []
    for name in ("tn_hash_encode_bwd", "tn_hash_encode_bwd_sorted from level 0", "hash_encode_bwd bucketed=True", "hash_encode_bwd overlap defer"):
        wants.append(assert_exact(BY_NAME[name], grid, case))
    assert all(torch.equal(bits(w), bits(wants[0])) for w in wants)
    assert_exact(BY_NAME["tn_hash_encode_bwd_sorted from the middle"], grid, case)


def test_same_index_pair_in_different_cells():
    """T = 2^12 (one slice): two cells with the same x and different (y, z) whose floor-(y, z) hashes agree modulo T give records with
    the SAME 16-bit index pair; with the samples alternating between the cells the owner pass merges them as one run — they are the
    same two entries, so the sums must still be right"""
    L, log2T = 8, 12
    grid = Grid.get(L, log2T, 512)
    level = L - 1
    side = int(grid.scalings[level])
    y, z = np.meshgrid(np.arange(2, side - 2), np.arange(2, side - 2), indexing="ij")
    h = ((y * R._P1) ^ (z * R._P2)) % grid.T
    order = np.argsort(h.reshape(-1), kind="stable")
    twin = np.flatnonzero(np.diff(h.reshape(-1)[order]) == 0)[0]
    (ya, za), (yb, zb) = ((int(y.reshape(-1)[i]), int(z.reshape(-1)[i])) for i in order[twin:twin + 2])
    assert (ya, za) != (yb, zb) and ((ya * R._P1) ^ (za * R._P2)) % grid.T == ((yb * R._P1) ^ (zb * R._P2)) % grid.T
    n = 600
    cells = np.where((np.arange(n) % 2 == 0)[:, None], np.array([[77, ya, za]]), np.array([[77, yb, zb]]))
    ks = np.random.default_rng(12).integers(1, 4, size=(n, 3))
    case = R.crafted_case("twins", grid.scalings, log2T, False, level, cells, ks, seed=12)
    fl, ce, _ = R.frozen_cell(R.normalized(case.positions, case.space)[0], grid.scalings[level])
    pair = ((ce[:, 0] ^ (fl[:, 1] * R._P1) ^ (fl[:, 2] * R._P2)) % grid.T) | (((fl[:, 0] ^ (fl[:, 1] * R._P1) ^ (fl[:, 2] * R._P2)) % grid.T) << 16)
    other_cell = (fl[1:] != fl[:-1]).any(axis=1)
    assert len(set(pair.tolist())) == 1 and int(other_cell.sum()) >= 100
    for form in _forms_on(L):
        assert_exact(form, grid, case)


def test_grid_stride_pass_of_the_atomic_kernel():
    """2^20 + 7 samples x 16 levels: more waves than the 2^16 blocks of the launch hold, the rest is the grid-stride loop's second
    pass.  Positions from the 343 points j / 8 of the unit box, d_enc in {-1, 0, 1}: up to ~1e4 terms per entry, still exact.
    Once, in the atomic form only."""
    L, log2T, n = 16, 15, (1 << 20) + 7
    grid = Grid.get(L, log2T, 2048)
    assert ((n + 63) // 64) * L > 4 * (1 << 16)
    case = R.exact_sum_large(grid.scalings, log2T, n)
    assert case.counts.max() >= 2000
    assert_exact(BY_NAME["tn_hash_encode_bwd"], grid, case, reps=1)


def test_accumulates_onto_a_prefilled_table():
    """(+=), spelled out on one case: the touched slots hold start + sum, every other slot of the call's levels, every row of the
    other levels and the guard rows keep the bits of the start"""
    grid = Grid.get(16, 15, 2048)
    case = next(c for c in grid.exact(False) if c.label.startswith("runs:random"))
    for name, (lo, hi) in (("tn_hash_encode_bwd_levels [3,7)", (3, 7)), ("tn_hash_encode_bwd_sorted from the middle", (8, 16)),
                           ("tn_hash_encode_bwd_spread", (0, 16))):
        got, _ = scatter(BY_NAME[name], grid, case.space, case.positions, case.d_enc, True)
        got = got.cpu().numpy()
        touched = np.zeros(grid.rows * 2, dtype=bool)
        inside = (case.slots >= lo * 2 * grid.T) & (case.slots < hi * 2 * grid.T)
        touched[case.slots[inside]] = True
        assert inside.any() and (~inside).any() == (hi - lo < 16)
        assert np.array_equal(got.reshape(-1)[~touched].view(np.int32), grid.start.reshape(-1)[~touched].view(np.int32))
        assert np.array_equal(got.reshape(-1)[case.slots[inside]].astype(np.float64),
                              grid.start.reshape(-1)[case.slots[inside]].astype(np.float64) + case.sums[inside])
        assert np.abs(grid.start).max() == R.START_MAX and (got.reshape(-1)[touched] != grid.start.reshape(-1)[touched]).any()


# ----------------------------------------------------------------------------------------------------------------------
# B. bounded cases
# ----------------------------------------------------------------------------------------------------------------------
def assert_bounded(form: Form, grid: Grid, tag: str, got: torch.Tensor, ref) -> float:
    """|got - (start + g)| <= (K_CONTRIBUTION + m) eps (|start| + B) per entry of the form's levels, after printing the worst
    ratio; entries without a term, and the rows of every other level, keep the start's bits.  ``ref``: (g, B, m) on the device."""
    g, B, m = ref
    lo, hi = form.levels(grid.L)
    inside = torch.zeros(grid.rows, 1, dtype=torch.bool, device=DEV)
    inside[lo * grid.T:hi * grid.T] = True
    start = grid.start_dev.double()
    live = inside & (m > 0)
    assert bool(torch.isfinite(got).all()), form.name
    assert torch.equal(bits(got)[~live], bits(grid.start_dev)[~live]), f"{form.name} {tag}: an entry without a term changed"
    err = (got.double() - (start + g)).abs()[live]
    scale = (start.abs() + B)[live]
    count = m[live]
    worst = float((err / (R.EPS32 * scale)).max()) if err.numel() else 0.0
    print(f"table-gradient bound | {form.name} | {grid.name} {tag} | worst {worst:.3f} | largest m {int(count.max()) if err.numel() else 0}")
    bad = err > (R.K_CONTRIBUTION + count).double() * R.EPS32 * scale + 1e-30
    assert not bool(bad.any()), f"{form.name} {grid.name} {tag}: {int(bad.sum())} entries outside (K + m) eps B, worst {worst:.2f} eps B"
    return worst


def _reference_on_device(grid: Grid, p32, d_enc):
    g, B, m = R.frozen_table_gradient(p32, d_enc, grid.scalings, grid.log2T)
    return torch.from_numpy(g).to(DEV), torch.from_numpy(B).to(DEV), torch.from_numpy(m).to(DEV)


@pytest.mark.parametrize("contraction", [False, True], ids=["box", "contraction"])
@pytest.mark.parametrize("L,log2T,max_res", GRIDS, ids=GRID_IDS)
def test_bounded_cases_every_form(L, log2T, max_res, contraction):
    """every sample count of COUNTS (the first n of the shuffled cases; 4097 cycles through all of them), d_enc normal with 20 %
    zero rows, every form, both calls of each"""
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32, sel = grid.mixed(contraction)
    rng = np.random.default_rng(L + 7 * contraction)
    for n in COUNTS:
        idx = np.resize(np.arange(len(cases)), n)
        d_enc = rng.standard_normal((n, 2 * L)).astype(np.float32)
        d_enc[rng.random(n) < 0.2] = 0.0
        ref = _reference_on_device(grid, p32[idx], d_enc)
        for form in _forms_on(L):
            for got in scatter(form, grid, space, cases.positions[idx], d_enc, False):
                assert_bounded(form, grid, f"{'contraction' if contraction else 'unit box'} n={n}", got, ref)


@pytest.mark.parametrize("L,log2T,max_res", [(16, 15, 2048), (5, 13, 128)], ids=["L16-T15", "L5-T13"])
def test_bounded_cases_one_level_at_a_time(L, log2T, max_res):
    """d_enc zero outside one level: a level that reads another level's scale, or writes another level's rows, shows here"""
    grid = Grid.get(L, log2T, max_res)
    cases, space, p32, sel = grid.mixed(False)
    n = len(cases)
    rng = np.random.default_rng(L)
    forms = [BY_NAME[k] for k in ("tn_hash_encode_bwd", "tn_hash_encode_bwd_spread", "tn_hash_encode_bwd_sorted from level 0",
                                  "hash_encode_bwd bucketed=int")]
    for l in range(L):
        d_enc = np.zeros((n, 2 * L), dtype=np.float32)
        d_enc[:, 2 * l:2 * l + 2] = rng.standard_normal((n, 2))
        ref = _reference_on_device(grid, p32, d_enc)
        assert int((ref[2][l * grid.T:(l + 1) * grid.T] > 0).sum()) > 0 and int(ref[2].sum()) == int(ref[2][l * grid.T:(l + 1) * grid.T].sum())
        for form in forms:
            got, _ = scatter(form, grid, space, cases.positions, d_enc, False, reps=1)
            assert_bounded(form, grid, f"unit box one-hot level {l}", got, ref)


def test_spread_one_ulp_below_the_far_face():
    """p one ulp below 1 on every axis: ceil(sx) is the level's highest vertex (index = the scaling) — the last but one vertex of a
    dense copy's side.  The offsets 1 - 2^-20 ... make the products inexact, so this one is held to the bound; its exact
    counterpart (offsets k / 4 in the last cell) is the family's ``top-vertex`` case."""
    grid = Grid.get(16, 15, 2048)
    n = 300
    pos = np.full((n, 3), np.nextafter(np.float32(1.0), np.float32(0.0)), dtype=np.float32)
    p32, sel = R.normalized(pos, R.UNIT_BOX)
    assert sel.all()
    for s in grid.scalings[:4]:
        assert np.array_equal(R.frozen_cell(p32[:1], s)[1][0], [int(s)] * 3)
    d_enc = np.random.default_rng(9).standard_normal((n, 32)).astype(np.float32)
    ref = _reference_on_device(grid, p32, d_enc)
    for name in ("tn_hash_encode_bwd_spread", "tn_hash_encode_bwd", "hash_encode_bwd bucketed=True"):
        for got in scatter(BY_NAME[name], grid, R.UNIT_BOX, pos, d_enc, False):
            assert_bounded(BY_NAME[name], grid, "one ulp below 1", got, ref)


# ----------------------------------------------------------------------------------------------------------------------
# C. refusals and no-ops
# ----------------------------------------------------------------------------------------------------------------------
def _untouched(grid, buf, out):
    torch.cuda.synchronize()
    return guards_intact(buf, grid.rows) and torch.equal(bits(out), bits(grid.start_dev))


def _inputs(grid, n=100):
    case = grid.exact(False)[-1]
    pos = torch.from_numpy(np.resize(case.positions, (n, 3))).to(DEV)
    d_enc = torch.ones(n, 2 * grid.L, device=DEV)
    buf, out = guarded(grid)
    out.copy_(grid.start_dev)
    return pos, d_enc, buf, out, c_space(R.UNIT_BOX)


def test_no_ops_return_ok_and_touch_nothing():
    grid = Grid.get(16, 15, 2048)
    lib, st = _lib(), _hip.current_stream()
    pos, d_enc, buf, out, sp = _inputs(grid)
    p, d, o = pos.data_ptr(), d_enc.data_ptr(), out.data_ptr()
    ws = _workspace("sorted", lib.tn_hash_encode_bwd_sorted_workspace_bytes(grid.c, 100, 0))
    sws = _workspace("spread", lib.tn_hash_encode_bwd_spread_workspace_bytes(grid.c))
    assert lib.tn_hash_encode_bwd(grid.c, sp, p, d, 0, o, st) == _hip.TN_OK
    assert lib.tn_hash_encode_bwd_levels(grid.c, sp, p, d, 0, o, 0, 16, st) == _hip.TN_OK
    assert lib.tn_hash_encode_bwd_spread(grid.c, sp, p, d, 0, o, 0, 16, sws.data_ptr(), sws.numel(), st) == _hip.TN_OK
    assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, p, d, 0, o, 0, ws.data_ptr(), ws.numel(), st) == _hip.TN_OK
    for l in (0, 5, 16):
        assert lib.tn_hash_encode_bwd_levels(grid.c, sp, p, d, 100, o, l, l, st) == _hip.TN_OK
        assert lib.tn_hash_encode_bwd_spread(grid.c, sp, p, d, 100, o, l, l, sws.data_ptr(), sws.numel(), st) == _hip.TN_OK
    assert _untouched(grid, buf, out)


def test_sorted_form_refusals():
    grid = Grid.get(16, 15, 2048)
    lib, st = _lib(), _hip.current_stream()
    n = 100
    pos, d_enc, buf, out, sp = _inputs(grid, n)
    p, d, o = pos.data_ptr(), d_enc.data_ptr(), out.data_ptr()
    need = lib.tn_hash_encode_bwd_sorted_workspace_bytes(grid.c, n, 0)
    ws = _workspace("refusals", need + 64)
    for first in (-1, 16):
        assert lib.tn_hash_encode_bwd_sorted_workspace_bytes(grid.c, n, first) == 0
        assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, p, d, n, o, first, ws.data_ptr(), ws.numel(), st) == TN_ERR_UNSUPPORTED
    assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, p, d, n, o, 0, ws.data_ptr(), need - 1, st) == TN_ERR_WORKSPACE
    assert ws.data_ptr() % 16 == 0
    for shift in (4, 8):
        assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, p, d, n, o, 0, ws.data_ptr() + shift, need, st) != _hip.TN_OK
    assert _untouched(grid, buf, out)
    # (and the same call with nothing wrong goes through)
    assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, p, d, n, o, 0, ws.data_ptr(), need, st) == _hip.TN_OK
    assert not _untouched(grid, buf, out)


def test_sorted_form_refuses_x_coordinates_that_reach_across_slices():
    """more than one slice and a finest scaling with + 2 >= 2^14: the two x-neighbours of a record could fall into different
    slices.  No workspace size, no advised level, the call refused, d_table untouched."""
    grid = Grid(2, 15, 32768, scalings=[16.0, 32768.0])
    lib, st = _lib(), _hip.current_stream()
    n = 100
    pos, d_enc, buf, out, sp = _inputs(Grid.get(16, 15, 2048), n)
    buf, out = guarded(grid)
    out.copy_(grid.start_dev)
    d_enc = d_enc[:, :4].contiguous()
    assert lib.tn_hash_encode_bwd_sorted_workspace_bytes(grid.c, n, 0) == 0
    assert lib.tn_hash_encode_bwd_sorted_first_level(grid.c, n) == -1
    ws = _workspace("refusals", 1 << 20)
    assert lib.tn_hash_encode_bwd_sorted(grid.c, sp, pos.data_ptr(), d_enc.data_ptr(), n, out.data_ptr(), 0, ws.data_ptr(), ws.numel(), st) == TN_ERR_UNSUPPORTED
    assert _untouched(grid, buf, out)
    # one slice (log2T = 14) has no such limit
    one = Grid(2, 14, 32768, scalings=[16.0, 32768.0])
    assert lib.tn_hash_encode_bwd_sorted_workspace_bytes(one.c, n, 0) > 0


def test_spread_form_refuses_a_short_workspace():
    grid = Grid.get(16, 15, 2048)
    lib, st = _lib(), _hip.current_stream()
    pos, d_enc, buf, out, sp = _inputs(grid)
    need = lib.tn_hash_encode_bwd_spread_workspace_bytes(grid.c)
    sides = [int(s) + 2 for s in grid.scalings if int(s) + 2 <= 48]
    assert need == 16 * sum(v ** 3 for v in sides) * 8 and len(sides) == 4
    ws = _workspace("spread", need)
    assert lib.tn_hash_encode_bwd_spread(grid.c, sp, pos.data_ptr(), d_enc.data_ptr(), 100, out.data_ptr(), 0, 16, ws.data_ptr(), need - 1, st) == TN_ERR_WORKSPACE
    assert _untouched(grid, buf, out)
