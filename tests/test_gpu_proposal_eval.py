"""The eval proposal pass on the device (tn_proposal_sample_fwd), level by level against the fp64 reference of
tests/proposal_eval_reference.py, in every form the pass can take:

  wave           proposal_kernel (kernel_family 2): one ray per wave
  general        proposal_rays_kernel<0, 0, false>, <5, 4, false> and <-1, -1, false> (kernel_family 1, every per-level output asked
                 for), on hashed grids, on the (5, 4) dense levels tn_hashgrid_prepare gives at 64 MB and on a (2, 2) budget
  LEAN           proposal_rays_kernel<0, 0, true> and <5, 4, true> (kernel_family 1, no per-level output, P0 < 64 or P1 < 32)
  split          proposal_density_segments_kernel<0 | 5, 0>, <0 | 4, 1> + proposal_resample_kernel<0>, <1> (the same with P0 >= 64, P1 >= 32)

Against fp64, stage by stage from the device's OWN output of the stage before (proposal_eval_reference.judge): the wave and the general
forms, every output — spacing_bins[0..2], eucl_bins[0..2], weights[0..1], prop_depth_0 / 1 and the workspace edges at tn_ws_bin — for
R in {1, 63, 64, 65, 129} x six (P0, P1, S) x both spacings, eval; training (one draw a ray, one an edge, anneal 0.75) at (70, 37, 48).
Bit for bit: the LEAN and the split forms against the general form of the same grids (workspace edges and both medians), the first,
a middle and the last tile of a call that takes a second grid-stride round against those rays run on their own, and the pinned
families (zero density, overflowing density, caller-chosen draws) in all four forms.  No bound was tuned against what the device
gives; run with -s for the worst ratio of every check (profiles/micro/proposal_eval_bounds.txt holds one such run).  Every output
lives in a buffer with two guard rows behind it, pre-filled with a sentinel; the workspace has a guard behind it too."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import proposal_eval_reference as P
from tests import ray_forward_reference as RF
from tests.test_gpu_field_eval import DevProposal, Out, config, dev, linear, space
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
SENT = f32(P.SENTINEL)
BUDGETS = {"hashed": (None, (0, 0)), "dense": (64 << 20, (5, 4)), "mixed": (1 << 20, (2, 2))}
WAVE_SLOTS = 256 * 4 * 4   # kPropRaysMaxBlocks (256 CUs x TN_PROP_WAVES) x 4 waves: the tiles of one grid-stride round


class DevNets(DevProposal):
    """the two proposal networks of a reference case on the device, their grids hashed or re-laid by tn_hashgrid_prepare"""

    def __init__(self, nets, budget=None, counts=(0, 0)):
        lib = _hip.load()
        self.keep, self.nets = [], []
        for level, n in enumerate(nets):
            table = dev(n.grid.table)
            d = _hip.tn_density_field()
            d.grid.table, d.grid.num_levels, d.grid.log2_hashmap_size = table.data_ptr(), 5, n.grid.log2T
            for l in range(5):
                d.grid.scalings[l] = float(n.grid.scalings[l])
            if budget is not None:
                nbytes = lib.tn_hashgrid_prepare_bytes(d.grid, budget)
                buf = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
                out = _hip.tn_hashgrid()
                _hip.check(lib.tn_hashgrid_prepare(d.grid, out, buf.data_ptr(), nbytes, _hip.current_stream()), "tn_hashgrid_prepare")
                self.keep.append(buf)
                d.grid = out
            assert d.grid.num_dense_levels == counts[level], (level, d.grid.num_dense_levels, counts)
            d.l0, d.l1 = linear(self.keep, n.w0, n.b0), linear(self.keep, n.w1, n.b1)
            d.space, d.average_init_density = space(True, P.SPACE.aabb), float(n.avg)
            self.keep.append(table)
            self.nets.append(d)


_NETS = {}


def dev_nets(nets, key, grids):
    if (key, grids) not in _NETS:
        _NETS[key, grids] = DevNets(nets, *BUDGETS[grids])
    return _NETS[key, grids]


@pytest.fixture(scope="module")
def nets():
    return P.random_nets(11)


def run(case: P.Case, dnets: DevNets, kernel_family: int, per_level: bool = True):
    """one tn_proposal_sample_fwd call -> every output asked for, the workspace edges un-tiled as "ws\""""
    lib, R, S = _hip.load(), case.R, case.S
    rc = config(S, case.lin, kernel_family=kernel_family, training=int(case.jitter is not None), pdf_anneal=float(case.anneal),
                per_sample_jitter=int(case.jper))
    rc.num_proposal_samples[0], rc.num_proposal_samples[1] = case.P0, case.P1
    ws_bytes = lib.tn_render_workspace_bytes(C.byref(rc), R)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    ws = torch.full((ws_bytes // 4 + 256,), float(SENT), device=DEV)
    keep = [dev(a) for a in case.rays] + [dev(case.lin0), dev(case.u1), dev(case.u2)]
    ins = _hip.tn_render_inputs()
    ins.origins, ins.directions, ins.nears, ins.fars, ins.lin_bins0, ins.u1, ins.u2 = (t.data_ptr() for t in keep)
    if case.jitter is not None:
        keep.append(dev(case.jitter))
        ins.jitter = keep[-1].data_ptr()
    bufs = dict(depth0=Out(R), depth1=Out(R))
    outs = _hip.tn_render_outputs()
    outs.prop_depth_0, outs.prop_depth_1 = bufs["depth0"].ptr, bufs["depth1"].ptr
    if per_level:
        for L, n in enumerate(case.counts):
            bufs[f"spacing{L}"], bufs[f"eucl{L}"] = Out(R, n + 1), Out(R, n + 1)
            outs.spacing_bins[L], outs.eucl_bins[L] = bufs[f"spacing{L}"].ptr, bufs[f"eucl{L}"].ptr
            if L < 2:
                bufs[f"weights{L}"] = Out(R, n)
                outs.weights[L] = bufs[f"weights{L}"].ptr
    _hip.check(lib.tn_proposal_sample_fwd(C.byref(dnets.nets[0]), C.byref(dnets.nets[1]), C.byref(rc), C.byref(ins), C.byref(outs), R,
                                          ws.data_ptr(), ws_bytes, _hip.current_stream()), "tn_proposal_sample_fwd")
    got = {k: b.read(k) for k, b in bufs.items()}
    host = ws.cpu().numpy()
    assert np.all(host[ws_bytes // 4:] == SENT), "the workspace's guard was written"
    tiles = (R + 63) // 64
    got["ws"] = host[:tiles * (S + 1) * 64].reshape(tiles, S + 1, 64).transpose(0, 2, 1).reshape(tiles * 64, S + 1)[:R].copy()
    assert np.all(np.isfinite(got["ws"]))
    return got


FAMILY = {2: P.WAVE, 1: P.SERIAL}
FORM = {2: "wave", 1: "general"}
_RECORD, _SHARES = [], []


def level_by_level(nets, key, R, shape, lin, seed, jitter=None, anneal=1.0):
    for grids in BUDGETS:
        dnets = dev_nets(nets, key, grids)
        for kf in (2, 1):
            name = f"{FORM[kf]} {grids} R={R} {shape} lin={int(lin)}" + (f" jitter={jitter} anneal={anneal}" if jitter else "")
            case, out, share = P.general_case(lambda c: run(c, dnets, kf), FAMILY[kf], nets, R, shape, lin, seed, jitter, anneal)
            _SHARES.append((name, share))
            _RECORD.append((f"{FORM[kf]} {grids}" + (" training" if jitter else ""), P.judge(name, case, out, FAMILY[kf])))


@pytest.mark.parametrize("lin", [False, True])
@pytest.mark.parametrize("shape", P.SHAPES)
@pytest.mark.parametrize("R", P.R_EDGES)
def test_wave_and_general_forms_level_by_level(nets, R, shape, lin):
    level_by_level(nets, "random", R, shape, lin, 1000 * shape[2] + R)


@pytest.mark.parametrize("jitter,anneal", [("ray", 1.0), ("edge", 1.0), ("ray", 0.75)])
@pytest.mark.parametrize("R", P.R_EDGES)
def test_training_level_by_level(nets, R, jitter, anneal):
    level_by_level(nets, "random", R, P.TRAIN_SHAPE, False, 31 + R, jitter, anneal)


# ----------------------------------------------------------------------------------------------------------------------
# bit for bit across forms
# ----------------------------------------------------------------------------------------------------------------------
def same_edges_and_medians(name, a, b):
    for k in ("ws", "depth0", "depth1"):
        RF.same_bits(f"{name} {k}", a[k], b[k])


@pytest.mark.parametrize("grids", ["hashed", "dense"])
@pytest.mark.parametrize("shape", [(63, 31, 12), (64, 32, 25), (70, 37, 48)])   # LEAN one-launch, split, split with ragged segments
@pytest.mark.parametrize("R", P.R_EDGES)
def test_lean_and_split_equal_the_general_form(nets, R, shape, grids):
    dnets = dev_nets(nets, "random", grids)
    case = P.make_case(nets, P.mixed_rays(R, 7 * R + shape[2]), shape, False)
    general = run(case, dnets, 1)
    RF.same_bits("workspace", general["ws"], general["spacing2"])
    same_edges_and_medians(f"{'LEAN' if shape[0] < 64 else 'split'} {grids} R={R} {shape}", run(case, dnets, 1, per_level=False), general)


@pytest.mark.parametrize("form,grids,shape,R", [("split", "dense", (64, 32, 4), (WAVE_SLOTS // 8 + 1) * 64 + 1),
                                                ("LEAN", "hashed", (63, 31, 4), WAVE_SLOTS * 64 + 1)])
def test_tiles_of_a_second_grid_stride_round(nets, form, grids, shape, R):
    """split: 8 level-0 segments a tile, so 514 tiles are 4 112 virtual tiles on 4 096 wave slots; LEAN: 4 097 tiles.  The last tile
    (one ray, ragged) is the second round.  Device results only."""
    dnets = dev_nets(nets, "random", grids)
    case = P.make_case(nets, P.mixed_rays(R, 5), shape, False)
    tiles = (R + 63) // 64
    assert tiles * (8 if form == "split" else 1) > WAVE_SLOTS >= (tiles - 2) * (8 if form == "split" else 1)
    whole = run(case, dnets, 1, per_level=False)
    for tile in (0, tiles // 2, tiles - 1):
        rows = slice(tile * 64, min(tile * 64 + 64, R))
        sub = case._replace(rays=P.F.Rays(*(a[rows] for a in case.rays)))
        alone = run(sub, dnets, 1, per_level=False)
        same_edges_and_medians(f"{form} tile {tile} of {tiles}", {k: v[rows] for k, v in whole.items()}, alone)


# ----------------------------------------------------------------------------------------------------------------------
# the pinned families, all four forms
# ----------------------------------------------------------------------------------------------------------------------
FOUR_FORMS = [("wave", 2, True, (70, 37, 48)), ("general", 1, True, (70, 37, 48)), ("LEAN", 1, False, (63, 31, 12)), ("split", 1, False, (64, 32, 25))]


def pinned_runs(nets, key, R, seed, **case_kw):
    """(form, grids, case, outputs, the general serial form's outputs of the same case) for the four forms on hashed and dense grids"""
    for form, kf, per_level, shape in FOUR_FORMS:
        for grids in ("hashed", "dense"):
            dnets = dev_nets(nets, key, grids)
            kw = {k: v(shape) for k, v in case_kw.items()}
            case = P.make_case(nets, P.mixed_rays(R, seed), shape, False, **kw)
            out = run(case, dnets, kf, per_level)
            full = out if per_level else run(case, dnets, 1)
            if per_level:
                P.judge(f"{form} {grids} {key}", case, out, FAMILY[kf])
            else:
                same_edges_and_medians(f"{form} {grids} {key}", out, full)
            yield form, grids, case, out, full


def last_midpoint(eucl):
    e = np.asarray(eucl, f32)
    return RF.midpoints_fp32(e[:, -2:-1], e[:, -1:])[:, 0]


@pytest.mark.parametrize("R", [65, 129])
def test_zero_density_every_weight_zero(nets, R):
    zero = [n._replace(avg=0.0) for n in nets]
    for form, grids, case, out, full in pinned_runs(zero, "zero", R, 3):
        for L in range(2):
            RF.same_bits(f"{form} weights{L}", full[f"weights{L}"], np.zeros((R, case.counts[L]), f32))
            RF.same_bits(f"{form} prop_depth_{L}: the last sample's mid-point", out[f"depth{L}"], last_midpoint(full[f"eucl{L}"]))
        assert np.all(np.isfinite(out["ws"])) and np.all(np.diff(out["ws"], axis=1) >= 0)


@pytest.mark.parametrize("R", [65, 129])
def test_overflowing_density_first_weight_one(nets, R):
    """density +inf: sample 0 takes everything; on the near = far ray (ray 1) 0 x inf = NaN zeroes every weight"""
    over = [n._replace(b1=np.array([P.OVERFLOW_BIAS], f32)) for n in nets]
    live = np.arange(R) != 1
    for form, grids, case, out, full in pinned_runs(over, "overflow", R, 4):
        for L in range(2):
            w, e = full[f"weights{L}"], full[f"eucl{L}"]
            assert np.all(e[live, 1] > e[live, 0]) and np.all(e[1] == e[1, 0])   # the premise: delta_0 > 0, and 0 on ray 1
            want = np.zeros_like(w)
            want[live, 0] = 1
            RF.same_bits(f"{form} weights{L}", w, want)
            first = RF.midpoints_fp32(e[:, :1], e[:, 1:2])[:, 0]
            RF.same_bits(f"{form} prop_depth_{L}", out[f"depth{L}"], np.where(live, first, last_midpoint(e)))


@pytest.mark.parametrize("R", [65, 129])
def test_caller_chosen_draws(nets, R):
    """sorted u1 and u2 holding 0.0, a repeated value, 1.0 and 1.25: u = 0 returns the level's first edge, u >= 1 its last edge,
    repeated draws repeated bits"""
    for form, grids, case, out, full in pinned_runs(nets, "random", R, 6, u1=lambda s: P.pinned_u(s[1]), u2=lambda s: P.pinned_u(s[2])):
        for L, u in ((1, case.u1), (2, case.u2)):
            prev, new = full[f"spacing{L - 1}"], (out["ws"] if L == 2 else full["spacing1"])
            rep = np.flatnonzero(np.diff(u) == 0)
            assert u[0] == 0 and len(rep) == 1 and (u >= 1).sum() == 2 and np.all(np.diff(u) >= 0)
            RF.same_bits(f"{form} level {L} u = 0", new[:, 0], prev[:, 0])
            RF.same_bits(f"{form} level {L} u >= 1", new[:, u >= 1], np.repeat(prev[:, -1:], 2, axis=1))
            RF.same_bits(f"{form} level {L} repeated u", new[:, rep[0]], new[:, rep[0] + 1])
            P.sorted_within(f"{form} level {L}", new, prev[:, 0], prev[:, -1])


def test_zz_print_the_worst_ratios():
    """(last in the module) one line per form and grid: the worst ratio to the bound of every output over the tests above, and the
    share of rays redrawn for a median near a tie"""
    print()   # (the rows start on a line of their own behind pytest's progress mark)
    table = {}
    for name, worst in _RECORD:
        row = table.setdefault(name, {})
        for k, v in worst.items():
            row[k] = max(row.get(k, 0.0), v)
    for name in sorted(table):
        print(f"{name:24s} " + "  ".join(f"{k} {v:.4f}" for k, v in table[name].items()))
    shares = [s for _, s in _SHARES]
    print(f"cases {len(shares)}; rays redrawn for a median near a tie: largest share of a case {max(shares, default=0.0):.4f}, "
          f"cases with any {sum(s > 0 for s in shares)} (cap {P.REDRAW_CAP})")
    assert all(v <= 1.0 for row in table.values() for v in row.values()) and all(s <= P.REDRAW_CAP for s in shares)
