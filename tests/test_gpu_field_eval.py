"""The eval field pass on the device, ray by ray against the fp64 reference of tests/field_eval_reference.py, through the C entry
points tn_proposal_sample_fwd (for the workspace and the final level's spacing edges the reference starts from),
tn_field_render_fwd, tn_field_render_chunked_fwd and tn_expected_depth_clip_chunked, in every form the field pass can take:

  valu          main_valu_kernel (no prepared blob)
  mfma          main_mfma_kernel (kernel_family 2), also with weights[2] requested: the one place per-sample weights exist
  rays          main_mfma_rays_kernel, the whole march (kernel_family 1, sample_split 1), hashed and dense grids
  split k       the sample-split form + segments_combine_kernel, k = 2, 3, 4 and a k the library caps
  tail          field_records_kernel + field_replay_kernel: tail_slots 16, tail_balance 0, 2, 3, 2 305 rays
  f16x3, bf16x6 main_split_rays_kernel

Bit for bit: the first-hit family (every weight exactly 0 or 1) through every form: rgb 1/2, thermal b, accumulation, the median
AND the expected depth equal to the named sample's fp32 mid-point, a miss ray's expected depth equal to its call's or chunk's
smallest mid-point, the per-chunk depth bounds.  Bounded per ray by the counted bounds of the reference (none tuned against what the
device gives; run with -s for the worst ratio of every check; profiles/micro/field_eval_bounds.txt holds one such run): random
sparse fields through every form.  The median depth is compared bit for bit on EVERY ray: the builder redraws, from the fp64
reference alone, the rays whose cumulative weight comes within its bound of 0.5, and asserts that none is left.  Every output lives
in a buffer with two guard rows behind it, pre-filled with a sentinel.

Where the FAST kernels reach a v_rcp_f32 division of the geometry (samples at |x|_inf >= 1 under the contraction, the piecewise
sampler beyond far = 1: the "beyond" scene) the reference bounds their geometry instead of freezing it (field_eval_reference,
"FAST geometry"); everywhere else field_eval_reference.geometry's fast_exact holds for every ray and they are held to the frozen
bits.  NaN handling: a first-hit field whose density overflows puts a NaN optical depth on the path of every ray that starts outside
the box (test_nan_on_the_path_zeroes_everything_behind_it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import field_eval_reference as F
from thermo_nerf_amd import _hip
from thermo_nerf_amd.samplers import linspace_bins, pdf_positions

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
SENT = f32(F.SENTINEL)
P = (64, 32)
SLOTS = 16
TAIL_RAYS = SLOTS * 64 * 2 + 4 * 64 + 1   # 2 305: two rounds, four whole tiles and a ragged fifth


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).to(DEV)


class Out:
    """[R, w] output with two guard rows, everything pre-filled with the sentinel"""

    def __init__(self, R, w=None):
        self.R, self.w, self.vector = R, w or 1, w is None
        self.t = torch.full(((R + 2) * self.w,), float(SENT), device=DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self, name):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy().reshape(self.R + 2, self.w)
        assert np.all(a[self.R:] == SENT), f"{name}: guard rows written"
        out = a[:self.R]
        return out[:, 0].copy() if self.vector else out.copy()


def linear(keep, w, b):
    wt, bt = dev(w), dev(b)
    keep += [wt, bt]
    return _hip.tn_linear(wt.data_ptr(), bt.data_ptr(), w.shape[1], w.shape[0])


def space(contraction, aabb):
    s = _hip.tn_space()
    s.contraction = 1 if contraction else 0
    for i in range(3):
        s.aabb_min[i], s.aabb_max[i] = float(aabb[0][i]), float(aabb[1][i])
    return s


class DevField:
    """a hand-built tn_thermal_field over a reference Field; struct(kind, dense) adds the prepared blobs"""

    def __init__(self, field: F.Field):
        self.field, self.keep, self.cache = field, [], {}
        self.table, self.emb = dev(field.table), dev(field.emb)

    def struct(self, kind=None, dense=False):
        if (kind, dense) in self.cache:
            return self.cache[kind, dense]
        lib, fd, keep = _hip.load(), self.field, self.keep
        f = _hip.tn_thermal_field()
        g = _hip.tn_hashgrid()
        g.table, g.num_levels, g.log2_hashmap_size = self.table.data_ptr(), F.LEVELS, fd.log2T
        for l in range(F.LEVELS):
            g.scalings[l] = float(fd.scalings[l])
        if dense:
            nbytes = lib.tn_hashgrid_prepare_bytes(g, 16 << 20)
            buf = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=DEV)
            out = _hip.tn_hashgrid()
            _hip.check(lib.tn_hashgrid_prepare(g, out, buf.data_ptr(), nbytes, _hip.current_stream()), "tn_hashgrid_prepare")
            assert out.num_dense_levels >= 6
            keep.append(buf)
            g = out
        f.grid = g
        for name in ("base0", "base1", "head0", "head1", "head2", "th0", "th1", "thead"):
            setattr(f, name, linear(keep, fd.w[name + "_w"], fd.w[name + "_b"]))
        f.appearance, f.num_images, f.app_dim, f.geo_feat_dim = self.emb.data_ptr(), fd.emb.shape[0], F.APP, F.GF
        f.use_average_appearance, f.sh_shifted = int(fd.use_avg), int(fd.sh_shifted)
        f.space, f.average_init_density = space(fd.contraction, fd.aabb), float(fd.avg)
        if kind is not None:
            for member, which in (("prepared", ""), ("prepared_f16x3", "_f16x3"), ("prepared_bf16x6", "_bf16x6")):
                if which and which[1:] != kind:
                    continue
                nbytes = getattr(lib, f"tn_field_prepare{which}_bytes")(f)
                assert nbytes > 0
                buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
                _hip.check(getattr(lib, f"tn_field_prepare{which}")(f, buf.data_ptr(), nbytes, _hip.current_stream()), "prepare" + which)
                keep.append(buf)
                setattr(f, member, buf.data_ptr())
        self.cache[kind, dense] = f
        return f


class DevProposal:
    """two proposal networks (5 levels, 16 hidden, contraction on): uniform (all zero: density 1 everywhere, so that the edges depend
    on a ray's near and far planes alone) or random"""

    def __init__(self, seed=None):
        r = np.random.default_rng(0 if seed is None else seed)
        self.keep, self.nets = [], []
        for level in range(2):
            scale = 0.0 if seed is None else 1.0
            table = dev(r.uniform(-1, 1, (5 << 10, 2)) * scale)
            d = _hip.tn_density_field()
            d.grid.table, d.grid.num_levels, d.grid.log2_hashmap_size = table.data_ptr(), 5, 10
            for l, s in enumerate((16.0, 26.0, 45.0, 76.0, 127.0 + 128 * level)):
                d.grid.scalings[l] = s
            d.l0 = linear(self.keep, r.standard_normal((16, 10)) * 0.6 * scale, r.standard_normal(16) * 0.2 * scale)
            d.l1 = linear(self.keep, r.standard_normal((1, 16)) * 0.6 * scale, np.zeros(1))
            d.space, d.average_init_density = space(True, [[-1, -1, -1], [1, 1, 1]]), 1.0
            self.keep.append(table)
            self.nets.append(d)


def config(S, lin, **over):
    rc = _hip.tn_render_config()
    rc.num_proposal_samples[0], rc.num_proposal_samples[1] = P
    rc.num_nerf_samples, rc.training, rc.pdf_anneal, rc.initial_sampler = S, 0, 1.0, int(lin)
    for k, v in over.items():
        setattr(rc, k, v)
    return rc


# form name -> (flavour, prepared blob, dense grid, config members).  The library caps a split request at
# min(8, S / 8, (max(P0, P1) + P1 + 1 - S) / 12): with P = (64, 32) the k used is S = 25: 2, 3, 3, 3; S = 48: 2, 3, 4, 4; S = 64: 2, 2, 2, 2
# for "split 2 / 3 / 4 / 8"; S <= 12 marches whole.
WHOLE = dict(kernel_family=1, sample_split=1, tail_balance=1)
FORMS = {
    "valu": (F.VALU, None, False, dict(kernel_family=2)),
    "mfma": (F.MFMA, "f32", False, dict(kernel_family=2)),
    "mfma dense": (F.MFMA, "f32", True, dict(kernel_family=2)),
    "rays hashed": (F.RAYS, "f32", False, WHOLE),
    "rays dense": (F.RAYS, "f32", True, WHOLE),
    "split 2": (F.RAYS, "f32", True, dict(kernel_family=1, sample_split=2)),
    "split 3": (F.RAYS, "f32", False, dict(kernel_family=1, sample_split=3)),
    "split 4": (F.RAYS, "f32", True, dict(kernel_family=1, sample_split=4)),
    "split 8": (F.RAYS, "f32", True, dict(kernel_family=1, sample_split=8)),   # above the library's cap for every S here
    "f16x3": (F.F16X3, "f16x3", True, WHOLE),
    "bf16x6": (F.BF16X6, "bf16x6", False, WHOLE),
}
TAIL_FORMS = {f"tail {tb}": (F.RAYS, "f32", tb != 2, dict(kernel_family=1, sample_split=1, tail_balance=tb, tail_slots=SLOTS)) for tb in (0, 2, 3)}
TAIL_FORMS["tail off"] = (F.RAYS, "f32", True, dict(kernel_family=1, sample_split=1, tail_balance=1, tail_slots=SLOTS))


class Call:
    """the rays of one call on the device, its workspace (sized for every form, the tail records included) and the proposal pass"""

    def __init__(self, rays: F.Rays, S, lin, prop: DevProposal, prop_family=2):
        self.rays, self.S, self.lin, self.R = rays, S, lin, len(rays.nears)
        self.t = [dev(a) for a in rays]
        lib = _hip.load()
        self.ws_bytes = max(lib.tn_render_workspace_bytes(config(S, lin, **o), self.R) for o in
                            [WHOLE] + [v[3] for v in TAIL_FORMS.values()])
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=DEV)
        self.ins = _hip.tn_render_inputs()
        self.ins.origins, self.ins.directions, self.ins.nears, self.ins.fars = (t.data_ptr() for t in self.t)
        self.ins.lin_bins0 = linspace_bins(P[0], DEV).data_ptr()
        self.ins.u1 = pdf_positions(P[1] + 1, DEV, False).data_ptr()
        self.ins.u2 = pdf_positions(S + 1, DEV, False).data_ptr()
        edges = Out(self.R, S + 1)
        outs = _hip.tn_render_outputs()
        outs.spacing_bins[2] = edges.ptr
        rc = config(S, lin, kernel_family=prop_family)
        _hip.check(lib.tn_proposal_sample_fwd(C.byref(prop.nets[0]), C.byref(prop.nets[1]), C.byref(rc), C.byref(self.ins), C.byref(outs),
                                              self.R, self.ws.data_ptr(), self.ws_bytes, _hip.current_stream()), "tn_proposal_sample_fwd")
        self.spacing = edges.read("spacing_bins[2]")
        assert np.all(np.isfinite(self.spacing))

    def field(self, f, over, want_weights=False, chunk=None, clip=1):
        """-> dict of outputs (+ "weights", "bounds"); chunk = (first_ray, chunk_rays)"""
        lib, R, S = _hip.load(), self.R, self.S
        rc = config(S, self.lin, **over)
        bufs = dict(rgb=Out(R, 3), accumulation=Out(R), depth=Out(R), expected_depth=Out(R), thermal=Out(R))
        outs = _hip.tn_render_outputs()
        for k, b in bufs.items():
            setattr(outs, k, b.ptr)
        if want_weights:
            bufs["weights"] = Out(R, S)
            outs.weights[2] = bufs["weights"].ptr
        if chunk is None:
            _hip.check(lib.tn_field_render_fwd(C.byref(f), C.byref(rc), C.byref(self.ins), C.byref(outs), R, self.ws.data_ptr(),
                                               self.ws_bytes, _hip.current_stream()), "tn_field_render_fwd")
        else:
            slots = lib.tn_depth_bound_slots(chunk[0], R, chunk[1])
            bufs["bounds"] = Out(slots, 2)
            _hip.check(lib.tn_field_render_chunked_fwd(C.byref(f), C.byref(rc), C.byref(self.ins), C.byref(outs), R, self.ws.data_ptr(),
                                                       self.ws_bytes, chunk[0], chunk[1], bufs["bounds"].ptr, clip, _hip.current_stream()),
                       "tn_field_render_chunked_fwd")
        got = {k: b.read(k) for k, b in bufs.items()}
        if chunk is not None and not clip:
            got["expected_unclipped"] = got["expected_depth"]
            _hip.check(lib.tn_expected_depth_clip_chunked(bufs["expected_depth"].ptr, R, chunk[0], chunk[1], bufs["bounds"].ptr,
                                                          _hip.current_stream()), "tn_expected_depth_clip_chunked")
            got["expected_depth"] = bufs["expected_depth"].read("expected_depth")
        return got

    def used_split(self, f, over):
        return _hip.load().tn_render_sample_split(C.byref(f), C.byref(config(self.S, self.lin, **over)), self.R)

    def used_tail(self, f, over):
        return _hip.load().tn_render_tail_plan(C.byref(f), C.byref(config(self.S, self.lin, **over)), self.R)


def same_outputs(name, a, b):
    for k in F.OUTPUTS:
        F.same_bits(f"{name} {k}", a[k], b[k])


# ----------------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------------
_UNIFORM = {}


def uniform_proposal():
    if "p" not in _UNIFORM:
        _UNIFORM["p"] = DevProposal(None)
    return _UNIFORM["p"]


def planes(R, S, first_ray=0, chunk_rays=0):
    """near planes that differ from chunk to chunk (the chunks' smallest mid-points then differ) and a little within one"""
    ray = first_ray + np.arange(R)
    nears = (0.05 + 0.004 * ((ray // max(chunk_rays, 64)) % 5) + 0.0003 * (ray % 4)).astype(f32)
    return nears, np.full(R, 0.9 if S > 2 else 0.3, f32)


def exact_call(dfield, R, S, lin, ks, seed, first_ray=0, chunk_rays=0, targets=None, overflow=False):
    """the first-hit rays of a call: first in-box samples at 0, S - 1, mid-march, both sides of every seam of ``ks`` segments, and
    misses (a chunk's last ray always misses).  The edges come from a first proposal pass over placeholder rays with the same
    planes; the pass over the real rays must leave the same edges."""
    prop = uniform_proposal()
    nears, fars = planes(R, S, first_ray, chunk_rays)
    placeholder = F.random_rays(R, seed, True)._replace(nears=nears, fars=fars)
    edges = Call(placeholder, S, lin, prop).spacing
    pool = F.seam_targets(S, ks)
    pool = sorted(set(pool[:-1] + [S // 2, min(S // 2 + 1, S - 1)])) + [-1]
    given = targets is not None
    targets = np.array(targets if given else [pool[i % len(pool)] for i in range(R)])
    if chunk_rays and not given:
        targets[(first_ray + np.arange(R)) % chunk_rays == chunk_rays - 1] = -1
    case = F.first_hit_rays(dfield.field, edges, nears, fars, lin, targets, seed, first_ray, chunk_rays, overflow)
    call = Call(case.rays, S, lin, prop)
    F.same_bits("the edges do not depend on origin and direction", call.spacing, edges)
    return case, call


def check_exact(name, case, got):
    for k in F.OUTPUTS:
        F.same_bits(f"{name} {k}", got[k], case.want[k])


@pytest.fixture(scope="module")
def exact_fields():
    return {shifted: DevField(F.exact_field(7 + shifted, sh_shifted=bool(shifted), use_avg=bool(shifted))) for shifted in (0, 1)}


def test_fast_sigmoid_of_zero_is_one_half(exact_fields):
    """the exact family's premise, through an S = 1 call of every form: a hit ray returns its sample's own colour"""
    dfield = exact_fields[1]
    case, call = exact_call(dfield, 65, 1, False, (), 1)
    assert (case.index == 0).any() and (case.index < 0).any()
    for name, (fl, kind, dense, over) in FORMS.items():
        got = call.field(dfield.struct(kind, dense), over)
        F.same_bits(name, got["rgb"], np.full((65, 3), 0.5))
        check_exact(name, case, got)


@pytest.mark.parametrize("R,S,lin", [(1, 2, 0), (63, 12, 1), (64, 25, 0), (65, 48, 1), (129, 64, 0), (129, 25, 1)])
def test_first_hit_bit_for_bit_in_every_form(exact_fields, R, S, lin):
    dfield = exact_fields[lin]
    probe = Call(F.random_rays(R, 0, True), S, bool(lin), uniform_proposal())
    ks = {name: probe.used_split(dfield.struct(kind, dense), over) for name, (fl, kind, dense, over) in FORMS.items()}
    assert ks["rays dense"] == 1 and ks["f16x3"] == 1 and ks["valu"] == 1
    if S >= 16:
        assert ks["split 2"] == 2 and ks["split 8"] == min(S // 8, 8, (P[0] + P[1] + 1 - S) // 12) < 8
    case, call = exact_call(dfield, R, S, bool(lin), sorted(set(ks.values())), 100 * S + R)
    for name, (fl, kind, dense, over) in FORMS.items():
        f = dfield.struct(kind, dense)
        got = call.field(f, over)
        check_exact(f"{name} R={R} S={S}", case, got)
        if name == "mfma":
            w = call.field(f, over, want_weights=True)
            same_outputs("asking for the weights changes no other output", w, got)
            F.same_bits("weights", w["weights"], case.weights)


@pytest.mark.parametrize("S", [48, 25])
def test_first_hit_through_tail_records_and_replay(exact_fields, S):
    dfield = exact_fields[1]
    f = {name: dfield.struct(kind, dense) for name, (fl, kind, dense, over) in TAIL_FORMS.items()}
    probe = Call(F.random_rays(TAIL_RAYS, 0, True), S, False, uniform_proposal())
    plan = {name: probe.used_tail(f[name], TAIL_FORMS[name][3]) for name in TAIL_FORMS}
    assert plan == ({"tail 0": 3, "tail 2": 2, "tail 3": 3, "tail off": 1} if S == 48 else {"tail 0": 2, "tail 2": 2, "tail 3": 2, "tail off": 1})
    case, call = exact_call(dfield, TAIL_RAYS, S, False, sorted(set(plan.values())), S)
    assert (case.index[-65:] >= 0).any() and (case.index[-65:] < 0).any()   # the replayed tiles hold hits and misses
    for name, (fl, kind, dense, over) in TAIL_FORMS.items():
        check_exact(f"{name} S={S}", case, call.field(f[name], over))


@pytest.mark.parametrize("chunk_rays,form", [(64, "rays dense"), (128, "split 3"), (64, "valu"), (128, "mfma")])
def test_first_hit_chunked(exact_fields, chunk_rays, form):
    """first_ray != 0, several chunks, the last one partial: the per-chunk bounds bit for bit, clip 1, and clip 0 followed by
    tn_expected_depth_clip_chunked"""
    dfield, R, S, first = exact_fields[0], 321, 25, 128
    fl, kind, dense, over = FORMS[form]
    f = dfield.struct(kind, dense)
    probe = Call(F.random_rays(R, 0, True), S, True, uniform_proposal())
    case, call = exact_call(dfield, R, S, True, [probe.used_split(f, over)], chunk_rays, first, chunk_rays)
    assert case.bounds.shape[0] >= 3 and len(set(case.bounds[:, 0].tolist())) >= 3
    for clip in (1, 0):
        got = call.field(f, over, chunk=(first, chunk_rays), clip=clip)
        F.same_bits(f"{form} depth_bounds", got["bounds"], case.bounds)
        check_exact(f"{form} chunk {chunk_rays} clip {clip}", case, got)
        if not clip:   # unclipped: a miss ray's 0 / 1e-10 stays 0
            F.same_bits("unclipped", got["expected_unclipped"], np.where(case.index >= 0, case.want["expected_depth"], 0.0))


@pytest.mark.parametrize("S", [25, 48])
def test_nan_on_the_path_zeroes_everything_behind_it(S):
    """raw density 100: exp overflows, a sample outside the box has the density inf x 0 = NaN.  A ray that starts outside carries a
    NaN optical depth from sample 0 on: nan_to_num zeroes every weight behind it, although the ray enters the box later — at sample
    S - 1, mid-march or on either side of a segment seam, where the split form's T_j (NaN -> 0) and the replay must agree with the
    serial march.  A ray that starts inside keeps weight 1 on sample 0 and 0 behind it.  Bit for bit, every form."""
    dfield = DevField(F.exact_field(17, raw=F.OVERFLOW_RAW))
    case, call = exact_call(dfield, 129, S, False, (2, 3, 4), 700 + S, overflow=True)
    assert (case.index == 0).any() and (case.index < 0).sum() > 64 and not (case.index > 0).any()
    for name, (fl, kind, dense, over) in FORMS.items():
        f = dfield.struct(kind, dense)
        got = call.field(f, over)
        check_exact(f"{name} NaN S={S}", case, got)
        if name in ("mfma", "valu"):
            F.same_bits("weights", call.field(f, over, want_weights=True)["weights"], case.weights)
    case, call = exact_call(dfield, TAIL_RAYS, S, False, (2, 3), 800 + S, overflow=True)
    for name, (fl, kind, dense, over) in TAIL_FORMS.items():
        check_exact(f"{name} NaN S={S}", case, call.field(dfield.struct(kind, dense), over))


EARLY_FORMS = ("rays hashed", "rays dense", "f16x3", "bf16x6")   # the forms that take early_stop_transmittance


def test_first_hit_with_early_termination(exact_fields):
    """tile 0: every ray hits at sample 0, so the wave stops after ONE sample — its chunk's bounds must still be the smallest and
    the largest mid-point of all its samples; tile 1 holds misses and marches on.  Same bits as without the switch."""
    dfield, R, S = exact_fields[1], 128, 25
    pool = F.seam_targets(S, (3,))
    targets = [0] * 64 + [pool[i % len(pool)] for i in range(64)]
    case, call = exact_call(dfield, R, S, False, (), 9, 0, 64, targets=targets)
    for name in EARLY_FORMS:
        fl, kind, dense, over = FORMS[name]
        f = dfield.struct(kind, dense)
        over = dict(over, early_stop_transmittance=1e-3)
        whole = call.field(f, over)   # one chunk: a miss ray's expected depth is the CALL's smallest mid-point
        for k in F.OUTPUTS[:-1]:
            F.same_bits(f"{name} early {k}", whole[k], case.want[k])
        F.same_bits(f"{name} early expected_depth", whole["expected_depth"],
                    np.where(case.index >= 0, case.want["expected_depth"], case.bounds[:, 0].min()))
        got = call.field(f, over, chunk=(0, 64))
        F.same_bits(f"{name} early depth_bounds", got["bounds"], case.bounds)
        check_exact(f"{name} early chunked", case, got)


def test_median_on_a_tie():
    """the first sample's weight is 1/2 to the last bit (density a with fl32(fl32(delta a) log2 e) = 1: __expf gives v_exp_f32(-1)):
    the cumulative weight EQUALS the split there, and searchsorted(side = left) names that sample.  The premise is checked on the
    per-sample weights of main_mfma_kernel; main_valu_kernel (expf) has no such input."""
    R, S = 65, 16
    prop = uniform_proposal()
    o = np.tile(np.array([[0.27, 0.01, -0.02]], f32), (R, 1))
    d = np.tile(np.array([[1.0, 0.0, 0.0]], f32), (R, 1))
    for far in (0.2, 0.19, 0.18, 0.17, 0.16, 0.15):
        rays = F.Rays(o, d, np.full(R, 0.01, f32), np.full(R, far, f32))
        call = Call(rays, S, False, prop)
        g = F.geometry(F.exact_field(3), *rays, call.spacing, False)
        density = F.tie_density(g.delta[0, 0])
        if density is not None:
            break
    assert density is not None and g.sel.all() and g.fast_exact.all() and np.all(g.delta[:, 0] == g.delta[0, 0])
    dfield = DevField(F.tie_field(3, density))
    fl, kind, dense, over = FORMS["mfma"]
    w = call.field(dfield.struct(kind, dense), over, want_weights=True)["weights"]
    F.same_bits("premise: the first weight is one half", w[:, 0], np.full(R, 0.5))
    for name, (fl, kind, dense, over) in FORMS.items():
        if name == "valu":
            continue
        f = dfield.struct(kind, dense)
        if name.startswith("split"):
            assert call.used_split(f, over) == 2
        F.same_bits(f"{name}: the median on a tie", call.field(f, over)["depth"], g.step[:, 0])


# ----------------------------------------------------------------------------------------------------------------------
# the bounded family
# ----------------------------------------------------------------------------------------------------------------------
SCENES = {
    # name: (field arguments, rays inside the unit cube, uniform sampler, far, forms)
    "inside": (dict(contraction=True, sh_shifted=True, use_avg=True, log2T=11), True, False, None, "all"),
    "box": (dict(contraction=False, aabb=[[-1, -1, -1], [1, 1, 1]], sh_shifted=False, use_avg=False, log2T=10), False, True, None, "all"),
    # samples at and beyond |x|_inf = 1, the piecewise sampler beyond u = 1/2: the FAST forms' v_rcp_f32 geometry is BOUNDED here
    # (Geo.e_step / e_delta / e_p), not frozen: their bounds are about 1e-2, main_valu_kernel's stay at 1e-5
    "beyond": (dict(contraction=True, sh_shifted=True, use_avg=False, log2T=12), False, False, None, "all"),
}
_RECORD = []


def bounded_call(scene, R, S, seed, prop_family=2, near_eq_far=True, criterion=(F.WIDEST, (1, 2, 3, 4, 8))):
    """(field, call, geometry, samples by flavour): random rays through random proposal networks.  Rays whose fp64 cumulative weight
    comes within its bound of 0.5 at any sample are redrawn before anything is compared — under ``criterion``, by default the
    widest flavour there is (every count at its largest) in the serial march and in 2, 3, 4 and 8 segments; a ray's edges depend on that ray alone, so only the
    redrawn rays go through the proposal pass again, and the final pass covers them all.  field_eval_reference.judge asserts, form by
    form, that no such ray is left."""
    kw, inside, lin, far, forms = SCENES[scene]
    field = F.random_field(seed, **kw)
    prop = DevProposal(seed + 1)
    rays = F.random_rays(R, seed + 2, inside, far=far)
    if near_eq_far and R > 2:   # one ray with near == far: every sample at one point, every weight 0
        rays.nears[1] = rays.fars[1] = 0.5
    cache = {}

    def med_ok(sub):
        c = Call(sub, S, lin, prop, prop_family)
        g = F.geometry(field, *sub, c.spacing, lin, fast=True)
        s = F.field_samples(field, g.p32, g.sel, sub.directions, np.repeat(np.arange(len(sub.nears)), S), criterion[0], e_p=g.e_p)
        ok = np.ones(len(sub.nears), bool)
        for k in criterion[1]:   # (a bound is not monotone in the number of segments: every association the forms use is asked)
            ok &= F.render(s, g, criterion[0], k).med_ok
        return ok, c, g, s

    ok, call, g, s = med_ok(rays)
    redrawn = 0
    for attempt in range(40):
        if ok.all():
            break
        idx = np.flatnonzero(~ok)
        redrawn += len(idx)
        fresh = F.random_rays(len(idx), seed + 10 + attempt, inside, far=far)._replace(nears=rays.nears[idx], fars=rays.fars[idx])
        good = med_ok(fresh)[0]
        rays.origins[idx[good]], rays.directions[idx[good]] = fresh.origins[good], fresh.directions[good]
        ok[idx[good]] = True
    assert ok.all(), "a ray within its bound of the median split is left"
    if redrawn:
        call = Call(rays, S, lin, prop, prop_family)
        g = F.geometry(field, *rays, call.spacing, lin, fast=True)
    else:
        cache[criterion[0].name] = s
    assert scene == "beyond" or (g.e_p is None and redrawn <= 0.1 * R + 2), redrawn
    if scene == "beyond" and R >= 63:
        assert (np.abs(g.pos).max(-1) > 1).any() and not g.fast_exact.all()
    ray_of = np.repeat(np.arange(R), S)

    def samples(fl):
        if fl.name not in cache:
            cache[fl.name] = F.field_samples(field, g.p32, g.sel, rays.directions, ray_of, fl, e_p=g.e_p)
            assert np.abs(cache[fl.name].raw).max() < F.FEXP_MAX_ARG
        return cache[fl.name]
    return field, call, g, samples


def record(name, worst):
    _RECORD.append((name, worst))


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("R,S", [(1, 1), (63, 2), (64, 12), (65, 25), (129, 48), (65, 64)])
def test_every_form_inside_the_counted_bounds(scene, R, S):
    field, call, g, samples = bounded_call(scene, R, S, 1000 * S + R)
    dfield = DevField(field)
    for name, (fl, kind, dense, over) in FORMS.items():
        f = dfield.struct(kind, dense)
        k = call.used_split(f, over)
        ref = F.render(samples(fl), g, fl, k)
        got = call.field(f, over)
        label = name if not name.startswith("split") else ("split, k used = " + str(k) if k > 1 else "split request capped to the whole march")
        record(f"{label} | {scene}", F.judge(f"{name} | {scene} R={R} S={S} (split {k})", ref, got))
        if name == "mfma":
            w = call.field(f, over, want_weights=True)
            same_outputs("asking for the weights changes no other output", w, got)
            record(f"{name} {scene}", F.judge(f"{name} | {scene} R={R} S={S} weights", ref, w, ["weights"]))
        if name == "valu":
            w = call.field(f, over, want_weights=True)
            same_outputs("asking for the weights changes no other output", w, got)
            record(f"{name} {scene}", F.judge(f"{name} | {scene} R={R} S={S} weights", ref, w, ["weights"]))


@pytest.mark.parametrize("S", [48, 25])
def test_tail_records_and_replay_inside_the_counted_bounds(S):
    """2 305 rays on 16 wave slots: two rounds, four whole tiles and one ragged tile replayed; the proposal pass in its lane = ray
    form.  The replay must also give the whole march's bits."""
    field, call, g, samples = bounded_call("inside", TAIL_RAYS, S, 77 + S, prop_family=1, criterion=(F.RAYS, (1,)))
    dfield = DevField(field)
    ref = F.render(samples(F.RAYS), g, F.RAYS)
    off = call.field(dfield.struct("f32", True), TAIL_FORMS["tail off"][3])
    record("tail inside", F.judge(f"tail off S={S}", ref, off))
    for name, (fl, kind, dense, over) in TAIL_FORMS.items():
        f = dfield.struct(kind, dense)
        assert (call.used_tail(f, over) > 1) == (name != "tail off")
        got = call.field(f, over)
        record("tail inside", F.judge(f"{name} S={S}", ref, got))
        same_outputs(f"{name} against the whole march", got, off)


@pytest.mark.parametrize("chunk_rays,form,scene", [(64, "rays hashed", "inside"), (128, "split 4", "box"), (64, "valu", "beyond"), (128, "bf16x6", "box"),
                                                    (64, "rays dense", "beyond"), (128, "split 3", "beyond")])
def test_chunked_calls_inside_the_counted_bounds(chunk_rays, form, scene):
    R, S, first = 321, 25, 256
    field, call, g, samples = bounded_call(scene, R, S, 5 + chunk_rays)
    fl, kind, dense, over = FORMS[form]
    dfield = DevField(field)   # (owns the device copies the struct points at)
    f = dfield.struct(kind, dense)
    ref = F.render(samples(fl), g, fl, call.used_split(f, over), first, chunk_rays)
    for clip in (1, 0):
        got = call.field(f, over, chunk=(first, chunk_rays), clip=clip)
        if fl is F.VALU or g.e_step is None:
            F.same_bits("depth_bounds", got["bounds"], ref.bounds)
        else:
            assert np.all(np.abs(got["bounds"].astype(f64) - ref.bounds) <= g.e_step.max())
        record(f"chunked {form} {scene}", F.judge(f"{form} | {scene} chunks of {chunk_rays} clip {clip}", ref, got))
        if not clip:
            tol = ref.tol["expected_unclipped"] + F.U * np.abs(ref.expected_unclipped)
            assert np.all(np.abs(got["expected_unclipped"] - ref.expected_unclipped) <= tol)


# ----------------------------------------------------------------------------------------------------------------------
# the plugin surface: tn_density_fwd, tn_field_density_fwd, tn_field_heads_fwd (torch-order arithmetic, expf)
# ----------------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096 * 256   # lanes of the per-sample kernels' grid: one sample more takes a lane's second trip
SURFACE_N = [1, 255, 256, 257, GRID_CAP + 1]
DISTINCT = 257


def within(name, got, want, tol):
    """got [n, ...] against want [m, ...] repeated along the first axis (n > m: the sample set is the m samples over and over)"""
    got = np.asarray(got, f32)
    assert np.all(np.isfinite(got)), name
    m = want.shape[0]
    bound = tol + F.U * np.abs(want)
    worst = 0.0
    for lo in range(0, got.shape[0], m):
        part = got[lo:lo + m].astype(f64)
        err = np.abs(part - want[:len(part)])
        assert np.all(err <= bound[:len(part)]), (name, lo, float((err / np.maximum(bound[:len(part)], 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound[:len(part)], 1e-300)).max()))
    print(f"{name}: worst |device - fp64| / bound = {worst:.4f}")
    record(name.split(" n=")[0], {"value": worst})


def surface_positions(n, seed, contraction):
    r = np.random.default_rng(seed)
    pos = r.uniform(-1.6, 1.6, (min(n, DISTINCT), 3)).astype(f32)
    pos[0] = 0   # the origin; with the contraction on, a face of the unit cube and a point beyond it
    if len(pos) > 2:
        pos[1], pos[2] = (1.0, 0.25, -0.5), (-3.0, 0.5, 1.0)
    return pos, dev(np.resize(pos, (n, 3)))


@pytest.mark.parametrize("hidden", [16, 64])
@pytest.mark.parametrize("contraction", [True, False])
def test_density_fwd_per_sample(hidden, contraction):
    r = np.random.default_rng(hidden)
    grid = F.GridRef((r.uniform(-1, 1, (5 << 10, 2)) * 0.6).astype(f32), np.array([16, 26, 45, 76, 127], f32), 10)
    w0, b0 = (r.standard_normal((hidden, 10)) * 0.5).astype(f32), (r.standard_normal(hidden) * 0.2).astype(f32)
    w1, b1 = (r.standard_normal((1, hidden)) * (2.0 / hidden)).astype(f32), np.array([0.25], f32)
    keep = [dev(grid.table)]
    d = _hip.tn_density_field()
    d.grid.table, d.grid.num_levels, d.grid.log2_hashmap_size = keep[0].data_ptr(), 5, 10
    for l in range(5):
        d.grid.scalings[l] = float(grid.scalings[l])
    d.l0, d.l1 = linear(keep, w0, b0), linear(keep, w1, b1)
    box = np.array([[-1, -1.5, -1], [1, 1, 1.25]], f32)
    d.space, d.average_init_density = space(contraction, box), 1.5
    for n in SURFACE_N:
        pos, pos_dev = surface_positions(n, n % 1000, contraction)
        p32, sel = F.PG.normalized(pos, F.PG.Space(contraction, box))
        want, tol = F.proposal_density(grid, w0, b0, w1, b1, 1.5, p32, sel)
        out = Out(n)
        _hip.check(_hip.load().tn_density_fwd(C.byref(d), pos_dev.data_ptr(), n, out.ptr, _hip.current_stream()), "tn_density_fwd")
        within(f"tn_density_fwd hidden {hidden} contraction {contraction} n={n}", out.read("density"), want, tol)


@pytest.mark.parametrize("contraction", [True, False])
def test_field_density_and_heads_per_sample(contraction):
    field = F.random_field(300 + contraction, contraction=contraction, aabb=[[-1, -1.5, -1], [1, 1, 1.25]], sh_shifted=contraction,
                           use_avg=contraction, avg=0.75)
    dfield = DevField(field)   # (owns the device copies the struct points at)
    f = dfield.struct()
    lib = _hip.load()
    for n in SURFACE_N:
        pos, pos_dev = surface_positions(n, n % 1000 + 1, contraction)
        m = len(pos)
        p32, sel = F.PG.normalized(pos, F.PG.Space(contraction, field.aabb))
        r = np.random.default_rng(n % 1000)
        dirs = r.standard_normal((m, 3))
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
        s = F.field_samples(field, p32, sel, dirs, np.arange(m), F.VALU)
        density, geo = Out(n), Out(n, F.GF)
        _hip.check(lib.tn_field_density_fwd(C.byref(f), pos_dev.data_ptr(), n, density.ptr, geo.ptr, _hip.current_stream()), "tn_field_density_fwd")
        within(f"tn_field_density_fwd density n={n}", density.read("density"), s.density, s.e_density)
        geo_dev = geo.read("geo")
        within(f"tn_field_density_fwd geo n={n}", geo_dev, s.geo, s.e_geo)
        # the heads on the DEVICE's geo rows (an exact fp32 input of theirs), eval and training appearance
        cams = r.integers(0, field.emb.shape[0], m).astype(np.int32)
        sh = F.sh16(dirs, field.sh_shifted)
        for training in (0, 1):
            app = field.emb[cams].astype(f64) if training else np.broadcast_to(F.appearance_fp32(field).astype(f64), (m, F.APP))
            h = F.field_heads(field, geo_dev[:m].astype(f64), np.zeros((m, F.GF)), sh, app, F.VALU)
            rgb, th = Out(n, 3), Out(n)
            dirs_dev, cam_dev = dev(np.resize(dirs, (n, 3))), dev(np.resize(cams, n), np.int32)
            _hip.check(lib.tn_field_heads_fwd(C.byref(f), dirs_dev.data_ptr(), geo.ptr, cam_dev.data_ptr(), n, training, rgb.ptr, th.ptr,
                                              _hip.current_stream()), "tn_field_heads_fwd")
            within(f"tn_field_heads_fwd training {training} rgb n={n}", rgb.read("rgb"), h.rgb, h.e_rgb)
            within(f"tn_field_heads_fwd training {training} thermal n={n}", th.read("thermal"), h.thermal, h.e_thermal)


def test_zz_print_the_worst_ratios():
    """(last in the module) one line per form and scene: the worst ratio to the bound of every output over the tests above"""
    table = {}
    for name, worst in _RECORD:
        row = table.setdefault(name, {})
        for k, v in worst.items():
            row[k] = max(row.get(k, 0.0), v)
    for name in sorted(table):
        print(f"{name:28s} " + "  ".join(f"{k} {v:.4f}" for k, v in table[name].items()))
    assert all(v <= 1.0 for row in table.values() for v in row.values())
