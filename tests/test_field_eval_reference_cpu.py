"""tests/field_eval_reference.py against itself and against the oracle, no device: the fp64 field and renderers equal
oracle/hotpath.py's in fp64 where nothing is frozen; fp32 emulations of the serial march and of the sample-split association stay
inside the bounds; the exact family is exact in both associations; and every planted fault fails the very check
(``field_eval_reference.judge``) the GPU tests apply."""
import numpy as np
import pytest
import torch

from oracle import hotpath as H
from tests import field_eval_reference as F
from tests import ray_forward_reference as RF

f32, f64 = np.float32, np.float64


def sorted_edges(R, S, seed, per_ray=True):
    """spacing edges as a sampler might leave them: increasing, from 0 to 1, uneven"""
    r = np.random.default_rng(seed)
    e = np.sort(r.uniform(0, 1, (R if per_ray else 1, S + 1)).astype(f32), axis=1)
    e[:, 0], e[:, -1] = 0, 1
    return np.broadcast_to(e, (R, S + 1)).copy()


def scene(R, S, seed, inside=True, lin=False, **field_kw):
    field = F.random_field(seed, **field_kw)
    rays = F.random_rays(R, seed + 1, inside)
    g = F.geometry(field, *rays, sorted_edges(R, S, seed + 2), lin)
    return field, rays, g


def samples(field, rays, g, fl, fault=None):
    R, S = g.step.shape
    return F.field_samples(field, g.p32, g.sel, rays.directions, np.repeat(np.arange(R), S), fl, fault)


def emulate(s, g, split=1, fault=None, **kw):
    """an fp32 'device': the reference's sample values rounded to fp32, composited in fp32 in the given association"""
    R, S = g.step.shape
    return F.march_fp32(g.delta, s.density.reshape(R, S).astype(f32), s.rgb.reshape(R, S, 3).astype(f32),
                        s.thermal.reshape(R, S).astype(f32), g.step, split, fault, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------------------------------------------------
def state_dict(field):
    t = lambda a: torch.from_numpy(np.asarray(a, f64))
    w = field.w
    sd = {"field.mlp_base.encoder.hash_table": t(field.table), "field.mlp_base.encoder.scalings": t(field.scalings),
          "field.embedding_appearance.embedding.weight": t(field.emb), "field.aabb": t(field.aabb),
          "field.field_head_thermal.net.weight": t(w["thead_w"]), "field.field_head_thermal.net.bias": t(w["thead_b"])}
    for name, keys in (("field.mlp_base.mlp", ("base0", "base1")), ("field.mlp_head", ("head0", "head1", "head2")),
                       ("field.mlp_thermal", ("th0", "th1"))):
        for i, k in enumerate(keys):
            sd[f"{name}.layers.{i}.weight"], sd[f"{name}.layers.{i}.bias"] = t(w[k + "_w"]), t(w[k + "_b"])
    return sd


@pytest.mark.parametrize("sh_shifted,use_avg", [(True, True), (False, False)])
def test_field_and_renderers_equal_the_oracle_in_fp64(sh_shifted, use_avg):
    """dyadic positions in the unit box (p s is exact: the frozen cell is the oracle's cell), dyadic embedding rows over 8 images
    (the fp32 mean is exact), SH in fp64: nothing is frozen, and the two agree to 1e-12"""
    R, S = 7, 9
    r = np.random.default_rng(3)
    field = F.random_field(5, contraction=False, aabb=[[0, 0, 0], [1, 1, 1]], sh_shifted=sh_shifted, use_avg=use_avg, num_images=8)
    field = field._replace(emb=(r.integers(-8, 9, (8, F.APP)) / 4.0).astype(f32))
    pos = (r.integers(0, 65, (R * S, 3)) / 64.0).astype(f32)          # 0 and 1 occur: the selector is exercised
    d = r.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    sel = np.all((pos > 0) & (pos < 1), axis=1)
    assert 0 < sel.sum() < len(sel)
    p32 = (pos * sel[:, None]).astype(f32)
    s = F.field_samples(field, p32, sel, d, np.repeat(np.arange(R), S), F.VALU, sh_fp64=True)
    cfg = H.OracleConfig(log2_hashmap_size=field.log2T, disable_scene_contraction=True, sh_input="shifted" if sh_shifted else "unit",
                         use_average_appearance_embedding=use_avg, average_init_density=field.avg)
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        sd = state_dict(field)
        density, geo = H.field_density(sd, torch.from_numpy(pos.astype(f64)).view(R, S, 3), cfg)
        dirs = torch.from_numpy(d.astype(f64))[:, None, :].expand(R, S, 3)
        rgb, th = H.field_outputs(sd, dirs, geo, None, cfg, False)
        assert np.abs(density.numpy().reshape(-1) - s.density).max() < 1e-12
        assert np.abs(rgb.numpy().reshape(-1, 3) - s.rgb).max() < 1e-12
        assert np.abs(th.numpy().reshape(-1) - s.thermal).max() < 1e-12
        # renderers: dyadic edges, so that the fp32 mid-points and deltas are the oracle's fp64 ones
        edges = np.cumsum(r.integers(1, 5, (R, S + 1)), axis=1).astype(f32) / 64
        st, en = edges[:, :-1], edges[:, 1:]
        g = F.Geo(st, en, RF.midpoints_fp32(st, en), (en - st).astype(f32), None, None, None, np.ones(R, bool))
        ref = F.render(s, g, F.VALU)
        T = lambda a: torch.from_numpy(np.asarray(a, f64))[..., None]
        w = H.get_weights(T(g.delta), density)
        assert np.abs(w.numpy()[..., 0] - ref.weights).max() < 1e-12
        assert np.abs(H.render_rgb(rgb, w, False).numpy() - ref.rgb).max() < 1e-12
        assert np.abs(H.render_thermal(th, w, False).numpy()[:, 0] - ref.thermal).max() < 1e-12
        assert np.abs(H.render_accumulation(w).numpy()[:, 0] - ref.accumulation).max() < 1e-12
        assert np.array_equal(H.render_depth_median(w, T(st), T(en)).numpy()[:, 0], ref.depth)
        assert np.abs(H.render_depth_expected(w, T(st), T(en)).numpy()[:, 0] - ref.expected_depth).max() < 1e-9   # (1e-10 as fp32)
    finally:
        torch.set_default_dtype(before)


def test_contraction_geometry_is_the_oracles_fp32():
    """samples at |x|_inf = 1, beyond it and at the origin: p and the selector are the fp32 oracle's"""
    field = F.random_field(2)
    o = np.array([[-1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.25, 0.0]], f32)
    d = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], f32)
    edges = np.broadcast_to(np.array([0.0, 0.0, 0.5, 1.0], f32), (3, 4)).copy()   # mid-points 0, 1 / 4, 3 / 4 of far = 4
    g = F.geometry(field, o, d, np.zeros(3, f32), np.full(3, 4.0, f32), edges, True)
    assert np.array_equal(g.pos[1, 0], [0, 0, 0]) and np.array_equal(g.pos[0, 1], [0, 0, 0]) and g.pos[0, 2, 0] == 2.0
    assert np.abs(g.pos).max(-1).tolist()[1] == [0.0, 1.0, 3.0]
    assert not g.fast_exact.any() and g.sel.all()
    assert np.array_equal(g.p32.reshape(3, 3, 3)[1, 2], np.array([2.0, (2 - f32(1) / f32(3)) + 2, 2.0], f32) / 4)


def test_fast_geometry_bound_covers_a_reciprocal_form_of_the_contraction():
    """x (1 / m) for x / m and 2 - (1 / m), every operation rounded to fp32 — the FAST kernels' statements with a correctly rounded
    reciprocal standing in for v_rcp_f32 — stays within Geo.e_p of the frozen p; rays inside the unit cube carry no such bound"""
    field, rays, g = scene(40, 12, 81, inside=True)
    assert F.geometry(field, *rays, sorted_edges(40, 12, 83), False, fast=True).e_p is None and g.e_p is None
    rays = F.random_rays(40, 82, False)
    g = F.geometry(field, *rays, sorted_edges(40, 12, 83), True, fast=True)   # uniform sampler: the positions themselves are exact
    assert g.e_p is not None and not g.fast_exact.all() and np.all(g.e_step <= F.U * np.abs(g.step)) and np.all(g.e_p >= 0)
    x = g.pos.reshape(-1, 3)
    m = np.abs(x).max(1, keepdims=True)
    rinv = (f32(1) / m).astype(f32)
    c = np.where(m < 1, x, ((f32(2) - rinv).astype(f32) * (x * rinv).astype(f32)).astype(f32))
    p = ((c + f32(2)).astype(f32) / f32(4)).astype(f32)
    moved = np.abs(p.astype(f64) - g.p32)
    assert (moved > 0).any() and np.all(moved <= g.e_p) and np.all(g.e_p[(m < 1)[:, 0]] == 0)
    # and what it does to the features: one level's slope bound holds for a position moved across a cell face
    grid = F.GridRef(field.table, field.scalings, field.log2T)
    a = np.full((1, 3), 0.5, f32)
    b = np.nextafter(a, f32(0))
    ea, _ = F.encode(grid, a)
    eb, err = F.encode(grid, b, e_p=np.abs(a.astype(f64) - b))
    assert np.all(np.abs(ea - eb) <= err)


def test_overflow_family_puts_a_nan_on_the_path():
    """the NaN family in both associations of the fp32 emulation: a ray that starts outside the box has every weight zeroed, the box
    it enters later included; a ray that starts inside keeps weight 1 on sample 0"""
    S, ks = 25, (3,)
    field = F.exact_field(19, raw=F.OVERFLOW_RAW)
    targets = np.array(F.seam_targets(S, ks) * 3)
    R = len(targets)
    edges = np.broadcast_to(np.linspace(0, 1, S + 1, dtype=f32), (R, S + 1)).copy()
    c = F.first_hit_rays(field, edges, np.full(R, 0.05, f32), np.full(R, 0.9, f32), False, targets, 5, overflow=True)
    assert set(c.index.tolist()) == {0, -1} and (targets > 0).any()
    with np.errstate(over="ignore", invalid="ignore"):
        dens = np.where(c.geo.sel.reshape(R, S), f32(np.inf), f32(np.inf) * f32(0)).astype(f32)
    assert np.isnan(dens).any() and np.isinf(dens).any()
    half, b = np.full((R, S, 3), 0.5, f32), np.full((R, S), F.EXACT_THERMAL, f32)
    for split in (1, 3):
        got = F.march_fp32(c.geo.delta, dens, half, b, c.geo.step, split)
        for k in F.OUTPUTS:
            F.same_bits(f"{k} split {split}", got[k], c.want[k])
        F.same_bits("weights", got["weights"], c.weights)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 emulations inside the bounds
# ----------------------------------------------------------------------------------------------------------------------
CASES = [(5, 1, 1), (5, 2, 1), (33, 12, 1), (33, 25, 1), (33, 25, 3), (33, 25, 4), (20, 48, 2), (20, 48, 4), (20, 64, 1), (20, 64, 8)]


@pytest.mark.parametrize("R,S,split", CASES)
def test_fp32_associations_stay_inside_the_bounds(R, S, split):
    for seed, inside, lin in ((11, True, False), (12, False, True), (13, False, False)):
        field, rays, g = scene(R, S, seed, inside, lin, contraction=seed != 12, aabb=[[-2, -2, -2], [2, 2, 2]])
        s = samples(field, rays, g, F.VALU)
        assert np.abs(s.raw).max() < F.FEXP_MAX_ARG
        ref = F.render(s, g, F.VALU, split)
        got = emulate(s, g, split)
        ok = ref.med_ok
        F.judge(f"fp32 {R}x{S} split {split}", ref, got, [k for k in F.OUTPUTS if k != "depth"] + ["weights"])
        F.same_bits("median", got["depth"][ok], ref.depth[ok])
        assert ok.mean() > 0.9


def test_the_median_condition_marks_a_tie():
    """one opaque sample whose weight is 1/2 to the last bit sits ON the split: the ray is marked, its neighbours are not"""
    field, rays, g = scene(3, 8, 21)
    s = samples(field, rays, g, F.VALU)
    dens = s.density.reshape(3, 8).copy()
    dens[1] = 0
    dens[1, 3] = np.log(2.0) / f64(g.delta[1, 3])
    ref = F.render(s._replace(density=dens.reshape(-1)), g, F.VALU)
    assert ref.med_ok.tolist() == [True, False, True]


# ----------------------------------------------------------------------------------------------------------------------
# the exact family
# ----------------------------------------------------------------------------------------------------------------------
def exact_case(S, ks, seed, chunk_rays=0, first_ray=0, lin=False, reps=3):
    field = F.exact_field(seed)
    targets = np.array(F.seam_targets(S, ks) * reps)
    R = len(targets)
    ray = first_ray + np.arange(R)
    if chunk_rays:   # a chunk's last ray misses: its expected depth is the chunk's own minimum, which differs from the next chunk's
        targets[ray % chunk_rays == chunk_rays - 1] = -1
    nears = (0.05 + 0.004 * ((ray // max(chunk_rays, 64)) % 5) + 0.0003 * (ray % 4)).astype(f32)
    fars = np.full(R, 0.9 if S > 2 else 0.3, f32)
    edges = np.broadcast_to(np.linspace(0, 1, S + 1, dtype=f32), (R, S + 1)).copy()
    return field, F.first_hit_rays(field, edges, nears, fars, lin, targets, seed, first_ray, chunk_rays)


@pytest.mark.parametrize("S,ks", [(1, ()), (2, ()), (12, ()), (25, (2, 3, 4)), (48, (2, 3, 4)), (64, (8,))])
def test_exact_family_is_exact_in_both_associations(S, ks):
    for lin in (False, True):
        field, c = exact_case(S, ks, 30 + S, lin=lin)
        R = len(c.index)
        assert set(c.index.tolist()) == set(F.seam_targets(S, ks))
        s = F.field_samples(field, c.geo.p32, c.geo.sel, c.rays.directions, np.repeat(np.arange(R), S), F.RAYS)
        assert np.all(s.rgb == 0.5) and np.all(s.thermal == F.EXACT_THERMAL) and np.all(s.raw == F.EXACT_RAW)
        for split in (1,) + tuple(ks):
            ref = F.render(s, c.geo, F.RAYS, split)
            got = emulate(s, c.geo, split)
            for k in F.OUTPUTS:
                F.same_bits(f"reference {k}", c.want[k], getattr(ref, k))
                F.same_bits(f"emulation {k} split {split}", got[k], c.want[k])
            F.same_bits("weights", got["weights"], c.weights)


def test_exact_family_chunk_bounds_differ_between_chunks():
    field, c = exact_case(25, (3,), 40, chunk_rays=64, first_ray=128, reps=20)
    assert c.bounds.shape[0] >= 3 and len(set(c.bounds[:, 0].tolist())) > 1
    miss = c.index < 0
    assert miss.any() and len(set(c.want["expected_depth"][miss].tolist())) > 1


def test_tie_density_meets_its_own_premise():
    r = np.random.default_rng(4)
    found = 0
    for delta in r.uniform(0.001, 0.1, 200).astype(f32):
        a = F.tie_density(delta)
        if a is not None:
            found += 1
            assert f32(f32(delta * f32(a)) * F.LOG2E32) == f32(1) and f32(a) == a
    assert found > 150


# ----------------------------------------------------------------------------------------------------------------------
# planted faults
# ----------------------------------------------------------------------------------------------------------------------
def test_renderer_faults_fail_the_exact_family():
    S, k = 25, 3
    field, c = exact_case(S, (k,), 50, chunk_rays=64, first_ray=64, reps=20)
    R = len(c.index)
    s = F.field_samples(field, c.geo.p32, c.geo.sel, c.rays.directions, np.repeat(np.arange(R), S), F.RAYS)
    ref = F.render(s, c.geo, F.RAYS, k, 64, 64)
    kw = dict(first_ray=64, chunk_rays=64)
    F.judge("sound", ref, emulate(s, c.geo, k, **kw), exact=True)
    for fault, output in (("seam_sample_dropped", "accumulation"), ("median_off_by_one", "depth"), ("minmax_live", "expected_depth"),
                          ("chunk_slot", "expected_depth")):
        got = emulate(s, c.geo, k, fault, **kw)
        assert F.fails(F.judge, fault, ref, got, [output], exact=True), fault
    assert F.fails(F.same_bits, "bounds", emulate(s, c.geo, k, "chunk_slot", **kw)["bounds"], ref.bounds)
    assert F.fails(F.same_bits, "bounds", emulate(s, c.geo, k, "minmax_live", **kw)["bounds"], ref.bounds)


def test_renderer_faults_fail_the_bounded_family():
    R, S, k = 40, 25, 3
    field, rays, g = scene(R, S, 61)
    s = samples(field, rays, g, F.RAYS)
    ref = F.render(s, g, F.RAYS, k)
    F.judge("sound", ref, emulate(s, g, k), [o for o in F.OUTPUTS if o != "depth"])
    for fault, output in (("seam_sample_dropped", "accumulation"), ("T_not_applied_to_thermal", "thermal"),
                          ("no_thermal_background", "thermal")):
        assert F.fails(F.judge, fault, ref, emulate(s, g, k, fault), [output]), fault
    ok = ref.med_ok
    assert F.fails(F.same_bits, "median", emulate(s, g, k, "median_off_by_one")["depth"][ok], ref.depth[ok])


@pytest.mark.parametrize("fault", F.FIELD_FAULTS)
def test_field_faults_fail_the_bounded_family(fault):
    R, S = 40, 12
    field, rays, g = scene(R, S, 71, inside=fault != "no_selector", contraction=fault != "no_selector", aabb=[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]])
    ref = F.render(samples(field, rays, g, F.RAYS), g, F.RAYS)
    F.judge("sound", ref, emulate(samples(field, rays, g, F.RAYS), g), ["rgb", "thermal", "accumulation"])
    got = emulate(samples(field, rays, g, F.RAYS, fault), g)
    output = {"sh_shifted_ignored": "rgb", "appearance_zeros": "rgb", "level_offset": "accumulation", "no_selector": "accumulation"}[fault]
    assert F.fails(F.judge, fault, ref, got, [output]), fault
    if fault in ("sh_shifted_ignored", "appearance_zeros"):   # the colour head alone: the other outputs must not move
        F.judge(fault, ref, got, ["thermal", "accumulation"])
