"""The last partial round of a whole-march field call as (tile, segment) records plus a replay pass (field_records_kernel,
field_replay_kernel, tn_render_tail_plan) must give the whole march's BITS: every comparison here is torch.equal on all outputs of
RayRenderEngine.render, tail_balance forced (or "auto") against "off".

The slot override (tn_render_config.tail_slots = 16: a grid of two blocks) makes a few thousand rays whole rounds plus a
remainder.  The models force the lane = ray form and sample_split = 1, the form the plan applies to."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOTS = 16
TWO_ROUNDS_FIVE = SLOTS * 64 * 2 + 5 * 64
RAY_COUNTS = [TWO_ROUNDS_FIVE,      # two full rounds and five remainder tiles
              TWO_ROUNDS_FIVE + 37,  # ... and a partial last tile
              SLOTS * 64 + 64,      # one remainder tile
              15 * 64,              # no full round: the plan declines
              SLOTS * 64 * 3]       # no remainder: the plan declines
MIN_SEGMENT = 12


@pytest.fixture(scope="module")
def rays():
    from thermo_nerf_amd import synthetic

    o, d, _ = synthetic.orbit_camera_rays(64, 64, view=0)
    return o.reshape(-1, 3).contiguous().to(DEV), d.reshape(-1, 3).contiguous().to(DEV)


@pytest.fixture(scope="module")
def models():
    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic

    cache = {}

    def get(S, kind="scene"):
        if (S, kind) not in cache:
            cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=S, kernel_family="lane_ray", sample_split=1)
            model = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=8)
            synthetic.fill_model_(model, kind)
            cache[S, kind] = model.to(DEV).eval()
        return cache[S, kind]
    return get


def _engine(model, chunk=4096, slots=SLOTS):
    from thermo_nerf_amd.engine import RayRenderEngine

    eng = RayRenderEngine(model, chunk=chunk)
    eng.rc.tail_slots = slots
    return eng


def _want_plan(n, S, k, slots=SLOTS):
    """the issue's rules, written out: whole rounds and a remainder, k capped at 16 and at segments of >= 12 samples, none empty"""
    tiles = -(-n // 64)
    full = tiles // slots * slots
    if full == 0 or tiles == full:
        return 1
    k = min(k, 16, S // MIN_SEGMENT)
    if k < 2:
        return 1
    seg = -(-S // k)
    return -(-S // seg)


def _clone(out):
    return {k: v.clone() for k, v in out.items()}


def _assert_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("S", [1, 2, 13, 48])
def test_forced_segments_equal_the_whole_march(rays, models, S):
    eng = _engine(models(S))
    planned = set()
    for n in RAY_COUNTS:
        o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
        off = _clone(eng.render(o, d, tail_balance="off"))
        assert eng.tail_plan(n, tail_balance="off") == 1
        for k in (2, 3, 7, 16):
            plan = eng.tail_plan(n, tail_balance=k)
            assert plan == _want_plan(n, S, k), (n, S, k, plan)
            planned.add(plan)
            _assert_equal(eng.render(o, d, tail_balance=k), off, (n, S, k))
    torch.cuda.synchronize()
    # k > S and segments below the minimum degrade to fewer segments (S = 48: 7 and 16 -> 4), down to the whole march
    assert planned == ({1, 2, 3, 4} if S == 48 else {1})


def test_the_records_are_written_and_replayed(rays, models):
    """the comparison above would also hold if the plan silently never ran: the record region of the workspace, poisoned, is
    rewritten by a planned call (finite optical depths and colours for the scene weights) and left alone by an "off" call"""
    S, k, n = 48, 3, TWO_ROUNDS_FIVE + 37
    eng = _engine(models(S))
    o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
    off = _clone(eng.render(o, d, tail_balance="off"))
    _assert_equal(eng.render(o, d, tail_balance=k), off, "first planned call")  # (sizes the workspace for the records)
    eng.rc.kernel_family, eng.rc.sample_split, eng.rc.tail_balance = 1, 1, k
    whole, rec = eng.lib.tn_render_workspace_bytes(eng.rc, n), eng.lib.tn_render_tail_records_bytes(eng.rc, n)
    eng.rc.kernel_family, eng.rc.sample_split, eng.rc.tail_balance = 0, 0, 0
    assert rec == 6 * S * 5 * 64 * 4 and whole - rec > 0 and (whole - rec) % 256 == 0 and eng._ws.shape[1] >= whole
    region = eng._ws[0, whole - rec:whole].view(torch.float32)
    region.fill_(float("nan"))
    _assert_equal(eng.render(o, d, tail_balance="off"), off, "off")
    assert torch.isnan(region).all()
    _assert_equal(eng.render(o, d, tail_balance=k), off, "planned")
    assert torch.isfinite(region).all()


@pytest.mark.parametrize("dense", [True, False])
def test_records_on_dense_and_on_hashed_field_grids(rays, models, dense):
    """field_records_kernel<true> / <false>: 19 tiles on 8 slots (one block) are two full rounds plus three tiles; with the field's
    dense re-layout and without it, the planned call gives the whole march's bits and rewrites the poisoned record region, which
    the "off" call leaves alone (as in test_the_records_are_written_and_replayed)"""
    model = models(48)
    n = 8 * 64 * 2 + 3 * 64
    o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
    budget = model.field.dense_budget_bytes
    try:
        if not dense:
            model.field.dense_budget_bytes = 0
            model.invalidate_prepared()
        assert (model.field.c_struct(prepare=True).grid.num_dense_levels >= 6) == dense
        eng = _engine(model, slots=8)
        assert eng.tail_plan(n, tail_balance=3) == 3
        off = _clone(eng.render(o, d, tail_balance="off"))
        _assert_equal(eng.render(o, d, tail_balance=3), off, ("first planned call", dense))  # (sizes the workspace for the records)
        eng.rc.kernel_family, eng.rc.sample_split, eng.rc.tail_balance = 1, 1, 3
        whole, rec = eng.lib.tn_render_workspace_bytes(eng.rc, n), eng.lib.tn_render_tail_records_bytes(eng.rc, n)
        eng.rc.kernel_family, eng.rc.sample_split, eng.rc.tail_balance = 0, 0, 0
        assert rec == 3 * 48 * 5 * 64 * 4 and eng._ws.shape[1] >= whole
        region = eng._ws[0, whole - rec:whole].view(torch.float32)
        region.fill_(float("nan"))
        _assert_equal(eng.render(o, d, tail_balance="off"), off, ("off", dense))
        assert torch.isnan(region).all()
        _assert_equal(eng.render(o, d, tail_balance=3), off, ("planned", dense))
        assert torch.isfinite(region).all()
    finally:
        model.field.dense_budget_bytes = budget
        model.invalidate_prepared()


def test_stress_weights_reach_nan_to_num(rays, models):
    S, n = 48, TWO_ROUNDS_FIVE + 37
    eng = _engine(models(S, "stress"))
    o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
    off = _clone(eng.render(o, d, tail_balance="off"))
    assert eng.tail_plan(n, tail_balance=3) == 3
    got = eng.render(o, d, tail_balance=3)
    _assert_equal(got, off, "stress")
    for k, v in got.items():
        assert torch.isfinite(v).all(), k


def test_a_remainder_tile_in_the_last_chunk_keeps_the_chunk_bounds(rays, models):
    """chunk 1 024: the five remainder tiles lie in the third chunk, whose depth bounds then come from both the whole march's and
    the replay's flushes; the per-chunk bounds, and expected_depth clipped with them, equal the unsplit call's"""
    S, n = 48, TWO_ROUNDS_FIVE
    eng = _engine(models(S), chunk=1024)
    o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
    assert eng.tail_plan(n, tail_balance=3) == 3
    off = _clone(eng.render(o, d, tail_balance="off"))
    _assert_equal(eng.render(o, d, tail_balance=3), off, "chunked render")
    res = {}
    for tb in ("off", 3):
        out, bounds = eng.render_shard(o, d, 0, n, tail_balance=tb)
        unclipped = out["expected_depth"].clone()
        eng.apply_depth_bounds(out, 0, bounds)
        res[tb] = (_clone(out), bounds.clone(), unclipped)
    torch.cuda.synchronize()
    assert res["off"][1].shape == (3, 2) and torch.isfinite(res["off"][1]).all()
    assert torch.equal(res["off"][1], res[3][1])
    assert torch.equal(res["off"][2], res[3][2])
    _assert_equal(res["off"][0], res[3][0], "shard")
    assert torch.equal(res[3][0]["expected_depth"], off["expected_depth"])


def test_requested_weights_are_equal(rays, models):
    """a call that asks for the final level's weights (the model's forward with samples) gives the same weights under any setting"""
    from thermo_nerf_amd import RayBundle

    model = models(48)
    n = TWO_ROUNDS_FIVE
    bundle = model.collider(RayBundle(origins=rays[0][:n].contiguous(), directions=rays[1][:n].contiguous()))
    got = {}
    try:
        for tb in ("off", 7, "auto"):
            model.config.tail_balance = tb
            with torch.no_grad():
                out = model._get_outputs_fused(bundle, want_samples=True)
            got[tb] = (out["weights_list"][2].clone(), out["rgb"].clone(), out["thermal"].clone())
    finally:
        model.config.tail_balance = "auto"
    for tb in (7, "auto"):
        for a, b in zip(got["off"], got[tb]):
            assert torch.equal(a, b), tb


def test_auto_follows_the_library_plan(rays, models):
    S = 48
    model = models(S)
    # a 65 536-ray call on the real 2 048 slots: 1 024 tiles, no whole round — such calls stay with the split form
    n = 65536
    o, d = rays[0].repeat(16, 1).contiguous(), rays[1].repeat(16, 1).contiguous()
    eng = _engine(model, chunk=n, slots=0)
    assert eng.tail_plan(n) == eng.lib.tn_render_tail_segments(n // 64, 2048, S, 0) == 1
    off = _clone(eng.render(o, d, tail_balance="off"))
    _assert_equal(eng.render(o, d), off, "auto, 65 536 rays")
    # 37 tiles on 16 slots: five remainder tiles, 3 segments are 15 units = one round of a third
    n = TWO_ROUNDS_FIVE
    eng = _engine(model)
    assert eng.tail_plan(n) == eng.lib.tn_render_tail_segments(37, SLOTS, S, 0) == 3
    o, d = rays[0][:n].contiguous(), rays[1][:n].contiguous()
    off = _clone(eng.render(o, d, tail_balance="off"))
    _assert_equal(eng.render(o, d), off, "auto, 16 slots")
    _assert_equal(eng.render(o, d, tail_balance="auto"), off, "auto by name, 16 slots")
