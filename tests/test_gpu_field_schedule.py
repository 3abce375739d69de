"""The field kernel's scheduling (wave priorities along the MLP block, the per-workgroup control words in LDS) must not show in
its results: ray counts at the edges of a workgroup's tile distribution (one tile, one lane short of / past a tile, one lane
short of a workgroup's 8 tiles, 8 workgroups plus one tile, a reference chunk, the benchmark's frame) against the ray-per-wave
kernels, which share none of it; a frame rendered twice; a shard's sample-split call against the whole frame.

Tolerance between the two kernel families: what tests/test_gpu_parity.py holds them to (max |difference| 2e-5 on rgb and
thermal: test_small_calls_take_the_ray_per_wave_kernels)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILY_TOL = 2e-5
RAY_COUNTS = [1, 63, 64, 65, 511, 512 * 8 + 64, 65536, 800 * 800]


def _model(S):
    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic

    cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=S)
    model = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=8)
    synthetic.fill_model_(model, "scene")
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def frame():
    from thermo_nerf_amd import synthetic

    o, d, _ = synthetic.orbit_camera_rays(800, 800, view=0)
    return o.reshape(-1, 3).contiguous().to(DEV), d.reshape(-1, 3).contiguous().to(DEV)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(S):
        if S not in cache:
            cache[S] = _model(S)
        return cache[S]
    return get


@pytest.mark.parametrize("S", [1, 2, 48, 192])
@pytest.mark.parametrize("n", RAY_COUNTS)
def test_lane_ray_against_ray_per_wave(frame, models, n, S):
    from thermo_nerf_amd.engine import RayRenderEngine

    model = models(S)
    o, d = frame[0][:n].contiguous(), frame[1][:n].contiguous()
    out = {}
    for family in ("lane_ray", "ray_per_wave"):
        model.config.kernel_family = family
        out[family] = {k: v.clone() for k, v in RayRenderEngine(model, chunk=max(n, 64)).render(o, d).items()}
    torch.cuda.synchronize()
    model.config.kernel_family = "auto"
    for k in ("rgb", "thermal"):
        a, b = out["lane_ray"][k], out["ray_per_wave"][k]
        assert torch.isfinite(a).all(), k
        err = (a - b).abs().max().item()
        print(f"n={n} S={S} {k}: max |lane_ray - ray_per_wave| = {err:.3e}")
        assert err <= FAMILY_TOL, (k, err)


def test_two_renders_of_a_frame_are_bit_identical(frame, models):
    """a hand-over between the waves of a workgroup that races shows as a difference between two runs"""
    from thermo_nerf_amd.engine import RayRenderEngine

    model = models(192)
    model.config.kernel_family = "lane_ray"
    eng = RayRenderEngine(model, chunk=frame[0].shape[0])
    first = {k: v.clone() for k, v in eng.render(*frame).items()}
    second = eng.render(*frame)
    torch.cuda.synchronize()
    model.config.kernel_family = "auto"
    for k in first:
        assert torch.equal(first[k], second[k]), k


def test_sample_split_shard_equals_the_whole_frame(frame, models):
    """main_mfma_rays_kernel<., true>: the 8 shards of the frame, marched in the k segments per tile the engine picks for a
    shard, equal the frame rendered with that k bit for bit (expected depth after the bounds' reduction included)"""
    from thermo_nerf_amd import distributed as D
    from thermo_nerf_amd.engine import RayRenderEngine

    model = models(48)
    model.config.kernel_family = "auto"
    o, d = frame
    n, world = o.shape[0], 8
    eng = RayRenderEngine(model, chunk=1 << 16)
    k = eng.shard_sample_split(D.ray_block(n, 0, world)[1])
    assert k > 1
    want = {key: v.clone() for key, v in eng.render(o, d, sample_split=k).items()}
    shards = []
    for r in range(world):
        a, b = D.ray_block(n, r, world)
        out, bounds = eng.render_shard(o[a:b].contiguous(), d[a:b].contiguous(), a, n, sample_split=k)
        shards.append(({key: v.clone() for key, v in out.items()}, a, bounds.clone()))
    lo = torch.stack([b[:, 0] for _, _, b in shards]).min(dim=0).values
    hi = torch.stack([b[:, 1] for _, _, b in shards]).max(dim=0).values
    bounds = torch.stack([lo, hi], dim=1).contiguous()
    for out, a, _ in shards:
        eng.apply_depth_bounds(out, a, bounds)
    torch.cuda.synchronize()
    for key in D.OUTPUT_KEYS:
        got = torch.cat([out[key] for out, _, _ in shards])
        assert torch.equal(got, want[key]), (key, (got - want[key]).abs().max().item())
