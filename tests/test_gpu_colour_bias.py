"""The lane = ray field kernel folds the colour layer's spherical-harmonics term into a per-ray bias, computed once per 64-ray tile
in the layout of the layer's accumulators (one ray per accumulator column).  These cases would catch a bias that lands on the wrong
ray: tiles whose 64 rays all look in different directions, a ragged last tile, and the sample-split form, each against the oracle."""
import pytest
import torch

from oracle import hotpath as H
from tests import helpers
from tests.test_gpu_parity import bundle, check_outputs, gpu_model

pytestmark = pytest.mark.gpu

RGB_MAX = 1e-5  # the kernel against the oracle, per channel (measured: 1e-7 typical)


def scrambled_rays(n, seed):
    """n camera rays of a 40x40 view in a seeded random order: the 64 rays of a tile come from all over the image."""
    o, d = helpers.rays(40, 40, view=3)
    idx = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(seed))[:n]
    return o[idx].contiguous(), d[idx].contiguous()


def render(gm, o, d, split):
    gm.config.fused, gm.config.use_mfma, gm.config.mlp_precision = True, True, "f32"
    gm.config.sample_split = split
    with torch.no_grad():
        return {k: v.clone() for k, v in gm(bundle(o, d)).items()}


def check(got, want, tag):
    check_outputs(got, want, tag)
    err = (got["rgb"].cpu() - want["rgb"]).abs().max().item()
    assert err <= RGB_MAX, f"{tag}: rgb max |err| {err:.3e}"


@pytest.mark.parametrize("kind", ["stress", "scene"])
@pytest.mark.parametrize("small", [True, False])
def test_tiles_of_64_directions(kind, small):
    gm, sd, ocfg = gpu_model(kind, 48, small=small)
    o, d = scrambled_rays(256, seed=11)
    for t in range(0, 256, 64):  # every tile: 64 distinct directions
        assert torch.unique(d[t:t + 64], dim=0).shape[0] == 64
    want = H.get_outputs(sd, o, d, None, ocfg)
    check(render(gm, o, d, 1), want, f"{kind}/small={small}/64 directions")


@pytest.mark.parametrize("R", [357, 65, 1])
def test_ragged_last_tile(R):
    gm, sd, ocfg = gpu_model("stress", 50)
    o, d = scrambled_rays(R, seed=R)
    want = H.get_outputs(sd, o, d, None, ocfg)
    check(render(gm, o, d, 1), want, f"R={R}")


@pytest.mark.parametrize("split", [2, 3, 0])
def test_sample_split(split):
    """Scrambled rays (test_gpu_parity's sample-split test renders raster order): each segment's wave builds its own bias."""
    gm, sd, ocfg = gpu_model("stress", 192)
    o, d = scrambled_rays(201, seed=5)
    want = H.get_outputs(sd, o, d, None, ocfg)
    got = render(gm, o, d, split)
    check(got, want, f"sample_split={split}")
    serial = render(gm, o, d, 1)
    assert (got["rgb"] - serial["rgb"]).abs().max().item() <= 3e-6
