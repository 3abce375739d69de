"""The dense re-layout stores x-differences: dense[x][y][z] = (e(x,y,z), e(x+1,y,z) - e(x,y,z)), e(.) = table[hash(.)].

1. The buffer tn_hashgrid_prepare writes, against a torch restatement of that layout, as int32 bits.
2. Renders and plugin-surface calls with the dense copies against the same calls on the hashed tables (budget 0), as int32 bits, on
   rays that sit on grid planes (interpolation offset exactly 0) and rays that run to the far corner of the contracted scene box
   (the largest grid indices), with subnormal, duplicated and large table entries planted in every level.
"""
import copy

import pytest
import torch

from tests import helpers
from thermo_nerf_amd import RayBundle, _hip
from thermo_nerf_amd.fields import HashEncoding

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P1, P2, M32 = 2654435761, 805459861, 0xFFFFFFFF


def plant(table: torch.Tensor, big: float, seed: int) -> torch.Tensor:
    """Entries whose x-difference overflows (+-big pairs; big = 3e38 in the layout test), is subnormal or is exactly 0 (runs of
    duplicates), spread over the whole table between ordinary values."""
    g = torch.Generator().manual_seed(seed)
    n = table.shape[0]
    t = table.clone()
    kind = torch.randint(0, 8, (n,), generator=g)
    sign = (torch.randint(0, 2, (n, 2), generator=g) * 2 - 1).float()
    t[kind == 0] = (sign * big)[kind == 0]
    t[kind == 1] = (sign * 1e-40)[kind == 1]
    t[kind == 2] = torch.tensor([0.5, -0.25])
    t[kind == 3] = 2e-40
    return t


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().cpu().view(torch.int32)


# ---- 1. the layout ----------------------------------------------------------------------------------------------------------
def test_dense_buffer_holds_entries_and_x_differences():
    enc = HashEncoding(num_levels=3, min_res=4, max_res=8, log2_hashmap_size=8)
    T = 1 << 8
    table = plant(torch.randn(3 * T, 2, generator=torch.Generator().manual_seed(1)), 3e38, 2)
    with torch.no_grad():
        enc.hash_table.copy_(table)
    enc = enc.to(DEV)
    lib = _hip.load()
    g = enc.c_struct(0)
    nbytes = lib.tn_hashgrid_prepare_bytes(g, 1 << 20)
    out = _hip.tn_hashgrid()
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    _hip.check(lib.tn_hashgrid_prepare(g, out, buf.data_ptr(), nbytes, _hip.current_stream()), "tn_hashgrid_prepare")
    torch.cuda.synchronize()
    assert out.num_dense_levels == 3
    got = buf.cpu().view(torch.int32).view(-1, 4)
    sides = [int(s) + 2 for s in enc.scalings.tolist()]
    assert max(sides) <= 10 and nbytes == 16 * sum(s ** 3 for s in sides)
    collisions, diffs = 0, []
    for l, side in enumerate(sides):
        assert out.dense_res[l] == side
        r = torch.arange(side, dtype=torch.int64)
        x, y, z = torch.meshgrid(r, r, r, indexing="ij")  # [x][y][z], z fastest

        def entry(xx):
            idx = (xx ^ ((y * P1) & M32) ^ ((z * P2) & M32)) & (T - 1)
            return idx, table[l * T + idx]

        idx, e = entry(x)
        _, e1 = entry(x + 1)
        want = torch.cat([e, e1 - e], dim=-1).reshape(-1, 4)  # one fp32 subtraction per component
        collisions += side ** 3 - idx.unique().numel()
        off = out.dense_offset[l]
        have = got[off:off + side ** 3]
        assert torch.equal(have, bits(want)), (l, (have != bits(want)).nonzero()[:4])
        diffs.append(want[:, 2:])
    assert collisions > 0
    d = torch.cat(diffs)  # the planted values did land in differences: overflow, subnormal, exactly zero
    assert torch.isinf(d).any() and (d == 0).any() and ((d != 0) & (d.abs() < 1e-38)).any()


# ---- 2. renders: dense against budget 0 ------------------------------------------------------------------------------------
def special_rays():
    """3 full tiles + 5 rays: camera rays, rays inside grid planes of level 0 (scaling 16: a normalised coordinate k/16 has offset 0
    at every level with an even scaling) and rays towards the far corners of the scene box."""
    o, d = helpers.rays(12, 12, view=3)  # 144 ordinary rays
    plane_o, plane_d = [], []
    for axis in range(3):
        for c in (0.0, 0.25, -0.5, 0.75):  # contracted coordinate c -> normalised (c + 2) / 4 = k / 16
            oo = torch.tensor([-0.7, 0.3, -0.4])
            oo[axis] = c
            dd = torch.zeros(3)  # no component along the axis: every sample of the ray keeps the coordinate c exactly
            dd[(axis + 1) % 3], dd[(axis + 2) % 3] = 0.6, 0.8
            plane_o.append(oo)
            plane_d.append(dd)
    corner_o, corner_d = [], []
    k = 0
    while len(corner_o) + len(plane_o) + o.shape[0] < 3 * 64 + 5:
        sgn = torch.tensor([1.0 if (k >> b) & 1 == 0 else -1.0 for b in range(3)])
        oo = sgn * torch.tensor([0.1, 0.2, 0.05]) * (1 + k // 8)
        dd = sgn * torch.tensor([1.0, 1.0, 1.0]) if k % 3 else sgn * torch.tensor([1.0, 0.999, 0.998])
        corner_o.append(oo)
        corner_d.append(dd / dd.norm())
        k += 1
    o = torch.cat([o, torch.stack(plane_o), torch.stack(corner_o)])
    d = torch.cat([d, torch.stack(plane_d), torch.stack(corner_d)])
    assert o.shape[0] == 3 * 64 + 5
    return o.contiguous(), d.contiguous()


@pytest.fixture(scope="module")
def planted_model():
    model, _, _ = helpers.build("scene", 8)
    gm = copy.deepcopy(model).to(DEV).eval()
    with torch.no_grad():
        for i, enc in enumerate([gm.field.mlp_base.encoder] + [n.mlp_base.encoder for n in gm.proposal_networks]):
            t = enc.hash_table
            t.copy_(plant(t.cpu(), 3.0, 10 + i).to(DEV))  # the layout test's +-3e38 pairs scaled to +-3
    gm.invalidate_prepared()
    return gm


def with_and_without_dense(gm, call):
    mods = [gm.field] + list(gm.proposal_networks)
    budgets = [m.dense_budget_bytes for m in mods]
    assert all(b > 0 for b in budgets)
    with torch.no_grad():
        dense = call()
        assert gm.field.c_struct(prepare=True).grid.num_dense_levels >= 6
        assert gm.proposal_networks[0].c_struct().grid.num_dense_levels == 5
        assert gm.proposal_networks[1].c_struct().grid.num_dense_levels == 4
        for m in mods:
            m.dense_budget_bytes = 0
        gm.invalidate_prepared()
        try:
            assert gm.field.c_struct(prepare=True).grid.num_dense_levels == 0
            hashed = call()
        finally:
            for m, b in zip(mods, budgets):
                m.dense_budget_bytes = b
            gm.invalidate_prepared()
    return dense, hashed


@pytest.mark.parametrize("family,precision", [("lane_ray", "f32"), ("ray_per_wave", "f32"), ("lane_ray", "f16x3"),
                                              ("lane_ray", "bf16x6")])
def test_render_bits_dense_against_hashed(planted_model, family, precision):
    gm = planted_model
    gm.config.kernel_family, gm.config.mlp_precision = family, precision
    o, d = special_rays()
    rb = RayBundle(origins=o.to(DEV), directions=d.to(DEV), camera_indices=torch.zeros((o.shape[0], 1), dtype=torch.long, device=DEV))
    try:
        dense, hashed = with_and_without_dense(gm, lambda: {k: v.clone() for k, v in gm(rb).items()})
    finally:
        gm.config.kernel_family, gm.config.mlp_precision = "lane_ray", "f32"
    for k in ("rgb", "thermal", "accumulation", "depth", "expected_depth", "prop_depth_0", "prop_depth_1"):
        assert torch.equal(bits(dense[k]), bits(hashed[k])), (k, (bits(dense[k]) != bits(hashed[k])).nonzero()[:4])
    assert float(dense["accumulation"].float().nan_to_num().abs().sum()) > 0  # the rays did meet the planted medium


def special_positions():
    """World positions on level-0 grid planes, at and next to the far corners of the contracted box, and ordinary ones."""
    g = torch.Generator().manual_seed(4)
    p = torch.rand(509, 3, generator=g) * 2 - 1
    p[::5, 0] = 0.25
    p[1::5, 1] = -0.5
    p[2::5, 2] = 0.0
    far = torch.tensor([[1e3, 1e3, 1e3], [1e7, 1e7, 1e7], [3e4, 2.9e4, 3e4], [-1e3, 1e3, 1e3], [50.0, 50.0, 49.0], [1.0, 1.0, 1.0],
                        [8.0, 8.0, 8.0], [1e30, 1e30, 1e30]])
    return torch.cat([p, far, -far]).contiguous()


def test_torch_order_calls_bits_dense_against_hashed(planted_model):
    """The plugin-surface kernels (torch op order, a o + b (1 - o)) read the raw entries of all eight corners from the base halves."""
    gm = planted_model
    pos = special_positions().to(DEV)

    def call():
        density, geo = gm.field.density_at(pos)
        return [density.clone(), geo.clone()] + [n.density_fn(pos).clone() for n in gm.proposal_networks]

    dense, hashed = with_and_without_dense(gm, call)
    for i, (a, b) in enumerate(zip(dense, hashed)):
        assert torch.equal(bits(a), bits(b)), (i, (bits(a) != bits(b)).nonzero()[:4])
