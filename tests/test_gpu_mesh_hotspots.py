"""tn_mesh_peaks, tn_basin_persistence and tn_mesh_spots on the device against tests/mesh_hotspots_reference.py, exactly — every integer
and every float bit pattern, no tolerance anywhere — into guarded buffers with the workspace guard kept and the inputs unwritten: the
cases worked by hand (two bumps on the 5 x 5 lattice, a constant mesh with shuffled numbering, a ring of NaN between two areas), the
long ascent of a 2 x 600 strip, random meshes around the tile size with ties, NaN and a foreign index, a hub of 10^4 corners, one spot
of 70 000 faces, cold spots against the negated field, the invariance under a vertex permutation, ``extent_drop``, capacities, empty
meshes, and the Python layer with ``regions_mesh``, ``region_map``, ``smooth_iterations`` and the command line."""
from __future__ import annotations

import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_components_reference as C
from tests import mesh_hotspots_reference as H
from tests import mesh_regions_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (SPOT_DTYPE, ThermalHotspots, ThermalMesh, basin_persistence, choose_spots, fit_view, merge_basins,
                                    mesh_incidence, mesh_peaks, mesh_peaks_workspace_bytes, mesh_spots_workspace_bytes, mesh_thermogram,
                                    prominence_of, read_mesh_ply, regions_mesh, smooth_temperature, spot_bounds, thermal_hotspots,
                                    write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F, D = np.float32, np.float64
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILLS = {torch.int32: -5, torch.uint8: 0xEE, torch.int64: -9}
PEAKS = ("temperature", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "coldest", "rank", "vertex_basin", "basin_peak",
         "capacity_basins", "saddles", "capacity_saddles", "counts", "workspace", "workspace_bytes", "stream")
SPOTS = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "rank", "vertex_basin", "basin_spot", "num_basins",
         "spot_peak", "spot_limit", "spot_bound", "num_spots", "coldest", "vertex_spot", "face_spot", "spots", "counts", "workspace",
         "workspace_bytes", "stream")


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _unwritten(given, now):
    for g, n in zip(given, now):
        assert np.ascontiguousarray(g).tobytes() == n.cpu().numpy().tobytes(), "an input was written"


def raw_peaks(temp, tri, coldest=False, lists=None, cap_basins=None, cap_saddles=None):
    """tn_mesh_peaks into guarded buffers; ``lists``: (offsets, corners) host arrays, default tn_mesh_incidence's own"""
    temp, tri = np.asarray(temp, F), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    v, t = len(temp), len(tri)
    if lists is None:
        index = mesh_incidence(_device(tri), v)
        lists = (index.offsets.cpu().numpy(), index.corners.cpu().numpy())
    given = [temp, tri, np.asarray(lists[0], np.int32), np.asarray(lists[1], np.int32)]
    inputs = [_device(a) for a in given]
    cap_basins = v if cap_basins is None else cap_basins
    cap_saddles = 3 * t if cap_saddles is None else cap_saddles
    out = {"rank": _buffer(v, torch.int32), "vertex_basin": _buffer(v, torch.int32),
           "basin_peak": _buffer(cap_basins, torch.int32) if cap_basins else None,
           "saddles": _buffer(4 * cap_saddles, torch.int32) if cap_saddles else None}
    counts = _buffer(3, torch.int64)
    need = mesh_peaks_workspace_bytes(v, t)
    assert need > 0
    workspace = _buffer(need, torch.uint8)
    args = dict(temperature=inputs[0].data_ptr() if v else None, triangles=inputs[1].data_ptr() if t else None, num_triangles=t,
                num_vertices=v, offsets=inputs[2].data_ptr(), corners=inputs[3].data_ptr() if t else None, coldest=1 if coldest else 0,
                capacity_basins=cap_basins, capacity_saddles=cap_saddles, counts=counts.data_ptr(), workspace=workspace.data_ptr(),
                workspace_bytes=need, stream=_hip.current_stream(), **{k: _hip.ptr(b) for k, b in out.items()})
    _hip.check(_hip.load().tn_mesh_peaks(*[args[k] for k in PEAKS]), "tn_mesh_peaks")
    torch.cuda.synchronize()
    _untouched(counts, 3, "counts")
    _untouched(workspace, need, "workspace")
    for name, buf in out.items():
        if buf is not None:
            _untouched(buf, buf.numel() - GUARD, name)
    _unwritten(given, inputs)
    return {"buffers": out, "counts": counts[:3].cpu().numpy(), "caps": (cap_basins, cap_saddles), "v": v, "t": t}


def peaks_arrays(got):
    """the host copies of what a raw call wrote, cut to the counts and the capacities"""
    b, s = min(int(got["counts"][0]), got["caps"][0]), min(int(got["counts"][1]), got["caps"][1])
    buf = got["buffers"]
    return {"rank": buf["rank"][:got["v"]].cpu().numpy(), "vertex_basin": buf["vertex_basin"][:got["v"]].cpu().numpy(),
            "basin_peak": buf["basin_peak"][:b].cpu().numpy() if b else np.zeros(0, np.int32),
            "saddles": (np.ascontiguousarray(buf["saddles"][:4 * s].cpu().numpy()).view(H.SADDLE_DTYPE) if s else np.zeros(0, H.SADDLE_DTYPE))}


def check_peaks(temp, tri, want=None, **kw):
    want = H.peaks(temp, tri, kw.get("coldest", False), kw.get("lists")) if want is None else want
    got = raw_peaks(temp, tri, **kw)
    assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
    mine = peaks_arrays(got)
    b, s = len(mine["basin_peak"]), len(mine["saddles"])
    assert mine["rank"].tobytes() == want["rank"].tobytes(), "rank"
    assert mine["vertex_basin"].tobytes() == want["vertex_basin"].tobytes(), "vertex_basin"
    assert mine["basin_peak"].tobytes() == want["basin_peak"][:b].tobytes(), "basin_peak"
    assert mine["saddles"].tobytes() == want["saddles"][:s].tobytes(), ("saddles", mine["saddles"][:8], want["saddles"][:8])
    for name, n, width in (("basin_peak", b, 1), ("saddles", s, 4)):
        if got["buffers"][name] is not None:
            _untouched(got["buffers"][name], n * width, name)
    return want, got, mine


def raw_spots(pos, temp, tri, found, basin_spot, spot_peak, spot_limit, spot_bound, coldest=False):
    """tn_mesh_spots into guarded buffers; ``found``: rank and vertex_basin as host arrays"""
    pos, temp, tri = np.asarray(pos, F).reshape(-1, 3), np.asarray(temp, F), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    v, t, b, k = len(temp), len(tri), len(basin_spot), len(spot_peak)
    given = [pos, temp, tri, found["rank"], found["vertex_basin"], np.asarray(basin_spot, np.int32), np.asarray(spot_peak, np.int32),
             np.asarray(spot_limit, np.int32), np.asarray(spot_bound, F)]
    inputs = [_device(a) for a in given]
    out = {"vertex_spot": _buffer(v, torch.int32), "face_spot": _buffer(t, torch.int32), "spots": _buffer(80 * k, torch.uint8) if k else None}
    counts = _buffer(3, torch.int64)
    need = mesh_spots_workspace_bytes(v, t, k)
    assert need > 0
    workspace = _buffer(need, torch.uint8)

    def address(i, n):
        return inputs[i].data_ptr() if n else None

    args = dict(positions=address(0, v), temperature=address(1, v), triangles=address(2, t), num_vertices=v, num_triangles=t,
                rank=address(3, v), vertex_basin=address(4, v), basin_spot=address(5, b), num_basins=b, spot_peak=address(6, k),
                spot_limit=address(7, k), spot_bound=address(8, k), num_spots=k, coldest=1 if coldest else 0, counts=counts.data_ptr(),
                workspace=workspace.data_ptr(), workspace_bytes=need, stream=_hip.current_stream(),
                vertex_spot=out["vertex_spot"].data_ptr() if v else None, face_spot=out["face_spot"].data_ptr() if t else None,
                spots=_hip.ptr(out["spots"]))
    _hip.check(_hip.load().tn_mesh_spots(*[args[n] for n in SPOTS]), "tn_mesh_spots")
    torch.cuda.synchronize()
    _untouched(counts, 3, "counts")
    _untouched(workspace, need, "workspace")
    for name, buf in out.items():
        if buf is not None:
            _untouched(buf, buf.numel() - GUARD, name)
    _unwritten(given, inputs)
    rows = np.frombuffer(out["spots"][:80 * k].cpu().numpy().tobytes(), dtype=SPOT_DTYPE) if k else np.zeros(0, SPOT_DTYPE)
    return {"vertex_spot": out["vertex_spot"][:v].cpu().numpy(), "face_spot": out["face_spot"][:t].cpu().numpy(), "spots": rows,
            "counts": counts[:3].cpu().numpy()}


def check(pos, temp, tri, min_prominence, coldest=False, extent_drop=math.inf, want=None):
    """the whole chain — the kernel's peaks, the library's merge, the Python layer's choice of spots, the kernel's spots — compared
    with the yardstick stage by stage, bit for bit"""
    want = H.hotspots(pos, temp, tri, min_prominence, coldest, extent_drop) if want is None else want
    _, _, mine = check_peaks(temp, tri, want=want["peaks"], coldest=coldest)
    temp = np.asarray(temp, F)
    basin_rank = mine["rank"][mine["basin_peak"]] if len(mine["basin_peak"]) else np.zeros(0, np.int32)
    death, parent = merge_basins(basin_rank, mine["saddles"])
    assert death.tolist() == want["death_saddle"].tolist() and parent.tolist() == want["parent"].tolist(), "the merge"
    saddle_temperature = temp[mine["saddles"]["pass_vertex"]]
    prominence = prominence_of(temp[mine["basin_peak"]], saddle_temperature, death, coldest)
    assert R.bits(prominence).tolist() == R.bits(want["prominence"]).tolist(), "prominence"
    from thermo_nerf_amd.export import BasinPersistence
    p = BasinPersistence(mine["basin_peak"], basin_rank, temp[mine["basin_peak"]], mine["saddles"], saddle_temperature, death, parent, prominence)
    basin_spot, spot_basin = choose_spots(p, min_prominence)
    assert basin_spot.tolist() == want["basin_spot"].tolist() and spot_basin.tolist() == want["spot_basin"].tolist(), "the spots"
    bound = spot_bounds(temp[mine["basin_peak"][spot_basin]], extent_drop, coldest)
    assert R.bits(bound).tolist() == R.bits(want["spot_bound"]).tolist(), "the bounds"
    got = raw_spots(pos, temp, tri, mine, basin_spot, mine["basin_peak"][spot_basin], want["spot_limit"], bound, coldest)
    assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
    assert got["vertex_spot"].tobytes() == want["vertex_spot"].tobytes(), "vertex_spot"
    assert got["face_spot"].tobytes() == want["face_spot"].tobytes(), "face_spot"
    for name in SPOT_DTYPE.names:
        assert R.bits(got["spots"][name]).tolist() == R.bits(want["spots"][name]).tolist(), (name, got["spots"][name], want["spots"][name])
    assert got["spots"].tobytes() == want["spots"].tobytes()
    return want, got


def _mesh(pos, temp, tri, colors=None):
    colors = np.zeros((len(pos), 3), np.uint8) if colors is None else colors
    return ThermalMesh(_device(np.asarray(pos, F)), _device(colors), _device(np.asarray(temp, F)), None,
                       _device(np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)), (0.0, 40.0))


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------

def test_two_bumps_on_the_lattice_whose_saddle_is_known():
    pos, temp, tri = H.two_bumps()
    want, got = check(pos, temp, tri, 1.0)
    assert want["peaks"]["basin_peak"].tolist() == [6, 18] and want["peaks"]["saddles"].tolist() == [(0, 1, 12, 2)]
    assert want["prominence"].tolist() == [math.inf, 3.0] and got["spots"]["label"].tolist() == [6, 18]
    assert got["spots"]["vertices"].tolist() == [int((want["vertex_spot"] == 0).sum()), 1] and got["spots"]["faces"][1] == 0
    assert R.bits(got["spots"]["mean_temperature"][1:]).tolist() == [0x7fc00000] and got["spots"]["area"][1] == 0.0
    want, got = check(pos, temp, tri, 3.0)
    assert len(got["spots"]) == 1 and int(got["spots"]["faces"][0]) == len(tri) == int(got["counts"][1]) and (got["vertex_spot"] == 0).all()
    whole = R.regions(pos, temp, tri)["regions"][0]
    for name in R.REGION_DTYPE.names:
        if name != "label":
            assert R.bits(got["spots"][name][:1]).tolist() == R.bits(np.array([whole[name]]).reshape(got["spots"][name][:1].shape)).tolist(), name


def test_a_constant_mesh_with_shuffled_numbering_is_one_spot_per_component():
    pos, tri = R.lattice(9, 7, 5)
    other = tri + len(pos)  # a second component
    order = np.random.default_rng(11).permutation(2 * len(pos))
    pos2, tri2 = np.concatenate([pos, pos + F(20.0)])[np.argsort(order)], order[np.concatenate([tri, other])].astype(np.int32)
    temp = np.full(len(pos2), 21.25, F)
    want, got = check(pos2, temp, tri2, 0.0)
    assert want["peaks"]["counts"][0] > 2 and len(got["spots"]) == 2, "B > 1, and exactly one spot per component"
    assert np.isinf(want["prominence"]).sum() == 2 and (want["prominence"][np.isfinite(want["prominence"])] == 0.0).all()
    assert (got["vertex_spot"] >= 0).all() and sorted(got["spots"]["faces"].tolist()) == [len(tri), len(tri)]
    assert sorted(got["spots"]["vertices"].tolist()) == [len(pos), len(pos)]


def test_a_ring_of_nan_separates_two_spots_that_never_die():
    pos, tri = H.grid(9, 9)
    x, y = np.rint(pos[:, 0]).astype(int), np.rint(pos[:, 1]).astype(int)
    ring = np.maximum(np.abs(x - 4), np.abs(y - 4)) == 2
    temp = (20.0 - np.hypot(x - 4, y - 4)).astype(F)  # one bump in the middle; outside the ring the field falls towards the corners
    temp[ring] = np.nan
    want, got = check(pos, temp, tri, 0.5)
    inside = np.maximum(np.abs(x - 4), np.abs(y - 4)) < 2
    assert len(got["spots"]) >= 2 and np.isinf(want["prominence"]).sum() == 2, "two never-dying spots"
    assert (got["vertex_spot"][ring] == -1).all() and (want["peaks"]["vertex_basin"][ring] == -1).all()
    assert set(got["vertex_spot"][inside].tolist()) == {0} and 0 not in set(got["vertex_spot"][~inside & ~ring].tolist())
    assert int(want["peaks"]["counts"][2]) == len(pos) - int(ring.sum())
    assert not set(want["peaks"]["vertex_basin"][inside].tolist()) & set(want["peaks"]["vertex_basin"][~inside & ~ring].tolist())


# ---- the long ascent ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("coldest", [False, True])
def test_long_ascent_along_a_strip_of_600(coldest):
    pos, tri = H.grid(600, 2)
    temp = (10.0 + 0.01 * np.rint(pos[:, 0]) + 0.001 * np.rint(pos[:, 1])).astype(F)  # monotone along the strip: a chain of 600 steps
    assert len(set(temp.tolist())) == 1200
    want, got = check(pos, temp, tri, 0.0, coldest=coldest)
    assert want["peaks"]["counts"].tolist() == [1, 0, 1200] and want["peaks"]["basin_peak"].tolist() == [0 if coldest else 1199]
    assert 600 > 512 and (got["vertex_spot"] == 0).all() and got["spots"]["faces"].tolist() == [len(tri)]


# ---- sizes around the tile ------------------------------------------------------------------------------------------------------------------

def _random_case(v, seed):
    tri = C.random_mesh(seed, v, 2 * v)
    rng = np.random.default_rng(seed + 100)
    temp = rng.integers(0, 4, v).astype(F) * F(1.5) + F(18.0)
    temp[rng.uniform(size=v) < 0.1] = np.nan
    pos = rng.uniform(-1.0, 1.0, (v, 3)).astype(F)
    return pos, temp, tri


RANDOM_SEEDS = {255: 1, 256: 2, 257: 3}


@pytest.mark.parametrize("v", [255, 256, 257])
@pytest.mark.parametrize("coldest", [False, True])
def test_random_meshes_around_the_tile_with_ties_nan_and_bad_triangles(v, coldest):
    pos, temp, tri = _random_case(v, RANDOM_SEEDS[v])
    want, got = check(pos, temp, tri, 0.0, coldest=coldest)
    finite = want["prominence"][np.isfinite(want["prominence"])]
    assert want["peaks"]["counts"][0] >= 2 and want["peaks"]["counts"][1] >= 1 and (finite > 0.0).sum() >= 1, "the seed's promise"
    assert np.isnan(temp).any() and (got["vertex_spot"][np.isnan(temp)] == -1).all()
    check(pos, temp, tri, 1.5, coldest=coldest)
    check(pos, temp, tri, 0.0, coldest=coldest, extent_drop=1.5)


@pytest.mark.parametrize("v", [255, 257])
def test_a_foreign_index_gives_other_numbers_and_no_access_outside(v):
    pos, temp, tri = _random_case(v, RANDOM_SEEDS[v])
    offsets, corners = H.incidence(tri, v)
    rng = np.random.default_rng(v)
    corners = corners.copy()
    spoiled = rng.choice(len(corners), 40, replace=False)
    corners[spoiled] = rng.choice([-1, -2 ** 31, 3 * len(tri), 3 * len(tri) + 9, 2 ** 31 - 1], 40)
    offsets = offsets.copy()
    offsets[rng.choice(v + 1, 12, replace=False)] = rng.choice([-7, 3 * len(tri) + 100, 2 ** 31 - 1, 0], 12)
    want, _, _ = check_peaks(temp, tri, lists=(offsets, corners))
    plain = H.peaks(temp, tri)
    assert want["vertex_basin"].tolist() != plain["vertex_basin"].tolist(), "other numbers"
    assert want["rank"].tolist() == plain["rank"].tolist()


# ---- a hub, a large spot --------------------------------------------------------------------------------------------------------------------

def test_a_fan_whose_hub_has_ten_thousand_corners():
    n = 10000
    angle = np.arange(n) * (2.0 * math.pi / n)
    pos = np.concatenate([[(0.0, 0.0, 0.0)], np.stack([np.cos(angle), np.sin(angle), np.zeros(n)], axis=1)]).astype(F)
    rim = 1 + np.arange(n)
    tri = np.stack([np.zeros(n, np.int64), rim, 1 + (np.arange(n) + 1) % n], axis=1).astype(np.int32)
    temp = np.concatenate([[20.0], 20.0 + 5.0 * np.sin(3.0 * angle) + 0.001 * np.cos(17.0 * angle)]).astype(F)  # three lobes on the rim
    want, got = check(pos, temp, tri, 1.0)
    assert want["peaks"]["counts"][0] >= 3 and len(got["spots"]) == 3 and int(want["peaks"]["vertex_basin"][0]) >= 0
    cold, _ = check(pos, temp, tri, 1.0, coldest=True)
    assert len(cold["spots"]) == 3


@functools.lru_cache(maxsize=None)
def _large():
    pos, tri = R.strip(70000, R.STRIP_SEED)
    temp = (15.0 + 1e-4 * np.arange(len(pos))).astype(F)
    return pos, temp, tri


def test_one_spot_of_70000_faces_takes_the_second_level_of_sum2():
    pos, temp, tri = _large()
    want, got = check(pos, temp, tri, 0.5)
    assert got["spots"]["faces"].tolist() == [70000] and 70000 > 256 * 256, "more than 256 partials"
    whole = R.regions(pos, temp, tri)["regions"][0]
    assert R.bits(got["spots"]["area"]).tolist() == R.bits(np.array([whole["area"]])).tolist()
    assert got["spots"]["mean_temperature"][0] == whole["mean_temperature"] and got["spots"]["centroid"][0].tolist() == whole["centroid"].tolist()


# ---- the order ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bumpy():
    """a 24 x 20 jittered lattice with a seeded field of several bumps and noise, every temperature distinct"""
    pos, tri = R.lattice(24, 20, 9)
    rng = np.random.default_rng(77)
    p = pos.astype(D)
    field = 20.0 + 4.0 * np.sin(p[:, 0] / 2.5) * np.cos(p[:, 1] / 3.0) + rng.uniform(-0.6, 0.6, len(p))
    temp = field.astype(F)
    assert len(set(temp.tolist())) == len(temp)
    return pos, temp, tri


@functools.lru_cache(maxsize=None)
def _bumpy_want(min_prominence=1.0, coldest=False, extent_drop=math.inf):
    pos, temp, tri = _bumpy()
    return H.hotspots(pos, temp, tri, min_prominence, coldest, extent_drop)


def test_bumpy_lattice_with_many_basins():
    pos, temp, tri = _bumpy()
    want, got = check(pos, temp, tri, 1.0, want=_bumpy_want())
    assert want["peaks"]["counts"][0] > 10 and want["peaks"]["counts"][1] > 30 and 2 <= len(got["spots"]) < want["peaks"]["counts"][0]
    assert (np.diff(want["prominence"][want["spot_basin"]]) <= 0).all() and (got["spots"]["faces"] > 0).sum() >= 2


def test_coldest_equals_hottest_of_the_negated_field():
    pos, temp, tri = _bumpy()
    mesh, negated = _mesh(pos, temp, tri), _mesh(pos, -temp, tri)
    cold, hot = thermal_hotspots(mesh, 1.0, coldest=True), thermal_hotspots(negated, 1.0)
    assert len(cold) >= 2 and cold.coldest and not hot.coldest
    for name in ("peak_vertex", "prominence", "saddle_vertex", "basins", "is_maximum", "spot_index"):
        assert getattr(cold, name).tolist() == getattr(hot, name).tolist(), name
    assert torch.equal(cold.vertex_spot, hot.vertex_spot) and torch.equal(cold.face_spot, hot.face_spot)
    assert (cold.num_basins, cold.num_saddles, cold.num_spots) == (hot.num_basins, hot.num_saddles, hot.num_spots)
    for name in ("label", "faces", "vertices", "area"):
        assert cold.spots[name].tolist() == hot.spots[name].tolist(), name
    a, b = mesh_peaks(mesh, coldest=True), mesh_peaks(negated)
    for name in ("rank", "vertex_basin", "basin_peak", "saddles"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    want = _bumpy_want(1.0, True)
    assert cold.peak_vertex.tolist() == want["peaks"]["basin_peak"][want["spot_basin"]].tolist()


def test_basins_and_persistence_pairs_are_invariant_under_a_vertex_permutation():
    pos, temp, tri = _bumpy()
    order = np.random.default_rng(5).permutation(len(pos))  # old vertex i becomes vertex order[i]
    back = np.argsort(order)
    moved = _mesh(pos[back], temp[back], order[tri])
    first, second = mesh_peaks(_mesh(pos, temp, tri)), mesh_peaks(moved)
    p1, p2 = basin_persistence(first, _device(temp)), basin_persistence(second, _device(temp[back]))
    assert first.num_basins == second.num_basins and first.num_saddles == second.num_saddles
    assert sorted(order[p1.basin_peak].tolist()) == sorted(p2.basin_peak.tolist())
    basin1, basin2 = first.vertex_basin.cpu().numpy(), second.vertex_basin.cpu().numpy()
    assert (order[p1.basin_peak[basin1]] == p2.basin_peak[basin2[order]]).all(), "the partition, named by its peaks"

    def pairs(p, rename):
        return sorted((int(rename[p.basin_peak[b]]), int(rename[p.saddles["pass_vertex"][s]]) if s >= 0 else -1,
                       int(rename[p.basin_peak[p.parent[b]]]) if s >= 0 else -1, float(p.prominence[b]))
                      for b, s in enumerate(p.death_saddle.tolist()))

    assert pairs(p1, order) == pairs(p2, np.arange(len(pos)))


def test_extent_drop_of_zero_keeps_the_peak_and_its_equals_and_infinity_changes_nothing():
    pos, temp, tri = _bumpy()
    flat = np.round(temp.astype(D) * 2.0) / 2.0  # half degrees: plateaus
    want, got = check(pos, flat.astype(F), tri, 0.75, extent_drop=0.0)
    for k, peak in enumerate(got["spots"]["label"]):
        inside = np.flatnonzero(got["vertex_spot"] == k)
        assert peak in inside and (flat[inside] == flat[peak]).all()
    open_, _ = check(pos, flat.astype(F), tri, 0.75, extent_drop=math.inf)
    huge, _ = check(pos, flat.astype(F), tri, 0.75, extent_drop=1e30)
    assert open_["vertex_spot"].tolist() == huge["vertex_spot"].tolist() and open_["spots"].tobytes() == huge["spots"].tobytes()
    assert (open_["vertex_spot"] >= 0).sum() > (want["vertex_spot"] >= 0).sum()
    some, _ = check(pos, temp, tri, 1.0, extent_drop=1.0)
    assert 0 < (some["vertex_spot"] >= 0).sum() < (_bumpy_want()["vertex_spot"] >= 0).sum()


# ---- capacities, empty meshes ---------------------------------------------------------------------------------------------------------------

def test_sizing_call_and_capacities_one_short():
    pos, temp, tri = _bumpy()
    want = _bumpy_want()["peaks"]
    b, s = int(want["counts"][0]), int(want["counts"][1])
    check_peaks(temp, tri, want=want, cap_basins=0, cap_saddles=0)  # NULL tables: the FULL counts alone
    _, got, mine = check_peaks(temp, tri, want=want, cap_basins=b - 1, cap_saddles=s - 1)
    assert len(mine["basin_peak"]) == b - 1 and len(mine["saddles"]) == s - 1 and got["counts"].tolist() == want["counts"].tolist()
    check_peaks(temp, tri, want=want, cap_basins=b, cap_saddles=s)
    check_peaks(temp, tri, want=want, cap_basins=1, cap_saddles=b)


def test_empty_meshes_and_meshes_without_faces_or_values():
    none = np.zeros((0, 3), np.int32)
    got = raw_peaks(np.zeros(0, F), none, lists=(np.zeros(1, np.int32), np.zeros(0, np.int32)))
    assert got["counts"].tolist() == [0, 0, 0]
    temp = np.array([3.0, np.nan, 5.0, 5.0, -np.inf, 1.0], F)
    pos = np.arange(18, dtype=F).reshape(6, 3)
    want, got = check(pos, temp, none, 0.0)  # T == 0: every finite vertex is a peak and a spot that never dies
    assert want["peaks"]["counts"].tolist() == [4, 0, 4] and want["peaks"]["rank"].tolist() == [2, 4, 0, 1, 5, 3]
    assert got["vertex_spot"].tolist() == [2, -1, 0, 1, -1, 3] and got["spots"]["vertices"].tolist() == [1, 1, 1, 1]
    assert got["counts"].tolist() == [0, 0, 0] and (got["spots"]["faces"] == 0).all() and got["spots"]["label"].tolist() == [2, 3, 0, 5]
    tri = np.array([(0, 1, 2), (2, 3, 5), (0, 6, 1), (-1, 2, 3)], np.int32)
    want, got = check(pos, np.full(6, np.nan, F), tri, 0.0)  # no vertex has a value
    assert want["peaks"]["counts"].tolist() == [0, 0, 0] and (got["vertex_spot"] == -1).all() and (got["face_spot"] == -1).all()
    want, got = check(pos, temp, tri, math.inf)  # nothing survives: K == 0, the usable faces are still counted
    assert len(got["spots"]) == 0 and got["counts"].tolist() == [0, 0, 1] and (got["vertex_spot"] == -1).all()
    empty = raw_spots(np.zeros((0, 3), F), np.zeros(0, F), tri, {"rank": np.zeros(0, np.int32), "vertex_basin": np.zeros(0, np.int32)},
                      np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    assert empty["counts"].tolist() == [0, 0, 0] and empty["face_spot"].tolist() == [-1] * 4
    mesh = _mesh(pos, temp, none)
    found = thermal_hotspots(mesh, 0.0)
    assert len(found) == 4 and found.peak_vertex.tolist() == [2, 3, 0, 5] and found.is_maximum.all() and found.num_saddles == 0
    nothing = thermal_hotspots(_mesh(np.zeros((0, 3), F), np.zeros(0, F), none), 0.0)
    assert len(nothing) == 0 and (nothing.num_basins, nothing.num_saddles, nothing.num_spots) == (0, 0, 0)


def test_the_same_call_twice_gives_the_same_bytes():
    pos, temp, tri = _bumpy()
    a, b = peaks_arrays(raw_peaks(temp, tri)), peaks_arrays(raw_peaks(temp, tri))
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def _same_result(found, want, temp, pos, keep=None):
    keep = np.arange(len(want["spot_basin"])) if keep is None else np.asarray(keep)
    basins = want["spot_basin"][keep]
    assert found.spot_index.tolist() == keep.tolist() and found.num_spots == len(want["spot_basin"])
    assert (found.num_basins, found.num_saddles) == tuple(int(c) for c in want["peaks"]["counts"][:2])
    peak = want["peaks"]["basin_peak"][basins]
    assert found.peak_vertex.tolist() == peak.tolist() and found.peak_position.tobytes() == np.asarray(pos, F)[peak].tobytes()
    assert R.bits(found.peak_temperature).tolist() == R.bits(np.asarray(temp, F)[peak]).tolist()
    assert R.bits(found.prominence).tolist() == R.bits(want["prominence"][basins]).tolist()
    death = want["death_saddle"][basins]
    assert found.is_maximum.tolist() == (death < 0).tolist()
    saddle = np.where(death >= 0, want["peaks"]["saddles"]["pass_vertex"][np.maximum(death, 0)] if len(want["peaks"]["saddles"]) else -1, -1)
    assert found.saddle_vertex.tolist() == saddle.tolist()
    assert [float(x) for x in found.saddle_temperature[death >= 0]] == [float(np.asarray(temp, F)[s]) for s in saddle[death >= 0]]
    assert np.isnan(found.saddle_temperature[death < 0]).all()
    assert found.basins.tolist() == np.bincount(want["basin_spot"][want["basin_spot"] >= 0], minlength=len(want["spot_basin"]))[keep].tolist()
    assert found.spots.tobytes() == want["spots"][keep].tobytes()
    assert found.vertex_spot.cpu().numpy().tobytes() == want["vertex_spot"].tobytes()
    assert found.face_spot.cpu().numpy().tobytes() == want["face_spot"].tobytes()


def test_thermal_hotspots_end_to_end_with_regions_mesh_and_region_map():
    pos, temp, tri = _bumpy()
    colors = np.random.default_rng(23).integers(0, 256, (len(pos), 3)).astype(np.uint8)
    mesh = _mesh(pos, temp, tri, colors)
    want = _bumpy_want()
    found = thermal_hotspots(mesh, 1.0)
    assert isinstance(found, ThermalHotspots) and len(found) == len(want["spot_basin"]) >= 2
    _same_result(found, want, temp, pos)
    area = want["spots"]["area"]
    floor = float(np.sort(area)[len(area) // 2])
    keep = np.flatnonzero(area >= floor)[:3]
    cut = thermal_hotspots(mesh, 1.0, min_area=floor, top=3)
    _same_result(cut, want, temp, pos, keep)
    assert 0 < len(cut) < len(found)
    part = regions_mesh(mesh, cut)
    faces = np.isin(want["face_spot"], keep)
    vertices = np.unique(tri[faces])
    assert part.triangles.cpu().numpy().tolist() == np.searchsorted(vertices, tri[faces]).tolist() and faces.sum() > 0
    assert part.positions.cpu().numpy().tobytes() == pos[vertices].tobytes() and part.colors.cpu().numpy().tolist() == colors[vertices].tolist()
    view = fit_view(mesh.positions, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), pixel_size=0.25)
    image = mesh_thermogram(mesh, view)
    joined = image.region_map(found).cpu().numpy()
    pixel_face = image.pixel_face.cpu().numpy()
    assert (joined == np.where(pixel_face >= 0, want["face_spot"][np.maximum(pixel_face, 0)], -1)).all() and (joined >= 0).sum() > 100
    dropped = thermal_hotspots(mesh, 1.0, extent_drop=1.0)
    _same_result(dropped, _bumpy_want(1.0, False, 1.0), temp, pos)


def test_smooth_iterations_reports_the_peaks_of_the_smoothed_field():
    pos, temp, tri = _bumpy()
    mesh = _mesh(pos, temp, tri)
    smoothed = smooth_temperature(mesh, 2)
    soft = smoothed.temperature.cpu().numpy()
    want = H.hotspots(pos, soft, tri, 0.5)
    found = thermal_hotspots(mesh, 0.5, smooth_iterations=2)
    _same_result(found, want, soft, pos)
    rough = thermal_hotspots(mesh, 0.5)
    assert found.num_basins < rough.num_basins and len(found) >= 1, "smoothing removes the noise's peaks"
    assert torch.equal(mesh.temperature, _device(temp)), "the input mesh keeps its temperature"


def test_command_line_end_to_end(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("mesh_hotspots_tool", os.path.join(ROOT, "tools", "mesh_hotspots.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pos, temp, tri = _bumpy()
    temp = temp.copy()
    temp[[5, 77, 300]] = np.nan  # as mesh_compare.py and mesh_project.py leave a vertex nothing saw
    colors = np.random.default_rng(23).integers(0, 256, (len(pos), 3)).astype(np.uint8)
    mesh = _mesh(pos, temp, tri, colors)
    source, report_file, part_file = tmp_path / "bumpy.ply", tmp_path / "out" / "spots.json", tmp_path / "spots.ply"
    write_mesh_ply(source, mesh)
    assert tool.main([str(source), "--min-prominence", "1.0", "--top", "3", "--extent-drop", "2.5", "--report", str(report_file),
                      "--output", str(part_file), "--device", DEV]) == 0
    printed = capsys.readouterr().out
    found = thermal_hotspots(mesh, 1.0, top=3, extent_drop=2.5)
    want = H.hotspots(pos, temp, tri, 1.0, extent_drop=2.5)
    _same_result(found, want, temp, pos, np.arange(3))
    report = json.loads(report_file.read_text())
    assert report == json.loads(json.dumps(tool.build_report(found, len(pos), len(tri), 2.5, 0, 1.0, str(source))))
    assert report["counts"]["reported_spots"] == 3 == printed.count("\nspot ") and report["counts"]["basins"] == int(want["peaks"]["counts"][0])
    assert [r["peak"]["index"] for r in report["spots"]] == found.peak_vertex.tolist()
    part = read_mesh_ply(part_file)
    faces = np.isin(want["face_spot"], np.arange(3))
    vertices = np.unique(tri[faces])
    assert part["triangles"].tolist() == np.searchsorted(vertices, tri[faces]).tolist() and faces.sum() > 0
    assert part["positions"].tobytes() == pos[vertices].tobytes() and part["colors"].tolist() == colors[vertices].tolist()
    # cold spots, smoothed, scaled: lengths doubled, areas four-fold, degrees as they are
    flags = [str(source), "--min-prominence", "0.5", "--coldest", "--smooth-iterations", "1", "--report", str(report_file), "--device", DEV]
    assert tool.main(flags) == 0
    plain = json.loads(report_file.read_text())
    assert tool.main(flags + ["--length-scale", "2"]) == 0
    scaled = json.loads(report_file.read_text())
    cold = thermal_hotspots(mesh, 0.5, coldest=True, smooth_iterations=1)
    assert plain["coldest"] and [r["peak"]["index"] for r in plain["spots"]] == cold.peak_vertex.tolist() and len(cold) >= 1
    assert [r["area"] for r in scaled["spots"]] == [4.0 * r["area"] for r in plain["spots"]]
    assert [r["peak"]["position"] for r in scaled["spots"]] == [[2.0 * c for c in r["peak"]["position"]] for r in plain["spots"]]
    for name in ("prominence", "mean_temperature", "faces", "vertices", "saddle"):
        assert [r[name] for r in scaled["spots"]] == [r[name] for r in plain["spots"]], name
