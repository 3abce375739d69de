"""tn_mesh_geodesic and tn_mesh_distance_bands on the device against tests/mesh_geodesic_reference.py — the plain every-vertex
definition — exactly: every distance's bit pattern, every label, every count and every byte of the band rows, no tolerance anywhere,
into guarded buffers with the workspace guard kept and the inputs unwritten: the 5 x 5 lattice by hand, a 2 x 600 strip over several
batches, the iterate of either parity under a cut, the 129 x 129 lattice, the slit whose front turns around its end, random meshes around the
block size with ties, NaN and foreign indices, a hub of 10^4 corners, two components, a finite max_distance, a vertex permutation, a
continued solve, empty meshes, the bands, and the Python layer with the command line."""
from __future__ import annotations

import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_geodesic_reference as G
from tests import mesh_regions_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (BAND_DTYPE, ThermalMesh, build_mesh_bvh, distance_at_points, distance_profile, geodesic_distance,
                                    isotherms, mesh_closest, mesh_distance_bands_workspace_bytes, mesh_geodesic_workspace_bytes, mesh_incidence,
                                    read_mesh_ply, seeds_at_points, seeds_of_regions, surface_distance, thermal_hotspots,
                                    thermal_regions, write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F, D = np.float32, np.float64
GUARD = 96
FILLS = {torch.int32: -5, torch.uint8: 0xEE, torch.int64: -9, torch.float64: -7.25}
GEODESIC = ("positions", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "seed_vertex", "seed_offset", "num_seeds",
            "max_distance", "restart", "rounds", "distance", "nearest_seed", "counts", "workspace", "workspace_bytes",
            "stream")
BANDS = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "distance", "nearest_seed", "width", "bands", "cell",
         "rows", "counts", "workspace", "workspace_bytes", "stream")


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Solver:
    """tn_mesh_geodesic into guarded buffers, call after call on the same state"""

    def __init__(self, pos, tri, seeds, offsets=None, limit=math.inf, lists=None):
        pos, tri = np.asarray(pos, F).reshape(-1, 3), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.v, self.t = len(pos), len(tri)
        if lists is None and self.v:
            index = mesh_incidence(_device(tri), self.v)
            lists = (index.offsets.cpu().numpy(), index.corners.cpu().numpy())
        seeds = np.asarray(seeds, np.int32).reshape(-1)
        offsets = np.zeros(len(seeds), D) if offsets is None else np.asarray(offsets, D).reshape(-1)
        self.given = [pos, tri, np.asarray(lists[0], np.int32), np.asarray(lists[1], np.int32), seeds, offsets] if self.v else []
        self.inputs = [_device(a) for a in self.given]
        self.distance, self.nearest = _buffer(self.v, torch.float64), _buffer(self.v, torch.int32)
        self.counts = _buffer(2, torch.int64)
        self.need = mesh_geodesic_workspace_bytes(self.v, self.t)
        assert self.need > 0
        self.workspace = _buffer(self.need, torch.uint8)
        self.limit, self.seeds = float(limit), len(seeds)

    def call(self, restart, rounds):
        i = self.inputs
        args = dict(positions=i[0].data_ptr(), triangles=i[1].data_ptr() if self.t else None, num_triangles=self.t, num_vertices=self.v,
                    offsets=i[2].data_ptr(), corners=i[3].data_ptr() if self.t else None, seed_vertex=i[4].data_ptr() if self.seeds else None,
                    seed_offset=i[5].data_ptr() if self.seeds else None, num_seeds=self.seeds, max_distance=self.limit, restart=restart,
                    rounds=rounds, distance=self.distance.data_ptr(), nearest_seed=self.nearest.data_ptr(),
                    counts=self.counts.data_ptr(), workspace=self.workspace.data_ptr(), workspace_bytes=self.need,
                    stream=_hip.current_stream())
        _hip.check(_hip.load().tn_mesh_geodesic(*[args[k] for k in GEODESIC]), "tn_mesh_geodesic")
        torch.cuda.synchronize()
        _untouched(self.counts, 2, "counts")
        _untouched(self.workspace, self.need, "workspace")
        _untouched(self.distance, self.v, "distance")
        _untouched(self.nearest, self.v, "nearest_seed")
        for g, n in zip(self.given, self.inputs):
            assert g.tobytes() == n.cpu().numpy().tobytes(), "an input was written"
        return self.state()

    def state(self):
        rounds, fixed = self.counts[:2].cpu().tolist()
        return dict(distance=self.distance[:self.v].cpu().numpy(), nearest_seed=self.nearest[:self.v].cpu().numpy(), rounds=int(rounds),
                    converged=bool(fixed))

    def run(self, batch=256, limit_calls=64):
        got = self.call(1, batch)
        calls = 1
        while not got["converged"]:
            assert calls < limit_calls, "the solve does not end"
            got = self.call(0, batch)
            calls += 1
        return got, calls


def same(got, want, what=""):
    assert (got["rounds"], got["converged"]) == (want["rounds"], want["converged"]), (what, got["rounds"], got["converged"], want["rounds"])
    mine, theirs = R.bits(got["distance"]), R.bits(want["distance"])
    wrong = np.flatnonzero(mine != theirs)
    assert len(wrong) == 0, (what, "distance", len(wrong), wrong[:5], got["distance"][wrong[:5]], want["distance"][wrong[:5]])
    wrong = np.flatnonzero(got["nearest_seed"] != want["nearest_seed"])
    assert len(wrong) == 0, (what, "nearest_seed", len(wrong), wrong[:5], got["nearest_seed"][wrong[:5]], want["nearest_seed"][wrong[:5]])


def check(pos, tri, seeds, offsets=None, limit=math.inf, lists=None, batch=256, want=None, **kw):
    want = G.solve(pos, tri, seeds, offsets, limit, lists=lists) if want is None else want
    got, calls = Solver(pos, tri, seeds, offsets, limit, lists, **kw).run(batch)
    same(got, want)
    return want, got, calls


def _mesh(pos, temp, tri):
    return ThermalMesh(_device(np.asarray(pos, F)), _device(np.zeros((len(pos), 3), np.uint8)), _device(np.asarray(temp, F)), None,
                       _device(np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)), (0.0, 40.0))


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------

def test_the_5_x_5_lattice_from_its_centre_is_the_euclidean_distance():
    pos, tri = G.lattice(5, 5)
    want, got, _ = check(pos, tri, [12])
    assert got["distance"][12] == 0.0 and got["distance"][7] == 1.0 and got["distance"][6] == math.sqrt(2.0)  # an edge, the diagonal
    assert got["distance"][0] == 2.0 * math.sqrt(2.0)                     # along the cells' own diagonal
    assert abs(got["distance"][5 * 1 + 4] - math.sqrt(5.0)) < 1e-15       # (1, 4): through two faces, no edge leads there
    assert abs(got["distance"][4] - 2.0 * math.sqrt(2.0)) < 4e-15         # (0, 4): across the cells' diagonals
    assert (got["nearest_seed"] == 0).all() and got["converged"] and got["rounds"] == want["rounds"] <= 5


def test_two_seeds_on_the_5_x_5_lattice_share_it_along_the_tie_line():
    pos, tri = G.lattice(5, 5)
    want, got, _ = check(pos, tri, [2 * 5 + 0, 2 * 5 + 4])  # (2, 0) and (2, 4): the vertices with y = 2 are as far from either
    label = got["nearest_seed"].reshape(5, 5)
    assert (label[:, :2] == 0).all() and (label[:, 3:] == 1).all()
    row = got["distance"].reshape(5, 5)[2]
    assert row[[0, 1, 3, 4]].tolist() == [0.0, 1.0, 1.0, 0.0] and abs(row[2] - 2.0) < 1e-15  # (a face candidate rounds below the edges' 2)
    tie = want["nearest_seed"].reshape(5, 5)[:, 2]
    assert label[:, 2].tolist() == tie.tolist() and set(tie.tolist()) <= {0, 1}  # the first candidate in list order keeps a tie
    # a duplicate seed keeps the smallest offset and then the lowest number; a seed outside [0, V) is ignored
    want, got, _ = check(pos, tri, [10, 14, 10, 14, 99, -3], [0.5, 0.25, 0.25, 0.25, 0.0, 0.0])
    assert got["nearest_seed"][10] == 2 and got["nearest_seed"][14] == 1 and got["distance"][10] == 0.25
    assert set(got["nearest_seed"].tolist()) == {1, 2}


# ---- batches, the flag, the parity ------------------------------------------------------------------------------------------------------

def test_the_2_x_600_strip_takes_several_batches_and_then_changes_nothing():
    pos, tri = G.lattice(2, 600)
    want = G.solve(pos, tri, [0])
    assert 590 <= want["rounds"] <= 600
    solver = Solver(pos, tri, [0])
    got, calls = solver.run(batch=256)
    same(got, want)
    assert calls == want["rounds"] // 256 + 1, "the rounds queued after the one that changed nothing returned on the flag"
    again = solver.call(0, 64)
    same(again, want, "a further call")
    assert abs(got["distance"][599] - 599.0) < 1e-9 and abs(got["distance"][600 + 599] - math.hypot(599.0, 1.0)) < 1e-9


@pytest.mark.parametrize("cut", [10, 11])
def test_a_cut_gives_the_iterate_of_either_parity(cut):
    pos, tri = G.lattice(2, 600)
    want = G.solve(pos, tri, [0], max_rounds=cut)
    assert want["rounds"] == cut and not want["converged"]
    solver = Solver(pos, tri, [0])
    same(solver.call(1, cut), want)
    assert np.isfinite(want["distance"]).sum() < 2 * (cut + 2)
    # in two calls of odd length, then on to the end
    solver = Solver(pos, tri, [0])
    solver.call(1, 3)
    same(solver.call(0, cut - 3), want, "3 + the rest")
    got = solver.call(0, 4096)
    same(got, G.solve(pos, tri, [0]), "continued to the end")


def test_restart_0_continues_and_restart_1_starts_again():
    pos, tri = G.lattice(9, 7, "alternating", jitter=0.3, seed=4)
    whole = G.solve(pos, tri, [3, 40], [0.0, 0.5])
    solver = Solver(pos, tri, [3, 40], [0.0, 0.5])
    for rounds in (0, 1, 2, 1):
        part = solver.call(0 if rounds != 0 else 1, rounds)
    same(part, G.solve(pos, tri, [3, 40], [0.0, 0.5], max_rounds=4), "0 + 1 + 2 + 1 rounds")
    same(solver.call(0, 100), whole)
    same(solver.call(1, 100), whole, "started again")
    half = G.solve(pos, tri, [3, 40], [0.0, 0.5], max_rounds=2)
    same(Solver(pos, tri, [3, 40], [0.0, 0.5]).call(1, 2), half)
    assert G.solve(pos, tri, [], start=(half["distance"], half["nearest_seed"]))["distance"].tobytes() == whole["distance"].tobytes()


# ---- the lattices -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big(pattern):
    return G.lattice(129, 129, pattern)


def test_the_129_x_129_lattice_from_a_corner():
    pos, tri = _big("same")
    want, got, calls = check(pos, tri, [0], batch=64)
    assert calls >= 3
    euclid = np.linalg.norm(pos.astype(D), axis=1)
    assert np.abs(got["distance"][1:] / euclid[1:] - 1.0).max() < 1e-12


def test_the_129_x_129_lattice_from_three_seeds_with_offsets():
    pos, tri = _big("alternating")
    want, got, _ = check(pos, tri, [5 * 129 + 7, 100 * 129 + 20, 64 * 129 + 120], [0.0, 3.5, 10.0])
    assert set(got["nearest_seed"].tolist()) == {0, 1, 2}


def test_the_slit_lattice_whose_front_turns_around_the_end():
    pos, tri = G.slit_lattice()
    seed, goal = 16 * 65 + 16, 16 * 65 + 49
    want, got, _ = check(pos, tri, [seed], batch=100)
    around = 2.0 * math.hypot(32.0, 16.0) + 1.0  # to the slit's end at (48, 32), across it, back
    assert around < got["distance"][goal] < 1.01 * around


# ---- random meshes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,lo,hi", [(1, 250, 270), (2, 250, 270), (3, 250, 270), (6, 500, 530), (7, 500, 530), (10, 500, 530),
                                        (35, 500, 530)])
def test_random_meshes_around_the_block_size(seed, lo, hi):
    pos, tri, seeds, offsets, limit = G.soup(seed, lo, hi)
    want, got, _ = check(pos, tri, seeds, offsets, limit)
    assert np.isfinite(want["distance"]).sum() > 2


def test_a_hub_of_10_000_corners():
    pos, tri = G.hub(10_000)
    want, got, _ = check(pos, tri, [0])
    assert (np.abs(got["distance"][1:] - 1.0) < 1e-6).all() and got["rounds"] == 1
    # from every 100th vertex of the rim: the hub's thread walks its 10^4 corners in every one of some 50 rounds
    want, got, _ = check(pos, tri, 1 + 100 * np.arange(100), 0.001 * (np.arange(100) % 7))
    assert abs(got["distance"][0] - 1.0) < 1e-6 and 45 <= got["rounds"] <= 55 and len(set(got["nearest_seed"].tolist())) == 100


def test_two_components_with_a_seed_in_one():
    pos, tri = G.lattice(6, 6)
    pos2 = pos.copy()
    pos2[:, 0] += 10.0
    both, faces = np.concatenate([pos, pos2]), np.concatenate([tri, tri + 36])
    want, got, _ = check(both, faces, [7])
    assert np.isfinite(got["distance"][:36]).all() and (got["distance"][36:] == math.inf).all() and (got["nearest_seed"][36:] == -1).all()


def test_a_finite_max_distance():
    pos, tri = G.lattice(33, 33, "alternating", jitter=0.3, seed=9)
    free = G.solve(pos, tri, [16 * 33 + 16])
    want, got, _ = check(pos, tri, [16 * 33 + 16], limit=9.5)
    reached = np.isfinite(got["distance"])
    assert (got["distance"][reached] <= 9.5).all() and 0 < reached.sum() < len(pos) and (got["nearest_seed"][~reached] == -1).all()
    # what is reached has the unlimited run's distance; a vertex the unlimited run reaches within 9.5 only through a face whose other
    # vertex lies beyond 9.5 stays unreached, so the converse does not hold
    assert (want["distance"][reached] == free["distance"][reached]).all() and (free["distance"][~reached] > 8.0).all()


def test_the_distances_do_not_depend_on_the_numbering():
    pos, tri = G.lattice(33, 33, "same", jitter=0.3, seed=5)
    rng = np.random.default_rng(11)
    new_of_old = rng.permutation(len(pos))
    moved = np.empty_like(pos)
    moved[new_of_old] = pos
    faces = new_of_old[tri][rng.permutation(len(tri))].astype(np.int32)
    want, _, _ = check(pos, tri, [40, 900], [0.0, 1.25])
    other, got, _ = check(moved, faces, new_of_old[[40, 900]], [0.0, 1.25])
    assert want["distance"].tobytes() == other["distance"][new_of_old].tobytes(), "the yardstick shows it"
    assert got["distance"][new_of_old].tobytes() == want["distance"].tobytes()


def test_no_vertices_and_no_triangles():
    lib = _hip.load()
    args = dict(positions=None, triangles=None, num_triangles=0, num_vertices=0, offsets=None, corners=None, seed_vertex=None,
                seed_offset=None, num_seeds=0, max_distance=math.inf, restart=1, rounds=3, distance=None, nearest_seed=None,
                counts=None, workspace=None, workspace_bytes=0, stream=_hip.current_stream())
    assert lib.tn_mesh_geodesic(*[args[k] for k in GEODESIC]) == 0
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F)
    got, calls = Solver(pos, np.zeros((0, 3), np.int32), [1], [0.5], lists=(np.zeros(4, np.int32), np.zeros(0, np.int32))).run()
    assert got["distance"].tolist() == [math.inf, 0.5, math.inf] and got["nearest_seed"].tolist() == [-1, 0, -1]
    assert got["rounds"] == 0 and got["converged"] and calls == 1


# ---- the bands --------------------------------------------------------------------------------------------------------------------------

def raw_bands(pos, temp, tri, dist, seed, width, k, cell=-1):
    pos, temp, tri = np.asarray(pos, F).reshape(-1, 3), np.asarray(temp, F), np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    dist, seed = np.asarray(dist, D), np.asarray(seed, np.int32)
    v, t = len(pos), len(tri)
    given = [pos, temp, tri, dist, seed]
    inputs = [_device(a) for a in given]
    rows, counts = _buffer(40 * k, torch.uint8), _buffer(3, torch.int64)
    need = mesh_distance_bands_workspace_bytes(v, t, k)
    assert need > 0
    workspace = _buffer(need, torch.uint8)
    args = dict(positions=inputs[0].data_ptr() if v else None, temperature=inputs[1].data_ptr() if v else None,
                triangles=inputs[2].data_ptr() if t else None, num_vertices=v, num_triangles=t, distance=inputs[3].data_ptr() if v else None,
                nearest_seed=inputs[4].data_ptr() if v else None, width=float(width), bands=k, cell=cell, rows=rows.data_ptr(),
                counts=counts.data_ptr(), workspace=workspace.data_ptr(), workspace_bytes=need, stream=_hip.current_stream())
    _hip.check(_hip.load().tn_mesh_distance_bands(*[args[n] for n in BANDS]), "tn_mesh_distance_bands")
    torch.cuda.synchronize()
    _untouched(rows, 40 * k, "rows")
    _untouched(counts, 3, "counts")
    _untouched(workspace, need, "workspace")
    for g, n in zip(given, inputs):
        assert g.tobytes() == n.cpu().numpy().tobytes(), "an input was written"
    return np.frombuffer(rows[:40 * k].cpu().numpy().tobytes(), dtype=BAND_DTYPE), counts[:3].cpu().numpy()


def check_bands(pos, temp, tri, dist, seed, width, k, cell=-1):
    want, counts, _ = G.bands(pos, temp, tri, dist, seed, width, k, cell)
    got, mine = raw_bands(pos, temp, tri, dist, seed, width, k, cell)
    assert mine.tolist() == counts.tolist(), (mine, counts)
    for name in BAND_DTYPE.names:
        assert R.bits(got[name]).tolist() == R.bits(want[name]).tolist(), (name, got[name][:8], want[name][:8])
    assert got.tobytes() == want.tobytes()
    return got, mine


def test_bands_by_hand_on_the_5_x_5_lattice():
    pos, tri = G.lattice(5, 5)
    dist = pos[:, 0].astype(D)            # the distance from the edge x = 0
    temp = (20.0 + 2.0 * pos[:, 0]).astype(F)
    got, counts = check_bands(pos, temp, tri, dist, np.zeros(25, np.int32), 1.0, 6)
    # a column of cells is 8 faces of area 1/2 with mean distances x + 1/3 and x + 2/3: band x
    assert got["faces"].tolist() == [8, 8, 8, 8, 0, 0] and got["area"].tolist() == [4.0, 4.0, 4.0, 4.0, 0.0, 0.0]
    assert counts.tolist() == [4, 32, 32] and got["warm_area"].tolist() == got["area"].tolist()
    assert got["mean_temperature"][:4].tolist() == [21.0, 23.0, 25.0, 27.0] and np.isnan(got["mean_temperature"][4:]).all()
    assert R.bits(got["min_temperature"][4:]).tolist() == [0x7fc00000] * 2 == R.bits(got["max_temperature"][4:]).tolist()
    # two bands are too few: the faces beyond them are measured, not banded
    got, counts = check_bands(pos, temp, tri, dist, np.zeros(25, np.int32), 1.0, 2)
    assert counts.tolist() == [2, 16, 32]


def test_bands_with_cells_nan_temperatures_unreached_vertices_and_empty_bands():
    pos, tri = G.lattice(21, 17, "alternating", jitter=0.3, seed=3)
    solved = G.solve(pos, tri, [2 * 17 + 3, 15 * 17 + 12], max_distance=11.0)
    dist, seed = solved["distance"], solved["nearest_seed"]
    assert not np.isfinite(dist).all()
    rng = np.random.default_rng(8)
    temp = rng.uniform(15.0, 30.0, len(pos)).astype(F)
    temp[rng.uniform(size=len(pos)) < 0.1] = np.nan
    faces = tri.copy()
    faces[5, 1], faces[9, 2], faces[11] = faces[5, 0], len(pos), (3, 4, -1)
    for cell in (-1, 0, 1, 7):
        got, counts = check_bands(pos, temp, faces, dist, seed, 0.75, 24, cell)
        assert (counts[0] > 0) == (cell != 7)
    whole, _ = check_bands(pos, temp, faces, dist, seed, 0.75, 24)
    assert (whole["warm_faces"] < whole["faces"]).any() and (whole["faces"] == 0).any() and (whole["warm_area"] < whole["area"]).any()


def test_one_band_of_70_000_faces_and_4096_bands():
    pos, tri = G.lattice(190, 190, "same", jitter=0.25, seed=2)
    assert len(tri) > 70_000
    dist = np.linalg.norm(pos.astype(D), axis=1)
    temp = (20.0 + np.sin(0.1 * pos[:, 0]) * 5.0 + 0.01 * pos[:, 1]).astype(F)
    got, counts = check_bands(pos, temp, tri, dist, np.zeros(len(pos), np.int32), 1000.0, 1)   # partials of partials
    assert counts.tolist() == [1, len(tri), len(tri)] and got["faces"][0] == len(tri)
    got, counts = check_bands(pos, temp, tri, dist, np.zeros(len(pos), np.int32), 0.0625, 4096)
    assert counts[0] > 3000 and counts[1] < counts[2] == len(tri)


def test_bands_of_an_empty_mesh():
    got, counts = raw_bands(np.zeros((0, 3), F), np.zeros(0, F), np.zeros((0, 3), np.int32), np.zeros(0, D), np.zeros(0, np.int32), 1.0, 3)
    assert got["faces"].tolist() == [0, 0, 0] and got["area"].tolist() == [0.0] * 3 and np.isnan(got["mean_temperature"]).all()
    assert counts.tolist() == [0, 0, 0]
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F)
    got, counts = check_bands(pos, np.ones(3, F), np.zeros((0, 3), np.int32), np.zeros(3, D), np.zeros(3, np.int32), 1.0, 2)
    assert counts.tolist() == [0, 0, 0]


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def _bumps():
    pos, tri = G.lattice(41, 41, "alternating", jitter=0.2, seed=6)
    x, y = pos[:, 0].astype(D), pos[:, 1].astype(D)
    temp = 18.0 + 8.0 * np.exp(-((x - 10) ** 2 + (y - 12) ** 2) / 18.0) + 6.0 * np.exp(-((x - 30) ** 2 + (y - 28) ** 2) / 30.0)
    return pos, temp.astype(F), tri


def test_geodesic_distance_and_its_mesh_through_regions_and_isotherms():
    pos, temp, tri = _bumps()
    mesh = _mesh(pos, temp, tri)
    seeds = [10 * 41 + 12, 30 * 41 + 28]
    want = G.solve(pos, tri, seeds, [0.0, 1.0], 25.0)
    d = geodesic_distance(mesh, seeds, [0.0, 1.0], max_distance=25.0)
    same(dict(distance=d.distance.cpu().numpy(), nearest_seed=d.nearest_seed.cpu().numpy(), rounds=d.rounds, converged=d.converged), want)
    assert d.reached == int(np.isfinite(want["distance"]).sum()) < len(pos) and d.num_seeds == 2
    cut = geodesic_distance(mesh, seeds, [0.0, 1.0], max_distance=25.0, max_rounds=7)
    part = G.solve(pos, tri, seeds, [0.0, 1.0], 25.0, max_rounds=7)
    same(dict(distance=cut.distance.cpu().numpy(), nearest_seed=cut.nearest_seed.cpu().numpy(), rounds=cut.rounds, converged=cut.converged), part)
    assert not cut.converged and cut.rounds == 7
    as_degrees = d.mesh.temperature.cpu().numpy().reshape(-1)
    value = want["distance"].astype(F)
    assert R.bits(as_degrees).tolist() == R.bits(np.where(np.isfinite(value), value, R.NAN)).tolist()
    assert torch.equal(mesh.temperature, _device(temp)), "the input mesh keeps its temperature"
    near = thermal_regions(d.mesh, max_temperature=5.0)
    plain = R.regions(pos, as_degrees, tri, -math.inf, 5.0)
    assert near.face_region.cpu().numpy().tobytes() == plain["face_region"].tobytes() and len(near) == 2
    curves = isotherms(d.mesh, [3.0])
    assert len(curves.curves) == 2 and bool(curves.curves["closed"].all())
    profile = distance_profile(mesh, d, 1.0, 30, cell=0)
    rows, counts, _ = G.bands(pos, temp, tri, want["distance"], want["nearest_seed"], 1.0, 30, 0)
    assert profile.bands.tobytes() == rows.tobytes() and (profile.banded_faces, profile.measured_faces) == (int(counts[1]), int(counts[2]))
    assert profile.cumulative_area.tolist() == np.cumsum(rows["area"]).tolist() and profile.centres[:2].tolist() == [0.5, 1.5]
    mean = profile.bands["mean_temperature"]
    assert mean[0] > mean[3] > mean[6], "the bump's temperature decays with the distance from its peak"


def test_seeds_of_regions_from_the_hot_spots():
    pos, temp, tri = _bumps()
    mesh = _mesh(pos, temp, tri)
    spots = thermal_hotspots(mesh, 1.0, extent_drop=2.0)
    assert len(spots) == 2
    face_spot = spots.face_spot.cpu().numpy()
    for k, faces in ((None, face_spot >= 0), (1, face_spot == 1)):
        seeds, offsets = seeds_of_regions(mesh, spots, k)
        assert offsets is None and seeds.tolist() == np.unique(tri[faces]).tolist() and len(seeds) > 3
    d = geodesic_distance(mesh, seeds)
    want = G.solve(pos, tri, seeds)
    same(dict(distance=d.distance.cpu().numpy(), nearest_seed=d.nearest_seed.cpu().numpy(), rounds=d.rounds, converged=d.converged), want)
    warm = thermal_regions(mesh, min_temperature=22.0)
    seeds, _ = seeds_of_regions(mesh, warm)
    assert seeds.tolist() == np.unique(tri[warm.face_region.cpu().numpy() >= 0]).tolist()
    with pytest.raises(ValueError):
        seeds_of_regions(_mesh(*_small()), spots)


def _small():
    pos, tri = G.lattice(5, 5)
    return pos, np.linspace(10.0, 20.0, 25).astype(F), tri


def _inside(pos, face, p):
    """p lies strictly inside the face, in the plane z = 0"""
    a, b, c = (pos[i].astype(D) for i in face)
    side = lambda u, w: (w[0] - u[0]) * (p[1] - u[1]) - (w[1] - u[1]) * (p[0] - u[0])  # noqa: E731
    s = [side(a, b), side(b, c), side(c, a)]
    return all(x > 0 for x in s) or all(x < 0 for x in s)


def test_the_tape_measure_across_the_slit():
    pos, tri = G.slit_lattice()
    mesh = _mesh(pos, np.full(len(pos), 20.0, F), tri)
    bvh = build_mesh_bvh(mesh)
    a, b = (16.3, 16.4, 0.0), (16.6, 49.7, 0.0)
    got = surface_distance(mesh, bvh, a, b)
    around = math.hypot(48.0 - 16.3, 32.0 - 16.4) + 1.0 + math.hypot(48.0 - 16.6, 49.7 - 33.0)
    assert got > around, "no path is shorter than the one around the slit's end"
    # the same through the yardstick: the seeds of a's face with their offsets, then the update at b
    pa, pb = _device(np.array([a], F)), _device(np.array([b], F))
    seeds, offsets = seeds_at_points(bvh, pa)
    face = np.flatnonzero([(set(f) == set(seeds.tolist())) for f in tri.tolist()])
    assert len(face) == 1 and np.allclose(offsets, np.linalg.norm(pos[seeds].astype(D) - np.array(a, F).astype(D), axis=1), atol=1e-6)
    want = G.solve(pos, tri, seeds, offsets)
    d = geodesic_distance(mesh, seeds, offsets)
    assert d.distance.cpu().numpy().tobytes() == want["distance"].tobytes()
    there = distance_at_points(mesh, d, bvh, pb)
    assert there.shape == (1,) and there[0] == got
    placed = mesh_closest(bvh, pb).closest_point.cpu().numpy()[0].astype(D)  # where the layer placed b, in float32
    face = [f for f in tri.tolist() if _inside(pos, f, placed)]
    assert len(face) == 1
    by_hand = math.inf
    for i in range(3):
        va, vb = face[0][i], face[0][(i + 1) % 3]
        for cand, _ in G.candidates(placed, pos[va].astype(D), pos[vb].astype(D), want["distance"][va], want["distance"][vb]):
            by_hand = min(by_hand, float(cand))
    assert got == by_hand, (got, by_hand)  # the yardstick's update at the placed point, to the bit
    # a limit between the face's vertices and the point's own distance: the point is not reached
    short = geodesic_distance(mesh, seeds, offsets, max_distance=math.nextafter(got, 0.0))
    assert math.isinf(distance_at_points(mesh, short, bvh, pb)[0])
    assert surface_distance(mesh, bvh, a, b, max_distance=30.0) == math.inf
    # on the plane next to the seed the measure is the straight line
    c = (18.1, 15.2, 0.0)
    assert abs(surface_distance(mesh, bvh, a, c) - math.dist(np.array(a, F).astype(D), np.array(c, F).astype(D))) < 1e-5


def test_command_line_end_to_end(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("mesh_distance_tool", os.path.join(ROOT, "tools", "mesh_distance.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pos, temp, tri = _bumps()
    mesh = _mesh(pos, temp, tri)
    source = tmp_path / "bumps.ply"
    write_mesh_ply(source, mesh)
    report_file, profile_file, out_file = tmp_path / "out" / "distance.json", tmp_path / "out" / "profile.csv", tmp_path / "distance.ply"
    flags = [str(source), "--from-hotspots", "1.0", "--band-width", "2.0", "--bands", "8", "--to-point", "20.2", "20.7", "0",
             "--report", str(report_file), "--profile", str(profile_file), "--output", str(out_file), "--device", DEV]
    assert tool.main(flags) == 0
    printed = capsys.readouterr().out
    spots = thermal_hotspots(mesh, 1.0)
    want = G.solve(pos, tri, spots.peak_vertex)
    report = json.loads(report_file.read_text())
    assert (report["rounds"], report["converged"], report["seeds"]) == (want["rounds"], True, 2) and "2 seeds" in printed
    far = int(np.argmax(want["distance"]))
    assert report["farthest"]["index"] == far and report["farthest"]["distance"] == float(want["distance"][far])
    assert report["reached_share"] == 1.0 and report["sources"] == {"hotspots": 2}
    d = geodesic_distance(mesh, spots.peak_vertex)
    there = distance_at_points(mesh, d, build_mesh_bvh(mesh), _device(np.array([(20.2, 20.7, 0.0)], F)))
    assert report["to_point"]["distance"] == float(there[0]) and 8.0 < there[0] < 16.0
    cells = report["cells"]
    assert [c["vertex"] for c in cells] == spots.peak_vertex.tolist() and sum(c["vertices"] for c in cells) == len(pos)
    for c in cells:
        one, _, _ = G.bands(pos, temp, tri, want["distance"], want["nearest_seed"], 2.0 * float(want["distance"][far]) + 1.0, 1, c["seed"])
        assert c["area"] == float(one["area"][0]) and c["mean_temperature"] == float(one["mean_temperature"][0])
        assert c["farthest_distance"] == float(want["distance"][want["nearest_seed"] == c["seed"]].max())
    lines = profile_file.read_text().splitlines()
    assert lines[0] == "seed,band,from,to,area,mean_temperature,min_temperature,max_temperature" and len(lines) == 1 + 3 * 8
    rows, _, _ = G.bands(pos, temp, tri, want["distance"], want["nearest_seed"], 2.0, 8)
    first = lines[1].split(",")
    assert first[:4] == ["-1", "0", "0.0", "2.0"] and float(first[4]) == float(rows["area"][0]) and float(first[5]) == float(rows["mean_temperature"][0])
    written = read_mesh_ply(out_file)
    assert written["positions"].tobytes() == pos.tobytes() and written["triangles"].tolist() == tri.tolist()
    assert R.bits(written["temperature"].reshape(-1)).tolist() == R.bits(want["distance"].astype(F)).tolist()
    # from a vertex and a temperature window, scaled: lengths doubled, areas four-fold
    flags = [str(source), "--from-vertex", "0", "--from-min-temperature", "24", "--band-width", "2.0", "--bands", "4", "--max-distance", "12",
             "--report", str(report_file), "--profile", str(profile_file), "--device", DEV]
    assert tool.main(flags) == 0
    plain, plain_lines = json.loads(report_file.read_text()), profile_file.read_text().splitlines()
    assert tool.main(flags + ["--length-scale", "2"]) == 0
    scaled, scaled_lines = json.loads(report_file.read_text()), profile_file.read_text().splitlines()
    assert plain["sources"]["vertices"] == 1 and plain["sources"]["region_vertices"] > 10 and plain["reached_share"] < 1.0
    assert scaled["farthest"]["distance"] == 2.0 * plain["farthest"]["distance"] <= 24.0 and scaled["rounds"] == plain["rounds"]
    for a, b in zip(plain_lines[1:], scaled_lines[1:]):
        a, b = a.split(","), b.split(",")
        assert float(b[3]) == 2.0 * float(a[3]) and float(b[4]) == 4.0 * float(a[4]) and a[5:] == b[5:]
