"""The geodesic layer without a device: the two forms of the yardstick against each other, the method against what is known (the
Euclidean distance on a plane, the path around a slit), the declarations, every error code the entries return before a launch, the
Python layer's refusals and the command line."""
from __future__ import annotations

import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_geodesic_reference as G
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (BAND_BYTES, BAND_DTYPE, DistanceProfile, ThermalMesh, distance_profile, geodesic_distance,
                                    mesh_distance_bands_workspace_bytes, mesh_geodesic_workspace_bytes, seeds_of_regions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
GEODESIC = ("positions", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "seed_vertex", "seed_offset", "num_seeds",
            "max_distance", "restart", "rounds", "distance", "nearest_seed", "counts", "workspace", "workspace_bytes",
            "stream")
BANDS = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "distance", "nearest_seed", "width", "bands", "cell",
         "rows", "counts", "workspace", "workspace_bytes", "stream")


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_distance_tool", os.path.join(ROOT, "tools", "mesh_distance.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------

def test_the_two_forms_of_the_yardstick_agree_to_the_bit_on_300_soups():
    reached, limited, doubled, outside = 0, 0, 0, 0
    for seed in range(300):
        pos, tri, seeds, offsets, limit = G.soup(seed)
        fast = G.solve(pos, tri, seeds, offsets, limit)
        slow = G.solve(pos, tri, seeds, offsets, limit, scalar=True)
        assert fast["distance"].tobytes() == slow["distance"].tobytes(), seed
        assert fast["nearest_seed"].tobytes() == slow["nearest_seed"].tobytes(), seed
        assert (fast["rounds"], fast["converged"]) == (slow["rounds"], True), seed
        assert ((fast["nearest_seed"] >= 0) == np.isfinite(fast["distance"])).all()
        reached += int(np.isfinite(fast["distance"]).sum() > 3)
        limited += int(math.isfinite(limit))
        doubled += int(seeds[0] == seeds[1])
        outside += int(seeds[1] >= len(pos))
    assert reached > 200 and limited == 150 and doubled >= 50 and outside >= 40, "the soups cover what they are meant to"


@pytest.mark.parametrize("pattern", ["same", "alternating"])
def test_the_flat_lattice_gives_the_euclidean_distance(pattern):
    pos, tri = G.lattice(129, 129, pattern)
    centre = 64 * 129 + 64
    got = G.solve(pos, tri, [centre])
    euclid = np.linalg.norm(pos.astype(D) - pos[centre].astype(D), axis=1)
    away = euclid > 0.0
    assert got["converged"] and np.abs(got["distance"][away] / euclid[away] - 1.0).max() < 1e-12
    assert got["rounds"] <= 129, "about the edge hops to the farthest vertex"
    # to vertex (0, 128), across the "same" pattern's diagonals, the shortest path over the edges has 64 + 64 unit edges: 41 % too
    # long, which is what the method must not be
    far = 128
    assert euclid[far] == 64.0 * math.sqrt(2.0) and abs(got["distance"][far] / euclid[far] - 1.0) < 1e-12 and 128.0 / euclid[far] > 1.41


def test_a_seed_inside_a_face_is_exact_through_the_offsets():
    pos, tri = G.lattice(129, 129)
    point = np.array([64.3, 64.2, 0.0])  # inside the face (64, 64), (65, 64), (65, 65)
    face = np.array([64 * 129 + 64, 65 * 129 + 64, 65 * 129 + 65])
    offsets = np.linalg.norm(pos[face].astype(D) - point, axis=1)
    got = G.solve(pos, tri, face, offsets)
    euclid = np.linalg.norm(pos.astype(D) - point, axis=1)
    assert np.abs(got["distance"] / euclid - 1.0).max() < 1e-12


def test_the_path_around_the_end_of_the_slit():
    pos, tri = G.slit_lattice()
    seed, goal = 16 * 65 + 16, 16 * 65 + 49            # (16, 16) and (16, 49): the slit lies between the rows y = 32 and y = 33
    got = G.solve(pos, tri, [seed])
    around = 2.0 * math.hypot(32.0, 16.0) + 1.0        # to the slit's end at (48, 32), across it, back
    straight = 33.0
    assert around < got["distance"][goal] < 1.01 * around and straight < 0.5 * around
    whole = G.solve(*G.lattice(65, 65), [seed])
    assert abs(whole["distance"][goal] - straight) < 1e-12, "without the slit it is the straight line"


def test_bands_of_the_yardstick_by_hand():
    pos, tri = G.lattice(5, 5)
    rows, counts, face_band = G.bands(pos, (20.0 + 2.0 * pos[:, 0]).astype(F), tri, pos[:, 0].astype(D), np.zeros(25, np.int32), 1.0, 6)
    assert rows["faces"].tolist() == [8, 8, 8, 8, 0, 0] and rows["area"].tolist() == [4.0, 4.0, 4.0, 4.0, 0.0, 0.0]
    assert rows["mean_temperature"][:4].tolist() == [21.0, 23.0, 25.0, 27.0] and counts.tolist() == [4, 32, 32]
    assert face_band.tolist() == np.repeat(np.arange(4), 8).tolist() and rows.dtype == BAND_DTYPE and BAND_DTYPE.itemsize == 40


# ---- the declarations -------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_built_and_bound():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    for name, names in (("tn_mesh_geodesic", GEODESIC), ("tn_mesh_distance_bands", BANDS)):
        body = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert re.findall(r"(\w+)(?=,|$)", body.replace("\n", " ")) == list(names), name
        assert len(_hip.SIGNATURES[name][1]) == len(names), name
    assert re.search(r"\bsize_t tn_mesh_geodesic_workspace_bytes\(int64_t num_vertices, int64_t num_triangles\);", header)
    assert re.search(r"\bsize_t tn_mesh_distance_bands_workspace_bytes\(int64_t num_vertices, int64_t num_triangles, int64_t bands\);", header)
    lib = _hip.load()
    for name in ("tn_mesh_geodesic", "tn_mesh_geodesic_workspace_bytes", "tn_mesh_distance_bands", "tn_mesh_distance_bands_workspace_bytes"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES, name
    assert "tn_mesh_geodesic.hip" in open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    body = re.search(r"typedef struct tn_mesh_band \{([^}]*)\} tn_mesh_band;", header).group(1)
    assert re.findall(r"\b([a-z_]+)(?=[,;])", body) == list(BAND_DTYPE.names)
    assert BAND_BYTES == 40 == G.BAND_DTYPE.itemsize and BAND_DTYPE == G.BAND_DTYPE


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _hip.load()
    v, t = 1000, 2000
    limit = (2 ** 31 - 1) // 3
    need = mesh_geodesic_workspace_bytes(v, t)
    assert need > 0 and need % 8 == 0 and mesh_geodesic_workspace_bytes(2 ** 31 - 1, limit) > 0 and mesh_geodesic_workspace_bytes(v, 0) == need
    assert mesh_geodesic_workspace_bytes(2 * v, t) > need and mesh_geodesic_workspace_bytes(0, 0) > 0
    for bad in ((-1, t), (v, -1), (2 ** 31, t), (v, limit + 1)):
        assert mesh_geodesic_workspace_bytes(*bad) == 0 and mesh_distance_bands_workspace_bytes(*bad, 4) == 0, bad
    dummy = 4096  # a non-null address: nothing is dereferenced, allocated or launched
    good = dict(zip(GEODESIC, [dummy, dummy, t, v, dummy, dummy, dummy, dummy, 3, math.inf, 1, 10, dummy, dummy, dummy, dummy, need, None]))

    def solve(**change):
        args = dict(good, **change)
        return lib.tn_mesh_geodesic(*[args[n] for n in GEODESIC])

    for n in GEODESIC:
        if good[n] == dummy:
            assert solve(**{n: None}, workspace_bytes=0) == -1, n
    assert solve(seed_vertex=None, seed_offset=None, num_seeds=0, workspace_bytes=0) == -4, "no seeds: the pointers are not needed"
    assert solve(seed_vertex=None, seed_offset=None, restart=0, workspace_bytes=0) == -4, "nor without a restart"
    assert solve(triangles=None, corners=None, num_triangles=0, workspace_bytes=0) == -4
    assert solve(num_vertices=-1) == -2 and solve(num_vertices=2 ** 31) == -2 and solve(num_triangles=-1) == -2
    assert solve(num_triangles=limit + 1, workspace_bytes=2 ** 60) == -2
    assert solve(num_seeds=-1) == -2 and solve(num_seeds=2 ** 31) == -2
    assert solve(max_distance=-1.0) == -2 and solve(max_distance=math.nan) == -2 and solve(max_distance=0.0, workspace_bytes=0) == -4
    assert solve(rounds=-1) == -2 and solve(rounds=4097) == -2 and solve(rounds=4096, workspace_bytes=0) == -4
    for n in ("positions", "triangles", "offsets", "corners", "seed_vertex", "nearest_seed"):
        assert solve(**{n: dummy + 2}) == -2, n
    for n in ("distance", "seed_offset", "counts", "workspace"):
        assert solve(**{n: dummy + 4}) == -2, n
    assert solve(workspace_bytes=need - 1) == -4 and solve(workspace_bytes=0) == -4
    assert solve(positions=None, num_triangles=-1) == -1 and solve(rounds=-1, nearest_seed=None) == -1, "in the order of the code"
    assert solve(num_vertices=0, positions=None, offsets=None, distance=None, nearest_seed=None, counts=None, workspace=None,
                 workspace_bytes=0) == 0, "no vertex: nothing to do"

    k = 64
    need = mesh_distance_bands_workspace_bytes(v, t, k)
    assert need > 0 and need % 8 == 0 and mesh_distance_bands_workspace_bytes(v, t, 4096) > need
    assert mesh_distance_bands_workspace_bytes(v, t, 0) == 0 and mesh_distance_bands_workspace_bytes(v, t, 4097) == 0
    good_bands = dict(zip(BANDS, [dummy, dummy, dummy, v, t, dummy, dummy, 0.5, k, -1, dummy, dummy, dummy, need, None]))

    def bands(**change):
        args = dict(good_bands, **change)
        return lib.tn_mesh_distance_bands(*[args[n] for n in BANDS])

    for n in BANDS:
        if good_bands[n] == dummy:
            assert bands(**{n: None}, workspace_bytes=0) == -1, n
    assert bands(num_vertices=-1) == -2 and bands(num_triangles=limit + 1) == -2 and bands(bands=0) == -2 and bands(bands=4097) == -2
    assert bands(width=0.0) == -2 and bands(width=-1.0) == -2 and bands(width=math.nan) == -2 and bands(width=math.inf) == -2
    assert bands(cell=-2) == -2 and bands(cell=5, workspace_bytes=0) == -4
    for n in BANDS:
        if good_bands[n] == dummy:
            assert bands(**{n: dummy + (4 if n in ("distance", "rows", "counts", "workspace") else 2)}) == -2, n
    assert bands(workspace_bytes=need - 1) == -4 and bands(workspace_bytes=0) == -4
    assert bands(rows=None, bands=0) == -1, "in the order of the code"


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def test_python_layer_refuses_before_it_reaches_a_kernel():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    bare = ThermalMesh(pos, mesh.colors, mesh.temperature)
    with pytest.raises(ValueError, match="no triangles"):
        geodesic_distance(bare, [0])
    with pytest.raises(ValueError, match="no triangles"):
        seeds_of_regions(bare, None)
    for bad in (dict(seed_vertices=[0], max_distance=-1.0), dict(seed_vertices=[0], max_distance=math.nan),
                dict(seed_vertices=[0], max_rounds=-1), dict(seed_vertices=[]), dict(seed_vertices=[0.5]), dict(seed_vertices=[-1]),
                dict(seed_vertices=[0, 1], seed_offsets=[0.0]), dict(seed_vertices=[0], seed_offsets=[-0.5]),
                dict(seed_vertices=[0], seed_offsets=[math.nan]), dict(seed_vertices=[0], seed_offsets=[math.inf])):
        with pytest.raises(ValueError):
            geodesic_distance(mesh, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geodesic_distance(mesh, [0])
    d = None
    for bad in ((0.0, 4), (-1.0, 4), (math.nan, 4), (math.inf, 4), (1.0, 0), (1.0, 4097)):
        with pytest.raises(ValueError):
            distance_profile(mesh, d, *bad)
    with pytest.raises(ValueError, match="cell"):
        distance_profile(mesh, d, 1.0, 4, cell=-1)
    with pytest.raises(ValueError, match="k must be"):
        seeds_of_regions(mesh, None, -1)
    with pytest.raises(ValueError, match="face_region"):
        seeds_of_regions(mesh, object())
    profile = DistanceProfile(np.zeros(3, BAND_DTYPE), np.array([0.5, 1.5, 2.5]), np.zeros(3), 1.0, None, 0, 0)
    assert len(profile) == 3


# ---- the command line -------------------------------------------------------------------------------------------------------------------

FLAGS = ("--from-vertex", "--from-point", "--from-hotspots", "--top", "--coldest", "--from-min-temperature", "--from-max-temperature",
         "--max-distance", "--to-point", "--band-width", "--bands", "--length-scale", "--output", "--profile", "--report")


def test_command_line_arguments(capsys):
    tool = _tool()
    args = tool.parse(["mesh.ply", "--from-vertex", "3", "9"])
    assert (args.from_vertex, args.from_point, args.from_hotspots, args.max_distance, args.bands, args.length_scale) == \
        ([3, 9], [], None, math.inf, None, 1.0) and args.report is None and args.output is None and args.to_point is None
    args = tool.parse(["mesh.ply", "--from-point", "1", "2", "3", "--from-point", "4", "5", "6", "--from-hotspots", "0.5", "--top", "2",
                       "--coldest", "--from-min-temperature", "25", "--max-distance", "3", "--to-point", "0", "0", "1", "--band-width", "0.1",
                       "--bands", "20", "--length-scale", "0.37", "--profile", "p.csv", "--report", "r.json", "--output", "o.ply"])
    assert args.from_point == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]] and (args.from_hotspots, args.top, args.coldest) == (0.5, 2, True)
    assert (args.from_min_temperature, args.from_max_temperature, args.max_distance, args.to_point) == (25.0, None, 3.0, [0.0, 0.0, 1.0])
    assert (args.band_width, args.bands, args.length_scale) == (0.1, 20, 0.37)
    ok = ["--from-vertex", "0"]
    for bad, word in (([], "at least one source"), (["--from-vertex=-1"], "--from-vertex"), (["--from-hotspots=-1"], "--from-hotspots"),
                      (["--from-hotspots=nan"], "--from-hotspots"), (ok + ["--top", "2"], "--top"),
                      (["--from-hotspots", "1", "--top", "0"], "--top"), (ok + ["--coldest"], "--coldest"),
                      (["--from-min-temperature=nan"], "--from-min-temperature"), (ok + ["--max-distance=-1"], "--max-distance"),
                      (ok + ["--max-distance=nan"], "--max-distance"), (ok + ["--band-width", "1"], "go together"),
                      (ok + ["--bands", "4"], "go together"), (ok + ["--band-width", "0", "--bands", "4"], "--band-width"),
                      (ok + ["--band-width", "1", "--bands", "0"], "--bands"), (ok + ["--band-width", "1", "--bands", "4097"], "--bands"),
                      (ok + ["--profile", "p.csv"], "--profile"), (ok + ["--length-scale", "0"], "--length-scale"),
                      (ok + ["--length-scale", "inf"], "--length-scale"), (ok + ["--to-point", "1", "2"], "--to-point")):
        with pytest.raises(SystemExit):
            tool.parse(["mesh.ply"] + bad)
        assert word in capsys.readouterr().err, bad
    for flag in FLAGS:
        assert flag in tool.__doc__, flag


def test_command_line_help_names_every_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_distance.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in FLAGS:
        assert flag in out.stdout, flag


def test_profile_rows_and_length_scale():
    tool = _tool()
    table = np.zeros(2, BAND_DTYPE)
    table[0] = (2.0, 1.5, 24.0, 23.0, 25.0, 4, 3, 0)
    table[1]["mean_temperature"] = table[1]["min_temperature"] = table[1]["max_temperature"] = np.nan
    profile = DistanceProfile(table, np.array([0.25, 0.75]), np.array([2.0, 2.0]), 0.5, None, 4, 4)
    plain, scaled = tool.profile_rows(profile, -1), tool.profile_rows(profile, 3, 2.0)
    assert plain[0] == {"seed": -1, "band": 0, "from": 0.0, "to": 0.5, "area": 2.0, "mean_temperature": 24.0, "min_temperature": 23.0,
                        "max_temperature": 25.0}
    assert plain[1]["mean_temperature"] is None and plain[1]["area"] == 0.0 and (plain[1]["from"], plain[1]["to"]) == (0.5, 1.0)
    assert scaled[0]["seed"] == 3 and (scaled[0]["to"], scaled[0]["area"], scaled[0]["mean_temperature"]) == (1.0, 8.0, 24.0)
    assert (scaled[1]["from"], scaled[1]["to"]) == (1.0, 2.0), "lengths times L, areas times L^2, degrees as they are"


def test_profile_csv(tmp_path, capsys):
    tool = _tool()
    table = np.zeros(2, BAND_DTYPE)
    table[0] = (2.0, 1.5, 24.0, 23.0, 25.0, 4, 3, 0)
    table[1]["mean_temperature"] = table[1]["min_temperature"] = table[1]["max_temperature"] = np.nan
    profile = DistanceProfile(table, np.array([0.25, 0.75]), np.array([2.0, 2.0]), 0.5, None, 4, 4)
    path = tmp_path / "deep" / "profile.csv"
    tool.write_profile(path, tool.profile_rows(profile, -1))
    assert path.read_text().splitlines() == ["seed,band,from,to,area,mean_temperature,min_temperature,max_temperature",
                                             "-1,0,0.0,0.5,2.0,24.0,23.0,25.0", "-1,1,0.5,1.0,0.0,,,"]
    assert "2 bands" in capsys.readouterr().out
