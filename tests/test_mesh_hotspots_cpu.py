"""What of the thermal hot spots needs no device: the host persistence (tn_basin_persistence) against the classical vertex sweep of
tests/mesh_hotspots_reference.py over 300 random triangle soups with heavy ties and NaN, the cases worked by hand (a chain of three
peaks, a batch in which one pass vertex joins three components, a plateau, the two bumps of the 5 x 5 lattice), the new entries in
header, Makefile, ctypes table and library, workspace sizes and the error codes returned before any launch, the refusals of the Python
layer, and the command line's arguments, ``--help`` and ``--length-scale``."""
from __future__ import annotations

import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_hotspots_reference as H
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (SADDLE_DTYPE, SPOT_BYTES, SPOT_DTYPE, BasinPersistence, ThermalHotspots, ThermalMesh, choose_spots,
                                    merge_basins, mesh_peaks, mesh_peaks_workspace_bytes, mesh_spots_workspace_bytes, prominence_of,
                                    regions_mesh, spot_bounds, thermal_hotspots)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_hotspots_tool", os.path.join(ROOT, "tools", "mesh_hotspots.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _saddles(rows):
    out = np.zeros(len(rows), SADDLE_DTYPE)
    for s, row in enumerate(rows):
        out[s] = row
    return out


# ---- the host persistence ---------------------------------------------------------------------------------------------------------------

def test_host_persistence_equals_the_vertex_sweep_on_300_random_soups():
    died = batches = 0
    for seed in range(300):
        temp, tri = H.soup(seed)
        for coldest in (False, True):
            found = H.peaks(temp, tri, coldest)
            basin_rank = found["rank"][found["basin_peak"]] if len(found["basin_peak"]) else np.zeros(0, np.int32)
            death, parent = merge_basins(basin_rank, found["saddles"])
            want_vertex, want_parent = H.sweep(found)
            got_vertex = np.where(death >= 0, found["saddles"]["pass_vertex"][np.maximum(death, 0)] if len(found["saddles"]) else -1, -1)
            assert got_vertex.tolist() == want_vertex.tolist(), (seed, coldest, "death vertices")
            assert parent.tolist() == want_parent.tolist(), (seed, coldest, "parents")
            yard_death, yard_parent = H.merge(basin_rank, found["saddles"])
            assert death.tolist() == yard_death.tolist() and parent.tolist() == yard_parent.tolist(), (seed, coldest, "the batches")
            died += int((death >= 0).sum())
            ranks = found["saddles"]["pass_rank"][death[death >= 0]]
            batches += len(ranks) - len(set(ranks.tolist()))
            assert ((death < 0) == (parent < 0)).all()
    assert died > 300 and batches > 20, "the soups exercise deaths and batches of several deaths at one pass vertex"


def test_chain_of_three_peaks_by_hand():
    # basins 0, 1, 2 with peak ranks 0, 1, 2; 1 - 2 meet at pass 5, 0 - 1 at pass 9: 2 dies into 1 at 5, then 1 into 0 at 9
    death, parent = merge_basins(np.array([0, 1, 2], np.int32), _saddles([(0, 1, 90, 9), (1, 2, 50, 5)]))
    assert death.tolist() == [-1, 0, 1] and parent.tolist() == [-1, 0, 1]
    # the passes the other way round: 1 dies into 0 first, and 2 then dies into the component's eldest, 0, not into 1
    death, parent = merge_basins(np.array([0, 1, 2], np.int32), _saddles([(0, 1, 50, 5), (1, 2, 90, 9)]))
    assert death.tolist() == [-1, 0, 1] and parent.tolist() == [-1, 0, 0]
    # the eldest is decided by the peak rank, not by the basin number
    death, parent = merge_basins(np.array([7, 3, 0], np.int32), _saddles([(0, 1, 50, 8), (1, 2, 90, 9)]))
    assert death.tolist() == [0, 1, -1] and parent.tolist() == [1, 2, -1]


def test_one_pass_vertex_joins_three_components_in_one_batch():
    # all three saddles at pass rank 6: within the batch in ascending (a, b).  (0, 1): 1 dies; (0, 2): 2 dies; (1, 2): already joined.
    # Peak ranks 2, 0, 1: basin 1 is the eldest.  (0, 1) kills 0 (rank 2 against 0); (0, 2): the components are {0, 1} led by 1 and
    # {2}: 2 dies; both get parent 1 after the batch
    death, parent = merge_basins(np.array([2, 0, 1], np.int32), _saddles([(0, 1, 60, 6), (0, 2, 60, 6), (1, 2, 60, 6)]))
    assert death.tolist() == [0, -1, 1] and parent.tolist() == [1, -1, 1]
    # peak ranks 1, 2, 0: (0, 1) kills 1 into 0, then (0, 2) kills 0 — the representative of {0, 1} — into 2; after the batch both
    # name the eldest of everything joined there, 2
    death, parent = merge_basins(np.array([1, 2, 0], np.int32), _saddles([(0, 1, 60, 6), (0, 2, 60, 6), (1, 2, 60, 6)]))
    assert death.tolist() == [1, 0, -1] and parent.tolist() == [2, 2, -1]


def test_plateau_by_hand_collapses_to_one_spot_at_zero_prominence():
    # a path 0 - 1 - 2 - 3 - 4 of triangles (i, i + 1, i + 1) at one temperature: ties go by index, every vertex climbs to its lower
    # neighbour: one basin.  With the numbering shuffled there are several peaks, all of prominence 0: one survivor
    temp = np.full(5, 21.5, F)
    tri = np.array([(0, 1, 1), (1, 2, 2), (2, 3, 3), (3, 4, 4)], np.int32)
    found = H.peaks(temp, tri)
    assert found["counts"].tolist() == [1, 0, 5] and found["vertex_basin"].tolist() == [0] * 5
    order = np.array([3, 0, 4, 1, 2])  # path vertex i is vertex order[i]
    shuffled = order[tri]
    got = H.hotspots(np.zeros((5, 3), F), temp, shuffled, 0.0)
    assert got["peaks"]["counts"].tolist() == [2, 1, 5], "vertices 0 and 1 have no lower-numbered neighbour"
    assert got["prominence"].tolist() == [math.inf, 0.0] and got["spot_basin"].tolist() == [0]
    assert got["basin_spot"].tolist() == [0, 0] and got["vertex_spot"].tolist() == [0] * 5
    p = BasinPersistence(got["peaks"]["basin_peak"], got["basin_rank"], temp[got["peaks"]["basin_peak"]], got["peaks"]["saddles"],
                         temp[got["peaks"]["saddles"]["pass_vertex"]], got["death_saddle"], got["parent"], got["prominence"])
    basin_spot, spot_basin = choose_spots(p, 0.0)
    assert basin_spot.tolist() == [0, 0] and spot_basin.tolist() == [0]
    assert choose_spots(p, math.inf)[1].tolist() == [] and choose_spots(p, math.inf)[0].tolist() == [-1, -1]


def test_two_bumps_of_the_lattice_by_hand():
    pos, temp, tri = H.two_bumps()
    got = H.hotspots(pos, temp, tri, 1.0)
    found = got["peaks"]
    assert found["basin_peak"].tolist() == [6, 18] and found["counts"].tolist() == [2, 1, 25]
    assert found["saddles"].tolist() == [(0, 1, 12, 2)], "the cell between the bumps, third in the order"
    assert got["death_saddle"].tolist() == [-1, 0] and got["parent"].tolist() == [-1, 0]
    assert got["prominence"].tolist() == [math.inf, 3.0]
    assert got["spot_limit"].tolist() == [H.NEVER, 2] and got["spots"]["label"].tolist() == [6, 18]
    assert got["vertex_spot"][18] == 1 and (got["vertex_spot"] == 1).sum() == 1, "only the peak lies above its saddle"
    assert got["spots"]["faces"][1] == 0 and got["spots"]["area"][1] == 0.0 and np.isnan(got["spots"]["mean_temperature"][1])
    assert got["spots"]["faces"][0] > 0 and got["spots"]["vertices"].tolist() == [int((got["vertex_spot"] == 0).sum()), 1]
    only = H.hotspots(pos, temp, tri, 3.0)  # strictly above: the second bump's 3 degrees do not survive 3
    assert only["spot_basin"].tolist() == [0] and only["basin_spot"].tolist() == [0, 0] and (only["vertex_spot"] == 0).all()
    near = H.hotspots(pos, temp, tri, 1.0, extent_drop=0.0)
    assert np.flatnonzero(near["vertex_spot"] >= 0).tolist() == [6, 18], "a drop of 0 keeps the peaks and their equals only"
    cold = H.hotspots(pos, -temp, tri, 1.0, coldest=True)
    for name in ("vertex_spot", "face_spot", "prominence", "basin_spot", "spot_limit"):
        assert cold[name].tolist() == got[name].tolist(), name
    assert prominence_of(temp[[6, 18]], temp[[12]], np.array([-1, 0], np.int32), False).tolist() == [math.inf, 3.0]
    assert prominence_of(-temp[[6, 18]], -temp[[12]], np.array([-1, 0], np.int32), True).tolist() == [math.inf, 3.0]
    assert spot_bounds(np.array([9.0], F), 2.5, False).tolist() == [6.5] and spot_bounds(np.array([9.0], F), 2.5, True).tolist() == [11.5]
    assert spot_bounds(np.array([9.0], F), math.inf, False).tolist() == [-math.inf]


# ---- the declarations ------------------------------------------------------------------------------------------------------------------

PEAKS = ("temperature", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "coldest", "rank", "vertex_basin", "basin_peak",
         "capacity_basins", "saddles", "capacity_saddles", "counts", "workspace", "workspace_bytes", "stream")
SPOTS = ("positions", "temperature", "triangles", "num_vertices", "num_triangles", "rank", "vertex_basin", "basin_spot", "num_basins",
         "spot_peak", "spot_limit", "spot_bound", "num_spots", "coldest", "vertex_spot", "face_spot", "spots", "counts", "workspace",
         "workspace_bytes", "stream")


def test_entries_structs_and_makefile_are_declared():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    for name, names in (("tn_mesh_peaks", PEAKS), ("tn_mesh_spots", SPOTS)):
        declared = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert [re.search(r"(\w+)$", a.strip()).group(1) for a in declared.split(",")] == list(names), name
        assert len(_hip.SIGNATURES[name][1]) == len(names), name
    assert re.search(r"\bsize_t tn_mesh_peaks_workspace_bytes\(int64_t num_vertices, int64_t num_triangles\);", header)
    assert re.search(r"\bsize_t tn_mesh_spots_workspace_bytes\(int64_t num_vertices, int64_t num_triangles, int64_t num_spots\);", header)
    assert re.search(r"\bint tn_basin_persistence\(const int32_t \*basin_rank, int64_t num_basins, const tn_mesh_saddle \*saddles", header)
    assert len(_hip.SIGNATURES["tn_basin_persistence"][1]) == 6 and len(_hip.SIGNATURES["tn_mesh_spots_workspace_bytes"][1]) == 3
    lib = _hip.load()
    for name in ("tn_mesh_peaks", "tn_mesh_peaks_workspace_bytes", "tn_basin_persistence", "tn_mesh_spots", "tn_mesh_spots_workspace_bytes"):
        assert hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert "tn_mesh_hotspots.hip" in makefile and "tn_persistence.h" in makefile
    for struct, dtype in (("tn_mesh_saddle", SADDLE_DTYPE), ("tn_mesh_spot", SPOT_DTYPE)):
        body = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (struct, struct), header).group(1)
        assert re.findall(r"\b([a-z_]+)(?:\[\d\])?(?=[,;])", body) == list(dtype.names), struct
    assert SADDLE_DTYPE.itemsize == 16 == H.SADDLE_DTYPE.itemsize and SPOT_DTYPE.itemsize == 80 == SPOT_BYTES == H.SPOT_DTYPE.itemsize
    assert [SPOT_DTYPE.fields[n][1] for n in SPOT_DTYPE.names] == [H.SPOT_DTYPE.fields[n][1] for n in SPOT_DTYPE.names]
    assert SPOT_DTYPE.fields["vertices"][1] == 72 and SPOT_DTYPE.names[:10] == H.R.REGION_DTYPE.names
    # the persistence is a header of its own without a device in it, and the new source restates neither the face nor the sums
    persistence = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_persistence.h")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)", persistence) == ["algorithm", "cstdint", "new", "vector"]
    assert "__global__" not in persistence and "__device__" not in persistence and "malloc" not in persistence
    source = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_mesh_hotspots.hip")).read()
    assert '#include "tn_group_sum.h"' in source and "load_face(" in source and "group_sum(" in source
    assert "__dsqrt_rn" not in source and "Face load_face" not in source and "block_sums_kernel" not in source


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _hip.load()
    v, t, k = 1000, 2000, 7
    limit = (2 ** 31 - 1) // 3
    need = mesh_peaks_workspace_bytes(v, t)
    assert need > 0 and need % 8 == 0 and mesh_peaks_workspace_bytes(2 ** 31 - 1, limit) > 0 and mesh_peaks_workspace_bytes(v, 0) > 0
    for bad in ((-1, t), (v, -1), (2 ** 31, t), (v, limit + 1)):
        assert mesh_peaks_workspace_bytes(*bad) == 0 and mesh_spots_workspace_bytes(*bad, 1) == 0, bad
    assert mesh_peaks_workspace_bytes(v, 2 * t) > need
    dummy = 4096  # a non-null address: nothing is dereferenced, allocated or launched
    good = dict(zip(PEAKS, [dummy, dummy, t, v, dummy, dummy, 0, dummy, dummy, dummy, 10, dummy, 10, dummy, dummy, need, None]))

    def peaks(**change):
        args = dict(good, **change)
        return lib.tn_mesh_peaks(*[args[n] for n in PEAKS])

    for n in ("temperature", "triangles", "offsets", "corners", "rank", "vertex_basin", "basin_peak", "saddles", "counts", "workspace"):
        assert peaks(**{n: None}, workspace_bytes=0) == -1, n
    assert peaks(num_vertices=-1) == -2 and peaks(num_vertices=2 ** 31) == -2 and peaks(num_triangles=-1) == -2
    assert peaks(num_triangles=limit + 1, workspace_bytes=2 ** 60) == -2 and peaks(capacity_basins=-1) == -2 and peaks(capacity_saddles=-1) == -2
    for n in ("temperature", "triangles", "offsets", "corners", "rank", "vertex_basin", "basin_peak", "saddles"):
        assert peaks(**{n: dummy + 2}) == -2, n
    assert peaks(counts=dummy + 4) == -2 and peaks(workspace=dummy + 4) == -2
    assert peaks(workspace_bytes=need - 1) == -4 and peaks(workspace_bytes=0) == -4
    assert peaks(basin_peak=None, capacity_basins=0, saddles=None, capacity_saddles=0, workspace_bytes=0) == -4, "the sizing call"
    assert peaks(counts=None, num_vertices=-1) == -1 and peaks(num_vertices=-1, rank=None) == -2, "in the order of the code"

    need = mesh_spots_workspace_bytes(v, t, k)
    assert need > 0 and need % 8 == 0 and mesh_spots_workspace_bytes(v, t, 0) > 0 and mesh_spots_workspace_bytes(v, t, v) > need
    assert mesh_spots_workspace_bytes(v, t, -1) == 0 and mesh_spots_workspace_bytes(v, t, v + 1) == 0
    good_spots = dict(zip(SPOTS, [dummy, dummy, dummy, v, t, dummy, dummy, dummy, 20, dummy, dummy, dummy, k, 0, dummy, dummy, dummy, dummy,
                                  dummy, need, None]))

    def spots(**change):
        args = dict(good_spots, **change)
        return lib.tn_mesh_spots(*[args[n] for n in SPOTS])

    for n in SPOTS:
        if good_spots[n] == dummy:
            assert spots(**{n: None}, workspace_bytes=0) == -1, n
    assert spots(num_vertices=-1) == -2 and spots(num_triangles=limit + 1) == -2
    assert spots(num_basins=-1) == -2 and spots(num_basins=v + 1) == -2 and spots(num_spots=-1) == -2 and spots(num_spots=21) == -2
    for n in SPOTS:
        if good_spots[n] == dummy:
            assert spots(**{n: dummy + (4 if n in ("spots", "counts", "workspace") else 2)}) == -2, n
    assert spots(workspace_bytes=need - 1) == -4 and spots(workspace_bytes=0) == -4
    assert spots(num_spots=0, spot_peak=None, spot_limit=None, spot_bound=None, spots=None, workspace_bytes=0) == -4

    def merge(rank, b, rows, s, death, parent):
        return lib.tn_basin_persistence(rank, b, rows, s, death, parent)

    assert merge(None, 0, None, 0, None, None) == 0, "nothing to do"
    assert merge(None, 1, None, 0, dummy, dummy) == -1 and merge(dummy, 1, None, 1, dummy, dummy) == -1
    assert merge(dummy, -1, None, 0, dummy, dummy) == -2 and merge(dummy, 2 ** 31, None, 0, dummy, dummy) == -2
    assert merge(dummy + 2, 1, None, 0, dummy, dummy) == -2
    rank = np.array([0, 1], np.int32)
    for row in ((0, 2, 5, 5), (-1, 1, 5, 5), (1, 1, 5, 5)):
        death, parent = np.full(2, 77, np.int32), np.full(2, 77, np.int32)
        rows = np.array([row], np.int32)
        assert merge(rank.ctypes.data, 2, rows.ctypes.data, 1, death.ctypes.data, parent.ctypes.data) == -3, row
        assert death.tolist() == [77, 77] and parent.tolist() == [77, 77], "nothing is written"
    with pytest.raises(RuntimeError, match="tn_basin_persistence"):
        merge_basins(rank, _saddles([(0, 5, 1, 1)]))
    assert [a.tolist() for a in merge_basins(np.zeros(0, np.int32), _saddles([]))] == [[], []]
    assert [a.tolist() for a in merge_basins(np.array([4, 2], np.int32), np.array([[0, 1, 9, 3]], np.int32))] == [[0, -1], [1, -1]]


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def test_python_layer_refuses_before_it_reaches_a_kernel():
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    bare = ThermalMesh(pos, mesh.colors, mesh.temperature)
    with pytest.raises(ValueError, match="no triangles"):
        thermal_hotspots(bare, 1.0)
    with pytest.raises(ValueError, match="no triangles"):
        mesh_peaks(bare)
    for bad in (dict(min_prominence=-1.0), dict(min_prominence=float("nan")), dict(min_prominence=1.0, extent_drop=-0.5),
                dict(min_prominence=1.0, extent_drop=float("nan")), dict(min_prominence=1.0, smooth_iterations=-1),
                dict(min_prominence=1.0, min_area=-1.0), dict(min_prominence=1.0, min_area=float("nan")), dict(min_prominence=1.0, top=-2)):
        with pytest.raises(ValueError):
            thermal_hotspots(mesh, **bad)
    for call in (lambda: thermal_hotspots(mesh, 1.0), lambda: mesh_peaks(mesh), lambda: thermal_hotspots(mesh, 1.0, smooth_iterations=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def _fake():
    table = np.zeros(2, SPOT_DTYPE)
    table[0] = (1.0, 3, 2, 24.0, 23.0, 25.0, (0.5, 0.5, 0.0), (0, 0, 0, 1, 1, 0), 0, 3, 4, 0)
    table[1]["label"], table[1]["vertices"] = 1, 1
    for name in ("mean_temperature", "min_temperature", "max_temperature", "centroid", "bounds"):
        table[1][name] = np.nan
    table[1]["hottest_vertex"] = table[1]["coldest_vertex"] = -1
    return ThermalHotspots(np.array([3, 1], np.int32), np.array([(0, 1, 0), (1, 0, 0)], F), np.array([29.0, 23.0], F),
                           np.array([np.inf, 1.5], F), np.array([-1, 2], np.int32), np.array([np.nan, 21.5], F), np.array([3, 1]),
                           np.array([True, False]), table, np.array([0, 2], np.int64), torch.tensor([0, 2, 0, 0, -1], dtype=torch.int32),
                           torch.tensor([0, 0, -1], dtype=torch.int32), 5, 6, 3, 1.0, False)


def test_result_reads_as_regions_for_regions_mesh():
    found = _fake()
    assert len(found) == 2 and found.num_regions == 3 and found.region_index.tolist() == [0, 2] and found.face_region is found.face_spot
    v = 5
    pos = torch.arange(3 * v, dtype=torch.float32).reshape(v, 3)
    mesh = ThermalMesh(pos, torch.zeros((v, 3), dtype=torch.uint8), torch.arange(v, dtype=torch.float32), None,
                       torch.tensor([[0, 2, 3], [0, 3, 2], [1, 2, 4]], dtype=torch.int32))
    part = regions_mesh(mesh, found)
    assert part.triangles.tolist() == [[0, 1, 2], [0, 2, 1]] and part.temperature.tolist() == [0.0, 2.0, 3.0]


# ---- the command line -------------------------------------------------------------------------------------------------------------------

FLAGS = ("--min-prominence", "--coldest", "--extent-drop", "--smooth-iterations", "--min-area", "--top", "--length-scale", "--report",
         "--output", "--colors")


def test_command_line_arguments(capsys):
    tool = _tool()
    base = ["mesh.ply", "--report", "r.json"]
    args = tool.parse(base + ["--min-prominence", "1.5"])
    assert (args.min_prominence, args.coldest, args.extent_drop, args.smooth_iterations, args.min_area, args.top, args.length_scale) == \
        (1.5, False, math.inf, 0, 0.0, None, 1.0) and args.output is None and args.colors == "rgb"
    args = tool.parse(base + ["--min-prominence", "0", "--coldest", "--extent-drop", "2", "--smooth-iterations", "3", "--min-area", "0.5",
                              "--top", "4", "--length-scale", "2.5", "--output", "o.ply", "--colors", "thermal"])
    assert (args.min_prominence, args.coldest, args.extent_drop, args.smooth_iterations, args.min_area, args.top, args.length_scale) == \
        (0.0, True, 2.0, 3, 0.5, 4, 2.5)
    ok = ["--min-prominence", "1"]
    for bad, flag in (([], "--min-prominence"), (["--min-prominence=nan"], "--min-prominence"), (["--min-prominence=-1"], "--min-prominence"),
                      (ok + ["--extent-drop=-1"], "--extent-drop"), (ok + ["--extent-drop=nan"], "--extent-drop"),
                      (ok + ["--smooth-iterations=-1"], "--smooth-iterations"), (ok + ["--min-area=-1"], "--min-area"),
                      (ok + ["--top=-1"], "--top"), (ok + ["--length-scale", "0"], "--length-scale"),
                      (ok + ["--length-scale", "inf"], "--length-scale"), (ok + ["--colors", "x"], "--colors")):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
        assert flag in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        tool.parse(["mesh.ply"] + ok)  # no --report
    assert "--report" in capsys.readouterr().err
    for flag in FLAGS:
        assert flag in tool.__doc__, flag


def test_command_line_help_names_every_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_hotspots.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in FLAGS:
        assert flag in out.stdout, flag


def test_report_schema_and_length_scale_with_a_fake_result():
    tool = _tool()
    found = _fake()
    plain = tool.build_report(found, 5, 3, math.inf, 2, 1.0, "mesh.ply")
    assert json.loads(json.dumps(plain, allow_nan=False)) == plain, "plain JSON: no numpy scalars, no infinities, no NaN"
    assert set(plain) == {"mesh", "length_scale", "coldest", "min_prominence", "extent_drop", "smooth_iterations", "counts", "spots"}
    assert plain["counts"] == {"vertices": 5, "faces": 3, "basins": 5, "saddles": 6, "spots": 3, "reported_spots": 2}
    assert (plain["extent_drop"], plain["smooth_iterations"], plain["coldest"], plain["min_prominence"]) == (None, 2, False, 1.0)
    first, second = plain["spots"]
    assert first == {"spot": 0, "peak": {"index": 3, "position": [0.0, 1.0, 0.0], "temperature": 29.0}, "prominence": None, "saddle": None,
                     "component_extreme": True, "basins": 3, "vertices": 4, "faces": 2, "area": 1.0, "mean_temperature": 24.0,
                     "min_temperature": 23.0, "max_temperature": 25.0, "centroid": [0.5, 0.5, 0.0],
                     "bounds": {"min": [0.0, 0.0, 0.0], "max": [1.0, 1.0, 0.0]}}
    assert second["spot"] == 2 and second["prominence"] == 1.5 and second["saddle"] == {"index": 2, "temperature": 21.5}
    assert second["mean_temperature"] is None and second["centroid"] == [None, None, None] and second["area"] == 0.0
    scaled = tool.build_report(found, 5, 3, 2.0, 0, 2.0, "mesh.ply")
    s = scaled["spots"][0]
    assert scaled["length_scale"] == 2.0 and scaled["extent_drop"] == 2.0, "degrees are not lengths"
    assert s["area"] == 4.0 and s["centroid"] == [1.0, 1.0, 0.0] and s["bounds"]["max"] == [2.0, 2.0, 0.0]
    assert s["peak"] == {"index": 3, "position": [0.0, 2.0, 0.0], "temperature": 29.0}
    for name in ("mean_temperature", "min_temperature", "max_temperature", "faces", "vertices", "prominence", "basins"):
        assert s[name] == first[name], name
    assert scaled["spots"][1]["prominence"] == 1.5 and scaled["spots"][1]["saddle"] == second["saddle"]
    lines = tool.spot_lines(plain)
    assert len(lines) == 2 and lines[0].startswith("spot 0: peak 29.00 C at vertex 3") and "the extreme of its component" in lines[0]
    assert "prominence 1.50 C over the saddle at vertex 2 (21.50 C)" in lines[1] and "no whole face" in lines[1]
