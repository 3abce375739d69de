#!/usr/bin/env python
"""What the thermal hot spots cost on a mesh of a survey's size, part by part, beside ``tn_mesh_regions`` on the same mesh for scale:
the closed lattice surface of about 2 M faces of tools/mesh_isolines_bench.py (a torus of ``--side`` x ``--side`` two-triangle cells;
no file, no reference data) with a smooth field of several bumps — and, as the other extreme, with the per-vertex noise of an
unsmoothed surface-nets mesh on top, where every few vertices are a peak.

The entries are timed into preallocated outputs with device events around each call (3 warm-up calls, then ``--repeats`` timed calls:
median and range), the two sorts of ``tn_mesh_peaks`` as ``tn_sort_pairs`` calls of the same sizes and key widths, the host merge
with the host's clock, the public call beside them with its allocations, the incidence build and its host reads.  The times of the
single kernels — the ascent, the jumps, the saddles, the spots — come from a kernel trace taken in a run of its own, in which only the
two device entries run (the set-up's single ``mesh_peaks`` call and incidence build are in it too):

    python tools/mesh_hotspots_bench.py [--side 1024] [--repeats 11] --out profiles/micro/mesh_hotspots.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_hotspots_bench.py --trace-pass
    python tools/mesh_hotspots_bench.py --kernels-from DIR --out profiles/micro/mesh_hotspots.txt      # appends the kernels

A record, not a gate.
"""
from __future__ import annotations

import argparse
import glob
import math
import os
import sqlite3
import sys
import time

import mesh_scenes  # the sibling module: event_ms, emit; it puts the repository on sys.path
from mesh_isolines_bench import torus  # the sibling module: the closed lattice surface

# the kernels of the traced calls, under the names a trace gives them: what they are; the launches per traced round come from the trace
KERNELS = (("rank_keys_kernel", "peaks: the rank keys"), ("ranks_kernel", "peaks: rank[v] from the sorted order"),
           ("ascent_kernel", "peaks: the ascent, one thread per vertex"), ("jump_kernel", "peaks: one pointer jump"),
           ("count_peaks_kernel", "peaks: basins, count"), ("emit_peaks_kernel", "peaks: basins, emit"),
           ("basins_kernel", "peaks: vertex_basin"), ("edge_keys_kernel", "peaks: the half-edge keys"),
           ("count_pairs_kernel", "peaks: saddles, count"), ("emit_saddles_kernel", "peaks: saddles, emit and walk"),
           ("spot_vertices_kernel", "spots: the extents"), ("spot_faces_kernel", "spots: the faces"),
           ("spot_assign_kernel", "spots: the block heads"), ("block_sums_kernel<Acc>", "spots: the 256-blocks"),
           ("spot_rows_kernel", "spots: the rows"), ("histogram_kernel", "the sorts: histogram"), ("scan_kernel", "the sorts: scan"),
           ("scatter_kernel<false>", "the sorts: scatter"), ("scatter_kernel<true>", "the sorts: scatter, the values 0 .. n-1"))


def short_name(name: str) -> str:
    """a traced kernel name without its namespace, return type and arguments"""
    name = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()
    return name.replace("tn::", "")


def kernel_us(directory: str) -> dict:
    """{kernel: (us in all its launches, launches)} from the rocpd database(s) of a kernel trace under ``directory``"""
    spent = {}
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        for name, calls, duration in sqlite3.connect(path).cursor().execute("select name,total_calls,total_duration from top_kernels"):
            short = short_name(name)
            before = spent.get(short, (0.0, 0))
            spent[short] = (before[0] + duration, before[1] + calls)
    return spent


def bumps(side: int, dev, noise: float):
    """the torus with a smooth field of several bumps (two waves of different period), ``noise`` degrees of per-vertex noise on top"""
    import dataclasses

    import torch

    mesh, v, t = torus(side, dev)
    u = torch.arange(side, device=dev, dtype=torch.float64) * (2.0 * math.pi / side)
    uu, vv = torch.meshgrid(u, u, indexing="ij")
    field = (22.0 + 6.0 * torch.sin(3.0 * uu) * torch.cos(2.0 * vv) + 1.5 * torch.sin(11.0 * uu + 0.3) * torch.cos(9.0 * vv)).reshape(-1)
    if noise:
        gen = torch.Generator(device="cpu").manual_seed(1)
        field = field + noise * (torch.rand((side * side,), generator=gen, dtype=torch.float64).to(dev) - 0.5)
    return dataclasses.replace(mesh, temperature=field.to(torch.float32).contiguous()), v, t


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=1024, help="cells along each way around the torus: 2 side^2 faces")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--min-prominence", type=float, default=1.0)
    ap.add_argument("--noise", type=float, default=0.2, help="degrees of per-vertex noise of the second field")
    ap.add_argument("--trace-pass", action="store_true", help="only run --trace-rounds rounds of the two device entries: the run to trace")
    ap.add_argument("--trace-rounds", type=int, default=5)
    ap.add_argument("--kernels-from", default=None, metavar="DIR", help="append the times of the single kernels from this trace to --out")
    ap.add_argument("--out", default=None, help="also write the report to this file (--kernels-from: append to it)")
    args = ap.parse_args()

    if args.kernels_from is not None:
        spent = kernel_us(args.kernels_from)
        missing = [name for name, _ in KERNELS if name not in spent]
        if missing or args.trace_rounds < 1:
            raise RuntimeError(f"the trace under {args.kernels_from} lacks {missing}; it has {sorted(spent)}")
        lines = [f"kernel trace of {args.trace_rounds} rounds of tn_mesh_peaks and tn_mesh_spots on the smooth field (and of the one mesh_peaks call and "
                 "the incidence build that set the tables up: the peaks' kernels have one round more, the sorts' kernels are also the "
                 "index's): launches, us per launch, us in all launches"]
        for name, what in KERNELS:
            us, calls = spent[name]
            lines.append(f"  {what:44s} {name:24s} {calls:7d} {us / calls:9.1f} {us:10.1f}")
        print("\n".join(lines))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0

    import numpy as np
    import torch

    from pmc_summary import head_stamp  # the sibling module
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.export import (basin_persistence, choose_spots, merge_basins, mesh_incidence, mesh_peaks,
                                        mesh_peaks_workspace_bytes, mesh_regions_into, mesh_regions_workspace_bytes,
                                        mesh_spots_workspace_bytes, smooth_temperature, sort_pairs_workspace_bytes, spot_bounds,
                                        thermal_hotspots)
    from thermo_nerf_amd.export.hotspots import NEVER

    dev = torch.device("cuda")
    lib, stream = _hip.load(), _hip.current_stream()
    lines = []

    def row(what, m):
        lines.append(f"{what:76s} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")

    for noise in (0.0, args.noise):
        mesh, v, t = bumps(args.side, dev, noise)
        index = mesh_incidence(mesh.triangles, v)
        pos, temp, tri = mesh.positions, mesh.temperature, mesh.triangles
        # what the public call does, once, to have the tables of the later parts
        found = mesh_peaks(mesh, index)
        p = basin_persistence(found, temp)
        basin_spot, spot_basin = choose_spots(p, args.min_prominence)
        b, s, k = found.num_basins, found.num_saddles, len(spot_basin)
        death = p.death_saddle[spot_basin]
        limit = np.where(death >= 0, p.saddles["pass_rank"][np.maximum(death, 0)] if s else NEVER, NEVER).astype(np.int32)
        up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
              (basin_spot, p.basin_peak[spot_basin], limit, spot_bounds(p.peak_temperature[spot_basin], math.inf, False))]
        rank, vertex_basin = found.rank, found.vertex_basin
        basin_peak, saddles = torch.empty((v,), dtype=torch.int32, device=dev), torch.empty((3 * t, 4), dtype=torch.int32, device=dev)
        counts = torch.empty((3,), dtype=torch.int64, device=dev)
        need_peaks, need_spots = mesh_peaks_workspace_bytes(v, t), mesh_spots_workspace_bytes(v, t, k)
        need_regions = mesh_regions_workspace_bytes(v, t)
        ws = torch.empty((max(need_peaks, need_spots, need_regions),), dtype=torch.uint8, device=dev)
        vertex_spot, face_spot = torch.empty((v,), dtype=torch.int32, device=dev), torch.empty((t,), dtype=torch.int32, device=dev)
        rows = torch.empty((max(k, 1) * 80,), dtype=torch.uint8, device=dev)

        def peaks():
            _hip.check(lib.tn_mesh_peaks(temp.data_ptr(), tri.data_ptr(), t, v, index.offsets.data_ptr(), index.corners.data_ptr(), 0,
                                         rank.data_ptr(), vertex_basin.data_ptr(), basin_peak.data_ptr(), v, saddles.data_ptr(), 3 * t,
                                         counts.data_ptr(), ws.data_ptr(), need_peaks, stream), "tn_mesh_peaks")

        def spots():
            _hip.check(lib.tn_mesh_spots(pos.data_ptr(), temp.data_ptr(), tri.data_ptr(), v, t, rank.data_ptr(), vertex_basin.data_ptr(),
                                         up[0].data_ptr(), b, up[1].data_ptr(), up[2].data_ptr(), up[3].data_ptr(), k, 0,
                                         vertex_spot.data_ptr(), face_spot.data_ptr(), rows.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                         need_spots, stream), "tn_mesh_spots")

        if args.trace_pass:
            for _ in range(args.trace_rounds):
                peaks(), spots()
            torch.cuda.synchronize()
            return 0

        n = max(v, 3 * t)
        keys = torch.randint(0, 2 ** 31, (n,), dtype=torch.int64, device=dev)
        sorted_keys, order = torch.empty_like(keys), torch.empty((n,), dtype=torch.int32, device=dev)
        sort_ws = torch.empty((sort_pairs_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        edge_bits = 2 * max(1, int(v).bit_length())

        def sort(count, bits):
            _hip.check(lib.tn_sort_pairs(keys.data_ptr(), None, count, bits, sorted_keys.data_ptr(), order.data_ptr(), sort_ws.data_ptr(),
                                         sort_ws.numel(), stream), "tn_sort_pairs")

        region_rows = torch.empty((min(v // 3, t) * 72,), dtype=torch.uint8, device=dev)
        head = torch.empty((5,), dtype=torch.int64, device=dev)

        def regions():
            mesh_regions_into(mesh, 24.0, math.inf, counts=head[:3], totals=head[3:].view(torch.float64), face_region=face_spot,
                              regions=region_rows, workspace=ws)

        def merge():
            start = time.perf_counter()
            merge_basins(p.basin_rank, p.saddles)
            return (time.perf_counter() - start) * 1e3

        merges = sorted(merge() for _ in range(args.repeats))
        lines += [f"thermal hot spots on a closed lattice surface (a torus of {args.side} x {args.side} cells with a relief): {v} vertices, {t} "
                  f"triangles; a smooth field of several bumps" + (f" with {noise} degrees of per-vertex noise" if noise else "") +
                  f": {b} basins, {s} saddles, {k} spots above {args.min_prominence} degrees; workspaces {need_peaks / 2 ** 20:.1f} MiB "
                  f"(peaks), {need_spots / 2 ** 20:.1f} MiB (spots), {need_regions / 2 ** 20:.1f} MiB (regions); device events around each "
                  f"call, 3 warm-up calls, {args.repeats} timed calls, ms per call",
                  f"measured at commit {head_stamp()}",
                  "what                                                                            median ms   min .. max"]
        row("tn_mesh_peaks alone (rank, ascent, jumps, basins, saddles)", mesh_scenes.event_ms(peaks, args.repeats))
        row(f"  of it the rank sort: tn_sort_pairs of {v} pairs, 32 key bits", mesh_scenes.event_ms(lambda: sort(v, 32), args.repeats))
        row(f"  of it the half-edge sort: tn_sort_pairs of {3 * t} pairs, {edge_bits} key bits", mesh_scenes.event_ms(lambda: sort(3 * t, edge_bits), args.repeats))
        row(f"tn_basin_persistence on the host ({b} basins, {s} saddles; the host's clock)", (merges[len(merges) // 2], merges[0], merges[-1]))
        row(f"tn_mesh_spots alone ({k} spots)", mesh_scenes.event_ms(spots, args.repeats))
        row("tn_mesh_regions alone on the same mesh, from 24 degrees up (for scale)", mesh_scenes.event_ms(regions, args.repeats))
        row("thermal_hotspots (the index, the three entries, the host reads)", mesh_scenes.event_ms(lambda: thermal_hotspots(mesh, args.min_prominence), args.repeats))
        if noise:
            row("thermal_hotspots after 5 smoothing iterations", mesh_scenes.event_ms(lambda: thermal_hotspots(mesh, args.min_prominence, smooth_iterations=5), args.repeats))
            calm = mesh_peaks(smooth_temperature(mesh, 5), index)
            lines.append(f"(after 5 smoothing iterations: {calm.num_basins} basins, {calm.num_saddles} saddles)")
        lines.append("")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
