#!/usr/bin/env python
"""What the planar patches cost on a mesh of a survey's size: the half-edge build, ``tn_mesh_patches`` at 10 and at 180 degrees, and —
the nearest thing the layer could do before, on the same sort and the same ordered sums — ``thermal_regions`` over the whole window, on
the closed lattice surface of about 2 M faces of tools/mesh_isolines_bench.py (a torus of ``--side`` x ``--side`` two-triangle cells with
a smooth relief; no file, no reference data).  Neighbouring faces of that surface differ by well under a degree, so both limits give ONE
patch of the whole surface: the longest union-find chains and the longest walks.

``mesh_half_edges``, ``planar_patches`` and ``thermal_regions`` are timed as their callers run them — allocation, the kernels, the host
reads — with device events around the call; the raw ``tn_mesh_patches`` and ``tn_mesh_regions`` entries into preallocated outputs are
timed beside them.  3 warm-up calls, then ``--repeats`` timed calls each; the report gives the median and the range, the mesh size and
the commit.  A record, not a gate.

The shares of the hook, the sort and the two sum passes come from a kernel trace taken in a run of its own:

    python tools/mesh_patches_bench.py [--side 1024] [--repeats 11] --out profiles/micro/mesh_patches.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_patches_bench.py --trace-pass
    rocprofv3 --kernel-trace --stats -d BASE -- python tools/mesh_patches_bench.py --trace-pass --trace-calls 0
    python tools/mesh_patches_bench.py --share-from DIR --baseline BASE --out profiles/micro/mesh_patches.txt     # appends the shares

The traced process also builds the mesh and its half-edges (``tn_mesh_half_edges`` sorts with the same ``tn_sort_pairs`` kernels) and
makes the sizing call; the baseline run is that process without the full calls, and the shares are the difference per call, kernel
names matched whole.
"""
from __future__ import annotations

import argparse
import glob
import math
import os
import sqlite3
import sys

import mesh_scenes  # the sibling module: event_ms, emit; it puts the repository on sys.path
from mesh_isolines_bench import torus  # the sibling module: the closed lattice surface

GROUPS = (("hook (the union-find)", ("hook_kernel", "flatten_kernel")),
          ("sort (tn_sort_pairs)", ("histogram_kernel", "scatter_kernel", "scan_kernel")),
          ("first sum pass (block sums, rows)", ("block_sums_kernel<Acc>", "rows_kernel")),
          ("second sum pass (deviations, block sums, rows)", ("deviations_kernel", "block_sums_kernel<Dev>", "finish_rows_kernel")),
          ("the rest (faces, lists, keys, numbering, totals)", ("faces_kernel", "scan_faces_kernel", "lists_kernel", "keys_kernel", "count_heads_kernel",
                                                                 "scan_counts_kernel", "emit_heads_kernel", "count_blocks_kernel", "emit_blocks_kernel",
                                                                 "assign_kernel", "total_blocks_kernel", "totals_kernel")))
GROUP_OF = {kernel: group for group, kernels in GROUPS for kernel in kernels}


def short_name(name: str) -> str:
    """a traced kernel name without its namespace, return type and arguments: ``block_sums_kernel<Acc>``"""
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()


def kernel_us(directory: str) -> dict:
    """{whole kernel name: us} of the kernels that tn_mesh_patches launches, from the rocpd database(s) of a kernel trace under
    ``directory``.  Names are matched WHOLE; other entries launch kernels of the same names (the half-edge build sorts too), which is
    why a trace is only read beside its baseline (``shares``)."""
    spent = {}
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        for name, duration in sqlite3.connect(path).cursor().execute("select name,total_duration from top_kernels"):
            short = short_name(name)
            if short in GROUP_OF:
                spent[short] = spent.get(short, 0.0) + duration
    return spent


def shares(directory: str, baseline: str, calls: int):
    """({group: us per call}, {kernel: us per call}) of ONE full tn_mesh_patches call: the trace of ``--trace-pass --trace-calls N``
    under ``directory`` minus the trace of ``--trace-pass --trace-calls 0`` under ``baseline`` — the same process up to the timed
    calls: the mesh, the half-edge build with its own sort, the sizing call — over N"""
    traced, before = kernel_us(directory), kernel_us(baseline)
    kernels = {k: (us - before.get(k, 0.0)) / calls for k, us in traced.items()}
    spent = {group: sum(kernels.get(k, 0.0) for k in names) for group, names in GROUPS}
    if calls < 1 or sum(spent.values()) <= 0.0 or min(kernels.values()) < 0.0:
        raise RuntimeError(f"the traces under {directory} and {baseline} are not a run of {calls} calls and its baseline")
    return spent, kernels


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=1024, help="cells along each way around the torus: 2 side^2 faces")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--trace-pass", action="store_true", help="only run the raw 10-degree call --trace-calls times: the run to trace")
    ap.add_argument("--trace-calls", type=int, default=5, help="full calls of the traced run; 0: the baseline, everything but them")
    ap.add_argument("--share-from", default=None, metavar="DIR", help="append the shares of the kernel groups from this trace to --out")
    ap.add_argument("--baseline", default=None, metavar="DIR", help="the trace of --trace-calls 0 that --share-from subtracts")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    if args.share_from is not None:
        if args.baseline is None:
            ap.error("--share-from needs --baseline: other entries of the traced process launch kernels of the same names")
        spent, kernels = shares(args.share_from, args.baseline, args.trace_calls)
        total = sum(spent.values())
        lines = [f"kernel trace of the raw 10-degree call, full calls only ({args.trace_calls} calls minus a baseline run without them: the "
                 f"half-edge build, its sort and the sizing call are not in it): {total:.0f} us of kernels per call"]
        lines += [f"  {group:52s} {100.0 * us / total:5.1f} %  ({us:.0f} us)" for group, us in spent.items()]
        top = sorted(kernels.items(), key=lambda item: -item[1])[:6]
        lines.append("  the longest kernels: " + ", ".join(f"{name} {100.0 * us / total:.1f} %" for name, us in top))
        print("\n".join(lines))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0

    import torch

    from pmc_summary import head_stamp  # the sibling module
    from thermo_nerf_amd.export import (mesh_half_edges, mesh_half_edges_workspace_bytes, mesh_patches_into, mesh_patches_workspace_bytes,
                                        mesh_regions_into, mesh_regions_workspace_bytes, planar_patches, thermal_regions)
    from thermo_nerf_amd.export.patches import PATCH_BYTES
    from thermo_nerf_amd.export.regions import REGION_BYTES, max_regions

    dev = torch.device("cuda")
    mesh, v, t = torus(args.side, dev)
    edges = mesh_half_edges(mesh.triangles, v)
    assert edges.closed_manifold, "the torus is closed, manifold and consistently oriented"
    three, two = torch.empty((3,), dtype=torch.int64, device=dev), torch.empty((2,), dtype=torch.float64, device=dev)
    face_patch = torch.empty((t,), dtype=torch.int32, device=dev)
    pws = torch.empty((mesh_patches_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)

    def raw_of(min_cos):
        mesh_patches_into(mesh, edges.twin, min_cos, counts=three, totals=two, face_patch=face_patch, workspace=pws)  # the sizing call
        q = int(three[0].item())
        rows = torch.empty((q * PATCH_BYTES,), dtype=torch.uint8, device=dev)
        return q, lambda: mesh_patches_into(mesh, edges.twin, min_cos, counts=three, totals=two, face_patch=face_patch, patches=rows,
                                            workspace=pws)

    if args.trace_pass:
        _, call = raw_of(math.cos(math.radians(10.0)))
        for _ in range(args.trace_calls):
            call()
        torch.cuda.synchronize()
        return 0

    ews = torch.empty((mesh_half_edges_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)
    lines = [f"planar patches on a closed lattice surface (a torus of {args.side} x {args.side} cells with a relief): {v} vertices, {t} triangles, "
             f"{edges.edges} edges, none boundary, non-manifold or inconsistent; workspace of tn_mesh_patches {pws.numel() / 2 ** 20:.1f} MiB; device "
             f"events around each call, 3 warm-up calls, {args.repeats} timed calls, ms per call",
             f"measured at commit {head_stamp()}",
             "what                                                                       patches  largest patch   median ms   min .. max"]

    def row(what, patches, largest, m):
        lines.append(f"{what:72s} {patches:>9} {largest:>14} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")

    row("mesh_half_edges (tn_mesh_half_edges and the read of its counts)", "-", "-",
        mesh_scenes.event_ms(lambda: mesh_half_edges(mesh.triangles, v, workspace=ews), args.repeats))
    for degrees in (10.0, 180.0, 0.1):
        found = planar_patches(mesh, degrees, half_edges=edges)
        largest = int(found.patches["faces"].max()) if len(found) else 0
        q, call = raw_of(math.cos(math.radians(degrees)))
        assert q == found.num_patches
        row(f"tn_mesh_patches alone, {degrees:g} degrees", q, largest, mesh_scenes.event_ms(call, args.repeats))
        row(f"planar_patches, {degrees:g} degrees (rows for T patches, two host reads)", q, largest,
            mesh_scenes.event_ms(lambda: planar_patches(mesh, degrees, half_edges=edges), args.repeats))
    window = (-math.inf, math.inf)
    found = thermal_regions(mesh, *window)
    largest = int(found.regions["faces"].max()) if len(found) else 0
    rows = torch.empty((max_regions(v, t) * REGION_BYTES,), dtype=torch.uint8, device=dev)
    rws = torch.empty((mesh_regions_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)
    row("tn_mesh_regions alone, the whole window (vertex connectivity)", found.num_regions, largest,
        mesh_scenes.event_ms(lambda: mesh_regions_into(mesh, *window, counts=three, totals=two, face_region=face_patch, regions=rows,
                                                       workspace=rws), args.repeats))
    row("thermal_regions, the whole window", found.num_regions, largest, mesh_scenes.event_ms(lambda: thermal_regions(mesh, *window), args.repeats))
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
