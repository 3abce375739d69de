#!/usr/bin/env python
"""What the level-set curves cost on a mesh of a survey's size: the half-edge build, one plane section and 32 isotherms in one call on
a closed lattice surface of about 2 M faces generated here (a torus of ``--side`` x ``--side`` two-triangle cells with a smooth relief and
a smooth temperature field with seeded per-vertex noise; no file, no reference data).

``mesh_half_edges``, ``mesh_sections`` and ``isotherms`` are timed as their callers run them — allocation, the kernels, the host reads —
with device events around the call; the raw ``tn_mesh_isolines`` entry into preallocated outputs of exactly S segments is timed beside
them.  3 warm-up calls, then ``--repeats`` timed calls each; the report gives the median and the range, the mesh size and the commit.
A record, not a gate.

The share of the pointer-jumping rounds comes from a kernel trace taken in a run of its own:

    python tools/mesh_isolines_bench.py [--side 1024] [--repeats 11] --out profiles/micro/mesh_isolines.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_isolines_bench.py --trace-pass
    python tools/mesh_isolines_bench.py --share-from DIR --out profiles/micro/mesh_isolines.txt     # appends the share
"""
from __future__ import annotations

import argparse
import glob
import math
import os
import sqlite3
import sys

import mesh_scenes  # the sibling module: event_ms, emit; it puts the repository on sys.path

JUMP_KERNELS = ("sweep1_kernel", "sweep2_kernel")
OWN_KERNELS = ("faces_kernel", "scan_faces_kernel", "bases_kernel", "segments_kernel", "preds_kernel", "sweep1_start_kernel", "cut_kernel",
               "lengths_kernel", "count_curves_kernel", "scan_curves_kernel", "emit_curves_kernel", "points_kernel", "walk_kernel") + JUMP_KERNELS


def torus(side: int, dev, seed: int = 0):
    """a closed, consistently oriented lattice surface: side x side cells around a torus (major radius 2, minor radius 0.7 with a relief
    of 0.08), two triangles per cell: (ThermalMesh, vertices, faces)"""
    import torch

    from thermo_nerf_amd.export import ThermalMesh

    u = torch.arange(side, device=dev, dtype=torch.float64) * (2.0 * math.pi / side)
    uu, vv = torch.meshgrid(u, u, indexing="ij")
    minor = 0.7 + 0.08 * torch.sin(5.0 * uu) * torch.cos(7.0 * vv)
    ring = 2.0 + minor * torch.cos(vv)
    pos = torch.stack([ring * torch.cos(uu), ring * torch.sin(uu), minor * torch.sin(vv)], dim=-1).reshape(-1, 3).to(torch.float32)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    noise = torch.rand((side * side,), generator=gen, dtype=torch.float64).to(dev)
    temp = (22.0 + 6.0 * torch.sin(3.0 * uu) * torch.cos(2.0 * vv)).reshape(-1) + 0.2 * (noise - 0.5)
    i = torch.arange(side, device=dev)
    a = (i[:, None] * side + i[None, :]).reshape(-1)
    b = (((i + 1) % side)[:, None] * side + i[None, :]).reshape(-1)
    c = (((i + 1) % side)[:, None] * side + ((i + 1) % side)[None, :]).reshape(-1)
    d = (i[:, None] * side + ((i + 1) % side)[None, :]).reshape(-1)
    tri = torch.stack([torch.stack([a, b, c], dim=1), torch.stack([a, c, d], dim=1)], dim=1).reshape(-1, 3).to(torch.int32)
    mesh = ThermalMesh(pos.contiguous(), torch.zeros((side * side, 3), dtype=torch.uint8, device=dev), temp.to(torch.float32).contiguous(),
                       None, tri.contiguous(), (14.0, 30.0))
    return mesh, side * side, 2 * side * side


def jump_share(directory: str):
    """(share of the pointer-jumping kernels in the time of tn_mesh_isolines' kernels, their time in us, all in us) from the rocpd
    database(s) of a kernel trace under ``directory``"""
    jump = total = 0.0
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        for name, duration in sqlite3.connect(path).cursor().execute("select name,total_duration from top_kernels"):
            if any(k in name for k in OWN_KERNELS):
                total += duration
                if any(k in name for k in JUMP_KERNELS):
                    jump += duration
    if total <= 0.0:
        raise RuntimeError(f"no kernel of tn_mesh_isolines in the trace under {directory}")
    return jump / total, jump, total


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=1024, help="cells along each way around the torus: 2 side^2 faces")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--isotherms", type=int, default=32)
    ap.add_argument("--trace-pass", action="store_true", help="only run the raw 32-isotherm call a few times: the run to trace")
    ap.add_argument("--share-from", default=None, metavar="DIR", help="append the share of the pointer-jumping rounds from this trace to --out")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    if args.share_from is not None:
        share, jump, total = jump_share(args.share_from)
        line = (f"pointer-jumping rounds ({' + '.join(JUMP_KERNELS)}) in a kernel trace of the raw {args.isotherms}-isotherm call: "
                f"{100.0 * share:.1f} % of the time of tn_mesh_isolines' kernels ({jump:.0f} of {total:.0f} us over the traced calls)")
        print(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return 0

    import torch

    from pmc_summary import head_stamp  # the sibling module
    from thermo_nerf_amd.export import (isotherms, mesh_half_edges, mesh_half_edges_workspace_bytes, mesh_isolines_into,
                                        mesh_isolines_workspace_bytes, mesh_sections)
    from thermo_nerf_amd.export.isolines import CURVE_BYTES

    dev = torch.device("cuda")
    mesh, v, t = torus(args.side, dev)
    edges = mesh_half_edges(mesh.triangles, v)
    assert edges.closed_manifold, "the torus is closed, manifold and consistently oriented"
    lo, hi = float(mesh.temperature.min()), float(mesh.temperature.max())
    levels = [lo + (hi - lo) * (k + 0.5) / args.isotherms for k in range(args.isotherms)]
    cases = (("one plane section (z = 0.1)", dict(plane_normal=(0.0, 0.0, 1.0)), [0.1], lambda: mesh_sections(mesh, (0.0, 0.0, 1.0), [0.1], half_edges=edges)),
             (f"{args.isotherms} isotherms in one call", dict(scalar=mesh.temperature), levels, lambda: isotherms(mesh, levels, half_edges=edges)))
    counts = torch.empty((5,), dtype=torch.int64, device=dev)

    def raw_of(kw, values):
        mesh_isolines_into(mesh, edges.twin, values, counts=counts, **kw)  # the sizing call
        s = int(counts[0].item())
        out = dict(positions=torch.empty((2 * s, 3), device=dev), temperature=torch.empty((2 * s,), device=dev),
                   arc=torch.empty((2 * s,), dtype=torch.float64, device=dev), face=torch.empty((2 * s,), dtype=torch.int32, device=dev),
                   curves=torch.empty((s * CURVE_BYTES,), dtype=torch.uint8, device=dev),
                   workspace=torch.empty((mesh_isolines_workspace_bytes(v, t, s),), dtype=torch.uint8, device=dev))
        return s, out, lambda: mesh_isolines_into(mesh, edges.twin, values, counts=counts, capacity_segments=s, **kw, **out)

    if args.trace_pass:
        _, _, call = raw_of(cases[1][1], cases[1][2])
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        return 0

    ws = torch.empty((mesh_half_edges_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)
    lines = [f"level-set curves on a closed lattice surface (a torus of {args.side} x {args.side} cells with a relief): {v} vertices, {t} triangles, "
             f"{edges.edges} edges, none boundary, non-manifold or inconsistent; device events around each call, 3 warm-up calls, "
             f"{args.repeats} timed calls, ms per call",
             f"measured at commit {head_stamp()}",
             "what                                                          segments    curves    closed  jump rounds   median ms   min .. max"]
    m = mesh_scenes.event_ms(lambda: mesh_half_edges(mesh.triangles, v, workspace=ws), args.repeats)
    lines.append(f"{'mesh_half_edges (tn_mesh_half_edges and the read of its counts)':60s} {'-':>9s} {'-':>9s} {'-':>9s} {'-':>12s} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")
    for name, kw, values, public in cases:
        found = public()
        s, out, call = raw_of(kw, values)
        rounds = 2 * max(1, math.ceil(math.log2(max(2, s))))
        tail = f"{found.num_segments:9d} {found.num_curves:9d} {found.closed_curves:9d} {rounds:12d}"
        for what, fn in ((f"tn_mesh_isolines alone, {name}", call), (f"the public call, {name}", public)):
            m = mesh_scenes.event_ms(fn, args.repeats)
            lines.append(f"{what:60s} {tail} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")
        lines.append(f"{'  workspace of that call':60s} {out['workspace'].numel() / 2 ** 20:9.1f} MiB")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
