#!/usr/bin/env python
"""What the vertex-clustering simplification costs beside the extraction it rides behind: ``simplify_mesh`` on the surface-nets mesh
of an analytic sphere (radius 0.3 in a 256^3 volume over [-0.5, 0.5]^3, written directly as a TSDF volume: no model, no render) at
cell sizes of 2 and 4 grid steps, and one emitting ``tn_mesh_extract`` call on the same volume.

``simplify_mesh`` is timed as its callers run it — grid from the bounding box, allocation at the upper bounds, the kernel, the two
host reads — with device events around the call; the raw ``tn_mesh_simplify`` entry into preallocated outputs is timed beside it.
3 warm-up calls, then ``--repeats`` timed calls each; the report gives the median and the range.  A record, not a gate.

    python tools/mesh_simplify_bench.py [--resolution 256] [--repeats 21] [--out profiles/micro/mesh_simplify.txt]
"""
from __future__ import annotations

import argparse
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path
from mesh_scenes import HALF, RADIUS, TRUNCATION_STEPS, event_ms, sphere_volume


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd import colormaps
    from thermo_nerf_amd.export import (ThermalMesh, mesh_extract, mesh_simplify_into, mesh_simplify_workspace_bytes,
                                        mesh_workspace_bytes, simplify_mesh, voxel_grid, voxel_params)

    dev = torch.device("cuda")
    n = args.resolution
    volume, params, step = sphere_volume(n, dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((mesh_workspace_bytes((n,) * 3),), dtype=torch.uint8, device=dev)
    mesh_extract(volume, params, counts=counts, workspace=ws)
    v, t = (int(c) for c in counts.tolist())
    mesh = ThermalMesh(torch.empty((v, 3), device=dev), torch.empty((v, 3), dtype=torch.uint8, device=dev), torch.empty((v,), device=dev),
                       torch.empty((v, 3), dtype=torch.uint8, device=dev), torch.empty((t, 3), dtype=torch.int32, device=dev), (14.0, 33.0))
    table = colormaps.get_table("magma", dev)[1]

    def extract_call():
        mesh_extract(volume, params, counts=counts, positions=mesh.positions, colors=mesh.colors, temperature=mesh.temperature,
                     thermal_colors=mesh.thermal_colors, thermal_table=table, triangles=mesh.triangles, workspace=ws)

    extract_call()
    lines = [f"vertex-clustering simplification of the surface-nets mesh of an analytic sphere (radius {RADIUS}, {n}^3 volume over "
             f"[-{HALF}, {HALF}]^3, truncation {TRUNCATION_STEPS:g} steps), beside one emitting tn_mesh_extract call on the same volume; "
             f"device events around each call, 3 warm-up calls, {args.repeats} timed calls, ms per call",
             "what                                          vertices   triangles   -> vertices   triangles  degenerate  duplicate   median ms   min .. max"]
    e = event_ms(extract_call, args.repeats)
    lines.append(f"{'tn_mesh_extract (emitting call)':44s} {v:9d} {t:11d}   {'-':>11s} {'-':>11s} {'-':>11s} {'-':>10s} {e[0]:11.4f}   {e[1]:.4f} .. {e[2]:.4f}")
    lo, hi = mesh.positions.amin(dim=0).tolist(), mesh.positions.amax(dim=0).tolist()
    out = dict(positions=torch.empty((v, 3), device=dev), colors=torch.empty((v, 3), dtype=torch.uint8, device=dev),
               temperature=torch.empty((v,), device=dev), cluster_count=torch.empty((v,), dtype=torch.int32, device=dev),
               thermal_colors=torch.empty((v, 3), dtype=torch.uint8, device=dev), triangles=torch.empty((t, 3), dtype=torch.int32, device=dev))
    four = torch.empty((4,), dtype=torch.int64, device=dev)
    sws = torch.empty((mesh_simplify_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)
    for steps in (2.0, 4.0):
        size = steps * step
        _, info = simplify_mesh(mesh, size)
        origin, dims = voxel_grid(lo, hi, size)
        grid = voxel_params(origin, size, dims)
        tail = (f"{info.vertices_after:11d} {info.triangles_after:11d} {info.degenerate_triangles:11d} {info.duplicate_triangles:10d}")
        for name, fn in ((f"simplify_mesh, cell {steps:g} steps", lambda: simplify_mesh(mesh, size)),
                         (f"tn_mesh_simplify alone, cell {steps:g} steps", lambda: mesh_simplify_into(mesh, grid, counts=four, workspace=sws, **out))):
            m = event_ms(fn, args.repeats)
            lines.append(f"{name:44s} {v:9d} {t:11d}   {tail} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
