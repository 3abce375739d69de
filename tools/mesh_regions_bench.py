#!/usr/bin/env python
"""What the thermal-region analysis costs beside the labelling it is built on: ``tn_mesh_regions`` and ``thermal_regions`` on the
surface-nets mesh of an analytic sphere (radius 0.3 in a 256^3 volume, the mesh of tools/mesh_simplify_bench.py) with two
temperature fields — (a) the extraction's own, with a window that holds all of it: ONE region of the whole surface, the longest
walks; (b) a three-dimensional checkerboard of warm (30 degrees) and cold (15 degrees) cells with a window from 26 degrees, which only
the faces with three warm vertices pass: MANY small regions, one per warm cell the surface cuts — and, as the
yardstick, ``tn_mesh_components`` on the same triangles.

``thermal_regions`` is timed as its callers run it — allocation at the upper bounds, the kernels, the two host reads, the ordering of
the table — with device events around the call; the raw ``tn_mesh_regions`` entry into preallocated outputs is timed beside it.
3 warm-up calls, then ``--repeats`` timed calls each; the report gives the median and the range.  A record, not a gate.

    python tools/mesh_regions_bench.py [--resolution 256] [--repeats 21] [--out profiles/micro/mesh_regions.txt]
"""
from __future__ import annotations

import argparse
import math
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cells", type=float, default=48.0, help="checkerboard cells along the volume's edge")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import (ThermalMesh, mesh_components, mesh_extract, mesh_regions_into, mesh_regions_workspace_bytes,
                                        mesh_workspace_bytes, thermal_regions)
    from thermo_nerf_amd.export.regions import REGION_BYTES, max_regions

    dev = torch.device("cuda")
    n = args.resolution
    volume, params, _ = mesh_scenes.sphere_volume(n, dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((mesh_workspace_bytes((n,) * 3),), dtype=torch.uint8, device=dev)
    mesh_extract(volume, params, counts=counts, workspace=ws)
    v, t = (int(c) for c in counts.tolist())
    mesh = ThermalMesh(torch.empty((v, 3), device=dev), torch.empty((v, 3), dtype=torch.uint8, device=dev), torch.empty((v,), device=dev),
                       None, torch.empty((t, 3), dtype=torch.int32, device=dev), (14.0, 33.0))
    mesh_extract(volume, params, counts=counts, positions=mesh.positions, colors=mesh.colors, temperature=mesh.temperature,
                 triangles=mesh.triangles, workspace=ws)
    del volume, ws
    p = mesh.positions * (args.cells * math.pi / (2 * mesh_scenes.HALF))
    checker = torch.where(torch.sin(p[:, 0]) * torch.sin(p[:, 1]) * torch.sin(p[:, 2]) > 0, 30.0, 15.0).to(torch.float32)
    fields = (("one region of the whole surface", mesh.temperature, (-math.inf, math.inf)),
              (f"checkerboard of {args.cells:g} cells, the warm ones", checker, (26.0, math.inf)))

    cap = max_regions(v, t)
    three, two = torch.empty((3,), dtype=torch.int64, device=dev), torch.empty((2,), dtype=torch.float64, device=dev)
    rows = torch.empty((cap * REGION_BYTES,), dtype=torch.uint8, device=dev)
    face_region = torch.empty((t,), dtype=torch.int32, device=dev)
    rws = torch.empty((mesh_regions_workspace_bytes(v, t),), dtype=torch.uint8, device=dev)
    lines = [f"thermal regions of the surface-nets mesh of an analytic sphere (radius {mesh_scenes.RADIUS}, {n}^3 volume over "
             f"[-{mesh_scenes.HALF}, {mesh_scenes.HALF}]^3): {v} vertices, {t} triangles; workspace {rws.numel() / 2 ** 20:.1f} MiB; device events "
             f"around each call, 3 warm-up calls, {args.repeats} timed calls, ms per call",
             "what                                                                      regions    selected  largest region   median ms   min .. max"]
    c = mesh_scenes.event_ms(lambda: mesh_components(mesh.triangles, v), args.repeats)
    lines.append(f"{'tn_mesh_components of all triangles (the yardstick)':72s} {'-':>8s} {'-':>11s} {'-':>15s} {c[0]:11.4f}   {c[1]:.4f} .. {c[2]:.4f}")
    for name, temperature, window in fields:
        field = ThermalMesh(mesh.positions, mesh.colors, temperature, None, mesh.triangles, mesh.temperature_bounds)
        found = thermal_regions(field, *window)
        largest = int(found.regions["faces"].max()) if len(found) else 0
        tail = f"{found.num_regions:8d} {found.selected_faces:11d} {largest:15d}"

        def raw_call():
            mesh_regions_into(field, *window, counts=three, totals=two, face_region=face_region, regions=rows, workspace=rws)

        for what, fn in ((f"tn_mesh_regions alone, {name}", raw_call), (f"thermal_regions, {name}", lambda: thermal_regions(field, *window))):
            m = mesh_scenes.event_ms(fn, args.repeats)
            lines.append(f"{what:72s} {tail} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
