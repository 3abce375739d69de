#!/usr/bin/env python
"""What a closest-point query costs: ``tn_mesh_closest`` through its raw wrapper into preallocated buffers, device events around each
call, on the room of ``tools/mesh_raycast_bench.py`` at its two face counts (about 250 000 and about 1 000 000 faces), 1920 x 1080
query points.  Two sets of points per mesh: the surface's own vertices, cycled, each moved by 1 % of the room's extent in a random
direction — the mesh-to-mesh case, every point next to the surface and neighbouring lanes next to each other —, and uniform points in
the room's extent — the hard case, far from the surface and without order.  Beside each: the closest-hit ``tn_mesh_raycast`` of the
same number of camera rays on the same mesh and tree, timed in the same run — the yardstick.  Every output array is written by both.
3 warm-up calls, then ``--repeats`` timed calls each; median and range.  A record, not a gate.

    python tools/mesh_closest_bench.py [--width 1920 --height 1080] [--repeats 21] [--out profiles/micro/mesh_closest.txt]
"""
from __future__ import annotations

import argparse
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cells", type=int, nargs="+", default=[126, 252], help="cells per side of a wall: 12 cells^2 faces and the boxes'")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import ThermalMesh, build_mesh_bvh, camera_rays, mesh_closest_into, mesh_raycast_into

    event_ms, cell = mesh_scenes.event_ms, mesh_scenes.cell
    dev = torch.device("cuda")
    w, h = args.width, args.height
    n = w * h
    camera = mesh_scenes.room_camera(w, h)
    origins, directions = camera_rays(camera, dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    distance, temperature, difference = torch.empty((n,), device=dev), torch.empty((n,), device=dev), torch.empty((n,), device=dev)
    where, uv = torch.empty((n, 3), device=dev), torch.empty((n, 2), device=dev)
    colors = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    counts = torch.empty((4,), dtype=torch.int64, device=dev)
    stats, cast_stats = torch.empty((8,), dtype=torch.float64, device=dev), torch.empty((3,), dtype=torch.float64, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(7)
    extent = torch.tensor([6.0, 4.0, 3.0])
    step = torch.randn((n, 3), generator=gen)
    step = (step / step.norm(dim=1, keepdim=True) * (0.01 * float(extent.max()))).to(dev)
    uniform = (torch.rand((n, 3), generator=gen) * extent).to(dev)
    own = torch.full((n,), 20.0, device=dev)
    lines = [f"tn_mesh_closest on the room of mesh_raycast_bench, {n} query points ({w} x {h}), every output array written; beside it the "
             f"closest-hit tn_mesh_raycast of {n} camera rays on the same tree; device events around each call, 3 warm-up calls, "
             f"{args.repeats} timed calls, ms per call (median, min .. max)",
             "faces      depth   near-surface ms                 Mpoints/s  mean dist   uniform ms                      Mpoints/s  mean dist   "
             "cast ms                         Mrays/s   near / cast   uniform / cast"]
    rows = []
    for cells in args.cells:
        pos, temp, col, tri = mesh_scenes.room(cells, 1, dev)
        mesh = ThermalMesh(pos, col, temp, None, tri)
        faces = int(tri.shape[0])
        bvh = build_mesh_bvh(mesh)
        depth = bvh.tree()["depth"]
        near = (pos[torch.arange(n, device=dev) % pos.shape[0]] + step).contiguous()

        def query(points):
            mesh_closest_into(bvh, points, point_temperature=own, closest_face=face, closest_distance=distance, closest_point=where,
                              closest_uv=uv, closest_temperature=temperature, closest_colors=colors, difference=difference, counts=counts,
                              stats=stats)

        found = []
        for points in (near, uniform):
            ms = event_ms(lambda: query(points), args.repeats)
            got, total = counts.cpu().tolist(), stats.cpu().tolist()
            assert got[0] == n and got[3] == 0, got
            found.append((ms, total[0] / n))
        cast = event_ms(lambda: mesh_raycast_into(bvh, origins, directions, hit_face=face, hit_t=distance, hit_uv=uv, hit_temperature=temperature,
                                                  hit_colors=colors, counts=counts, stats=cast_stats), args.repeats)

        (a, da), (b, db) = found
        lines.append(f"{faces:<10d} {depth:<7d} {cell(a):<31s} {n / a[0] / 1e3:<10.1f} {da:<11.5f} {cell(b):<31s} {n / b[0] / 1e3:<10.1f} {db:<11.5f} "
                     f"{cell(cast):<31s} {n / cast[0] / 1e3:<9.1f} {a[0] / cast[0]:<13.2f} {b[0] / cast[0]:.2f}")
        rows.append((faces, a[0], b[0], cast[0]))
        del bvh
    if len(rows) > 1:
        (f0, a0, b0, c0), (f1, a1, b1, c1) = rows[0], rows[-1]
        lines.append(f"at {f1} faces / at {f0} faces ({f1 / f0:.2f} x the faces): near-surface {a1 / a0:.2f} x, uniform {b1 / b0:.2f} x, "
                     f"cast {c1 / c0:.2f} x (medians above)")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
