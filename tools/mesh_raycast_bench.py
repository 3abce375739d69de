#!/usr/bin/env python
"""What a camera view of a mesh costs: ``tn_mesh_bvh_build`` and ``tn_mesh_raycast`` through their raw wrappers into preallocated
buffers, device events around each call, on a synthetic room — a closed box of 6 x 4 x 3 units seen from inside, every wall a jittered
lattice of two-triangle cells, with boxes standing on the floor — at about 250 000 and about 1 000 000 faces under the 1920 x 1080
rays of one pinhole camera (``tn_generate_rays``).  Recorded per mesh: build ms, closest-hit cast ms and rays per second, any-hit cast
ms, the tree's depth, the hit share.  Beside them, for context: ``tn_mesh_rasterize`` on the same mesh at the same pixel count (an
orthographic view along -z from above: a different projection, the same number of faces and pixels), and the ratio of the cast time at
the large mesh to the cast time at the small one — a working hierarchy keeps it well under the ratio of the face counts.  3 warm-up
calls, then ``--repeats`` timed calls each; median and range.  A record, not a gate.

    python tools/mesh_raycast_bench.py [--width 1920 --height 1080] [--repeats 21] [--out profiles/micro/mesh_raycast.txt]
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

    from thermo_nerf_amd.export import (MeshBVH, RasterView, ThermalMesh, camera_rays, mesh_bvh_bytes, mesh_bvh_workspace_bytes,
                                        build_mesh_bvh, mesh_raycast_into, mesh_rasterize_into, mesh_rasterize_workspace_bytes)

    event_ms, cell = mesh_scenes.event_ms, mesh_scenes.cell
    dev = torch.device("cuda")
    w, h = args.width, args.height
    n = w * h
    camera = mesh_scenes.room_camera(w, h)
    origins, directions = camera_rays(camera, dev)
    face = torch.empty((n,), dtype=torch.int32, device=dev)
    t, temperature = torch.empty((n,), device=dev), torch.empty((n,), device=dev)
    uv, colors = torch.empty((n, 2), device=dev), torch.empty((n, 3), dtype=torch.uint8, device=dev)
    some = torch.empty((n,), dtype=torch.uint8, device=dev)
    counts, stats = torch.empty((4,), dtype=torch.int64, device=dev), torch.empty((3,), dtype=torch.float64, device=dev)
    lines = [f"tn_mesh_bvh_build and tn_mesh_raycast on a room seen from inside, {w} x {h} camera rays, every output array written; device "
             f"events around each call, 3 warm-up calls, {args.repeats} timed calls, ms per call (median, min .. max)",
             "faces      depth   hit share   build ms                      closest-hit ms                 Mrays/s   any-hit ms                     "
             "rasterise ms (same mesh, same pixel count, orthographic)"]
    cast_ms = []
    for cells in args.cells:
        pos, temp, col, tri = mesh_scenes.room(cells, 1, dev)
        mesh = ThermalMesh(pos, col, temp, None, tri)
        faces = int(tri.shape[0])
        blob = torch.empty((mesh_bvh_bytes(faces),), dtype=torch.uint8, device=dev)
        ws = torch.empty((mesh_bvh_workspace_bytes(faces),), dtype=torch.uint8, device=dev)
        build = event_ms(lambda: build_mesh_bvh(mesh, blob=blob, workspace=ws), args.repeats)
        bvh = MeshBVH(blob, int(pos.shape[0]), faces, mesh)
        depth = bvh.tree()["depth"]
        closest = event_ms(lambda: mesh_raycast_into(bvh, origins, directions, hit_face=face, hit_t=t, hit_uv=uv, hit_temperature=temperature,
                                                     hit_colors=colors, counts=counts, stats=stats), args.repeats)
        got = counts.cpu().tolist()
        any_hit = event_ms(lambda: mesh_raycast_into(bvh, origins, directions, any_hit=True, hit_any=some), args.repeats)
        view = RasterView((0.0, 4.0, 3.5), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), 6.0 / w, w, h)
        rws = torch.empty((mesh_rasterize_workspace_bytes(faces, w, h),), dtype=torch.uint8, device=dev)
        rc, rs = torch.empty((3,), dtype=torch.int64, device=dev), torch.empty((3,), dtype=torch.float64, device=dev)
        raster = event_ms(lambda: mesh_rasterize_into(mesh, view, counts=rc, stats=rs, pixel_face=face.view(h, w), pixel_depth=t.view(h, w),
                                                      pixel_temperature=temperature.view(h, w), pixel_colors=colors.view(h, w, 3),
                                                      workspace=rws), args.repeats)
        cast_ms.append((faces, closest[0]))

        lines.append(f"{faces:<10d} {depth:<7d} {got[0] / n:<11.4f} {cell(build):<29s} {cell(closest):<30s} {n / closest[0] / 1e3:<9.1f} "
                     f"{cell(any_hit):<30s} {cell(raster)}")
        if got[3] != 0:
            lines.append(f"    {got[3]} rays reached the stack limit")
        del blob, ws, rws
    if len(cast_ms) > 1:
        (f0, m0), (f1, m1) = cast_ms[0], cast_ms[-1]
        lines.append(f"closest-hit cast at {f1} faces / at {f0} faces = {m1 / m0:.2f} x for {f1 / f0:.2f} x the faces (medians above)")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
