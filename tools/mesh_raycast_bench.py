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
import importlib.util
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _simplify_bench():
    spec = importlib.util.spec_from_file_location("mesh_simplify_bench", os.path.join(ROOT, "tools", "mesh_simplify_bench.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def lattice_box(lo, hi, cells: int, inward: bool, jitter: float, gen):
    """the six sides of an axis-aligned box as lattices of ``cells`` x ``cells`` two-triangle cells, the inner vertices of every side
    moved by ``jitter`` of a cell inside its plane: (positions float64 [V, 3], triangles int64 [T, 3]) on the host"""
    import torch

    positions, triangles, base = [], [], 0
    g = torch.linspace(0.0, 1.0, cells + 1, dtype=torch.float64)
    ga, gb = torch.meshgrid(g, g, indexing="ij")
    inner = ((ga > 0) & (ga < 1) & (gb > 0) & (gb < 1)).double()
    i, j = torch.meshgrid(torch.arange(cells), torch.arange(cells), indexing="ij")
    for axis in range(3):
        for side in range(2):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            shift = (torch.rand((2, cells + 1, cells + 1), generator=gen, dtype=torch.float64) - 0.5) * jitter / cells
            p = torch.zeros((cells + 1, cells + 1, 3), dtype=torch.float64)
            p[..., axis] = hi[axis] if side else lo[axis]
            p[..., a] = lo[a] + (ga + inner * shift[0]) * (hi[a] - lo[a])
            p[..., b] = lo[b] + (gb + inner * shift[1]) * (hi[b] - lo[b])
            v00 = base + i * (cells + 1) + j
            v10, v01, v11 = v00 + cells + 1, v00 + 1, v00 + cells + 2
            quads = torch.stack([torch.stack([v00, v10, v11], -1), torch.stack([v00, v11, v01], -1)], -2).reshape(-1, 3)
            if bool(side) == bool(inward):
                quads = quads[:, [0, 2, 1]]
            positions.append(p.reshape(-1, 3))
            triangles.append(quads)
            base += (cells + 1) ** 2
    return torch.cat(positions), torch.cat(triangles)


def room(cells: int, seed: int, dev):
    """the room with five boxes in it, 12 cells^2 + 5 * 12 (cells / 4)^2 faces: (positions, temperature, colors, triangles)"""
    import torch

    gen = torch.Generator(device="cpu").manual_seed(seed)
    parts = [lattice_box((0.0, 0.0, 0.0), (6.0, 4.0, 3.0), cells, True, 0.6, gen)]
    for corner, size in (((0.5, 0.5, 0.0), (1.0, 0.8, 1.1)), ((2.2, 2.6, 0.0), (0.7, 0.9, 1.9)), ((3.6, 0.6, 0.0), (1.2, 1.2, 0.6)),
                         ((0.6, 2.4, 0.0), (0.8, 1.0, 0.9)), ((4.6, 2.5, 0.0), (0.9, 0.9, 1.4))):
        hi = tuple(c + s for c, s in zip(corner, size))
        parts.append(lattice_box(corner, hi, max(cells // 4, 1), False, 0.6, gen))
    positions, triangles, base = [], [], 0
    for p, t in parts:
        positions.append(p)
        triangles.append(t + base)
        base += p.shape[0]
    pos = torch.cat(positions)
    temp = 21.0 + 5.0 * torch.sin(pos[:, 0] * 1.7) * torch.cos(pos[:, 1] * 2.3) + 1.5 * pos[:, 2]
    colors = (torch.rand((pos.shape[0], 3), generator=gen) * 255).to(torch.uint8)
    return pos.float().to(dev), temp.float().to(dev), colors.to(dev), torch.cat(triangles).int().to(dev)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """3 x 4 camera-to-world rows in nerfstudio's convention (the camera looks along its -z, +y is up)"""
    def sub(a, b):
        return [x - y for x, y in zip(a, b)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def unit(a):
        n = math.sqrt(sum(x * x for x in a))
        return [x / n for x in a]

    back = unit(sub(eye, target))
    right = unit(cross(up, back))
    true_up = cross(back, right)
    return [[right[k], true_up[k], back[k], eye[k]] for k in range(3)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--cells", type=int, nargs="+", default=[126, 252], help="cells per side of a wall: 12 cells^2 faces and the boxes'")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import (CameraView, MeshBVH, RasterView, ThermalMesh, camera_rays, mesh_bvh_bytes, mesh_bvh_workspace_bytes,
                                        build_mesh_bvh, mesh_raycast_into, mesh_rasterize_into, mesh_rasterize_workspace_bytes)

    event_ms = _simplify_bench().event_ms
    dev = torch.device("cuda")
    w, h = args.width, args.height
    n = w * h
    camera = CameraView(look_at((5.4, 3.5, 2.3), (1.6, 1.2, 0.5)), 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, w, h)
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
        pos, temp, col, tri = room(cells, 1, dev)
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

        def cell(ms):
            return f"{ms[0]:8.4f} ({ms[1]:.4f} .. {ms[2]:.4f})"

        lines.append(f"{faces:<10d} {depth:<7d} {got[0] / n:<11.4f} {cell(build):<29s} {cell(closest):<30s} {n / closest[0] / 1e3:<9.1f} "
                     f"{cell(any_hit):<30s} {cell(raster)}")
        if got[3] != 0:
            lines.append(f"    {got[3]} rays reached the stack limit")
        del blob, ws, rws
    if len(cast_ms) > 1:
        (f0, m0), (f1, m1) = cast_ms[0], cast_ms[-1]
        lines.append(f"closest-hit cast at {f1} faces / at {f0} faces = {m1 / m0:.2f} x for {f1 / f0:.2f} x the faces (medians above)")
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
