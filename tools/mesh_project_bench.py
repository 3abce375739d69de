#!/usr/bin/env python
"""What projecting the photos onto a mesh costs: ``tn_mesh_project`` through its raw wrapper into preallocated buffers — every output
array, the counts and the statistics — on the vertices of the room of ``tools/mesh_raycast_bench.py`` (``--cells`` 252: about
1 000 000 faces, about 500 000 vertices) with their ``vertex_normals``, under ``--cameras`` pinhole cameras on a ring inside the room
with random-byte photos of ``--width`` x ``--height``.  Beside it the same result COMPOSED from the public API as it stood before the
kernel: one ``visible_from`` call per camera (an occlusion ray for every vertex) and torch fp64 arithmetic over [V] and [V, 3]
temporaries for the projection, the facing test, the bilinear sample and the weighted sums, cameras in ascending order.  The
composition lives here only; it is checked against the kernel in the same run (the views agree on all but a handful of pairs that sit
on a clause's edge, where torch's sums round otherwise; the measured degrees agree to float rounding where the views do).  Device
events around each call; 3 warm-up calls each, then ``--repeats`` rounds that alternate the two; median and range.  A record, not a
gate.

    python tools/mesh_project_bench.py [--cells 252] [--cameras 100] [--width 640 --height 480] [--repeats 7]
           [--out profiles/micro/mesh_project.txt]
"""
from __future__ import annotations

import argparse
import math
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path


def ring_cameras(count: int, width: int, height: int, look_at):
    """``count`` CameraView on a ring inside the 6 x 4 x 3 room, each looking across it"""
    from thermo_nerf_amd.export import CameraView

    views = []
    for k in range(count):
        a = 2.0 * math.pi * k / count
        eye = (3.0 + 2.2 * math.cos(a), 2.0 + 1.3 * math.sin(a), 1.2 + 0.8 * math.sin(3.0 * a))
        target = (3.0 - 2.5 * math.cos(a + 0.4), 2.0 - 1.6 * math.sin(a + 0.4), 1.0 + 0.6 * math.cos(5.0 * a))
        views.append(CameraView(look_at(eye, target), 0.7 * width, 0.7 * width, width / 2.0, height / 2.0, width, height))
    return views


def composed(bvh, points, normals, own, records, rotations, images, bounds, min_cos):
    """the projection composed from ``visible_from`` and torch: (measured, views, best_camera, spread, difference)"""
    import torch

    from thermo_nerf_amd.export import visible_from

    lo, hi = bounds
    count, dev = points.shape[0], points.device
    height, width = images.shape[1:]
    n64 = normals.double()
    nlen = n64.norm(dim=1)
    sw, swt = torch.zeros(count, dtype=torch.float64, device=dev), torch.zeros(count, dtype=torch.float64, device=dev)
    low, high = torch.full_like(sw, math.inf), torch.full_like(sw, -math.inf)
    best_w, best = torch.zeros_like(sw), torch.full((count,), -1, dtype=torch.int32, device=dev)
    views = torch.zeros(count, dtype=torch.int32, device=dev)
    for k in range(len(records)):
        c = records[k]
        eye = [float(c[3]), float(c[7]), float(c[11])]
        seen = visible_from(bvh, points, eye)
        d = (points - torch.tensor(eye, dtype=torch.float32, device=dev)).double()
        cam = d @ rotations[k]
        z = -cam[:, 2]
        u = float(c[12]) * (cam[:, 0] / z) + float(c[14])
        v = float(c[15]) - float(c[13]) * (cam[:, 1] / z)
        dist2 = (d * d).sum(dim=1)
        cos = -(n64 * d).sum(dim=1) / (dist2.sqrt() * nlen)
        ok = seen & (z > 0) & (u >= 0.5) & (u <= width - 0.5) & (v >= 0.5) & (v <= height - 0.5) & (cos >= min_cos)
        a, b = torch.where(ok, u - 0.5, 0.0), torch.where(ok, v - 0.5, 0.0)
        x0, y0 = a.floor().clamp(0, width - 2).long(), b.floor().clamp(0, height - 2).long()
        fa, fb = a - x0, b - y0
        photo = images[k].double()
        top = photo[y0, x0] + fa * (photo[y0, x0 + 1] - photo[y0, x0])
        bottom = photo[y0 + 1, x0] + fa * (photo[y0 + 1, x0 + 1] - photo[y0 + 1, x0])
        t = lo + ((top + fb * (bottom - top)) / 255.0) * (hi - lo)
        w = torch.where(ok, cos / dist2, 0.0)
        sw += w
        swt += w * t
        low, high = torch.where(ok & (t < low), t, low), torch.where(ok & (t > high), t, high)
        better = ok & (w > best_w)
        best_w, best = torch.where(better, w, best_w), torch.where(better, k, best).int()
        views += ok.int()
    measured = (swt / sw).float()
    return measured, views, best, torch.where(views > 0, (high - low).float(), torch.full_like(measured, math.nan)), (own.double() - measured.double()).float()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cells", type=int, default=252, help="cells per side of a wall: 12 cells^2 faces and the boxes'")
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import ThermalMesh, build_mesh_bvh, camera_records, project_images_into, vertex_normals

    dev = torch.device("cuda")
    pos, temp, col, tri = mesh_scenes.room(args.cells, 1, dev)
    mesh = ThermalMesh(pos, col, temp, None, tri)
    bvh = build_mesh_bvh(mesh)
    normals = vertex_normals(pos, tri)
    count, faces, k = int(pos.shape[0]), int(tri.shape[0]), args.cameras
    records, width, height = camera_records(ring_cameras(k, args.width, args.height, mesh_scenes.look_at))
    table = torch.from_numpy(records).to(dev)
    rotations = [torch.from_numpy(records[i, :12].reshape(3, 4)[:, :3].copy()).double().to(dev) for i in range(k)]
    gen = torch.Generator(device="cpu").manual_seed(11)
    images = torch.randint(0, 256, (k, height, width), generator=gen, dtype=torch.uint8).to(dev)
    bounds, min_cos = (10.0, 40.0), 0.2
    measured, spread, difference = (torch.empty((count,), device=dev) for _ in range(3))
    views, best = torch.empty((count,), dtype=torch.int32, device=dev), torch.empty((count,), dtype=torch.int32, device=dev)
    counts, stats = torch.empty((6,), dtype=torch.int64, device=dev), torch.empty((8,), dtype=torch.float64, device=dev)

    def fused():
        project_images_into(bvh, pos, normals, table, images, bounds, point_temperature=temp, min_cos=min_cos, measured=measured, views=views,
                            best_camera=best, spread=spread, difference=difference, counts=counts, stats=stats)

    def baseline():
        return composed(bvh, pos, normals, temp, records, rotations, images, bounds, min_cos)

    for _ in range(3):
        fused()
        other = baseline()
    torch.cuda.synchronize()
    got = counts.cpu().tolist()
    assert got[5] == 0 and got[2] == k, got
    differ = int((other[1] != views).sum())
    same = (other[1] == views) & (views > 0)
    worst = float((other[0][same].double() - measured[same].double()).abs().max()) if bool(same.any()) else 0.0
    assert differ <= 1e-3 * max(got[4], 1) and worst <= 1e-3, (differ, worst)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    a, b = [], []
    for _ in range(args.repeats):  # the two alternate: what else the device does meanwhile falls on both
        a.append(timed(fused))
        b.append(timed(baseline))
    a.sort(), b.sort()

    def cell(ms):
        return f"{ms[len(ms) // 2]:9.3f} ({ms[0]:.3f} .. {ms[-1]:.3f})"

    fa, fb = a[len(a) // 2], b[len(b) // 2]
    pairs = got[1] * got[2]
    lines = [f"tn_mesh_project on the vertices of the room of mesh_raycast_bench: V = {count} points, T = {faces} faces, K = {k} cameras, photos "
             f"{width} x {height}, min_cos {min_cos}, every output array, the counts and the statistics written; beside it the same result "
             f"composed from K visible_from calls and torch fp64 arithmetic; device events around each call, 3 warm-up calls each, "
             f"{args.repeats} alternating timed calls, ms per call (median, min .. max)",
             f"fused ms                          composed ms                        composed / fused   pairs        tested pairs  accepted pairs  "
             f"accepted share  Mpairs/s fused  Mpairs/s composed",
             f"{cell(a):<33s} {cell(b):<34s} {fb / fa:<18.2f} {pairs:<12d} {got[3]:<13d} {got[4]:<15d} {got[4] / max(pairs, 1):<15.4f} "
             f"{pairs / fa / 1e3:<15.1f} {pairs / fb / 1e3:.1f}",
             f"seen vertices {got[0]} of {count}; views differing between the two: {differ} of {count} vertices; largest |measured| difference "
             f"where the views agree: {worst:.3g} C"]
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
