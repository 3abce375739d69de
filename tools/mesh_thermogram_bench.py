#!/usr/bin/env python
"""What an orthographic thermogram costs: the raw ``tn_mesh_rasterize`` entry into preallocated outputs, device events around each
call, on two scenes at 2048 x 2048 pixels —

(a) a TSDF-like sheet: a jittered 724 x 724 vertex lattice, 1 045 458 faces of one to a few pixels (every face takes the one-thread
    path), every pixel covered once;
(b) 1000 right triangles of about 10^4 pixels each (legs of 141 pixels) at random places and depths — once with the small / large
    threshold as built (every face is swept in 16 x 16 tiles by blocks of 256 threads), once with the threshold raised to the whole
    image so that every face is rasterised by its own thread.  The large-face path stays in the library only if it is clearly faster.

Beside the times: the bytes each pass has to move at the least, and what those would cost at the rate of a plain device copy measured
in the same run (``dst.copy_(src)`` of 256 MiB: read + write).  3 warm-up calls, then ``--repeats`` timed calls each; median and range.
A record, not a gate.

    python tools/mesh_thermogram_bench.py [--side 2048] [--repeats 21] [--out profiles/micro/mesh_thermogram.txt]
"""
from __future__ import annotations

import argparse
import math
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path


def sheet(n: int, side: int, depth: float, seed: int, dev):
    """an n x n vertex lattice over the image with seeded jitter, two faces per cell: (positions, temperature, colors, triangles)"""
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    step = (side - 4.0) / (n - 1)
    a, b = torch.meshgrid(torch.arange(n, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij")
    jitter = torch.rand((n, n, 3), generator=g, dtype=torch.float64) - 0.5
    inner = ((a > 0) & (a < n - 1) & (b > 0) & (b < n - 1)).double()
    x, y = 2.0 + step * (a + 0.6 * inner * jitter[..., 0]), 2.0 + step * (b + 0.6 * inner * jitter[..., 1])
    z = depth + 0.3 * torch.sin(x / 70.0) * torch.cos(y / 50.0) + 0.05 * jitter[..., 2]
    pos = torch.stack([x, y, z], dim=-1).reshape(-1, 3).float()
    k = (torch.arange(n).reshape(-1, 1) * n + torch.arange(n).reshape(1, -1))[:-1, :-1].reshape(-1)
    tri = torch.stack([torch.stack([k, k + n, k + n + 1], 1), torch.stack([k, k + n + 1, k + 1], 1)], 1).reshape(-1, 3).int()
    temp = (22.0 + 6.0 * torch.sin(x / 90.0) + 2.0 * jitter[..., 2]).reshape(-1).float()
    colors = (torch.rand((n * n, 3), generator=g) * 255).to(torch.uint8)
    return pos.to(dev), temp.to(dev), colors.to(dev), tri.to(dev)


def triangles(count: int, leg: float, side: int, seed: int, dev):
    """``count`` right triangles with legs of ``leg`` pixels at seeded places inside the image and seeded depths"""
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    corner = torch.rand((count, 2), generator=g, dtype=torch.float64) * (side - leg - 2.0) + 1.0
    z = 2.0 + 4.0 * torch.rand((count, 3), generator=g, dtype=torch.float64)
    p0 = torch.cat([corner, z[:, :1]], 1)
    p1 = torch.cat([corner + torch.tensor([leg, 0.0]), z[:, 1:2]], 1)
    p2 = torch.cat([corner + torch.tensor([0.0, leg]), z[:, 2:3]], 1)
    pos = torch.stack([p0, p1, p2], 1).reshape(-1, 3).float()
    tri = torch.arange(3 * count).reshape(-1, 3).int()
    temp = (15.0 + 20.0 * torch.rand((3 * count,), generator=g)).float()
    colors = (torch.rand((3 * count, 3), generator=g) * 255).to(torch.uint8)
    return pos.to(dev), temp.to(dev), colors.to(dev), tri.to(dev)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import (RasterView, ThermalMesh, mesh_raster_small_box, mesh_rasterize_into,
                                        mesh_rasterize_workspace_bytes)

    event_ms = mesh_scenes.event_ms
    dev = torch.device("cuda")
    side = args.side
    pixels = side * side
    view = RasterView((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 1.0, side, side)
    counts, stats = torch.empty((3,), dtype=torch.int64, device=dev), torch.empty((3,), dtype=torch.float64, device=dev)
    face = torch.empty((pixels,), dtype=torch.int32, device=dev)
    depth, temperature = torch.empty((pixels,), device=dev), torch.empty((pixels,), device=dev)
    colors = torch.empty((pixels, 3), dtype=torch.uint8, device=dev)

    # the yardstick: a plain device copy, read + write
    n_copy = 256 << 20
    src, dst = torch.empty((n_copy,), dtype=torch.uint8, device=dev), torch.empty((n_copy,), dtype=torch.uint8, device=dev)
    c = event_ms(lambda: dst.copy_(src), args.repeats)
    rate = 2.0 * n_copy / (c[0] * 1e-3)  # bytes per second, read and written
    del src, dst

    lines = [f"tn_mesh_rasterize at {side} x {side} pixels, all four pixel arrays written; device events around each call, 3 warm-up calls, "
             f"{args.repeats} timed calls, ms per call; small box {mesh_raster_small_box()} pixels",
             f"device copy of 256 MiB: {c[0]:.4f} ms ({c[1]:.4f} .. {c[2]:.4f}) = {rate / 1e12:.2f} TB/s read + written",
             "scene                                                                        faces   samples/covered   median ms   min .. max     "
             "least bytes   at copy rate"]

    def run(name, mesh, small_box=0):
        m = ThermalMesh(mesh[0], mesh[2], mesh[1], None, mesh[3])
        t, v = int(mesh[3].shape[0]), int(mesh[0].shape[0])
        ws = torch.empty((mesh_rasterize_workspace_bytes(t, side, side),), dtype=torch.uint8, device=dev)

        def call():
            mesh_rasterize_into(m, view, counts=counts, stats=stats, pixel_face=face, pixel_depth=depth, pixel_temperature=temperature,
                                pixel_colors=colors, workspace=ws, small_box=small_box)

        ms = event_ms(call, args.repeats)
        covered = int(counts[0])
        # at the least, pass by pass: the key plane is cleared; every face's indices are read and its record and flags written, every
        # vertex read once, a key hit once per covered pixel (by the face pass or by the sweep, which reads the large faces' records);
        # the resolve pass reads the plane, once the record of every face shown and its three vertices' temperature and colour, and
        # writes the four arrays and a partial per 256 pixels
        shown = int(torch.unique(face[face >= 0]).numel())
        large = t if small_box == 0 and t <= 1000 else 0  # (scene (b) as built: every face is large; scene (a): none)
        passes = {"clear": pixels * 8, "faces": t * (12 + 72 + 4) + v * (12 + 4) + (0 if large else covered * 8),
                  "sweep": large * (4 + 72) + (covered * 8 if large else 0),
                  "resolve": pixels * 8 + shown * (72 + 3 * (4 + 3)) + pixels * (4 + 4 + 4 + 3) + (pixels // 256) * 24}
        least = sum(passes.values())
        lines.append(f"{name:74s} {t:9d} {covered:17d} {ms[0]:11.4f}   {ms[1]:.4f} .. {ms[2]:.4f} {least / 2 ** 20:9.1f} MiB {least / rate * 1e3:9.4f} ms")
        lines.append("    least bytes by pass: " + ", ".join(f"{k} {b / 2 ** 20:.1f} MiB = {b / rate * 1e6:.1f} us" for k, b in passes.items()))
        return ms

    n = int(round(math.sqrt(1.0e6 / 2.0))) + 17  # 724 at the default: 1 045 458 faces
    run(f"(a) sheet of {n} x {n} vertices, faces of a few pixels", sheet(n, side, 4.0, 1, dev))
    big = triangles(1000, 141.0, side, 2, dev)
    swept = run("(b) 1000 faces of ~10^4 pixels, swept in tiles (as built)", big)
    alone = run("(b) the same, every face by its own thread (threshold 16384)", big, small_box=16384)
    lines.append(f"(b) one thread per face / swept in tiles = {alone[0] / swept[0]:.1f} x (ranges above)")
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
