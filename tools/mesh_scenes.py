"""What the mesh timing scripts (tools/mesh_*_bench.py) share: the synthetic scenes they time on — the TSDF volume of an analytic
sphere, the room of jittered lattices seen from inside with its camera —, the event-timing loop and the tail that prints and
writes a report.  Imported as a sibling module by scripts started as ``python tools/mesh_..._bench.py``; not a command line."""
from __future__ import annotations

import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
RADIUS, HALF, TRUNCATION_STEPS = 0.3, 0.5, 4.0


def event_ms(fn, repeats: int, calls: int = 1):
    """(median, min, max) ms per call of ``fn``: 3 warm-up calls, then ``repeats`` windows of ``calls`` back-to-back calls, each window
    between two device events"""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / calls)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def cell(ms) -> str:
    """a (median, min, max) of ``event_ms`` as a report's cell"""
    return f"{ms[0]:8.4f} ({ms[1]:.4f} .. {ms[2]:.4f})"


def emit(lines, out) -> None:
    """print the report and, with ``out``, write it there"""
    report = "\n".join(lines) + "\n"
    print(report)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(report)


def sphere_volume(n: int, dev):
    """(volume [7, n, n, n], params): tsdf = clamp((|p| - RADIUS) / truncation, -1, 1) with weight 1, thermal (z / RADIUS + 1) / 2"""
    import torch

    from thermo_nerf_amd.export import mesh_params

    step = 2 * HALF / (n - 1)
    truncation = TRUNCATION_STEPS * step
    g = torch.linspace(-HALF, HALF, n, device=dev)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    volume = torch.zeros((7, n, n, n), dtype=torch.float32, device=dev)
    volume[0] = (((x * x + y * y + z * z).sqrt() - RADIUS) / truncation).clamp(-1.0, 1.0)
    volume[1] = 1.0
    volume[2] = ((z / RADIUS + 1.0) / 2.0).clamp(0.0, 1.0)
    volume[3], volume[4], volume[5], volume[6] = 0.25, 0.5, 0.75, 1.0
    return volume, mesh_params((-HALF,) * 3, (HALF,) * 3, (n,) * 3, truncation, max_temperature=33.0, min_temperature=14.0), step


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


def room_camera(width: int, height: int):
    """the ``CameraView`` the ray-cast and closest-point timings look through: from a corner of the room across it"""
    from thermo_nerf_amd.export import CameraView

    return CameraView(look_at((5.4, 3.5, 2.3), (1.6, 1.2, 0.5)), 0.8 * width, 0.8 * width, width / 2.0, height / 2.0, width, height)
