#!/usr/bin/env python
"""What an iteration of the registration costs: ``tn_mesh_register`` through its raw wrapper into preallocated buffers, device events
around each call, on the room of ``tools/mesh_raycast_bench.py`` at its two face counts (about 250 000 and about 1 000 000 faces).  The
cloud is the room's own vertices under a small known similarity (0.02 rad, 1 % of the extent, 1 % in size): the mesh-to-mesh case
of two surveys.  Point to plane, with scale.  Beside the fused iteration, timed in the same run:

  (a) a bare ``tn_mesh_closest`` call on the same points at the starting pose with only the face and the point written — the walk's
      floor: what finding the pairs costs when nothing is done with them;
  (b) the same iteration composed from ``mesh_closest_into``, torch fp64 arithmetic and sums and a host solve — the only route
      without the fused kernel: seven arrays per iteration that nobody reads, and one host synchronisation.

The fused call is timed with 1 iteration (one walk, one finish, the memset) and with ``--iterations`` of them (tolerance 0, so none
ends the run early), the composed one per iteration.  3 warm-up calls, then ``--repeats`` timed calls each; median and range.  A
record, not a gate.

    python tools/mesh_register_bench.py [--repeats 21] [--iterations 8] [--out profiles/micro/mesh_register.txt]
"""
from __future__ import annotations

import argparse
import sys

import mesh_scenes  # the sibling module: the scenes, event_ms, emit; it puts the repository on sys.path


def small_similarity(center):
    """4 x 4: 0.02 rad about (1, -1, 1) / sqrt 3, 1 % larger, moved by 1 % of the room's largest extent, about ``center``"""
    import numpy as np

    w = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    r = np.eye(3) + np.sin(0.02) * k + (1.0 - np.cos(0.02)) * (k @ k)
    c = np.asarray(center, np.float64)
    out = np.eye(4)
    out[:3, :3] = 1.01 * r
    out[:3, 3] = c - 1.01 * r @ c + np.array([0.06, -0.04, 0.03])
    return out


def cayley_update(matrix, delta, center):
    """the header's update on the host (numpy, for the composed route)"""
    import numpy as np

    a = 0.5 * delta[:3]
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    u = (1.0 + delta[6]) * (np.eye(3) + 2.0 / (1.0 + a @ a) * (k + k @ k))
    out = matrix.copy()
    out[:, :3] = u @ matrix[:, :3]
    out[:, 3] = center + u @ (matrix[:, 3] - center) + delta[3:6]
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--cells", type=int, nargs="+", default=[126, 252], help="cells per side of a wall: 12 cells^2 faces and the boxes'")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from thermo_nerf_amd.export import (ThermalMesh, build_mesh_bvh, mesh_closest_into, register_points_into, register_workspace_bytes)

    event_ms = mesh_scenes.event_ms
    dev = torch.device("cuda")
    k, damping, radius = args.iterations, 1e-6, 0.25
    lines = [f"tn_mesh_register on the room of mesh_raycast_bench, the cloud its own vertices under a small similarity (0.02 rad, 1 % "
             f"in size, 0.06 / 0.04 / 0.03 units), point to plane with scale, max_distance {radius}, damping {damping}; beside it (a) a "
             f"bare tn_mesh_closest on the same points at the start with the face and the point written, (b) the same iteration composed "
             f"from mesh_closest_into, torch fp64 sums and a host solve; device events around each call, 3 warm-up calls, {args.repeats} "
             f"timed calls, ms (median, min .. max)",
             f"faces      points    fused, 1 iteration ms           fused, {k} iterations: ms / iteration   (a) closest ms                  "
             f"(b) composed iteration ms       fused / (a)   (b) / fused   matched   |fused - composed| after 1"]
    for cells in args.cells:
        pos, temp, col, tri = mesh_scenes.room(cells, 1, dev)
        mesh = ThermalMesh(pos, col, temp, None, tri)
        faces, n = int(tri.shape[0]), int(pos.shape[0])
        bvh = build_mesh_bvh(mesh)
        box = bvh.tree()
        lo, hi = np.array(box["lo"], np.float64), np.array(box["hi"], np.float64)
        center, length = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
        truth = small_similarity(center)
        inverse = np.linalg.inv(truth)
        cloud = (pos.double() @ torch.from_numpy(inverse[:3, :3].T.copy()).to(dev) + torch.from_numpy(inverse[:3, 3].copy()).to(dev)).float().contiguous()
        start = torch.from_numpy(np.eye(4)[:3].reshape(12).copy()).to(dev)
        transform = torch.empty((12,), dtype=torch.float64, device=dev)
        history = torch.empty((4 * k,), dtype=torch.float64, device=dev)
        result = torch.empty((4,), dtype=torch.int64, device=dev)
        workspace = torch.empty((register_workspace_bytes(n),), dtype=torch.uint8, device=dev)

        def fused(iterations):
            transform.copy_(start)
            register_points_into(bvh, cloud, transform, history, result, max_distance=radius, center=tuple(center), length=length, metric="plane",
                                 with_scale=True, iterations=iterations, tolerance=0.0, damping=damping, min_pairs=6, workspace=workspace)

        one = event_ms(lambda: fused(1), args.repeats)
        after_one = transform.cpu().numpy().reshape(3, 4)
        matched = int(result.cpu()[2])
        many = event_ms(lambda: fused(k), args.repeats)
        status, ran = result.cpu().tolist()[:2]
        assert (status, ran) == (1, k), (status, ran)
        error = float(np.abs(transform.cpu().numpy().reshape(3, 4) - truth[:3]).max())

        face = torch.empty((n,), dtype=torch.int32, device=dev)
        where = torch.empty((n, 3), device=dev)
        floor = event_ms(lambda: mesh_closest_into(bvh, cloud, max_distance=radius, closest_face=face, closest_point=where), args.repeats)

        cloud64, pos64, tri64 = cloud.double(), pos.double(), tri.long()
        center_d = torch.from_numpy(center.copy()).to(dev)
        weights = np.array([length * length] * 3 + [1.0] * 3 + [length * length])

        def composed(matrix):
            m = torch.from_numpy(matrix.copy()).to(dev)
            x = cloud64 @ m[:, :3].T + m[:, 3]
            mesh_closest_into(bvh, x.float().contiguous(), max_distance=radius, closest_face=face, closest_point=where)
            found = face >= 0
            corner = pos64[tri64[face.clamp_min(0).long()]]
            normal = torch.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0], dim=1)
            normal = normal / normal.norm(dim=1, keepdim=True)
            y = x - center_d
            g = torch.cat([torch.cross(y, normal, dim=1), normal, (normal * y).sum(dim=1, keepdim=True)], dim=1) * found[:, None]
            r = (normal * (x - where.double())).sum(dim=1) * found
            sums = torch.cat([(g.T @ g).reshape(-1), g.T @ r, found.sum().double().reshape(1)]).cpu().numpy()  # the host synchronisation
            a, b, count = sums[:49].reshape(7, 7), sums[49:56], sums[56]
            delta = np.linalg.solve(a + np.diag(damping * count * weights), -b)
            return cayley_update(matrix, delta, center)

        identity = np.eye(4)[:3]
        split = event_ms(lambda: composed(identity), args.repeats)
        apart = float(np.abs(composed(identity) - after_one).max())

        def cell(ms, per=1):
            return f"{ms[0] / per:8.4f} ({ms[1] / per:.4f} .. {ms[2] / per:.4f})"

        lines.append(f"{faces:<10d} {n:<9d} {cell(one):<31s} {cell(many, k):<38s} {cell(floor):<31s} {cell(split):<31s} "
                     f"{one[0] / floor[0]:<13.2f} {split[0] / (many[0] / k):<13.2f} {matched:<9d} {apart:.3g}")
        lines.append(f"           after {k} fused iterations: max |entry| of the transform minus the known similarity {error:.3g}")
        del bvh
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
