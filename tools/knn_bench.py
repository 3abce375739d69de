#!/usr/bin/env python
"""What the neighbour search of the point-cloud export costs: ms per ``tn_knn`` call at k = 19 (outlier removal's 20 neighbours)
and k = 30 (the normals) on ``--points`` points (default 10^6: the exporter's default cloud) of a noisy analytic surface — a
sphere of radius 0.3 with 0.4 % radial noise plus 0.1 % of points uniform in the +-1 box, the floaters the filter is for.

Routes: one per (k, grid_resolution) with grid_resolution from ``--resolutions`` (0 = the library's own choice, printed).
One warm-up call per route, then ``--passes`` timed calls per route, alternating over the routes so that drift of a shared
machine hits all alike; a call is timed with the host clock around work that ends in a device synchronise.  The report gives
the median and the range per route, and for context (not a pass mark) the wall time of ``scipy.spatial.cKDTree.query`` with 16
workers on the same points.  A record, not a gate.

    python tools/knn_bench.py [--passes 5] [--points 1000000] [--resolutions 0 48 64 100 128 160 200] [--out profiles/micro/pointcloud_knn.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
KS = (19, 30)


def surface(num_points: int, seed: int = 0):
    import numpy as np

    rng = np.random.default_rng(seed)
    floaters = num_points // 1000
    d = rng.normal(size=(num_points - floaters, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (0.3 * (1.0 + 0.004 * rng.normal(size=(len(d), 1))))
    p = np.concatenate([p, rng.uniform(-1.0, 1.0, (floaters, 3))])
    return rng.permutation(p).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[0, 48, 64, 100, 128, 160, 200])
    ap.add_argument("--no-scipy", action="store_true", help="skip the cKDTree context line")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd.export import knn, knn_grid_resolution, knn_workspace_bytes

    host = surface(args.points)
    pos = torch.from_numpy(host).to("cuda")
    n = pos.shape[0]
    routes = [(k, r) for k in KS for r in args.resolutions]
    workspace = torch.empty((max(knn_workspace_bytes(n, r) for r in args.resolutions),), dtype=torch.uint8, device="cuda")
    check = {}

    def call(k, r):
        out = knn(pos, k, grid_resolution=r, mean_distance=True, workspace=workspace)
        torch.cuda.synchronize()
        return out

    for k, r in routes:  # warm-up: code objects, the allocator's pools; and the outputs must not depend on the resolution
        out = call(k, r)
        sums = (int(out.indices.long().sum()), float(out.distances.double().sum()))
        assert check.setdefault(k, sums) == sums, f"k = {k}: resolution {r} gives another result"
    times = {route: [] for route in routes}
    lines = []
    for p in range(args.passes):
        for route in routes:
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(*route)
            times[route].append((time.perf_counter() - t) * 1e3)
            lines.append(f"pass {p}  k {route[0]:2d}  resolution {route[1]:3d}  {times[route][-1]:9.3f} ms")
            print(lines[-1], flush=True)
    head = [f"tn_knn on {n} points (sphere of radius 0.3, 0.4 % radial noise, 0.1 % uniform floaters in +-1, shuffled), indices + d2 + mean "
            f"distance; grid_resolution 0 chooses {knn_grid_resolution(n)}; 1 warm-up + {args.passes} timed calls per route, alternating",
            " k  resolution   median ms   min .. max"]
    for route in routes:
        v = sorted(times[route])
        head.append(f"{route[0]:2d}  {route[1]:10d}  {v[len(v) // 2]:10.3f}   {v[0]:.3f} .. {v[-1]:.3f}")
    if not args.no_scipy:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            head.append("context: scipy is not installed here, no cKDTree line")
        else:
            t = time.perf_counter()
            tree = cKDTree(host)
            built = time.perf_counter() - t
            for k in KS:
                t = time.perf_counter()
                tree.query(host, k=k + 1, workers=16)  # (the point itself comes first)
                head.append(f"context: scipy cKDTree.query(k = {k} + self, workers = 16) {1e3 * (time.perf_counter() - t):.0f} ms "
                            f"after a {1e3 * built:.0f} ms build, on the host")
    report = "\n".join(head + [""] + lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
