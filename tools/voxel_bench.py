#!/usr/bin/env python
"""What voxel down-sampling of the point-cloud export costs: ms per call on the noisy sphere of tools/knn_bench.py at ``--points``
points (default 10^6 and 10^7), each at two voxel sizes that give about 10 and about 100 members per voxel (the measured mean
is printed).

Routes, per (points, voxel size):
  voxel_downsample   the host function: bounding box, ``tn_voxel_downsample`` (keys, ``tn_sort_pairs``, heads, averages), two host reads
  tn_sort_pairs      the sort alone on the same voxel keys over the same key bits (values 0 .. n-1), and once per cloud on uniform random
                     64-bit keys over 64 bits
  torch              what a user would write otherwise: keys in torch, ``torch.sort(stable=True)``, ``unique_consecutive``, fp64
                     ``index_add_`` of positions, colours and temperature, divide.  A yardstick for TIME only: its sums follow the order
                     of arrival, so its output is not defined to the bit.
One warm-up call per route, then ``--passes`` timed calls per route, alternating over the routes so that drift of a shared machine
hits all alike; a call is timed with the host clock around work that ends in a device synchronise.  The report gives the median and
the range per route.  Last, on the largest cloud: ``tn_knn`` as ``--remove-outliers`` calls it (k = 19, mean distance only) before
and after down-sampling at the larger voxel size.  A record, not a gate.

    python tools/voxel_bench.py [--passes 5] [--points 1000000 10000000] [--out profiles/micro/pointcloud_voxel.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# voxel sizes that give 10 / 100 members per occupied voxel on knn_bench.surface(n), found on the host by counting distinct keys
SIZES = {10 ** 6: (0.00475, 0.0145), 10 ** 7: (0.00201, 0.00544)}


def sizes_for(n: int):
    if n in SIZES:
        return SIZES[n]
    return tuple((2.0 * 1.131 * m / n) ** 0.5 for m in (10, 100))  # the sphere's area over the voxel's face, about two layers


def torch_route(cloud, size: float):
    """(positions, colors, temperature, counts) per occupied voxel the way one writes it with torch alone"""
    import numpy as np
    import torch

    p = cloud.positions
    lo = p.amin(dim=0)
    c = ((p.double() - lo.double()) * (1.0 / float(np.float32(size)))).long()  # (the kernel's own coordinate steps)
    dims = c.amax(dim=0) + 1
    keys = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    sorted_keys, order = torch.sort(keys, stable=True)
    _, inverse, counts = torch.unique_consecutive(sorted_keys, return_inverse=True, return_counts=True)
    v = counts.shape[0]
    rows = torch.cat([p.double(), cloud.colors.double(), cloud.temperature.double()[:, None]], dim=1)[order]
    sums = torch.zeros((v, 7), dtype=torch.float64, device=p.device).index_add_(0, inverse, rows)
    mean = sums / counts[:, None].double()
    return mean[:, :3].float(), (mean[:, 3:6] + 0.5).floor().to(torch.uint8), mean[:, 6].float(), counts


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--points", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--no-knn", action="store_true", help="skip the tn_knn before / after line")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from knn_bench import surface

    from thermo_nerf_amd.export import ThermalPointCloud, knn, sort_pairs, voxel_downsample
    from thermo_nerf_amd.export.voxel import voxel_grid

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    head, lines = [], []
    cloud = None
    for n in args.points:
        rng = np.random.default_rng(1)
        cloud = ThermalPointCloud(torch.from_numpy(surface(n)).to("cuda"),
                                  torch.from_numpy(rng.integers(0, 256, (n, 3), dtype=np.uint8)).to("cuda"),
                                  torch.from_numpy(rng.uniform(14.0, 33.0, n).astype(np.float32)).to("cuda"))
        random_keys = torch.from_numpy(rng.integers(0, 2 ** 63, n, dtype=np.int64)).to("cuda")
        routes = {}
        for size in sizes_for(n):
            p = cloud.positions
            lo, hi = p.amin(dim=0).tolist(), p.amax(dim=0).tolist()
            _, dims = voxel_grid(lo, hi, size)
            bits = (dims[0] * dims[1] * dims[2]).bit_length()
            c = ((p.double() - torch.tensor(lo, dtype=torch.float64, device="cuda")) * (1.0 / float(np.float32(size)))).long()
            keys = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
            routes[(size, "voxel_downsample")] = lambda size=size: voxel_downsample(cloud, size)
            routes[(size, f"tn_sort_pairs, {bits} key bits")] = lambda keys=keys, bits=bits: sort_pairs(keys, key_bits=bits)
            routes[(size, "torch sort + unique_consecutive + index_add_")] = lambda size=size: torch_route(cloud, size)
        routes[(0.0, "tn_sort_pairs, random keys, 64 key bits")] = lambda: sort_pairs(random_keys, key_bits=64)
        members = {}
        for (size, name), fn in routes.items():  # warm-up: code objects, the allocator's pools; and the two routes must agree on the voxels
            out = fn()
            torch.cuda.synchronize()
            if name == "voxel_downsample":
                members[size] = n / len(out[0])
                assert int(out[1].sum()) == n
            elif name.startswith("torch"):
                assert n / out[3].shape[0] == members[size], "the torch route finds another number of voxels"
            del out
        times = {route: [] for route in routes}
        for k in range(args.passes):
            for route, fn in routes.items():
                times[route].append(timed(fn))
                lines.append(f"pass {k}  points {n:9d}  voxel size {route[0]:.5f}  {route[1]:46s} {times[route][-1]:10.3f} ms")
                print(lines[-1], flush=True)
        head.append(f"{n} points (sphere of radius 0.3, 0.4 % radial noise, 0.1 % uniform floaters in +-1, shuffled), random colours and "
                    f"temperatures; 1 warm-up + {args.passes} timed calls per route, alternating")
        head.append(" voxel size  members/voxel  route                                            median ms   min .. max")
        for route in routes:
            v = sorted(times[route])
            m = f"{members[route[0]]:13.2f}" if route[0] in members else " " * 13
            head.append(f"{route[0]:11.5f}  {m}  {route[1]:46s} {v[len(v) // 2]:10.3f}   {v[0]:.3f} .. {v[-1]:.3f}")
        head.append("")
        del routes, random_keys
    if not args.no_knn and cloud is not None:
        n, size = len(cloud), sizes_for(len(cloud))[1]
        down, _ = voxel_downsample(cloud, size)
        knn(down.positions, 19, indices=False, distances=False, mean_distance=True)  # warm-up at the small size
        after = timed(lambda: knn(down.positions, 19, indices=False, distances=False, mean_distance=True))
        before = timed(lambda: knn(cloud.positions, 19, indices=False, distances=False, mean_distance=True))
        head.append(f"tn_knn (k = 19, mean distance only: what --remove-outliers runs) on the {n}-point cloud {before:.1f} ms; on the "
                    f"{len(down)} points that --voxel-size {size} leaves of it {after:.1f} ms (one call each after a warm-up call)")
        head.append("")
    report = "\n".join(head + lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
