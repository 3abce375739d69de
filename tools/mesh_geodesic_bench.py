#!/usr/bin/env python
"""What the geodesic distance costs on a mesh of a survey's size: the closed lattice surface of about 2 M faces of
tools/mesh_isolines_bench.py (a torus of ``--side`` x ``--side`` two-triangle cells; no file, no reference data), solved from one
seed and from the hot spots of the bumps field of tools/mesh_hotspots_bench.py — the rounds, the whole solve, the time per round,
and ``tn_mesh_distance_bands`` for 64 bands.

A solve runs from the restart to the round that changes nothing, the host's clock around it with a device synchronise at its end (a
solve reads its 16 bytes of counts between the batches); the queue alone — one call of ``--queue`` rounds after a restart, no host
read — between two device events.

    python tools/mesh_geodesic_bench.py [--side 1024] [--repeats 5] --out profiles/micro/mesh_geodesic.txt

A record, not a gate.
"""
from __future__ import annotations

import argparse
import sys
import time

import mesh_scenes  # the sibling module: event_ms, emit; it puts the repository on sys.path
from mesh_hotspots_bench import bumps  # the sibling module: the torus with its field


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=1024, help="cells along each way around the torus: 2 side^2 faces")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128, help="rounds queued between two reads of the counts")
    ap.add_argument("--queue", type=int, default=256, help="rounds of the call that is timed without a host read")
    ap.add_argument("--min-prominence", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from pmc_summary import head_stamp  # the sibling module
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.export import (distance_profile, geodesic_distance, mesh_distance_bands_workspace_bytes,
                                        mesh_geodesic_workspace_bytes, mesh_incidence, thermal_hotspots)

    dev = torch.device("cuda")
    lib, stream = _hip.load(), _hip.current_stream()
    mesh, v, t = bumps(args.side, dev, 0.0)
    index = mesh_incidence(mesh.triangles, v)
    pos, tri = mesh.positions, mesh.triangles
    need = mesh_geodesic_workspace_bytes(v, t)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    distance, nearest = torch.empty((v,), dtype=torch.float64, device=dev), torch.empty((v,), dtype=torch.int32, device=dev)
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    spots = thermal_hotspots(mesh, args.min_prominence)
    lines = [f"geodesic distance on a closed lattice surface (a torus of {args.side} x {args.side} cells with a relief): {v} vertices, {t} "
             f"triangles; workspace {need / 2 ** 20:.1f} MiB; batches of {args.batch} rounds; {args.repeats} solves",
             f"measured at commit {head_stamp()}"]

    def entry(seed_v, seed_o, restart, rounds):
        _hip.check(lib.tn_mesh_geodesic(pos.data_ptr(), tri.data_ptr(), t, v, index.offsets.data_ptr(), index.corners.data_ptr(),
                                        seed_v.data_ptr(), seed_o.data_ptr(), seed_v.numel(), float("inf"), restart, rounds,
                                        distance.data_ptr(), nearest.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, stream),
                   "tn_mesh_geodesic")

    def solve(seed_v, seed_o):
        """(ms, rounds) of one whole solve"""
        torch.cuda.synchronize()
        start = time.perf_counter()
        restart = 1
        while True:
            entry(seed_v, seed_o, restart, args.batch)
            restart = 0
            rounds, fixed = counts.cpu().tolist()
            if fixed:
                break
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e3, int(rounds)

    def median(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2], xs[0], xs[-1]

    cases = (("one seed (vertex 0)", np.zeros(1, np.int32)), (f"the {len(spots)} hot spots above {args.min_prominence} degrees", spots.peak_vertex))
    for what, seeds in cases:
        seed_v = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.int32)).to(dev)
        seed_o = torch.zeros((len(seeds),), dtype=torch.float64, device=dev)
        solve(seed_v, seed_o)  # warm-up
        times, rounds = [], 0
        for _ in range(args.repeats):
            ms, rounds = solve(seed_v, seed_o)
            times.append(ms)
        result = distance.clone()
        entry(seed_v, seed_o, 1, args.queue)
        torch.cuda.synchronize()
        queue = []
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            entry(seed_v, seed_o, 1, args.queue)
            stop.record()
            stop.synchronize()
            queue.append(start.elapsed_time(stop))
        reached = int(torch.isfinite(result).sum())
        lines += ["", f"from {what}: {rounds} rounds, {reached} of {v} vertices reached, the farthest at "
                      f"{float(result[torch.isfinite(result)].max()):.4f}",
                  "what                                                                            median ms   min .. max"]
        m, q = median(times), median(queue)
        lines.append(f"{'whole solve':76s} {m[0]:11.3f}   {m[1]:.3f} .. {m[2]:.3f}")
        lines.append(f"{'  per round (us)':76s} {1e3 * m[0] / max(rounds, 1):11.2f}   {1e3 * m[1] / max(rounds, 1):.2f} .. {1e3 * m[2] / max(rounds, 1):.2f}")
        lines.append(f"{f'one call: restart + the first {args.queue} rounds, no host read':76s} {q[0]:11.3f}   {q[1]:.3f} .. {q[2]:.3f}")
        lines.append(f"{'  per round (us)':76s} {1e3 * q[0] / args.queue:11.2f}   {1e3 * q[1] / args.queue:.2f} .. {1e3 * q[2] / args.queue:.2f}")
        m = mesh_scenes.event_ms(lambda: geodesic_distance(mesh, seeds, incidence=index), args.repeats)
        lines.append(f"{'geodesic_distance (its allocations, the batches, the host reads)':76s} {m[0]:11.3f}   {m[1]:.3f} .. {m[2]:.3f}")

    d = geodesic_distance(mesh, spots.peak_vertex, incidence=index)
    far = float(d.distance[torch.isfinite(d.distance)].max())
    need_bands = mesh_distance_bands_workspace_bytes(v, t, 64)
    band_ws = torch.empty((need_bands,), dtype=torch.uint8, device=dev)
    m = mesh_scenes.event_ms(lambda: distance_profile(mesh, d, far / 64.0 * 1.001, 64, workspace=band_ws), args.repeats)
    profile = distance_profile(mesh, d, far / 64.0 * 1.001, 64, workspace=band_ws)
    lines += ["", f"tn_mesh_distance_bands, 64 bands over the distance from the hot spots ({profile.banded_faces} of {t} faces banded; workspace "
                  f"{need_bands / 2 ** 20:.1f} MiB), through distance_profile with its one host read",
              f"{'distance_profile':76s} {m[0]:11.3f}   {m[1]:.3f} .. {m[2]:.3f}"]
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
