#!/usr/bin/env python
"""Measure along the surface of a thermal mesh: the geodesic distance from a set of seeds to every vertex of a PLY that
``tools/export_mesh.py`` wrote — the tape measure between two picked points, the surface within a distance of a hot spot or of a
warm region, and the decay profile: how the degrees Celsius fall off with the distance.  No run directory and no model.

    python tools/mesh_distance.py mesh.ply (--from-vertex N ... | --from-point x y z | --from-hotspots P [--top N] [--coldest]
           | --from-min-temperature T | --from-max-temperature T) [--max-distance D] [--to-point x y z]
           [--band-width W --bands K --profile profile.csv] [--length-scale L] [--report distance.json] [--output distance.ply]

The seeds: vertices by number; a picked point, placed on its closest face (the distance is then exact on a plane); the peaks of
the hot spots that stand out by more than P degrees (``--coldest``: the cold spots; ``--top N``: the N most prominent); or every vertex
of the faces at least / at most T degrees warm.  Several sources add up to one set of seeds.  ``--to-point`` is the tape measure's other
end.  ``--profile`` writes one line per band of W units of distance (seed, band, from, to, area, mean / min / max degrees), for the
whole mesh (seed -1) and, with up to 256 seeds, for every seed's own cell — the vertices nearer to it than to any other seed.
``--output`` writes the mesh with the distance in the place of the temperature (NaN where the seeds do not reach).  ``--length-scale
L`` multiplies the lengths of the report and the profile by L and the areas by L^2; ``--max-distance``, ``--band-width`` and the
written PLY stay in the mesh's own units.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from thermo_nerf_amd.export.cli import json_number, load_mesh_ply, require_rocm_device, write_report  # noqa: E402

MAX_CELLS = 256  # seeds up to which every seed's own cell is reported


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--from-vertex", type=int, nargs="+", default=[], metavar="N", help="seed vertices by number")
    ap.add_argument("--from-point", type=float, nargs=3, action="append", default=[], metavar=("X", "Y", "Z"), help="a picked point")
    ap.add_argument("--from-hotspots", type=float, default=None, metavar="P", help="the peaks of the hot spots above P degrees of prominence")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="with --from-hotspots: the N most prominent spots only")
    ap.add_argument("--coldest", action="store_true", help="with --from-hotspots: the cold spots")
    ap.add_argument("--from-min-temperature", type=float, default=None, metavar="T", help="the faces at least T degrees warm")
    ap.add_argument("--from-max-temperature", type=float, default=None, metavar="T", help="the faces at most T degrees warm")
    ap.add_argument("--max-distance", type=float, default=math.inf, metavar="D", help="stop at this distance (the mesh's units)")
    ap.add_argument("--to-point", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="the tape measure's other end")
    ap.add_argument("--band-width", type=float, default=None, metavar="W", help="the width of a band of the profile (the mesh's units)")
    ap.add_argument("--bands", type=int, default=None, metavar="K", help="the bands of the profile, 1 .. 4096")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the reported lengths by L and the areas by L^2")
    ap.add_argument("--output", type=Path, default=None, help="write the mesh with the distance as its temperature")
    ap.add_argument("--profile", type=Path, default=None, help="the CSV of the decay profile")
    ap.add_argument("--report", type=Path, default=None, help="the JSON report")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not (args.from_vertex or args.from_point or args.from_hotspots is not None or args.from_min_temperature is not None
            or args.from_max_temperature is not None):
        ap.error("give at least one source of seeds: --from-vertex, --from-point, --from-hotspots, --from-min-temperature or "
                 "--from-max-temperature")
    if any(n < 0 for n in args.from_vertex):
        ap.error("--from-vertex takes vertex numbers >= 0")
    if args.from_hotspots is not None and (math.isnan(args.from_hotspots) or args.from_hotspots < 0.0):
        ap.error("--from-hotspots must be a number >= 0")
    if args.top is not None and (args.from_hotspots is None or args.top < 1):
        ap.error("--top goes with --from-hotspots and must be >= 1")
    if args.coldest and args.from_hotspots is None:
        ap.error("--coldest goes with --from-hotspots")
    for t in (args.from_min_temperature, args.from_max_temperature):
        if t is not None and math.isnan(t):
            ap.error("--from-min-temperature and --from-max-temperature take numbers")
    if math.isnan(args.max_distance) or args.max_distance < 0.0:
        ap.error("--max-distance must be a number >= 0")
    if (args.band_width is None) != (args.bands is None):
        ap.error("--band-width and --bands go together")
    if args.band_width is not None and not (args.band_width > 0.0 and math.isfinite(args.band_width)):
        ap.error("--band-width must be positive and finite")
    if args.bands is not None and not 1 <= args.bands <= 4096:
        ap.error("--bands must lie in 1 .. 4096")
    if args.profile is not None and args.bands is None:
        ap.error("--profile needs --band-width and --bands")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def profile_rows(profile, seed: int, length_scale: float = 1.0) -> list:
    """the lines of the CSV for one ``DistanceProfile``: lengths times ``length_scale``, areas times its square"""
    s = float(length_scale)
    w = profile.band_width
    return [{"seed": int(seed), "band": k, "from": k * w * s, "to": (k + 1) * w * s, "area": float(row["area"]) * s * s,
             "mean_temperature": json_number(row["mean_temperature"]), "min_temperature": json_number(row["min_temperature"]),
             "max_temperature": json_number(row["max_temperature"])} for k, row in enumerate(profile.bands)]


def write_profile(path: Path, rows: list) -> None:
    path.parent.mkdir(parents=True, exist_ok=True)
    names = ("seed", "band", "from", "to", "area", "mean_temperature", "min_temperature", "max_temperature")
    lines = [",".join(names)] + [",".join("" if r[n] is None else repr(r[n]) for n in names) for r in rows]
    path.write_text("\n".join(lines) + "\n")
    print(f"wrote {path}: {len(rows)} bands")


def main(argv=None) -> int:
    args = parse(argv)

    import numpy as np
    import torch

    from thermo_nerf_amd.export import (build_mesh_bvh, distance_at_points, distance_profile, geodesic_distance, seeds_at_points,
                                        seeds_of_regions, thermal_hotspots, thermal_regions, write_mesh_ply)

    dev = require_rocm_device(args.device, "analyses meshes")
    mesh, data = load_mesh_ply(args.mesh, dev, with_bounds=True)
    v = len(data["positions"])
    if any(n >= v for n in args.from_vertex):
        print(f"error: --from-vertex names a vertex beyond the mesh's {v}", file=sys.stderr)
        return 2
    s = float(args.length_scale)
    bvh = build_mesh_bvh(mesh) if (args.from_point or args.to_point is not None) else None
    seeds, offsets, sources = [np.asarray(args.from_vertex, np.int32)], [np.zeros(len(args.from_vertex))], {}
    if args.from_vertex:
        sources["vertices"] = len(args.from_vertex)
    if args.from_point:
        sv, so = seeds_at_points(bvh, torch.tensor(args.from_point, dtype=torch.float32, device=dev))
        seeds.append(sv), offsets.append(so)
        sources["points"] = len(args.from_point)
    if args.from_hotspots is not None:
        spots = thermal_hotspots(mesh, args.from_hotspots, coldest=args.coldest, top=args.top)
        seeds.append(spots.peak_vertex.astype(np.int32)), offsets.append(np.zeros(len(spots)))
        sources["hotspots"] = len(spots)
    if args.from_min_temperature is not None or args.from_max_temperature is not None:
        lo = -math.inf if args.from_min_temperature is None else args.from_min_temperature
        hi = math.inf if args.from_max_temperature is None else args.from_max_temperature
        sv, _ = seeds_of_regions(mesh, thermal_regions(mesh, lo, hi))
        seeds.append(sv), offsets.append(np.zeros(len(sv)))
        sources["region_vertices"] = len(sv)
    seeds, offsets = np.concatenate(seeds), np.concatenate(offsets)
    if len(seeds) == 0:
        print("error: the sources give no seed", file=sys.stderr)
        return 2

    d = geodesic_distance(mesh, seeds, offsets, max_distance=args.max_distance)
    dist = d.distance
    reach = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, -1.0))
    far = int(reach.argmax()) if d.reached else -1
    report = {"mesh": str(args.mesh), "length_scale": s, "seeds": int(len(seeds)), "sources": sources,
              "max_distance": json_number(args.max_distance), "rounds": d.rounds, "converged": d.converged,
              "counts": {"vertices": v, "faces": len(data["triangles"]), "reached": d.reached},
              "reached_share": d.reached / v if v else 0.0,
              "farthest": None if far < 0 else {"index": far, "distance": float(dist[far]) * s,
                                                "position": [float(c) * s for c in data["positions"][far]]}}
    print(f"{args.mesh}: {v} vertices, {len(data['triangles'])} faces; {len(seeds)} seeds, {d.rounds} rounds, "
          f"{'converged' if d.converged else 'NOT converged'}, {d.reached} vertices reached"
          + ("" if far < 0 else f", the farthest at {float(dist[far]) * s:.6g} (vertex {far})"))
    if args.to_point is not None:
        there = float(distance_at_points(mesh, d, bvh, torch.tensor([args.to_point], dtype=torch.float32, device=dev))[0])
        report["to_point"] = {"point": [float(c) for c in args.to_point], "distance": json_number(there * s)}
        print(f"distance to ({args.to_point[0]:g}, {args.to_point[1]:g}, {args.to_point[2]:g}): "
              + (f"{there * s:.6g}" if math.isfinite(there) else "not reached"))
    rows = []
    if args.bands is not None:
        whole = distance_profile(mesh, d, args.band_width, args.bands)
        rows += profile_rows(whole, -1, s)
        report["profile"] = {"band_width": args.band_width * s, "bands": args.bands, "banded_faces": whole.banded_faces,
                             "measured_faces": whole.measured_faces}
    if 1 < len(seeds) <= MAX_CELLS and d.reached:
        top = float(dist[far])
        cells = []
        for i in range(len(seeds)):
            inside = d.nearest_seed == i
            one = distance_profile(mesh, d, 2.0 * top + 1.0, 1, cell=i).bands[0]
            cells.append({"seed": i, "vertex": int(seeds[i]), "vertices": int(inside.sum()), "faces": int(one["faces"]),
                          "area": float(one["area"]) * s * s, "mean_temperature": json_number(one["mean_temperature"]),
                          "farthest_distance": json_number(float(reach[inside].max()) * s if bool(inside.any()) else None)})
            if args.bands is not None:
                rows += profile_rows(distance_profile(mesh, d, args.band_width, args.bands, cell=i), i, s)
        report["cells"] = cells
    if args.profile is not None:
        write_profile(args.profile, rows)
    if args.report is not None:
        write_report(args.report, report)
    if args.output is not None:
        write_mesh_ply(args.output, d.mesh)
        print(f"wrote {args.output}: vertices {v}, the distance as the temperature")
    return 0


if __name__ == "__main__":
    sys.exit(main())
