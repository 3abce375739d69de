#!/usr/bin/env python
"""Ask a thermal mesh where its anomalies are and how strong each is against its own surroundings: the local maxima of the degrees
Celsius of a PLY that ``tools/export_mesh.py`` wrote (or ``mesh_compare.py`` / ``mesh_project.py``: vertices without a value are
NaN and belong to nothing), ranked by their prominence — how far one descends from the peak before a hotter one can be reached.
No run directory and no model: the PLY is all it reads.

    python tools/mesh_hotspots.py mesh.ply --min-prominence 1.0 [--coldest] [--extent-drop D] [--smooth-iterations N]
           [--min-area A] [--top N] [--length-scale L] --report spots.json [--output spots.ply --colors rgb|thermal]

One line per spot is printed, most prominent first; ``--report`` gets the same as JSON with the counts.  ``--coldest`` looks for cold
spots (air leaks, wet patches) instead.  A spot's extent is what lies above the saddle where it joins a stronger spot;
``--extent-drop D`` cuts it to the vertices within D degrees of the peak.  ``--smooth-iterations N`` smooths the degrees first (the
peaks, saddles and every reported temperature are then those of the smoothed field).  ``--min-area`` is in the mesh's own units
squared.  ``--length-scale L`` multiplies the lengths of the report (positions, centroid, bounds) by L and its areas by L^2; the
degrees, the mesh, ``--min-area`` and the written PLY are not scaled.  ``--output`` writes the faces of the reported spots as a
mesh: ``--colors rgb`` keeps the file's colours, ``thermal`` maps the temperatures through the magma table over the file's
``temperature_bounds`` (over the written vertices' own range if the file names none).
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

from thermo_nerf_amd.export.cli import (json_number, load_mesh_ply, require_rocm_device, thermal_bytes,  # noqa: E402,F401
                                        write_report)


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--min-prominence", type=float, required=True, metavar="P", help="spots that stand out by more than P degrees Celsius")
    ap.add_argument("--coldest", action="store_true", help="cold spots: the local minima")
    ap.add_argument("--extent-drop", type=float, default=math.inf, metavar="D", help="a spot's extent reaches D degrees below its peak")
    ap.add_argument("--smooth-iterations", type=int, default=0, metavar="N", help="smooth the degrees N times first")
    ap.add_argument("--min-area", type=float, default=0.0, metavar="A", help="drop spots below this area (the mesh's units squared)")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="report the N most prominent spots only")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the report's lengths by L and its areas by L^2")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--output", type=Path, default=None, help="also write the faces of the reported spots as a PLY")
    ap.add_argument("--colors", choices=("rgb", "thermal"), default="rgb", help="what fills red / green / blue of --output")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if math.isnan(args.min_prominence) or args.min_prominence < 0.0:
        ap.error("--min-prominence must be a number >= 0")
    if math.isnan(args.extent_drop) or args.extent_drop < 0.0:
        ap.error("--extent-drop must be a number >= 0")
    if args.smooth_iterations < 0:
        ap.error("--smooth-iterations must be >= 0")
    if math.isnan(args.min_area) or args.min_area < 0.0:
        ap.error("--min-area must be a number >= 0")
    if args.top is not None and args.top < 0:
        ap.error("--top must be >= 0")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def build_report(found, num_vertices: int, num_faces: int, extent_drop: float = math.inf, smooth_iterations: int = 0,
                 length_scale: float = 1.0, source: str = "") -> dict:
    """the JSON report of ``found`` (a ``ThermalHotspots``): plain Python numbers; lengths times ``length_scale``, areas times its
    square, degrees as they are; None where JSON cannot say it (an infinite prominence, the saddle of a component's maximum)"""
    s, s2 = float(length_scale), float(length_scale) ** 2

    def point(p):
        return [json_number(float(c) * s, keep_nan=False) for c in p]

    rows = []
    for n in range(len(found)):
        row = found.spots[n]
        rows.append({"spot": int(found.spot_index[n]),
                     "peak": {"index": int(found.peak_vertex[n]), "position": point(found.peak_position[n]),
                              "temperature": float(found.peak_temperature[n])},
                     "prominence": json_number(found.prominence[n]),
                     "saddle": None if found.is_maximum[n] else {"index": int(found.saddle_vertex[n]),
                                                                 "temperature": float(found.saddle_temperature[n])},
                     "component_extreme": bool(found.is_maximum[n]), "basins": int(found.basins[n]), "vertices": int(row["vertices"]),
                     "faces": int(row["faces"]), "area": float(row["area"]) * s2,
                     "mean_temperature": json_number(row["mean_temperature"]), "min_temperature": json_number(row["min_temperature"]),
                     "max_temperature": json_number(row["max_temperature"]), "centroid": point(row["centroid"]),
                     "bounds": {"min": point(row["bounds"][:3]), "max": point(row["bounds"][3:])}})
    return {"mesh": source, "length_scale": s, "coldest": bool(found.coldest), "min_prominence": float(found.min_prominence),
            "extent_drop": json_number(extent_drop), "smooth_iterations": int(smooth_iterations),
            "counts": {"vertices": int(num_vertices), "faces": int(num_faces), "basins": int(found.num_basins),
                       "saddles": int(found.num_saddles), "spots": int(found.num_spots), "reported_spots": len(rows)},
            "spots": rows}


def spot_lines(report: dict) -> list:
    lines = []
    for k, row in enumerate(report["spots"]):
        p = row["peak"]
        x = p["position"]
        stands = "the extreme of its component" if row["saddle"] is None else (
            f"prominence {row['prominence']:.2f} C over the saddle at vertex {row['saddle']['index']} ({row['saddle']['temperature']:.2f} C)")
        mean = "no whole face" if row["mean_temperature"] is None else f"mean {row['mean_temperature']:.2f} C"
        lines.append(f"spot {k}: peak {p['temperature']:.2f} C at vertex {p['index']} ({x[0]:.4g}, {x[1]:.4g}, {x[2]:.4g}), {stands}, "
                     f"area {row['area']:.6g}, {row['faces']} faces, {row['vertices']} vertices, {mean}, {row['basins']} basins")
    return lines


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import regions_mesh, thermal_hotspots, write_mesh_ply

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "analyses meshes"), with_bounds=True)
    found = thermal_hotspots(mesh, args.min_prominence, coldest=args.coldest, extent_drop=args.extent_drop,
                             smooth_iterations=args.smooth_iterations, min_area=args.min_area, top=args.top)
    report = build_report(found, len(data["positions"]), len(data["triangles"]), args.extent_drop, args.smooth_iterations,
                          args.length_scale, str(args.mesh))
    c = report["counts"]
    print(f"{args.mesh}: {c['vertices']} vertices, {c['faces']} faces; {c['basins']} {'minima' if args.coldest else 'maxima'}, "
          f"{c['saddles']} saddles, {c['spots']} spots above {args.min_prominence:g} C, {c['reported_spots']} reported")
    for line in spot_lines(report):
        print(line)
    write_report(args.report, report)
    if args.output is not None:
        part = regions_mesh(mesh, found)
        if args.colors == "thermal":
            part.thermal_colors = torch.from_numpy(thermal_bytes(part.temperature.cpu().numpy(), mesh.temperature_bounds))
        write_mesh_ply(args.output, part, colors=args.colors)
        print(f"wrote {args.output}: vertices {len(part)}, triangles {int(part.triangles.shape[0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
