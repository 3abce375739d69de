#!/usr/bin/env python
"""Ask a thermal mesh where it is warmer than X (or colder than Y): the faces of a PLY that ``tools/export_mesh.py`` wrote whose
temperature lies in a window, joined into regions through shared vertices; per region the area, the mean / min / max degrees Celsius,
the centroid, the bounds and the hottest and coldest vertex.  No run directory and no model: the PLY is all it reads.

    python tools/mesh_regions.py mesh.ply --min-temperature 28 [--max-temperature T] [--min-area A] [--top N]
           [--length-scale L] --report regions.json [--output regions.ply --colors rgb|thermal]

One line per region is printed, largest area first; ``--report`` gets the same as JSON with the window, the counts, the mesh's area
and the selected area with its share.  ``--min-area`` is in the mesh's own units squared.  ``--length-scale L`` multiplies the lengths
of the report (centroid, bounds, vertex positions) by L and its areas by L^2 — the world frame of a COLMAP reconstruction has an
arbitrary unit; the mesh, ``--min-area`` and the written PLY are not scaled.  ``--output`` writes the faces of the reported regions
as a mesh: ``--colors rgb`` keeps the file's colours, ``thermal`` maps the temperatures through the magma table over the file's
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

from thermo_nerf_amd.export.cli import (file_bounds, json_number, load_mesh_ply, require_rocm_device, thermal_bytes,  # noqa: E402,F401
                                        write_report)


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--min-temperature", type=float, default=-math.inf, metavar="T", help="faces at least this warm (degrees Celsius)")
    ap.add_argument("--max-temperature", type=float, default=math.inf, metavar="T", help="faces at most this warm (degrees Celsius)")
    ap.add_argument("--min-area", type=float, default=0.0, metavar="A", help="drop regions below this area (the mesh's units squared)")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="report the N largest regions only")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the report's lengths by L and its areas by L^2")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--output", type=Path, default=None, help="also write the faces of the reported regions as a PLY")
    ap.add_argument("--colors", choices=("rgb", "thermal"), default="rgb", help="what fills red / green / blue of --output")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if math.isnan(args.min_temperature) or math.isnan(args.max_temperature):
        ap.error("--min-temperature / --max-temperature must not be NaN")
    if args.min_temperature == -math.inf and args.max_temperature == math.inf:
        ap.error("give --min-temperature, --max-temperature or both: without a window every face is selected")
    if math.isnan(args.min_area) or args.min_area < 0.0:
        ap.error("--min-area must be a number >= 0")
    if args.top is not None and args.top < 0:
        ap.error("--top must be >= 0")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def build_report(found, positions, temperature, num_faces: int, length_scale: float = 1.0, source: str = "") -> dict:
    """the JSON report of ``found`` (a ``ThermalRegions``) over the host arrays ``positions`` [V,3] and ``temperature`` [V] of its
    mesh: plain Python numbers; lengths times ``length_scale``, areas times its square"""
    s, s2 = float(length_scale), float(length_scale) ** 2

    def point(p):
        return [float(c) * s for c in p]

    def vertex(i):
        i = int(i)
        return {"index": i, "position": point(positions[i]), "temperature": float(temperature[i])}

    rows = []
    for r, row in zip(found.region_index.tolist(), found.regions):
        rows.append({"region": int(r), "label": int(row["label"]), "faces": int(row["faces"]), "area": float(row["area"]) * s2,
                     "mean_temperature": float(row["mean_temperature"]), "min_temperature": float(row["min_temperature"]),
                     "max_temperature": float(row["max_temperature"]), "centroid": point(row["centroid"]),
                     "bounds": {"min": point(row["bounds"][:3]), "max": point(row["bounds"][3:])},
                     "hottest_vertex": vertex(row["hottest_vertex"]), "coldest_vertex": vertex(row["coldest_vertex"])})
    mesh_area, selected_area = float(found.mesh_area) * s2, float(found.selected_area) * s2
    return {"mesh": source, "length_scale": s,
            "window": {"min_temperature": json_number(found.window[0], keep_nan=True), "max_temperature": json_number(found.window[1], keep_nan=True)},
            "counts": {"vertices": int(len(positions)), "faces": int(num_faces), "usable_faces": int(found.usable_faces),
                       "selected_faces": int(found.selected_faces), "regions": int(found.num_regions), "reported_regions": len(rows)},
            "mesh_area": mesh_area, "selected_area": selected_area,
            "selected_share": selected_area / mesh_area if mesh_area > 0.0 else 0.0, "regions": rows}


def region_lines(report: dict) -> list:
    lines = []
    for k, row in enumerate(report["regions"]):
        c, hot = row["centroid"], row["hottest_vertex"]
        lines.append(f"region {k}: area {row['area']:.6g}, {row['faces']} faces, mean {row['mean_temperature']:.2f} C "
                     f"(min {row['min_temperature']:.2f}, max {row['max_temperature']:.2f}), centroid ({c[0]:.4g}, {c[1]:.4g}, {c[2]:.4g}), "
                     f"hottest vertex {hot['index']} at {hot['temperature']:.2f} C, label {row['label']}")
    return lines


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import regions_mesh, thermal_regions, write_mesh_ply

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "analyses meshes"), with_bounds=True)
    found = thermal_regions(mesh, args.min_temperature, args.max_temperature, min_area=args.min_area, top=args.top)
    report = build_report(found, data["positions"], data["temperature"], len(data["triangles"]), args.length_scale, str(args.mesh))
    share = 100.0 * report["selected_share"]
    print(f"{args.mesh}: {report['counts']['vertices']} vertices, {report['counts']['faces']} faces, area {report['mesh_area']:.6g}; "
          f"in the window {report['counts']['selected_faces']} faces, area {report['selected_area']:.6g} ({share:.2f} %), "
          f"{report['counts']['regions']} regions, {report['counts']['reported_regions']} reported")
    for line in region_lines(report):
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
