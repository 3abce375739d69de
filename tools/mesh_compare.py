#!/usr/bin/env python
"""Compare two thermal meshes of one object — this survey and the one before the retrofit: where did the surface warm or cool, by
how much, over what area.  Both are PLYs that ``tools/export_mesh.py`` wrote, in ONE frame (the same world transform).  Every vertex
of the first mesh is matched with the nearest point of the second mesh's surface within ``--max-distance``; its difference is its own
degrees Celsius minus the surface's there.  No run directory and no model: the two PLYs are all it reads.

    python tools/mesh_compare.py now.ply before.ply --max-distance 0.05 --output diff.ply --report diff.json
           [--min-change 2.0] [--length-scale S]

``--output`` gets the first mesh with the difference as its ``temperature`` (NaN where the second mesh has no surface within
``--max-distance``) and ``temperature_bounds`` -m m, m the largest change: ``tools/mesh_regions.py``, ``tools/mesh_thermogram.py`` and
``tools/mesh_camera_view.py`` read it like any mesh.  ``--report`` gets the vertex and face counts of both meshes, the matched share,
the mean / RMS / max distance and the mean / RMS / min / max difference.  ``--min-change X`` adds the regions that warmed by at least
X and those that cooled by at least X (``thermal_regions`` on the difference: faces joined through shared vertices) with area, mean
difference, centroid and largest change per region, and prints one line each.  ``--length-scale S`` multiplies the report's lengths
by S and its areas by S^2 (the world frame of a COLMAP reconstruction has an arbitrary unit); ``--max-distance`` and the written PLY
are in the meshes' own units.
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

from thermo_nerf_amd.export.cli import (add_difference_regions, difference_region_lines, json_number, load_mesh_ply,  # noqa: E402,F401
                                        region_rows, require_rocm_device, write_report)


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="the mesh whose vertices are compared (a PLY written by tools/export_mesh.py)")
    ap.add_argument("reference", type=Path, help="the mesh they are compared with: its surface is searched")
    ap.add_argument("--max-distance", type=float, required=True, metavar="R", help="match a vertex with surface at most this far (the meshes' units)")
    ap.add_argument("--output", type=Path, required=True, help="the first mesh with the difference as its temperature, as a PLY")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--min-change", type=float, default=None, metavar="X", help="also report the regions that changed by at least X degrees")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="S", help="multiply the report's lengths by S and its areas by S^2")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if math.isnan(args.max_distance) or args.max_distance < 0.0:
        ap.error("--max-distance must be a number >= 0")
    if args.min_change is not None and not (args.min_change > 0.0 and math.isfinite(args.min_change)):
        ap.error("--min-change must be positive and finite")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def build_report(found, vertices, faces, reference_vertices, reference_faces, max_distance: float, length_scale: float = 1.0,
                 warmed=None, cooled=None, min_change=None, source: str = "", reference: str = "") -> dict:
    """the JSON report of ``found`` (a ``MeshDifference``): plain Python numbers, None where there is no value; distances times
    ``length_scale``, areas times its square.  ``warmed`` / ``cooled``: the ``ThermalRegions`` of --min-change, or None."""
    s = float(length_scale)

    def length(x):
        x = json_number(x)
        return None if x is None else x * s

    report = {"mesh": source, "reference": reference, "length_scale": s, "max_distance": json_number(max_distance),
              "counts": {"vertices": int(vertices), "faces": int(faces), "reference_vertices": int(reference_vertices),
                         "reference_faces": int(reference_faces), "reference_usable_faces": int(found.closest.usable_faces),
                         "matched_vertices": int(found.matched), "stack_limit_points": int(found.closest.stack_limit_points)},
              "matched_share": float(found.matched_share),
              "distance": {"mean": length(found.mean_distance), "rms": length(found.rms_distance), "max": length(found.max_distance)},
              "difference": {"mean": json_number(found.mean_difference), "rms": json_number(found.rms_difference),
                             "min": json_number(found.min_difference), "max": json_number(found.max_difference)}}
    if min_change is not None:
        add_difference_regions(report, ("warmed", "cooled"), warmed, cooled, min_change, s)
    return report


def summary_line(report: dict) -> str:
    c, d, t = report["counts"], report["distance"], report["difference"]
    if not c["matched_vertices"]:
        return f"{report['mesh']} against {report['reference']}: {c['vertices']} vertices, none within {report['max_distance']} of the reference"
    return (f"{report['mesh']} against {report['reference']}: {c['vertices']} vertices, {c['matched_vertices']} matched "
            f"({100.0 * report['matched_share']:.1f} %), distance mean {d['mean']:.4g} rms {d['rms']:.4g} max {d['max']:.4g}, "
            f"difference mean {t['mean']:+.2f} C rms {t['rms']:.2f} min {t['min']:+.2f} max {t['max']:+.2f}")


def region_lines(report: dict) -> list:
    return difference_region_lines(report, ("warmed", "cooled"))


def main(argv=None) -> int:
    args = parse(argv)

    from thermo_nerf_amd.export import build_mesh_bvh, mesh_difference, thermal_regions, write_mesh_ply

    dev = require_rocm_device(args.device, "compares meshes")
    mesh, data = load_mesh_ply(args.mesh, dev, with_bounds=False)
    reference, reference_data = load_mesh_ply(args.reference, dev, with_bounds=False)
    found = mesh_difference(mesh, build_mesh_bvh(reference), max_distance=args.max_distance)
    warmed = cooled = None
    if args.min_change is not None:
        warmed = thermal_regions(found.mesh, min_temperature=args.min_change)
        cooled = thermal_regions(found.mesh, max_temperature=-args.min_change)
    report = build_report(found, len(data["positions"]), len(data["triangles"]), len(reference_data["positions"]), len(reference_data["triangles"]),
                          args.max_distance, args.length_scale, warmed, cooled, args.min_change, str(args.mesh), str(args.reference))
    print(summary_line(report))
    for line in region_lines(report):
        print(line)
    write_report(args.report, report)
    write_mesh_ply(args.output, found.mesh)
    print(f"wrote {args.output}: vertices {len(found.mesh)}, triangles {int(found.mesh.triangles.shape[0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
