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
import json
import math
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def _bound(x: float):
    return None if math.isinf(x) else float(x)


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
            "window": {"min_temperature": _bound(found.window[0]), "max_temperature": _bound(found.window[1])},
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


def thermal_bytes(temperature, bounds):
    """uint8 [M,3]: the magma table at trunc(256 (t - lo) / (hi - lo)), clamped to the table"""
    import numpy as np

    from thermo_nerf_amd import colormaps

    t = np.asarray(temperature, np.float64)
    lo, hi = bounds if bounds is not None else ((float(t.min()), float(t.max())) if len(t) else (0.0, 1.0))
    x = (t - lo) / (hi - lo) if hi > lo else np.zeros_like(t)
    index = np.clip(np.nan_to_num(np.trunc(x * 256.0), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.int64)
    return colormaps.table_u8("magma")[index]


def file_bounds(comments):
    """the (lo, hi) of the file's ``temperature_bounds`` comment, or None"""
    for line in comments:
        parts = line.split()
        if len(parts) == 3 and parts[0] == "temperature_bounds" and parts[1] != "none":
            return float(parts[1]), float(parts[2])
    return None


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import ThermalMesh, read_mesh_ply, regions_mesh, thermal_regions, write_mesh_ply

    data = read_mesh_ply(args.mesh)
    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise RuntimeError(f"--device {args.device}: thermo_nerf_amd analyses meshes only on a ROCm device (no CPU fallback exists)")
    bounds = file_bounds(data["comments"])
    normals = data.get("normals")
    mesh = ThermalMesh(torch.from_numpy(data["positions"].copy()).to(dev), torch.from_numpy(data["colors"].copy()).to(dev),
                       torch.from_numpy(data["temperature"].copy()).to(dev), None, torch.from_numpy(data["triangles"].copy()).to(dev),
                       bounds, None if normals is None else torch.from_numpy(normals.copy()).to(dev))
    found = thermal_regions(mesh, args.min_temperature, args.max_temperature, min_area=args.min_area, top=args.top)
    report = build_report(found, data["positions"], data["temperature"], len(data["triangles"]), args.length_scale, str(args.mesh))
    share = 100.0 * report["selected_share"]
    print(f"{args.mesh}: {report['counts']['vertices']} vertices, {report['counts']['faces']} faces, area {report['mesh_area']:.6g}; "
          f"in the window {report['counts']['selected_faces']} faces, area {report['selected_area']:.6g} ({share:.2f} %), "
          f"{report['counts']['regions']} regions, {report['counts']['reported_regions']} reported")
    for line in region_lines(report):
        print(line)
    args.report.parent.mkdir(parents=True, exist_ok=True)
    args.report.write_text(json.dumps(report, indent=1) + "\n")
    print(f"wrote {args.report}")
    if args.output is not None:
        part = regions_mesh(mesh, found)
        if args.colors == "thermal":
            part.thermal_colors = torch.from_numpy(thermal_bytes(part.temperature.cpu().numpy(), bounds))
        write_mesh_ply(args.output, part, colors=args.colors)
        print(f"wrote {args.output}: vertices {len(part)}, triangles {int(part.triangles.shape[0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
