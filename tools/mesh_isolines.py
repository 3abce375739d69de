#!/usr/bin/env python
"""Draw curves on a thermal mesh: the isotherms of a PLY that ``tools/export_mesh.py`` wrote, or its sections by parallel planes, as
ordered polylines with their length and the degrees Celsius along them.  No run directory and no model: the PLY is all it reads.

    python tools/mesh_isolines.py mesh.ply --plane NX NY NZ --offsets D [D ...] [--length-scale L]
           [--output cut.ply] [--profile cut.csv] [--report cut.json]
    python tools/mesh_isolines.py mesh.ply --isotherms T [T ...] | --isotherm-step DT [...]

``--plane`` with ``--offsets``: the cuts at the given distances (the mesh's units) from the origin along the normal.  ``--isotherms``:
the lines at the given temperatures; ``--isotherm-step DT``: at every multiple of DT inside the file's range of temperatures.  One
line per curve is printed: level, open or closed, length, mean / min / max degrees.  ``--output`` writes the curves as a PLY line set
(vertices ``x y z temperature``, an ``edge`` element), ``--profile`` a CSV with the columns ``curve,level,arc,x,y,z,temperature``,
``--report`` a JSON with the mesh's edge counts (edges, boundary, non-manifold, inconsistent), per level the number of curves, their
total length and length-weighted mean temperature, and the curve table.  ``--length-scale L`` multiplies the lengths of the report, of
the printed lines and of the CSV (arc, x, y, z) by L — the world frame of a COLMAP reconstruction has an arbitrary unit; the offsets
and the written PLY are not scaled.  Curves that stay open on a mesh with boundary or inconsistent edges get a warning.
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


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--plane", type=float, nargs=3, default=None, metavar=("NX", "NY", "NZ"), help="the normal of the cutting planes")
    ap.add_argument("--offsets", type=float, nargs="+", default=None, metavar="D", help="distances of the planes from the origin along the normal")
    ap.add_argument("--isotherms", type=float, nargs="+", default=None, metavar="T", help="temperatures of the lines (degrees Celsius)")
    ap.add_argument("--isotherm-step", type=float, default=None, metavar="DT", help="a line at every multiple of DT in the file's range")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the lengths of the report and the CSV by L")
    ap.add_argument("--output", type=Path, default=None, help="write the curves as a PLY line set")
    ap.add_argument("--profile", type=Path, default=None, help="write the points of the curves as CSV")
    ap.add_argument("--report", type=Path, default=None, help="write the JSON report")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    modes = [args.plane is not None, args.isotherms is not None, args.isotherm_step is not None]
    if sum(modes) != 1:
        ap.error("give exactly one of --plane, --isotherms and --isotherm-step")
    if (args.plane is not None) != (args.offsets is not None):
        ap.error("--plane and --offsets go together")
    if args.plane is not None and (not all(math.isfinite(x) for x in args.plane) or not any(args.plane)):
        ap.error("--plane must be three finite numbers, not all zero")
    if args.isotherm_step is not None and not (args.isotherm_step > 0.0 and math.isfinite(args.isotherm_step)):
        ap.error("--isotherm-step must be positive and finite")
    for name in ("offsets", "isotherms"):
        values = getattr(args, name)
        if values is not None:
            if not all(math.isfinite(x) for x in values):
                ap.error(f"--{name} must be finite")
            setattr(args, name, sorted(set(values)))
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def step_levels(temperature, step: float) -> list:
    """the multiples of ``step`` inside the range of the finite values of ``temperature``"""
    import numpy as np

    t = np.asarray(temperature, np.float64)
    t = t[np.isfinite(t)]
    if not len(t):
        return []
    first, last = math.ceil(float(t.min()) / step), math.floor(float(t.max()) / step)
    return [k * step for k in range(first, last + 1)]


def build_report(found, edges, length_scale: float = 1.0, source: str = "", mode: dict = None) -> dict:
    """the JSON report of ``found`` (a ``MeshCurves``) and ``edges`` (the ``MeshHalfEdges`` of its mesh): plain Python numbers, lengths
    times ``length_scale``"""
    s = float(length_scale)
    rows = [{"curve": q, "level": int(row["level"]), "value": float(found.levels[int(row["level"])]), "closed": bool(row["closed"]),
             "points": int(row["points"]), "first_point": int(row["first_point"]), "first_face": int(row["first_face"]),
             "length": float(row["length"]) * s, "mean_temperature": json_number(row["mean_temperature"]),
             "min_temperature": float(row["min_temperature"]), "max_temperature": float(row["max_temperature"])}
            for q, row in enumerate(found.curves)]
    levels = []
    for k, value in enumerate(found.levels):
        mine = found.curves[found.curves["level"] == k]
        weighted = [float(r["length"]) * float(r["mean_temperature"]) for r in mine if float(r["length"]) > 0.0]
        length = sum(float(r["length"]) for r in mine)
        levels.append({"level": k, "value": float(value), "curves": int(len(mine)), "closed_curves": int(mine["closed"].sum()),
                       "length": length * s, "mean_temperature": sum(weighted) / length if length > 0.0 else None})
    return {"mesh": source, "length_scale": s, "mode": mode or {},
            "edges": {"edges": int(edges.edges), "boundary": int(edges.boundary_edges), "nonmanifold": int(edges.nonmanifold_edges),
                      "inconsistent": int(edges.inconsistent_edges), "closed_manifold": bool(edges.closed_manifold)},
            "counts": {"segments": int(found.num_segments), "curves": int(found.num_curves), "points": int(found.num_points),
                       "closed_curves": int(found.closed_curves), "usable_faces": int(found.usable_faces)},
            "levels": levels, "curves": rows}


def curve_lines(report: dict) -> list:
    lines = []
    for row in report["curves"]:
        mean = "nan" if row["mean_temperature"] is None else f"{row['mean_temperature']:.2f}"
        lines.append(f"curve {row['curve']}: level {row['value']:.6g}, {'closed' if row['closed'] else 'open'}, length {row['length']:.6g}, "
                     f"{row['points']} points, mean {mean} C (min {row['min_temperature']:.2f}, max {row['max_temperature']:.2f})")
    return lines


def write_profile(path: Path, found, length_scale: float = 1.0) -> None:
    """``curve,level,arc,x,y,z,temperature``, one row per point; arc and position times ``length_scale``, numbers as ``repr``"""
    s = float(length_scale)
    arc, xyz, temp = found.arc.cpu().numpy(), found.positions.cpu().numpy(), found.temperature.cpu().numpy()
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        f.write("curve,level,arc,x,y,z,temperature\n")
        for q, row in enumerate(found.curves):
            value = float(found.levels[int(row["level"])])
            for j in range(int(row["first_point"]), int(row["first_point"]) + int(row["points"])):
                f.write(f"{q},{value!r},{float(arc[j]) * s!r},{float(xyz[j, 0]) * s!r},{float(xyz[j, 1]) * s!r},{float(xyz[j, 2]) * s!r},"
                        f"{float(temp[j])!r}\n")


def main(argv=None) -> int:
    args = parse(argv)

    from thermo_nerf_amd.export import isotherms, mesh_half_edges, mesh_sections, write_curves_ply

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "analyses meshes"), with_bounds=True)
    edges = mesh_half_edges(mesh.triangles, len(data["positions"]))
    if args.plane is not None:
        mode = {"plane": [float(x) for x in args.plane], "offsets": [float(x) for x in args.offsets]}
        found = mesh_sections(mesh, args.plane, args.offsets, half_edges=edges) if len(data["triangles"]) else None
    else:
        levels = args.isotherms if args.isotherms is not None else step_levels(data["temperature"], args.isotherm_step)
        if not levels:
            print(f"{args.mesh}: no multiple of {args.isotherm_step} lies in the file's range of temperatures", file=sys.stderr)
            return 1
        mode = {"isotherms": [float(x) for x in levels]}
        found = isotherms(mesh, levels, half_edges=edges) if len(data["triangles"]) else None
    if found is None:
        print(f"{args.mesh}: the mesh has no triangles", file=sys.stderr)
        return 1
    report = build_report(found, edges, args.length_scale, str(args.mesh), mode)
    e = report["edges"]
    print(f"{args.mesh}: {len(data['positions'])} vertices, {len(data['triangles'])} faces, {e['edges']} edges ({e['boundary']} boundary, "
          f"{e['nonmanifold']} non-manifold, {e['inconsistent']} inconsistent); {found.num_curves} curves, {found.closed_curves} closed, "
          f"{found.num_segments} segments")
    for line in curve_lines(report):
        print(line)
    open_curves = found.num_curves - found.closed_curves
    if open_curves and (edges.boundary_edges or edges.inconsistent_edges):
        print(f"warning: {open_curves} curves are open; the mesh has {edges.boundary_edges} boundary and {edges.inconsistent_edges} "
              "inconsistently oriented edges, where curves end", file=sys.stderr)
    if args.output is not None:
        write_curves_ply(args.output, found, mesh.temperature_bounds)
        print(f"wrote {args.output}: points {found.num_points}, segments {found.num_segments}")
    if args.profile is not None:
        write_profile(args.profile, found, args.length_scale)
        print(f"wrote {args.profile}")
    if args.report is not None:
        write_report(args.report, report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
