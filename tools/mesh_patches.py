#!/usr/bin/env python
"""Ask a thermal mesh which walls, floors and roof planes it consists of: the faces of a PLY that ``tools/export_mesh.py`` wrote joined
across edges while the angle between their normals stays under a limit; per patch the area, the fitted plane, the flatness, the rms /
max deviation from the plane, the mean / min / max degrees Celsius, the centroid and the bounds.  No run directory and no model: the
PLY is all it reads.

    python tools/mesh_patches.py mesh.ply [--max-angle 10] [--min-area A] [--top N] [--length-scale L] --report patches.json
           [--output patches.ply --colors rgb|thermal] [--thermograms DIR --pixel-size S]

One line per patch is printed, largest area first; ``--report`` gets the same as JSON with the mesh's edge counts (boundary,
non-manifold, inconsistent orientation), the mesh's area and the share of it that lies in the reported patches.  The criterion is
adjacency chaining: a gently curved surface whose neighbouring faces all stay under ``--max-angle`` is ONE patch — ``flatness`` (1 for a
plane, 0 for a closed surface) and ``rms_deviation`` show it; a noisy surface-nets mesh wants ``export_mesh.py --smooth-iterations``
first.  ``--max-angle 180`` gives the edge-connected components.  ``--min-area`` is in the mesh's own units squared.
``--length-scale L`` multiplies the lengths of the report (plane offset, deviations, centroid, bounds) by L and its areas by L^2; the
mesh, ``--min-area``, ``--pixel-size`` and the written files are not scaled.  ``--output`` writes the faces of the reported patches as a
mesh.  ``--thermograms DIR`` writes ``patch_<k>.png`` per reported patch: the patch alone, seen straight on (against its normal), at
``--pixel-size`` world units per pixel, degrees through the magma table over the file's ``temperature_bounds``.
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

from thermo_nerf_amd.export.cli import json_number, load_mesh_ply, require_rocm_device, thermal_bytes, write_report  # noqa: E402


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--max-angle", type=float, default=10.0, metavar="DEG", help="join faces across an edge up to this angle between their normals")
    ap.add_argument("--min-area", type=float, default=0.0, metavar="A", help="drop patches below this area (the mesh's units squared)")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="report the N largest patches only")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the report's lengths by L and its areas by L^2")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--output", type=Path, default=None, help="also write the faces of the reported patches as a PLY")
    ap.add_argument("--colors", choices=("rgb", "thermal"), default="rgb", help="what fills red / green / blue of --output")
    ap.add_argument("--thermograms", type=Path, default=None, metavar="DIR", help="also write one PNG per reported patch, seen straight on")
    ap.add_argument("--pixel-size", type=float, default=None, metavar="S", help="world units per pixel of --thermograms")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if math.isnan(args.max_angle) or not 0.0 <= args.max_angle <= 180.0:
        ap.error("--max-angle must be within 0 .. 180 degrees")
    if math.isnan(args.min_area) or args.min_area < 0.0:
        ap.error("--min-area must be a number >= 0")
    if args.top is not None and args.top < 0:
        ap.error("--top must be >= 0")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    if (args.thermograms is None) != (args.pixel_size is None):
        ap.error("--thermograms and --pixel-size go together")
    if args.pixel_size is not None and not (args.pixel_size > 0.0 and math.isfinite(args.pixel_size)):
        ap.error("--pixel-size must be positive and finite")
    return args


def build_report(found, edges, num_vertices: int, num_faces: int, max_angle: float, length_scale: float = 1.0, source: str = "") -> dict:
    """the JSON report of ``found`` (a ``MeshPatches``) and ``edges`` (the ``MeshHalfEdges`` of its mesh): plain Python numbers; lengths
    times ``length_scale``, areas times its square; a NaN (no plane, no thermal face) is null"""
    s, s2 = float(length_scale), float(length_scale) ** 2

    def point(p):
        return [float(c) * s for c in p]

    def scaled(x):
        return None if json_number(x) is None else float(x) * s

    rows = []
    for q, row in zip(found.patch_index.tolist(), found.patches):
        plane = [float(c) for c in row["plane"]]
        rows.append({"patch": int(q), "label": int(row["label"]), "faces": int(row["faces"]), "thermal_faces": int(row["thermal_faces"]),
                     "area": float(row["area"]) * s2, "thermal_area": float(row["thermal_area"]) * s2,
                     "plane": {"normal": plane[:3], "offset": plane[3] * s}, "flatness": float(row["flatness"]),
                     "rms_deviation": scaled(row["rms_deviation"]), "max_deviation": scaled(row["max_deviation"]),
                     "mean_temperature": json_number(row["mean_temperature"]), "min_temperature": json_number(row["min_temperature"]),
                     "max_temperature": json_number(row["max_temperature"]), "centroid": point(row["centroid"]),
                     "bounds": {"min": point(row["bounds"][:3]), "max": point(row["bounds"][3:])}})
    mesh_area = float(found.mesh_area) * s2
    reported = sum(r["area"] for r in rows)
    return {"mesh": source, "length_scale": s, "max_angle_degrees": float(max_angle),
            "edges": {"edges": int(edges.edges), "boundary": int(edges.boundary_edges), "nonmanifold": int(edges.nonmanifold_edges),
                      "inconsistent": int(edges.inconsistent_edges), "closed_manifold": bool(edges.closed_manifold),
                      "joined_half_edges": int(found.joined_half_edges)},
            "counts": {"vertices": int(num_vertices), "faces": int(num_faces), "geometric_faces": int(found.geometric_faces),
                       "patches": int(found.num_patches), "reported_patches": len(rows)},
            "mesh_area": mesh_area, "thermal_area": float(found.thermal_area) * s2, "reported_area": reported,
            "reported_share": reported / mesh_area if mesh_area > 0.0 else 0.0, "patches": rows}


def _degrees(x) -> str:
    return "none" if x is None else f"{x:.2f}"


def patch_lines(report: dict) -> list:
    lines = []
    for k, row in enumerate(report["patches"]):
        c, n = row["centroid"], row["plane"]["normal"]
        rms = "none" if row["rms_deviation"] is None else f"{row['rms_deviation']:.4g}"
        lines.append(f"patch {k}: area {row['area']:.6g}, {row['faces']} faces, normal ({n[0]:+.3f}, {n[1]:+.3f}, {n[2]:+.3f}), flatness "
                     f"{row['flatness']:.4f}, rms deviation {rms}, mean {_degrees(row['mean_temperature'])} C (min "
                     f"{_degrees(row['min_temperature'])}, max {_degrees(row['max_temperature'])}), centroid ({c[0]:.4g}, {c[1]:.4g}, "
                     f"{c[2]:.4g}), label {row['label']}")
    return lines


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import mesh_half_edges, mesh_thermogram, patch_view, planar_patches, regions_mesh, write_mesh_ply

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "analyses meshes"), with_bounds=True)
    edges = mesh_half_edges(mesh.triangles, len(data["positions"]))
    found = planar_patches(mesh, args.max_angle, half_edges=edges, min_area=args.min_area, top=args.top)
    report = build_report(found, edges, len(data["positions"]), len(data["triangles"]), args.max_angle, args.length_scale, str(args.mesh))
    counts = report["counts"]
    print(f"{args.mesh}: {counts['vertices']} vertices, {counts['faces']} faces, area {report['mesh_area']:.6g}, {report['edges']['edges']} "
          f"edges ({report['edges']['boundary']} boundary, {report['edges']['nonmanifold']} non-manifold); {counts['patches']} patches up to "
          f"{args.max_angle:g} degrees, {counts['reported_patches']} reported with {100.0 * report['reported_share']:.2f} % of the area")
    for line in patch_lines(report):
        print(line)
    write_report(args.report, report)
    if args.output is not None:
        part = regions_mesh(mesh, found)
        if args.colors == "thermal":
            part.thermal_colors = torch.from_numpy(thermal_bytes(part.temperature.cpu().numpy(), mesh.temperature_bounds))
        write_mesh_ply(args.output, part, colors=args.colors)
        print(f"wrote {args.output}: vertices {len(part)}, triangles {int(part.triangles.shape[0])}")
    if args.thermograms is not None:
        from PIL import Image

        args.thermograms.mkdir(parents=True, exist_ok=True)
        written = 0
        for k in range(len(found)):
            if not any(found.patches[k]["plane"][:3]):
                print(f"patch {k}: no plane, no thermogram")
                continue
            view = patch_view(mesh, found, k, pixel_size=args.pixel_size)
            image = mesh_thermogram(regions_mesh(mesh, found.only(k)), view).to_rgb8("thermal").cpu().numpy()
            Image.fromarray(image, "RGB").save(args.thermograms / f"patch_{k}.png")
            written += 1
        print(f"wrote {written} thermograms to {args.thermograms}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
