#!/usr/bin/env python
"""Ask a thermal mesh where its temperature changes fastest: the surface gradient of the degrees Celsius of a PLY that
``tools/export_mesh.py`` (or ``mesh_project.py``, ``mesh_compare.py``) wrote, in degrees per metre — what shows a thermal bridge, a wet
patch or an air leak where a threshold on the degrees only finds the radiator.  No run directory and no model: the PLY is all it reads.

    python tools/mesh_gradient.py mesh.ply [--smooth-iterations N] [--lambda L] [--mu M] [--fill N] --output gradient.ply
           --report gradient.json [--min-gradient G [--min-area A] [--top K]] [--length-scale S] [--smoothed smoothed.ply]

The steps, in this order: ``--fill N`` fills the vertices without a temperature (NaN: nothing was measured there) from their neighbours,
one ring of a hole per pass, at most N passes, and leaves every other vertex alone; ``--smooth-iterations N`` smooths the degrees (a
pass with ``--lambda`` and, unless it is 0, a pass with ``--mu`` per iteration: the degrees of a vertex are one voxel's noisy sample and
their derivative mostly noise); then the gradient.  ``--output`` is the same mesh with the gradient's length, degrees per WORLD UNIT,
in its ``temperature`` property, its ``temperature_bounds`` from 0 to the steepest face: every tool that reads degrees reads it
(``mesh_thermogram.py`` draws the gradient image).  ``--smoothed`` writes the filled and smoothed degrees the gradient was taken of.
``--length-scale S`` is metres per world unit: the gradients of the report and ``--min-gradient`` are then degrees per metre (the
value per unit divided by S) and the report's areas square metres; the meshes and ``--min-area`` are not scaled.  ``--min-gradient G``
adds the regions that change faster than G, largest area first.
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

from thermo_nerf_amd.export.cli import json_number, load_mesh_ply, region_rows, require_rocm_device, write_report  # noqa: E402


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--smooth-iterations", type=int, default=0, metavar="N", help="smooth the degrees by N iterations first")
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.5, metavar="L", help="the factor of an iteration's first pass")
    ap.add_argument("--mu", type=float, default=0.0, metavar="M", help="the factor of its second pass; 0: none (plain diffusion)")
    ap.add_argument("--fill", type=int, default=0, metavar="N", help="fill the vertices without a temperature by at most N passes first")
    ap.add_argument("--output", type=Path, required=True, help="the mesh with degrees per world unit as its temperature")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--min-gradient", type=float, default=None, metavar="G", help="report the regions steeper than G degrees per metre")
    ap.add_argument("--min-area", type=float, default=0.0, metavar="A", help="drop regions below this area (the mesh's units squared)")
    ap.add_argument("--top", type=int, default=None, metavar="K", help="report the K largest regions only")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="S", help="metres per world unit")
    ap.add_argument("--smoothed", type=Path, default=None, help="also write the filled and smoothed degrees as a PLY")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.smooth_iterations < 0 or args.fill < 0:
        ap.error("--smooth-iterations and --fill must be >= 0")
    if not (math.isfinite(args.lambda_) and math.isfinite(args.mu)):
        ap.error("--lambda and --mu must be finite")
    if args.min_gradient is not None and (math.isnan(args.min_gradient) or args.min_gradient < 0.0):
        ap.error("--min-gradient must be a number >= 0")
    if args.min_gradient is None and (args.min_area != 0.0 or args.top is not None):
        ap.error("--min-area and --top go with --min-gradient")
    if math.isnan(args.min_area) or args.min_area < 0.0:
        ap.error("--min-area must be a number >= 0")
    if args.top is not None and args.top < 0:
        ap.error("--top must be >= 0")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def steep_rows(found, length_scale: float) -> list:
    """the rows of the regions above --min-gradient: ``region_rows``' area and centroid, the gradients in degrees per metre"""
    rows = []
    for base, row in zip(region_rows(found, True, length_scale), found.regions):
        rows.append({"region": base["region"], "faces": base["faces"], "area": base["area"], "centroid": base["centroid"],
                     "mean_gradient": float(row["mean_temperature"]) / length_scale, "max_gradient": float(row["max_temperature"]) / length_scale})
    return rows


def build_report(gradient, steep, num_vertices: int, num_faces: int, empty_before: int, empty_after: int, args) -> dict:
    """the JSON report: plain Python numbers; gradients divided by ``--length-scale`` (degrees per metre), areas times its square; a
    mesh without a usable face has null gradients"""
    s = float(args.length_scale)

    def per_metre(x):
        return None if json_number(x) is None else float(x) / s

    report = {"mesh": str(args.mesh), "length_scale": s, "smooth_iterations": int(args.smooth_iterations), "lambda": float(args.lambda_),
              "mu": float(args.mu), "fill_passes": int(args.fill),
              "counts": {"vertices": int(num_vertices), "faces": int(num_faces), "usable_faces": int(gradient.usable_faces)},
              "nan_vertices": {"before": int(empty_before), "after": int(empty_after)},
              "mean_gradient": per_metre(gradient.mean_magnitude), "max_gradient": per_metre(gradient.max_magnitude)}
    if steep is not None:
        report["min_gradient"] = float(args.min_gradient)
        report["steep"] = {"regions": steep_rows(steep, s), "area": float(steep.selected_area) * s * s,
                           "share": float(steep.selected_area / steep.mesh_area) if steep.mesh_area > 0.0 else 0.0}
        report["mesh_area"] = float(steep.mesh_area) * s * s
    return report


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import fill_temperature, smooth_temperature, thermal_gradient, thermal_regions, write_mesh_ply

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "analyses meshes"), with_bounds=True)
    empty_before = empty_after = int((~torch.isfinite(mesh.temperature)).sum().item())
    if args.fill:
        mesh, empty_after = fill_temperature(mesh, args.fill)
    if args.smooth_iterations:
        mesh = smooth_temperature(mesh, args.smooth_iterations, args.lambda_, args.mu)
    gradient = thermal_gradient(mesh)
    steep = None
    if args.min_gradient is not None:
        steep = thermal_regions(gradient.mesh, min_temperature=args.min_gradient * args.length_scale, min_area=args.min_area, top=args.top)
    report = build_report(gradient, steep, len(data["positions"]), len(data["triangles"]), empty_before, empty_after, args)

    def shown(x):
        return "none" if x is None else f"{x:.4g}"

    print(f"{args.mesh}: {report['counts']['vertices']} vertices, {report['counts']['faces']} faces, {report['counts']['usable_faces']} "
          f"usable; vertices without a temperature {empty_before} -> {empty_after}; gradient mean {shown(report['mean_gradient'])}, max "
          f"{shown(report['max_gradient'])} C per metre")
    for k, row in enumerate(report.get("steep", {}).get("regions", [])):
        c = row["centroid"]
        print(f"steep {k}: area {row['area']:.6g}, {row['faces']} faces, mean {row['mean_gradient']:.4g}, max {row['max_gradient']:.4g} C per "
              f"metre, centroid ({c[0]:.4g}, {c[1]:.4g}, {c[2]:.4g})")
    write_report(args.report, report)
    write_mesh_ply(args.output, gradient.mesh)
    print(f"wrote {args.output}: vertices {len(gradient.mesh)}, triangles {int(gradient.mesh.triangles.shape[0])}")
    if args.smoothed is not None:
        write_mesh_ply(args.smoothed, mesh)
        print(f"wrote {args.smoothed}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
