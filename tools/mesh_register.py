#!/usr/bin/env python
"""Register one thermal mesh to another — this winter's survey into the frame of last winter's, the step between
``tools/export_mesh.py`` and ``tools/mesh_compare.py``: two reconstructions of one building have each their own origin, orientation
and unit, and the comparison needs both in ONE frame.  Both are PLYs that ``tools/export_mesh.py`` wrote; no run directory and no
model.

    python tools/mesh_register.py moving.ply fixed.ply [--initial M.txt | --pairs pairs.txt] --max-distance R [R2 ...]
           [--metric plane|point] [--with-scale] [--iterations N] [--max-points P]
           --output registered.ply --matrix out.txt --report register.json

The vertices of the moving mesh are matched with the nearest points of the fixed mesh's surface within ``--max-distance`` and a
Gauss-Newton step moves them closer, until nothing moves (iterated closest points on the device).  It needs a start near the answer:
``--initial`` is a text file with a 3 x 4 or 4 x 4 matrix (moving -> fixed), ``--pairs`` a text file with one picked pair per line,
``x y z  X Y Z`` — a point of the moving mesh and the same point in the fixed mesh, at least three, not on one line —, from which the
closed-form similarity is the start (with its scale under ``--with-scale``).  Several radii run coarse to fine, each stage from the
last result.  ``--with-scale`` also estimates a uniform scale (two COLMAP frames differ in unit).  ``--max-points`` strides the
vertices down.  ``--output`` gets the moving mesh in the fixed mesh's frame, which ``tools/mesh_compare.py`` reads as it is;
``--matrix`` the 4 x 4 matrix as text; ``--report`` the status, iterations, scale, matrix, matched share and the RMS per stage.
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
    ap.add_argument("moving", type=Path, help="the mesh that is moved (a PLY written by tools/export_mesh.py)")
    ap.add_argument("fixed", type=Path, help="the mesh whose frame is kept: its surface is searched")
    start = ap.add_mutually_exclusive_group()
    start.add_argument("--initial", type=Path, default=None, metavar="M.txt", help="a 3 x 4 or 4 x 4 matrix as text: the start")
    start.add_argument("--pairs", type=Path, default=None, metavar="pairs.txt", help="picked pairs 'x y z X Y Z', one per line: the start")
    ap.add_argument("--max-distance", type=float, nargs="+", required=True, metavar="R", help="match within this distance (the fixed mesh's units); several: coarse to fine")
    ap.add_argument("--metric", choices=("plane", "point"), default="plane")
    ap.add_argument("--with-scale", action="store_true", help="also estimate a uniform scale")
    ap.add_argument("--iterations", type=int, default=30, metavar="N", help="at most N iterations per stage")
    ap.add_argument("--max-points", type=int, default=None, metavar="P", help="use about P of the moving mesh's vertices")
    ap.add_argument("--output", type=Path, required=True, help="the moving mesh in the fixed mesh's frame, as a PLY")
    ap.add_argument("--matrix", type=Path, required=True, help="the 4 x 4 matrix (moving -> fixed) as text")
    ap.add_argument("--report", type=Path, required=True, help="the JSON report to write")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if any(math.isnan(r) or r < 0.0 for r in args.max_distance):
        ap.error("--max-distance must be numbers >= 0")
    if not 1 <= args.iterations <= 1024:
        ap.error("--iterations must be in 1 .. 1024")
    if args.max_points is not None and args.max_points < 1:
        ap.error("--max-points must be >= 1")
    return args


def starting_matrix(initial, pairs, with_scale: bool):
    """the 4 x 4 start from --initial or --pairs; None without either (the identity)"""
    import numpy as np

    from thermo_nerf_amd.export import similarity_from_pairs

    if initial is not None:
        m = np.loadtxt(initial, dtype=np.float64)
        if m.shape == (3, 4):
            m = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
        if m.shape != (4, 4):
            raise ValueError(f"{initial}: a 3 x 4 or 4 x 4 matrix is expected, found {m.shape}")
        return m
    if pairs is not None:
        rows = np.atleast_2d(np.loadtxt(pairs, dtype=np.float64))
        if rows.shape[1] != 6 or len(rows) < 3:
            raise ValueError(f"{pairs}: at least three lines of six numbers 'x y z X Y Z' are expected")
        return similarity_from_pairs(rows[:, :3], rows[:, 3:], with_scale=with_scale)
    return None


def build_report(found, vertices: int, points: int, source: str = "", reference: str = "", metric: str = "plane", with_scale: bool = False,
                 start=None) -> dict:
    """the JSON report of ``found`` (a ``Registration``): plain Python numbers, None where there is no value"""
    return {"moving": source, "fixed": reference, "metric": metric, "with_scale": bool(with_scale), "vertices": int(vertices),
            "points": int(points), "status": found.status, "iterations": int(found.iterations), "scale": float(found.scale),
            "matrix": [[float(x) for x in row] for row in found.matrix], "start": None if start is None else [[float(x) for x in row] for row in start],
            "matched": int(found.matched), "matched_share": float(found.matched_share), "usable_points": int(found.usable_points),
            "rms": [json_number(x) for x in found.rms],
            "stages": [{"max_distance": json_number(s["max_distance"]), "status": s["status"], "iterations": int(s["iterations"]),
                        "matched": int(s["matched"]), "matched_share": float(s["matched_share"]), "rms": json_number(s["rms"])} for s in found.stages]}


def summary_line(report: dict) -> str:
    last = report["stages"][-1]
    rms = "-" if last["rms"] is None else f"{last['rms']:.4g}"
    return (f"{report['moving']} onto {report['fixed']}: {report['status']} after {report['iterations']} iterations in {len(report['stages'])} "
            f"stage(s), {report['matched']} of {report['points']} matched ({100.0 * report['matched_share']:.1f} %), rms {rms}, scale {report['scale']:.6g}")


def main(argv=None) -> int:
    args = parse(argv)

    import numpy as np

    from thermo_nerf_amd.export import build_mesh_bvh, register_mesh, transform_mesh, write_mesh_ply

    dev = require_rocm_device(args.device, "registers meshes")
    moving, data = load_mesh_ply(args.moving, dev, with_bounds=False)
    fixed, _ = load_mesh_ply(args.fixed, dev, with_bounds=False)
    start = starting_matrix(args.initial, args.pairs, args.with_scale)
    found = register_mesh(moving, build_mesh_bvh(fixed), max_points=args.max_points, initial=start, max_distance=list(args.max_distance),
                          metric=args.metric, with_scale=args.with_scale, iterations=args.iterations)
    points = len(data["positions"]) if args.max_points is None else len(range(0, len(data["positions"]), -(-len(data["positions"]) // args.max_points)))
    report = build_report(found, len(data["positions"]), points, str(args.moving), str(args.fixed), args.metric, args.with_scale, start)
    print(summary_line(report))
    for path in (args.matrix, args.output):
        path.parent.mkdir(parents=True, exist_ok=True)
    write_report(args.report, report)
    np.savetxt(args.matrix, found.matrix, fmt="%.17g")
    print(f"wrote {args.matrix}")
    if found.status in ("too_few", "degenerate"):
        print(f"nothing was registered ({found.status}): {args.output} is not written; give a start (--initial, --pairs) or a larger --max-distance")
        return 1
    moved = transform_mesh(moving, found.matrix)
    write_mesh_ply(args.output, moved)
    print(f"wrote {args.output}: vertices {len(moved)}, triangles {int(moved.triangles.shape[0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
