#!/usr/bin/env python
"""An orthographic thermogram of a thermal mesh: a scaled, distortion-free image of a PLY that ``tools/export_mesh.py`` wrote, seen
along an axis or any direction — every pixel has a known size in the mesh's units, a temperature and a position on the surface.
No run directory and no model: the PLY is all it reads.

    python tools/mesh_thermogram.py mesh.ply (--view +x|-x|+y|-y|+z|-z | --forward X Y Z --up X Y Z)
           (--pixel-size S | --width N) [--near A --far B] [--cull-back] [--colors thermal|rgb] [--length-scale L]
           --output thermogram.png [--temperatures t.npy] [--report thermogram.json]

``--view -y`` looks along -y with +z up (``+z`` / ``-z`` look along the z axis with +y up); ``--forward`` with ``--up`` gives any
other direction.  ``--pixel-size`` is in the mesh's units, ``--width`` in pixels (two empty pixels of margin on every side included).
``--near`` / ``--far`` keep the surface between two depths, counted along the view from the mesh's nearest vertex: a slab that cuts
the mesh open.  ``--cull-back`` drops the faces seen from behind.  ``--colors thermal`` maps the temperatures through the magma table
over the file's ``temperature_bounds`` (over the image's own range if the file names none), ``rgb`` shows the file's colours; empty
pixels are black.  ``--temperatures`` writes the degrees Celsius per pixel as a float32 ``.npy``, NaN where empty.  ``--report``
writes the view (origin, axes, pixel size, width, height, near, far), the counts, the covered area, the mean / min / max degrees and
the hottest and coldest pixel with row, column, world position and face as JSON; ``--length-scale L`` multiplies its lengths by L
and its areas by L^2, as in ``tools/mesh_regions.py``.  One summary line is printed.
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

# --view: (forward, up)
VIEWS = {"+x": ((1, 0, 0), (0, 0, 1)), "-x": ((-1, 0, 0), (0, 0, 1)), "+y": ((0, 1, 0), (0, 0, 1)), "-y": ((0, -1, 0), (0, 0, 1)),
         "+z": ((0, 0, 1), (0, 1, 0)), "-z": ((0, 0, -1), (0, 1, 0))}


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--view", choices=sorted(VIEWS), default=None, help="look along an axis")
    ap.add_argument("--forward", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="look along this direction (with --up)")
    ap.add_argument("--up", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="what points up in the image")
    ap.add_argument("--pixel-size", type=float, default=None, metavar="S", help="the mesh's units per pixel")
    ap.add_argument("--width", type=int, default=None, metavar="N", help="the image's width in pixels, margins included")
    ap.add_argument("--near", type=float, default=-math.inf, metavar="A", help="keep the surface from this depth on")
    ap.add_argument("--far", type=float, default=math.inf, metavar="B", help="keep the surface up to this depth")
    ap.add_argument("--cull-back", action="store_true", help="drop the faces seen from behind")
    ap.add_argument("--colors", choices=("thermal", "rgb"), default="thermal", help="what the PNG shows")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="L", help="multiply the report's lengths by L and its areas by L^2")
    ap.add_argument("--output", type=Path, required=True, help="the PNG to write")
    ap.add_argument("--temperatures", type=Path, default=None, help="also write the degrees Celsius per pixel as .npy")
    ap.add_argument("--report", type=Path, default=None, help="also write a JSON report")
    ap.add_argument("--device", default="cuda")
    given, joined = list(sys.argv[1:] if argv is None else argv), []
    for a in given:  # "--view -y": argparse would take -y for an option
        if joined and joined[-1] == "--view" and a in VIEWS:
            joined[-1] = f"--view={a}"
        else:
            joined.append(a)
    args = ap.parse_args(joined)
    if (args.view is None) == (args.forward is None):
        ap.error("give --view, or --forward with --up (not both)")
    if args.view is not None and args.up is not None:
        ap.error("--up goes with --forward; --view has its own")
    if args.forward is not None and args.up is None:
        ap.error("--forward needs --up")
    if (args.pixel_size is None) == (args.width is None):
        ap.error("give exactly one of --pixel-size and --width")
    if args.pixel_size is not None and not (args.pixel_size > 0.0 and math.isfinite(args.pixel_size)):
        ap.error("--pixel-size must be positive and finite")
    if args.width is not None and not 5 <= args.width <= 16384:
        ap.error("--width must be 5 .. 16384 (two pixels of margin on each side)")
    if math.isnan(args.near) or math.isnan(args.far):
        ap.error("--near / --far must not be NaN")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    args.forward, args.up = VIEWS[args.view] if args.view is not None else (tuple(args.forward), tuple(args.up))
    return args


def build_report(found, temperature, face, depth, num_vertices: int, num_faces: int, length_scale: float = 1.0, source: str = "") -> dict:
    """the JSON report of ``found`` (a ``Thermogram``) over the host arrays ``temperature``, ``face`` and ``depth`` [H, W] of its
    images: plain Python numbers; lengths times ``length_scale``, areas times its square.  The hottest / coldest pixel is the first
    in row-major order among the equals."""
    import numpy as np

    from thermo_nerf_amd.export.thermogram import pixel_position

    s, s2 = float(length_scale), float(length_scale) ** 2
    view = found.view

    def pixel(flat):
        row, col = divmod(int(flat), int(view.width))
        return {"row": row, "column": col, "temperature": float(temperature[row, col]), "face": int(face[row, col]),
                "position": [c * s for c in pixel_position(view, row, col, float(depth[row, col]))]}

    covered = ~np.isnan(temperature)
    hottest = coldest = None
    if covered.any():
        hottest = pixel(np.argmax(np.where(covered, temperature, -np.inf)))
        coldest = pixel(np.argmin(np.where(covered, temperature, np.inf)))
    return {"mesh": source, "length_scale": s,
            "view": {"origin": [float(c) * s for c in view.origin], "right": [float(c) for c in view.right],
                     "down": [float(c) for c in view.down], "forward": [float(c) for c in view.forward],
                     "pixel_size": float(view.pixel_size) * s, "width": int(view.width), "height": int(view.height),
                     "near": None if json_number(view.near) is None else view.near * s, "far": None if json_number(view.far) is None else view.far * s,
                     "cull_back": bool(view.cull)},
            "counts": {"vertices": int(num_vertices), "faces": int(num_faces), "usable_faces": int(found.usable_faces),
                       "drawn_faces": int(found.drawn_faces), "pixels": int(view.width) * int(view.height),
                       "covered_pixels": int(found.covered)},
            "covered_area": float(found.covered_area) * s2,
            "mean_temperature": json_number(found.mean_temperature), "min_temperature": json_number(found.min_temperature),
            "max_temperature": json_number(found.max_temperature), "hottest_pixel": hottest, "coldest_pixel": coldest}


def summary_line(report: dict, source) -> str:
    c, v = report["counts"], report["view"]
    if not c["covered_pixels"]:
        return f"{source}: {v['width']} x {v['height']} pixels of {v['pixel_size']:.6g}, nothing covered ({c['drawn_faces']} of {c['faces']} faces drawn)"
    return (f"{source}: {v['width']} x {v['height']} pixels of {v['pixel_size']:.6g}, {c['covered_pixels']} covered "
            f"(area {report['covered_area']:.6g}), {c['drawn_faces']} of {c['faces']} faces drawn, mean {report['mean_temperature']:.2f} C "
            f"(min {report['min_temperature']:.2f}, max {report['max_temperature']:.2f})")


def main(argv=None) -> int:
    args = parse(argv)

    import numpy as np
    from PIL import Image

    from thermo_nerf_amd.export import fit_view, mesh_thermogram

    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "rasterises meshes"), with_bounds=True)
    view = fit_view(mesh.positions, args.forward, args.up, pixel_size=args.pixel_size, width=args.width, near=args.near, far=args.far,
                    cull=args.cull_back)
    found = mesh_thermogram(mesh, view)
    image = found.to_rgb8(args.colors).cpu().numpy()
    args.output.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(image, "RGB").save(args.output)
    temperature = found.pixel_temperature.cpu().numpy()
    report = build_report(found, temperature, found.pixel_face.cpu().numpy(), found.pixel_depth.cpu().numpy(), len(data["positions"]),
                          len(data["triangles"]), args.length_scale, str(args.mesh))
    print(summary_line(report, args.mesh))
    if args.temperatures is not None:
        args.temperatures.parent.mkdir(parents=True, exist_ok=True)
        with open(args.temperatures, "wb") as f:  # (np.save given a name would append .npy to one without it)
            np.save(f, temperature)
    if args.report is not None:
        write_report(args.report, report, say=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
