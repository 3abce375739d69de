#!/usr/bin/env python
"""Project the dataset's measured thermal photos onto a thermal mesh: what did the camera actually measure at every vertex, from how
many photos was it seen and do they agree, and where does the model differ from the photos.  No run directory and no model: a PLY
that ``tools/export_mesh.py`` wrote and the dataset's ``transforms.json`` with its thermal images are all it reads.

    python tools/mesh_project.py mesh.ply --transforms DATASET/transforms.json [--frames all|train|eval]
           --output measured.ply [--residual residual.ply] [--report project.json]
           [--temperature-bounds MAX MIN] [--min-cos 0.2] [--two-sided] [--min-change X] [--length-scale S]

Every frame's camera is ``frame_camera`` of ``tools/mesh_camera_view.py`` (the intrinsics from the file's top level, else from the
frame; the pose as written with ``applied_transform`` / ``applied_scale`` undone: the exporters write their PLYs in the dataset's
original world frame, a PLY written with ``--scene-frame`` does not match).  Lens distortion is ignored, as there.  Every frame's photo
is its ``thermal_file_path`` beside the transforms file, read as ``thermo_nerf_amd/data/thermal_dataset.py`` reads it (greyscale, 8
bits); all photos share one size, which must be the cameras'.  ``--frames train`` / ``eval`` keeps the frames with "train" / "eval"
in the base name of their ``file_path`` (the dataset's filename split).  Byte 0 is the lower and byte 255 the upper of the
temperature bounds: the PLY's ``temperature_bounds`` comment, or ``--temperature-bounds MAX MIN`` in degrees Celsius (the order of
the training command line).  A vertex takes a photo when it lies in front of the camera and inside the image, faces it with
cos >= ``--min-cos`` against its vertex normal (``--two-sided``: |cos|, for meshes whose normals point inward) and nothing of the mesh
hides it; the photos are fused with the weight cos / distance^2.

``--output`` gets the mesh with the MEASURED degrees as its ``temperature`` (NaN where no photo shows the vertex), ``--residual`` the
mesh with model minus measurement and ``temperature_bounds`` -m m: ``tools/mesh_regions.py``, ``tools/mesh_thermogram.py`` and
``tools/mesh_camera_view.py`` read both like any mesh.  ``--report`` gets the counts, the seen share, the mean number of views, the
residual's mean / RMS / min / max and the mean / max spread (warmest minus coldest view of a vertex: what moves with the viewpoint is a
reflection).  ``--min-change X`` adds the regions where the model is at least X degrees above the photos and those where it is at least
X below (``thermal_regions`` on the residual mesh, as ``tools/mesh_compare.py`` builds warmed / cooled) and prints one line each.
``--length-scale S`` multiplies the report's areas by S^2 and its centroids by S.  One summary line is printed.
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

from thermo_nerf_amd.export.cli import (add_difference_regions, difference_region_lines, file_bounds, frame_camera,  # noqa: E402
                                        json_number, load_mesh_ply, require_rocm_device, write_report)


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--transforms", type=Path, required=True, help="the dataset's transforms.json (the thermal images lie beside it)")
    ap.add_argument("--frames", choices=("all", "train", "eval"), default="all", help="which frames' photos to project")
    ap.add_argument("--output", type=Path, required=True, help="the mesh with the measured degrees as its temperature, as a PLY")
    ap.add_argument("--residual", type=Path, default=None, help="also write the mesh with model minus measurement, as a PLY")
    ap.add_argument("--report", type=Path, default=None, help="also write a JSON report")
    ap.add_argument("--temperature-bounds", type=float, nargs=2, default=None, metavar=("MAX", "MIN"),
                    help="degrees Celsius of byte 255 and of byte 0 (default: the PLY's temperature_bounds comment)")
    ap.add_argument("--min-cos", type=float, default=0.2, help="take a photo only where cos(normal, direction to the camera) >= this")
    ap.add_argument("--two-sided", action="store_true", help="use |cos|: the normals may point either way")
    ap.add_argument("--min-change", type=float, default=None, metavar="X", help="also report the regions where model and photos differ by >= X degrees")
    ap.add_argument("--length-scale", type=float, default=1.0, metavar="S", help="multiply the report's areas by S^2 and its centroids by S")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not 0.0 < args.min_cos <= 1.0:
        ap.error("--min-cos must be in (0, 1]")
    if args.temperature_bounds is not None:
        high, low = args.temperature_bounds
        if not (math.isfinite(high) and math.isfinite(low) and high > low):
            ap.error("--temperature-bounds takes MAX MIN, finite, MAX above MIN")
    if args.min_change is not None and not (args.min_change > 0.0 and math.isfinite(args.min_change)):
        ap.error("--min-change must be positive and finite")
    if not (args.length_scale > 0.0 and math.isfinite(args.length_scale)):
        ap.error("--length-scale must be positive and finite")
    return args


def select_frames(meta: dict, which: str) -> list:
    """the indices in ``meta["frames"]`` of the frames to project: all, or those with "train" / "eval" in their file's base name"""
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError("the transforms file has no frames")
    index = [k for k, f in enumerate(frames) if which == "all" or which in Path(str(f.get("file_path", ""))).name]
    if not index:
        raise ValueError(f"--frames {which}: none of the {len(frames)} frames carries \"{which}\" in its file name")
    missing = [k for k in index if "thermal_file_path" not in frames[k]]
    if missing:
        raise ValueError(f"frame {missing[0]} names no thermal_file_path ({len(missing)} of {len(index)} frames do not)")
    return index


def load_photos(meta: dict, index, data_dir: Path, width: int, height: int):
    """uint8 [K, H, W]: the thermal photo of every chosen frame, read as the dataset reads it"""
    import numpy as np
    from PIL import Image

    photos = np.zeros((len(index), height, width), np.uint8)
    for row, k in enumerate(index):
        path = data_dir / meta["frames"][k]["thermal_file_path"]
        if not path.exists():
            raise FileNotFoundError(f"No file found at {path}")
        pil = Image.open(path)
        if pil.mode != "L":
            pil = pil.convert("L")
        image = np.asarray(pil, dtype=np.uint8)
        if image.shape != (height, width):
            raise ValueError(f"{path} is {image.shape[1]} x {image.shape[0]} pixels, the cameras are {width} x {height}: all photos share one size")
        photos[row] = image
    return photos


def build_report(found, vertices, faces, frames, width, height, bounds, min_cos: float, two_sided: bool, length_scale: float = 1.0,
                 above=None, below=None, min_change=None, source: str = "", transforms: str = "", which: str = "all") -> dict:
    """the JSON report of ``found`` (a ``MeshMeasurement``, or anything with its numbers): plain Python numbers, None where there is
    no value.  ``above`` / ``below``: the ``ThermalRegions`` of --min-change (model above / below the photos), or None."""
    s = float(length_scale)
    p = found.projected
    report = {"mesh": source, "transforms": transforms, "frames": which, "length_scale": s,
              "temperature_bounds": [float(bounds[0]), float(bounds[1])], "min_cos": float(min_cos), "two_sided": bool(two_sided),
              "image": {"width": int(width), "height": int(height)},
              "counts": {"vertices": int(vertices), "faces": int(faces), "frames": int(frames), "usable_vertices": int(p.usable_points),
                         "usable_cameras": int(p.usable_cameras), "seen_vertices": int(found.seen), "tested_pairs": int(p.tested_pairs),
                         "accepted_pairs": int(p.accepted_pairs), "stack_limit_pairs": int(p.stack_limit_pairs)},
              "seen_share": float(found.seen_share), "mean_views": float(found.mean_views),
              "residual": {"mean": json_number(found.mean_difference), "rms": json_number(found.rms_difference), "min": json_number(found.min_difference),
                           "max": json_number(found.max_difference)},
              "spread": {"mean": json_number(found.mean_spread), "max": json_number(found.max_spread)}}
    if min_change is not None:
        add_difference_regions(report, ("model_above", "model_below"), above, below, min_change, s)
    return report


def summary_line(report: dict) -> str:
    c, r, sp = report["counts"], report["residual"], report["spread"]
    head = f"{report['mesh']} under {c['frames']} photos: {c['vertices']} vertices"
    if not c["seen_vertices"]:
        return f"{head}, none seen ({c['usable_cameras']} usable cameras, {c['tested_pairs']} pairs in view)"
    return (f"{head}, {c['seen_vertices']} seen ({100.0 * report['seen_share']:.1f} %), {report['mean_views']:.2f} views each, "
            f"model - photos mean {r['mean']:+.2f} C rms {r['rms']:.2f} min {r['min']:+.2f} max {r['max']:+.2f}, "
            f"spread mean {sp['mean']:.2f} max {sp['max']:.2f}")


def region_lines(report: dict) -> list:
    return difference_region_lines(report, ("model_above", "model_below"))


def main(argv=None) -> int:
    args = parse(argv)

    import torch

    from thermo_nerf_amd.export import CameraView, build_mesh_bvh, mesh_measurement, thermal_regions, write_mesh_ply

    meta = json.loads(args.transforms.read_text())
    index = select_frames(meta, args.frames)
    cameras = [frame_camera(meta, k) for k in index]
    views = [CameraView(c["c2w"], c["fx"], c["fy"], c["cx"], c["cy"], c["width"], c["height"]) for c in cameras]
    width, height = views[0].width, views[0].height
    photos = load_photos(meta, index, args.transforms.parent, width, height)
    dev = require_rocm_device(args.device, "projects photos")
    mesh, data = load_mesh_ply(args.mesh, dev, with_bounds=False)
    if args.temperature_bounds is not None:
        bounds = (args.temperature_bounds[1], args.temperature_bounds[0])
    else:
        bounds = file_bounds(data["comments"])
        if bounds is None:
            raise ValueError(f"{args.mesh} names no temperature_bounds: pass --temperature-bounds MAX MIN")
    found = mesh_measurement(mesh, build_mesh_bvh(mesh), views, torch.from_numpy(photos).to(dev), bounds, min_cos=args.min_cos,
                             two_sided=args.two_sided)
    above = below = None
    if args.min_change is not None:
        above = thermal_regions(found.residual, min_temperature=args.min_change)
        below = thermal_regions(found.residual, max_temperature=-args.min_change)
    report = build_report(found, len(data["positions"]), len(data["triangles"]), len(index), width, height, bounds, args.min_cos,
                          args.two_sided, args.length_scale, above, below, args.min_change, str(args.mesh), str(args.transforms), args.frames)
    print(summary_line(report))
    for line in region_lines(report):
        print(line)
    write_mesh_ply(args.output, found.measured)
    print(f"wrote {args.output}: vertices {len(found.measured)}, triangles {int(found.measured.triangles.shape[0])}")
    if args.residual is not None:
        write_mesh_ply(args.residual, found.residual)
        print(f"wrote {args.residual}")
    if args.report is not None:
        write_report(args.report, report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
