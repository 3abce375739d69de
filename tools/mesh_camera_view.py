#!/usr/bin/env python
"""A thermal mesh seen from the camera that took one of the dataset's photos: the image that can be laid beside — or over — the
measured thermal image of that frame, pixel for pixel, and what lies behind single pixels.  No run directory and no model: a PLY
that ``tools/export_mesh.py`` wrote and the dataset's ``transforms.json`` are all it reads.

    python tools/mesh_camera_view.py mesh.ply --transforms transforms.json --frame NAME_OR_INDEX [--scale F] [--cull-back]
           [--colors thermal|rgb] --output view.png [--temperatures t.npy] [--report view.json] [--probe ROW COL ...]

``--frame`` is a frame's ``file_path`` (or its last component) or its index in the file's ``frames`` list as written.  The intrinsics
(``fl_x``, ``fl_y``, ``cx``, ``cy``, ``w``, ``h``) are read the way ``thermo_nerf_amd/data/thermal_dataparser.py`` reads them: from
the file's top level, else from the frame; the pose is the frame's ``transform_matrix`` (camera-to-world, the camera looks along its
-z with +y up).  Lens distortion is ignored.  The exporters write their PLYs in the dataset's original world frame
(``thermo_nerf_amd/export/pointcloud.py``'s ``world_transform`` undoes the dataparser's orientation, centring and scale, and the
``applied_transform`` / ``applied_scale`` the file names), so a pose is used as written, after undoing ``applied_transform`` and
``applied_scale`` where the file carries them; a PLY written with ``--scene-frame`` does not match.  ``--scale F`` multiplies the
image size and the intrinsics by F (0.5: half the resolution).  ``--cull-back`` drops the faces seen from behind.  ``--colors
thermal`` maps the temperatures through the magma table over the file's ``temperature_bounds`` (the image's own range if the PLY
names none), ``rgb`` shows the PLY's colours; empty pixels are black.  ``--temperatures`` writes the degrees Celsius per pixel as a
float32 ``.npy``, NaN where empty.  ``--report`` writes the camera, the counts, the covered share, the mean / min / max degrees and
the hottest and coldest pixel with row, column, distance, world position and face as JSON.  Each ``--probe ROW COL`` prints the
degrees, the distance, the face and the world position behind that pixel.  One summary line is printed.
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

from thermo_nerf_amd.export.cli import frame_camera, json_number, load_mesh_ply, require_rocm_device, write_report  # noqa: E402,F401

def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", type=Path, help="a mesh PLY written by tools/export_mesh.py")
    ap.add_argument("--transforms", type=Path, required=True, help="the dataset's transforms.json")
    ap.add_argument("--frame", required=True, metavar="NAME_OR_INDEX", help="a frame's file_path, its last component, or its index")
    ap.add_argument("--scale", type=float, default=1.0, metavar="F", help="multiply the image size and the intrinsics by F")
    ap.add_argument("--cull-back", action="store_true", help="drop the faces seen from behind")
    ap.add_argument("--colors", choices=("thermal", "rgb"), default="thermal", help="what the PNG shows")
    ap.add_argument("--output", type=Path, required=True, help="the PNG to write")
    ap.add_argument("--temperatures", type=Path, default=None, help="also write the degrees Celsius per pixel as .npy")
    ap.add_argument("--report", type=Path, default=None, help="also write a JSON report")
    ap.add_argument("--probe", type=int, nargs=2, action="append", default=[], metavar=("ROW", "COL"), help="print what lies behind a pixel")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not (args.scale > 0.0 and math.isfinite(args.scale)):
        ap.error("--scale must be positive and finite")
    if any(r < 0 or c < 0 for r, c in args.probe):
        ap.error("--probe takes a row and a column, both >= 0")
    return args


def find_frame(meta: dict, wanted: str) -> int:
    """the index in ``meta["frames"]`` of the frame named ``wanted``: its file_path, the last component of it, or an index"""
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError("the transforms file has no frames")
    names = [str(f.get("file_path", "")) for f in frames]
    exact = [k for k, n in enumerate(names) if n == wanted]
    tail = [k for k, n in enumerate(names) if Path(n).name == wanted or Path(n).stem == wanted]
    for found in (exact, tail):
        if len(found) == 1:
            return found[0]
        if len(found) > 1:
            raise ValueError(f"--frame {wanted}: {len(found)} frames carry that name")
    try:
        index = int(wanted)
    except ValueError:
        raise ValueError(f"--frame {wanted}: no frame of that name among {len(frames)}") from None
    if not 0 <= index < len(frames):
        raise ValueError(f"--frame {index}: the file has frames 0 .. {len(frames) - 1}")
    return index


def pixel_record(camera: dict, origins, directions, temperature, face, distance, row: int, col: int) -> dict:
    """what lies behind pixel (row, col), over host arrays: ``origins`` / ``directions`` [H W, 3], the images [H, W]"""
    k = row * int(camera["width"]) + col
    d = float(distance[row, col])
    position = [float(origins[k][a]) + d * float(directions[k][a]) for a in range(3)]
    shown = not math.isnan(float(temperature[row, col]))
    return {"row": int(row), "column": int(col), "temperature": float(temperature[row, col]) if shown else None,
            "distance": d if shown else None, "face": int(face[row, col]), "position": position if shown else None}


def build_report(camera: dict, frame_name: str, frame_index: int, found, origins, directions, temperature, face, distance,
                 num_vertices: int, num_faces: int, cull_back: bool, source: str = "") -> dict:
    """the JSON report of ``found`` (a ``CameraThermogram``, or anything with its numbers) over the host arrays of its images and
    rays: plain Python numbers.  The hottest / coldest pixel is the first in row-major order among the equals."""
    import numpy as np

    width, height = int(camera["width"]), int(camera["height"])
    covered = ~np.isnan(temperature)
    hottest = coldest = None
    if covered.any():
        hot, cold = int(np.argmax(np.where(covered, temperature, -np.inf))), int(np.argmin(np.where(covered, temperature, np.inf)))
        hottest = pixel_record(camera, origins, directions, temperature, face, distance, *divmod(hot, width))
        coldest = pixel_record(camera, origins, directions, temperature, face, distance, *divmod(cold, width))
    pixels = width * height
    return {"mesh": source, "frame": frame_name, "frame_index": int(frame_index),
            "camera": {"c2w": [[float(x) for x in row] for row in camera["c2w"]], "fx": float(camera["fx"]), "fy": float(camera["fy"]),
                       "cx": float(camera["cx"]), "cy": float(camera["cy"]), "width": width, "height": height, "cull_back": bool(cull_back)},
            "counts": {"vertices": int(num_vertices), "faces": int(num_faces), "usable_faces": int(found.usable_faces), "pixels": pixels,
                       "covered_pixels": int(found.covered), "stack_limit_rays": int(found.stack_limit_rays)},
            "covered_share": float(found.covered) / pixels,
            "mean_temperature": json_number(found.mean_temperature), "min_temperature": json_number(found.min_temperature),
            "max_temperature": json_number(found.max_temperature), "hottest_pixel": hottest, "coldest_pixel": coldest}


def summary_line(report: dict, source) -> str:
    c, cam = report["counts"], report["camera"]
    head = f"{source} from {report['frame']}: {cam['width']} x {cam['height']} pixels"
    if not c["covered_pixels"]:
        return f"{head}, nothing covered ({c['usable_faces']} of {c['faces']} faces usable)"
    return (f"{head}, {c['covered_pixels']} covered ({100.0 * report['covered_share']:.1f} %), mean {report['mean_temperature']:.2f} C "
            f"(min {report['min_temperature']:.2f}, max {report['max_temperature']:.2f})")


def probe_line(record: dict) -> str:
    at = f"probe ({record['row']}, {record['column']})"
    if record["temperature"] is None:
        return f"{at}: nothing there"
    x, y, z = record["position"]
    return f"{at}: {record['temperature']:.2f} C at distance {record['distance']:.6g}, face {record['face']}, position ({x:.6g}, {y:.6g}, {z:.6g})"


def main(argv=None) -> int:
    args = parse(argv)

    import numpy as np
    from PIL import Image

    from thermo_nerf_amd.export import CameraView, build_mesh_bvh, mesh_camera_thermogram

    meta = json.loads(args.transforms.read_text())
    index = find_frame(meta, args.frame)
    camera = frame_camera(meta, index, args.scale)
    for row, col in args.probe:
        if row >= camera["height"] or col >= camera["width"]:
            raise ValueError(f"--probe {row} {col}: the image has {camera['height']} rows and {camera['width']} columns")
    mesh, data = load_mesh_ply(args.mesh, require_rocm_device(args.device, "casts rays"), with_bounds=True)
    view = CameraView(camera["c2w"], camera["fx"], camera["fy"], camera["cx"], camera["cy"], camera["width"], camera["height"])
    found = mesh_camera_thermogram(build_mesh_bvh(mesh), view, cull=args.cull_back)
    image = found.to_rgb8(args.colors).cpu().numpy()
    args.output.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(image, "RGB").save(args.output)
    temperature, face, distance = (x.cpu().numpy() for x in (found.pixel_temperature, found.pixel_face, found.pixel_distance))
    origins, directions = found.origins.cpu().numpy(), found.directions.cpu().numpy()
    name = str(meta["frames"][index].get("file_path", index))
    report = build_report(camera, name, index, found, origins, directions, temperature, face, distance, len(data["positions"]),
                          len(data["triangles"]), args.cull_back, str(args.mesh))
    print(summary_line(report, args.mesh))
    for row, col in args.probe:
        print(probe_line(pixel_record(camera, origins, directions, temperature, face, distance, row, col)))
    if args.temperatures is not None:
        args.temperatures.parent.mkdir(parents=True, exist_ok=True)
        with open(args.temperatures, "wb") as f:  # (np.save given a name would append .npy to one without it)
            np.save(f, temperature)
    if args.report is not None:
        write_report(args.report, report, say=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
