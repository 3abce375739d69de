"""What the mesh command lines under tools/ share: a PLY onto the device, the ``--device`` refusal, the numbers and the tail of a JSON
report, the rows and lines of the regions of a difference mesh, a frame of a ``transforms.json`` as a camera."""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import torch

from .. import colormaps
from .mesh import ThermalMesh
from .ply import read_mesh_ply


def require_rocm_device(name: str, verb: str) -> torch.device:
    """``--device NAME`` as a device; ``verb``: what the command line does to meshes, for the refusal of anything but a ROCm device"""
    dev = torch.device(name)
    if dev.type != "cuda":
        raise RuntimeError(f"--device {name}: thermo_nerf_amd {verb} only on a ROCm device (no CPU fallback exists)")
    return dev


def file_bounds(comments):
    """the (lo, hi) of the file's ``temperature_bounds`` comment, or None"""
    for line in comments:
        parts = line.split()
        if len(parts) == 3 and parts[0] == "temperature_bounds" and parts[1] != "none":
            return float(parts[1]), float(parts[2])
    return None


def load_mesh_ply(path, device, with_bounds: bool):
    """(the ``ThermalMesh`` of a PLY on ``device``, the host arrays of ``read_mesh_ply``); ``with_bounds``: the mesh carries the file's
    ``temperature_bounds``, else none"""
    data = read_mesh_ply(path)
    normals = data.get("normals")
    mesh = ThermalMesh(torch.from_numpy(data["positions"].copy()).to(device), torch.from_numpy(data["colors"].copy()).to(device),
                       torch.from_numpy(data["temperature"].copy()).to(device), None, torch.from_numpy(data["triangles"].copy()).to(device),
                       file_bounds(data["comments"]) if with_bounds else None,
                       None if normals is None else torch.from_numpy(normals.copy()).to(device))
    return mesh, data


def thermal_bytes(temperature, bounds):
    """uint8 [M,3]: the magma table at trunc(256 (t - lo) / (hi - lo)), clamped to the table"""
    t = np.asarray(temperature, np.float64)
    lo, hi = bounds if bounds is not None else ((float(t.min()), float(t.max())) if len(t) else (0.0, 1.0))
    x = (t - lo) / (hi - lo) if hi > lo else np.zeros_like(t)
    index = np.clip(np.nan_to_num(np.trunc(x * 256.0), nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.int64)
    return colormaps.table_u8("magma")[index]


def json_number(x, keep_nan: bool = False):
    """a float for JSON: None for what JSON cannot say (an absent value, the infinities, NaN unless ``keep_nan``)"""
    if x is None or math.isinf(float(x)) or (math.isnan(float(x)) and not keep_nan):
        return None
    return float(x)


def write_report(path: Path, report: dict, say: bool = True) -> None:
    """the report as JSON, its directory made; ``say``: print where it went"""
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    if say:
        print(f"wrote {path}")


def region_rows(found, warmed: bool, length_scale: float = 1.0) -> list:
    """the rows of a ``ThermalRegions`` of a difference mesh: area, mean difference, centroid, the largest change of a face"""
    s = float(length_scale)
    return [{"region": int(r), "faces": int(row["faces"]), "area": float(row["area"]) * s * s, "mean_difference": float(row["mean_temperature"]),
             "largest_change": float(row["max_temperature"] if warmed else row["min_temperature"]),
             "centroid": [float(c) * s for c in row["centroid"]]} for r, row in zip(found.region_index.tolist(), found.regions)]


def add_difference_regions(report: dict, names, above, below, min_change: float, length_scale: float) -> None:
    """the --min-change part of a report: under ``names`` = (above, below) the ``ThermalRegions`` where the difference mesh is at
    least ``min_change`` above zero and at least that below, then the area they were taken from"""
    s = float(length_scale)
    report["min_change"] = float(min_change)
    for name, regions, sign in ((names[0], above, True), (names[1], below, False)):
        report[name] = {"regions": region_rows(regions, sign, s), "area": float(regions.selected_area) * s * s,
                        "share": float(regions.selected_area / regions.mesh_area) if regions.mesh_area > 0.0 else 0.0}
    report["compared_area"] = float(above.mesh_area) * s * s


def difference_region_lines(report: dict, names) -> list:
    lines = []
    for name in names:
        for k, row in enumerate(report.get(name, {}).get("regions", [])):
            c = row["centroid"]
            lines.append(f"{name} {k}: area {row['area']:.6g}, {row['faces']} faces, mean {row['mean_difference']:+.2f} C, largest "
                         f"{row['largest_change']:+.2f} C, centroid ({c[0]:.4g}, {c[1]:.4g}, {c[2]:.4g})")
    return lines


INTRINSICS = ("fl_x", "fl_y", "cx", "cy", "w", "h")


def frame_camera(meta: dict, index: int, scale: float = 1.0) -> dict:
    """{"c2w": 3 x 4 rows, "fx", "fy", "cx", "cy", "width", "height"} of frame ``index``: the intrinsics from the file's top level,
    else from the frame (the dataparser's rule); the pose as written with ``applied_transform`` and ``applied_scale`` undone; the
    image size and the intrinsics times ``scale`` (the size truncated, as ``Cameras.rescale_output_resolution`` does)"""
    if meta.get("camera_model", "OPENCV") not in ("OPENCV", "PINHOLE", "SIMPLE_PINHOLE"):
        raise ValueError(f"camera_model {meta['camera_model']}: only perspective cameras")
    frame = meta["frames"][index]
    values = {}
    for k in INTRINSICS:
        if k in meta:
            values[k] = float(meta[k])
        elif k in frame:
            values[k] = float(frame[k])
        else:
            raise ValueError(f"{k} is neither in the file nor in the frame")
    pose = np.asarray(frame["transform_matrix"], dtype=np.float64)
    if pose.shape == (3, 4):
        pose = np.concatenate([pose, [[0.0, 0.0, 0.0, 1.0]]])
    if pose.shape != (4, 4) or not np.isfinite(pose).all():
        raise ValueError("transform_matrix is a finite 4 x 4 (or 3 x 4) matrix")
    if "applied_transform" in meta:
        applied = np.concatenate([np.asarray(meta["applied_transform"], dtype=np.float64).reshape(3, 4), [[0.0, 0.0, 0.0, 1.0]]])
        pose = np.linalg.inv(applied) @ pose
    if "applied_scale" in meta:
        pose[:3, 3] /= float(meta["applied_scale"])
    width, height = int(values["w"] * scale), int(values["h"] * scale)
    if width < 1 or height < 1:
        raise ValueError(f"--scale {scale} leaves an image of {width} x {height} pixels")
    return {"c2w": pose[:3].tolist(), "fx": values["fl_x"] * scale, "fy": values["fl_y"] * scale, "cx": values["cx"] * scale,
            "cy": values["cy"] * scale, "width": width, "height": height}
