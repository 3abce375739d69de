#!/usr/bin/env python
"""Export a finished run as a thermal point cloud: a binary PLY with a position, a colour and a temperature in degrees Celsius per point.

    python tools/export_pointcloud.py RUN_DIR DATASET --output cloud.ply --num-points 1000000 --threshold auto --colors thermal

RUN_DIR is a run directory of tools/train_eval.py: its ``config.json`` supplies the model settings, the number of training
cameras, the temperature bounds and ``cold`` (``--config-json`` overrides model fields), its newest ``step-*.ckpt`` the weights.
Every camera of the chosen split of DATASET is rendered; a ray becomes a point when its accumulation exceeds
``--min-accumulation``, its back-projected depth lies strictly inside the bounding box (the dataset's scene box unless
``--bounding-box-min/-max`` or ``--no-bounding-box``) and, with ``--threshold``, its predicted normalised temperature lies beyond it
(above; below for a ``cold`` run).  Training cameras are rendered with their optimised poses.

Positions are written in the dataset's original world frame (the inverse of the dataparser's orientation, centring and
scaling); ``--scene-frame`` keeps the normalised frame the model was trained in.  ``--num-points`` thins a larger cloud evenly
and deterministically (point floor(j M / N) for j < N).

``--remove-outliers`` drops the floaters first (statistical outlier removal over ``--outlier-neighbors`` neighbours: a point goes
when its mean neighbour distance is ``--outlier-std-ratio`` standard deviations above the cloud's mean); ``--normals`` gives every
written point a normal (nx ny nz in the file) from its ``--normal-neighbors`` nearest neighbours, turned towards the camera the
point was seen from.  ``--voxel-size S`` replaces the points of every occupied voxel of edge S — in the units of the frame that is
written: the world frame, or the scene frame with ``--scene-frame`` — by ONE point with their mean position, colours and
temperature: a wall seen by forty cameras is in the cloud once, at the mean of the forty measurements.  Order: export, outlier
removal, voxel down-sampling, thinning, normals — the normals are those of the cloud that is written.
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


def threshold_argument(text: str):
    """none | auto | FLOAT"""
    low = text.lower()
    if low == "none":
        return None
    if low == "auto":
        return "auto"
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not none, auto or a number")


def parse(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model_uri", type=Path, help="run directory of the model")
    ap.add_argument("dataset_path", type=Path, help="dataset directory or its transforms.json")
    ap.add_argument("--output", type=Path, required=True, help="the PLY file to write")
    ap.add_argument("--split", choices=("train", "val"), default="train", help="which cameras of the dataset to render")
    ap.add_argument("--num-points", type=int, default=1000000, help="thin the cloud to at most this many points")
    ap.add_argument("--resolution-scale", type=float, default=1.0, help="scale of the rendered resolution")
    ap.add_argument("--depth", choices=("depth", "expected_depth"), default="depth",
                    help="the depth output to back-project (expected_depth depends on the eval chunk size)")
    ap.add_argument("--min-accumulation", type=float, default=0.5, help="drop rays at or below this opacity")
    ap.add_argument("--no-bounding-box", action="store_true", help="keep points outside the scene box")
    ap.add_argument("--bounding-box-min", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--bounding-box-max", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--threshold", type=threshold_argument, default=None, metavar="none|auto|FLOAT",
                    help="keep points whose predicted normalised temperature lies beyond it")
    ap.add_argument("--colors", choices=("rgb", "thermal"), default="rgb", help="what fills red / green / blue")
    ap.add_argument("--scene-frame", action="store_true", help="write the normalised scene frame, not the dataset's world frame")
    ap.add_argument("--config-json", type=Path, default=None, help="model fields that override the run's config.json")
    ap.add_argument("--remove-outliers", action="store_true", help="drop statistical outliers before thinning")
    ap.add_argument("--outlier-neighbors", type=int, default=20, help="neighbours of the outlier statistic, the point included")
    ap.add_argument("--outlier-std-ratio", type=float, default=10.0, help="standard deviations above the mean that make an outlier")
    ap.add_argument("--voxel-size", type=float, default=None, metavar="S",
                    help="one averaged point per occupied voxel of edge S, in the units of the frame that is written")
    ap.add_argument("--normals", action="store_true", help="estimate a normal per written point (nx ny nz in the file)")
    ap.add_argument("--normal-neighbors", type=int, default=30, help="nearest neighbours a normal is fitted to")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if not 2 <= args.outlier_neighbors <= 33:
        ap.error("--outlier-neighbors must be 2 .. 33 (the point and up to 32 others)")
    if not args.outlier_std_ratio > 0.0:
        ap.error("--outlier-std-ratio must be positive")
    if not 2 <= args.normal_neighbors <= 32:
        ap.error("--normal-neighbors must be 2 .. 32")
    if (args.bounding_box_min is None) != (args.bounding_box_max is None):
        ap.error("--bounding-box-min and --bounding-box-max go together")
    if args.no_bounding_box and args.bounding_box_min is not None:
        ap.error("--no-bounding-box contradicts --bounding-box-min/-max")
    if args.voxel_size is not None and not (args.voxel_size > 0.0 and math.isfinite(args.voxel_size)):
        ap.error("--voxel-size must be positive and finite")
    if args.num_points < 0:
        ap.error("--num-points must not be negative")
    return args


def build_exporter(args):
    """(exporter, cameras of the split, apply_camera_optimizer) as ``main`` sets them up — also what a caller that wants the cloud
    in-process uses"""
    from thermo_nerf_amd.export import PointCloudExporter, world_transform
    from thermo_nerf_amd.model_type import ModelType
    from thermo_nerf_amd.run_config import load_run_for_export
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import calculate_threshold

    r = load_run_for_export(args)
    threshold = args.threshold
    if threshold == "auto":
        threshold = calculate_threshold(args.dataset_path, ModelType.THERMONERF, device=args.device)
    exporter = PointCloudExporter(r["model"], max_temperature=r["max_temperature"], min_temperature=r["min_temperature"],
                                  depth_output_name=args.depth, min_accumulation=args.min_accumulation,
                                  bounding_box=r["bounding_box"], threshold=threshold, cold=bool(r["run"].get("cold", False)),
                                  to_world=None if args.scene_frame else world_transform(r["parsed"]))
    return exporter, r["cameras"], args.split == "train"


def main(argv=None) -> int:
    args = parse(argv)
    from thermo_nerf_amd.export import subsample, write_ply

    exporter, cameras, adjust = build_exporter(args)
    cloud = exporter.export(cameras, apply_camera_optimizer=adjust)
    kept = len(cloud)
    removed = ""
    if args.remove_outliers:
        from thermo_nerf_amd.export import remove_statistical_outliers

        cloud, _ = remove_statistical_outliers(cloud, args.outlier_neighbors, args.outlier_std_ratio)
        removed = f", outliers removed {kept - len(cloud)}"
    if args.voxel_size is not None:
        from thermo_nerf_amd.export import voxel_downsample

        before = len(cloud)
        cloud, _ = voxel_downsample(cloud, args.voxel_size)
        removed += f", voxels {len(cloud)} of {before}"
    cloud = subsample(cloud, args.num_points)
    if args.normals:
        from thermo_nerf_amd.export import estimate_normals

        cloud = estimate_normals(cloud, args.normal_neighbors, exporter.viewpoints(cloud))
    write_ply(args.output, cloud, colors=args.colors)
    print(f"rays cast {exporter.last_rays}, kept {kept}{removed}, written {len(cloud)} -> {args.output}")
    if len(cloud):
        print(f"temperature min {float(cloud.temperature.min()):.3f} C, max {float(cloud.temperature.max()):.3f} C")
    else:
        print("temperature min -, max - (no point passed the filter)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
