#!/usr/bin/env python
"""Render a camera path of a trained model to JPEG frames and GIFs — the command line around thermo_nerf_amd.render.Renderer, an
argparse mirror of the reference's scripts/render_video_script.py [REF thermo_nerf/scripts/render_video_script.py:15-91].

    python tools/render_video.py RUN_DIR CAMERA_PATH.json --output-dir outputs --save-images \\
        --rendered-image-modalities rgb thermal --downscale-factor 2

RUN_DIR holds nerfstudio ``step-*.ckpt`` files (the newest is loaded).  The reference rebuilds the model from a pickled
``config.yml``; here the model settings that differ from ThermalNerfModelConfig's defaults come from ``--config-json`` (a JSON
object of field names and values), and the number of training cameras from ``--num-train-data`` or, absent, from the
checkpoint's appearance-embedding table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None) -> argparse.Namespace:
    from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM

    names = {m.name.lower(): m for m in RM}
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model_uri", type=Path, help="run directory with the model's *.ckpt files")
    ap.add_argument("camera_path_filename", type=Path, help="camera path JSON to render")
    ap.add_argument("--config-json", type=Path, default=None, help="ThermalNerfModelConfig fields that differ from the defaults")
    ap.add_argument("--num-train-data", type=int, default=None, help="training cameras of the run (default: from the checkpoint)")
    ap.add_argument("--save-video", action=argparse.BooleanOptionalAction, default=True, help="write a GIF per modality")
    ap.add_argument("--save-images", action=argparse.BooleanOptionalAction, default=False, help="write a JPEG per frame")
    ap.add_argument("--rendered-image-modalities", nargs="+", default=["rgb", "thermal"], choices=sorted(names),
                    help="outputs to render")
    ap.add_argument("--downscale-factor", type=int, default=1, help="divide the path's resolution by this")
    ap.add_argument("--output-dir", type=Path, default=Path("./outputs"))
    ap.add_argument("--seconds", type=float, default=5.0, help="duration handed to the GIF writer (per frame, as the reference does)")
    ap.add_argument("--eval-num-rays-per-chunk", type=int, default=None)
    ap.add_argument("--thermal-color-map", default="magma")
    ap.add_argument("--depth-color-map", default=None, help="colour depth like nerfstudio's viewer (e.g. turbo); default: depth x 255")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    args.modalities = [names[n] for n in args.rendered_image_modalities]
    if not args.camera_path_filename.is_file():
        ap.error(f"the camera path {args.camera_path_filename} could not be resolved")
    return args


def model_config(path):
    from thermo_nerf_amd import ThermalNerfModelConfig

    over = json.loads(Path(path).read_text()) if path else {}
    if "num_proposal_samples_per_ray" in over:
        over["num_proposal_samples_per_ray"] = tuple(over["num_proposal_samples_per_ray"])
    return ThermalNerfModelConfig(**over)


def train_cameras_of(run_dir) -> int:
    """rows of the appearance embedding = the num_train_data the run was built with"""
    import torch

    from thermo_nerf_amd.checkpoint import latest_checkpoint, model_state_from_pipeline

    state = torch.load(latest_checkpoint(run_dir), map_location="cpu", weights_only=True)
    sd, _ = model_state_from_pipeline(state.get("pipeline", state))
    return int(sd["field.embedding_appearance.embedding.weight"].shape[0])


def main(argv=None) -> int:
    args = parse(argv)
    from thermo_nerf_amd.render import Renderer

    cameras = Renderer.load_cameras(args.camera_path_filename, rendered_resolution_scaling_factor=1.0 / args.downscale_factor)
    num_train_data = args.num_train_data if args.num_train_data is not None else train_cameras_of(args.model_uri)
    renderer = Renderer.from_checkpoint(args.model_uri, model_config(args.config_json), num_train_data,
                                        eval_num_rays_per_chunk=args.eval_num_rays_per_chunk, device=args.device)
    renderer.render(args.modalities, cameras, thermal_color_map=args.thermal_color_map, depth_color_map=args.depth_color_map)
    if args.save_images:
        renderer.save_images(args.modalities, args.output_dir)
    if args.save_video:
        renderer.save_gif(args.modalities, args.seconds, args.output_dir)
    print(f"rendered {cameras.size} poses at {cameras.width}x{cameras.height}: {', '.join(m.value for m in args.modalities)} -> {args.output_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
