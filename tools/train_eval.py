#!/usr/bin/env python
"""Train ThermoNeRF on a ThermoScenes folder, compute the foreground threshold, evaluate the eval split — the reference's main
workflow in one command, an argparse mirror of its TrainingParameters [REF thermo_nerf/scripts/train_eval_script.py:22-123].

    python tools/train_eval.py --data DATASET --experiment-name kettle --model-output-folder outputs \\
        --metrics-output-folder outputs/kettle_metrics --temperature-bounds 33 14

writes ``<model-output-folder>/<experiment-name>/thermal-nerf/<timestamp>/`` (``nerfstudio_models/step-*.ckpt`` and a
``config.json`` that tools/evaluate.py and tools/render_video.py --config-json read back) and, into the metrics folder,
``metrics.json`` plus the eval images ``img_*.jpg``, ``thermal_*.jpg``, ``thermal_combined_*.jpg``.

The method configuration is ``thermal_nerf_config`` (thermo_nerf_amd/thermal_nerf/config_thermal_nerf.py); ``--config-json``
overrides model fields.  Not mirrored: mlflow tracking, the viewer, and the three baseline methods, which are not built here.
"""
from __future__ import annotations

import argparse
import copy
import dataclasses
import json
import os
import sys
from datetime import datetime
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None) -> argparse.Namespace:
    from thermo_nerf_amd.model_type import ModelType

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model-type", default="thermonerf", choices=[m.name.lower() for m in ModelType],
                    help="what NeRF model to train (only thermonerf is built here)")
    ap.add_argument("--experiment-name", default="nerfacto training", help="name of the model to train")
    ap.add_argument("--model-output-folder", type=Path, default=Path("./outputs"), help="where to save the model")
    ap.add_argument("--max-num-iterations", type=int, default=30000)
    ap.add_argument("--data", type=Path, default=Path("./inputs"), help="dataset directory or its transforms.json")
    ap.add_argument("--metrics-output-folder", type=Path, default=Path("./outputs/"))
    ap.add_argument("--seed", type=int, default=0, help="seed of the random number generators")
    ap.add_argument("--temperature-bounds", type=float, nargs=2, default=[1.0, 0.0], metavar=("MAX", "MIN"),
                    help="temperature bounds of the dataset, in degrees")
    ap.add_argument("--cold", action=argparse.BooleanOptionalAction, default=False, help="settings for cold temperatures")
    ap.add_argument("--camera-optimizer-mode", default="SO3xR3", choices=["off", "SO3xR3", "SE3"], help="pose optimisation")
    ap.add_argument("--eval-mode", default="filename", choices=["fraction", "filename", "interval", "all"],
                    help="how the dataset is split into train and eval")
    ap.add_argument("--config-json", type=Path, default=None, help="ThermalNerfModelConfig fields that differ from the method's")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    args.model_type = ModelType[args.model_type.upper()]
    if args.model_type != ModelType.THERMONERF:
        ap.error(f"--model-type {args.model_type.name.lower()}: the baseline models (thermalnerfacto, concatnerf, nerfacto) are not "
                 "built here; only thermonerf is")
    if args.max_num_iterations < 1:
        ap.error("--max-num-iterations must be at least 1")
    return args


def main(argv=None) -> int:
    args = parse(argv)
    import torch

    from thermo_nerf_amd import ThermalNerfModel, run_config
    from thermo_nerf_amd.data import ThermalDataParserConfig, ThermalDataset
    from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import calculate_threshold
    from thermo_nerf_amd.thermal_nerf.config_thermal_nerf import thermal_nerf_config
    from thermo_nerf_amd.trainer import Trainer

    modalities = [RM.RGB, RM.THERMAL, RM.THERMAL_COMBINED]  # REF :60-64
    train_out = ThermalDataParserConfig(data=args.data, eval_mode=args.eval_mode).setup().get_dataparser_outputs("train")
    train_set = ThermalDataset(train_out)
    rays = train_set.to_ray_table(args.device)

    method = copy.deepcopy(thermal_nerf_config)
    over = run_config.load_overrides(args.config_json)
    if "num_proposal_samples_per_ray" in over:
        over["num_proposal_samples_per_ray"] = tuple(over["num_proposal_samples_per_ray"])
    model_cfg = dataclasses.replace(method.model, **over)
    model_cfg.max_temperature, model_cfg.min_temperature = args.temperature_bounds  # REF :93-94
    model_cfg.cold = args.cold
    model_cfg.camera_optimizer_mode = args.camera_optimizer_mode
    method.trainer.max_num_iterations = args.max_num_iterations
    method.trainer.seed = args.seed
    saved_cfg = copy.deepcopy(model_cfg)  # (the trainer switches run-time fields of the live config on)

    torch.manual_seed(args.seed)  # before the model draws its initial weights
    model = ThermalNerfModel(model_cfg, metadata=train_out.metadata, scene_box=train_out.scene_box,
                             num_train_data=len(train_set)).to(args.device)
    run_dir = args.model_output_folder / args.experiment_name / method.method_name / datetime.now().strftime("%Y-%m-%d_%H%M%S")
    ckpt_dir = run_dir / run_config.CHECKPOINT_DIR

    def write_config(threshold):
        run_config.write_run_config(run_dir, saved_cfg, len(train_set), args.temperature_bounds, args.cold, args.eval_mode,
                                    args.data, threshold, experiment_name=args.experiment_name, seed=args.seed,
                                    max_num_iterations=args.max_num_iterations)

    write_config(None)  # a run that is interrupted can still be reloaded
    trainer = Trainer(model, rays, method.trainer)
    trainer.train(checkpoint_dir=ckpt_dir)
    if trainer.step % method.trainer.steps_per_save != 0:  # always one at the last step
        trainer.save_checkpoint(ckpt_dir)
    del trainer, rays

    threshold = calculate_threshold(args.data, args.model_type, device=args.device)
    write_config(threshold)
    evaluator = run_config.evaluate_run(run_dir, args.data, saved_cfg, len(train_set), eval_mode=args.eval_mode,
                                        modalities=modalities, threshold=threshold, experiment_name=args.experiment_name,
                                        device=args.device)
    evaluator.save_metrics(args.metrics_output_folder)
    evaluator.save_images(modalities, args.metrics_output_folder)

    print(f"threshold {threshold:.6f}")
    print(f"run directory {run_dir}")
    print(json.dumps({k: v for k, v in evaluator.metrics.items() if k.endswith(("_mean", "_std"))}, indent=2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
