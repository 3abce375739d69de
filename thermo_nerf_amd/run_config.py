"""What a training run leaves beside its checkpoints so that it can be reloaded without remembering its flags, and the
evaluation both command lines end in (tools/train_eval.py, tools/evaluate.py).

The reference pickles nerfstudio objects into ``config.yml`` and rebuilds the pipeline from it
[REF thermo_nerf/render/renderer.py:34-116]; ``checkpoint.py`` never touches that file by design.  A run directory here is

    <model_output_folder>/<experiment_name>/thermal-nerf/<timestamp>/
        config.json                     see ``write_run_config``
        nerfstudio_models/step-*.ckpt   nerfstudio's checkpoint layout (trainer.Trainer.save_checkpoint)

``config.json["model"]`` holds the ThermalNerfModelConfig fields that differ from the defaults — the object the tools'
``--config-json`` accepts.
"""
from __future__ import annotations

import dataclasses
import json
from pathlib import Path
from typing import Dict, Optional, Sequence

from .rendered_image_modalities import RenderedImageModality

RUN_CONFIG = "config.json"
CHECKPOINT_DIR = "nerfstudio_models"
# derived in the model's constructor (camera_optimizer <- camera_optimizer_mode) / not data
_NOT_SAVED = ("_target", "camera_optimizer")


def model_config(overrides: Optional[Dict] = None):
    """ThermalNerfModelConfig with ``overrides`` (a JSON object of field names and values) applied"""
    from .thermal_nerf.thermal_nerf_model import ThermalNerfModelConfig

    over = dict(overrides or {})
    if "num_proposal_samples_per_ray" in over:
        over["num_proposal_samples_per_ray"] = tuple(over["num_proposal_samples_per_ray"])
    return ThermalNerfModelConfig(**over)


def model_config_overrides(config) -> Dict:
    """the fields of ``config`` that differ from ThermalNerfModelConfig's defaults, as JSON values"""
    default = model_config()
    out = {}
    for f in dataclasses.fields(config):
        if f.name in _NOT_SAVED:
            continue
        value = getattr(config, f.name)
        if value != getattr(default, f.name):
            out[f.name] = list(value) if isinstance(value, tuple) else value
    return out


def load_overrides(path) -> Dict:
    """a ``--config-json`` file: the model object itself, or a run's config.json (its "model" entry)"""
    over = json.loads(Path(path).read_text()) if path else {}
    return over["model"] if isinstance(over.get("model"), dict) else over


def write_run_config(run_dir, config, num_train_data: int, temperature_bounds: Sequence[float], cold: bool, eval_mode: str,
                     data, threshold: Optional[float], **extra) -> Path:
    path = Path(run_dir) / RUN_CONFIG
    path.parent.mkdir(parents=True, exist_ok=True)
    body = {"method_name": "thermal-nerf", "model": model_config_overrides(config), "num_train_data": int(num_train_data),
            "temperature_bounds": [float(t) for t in temperature_bounds], "cold": bool(cold), "eval_mode": eval_mode,
            "data": str(data), "threshold": threshold}
    body.update(extra)
    path.write_text(json.dumps(body, indent=2), "utf8")
    return path


def read_run_config(run_dir) -> Dict:
    path = Path(run_dir) / RUN_CONFIG
    if not path.is_file():
        raise FileNotFoundError(f"{path} not found: {run_dir} is not a run directory of tools/train_eval.py "
                                "(pass the model settings with --config-json)")
    return json.loads(path.read_text())


def evaluate_run(run_dir, data, config, num_train_data: int, eval_mode: str = "filename",
                 modalities: Sequence[RenderedImageModality] = (RenderedImageModality.RGB,), threshold: Optional[float] = None,
                 experiment_name: str = "", device="cuda"):
    """Load the newest checkpoint under ``run_dir`` into a fresh model with the dataset's scene box and evaluate the eval split
    of ``data`` [REF thermo_nerf/scripts/eval_script.py:37-47]: the training command evaluates through the same reload, as the
    reference's does [REF thermo_nerf/scripts/train_eval_script.py:111-119]."""
    from .data import ThermalDataParserConfig, ThermalDataset
    from .evaluator import Evaluator
    from .render import Renderer

    eval_out = ThermalDataParserConfig(data=Path(data), eval_mode=eval_mode).setup().get_dataparser_outputs("val")
    renderer = Renderer.from_checkpoint(run_dir, config, num_train_data, device=device, scene_box=eval_out.scene_box)
    return Evaluator(renderer.model, ThermalDataset(eval_out), experiment_name=experiment_name, modalities_to_save=list(modalities),
                     threshold=threshold, device=device)


def load_run_for_export(args) -> Dict:
    """What an export command line starts from.  ``args``: ``model_uri``, ``dataset_path``, ``split``, ``config_json``,
    ``resolution_scale``, ``device``, ``bounding_box_min`` / ``bounding_box_max`` and, optionally, ``no_bounding_box``.  Returns
    ``run`` (the run's config.json), ``parsed`` (the split's dataparser outputs), ``model`` (the newest checkpoint, eval mode, on
    the device), ``cameras`` (the split's, rescaled), ``max_temperature`` / ``min_temperature`` and ``bounding_box`` (the explicit
    one, None with ``no_bounding_box``, else the dataset's scene box)."""
    from .data import ThermalDataParserConfig
    from .render import Renderer

    run = read_run_config(args.model_uri)
    over = dict(run.get("model", {}))
    over.update(load_overrides(args.config_json))
    parsed = ThermalDataParserConfig(data=Path(args.dataset_path), eval_mode=run.get("eval_mode", "filename")).setup() \
        .get_dataparser_outputs(args.split)
    renderer = Renderer.from_checkpoint(args.model_uri, model_config(over), int(run["num_train_data"]), device=args.device,
                                        scene_box=parsed.scene_box)
    cameras = parsed.cameras
    if args.resolution_scale != 1.0:
        cameras.rescale_output_resolution(args.resolution_scale)
    max_t, min_t = (float(v) for v in run["temperature_bounds"])
    if getattr(args, "no_bounding_box", False):
        box = None
    elif args.bounding_box_min is not None:
        box = [args.bounding_box_min, args.bounding_box_max]
    else:
        box = parsed.scene_box.aabb
    return dict(run=run, parsed=parsed, model=renderer.model, cameras=cameras, max_temperature=max_t, min_temperature=min_t,
                bounding_box=box)
