"""tn_render_config / tn_render_inputs of a library call, built in one place for everything that makes one: the model's fused
forward, the render engine and the two training forwards."""
from __future__ import annotations

from typing import Optional

from torch import Tensor

from . import _hip
from .samplers import linspace_bins, pdf_positions


def render_config(model, training: bool, **overrides) -> _hip.tn_render_config:
    """What every call takes from the model: sample counts, training flag, the sampler's annealing exponent and initial spacing,
    and in eval the config's early-termination threshold.  Every other field stays 0 — the library's own choice — unless
    ``overrides`` names it (kernel_family, sample_split, per_sample_jitter, tail_balance, tail_slots)."""
    cfg = model.config
    rc = _hip.tn_render_config()
    rc.num_proposal_samples[0], rc.num_proposal_samples[1] = cfg.num_proposal_samples_per_ray
    rc.num_nerf_samples = cfg.num_nerf_samples_per_ray
    rc.training = 1 if training else 0
    rc.pdf_anneal = float(model.proposal_sampler._anneal)
    rc.early_stop_transmittance = 0.0 if training else float(cfg.early_termination_eps)
    rc.initial_sampler = int(model.proposal_sampler.initial_sampler.uniform_spacing)
    for name, value in overrides.items():
        setattr(rc, name, value)
    return rc


def render_inputs(rc: _hip.tn_render_config, dev, rays=None, cam: Optional[Tensor] = None,
                  jitter: Optional[Tensor] = None) -> _hip.tn_render_inputs:
    """The samplers' constant tables for ``rc``'s sample counts on ``dev``, the camera indices and stratified draws of a training
    call, and ``rays`` = (origins, directions, nears, fars) where the caller does not set them launch by launch."""
    ins = _hip.tn_render_inputs()
    if rays is not None:
        ins.origins, ins.directions, ins.nears, ins.fars = (t.data_ptr() for t in rays)
    ins.camera_indices, ins.jitter = _hip.ptr(cam), _hip.ptr(jitter)
    ins.lin_bins0 = linspace_bins(rc.num_proposal_samples[0], dev).data_ptr()
    ins.u1 = pdf_positions(rc.num_proposal_samples[1] + 1, dev, bool(rc.training)).data_ptr()
    ins.u2 = pdf_positions(rc.num_nerf_samples + 1, dev, bool(rc.training)).data_ptr()
    return ins
