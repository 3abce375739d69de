"""Inference harness: camera path -> 8-bit frames on disk [REF thermo_nerf/render/]."""
from .renderer import Renderer, frame_to_rgb8  # noqa: F401
