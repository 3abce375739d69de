"""Colour tables for frame finishing: matplotlib's 256-entry ``magma``, ``turbo`` and ``gray`` without matplotlib.

The reference colours a thermal frame with ``plt.colormaps["magma"]`` [REF thermo_nerf/render/renderer.py:164,193-196] and
nerfstudio colours depth with ``turbo``; the machines this package runs on need not have matplotlib, so the tables are data:
``colormap_tables.txt`` next to this module, written once by ``tools/make_colormap_tables.py`` (float64, exact).

    table_f64(name)   [256, 3] float64 numpy — matplotlib's values
    table_f32(name)   the same rounded to float32 (what nerfstudio's ``colormap[index]`` reads; TN_FRAME_DEPTH)
    table_u8(name)    trunc(float64 * 255) as uint8 — ``(cmap(x)[..., :3] * 255).astype(np.uint8)`` per entry (TN_FRAME_LUT)
    get_table(name, device)   (float32 [256,3], uint8 [256,3]) tensors on ``device``, cached per (name, device)
"""
from __future__ import annotations

import os
from typing import Dict, Tuple

import numpy as np
import torch

NAMES = ("magma", "turbo", "gray")
_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormap_tables.txt")
_F64: Dict[str, np.ndarray] = {}
_DEVICE: Dict[Tuple[str, str], Tuple[torch.Tensor, torch.Tensor]] = {}


def _load() -> None:
    name, rows = None, []
    tables: Dict[str, list] = {}
    with open(_PATH, "r", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            if line.startswith("["):
                name = line.strip("[]")
                rows = tables.setdefault(name, [])
                continue
            rows.append([float(v) for v in line.split()])
    for k, v in tables.items():
        t = np.asarray(v, dtype=np.float64)
        if t.shape != (256, 3):
            raise RuntimeError(f"{_PATH}: table '{k}' has shape {t.shape}, expected (256, 3)")
        t.setflags(write=False)
        _F64[k] = t


def table_f64(name: str) -> np.ndarray:
    if not _F64:
        _load()
    if name not in _F64:
        raise KeyError(f"unknown colour map '{name}' (available: {', '.join(sorted(_F64))})")
    return _F64[name]


def table_f32(name: str) -> np.ndarray:
    return table_f64(name).astype(np.float32)


def table_u8(name: str) -> np.ndarray:
    return (table_f64(name) * 255).astype(np.uint8)


def get_table(name: str, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """(float32 [256,3], uint8 [256,3]) on ``device``; uploaded once per (name, device)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (name, str(dev))
    hit = _DEVICE.get(key)
    if hit is None:
        hit = _DEVICE[key] = (torch.from_numpy(table_f32(name)).to(dev), torch.from_numpy(table_u8(name)).to(dev))
    return hit
