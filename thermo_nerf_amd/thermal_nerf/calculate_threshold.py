"""Foreground threshold of a thermal dataset [REF thermo_nerf/thermal_nerf/calculate_threshold.py:10-38]: the mean over ALL
frames of a ``transforms.json`` (train and eval alike, at full resolution) of the image's Otsu threshold, divided by 255 — the
number ``mae_thermal_foreground`` cuts the region of interest with.

The reference calls OpenCV per image on the host.  Here the images are packed into one device buffer and ``tn_otsu_thresholds``
(csrc/tn_threshold.hip) leaves one exact integer per image: histograms by integer atomics, the threshold by OpenCV's recurrence
in fp64 with one rounding per step (include/thermonerf_hip.h has the definition).  The mean and the division by 255 are Python
doubles on the host, as in the reference.

Grey values are read as ``ThermalDataset.get_thermal_tensors_from_path`` reads them: single-channel files as their bytes, any
other mode through PIL's ``convert("L")``.  OpenCV's own colour-to-grey conversion (``IMREAD_GRAYSCALE`` of a colour file: other
weights and rounding than PIL's) is NOT reproduced; ThermoScenes thermal images are single-channel.
"""
from __future__ import annotations

import ctypes
import json
from pathlib import Path
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image
from torch import Tensor

from .. import _hip
from ..model_type import ModelType


def otsu_thresholds(images: Sequence[Tensor], return_histograms: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """``images``: uint8 device tensors of any shapes -> int32 [N] on the device, one ``tn_otsu_thresholds`` call on the current
    stream (no host synchronisation).  ``return_histograms``: also the exact int32 [N, 256] grey-level counts (the bit pattern
    of the call's uint32 bins: an image of 2^31 pixels or more may show a negative entry)."""
    images = list(images)
    if not images:
        raise ValueError("otsu_thresholds needs at least one image")
    flat = [_hip.require_device_tensor(im, f"images[{i}]", torch.uint8).reshape(-1) for i, im in enumerate(images)]
    device = flat[0].device
    if any(f.device != device for f in flat):
        raise ValueError("all images must live on one device")
    if any(f.numel() == 0 for f in flat):
        raise ValueError("an image without pixels has no threshold")
    packed = flat[0] if len(flat) == 1 else torch.cat(flat)
    n = len(flat)
    offsets = (ctypes.c_int64 * (n + 1))()
    for i, f in enumerate(flat):
        offsets[i + 1] = offsets[i] + f.numel()
    histograms = torch.empty((n, 256), dtype=torch.int32, device=device)
    thresholds = torch.empty((n,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _hip.check(_hip.load().tn_otsu_thresholds(packed.data_ptr(), offsets, n, histograms.data_ptr(), thresholds.data_ptr(),
                                                  _hip.current_stream()), "tn_otsu_thresholds")
    return (thresholds, histograms) if return_histograms else thresholds


def thermal_image_paths(data: Path, model_type: ModelType = ModelType.THERMONERF) -> List[Path]:
    """The files the threshold is computed from: every frame of the json, in its order — ``data`` is a dataset directory or the
    path of its ``transforms.json``; the frame key is ``thermal_file_path`` (``file_path`` for ModelType.NERFACTO, whose "RGB"
    images are the thermal ones) [REF :17-31]."""
    data = Path(data)
    json_path, data_dir = (data, data.parent) if data.suffix == ".json" else (data / "transforms.json", data)
    meta = json.loads(json_path.read_text())
    key = "file_path" if model_type == ModelType.NERFACTO else "thermal_file_path"
    return [data_dir / Path(frame[key]) for frame in meta["frames"]]


def load_grey_image(path: Path) -> np.ndarray:
    """uint8 [H, W]: the grey values ThermalDataset.get_thermal_tensors_from_path divides by 255 (full resolution)"""
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"No file found at {path}")
    pil = Image.open(path)
    if pil.mode != "L":
        pil = pil.convert("L")
    return np.array(pil, dtype=np.uint8)  # (a copy: PIL's buffer is read-only)


def calculate_threshold(data: Path, model_type: ModelType = ModelType.THERMONERF, device="cuda") -> float:
    """Mean Otsu threshold of the dataset's thermal images / 255 [REF :10-38]."""
    device = torch.device(device)
    if device.type != "cuda":  # the same refusal as every other entry, before any file is read
        _hip.require_device_tensor(torch.empty(0, dtype=torch.uint8, device=device), "calculate_threshold's images", torch.uint8)
    paths = thermal_image_paths(data, model_type)
    if not paths:
        raise ValueError(f"{data} lists no frames")
    images = [torch.from_numpy(load_grey_image(p)).to(device) for p in paths]
    thresholds = otsu_thresholds(images).cpu().tolist()  # exact integers
    return sum(thresholds) / len(thresholds) / 255.0
