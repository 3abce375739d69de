"""What the export entry points share: the argument checks of the kernel wrappers (pointcloud.py, mesh.py, neighbors.py) and the
pose loop of the two exporters — render camera after camera through one cached ``RayRenderEngine``, nothing synchronising
between poses."""
from __future__ import annotations

import dataclasses
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

SCENE_BOX = "scene_box"
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def out_tensor(t: Optional[Tensor], name: str, dtype: torch.dtype, capacity: int, width: int) -> Optional[Tensor]:
    if t is None:
        return None
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < capacity * width:
        raise ValueError(f"{name} must be a contiguous {dtype} device tensor of at least {capacity * width} elements")
    return t


def check_color_table(t: Optional[Tensor]) -> None:
    """the table that ``thermal_colors`` needs"""
    if t is None or t.dtype != torch.uint8 or tuple(t.shape) != (256, 3) or not t.is_cuda or not t.is_contiguous():
        raise ValueError("thermal_colors needs a contiguous uint8 [256, 3] device table")


def workspace_of(workspace: Optional[Tensor], need: int, device) -> Tuple[Tensor, int]:
    """(the caller's workspace, checked, or a fresh one of ``need`` bytes; its size in bytes)"""
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=device)
    size = workspace.numel() * workspace.element_size()
    if not workspace.is_cuda or not workspace.is_contiguous() or size < need:
        raise ValueError(f"workspace must be a contiguous device tensor of at least {need} bytes")
    return workspace, size


def affine12(to_world) -> Tuple[float, ...]:
    """a row-major 3 x 4 ``to_world`` (None: identity) as twelve Python floats"""
    m = _IDENTITY if to_world is None else tuple(float(v) for v in np.asarray(to_world, dtype=np.float64).reshape(-1))
    if len(m) != 12:
        raise ValueError("to_world is a 3 x 4 matrix")
    return m


def resolve_box(model, bounding_box) -> Optional[List[List[float]]]:
    """[[min x3], [max x3]] in double: ``"scene_box"`` is the model's ``scene_box.aabb``; None stays None (no box)"""
    if isinstance(bounding_box, str) and bounding_box == SCENE_BOX:
        bounding_box = model.scene_box.aabb
    if bounding_box is None:
        return None
    return torch.as_tensor(bounding_box).detach().double().cpu().reshape(2, 3).tolist()


class PoseExporter:
    """The part of ``PointCloudExporter`` and ``MeshExporter`` that renders: the model checks, the engine, the loop over poses."""

    def __init__(self, model, depth_output_name: str, thermal_color_map: str, min_temperature: float, max_temperature: float) -> None:
        if depth_output_name not in ("depth", "expected_depth"):
            raise ValueError('depth_output_name must be "depth" or "expected_depth"')
        if not model._fusable():
            raise RuntimeError(f"{type(self).__name__} drives the fused kernels through RayRenderEngine; this model is not fusable "
                               "(staged field or non-default proposal structure)")
        self.model = model
        self.depth_output_name = depth_output_name
        self.thermal_color_map = thermal_color_map
        self.temperature_bounds = (float(min_temperature), float(max_temperature))
        self._engine = None

    def _render(self, origins: Tensor, directions: Tensor, out):
        from ..engine import engine_for

        self._engine = engine_for(self.model, self._engine)
        return self._engine.render(origins, directions, out=out)

    def _poses(self, cameras, camera_indices: Optional[Sequence[int]], apply_camera_optimizer: bool, pinhole: bool = False
               ) -> Tuple[torch.device, bool, List[int], Iterator]:
        """(device, adjust, the camera indices, a generator of (k, flat ray bundle of camera k)) after the checks every export
        starts with.  ``adjust``: the rays carry row k of the model's pose table; ``pinhole``: they ignore ``distortion_params``."""
        model = self.model
        if model.training:
            raise RuntimeError(f"{type(self).__name__} renders in eval mode; call model.eval() first")
        dev = torch.device(model.device)
        if dev.type != "cuda":
            raise RuntimeError(f"the model is on {dev}; thermo_nerf_amd exports only on a ROCm device (no CPU fallback exists)")
        index = list(range(cameras.size)) if camera_indices is None else [int(k) for k in camera_indices]
        if any(k < 0 or k >= cameras.size for k in index):
            raise IndexError("camera index outside the camera set")
        opt = model.camera_optimizer
        adjust = bool(apply_camera_optimizer) and opt.config.mode != "off"
        if adjust and any(k >= opt.num_cameras for k in index):
            raise IndexError(f"the camera optimizer holds {opt.num_cameras} poses; pass apply_camera_optimizer=False for other views")
        source = dataclasses.replace(cameras, distortion_params=None) if pinhole else cameras

        def bundles():
            for k in index:
                rb = source.generate_rays(k, device=dev, flat=True)
                if adjust:
                    opt.apply_to_raybundle(rb)  # camera_indices = k for every ray of the pose
                yield k, rb

        return dev, adjust, index, bundles()
