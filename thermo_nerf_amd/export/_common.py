"""What the export entry points share: the argument checks of the kernel wrappers (pointcloud.py, mesh.py, neighbors.py), the checks
of a ``ThermalMesh``, of a tree and of query points that every mesh analysis entry starts with, and the pose loop of the two
exporters — render camera after camera through one cached ``RayRenderEngine``, nothing synchronising between poses."""
from __future__ import annotations

import dataclasses
import math
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip

SCENE_BOX = "scene_box"
MAX_COUNT = 2 ** 31 - 1  # vertices, triangles, points or the pairs of a sort: indices are int32
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


def triangle_array(triangles) -> Tensor:
    """``triangles`` as every mesh kernel reads them: int32 [T, 3] on the device, 3 T within an int32"""
    tri = _hip.require_device_tensor(triangles, "triangles", torch.int32)
    if tri.dim() != 2 or tri.shape[1] != 3 or 3 * tri.shape[0] > MAX_COUNT:
        raise ValueError("triangles must be [T, 3] with 3 T <= 2^31 - 1")
    return tri


def require_triangles(mesh) -> None:
    """the first refusal of every mesh entry, for those that check their own parameters before the rest of ``mesh_arrays``"""
    if mesh.triangles is None:
        raise ValueError("the mesh has no triangles")


def mesh_arrays(mesh, temperature: bool = True) -> Tuple[Tensor, Optional[Tensor], Tensor, int, int]:
    """(positions, temperature, triangles, V, T) of a ``ThermalMesh`` after the checks every mesh entry starts with; without
    ``temperature`` (an entry that reads the geometry alone) it is not looked at and comes back as None"""
    require_triangles(mesh)
    p =_hip.require_device_tensor(mesh.positions, "positions")
    v = p.shape[0] if p.dim() == 2 and p.shape[1] == 3 else -1
    if v < 0 or v > MAX_COUNT:
        raise ValueError("positions must be [V, 3] with V <= 2^31 - 1")
    t = _hip.require_device_tensor(mesh.temperature, "temperature") if temperature else None
    tri = triangle_array(mesh.triangles)
    if t is not None and t.numel() != v:
        raise ValueError("temperature must hold V values")
    if tri.device != p.device or (t is not None and t.device != p.device):
        raise ValueError("positions, temperature and triangles must be on one device")
    return p, t, tri, int(v), int(tri.shape[0])


def check_incidence(incidence, tri: Tensor, v: int, t: int):
    """a caller's ``MeshIncidence`` for an entry that walks its lists: int32 device tensors of V + 1 offsets and 3 T corners on the
    triangles' device"""
    offsets = _hip.require_device_tensor(incidence.offsets, "offsets", torch.int32)
    corners = _hip.require_device_tensor(incidence.corners, "corners", torch.int32)
    if offsets.numel() != v + 1 or corners.numel() != 3 * t or offsets.device != tri.device or corners.device != tri.device:
        raise ValueError("incidence does not belong to a mesh of these vertices and triangles")
    return incidence


def color_array(colors, name: str, v: int, dev) -> Tensor:
    """a mesh's ``colors`` or ``thermal_colors`` for an entry that reads them: uint8 [V, 3]; one placeholder row for a mesh without
    vertices, whose colours nothing reads (an empty tensor has no address)"""
    c = _hip.require_device_tensor(colors, name, torch.uint8)
    if tuple(c.shape) != (v, 3) or c.device != dev:
        raise ValueError(f"{name} must be [V, 3] on the mesh's device")
    return c if v else torch.zeros((1, 3), dtype=torch.uint8, device=dev)


def tree_arrays(bvh):
    """(positions, temperature, triangles, V, T, device, blob) of a ``MeshBVH`` after the checks every reader of the tree starts with"""
    p, t, tri, v, n = mesh_arrays(bvh.mesh)
    if v != bvh.num_vertices or n != bvh.num_triangles:
        raise ValueError("the tree belongs to another mesh: its vertex and face counts differ")
    dev = p.device
    blob = bvh.blob
    if not isinstance(blob, Tensor) or not blob.is_cuda or blob.device != dev or not blob.is_contiguous():
        raise ValueError("the tree's blob must be a contiguous tensor on the mesh's device")
    return p, t, tri, v, n, dev, blob


def query_points(points: Tensor, letter: str, rows_only: bool = False) -> Tensor:
    """the query points, [``letter``, 3] as the message names them; ``rows_only``: two dimensions are all a public call asks before
    its ``*_into`` checks the rest"""
    q = _hip.require_device_tensor(points, "points")
    if q.dim() != 2 or not (rows_only or (q.shape[1] == 3 and 3 * q.shape[0] <= MAX_COUNT)):
        raise ValueError(f"points must be [{letter}, 3] with 3 {letter} <= 2^31 - 1")
    return q


def moments(total: float, squares: float, count: int) -> Tuple[float, float]:
    """(mean, root mean square) from the sum, the sum of squares and the count; NaN without a value"""
    return (total / count, math.sqrt(squares / count)) if count else (math.nan, math.nan)


def fill_differences(out, matched: int, s) -> None:
    """the five "differences" fields of ``ClosestPoints`` / ``ProjectedTemperatures`` from the host read: the points whose difference is
    a number, and ``s`` = the ordered sum, the ordered sum of squares, the minimum and the maximum of the differences"""
    out.matched = matched
    out.mean_difference, out.rms_difference = moments(s[0], s[1], matched)
    out.min_difference, out.max_difference = s[2], s[3]


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
