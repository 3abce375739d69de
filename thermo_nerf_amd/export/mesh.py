"""Thermal triangle mesh of a trained scene — nerfstudio's TSDF exporter (fuse the rendered depth of every pose into a voxel
volume, extract a surface) with a temperature in degrees per vertex.

Pose by pose: rays -> ``RayRenderEngine.render`` -> ``tn_tsdf_integrate`` (one thread per voxel, nearest pixel, sums only); then
``tn_mesh_extract`` turns the volume into an indexed triangle list by surface nets — one vertex per sign-changing cell, one quad
per sign-changing grid edge, both compacted in order by count / scan / emit (include/thermonerf_hip.h and DESIGN.md "Mesh export"
define every value bit for bit).  Nothing synchronises between poses; the two counts are read once.  There is no CPU path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip, colormaps
from ._common import SCENE_BOX, PoseExporter, affine12, check_color_table, out_tensor, resolve_box, workspace_of

PLANES = 7  # tsdf_sum, weight, thermal_sum, r_sum, g_sum, b_sum, colour_weight
_POSE_CLAMP = float(np.float32(1e-4))  # the pose kernel's lower bound of |w|^2


def mesh_tile() -> int:
    """cells / grid points per tile of the count / emit kernels (one block each)"""
    return int(_hip.load().tn_mesh_tile())


def mesh_scan_width() -> int:
    """tile counts the one scan block takes per pass"""
    return int(_hip.load().tn_mesh_scan_width())


def mesh_workspace_bytes(dims: Sequence[int]) -> int:
    return int(_hip.load().tn_mesh_workspace_bytes(*(int(v) for v in dims)))


def grid_dims(lo: Sequence[float], hi: Sequence[float], resolution) -> Tuple[int, int, int]:
    """(Nx, Ny, Nz) grid points over the box.  ``resolution``: an int — the points along the longest side; a shorter side gets
    ``round(side / step) + 1`` with ``step = longest / (resolution - 1)``, at least 2 — or a triple taken as it is."""
    side = [float(h) - float(l) for l, h in zip(lo, hi)]
    if any(not s > 0.0 or math.isinf(s) for s in side):
        raise ValueError("the bounding box must have a finite positive extent on every axis")
    if isinstance(resolution, (int, np.integer)):
        if resolution < 2:
            raise ValueError("resolution must be at least 2")
        step = max(side) / (int(resolution) - 1)
        dims = tuple(max(2, int(round(s / step)) + 1) for s in side)
    else:
        dims = tuple(int(v) for v in resolution)
        if len(dims) != 3 or any(v < 2 for v in dims):
            raise ValueError("resolution is an int or three ints, each at least 2")
    return dims


def world_to_camera(c2w) -> np.ndarray:
    """fp64 [3,4]: [R^T | -R^T t] of a camera-to-world [R | t]"""
    m = np.asarray(c2w, dtype=np.float64).reshape(3, 4)
    rt = m[:, :3].T
    return np.concatenate([rt, -(rt @ m[:, 3:])], axis=1)


def set_camera(params, fx: float, fy: float, cx: float, cy: float, c2w) -> None:
    """the pose of ``tn_tsdf_integrate`` into ``params``: a pinhole and ``w2c``, composed in fp64 and rounded once"""
    params.fx, params.fy, params.cx, params.cy = float(fx), float(fy), float(cx), float(cy)
    w2c = world_to_camera(c2w).reshape(-1)
    for k in range(12):
        params.w2c[k] = float(w2c[k])


def mesh_params(lo: Sequence[float], hi: Sequence[float], dims: Sequence[int], truncation: float, min_accumulation: float = 0.5,
                max_temperature: float = 1.0, min_temperature: float = 0.0, to_world=None, camera=None) -> "_hip.tn_mesh_params":
    """The by-value parameter block of ``tn_tsdf_integrate`` and ``tn_mesh_extract``.  Every number is formed in double and rounded
    ONCE to fp32: ``step[c] = (hi[c] - lo[c]) / (dims[c] - 1)``, ``inv_truncation = 1 / truncation``, ``temperature_span = max -
    min``, ``to_world`` (row-major 3 x 4, default identity).  ``camera``: (fx, fy, cx, cy, c2w [3,4]) for ``set_camera``."""
    q = _hip.tn_mesh_params()
    if len(dims) != 3 or any(int(v) < 2 for v in dims):
        raise ValueError("dims are three grid-point counts, each at least 2")
    if not float(truncation) > 0.0:
        raise ValueError("truncation must be positive")
    for c in range(3):
        q.lo[c] = float(lo[c])
        q.step[c] = (float(hi[c]) - float(lo[c])) / (int(dims[c]) - 1)
        q.dims[c] = int(dims[c])
    q.truncation, q.inv_truncation = float(truncation), 1.0 / float(truncation)
    q.min_accumulation = float(min_accumulation)
    q.temperature_span = float(max_temperature) - float(min_temperature)
    q.temperature_min = float(min_temperature)
    q.to_world[:] = affine12(to_world)
    set_camera(q, *(camera if camera is not None else (1.0, 1.0, 0.0, 0.0, np.eye(3, 4))))
    return q


def _volume(volume: Tensor, params) -> Tensor:
    points = params.dims[0] * params.dims[1] * params.dims[2]
    v = _hip.require_device_tensor(volume, "volume")
    if v is not volume or v.numel() != PLANES * points:
        raise ValueError(f"volume must be a contiguous float32 device tensor of {PLANES} x {points} elements")
    return v


def tsdf_integrate(depth: Tensor, accumulation: Tensor, thermal: Tensor, rgb: Tensor, height: int, width: int, params,
                   volume: Tensor) -> None:
    """Fuse one rendered pose into ``volume`` ([7, Nz, Ny, Nx] float32, zeroed before the first pose) through
    ``tn_tsdf_integrate``, on the current stream, without a host synchronisation.  depth / accumulation / thermal hold
    ``height * width`` device floats, rgb [height * width, 3] (views into a larger allocation are fine); ``params``:
    ``mesh_params(...)`` with the pose's camera set (``set_camera``)."""
    n = int(height) * int(width)
    per_ray = [_hip.require_device_tensor(t, k) for t, k in ((depth, "depth"), (accumulation, "accumulation"), (thermal, "thermal"))]
    c = _hip.require_device_tensor(rgb, "rgb")
    if n < 1 or any(t.numel() != n for t in per_ray) or c.numel() != 3 * n:
        raise ValueError("depth / accumulation / thermal must hold height * width values and rgb three times as many")
    v = _volume(volume, params)
    with torch.cuda.device(v.device):
        _hip.check(_hip.load().tn_tsdf_integrate(per_ray[0].data_ptr(), per_ray[1].data_ptr(), per_ray[2].data_ptr(), c.data_ptr(),
                                                 int(height), int(width), params, v.data_ptr(), _hip.current_stream()),
                   "tn_tsdf_integrate")


def mesh_extract(volume: Tensor, params, *, counts: Tensor, positions: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                 temperature: Optional[Tensor] = None, thermal_colors: Optional[Tensor] = None,
                 thermal_table: Optional[Tensor] = None, triangles: Optional[Tensor] = None, capacity_vertices: Optional[int] = None,
                 capacity_triangles: Optional[int] = None, workspace: Optional[Tensor] = None) -> None:
    """Extract the surface of ``volume`` through ``tn_mesh_extract``, on the current stream, without a host synchronisation.
    ``counts``: two device int64, OVERWRITTEN with the full numbers of vertices and triangles.  Outputs: positions [V,3] float32,
    colors [V,3] uint8, temperature [V] float32, optionally thermal_colors [V,3] uint8 (with ``thermal_table`` uint8 [256,3]),
    triangles [T,3] int32; the capacities default to the rows of ``positions`` / ``triangles`` (0 without them: the sizing call).
    ``workspace``: ``mesh_workspace_bytes(dims)`` device bytes (allocated if absent); its first int32 per cell is ``cell_index``."""
    v = _volume(volume, params)
    cap_v = int(positions.shape[0] if positions is not None else 0) if capacity_vertices is None else int(capacity_vertices)
    cap_t = int(triangles.shape[0] if triangles is not None else 0) if capacity_triangles is None else int(capacity_triangles)
    if cap_v < 0 or cap_t < 0:
        raise ValueError("a capacity must not be negative")
    positions = out_tensor(positions, "positions", torch.float32, cap_v, 3)
    colors = out_tensor(colors, "colors", torch.uint8, cap_v, 3)
    temperature = out_tensor(temperature, "temperature", torch.float32, cap_v, 1)
    thermal_colors = out_tensor(thermal_colors, "thermal_colors", torch.uint8, cap_v, 3)
    triangles = out_tensor(triangles, "triangles", torch.int32, cap_t, 3)
    counts = out_tensor(counts, "counts", torch.int64, 2, 1)
    if cap_v > 0 and (positions is None or colors is None or temperature is None):
        raise ValueError("positions, colors and temperature are required when capacity_vertices > 0")
    if cap_t > 0 and triangles is None:
        raise ValueError("triangles are required when capacity_triangles > 0")
    if thermal_colors is not None:
        check_color_table(thermal_table)
    workspace, workspace_size = workspace_of(workspace, mesh_workspace_bytes(params.dims), v.device)
    with torch.cuda.device(v.device):
        _hip.check(_hip.load().tn_mesh_extract(
            v.data_ptr(), params, _hip.ptr(thermal_table) if thermal_colors is not None else None, _hip.ptr(positions),
            _hip.ptr(colors), _hip.ptr(temperature), _hip.ptr(thermal_colors), cap_v, _hip.ptr(triangles), cap_t, counts.data_ptr(),
            workspace.data_ptr(), workspace_size, _hip.current_stream()), "tn_mesh_extract")


@dataclass
class ThermalMesh:
    """V vertices and T triangles on the device: positions [V,3] float32, colors [V,3] uint8 (rendered RGB), temperature [V] float32
    in degrees Celsius, thermal_colors [V,3] uint8 (the colour-mapped normalised temperature), triangles [T,3] int32 (vertex
    indices, normals from inside to outside).  ``temperature_bounds``: the (min, max) degrees the normalised output was scaled with.
    ``normals``: [V,3] float32 unit vertex normals (``vertex_normals``), None unless asked for."""

    positions: Tensor
    colors: Tensor
    temperature: Tensor
    thermal_colors: Optional[Tensor] = None
    triangles: Optional[Tensor] = None
    temperature_bounds: Optional[Tuple[float, float]] = None
    normals: Optional[Tensor] = None

    def __len__(self) -> int:
        return int(self.positions.shape[0])


def _corrections(optimizer) -> Optional[np.ndarray]:
    """fp64 [N,3,4]: the rigid motion ``apply_to_raybundle`` applies per camera — directions <- R(w) directions, origins <- origins +
    t — from ONE read of the pose table; None when the optimizer is off.  R = I + a K(w) + b K(w)^2 with theta = sqrt(max(|w|^2,
    1e-4)), a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2 (tn_camera_opt_fwd); SE3: t = V(w) u, V = I + b K + c K^2,
    c = (theta - sin(theta)) / theta^3."""
    mode = optimizer.config.mode
    if mode == "off":
        return None
    table = optimizer.pose_adjustment.detach().double().cpu().numpy()
    out = np.zeros((table.shape[0], 3, 4), dtype=np.float64)
    for k, row in enumerate(table):
        u, w = row[:3], row[3:]
        theta = math.sqrt(max(float(w @ w), _POSE_CLAMP))
        a, b = math.sin(theta) / theta, (1.0 - math.cos(theta)) / theta ** 2
        kw = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        out[k, :, :3] = np.eye(3) + a * kw + b * (kw @ kw)
        if mode == "SE3":
            c = (theta - math.sin(theta)) / theta ** 3
            u = (np.eye(3) + b * kw + c * (kw @ kw)) @ u
        out[k, :, 3] = u
    return out


def _compose(c2w, correction: Optional[np.ndarray]) -> np.ndarray:
    m = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), dtype=np.float64).reshape(3, 4).copy()
    if correction is not None:  # the rotation acts on the directions (R_corr R), the translation is ADDED to the origins
        m[:, :3] = correction[:, :3] @ m[:, :3]
        m[:, 3] += correction[:, 3]
    return m


def camera_pose(model, cameras, k: int, apply_camera_optimizer: bool = True) -> np.ndarray:
    """fp64 [3,4]: the camera-to-world the rays of camera ``k`` are actually cast from — ``camera_to_worlds[k]`` composed with row
    ``k`` of the model's pose table exactly as ``CameraOptimizer.apply_to_raybundle`` applies it (the correction's rotation on the
    directions, its translation added to the origins; modes SO3xR3 and SE3), or the plain pose when the optimizer is off or
    ``apply_camera_optimizer`` is False."""
    corr = _corrections(model.camera_optimizer) if apply_camera_optimizer else None
    return _compose(cameras.camera_to_worlds[int(k)], None if corr is None else corr[int(k)])


class MeshExporter(PoseExporter):
    def __init__(self, model, *, max_temperature: float, min_temperature: float, resolution=256, bounding_box=SCENE_BOX,
                 truncation: Optional[float] = None, min_accumulation: float = 0.5, depth_output_name: str = "depth",
                 thermal_color_map: str = "magma", to_world=None) -> None:
        """``model``: a fusable ThermalNerfModel in eval mode on a ROCm device.
        ``max_temperature`` / ``min_temperature``: the degrees of normalised thermal 1 and 0.
        ``resolution``: grid points along the longest side of the box (``grid_dims``), or a triple (Nx, Ny, Nz).
        ``bounding_box``: [2,3] (min, max) in the normalised scene frame — the extent of the volume; default the model's
        ``scene_box.aabb``.  A box is required.
        ``truncation``: the TSDF band in scene units; default 4 x the largest grid step.  Below sqrt(3) x the largest step (a
        cell's diagonal) corners just behind the surface stay unobserved and their cells drop out: refused.
        ``min_accumulation``: pixels at or below this opacity observe nothing.
        ``depth_output_name``: "depth" (the median depth; default) or "expected_depth" (depends on the eval chunk size).
        ``thermal_color_map``: a name of ``colormaps.NAMES`` for ``thermal_colors``.
        ``to_world``: [3,4] applied to a vertex (``world_transform``); None: identity."""
        super().__init__(model, depth_output_name, thermal_color_map, min_temperature, max_temperature)
        box = resolve_box(model, bounding_box)
        if box is None:
            raise ValueError("a mesh needs a bounding box: it is the extent of the voxel volume")
        self.dims = grid_dims(box[0], box[1], resolution)
        largest = max((box[1][c] - box[0][c]) / (self.dims[c] - 1) for c in range(3))
        if truncation is None:
            truncation = 4.0 * largest
        if not float(truncation) >= math.sqrt(3.0) * largest:
            raise ValueError(f"truncation {float(truncation):.6g} is below sqrt(3) x the largest grid step {largest:.6g}")
        self.truncation = float(truncation)
        self.params = mesh_params(box[0], box[1], self.dims, truncation, min_accumulation, max_temperature, min_temperature, to_world)
        self.last_poses = 0  # poses fused by the last export
        self.last_components = None  # the ComponentsInfo of the last export, None when it removed no components
        self.last_simplify = None  # the SimplifyInfo of the last export, None when it did not simplify

    @torch.no_grad()
    def fuse(self, cameras, camera_indices: Optional[Sequence[int]] = None, apply_camera_optimizer: bool = True) -> Tensor:
        """Render ``cameras`` (all, or ``camera_indices``) and return the fused volume [7, Nz, Ny, Nx]; no host synchronisation
        after the pose table's one read."""
        dev, adjust, index, bundles = self._poses(cameras, camera_indices, apply_camera_optimizer, pinhole=True)
        corr = _corrections(self.model.camera_optimizer) if adjust else None
        nx, ny, nz = self.dims
        self.last_poses = len(index)
        with torch.cuda.device(dev):
            volume = torch.zeros((PLANES, nz, ny, nx), dtype=torch.float32, device=dev)
            out = None
            for k, rb in bundles:
                out = self._render(rb.origins, rb.directions, out)
                set_camera(self.params, float(cameras.fx[k]), float(cameras.fy[k]), float(cameras.cx), float(cameras.cy),
                           _compose(cameras.camera_to_worlds[k], None if corr is None else corr[k]))
                tsdf_integrate(out[self.depth_output_name], out["accumulation"], out["thermal"], out["rgb"], cameras.height,
                               cameras.width, self.params, volume)
        return volume

    @torch.no_grad()
    def extract(self, volume: Tensor) -> ThermalMesh:
        """the mesh of a fused volume: the sizing call, ONE host read of the two counts, exact allocation, the emitting call"""
        dev = volume.device
        with torch.cuda.device(dev):
            counts = torch.zeros((2,), dtype=torch.int64, device=dev)
            workspace = torch.empty((mesh_workspace_bytes(self.dims),), dtype=torch.uint8, device=dev)
            mesh_extract(volume, self.params, counts=counts, workspace=workspace)
            v, t = (int(c) for c in counts.tolist())  # the one synchronising read
            positions = torch.empty((v, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((v, 3), dtype=torch.uint8, device=dev)
            temperature = torch.empty((v,), dtype=torch.float32, device=dev)
            thermal_colors = torch.empty((v, 3), dtype=torch.uint8, device=dev)
            triangles = torch.empty((t, 3), dtype=torch.int32, device=dev)
            mesh_extract(volume, self.params, counts=counts, positions=positions, colors=colors, temperature=temperature,
                         thermal_colors=thermal_colors, thermal_table=colormaps.get_table(self.thermal_color_map, dev)[1],
                         triangles=triangles, workspace=workspace)
        return ThermalMesh(positions, colors, temperature, thermal_colors, triangles, self.temperature_bounds)

    def export(self, cameras, camera_indices: Optional[Sequence[int]] = None, apply_camera_optimizer: bool = True,
               min_component_triangles: int = 0, largest_component: bool = False, smooth_iterations: int = 0,
               smooth_lambda: float = 0.5, smooth_mu: float = -0.53, normals: bool = False,
               simplify_cell_size: float = 0.0) -> ThermalMesh:
        """Fuse ``cameras`` (all, or ``camera_indices``) in that order and return the surface.  ``apply_camera_optimizer``: adjust
        camera k's rays with row k of the model's pose table — right for the TRAINING cameras (pass False for other views).
        Cameras are rendered as PINHOLE views: ``distortion_params`` is ignored, because the export renders the model — it does
        not match photographs — and the fusion kernel projects a voxel through a pinhole.
        ``min_component_triangles`` > 0 drops the connected components (the islands floaters turn into) of fewer triangles,
        ``largest_component`` all but the largest (``remove_small_components``; ``last_components`` then tells what went).  With
        both off the mesh is the extraction's, untouched.
        ``simplify_cell_size`` > 0 then merges the vertices that share a grid cell of that edge — in the units of the positions as
        written, world units with ``to_world`` — into one averaged vertex and drops the triangles that collapse or repeat
        (``simplify_mesh``; ``last_simplify`` then tells what went).  It runs after the components are removed and before the
        smoothing, which relaxes the clustered surface; the normals are those of the final surface.
        ``smooth_iterations`` > 0 then relaxes the positions by that many Taubin iterations with the factors ``smooth_lambda`` /
        ``smooth_mu`` (``smooth_mesh``; colours and temperature do not move), and ``normals`` adds the area-weighted vertex normals
        of the FINAL positions and triangles.  With both off none of that code is called."""
        if int(min_component_triangles) < 0:
            raise ValueError("min_component_triangles must not be negative")
        if int(smooth_iterations) < 0:
            raise ValueError("smooth_iterations must not be negative")
        cell_size = float(simplify_cell_size)
        if not (cell_size >= 0.0 and math.isfinite(cell_size)):
            raise ValueError("simplify_cell_size must be finite and not negative")
        mesh = self.extract(self.fuse(cameras, camera_indices, apply_camera_optimizer))
        self.last_components = self.last_simplify = None
        if int(min_component_triangles) > 0 or largest_component:
            from .components import remove_small_components

            mesh, self.last_components = remove_small_components(mesh, int(min_component_triangles), bool(largest_component))
        if cell_size > 0.0:
            from .simplify import simplify_mesh

            mesh, self.last_simplify = simplify_mesh(mesh, cell_size)
        if int(smooth_iterations) > 0 or normals:
            from .smooth import smooth_mesh

            mesh = smooth_mesh(mesh, int(smooth_iterations), smooth_lambda, smooth_mu, normals=bool(normals))
        return mesh
