"""Thermal point cloud of a trained scene — nerfstudio's point-cloud exporter (back-project the rendered depth, drop transparent
and out-of-box rays, keep positions and colours) with a temperature in degrees per point.

Pose by pose: rays -> ``RayRenderEngine.render`` -> ``tn_pointcloud_append`` (filter, back-projection, ORDERED compaction behind a
device-resident counter, degrees and 8-bit colours; include/thermonerf_hip.h and DESIGN.md "Point-cloud export" define every
value bit for bit).  Nothing synchronises between poses: pose k+1 is queued behind pose k, and the counter is read once, at the
end.  There is no CPU path.
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

_INF = float("inf")


def tile_rays() -> int:
    """rays per tile of the count / emit kernels (one block each)"""
    return int(_hip.load().tn_pointcloud_tile_rays())


def scan_width() -> int:
    """tile counts the one scan block takes per pass"""
    return int(_hip.load().tn_pointcloud_scan_width())


def workspace_bytes(num_rays: int) -> int:
    return int(_hip.load().tn_pointcloud_workspace_bytes(int(num_rays)))


def pointcloud_params(min_accumulation: float = 0.5, box_min: Sequence[float] = (-_INF,) * 3, box_max: Sequence[float] = (_INF,) * 3,
                      thermal_lo: float = -_INF, thermal_hi: float = _INF, max_temperature: float = 1.0,
                      min_temperature: float = 0.0, to_world=None) -> "_hip.tn_pointcloud_params":
    """The by-value parameter block of ``tn_pointcloud_append``.  Every number is rounded ONCE, from a Python float (a double) to
    fp32: ``temperature_span`` is ``max - min`` in double, then rounded; ``to_world`` (row-major 3 x 4, default identity) likewise."""
    q = _hip.tn_pointcloud_params()
    q.min_accumulation = float(min_accumulation)
    for c in range(3):
        q.box_min[c], q.box_max[c] = float(box_min[c]), float(box_max[c])
    q.thermal_lo, q.thermal_hi = float(thermal_lo), float(thermal_hi)
    q.temperature_span = float(max_temperature) - float(min_temperature)
    q.temperature_min = float(min_temperature)
    q.to_world[:] = affine12(to_world)
    return q


def pointcloud_append(origins: Tensor, directions: Tensor, depth: Tensor, accumulation: Tensor, rgb: Tensor, thermal: Tensor,
                      params, *, positions: Tensor, colors: Tensor, temperature: Tensor, count: Tensor,
                      thermal_colors: Optional[Tensor] = None, thermal_table: Optional[Tensor] = None,
                      source: Optional[Tensor] = None, source_base: int = 0, capacity: Optional[int] = None,
                      workspace: Optional[Tensor] = None) -> None:
    """Append the surviving points of ``N`` rays behind ``count[0]`` through ``tn_pointcloud_append``, on the current stream, without
    a host synchronisation.  origins / directions / rgb [N,3], depth / accumulation / thermal [N] or [N,1] device floats (views at
    any ray of a larger allocation are fine); ``params``: ``pointcloud_params(...)``.  Outputs: positions [capacity,3] float32,
    colors [capacity,3] uint8, temperature [capacity] float32, optionally thermal_colors [capacity,3] uint8 (with
    ``thermal_table`` uint8 [256,3]) and source [capacity] int64; ``count``: one device int64, advanced by the FULL number kept —
    ``count > capacity`` after the caller's read-back means the buffers were too small (nothing is written beyond them).
    ``capacity`` defaults to the rows of ``positions``; ``workspace``: ``workspace_bytes(N)`` device bytes (allocated if absent)."""
    o = _hip.require_device_tensor(origins, "origins")
    n = o.shape[0] if o.dim() == 2 else -1
    if n < 0 or o.shape[1] != 3:
        raise ValueError("origins must be [N, 3]")
    d = _hip.require_device_tensor(directions, "directions")
    c = _hip.require_device_tensor(rgb, "rgb")
    per_ray = [_hip.require_device_tensor(t, k) for t, k in ((depth, "depth"), (accumulation, "accumulation"), (thermal, "thermal"))]
    if tuple(d.shape) != (n, 3) or tuple(c.shape) != (n, 3) or any(t.numel() != n for t in per_ray):
        raise ValueError("directions / rgb must be [N, 3] and depth / accumulation / thermal must hold N values")
    if capacity is None:
        capacity = positions.shape[0]
    capacity = int(capacity)
    if capacity < 0:
        raise ValueError("capacity must not be negative")
    positions = out_tensor(positions, "positions", torch.float32, capacity, 3)
    colors = out_tensor(colors, "colors", torch.uint8, capacity, 3)
    temperature = out_tensor(temperature, "temperature", torch.float32, capacity, 1)
    thermal_colors = out_tensor(thermal_colors, "thermal_colors", torch.uint8, capacity, 3)
    source = out_tensor(source, "source", torch.int64, capacity, 1)
    count = out_tensor(count, "count", torch.int64, 1, 1)
    if thermal_colors is not None:
        check_color_table(thermal_table)
    if n == 0:
        return
    workspace, workspace_size = workspace_of(workspace, workspace_bytes(n), o.device)
    with torch.cuda.device(o.device):
        _hip.check(_hip.load().tn_pointcloud_append(
            o.data_ptr(), d.data_ptr(), per_ray[0].data_ptr(), per_ray[1].data_ptr(), c.data_ptr(), per_ray[2].data_ptr(), n,
            int(source_base), params, _hip.ptr(thermal_table) if thermal_colors is not None else None, positions.data_ptr(),
            colors.data_ptr(), temperature.data_ptr(), _hip.ptr(thermal_colors), _hip.ptr(source), capacity, count.data_ptr(),
            workspace.data_ptr(), workspace_size, _hip.current_stream()), "tn_pointcloud_append")


@dataclass
class ThermalPointCloud:
    """M points on the device: positions [M,3] float32, colors [M,3] uint8 (rendered RGB), temperature [M] float32 in degrees
    Celsius, thermal_colors [M,3] uint8 (the colour-mapped normalised temperature), source [M] int64 (camera * H * W + pixel of
    the ray a point came from).  ``temperature_bounds``: the (min, max) degrees the normalised output was scaled with.  normals
    [M,3] float32 (unit, or zero where none could be estimated) once ``estimate_normals`` has run."""

    positions: Tensor
    colors: Tensor
    temperature: Tensor
    thermal_colors: Optional[Tensor] = None
    source: Optional[Tensor] = None
    temperature_bounds: Optional[Tuple[float, float]] = None
    normals: Optional[Tensor] = None

    def __len__(self) -> int:
        return int(self.positions.shape[0])

    def select(self, index) -> "ThermalPointCloud":
        """the points ``index`` picks (a slice or an int64 index tensor), in that order"""
        def pick(t):
            return None if t is None else t[index]

        return ThermalPointCloud(pick(self.positions), pick(self.colors), pick(self.temperature), pick(self.thermal_colors),
                                 pick(self.source), self.temperature_bounds, pick(self.normals))


def subsample_indices(num_points: int, keep: int, device="cpu") -> Tensor:
    """The deterministic thinning rule: of M points keep N < M, those at ``floor(j * M / N)`` for j < N (evenly spread over the
    cloud's order, first point included); M <= N keeps everything.  Integer arithmetic on ``device``."""
    m, n = int(num_points), int(keep)
    if n < 0:
        raise ValueError("the number of points to keep must not be negative")
    if m <= n:
        return torch.arange(m, dtype=torch.int64, device=device)
    return torch.arange(n, dtype=torch.int64, device=device) * m // n


def subsample(cloud: ThermalPointCloud, num_points: int) -> ThermalPointCloud:
    """``cloud`` thinned to at most ``num_points`` by ``subsample_indices`` (on the cloud's device); unchanged when it is smaller."""
    if len(cloud) <= int(num_points):
        return cloud
    return cloud.select(subsample_indices(len(cloud), num_points, cloud.positions.device))


def world_transform(dataparser_outputs) -> Tensor:
    """float32 [3,4]: normalised scene frame -> the dataset's original world frame, the inverse of the dataparser's pose
    normalisation (poses <- T poses, then translations * scale):  p_world = inverse([T; 0 0 0 1]) [p / scale; 1]  with
    T = ``dataparser_transform`` and scale = ``dataparser_scale``.  Composed in fp64 on the host, rounded once to fp32."""
    t = np.eye(4, dtype=np.float64)
    t[:3, :4] = np.asarray(torch.as_tensor(dataparser_outputs.dataparser_transform).detach().cpu().numpy(), dtype=np.float64)
    inv = np.linalg.inv(t)
    m = inv[:3, :4].copy()
    m[:, :3] /= float(dataparser_outputs.dataparser_scale)
    return torch.from_numpy(m.astype(np.float32))


class PointCloudExporter(PoseExporter):
    def __init__(self, model, *, max_temperature: float, min_temperature: float, depth_output_name: str = "depth",
                 min_accumulation: float = 0.5, bounding_box=SCENE_BOX, threshold: Optional[float] = None, cold: bool = False,
                 thermal_color_map: str = "magma", to_world=None) -> None:
        """``model``: a fusable ThermalNerfModel in eval mode on a ROCm device.
        ``max_temperature`` / ``min_temperature``: the degrees of normalised thermal 1 and 0 (``mae_thermal``'s de-normalisation).
        ``depth_output_name``: "depth" (the median depth; default) or "expected_depth" — the latter is clipped to the sample range
        of its eval CHUNK, so it depends on ``eval_num_rays_per_chunk`` (``RayRenderEngine.render``); "depth" does not.
        ``min_accumulation``: rays at or below this opacity are dropped (0.5: nerfstudio's exporter default, from recall).
        ``bounding_box``: [2,3] (min, max) in the normalised scene frame, strict on both sides; default the model's
        ``scene_box.aabb``; None: no box.
        ``threshold`` / ``cold``: keep predicted thermal > threshold, or < threshold when ``cold`` — the predicate ``mae_thermal``
        applies to ground truth; None: no thermal cut.
        ``thermal_color_map``: a name of ``colormaps.NAMES`` for ``thermal_colors``.
        ``to_world``: [3,4] applied to a kept point AFTER the box test (``world_transform``); None: identity."""
        super().__init__(model, depth_output_name, thermal_color_map, min_temperature, max_temperature)
        box = resolve_box(model, bounding_box) or [[-_INF] * 3, [_INF] * 3]
        lo, hi = -_INF, _INF
        if threshold is not None:
            if math.isnan(float(threshold)):
                raise ValueError("threshold is NaN")
            lo, hi = (-_INF, float(threshold)) if cold else (float(threshold), _INF)
        self.params = pointcloud_params(min_accumulation, box[0], box[1], lo, hi, max_temperature, min_temperature, to_world)
        self.last_rays = 0  # rays cast by the last export
        self.camera_viewpoints = None  # float32 [cameras.size, 3] on the device: where the last export's cameras stood (NaN rows: not rendered)
        self._rays_per_camera = 0

    @torch.no_grad()
    def export(self, cameras, camera_indices: Optional[Sequence[int]] = None, apply_camera_optimizer: bool = True,
               max_points: Optional[int] = None) -> ThermalPointCloud:
        """Render ``cameras`` (all, or ``camera_indices``) and return the points that pass the filter, in (camera, pixel) order.
        ``apply_camera_optimizer``: adjust camera k's rays with row k of the model's pose table — right for the TRAINING
        cameras, whose corrected poses the field was fitted to (pass False for other views).  ``max_points``: the buffers'
        capacity (default: every ray); a cloud that outgrows it raises with both numbers.  One host read at the end."""
        dev, _, index, bundles = self._poses(cameras, camera_indices, apply_camera_optimizer)
        n = cameras.height * cameras.width
        self.last_rays = n * len(index)
        capacity = self.last_rays if max_points is None else int(max_points)
        if capacity < 0:
            raise ValueError("max_points must not be negative")
        with torch.cuda.device(dev):
            positions = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
            temperature = torch.empty((capacity,), dtype=torch.float32, device=dev)
            thermal_colors = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
            source = torch.empty((capacity,), dtype=torch.int64, device=dev)
            count = torch.zeros((1,), dtype=torch.int64, device=dev)
            workspace = torch.empty((max(workspace_bytes(n), 8),), dtype=torch.uint8, device=dev)
            table = colormaps.get_table(self.thermal_color_map, dev)[1]
            viewpoints = torch.full((cameras.size, 3), float("nan"), dtype=torch.float32, device=dev)
            to_world = torch.tensor(list(self.params.to_world), dtype=torch.float32, device=dev).reshape(3, 4)
            out = None
            for k, rb in bundles:
                viewpoints[k] = to_world[:, :3] @ rb.origins[0] + to_world[:, 3]  # the corrected pose's centre, as the points are mapped
                out = self._render(rb.origins, rb.directions, out)
                pointcloud_append(rb.origins, rb.directions, out[self.depth_output_name], out["accumulation"], out["rgb"],
                                  out["thermal"], self.params, positions=positions, colors=colors, temperature=temperature,
                                  count=count, thermal_colors=thermal_colors, thermal_table=table, source=source,
                                  source_base=k * n, capacity=capacity, workspace=workspace)
            kept = int(count.item())  # the one synchronising read
        self.camera_viewpoints, self._rays_per_camera = viewpoints, n
        if kept > capacity:
            raise RuntimeError(f"the point cloud holds {kept} points but max_points = {capacity}; raise max_points or tighten the filter")
        return ThermalPointCloud(positions[:kept], colors[:kept], temperature[:kept], thermal_colors[:kept], source[:kept],
                                 self.temperature_bounds)

    def viewpoints(self, cloud: ThermalPointCloud) -> Tensor:
        """float32 [M,3]: for every point of ``cloud`` (a cloud of the last ``export``, or a selection of it) the centre of the camera
        it was seen from — the ray origin after the optimizer's correction, mapped through ``to_world`` like the points — gathered
        through ``cloud.source // (H * W)``.  What ``estimate_normals`` turns the normals towards."""
        if self.camera_viewpoints is None:
            raise RuntimeError("viewpoints() follows export()")
        if cloud.source is None:
            raise ValueError("the cloud carries no source indices")
        return self.camera_viewpoints[cloud.source // self._rays_per_camera]
