"""The measured thermal photos projected onto a mesh — what the camera actually measured at a spot of the reconstructed surface, from
how many photos the spot was seen and whether they agree (a hot spot that moves with the viewpoint is a reflection, not a defect),
and where the model's temperature differs from the photos.

``tn_mesh_project`` walks the tree of ``build_mesh_bvh`` with one point per lane and the loop over the cameras inside the lane: for
every camera the point is projected into the image (pinhole, no lens distortion), tested for facing and, with the ray ``visible_from``
casts, for occlusion, the 8-bit thermal image is sampled bilinearly and the samples are fused with the weight cos / distance^2.
include/thermonerf_hip.h and DESIGN.md "Projection" define every output to the bit.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import fill_differences, mesh_arrays, out_tensor, query_points, tree_arrays
from .mesh import ThermalMesh
from .raycast import CameraView, MeshBVH, check_camera
from .smooth import vertex_normals
from .thermogram import MAX_SIDE


def check_projection(temperature_bounds, min_cos: float, near: float) -> Tuple[float, float]:
    """what ``tn_mesh_project`` refuses of its parameters, with words; the bounds as (degrees of byte 0, degrees of byte 255)"""
    try:
        lo, hi = (float(x) for x in temperature_bounds)
    except (TypeError, ValueError):
        raise ValueError("temperature_bounds is (degrees of byte 0, degrees of byte 255): two numbers") from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"temperature_bounds must be finite, got ({lo}, {hi})")
    if not 0.0 < min_cos <= 1.0:
        raise ValueError(f"min_cos must be in (0, 1], got {min_cos}")
    if not near >= 0.0:
        raise ValueError(f"near must be >= 0, got {near}")
    return lo, hi


def camera_records(cameras: Sequence[CameraView]) -> Tuple[np.ndarray, int, int]:
    """(float32 [K, 16] — the ``tn_project_camera`` records —, width, height) of views that share one image size; (0, 0) without a
    view"""
    cameras = list(cameras)
    records = np.zeros((len(cameras), 16), np.float32)
    width = height = 0
    for k, camera in enumerate(cameras):
        check_camera(camera)
        if k == 0:
            width, height = int(camera.width), int(camera.height)
        elif (int(camera.width), int(camera.height)) != (width, height):
            raise ValueError(f"all views must share one image size: view 0 is {width} x {height}, view {k} is {camera.width} x {camera.height}")
        records[k, :12] = camera.matrix().reshape(-1)
        records[k, 12:] = (camera.fx, camera.fy, camera.cx, camera.cy)
    if cameras and not (2 <= width <= MAX_SIDE and 2 <= height <= MAX_SIDE):
        raise ValueError(f"a photo is 2 .. {MAX_SIDE} pixels on each side, got {width} x {height}")
    return records, width, height


def project_images_into(bvh: MeshBVH, points: Tensor, normals: Optional[Tensor], camera_table: Tensor, images: Tensor, temperature_bounds,
                        *, point_temperature: Optional[Tensor] = None, min_cos: float = 0.2, near: float = 0.0, two_sided: bool = False,
                        measured: Optional[Tensor] = None, views: Optional[Tensor] = None, best_camera: Optional[Tensor] = None,
                        spread: Optional[Tensor] = None, difference: Optional[Tensor] = None, counts: Optional[Tensor] = None,
                        stats: Optional[Tensor] = None) -> None:
    """``tn_mesh_project`` on the current stream, without a host synchronisation: the photos ``images`` uint8 [K, H, W] of the cameras
    ``camera_table`` float32 [K, 16] (``camera_records``, on the device) projected onto ``points`` [P, 3] with ``normals`` [P, 3] (None:
    no facing test) through the mesh of ``bvh``.  ``temperature_bounds``: the degrees of byte 0 and of byte 255.  ``measured`` and
    ``spread`` float32 [P] (NaN where no camera saw the point), ``views`` and ``best_camera`` int32 [P] (-1: unseen), ``difference``
    float32 [P] = ``point_temperature`` - measured (needs ``point_temperature``), ``counts`` int64 [6] (points seen, usable points,
    usable cameras, pairs that reached the occlusion test, pairs accepted, pairs at the stack limit), ``stats`` float64 [8] (ordered
    sum, sum of squares, minimum, maximum of the differences; sum and maximum of the spreads; sum of the measurements; 0 — each from
    its output array): each optional."""
    lo, hi = check_projection(temperature_bounds, float(min_cos), float(near))
    p, t, tri, v, n, dev, blob = tree_arrays(bvh)
    q = query_points(points, "P")
    count = int(q.shape[0])
    if normals is not None:
        normals = _hip.require_device_tensor(normals, "normals")
        if tuple(normals.shape) != (count, 3):
            raise ValueError(f"normals must be [P, 3] like the points, got {tuple(normals.shape)} for {count} points")
    table = _hip.require_device_tensor(camera_table, "camera_table")
    if table.dim() != 2 or table.shape[1] != 16:
        raise ValueError("camera_table must be [K, 16]: c2w (3 x 4, row-major), fx, fy, cx, cy")
    k = int(table.shape[0])
    photos = _hip.require_device_tensor(images, "images", torch.uint8)
    if photos.dim() != 3 or photos.shape[0] != k:
        raise ValueError(f"images must be uint8 [K, H, W] with one photo per camera, got {tuple(photos.shape)} for {k} cameras")
    height, width = int(photos.shape[1]), int(photos.shape[2])
    if not (2 <= width <= MAX_SIDE and 2 <= height <= MAX_SIDE):
        raise ValueError(f"a photo is 2 .. {MAX_SIDE} pixels on each side, got {width} x {height}")
    if point_temperature is not None:
        point_temperature = _hip.require_device_tensor(point_temperature, "point_temperature")
        if point_temperature.numel() != count:
            raise ValueError("point_temperature must hold P values")
    if any(x is not None and x.device != dev for x in (q, normals, table, photos, point_temperature)):
        raise ValueError("points, normals, cameras, images and point_temperature must be on the mesh's device")
    if difference is not None and point_temperature is None:
        raise ValueError("difference is point_temperature - measured: give point_temperature")
    measured = out_tensor(measured, "measured", torch.float32, count, 1)
    views = out_tensor(views, "views", torch.int32, count, 1)
    best_camera = out_tensor(best_camera, "best_camera", torch.int32, count, 1)
    spread = out_tensor(spread, "spread", torch.float32, count, 1)
    difference = out_tensor(difference, "difference", torch.float32, count, 1)
    counts = out_tensor(counts, "counts", torch.int64, 6, 1)
    stats = out_tensor(stats, "stats", torch.float64, 8, 1)
    params = _hip.tn_project_params(lo, hi, float(min_cos), float(near), width, height, 1 if two_sided else 0, 0)
    work = v > 0 and n > 0
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_project(
            p.data_ptr() if work else None, t.data_ptr() if work else None, tri.data_ptr() if n else None, v, n, blob.data_ptr(),
            blob.numel() * blob.element_size(), q.data_ptr() if count else None, _hip.ptr(normals) if count else None,
            _hip.ptr(point_temperature) if count else None, count, table.data_ptr() if k else None, photos.data_ptr() if k else None, k,
            ctypes.byref(params), _hip.ptr(measured), _hip.ptr(views), _hip.ptr(best_camera), _hip.ptr(spread),
            _hip.ptr(difference) if count else None, _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()), "tn_mesh_project")


@dataclasses.dataclass
class ProjectedTemperatures:
    """what ``project_images`` made: the arrays on the device and the numbers of the one host read.  Means and extremes are over the
    points that have the value; NaN, +inf and -inf without one."""

    measured: Tensor                  # float32 [P]: degrees Celsius the photos measured, NaN where no camera saw the point
    views: Tensor                     # int32 [P]: the cameras that saw the point
    best_camera: Tensor               # int32 [P]: the view of the largest weight (nearest and most frontal), -1 when unseen
    spread: Tensor                    # float32 [P]: warmest minus coldest view — what moves with the viewpoint is a reflection
    difference: Optional[Tensor]      # float32 [P]: point_temperature - measured, model minus measurement
    seen: int
    usable_points: int
    usable_cameras: int
    tested_pairs: int                 # (point, camera) pairs in the image and facing it: those that reached the occlusion test
    accepted_pairs: int
    stack_limit_pairs: int            # 0: the stack covers the tree's depth bound
    seen_share: float                 # of all points; 0.0 without a point
    mean_views: float                 # accepted pairs per point
    mean_measured: float
    mean_spread: float
    max_spread: float
    mean_difference: Optional[float] = None   # the four: None unless point temperatures were given
    rms_difference: Optional[float] = None
    min_difference: Optional[float] = None
    max_difference: Optional[float] = None
    matched: int = 0                  # points with a difference that is a number


@torch.no_grad()
def project_images(bvh: MeshBVH, points: Tensor, normals: Optional[Tensor], cameras: Sequence[CameraView], images: Tensor,
                   temperature_bounds, *, point_temperature: Optional[Tensor] = None, min_cos: float = 0.2, near: float = 0.0,
                   two_sided: bool = False) -> ProjectedTemperatures:
    """The photos ``images`` (uint8 [K, H, W] on the device, the dataset's 8-bit thermal images) of ``cameras`` (K ``CameraView`` of one
    width and height; lens distortion is ignored) projected onto ``points`` as ``ProjectedTemperatures`` (see ``project_images_into``).
    One host read: the six counts, the eight statistics and, with temperatures, the number of differences that are numbers."""
    check_projection(temperature_bounds, float(min_cos), float(near))
    records, width, height = camera_records(cameras)
    p = _hip.require_device_tensor(bvh.mesh.positions, "positions")
    dev = p.device
    n = int(query_points(points, "P", rows_only=True).shape[0])
    photos = _hip.require_device_tensor(images, "images", torch.uint8)
    if photos.dim() != 3 or photos.shape[0] != len(records) or (len(records) and tuple(photos.shape[1:]) != (height, width)):
        raise ValueError(f"images must be uint8 [K, H, W] = [{len(records)}, {height}, {width}] like the views, got {tuple(photos.shape)}")
    with torch.cuda.device(dev):
        table = torch.from_numpy(records).to(dev)
        head = torch.zeros((15,), dtype=torch.int64, device=dev)  # the six counts, the eight statistics, the matched points
        measured, spread = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
        views, best = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
        difference = torch.empty((n,), dtype=torch.float32, device=dev) if point_temperature is not None else None
        project_images_into(bvh, points, normals, table, photos, temperature_bounds, point_temperature=point_temperature, min_cos=min_cos,
                            near=near, two_sided=two_sided, measured=measured, views=views, best_camera=best, spread=spread,
                            difference=difference, counts=head[:6], stats=head[6:14].view(torch.float64))
        if difference is not None:
            head[14] = (difference == difference).sum()
        first = head.cpu().numpy()  # the one read
    seen, usable_points, usable_cameras, tested, accepted, limit = (int(x) for x in first[:6])
    s = [float(x) for x in first[6:14].view(np.float64)]
    out = ProjectedTemperatures(measured, views, best, spread, difference, seen, usable_points, usable_cameras, tested, accepted, limit,
                                seen / n if n else 0.0, accepted / n if n else 0.0, s[6] / seen if seen else math.nan,
                                s[4] / seen if seen else math.nan, s[5])
    if difference is not None:
        fill_differences(out, int(first[14]), s[0:4])
    return out


@dataclasses.dataclass
class MeshMeasurement:
    """what ``mesh_measurement`` made"""

    projected: ProjectedTemperatures
    measured: ThermalMesh         # the mesh with temperature = what the photos measured, NaN where no camera saw the vertex
    residual: ThermalMesh         # the mesh with temperature = model minus measurement, NaN where unseen; bounds (-m, m)
    seen: int                     # vertices at least one camera saw
    seen_share: float             # of all vertices; 0.0 for a mesh without vertices
    mean_views: float
    mean_difference: float
    rms_difference: float
    min_difference: float
    max_difference: float
    mean_spread: float
    max_spread: float


@torch.no_grad()
def mesh_measurement(mesh: ThermalMesh, bvh: MeshBVH, cameras: Sequence[CameraView], images: Tensor, temperature_bounds, *,
                     min_cos: float = 0.2, near: float = 0.0, two_sided: bool = False) -> MeshMeasurement:
    """The photos projected onto the vertices of ``mesh`` (``bvh``: its tree): the points are the vertices, the normals are
    ``vertex_normals`` of the mesh (``mesh.normals`` where set), ``point_temperature`` is the mesh's degrees Celsius.  ``measured``
    has ``mesh``'s positions, colours, triangles and normals and the measurement as its ``temperature`` — NaN where no camera saw the
    vertex, or its normal is (0, 0, 0) —, ``thermal_colors`` None and ``temperature_bounds`` the photos' (ascending).  ``residual``
    carries model minus measurement with ``temperature_bounds`` (-m, m), m the largest |difference| (None when nothing was seen).
    A NaN vertex makes its faces unusable for ``thermal_regions`` and the rasteriser: the parts of ``mesh`` that no photo shows are
    left out of every area, region and image of either mesh.  One host read."""
    lo, hi = check_projection(temperature_bounds, float(min_cos), float(near))
    points, own, triangles, _, _ = mesh_arrays(mesh)
    normals = mesh.normals if mesh.normals is not None else vertex_normals(points, triangles)
    got = project_images(bvh, points, normals, cameras, images, (lo, hi), point_temperature=own.reshape(-1), min_cos=min_cos, near=near,
                         two_sided=two_sided)
    m = max(abs(got.min_difference), abs(got.max_difference)) if got.matched else None
    shown = ThermalMesh(mesh.positions, mesh.colors, got.measured, None, mesh.triangles, (min(lo, hi), max(lo, hi)), mesh.normals)
    residual = ThermalMesh(mesh.positions, mesh.colors, got.difference, None, mesh.triangles, None if m is None else (-m, m), mesh.normals)
    return MeshMeasurement(got, shown, residual, got.seen, got.seen_share, got.mean_views, got.mean_difference, got.rms_difference,
                           got.min_difference, got.max_difference, got.mean_spread, got.max_spread)
