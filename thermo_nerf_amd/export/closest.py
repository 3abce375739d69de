"""The nearest point of a thermal mesh to any point — how far a cloud or a simplified mesh lies from the full one, what temperature the
surface has next to a point, and, between two surveys of one building, where the surface warmed or cooled and by how much: the
vertices of one mesh against the surface of the other give a per-vertex difference in degrees Celsius, as a ``ThermalMesh`` that
``thermal_regions`` and the thermograms read like any other.

``tn_mesh_closest`` walks the tree of ``build_mesh_bvh`` with one point per lane.  include/thermonerf_hip.h and DESIGN.md "Closest
point" define every output to the bit, without reference to the tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import color_array, fill_differences, mesh_arrays, moments, out_tensor, query_points, tree_arrays
from .mesh import ThermalMesh
from .raycast import MeshBVH


def check_max_distance(max_distance: float) -> None:
    """what ``tn_mesh_closest`` refuses of a search radius, with words"""
    if math.isnan(max_distance) or max_distance < 0.0:
        raise ValueError(f"max_distance must be a number >= 0 (it may be inf), got {max_distance}")


def mesh_closest_into(bvh: MeshBVH, points: Tensor, *, max_distance: float = math.inf, point_temperature: Optional[Tensor] = None,
                      closest_face: Optional[Tensor] = None, closest_distance: Optional[Tensor] = None,
                      closest_point: Optional[Tensor] = None, closest_uv: Optional[Tensor] = None,
                      closest_temperature: Optional[Tensor] = None, closest_colors: Optional[Tensor] = None,
                      difference: Optional[Tensor] = None, counts: Optional[Tensor] = None, stats: Optional[Tensor] = None) -> None:
    """``tn_mesh_closest`` on the current stream, without a host synchronisation: for every row of ``points`` [N, 3] the nearest
    point of the mesh of ``bvh`` within ``max_distance``.  ``closest_face`` int32 [N] (-1: none), ``closest_distance`` and
    ``closest_temperature`` float32 [N], ``closest_point`` float32 [N, 3], ``closest_uv`` float32 [N, 2] (NaN without a face),
    ``closest_colors`` uint8 [N, 3] (from ``mesh.colors``), ``difference`` float32 [N] = ``point_temperature`` - ``closest_temperature``
    (needs both), ``counts`` int64 [4] (points with a face, usable points, usable faces, points that reached the stack limit),
    ``stats`` float64 [8] (ordered sum, ordered sum of squares, minimum, maximum of the distances, then of the differences; needs
    ``closest_distance``): each optional."""
    check_max_distance(float(max_distance))
    p, t, tri, v, n, dev, blob = tree_arrays(bvh)
    q = query_points(points, "N")
    if q.device != dev:
        raise ValueError("the points must be on the mesh's device")
    count = int(q.shape[0])
    if point_temperature is not None:
        point_temperature = _hip.require_device_tensor(point_temperature, "point_temperature")
        if point_temperature.numel() != count or point_temperature.device != dev:
            raise ValueError("point_temperature must hold N values on the mesh's device")
    colors = color_array(bvh.mesh.colors, "colors", v, dev) if closest_colors is not None else None
    if difference is not None and (point_temperature is None or closest_temperature is None):
        raise ValueError("difference is point_temperature - closest_temperature: give both")
    if stats is not None and closest_distance is None:
        raise ValueError("stats are taken from closest_distance: give both")
    closest_face = out_tensor(closest_face, "closest_face", torch.int32, count, 1)
    closest_distance = out_tensor(closest_distance, "closest_distance", torch.float32, count, 1)
    closest_point = out_tensor(closest_point, "closest_point", torch.float32, count, 3)
    closest_uv = out_tensor(closest_uv, "closest_uv", torch.float32, count, 2)
    closest_temperature = out_tensor(closest_temperature, "closest_temperature", torch.float32, count, 1)
    closest_colors = out_tensor(closest_colors, "closest_colors", torch.uint8, count, 3)
    difference = out_tensor(difference, "difference", torch.float32, count, 1)
    counts = out_tensor(counts, "counts", torch.int64, 4, 1)
    stats = out_tensor(stats, "stats", torch.float64, 8, 1)
    if stats is not None and closest_distance.numel() == 0:  # no point: an empty tensor has no address, and NULL means "not given"
        closest_distance = closest_distance.new_empty((1,))
    params = _hip.tn_closest_params(float(max_distance))
    work = v > 0 and n > 0
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_closest(
            p.data_ptr() if work else None, t.data_ptr() if work else None, _hip.ptr(colors), tri.data_ptr() if n else None, v, n,
            blob.data_ptr(), blob.numel() * blob.element_size(), q.data_ptr() if count else None,
            _hip.ptr(point_temperature) if count else None, count, ctypes.byref(params), _hip.ptr(closest_face), _hip.ptr(closest_distance),
            _hip.ptr(closest_point), _hip.ptr(closest_uv), _hip.ptr(closest_temperature), _hip.ptr(closest_colors),
            _hip.ptr(difference) if count else None, _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()), "tn_mesh_closest")


@dataclasses.dataclass
class ClosestPoints:
    """what ``mesh_closest`` made: the arrays on the device and the numbers of the one host read.  Means and extremes are over the
    points that have the value; NaN, +inf and -inf without one."""

    closest_face: Tensor                  # int32 [N]: the nearest face, -1 without one within max_distance
    closest_distance: Tensor              # float32 [N]: NaN without a face
    closest_point: Tensor                 # float32 [N, 3]
    closest_uv: Tensor                    # float32 [N, 2]: the barycentrics of the face's second and third corner
    closest_temperature: Tensor           # float32 [N]: degrees Celsius of the surface there
    closest_colors: Optional[Tensor]      # uint8 [N, 3]
    difference: Optional[Tensor]          # float32 [N]: point_temperature - closest_temperature
    found: int
    usable_points: int
    usable_faces: int
    stack_limit_points: int               # 0: the stack covers the tree's depth bound
    mean_distance: float
    rms_distance: float
    min_distance: float
    max_distance: float
    mean_difference: Optional[float] = None   # the four: None unless temperatures were given
    rms_difference: Optional[float] = None
    min_difference: Optional[float] = None
    max_difference: Optional[float] = None
    matched: int = 0                      # points with a difference that is a number


@torch.no_grad()
def mesh_closest(bvh: MeshBVH, points: Tensor, *, max_distance: float = math.inf, point_temperature: Optional[Tensor] = None
                 ) -> ClosestPoints:
    """The nearest point of the mesh of ``bvh`` to every row of ``points`` as ``ClosestPoints`` (see ``mesh_closest_into``).  One
    host read: the four counts, the eight statistics and, with temperatures, the number of differences that are numbers."""
    check_max_distance(float(max_distance))
    p = _hip.require_device_tensor(bvh.mesh.positions, "positions")
    dev = p.device
    n = int(query_points(points, "N", rows_only=True).shape[0])
    with torch.cuda.device(dev):
        head = torch.zeros((13,), dtype=torch.int64, device=dev)  # the four counts, the eight statistics, the matched points
        face = torch.empty((n,), dtype=torch.int32, device=dev)
        distance, temperature = torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev)
        where, uv = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev) if bvh.mesh.colors is not None else None
        difference = torch.empty((n,), dtype=torch.float32, device=dev) if point_temperature is not None else None
        mesh_closest_into(bvh, points, max_distance=max_distance, point_temperature=point_temperature, closest_face=face,
                          closest_distance=distance, closest_point=where, closest_uv=uv, closest_temperature=temperature,
                          closest_colors=colors, difference=difference, counts=head[:4], stats=head[4:12].view(torch.float64))
        if difference is not None:
            head[12] = (difference == difference).sum()
        first = head.cpu().numpy()  # the one read
    found, usable_points, usable_faces, limit = (int(x) for x in first[:4])
    s = [float(x) for x in first[4:12].view(np.float64)]
    mean, rms = moments(s[0], s[1], found)
    out = ClosestPoints(face, distance, where, uv, temperature, colors, difference, found, usable_points, usable_faces, limit, mean, rms,
                        s[2], s[3])
    if difference is not None:
        fill_differences(out, int(first[12]), s[4:8])
    return out


@dataclasses.dataclass
class MeshDifference:
    """what ``mesh_difference`` made"""

    closest: ClosestPoints
    mesh: ThermalMesh             # the queried mesh with temperature = its own minus the reference surface's, NaN where unmatched
    matched: int                  # vertices with a difference
    matched_share: float          # of all vertices; 0.0 for a mesh without vertices
    mean_distance: float
    rms_distance: float
    max_distance: float
    mean_difference: float
    rms_difference: float
    min_difference: float
    max_difference: float


@torch.no_grad()
def mesh_difference(mesh: ThermalMesh, reference_bvh: MeshBVH, *, max_distance: float) -> MeshDifference:
    """Degrees Celsius of ``mesh`` minus degrees Celsius of the reference surface, per vertex of ``mesh``: every vertex is matched
    with the nearest point of the mesh of ``reference_bvh`` within ``max_distance`` (in the meshes' units; both must be in one
    frame).  The result's ``mesh`` has ``mesh``'s positions, colours, triangles and normals; its ``temperature`` is the difference —
    NaN where no reference surface lies within ``max_distance`` or the vertex's own temperature is not a number —, its
    ``thermal_colors`` is None and its ``temperature_bounds`` is (-m, m) with m the largest |difference| (None when nothing
    matched).  A NaN vertex makes its faces unusable for ``thermal_regions`` and the rasteriser: the parts of ``mesh`` without a
    counterpart are left out of every area, region and image of the difference.  One host read."""
    check_max_distance(float(max_distance))
    points, own, _, _, _ = mesh_arrays(mesh)
    found = mesh_closest(reference_bvh, points, max_distance=max_distance, point_temperature=own.reshape(-1))
    m = max(abs(found.min_difference), abs(found.max_difference)) if found.matched else None
    delta = ThermalMesh(mesh.positions, mesh.colors, found.difference, None, mesh.triangles, None if m is None else (-m, m), mesh.normals)
    return MeshDifference(found, delta, found.matched, found.matched / len(mesh) if len(mesh) else 0.0, found.mean_distance,
                          found.rms_distance, found.max_distance, found.mean_difference, found.rms_difference, found.min_difference,
                          found.max_difference)
