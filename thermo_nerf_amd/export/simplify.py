"""Simplification of a thermal triangle mesh by vertex clustering — the "simplify: vertex clustering" of open3d / MeshLab, with a
temperature: the vertices that fall in one cell of a grid of edge ``cell_size`` become one vertex whose position, colours and
temperature are the mean over ALL of them (for a thermal mesh also the better measurement), the triangles are re-indexed, and those
that collapse (two corners in one cell) or repeat (the same three cells in the same orientation) go, with the cells no triangle
names any more.

``tn_mesh_simplify`` clusters the vertices exactly as ``tn_voxel_downsample`` clusters points (the same grid, keys, stable device
sort and ordered fp64 means), sorts the triangles' canonical cluster triples to find the repeats, and compacts vertices and
triangles in order; include/thermonerf_hip.h and DESIGN.md "Mesh simplification" define every output to the bit.  There is no CPU
path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import color_array, mesh_arrays, out_tensor, require_triangles, workspace_of
from .mesh import ThermalMesh
from .voxel import voxel_grid, voxel_params


@dataclasses.dataclass
class SimplifyInfo:
    """what ``simplify_mesh`` did"""

    vertices_before: int
    triangles_before: int
    vertices_after: int
    triangles_after: int
    degenerate_triangles: int   # dropped: an index out of range, a vertex outside the grid or not finite, two corners in one cell
    duplicate_triangles: int    # dropped: the same three cells in the same orientation as an earlier triangle
    cluster_count: Tensor       # int32 [vertices_after] on the device: the input vertices averaged into each output vertex


def mesh_simplify_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_simplify_workspace_bytes(int(num_vertices), int(num_triangles)))


def _simplify_arrays(mesh: ThermalMesh):
    """(positions, colors, temperature, thermal_colors or None, triangles, V, T): ``mesh_arrays`` and the colours the kernel averages"""
    p, t, tri, v, n = mesh_arrays(mesh)
    c = color_array(mesh.colors, "colors", v, p.device)
    tc = None if mesh.thermal_colors is None else color_array(mesh.thermal_colors, "thermal_colors", v, p.device)
    return p, c, t, tc, tri, v, n


def mesh_simplify_into(mesh: ThermalMesh, params, *, counts: Tensor, positions: Optional[Tensor] = None, colors: Optional[Tensor] = None,
                       temperature: Optional[Tensor] = None, cluster_count: Optional[Tensor] = None,
                       thermal_colors: Optional[Tensor] = None, triangles: Optional[Tensor] = None,
                       triangle_source: Optional[Tensor] = None, vertex_map: Optional[Tensor] = None,
                       capacity_vertices: Optional[int] = None, capacity_triangles: Optional[int] = None,
                       workspace: Optional[Tensor] = None) -> None:
    """``tn_mesh_simplify`` on the current stream, without a host synchronisation: ``mesh`` clustered over the grid ``params``
    (``voxel_params(...)``) into positions [V',3] float32, colors [V',3] uint8, temperature [V'] float32, cluster_count [V'] int32,
    optionally thermal_colors [V',3] uint8 (only if the mesh has them), triangles [T',3] int32, optionally triangle_source [T']
    int32 and vertex_map [V] int32.  ``counts``: four device int64, OVERWRITTEN with the full numbers of output vertices, output
    triangles, triangles dropped as invalid or degenerate and triangles dropped as duplicates.  The capacities default to the rows
    of ``positions`` / ``triangles`` (0 without them: the sizing call).  ``workspace``: ``mesh_simplify_workspace_bytes(V, T)``
    device bytes (allocated if absent)."""
    p, c, t, tc, tri, v, n = _simplify_arrays(mesh)
    cap_v = int(positions.shape[0] if positions is not None else 0) if capacity_vertices is None else int(capacity_vertices)
    cap_t = int(triangles.shape[0] if triangles is not None else 0) if capacity_triangles is None else int(capacity_triangles)
    if cap_v < 0 or cap_t < 0:
        raise ValueError("a capacity must not be negative")
    positions = out_tensor(positions, "positions", torch.float32, cap_v, 3)
    colors = out_tensor(colors, "colors", torch.uint8, cap_v, 3)
    temperature = out_tensor(temperature, "temperature", torch.float32, cap_v, 1)
    cluster_count = out_tensor(cluster_count, "cluster_count", torch.int32, cap_v, 1)
    thermal_colors = out_tensor(thermal_colors, "thermal_colors", torch.uint8, cap_v, 3)
    triangles = out_tensor(triangles, "triangles", torch.int32, cap_t, 3)
    triangle_source = out_tensor(triangle_source, "triangle_source", torch.int32, cap_t, 1)
    vertex_map = out_tensor(vertex_map, "vertex_map", torch.int32, v, 1)
    counts = out_tensor(counts, "counts", torch.int64, 4, 1)
    if counts is None:
        raise ValueError("counts is required")
    if cap_v > 0 and (positions is None or colors is None or temperature is None or cluster_count is None):
        raise ValueError("positions, colors, temperature and cluster_count are required when capacity_vertices > 0")
    if cap_t > 0 and triangles is None:
        raise ValueError("triangles are required when capacity_triangles > 0")
    if thermal_colors is not None and tc is None:
        raise ValueError("the mesh has no thermal_colors to average into the output given for it")
    dev = p.device
    workspace, size = workspace_of(workspace, mesh_simplify_workspace_bytes(v, n), dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_simplify(
            p.data_ptr() if v else None, c.data_ptr() if v else None, t.data_ptr() if v else None, _hip.ptr(tc) if v else None,
            tri.data_ptr() if n else None, v, n, C.byref(params), _hip.ptr(positions), _hip.ptr(colors), _hip.ptr(temperature),
            _hip.ptr(thermal_colors), _hip.ptr(cluster_count), cap_v, _hip.ptr(triangles), _hip.ptr(triangle_source), cap_t,
            _hip.ptr(vertex_map), counts.data_ptr(), workspace.data_ptr() if v else None, size, _hip.current_stream()),
            "tn_mesh_simplify")


def _cell_size(cell_size: float) -> float:
    size = C.c_float(float(cell_size)).value
    if not (size > 0.0 and math.isfinite(size)):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size}")
    return size


def _empty(mesh: ThermalMesh, before: Tuple[int, int], dropped: int) -> Tuple[ThermalMesh, SimplifyInfo]:
    dev = mesh.positions.device
    none = slice(0, 0)
    out = ThermalMesh(mesh.positions[none], mesh.colors[none], mesh.temperature[none],
                      None if mesh.thermal_colors is None else mesh.thermal_colors[none],
                      torch.empty((0, 3), dtype=torch.int32, device=dev), mesh.temperature_bounds)
    return out, SimplifyInfo(before[0], before[1], 0, 0, dropped, 0, torch.empty((0,), dtype=torch.int32, device=dev))


@torch.no_grad()
def simplify_mesh(mesh: ThermalMesh, cell_size: float) -> Tuple[ThermalMesh, SimplifyInfo]:
    """``mesh`` with one vertex per grid cell of edge ``cell_size`` (in the mesh's units) that a surviving triangle names: position,
    colours and temperature averaged over all the cell's vertices, vertices in ascending cell order, triangles in their input
    order.  The grid starts at the component-wise minimum of the finite vertices and ends with the cell of their maximum
    (``voxel_grid``, as ``voxel_downsample``).  Normals, if present, are dropped (they would be stale; compute them afterwards);
    ``temperature_bounds`` is carried over.  Two host reads: the six numbers of the bounding box, then the four counts.  Returns
    (the simplified mesh, ``SimplifyInfo``).  A ``cell_size`` that needs more than 2^21 cells on an axis raises ``ValueError``."""
    require_triangles(mesh)
    size = _cell_size(cell_size)
    p, _, _, _, _, v, t = _simplify_arrays(mesh)
    dev = p.device
    if v == 0:
        return _empty(mesh, (v, t), t)
    with torch.cuda.device(dev):
        finite = torch.isfinite(p).all(dim=1, keepdim=True)
        lo = torch.where(finite, p, torch.full_like(p, float("inf"))).amin(dim=0)
        hi = torch.where(finite, p, torch.full_like(p, float("-inf"))).amax(dim=0)
        box = torch.cat([lo, hi]).tolist()  # the one read of the six numbers
        if not math.isfinite(box[0]):
            return _empty(mesh, (v, t), t)
        origin, dims = voxel_grid(box[:3], box[3:], size)
        positions = torch.empty((v, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((v, 3), dtype=torch.uint8, device=dev)
        temperature = torch.empty((v,), dtype=torch.float32, device=dev)
        thermal_colors = None if mesh.thermal_colors is None else torch.empty((v, 3), dtype=torch.uint8, device=dev)
        cluster_count = torch.empty((v,), dtype=torch.int32, device=dev)
        triangles = torch.empty((t, 3), dtype=torch.int32, device=dev)
        counts = torch.empty((4,), dtype=torch.int64, device=dev)
        mesh_simplify_into(mesh, voxel_params(origin, size, dims), counts=counts, positions=positions, colors=colors,
                           temperature=temperature, cluster_count=cluster_count, thermal_colors=thermal_colors, triangles=triangles)
        m, k, degenerate, duplicate = (int(x) for x in counts.tolist())  # the one read of the counts
    out = ThermalMesh(positions[:m], colors[:m], temperature[:m], None if thermal_colors is None else thermal_colors[:m],
                      triangles[:k], mesh.temperature_bounds)
    return out, SimplifyInfo(v, t, m, k, degenerate, duplicate, cluster_count[:m])
