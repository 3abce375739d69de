"""Connected components of a triangle mesh and the removal of small ones — what a viewer's "remove small connected components"
does to the islands a TSDF volume makes of floaters, without losing the ``temperature`` of a vertex.

``tn_mesh_components`` labels every vertex with the smallest vertex index of its component (vertex connectivity: two triangles
that share one vertex are connected) by a lock-free union-find on the device and counts the triangles per component;
``tn_mesh_filter_components`` compacts the kept vertices and triangles in order (include/thermonerf_hip.h and DESIGN.md "Mesh
export" define every integer).  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import MAX_COUNT, out_tensor, triangle_array, workspace_of
from .mesh import ThermalMesh


class MeshComponents(NamedTuple):
    """``mesh_components``' outputs on the device: labels int32 [V] (the smallest vertex index of the vertex's component),
    component_triangles int32 [V] (at a label: its valid triangles; 0 elsewhere), summary int64 [3] (components, the largest
    triangle count, the label that holds it — the lowest on a tie)."""

    labels: Tensor
    component_triangles: Tensor
    summary: Tensor


@dataclasses.dataclass
class ComponentsInfo:
    """what ``remove_small_components`` found and took away"""

    components: int          # before the filter, isolated vertices included
    largest_triangles: int   # the triangle count of the largest component
    vertices_removed: int
    triangles_removed: int


def mesh_components_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_components_workspace_bytes(int(num_vertices), int(num_triangles)))


def _triangles(triangles: Tensor, num_vertices: int) -> Tuple[Tensor, int, int]:
    t = triangle_array(triangles)
    v = int(num_vertices)
    if not 0 <= v <= MAX_COUNT:
        raise ValueError("num_vertices must be 0 .. 2^31 - 1")
    return t, int(t.shape[0]), v


def mesh_components(triangles: Tensor, num_vertices: int) -> MeshComponents:
    """The connected components of ``triangles`` ([T,3] int32 on the device) over ``num_vertices`` vertices through
    ``tn_mesh_components``, on the current stream, without a host synchronisation.  A triangle with an index outside
    [0, num_vertices) connects nothing."""
    tri, t, v = _triangles(triangles, num_vertices)
    dev = tri.device
    with torch.cuda.device(dev):
        labels = torch.empty((v,), dtype=torch.int32, device=dev)
        component_triangles = torch.empty((v,), dtype=torch.int32, device=dev)
        summary = torch.empty((3,), dtype=torch.int64, device=dev)
        _hip.check(_hip.load().tn_mesh_components(tri.data_ptr() if t else None, t, v, labels.data_ptr() if v else None,
                                                  component_triangles.data_ptr() if v else None, summary.data_ptr(),
                                                  _hip.current_stream()), "tn_mesh_components")
    return MeshComponents(labels, component_triangles, summary)


def filter_components(triangles: Tensor, num_vertices: int, components: MeshComponents, *, counts: Tensor, min_triangles: int = 1,
                      largest_only: bool = False, vertex_source: Optional[Tensor] = None, triangles_out: Optional[Tensor] = None,
                      capacity_vertices: Optional[int] = None, capacity_triangles: Optional[int] = None,
                      workspace: Optional[Tensor] = None) -> None:
    """Keep the components with at least ``max(min_triangles, 1)`` triangles (``largest_only``: of those only the largest, the
    lowest label on a tie) through ``tn_mesh_filter_components``, on the current stream, without a host synchronisation.
    ``counts``: two device int64, OVERWRITTEN with the full numbers of kept vertices and triangles.  Outputs: vertex_source int32
    [V'] (the old indices of the kept vertices, ascending), triangles_out int32 [T',3] (the kept triangles in order, re-indexed);
    the capacities default to their rows (0 without them: the sizing call).  ``workspace``:
    ``mesh_components_workspace_bytes(V, T)`` device bytes (allocated if absent); its first int32 per vertex is the new index or -1."""
    tri, t, v = _triangles(triangles, num_vertices)
    if int(min_triangles) < 0:
        raise ValueError("min_triangles must not be negative")
    labels = _hip.require_device_tensor(components.labels, "labels", torch.int32)
    component_triangles = _hip.require_device_tensor(components.component_triangles, "component_triangles", torch.int32)
    summary = _hip.require_device_tensor(components.summary, "summary", torch.int64)
    if labels.numel() != v or component_triangles.numel() != v or summary.numel() != 3:
        raise ValueError("components does not belong to a mesh of num_vertices vertices")
    cap_v = int(vertex_source.shape[0] if vertex_source is not None else 0) if capacity_vertices is None else int(capacity_vertices)
    cap_t = int(triangles_out.shape[0] if triangles_out is not None else 0) if capacity_triangles is None else int(capacity_triangles)
    if cap_v < 0 or cap_t < 0:
        raise ValueError("a capacity must not be negative")
    vertex_source = out_tensor(vertex_source, "vertex_source", torch.int32, cap_v, 1)
    triangles_out = out_tensor(triangles_out, "triangles_out", torch.int32, cap_t, 3)
    counts = out_tensor(counts, "counts", torch.int64, 2, 1)
    if cap_v > 0 and vertex_source is None:
        raise ValueError("vertex_source is required when capacity_vertices > 0")
    if cap_t > 0 and triangles_out is None:
        raise ValueError("triangles_out is required when capacity_triangles > 0")
    workspace, workspace_size = workspace_of(workspace, mesh_components_workspace_bytes(v, t), tri.device)
    with torch.cuda.device(tri.device):
        _hip.check(_hip.load().tn_mesh_filter_components(
            tri.data_ptr() if t else None, t, v, labels.data_ptr() if v else None, component_triangles.data_ptr() if v else None,
            summary.data_ptr(), int(min_triangles), int(bool(largest_only)), _hip.ptr(vertex_source) if cap_v else None, cap_v,
            _hip.ptr(triangles_out) if cap_t else None, cap_t, counts.data_ptr(), workspace.data_ptr() if v else None,
            workspace_size, _hip.current_stream()), "tn_mesh_filter_components")


@torch.no_grad()
def remove_small_components(mesh: ThermalMesh, min_triangles: int = 1, largest_only: bool = False
                            ) -> Tuple[ThermalMesh, ComponentsInfo]:
    """``mesh`` without the components of fewer than ``max(min_triangles, 1)`` triangles — and, with ``largest_only``, without all
    but the largest.  Vertices in no triangle always go.  Both kernels run into outputs at their upper bounds (V and T); ONE host
    read fetches the two counts and the summary; the vertex attributes are gathered with ``index_select`` on ``vertex_source``.
    Returns (the filtered mesh, ``ComponentsInfo``)."""
    if mesh.triangles is None:
        raise ValueError("the mesh has no triangles")
    v, t = len(mesh), int(mesh.triangles.shape[0])
    dev = mesh.triangles.device
    with torch.cuda.device(dev):
        comp = mesh_components(mesh.triangles, v)
        counts = torch.empty((2,), dtype=torch.int64, device=dev)
        vertex_source = torch.empty((v,), dtype=torch.int32, device=dev)
        triangles = torch.empty((t, 3), dtype=torch.int32, device=dev)
        filter_components(mesh.triangles, v, comp, counts=counts, min_triangles=min_triangles, largest_only=largest_only,
                          vertex_source=vertex_source, triangles_out=triangles)
        kept_v, kept_t, components, largest, _ = (int(c) for c in torch.cat([counts, comp.summary]).tolist())  # the one read
        source = vertex_source[:kept_v].long()
        out = ThermalMesh(mesh.positions.index_select(0, source), mesh.colors.index_select(0, source),
                          mesh.temperature.index_select(0, source),
                          None if mesh.thermal_colors is None else mesh.thermal_colors.index_select(0, source),
                          triangles[:kept_t], mesh.temperature_bounds,
                          None if mesh.normals is None else mesh.normals.index_select(0, source))
    return out, ComponentsInfo(components, largest, v - kept_v, t - kept_t)
