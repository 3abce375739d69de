"""Vertex normals and Taubin smoothing of a triangle mesh — what every viewer and every downstream tool asks a surface-nets mesh
for — on a device incidence index, without moving the ``temperature`` of a vertex.

``tn_mesh_incidence`` lists, per vertex, its incident triangle corners in a fixed order (a stable device sort of the corners by the
vertex they name); ``tn_mesh_vertex_normals`` sums the area-weighted face vectors of a list and normalises; ``tn_mesh_smooth`` runs
``iterations`` pairs of Jacobi passes (lambda, then mu: Taubin's filter, which does not shrink the surface the way plain Laplacian
smoothing does).  include/thermonerf_hip.h and DESIGN.md "Mesh export" define every value bit for bit.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import workspace_of
from .components import _triangles
from .mesh import ThermalMesh


class MeshIncidence(NamedTuple):
    """``mesh_incidence``'s outputs on the device: offsets int32 [V + 1], corners int32 [3 T] — corner ``c = 3 t + j`` is index j of
    triangle t; the list of vertex v is ``corners[offsets[v]:offsets[v + 1]]``, ascending; the corners of triangles with an index
    outside [0, V) follow ``offsets[V]``."""

    offsets: Tensor
    corners: Tensor


def mesh_incidence_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_incidence_workspace_bytes(int(num_vertices), int(num_triangles)))


def mesh_incidence(triangles: Tensor, num_vertices: int, workspace: Optional[Tensor] = None) -> MeshIncidence:
    """The incidence index of ``triangles`` ([T,3] int32 on the device) over ``num_vertices`` vertices through
    ``tn_mesh_incidence``, on the current stream, without a host synchronisation.  ``workspace``:
    ``mesh_incidence_workspace_bytes(V, T)`` device bytes (allocated if absent)."""
    tri, t, v = _triangles(triangles, num_vertices)
    dev = tri.device
    workspace, workspace_size = workspace_of(workspace, mesh_incidence_workspace_bytes(v, t), dev)
    with torch.cuda.device(dev):
        offsets = torch.empty((v + 1,), dtype=torch.int32, device=dev)
        corners = torch.empty((3 * t,), dtype=torch.int32, device=dev)
        _hip.check(_hip.load().tn_mesh_incidence(tri.data_ptr() if t else None, t, v, offsets.data_ptr(),
                                                 corners.data_ptr() if t else None, workspace.data_ptr() if workspace_size else None,
                                                 workspace_size, _hip.current_stream()), "tn_mesh_incidence")
    return MeshIncidence(offsets, corners)


def _indexed(positions: Tensor, triangles: Tensor, incidence: Optional[MeshIncidence]) -> Tuple[Tensor, Tensor, int, int, Tensor, Tensor]:
    """(positions, triangles, T, V, offsets, corners) after the checks the two per-vertex entries share; the index is built if absent"""
    pos = _hip.require_device_tensor(positions, "positions")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("positions must be [V, 3]")
    tri, t, v = _triangles(triangles, int(pos.shape[0]))
    if tri.device != pos.device:
        raise ValueError("positions and triangles must be on one device")
    if incidence is None:
        incidence = mesh_incidence(tri, v)
    offsets = _hip.require_device_tensor(incidence.offsets, "offsets", torch.int32)
    corners = _hip.require_device_tensor(incidence.corners, "corners", torch.int32)
    if offsets.numel() != v + 1 or corners.numel() != 3 * t:
        raise ValueError("incidence does not belong to a mesh of these vertices and triangles")
    return pos, tri, t, v, offsets, corners


def vertex_normals(positions: Tensor, triangles: Tensor, incidence: Optional[MeshIncidence] = None) -> Tensor:
    """float32 [V,3]: the area-weighted unit normal of every vertex through ``tn_mesh_vertex_normals`` — outward for a mesh of
    ``MeshExporter`` — or (0, 0, 0) for a vertex in no triangle of positive area.  On the current stream, without a host
    synchronisation.  ``incidence``: ``mesh_incidence(triangles, V)``, built if absent."""
    pos, tri, t, v, offsets, corners = _indexed(positions, triangles, incidence)
    with torch.cuda.device(pos.device):
        normals = torch.empty((v, 3), dtype=torch.float32, device=pos.device)
        _hip.check(_hip.load().tn_mesh_vertex_normals(pos.data_ptr() if v else None, tri.data_ptr() if t else None, t, v,
                                                      offsets.data_ptr(), corners.data_ptr() if t else None,
                                                      normals.data_ptr() if v else None, _hip.current_stream()),
                   "tn_mesh_vertex_normals")
    return normals


def _taubin(iterations: int, lambda_: float, mu: float) -> Tuple[int, float, float]:
    iterations, lambda_, mu = int(iterations), float(lambda_), float(mu)
    if iterations < 0:
        raise ValueError("iterations must not be negative")
    if not (lambda_ > 0.0 and mu < -lambda_ and math.isfinite(lambda_) and math.isfinite(mu)):
        raise ValueError("Taubin smoothing needs finite factors with lambda_ > 0 and mu < -lambda_")
    return iterations, lambda_, mu


def smooth_positions(positions: Tensor, triangles: Tensor, iterations: int, lambda_: float = 0.5, mu: float = -0.53,
                     incidence: Optional[MeshIncidence] = None) -> Tensor:
    """float32 [V,3]: ``positions`` after ``iterations`` Taubin iterations (a pass with ``lambda_``, a pass with ``mu``) through
    ``tn_mesh_smooth``; a new tensor, the input is left alone.  On the current stream, without a host synchronisation."""
    iterations, lambda_, mu = _taubin(iterations, lambda_, mu)
    pos, tri, t, v, offsets, corners = _indexed(positions, triangles, incidence)
    with torch.cuda.device(pos.device):
        out = torch.empty((v, 3), dtype=torch.float32, device=pos.device)
        scratch = torch.empty((v, 3), dtype=torch.float32, device=pos.device) if iterations else None
        _hip.check(_hip.load().tn_mesh_smooth(pos.data_ptr() if v else None, tri.data_ptr() if t else None, t, v, offsets.data_ptr(),
                                              corners.data_ptr() if t else None, iterations, lambda_, mu, out.data_ptr() if v else None,
                                              _hip.ptr(scratch) if v else None, _hip.current_stream()), "tn_mesh_smooth")
    return out


@torch.no_grad()
def smooth_mesh(mesh: ThermalMesh, iterations: int = 10, lambda_: float = 0.5, mu: float = -0.53, normals: bool = False) -> ThermalMesh:
    """``mesh`` with its positions smoothed by ``iterations`` Taubin iterations and, with ``normals``, the vertex normals of the
    smoothed surface.  The incidence index is built once; colours, temperature and triangles are the input's own tensors — a vertex
    keeps the measurement it was born with.  Without ``normals`` the result carries none (those of the input would be stale)."""
    if mesh.triangles is None:
        raise ValueError("the mesh has no triangles")
    _taubin(iterations, lambda_, mu)
    incidence = mesh_incidence(mesh.triangles, len(mesh))
    positions = smooth_positions(mesh.positions, mesh.triangles, iterations, lambda_, mu, incidence)
    return dataclasses.replace(mesh, positions=positions,
                               normals=vertex_normals(positions, mesh.triangles, incidence) if normals else None)
