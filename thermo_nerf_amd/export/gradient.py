"""Where the temperature of a mesh changes fastest — the surface gradient of its degrees Celsius in degrees per world unit, which is
what shows a thermal bridge, a wet patch or an air leak where a threshold on the degrees themselves only finds the radiator — and the
filter such a derivative needs first: a NaN-aware Jacobi smoothing of the per-vertex scalar that can also fill the holes
``mesh_measurement`` and ``mesh_difference`` leave where nothing was seen.

``tn_mesh_scalar_smooth`` and ``tn_mesh_scalar_gradient`` walk the corner lists of ``mesh_incidence`` (smooth.py), one thread per
vertex; include/thermonerf_hip.h and DESIGN.md "Mesh export" define every value bit for bit.  Both results are ordinary
``ThermalMesh``es, so ``thermal_regions``, the thermograms, the camera view, ``isotherms`` and ``planar_patches`` read them unchanged:

    g = thermal_gradient(mesh, smooth_iterations=5)
    steep = thermal_regions(g.mesh, min_temperature=5.0)     # where it changes faster than 5 degrees Celsius per unit
    image = mesh_thermogram(g.mesh, view)                    # the gradient image

There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import mesh_arrays, workspace_of
from .components import _triangles
from .mesh import ThermalMesh
from .smooth import MeshIncidence, _indexed, mesh_incidence


class ScalarGradient(NamedTuple):
    """``scalar_gradient``'s outputs on the device: face_gradient float64 [T, 3] (NaN rows for the faces that are not usable),
    vertex_gradient float32 [V, 3] and vertex_magnitude float32 [V] (NaN for a vertex without a usable face), totals float64 [4]:
    the usable faces, the sum of twice their areas, the sum of twice the area times |g|, the largest |g|."""

    face_gradient: Tensor
    vertex_gradient: Tensor
    vertex_magnitude: Tensor
    totals: Tensor


@dataclasses.dataclass
class MeshGradient:
    """what ``thermal_gradient`` made"""

    face_gradient: Tensor        # float64 [T, 3] on the device, degrees per world unit; NaN rows for the faces that are not usable
    vertex_gradient: Tensor      # float32 [V, 3] on the device; NaN for a vertex without a usable face
    mesh: ThermalMesh            # the input mesh with temperature = |vertex gradient|, bounds (0, max_magnitude) or None
    usable_faces: int
    mean_magnitude: float        # over the usable faces, weighted by area; NaN without one
    max_magnitude: float         # the steepest usable face; NaN without one


def mesh_scalar_gradient_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_scalar_gradient_workspace_bytes(int(num_vertices), int(num_triangles)))


def _factors(iterations: int, lambda_: float, mu: float) -> Tuple[int, float, float]:
    iterations, lambda_, mu = int(iterations), float(lambda_), float(mu)
    if iterations < 0:
        raise ValueError("iterations must not be negative")
    if not (math.isfinite(lambda_) and math.isfinite(mu)):
        raise ValueError("lambda_ and mu must be finite")
    return iterations, lambda_, mu


def _values(values: Tensor, v: int, dev) -> Tensor:
    x = _hip.require_device_tensor(values, "values")
    if x.dim() != 1 or x.shape[0] != v or x.device != dev:
        raise ValueError("values must be [V] on the device of the triangles")
    return x


def smooth_values(values: Tensor, triangles: Tensor, num_vertices: int, iterations: int, lambda_: float = 0.5, mu: float = 0.0,
                  fill: bool = False, incidence: Optional[MeshIncidence] = None) -> Tensor:
    """float32 [V]: ``values`` after ``iterations`` iterations of ``tn_mesh_scalar_smooth`` — a pass with ``lambda_`` and, unless
    ``mu`` is 0, a pass with ``mu`` — over the finite values: a NaN is no neighbour of anything and stays a NaN, or, with ``fill``,
    takes the mean of its finite neighbours, one ring of a hole per pass.  A new tensor; on the current stream, without a host
    synchronisation.  ``incidence``: ``mesh_incidence(triangles, V)``, built if absent."""
    iterations, lambda_, mu = _factors(iterations, lambda_, mu)
    tri, t, v = _triangles(triangles, num_vertices)
    x = _values(values, v, tri.device)
    if incidence is None:
        incidence = mesh_incidence(tri, v)
    offsets = _hip.require_device_tensor(incidence.offsets, "offsets", torch.int32)
    corners = _hip.require_device_tensor(incidence.corners, "corners", torch.int32)
    if offsets.numel() != v + 1 or corners.numel() != 3 * t:
        raise ValueError("incidence does not belong to a mesh of these vertices and triangles")
    with torch.cuda.device(x.device):
        out = torch.empty((v,), dtype=torch.float32, device=x.device)
        scratch = torch.empty((v,), dtype=torch.float32, device=x.device) if iterations else None
        _hip.check(_hip.load().tn_mesh_scalar_smooth(x.data_ptr() if v else None, tri.data_ptr() if t else None, t, v, offsets.data_ptr(),
                                                     corners.data_ptr() if t else None, iterations, lambda_, mu, 1 if fill else 0,
                                                     out.data_ptr() if v else None, _hip.ptr(scratch) if v else None,
                                                     _hip.current_stream()), "tn_mesh_scalar_smooth")
    return out


def _replaced(mesh: ThermalMesh, temperature: Tensor, bounds) -> ThermalMesh:
    """``mesh`` with another temperature: the thermal colours of the old one would be stale"""
    return dataclasses.replace(mesh, temperature=temperature, thermal_colors=None, temperature_bounds=bounds)


@torch.no_grad()
def smooth_temperature(mesh: ThermalMesh, iterations: int, lambda_: float = 0.5, mu: float = 0.0, fill: bool = False) -> ThermalMesh:
    """``mesh`` with its temperature smoothed by ``smooth_values``: positions, colours, triangles, normals and
    ``temperature_bounds`` are the input's own; ``thermal_colors`` is None (those of the input would be stale).  No host read."""
    _factors(iterations, lambda_, mu)
    _, temperature, tri, v, _ = mesh_arrays(mesh)
    return _replaced(mesh, smooth_values(temperature.reshape(-1), tri, v, iterations, lambda_, mu, fill), mesh.temperature_bounds)


@torch.no_grad()
def fill_temperature(mesh: ThermalMesh, max_iterations: int) -> Tuple[ThermalMesh, int]:
    """(``mesh`` with the vertices that have no temperature — NaN or infinite, as ``mesh_measurement`` and ``mesh_difference`` leave
    them where nothing was seen — filled from their neighbours, how many such vertices remain).  ``max_iterations`` passes with
    factor 0 and ``fill``: a vertex with a temperature keeps it, a hole closes by one ring of vertices per pass, an island without any
    temperature stays empty.  One host read: the count."""
    filled = smooth_temperature(mesh, max_iterations, lambda_=0.0, mu=0.0, fill=True)
    return filled, int((~torch.isfinite(filled.temperature)).sum().item())


def scalar_gradient(positions: Tensor, values: Tensor, triangles: Tensor, incidence: Optional[MeshIncidence] = None,
                    workspace: Optional[Tensor] = None) -> ScalarGradient:
    """The gradient of the piecewise linear interpolant of ``values`` [V] over the mesh through ``tn_mesh_scalar_gradient``: per face,
    per vertex (the mean of the usable faces around it, weighted by area) and its length, and the totals.  On the current stream,
    without a host synchronisation.  ``workspace``: ``mesh_scalar_gradient_workspace_bytes(V, T)`` device bytes (allocated if
    absent)."""
    pos, tri, t, v, offsets, corners = _indexed(positions, triangles, incidence)
    x = _values(values, v, pos.device)
    dev = pos.device
    workspace, size = workspace_of(workspace, mesh_scalar_gradient_workspace_bytes(v, t) if t else 0, dev)
    with torch.cuda.device(dev):
        face_gradient = torch.empty((t, 3), dtype=torch.float64, device=dev)
        vertex_gradient = torch.empty((v, 3), dtype=torch.float32, device=dev)
        vertex_magnitude = torch.empty((v,), dtype=torch.float32, device=dev)
        totals = torch.empty((4,), dtype=torch.float64, device=dev)
        _hip.check(_hip.load().tn_mesh_scalar_gradient(
            pos.data_ptr() if v else None, x.data_ptr() if v else None, tri.data_ptr() if t else None, t, v, offsets.data_ptr(),
            corners.data_ptr() if t else None, face_gradient.data_ptr() if t else None, vertex_gradient.data_ptr() if v else None,
            vertex_magnitude.data_ptr() if v else None, totals.data_ptr(), workspace.data_ptr() if t else None, size,
            _hip.current_stream()), "tn_mesh_scalar_gradient")
    return ScalarGradient(face_gradient, vertex_gradient, vertex_magnitude, totals)


@torch.no_grad()
def thermal_gradient(mesh: ThermalMesh, smooth_iterations: int = 0, lambda_: float = 0.5, mu: float = 0.0) -> MeshGradient:
    """The surface gradient of ``mesh``'s temperature in degrees Celsius per world unit, after ``smooth_iterations`` iterations of
    ``smooth_values`` (the degrees of a surface-nets vertex are one voxel's noisy sample: a derivative of them is mostly noise).  The
    result's ``mesh`` has the input's positions, colours, triangles and normals, ``temperature`` = the length of the vertex gradient,
    ``thermal_colors`` None and ``temperature_bounds`` (0, the steepest face) — None when no face is usable —, so that

        thermal_regions(g.mesh, min_temperature=5.0)    # the regions that change faster than 5 degrees Celsius per unit
        mesh_thermogram(g.mesh, view)                   # the gradient image

    work as they do on degrees.  The incidence index is built once.  One host read: the totals."""
    iterations, lambda_, mu = _factors(smooth_iterations, lambda_, mu)
    positions, temperature, tri, v, _ = mesh_arrays(mesh)
    incidence = mesh_incidence(tri, v)
    values = temperature.reshape(-1)
    if iterations:
        values = smooth_values(values, tri, v, iterations, lambda_, mu, incidence=incidence)
    found = scalar_gradient(positions, values, tri, incidence)
    usable, weight, weighted, steepest = found.totals.cpu().tolist()  # the one read
    usable = int(usable)
    gradient_mesh = _replaced(mesh, found.vertex_magnitude, (0.0, steepest) if usable else None)
    return MeshGradient(found.face_gradient, found.vertex_gradient, gradient_mesh, usable,
                        weighted / weight if usable else math.nan, steepest if usable else math.nan)
