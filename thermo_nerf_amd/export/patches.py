"""Planar patches of a mesh — which walls, floors and roof planes does this model consist of, how large is each and how warm: the
faces are joined across edges (the half-edge twins of ``mesh_half_edges``) while the angle between their normals stays under a limit,
and every patch gets its fitted plane, area, flatness, deviation from the plane and its area-weighted mean / min / max temperature.
With the limit at 180 degrees the patches are the edge-connected components.  ``patch_view`` turns "patch k" into the view that looks
straight at it, so nobody types a normal.

The criterion is adjacency chaining: a gently curved surface whose neighbouring faces all stay under the angle is ONE patch;
``flatness`` and ``rms_deviation`` are how the caller sees that.

``tn_mesh_patches`` does all of it on the device (a record per face, a lock-free union-find over the faces hooked per half-edge, the
stable device sort, ordered fp64 sums in blocks of 256, twice); include/thermonerf_hip.h and DESIGN.md "Planar patches" define every
output to the bit.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import mesh_arrays, out_tensor, require_triangles, workspace_of
from .isolines import MeshHalfEdges, mesh_half_edges
from .mesh import ThermalMesh
from .regions import order_regions
from .thermogram import RasterView, fit_view

# a row of the patch table: tn_mesh_patch, field for field (136 bytes, no padding)
PATCH_DTYPE = np.dtype([("area", "<f8"), ("thermal_area", "<f8"), ("plane", "<f8", (4,)), ("centroid", "<f8", (3,)), ("flatness", "<f4"),
                        ("rms_deviation", "<f4"), ("max_deviation", "<f4"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                        ("max_temperature", "<f4"), ("bounds", "<f4", (6,)), ("label", "<i4"), ("faces", "<i4"),
                        ("thermal_faces", "<i4"), ("reserved", "<i4")])
PATCH_BYTES = PATCH_DTYPE.itemsize


@dataclasses.dataclass
class MeshPatches:
    """what ``planar_patches`` found"""

    patches: np.ndarray        # PATCH_DTYPE [K] on the host: the kept patches, largest area first
    patch_index: np.ndarray    # int64 [K]: the number q of every kept patch, as ``face_patch`` names it
    face_patch: Tensor         # int32 [T] on the device: q of every geometric face (kept or not), -1 of every other
    mesh_area: float           # the area of all geometric faces
    thermal_area: float        # the area of those with three finite temperatures
    num_patches: int           # Q: all patches, before ``min_area`` and ``top``
    geometric_faces: int
    joined_half_edges: int     # half-edges across which two faces were joined
    min_cos: float

    def __len__(self) -> int:
        return int(self.patches.shape[0])

    # what ``regions_mesh`` and ``PixelImage.region_map`` read of a ``ThermalRegions``
    @property
    def face_region(self) -> Tensor:
        return self.face_patch

    @property
    def region_index(self) -> np.ndarray:
        return self.patch_index

    @property
    def num_regions(self) -> int:
        return self.num_patches

    def only(self, k: int) -> "MeshPatches":
        """kept patch ``k`` alone: ``regions_mesh(mesh, patches.only(k))`` is that wall as a mesh"""
        k = _kept(self, k)
        return dataclasses.replace(self, patches=self.patches[k:k + 1].copy(), patch_index=self.patch_index[k:k + 1].copy())


def mesh_patches_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_patches_workspace_bytes(int(num_vertices), int(num_triangles)))


def _min_cos(min_cos: float) -> float:
    c = float(min_cos)
    if math.isnan(c) or c < -1.0 or c > 1.0:
        raise ValueError(f"min_cos must be a number within -1 .. 1, got {min_cos}")
    return c


def _cos_of_degrees(max_angle_degrees: float) -> float:
    a = float(max_angle_degrees)
    if math.isnan(a) or a < 0.0 or a > 180.0:
        raise ValueError(f"max_angle_degrees must be a number within 0 .. 180, got {max_angle_degrees}")
    return math.cos(math.radians(a))


def mesh_patches_into(mesh: ThermalMesh, twin: Tensor, min_cos: float, *, counts: Tensor, totals: Tensor,
                      face_patch: Optional[Tensor] = None, patches: Optional[Tensor] = None, capacity_patches: Optional[int] = None,
                      workspace: Optional[Tensor] = None) -> None:
    """``tn_mesh_patches`` on the current stream, without a host synchronisation: the geometric faces of ``mesh`` joined across the
    edges of ``twin`` (int32 [3T], as ``mesh_half_edges`` returns it) where the dot product of their unit normals is at least
    ``min_cos`` (a number within -1 .. 1).  ``counts``: three device int64, OVERWRITTEN with the full number of patches, the geometric
    faces and the joined half-edges; ``totals``: two device float64, the mesh's area and the thermal area; ``face_patch``: int32 [T]
    (required when the mesh has faces); ``patches``: a uint8 device tensor of ``PATCH_BYTES`` per row, read on the host as
    ``PATCH_DTYPE``.  ``capacity_patches`` defaults to the rows ``patches`` can hold (0 without it: the sizing call).  ``workspace``:
    ``mesh_patches_workspace_bytes(V, T)`` device bytes (allocated if absent)."""
    require_triangles(mesh)
    c = _min_cos(min_cos)
    # (the type and the length of twin need no device: refused before the checks that do)
    if not isinstance(twin, Tensor) or twin.dtype != torch.int32:
        raise TypeError("twin must be an int32 torch.Tensor")
    if not isinstance(mesh.triangles, Tensor) or twin.numel() != mesh.triangles.numel():
        raise ValueError("twin must hold 3 T values, one per half-edge of the mesh")
    p, t, tri, v, n = mesh_arrays(mesh)
    twin = _hip.require_device_tensor(twin, "twin", torch.int32)
    if twin.device != p.device:
        raise ValueError("twin must be on the mesh's device")
    if patches is not None and (not isinstance(patches, Tensor) or patches.dtype != torch.uint8):
        raise ValueError("patches must be a uint8 device tensor")
    cap = int(patches.numel() // PATCH_BYTES if patches is not None else 0) if capacity_patches is None else int(capacity_patches)
    if cap < 0:
        raise ValueError("a capacity must not be negative")
    patches = out_tensor(patches, "patches", torch.uint8, cap, PATCH_BYTES)
    face_patch = out_tensor(face_patch, "face_patch", torch.int32, n, 1)
    counts = out_tensor(counts, "counts", torch.int64, 3, 1)
    totals = out_tensor(totals, "totals", torch.float64, 2, 1)
    if counts is None or totals is None:
        raise ValueError("counts and totals are required")
    if n > 0 and face_patch is None:
        raise ValueError("face_patch is required when the mesh has faces")
    if cap > 0 and patches is None:
        raise ValueError("patches are required when capacity_patches > 0")
    dev = p.device
    work = v > 0 and n > 0
    workspace, size = workspace_of(workspace, mesh_patches_workspace_bytes(v, n) if work else 0, dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_patches(
            p.data_ptr() if v else None, t.data_ptr() if v else None, tri.data_ptr() if n else None, v, n, twin.data_ptr() if n else None,
            c, _hip.ptr(patches), cap, _hip.ptr(face_patch) if n else None, counts.data_ptr(), totals.data_ptr(),
            workspace.data_ptr() if work else None, size, _hip.current_stream()), "tn_mesh_patches")


def _patches(mesh: ThermalMesh, min_cos: float, half_edges: Optional[MeshHalfEdges], min_area: float, top: Optional[int]) -> MeshPatches:
    order_regions(np.zeros(0, PATCH_DTYPE), min_area, top)  # the refusals, before anything runs
    p, _, tri, v, t = mesh_arrays(mesh)
    if half_edges is None:
        half_edges = mesh_half_edges(tri, v)
    dev = p.device
    cap = t  # a patch has a face
    with torch.cuda.device(dev):
        head = torch.empty((5,), dtype=torch.int64, device=dev)  # the three counts and, behind them, the two areas
        rows = torch.empty((cap * PATCH_BYTES,), dtype=torch.uint8, device=dev)
        face_patch = torch.empty((t,), dtype=torch.int32, device=dev)
        mesh_patches_into(mesh, half_edges.twin, min_cos, counts=head[:3], totals=head[3:].view(torch.float64), face_patch=face_patch,
                          patches=rows if cap else None, capacity_patches=cap)
        first = head.cpu().numpy()  # the one read of the counts and the areas
        q, geometric, joined = (int(x) for x in first[:3])
        mesh_area, thermal_area = (float(x) for x in first[3:].view(np.float64))
        table = np.frombuffer(rows[:q * PATCH_BYTES].cpu().numpy().tobytes(), dtype=PATCH_DTYPE) if q else np.zeros(0, PATCH_DTYPE)
    keep = order_regions(table, min_area, top)
    return MeshPatches(table[keep].copy(), keep, face_patch, mesh_area, thermal_area, q, geometric, joined, min_cos)


@torch.no_grad()
def planar_patches(mesh: ThermalMesh, max_angle_degrees: float = 10.0, *, half_edges: Optional[MeshHalfEdges] = None,
                   min_area: float = 0.0, top: Optional[int] = None) -> MeshPatches:
    """The planar patches of ``mesh``: faces that share an edge are one patch while the angle between their normals is at most
    ``max_angle_degrees`` (0 .. 180; the cosine is taken here, in fp64).  ``half_edges``: the table of ``mesh_half_edges`` for this
    mesh, built when absent.  Patches below ``min_area`` (in the mesh's units squared) are dropped; the rest come largest first, ties
    by ascending label, cut to ``top`` (``order_regions``' rule).  Two host reads: the counts with the two areas, then the Q rows
    (and the one of ``mesh_half_edges`` when it is built here)."""
    require_triangles(mesh)
    return _patches(mesh, _cos_of_degrees(max_angle_degrees), half_edges, min_area, top)


@torch.no_grad()
def edge_components(mesh: ThermalMesh, half_edges: Optional[MeshHalfEdges] = None) -> MeshPatches:
    """The edge-connected components of ``mesh``: faces that share an edge (``mesh_components`` joins those that share a vertex).
    The same call with ``min_cos = -1``: every row carries the component's area, vector-area plane and temperatures."""
    require_triangles(mesh)
    return _patches(mesh, -1.0, half_edges, 0.0, None)


def _kept(patches: MeshPatches, k: int) -> int:
    k = int(k)
    if k < 0 or k >= len(patches):
        raise IndexError(f"kept patch {k} of {len(patches)}")
    return k


@torch.no_grad()
def patch_view(mesh: ThermalMesh, patches: MeshPatches, k: int, *, up: Optional[Sequence[float]] = None,
               pixel_size: Optional[float] = None, width: Optional[int] = None, margin_pixels: int = 2, cull: bool = True) -> RasterView:
    """The view that looks straight at kept patch ``k``: against its normal (forward = -normal), framing the patch's vertices (gathered
    through ``face_patch``) with ``fit_view``.  ``up`` defaults to world z, or to world y when the normal is within 1e-3 of +-z.
    ``mesh_thermogram(regions_mesh(mesh, patches.only(k)), view)`` is the wall's thermogram."""
    require_triangles(mesh)
    k = _kept(patches, k)
    row = patches.patches[k]
    normal = np.asarray(row["plane"][:3], dtype=np.float64)
    if not np.isfinite(normal).all() or not np.any(normal):
        raise ValueError(f"patch {k} has no plane (its vector area is zero): give a view by hand")
    if up is None:
        up = (0.0, 1.0, 0.0) if abs(abs(float(normal[2])) - 1.0) <= 1e-3 else (0.0, 0.0, 1.0)
    tri, face_patch = mesh.triangles, patches.face_patch
    if face_patch.shape[0] != tri.shape[0]:
        raise ValueError("the patches belong to another mesh: face_patch and triangles differ in length")
    vertices = torch.unique(tri[face_patch == int(patches.patch_index[k])].long().reshape(-1))
    return fit_view(mesh.positions[vertices], tuple(-normal), up, pixel_size=pixel_size, width=width, margin_pixels=margin_pixels,
                    cull=cull)
