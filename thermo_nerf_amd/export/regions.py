"""Thermal regions of a mesh — where is it warmer than X (or colder than Y), how large is each such patch, how hot is it: the faces
whose temperature (the mean of their three vertices) lies in a window are joined into regions through shared vertices, and every
region gets its area, its area-weighted mean temperature and centroid, its extremes, its bounds and its hottest and coldest vertex.

``tn_mesh_regions`` does all of it on the device (a record per face, ``tn_mesh_components`` over the faces in the window, the stable
device sort, ordered fp64 sums in blocks of 256); include/thermonerf_hip.h and DESIGN.md "Thermal regions" define every output to the
bit.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import mesh_arrays, out_tensor, require_triangles, workspace_of
from .mesh import ThermalMesh

# a row of the region table: tn_mesh_region, field for field (72 bytes, no padding)
REGION_DTYPE = np.dtype([("area", "<f8"), ("label", "<i4"), ("faces", "<i4"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                         ("max_temperature", "<f4"), ("centroid", "<f4", (3,)), ("bounds", "<f4", (6,)), ("coldest_vertex", "<i4"),
                         ("hottest_vertex", "<i4")])
REGION_BYTES = REGION_DTYPE.itemsize


@dataclasses.dataclass
class ThermalRegions:
    """what ``thermal_regions`` found"""

    regions: np.ndarray         # REGION_DTYPE [K] on the host: the kept regions, largest area first
    region_index: np.ndarray    # int64 [K]: the number r of every kept region, as ``face_region`` names it
    face_region: Tensor         # int32 [T] on the device: r of every face in the window (kept or not), -1 of every other
    mesh_area: float            # the area of all usable faces
    selected_area: float        # the area of the faces in the window
    num_regions: int            # R: all regions, before ``min_area`` and ``top``
    selected_faces: int
    usable_faces: int
    window: Tuple[float, float]

    def __len__(self) -> int:
        return int(self.regions.shape[0])


def mesh_regions_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_regions_workspace_bytes(int(num_vertices), int(num_triangles)))


def max_regions(num_vertices: int, num_triangles: int) -> int:
    """the most regions a mesh can have: a region has a face, and three vertices of its own"""
    return min(int(num_vertices) // 3, int(num_triangles))


def _window(min_temperature: float, max_temperature: float) -> Tuple[float, float]:
    lo, hi = float(min_temperature), float(max_temperature)
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError("the temperature window must not be NaN")
    return lo, hi


def mesh_regions_into(mesh: ThermalMesh, min_temperature: float, max_temperature: float, *, counts: Tensor, totals: Tensor,
                      face_region: Optional[Tensor] = None, regions: Optional[Tensor] = None, face_area: Optional[Tensor] = None,
                      capacity_regions: Optional[int] = None, workspace: Optional[Tensor] = None) -> None:
    """``tn_mesh_regions`` on the current stream, without a host synchronisation: the faces of ``mesh`` whose temperature lies in
    [min_temperature, max_temperature] as regions.  ``counts``: three device int64, OVERWRITTEN with the full numbers of regions,
    selected faces and usable faces; ``totals``: two device float64, the mesh's area and the selected area; ``face_region``: int32
    [T] (required when the mesh has faces); ``regions``: a uint8 device tensor of ``REGION_BYTES`` per row, read on the host as
    ``REGION_DTYPE``; ``face_area``: float64 [T], optional.  ``capacity_regions`` defaults to the rows ``regions`` can hold (0
    without it: the sizing call).  ``workspace``: ``mesh_regions_workspace_bytes(V, T)`` device bytes (allocated if absent)."""
    require_triangles(mesh)
    lo, hi = _window(min_temperature, max_temperature)
    p, t, tri, v, n = mesh_arrays(mesh)
    if regions is not None and (not isinstance(regions, Tensor) or regions.dtype != torch.uint8):
        raise ValueError("regions must be a uint8 device tensor")
    cap = int(regions.numel() // REGION_BYTES if regions is not None else 0) if capacity_regions is None else int(capacity_regions)
    if cap < 0:
        raise ValueError("a capacity must not be negative")
    regions = out_tensor(regions, "regions", torch.uint8, cap, REGION_BYTES)
    face_region = out_tensor(face_region, "face_region", torch.int32, n, 1)
    face_area = out_tensor(face_area, "face_area", torch.float64, n, 1)
    counts = out_tensor(counts, "counts", torch.int64, 3, 1)
    totals = out_tensor(totals, "totals", torch.float64, 2, 1)
    if counts is None or totals is None:
        raise ValueError("counts and totals are required")
    if n > 0 and face_region is None:
        raise ValueError("face_region is required when the mesh has faces")
    if cap > 0 and regions is None:
        raise ValueError("regions are required when capacity_regions > 0")
    dev = p.device
    work = v > 0 and n > 0
    workspace, size = workspace_of(workspace, mesh_regions_workspace_bytes(v, n) if work else 0, dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_regions(
            p.data_ptr() if v else None, t.data_ptr() if v else None, tri.data_ptr() if n else None, v, n, lo, hi, _hip.ptr(regions),
            cap, _hip.ptr(face_region) if n else None, _hip.ptr(face_area) if n else None, counts.data_ptr(), totals.data_ptr(),
            workspace.data_ptr() if work else None, size, _hip.current_stream()), "tn_mesh_regions")


def order_regions(table: np.ndarray, min_area: float = 0.0, top: Optional[int] = None) -> np.ndarray:
    """the rows of a region table that ``thermal_regions`` keeps, in its order: zero-area regions and those below ``min_area`` go,
    the rest by area descending, ties by ascending label, cut to ``top``.  Returns row numbers (int64)."""
    min_area = float(min_area)
    if math.isnan(min_area) or min_area < 0.0:
        raise ValueError(f"min_area must be a number >= 0, got {min_area}")
    if top is not None and int(top) < 0:
        raise ValueError(f"top must be >= 0, got {top}")
    area = np.asarray(table["area"], dtype=np.float64)
    rows = np.flatnonzero((area > 0.0) & (area >= min_area))
    rows = rows[np.lexsort((table["label"][rows], -area[rows]))]
    return (rows if top is None else rows[:int(top)]).astype(np.int64)


@torch.no_grad()
def thermal_regions(mesh: ThermalMesh, min_temperature: float = -math.inf, max_temperature: float = math.inf, *, min_area: float = 0.0,
                    top: Optional[int] = None) -> ThermalRegions:
    """The regions of ``mesh`` whose faces are at least ``min_temperature`` and at most ``max_temperature`` warm (degrees Celsius;
    a face's temperature is the mean of its three vertices; faces that share a vertex are one region).  Regions of no area are
    dropped, so are those below ``min_area`` (in the mesh's units squared); the rest come largest first, ties by ascending label,
    cut to ``top``.  Two host reads: the counts with the two areas, then the R rows."""
    require_triangles(mesh)
    window = _window(min_temperature, max_temperature)
    order_regions(np.zeros(0, REGION_DTYPE), min_area, top)  # the refusals, before anything runs
    p, _, _, v, t = mesh_arrays(mesh)
    dev = p.device
    cap = max_regions(v, t)
    with torch.cuda.device(dev):
        head = torch.empty((5,), dtype=torch.int64, device=dev)  # the three counts and, behind them, the two areas
        rows = torch.empty((cap * REGION_BYTES,), dtype=torch.uint8, device=dev)
        face_region = torch.empty((t,), dtype=torch.int32, device=dev)
        mesh_regions_into(mesh, window[0], window[1], counts=head[:3], totals=head[3:].view(torch.float64), face_region=face_region,
                          regions=rows if cap else None, capacity_regions=cap)
        first = head.cpu().numpy()  # the one read of the counts and the areas
        r, selected, usable = (int(x) for x in first[:3])
        mesh_area, selected_area = (float(x) for x in first[3:].view(np.float64))
        table = np.frombuffer(rows[:r * REGION_BYTES].cpu().numpy().tobytes(), dtype=REGION_DTYPE) if r else np.zeros(0, REGION_DTYPE)
    keep = order_regions(table, min_area, top)
    return ThermalRegions(table[keep].copy(), keep, face_region, mesh_area, selected_area, r, selected, usable, window)


@torch.no_grad()
def regions_mesh(mesh: ThermalMesh, regions: ThermalRegions) -> ThermalMesh:
    """The faces of the kept regions as a mesh of their own: faces in face order, the vertices they name in ascending index, every
    attribute carried (normals too); ``write_mesh_ply`` writes it.  Torch indexing on the device."""
    require_triangles(mesh)
    tri, face_region = mesh.triangles, regions.face_region
    if face_region.shape[0] != tri.shape[0]:
        raise ValueError("the regions belong to another mesh: face_region and triangles differ in length")
    dev = tri.device
    kept = torch.zeros((regions.num_regions + 1,), dtype=torch.bool, device=dev)  # (the last slot takes the -1 of the other faces)
    if len(regions.region_index):
        kept[torch.from_numpy(np.ascontiguousarray(regions.region_index)).to(dev)] = True
    faces = tri[kept[face_region.long()]].long()
    used = torch.zeros((len(mesh),), dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    new_index = torch.cumsum(used, dim=0, dtype=torch.int64) - 1
    vertices = torch.nonzero(used).reshape(-1)
    return ThermalMesh(mesh.positions[vertices], mesh.colors[vertices], mesh.temperature[vertices],
                       None if mesh.thermal_colors is None else mesh.thermal_colors[vertices],
                       new_index[faces].to(torch.int32).reshape(-1, 3), mesh.temperature_bounds,
                       None if mesh.normals is None else mesh.normals[vertices])
