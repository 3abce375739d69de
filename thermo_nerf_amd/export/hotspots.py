"""Thermal hot spots of a mesh — where are the anomalies, and how strong is each against its own surroundings: every local maximum
of the per-vertex temperature is a peak with a basin, the basins meet in saddles, and the topological persistence of the temperature
gives every peak its prominence in degrees Celsius: how far one has to descend from it before a hotter peak can be reached.  "All
hot spots that stand out by more than 1 degree" is one call with one physical parameter; cold spots (air leaks, wet patches, missing
insulation) are the same call with ``coldest=True``.

``tn_mesh_peaks`` ranks the vertices with the stable device sort, walks the corner lists of ``mesh_incidence`` to the steepest
neighbour, follows the ascent by pointer jumping and finds the saddle of every pair of adjacent basins; ``tn_basin_persistence`` merges
the basin graph on the host in integers; ``tn_mesh_spots`` gives every surviving spot its extent and the row of a thermal region.
include/thermonerf_hip.h and DESIGN.md "Thermal hot spots" define every output to the bit.  There is no CPU path for the device parts.

    spots = thermal_hotspots(mesh, min_prominence=1.0, smooth_iterations=3)
    regions_mesh(mesh, spots)                  # the faces of the spots as a mesh
    mesh_thermogram(mesh, view).region_map(spots)
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import check_incidence, mesh_arrays, require_triangles, workspace_of
from .gradient import smooth_temperature
from .mesh import ThermalMesh
from .smooth import MeshIncidence, mesh_incidence

# a row of the saddle table: tn_mesh_saddle (16 bytes); a row of the spot table: tn_mesh_spot (80 bytes, no padding)
SADDLE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("pass_vertex", "<i4"), ("pass_rank", "<i4")])
SPOT_DTYPE = np.dtype([("area", "<f8"), ("label", "<i4"), ("faces", "<i4"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                       ("max_temperature", "<f4"), ("centroid", "<f4", (3,)), ("bounds", "<f4", (6,)), ("coldest_vertex", "<i4"),
                       ("hottest_vertex", "<i4"), ("vertices", "<i4"), ("reserved", "<i4")])
SPOT_BYTES = SPOT_DTYPE.itemsize
NEVER = 2 ** 31 - 1  # the limit of a spot that never dies: above every rank


@dataclasses.dataclass
class MeshPeaks:
    """what ``mesh_peaks`` found, on the device"""

    rank: Tensor            # int32 [V]: the position of every vertex in the order, 0 the top
    vertex_basin: Tensor    # int32 [V]: the basin of every finite vertex, -1 of every other
    basin_peak: Tensor      # int32 [B]: the peak vertex of every basin, ascending
    saddles: Tensor         # int32 [S, 4]: (a, b, pass_vertex, pass_rank) per adjacent pair of basins, ascending (a, b)
    finite_vertices: int
    coldest: bool

    @property
    def num_basins(self) -> int:
        return int(self.basin_peak.shape[0])

    @property
    def num_saddles(self) -> int:
        return int(self.saddles.shape[0])


@dataclasses.dataclass
class BasinPersistence:
    """what ``basin_persistence`` computed, on the host"""

    basin_peak: np.ndarray         # int32 [B]
    basin_rank: np.ndarray         # int32 [B]: the rank of the peak
    peak_temperature: np.ndarray   # float32 [B]
    saddles: np.ndarray            # SADDLE_DTYPE [S]
    saddle_temperature: np.ndarray  # float32 [S]: the temperature of every row's pass vertex
    death_saddle: np.ndarray       # int32 [B]: the row by which the basin dies, -1 of the maximum of a component
    parent: np.ndarray             # int32 [B]: the eldest basin of what it died into, -1 likewise
    prominence: np.ndarray         # float32 [B]: degrees Celsius, +inf where it never dies


@dataclasses.dataclass
class ThermalHotspots:
    """what ``thermal_hotspots`` found: per kept spot (in descending prominence, ties by ascending peak rank) the arrays below, on the
    host; ``vertex_spot`` / ``face_spot`` on the device name ALL K spots, kept or not, by their number k"""

    peak_vertex: np.ndarray         # int32 [N]
    peak_position: np.ndarray       # float32 [N, 3]
    peak_temperature: np.ndarray    # float32 [N] degrees Celsius (of the smoothed field with ``smooth_iterations``)
    prominence: np.ndarray          # float32 [N] degrees Celsius, +inf for the maximum of a component
    saddle_vertex: np.ndarray       # int32 [N]: where the spot joins a stronger one, -1 for the maximum of a component
    saddle_temperature: np.ndarray  # float32 [N], NaN likewise
    basins: np.ndarray              # int64 [N]: the basins merged into the spot, its own included
    is_maximum: np.ndarray          # bool [N]: the spot is its component's maximum (minimum for ``coldest``)
    spots: np.ndarray               # SPOT_DTYPE [N]: area, faces, mean temperature, centroid, extremes, bounds, vertices
    spot_index: np.ndarray          # int64 [N]: the number k of every kept spot
    vertex_spot: Tensor             # int32 [V] on the device: k of a vertex in the extent of spot k, -1 of every other
    face_spot: Tensor               # int32 [T] on the device: k of a usable face whose three vertices lie in one extent, -1 otherwise
    num_basins: int                 # B
    num_saddles: int                # S
    num_spots: int                  # K: all spots, before ``min_area`` and ``top``
    min_prominence: float
    coldest: bool

    def __len__(self) -> int:
        return int(self.spot_index.shape[0])

    # what regions_mesh and Thermogram.region_map read of a ThermalRegions
    @property
    def face_region(self) -> Tensor:
        return self.face_spot

    @property
    def region_index(self) -> np.ndarray:
        return self.spot_index

    @property
    def num_regions(self) -> int:
        return self.num_spots


def mesh_peaks_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_peaks_workspace_bytes(int(num_vertices), int(num_triangles)))


def mesh_spots_workspace_bytes(num_vertices: int, num_triangles: int, num_spots: int) -> int:
    return int(_hip.load().tn_mesh_spots_workspace_bytes(int(num_vertices), int(num_triangles), int(num_spots)))


@torch.no_grad()
def mesh_peaks(mesh: ThermalMesh, incidence: Optional[MeshIncidence] = None, coldest: bool = False,
               workspace: Optional[Tensor] = None) -> MeshPeaks:
    """The peaks of ``mesh``'s temperature (the local minima with ``coldest``), the basin of every vertex and the saddle of every pair
    of adjacent basins through ``tn_mesh_peaks``.  ``incidence``: ``mesh_incidence(triangles, V)``, built if absent.  One host
    read: the three counts."""
    _, temp, tri, v, t = mesh_arrays(mesh)
    temp = temp.reshape(-1)
    dev = tri.device
    inc = mesh_incidence(tri, v) if incidence is None else check_incidence(incidence, tri, v, t)
    workspace, size = workspace_of(workspace, mesh_peaks_workspace_bytes(v, t) if v else 0, dev)
    with torch.cuda.device(dev):
        rank = torch.empty((v,), dtype=torch.int32, device=dev)
        vertex_basin = torch.empty((v,), dtype=torch.int32, device=dev)
        basin_peak = torch.empty((v,), dtype=torch.int32, device=dev)
        saddles = torch.empty((3 * t, 4), dtype=torch.int32, device=dev)
        counts = torch.empty((3,), dtype=torch.int64, device=dev)
        _hip.check(_hip.load().tn_mesh_peaks(
            temp.data_ptr() if v else None, tri.data_ptr() if t else None, t, v, inc.offsets.data_ptr(),
            inc.corners.data_ptr() if t else None, 1 if coldest else 0, rank.data_ptr() if v else None,
            vertex_basin.data_ptr() if v else None, basin_peak.data_ptr() if v else None, v, saddles.data_ptr() if t else None, 3 * t,
            counts.data_ptr(), workspace.data_ptr() if v else None, size, _hip.current_stream()), "tn_mesh_peaks")
        b, s, finite = (int(x) for x in counts.cpu().tolist())  # the one read
        return MeshPeaks(rank, vertex_basin, basin_peak[:b].clone(), saddles[:s].clone(), finite, bool(coldest))


def merge_basins(basin_rank: np.ndarray, saddles: np.ndarray):
    """(death_saddle, parent), int32 [B] each: ``tn_basin_persistence`` on host arrays — ``basin_rank`` int32 [B], ``saddles``
    SADDLE_DTYPE [S] or int32 [S, 4]"""
    basin_rank = np.ascontiguousarray(basin_rank, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(saddles)
    if rows.dtype == SADDLE_DTYPE:
        rows = rows.view(np.int32).reshape(-1, 4)
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    b, s = len(basin_rank), len(rows)
    death, parent = np.empty(b, np.int32), np.empty(b, np.int32)
    _hip.check(_hip.load().tn_basin_persistence(basin_rank.ctypes.data if b else None, b, rows.ctypes.data if s else None, s,
                                                death.ctypes.data if b else None, parent.ctypes.data if b else None),
               "tn_basin_persistence")
    return death, parent


def prominence_of(peak_temperature: np.ndarray, saddle_temperature: np.ndarray, death_saddle: np.ndarray, coldest: bool) -> np.ndarray:
    """float32 [B]: (float)((double)T[peak] - (double)T[pass vertex]) of the death saddle, the operands swapped for ``coldest``; +inf
    for a basin that never dies"""
    out = np.full(len(death_saddle), np.inf, np.float32)
    died = np.flatnonzero(death_saddle >= 0)
    top = peak_temperature[died].astype(np.float64)
    low = saddle_temperature[death_saddle[died]].astype(np.float64)
    out[died] = ((low - top) if coldest else (top - low)).astype(np.float32)
    return out


@torch.no_grad()
def basin_persistence(peaks: MeshPeaks, temperature: Tensor) -> BasinPersistence:
    """The persistence of ``peaks``' basins over ``temperature`` (float32 [V] on the device, the field the peaks were found on): which
    saddle every basin dies by, into which elder basin, and its prominence in degrees.  One read-back of the basin and saddle tables
    with the temperatures at the peaks and pass vertices; the merge itself runs on the host (``tn_basin_persistence``)."""
    temp = _hip.require_device_tensor(temperature, "temperature").reshape(-1)
    if temp.shape[0] != peaks.rank.shape[0] or temp.device != peaks.rank.device:
        raise ValueError("temperature must hold V values on the device of the peaks")
    peak_index = peaks.basin_peak.long()
    pass_index = peaks.saddles[:, 2].long()
    basin_peak = peaks.basin_peak.cpu().numpy()
    basin_rank = peaks.rank[peak_index].cpu().numpy()
    peak_temperature = temp[peak_index].cpu().numpy()
    rows = np.ascontiguousarray(peaks.saddles.cpu().numpy()).view(SADDLE_DTYPE).reshape(-1)
    saddle_temperature = temp[pass_index].cpu().numpy()
    death, parent = merge_basins(basin_rank, rows)
    return BasinPersistence(basin_peak, basin_rank, peak_temperature, rows, saddle_temperature, death, parent,
                            prominence_of(peak_temperature, saddle_temperature, death, peaks.coldest))


def choose_spots(persistence: BasinPersistence, min_prominence: float):
    """(basin_spot int32 [B], spot_basin int64 [K]): the basins that survive ``min_prominence`` (strictly above it) as spots in
    descending prominence, ties by ascending peak rank; every other basin joins the first survivor on its parent chain"""
    prominence, parent = persistence.prominence, persistence.parent
    b = len(prominence)
    survive = prominence.astype(np.float64) > float(min_prominence)
    spot_basin = np.flatnonzero(survive)
    spot_basin = spot_basin[np.lexsort((persistence.basin_rank[spot_basin], -prominence[spot_basin].astype(np.float64)))]
    basin_spot = np.full(b, -1, np.int32)
    if len(spot_basin) == 0:
        return basin_spot, spot_basin.astype(np.int64)
    # a basin that does not survive has died: its parent exists, and a parent's prominence is never smaller: the chain ends
    target = np.where(survive, np.arange(b), parent).astype(np.int64)
    while True:
        following = target[target]
        if np.array_equal(following, target):
            break
        target = following
    number = np.full(b, -1, np.int32)
    number[spot_basin] = np.arange(len(spot_basin), dtype=np.int32)
    return number[target], spot_basin.astype(np.int64)


def spot_bounds(peak_temperature: np.ndarray, extent_drop: float, coldest: bool) -> np.ndarray:
    """float32: what a vertex of the extent reaches — (float)(T[peak] - extent_drop), or + for ``coldest``, in fp64"""
    top = np.asarray(peak_temperature, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return ((top + float(extent_drop)) if coldest else (top - float(extent_drop))).astype(np.float32)


@torch.no_grad()
def mesh_spots(mesh: ThermalMesh, peaks: MeshPeaks, basin_spot: np.ndarray, spot_peak: np.ndarray, spot_limit: np.ndarray,
               spot_bound: np.ndarray, workspace: Optional[Tensor] = None):
    """``tn_mesh_spots`` on the current stream: (vertex_spot int32 [V], face_spot int32 [T], the rows as a uint8 tensor of
    ``SPOT_BYTES`` per spot, counts int64 [3]), all on the device; no host read"""
    pos, temp, tri, v, t = mesh_arrays(mesh)
    temp = temp.reshape(-1)
    dev = pos.device
    basin_spot = np.ascontiguousarray(basin_spot, dtype=np.int32).reshape(-1)
    spot_peak = np.ascontiguousarray(spot_peak, dtype=np.int32).reshape(-1)
    spot_limit = np.ascontiguousarray(spot_limit, dtype=np.int32).reshape(-1)
    spot_bound = np.ascontiguousarray(spot_bound, dtype=np.float32).reshape(-1)
    b, k = len(basin_spot), len(spot_peak)
    if peaks.rank.shape[0] != v or peaks.vertex_basin.shape[0] != v or b != peaks.num_basins:
        raise ValueError("the peaks belong to another mesh: the vertex or basin counts differ")
    if len(spot_limit) != k or len(spot_bound) != k or k > b:
        raise ValueError("spot_peak, spot_limit and spot_bound hold one entry per spot, and at most one spot per basin")
    workspace, size = workspace_of(workspace, mesh_spots_workspace_bytes(v, t, k) if v else 0, dev)
    with torch.cuda.device(dev):
        up = [torch.from_numpy(a).to(dev) for a in (basin_spot, spot_peak, spot_limit, spot_bound)]
        vertex_spot = torch.empty((v,), dtype=torch.int32, device=dev)
        face_spot = torch.empty((t,), dtype=torch.int32, device=dev)
        rows = torch.empty((k * SPOT_BYTES,), dtype=torch.uint8, device=dev)
        counts = torch.empty((3,), dtype=torch.int64, device=dev)
        _hip.check(_hip.load().tn_mesh_spots(
            pos.data_ptr() if v else None, temp.data_ptr() if v else None, tri.data_ptr() if t else None, v, t,
            peaks.rank.data_ptr() if v else None, peaks.vertex_basin.data_ptr() if v else None, up[0].data_ptr() if b else None, b,
            up[1].data_ptr() if k else None, up[2].data_ptr() if k else None, up[3].data_ptr() if k else None, k,
            1 if peaks.coldest else 0, vertex_spot.data_ptr() if v else None, face_spot.data_ptr() if t else None,
            rows.data_ptr() if k else None, counts.data_ptr(), workspace.data_ptr() if v else None, size, _hip.current_stream()),
            "tn_mesh_spots")
    return vertex_spot, face_spot, rows, counts


def _parameters(min_prominence, extent_drop, smooth_iterations, min_area, top):
    min_prominence, extent_drop, min_area = float(min_prominence), float(extent_drop), float(min_area)
    if math.isnan(min_prominence) or min_prominence < 0.0:
        raise ValueError(f"min_prominence must be a number >= 0, got {min_prominence}")
    if math.isnan(extent_drop) or extent_drop < 0.0:
        raise ValueError(f"extent_drop must be a number >= 0 (inf: no limit), got {extent_drop}")
    if int(smooth_iterations) < 0:
        raise ValueError("smooth_iterations must not be negative")
    if math.isnan(min_area) or min_area < 0.0:
        raise ValueError(f"min_area must be a number >= 0, got {min_area}")
    if top is not None and int(top) < 0:
        raise ValueError(f"top must be >= 0, got {top}")
    return min_prominence, extent_drop, int(smooth_iterations), min_area, None if top is None else int(top)


@torch.no_grad()
def thermal_hotspots(mesh: ThermalMesh, min_prominence: float, *, coldest: bool = False, extent_drop: float = math.inf,
                     smooth_iterations: int = 0, min_area: float = 0.0, top: Optional[int] = None) -> ThermalHotspots:
    """The hot spots of ``mesh`` (the cold spots with ``coldest``) that stand out from their surroundings by more than
    ``min_prominence`` degrees Celsius, strongest first.  A spot is a peak of the per-vertex temperature together with every weaker
    peak that merges into it below the threshold; its EXTENT is what lies strictly above the saddle where it joins a stronger spot —
    and, with a finite ``extent_drop``, within that many degrees of its peak (connectivity is not re-checked for that cut) —, and
    its row has the area, the area-weighted mean temperature and centroid, the extremes and the bounds of the faces inside the extent.
    ``min_prominence = 0`` keeps every peak that stands out at all: a plateau is then one spot.  The maximum of a connected component
    has no saddle and prominence +inf.  Spots below ``min_area`` (the mesh's units squared) are dropped, the rest cut to ``top``.

    ``smooth_iterations`` runs ``smooth_temperature`` first (the degrees of a surface-nets vertex are one voxel's noisy sample): the
    peaks are then those of the SMOOTHED field, and every temperature reported — peaks, saddles, prominences, the rows — is the
    smoothed one.  Host reads: the counts, the basin and saddle tables, the rows."""
    require_triangles(mesh)
    min_prominence, extent_drop, smooth_iterations, min_area, top = _parameters(min_prominence, extent_drop, smooth_iterations, min_area,
                                                                               top)
    if smooth_iterations:
        mesh = smooth_temperature(mesh, smooth_iterations)
    pos, temp, tri, v, t = mesh_arrays(mesh)
    peaks = mesh_peaks(mesh, coldest=coldest)
    p = basin_persistence(peaks, temp.reshape(-1))
    basin_spot, spot_basin = choose_spots(p, min_prominence)
    k = len(spot_basin)
    death = p.death_saddle[spot_basin]
    dies = death >= 0
    limit = np.full(k, NEVER, np.int32)
    limit[dies] = p.saddles["pass_rank"][death[dies]]
    saddle_vertex = np.full(k, -1, np.int32)
    saddle_vertex[dies] = p.saddles["pass_vertex"][death[dies]]
    saddle_temperature = np.full(k, np.nan, np.float32)
    saddle_temperature[dies] = p.saddle_temperature[death[dies]]
    peak_vertex, peak_temperature = p.basin_peak[spot_basin], p.peak_temperature[spot_basin]
    vertex_spot, face_spot, rows, _ = mesh_spots(mesh, peaks, basin_spot, peak_vertex, limit,
                                                 spot_bounds(peak_temperature, extent_drop, coldest))
    table = np.frombuffer(rows.cpu().numpy().tobytes(), dtype=SPOT_DTYPE) if k else np.zeros(0, SPOT_DTYPE)
    keep = np.flatnonzero(np.asarray(table["area"], np.float64) >= min_area)
    keep = (keep if top is None else keep[:top]).astype(np.int64)
    positions = pos[torch.from_numpy(peak_vertex[keep].astype(np.int64)).to(pos.device)].cpu().numpy() if len(keep) else np.zeros((0, 3), np.float32)
    merged = np.bincount(basin_spot[basin_spot >= 0], minlength=k).astype(np.int64)
    return ThermalHotspots(peak_vertex[keep].copy(), positions, peak_temperature[keep].copy(), p.prominence[spot_basin][keep].copy(),
                           saddle_vertex[keep], saddle_temperature[keep], merged[keep], ~dies[keep], table[keep].copy(), keep, vertex_spot,
                           face_spot, peaks.num_basins, peaks.num_saddles, k, min_prominence, bool(coldest))
