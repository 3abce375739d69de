"""Geodesic distance on a mesh — what the other mesh analyses cannot measure: how far a spot is from the window frame ALONG THE WALL
(the tape measure), which part of the surface lies within 0.5 m of a thermal bridge (a buffer around a region), and how the
temperature falls off with the distance from a hot spot (the decay profile, which tells a point leak from a line bridge).

``tn_mesh_geodesic`` solves the eikonal equation on the triangles by Jacobi rounds of the virtual-source update over the corner lists
of ``mesh_incidence``: first order, exact on a plane from a point, no unfolding of obtuse triangles.  ``tn_mesh_distance_bands`` sums
area and temperature per band of distance with the grouped ordered sum of the regions.  include/thermonerf_hip.h and DESIGN.md
"Geodesic distance" define every output to the bit.  There is no CPU path for the device parts.

    d = geodesic_distance(mesh, *seeds_of_regions(mesh, thermal_hotspots(mesh, 1.0)))
    thermal_regions(d.mesh, max_temperature=0.5)        # the surface within 0.5 units of the hot spots
    isotherms(d.mesh, [0.5, 1.0, 1.5])                  # the equidistant curves
    distance_profile(mesh, d, 0.1, 20)                  # area and mean degrees per 0.1 units of distance
    surface_distance(mesh, bvh, a, b)                   # the tape measure between two picked points
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import MAX_COUNT, check_incidence, mesh_arrays, query_points, require_triangles, tree_arrays, workspace_of
from .closest import check_max_distance, mesh_closest
from .mesh import ThermalMesh
from .smooth import MeshIncidence, mesh_incidence

# a row of the band table: tn_mesh_band (40 bytes, no padding)
BAND_DTYPE = np.dtype([("area", "<f8"), ("warm_area", "<f8"), ("mean_temperature", "<f4"), ("min_temperature", "<f4"),
                       ("max_temperature", "<f4"), ("faces", "<i4"), ("warm_faces", "<i4"), ("reserved", "<i4")])
BAND_BYTES = BAND_DTYPE.itemsize
MAX_BANDS = 4096
MAX_ROUNDS_PER_CALL = 4096  # tn_mesh_geodesic's limit
BATCH = 128                 # rounds queued between two reads of the counts


@dataclasses.dataclass
class MeshDistance:
    """what ``geodesic_distance`` computed"""

    distance: Tensor        # float64 [V] on the device: +inf where the seeds do not reach (another component, beyond max_distance)
    nearest_seed: Tensor    # int32 [V] on the device: the number i of the seed the distance comes from, -1 where unreached
    rounds: int             # the rounds that changed a vertex
    converged: bool         # a round changed nothing: the arrays are the fixed point
    reached: int            # the vertices with a finite distance
    num_seeds: int
    max_distance: float
    source: ThermalMesh     # the mesh the distances belong to

    @property
    def mesh(self) -> ThermalMesh:
        """the source mesh with float32(distance) as its temperature, NaN where unreached: ``thermal_regions``, ``isotherms``,
        ``mesh_thermogram`` and ``write_mesh_ply`` then read distances where they read degrees"""
        value = self.distance.to(torch.float32)
        value = torch.where(torch.isfinite(value), value, torch.full_like(value, math.nan)).reshape(self.source.temperature.shape)
        finite = value[value == value]
        top = float(finite.max()) if finite.numel() else 0.0
        return dataclasses.replace(self.source, temperature=value, thermal_colors=None, temperature_bounds=(0.0, top))


@dataclasses.dataclass
class DistanceProfile:
    """what ``distance_profile`` computed, on the host: per band k = [k width, (k + 1) width) of the faces' mean distance"""

    bands: np.ndarray            # BAND_DTYPE [K]: area, warm_area, mean / min / max temperature, faces, warm_faces
    centres: np.ndarray          # float64 [K]: (k + 0.5) width
    cumulative_area: np.ndarray  # float64 [K]: the area up to and including band k
    band_width: float
    cell: Optional[int]
    banded_faces: int            # the faces that fell into a band
    measured_faces: int          # the placed faces with three finite distances (of the cell), those beyond the last band included

    def __len__(self) -> int:
        return int(self.bands.shape[0])


def mesh_geodesic_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_geodesic_workspace_bytes(int(num_vertices), int(num_triangles)))


def mesh_distance_bands_workspace_bytes(num_vertices: int, num_triangles: int, bands: int) -> int:
    return int(_hip.load().tn_mesh_distance_bands_workspace_bytes(int(num_vertices), int(num_triangles), int(bands)))


def _seeds(seed_vertices, seed_offsets) -> Tuple[np.ndarray, np.ndarray]:
    """(int64 seeds, float64 offsets) after every check that needs no mesh"""
    if isinstance(seed_vertices, Tensor):
        seed_vertices = seed_vertices.detach().cpu().numpy()
    if isinstance(seed_offsets, Tensor):
        seed_offsets = seed_offsets.detach().cpu().numpy()
    seeds = np.asarray(seed_vertices)
    if seeds.dtype.kind not in "iu" and seeds.size:
        raise ValueError("seed_vertices must be integers")
    seeds = seeds.astype(np.int64).reshape(-1)
    if len(seeds) == 0 or len(seeds) > MAX_COUNT:
        raise ValueError("seed_vertices must name at least one vertex and at most 2^31 - 1")
    if (seeds < 0).any():
        raise ValueError("seed_vertices must not be negative")
    offsets = np.zeros(len(seeds), np.float64) if seed_offsets is None else np.asarray(seed_offsets, np.float64).reshape(-1)
    if len(offsets) != len(seeds):
        raise ValueError("seed_offsets must hold one value per seed")
    if not (np.isfinite(offsets) & (offsets >= 0.0)).all():
        raise ValueError("seed_offsets must be finite numbers >= 0")
    return seeds, np.ascontiguousarray(offsets)


@torch.no_grad()
def geodesic_distance(mesh: ThermalMesh, seed_vertices, seed_offsets=None, *, max_distance: float = math.inf,
                      max_rounds: Optional[int] = None, incidence: Optional[MeshIncidence] = None,
                      workspace: Optional[Tensor] = None) -> MeshDistance:
    """The distance along the surface of ``mesh`` from the seeds to every vertex: seed i is vertex ``seed_vertices[i]`` at distance
    ``seed_offsets[i]`` (0 if absent; finite, >= 0).  A vertex beyond ``max_distance`` stays unreached.  The rounds are queued in
    batches, the 16 bytes of the counts read between them, until a round changes nothing — or until ``max_rounds`` have run: then
    ``converged`` is False and the arrays are exactly that iterate.  ``incidence``: ``mesh_incidence(triangles, V)``, built if absent."""
    require_triangles(mesh)
    max_distance = float(max_distance)
    check_max_distance(max_distance)
    if max_rounds is not None and int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    seeds, offsets = _seeds(seed_vertices, seed_offsets)
    pos, _, tri, v, t = mesh_arrays(mesh)
    if (seeds >= v).any():
        raise ValueError(f"seed_vertices must lie in [0, {v})")
    seeds = np.ascontiguousarray(seeds.astype(np.int32))
    dev = pos.device
    inc = mesh_incidence(tri, v) if incidence is None else check_incidence(incidence, tri, v, t)
    workspace, size = workspace_of(workspace, mesh_geodesic_workspace_bytes(v, t), dev)
    lib = _hip.load()
    with torch.cuda.device(dev):
        seed_v, seed_o = torch.from_numpy(seeds).to(dev), torch.from_numpy(offsets).to(dev)
        distance = torch.empty((v,), dtype=torch.float64, device=dev)
        nearest = torch.empty((v,), dtype=torch.int32, device=dev)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)

        def call(restart: int, rounds: int) -> Tuple[int, bool]:
            _hip.check(lib.tn_mesh_geodesic(
                pos.data_ptr(), tri.data_ptr() if t else None, t, v, inc.offsets.data_ptr(), inc.corners.data_ptr() if t else None,
                seed_v.data_ptr(), seed_o.data_ptr(), len(seeds), max_distance, restart, rounds,
                distance.data_ptr(), nearest.data_ptr(), counts.data_ptr(), workspace.data_ptr(), size, _hip.current_stream()),
                "tn_mesh_geodesic")
            done, fixed = counts.cpu().tolist()  # the 16 bytes
            return int(done), bool(fixed)

        left = None if max_rounds is None else int(max_rounds)
        rounds, converged, restart = 0, False, 1
        while True:
            batch = BATCH if left is None else min(BATCH, left)
            rounds, converged = call(restart, batch)
            restart = 0
            if left is not None:
                left -= batch
            if converged or (left is not None and left <= 0):
                break
        reached = int(torch.isfinite(distance).sum())
    return MeshDistance(distance, nearest, rounds, converged, reached, len(seeds), max_distance, mesh)


def _faces_of_points(bvh, points: Tensor):
    """(the three vertices int64 [N, 3], their positions float64 [N, 3, 3], the closest points float64 [N, 3]) on the host"""
    pos, _, tri, _, t, dev, _ = tree_arrays(bvh)
    q = query_points(points, "N")
    if q.device != dev:
        raise ValueError("the points must be on the mesh's device")
    if q.shape[0] == 0:
        raise ValueError("points must hold at least one point")
    found = mesh_closest(bvh, q)
    face = found.closest_face.long()
    if t == 0 or bool((face < 0).any()):
        raise ValueError("a point has no closest face on the mesh")
    ids = tri[face].long()
    return ids.cpu().numpy(), pos[ids].double().cpu().numpy(), found.closest_point.double().cpu().numpy()


@torch.no_grad()
def seeds_at_points(bvh, points: Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """(seed_vertices int32 [3 N], seed_offsets float64 [3 N]) for ``geodesic_distance``: every picked point placed on the mesh of
    ``bvh`` by ``mesh_closest``, its face's three vertices seeded with their fp64 distances from the placed point — the distance
    from a point inside a face is then exact on a plane"""
    ids, corners, where = _faces_of_points(bvh, points)
    offsets = np.sqrt(((corners - where[:, None, :]) ** 2).sum(axis=2))
    return ids.reshape(-1).astype(np.int32), offsets.reshape(-1)


@torch.no_grad()
def seeds_of_regions(mesh: ThermalMesh, table, k: Optional[int] = None) -> Tuple[np.ndarray, None]:
    """(seed_vertices int32, None): the vertices of the faces of ``mesh`` with ``table.face_region == k`` (``k`` None: of every face
    that has a region), so that the distance is measured from the whole region.  ``table`` is a ``ThermalRegions``,
    ``ThermalHotspots`` or ``MeshPatches`` of that mesh; the mesh is an argument of its own because a table holds ``face_region``
    and no triangles."""
    require_triangles(mesh)
    if k is not None and int(k) < 0:
        raise ValueError(f"k must be >= 0, got {k}")
    face_region = getattr(table, "face_region", None)
    if not isinstance(face_region, Tensor):
        raise ValueError("the table has no face_region: give a ThermalRegions, ThermalHotspots or MeshPatches")
    _, _, tri, _, t = mesh_arrays(mesh, temperature=False)
    if face_region.numel() != t or face_region.device != tri.device:
        raise ValueError("the table belongs to another mesh: face_region and triangles differ in length or device")
    chosen = face_region.reshape(-1) >= 0 if k is None else face_region.reshape(-1) == int(k)
    return torch.unique(tri[chosen].reshape(-1)).cpu().numpy().astype(np.int32), None


def _dot(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _norm(x: np.ndarray) -> np.ndarray:
    return np.sqrt(_dot(x, x))


def _edge_candidates(pc, pa, pb, da, db) -> np.ndarray:
    """the smallest of the round's three candidates for a point c over the edge (a, b), in fp64 on the host in the header's order of
    operations; +inf without one"""
    with np.errstate(all="ignore"):
        ac, bc, ab = pc - pa, pc - pb, pb - pa
        best = np.fmin(da + _norm(ac), db + _norm(bc))
        u = _norm(ab)
        cr = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                       ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], axis=-1)
        cx, cy = _dot(ab, ac) / u, _norm(cr) / u
        a2 = da * da
        sx = ((u * u + a2) - db * db) / (2.0 * u)
        sy2 = a2 - sx * sx
        sy = np.sqrt(np.where(sy2 >= 0.0, sy2, 0.0))
        dx, h = cx - sx, cy + sy
        xs = sx + (dx * sy) / h
        ok = np.isfinite(da) & np.isfinite(db) & (u > 0.0) & (cy > 0.0) & (sy2 >= 0.0) & (xs > 0.0) & (xs < u)
        face = np.where(ok, np.sqrt(dx * dx + h * h), np.inf)
    return np.fmin(np.where(np.isnan(best), np.inf, best), face)


@torch.no_grad()
def distance_at_points(mesh: ThermalMesh, d: MeshDistance, bvh, points: Tensor) -> np.ndarray:
    """float64 [N] on the host — the tape measure's other end: every point placed on the mesh by ``mesh_closest``, its distance the
    smallest candidate of the solver's own update over the three edges of its face, with the placed point as the vertex c; +inf
    where none of the face's vertices was reached or the candidate lies beyond ``d.max_distance``"""
    _, _, _, v, _ = mesh_arrays(mesh, temperature=False)
    if bvh.num_vertices != v or d.distance.shape[0] != v:
        raise ValueError("the distances or the tree belong to another mesh: the vertex counts differ")
    ids, corners, where = _faces_of_points(bvh, points)
    dist = d.distance[torch.from_numpy(ids).to(d.distance.device)].cpu().numpy()
    best = np.full(len(ids), np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        best = np.fmin(best, _edge_candidates(where, corners[:, a], corners[:, b], dist[:, a], dist[:, b]))
    return np.where(best <= d.max_distance, best, np.inf)  # the solver's own rule: a candidate beyond the limit does not count


@torch.no_grad()
def surface_distance(mesh: ThermalMesh, bvh, a, b, max_distance: float = math.inf) -> float:
    """the distance along the surface between the picked points ``a`` and ``b`` (three coordinates each): ``seeds_at_points`` of a,
    ``geodesic_distance``, ``distance_at_points`` of b; +inf if b is not reached within ``max_distance``"""
    dev = _hip.require_device_tensor(mesh.positions, "positions").device
    pa = torch.as_tensor(np.asarray(a, np.float32).reshape(1, 3)).to(dev)
    pb = torch.as_tensor(np.asarray(b, np.float32).reshape(1, 3)).to(dev)
    d = geodesic_distance(mesh, *seeds_at_points(bvh, pa), max_distance=max_distance)
    return float(distance_at_points(mesh, d, bvh, pb)[0])


@torch.no_grad()
def distance_profile(mesh: ThermalMesh, d: MeshDistance, band_width: float, bands: int, cell: Optional[int] = None,
                     workspace: Optional[Tensor] = None) -> DistanceProfile:
    """The decay profile: area, mean / min / max degrees and face counts per band of ``band_width`` of distance, ``bands`` of them
    (1 .. 4096); a face belongs to the band of the mean of its three distances.  ``cell``: only the faces whose three vertices are
    nearest to seed ``cell``.  One host read: the rows and the counts."""
    band_width, bands = float(band_width), int(bands)
    if not (band_width > 0.0 and math.isfinite(band_width)):
        raise ValueError(f"band_width must be positive and finite, got {band_width}")
    if bands < 1 or bands > MAX_BANDS:
        raise ValueError(f"bands must lie in 1 .. {MAX_BANDS}, got {bands}")
    if cell is not None and int(cell) < 0:
        raise ValueError(f"cell must be >= 0, got {cell}")
    pos, temp, tri, v, t = mesh_arrays(mesh)
    dev = pos.device
    distance = _hip.require_device_tensor(d.distance, "distance", torch.float64)
    nearest = _hip.require_device_tensor(d.nearest_seed, "nearest_seed", torch.int32)
    if distance.numel() != v or nearest.numel() != v or distance.device != dev or nearest.device != dev:
        raise ValueError("the distances belong to another mesh: they must hold V values on the mesh's device")
    workspace, size = workspace_of(workspace, mesh_distance_bands_workspace_bytes(v, t, bands), dev)
    with torch.cuda.device(dev):
        rows = torch.empty((bands * BAND_BYTES,), dtype=torch.uint8, device=dev)
        counts = torch.empty((3,), dtype=torch.int64, device=dev)
        _hip.check(_hip.load().tn_mesh_distance_bands(
            pos.data_ptr() if v else None, temp.data_ptr() if v else None, tri.data_ptr() if t else None, v, t,
            distance.data_ptr() if v else None, nearest.data_ptr() if v else None, band_width, bands, -1 if cell is None else int(cell),
            rows.data_ptr(), counts.data_ptr(), workspace.data_ptr(), size, _hip.current_stream()), "tn_mesh_distance_bands")
        table = np.frombuffer(rows.cpu().numpy().tobytes(), dtype=BAND_DTYPE).copy()
        _, banded, measured = (int(x) for x in counts.cpu().tolist())
    centres = (np.arange(bands, dtype=np.float64) + 0.5) * band_width
    return DistanceProfile(table, centres, np.cumsum(table["area"]), band_width, None if cell is None else int(cell), banded, measured)
