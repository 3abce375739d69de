"""Level-set curves of a mesh — draw the 18 degree line on this wall, cut the model at z = 1.2 m and give me degrees along the cut:
the level set of a per-vertex scalar (the temperature itself for isotherms, the signed distance to a plane for sections) chained into
ordered polylines with arc length, the temperature along them and per curve its length, mean temperature and extremes.  The curves
are chained through the half-edge twins of the mesh, which also say whether it is closed, manifold and consistently oriented.

``tn_mesh_half_edges`` and ``tn_mesh_isolines`` do all of it on the device (the stable device sort, count / scan / emit, list ranking
by pointer jumping, one wave per curve for the ordered sums); include/thermonerf_hip.h and DESIGN.md "Level-set curves" define every
output to the bit.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import mesh_arrays, out_tensor, require_triangles, triangle_array, workspace_of
from .mesh import ThermalMesh

# a row of the curve table: tn_mesh_curve, field for field (40 bytes, no padding)
CURVE_DTYPE = np.dtype([("length", "<f8"), ("level", "<i4"), ("first_point", "<i4"), ("points", "<i4"), ("closed", "<i4"),
                        ("mean_temperature", "<f4"), ("min_temperature", "<f4"), ("max_temperature", "<f4"), ("first_face", "<i4")])
CURVE_BYTES = CURVE_DTYPE.itemsize
MAX_LEVELS = 256  # of one call of the kernel; the public functions split longer lists


class MeshHalfEdges(NamedTuple):
    """what ``mesh_half_edges`` found"""

    twin: Tensor             # int32 [3T] on the device: the other half-edge across the edge, -1 without one
    edges: int
    boundary_edges: int      # edges with one face
    nonmanifold_edges: int   # edges with three or more faces
    inconsistent_edges: int  # edges whose two faces run the same way along them

    @property
    def closed_manifold(self) -> bool:
        """every edge has exactly two faces, and they agree on the orientation"""
        return self.boundary_edges == 0 and self.nonmanifold_edges == 0 and self.inconsistent_edges == 0


def mesh_half_edges_workspace_bytes(num_vertices: int, num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_half_edges_workspace_bytes(int(num_vertices), int(num_triangles)))


def mesh_isolines_workspace_bytes(num_vertices: int, num_triangles: int, capacity_segments: int) -> int:
    return int(_hip.load().tn_mesh_isolines_workspace_bytes(int(num_vertices), int(num_triangles), int(capacity_segments)))


@torch.no_grad()
def mesh_half_edges(triangles: Tensor, num_vertices: int, workspace: Optional[Tensor] = None) -> MeshHalfEdges:
    """The half-edge twins of ``triangles`` (int32 [T, 3] on the device) over ``num_vertices`` vertices, and the numbers of edges,
    boundary edges, non-manifold edges and edges of inconsistent orientation.  One host read."""
    tri = triangle_array(triangles)
    v, t = int(num_vertices), int(tri.shape[0])
    if v < 0 or v > 2 ** 31 - 1:
        raise ValueError("num_vertices must be within 0 .. 2^31 - 1")
    dev = tri.device
    workspace, size = workspace_of(workspace, mesh_half_edges_workspace_bytes(v, t) if t else 0, dev)
    with torch.cuda.device(dev):
        twin = torch.empty((3 * t,), dtype=torch.int32, device=dev)
        counts = torch.empty((4,), dtype=torch.int64, device=dev)
        _hip.check(_hip.load().tn_mesh_half_edges(tri.data_ptr() if t else None, t, v, twin.data_ptr() if t else None, counts.data_ptr(),
                                                  workspace.data_ptr() if t else None, size, _hip.current_stream()), "tn_mesh_half_edges")
        edges, boundary, nonmanifold, inconsistent = (int(c) for c in counts.cpu().tolist())  # the one read
    return MeshHalfEdges(twin, edges, boundary, nonmanifold, inconsistent)


def check_levels(levels) -> Tuple[float, ...]:
    """the levels as floats: at least one, finite, strictly ascending"""
    values = tuple(float(x) for x in np.asarray(levels, dtype=np.float64).reshape(-1))
    if not values:
        raise ValueError("at least one level is needed")
    if not all(math.isfinite(x) for x in values):
        raise ValueError("the levels must be finite")
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError("the levels must be strictly ascending")
    return values


def _isoline_params(levels: Sequence[float], plane_normal) -> _hip.tn_isoline_params:
    params = _hip.tn_isoline_params()
    params.num_levels = len(levels)
    for k, x in enumerate(levels):
        params.levels[k] = x
    if plane_normal is not None:
        for a in range(3):
            params.normal[a] = float(plane_normal[a])
    return params


def mesh_isolines_into(mesh: ThermalMesh, twin: Tensor, levels, *, counts: Tensor, scalar: Optional[Tensor] = None, plane_normal=None,
                       positions: Optional[Tensor] = None, temperature: Optional[Tensor] = None, arc: Optional[Tensor] = None,
                       face: Optional[Tensor] = None, curves: Optional[Tensor] = None, capacity_segments: int = 0,
                       workspace: Optional[Tensor] = None) -> None:
    """``tn_mesh_isolines`` on the current stream, without a host synchronisation: the curves of at most 256 ``levels`` of ``scalar``
    (a device float [V] tensor) or of the signed distance along ``plane_normal`` (three numbers, taken as given), chained through
    ``twin`` (int32 [3T], as ``mesh_half_edges`` returns it).  ``counts``: five device int64, OVERWRITTEN with the segments S, the
    curves, the points, the closed curves and the usable faces.  ``capacity_segments`` = 0 is the sizing call: nothing but ``counts`` is
    written; otherwise ``positions`` float32 [2 C, 3], ``temperature`` float32 [2 C], ``arc`` float64 [2 C], ``face`` int32 [2 C] and
    ``curves``, a uint8 tensor of ``CURVE_BYTES`` per row and C rows, are required, and are written only when S <= C.
    ``workspace``: ``mesh_isolines_workspace_bytes(V, T, C)`` device bytes (allocated if absent)."""
    require_triangles(mesh)
    values = check_levels(levels)
    if len(values) > MAX_LEVELS:
        raise ValueError(f"one call takes at most {MAX_LEVELS} levels")
    if (scalar is None) == (plane_normal is None):
        raise ValueError("exactly one of scalar and plane_normal must be given")
    p, t, tri, v, n = mesh_arrays(mesh)
    if plane_normal is not None:
        normal = tuple(float(x) for x in np.asarray(plane_normal, dtype=np.float64).reshape(-1))
        if len(normal) != 3 or not all(math.isfinite(x) for x in normal) or not any(normal):
            raise ValueError("plane_normal must be three finite numbers, not all zero")
    else:
        normal = None
        scalar = _hip.require_device_tensor(scalar, "scalar")
        if scalar.numel() != v or scalar.device != p.device:
            raise ValueError("scalar must hold V values on the mesh's device")
    twin = _hip.require_device_tensor(twin, "twin", torch.int32)
    if twin.numel() != 3 * n or twin.device != p.device:
        raise ValueError("twin must hold 3 T values on the mesh's device")
    cap = int(capacity_segments)
    if cap < 0 or cap > 2 ** 30:
        raise ValueError("capacity_segments must be within 0 .. 2^30")
    counts = out_tensor(counts, "counts", torch.int64, 5, 1)
    if counts is None:
        raise ValueError("counts are required")
    positions = out_tensor(positions, "positions", torch.float32, 2 * cap, 3)
    temperature = out_tensor(temperature, "temperature", torch.float32, 2 * cap, 1)
    arc = out_tensor(arc, "arc", torch.float64, 2 * cap, 1)
    face = out_tensor(face, "face", torch.int32, 2 * cap, 1)
    curves = out_tensor(curves, "curves", torch.uint8, cap, CURVE_BYTES)
    if cap > 0 and any(x is None for x in (positions, temperature, arc, face, curves)):
        raise ValueError("positions, temperature, arc, face and curves are required when capacity_segments > 0")
    dev = p.device
    work = v > 0 and n > 0
    workspace, size = workspace_of(workspace, mesh_isolines_workspace_bytes(v, n, cap) if work else 0, dev)
    params = _isoline_params(values, normal)
    outputs = [_hip.ptr(x) if cap else None for x in (positions, temperature, arc, face, curves)]
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_isolines(
            p.data_ptr() if v else None, t.data_ptr() if v else None, tri.data_ptr() if n else None, v, n, twin.data_ptr() if n else None,
            None if scalar is None or not v else scalar.data_ptr(), params, *outputs, cap, counts.data_ptr(),
            workspace.data_ptr() if work else None, size, _hip.current_stream()), "tn_mesh_isolines")


@dataclasses.dataclass
class MeshCurves:
    """what ``mesh_isolines`` found: Q curves over P points"""

    curves: np.ndarray      # CURVE_DTYPE [Q] on the host; ``level`` indexes ``levels``
    positions: Tensor       # float32 [P, 3] on the device
    temperature: Tensor     # float32 [P]
    arc: Tensor             # float64 [P]: the length along the curve from its first point
    face: Tensor            # int32 [P]: the face of the segment that starts at the point
    levels: Tuple[float, ...]
    num_segments: int
    num_curves: int
    num_points: int
    closed_curves: int
    usable_faces: int

    def __len__(self) -> int:
        return int(self.curves.shape[0])

    def curve_points(self, q: int) -> slice:
        """the rows of curve ``q`` in the point arrays"""
        row = self.curves[q]
        return slice(int(row["first_point"]), int(row["first_point"]) + int(row["points"]))

    def profile(self, q: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(arc float64 [n], xyz float32 [n, 3], degrees float32 [n]) of curve ``q`` on the host"""
        rows = self.curve_points(q)
        return self.arc[rows].cpu().numpy(), self.positions[rows].cpu().numpy(), self.temperature[rows].cpu().numpy()


def _isolines_call(mesh: ThermalMesh, twin: Tensor, levels: Sequence[float], scalar: Optional[Tensor], normal):
    """one call of at most 256 levels: the sizing call, the read of S, exact buffers, the full call, the read of the counts and the
    Q rows"""
    p, _, _, v, t = mesh_arrays(mesh)
    dev = p.device
    counts = torch.empty((5,), dtype=torch.int64, device=dev)
    mesh_isolines_into(mesh, twin, levels, counts=counts, scalar=scalar, plane_normal=normal)
    sized = counts.cpu().tolist()
    s, usable = int(sized[0]), int(sized[4])
    positions = torch.empty((2 * s, 3), dtype=torch.float32, device=dev)
    temperature = torch.empty((2 * s,), dtype=torch.float32, device=dev)
    arc = torch.empty((2 * s,), dtype=torch.float64, device=dev)
    face = torch.empty((2 * s,), dtype=torch.int32, device=dev)
    rows = torch.empty((s * CURVE_BYTES,), dtype=torch.uint8, device=dev)
    if s == 0:
        return np.zeros(0, CURVE_DTYPE), positions, temperature, arc, face, (0, 0, 0, 0, usable)
    mesh_isolines_into(mesh, twin, levels, counts=counts, scalar=scalar, plane_normal=normal, positions=positions,
                       temperature=temperature, arc=arc, face=face, curves=rows, capacity_segments=s)
    s, q, points, closed, usable = (int(c) for c in counts.cpu().tolist())
    table = np.frombuffer(rows[:q * CURVE_BYTES].cpu().numpy().tobytes(), dtype=CURVE_DTYPE).copy()
    return table, positions[:points], temperature[:points], arc[:points], face[:points], (s, q, points, closed, usable)


@torch.no_grad()
def mesh_isolines(mesh: ThermalMesh, levels, *, scalar: Optional[Tensor] = None, plane_normal=None,
                  half_edges: Optional[MeshHalfEdges] = None) -> MeshCurves:
    """The curves on which a per-vertex scalar of ``mesh`` takes the values ``levels`` (finite, strictly ascending), as ordered
    polylines.  Exactly one of ``scalar`` (a device float [V] tensor) and ``plane_normal`` must be given; the normal is normalised in
    fp64 here, so the levels of a plane are distances in world units along it.  ``half_edges``: the table of ``mesh_half_edges`` for
    this mesh, built when absent.  More than 256 levels are taken in calls of 256 and joined."""
    require_triangles(mesh)
    values = check_levels(levels)
    if (scalar is None) == (plane_normal is None):
        raise ValueError("exactly one of scalar and plane_normal must be given")
    normal = None
    if plane_normal is not None:
        n = np.asarray(plane_normal, dtype=np.float64).reshape(-1)
        length = float(np.sqrt((n * n).sum())) if n.shape == (3,) and np.isfinite(n).all() else 0.0
        if not length > 0.0 or not math.isfinite(length):
            raise ValueError("plane_normal must be three finite numbers, not all zero")
        normal = tuple(float(x) for x in n / length)
    p, _, tri, v, _ = mesh_arrays(mesh)
    if half_edges is None:
        half_edges = mesh_half_edges(tri, v)
    parts = [_isolines_call(mesh, half_edges.twin, values[k:k + MAX_LEVELS], scalar, normal) for k in range(0, len(values), MAX_LEVELS)]
    tables, totals, first_level, first_point = [], [0, 0, 0, 0, 0], 0, 0
    for k, part in enumerate(parts):
        table = part[0]
        table["level"] += first_level
        table["first_point"] += first_point
        tables.append(table)
        first_level += len(values[k * MAX_LEVELS:(k + 1) * MAX_LEVELS])
        first_point += part[5][2]
        for a in range(4):
            totals[a] += part[5][a]
        totals[4] = part[5][4]
    join = (lambda a: parts[0][a]) if len(parts) == 1 else (lambda a: torch.cat([part[a] for part in parts]))
    return MeshCurves(np.concatenate(tables), join(1), join(2), join(3), join(4), values, *totals)


def isotherms(mesh: ThermalMesh, temperatures, half_edges: Optional[MeshHalfEdges] = None) -> MeshCurves:
    """the lines of ``mesh`` at ``temperatures`` degrees Celsius"""
    return mesh_isolines(mesh, temperatures, scalar=mesh.temperature, half_edges=half_edges)


def mesh_sections(mesh: ThermalMesh, normal, offsets, half_edges: Optional[MeshHalfEdges] = None) -> MeshCurves:
    """the cuts of ``mesh`` by the planes at ``offsets`` (world units from the origin) along ``normal``"""
    return mesh_isolines(mesh, offsets, plane_normal=normal, half_edges=half_edges)
