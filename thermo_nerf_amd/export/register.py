"""Registration of two thermal meshes: this winter's survey into the frame of last winter's, so that ``mesh_difference`` and
``tools/mesh_compare.py`` — which need both in ONE frame — can compare them.  Two reconstructions of one building never share a
frame: each has its own origin, orientation and unit.  ``similarity_from_pairs`` gives the start from a few picked point pairs,
``register_points`` / ``register_mesh`` refine it by iterated closest points on the device, ``transform_mesh`` applies the result.

``tn_mesh_register`` walks the tree of ``build_mesh_bvh`` from the transformed points, leaves only the 36 sums of a damped
Gauss-Newton step and updates the transform on the device: a whole run is queued without a host read.  include/thermonerf_hip.h
and DESIGN.md "Registration" define every output to the bit, without reference to the tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import mesh_arrays, out_tensor, query_points, tree_arrays
from .closest import check_max_distance
from .mesh import ThermalMesh
from .raycast import MeshBVH

METRICS = {"point": _hip.TN_REGISTER_POINT, "plane": _hip.TN_REGISTER_PLANE}
MAX_ITERATIONS = 1024
DEFAULT_TOLERANCE = 1e-9   # of the rotation / scale update, and of the translation update over `length`
DEFAULT_DAMPING = 1e-6     # additive: see DESIGN.md "Registration"
DEFAULT_MIN_PAIRS = 6


def register_workspace_bytes(num_points: int) -> int:
    return int(_hip.load().tn_mesh_register_workspace_bytes(int(num_points)))


def check_register_params(max_distance: float, center, length: float, damping: float, tolerance: float, iterations: int, metric: str,
                          min_pairs: int) -> None:
    """what ``tn_mesh_register`` refuses of its parameters, with words"""
    check_max_distance(float(max_distance))
    if metric not in METRICS:
        raise ValueError(f"metric must be 'plane' or 'point', got {metric!r}")
    if len(center) != 3 or not all(math.isfinite(float(c)) for c in center):
        raise ValueError("center must be three finite numbers")
    if not (math.isfinite(length) and length > 0.0):
        raise ValueError(f"length must be a finite number > 0, got {length}")
    if not (math.isfinite(damping) and damping >= 0.0):
        raise ValueError(f"damping must be a finite number >= 0, got {damping}")
    if math.isnan(tolerance) or tolerance < 0.0:
        raise ValueError(f"tolerance must be a number >= 0, got {tolerance}")
    if not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be in 1 .. {MAX_ITERATIONS}, got {iterations}")
    if int(min_pairs) < 0:
        raise ValueError(f"min_pairs must be >= 0, got {min_pairs}")


def register_points_into(bvh: MeshBVH, points: Tensor, transform: Tensor, history: Tensor, result: Tensor, *, max_distance: float,
                         center: Sequence[float], length: float, metric: str = "plane", with_scale: bool = False, iterations: int = 30,
                         tolerance: float = DEFAULT_TOLERANCE, damping: float = DEFAULT_DAMPING, min_pairs: int = DEFAULT_MIN_PAIRS,
                         workspace: Optional[Tensor] = None) -> None:
    """``tn_mesh_register`` on the current stream, without a host synchronisation or a host read: ``iterations`` x (walk, finish) are
    queued.  ``transform`` float64 [12] (row-major 3 x 4, points -> the mesh's frame) is the start and becomes the result, ``history``
    float64 [iterations, 4] gets (matched points, sum of squared residuals, rotation / scale update, translation update / length) per
    iteration (-1 where none ran), ``result`` int64 [4] the status, the iterations run, the matched and the usable points of the
    last.  ``workspace``: uint8, at least ``register_workspace_bytes(N)``; allocated when absent."""
    check_register_params(max_distance, center, float(length), float(damping), float(tolerance), iterations, metric, min_pairs)
    p, t, tri, v, n, dev, blob = tree_arrays(bvh)
    q = query_points(points, "N")
    if q.device != dev:
        raise ValueError("the points must be on the mesh's device")
    count = int(q.shape[0])
    transform = out_tensor(transform, "transform", torch.float64, 12, 1)
    history = out_tensor(history, "history", torch.float64, int(iterations), 4)
    result = out_tensor(result, "result", torch.int64, 4, 1)
    need = register_workspace_bytes(count)
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        workspace = out_tensor(workspace, "workspace", torch.uint8, need, 1)
        params = _hip.tn_register_params(float(max_distance), (ctypes.c_double * 3)(*[float(c) for c in center]), float(length), float(damping),
                                         float(tolerance), int(iterations), METRICS[metric], 1 if with_scale else 0, int(min_pairs))
        work = v > 0 and n > 0
        _hip.check(_hip.load().tn_mesh_register(
            p.data_ptr() if work else None, t.data_ptr() if work else None, tri.data_ptr() if n else None, v, n, blob.data_ptr(),
            blob.numel() * blob.element_size(), q.data_ptr() if count else None, count, ctypes.byref(params), transform.data_ptr(),
            history.data_ptr(), result.data_ptr(), workspace.data_ptr(), workspace.numel(), _hip.current_stream()), "tn_mesh_register")


@dataclasses.dataclass
class Registration:
    """what ``register_points`` made.  ``matrix`` takes a point of the moving cloud into the mesh's frame."""

    matrix: np.ndarray            # float64 [4, 4]
    scale: float                  # the cube root of the linear part's determinant: 1 for a rigid motion
    status: str                   # "converged", "iterations", "too_few" or "degenerate" (of the last stage)
    iterations: int               # iterations run, all stages
    matched: int                  # points with a counterpart within max_distance in the last iteration
    matched_share: float          # of all points; 0.0 without points
    usable_points: int
    rms: List[float]              # per iteration run: the RMS residual (point to plane, or point to point) before its update
    stages: List[dict]            # per stage: max_distance, status, iterations, matched, matched_share, rms (the last iteration's)

    @property
    def converged(self) -> bool:
        return self.status == "converged"


def _as_matrix(initial) -> np.ndarray:
    if initial is None:
        return np.eye(4)
    m = np.array(initial.detach().cpu().numpy() if isinstance(initial, Tensor) else initial, dtype=np.float64)
    if m.shape == (3, 4):
        m = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    if m.shape != (4, 4) or not np.isfinite(m).all() or not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("initial must be a finite 3 x 4 or 4 x 4 matrix with the last row (0, 0, 0, 1)")
    return m


def _scale_of(matrix: np.ndarray) -> float:
    det = float(np.linalg.det(matrix[:3, :3]))
    return math.copysign(abs(det) ** (1.0 / 3.0), det)


@torch.no_grad()
def register_points(bvh: MeshBVH, points: Tensor, *, initial=None, max_distance: Union[float, Sequence[float]], metric: str = "plane",
                    with_scale: bool = False, iterations: int = 30, tolerance: float = DEFAULT_TOLERANCE, damping: float = DEFAULT_DAMPING,
                    min_pairs: int = DEFAULT_MIN_PAIRS, center: Optional[Sequence[float]] = None, length: Optional[float] = None
                    ) -> Registration:
    """Iterated closest points of ``points`` float32 [N, 3] against the mesh of ``bvh``, from ``initial`` (3 x 4 or 4 x 4, the
    identity when absent): every point is paired with the nearest point of the mesh within ``max_distance`` of where the current
    transform puts it, a damped Gauss-Newton step — point to plane, or point to point — moves the transform (rotation, translation
    and, ``with_scale``, a uniform scale), until an update is below ``tolerance`` or ``iterations`` are used.  ``max_distance`` may be
    a sequence: coarse-to-fine stages of ``iterations`` each, every one starting from the last result.  ``center`` and ``length``
    default to the centre and the diagonal of the tree's box.  One host read of the tree's header, then one per stage.  ICP needs a
    start near the answer: see ``similarity_from_pairs``."""
    radii = [float(r) for r in (max_distance if isinstance(max_distance, (list, tuple)) else [max_distance])]
    if not radii:
        raise ValueError("max_distance must be a number or a non-empty sequence of numbers")
    start = _as_matrix(initial)
    p, t, tri, v, n, dev, blob = tree_arrays(bvh)
    q = query_points(points, "N")
    count = int(q.shape[0])
    if center is None or length is None:
        box = bvh.tree()
        lo, hi = np.array(box["lo"], np.float64), np.array(box["hi"], np.float64)
        whole = bool(np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all())
        center = center if center is not None else (tuple((lo + hi) / 2) if whole else (0.0, 0.0, 0.0))
        diagonal = float(np.linalg.norm(hi - lo)) if whole else 0.0
        length = length if length is not None else (diagonal if diagonal > 0.0 else 1.0)
    for r in radii:
        check_register_params(r, center, float(length), float(damping), float(tolerance), iterations, metric, min_pairs)
    rms: List[float] = []
    stages: List[dict] = []
    total = 0
    with torch.cuda.device(dev):
        head = torch.zeros((16 + 4 * int(iterations),), dtype=torch.float64, device=dev)  # transform, result, history: one read
        head[:12] = torch.from_numpy(np.ascontiguousarray(start[:3].reshape(12))).to(dev)
        workspace = torch.empty((register_workspace_bytes(count),), dtype=torch.uint8, device=dev)
        for r in radii:
            register_points_into(bvh, q, head[:12], head[16:], head[12:16].view(torch.int64), max_distance=r, center=center, length=length,
                                 metric=metric, with_scale=with_scale, iterations=iterations, tolerance=tolerance, damping=damping,
                                 min_pairs=min_pairs, workspace=workspace)
            host = head.cpu().numpy()  # the stage's one read
            status, ran, matched, usable = (int(x) for x in host[12:16].view(np.int64))
            rows = host[16:].reshape(-1, 4)[:ran]
            stage_rms = [math.sqrt(float(e) / float(m)) if m > 0 else math.nan for m, e in rows[:, :2]]
            rms += stage_rms
            total += ran
            stages.append({"max_distance": r, "status": _hip.TN_REGISTER_STATUS[status], "iterations": ran, "matched": matched,
                           "matched_share": matched / count if count else 0.0, "rms": stage_rms[-1] if stage_rms else math.nan})
            if status in (2, 3):  # refused: a finer stage would start from nothing better
                break
    matrix = np.eye(4)
    matrix[:3] = host[:12].reshape(3, 4)
    last = stages[-1]
    return Registration(matrix, _scale_of(matrix), last["status"], total, last["matched"], last["matched_share"], usable, rms, stages)


@torch.no_grad()
def register_mesh(mesh: ThermalMesh, reference_bvh: MeshBVH, *, max_points: Optional[int] = None, **options) -> Registration:
    """``register_points`` of the vertices of ``mesh`` against the mesh of ``reference_bvh``; with ``max_points`` every s-th vertex,
    s = ceil(V / max_points).  The options are ``register_points``'s."""
    if max_points is not None and int(max_points) < 1:
        raise ValueError(f"max_points must be >= 1, got {max_points}")
    points = mesh_arrays(mesh, temperature=False)[0]
    if max_points is not None:
        stride = -(-int(points.shape[0]) // int(max_points))
        if stride > 1:
            points = points[::stride].contiguous()
    return register_points(reference_bvh, points, **options)


@torch.no_grad()
def transform_mesh(mesh: ThermalMesh, matrix) -> ThermalMesh:
    """``mesh`` under the 3 x 4 or 4 x 4 ``matrix``: the positions in fp64, rounded once to fp32; the normals turned by the linear part
    without its scale (its inverse transpose, normalised); colours, temperatures, triangles and bounds are the input's own tensors.
    A linear part that mirrors also reverses the triangles' orientation: it is refused."""
    m = _as_matrix(matrix)
    linear = m[:3, :3]
    if not np.linalg.det(linear) > 0.0:
        raise ValueError("the matrix's linear part must have a positive determinant")
    positions = mesh.positions
    if not isinstance(positions, Tensor) or positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError("positions must be [V, 3]")
    dev = positions.device
    a = torch.from_numpy(np.ascontiguousarray(linear.T)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(m[:3, 3])).to(dev)
    p = positions.double()
    moved = ((p[:, 0:1] * a[0] + p[:, 1:2] * a[1]) + p[:, 2:3] * a[2]) + b  # one written order, no library matmul
    normals = mesh.normals
    if normals is not None:
        turn = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(linear))).to(dev)  # n' = (A^-T) n: rows of (n A^-1)
        nd = normals.double()
        turned = (nd[:, 0:1] * turn[0] + nd[:, 1:2] * turn[1]) + nd[:, 2:3] * turn[2]
        norm = turned.norm(dim=1, keepdim=True)
        normals = torch.where(norm > 0, turned / torch.where(norm > 0, norm, torch.ones_like(norm)), turned).float()
    return ThermalMesh(moved.float(), mesh.colors, mesh.temperature, mesh.thermal_colors, mesh.triangles, mesh.temperature_bounds, normals)


def similarity_from_pairs(source, target, with_scale: bool = True) -> np.ndarray:
    """The least-squares similarity (Umeyama 1991) that takes the picked points ``source`` [K, 3] onto ``target`` [K, 3], K >= 3 and
    not collinear, as a 4 x 4 fp64 matrix, on the host: the start of a registration.  Without ``with_scale`` the best rigid motion."""
    src = np.array(source.detach().cpu().numpy() if isinstance(source, Tensor) else source, dtype=np.float64)
    dst = np.array(target.detach().cpu().numpy() if isinstance(target, Tensor) else target, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape or len(src) < 3:
        raise ValueError("source and target must both be [K, 3] with K >= 3")
    if not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError("the pairs must be finite")
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    xs, xd = src - ms, dst - md
    cov = xd.T @ xs / len(src)
    u, s, vt = np.linalg.svd(cov)
    if s[1] <= 1e-12 * max(s[0], 1e-300):
        raise ValueError("the picked points are collinear (or coincide): they do not fix a rotation")
    sign = np.ones(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        sign[2] = -1.0
    rotation = u @ np.diag(sign) @ vt
    variance = float((xs * xs).sum() / len(src))
    scale = float((s * sign).sum() / variance) if with_scale else 1.0
    out = np.eye(4)
    out[:3, :3] = scale * rotation
    out[:3, 3] = md - scale * rotation @ ms
    return out
