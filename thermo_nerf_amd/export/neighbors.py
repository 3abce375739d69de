"""Neighbourhoods of a thermal point cloud: the k nearest neighbours of every point (``tn_knn``, a grid search on the device whose
(distance, index) lists are defined bit for bit — include/thermonerf_hip.h, DESIGN.md "Point-cloud export"), and the two steps
nerfstudio's exporter takes through open3d on top of them: statistical outlier removal and normal estimation.  There is no CPU
path.
"""
from __future__ import annotations

import dataclasses
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import workspace_of
from .pointcloud import ThermalPointCloud

MAX_NEIGHBORS = 32  # tn_knn's largest k
MAX_GRID_RESOLUTION = 512


class Neighbors(NamedTuple):
    """``knn``'s outputs; the ones that were not asked for are None.  indices int32 [N,k] (-1: no neighbour), distances float32
    [N,k] — the SQUARED distances d2 (+inf: no neighbour), mean_distance float64 [N] (+inf without a full row)."""

    indices: Optional[Tensor]
    distances: Optional[Tensor]
    mean_distance: Optional[Tensor]


def knn_grid_resolution(num_points: int) -> int:
    """the grid resolution ``tn_knn`` chooses for ``num_points`` when it is given 0"""
    return int(_hip.load().tn_knn_grid_resolution(int(num_points)))


def knn_workspace_bytes(num_points: int, grid_resolution: int = 0) -> int:
    return int(_hip.load().tn_knn_workspace_bytes(int(num_points), int(grid_resolution)))


def _positions(positions: Tensor) -> Tensor:
    p = _hip.require_device_tensor(positions, "positions")
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("positions must be [N, 3]")
    if p.shape[0] > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 points")
    return p


def knn(positions: Tensor, k: int, *, grid_resolution: int = 0, indices: bool = True, distances: bool = True,
        mean_distance: bool = False, workspace: Optional[Tensor] = None) -> Neighbors:
    """The ``k`` nearest other finite points of every row of ``positions`` ([N,3] float32 on the device) through ``tn_knn``, on
    the current stream, without a host synchronisation.  Rows are in ascending (d2, index) order, ties to the lower index; a
    non-finite point has an empty row and is in nobody's.  ``grid_resolution``: 0 (the library chooses) or 1 .. 512 — the
    outputs do not depend on it.  ``workspace``: ``knn_workspace_bytes(N, grid_resolution)`` device bytes (allocated if absent)."""
    p = _positions(positions)
    n, k, res = int(p.shape[0]), int(k), int(grid_resolution)
    if not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"k must be 1 .. {MAX_NEIGHBORS}")
    if not 0 <= res <= MAX_GRID_RESOLUTION:
        raise ValueError(f"grid_resolution must be 0 .. {MAX_GRID_RESOLUTION}")
    dev = p.device
    with torch.cuda.device(dev):
        idx = torch.empty((n, k), dtype=torch.int32, device=dev) if indices else None
        d2 = torch.empty((n, k), dtype=torch.float32, device=dev) if distances else None
        mean = torch.empty((n,), dtype=torch.float64, device=dev) if mean_distance else None
        if n == 0:
            return Neighbors(idx, d2, mean)
        workspace, workspace_size = workspace_of(workspace, knn_workspace_bytes(n, res), dev)
        _hip.check(_hip.load().tn_knn(p.data_ptr(), n, k, res, _hip.ptr(idx), _hip.ptr(d2), _hip.ptr(mean), workspace.data_ptr(),
                                      workspace_size, _hip.current_stream()), "tn_knn")
    return Neighbors(idx, d2, mean)


def pointcloud_normals(positions: Tensor, neighbor_index: Tensor, viewpoints: Optional[Tensor] = None) -> Tensor:
    """float32 [N,3]: ``tn_pointcloud_normals`` on the current stream — the unit eigenvector of the smallest eigenvalue of the
    fp64 covariance of a point and its valid neighbours (``neighbor_index`` int32 [N,k], a row of ``knn``), turned towards
    ``viewpoints`` [N,3] where one is given and finite; (0,0,0) for a non-finite point or fewer than 2 neighbours."""
    p = _positions(positions)
    n = int(p.shape[0])
    idx = _hip.require_device_tensor(neighbor_index, "neighbor_index", torch.int32)
    if idx.dim() != 2 or idx.shape[0] != n or not 1 <= idx.shape[1] <= MAX_NEIGHBORS:
        raise ValueError(f"neighbor_index must be [N, k] with k in 1 .. {MAX_NEIGHBORS}")
    v = None
    if viewpoints is not None:
        v = _hip.require_device_tensor(viewpoints, "viewpoints")
        if tuple(v.shape) != (n, 3):
            raise ValueError("viewpoints must be [N, 3]")
    with torch.cuda.device(p.device):
        out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
        if n:
            _hip.check(_hip.load().tn_pointcloud_normals(p.data_ptr(), idx.data_ptr(), n, int(idx.shape[1]), _hip.ptr(v),
                                                         out.data_ptr(), _hip.current_stream()), "tn_pointcloud_normals")
    return out


def outlier_keep_mask(mean_distance: Tensor, std_ratio: float) -> Tensor:
    """bool [N]: ``m_i < mu + std_ratio * sigma`` with mu and sigma (the n - 1 form) over the finite ``m_i`` — fp64 reductions on
    the tensor's device.  No finite ``m_i`` at all (fewer points than a row needs): every point with a finite position had
    ``m_i = +inf`` too, so the caller decides; here everything is dropped."""
    m = mean_distance.double()
    finite = torch.isfinite(m)
    count = finite.sum()
    mu = torch.where(finite, m, torch.zeros_like(m)).sum() / count
    dev = torch.where(finite, m - mu, torch.zeros_like(m))
    sigma = torch.sqrt((dev * dev).sum() / (count - 1))
    tau = mu + float(std_ratio) * torch.where(count > 1, sigma, torch.zeros_like(sigma))
    return m < tau


def remove_statistical_outliers(cloud: ThermalPointCloud, nb_neighbors: int = 20, std_ratio: float = 10.0
                                ) -> Tuple[ThermalPointCloud, Tensor]:
    """open3d's ``remove_statistical_outlier`` as nerfstudio's exporter applies it (20 neighbours, ratio 10).  m_i = the mean
    distance of point i to its ``nb_neighbors - 1`` nearest others (open3d counts the point itself, at distance 0, among its
    ``nb_neighbors``; leaving it out scales every m_i alike and keeps the same points); over the finite m_i, mu = mean,
    sigma = sqrt(sum (m - mu)^2 / (n - 1)), tau = mu + std_ratio * sigma; a point is kept iff m_i < tau.  With fewer than
    ``nb_neighbors`` finite points only the non-finite ones go.  Returns (the kept points in order, the bool keep mask [M])."""
    k = int(nb_neighbors) - 1
    if not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"nb_neighbors must be 2 .. {MAX_NEIGHBORS + 1}")
    if not float(std_ratio) > 0.0:
        raise ValueError("std_ratio must be positive")
    pos = cloud.positions
    mean = knn(pos, k, indices=False, distances=False, mean_distance=True).mean_distance
    finite = torch.isfinite(pos).all(dim=1)
    few = finite.sum() < int(nb_neighbors)  # then no row is full and every m_i is +inf
    keep = torch.where(few, finite, outlier_keep_mask(mean, std_ratio))
    return cloud.select(keep.nonzero().squeeze(1)), keep  # (nonzero: the one synchronisation)


def estimate_normals(cloud: ThermalPointCloud, k: int = 30, viewpoints: Optional[Tensor] = None) -> ThermalPointCloud:
    """``cloud`` with ``normals`` [M,3] float32 from each point's ``k`` nearest neighbours, turned towards ``viewpoints`` [M,3]
    (``PointCloudExporter.viewpoints(cloud)``: the camera a point was seen from) where given."""
    idx = knn(cloud.positions, k, distances=False).indices
    return dataclasses.replace(cloud, normals=pointcloud_normals(cloud.positions, idx, viewpoints))
