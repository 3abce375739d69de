"""Voxel down-sampling of a thermal point cloud — the voxel grid filter of open3d / CloudCompare, with a temperature: one point per
occupied voxel, its position, colours and temperature the mean over the voxel's members (for a thermal cloud also the better
measurement: the mean over every view of a spot).

``tn_voxel_downsample`` keys every point with its voxel, sorts (key, point index) with ``tn_sort_pairs`` — a stable radix sort on
the device — and lets one thread per voxel average its members in ascending point index, in fp64; include/thermonerf_hip.h and
DESIGN.md "Point-cloud export" define every output to the bit.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _hip
from ._common import MAX_COUNT, out_tensor, workspace_of
from .pointcloud import ThermalPointCloud

MAX_VOXELS_PER_AXIS = 2 ** 21


def sort_tile() -> int:
    """keys per tile of the sort's histogram and scatter kernels (one block each)"""
    return int(_hip.load().tn_sort_tile())


def sort_pairs_workspace_bytes(n: int) -> int:
    return int(_hip.load().tn_sort_pairs_workspace_bytes(int(n)))


def voxel_downsample_workspace_bytes(num_points: int) -> int:
    return int(_hip.load().tn_voxel_downsample_workspace_bytes(int(num_points)))


def _as_uint64(t: Tensor, name: str) -> Tensor:
    """keys as the kernels read them: 64-bit patterns, given as torch.uint64 or torch.int64"""
    if not isinstance(t, Tensor) or t.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{name} must be a torch.int64 or torch.uint64 tensor")
    return _hip.require_device_tensor(t, name, t.dtype)


def sort_pairs(keys: Tensor, values: Optional[Tensor] = None, key_bits: int = 64, *, workspace: Optional[Tensor] = None
               ) -> Tuple[Tensor, Tensor]:
    """(sorted keys, their values): ``tn_sort_pairs`` on the current stream, without a host synchronisation — the pairs in
    ascending order of the keys' low ``8 * ceil(key_bits / 8)`` bits AS UNSIGNED NUMBERS, equal ones in input order (stable).
    ``keys``: [n] int64 or uint64 on the device (the 64-bit pattern is what is sorted; the result has the same dtype);
    ``values``: [n] int32 or None for 0 .. n-1, which makes the second result the sorting permutation.  The inputs are not
    modified.  ``workspace``: ``sort_pairs_workspace_bytes(n)`` device bytes (allocated if absent)."""
    k = _as_uint64(keys, "keys")
    if k.dim() != 1 or k.shape[0] > MAX_COUNT:
        raise ValueError("keys must be [n] with n <= 2^31 - 1")
    n, bits = int(k.shape[0]), int(key_bits)
    if not 1 <= bits <= 64:
        raise ValueError("key_bits must be 1 .. 64")
    v = None
    if values is not None:
        v = _hip.require_device_tensor(values, "values", torch.int32)
        if tuple(v.shape) != (n,):
            raise ValueError("values must be [n] like keys")
    dev = k.device
    with torch.cuda.device(dev):
        keys_out = torch.empty((n,), dtype=k.dtype, device=dev)
        values_out = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            workspace, size = workspace_of(workspace, sort_pairs_workspace_bytes(n), dev)
            _hip.check(_hip.load().tn_sort_pairs(k.data_ptr(), _hip.ptr(v), n, bits, keys_out.data_ptr(), values_out.data_ptr(),
                                                 workspace.data_ptr(), size, _hip.current_stream()), "tn_sort_pairs")
    return keys_out, values_out


def voxel_params(origin: Sequence[float], voxel_size: float, dims: Sequence[int]) -> "_hip.tn_voxel_params":
    """The by-value parameter block of ``tn_voxel_downsample``: ``origin`` and ``voxel_size`` are rounded ONCE to fp32."""
    q = _hip.tn_voxel_params()
    for a in range(3):
        q.origin[a], q.dims[a] = float(origin[a]), int(dims[a])
    q.voxel_size = float(voxel_size)
    return q


def voxel_grid(lo: Sequence[float], hi: Sequence[float], voxel_size: float) -> Tuple[Tuple[float, ...], Tuple[int, ...]]:
    """(origin, dims) of the grid that holds the box ``lo`` .. ``hi`` (fp32 values): origin = lo and
    dims_a = int(((double)hi_a - (double)lo_a) * inv) + 1 with inv = 1.0 / (double)(float)voxel_size — the kernel's own fp64 steps,
    so the point at ``hi`` falls in the last voxel.  More than 2^21 voxels on an axis raises ``ValueError``."""
    size = C.c_float(float(voxel_size)).value
    if not (size > 0.0 and math.isfinite(size)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    inv = 1.0 / size
    dims = []
    for a in range(3):
        u = (float(hi[a]) - float(lo[a])) * inv
        if not u < MAX_VOXELS_PER_AXIS:
            raise ValueError(f"voxel_size {voxel_size} needs more than 2^21 voxels on axis {a} (extent {float(hi[a]) - float(lo[a])}); "
                             "choose a larger voxel size")
        dims.append(int(u) + 1)
    return tuple(float(v) for v in lo), tuple(dims)


def voxel_downsample_into(cloud: ThermalPointCloud, params, *, positions: Optional[Tensor], colors: Optional[Tensor],
                          temperature: Optional[Tensor], voxel_count: Optional[Tensor], count: Tensor,
                          thermal_colors: Optional[Tensor] = None, source: Optional[Tensor] = None, capacity: Optional[int] = None,
                          workspace: Optional[Tensor] = None) -> None:
    """``tn_voxel_downsample`` on the current stream, without a host synchronisation: the averaged points of ``cloud`` over the
    grid ``params`` (``voxel_params(...)``) into positions [capacity,3] float32, colors [capacity,3] uint8, temperature [capacity]
    float32, voxel_count [capacity] int32 and, optionally, thermal_colors [capacity,3] uint8 and source [capacity] int64 (each
    only if the cloud has it).  ``count``: one device int64, OVERWRITTEN with the full number of occupied voxels.  ``capacity``
    defaults to the rows of ``positions`` (0 without it: the sizing call).  ``workspace``:
    ``voxel_downsample_workspace_bytes(len(cloud))`` device bytes (allocated if absent)."""
    p = _hip.require_device_tensor(cloud.positions, "positions")
    n = p.shape[0] if p.dim() == 2 and p.shape[1] == 3 else -1
    if n < 0 or n > MAX_COUNT:
        raise ValueError("positions must be [N, 3] with N <= 2^31 - 1")
    c = _hip.require_device_tensor(cloud.colors, "colors", torch.uint8)
    t = _hip.require_device_tensor(cloud.temperature, "temperature")
    tc = None if cloud.thermal_colors is None else _hip.require_device_tensor(cloud.thermal_colors, "thermal_colors", torch.uint8)
    src = None if cloud.source is None else _hip.require_device_tensor(cloud.source, "source", torch.int64)
    if tuple(c.shape) != (n, 3) or t.numel() != n or (tc is not None and tuple(tc.shape) != (n, 3)) or (src is not None and src.numel() != n):
        raise ValueError("colors / thermal_colors must be [N, 3] and temperature / source must hold N values")
    if capacity is None:
        capacity = 0 if positions is None else positions.shape[0]
    capacity = int(capacity)
    if capacity < 0:
        raise ValueError("capacity must not be negative")
    positions = out_tensor(positions, "positions", torch.float32, capacity, 3)
    colors = out_tensor(colors, "colors", torch.uint8, capacity, 3)
    temperature = out_tensor(temperature, "temperature", torch.float32, capacity, 1)
    voxel_count = out_tensor(voxel_count, "voxel_count", torch.int32, capacity, 1)
    thermal_colors = out_tensor(thermal_colors, "thermal_colors", torch.uint8, capacity, 3)
    source = out_tensor(source, "source", torch.int64, capacity, 1)
    count = out_tensor(count, "count", torch.int64, 1, 1)
    if capacity > 0 and (positions is None or colors is None or temperature is None or voxel_count is None):
        raise ValueError("positions, colors, temperature and voxel_count are required when capacity > 0")
    if (thermal_colors is not None and tc is None) or (source is not None and src is None):
        raise ValueError("the cloud has no thermal_colors / source to average into the output given for it")
    dev = p.device
    workspace, size = workspace_of(workspace, voxel_downsample_workspace_bytes(n), dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_voxel_downsample(
            p.data_ptr() if n else None, c.data_ptr() if n else None, t.data_ptr() if n else None, _hip.ptr(tc) if n else None,
            _hip.ptr(src) if n else None, n, C.byref(params), _hip.ptr(positions), _hip.ptr(colors), _hip.ptr(temperature),
            _hip.ptr(thermal_colors), _hip.ptr(source), _hip.ptr(voxel_count), capacity, count.data_ptr(),
            workspace.data_ptr() if n else None, size, _hip.current_stream()), "tn_voxel_downsample")


def _empty(cloud: ThermalPointCloud) -> Tuple[ThermalPointCloud, Tensor]:
    none = cloud.select(slice(0, 0))
    none.normals = None
    return none, torch.empty((0,), dtype=torch.int32, device=cloud.positions.device)


@torch.no_grad()
def voxel_downsample(cloud: ThermalPointCloud, voxel_size: float) -> Tuple[ThermalPointCloud, Tensor]:
    """``cloud`` with one point per occupied voxel of edge ``voxel_size`` (in the cloud's units): position, colours and temperature
    averaged over the voxel's members, ``source`` that of its first member, points in ascending voxel order.  The grid starts at
    the component-wise minimum of the finite points and ends with the voxel of their maximum (``voxel_grid``); non-finite points
    are dropped.  Normals, if present, are dropped too (estimate them afterwards); ``temperature_bounds`` is carried over.  Two
    host reads: the six numbers of the bounding box, then the voxel count.  Returns (the down-sampled cloud, int32 [M'] the
    members per output point).  A ``voxel_size`` that needs more than 2^21 voxels on an axis raises ``ValueError``."""
    size = C.c_float(float(voxel_size)).value
    if not (size > 0.0 and math.isfinite(size)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    p = _hip.require_device_tensor(cloud.positions, "positions")
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("positions must be [N, 3]")
    n, dev = int(p.shape[0]), p.device
    if n == 0:
        return _empty(cloud)
    with torch.cuda.device(dev):
        finite = torch.isfinite(p).all(dim=1, keepdim=True)
        lo = torch.where(finite, p, torch.full_like(p, float("inf"))).amin(dim=0)
        hi = torch.where(finite, p, torch.full_like(p, float("-inf"))).amax(dim=0)
        box = torch.cat([lo, hi]).tolist()  # the one read of the six numbers
        if not math.isfinite(box[0]):
            return _empty(cloud)
        origin, dims = voxel_grid(box[:3], box[3:], size)
        positions = torch.empty((n, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        temperature = torch.empty((n,), dtype=torch.float32, device=dev)
        thermal_colors = None if cloud.thermal_colors is None else torch.empty((n, 3), dtype=torch.uint8, device=dev)
        source = None if cloud.source is None else torch.empty((n,), dtype=torch.int64, device=dev)
        voxel_count = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.empty((1,), dtype=torch.int64, device=dev)
        voxel_downsample_into(cloud, voxel_params(origin, size, dims), positions=positions, colors=colors, temperature=temperature,
                              voxel_count=voxel_count, count=count, thermal_colors=thermal_colors, source=source)
        m = int(count.item())  # the one read of the count
    out = ThermalPointCloud(positions[:m], colors[:m], temperature[:m], None if thermal_colors is None else thermal_colors[:m],
                            None if source is None else source[:m], cloud.temperature_bounds)
    return out, voxel_count[:m]
