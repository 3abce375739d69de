"""Orthographic thermograms of a mesh — a scaled, distortion-free image of a façade, a floor or a wall: every pixel has a known size in
world units, the face it shows, its depth, its temperature and its colour, and can be traced back to the surface.  A depth slab
(``near`` / ``far``) cuts the mesh open to look at an interior wall.

``tn_mesh_rasterize`` does all of it on the device (a z-buffered triangle rasteriser on a 64-bit key plane, ordered fp64 sums in blocks
of 256); include/thermonerf_hip.h and DESIGN.md "Thermograms" define every output to the bit.  There is no CPU path.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip, colormaps
from ._common import color_array, mesh_arrays, out_tensor, require_triangles, workspace_of
from .mesh import ThermalMesh
from .regions import ThermalRegions

MAX_SIDE = 16384  # of an image, in pixels


@dataclasses.dataclass
class RasterView:
    """``tn_raster_view``, field for field: ``origin`` is the world position of the top-left corner of pixel (row 0, col 0) on the image
    plane; ``right``, ``down`` and ``forward`` are unit and orthogonal with right x down = forward (taken as given); ``pixel_size`` world
    units per pixel; faces are kept where near <= depth <= far; ``cull``: drop the faces seen from behind."""

    origin: Tuple[float, float, float]
    right: Tuple[float, float, float]
    down: Tuple[float, float, float]
    forward: Tuple[float, float, float]
    pixel_size: float
    width: int
    height: int
    near: float = -math.inf
    far: float = math.inf
    cull: bool = False

    def struct(self, small_box: int = 0) -> "_hip.tn_raster_view":
        """the C struct; ``small_box``: 0, or the small / large box threshold of a measurement (it cannot change the output)"""
        v = _hip.tn_raster_view()
        for name in ("origin", "right", "down", "forward"):
            axis = tuple(float(c) for c in getattr(self, name))
            if len(axis) != 3:
                raise ValueError(f"{name} has three components")
            for k in range(3):
                getattr(v, name)[k] = axis[k]
        v.pixel_size, v.near, v.far = float(self.pixel_size), float(self.near), float(self.far)
        v.width, v.height, v.cull, v.reserved = int(self.width), int(self.height), 1 if self.cull else 0, int(small_box)
        return v


def check_view(view: RasterView) -> None:
    """what ``tn_mesh_rasterize`` refuses, with words"""
    if not (1 <= int(view.width) <= MAX_SIDE and 1 <= int(view.height) <= MAX_SIDE):
        raise ValueError(f"an image is 1 .. {MAX_SIDE} pixels on each side, got {view.width} x {view.height}")
    if not (math.isfinite(view.pixel_size) and view.pixel_size > 0.0):
        raise ValueError(f"pixel_size must be positive and finite, got {view.pixel_size}")
    if not all(math.isfinite(float(c)) for name in ("origin", "right", "down", "forward") for c in getattr(view, name)):
        raise ValueError("the origin and the axes of a view must be finite")
    if math.isnan(view.near) or math.isnan(view.far):
        raise ValueError("near and far must not be NaN")


def view_axes(forward: Sequence[float], up: Sequence[float]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(right, down, forward) in fp64: forward normalised, right = normalise(forward x up), down = forward x right — unit, orthogonal,
    right x down = forward.  Refuses a zero or non-finite vector and an ``up`` along ``forward``."""
    f, u = np.asarray(forward, np.float64).reshape(-1), np.asarray(up, np.float64).reshape(-1)
    if f.shape != (3,) or u.shape != (3,) or not (np.isfinite(f).all() and np.isfinite(u).all()):
        raise ValueError("forward and up are three finite numbers each")
    if not np.linalg.norm(f) > 0.0 or not np.linalg.norm(u) > 0.0:
        raise ValueError("forward and up must not be zero")
    f, u = f / np.linalg.norm(f), u / np.linalg.norm(u)
    r = np.cross(f, u)
    if np.linalg.norm(r) < 1e-12:
        raise ValueError("up must not point along forward")
    r = r / np.linalg.norm(r)
    return r, np.cross(f, r), f


def place_view(axes, low: Sequence[float], high: Sequence[float], *, pixel_size: Optional[float] = None, width: Optional[int] = None,
               margin_pixels: int = 2, near: float = -math.inf, far: float = math.inf, cull: bool = False) -> RasterView:
    """The host arithmetic of ``fit_view``: the view with ``axes`` = (right, down, forward) that frames the box low .. high (the mesh's
    extent along the three axes) with ``margin_pixels`` empty pixels around it.  Exactly one of ``pixel_size`` and ``width`` is given.
    The image plane passes through the nearest vertex (depth 0 there), so ``near`` and ``far`` count from the front of the mesh."""
    right, down, forward = (np.asarray(a, np.float64) for a in axes)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    if (pixel_size is None) == (width is None):
        raise ValueError("give exactly one of pixel_size and width")
    margin = int(margin_pixels)
    if margin < 0:
        raise ValueError("margin_pixels must be >= 0")
    if not (np.isfinite(low).all() and np.isfinite(high).all() and (low <= high).all()):
        raise ValueError("the mesh has no finite vertex to frame")
    extent = high - low
    if width is not None:
        inner = int(width) - 2 * margin
        if inner < 1 or int(width) > MAX_SIDE:
            raise ValueError(f"width must leave at least one pixel between the margins and be at most {MAX_SIDE}, got {width}")
        if not extent[0] > 0.0:
            raise ValueError("the mesh has no extent along the view's right axis: give pixel_size instead of width")
        size = float(extent[0]) / inner
    else:
        size = float(pixel_size)
        if not (math.isfinite(size) and size > 0.0):
            raise ValueError(f"pixel_size must be positive and finite, got {pixel_size}")
    wide = int(width) if width is not None else max(int(math.ceil(float(extent[0]) / size)), 1) + 2 * margin
    tall = max(int(math.ceil(float(extent[1]) / size)), 1) + 2 * margin
    if wide > MAX_SIDE or tall > MAX_SIDE:
        if MAX_SIDE - 2 * margin < 1:
            raise ValueError(f"margin_pixels {margin} leaves no room in an image of {MAX_SIDE} pixels")
        fit = float(max(extent[0], extent[1])) / (MAX_SIDE - 2 * margin)
        raise ValueError(f"the image would be {wide} x {tall} pixels, beyond {MAX_SIDE}: a pixel size of {fit:.6g} or more fits")
    origin = right * (low[0] - margin * size) + down * (low[1] - margin * size) + forward * low[2]
    return RasterView(tuple(origin.tolist()), tuple(right.tolist()), tuple(down.tolist()), tuple(forward.tolist()), size, wide, tall,
                      float(near), float(far), bool(cull))


@torch.no_grad()
def fit_view(positions: Tensor, forward: Sequence[float], up: Sequence[float], *, pixel_size: Optional[float] = None,
             width: Optional[int] = None, margin_pixels: int = 2, near: float = -math.inf, far: float = math.inf,
             cull: bool = False) -> RasterView:
    """The view along ``forward`` with ``up`` pointing up in the image that frames the finite vertices of ``positions`` [V, 3]: the axes
    are orthonormalised in fp64 on the host (``view_axes``), the extent of the vertices along them is taken on the device (one host
    read of six numbers), the origin and the image size follow (``place_view``).  Exactly one of ``pixel_size`` (world units) and
    ``width`` (pixels, margins included) is given.  An image beyond 16384 pixels is refused with the pixel size that would fit."""
    axes = view_axes(forward, up)
    if (pixel_size is None) == (width is None):
        raise ValueError("give exactly one of pixel_size and width")
    p = _hip.require_device_tensor(positions, "positions")
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("positions must be [V, 3]")
    frame = torch.from_numpy(np.stack(axes, axis=1)).to(p.device)  # [3, 3]: the columns are right, down, forward
    q = p.double() @ frame
    finite = torch.isfinite(q).all(dim=1, keepdim=True)
    inf = torch.tensor(math.inf, dtype=torch.float64, device=p.device)
    both = torch.stack([torch.where(finite, q, inf).amin(dim=0), torch.where(finite, q, -inf).amax(dim=0)]) if p.shape[0] else \
        torch.stack([inf.expand(3), -inf.expand(3)])
    low, high = both.cpu().numpy()
    return place_view(axes, low, high, pixel_size=pixel_size, width=width, margin_pixels=margin_pixels, near=near, far=far, cull=cull)


def mesh_raster_small_box() -> int:
    """the largest box, in pixels per side, that a face's own thread rasterises"""
    return int(_hip.load().tn_mesh_raster_small_box())


def mesh_rasterize_workspace_bytes(num_triangles: int, width: int, height: int) -> int:
    return int(_hip.load().tn_mesh_rasterize_workspace_bytes(int(num_triangles), int(width), int(height)))


def mesh_rasterize_into(mesh: ThermalMesh, view: RasterView, *, counts: Tensor, stats: Tensor, pixel_face: Optional[Tensor] = None,
                        pixel_depth: Optional[Tensor] = None, pixel_temperature: Optional[Tensor] = None,
                        pixel_colors: Optional[Tensor] = None, workspace: Optional[Tensor] = None, small_box: int = 0) -> None:
    """``tn_mesh_rasterize`` on the current stream, without a host synchronisation: ``mesh`` seen through ``view``.  ``counts``: three
    device int64, OVERWRITTEN with the covered pixels, the drawn faces and the usable faces; ``stats``: three device float64, the
    ordered sum of the pixels' temperatures, their minimum and maximum; ``pixel_face`` int32, ``pixel_depth`` and
    ``pixel_temperature`` float32 [H, W], ``pixel_colors`` uint8 [H, W, 3] (from ``mesh.colors``): each optional.  ``workspace``:
    ``mesh_rasterize_workspace_bytes(T, W, H)`` device bytes (allocated if absent).  ``small_box``: measurements only."""
    require_triangles(mesh)
    check_view(view)
    p, t, tri, v, n = mesh_arrays(mesh)
    colors = color_array(mesh.colors, "colors", v, p.device) if pixel_colors is not None else None
    pixels = int(view.width) * int(view.height)
    pixel_face = out_tensor(pixel_face, "pixel_face", torch.int32, pixels, 1)
    pixel_depth = out_tensor(pixel_depth, "pixel_depth", torch.float32, pixels, 1)
    pixel_temperature = out_tensor(pixel_temperature, "pixel_temperature", torch.float32, pixels, 1)
    pixel_colors = out_tensor(pixel_colors, "pixel_colors", torch.uint8, pixels, 3)
    counts = out_tensor(counts, "counts", torch.int64, 3, 1)
    stats = out_tensor(stats, "stats", torch.float64, 3, 1)
    if counts is None or stats is None:
        raise ValueError("counts and stats are required")
    dev = p.device
    work = v > 0 and n > 0
    workspace, size = workspace_of(workspace, mesh_rasterize_workspace_bytes(n, view.width, view.height) if work else 0, dev)
    struct = view.struct(small_box)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_rasterize(
            p.data_ptr() if v else None, t.data_ptr() if v else None, _hip.ptr(colors), tri.data_ptr() if n else None, v, n,
            struct, _hip.ptr(pixel_face), _hip.ptr(pixel_depth), _hip.ptr(pixel_temperature), _hip.ptr(pixel_colors), counts.data_ptr(),
            stats.data_ptr(), workspace.data_ptr() if work else None, size, _hip.current_stream()), "tn_mesh_rasterize")


class PixelImage:
    """what ``Thermogram`` and ``CameraThermogram`` do alike with their images ``pixel_face``, ``pixel_temperature`` and
    ``pixel_colors`` [H, W], the mesh's ``temperature_bounds`` and the image's ``min_temperature`` / ``max_temperature``"""

    def to_rgb8(self, colors: str = "thermal", bounds: Optional[Tuple[float, float]] = None) -> Tensor:
        """uint8 [H, W, 3] on the device.  ``"rgb"``: the mesh's colours.  ``"thermal"``: (t - lo) / (hi - lo) through
        ``tn_frame_to_rgb8``'s ``TN_FRAME_LUT`` with the magma table; ``bounds`` = (lo, hi) defaults to the mesh's
        ``temperature_bounds``, then to the image's own range.  Empty pixels come out black."""
        if colors == "rgb":
            if self.pixel_colors is None:
                raise ValueError("the mesh has no colours")
            return self.pixel_colors
        if colors != "thermal":
            raise ValueError('colors is "thermal" or "rgb"')
        from ..render.renderer import LUT, frame_to_rgb8

        lo, hi = thermal_bounds(bounds, self.temperature_bounds, (self.min_temperature, self.max_temperature))
        t = self.pixel_temperature
        x = (t - lo) / (hi - lo) if hi > lo else torch.where(torch.isnan(t), t, torch.zeros_like(t))
        table = torch.from_numpy(colormaps.table_u8("magma")).to(t.device).contiguous()
        height, width = t.shape
        return frame_to_rgb8(x.reshape(-1, 1).contiguous(), LUT, table).reshape(height, width, 3)

    def region_map(self, regions: ThermalRegions) -> Tensor:
        """int32 [H, W]: ``regions.face_region`` gathered through ``pixel_face`` — the number of the thermal region every pixel
        shows, -1 where the pixel is empty or its face lies in no region"""
        face_region = regions.face_region
        if face_region.device != self.pixel_face.device:
            raise ValueError("the regions and the thermogram are on different devices")
        if bool((self.pixel_face >= face_region.shape[0]).any()):
            raise ValueError("the regions belong to another mesh: a pixel shows a face beyond face_region")
        padded = torch.cat([face_region, torch.full((1,), -1, dtype=face_region.dtype, device=face_region.device)])
        return padded[self.pixel_face.long()]  # (the last slot takes the -1 of the empty pixels)


@dataclasses.dataclass
class Thermogram(PixelImage):
    """what ``mesh_thermogram`` made: the four images on the device and the numbers of the one host read; ``to_rgb8`` and
    ``region_map`` are ``PixelImage``'s"""

    pixel_face: Tensor          # int32 [H, W]: the face every pixel shows, -1 where empty
    pixel_depth: Tensor         # float32 [H, W]: its depth along ``view.forward`` from the image plane, NaN where empty
    pixel_temperature: Tensor   # float32 [H, W]: degrees Celsius, NaN where empty
    pixel_colors: Tensor        # uint8 [H, W, 3]: the mesh's colours, 0 where empty
    view: RasterView
    covered: int                # pixels that show a face
    covered_area: float         # covered x pixel_size^2, in the mesh's units squared
    mean_temperature: float     # over the covered pixels; NaN when empty
    min_temperature: float
    max_temperature: float
    drawn_faces: int
    usable_faces: int
    temperature_bounds: Optional[Tuple[float, float]] = None  # the mesh's

    def world_position(self, row: int, col: int) -> Tuple[float, float, float]:
        """origin + (col + 0.5) s right + (row + 0.5) s down + depth forward: where the surface that pixel (row, col) shows lies (one
        host read; NaN where the pixel is empty)"""
        v = self.view
        return pixel_position(v, int(row), int(col), float(self.pixel_depth[int(row), int(col)]))


def thermal_bounds(given, of_mesh, of_image) -> Tuple[float, float]:
    """the (lo, hi) a thermal image is scaled with: the first of the three that is there"""
    for b in (given, of_mesh, of_image):
        if b is not None and all(math.isfinite(float(x)) for x in b):
            return float(b[0]), float(b[1])
    return 0.0, 1.0


def pixel_position(view: RasterView, row: int, col: int, depth: float) -> Tuple[float, float, float]:
    s = float(view.pixel_size)
    return tuple(float(view.origin[k]) + (col + 0.5) * s * float(view.right[k]) + (row + 0.5) * s * float(view.down[k]) +
                 depth * float(view.forward[k]) for k in range(3))


@torch.no_grad()
def mesh_thermogram(mesh: ThermalMesh, view: RasterView) -> Thermogram:
    """``mesh`` seen through ``view`` as a ``Thermogram``.  One host read: the three counts with the three statistics."""
    check_view(view)
    p = _hip.require_device_tensor(mesh.positions, "positions")
    dev, height, width = p.device, int(view.height), int(view.width)
    with torch.cuda.device(dev):
        head = torch.empty((6,), dtype=torch.int64, device=dev)  # the three counts and, behind them, the three statistics
        face = torch.empty((height, width), dtype=torch.int32, device=dev)
        depth = torch.empty((height, width), dtype=torch.float32, device=dev)
        temperature = torch.empty((height, width), dtype=torch.float32, device=dev)
        colors = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
        mesh_rasterize_into(mesh, view, counts=head[:3], stats=head[3:].view(torch.float64), pixel_face=face, pixel_depth=depth,
                            pixel_temperature=temperature, pixel_colors=colors)
        first = head.cpu().numpy()  # the one read
    covered, drawn, usable = (int(x) for x in first[:3])
    total, low, high = (float(x) for x in first[3:].view(np.float64))
    return Thermogram(face, depth, temperature, colors, view, covered, covered * float(view.pixel_size) ** 2,
                      total / covered if covered else math.nan, low, high, drawn, usable, mesh.temperature_bounds)
