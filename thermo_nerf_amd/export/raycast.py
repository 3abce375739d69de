"""Ray queries against a thermal mesh — what it looks like from the camera that took photo K, pixel for pixel beside the measured
thermal image; what temperature lies behind pixel (r, c) and where on the surface; whether a surface point is visible from a camera.

``tn_mesh_bvh_build`` builds a linear bounding-volume hierarchy on the device (Morton codes on the stable radix sort, Karras's radix
tree, boxes fitted bottom-up in launches), ``tn_mesh_raycast`` walks it with one ray per lane.  include/thermonerf_hip.h and DESIGN.md
"Ray casting" define the tree and every output to the bit — the outputs without reference to the tree.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _hip
from ._common import MAX_COUNT, color_array, mesh_arrays, out_tensor, tree_arrays, workspace_of
from .mesh import ThermalMesh
from .thermogram import MAX_SIDE, PixelImage

STACK_ENTRIES = 64  # per ray; the depth bound of the tree is 61
# ``visible_from`` stops every ray at this fraction of the way to its point: 2^-10 of the distance short of it, so that the
# surface the point lies on (whose computed t is 1 up to rounding, and up to the fp32 rounding of the point itself) does not hide it
VISIBLE_FRACTION = 1.0 - 2.0 ** -10


def mesh_bvh_depth_bound() -> int:
    return int(_hip.load().tn_mesh_bvh_depth_bound())


def mesh_bvh_bytes(num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_bvh_bytes(int(num_triangles)))


def mesh_bvh_workspace_bytes(num_triangles: int) -> int:
    return int(_hip.load().tn_mesh_bvh_workspace_bytes(int(num_triangles)))


@dataclasses.dataclass
class MeshBVH:
    """what ``build_mesh_bvh`` made: the blob on the device with the mesh it belongs to.  The tree holds face INDICES and boxes: it
    is valid for the positions and triangles it was built from; after smoothing or any other change, build again."""

    blob: Tensor  # uint8 [tn_mesh_bvh_bytes(T)]
    num_vertices: int
    num_triangles: int
    mesh: ThermalMesh

    def tree(self) -> Dict[str, object]:
        """the blob's documented layout as host numbers and device tensors (one host read of the header): ``num_faces``,
        ``num_usable``, ``num_unusable``, ``num_nodes``, ``root``, ``depth``, ``lo`` / ``hi`` (the extent, tuples), ``faces`` int32 [T]
        (the leaf order), ``child`` int32 [num_nodes, 2], ``level`` int32 [num_nodes], ``box_lo`` / ``box_hi`` float32 [num_nodes, 2, 3]"""
        t = self.num_triangles
        head = self.blob[:64].cpu().numpy()
        ints, floats = head.view(np.int32), head.view(np.float32)
        if int(head.view(np.uint32)[0]) != 0x56424E54 or int(ints[1]) != 1 or int(ints[2]) != t:
            raise ValueError("the blob does not carry the header of a tree of this mesh")
        n = int(ints[5])
        faces_bytes = (4 * t + 63) // 64 * 64
        nodes = self.blob[64 + faces_bytes: 64 + faces_bytes + 64 * n].view(torch.int32).reshape(n, 16)
        boxes = nodes[:, :12].contiguous().view(torch.float32)
        return {"num_faces": int(ints[2]), "num_usable": int(ints[3]), "num_unusable": int(ints[4]), "num_nodes": n, "root": int(ints[6]),
                "depth": int(ints[7]), "lo": tuple(float(x) for x in floats[8:11]), "hi": tuple(float(x) for x in floats[11:14]),
                "faces": self.blob[64: 64 + 4 * t].view(torch.int32), "child": nodes[:, 12:14].contiguous(), "level": nodes[:, 14].contiguous(),
                "box_lo": boxes[:, :6].reshape(n, 2, 3), "box_hi": boxes[:, 6:].reshape(n, 2, 3)}


@torch.no_grad()
def build_mesh_bvh(mesh: ThermalMesh, *, blob: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> MeshBVH:
    """``tn_mesh_bvh_build`` on the current stream, without a host synchronisation: the tree of ``mesh``'s usable faces.  ``blob``:
    ``mesh_bvh_bytes(T)`` device bytes to build into (allocated if absent); ``workspace``: ``mesh_bvh_workspace_bytes(T)``."""
    p, t, tri, v, n = mesh_arrays(mesh)
    dev = p.device
    with torch.cuda.device(dev):
        blob, blob_size = workspace_of(blob, mesh_bvh_bytes(n), dev)
        workspace, size = workspace_of(workspace, mesh_bvh_workspace_bytes(n) if n else 0, dev)
        _hip.check(_hip.load().tn_mesh_bvh_build(p.data_ptr() if v else None, t.data_ptr() if v else None, tri.data_ptr() if n else None, v, n,
                                                 blob.data_ptr(), blob_size, workspace.data_ptr() if n else None, size,
                                                 _hip.current_stream()), "tn_mesh_bvh_build")
    return MeshBVH(blob.view(torch.uint8).reshape(-1)[:mesh_bvh_bytes(n)], v, n, mesh)


def check_window(t_min: float, t_max: float) -> None:
    """what ``tn_mesh_raycast`` refuses of a t window, with words"""
    if math.isnan(t_min) or math.isnan(t_max):
        raise ValueError("t_min and t_max must not be NaN")
    if not t_min >= 0.0:
        raise ValueError(f"t_min must be >= 0, got {t_min}")


def _rays(origins: Tensor, directions: Tensor, ray_t_max: Optional[Tensor], device) -> Tuple[Tensor, Tensor, Optional[Tensor], int]:
    o = _hip.require_device_tensor(origins, "origins")
    d = _hip.require_device_tensor(directions, "directions")
    if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape or 3 * o.shape[0] > MAX_COUNT:
        raise ValueError("origins and directions must both be [N, 3] with 3 N <= 2^31 - 1")
    if o.device != device or d.device != device:
        raise ValueError("the rays must be on the mesh's device")
    n = int(o.shape[0])
    if ray_t_max is not None:
        ray_t_max = _hip.require_device_tensor(ray_t_max, "ray_t_max")
        if ray_t_max.numel() != n or ray_t_max.device != device:
            raise ValueError("ray_t_max must hold N values on the mesh's device")
    return o, d, ray_t_max, n


def mesh_raycast_into(bvh: MeshBVH, origins: Tensor, directions: Tensor, *, t_min: float = 0.0, t_max: float = math.inf,
                      ray_t_max: Optional[Tensor] = None, cull: bool = False, any_hit: bool = False, hit_face: Optional[Tensor] = None,
                      hit_t: Optional[Tensor] = None, hit_uv: Optional[Tensor] = None, hit_temperature: Optional[Tensor] = None,
                      hit_colors: Optional[Tensor] = None, hit_any: Optional[Tensor] = None, counts: Optional[Tensor] = None,
                      stats: Optional[Tensor] = None) -> None:
    """``tn_mesh_raycast`` on the current stream, without a host synchronisation: the rays ``origins`` + t ``directions`` [N, 3]
    (directions as given, not normalised; t in their units) against the mesh of ``bvh``, for t_min <= t <= min(t_max,
    ray_t_max[i]).  Closest hit: ``hit_face`` int32 [N] (-1: a miss), ``hit_t``, ``hit_temperature`` float32 [N] and ``hit_uv``
    float32 [N, 2] (NaN on a miss), ``hit_colors`` uint8 [N, 3] (from ``mesh.colors``), ``counts`` int64 [4] (rays that hit, usable
    rays, usable faces, rays that reached the stack limit), ``stats`` float64 [3] (the ordered sum, minimum and maximum of the hit
    temperatures; needs ``hit_temperature``): each optional.  ``any_hit``: only ``hit_any`` uint8 [N] is written, 1 where the ray
    meets anything in its window."""
    check_window(float(t_min), float(t_max))
    p, t, tri, v, n, dev, blob = tree_arrays(bvh)
    o, d, ray_t_max, rays = _rays(origins, directions, ray_t_max, dev)
    if any_hit:
        if hit_any is None:
            raise ValueError("any_hit writes hit_any alone: give it")
        if any(x is not None for x in (hit_face, hit_t, hit_uv, hit_temperature, hit_colors, counts, stats)):
            raise ValueError("any_hit writes hit_any alone: the other outputs stay None")
    elif hit_any is not None:
        raise ValueError("hit_any is written with any_hit=True only")
    colors = color_array(bvh.mesh.colors, "colors", v, dev) if hit_colors is not None else None
    if stats is not None and hit_temperature is None:
        raise ValueError("stats are taken from hit_temperature: give both")
    hit_face = out_tensor(hit_face, "hit_face", torch.int32, rays, 1)
    hit_t = out_tensor(hit_t, "hit_t", torch.float32, rays, 1)
    hit_uv = out_tensor(hit_uv, "hit_uv", torch.float32, rays, 2)
    hit_temperature = out_tensor(hit_temperature, "hit_temperature", torch.float32, rays, 1)
    hit_colors = out_tensor(hit_colors, "hit_colors", torch.uint8, rays, 3)
    hit_any = out_tensor(hit_any, "hit_any", torch.uint8, rays, 1)
    counts = out_tensor(counts, "counts", torch.int64, 4, 1)
    stats = out_tensor(stats, "stats", torch.float64, 3, 1)
    params = _hip.tn_raycast_params(float(t_min), float(t_max), 1 if cull else 0, _hip.TN_RAYCAST_ANY if any_hit else _hip.TN_RAYCAST_CLOSEST)
    work = v > 0 and n > 0
    with torch.cuda.device(dev):
        _hip.check(_hip.load().tn_mesh_raycast(
            p.data_ptr() if work else None, t.data_ptr() if work else None, _hip.ptr(colors), tri.data_ptr() if n else None, v, n,
            blob.data_ptr(), blob.numel() * blob.element_size(), o.data_ptr() if rays else None, d.data_ptr() if rays else None,
            _hip.ptr(ray_t_max) if rays else None, rays, ctypes.byref(params), _hip.ptr(hit_face), _hip.ptr(hit_t), _hip.ptr(hit_uv),
            _hip.ptr(hit_temperature), _hip.ptr(hit_colors), _hip.ptr(hit_any), _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()),
            "tn_mesh_raycast")


@dataclasses.dataclass
class RayHits:
    """what ``mesh_raycast`` made: the arrays on the device and the numbers of the one host read.  With ``any_hit`` only ``hit_any``
    is there, the other arrays are None and the numbers are those of ``hit_any`` alone."""

    hit_face: Optional[Tensor]          # int32 [N]: the face every ray meets first, -1 on a miss
    hit_t: Optional[Tensor]             # float32 [N]: where along the ray, in units of its direction; NaN on a miss
    hit_uv: Optional[Tensor]            # float32 [N, 2]: the barycentrics of the second and third corner
    hit_temperature: Optional[Tensor]   # float32 [N]: degrees Celsius there
    hit_colors: Optional[Tensor]        # uint8 [N, 3]
    hit_any: Optional[Tensor]           # uint8 [N]: any_hit only
    hits: int
    usable_rays: int
    usable_faces: int
    stack_limit_rays: int               # 0: the stack covers the tree's depth bound
    mean_temperature: float             # over the hits; NaN without one
    min_temperature: float
    max_temperature: float

    def positions(self, origins: Tensor, directions: Tensor) -> Tensor:
        """float32 [N, 3]: origins + hit_t directions, NaN on a miss"""
        return origins + self.hit_t[:, None] * directions


@torch.no_grad()
def mesh_raycast(bvh: MeshBVH, origins: Tensor, directions: Tensor, *, t_min: float = 0.0, t_max: float = math.inf,
                 ray_t_max: Optional[Tensor] = None, cull: bool = False, any_hit: bool = False) -> RayHits:
    """The rays against the mesh of ``bvh`` as ``RayHits`` (see ``mesh_raycast_into``).  One host read: the four counts with the
    three statistics, or with ``any_hit`` the number of rays that meet something."""
    check_window(float(t_min), float(t_max))
    p = _hip.require_device_tensor(bvh.mesh.positions, "positions")
    dev = p.device
    o = _hip.require_device_tensor(origins, "origins")
    n = int(o.shape[0]) if o.dim() == 2 else -1
    if n < 0:
        raise ValueError("origins and directions must both be [N, 3] with 3 N <= 2^31 - 1")
    with torch.cuda.device(dev):
        if any_hit:
            some = torch.empty((n,), dtype=torch.uint8, device=dev)
            mesh_raycast_into(bvh, origins, directions, t_min=t_min, t_max=t_max, ray_t_max=ray_t_max, cull=cull, any_hit=True, hit_any=some)
            hits = int(some.sum())  # the one read
            return RayHits(None, None, None, None, None, some, hits, -1, -1, 0, math.nan, math.inf, -math.inf)
        head = torch.empty((7,), dtype=torch.int64, device=dev)  # the four counts and, behind them, the three statistics
        face = torch.empty((n,), dtype=torch.int32, device=dev)
        t = torch.empty((n,), dtype=torch.float32, device=dev)
        uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
        temperature = torch.empty((n,), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev) if bvh.mesh.colors is not None else None
        mesh_raycast_into(bvh, origins, directions, t_min=t_min, t_max=t_max, ray_t_max=ray_t_max, cull=cull, hit_face=face, hit_t=t,
                          hit_uv=uv, hit_temperature=temperature, hit_colors=colors, counts=head[:4], stats=head[4:].view(torch.float64))
        first = head.cpu().numpy()  # the one read
    hits, usable_rays, usable_faces, limit = (int(x) for x in first[:4])
    total, low, high = (float(x) for x in first[4:].view(np.float64))
    return RayHits(face, t, uv, temperature, colors, None, hits, usable_rays, usable_faces, limit, total / hits if hits else math.nan, low,
                   high)


# ---- a camera's view -------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class CameraView:
    """a pinhole camera in nerfstudio's convention: ``c2w`` the 3 x 4 camera-to-world (the camera looks along its -z, +y is up, +x
    to the right), ``fx``, ``fy``, ``cx``, ``cy`` in pixels, the image ``width`` x ``height``.  No lens distortion."""

    c2w: Sequence[Sequence[float]]
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int

    def matrix(self) -> np.ndarray:
        m = np.asarray(self.c2w, dtype=np.float64)
        if m.shape == (4, 4):
            m = m[:3]
        if m.shape != (3, 4):
            raise ValueError("c2w is a 3 x 4 (or 4 x 4) camera-to-world matrix")
        return m


def check_camera(camera: CameraView) -> None:
    if not (1 <= int(camera.width) <= MAX_SIDE and 1 <= int(camera.height) <= MAX_SIDE):
        raise ValueError(f"an image is 1 .. {MAX_SIDE} pixels on each side, got {camera.width} x {camera.height}")
    if not all(math.isfinite(float(x)) for x in (camera.fx, camera.fy, camera.cx, camera.cy)) or not (camera.fx > 0.0 and camera.fy > 0.0):
        raise ValueError("fx and fy must be positive, and the intrinsics finite")
    if not np.isfinite(camera.matrix()).all():
        raise ValueError("the camera-to-world matrix must be finite")


def camera_rays(camera: CameraView, device) -> Tuple[Tensor, Tensor]:
    """(origins, unit directions) float32 [H W, 3] through the pixel centres, row-major: ``tn_generate_rays`` on the current stream"""
    check_camera(camera)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"the camera's rays are generated on {dev}; thermo_nerf_amd runs only on a ROCm device (no CPU fallback exists).")
    n = int(camera.width) * int(camera.height)
    c2w = (ctypes.c_float * 12)(*[float(x) for x in camera.matrix().reshape(-1)])
    with torch.cuda.device(dev):
        o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _hip.check(_hip.load().tn_generate_rays(c2w, float(camera.fx), float(camera.fy), float(camera.cx), float(camera.cy), int(camera.height),
                                                int(camera.width), None, 0, n, o.data_ptr(), d.data_ptr(), None, _hip.current_stream()),
                   "tn_generate_rays")
    return o, d


@dataclasses.dataclass
class CameraThermogram(PixelImage):
    """what ``mesh_camera_thermogram`` made: the four images on the device and the numbers of the one host read; ``to_rgb8`` and
    ``region_map`` are ``PixelImage``'s"""

    pixel_face: Tensor          # int32 [H, W]: the face every pixel shows, -1 where empty
    pixel_distance: Tensor      # float32 [H, W]: the distance from the camera centre along the pixel's ray, NaN where empty
    pixel_temperature: Tensor   # float32 [H, W]: degrees Celsius, NaN where empty
    pixel_colors: Optional[Tensor]  # uint8 [H, W, 3]: the mesh's colours, 0 where empty
    camera: CameraView
    origins: Tensor             # float32 [H W, 3]: the rays the images were cast with
    directions: Tensor
    covered: int
    mean_temperature: float     # over the covered pixels; NaN when empty
    min_temperature: float
    max_temperature: float
    usable_faces: int
    stack_limit_rays: int
    temperature_bounds: Optional[Tuple[float, float]] = None  # the mesh's

    def world_position(self, row: int, col: int) -> Tuple[float, float, float]:
        """origin + distance direction of pixel (row, col): where the surface it shows lies (one host read; NaN where empty)"""
        k = int(row) * int(self.camera.width) + int(col)
        o, d = self.origins[k].double(), self.directions[k].double()
        return tuple(float(x) for x in (o + self.pixel_distance[int(row), int(col)].double() * d).cpu())


@torch.no_grad()
def mesh_camera_thermogram(bvh: MeshBVH, camera: CameraView, *, cull: bool = False, t_min: float = 0.0, t_max: float = math.inf
                           ) -> CameraThermogram:
    """The mesh of ``bvh`` seen through ``camera``: one ray per pixel centre (``tn_generate_rays``: unit directions, so t is the
    distance from the camera centre), the closest hit of each.  One host read."""
    check_camera(camera)
    p = _hip.require_device_tensor(bvh.mesh.positions, "positions")
    o, d = camera_rays(camera, p.device)
    hits = mesh_raycast(bvh, o, d, t_min=t_min, t_max=t_max, cull=cull)
    h, w = int(camera.height), int(camera.width)
    return CameraThermogram(hits.hit_face.view(h, w), hits.hit_t.view(h, w), hits.hit_temperature.view(h, w),
                            None if hits.hit_colors is None else hits.hit_colors.view(h, w, 3), camera, o, d, hits.hits, hits.mean_temperature,
                            hits.min_temperature, hits.max_temperature, hits.usable_faces, hits.stack_limit_rays, bvh.mesh.temperature_bounds)


@torch.no_grad()
def visible_from(bvh: MeshBVH, points: Tensor, eye: Sequence[float]) -> Tensor:
    """bool [P]: is ``points[i]`` ([P, 3] float32 on the device) seen from ``eye`` — the occlusion test of a projection.  One
    ``any_hit`` ray per point from the eye with direction point - eye, so t = 1 is the point; every ray stops at
    ``VISIBLE_FRACTION`` = 1 - 2^-10 of the way, just short of the surface the point lies on.  A point is visible when nothing is
    met before that.  A point at the eye, or a non-finite one, makes an unusable ray and counts as visible: nothing hides it.  No
    host synchronisation."""
    e = [float(x) for x in eye]
    if len(e) != 3 or not all(math.isfinite(x) for x in e):
        raise ValueError("eye is three finite numbers")
    pts = _hip.require_device_tensor(points, "points")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [P, 3]")
    dev = pts.device
    with torch.cuda.device(dev):
        origin = torch.tensor(e, dtype=torch.float32, device=dev).expand(pts.shape[0], 3).contiguous()
        direction = (pts - origin).contiguous()
        stop = torch.full((pts.shape[0],), VISIBLE_FRACTION, dtype=torch.float32, device=dev)
        some = torch.empty((pts.shape[0],), dtype=torch.uint8, device=dev)
        mesh_raycast_into(bvh, origin, direction, ray_t_max=stop, any_hit=True, hit_any=some)
    return some == 0
