"""tn_mesh_rasterize on the device against tests/mesh_raster_reference.py, exactly — every integer and every float bit pattern, no
tolerance anywhere — into guarded buffers with the inputs unchanged afterwards: the literal cases, odd image sizes, the top-left rule,
watertight lattices, depth ties, the small / large threshold, faces over the borders, slivers, slabs, culling, unusable faces, a
tilted view, 66 586 faces on 300 x 300 pixels, absent outputs, empty meshes, the error codes, determinism, the Python layer and the
command line."""
from __future__ import annotations

import dataclasses
import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_raster_reference as R
from tests import mesh_regions_reference as G
from thermo_nerf_amd import _hip, colormaps
from thermo_nerf_amd.export import (RasterView, ThermalMesh, Thermogram, fit_view, mesh_raster_small_box, mesh_rasterize_into,
                                    mesh_rasterize_workspace_bytes, mesh_thermogram, thermal_regions, write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F, D = np.float32, np.float64
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILLS = {torch.int32: -5, torch.float32: -777.0, torch.float64: -777.0, torch.uint8: 0xEE, torch.int64: -9}
NAMES = ("positions", "temperature", "colors", "triangles", "num_vertices", "num_triangles", "view", "pixel_face", "pixel_depth",
         "pixel_temperature", "pixel_colors", "counts", "stats", "workspace", "workspace_bytes", "stream")
PIXELS = {"pixel_face": (torch.int32, 1), "pixel_depth": (torch.float32, 1), "pixel_temperature": (torch.float32, 1),
          "pixel_colors": (torch.uint8, 3)}


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _struct(vw, small_box=0):
    struct = RasterView(vw["origin"], vw["right"], vw["down"], vw["forward"], vw["pixel_size"], vw["width"], vw["height"], vw["near"],
                        vw["far"], bool(vw["cull"])).struct(small_box)
    struct.cull = int(vw["cull"])  # (the error cases pass other numbers than 0 and 1)
    return struct


def raw(mesh, vw, absent=(), small_box=0):
    """tn_mesh_rasterize into guarded buffers (``absent``: the outputs passed as NULL): the buffers and host copies of counts, stats"""
    pos, temp, col, tri = mesh
    tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
    v, t, pixels = len(pos), len(tri), vw["width"] * vw["height"]
    given = [pos, temp, tri] + ([col] if col is not None else [])
    inputs = [_device(a) for a in given]
    buffers = {k: None if k in absent or (k == "pixel_colors" and col is None) else _buffer(pixels * n, dtype)
               for k, (dtype, n) in PIXELS.items()}
    counts, stats = _buffer(3, torch.int64), _buffer(3, torch.float64)
    need = mesh_rasterize_workspace_bytes(t, vw["width"], vw["height"])
    assert need > 0 and need % 8 == 0
    workspace = _buffer(need, torch.uint8)
    args = dict(positions=inputs[0].data_ptr() if v else None, temperature=inputs[1].data_ptr() if v else None,
                colors=inputs[3].data_ptr() if col is not None and v else None, triangles=inputs[2].data_ptr() if t else None,
                num_vertices=v, num_triangles=t, view=_struct(vw, small_box), counts=counts.data_ptr(), stats=stats.data_ptr(),
                workspace=workspace.data_ptr(), workspace_bytes=need, stream=_hip.current_stream(),
                **{k: _hip.ptr(b) for k, b in buffers.items()})
    _hip.check(_hip.load().tn_mesh_rasterize(*[args[k] for k in NAMES]), "tn_mesh_rasterize")
    torch.cuda.synchronize()
    _untouched(counts, 3, "counts")
    _untouched(stats, 3, "stats")
    _untouched(workspace, need, "workspace")
    for name, buf in buffers.items():
        if buf is not None:
            _untouched(buf, buf.numel() - GUARD, name)
    for before, now in zip(given, inputs):
        assert np.ascontiguousarray(before).tobytes() == now.cpu().numpy().tobytes(), "an input was written"
    return {"buffers": buffers, "counts": counts[:3].cpu().numpy(), "stats": stats[:3].cpu().numpy()}


def images(got, vw):
    """the kernel's outputs in the shape of the reference's"""
    h, w = vw["height"], vw["width"]
    out = {"counts": got["counts"], "stats": got["stats"]}
    for name, (dtype, n) in PIXELS.items():
        buf = got["buffers"][name]
        out[name] = None if buf is None else buf[:h * w * n].cpu().numpy().reshape((h, w) if n == 1 else (h, w, n))
    return out


def check(mesh, vw, want=None, **kw):
    """one call compared with the yardstick (or ``want``), bit for bit, on every output it was given"""
    want = R.rasterize(*mesh, vw) if want is None else want
    got = images(raw(mesh, vw, **kw), vw)
    assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
    for name in PIXELS:
        if got[name] is not None:
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            differ = np.flatnonzero(np.ascontiguousarray(got[name]).view(np.uint8).reshape(-1) != np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1))
            assert len(differ) == 0, (name, len(differ), "first differing byte", int(differ[0]))
    assert R.bits(got["stats"]).tolist() == R.bits(want["stats"]).tolist(), ("stats", got["stats"], want["stats"])
    return want, got


def flat(z=3.0, t=(20.0, 25.0, 30.0), corners=((1.25, 0.75), (5.5, 1.5), (2.0, 4.25))):
    """one triangle in the default view's pixel units"""
    pos = np.array([(x, y, z) for x, y in corners], F)
    return pos, np.array(t, F), np.array([(10, 200, 30), (250, 5, 90), (60, 70, 255)], np.uint8), np.array([(0, 1, 2)], np.int32)


# ---- the literal cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_literal_cases_through_the_kernel(name):
    case = R.LITERAL[name]
    want, got = check(R.literal_arrays(case), case["view"])
    assert R.literal_mismatch(got, case["want"]) is None, R.literal_mismatch(got, case["want"])


# ---- image sizes, the top-left rule, watertightness -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,height", [(7, 5), (1, 1), (17, 33), (33, 17), (256, 1), (1, 257)])
def test_image_sizes_that_are_no_multiple_of_a_tile(width, height):
    mesh = R.quad_lattice(5, -1.5, max(width, height) / 4.0 + 1.0, 3, jitter=0.4)
    want, _ = check(mesh, R.view(width, height))
    assert want["counts"][0] > 0
    pos, temp, col, tri = flat(corners=((-2.0, -3.0), (3.0 * width, -1.0), (-1.0, 3.0 * height)))
    want, _ = check((pos, temp, col, tri), R.view(width, height))
    assert want["counts"][0] == width * height, "one face larger than the whole image"


@pytest.mark.parametrize("winding", [(0, 1, 2), (0, 2, 1)])
@pytest.mark.parametrize("shift", [0.0, 16.0])
def test_top_left_rule_on_edges_through_pixel_centres(winding, shift):
    # shift 16: the same triangle, 20 pixels across, takes the large-face path
    size = 4.0 + shift
    pos = np.array([(0.5, 0.5, 2), (0.5 + size, 0.5, 2), (0.5, 0.5 + size, 2)], F)
    mesh = (pos, np.array([10, 14, 12], F), None, np.array([winding], np.int32))
    n = int(size) + 2
    want, got = check(mesh, R.view(n, n))
    j, i = np.mgrid[0:n, 0:n]
    assert ((want["pixel_face"] == 0) == (i + j < size)).all(), "the top and the left edge keep their centres, the diagonal loses them"


def test_quad_with_the_shared_diagonal_through_pixel_centres_and_a_watertight_lattice():
    for tri in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(0, 1, 2), (0, 3, 2)], [(1, 2, 3), (1, 3, 0)]):
        mesh = (np.array([(1, 1, 1), (21, 1, 2), (21, 21, 1), (1, 21, 3)], F), np.array([20, 21, 22, 23], F), None, np.array(tri, np.int32))
        want, got = check(mesh, R.view(22, 22))
        assert want["counts"][0] == 400 == int(want["samples"].sum()), "every pixel of the square, each by one face"
    mesh = R.quad_lattice(12, 1.3125, 2.171875, 7, jitter=0.5)
    want, got = check(mesh, R.view(30, 30))
    per_face = np.bincount(got["pixel_face"][got["pixel_face"] >= 0], minlength=len(mesh[3]))
    assert int(per_face.sum()) == int(got["counts"][0]) == int(want["samples"].sum()), "watertight: no pixel is hit twice"
    x0, x1 = 1.3125, 1.3125 + 12 * 2.171875
    j, i = np.mgrid[0:30, 0:30]
    inner = (i + 0.5 > x0) & (i + 0.5 < x1) & (j + 0.5 > x0) & (j + 0.5 < x1)
    assert ((got["pixel_face"] >= 0) == inner).all(), "every pixel inside the rim is covered, none outside"


# ---- the winner ---------------------------------------------------------------------------------------------------------------------------

def test_equal_depths_go_to_the_lower_index_and_the_nearer_face_wins_wherever_it_is_listed():
    pos, temp, col, tri = flat(corners=((-1.0, -1.0), (30.0, -2.0), (-3.0, 30.0)))
    want, got = check((pos, temp, col, np.array([(0, 1, 2), (0, 1, 2)], np.int32)), R.view(9, 9))
    assert (got["pixel_face"] == 0).all() and want["ties"] == 81, "two identical faces"

    def pair(shift, order):  # the face at z = 3 as vertices 0 1 2, a copy moved by `shift` along z as 3 4 5
        return (np.concatenate([pos, pos + np.array([0, 0, shift], F)]).astype(F), np.concatenate([temp, temp + 1]),
                np.concatenate([col, 255 - col]), np.array(order, np.int32))

    for order in ([(0, 1, 2), (3, 4, 5)], [(3, 4, 5), (0, 1, 2)]):  # the nearer face listed after the farther one, and before it
        want, got = check(pair(-1.0, order), R.view(9, 9))
        assert want["ties"] == 0 and (got["pixel_face"] == (1 if order[0][0] == 0 else 0)).all() and (got["pixel_depth"] == 2.0).all()
    # seen from 1024 units away the depths 1027 and 1027 + 2^-22 differ in fp64 and are one fp32: the lower index wins, nearer or not
    far_view = R.view(9, 9, origin=(0.0, 0.0, -1024.0))
    for order in ([(0, 1, 2), (3, 4, 5)], [(3, 4, 5), (0, 1, 2)]):
        mesh = pair(2.0 ** -22, order)
        z = R.vertices(mesh[0], far_view)[2]
        assert (z[:3] < z[3:]).all() and (z[:3].astype(F) == z[3:].astype(F)).all()
        want, got = check(mesh, far_view)
        assert want["ties"] == 81 and (got["pixel_face"] == 0).all()
        assert (got["pixel_temperature"] == want["pixel_temperature"]).all() and (got["pixel_depth"] == 1027.0).all()


# ---- the small / large threshold ---------------------------------------------------------------------------------------------------------

def test_boxes_one_pixel_below_at_and_above_the_threshold_and_any_threshold_gives_the_same_bytes():
    box = mesh_raster_small_box()
    assert box == 8
    for side in (box - 1, box, box + 1):
        # a box of exactly `side` pixel centres: from centre 2.5 to centre 2.5 + side - 1
        a, b = 2.25, 2.5 + side - 1 + 0.25
        mesh = flat(corners=((a, a), (b, a + 0.5), (a + 0.25, b)))
        view = R.view(24, 20)
        want, got = check(mesh, view)
        assert want["counts"][0] > side
        for small_box in (1, side, side + 1, 16384):
            check(mesh, view, want=want, small_box=small_box)
    scene, view = _big(), R.view(R.BIG_SIDE, R.BIG_SIDE)
    first = raw(scene, view, small_box=1)
    second = raw(scene, view, small_box=64)
    for name, buf in first["buffers"].items():
        assert torch.equal(buf, second["buffers"][name]), name
    assert first["stats"].tobytes() == second["stats"].tobytes() and first["counts"].tobytes() == second["counts"].tobytes()


# ---- borders, slivers, slabs, culling -------------------------------------------------------------------------------------------------------

def test_faces_over_each_border_wholly_outside_and_a_sliver_without_a_pixel_centre():
    view = R.view(20, 14)
    parts = []
    for dx, dy in ((-6.0, 3.0), (15.0, 2.0), (5.0, -5.0), (6.0, 9.0), (-5.0, -4.0), (14.0, 9.5)):  # left, right, top, bottom, two corners
        parts.append(flat(corners=((dx, dy), (dx + 11.0, dy + 1.0), (dx + 2.0, dy + 10.0)), z=3.0 + dx / 100.0))
    for dx, dy in ((-40.0, 2.0), (25.0, 2.0), (3.0, -30.0), (3.0, 20.0), (1e6, 1e6)):  # wholly outside
        parts.append(flat(corners=((dx, dy), (dx + 9.0, dy + 1.0), (dx + 2.0, dy + 8.0))))
    want, got = check(R.merge(*parts), view)
    assert set(np.unique(want["pixel_face"]).tolist()) == {-1, 0, 1, 2, 3, 4, 5} and want["counts"].tolist()[1:] == [11, 11]
    sliver = flat(corners=((1.6, 1.6), (9.4, 1.7), (5.0, 1.9)))
    want, got = check(sliver, view)
    assert want["counts"].tolist() == [0, 1, 1] and (got["pixel_face"] == -1).all()
    assert R.bits(got["stats"]).tolist() == R.bits(np.array([0.0, math.inf, -math.inf])).tolist()


def test_near_and_far():
    pos = np.array([(-2, -2, 1.0), (60, -1, 9.0), (-1, 60, 2.0)], F)
    mesh = (pos, np.array([10, 30, 20], F), np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255)], np.uint8), np.array([(0, 1, 2)], np.int32))
    whole, _ = check(mesh, R.view(21, 19))
    assert whole["counts"][0] == 21 * 19
    cut, got = check(mesh, R.view(21, 19, near=2.5, far=4.0))
    assert 0 < cut["counts"][0] < 21 * 19
    depth = got["pixel_depth"][got["pixel_face"] >= 0]
    assert depth.min() >= 2.5 and depth.max() <= 4.0 and (whole["pixel_depth"][got["pixel_face"] < 0] != 3.0).all()
    one = float(whole["pixel_depth"][7, 9])
    exact, _ = check(mesh, R.view(21, 19, near=one, far=one))  # (the slab is compared in fp64: at most the pixels whose fp64 depth is `one`)
    assert exact["counts"][0] <= 1
    # legs of 64 pixels: the barycentrics are multiples of 2^-28 and add up to 1 exactly, so the depth is 3 exactly at every pixel
    flat_face = flat(z=3.0, corners=((-1.0, -1.0), (63.0, -1.0), (-1.0, 63.0)))
    both, _ = check(flat_face, R.view(21, 19, near=3.0, far=3.0))
    assert both["counts"][0] == 21 * 19, "near == far keeps the surface at exactly that depth"
    nothing, _ = check(mesh, R.view(21, 19, near=4.0, far=2.5))
    assert nothing["counts"].tolist() == [0, 1, 1]
    for near, far in ((-math.inf, math.inf), (-math.inf, 4.0), (2.5, math.inf)):
        check(mesh, R.view(21, 19, near=near, far=far))


def test_cull_on_a_closed_tetrahedron():
    mesh = R.tetrahedron()
    both, _ = check(mesh, R.view(16, 16, cull=0))
    front, got = check(mesh, R.view(16, 16, cull=1))
    p = mesh[0].astype(D)[mesh[3]]  # [4, 3, 3]
    area2 = ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])).tolist()
    facing = {f for f in range(4) if area2[f] < 0}
    assert facing and len(facing) < 4 and set(np.unique(got["pixel_face"]).tolist()) - {-1} == facing
    assert front["counts"].tolist() == [int(both["counts"][0]), len(facing), 4] and both["counts"].tolist()[1:] == [4, 4]
    assert (front["pixel_face"] == both["pixel_face"]).all(), "a closed surface shows its front faces either way"
    inside, got = check(mesh, R.view(16, 16, cull=0, near=5.0))  # cut open: the back faces from inside
    assert set(np.unique(got["pixel_face"]).tolist()) - {-1} - facing


# ---- unusable and edge-on faces, a tilted view -------------------------------------------------------------------------------------------------

def test_unusable_faces_scattered_through_the_list_the_first_and_the_last_included():
    pos, temp, col, tri = (a.copy() for a in R.quad_lattice(12, 1.3125, 2.171875, 7, jitter=0.5))
    v, t = len(pos), len(tri)
    rng = np.random.default_rng(17)
    tri[0], tri[-1] = (v, 1, 2), (5, -1, 6)
    rows = rng.permutation(np.arange(1, t - 1))[:40]
    tri[rows[:10], 0] = v + rng.integers(0, 5, 10)
    tri[rows[10:20], 1] = -1 - rng.integers(0, 5, 10)
    tri[rows[20:30], 2] = tri[rows[20:30], 0]
    tri[rows[30:40], 1] = tri[rows[30:40], 2]
    spoiled = rng.permutation(v)[:12]
    pos[spoiled[0], 0], pos[spoiled[1], 1], pos[spoiled[2], 2] = np.nan, np.inf, -np.inf
    temp[spoiled[3]], temp[spoiled[4]] = np.nan, np.inf
    pos[spoiled[5], 0], pos[spoiled[6], 1] = 2.0 ** 21 + 1.0, -(2.0 ** 22)  # beyond the fixed-point range of 2^21 pixels
    pos[spoiled[7], 0] = 2.0 ** 21  # exactly on it: rasterable
    want, got = check((pos, temp, col, tri), R.view(30, 30))
    assert want["counts"][2] < t - 42 and want["counts"][0] > 300 and -1 in want["pixel_face"][5:25, 5:25]
    usable = R.faces(pos, temp, tri, R.view(30, 30))[0]
    assert not usable[0] and not usable[-1] and usable[np.any(tri == spoiled[7], axis=1) & (tri < v).all(axis=1) & (tri >= 0).all(axis=1)].any()
    assert np.isfinite(got["pixel_temperature"][got["pixel_face"] >= 0]).all()


def test_edge_on_faces_are_usable_and_not_drawn():
    pos = np.array([(1, 1, 1), (9, 9, 5), (5, 5, 9), (1, 9, 2), (4.0, 4.0, 3.0), (4.0 + 2.0 ** -10, 4.0, 3.0)], F)
    mesh = (pos, np.full(6, 20.0, F), None, np.array([(0, 1, 2), (0, 3, 1), (3, 4, 5)], np.int32))
    want, got = check(mesh, R.view(10, 10))
    assert want["counts"].tolist()[1:] == [1, 3] and set(np.unique(got["pixel_face"]).tolist()) == {-1, 1}
    # seen along x the whole lattice (z nearly constant in y ... ) is edge-on or nearly so: whatever is drawn, the same bits
    check(R.quad_lattice(6, 1.0, 2.0, 5), R.view(16, 16, right=(0.0, 1.0, 0.0), down=(0.0, 0.0, 1.0), forward=(1.0, 0.0, 0.0), pixel_size=0.25,
                                                 origin=(0.0, 0.0, 3.0)))


def test_a_view_along_a_tilted_direction():
    from thermo_nerf_amd.export import place_view, view_axes

    pos, temp, col, tri = R.quad_lattice(12, -3.0, 0.73, 11, jitter=0.2, depth=1.0)
    axes = view_axes((0.3, -0.5, 0.81), (0.1, 0.2, 1.0))
    q = pos.astype(D) @ np.stack(axes, axis=1)
    v = place_view(axes, q.min(axis=0), q.max(axis=0), pixel_size=0.211, margin_pixels=1)
    vw = R.view(v.width, v.height, v.origin, v.right, v.down, v.forward, v.pixel_size)
    want, got = check((pos, temp, col, tri), vw)
    assert want["counts"][0] > 0.3 * v.width * v.height and want["counts"][1] == len(tri)
    check((pos, temp, col, tri), dict(vw, cull=1))


# ---- many faces ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big():
    return R.big_scene()


@functools.lru_cache(maxsize=None)
def _big_want():
    return R.rasterize(*_big(), R.view(R.BIG_SIDE, R.BIG_SIDE))


def test_sixty_six_thousand_faces_on_three_hundred_pixels_square():
    scene, want = _big(), _big_want()
    assert len(scene[3]) >= 65537 + 338 and R.BIG_SIDE ** 2 > 256 * 256
    check(scene, R.view(R.BIG_SIDE, R.BIG_SIDE), want=want)
    fine = 2 * 182 * 182
    coarse_rows = np.flatnonzero(np.arange(len(scene[3])) % 191 == 190)[:338]
    shown = np.isin(want["pixel_face"], coarse_rows)
    assert 0.1 < shown.mean() < 0.9 and len(scene[3]) == fine + 338, "the large faces pass in front of the small ones and behind them"


def test_the_same_call_twice_and_the_face_list_reversed():
    scene, want, view = _big(), _big_want(), R.view(R.BIG_SIDE, R.BIG_SIDE)
    first, second = raw(scene, view), raw(scene, view)
    for name, buf in first["buffers"].items():
        assert torch.equal(buf, second["buffers"][name]), name
    assert first["counts"].tobytes() == second["counts"].tobytes() and first["stats"].tobytes() == second["stats"].tobytes()
    assert want["ties"] == 0, "the scene has no key tie: choose another seed"
    pos, temp, col, tri = scene
    back = images(raw((pos, temp, col, tri[::-1].copy()), view), view)
    mine = images(first, view)
    for name in ("pixel_depth", "pixel_temperature", "pixel_colors"):
        assert back[name].tobytes() == mine[name].tobytes(), name
    assert ((back["pixel_face"] >= 0) == (mine["pixel_face"] >= 0)).all()
    shown = mine["pixel_face"] >= 0
    assert (back["pixel_face"][shown] == len(tri) - 1 - mine["pixel_face"][shown]).all()
    assert back["stats"].tobytes() == mine["stats"].tobytes() and back["counts"].tobytes() == mine["counts"].tobytes()


# ---- absent outputs, empty meshes, the error codes -------------------------------------------------------------------------------------------

def test_each_output_absent_in_turn_and_no_colours():
    mesh, view = R.quad_lattice(12, 1.3125, 2.171875, 7, jitter=0.5), R.view(30, 30)
    want = R.rasterize(*mesh, view)
    for name in PIXELS:
        check(mesh, view, want=want, absent=(name,))
    check(mesh, view, want=want, absent=tuple(PIXELS))
    pos, temp, col, tri = mesh
    check((pos, temp, None, tri), view, want=dict(want, pixel_colors=None))


def test_no_vertices_and_no_triangles():
    lib = _hip.load()
    pos, temp, col, tri = R.quad_lattice(4, 1.0, 2.0, 5)
    view = R.view(11, 6)
    for v, t in ((0, 0), (0, 7), (9, 0)):
        colors = col[:v] if v else None  # (without a vertex there is no colour array to point to)
        want = R.rasterize(pos[:v], temp[:v], colors, tri[:t], view)
        assert want["counts"].tolist() == [0, 0, 0] and (want["pixel_face"] == -1).all()
        _, got = check((pos[:v], temp[:v], colors, tri[:t]), view, want=want)
        assert R.bits(got["stats"]).tolist() == R.bits(np.array([0.0, math.inf, -math.inf])).tolist()
        assert R.bits(got["pixel_depth"]).tolist() == [[R.NAN_BITS] * 11] * 6 and (v == 0 or (got["pixel_colors"] == 0).all())
    # and without a workspace
    counts, stats, face = _buffer(3, torch.int64), _buffer(3, torch.float64), _buffer(66, torch.int32)
    code = lib.tn_mesh_rasterize(None, None, None, None, 0, 0, _struct(view), face.data_ptr(), None, None, None, counts.data_ptr(),
                                 stats.data_ptr(), None, 0, _hip.current_stream())
    torch.cuda.synchronize()
    assert code == 0 and counts[:3].tolist() == [0, 0, 0] and bool((face[:66] == -1).all())
    _untouched(face, 66, "pixel_face")


def test_error_codes_with_nothing_written():
    lib = _hip.load()
    pos, temp, col, tri = R.quad_lattice(4, 1.0, 2.0, 5)
    v, t, view = len(pos), len(tri), R.view(11, 6)
    inputs = [_device(pos), _device(temp), _device(col), _device(tri)]
    outs = {k: _buffer(66 * n, dtype) for k, (dtype, n) in PIXELS.items()}
    counts, stats = _buffer(3, torch.int64), _buffer(3, torch.float64)
    need = mesh_rasterize_workspace_bytes(t, 11, 6)
    ws = _buffer(need, torch.uint8)
    good = dict(positions=inputs[0].data_ptr(), temperature=inputs[1].data_ptr(), colors=inputs[2].data_ptr(), triangles=inputs[3].data_ptr(),
                num_vertices=v, num_triangles=t, view=_struct(view), counts=counts.data_ptr(), stats=stats.data_ptr(), workspace=ws.data_ptr(),
                workspace_bytes=need, stream=_hip.current_stream(), **{k: b.data_ptr() for k, b in outs.items()})

    def call(view_change=None, **change):
        args = dict(good, **change)
        if view_change is not None:
            args["view"] = _struct(dict(view, **{k: x for k, x in view_change.items() if k != "reserved"}), view_change.get("reserved", 0))
        return lib.tn_mesh_rasterize(*[args[k] for k in NAMES])

    for k in ("positions", "temperature", "colors", "triangles", "view", "counts", "stats", "workspace"):
        assert call(**{k: None}) == -1, k  # TN_ERR_NULL
    limit = (2 ** 31 - 1) // 3
    assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2 and call(num_triangles=-1) == -2  # TN_ERR_SHAPE
    assert call(num_triangles=limit + 1) == -2
    for change in (dict(width=0), dict(width=16385), dict(height=0), dict(height=16385), dict(pixel_size=0.0), dict(pixel_size=-1.0),
                   dict(pixel_size=math.inf), dict(pixel_size=math.nan), dict(origin=(0.0, math.inf, 0.0)), dict(right=(math.nan, 0.0, 0.0)),
                   dict(down=(0.0, 0.0, -math.inf)), dict(forward=(0.0, math.nan, 1.0))):
        assert call(view_change=change) == -2, change
    for k in ("positions", "temperature", "triangles", "pixel_face", "pixel_depth", "pixel_temperature"):
        assert call(**{k: good[k] + 2}) == -2, k
    for k in ("counts", "stats", "workspace"):
        assert call(**{k: good[k] + 4}) == -2, k
    for change in (dict(near=math.nan), dict(far=math.nan), dict(cull=2), dict(cull=-1), dict(reserved=-1), dict(reserved=16385)):
        assert call(view_change=change) == -3, change  # TN_ERR_UNSUPPORTED
    assert call(workspace_bytes=need - 1) == -4 and call(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    assert lib.tn_mesh_rasterize_workspace_bytes(-1, 11, 6) == 0 and lib.tn_mesh_rasterize_workspace_bytes(limit + 1, 11, 6) == 0
    assert lib.tn_mesh_rasterize_workspace_bytes(t, 0, 6) == 0 and lib.tn_mesh_rasterize_workspace_bytes(t, 11, 16385) == 0
    assert lib.tn_mesh_rasterize_workspace_bytes(limit, 16384, 16384) > 8 * 16384 * 16384
    torch.cuda.synchronize()
    for name, buf in list(outs.items()) + [("counts", counts), ("stats", stats), ("workspace", ws)]:
        _untouched(buf, 0, name)
    assert call() == 0
    torch.cuda.synchronize()
    assert counts[:3].tolist() == R.rasterize(pos, temp, col, tri, view)["counts"].tolist()


# ---- the Python layer and the command line ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _regions_lattice():
    pos, tri = G.lattice(40, 40, G.LATTICE_SEED)
    return pos, G.lattice_temperature(pos, G.LATTICE_SEED), tri


def _lattice_mesh():
    pos, temp, tri = _regions_lattice()
    colors = np.random.default_rng(23).integers(0, 256, (len(pos), 3)).astype(np.uint8)
    return ThermalMesh(_device(pos), _device(colors), _device(temp), None, _device(tri), (14.0, 33.0)), colors


def test_mesh_thermogram_to_rgb8_world_position_and_region_map():
    pos, temp, tri = _regions_lattice()
    mesh, colors = _lattice_mesh()
    view = fit_view(mesh.positions, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), pixel_size=0.11)
    assert isinstance(view, RasterView) and view.forward == (0.0, 0.0, -1.0) and view.width <= 400
    vw = R.view(view.width, view.height, view.origin, view.right, view.down, view.forward, view.pixel_size, view.near, view.far, int(view.cull))
    want = R.rasterize(pos, temp, colors, tri, vw)
    found = mesh_thermogram(mesh, view)
    assert isinstance(found, Thermogram) and tuple(found.pixel_face.shape) == (view.height, view.width)
    for name in PIXELS:
        assert getattr(found, name).cpu().numpy().tobytes() == want[name].tobytes(), name
    covered = int(want["counts"][0])
    assert (found.covered, found.drawn_faces, found.usable_faces) == tuple(int(c) for c in want["counts"]) and covered > 0
    assert found.covered_area == covered * view.pixel_size ** 2 and found.mean_temperature == float(want["stats"][0]) / covered
    assert (found.min_temperature, found.max_temperature) == (float(want["stats"][1]), float(want["stats"][2]))
    assert abs(found.covered_area - 39.0 * 39.0) < 0.05 * 39.0 * 39.0, "the lattice is 39 x 39 units"
    # the thermal picture against the magma table on the host; the mesh's bounds, then given ones, then the image's own range
    magma = colormaps.table_u8("magma")
    t = want["pixel_temperature"]
    for bounds, (lo, hi) in ((None, (14.0, 33.0)), ((20.0, 26.0), (20.0, 26.0))):
        x = (t - F(lo)) / F(hi - lo)
        index = np.clip(np.nan_to_num(np.trunc(x * F(256.0)), nan=0.0), 0, 255).astype(np.int64)
        picture = np.where(np.isnan(t)[..., None], 0, magma[index]).astype(np.uint8)
        got = found.to_rgb8("thermal", bounds)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (view.height, view.width, 3) and got.cpu().numpy().tolist() == picture.tolist()
    assert bool((found.to_rgb8("thermal")[found.pixel_face < 0] == 0).all()) and bool((found.pixel_face[0] < 0).all()), "the margin is black"
    assert found.to_rgb8("rgb").cpu().numpy().tobytes() == want["pixel_colors"].tobytes()
    own = dataclasses.replace(found, temperature_bounds=None).to_rgb8()
    lo, hi = found.min_temperature, found.max_temperature
    index = np.clip(np.nan_to_num(np.trunc((t - F(lo)) / F(hi - lo) * F(256.0)), nan=0.0), 0, 255).astype(np.int64)
    assert own.cpu().numpy().tolist() == np.where(np.isnan(t)[..., None], 0, magma[index]).astype(np.uint8).tolist()
    # a pixel's world position lies on the face it shows
    rows, cols = np.nonzero(want["pixel_face"] >= 0)
    for k in (0, len(rows) // 3, len(rows) - 1):
        row, col = int(rows[k]), int(cols[k])
        p = np.array(found.world_position(row, col))
        a, b, c = (pos[i].astype(D) for i in tri[want["pixel_face"][row, col]])
        normal = np.cross(b - a, c - a)
        # The rasteriser snaps a vertex to 1/256 pixel along right and down (at most half of that per axis, sqrt(2) / 512 pixels in the
        # image plane) and keeps its depth: the pixel lies on the snapped face, which is that close to the true one at the most.  The
        # fp32 depth (2^-24 of a depth below 2) and the fp64 arithmetic here are far below it.
        assert abs(np.dot(p - a, normal)) / np.linalg.norm(normal) <= math.sqrt(2.0) / 512.0 * view.pixel_size + 1e-6, "on the face's plane"
        assert p[0] == view.origin[0] + (col + 0.5) * view.pixel_size * view.right[0] + (row + 0.5) * view.pixel_size * view.down[0] + \
            float(want["pixel_depth"][row, col]) * view.forward[0]
    assert all(math.isnan(c) for c in found.world_position(0, 0))
    # joined with the region table
    regions = thermal_regions(mesh, *G.LATTICE_WINDOW)
    region_want = G.regions(pos, temp, tri, *G.LATTICE_WINDOW)["face_region"]
    joined = found.region_map(regions).cpu().numpy()
    assert joined.dtype == np.int32 and joined.shape == want["pixel_face"].shape
    assert (joined == np.where(want["pixel_face"] >= 0, region_want[np.maximum(want["pixel_face"], 0)], -1)).all() and joined.max() > 50
    # the raw entry of the Python layer
    counts, stats = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    mesh_rasterize_into(mesh, view, counts=counts, stats=stats)
    assert counts.tolist() == want["counts"].tolist() and stats.cpu().numpy().tobytes() == want["stats"].tobytes()
    with pytest.raises(ValueError):
        mesh_rasterize_into(mesh, view, counts=counts, stats=stats, pixel_face=torch.empty(5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        mesh_rasterize_into(mesh, view, counts=counts, stats=stats, workspace=torch.empty((64,), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="pixel size of"):
        fit_view(mesh.positions, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), pixel_size=0.001)
    by_width = fit_view(mesh.positions, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), width=104, margin_pixels=2)
    assert by_width.width == 104 and abs(by_width.pixel_size - (pos[:, 0].max() - pos[:, 0].min()) / 100.0) < 1e-6


def test_command_line_end_to_end_on_a_small_ply(tmp_path, capsys):
    from PIL import Image

    spec = importlib.util.spec_from_file_location("mesh_thermogram_tool", os.path.join(ROOT, "tools", "mesh_thermogram.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pos, temp, tri = _regions_lattice()
    mesh, colors = _lattice_mesh()
    source = tmp_path / "lattice.ply"
    write_mesh_ply(source, mesh)
    png, npy, report_file = tmp_path / "out" / "t.png", tmp_path / "out" / "t.npy", tmp_path / "out" / "t.json"
    assert tool.main([str(source), "--view", "-z", "--pixel-size", "0.25", "--length-scale", "2", "--output", str(png), "--temperatures", str(npy),
                      "--report", str(report_file), "--device", DEV]) == 0
    printed = capsys.readouterr().out
    view = fit_view(mesh.positions, (0, 0, -1), (0, 1, 0), pixel_size=0.25)
    found = mesh_thermogram(mesh, view)
    picture = np.asarray(Image.open(png))
    assert picture.shape == (view.height, view.width, 3) and picture.tobytes() == found.to_rgb8("thermal").cpu().numpy().tobytes()
    saved = np.load(npy)
    assert saved.dtype == F and saved.tobytes() == found.pixel_temperature.cpu().numpy().tobytes() and np.isnan(saved[0, 0])
    report = json.loads(report_file.read_text())
    assert report["view"]["width"] == view.width and report["view"]["height"] == view.height and report["view"]["pixel_size"] == 0.5
    assert report["view"]["forward"] == [0.0, 0.0, -1.0] and report["view"]["near"] is None and report["length_scale"] == 2.0
    assert report["view"]["origin"] == [2.0 * c for c in view.origin]
    assert report["counts"] == {"vertices": len(pos), "faces": len(tri), "usable_faces": len(tri), "drawn_faces": found.drawn_faces,
                                "pixels": view.width * view.height, "covered_pixels": found.covered}
    assert report["covered_area"] == 4.0 * found.covered_area and report["mean_temperature"] == found.mean_temperature
    assert (report["min_temperature"], report["max_temperature"]) == (found.min_temperature, found.max_temperature)
    t = found.pixel_temperature.cpu().numpy()
    row, col = np.unravel_index(np.nanargmax(t), t.shape)
    hot = report["hottest_pixel"]
    assert (hot["row"], hot["column"], hot["temperature"]) == (int(row), int(col), found.max_temperature)
    assert hot["face"] == int(found.pixel_face[row, col]) and hot["position"] == [2.0 * c for c in found.world_position(row, col)]
    assert report["coldest_pixel"]["temperature"] == found.min_temperature
    assert printed.count("\n") == 1 and f"{view.width} x {view.height} pixels" in printed and f"{found.covered} covered" in printed
    # the file's colours, a slab, culling
    assert tool.main([str(source), "--forward", "0", "0", "-1", "--up", "0", "1", "0", "--width", "64", "--colors", "rgb", "--cull-back",
                      "--near", "0.1", "--far", "0.4", "--output", str(png), "--device", DEV]) == 0
    view = fit_view(mesh.positions, (0, 0, -1), (0, 1, 0), width=64, near=0.1, far=0.4, cull=True)
    found = mesh_thermogram(mesh, view)
    picture = np.asarray(Image.open(png))
    assert picture.shape[1] == 64 and picture.tobytes() == found.pixel_colors.cpu().numpy().tobytes() and 0 < found.covered < 64 * 64
