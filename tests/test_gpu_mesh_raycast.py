"""tn_mesh_bvh_build and tn_mesh_raycast on the device against tests/mesh_raycast_reference.py, exactly — every integer and every
float bit pattern, no tolerance anywhere — into guarded buffers with the inputs unchanged afterwards: the tree (sizes around the tile,
unusable faces, 300 copies of one triangle, a flat mesh, a point, a chain 25 deep, determinism, the invariants of ``tree()``), the
rays (unusable rays, zero and sub-normal direction components, origins inside and on the mesh, shared edges and vertices, t windows,
per-ray ends, culling, absent outputs, any-hit, sizes around the wave), a room of 26 400 faces under 300 x 300 camera rays and a
soup, the Python layer and the command line."""
from __future__ import annotations

import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_raycast_reference as R
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (CameraView, ThermalMesh, build_mesh_bvh, camera_rays, mesh_bvh_bytes, mesh_bvh_depth_bound,
                                    mesh_bvh_workspace_bytes, mesh_camera_thermogram, mesh_raycast, thermal_regions, visible_from,
                                    write_mesh_ply)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F, D = np.float32, np.float64
GUARD = 96  # elements behind every output buffer that must keep their pattern
FILLS = {torch.int32: -5, torch.float32: -777.0, torch.float64: -777.0, torch.uint8: 0xEE, torch.int64: -9}
OUT = {"hit_face": (torch.int32, 1), "hit_t": (torch.float32, 1), "hit_uv": (torch.float32, 2), "hit_temperature": (torch.float32, 1),
       "hit_colors": (torch.uint8, 3)}


def _buffer(elements, dtype):
    return torch.full((elements + GUARD,), FILLS[dtype], dtype=dtype, device=DEV)


def _untouched(buf, start, name):
    assert bool((buf[start:] == FILLS[buf.dtype]).all()), f"{name} was written at or beyond element {start}"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Scene:
    """a mesh on the device with its tree, built through the raw entry into guarded buffers"""

    def __init__(self, positions, temperature, colors, triangles):
        self.host = (np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(temperature, F).reshape(-1),
                     None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3),
                     np.ascontiguousarray(triangles, np.int32).reshape(-1, 3))
        self.v, self.t = len(self.host[0]), len(self.host[3])
        self.given = [a for a in self.host if a is not None]
        self.inputs = [_device(a) for a in self.given]
        self.pos, self.temp = self.inputs[0], self.inputs[1]
        self.col = self.inputs[2] if colors is not None else None
        self.tri = self.inputs[-1]
        self.blob, self.blob_bytes = self.build()

    def pointers(self):
        return (self.pos.data_ptr() if self.v else None, self.temp.data_ptr() if self.v else None, self.tri.data_ptr() if self.t else None)

    def build(self):
        need, work = mesh_bvh_bytes(self.t), mesh_bvh_workspace_bytes(self.t)
        assert need == 64 + (4 * self.t + 63) // 64 * 64 + 64 * max(self.t - 1, 0) and work % 8 == 0
        blob, workspace = _buffer(need, torch.uint8), _buffer(work, torch.uint8)
        p, t, tri = self.pointers()
        _hip.check(_hip.load().tn_mesh_bvh_build(p, t, tri, self.v, self.t, blob.data_ptr(), need, workspace.data_ptr() if self.t else None,
                                                 work, _hip.current_stream()), "tn_mesh_bvh_build")
        torch.cuda.synchronize()
        _untouched(blob, need, "the blob")
        _untouched(workspace, work, "the workspace")
        self.unchanged()
        return blob, need

    def unchanged(self):
        for before, now in zip(self.given, self.inputs):
            assert before.tobytes() == now.cpu().numpy().tobytes(), "an input was written"

    def bvh(self):
        mesh = ThermalMesh(self.pos, self.col, self.temp, None, self.tri)
        from thermo_nerf_amd.export import MeshBVH

        return MeshBVH(self.blob[:self.blob_bytes], self.v, self.t, mesh)

    def cast(self, origins, directions, ray_t_max=None, t_min=0.0, t_max=math.inf, cull=0, mode=R.CLOSEST, absent=()):
        """tn_mesh_raycast into guarded buffers (``absent``: the outputs passed as NULL): host copies of what was written"""
        origins, directions = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(directions, F).reshape(-1, 3)
        n = len(origins)
        rays = [_device(origins), _device(directions)] + ([_device(np.ascontiguousarray(ray_t_max, F))] if ray_t_max is not None else [])
        closest = mode == R.CLOSEST
        buffers = {k: None if (not closest or k in absent or (k == "hit_colors" and (self.col is None or not self.v))) else _buffer(n * width, dtype)
                   for k, (dtype, width) in OUT.items()}
        some = None if closest else _buffer(n, torch.uint8)
        counts = None if (not closest or "counts" in absent) else _buffer(4, torch.int64)
        stats = None if (not closest or "stats" in absent or buffers["hit_temperature"] is None) else _buffer(3, torch.float64)
        params = _hip.tn_raycast_params(t_min, t_max, cull, mode)
        p, t, tri = self.pointers()
        work = self.v > 0 and self.t > 0
        _hip.check(_hip.load().tn_mesh_raycast(
            p if work else None, t if work else None, _hip.ptr(self.col) if self.v else None, tri, self.v, self.t, self.blob.data_ptr(),
            self.blob_bytes, rays[0].data_ptr() if n else None, rays[1].data_ptr() if n else None, rays[2].data_ptr() if len(rays) > 2 and n else None,
            n, params, *[_hip.ptr(buffers[k]) for k in OUT], _hip.ptr(some), _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()),
            "tn_mesh_raycast")
        torch.cuda.synchronize()
        out = {}
        for name, buf in list(buffers.items()) + [("hit_any", some), ("counts", counts), ("stats", stats)]:
            if buf is None:
                out[name] = None
                continue
            width = OUT[name][1] if name in OUT else 1
            size = {"counts": 4, "stats": 3}.get(name, n * width)
            _untouched(buf, size, name)
            host = buf[:size].cpu().numpy()
            out[name] = host.reshape(n, width) if width > 1 else host
        self.unchanged()
        for before, now in zip((origins, directions), rays):
            assert before.tobytes() == now.cpu().numpy().tobytes(), "a ray was written"
        return out

    def reference(self, origins, directions, **kw):
        return R.raycast(*self.host, origins, directions, **kw)

    def check(self, origins, directions, want=None, absent=(), **kw):
        """one closest-hit call compared with the yardstick, bit for bit, on every output it was given; then the any-hit call"""
        want = self.reference(origins, directions, **kw) if want is None else want
        got = self.cast(origins, directions, absent=absent, **kw)
        _same(got, want)
        some = self.cast(origins, directions, mode=R.ANY, **kw)
        assert all(some[k] is None for k in OUT) and some["counts"] is None and some["stats"] is None
        assert some["hit_any"].tolist() == want["hit_any"].tolist() == (want["hit_face"] >= 0).astype(np.uint8).tolist()
        return want, got


def _same(got, want):
    if got["counts"] is not None:
        assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
        assert got["counts"][3] == 0, "a ray reached the stack limit"
    for name in OUT:
        if got[name] is not None:
            assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            differ = np.flatnonzero(np.ascontiguousarray(got[name]).view(np.uint8).reshape(-1) != np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1))
            assert len(differ) == 0, (name, len(differ), "first differing byte", int(differ[0]))
    if got["stats"] is not None:
        assert got["stats"].view(np.uint64).tolist() == want["stats"].view(np.uint64).tolist(), ("stats", got["stats"], want["stats"])


def check_tree(scene, min_depth=0):
    """the blob against the reference tree, and the invariants of ``tree()`` on their own"""
    want = R.tree(scene.host[0], scene.host[1], scene.host[3])
    got = scene.bvh().tree()
    for name in ("num_faces", "num_usable", "num_unusable", "num_nodes", "root", "depth"):
        assert got[name] == want[name], (name, got[name], want[name])
    assert R.bits(np.array(got["lo"], F)).tolist() == R.bits(want["lo"]).tolist() and R.bits(np.array(got["hi"], F)).tolist() == R.bits(want["hi"]).tolist()
    faces, child, level = got["faces"].cpu().numpy(), got["child"].cpu().numpy(), got["level"].cpu().numpy()
    lo, hi = got["box_lo"].cpu().numpy(), got["box_hi"].cpu().numpy()
    assert faces.tolist() == want["faces"].tolist() and child.tolist() == want["child"].tolist() and level.tolist() == want["level"].tolist()
    assert lo.tobytes() == want["box_lo"].tobytes() and hi.tobytes() == want["box_hi"].tobytes()
    u, n = got["num_usable"], got["num_nodes"]
    assert sorted(faces.tolist()) == list(range(scene.t)) and n == max(u - 1, 0) and got["num_unusable"] == scene.t - u
    assert min_depth <= got["depth"] <= mesh_bvh_depth_bound() == R.DEPTH_BOUND == 61
    usable = R.usable_faces(scene.host[0], scene.host[1], scene.host[3])
    assert sorted(faces[:u].tolist()) == np.flatnonzero(usable).tolist(), "the usable faces come first in the leaf order"
    if n:
        leaves = np.sort(~child[child < 0])
        inner = np.sort(child[child >= 0])
        assert leaves.tolist() == list(range(u)), "every usable face sits in exactly one leaf"
        assert inner.tolist() == list(range(1, n)), "every internal node but the root has exactly one parent"
        face_lo, face_hi = R.face_boxes(scene.host[0], scene.host[3], usable)
        for i in range(n):
            for c in range(2):
                ref = int(child[i, c])
                if ref < 0:
                    a, b = face_lo[faces[~ref]], face_hi[faces[~ref]]
                else:
                    a, b = R.min_ord(lo[ref, 0], lo[ref, 1]), R.max_ord(hi[ref, 0], hi[ref, 1])
                assert lo[i, c].tobytes() == a.tobytes() and hi[i, c].tobytes() == b.tobytes(), (i, c)
        assert got["depth"] == level[0] and (level >= 1).all()
    # everything behind the tree is zero, and a second build gives the same bytes
    blob = scene.blob[:scene.blob_bytes].cpu().numpy()
    faces_bytes = (4 * scene.t + 63) // 64 * 64
    assert not blob[64 + 4 * scene.t: 64 + faces_bytes].any() and not blob[64 + faces_bytes + 64 * n:].any()
    again, _ = scene.build()
    assert again[:scene.blob_bytes].cpu().numpy().tobytes() == blob.tobytes(), "two builds of one mesh differ"
    return got


def rays_at(scene_host, count, seed):
    """rays from around the mesh towards points near it"""
    pos = scene_host[0]
    finite = pos[np.isfinite(pos).all(axis=1)] if len(pos) else np.zeros((0, 3), F)
    lo, hi = (finite.min(axis=0), finite.max(axis=0)) if len(finite) else (np.zeros(3), np.ones(3))
    span = np.maximum(hi - lo, 1e-3)
    rng = np.random.default_rng(seed)
    origins = rng.uniform(lo - span, hi + span, (count, 3))
    targets = rng.uniform(lo, hi, (count, 3))
    return origins.astype(F), (targets - origins).astype(F)


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces", [0, 1, 2, 3, 5, 64, 65, 257])
def test_tree_sizes_around_the_tile(faces):
    pos, tri = R.soup(faces, 10 + faces)
    temp, col = R.attributes(len(pos), 1)
    scene = Scene(pos, temp, col, tri)
    got = check_tree(scene)
    assert got["num_usable"] == faces and got["root"] == (0 if faces >= 2 else (-1 if faces == 1 else R.NONE))
    o, d = rays_at(scene.host, 130, faces)
    want, _ = scene.check(o, d)
    assert faces < 3 or want["counts"][0] > 0


def test_tree_without_vertices_and_with_one_usable_face_among_unusable_ones():
    scene = Scene(np.zeros((0, 3), F), np.zeros(0, F), None, np.array([(0, 1, 2), (0, 0, 0)], np.int32))
    assert check_tree(scene)["num_usable"] == 0
    want, _ = scene.check(*rays_at(scene.host, 70, 1))
    assert want["counts"].tolist() == [0, 70, 0, 0]
    pos, tri = R.soup(40, 4)
    temp, col = R.attributes(len(pos), 2)
    tri = tri.copy()
    tri[:, 1] = tri[:, 0]          # not distinct
    tri[3] = (9, 10, 11)
    tri[5] = (0, 1, len(pos))      # out of range
    tri[6] = (-1, 1, 2)
    tri[7], tri[8] = (21, 22, 23), (24, 25, 26)
    pos, temp = pos.copy(), temp.copy()
    pos[22, 1] = np.inf            # face 7
    temp[25] = np.nan              # face 8
    scene = Scene(pos, temp, col, tri)
    got = check_tree(scene)
    assert got["num_usable"] == 1 and got["root"] == -1 and got["faces"][0].item() == 3 and got["depth"] == 0
    o, d = rays_at((pos[9:12],), 200, 3)
    want, _ = scene.check(o, d)
    assert 0 < want["counts"][0] and set(np.unique(want["hit_face"]).tolist()) == {-1, 3}


def test_three_hundred_copies_of_one_triangle():
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F)
    temp = np.array([10, 20, 30], F)
    tri = np.tile(np.array([(0, 1, 2)], np.int32), (300, 1))
    scene = Scene(pos, temp, None, tri)
    got = check_tree(scene)
    assert got["faces"].tolist() == list(range(300)) and 9 <= got["depth"] <= 31, "the tree comes from the index tie-break alone"
    o = np.array([(0.25, 0.25, 1), (0.25, 0.25, -1), (2, 2, 1), (0, 0, 1), (0.5, 0.5, 1)], F)
    d = np.array([(0, 0, -1), (0, 0, 2), (0, 0, -1), (0, 0, -1), (0, 0, -1)], F)
    want, _ = scene.check(o, d)
    assert want["hit_face"].tolist() == [0, 0, -1, 0, 0], "equal t: the lowest face index"
    assert want["hit_t"][[0, 1, 3, 4]].tolist() == [1.0, 0.5, 1.0, 1.0] and want["hit_temperature"][0] == 17.5


def test_flat_mesh_and_all_vertices_at_one_point():
    pos, tri = R.soup(90, 8)
    pos = pos.copy()
    pos[:, 2] = 0.625  # zero extent along z
    temp, col = R.attributes(len(pos), 3)
    scene = Scene(pos, temp, col, tri)
    got = check_tree(scene)
    assert got["lo"][2] == got["hi"][2] == 0.625
    o, d = rays_at(scene.host, 300, 5)
    o[:, 2], d[:, 2] = 2.0, -1.0
    o[:40, 2], d[:40, 2] = 0.625, 0.0  # in the mesh's plane: det == 0 for every face
    want, _ = scene.check(o, d)
    assert want["counts"][0] > 50 and (want["hit_face"][:40] == -1).all()
    point = np.full((30, 3), 0.375, F)
    scene = Scene(point, temp[:30], col[:30], np.arange(30, dtype=np.int32).reshape(-1, 3))
    got = check_tree(scene)
    assert got["num_usable"] == 10 and got["lo"] == got["hi"] == (0.375, 0.375, 0.375)
    want, _ = scene.check(np.array([(0.375, 0.375, 1)], F), np.array([(0, 0, -1)], F))
    assert want["hit_face"].tolist() == [-1], "a face without area has det == 0"


def deep_chain():
    """32 faces in the unit cube whose box centres quantise to 0, to one power of two on one axis (centres at 2^-k, k = 1 .. 10, on
    each axis in turn) and to (1023, 1023, 1023): their Morton codes are 0, the 30 single bits and 2^30 - 1 — sorted, a chain that
    loses one leaf per level"""
    s = 2.0 ** -14
    boxes = [((0.0, 0.0, 0.0), (2 * s, 2 * s, 2 * s)), ((1.0 - 2 * s,) * 3, (1.0, 1.0, 1.0))]
    for axis in range(3):
        for k in range(1, 11):
            lo, hi = [0.0, 0.0, 0.0], [2 * s, 2 * s, 2 * s]
            lo[axis], hi[axis] = 2.0 ** -k - s, 2.0 ** -k + s
            boxes.append((tuple(lo), tuple(hi)))
    pos = np.array([c for lo, hi in boxes for c in ((lo[0], lo[1], lo[2]), (hi[0], lo[1], hi[2]), (lo[0], hi[1], hi[2]))], F)
    return pos, np.arange(len(pos), dtype=np.int32).reshape(-1, 3)


def test_centres_at_powers_of_two_make_a_chain_of_depth_25_or_more():
    pos, tri = deep_chain()
    key = R.keys(pos, np.zeros(len(pos), F), tri)[0]
    assert sorted(key.tolist()) == [0] + [1 << b for b in range(30)] + [2 ** 30 - 1]
    temp, col = R.attributes(len(pos), 4)
    scene = Scene(pos, temp, col, tri)
    got = check_tree(scene, min_depth=25)
    assert got["depth"] <= mesh_bvh_depth_bound()
    o, d = rays_at(scene.host, 200, 6)
    targets = pos.reshape(-1, 3, 3).astype(D).mean(axis=1)
    o2 = np.tile(np.array([(0.7, 0.6, 0.9)], F), (len(targets), 1))
    want, _ = scene.check(np.concatenate([o, o2]), np.concatenate([d, (targets - o2).astype(F)]))
    assert want["counts"][0] >= 20


# ---- the rays ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cube():
    pos, tri = R.cube_lattice(4)
    temp, col = R.attributes(len(pos), 6)
    return Scene(pos, temp, col, tri)


def test_unusable_rays_and_special_directions():
    scene = cube()
    sub = np.float32(1e-42)
    o = np.array([(0.5, 0.5, 2), (0.5, 0.5, 2), (np.nan, 0.5, 2), (0.5, np.inf, 2), (0.5, 0.5, 2), (0.5, 0.5, 2),
                  (0.25, 0.5, 2), (1.0, 0.5, 2), (0.0, 0.0, 2), (0.5, 0.5, 2), (0.3, 0.3, 2), (1.0, 1.0, -3)], F)
    d = np.array([(0, 0, 0), (0, 0, -1), (0, 0, -1), (0, 0, -1), (np.nan, 0, -1), (0, -np.inf, -1),
                  (0, 0, -1), (0, 0, -1), (0, 0, -1), (sub, 0, -1), (sub, -sub, -1), (0, 0, 1)], F)
    want, _ = scene.check(o, d)
    assert want["counts"].tolist()[1] == 7 and want["hit_face"][[0, 2, 3, 4, 5]].tolist() == [-1] * 5
    assert want["hit_t"][1] == 1.0 and (want["hit_face"][[6, 7, 8, 9, 10, 11]] >= 0).all(), \
        "a zero direction component with the origin on a box plane, and a sub-normal one, still hit"
    assert R.bits(want["hit_t"][[0, 2]]).tolist() == [R.NAN_BITS] * 2 and R.bits(want["hit_uv"][0]).tolist() == [R.NAN_BITS] * 2


def test_origins_inside_and_on_the_mesh_and_rays_through_edges_and_vertices():
    scene = cube()
    o, d = R.lattice_rays(4)
    want, _ = scene.check(o, d)
    assert want["rejected"] == 0 and want["counts"][0] == want["counts"][1] == len(o)
    on = np.array([(0.5, 0.5, 1.0), (0.25, 0.25, 0.0), (1.0, 0.375, 0.625), (0.5, 0.5, 0.5)], F)
    towards = np.array([(0, 0, -1), (0.1, 0.2, 1), (-1, 0, 0), (1, 1, 1)], F)
    want, _ = scene.check(on, towards)
    assert want["hit_t"][:3].tolist() == [0.0, 0.0, 0.0] and want["hit_t"][3] == 0.5, "an origin on a face meets it at t = 0"
    want, _ = scene.check(on, towards, t_min=2.0 ** -20)
    assert (want["hit_t"][:3] > 0.5).all(), "the far side, once the window leaves the origin's own face out"


def test_windows_per_ray_ends_and_cull():
    scene = cube()
    o, d = rays_at(scene.host, 257, 9)
    full, _ = scene.check(o, d)
    assert full["counts"][0] == 257, "every ray aims at a point inside the cube"
    near = full["hit_t"].astype(D)
    cut, _ = scene.check(o, d, t_min=float(np.nanmedian(near)))
    assert 0 < cut["counts"][0] and (cut["hit_face"] != full["hit_face"]).sum() > 20, "the nearest hit is cut away: the next one shows"
    short, _ = scene.check(o, d, t_max=float(np.nanmedian(near)))
    assert 0 < short["counts"][0] < full["counts"][0]
    nothing, _ = scene.check(o, d, t_min=3.0, t_max=2.0)
    assert nothing["counts"].tolist() == [0, 257, scene.t, 0]
    ends = np.where(np.arange(257) % 3 == 0, np.nan_to_num(full["hit_t"], nan=1.0) * F(0.5), F(np.inf)).astype(F)
    ends[1], ends[2], ends[4] = np.nan, -1.0, np.nan_to_num(full["hit_t"][4], nan=1.0)
    own, _ = scene.check(o, d, ray_t_max=ends)
    hit = full["hit_face"] >= 0
    assert (own["hit_face"][::3][hit[::3]] == -1).all() and (own["hit_face"][1::3] == full["hit_face"][1::3]).all()
    assert own["hit_face"][4] == full["hit_face"][4], "t == t_end is inside the window"
    front, _ = scene.check(o, d, cull=1)
    outside = ((o < 0.0) | (o > 1.0)).any(axis=1)
    assert 200 < outside.sum() < 257 and (front["hit_face"][outside] == full["hit_face"][outside]).all(), \
        "from outside a closed mesh with outward normals the first hit is a front face"
    assert (front["hit_face"][~outside] == -1).all()
    inside = np.tile(np.array([(0.5, 0.5, 0.5)], F), (64, 1))
    away = rays_at(scene.host, 64, 2)[1]
    both, _ = scene.check(inside, away)
    back, _ = scene.check(inside, away, cull=1)
    assert both["counts"][0] == 64 and back["counts"][0] == 0, "from inside every face is seen from behind"


@pytest.mark.parametrize("rays", [0, 1, 63, 64, 65])
def test_ray_counts_around_the_wave_and_absent_outputs(rays):
    scene = cube()
    o, d = rays_at(scene.host, rays, 20 + rays)
    want, _ = scene.check(o, d)
    for absent in (("hit_face", "hit_uv"), ("hit_t", "hit_temperature", "hit_colors"), ("counts",), ("stats",),
                   ("hit_face", "hit_t", "hit_uv", "hit_temperature", "hit_colors", "counts", "stats")):
        got = scene.cast(o, d, absent=absent)
        assert all(got[k] is None for k in absent)
        _same(got, want)


def test_error_codes_on_the_device_and_a_foreign_blob():
    scene = cube()
    o, d = rays_at(scene.host, 64, 1)
    good = scene.blob.clone()
    try:
        scene.blob[:4] = 0  # no magic: a tree without a face
        got = scene.cast(o, d)
        assert got["counts"].tolist() == [0, 64, 0, 0] and (got["hit_face"] == -1).all()
        scene.blob.copy_(good)
        nodes = scene.blob[64 + (4 * scene.t + 63) // 64 * 64: scene.blob_bytes].view(torch.int32).reshape(-1, 16)
        nodes[:, 12] = 2 ** 30      # child 0 of every node: beyond the tree
        nodes[:, 13] = 0            # child 1: the root again, a cycle
        got = scene.cast(o, d)      # other numbers, no fault, and it ends
        assert (got["hit_face"] == -1).all()
        scene.blob.copy_(good)
        faces = scene.blob[64: 64 + 4 * scene.t].view(torch.int32)
        faces[:] = 2 ** 30
        assert (scene.cast(o, d)["hit_face"] == -1).all()
    finally:
        scene.blob.copy_(good)
    _same(scene.cast(o, d), scene.reference(o, d))


# ---- the larger scenes --------------------------------------------------------------------------------------------------------------------

def test_device_reference_is_the_numpy_reference():
    pos, tri = R.soup(400, 12)
    temp, col = R.attributes(len(pos), 7)
    o, d = R.soup_rays(1500, 13)
    host = R.raycast(pos, temp, col, tri, o, d, cull=1, t_min=0.125)
    device = R.raycast(pos, temp, col, tri, o, d, cull=1, t_min=0.125, torch_device=DEV, chunk=512)
    for name in R.OUTPUTS + ("counts", "stats"):
        assert host[name].tobytes() == device[name].tobytes(), name
    assert host["rejected"] == device["rejected"] == 0


def test_room_of_26400_faces_under_300_x_300_camera_rays():
    pos, tri = R.room()
    temp, col = R.attributes(len(pos), 8)
    assert len(tri) == 26400
    scene = Scene(pos, temp, col, tri)
    tree = scene.bvh().tree()
    assert tree["num_usable"] == len(tri) and 15 <= tree["depth"] <= 61
    camera = CameraView(R.look_at((5.5, 3.6, 2.4), (1.5, 1.0, 0.4)), 150.0, 150.0, 150.0, 150.0, 300, 300)
    o, d = (x.cpu().numpy() for x in camera_rays(camera, DEV))
    want = R.raycast(*scene.host, o, d, torch_device=DEV, chunk=2048)
    share = want["counts"][0] / len(o)
    assert want["rejected"] == 0 and 0.2 <= share <= 1.0 and want["counts"][0] == 90000, "a closed room: every ray from inside hits"
    assert len(np.unique(want["hit_face"])) > 3000
    _same(scene.cast(o, d), want)
    some = scene.cast(o, d, mode=R.ANY)
    assert some["hit_any"].tolist() == want["hit_any"].tolist()
    culled = R.raycast(*scene.host, o, d, cull=1, torch_device=DEV, chunk=2048)
    assert 0.2 <= culled["counts"][0] / len(o) <= 1.0 and culled["rejected"] == 0
    _same(scene.cast(o, d, cull=1), culled)


def test_soup_of_6000_faces_with_half_the_rays_hitting():
    pos, tri = R.soup(6000, 21, size=0.02)
    temp, col = R.attributes(len(pos), 9)
    o, d = R.soup_rays(20000, 22)
    want = R.raycast(pos, temp, col, tri, o, d, torch_device=DEV, chunk=4096)
    share = want["counts"][0] / len(o)
    assert want["rejected"] == 0 and 0.2 <= share <= 0.8, share
    scene = Scene(pos, temp, col, tri)
    _same(scene.cast(o, d), want)
    assert scene.cast(o, d, mode=R.ANY)["hit_any"].tolist() == want["hit_any"].tolist()


# ---- the Python layer and the command line ------------------------------------------------------------------------------------------------

def _small_room():
    pos, tri = R.room(cells=6, boxes=2, box_cells=3, seed=5)
    temp, col = R.attributes(len(pos), 10)
    mesh = ThermalMesh(_device(pos), _device(col), _device(temp), None, _device(tri), (10.0, 35.0))
    return (pos, temp, col, tri), mesh


def test_python_layer_camera_thermogram_visibility_and_region_map():
    host, mesh = _small_room()
    bvh = build_mesh_bvh(mesh)
    assert bvh.tree()["num_usable"] == len(host[3])
    camera = CameraView(R.look_at((5.5, 3.6, 2.4), (1.5, 1.0, 0.4)), 40.0, 40.0, 33.0, 20.5, 66, 41)
    found = mesh_camera_thermogram(bvh, camera)
    o, d = found.origins.cpu().numpy(), found.directions.cpu().numpy()
    assert np.abs(np.linalg.norm(d.astype(D), axis=1) - 1.0).max() < 1e-6 and np.abs(R.camera_rays(camera.matrix(), 40.0, 40.0, 33.0, 20.5, 66, 41)[1] - d).max() < 1e-5
    want = R.raycast(*host, o, d)
    assert found.pixel_face.cpu().numpy().reshape(-1).tolist() == want["hit_face"].tolist() and found.covered == want["counts"][0] == 66 * 41
    assert found.pixel_distance.cpu().numpy().tobytes() == want["hit_t"].tobytes()
    assert found.pixel_temperature.cpu().numpy().tobytes() == want["hit_temperature"].tobytes()
    assert found.pixel_colors.cpu().numpy().tobytes() == want["hit_colors"].tobytes()
    assert (found.min_temperature, found.max_temperature) == (want["stats"][1], want["stats"][2]) and found.stack_limit_rays == 0
    assert found.mean_temperature == want["stats"][0] / want["counts"][0] and found.usable_faces == len(host[3])
    rgb = found.to_rgb8()
    assert rgb.shape == (41, 66, 3) and rgb.dtype == torch.uint8 and int(rgb.max()) > 0 and found.to_rgb8("rgb") is found.pixel_colors
    where = np.array(found.world_position(20, 33))
    face = host[3][want["hit_face"][20 * 66 + 33]]
    normal = np.cross(host[0][face[1]].astype(D) - host[0][face[0]], host[0][face[2]].astype(D) - host[0][face[0]])
    assert abs(np.dot(where - host[0][face[0]], normal / np.linalg.norm(normal))) < 1e-5, "the position lies in the face's plane"
    hits = mesh_raycast(bvh, found.origins, found.directions, cull=True)
    assert hits.hits == R.raycast(*host, o, d, cull=1)["counts"][0] and hits.usable_rays == len(o)
    # visibility: the surface points the camera shows are visible from it; seen from beyond the walls behind the camera, the walls hide them
    points = hits.positions(found.origins, found.directions)
    seen = visible_from(bvh, points, (5.5, 3.6, 2.4))
    shown = hits.hit_face >= 0
    assert seen.dtype == torch.bool and bool(seen[shown].all())
    ends = np.full(len(o), 1.0 - 2.0 ** -10, F)
    eye = np.array((9.0, 7.0, 1.0), F)
    direction = points.cpu().numpy() - eye
    hidden = R.raycast(*host, np.tile(eye, (len(o), 1)), direction, ray_t_max=ends)["hit_any"] == 1
    got = visible_from(bvh, points, tuple(eye.tolist())).cpu().numpy()
    assert (got == ~hidden).all() and hidden[shown.cpu().numpy()].mean() > 0.9
    regions = thermal_regions(mesh, min_temperature=25.0)
    labels = found.region_map(regions)
    assert labels.shape == (41, 66) and (labels.cpu().numpy().reshape(-1) == regions.face_region.cpu().numpy()[want["hit_face"]]).all()
    # any_hit through the wrapper, and a tree that belongs to another mesh
    assert mesh_raycast(bvh, found.origins, found.directions, any_hit=True).hits == 66 * 41
    other = ThermalMesh(mesh.positions, mesh.colors, mesh.temperature, None, mesh.triangles[:-1].contiguous())
    import dataclasses

    with pytest.raises(ValueError, match="another mesh"):
        mesh_raycast(dataclasses.replace(bvh, mesh=other), found.origins, found.directions)


def test_command_line_on_a_small_ply(tmp_path, capsys):
    host, mesh = _small_room()
    ply = tmp_path / "room.ply"
    write_mesh_ply(ply, mesh)
    c2w = np.concatenate([R.look_at((5.5, 3.6, 2.4), (1.5, 1.0, 0.4)).astype(D), [[0, 0, 0, 1]]]).tolist()
    transforms = {"fl_x": 80.0, "fl_y": 80.0, "cx": 66.0, "cy": 41.0, "w": 132, "h": 82,
                  "frames": [{"file_path": "images/b.png", "transform_matrix": np.eye(4).tolist()},
                             {"file_path": "images/a.png", "transform_matrix": c2w}]}
    (tmp_path / "transforms.json").write_text(json.dumps(transforms))
    spec = importlib.util.spec_from_file_location("mesh_camera_view_tool", os.path.join(ROOT, "tools", "mesh_camera_view.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, report, temps = tmp_path / "view.png", tmp_path / "view.json", tmp_path / "t.npy"
    assert tool.main([str(ply), "--transforms", str(tmp_path / "transforms.json"), "--frame", "a.png", "--scale", "0.5", "--output", str(out),
                      "--temperatures", str(temps), "--report", str(report), "--probe", "20", "33", "--probe", "0", "0"]) == 0
    printed = capsys.readouterr().out
    from PIL import Image

    assert np.asarray(Image.open(out)).shape == (41, 66, 3)
    camera = CameraView(np.array(c2w)[:3], 40.0, 40.0, 33.0, 20.5, 66, 41)
    o, d = (x.cpu().numpy() for x in camera_rays(camera, DEV))
    from thermo_nerf_amd.export import read_mesh_ply

    data = read_mesh_ply(ply)
    want = R.raycast(data["positions"], data["temperature"], data["colors"], data["triangles"], o, d)
    assert np.load(temps).tobytes() == want["hit_temperature"].tobytes()
    found = json.loads(report.read_text())
    assert found["counts"]["covered_pixels"] == 66 * 41 and found["counts"]["faces"] == len(host[3]) and found["covered_share"] == 1.0
    assert found["camera"]["width"] == 66 and found["camera"]["fx"] == 40.0 and found["frame"] == "images/a.png"
    hottest = found["hottest_pixel"]
    assert hottest["temperature"] == float(np.nanmax(want["hit_temperature"])) and hottest["face"] == int(want["hit_face"][hottest["row"] * 66 + hottest["column"]])
    assert "probe (20, 33)" in printed and f"face {int(want['hit_face'][20 * 66 + 33])}" in printed and "probe (0, 0)" in printed
