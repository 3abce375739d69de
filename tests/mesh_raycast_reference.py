"""The yardstick of the ray caster: include/thermonerf_hip.h's definition of ``tn_mesh_raycast`` as brute force in fp64, every ray
against every face, with no tree — and a plain reference for the tree of ``tn_mesh_bvh_build`` (keys, leaf order, Karras's nodes).

``raycast`` is written once over an array namespace: numpy on the host, or torch with fp64 tensors where the caller has a device
(the large scenes: 90 000 rays x 20 000 faces are 1.8e9 pairs, the host loops over chunks of rays).  Every step is one add, sub, mul
or div of fp64 arrays, which both round correctly and neither contracts; the device tests compare the two on a small scene first."""
from __future__ import annotations

import math

import numpy as np

F, D = np.float32, np.float64
NAN_BITS = 0x7FC00000
SLACK = 1.0 - 2.0 ** -32
CLOSEST, ANY = 0, 1
DEPTH_BOUND = 61
NONE = -2 ** 31


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def ord32(x):
    """the order-preserving map of fp32 bits to uint32: -0.0 below +0.0"""
    b = bits(x)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def min_ord(a, b):
    return np.where(ord32(b) < ord32(a), b, a).astype(F)


def max_ord(a, b):
    return np.where(ord32(b) > ord32(a), b, a).astype(F)


def usable_faces(positions, temperature, triangles):
    """bool [T]"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    v = len(positions)
    ok = ((tri >= 0) & (tri < v)).all(axis=1)
    ok &= (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    safe = np.where(ok[:, None], tri, 0)
    if v:
        ok &= np.isfinite(np.asarray(positions, F)[safe]).all(axis=(1, 2)) & np.isfinite(np.asarray(temperature, F)[safe]).all(axis=1)
    return ok


def face_boxes(positions, triangles, usable):
    """(lo, hi) float32 [T, 3]; zeros for a face that is not usable"""
    tri = np.where(usable[:, None], np.asarray(triangles, np.int64).reshape(-1, 3), 0)
    if not len(positions):
        return np.zeros((len(tri), 3), F), np.zeros((len(tri), 3), F)
    p = np.asarray(positions, F)[tri]  # [T, 3 corners, 3]
    lo = min_ord(min_ord(p[:, 0], p[:, 1]), p[:, 2])
    hi = max_ord(max_ord(p[:, 0], p[:, 1]), p[:, 2])
    return np.where(usable[:, None], lo, 0).astype(F), np.where(usable[:, None], hi, 0).astype(F)


# ---- the slab and the face test over an array namespace -----------------------------------------------------------------------------

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def slab(xp, o, d, inv, lo, hi, t_min, t_end):
    """(passes, s, exit) of rays (lists of three arrays o, d, inv) against boxes (lists lo, hi), broadcasting"""
    enter, exit_ = t_min, t_end
    ok = None
    for k in range(3):
        zero = d[k] == 0.0
        a, b = (lo[k] - o[k]) * inv[k], (hi[k] - o[k]) * inv[k]
        near, far = xp.minimum(a, b), xp.maximum(a, b)  # (of a zero axis: not used)
        enter = xp.where(~zero & (near > enter), near, enter)
        exit_ = xp.where(~zero & (far < exit_), far, exit_)
        axis = ~zero | ((lo[k] <= o[k]) & (o[k] <= hi[k]))
        ok = axis if ok is None else ok & axis
    s = enter * SLACK
    return ok & (s <= exit_), s, exit_


def _pairs(xp, o, d, inv, t_min, t_end, p0, e1, e2, lo, hi, usable, cull, good):
    """(hit [R, F], t, u, v, rejected): every ray against every face; ``good`` [R, 1]: the usable rays"""
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    tv = [o[k] - p0[k] for k in range(3)]
    u = _dot(tv, pv) / det
    qv = _cross(tv, e1)
    v = _dot(d, qv) / det
    t = _dot(e2, qv) / det
    ok = usable & good & (det != 0.0)
    if cull:
        ok = ok & ~(det < 0.0)
    mt = ok & (u >= 0.0) & (v >= 0.0) & ((u + v) <= 1.0) & (t_min <= t) & (t <= t_end)
    passes, s, _ = slab(xp, o, d, inv, lo, hi, t_min, t_end)
    boxed = passes & (s <= t)
    return mt & boxed, t, u, v, int((mt & ~boxed).sum())


def raycast(positions, temperature, colors, triangles, origins, directions, ray_t_max=None, t_min=0.0, t_max=math.inf, cull=0,
            chunk=4096, torch_device=None):
    """The definition.  A dict of ``hit_face`` int32 [N], ``hit_t``, ``hit_temperature`` float32 [N], ``hit_uv`` float32 [N, 2],
    ``hit_colors`` uint8 [N, 3] (None without colors), ``hit_any`` uint8 [N], ``counts`` int64 [4], ``stats`` float64 [3], and
    ``rejected``: the ray-face pairs that passed Moeller-Trumbore and the t window and were dropped by the box clause alone."""
    positions, temperature = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    origins, directions = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    n, faces = len(origins), len(tri)
    usable = usable_faces(positions, temperature, tri)
    lo32, hi32 = face_boxes(positions, tri, usable)
    safe = np.where(usable[:, None], tri.astype(np.int64), 0)
    corner = positions[safe].astype(D) if len(positions) else np.zeros((faces, 3, 3), D)
    good = np.isfinite(origins).all(axis=1) & np.isfinite(directions).all(axis=1) & (directions != 0).any(axis=1)
    t_end = np.full(n, t_max, D)
    if ray_t_max is not None:
        own = np.asarray(ray_t_max, F).astype(D)
        t_end = np.where(own < t_max, own, t_max)
    if torch_device is not None:
        import torch

        xp = torch

        def arr(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(torch_device)
    else:
        xp, arr = np, (lambda x: x)
    p0 = [arr(corner[None, :, 0, k]) for k in range(3)]
    e1 = [arr(corner[None, :, 1, k] - corner[None, :, 0, k]) for k in range(3)]
    e2 = [arr(corner[None, :, 2, k] - corner[None, :, 0, k]) for k in range(3)]
    lo, hi = [arr(lo32[None, :, k].astype(D)) for k in range(3)], [arr(hi32[None, :, k].astype(D)) for k in range(3)]
    use = arr(usable[None, :])
    face = np.full(n, -1, np.int32)
    best = np.zeros((n, 3), D)  # t, u, v
    rejected = 0
    with np.errstate(all="ignore"):
        for first in range(0, n if faces else 0, chunk):
            rows = slice(first, min(first + chunk, n))
            safe_o = np.where(good[rows, None], origins[rows], 0).astype(D)
            safe_d = np.where(good[rows, None], directions[rows], 1).astype(D)
            o, d = [arr(safe_o[:, k:k + 1]) for k in range(3)], [arr(safe_d[:, k:k + 1]) for k in range(3)]
            inv = [1.0 / x for x in d]
            end = arr(t_end[rows, None])
            hit, t, u, v, dropped = _pairs(xp, o, d, inv, t_min, end, p0, e1, e2, lo, hi, use, cull, arr(good[rows, None]))
            if xp is np:
                masked = np.where(hit, t, np.inf)
                tbest = masked.min(axis=1, keepdims=True)
                first_of = np.argmax(hit & (masked == tbest), axis=1)
                some = hit.any(axis=1)
                pick = (np.arange(len(first_of)), first_of)
                values = np.stack([t[pick], u[pick], v[pick]], axis=1)
            else:
                masked = torch.where(hit, t, torch.full_like(t, math.inf))
                tbest = masked.amin(dim=1, keepdim=True)
                first_of = torch.argmax((hit & (masked == tbest)).to(torch.int8), dim=1)
                some = hit.any(dim=1).cpu().numpy()
                at = first_of[:, None]
                values = torch.cat([t.gather(1, at), u.gather(1, at), v.gather(1, at)], dim=1).cpu().numpy()
                first_of = first_of.cpu().numpy()
            rejected += dropped
            face[rows] = np.where(some, first_of, -1)
            best[rows] = np.where(some[:, None], values, 0.0)
    return finish(positions, temperature, colors, tri, usable, good, face, best, rejected)


def sum2(values):
    """the ordered sum in blocks of 256 (tn_mesh_regions' SUM2)"""
    total = 0.0
    values = np.asarray(values, D)
    for first in range(0, len(values), 256):
        part = 0.0
        for x in values[first:first + 256].tolist():
            part += x
        total += part
    return total


def finish(positions, temperature, colors, tri, usable, good, face, best, rejected):
    n = len(face)
    hit = face >= 0
    t, u, v = best[:, 0], best[:, 1], best[:, 2]
    nan = np.uint32(NAN_BITS).view(F)
    corner = np.where(hit[:, None], tri[np.where(hit, face, 0)] if len(tri) else np.zeros((n, 3), np.int32), 0).astype(np.int64)
    out = {"hit_face": face.astype(np.int32), "hit_any": hit.astype(np.uint8), "rejected": rejected}
    out["hit_t"] = np.where(hit, t.astype(F), nan).astype(F)
    out["hit_uv"] = np.where(hit[:, None], np.stack([u, v], axis=1).astype(F), nan).astype(F)
    w = (1.0 - u) - v
    if len(positions):
        temp = temperature.astype(D)[corner]
        blend = (w * temp[:, 0] + u * temp[:, 1]) + v * temp[:, 2]
    else:
        blend = np.zeros(n, D)
    with np.errstate(all="ignore"):
        out["hit_temperature"] = np.where(hit, blend.astype(F), nan).astype(F)
    out["hit_colors"] = None
    if colors is not None:
        c = np.asarray(colors, np.uint8).reshape(-1, 3).astype(D)[corner] if len(positions) else np.zeros((n, 3, 3), D)
        mixed = (w[:, None] * c[:, 0] + u[:, None] * c[:, 1]) + v[:, None] * c[:, 2]
        out["hit_colors"] = np.where(hit[:, None], np.clip(np.floor(mixed + 0.5), 0.0, 255.0), 0.0).astype(np.uint8)
    out["counts"] = np.array([int(hit.sum()), int(good.sum()), int(usable.sum()), 0], np.int64)
    shown = out["hit_temperature"][hit]
    low = shown[np.argmin(ord32(shown))] if hit.any() else math.inf
    high = shown[np.argmax(ord32(shown))] if hit.any() else -math.inf
    out["stats"] = np.array([sum2(np.where(hit, out["hit_temperature"].astype(D), 0.0)), low, high], D)
    return out


OUTPUTS = ("hit_face", "hit_t", "hit_uv", "hit_temperature", "hit_colors")


# ---- the tree -----------------------------------------------------------------------------------------------------------------------

def spread3(x):
    x = np.asarray(x, np.uint32) & np.uint32(0x3FF)
    x = (x | x << np.uint32(16)) & np.uint32(0x030000FF)
    x = (x | x << np.uint32(8)) & np.uint32(0x0300F00F)
    x = (x | x << np.uint32(4)) & np.uint32(0x030C30C3)
    x = (x | x << np.uint32(2)) & np.uint32(0x09249249)
    return x


def keys(positions, temperature, triangles):
    """(uint32 key [T], usable [T], extent lo [3], extent hi [3])"""
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    usable = usable_faces(positions, temperature, tri)
    lo, hi = face_boxes(positions, tri, usable)
    if not usable.any():
        return np.full(len(tri), 1 << 30, np.uint32), usable, np.full(3, math.inf, F), np.full(3, -math.inf, F)
    e0 = np.array([lo[usable][np.argmin(ord32(lo[usable][:, k])), k] for k in range(3)], F)
    e1 = np.array([hi[usable][np.argmax(ord32(hi[usable][:, k])), k] for k in range(3)], F)
    centre = (lo.astype(D) + hi.astype(D)) * 0.5
    width = e1.astype(D) - e0.astype(D)
    with np.errstate(all="ignore"):
        q = np.floor((centre - e0.astype(D)) / width * 1024.0)
    q = np.where(width > 0.0, np.clip(q, 0.0, 1023.0), 0.0).astype(np.uint32)
    code = spread3(q[:, 0]) << np.uint32(2) | spread3(q[:, 1]) << np.uint32(1) | spread3(q[:, 2])
    return np.where(usable, code, np.uint32(1 << 30)).astype(np.uint32), usable, e0, e1


def _clz32(x):
    return 32 - int(x).bit_length()


def tree(positions, temperature, triangles):
    """the blob's content as a dict: ``num_usable``, ``root``, ``depth``, ``lo`` / ``hi`` (the extent), ``faces`` int32 [T] (the leaf
    order), ``child`` int32 [U - 1, 2], ``level`` int32 [U - 1], ``box_lo`` / ``box_hi`` float32 [U - 1, 2, 3]"""
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    key, usable, e0, e1 = keys(positions, temperature, tri)
    order = np.argsort(key, kind="stable").astype(np.int32)
    code = key[order].tolist()
    n = int(usable.sum())
    lo, hi = face_boxes(positions, tri, usable)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        return _clz32(code[i] ^ code[j]) if code[i] != code[j] else 32 + _clz32(i ^ j)

    nodes = max(n - 1, 0)
    child = np.zeros((nodes, 2), np.int32)
    for i in range(nodes):
        d = 1 if delta(i, i + 1) > delta(i, i - 1) else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        length, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (length + t) * d) > dmin:
                length += t
            t //= 2
        j = i + length * d
        dnode = delta(i, j)
        s, t = 0, length
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        split = i + s * d + min(d, 0)
        first, last = min(i, j), max(i, j)
        child[i, 0] = ~split if first == split else split
        child[i, 1] = ~(split + 1) if last == split + 1 else split + 1
    level = np.zeros(nodes, np.int32)
    box_lo, box_hi = np.zeros((nodes, 2, 3), F), np.zeros((nodes, 2, 3), F)
    if nodes:
        todo, seen = [0], []
        while todo:  # parents before children
            i = todo.pop()
            seen.append(i)
            todo.extend(int(c) for c in child[i] if c >= 0)
        for i in reversed(seen):
            below = 0
            for c in range(2):
                ref = int(child[i, c])
                if ref < 0:
                    box_lo[i, c], box_hi[i, c] = lo[order[~ref]], hi[order[~ref]]
                else:
                    box_lo[i, c], box_hi[i, c] = min_ord(box_lo[ref, 0], box_lo[ref, 1]), max_ord(box_hi[ref, 0], box_hi[ref, 1])
                    below = max(below, int(level[ref]))
            level[i] = below + 1
    root = 0 if n >= 2 else (-1 if n == 1 else NONE)
    return {"num_faces": len(tri), "num_usable": n, "num_unusable": len(tri) - n, "num_nodes": nodes, "root": root,
            "depth": int(level[0]) if nodes else 0, "lo": e0, "hi": e1, "faces": order, "child": child, "level": level, "box_lo": box_lo,
            "box_hi": box_hi}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

def attributes(num_vertices, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(10.0, 35.0, num_vertices).astype(F), rng.integers(0, 256, (num_vertices, 3)).astype(np.uint8)


def box_mesh(lo, hi, cells, inward=False):
    """the six faces of an axis-aligned box, each a lattice of ``cells`` x ``cells`` quads of two triangles: (positions, triangles);
    normals point out, or in with ``inward``"""
    lo, hi = np.asarray(lo, D), np.asarray(hi, D)
    positions, triangles = [], []
    for axis in range(3):
        for side in range(2):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            g = np.linspace(0.0, 1.0, cells + 1)
            ga, gb = np.meshgrid(g, g, indexing="ij")
            p = np.zeros((cells + 1, cells + 1, 3), D)
            p[..., axis] = hi[axis] if side else lo[axis]
            p[..., a] = lo[a] + ga * (hi[a] - lo[a])
            p[..., b] = lo[b] + gb * (hi[b] - lo[b])
            base = sum(len(x) for x in positions)
            positions.append(p.reshape(-1, 3))
            i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
            v00 = base + i * (cells + 1) + j
            v10, v01, v11 = v00 + cells + 1, v00 + 1, v00 + cells + 2
            quads = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], -2).reshape(-1, 3)
            if bool(side) == bool(inward):
                quads = quads[:, [0, 2, 1]]
            triangles.append(quads)
    return np.concatenate(positions).astype(F), np.concatenate(triangles).astype(np.int32)


def join(*meshes):
    positions, triangles, base = [], [], 0
    for p, t in meshes:
        positions.append(p)
        triangles.append(t + base)
        base += len(p)
    return np.concatenate(positions).astype(F), np.concatenate(triangles).astype(np.int32)


def cube_lattice(cells=4):
    """an axis-aligned unit cube of ``cells``^2 quads per side: every box of its tree is flat along one axis"""
    return box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), cells)


def lattice_rays(cells=4):
    """rays at the cube lattice through its vertices, its edge midpoints and along its axes, from outside and from the centre"""
    g = np.linspace(0.0, 1.0, 2 * cells + 1)  # vertices and edge midpoints
    targets = np.array([(x, y, z) for x in g for y in g for z in g if min(x, y, z) == 0.0 or max(x, y, z) == 1.0], D)
    eyes = np.array([(0.5, 0.5, 0.5), (3.0, 0.5, 0.5), (0.5, -2.0, 0.5), (0.5, 0.5, 4.0), (2.0, 2.0, 2.0), (-1.0, 0.25, 0.75)], D)
    origins = np.repeat(eyes, len(targets), axis=0)
    directions = np.tile(targets, (len(eyes), 1)) - origins
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    along_o = np.array([(x, y, z) for x in g[::2] for y in g[::2] for z in (-1.0,)], D)
    extra_o = np.concatenate([along_o, along_o[:, [2, 0, 1]], along_o[:, [1, 2, 0]]])
    extra_d = np.concatenate([np.tile(axes[2], (len(along_o), 1)), np.tile(axes[0], (len(along_o), 1)), np.tile(axes[1], (len(along_o), 1))])
    return np.concatenate([origins, extra_o]).astype(F), np.concatenate([directions, extra_d]).astype(F)


def soup(num_faces, seed, size=0.35):
    """random triangles in the unit cube: (positions, triangles)"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.0, 1.0, (num_faces, 1, 3))
    positions = (centre + rng.uniform(-size, size, (num_faces, 3, 3))).reshape(-1, 3).astype(F)
    return positions, np.arange(3 * num_faces, dtype=np.int32).reshape(-1, 3)


def soup_rays(num_rays, seed):
    rng = np.random.default_rng(seed)
    origins = rng.uniform(-0.5, 1.5, (num_rays, 3))
    return origins.astype(F), (rng.uniform(0.0, 1.0, (num_rays, 3)) - origins).astype(F)


def room(cells=40, boxes=6, box_cells=10, seed=3):
    """a closed room (normals inward) with boxes standing in it: 12 cells^2 + boxes * 12 box_cells^2 faces"""
    rng = np.random.default_rng(seed)
    parts = [box_mesh((0.0, 0.0, 0.0), (6.0, 4.0, 3.0), cells, inward=True)]
    for _ in range(boxes):
        corner = rng.uniform((0.3, 0.3, 0.0), (4.5, 2.8, 0.5))
        parts.append(box_mesh(corner, corner + rng.uniform(0.3, 1.2, 3), box_cells))
    return join(*parts)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """a 3 x 4 camera-to-world in nerfstudio's convention: the camera looks along -z, +y is up, +x to the right"""
    eye, target, up = np.asarray(eye, D), np.asarray(target, D), np.asarray(up, D)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], axis=1), eye[:, None]], axis=1).astype(F)


def camera_rays(c2w, fx, fy, cx, cy, width, height):
    """pinhole rays through the pixel centres, fp32 unit directions (close to ``tn_generate_rays``, not bit-equal: the device tests
    take the device's rays)"""
    j, i = np.mgrid[0:height, 0:width]
    local = np.stack([(i + 0.5 - cx) / fx, -(j + 0.5 - cy) / fy, -np.ones_like(i, D)], axis=-1).reshape(-1, 3)
    world = local @ np.asarray(c2w, D)[:, :3].T
    world /= np.linalg.norm(world, axis=1, keepdims=True)
    return np.tile(np.asarray(c2w, D)[:, 3], (len(world), 1)).astype(F), world.astype(F)
