"""The yardstick of tn_mesh_rasterize: the definition of include/thermonerf_hip.h restated in numpy int64 / float64 and plain Python,
and pinned by the hand-worked literal cases below.  Every numpy operation used on floats is one correctly rounded IEEE operation per
element (add, subtract, multiply, divide, rint, the int64 -> float64 and the float32 conversions), the fixed-point arithmetic is exact
in int64, and the winner of a pixel is literally the smallest key — which is what the header asks of the kernels."""
from __future__ import annotations

import math

import numpy as np

F, D, I = np.float32, np.float64, np.int64
BLOCK = 256
NAN_BITS = 0x7fc00000
EMPTY = np.uint64(0xffffffffffffffff)
LIMIT = 2.0 ** 29


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def view(width, height, origin=(0.0, 0.0, 0.0), right=(1.0, 0.0, 0.0), down=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0), pixel_size=1.0,
         near=-math.inf, far=math.inf, cull=0):
    """the fields of tn_raster_view; the default looks along +z with x to the right and y down, one world unit per pixel"""
    return dict(origin=tuple(float(c) for c in origin), right=tuple(float(c) for c in right), down=tuple(float(c) for c in down),
                forward=tuple(float(c) for c in forward), pixel_size=float(pixel_size), near=float(near), far=float(far),
                width=int(width), height=int(height), cull=int(cull))


# ---- the ordered sum and the orders ---------------------------------------------------------------------------------------------------

def sum2(values) -> float:
    """blocks of 256 from the start of the list, each from +0.0 in list order; then the block sums from +0.0 in block order"""
    values = [float(x) for x in values]
    total = 0.0
    for k in range(0, len(values), BLOCK):
        s = 0.0
        for x in values[k:k + BLOCK]:
            s = s + x
        total = total + s
    return total


def ord32(x):
    """the order-preserving map of fp32 bits to uint32"""
    b = bits(np.asarray(x, F)).astype(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


# ---- the vertices and the faces -------------------------------------------------------------------------------------------------------

def vertices(positions, vw):
    """X, Y (int64, 8 sub-pixel bits), z (float64), rasterable (bool) per vertex"""
    p = np.asarray(positions, F).reshape(-1, 3).astype(D)
    with np.errstate(all="ignore"):
        q = [p[:, k] - D(vw["origin"][k]) for k in range(3)]

        def along(axis):
            a = [D(c) for c in vw[axis]]
            return (q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]

        x, y, z = along("right") / D(vw["pixel_size"]), along("down") / D(vw["pixel_size"]), along("forward")
        fx, fy = x * 256.0, y * 256.0
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (np.abs(fx) <= LIMIT) & (np.abs(fy) <= LIMIT)
    X = np.rint(np.where(ok, fx, 0.0)).astype(I)  # rint: half to even
    Y = np.rint(np.where(ok, fy, 0.0)).astype(I)
    return X, Y, z, ok


def faces(positions, temperature, triangles, vw):
    """usable, drawn (bool [T]); the corners after the exchange: index [T, 3], X, Y (int64 [T, 3]), z (float64 [T, 3]); area2 > 0"""
    pos, temp = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, I).reshape(-1, 3)
    v, t = len(pos), len(tri)
    X, Y, z, ok = vertices(pos, vw)
    if v == 0:
        X, Y, z, ok, temp = (np.zeros(1, a.dtype) for a in (X, Y, z, ok, temp))
    valid = ((tri >= 0) & (tri < v)).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    safe = np.where(valid[:, None], tri, 0)
    usable = valid & distinct & np.isfinite(temp[safe]).all(axis=1) & ok[safe].all(axis=1)
    fx, fy = X[safe], Y[safe]
    area2 = (fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fy[:, 1] - fy[:, 0]) * (fx[:, 2] - fx[:, 0])
    area2 = np.where(usable, area2, 0)
    drawn = usable & (area2 != 0) & ~((vw["cull"] == 1) & (area2 > 0))
    order = np.where((area2 < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))  # the exchange of the second and third vertex
    index = np.take_along_axis(safe, order, axis=1)
    return usable, drawn, index, X[index], Y[index], z[index], np.abs(area2)


def cover(xs, ys, area2, i, j):
    """per (face, pixel) pair: covered (bool [n]) and the barycentrics (float64 [n, 3]; of a pair not covered: whatever)"""
    px, py = 256 * i + 128, 256 * j + 128

    def edge(a, b):
        return (xs[:, b] - xs[:, a]) * (py - ys[:, a]) - (ys[:, b] - ys[:, a]) * (px - xs[:, a])

    def top_left(a, b):
        dx, dy = xs[:, b] - xs[:, a], ys[:, b] - ys[:, a]
        return (dy < 0) | ((dy == 0) & (dx > 0))

    w = [edge(1, 2), edge(2, 0), edge(0, 1)]
    rule = [top_left(1, 2), top_left(2, 0), top_left(0, 1)]
    inside = np.ones(len(px), bool)
    for k in range(3):
        inside &= (w[k] > 0) | ((w[k] == 0) & rule[k])
    with np.errstate(all="ignore"):
        l = np.stack([w[k].astype(D) / area2.astype(D) for k in range(3)], axis=1)
    return inside, l


def blend(l, a):
    """add(add(mul(l0, a0), mul(l1, a1)), mul(l2, a2)) per row"""
    with np.errstate(all="ignore"):
        return (l[:, 0] * a[:, 0] + l[:, 1] * a[:, 1]) + l[:, 2] * a[:, 2]


def rasterize(positions, temperature, colors, triangles, vw):
    """everything tn_mesh_rasterize writes — pixel_face (int32 [H, W]), pixel_depth, pixel_temperature (float32 [H, W]), pixel_colors
    (uint8 [H, W, 3], None without colors), counts (int64 [3]), stats (float64 [3]) — and, for the tests' own invariants, samples
    (int64 [T]: the pixels every face covers inside the slab, before the depth test) and ties (the pixels at which two samples share
    the smallest fp32 depth, so that the face index decides)"""
    pos, temp = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, I).reshape(-1, 3)
    width, height, t = vw["width"], vw["height"], len(tri)
    usable, drawn, index, X, Y, z, area2 = faces(pos, temp, tri, vw)
    if len(pos) == 0:
        usable, drawn = np.zeros(t, bool), np.zeros(t, bool)
    rows = np.flatnonzero(drawn)
    # the pixels whose centres lie in the face's box, clipped to the image
    xl, xh, yl, yh = X[rows].min(axis=1), X[rows].max(axis=1), Y[rows].min(axis=1), Y[rows].max(axis=1)
    i0, i1 = np.maximum(-((128 - xl) // 256), 0), np.minimum((xh - 128) // 256, width - 1)   # ceil and floor of (x - 128) / 256
    j0, j1 = np.maximum(-((128 - yl) // 256), 0), np.minimum((yh - 128) // 256, height - 1)
    wide, tall = np.clip(i1 - i0 + 1, 0, None), np.clip(j1 - j0 + 1, 0, None)
    number = wide * tall
    some = number > 0
    rows, i0, j0, wide, number = rows[some], i0[some], j0[some], wide[some], number[some]
    face = np.repeat(rows, number)
    within = np.arange(int(number.sum()), dtype=I) - np.repeat(np.cumsum(number) - number, number)
    i, j = np.repeat(i0, number) + within % np.repeat(wide, number), np.repeat(j0, number) + within // np.repeat(wide, number)
    inside, l = cover(X[face], Y[face], area2[face], i, j)
    face, i, j, l = face[inside], i[inside], j[inside], l[inside]
    zp = blend(l, z[face])
    slab = (D(vw["near"]) <= zp) & (zp <= D(vw["far"]))
    face, i, j, l, zp = face[slab], i[slab], j[slab], l[slab], zp[slab]
    with np.errstate(all="ignore"):
        depth = zp.astype(F)
    depth = np.where(depth == 0, F(0.0), depth).astype(F)  # -0.0 is written as +0.0
    rank = ord32(depth)
    key = (rank.astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
    pixel = j * width + i
    plane = np.full(width * height, EMPTY, np.uint64)
    np.minimum.at(plane, pixel, key)  # the smallest key, in whatever order
    won = key == plane[pixel]
    assert len(np.unique(pixel[won])) == int(won.sum()), "one winner per pixel"
    ties = int((np.bincount(pixel[rank == (plane[pixel] >> np.uint64(32)).astype(np.uint32)], minlength=1) > 1).sum())
    wp, wf, wl = pixel[won], face[won], l[won]
    pixel_face = np.full(width * height, -1, np.int32)
    pixel_depth = np.full(width * height, 0, np.uint32)
    pixel_depth[:] = NAN_BITS
    pixel_temperature = pixel_depth.copy()
    pixel_face[wp] = wf
    pixel_depth[wp] = bits(depth[won])
    with np.errstate(all="ignore"):
        pixel_temperature[wp] = bits(blend(wl, temp[index[wf]].astype(D)).astype(F))
    pixel_depth, pixel_temperature = pixel_depth.view(F), pixel_temperature.view(F)
    pixel_colors = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).reshape(-1, 3)
        pixel_colors = np.zeros((width * height, 3), np.uint8)
        for c in range(3):
            value = np.floor(blend(wl, col[index[wf], c].astype(D)) + 0.5)
            pixel_colors[wp, c] = np.clip(value, 0.0, 255.0).astype(np.uint8)
        pixel_colors = pixel_colors.reshape(height, width, 3)
    covered = pixel_face >= 0
    shown = pixel_temperature[covered]
    total = sum2(np.where(covered, pixel_temperature, F(0.0)).astype(D).tolist())
    if len(shown):
        rank_shown = ord32(shown)
        low, high = D(shown[int(np.argmin(rank_shown))]), D(shown[int(np.argmax(rank_shown))])
    else:
        low, high = D(math.inf), D(-math.inf)
    return {"pixel_face": pixel_face.reshape(height, width), "pixel_depth": pixel_depth.reshape(height, width),
            "pixel_temperature": pixel_temperature.reshape(height, width), "pixel_colors": pixel_colors,
            "counts": np.array([int(covered.sum()), int(drawn.sum()), int(usable.sum())], I), "stats": np.array([total, low, high], D),
            "samples": np.bincount(face, minlength=max(t, 1))[:t].astype(I), "ties": ties}


# ---- the literal cases, worked by hand ----------------------------------------------------------------------------------------------------
# All of them look along +z, x to the right, y down, one unit per pixel: pixel (row j, col i) has its centre at (i + 0.5, j + 0.5).
_ = -1
N = math.nan
LITERAL = {
    # A right triangle whose top and left edge and whose diagonal all pass through pixel centres.  The top edge (y = 0.5, going right) and
    # the left edge (x = 0.5, going up) are top-left and keep their centres, the diagonal x + y = 5 is not and loses them: row j keeps
    # the columns 0 .. 3 - j.  Temperature 10 + (x - 0.5): 10 + i exactly (the barycentrics are multiples of 1/4); 46 + 33 + 21 + 10 = 110.
    # (X1 - X0)(Y2 - Y0) > 0: the face is seen from behind, and is drawn because nothing is culled.
    "top_left_rule": dict(
        positions=[(0.5, 0.5, 2), (4.5, 0.5, 2), (0.5, 4.5, 2)], temperature=[10, 14, 10], triangles=[(0, 1, 2)], view=view(5, 5),
        want=dict(pixel_face=[[0, 0, 0, 0, _], [0, 0, 0, _, _], [0, 0, _, _, _], [0, _, _, _, _], [_, _, _, _, _]],
                  pixel_temperature=[[10, 11, 12, 13, N], [10, 11, 12, N, N], [10, 11, N, N, N], [10, N, N, N, N], [N, N, N, N, N]],
                  pixel_depth=[[2, 2, 2, 2, N], [2, 2, 2, N, N], [2, 2, N, N, N], [2, N, N, N, N], [N, N, N, N, N]],
                  counts=[10, 1, 1], stats=[110.0, 10.0, 13.0])),
    # the same triangle wound the other way covers the same pixels; culled it is usable and not drawn
    "top_left_rule_other_winding": dict(
        positions=[(0.5, 0.5, 2), (4.5, 0.5, 2), (0.5, 4.5, 2)], temperature=[10, 14, 10], triangles=[(0, 2, 1)], view=view(5, 5, cull=1),
        want=dict(pixel_face=[[0, 0, 0, 0, _], [0, 0, 0, _, _], [0, 0, _, _, _], [0, _, _, _, _], [_, _, _, _, _]],
                  pixel_temperature=[[10, 11, 12, 13, N], [10, 11, 12, N, N], [10, 11, N, N, N], [10, N, N, N, N], [N, N, N, N, N]],
                  counts=[10, 1, 1], stats=[110.0, 10.0, 13.0])),
    "seen_from_behind_and_culled": dict(
        positions=[(0.5, 0.5, 2), (4.5, 0.5, 2), (0.5, 4.5, 2)], temperature=[10, 14, 10], triangles=[(0, 1, 2)], view=view(5, 5, cull=1),
        want=dict(pixel_face=[[_] * 5] * 5, pixel_temperature=[[N] * 5] * 5, pixel_depth=[[N] * 5] * 5, counts=[0, 0, 1],
                  stats=[0.0, math.inf, -math.inf])),
    # A square of two faces; the shared diagonal x = y passes through the centres of the pixels (k, k).  For face 0 it is the edge from
    # (4, 4) up to (0, 0): a left edge, which keeps them; for face 1 it runs down from (0, 0) to (4, 4) and does not.
    "shared_diagonal": dict(
        positions=[(0, 0, 1), (4, 0, 1), (4, 4, 1), (0, 4, 1)], temperature=[20, 20, 20, 20], triangles=[(0, 1, 2), (0, 2, 3)],
        view=view(4, 4), want=dict(pixel_face=[[0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]], pixel_temperature=[[20] * 4] * 4,
                                   counts=[16, 2, 2], stats=[320.0, 20.0, 20.0])),
    # two faces over the whole 2 x 2 image, the nearer one listed last: it wins; a third, identical to it, loses the tie to the lower
    # index.  The colours are constant per face, so a pixel shows its face's colour.
    "nearer_face_and_equal_depth": dict(
        positions=[(-1, -1, 5), (7, -1, 5), (-1, 7, 5), (-1, -1, 3), (7, -1, 3), (-1, 7, 3)], temperature=[30, 30, 30, 18, 18, 18],
        colors=[(200, 0, 0)] * 3 + [(0, 100, 50)] * 3, triangles=[(0, 1, 2), (3, 4, 5), (3, 4, 5)], view=view(2, 2),
        want=dict(pixel_face=[[1, 1], [1, 1]], pixel_depth=[[3, 3], [3, 3]], pixel_temperature=[[18, 18], [18, 18]],
                  pixel_colors=[[(0, 100, 50)] * 2] * 2, counts=[4, 3, 3], stats=[72.0, 18.0, 18.0])),
    # a face that rises with x: depth x exactly (corners at x = 0 and 8, barycentrics multiples of 1/16), so column i lies at i + 0.5
    # and the slab 1 .. 3 keeps the columns 1 and 2; temperature 2 x
    "slab_cuts_a_tilted_face": dict(
        positions=[(0, 0, 0), (8, 0, 8), (0, 8, 0)], temperature=[0, 16, 0], triangles=[(0, 1, 2)], view=view(4, 4, near=1.0, far=3.0),
        want=dict(pixel_face=[[_, 0, 0, _]] * 4, pixel_depth=[[N, 1.5, 2.5, N]] * 4, pixel_temperature=[[N, 3, 5, N]] * 4,
                  counts=[8, 1, 1], stats=[32.0, 3.0, 5.0])),
    # the view shifted and scaled: origin (10, 20, 30), half a unit per pixel; the same picture as the first case in those units
    "origin_and_pixel_size": dict(
        positions=[(10.25, 20.25, 31), (12.25, 20.25, 31), (10.25, 22.25, 31)], temperature=[10, 14, 10], triangles=[(0, 1, 2)],
        view=view(5, 5, origin=(10, 20, 30), pixel_size=0.5),
        want=dict(pixel_face=[[0, 0, 0, 0, _], [0, 0, 0, _, _], [0, 0, _, _, _], [0, _, _, _, _], [_, _, _, _, _]],
                  pixel_depth=[[1, 1, 1, 1, N], [1, 1, 1, N, N], [1, 1, N, N, N], [1, N, N, N, N], [N, N, N, N, N]],
                  counts=[10, 1, 1], stats=[110.0, 10.0, 13.0])),
}


def literal_arrays(case):
    colors = case.get("colors")
    return (np.array(case["positions"], F), np.array(case["temperature"], F), None if colors is None else np.array(colors, np.uint8),
            np.array(case["triangles"], np.int32))


def literal_mismatch(got, want):
    """None, or the first output of ``got`` (what ``rasterize`` returns, or the kernel's outputs in the same shape) that differs; a NaN
    of ``want`` asks for the NaN 0x7fc00000"""
    for name, w in want.items():
        g = np.asarray(got[name])
        if g.dtype == F:
            w = np.asarray(w, F)
            w_bits = np.where(np.isnan(w), np.uint32(NAN_BITS), bits(w))
            if g.shape != w.shape or bits(g).tolist() != w_bits.tolist():
                return f"{name}: {g.tolist()} != {w.tolist()}"
        elif g.shape != np.asarray(w).shape or np.asarray(g, D).tolist() != np.asarray(w, D).tolist():
            return f"{name}: {g.tolist()} != {w}"
    return None


# ---- the test meshes (in pixel units for the default view) -------------------------------------------------------------------------------

def quad_lattice(cells, first, step, seed, jitter=0.0, depth=4.0):
    """(cells + 1)^2 vertices from ``first`` on, ``step`` apart, every coordinate a multiple of 1/256 (exact in fixed point); the inner
    vertices moved by up to ``jitter`` (the rim stays a square); two faces per cell, the diagonal's direction alternating; a smooth
    depth with seeded noise, a seeded temperature and seeded colours: positions, temperature, colors, triangles"""
    rng = np.random.default_rng(seed)
    n = cells + 1
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x, y = first + step * a.astype(D), first + step * b.astype(D)
    inner = ((a > 0) & (a < cells) & (b > 0) & (b < cells)).astype(D)
    x, y = x + inner * rng.uniform(-jitter, jitter, a.shape), y + inner * rng.uniform(-jitter, jitter, a.shape)
    x, y = np.rint(x * 256.0) / 256.0, np.rint(y * 256.0) / 256.0
    z = depth + 0.3 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.uniform(-0.05, 0.05, a.shape)
    pos = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F)
    k = (a * n + b)[:-1, :-1].reshape(-1)
    even = (((a + b) % 2) == 0)[:-1, :-1].reshape(-1)
    one = np.where(even[:, None], np.stack([k, k + n, k + n + 1], 1), np.stack([k, k + n, k + 1], 1))
    two = np.where(even[:, None], np.stack([k, k + n + 1, k + 1], 1), np.stack([k + n, k + n + 1, k + 1], 1))
    tri = np.stack([one, two], axis=1).reshape(-1, 3).astype(np.int32)
    temp = (22.0 + 6.0 * np.sin(x / 9.0) + rng.uniform(-2.0, 2.0, a.shape)).reshape(-1).astype(F)
    colors = rng.integers(0, 256, (n * n, 3)).astype(np.uint8)
    return pos, temp, colors, tri


def merge(*meshes):
    """several (positions, temperature, colors, triangles) as one, the faces in the order given"""
    pos, temp, col, tri, base = [], [], [], [], 0
    for p, t, c, f in meshes:
        pos.append(p), temp.append(t), col.append(c), tri.append(f + base)
        base += len(p)
    return np.concatenate(pos), np.concatenate(temp), np.concatenate(col), np.concatenate(tri).astype(np.int32)


def interleave(tri, other, every):
    """the faces of ``other`` spread through ``tri``: one after every ``every`` faces, the rest at the end"""
    out, k = [], 0
    for start in range(0, len(tri), every):
        out.append(tri[start:start + every])
        if k < len(other):
            out.append(other[k:k + 1])
            k += 1
    out.append(other[k:])
    return np.concatenate(out).astype(np.int32)


BIG_SIDE = 300


def big_scene():
    """66 248 faces of one to three pixels over a 300 x 300 image (352 SUM2 blocks) and, spread through the list, the 338 faces of a
    coarse lattice that dips in front of and behind the fine one: more than one block of the large-face list"""
    fine = quad_lattice(182, 1.25, 1.625, 41, jitter=0.5, depth=4.0)
    # one corner just above freezing, at 1e-4 degrees: the pixels' temperatures span 18 binary orders of magnitude, so that their sum
    # is rounded and depends on its order (sums of fp32 numbers of one magnitude are exact in fp64, whatever the order)
    frost = (fine[0][:, 0] < 90.0) & (fine[0][:, 1] < 90.0)
    fine[1][frost] = np.random.default_rng(47).uniform(1e-4, 2e-4, int(frost.sum())).astype(F)
    coarse = quad_lattice(13, -7.5, 24.25, 43, jitter=6.0, depth=4.05)
    pos, temp, col, tri = merge(fine, coarse)
    n = len(fine[3])
    return pos, temp, col, interleave(tri[:n], tri[n:], 190)


def tetrahedron():
    """a closed tetrahedron wound outwards, 12 pixels across, in front of the default view of a 16 x 16 image"""
    pos = np.array([(2.25, 2.5, 6.0), (13.5, 3.25, 7.0), (7.75, 13.5, 6.5), (8.0, 6.5, 2.0)], F)
    tri = np.array([(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)], np.int32)
    centre = pos.astype(D).mean(axis=0)
    for f in range(4):  # every normal points away from the centre
        p = pos[tri[f]].astype(D)
        if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), p.mean(axis=0) - centre) < 0:
            tri[f] = tri[f][[0, 2, 1]]
    return pos, np.array([15.0, 20.0, 25.0, 30.0], F), np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)], np.uint8), tri
