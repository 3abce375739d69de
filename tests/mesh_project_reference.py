"""The yardstick of the projection of the measured thermal photos onto points of a mesh: include/thermonerf_hip.h's definition of
``tn_mesh_project`` in plain numpy fp64, pair by pair, with no tree — the occlusion clause is the brute-force any-hit of
tests/mesh_raycast_reference.py over all usable faces.  Every step is one add, sub, mul, div or sqrt of fp64 arrays (the ray's
direction: one fp32 sub), which numpy rounds correctly and never contracts.  The crafted scenes of both test files are here too."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import mesh_closest_reference as C
from tests import mesh_raycast_reference as R

F, D = np.float32, np.float64
NAN_BITS = R.NAN_BITS
VISIBLE_FRACTION = 1.0 - 2.0 ** -10
OUTPUTS = ("measured", "views", "best_camera", "spread", "difference")
bits = R.bits


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def camera_record(c2w, fx, fy, cx, cy):
    """the sixteen floats of a ``tn_project_camera``"""
    return np.concatenate([np.asarray(c2w, D)[:3].reshape(-1), [fx, fy, cx, cy]]).astype(F)


def usable_cameras(cameras):
    cameras = np.asarray(cameras, F).reshape(-1, 16)
    return np.isfinite(cameras).all(axis=1) & (cameras[:, 12] > 0) & (cameras[:, 13] > 0)


def usable_points(points, normals):
    ok = np.isfinite(points).all(axis=1)
    if normals is not None:
        ok &= np.isfinite(normals).all(axis=1) & (normals != 0).any(axis=1)
    return ok


def pair_geometry(camera, points, normals, width, height, min_cos=0.2, near=0.0, two_sided=False):
    """clauses 1 - 4 and 7 of one camera (sixteen floats) against all points: a dict of d32 float32 [P, 3], u, v, cos, dist2, w
    float64 [P] and the masks ``depth``, ``pixel``, ``facing`` (each clause on its own, whatever the earlier ones said)"""
    camera = np.asarray(camera, F)
    eye = camera[[3, 7, 11]]
    d32 = (np.asarray(points, F) - eye[None, :]).astype(F)
    d = [d32[:, j].astype(D) for j in range(3)]
    col = [[D(camera[j]), D(camera[4 + j]), D(camera[8 + j])] for j in range(3)]
    fx, fy, cx, cy = (D(x) for x in camera[12:])
    with np.errstate(all="ignore"):
        xc, yc, z = _dot(col[0], d), _dot(col[1], d), -_dot(col[2], d)
        depth = (z > 0.0) & (z >= near)
        u = fx * (xc / z) + cx
        v = cy - fy * (yc / z)
        pixel = (0.5 <= u) & (u <= width - 0.5) & (0.5 <= v) & (v <= height - 0.5)
        dist2 = _dot(d, d)
        if normals is None:
            cos = np.ones(len(d32), D)
        else:
            n = [np.asarray(normals, F)[:, j].astype(D) for j in range(3)]
            cos = -_dot(n, d) / (np.sqrt(dist2) * np.sqrt(_dot(n, n)))
            cos = np.abs(cos) if two_sided else cos
        facing = cos >= min_cos
        w = cos / dist2
    return {"eye": eye, "d32": d32, "u": u, "v": v, "cos": cos, "dist2": dist2, "w": w, "depth": depth, "pixel": pixel, "facing": facing}


def sample(image, u, v, t_lo, t_hi):
    """clause 6 for (u, v) inside the hull of the pixel centres of ``image`` uint8 [H, W]: degrees, float64"""
    height, width = image.shape
    a, b = u - 0.5, v - 0.5
    x0 = np.minimum(np.floor(a).astype(np.int64), width - 2)
    y0 = np.minimum(np.floor(b).astype(np.int64), height - 2)
    fa, fb = a - x0.astype(D), b - y0.astype(D)
    image = image.astype(D)
    p00, p01, p10, p11 = image[y0, x0], image[y0, x0 + 1], image[y0 + 1, x0], image[y0 + 1, x0 + 1]
    top = p00 + fa * (p01 - p00)
    bottom = p10 + fa * (p11 - p10)
    s = top + fb * (bottom - top)
    return D(t_lo) + (s / 255.0) * (D(t_hi) - D(t_lo))


def hidden(positions, temperature, triangles, eye, d32):
    """bool [N]: clause 5, the any-hit of the ray (eye, d32) over [0, VISIBLE_FRACTION] against every usable face"""
    if not len(d32):
        return np.zeros(0, bool)
    origins = np.tile(np.asarray(eye, F), (len(d32), 1))
    stop = np.full(len(d32), VISIBLE_FRACTION, F)
    assert float(stop[0]) == VISIBLE_FRACTION
    return R.raycast(positions, temperature, None, triangles, origins, d32, ray_t_max=stop)["hit_any"].astype(bool)


def project(positions, temperature, triangles, points, normals, cameras, images, t_lo, t_hi, point_temperature=None, min_cos=0.2,
            near=0.0, two_sided=False):
    """The definition.  ``cameras`` float32 [K, 16], ``images`` uint8 [K, H, W].  A dict of ``measured``, ``spread`` float32 [P],
    ``views``, ``best_camera`` int32 [P], ``difference`` float32 [P] (None without point_temperature), ``counts`` int64 [6], ``stats``
    float64 [8]; and, for the tests' conditions, ``pairs`` (usable point x usable camera), ``behind``, ``outside``, ``facing``, ``hidden``
    (the pairs each clause removed, in the clauses' order), ``reached`` and ``accepted`` bool [K, P]."""
    positions, temperature = np.asarray(positions, F).reshape(-1, 3), np.asarray(temperature, F).reshape(-1)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    points = np.asarray(points, F).reshape(-1, 3)
    normals = None if normals is None else np.asarray(normals, F).reshape(-1, 3)
    cameras = np.asarray(cameras, F).reshape(-1, 16)
    images = np.asarray(images, np.uint8)
    num_points, num_cameras = len(points), len(cameras)
    height, width = images.shape[1:]
    good_points, good_cameras = usable_points(points, normals), usable_cameras(cameras)
    sw, swt = np.zeros(num_points, D), np.zeros(num_points, D)
    low, high, best_w = np.zeros(num_points, D), np.zeros(num_points, D), np.zeros(num_points, D)
    views, best = np.zeros(num_points, np.int32), np.full(num_points, -1, np.int32)
    removed = {"behind": 0, "outside": 0, "facing": 0, "hidden": 0}
    reached_all, accepted_all = np.zeros((num_cameras, num_points), bool), np.zeros((num_cameras, num_points), bool)
    with np.errstate(all="ignore"):
        for k in range(num_cameras):
            if not good_cameras[k]:
                continue
            g = pair_geometry(cameras[k], points, normals, width, height, min_cos, near, two_sided)
            stage = good_points & g["depth"]
            removed["behind"] += int((good_points & ~g["depth"]).sum())
            removed["outside"] += int((stage & ~g["pixel"]).sum())
            stage = stage & g["pixel"]
            removed["facing"] += int((stage & ~g["facing"]).sum())
            reached = stage & g["facing"]
            accepted = reached.copy()
            rows = np.flatnonzero(reached)
            accepted[rows] = ~hidden(positions, temperature, tri, g["eye"], g["d32"][rows])
            removed["hidden"] += int((reached & ~accepted).sum())
            reached_all[k], accepted_all[k] = reached, accepted
            at = np.flatnonzero(accepted)
            t = sample(images[k], g["u"][at], g["v"][at], t_lo, t_hi)
            w = g["w"][at]
            sw[at] = sw[at] + w
            swt[at] = swt[at] + w * t
            first = views[at] == 0
            low[at] = np.where(first | (t < low[at]), t, low[at])
            high[at] = np.where(first | (t > high[at]), t, high[at])
            better = first | (w > best_w[at])
            best_w[at] = np.where(better, w, best_w[at])
            best[at] = np.where(better, k, best[at])
            views[at] += 1
        seen = views > 0
        nan = np.uint32(NAN_BITS).view(F)
        measured = np.where(seen, (swt / sw).astype(F), nan).astype(F)
        measured = np.where(np.isnan(measured), nan, measured).astype(F)
        out = {"measured": measured, "views": views, "best_camera": best, "spread": np.where(seen, (high - low).astype(F), nan).astype(F),
               "difference": None}
        if point_temperature is not None:
            delta = (np.asarray(point_temperature, F).reshape(-1).astype(D) - measured.astype(D)).astype(F)
            out["difference"] = np.where(np.isnan(delta), nan, delta).astype(F)
    out["counts"] = np.array([int(seen.sum()), int(good_points.sum()), int(good_cameras.sum()), int(reached_all.sum()),
                              int(accepted_all.sum()), 0], np.int64)
    out["stats"] = stats_of(out["difference"], out["spread"], out["measured"])
    out.update(removed, pairs=int(good_points.sum()) * int(good_cameras.sum()), reached=reached_all, accepted=accepted_all)
    return out


def stats_of(difference, spread, measured):
    """float64 [8] from the three output arrays (None: absent)"""
    none = [0.0, 0.0, math.inf, -math.inf]
    d = C.stats_of(difference) if difference is not None else none
    s = C.stats_of(spread) if spread is not None else none
    m = C.stats_of(measured) if measured is not None else none
    return np.array(d + [s[0], s[3], m[0], 0.0], D)


# ---- crafted scenes ---------------------------------------------------------------------------------------------------------------------

def quad(x0, x1, y0, y1, z):
    """two triangles in the plane z, normal +z: (positions, triangles)"""
    return (np.array([(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)], F), np.array([(0, 1, 2), (0, 2, 3)], np.int32))


def down_camera(x=0.0, y=0.0, z=4.0, fx=1.0, fy=1.0, cx=2.0, cy=2.0):
    """a camera at (x, y, z) with the identity rotation: it looks down -z, +x to the right, +y up"""
    return camera_record(np.concatenate([np.eye(3), [[x], [y], [z]]], axis=1), fx, fy, cx, cy)


# a wall in z = 0 seen head-on from (0, 0, 4) through a 4 x 4 image with fx = fy = 1, cx = cy = 2: the point (x, y, 0) lands at
# u = 2 + x / 4, v = 2 - y / 4, every step exact for the x, y below
WALL = quad(-16.0, 16.0, -16.0, 16.0, 0.0)
WALL_IMAGE = np.array([[0, 10, 20, 30], [40, 50, 60, 70], [80, 90, 100, 110], [255, 0, 51, 102]], np.uint8)


def two_walls():
    """a back wall in z = -2 and a front wall in z = 0 over -1 <= x <= 1 before it: (positions, temperature, triangles)"""
    pos, tri = R.join(quad(-16.0, 16.0, -16.0, 16.0, -2.0), quad(-1.0, 1.0, -16.0, 16.0, 0.0))
    return pos, np.full(len(pos), 20.0, F), tri


def random_scene(seed=7, blocks=9):
    """the random scene of both test files: a closed room of 1200 faces (normals inward) with a box of 432 faces standing in it, six
    cameras inside the room around the box, P = 64 blocks + 37 points on the surfaces with their faces' normals (a few of them made
    unusable), 32 x 24 random-byte images.  A dict of the arguments of ``project``."""
    rng = np.random.default_rng(seed)
    pos, tri = R.join(R.box_mesh((0.0, 0.0, 0.0), (4.0, 4.0, 3.0), 10, inward=True), R.box_mesh((1.5, 1.5, 0.0), (2.5, 2.5, 2.25), 6))
    temp = rng.uniform(10.0, 35.0, len(pos)).astype(F)
    count = 64 * blocks + 37
    face = rng.integers(0, len(tri), count)
    bary = rng.dirichlet((1.0, 1.0, 1.0), count)
    points = (pos[tri[face]].astype(D) * bary[:, :, None]).sum(axis=1).astype(F)
    normals = C.face_normals(pos, tri)[face].astype(F)
    points[5], points[70, 1], normals[130], normals[300, 2] = np.nan, np.inf, 0.0, np.nan
    width, height = 32, 24
    cameras = []
    for k in range(6):
        angle = 2.0 * math.pi * (k + 0.25) / 6.0
        eye = (2.0 + 1.7 * math.cos(angle), 2.0 + 1.7 * math.sin(angle), 0.6 + 0.35 * k)
        cameras.append(camera_record(R.look_at(eye, (2.0, 2.0, 1.2)), 11.0, 11.0, width / 2.0 + 0.3 * k, height / 2.0 - 0.2 * k))
    images = rng.integers(0, 256, (6, height, width)).astype(np.uint8)
    return {"positions": pos, "temperature": temp, "triangles": tri, "points": points, "normals": normals, "cameras": np.stack(cameras),
            "images": images, "t_lo": 12.5, "t_hi": 41.25, "point_temperature": rng.uniform(10.0, 40.0, count).astype(F), "min_cos": 0.2}


@functools.lru_cache(maxsize=None)
def random_reference():
    """(the random scene, what ``project`` makes of it): computed once, shared by the tests, not to be written to"""
    scene = random_scene()
    return scene, project(**scene)


def conditions(out):
    """what the random scene must satisfy so that a test on it cannot pass vacuously"""
    reached, accepted = int(out["counts"][3]), int(out["counts"][4])
    assert accepted >= 0.2 * out["pairs"], ("accepted pairs", accepted, out["pairs"])
    assert out["hidden"] >= 0.1 * reached and out["hidden"] == reached - accepted, ("hidden pairs", out["hidden"], reached)
    assert out["behind"] >= 1 and out["outside"] >= 1 and out["facing"] >= 1, (out["behind"], out["outside"], out["facing"])
    assert out["counts"][5] == 0


def crafted():
    """the crafted scenes of the device test, name -> the arguments of ``project``: the literal cases of tests/test_mesh_project_cpu.py"""
    up = np.array([0.0, 0.0, 1.0], F)
    pos, tri = WALL
    wall = {"positions": pos, "temperature": np.full(len(pos), 20.0, F), "triangles": tri, "t_lo": 10.0, "t_hi": 40.0}
    one = {"cameras": np.stack([down_camera()]), "images": WALL_IMAGE[None]}
    after = lambda x, to: np.nextafter(F(x), F(to))  # noqa: E731
    points = np.array([(-2, 2, 0), (-6, -6, 0), (-6, 6, 0), (0, 0, 0), (1, 0, 0), (2, -2, 0), (6, 0, 0), (after(6, np.inf), 0, 0), (-6, 0, 0),
                       (after(-6, -np.inf), 0, 0), (0, 6, 0), (0, after(6, np.inf), 0), (0, -6, 0), (0, after(-6, -np.inf), 0), (0, 0, 5), (0, 0, 4),
                       (0, 0, 3), (3, 0, 0)], F)
    scenes = {"wall": dict(wall, **one, points=points, normals=np.tile(up, (len(points), 1)), point_temperature=np.full(len(points), 25.0, F))}
    scenes["wall-no-normals"] = dict(wall, **one, points=points, normals=None, near=2.0)
    scenes["cos-equal"] = dict(wall, **one, points=points[-1:], normals=up[None], min_cos=0.8)
    scenes["cos-above"] = dict(wall, **one, points=points[-1:], normals=up[None], min_cos=float(np.nextafter(0.8, 1.0)))
    scenes["two-sided"] = dict(wall, **one, points=points, normals=np.tile(-up, (len(points), 1)), two_sided=True, min_cos=0.8)
    other = (255 - WALL_IMAGE.astype(np.int64)).astype(np.uint8)
    far = down_camera(z=8.0, fx=2.0, fy=2.0)
    scenes["equal-weights"] = dict(wall, cameras=np.stack([down_camera(), down_camera(), far]), images=np.stack([WALL_IMAGE, other, WALL_IMAGE]),
                                   points=points, normals=np.tile(up, (len(points), 1)), point_temperature=np.full(len(points), 25.0, F))
    scenes["far-first"] = dict(wall, cameras=np.stack([far, down_camera()]), images=np.stack([WALL_IMAGE, other]), points=points, normals=None)
    wpos, wtemp, wtri = two_walls()
    behind = np.array([(0, 0, -2), (0, 0, 0), (3, 0, -2), (0.5, 1, -2), (-4, 2, -2)], F)
    scenes["two-walls"] = {"positions": wpos, "temperature": wtemp, "triangles": wtri, "points": behind, "normals": np.tile(up, (5, 1)),
                           "cameras": np.stack([down_camera(), down_camera(x=5.0)]), "t_lo": 0.0, "t_hi": 51.0,
                           "images": np.stack([np.full((4, 4), 100, np.uint8), np.full((4, 4), 200, np.uint8)])}
    scenes["no-faces"] = dict(scenes["two-walls"], triangles=wtri[:0])
    scenes["no-vertices"] = dict(scenes["two-walls"], positions=wpos[:0], temperature=wtemp[:0])
    mixed = np.array([(0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0)], F)
    normals = np.tile(up, (6, 1))
    normals[3], normals[4, 0] = 0.0, np.nan
    cameras = np.stack([down_camera(fx=0.0), down_camera(), down_camera(x=np.inf), down_camera(fy=-1.0), down_camera(cx=np.nan)])
    scenes["unusable"] = dict(wall, cameras=cameras, images=np.stack([WALL_IMAGE] * 5), points=mixed, normals=normals,
                              point_temperature=np.array([30, 30, 30, 30, 30, np.nan], F))
    scenes["no-cameras"] = dict(scenes["unusable"], cameras=cameras[:0], images=np.zeros((0, 4, 4), np.uint8))
    scenes["no-points"] = dict(scenes["unusable"], points=mixed[:0], normals=normals[:0], point_temperature=np.zeros(0, F))
    rng = np.random.default_rng(5)
    many = np.concatenate([rng.uniform(-5.0, 5.0, (600, 2)), np.zeros((600, 1))], axis=1).astype(F)
    many[[3, 300, 599], 0] = 50.0
    scenes["blocks"] = dict(wall, cameras=np.stack([down_camera(), down_camera(x=0.5, z=5.0)]), images=rng.integers(0, 256, (2, 4, 4)).astype(np.uint8),
                            points=many, normals=np.tile(up, (600, 1)), point_temperature=rng.uniform(10.0, 40.0, 600).astype(F))
    return scenes


@functools.lru_cache(maxsize=None)
def self_photographed_room(t_lo=10.0, t_hi=40.0):
    """the random scene's room with a vertex temperature that is a function of the position (15 + 4 x + 2 z degrees) and, as photos,
    what its six cameras see of that temperature: one closest-hit ray per pixel centre against the mesh, the hit's temperature as the
    byte nearest to 255 (T - t_lo) / (t_hi - t_lo), 0 where a ray meets nothing.  (positions, temperature, triangles, cameras, images)"""
    scene = random_scene()
    pos, tri, cameras = scene["positions"], scene["triangles"], scene["cameras"]
    temp = (15.0 + 4.0 * pos[:, 0].astype(D) + 2.0 * pos[:, 2].astype(D)).astype(F)
    height, width = scene["images"].shape[1:]
    images = np.zeros((len(cameras), height, width), np.uint8)
    for k, c in enumerate(cameras):
        origins, directions = R.camera_rays(c[:12].reshape(3, 4), c[12], c[13], c[14], c[15], width, height)
        shown = R.raycast(pos, temp, None, tri, origins, directions)["hit_temperature"].astype(D)
        byte = np.floor((shown - t_lo) / (t_hi - t_lo) * 255.0 + 0.5)
        images[k] = np.where(np.isnan(shown), 0.0, np.clip(byte, 0.0, 255.0)).astype(np.uint8).reshape(height, width)
    return pos, temp, tri, cameras, images
