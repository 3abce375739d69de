"""The three readers of one tree — ``tn_mesh_raycast``, ``tn_mesh_closest``, ``tn_mesh_project`` — on ONE blob and ONE set of points in a
single test, and the ray cast's statistics against its own ``hit_temperature`` output: its finish kernel is the statistics pass of the
other two (tn_mesh_bvh.h ``finish_one``) without the squares.  Query counts around the wave and across the 256-run boundary of the
ordered sum.  Everything bit for bit against the numpy references.  (The chain's points, pushed off the vertices of faces 2^-13 wide,
are also the only ones in the suite that a face hides between 1 - 2^-10 and 1 - 2^-11 of the way from a camera: clause 5's end.)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

from tests import mesh_closest_reference as C
from tests import mesh_project_reference as P
from tests import mesh_raycast_reference as R
from tests import test_gpu_mesh_closest as closest_tests
from tests import test_gpu_mesh_project as project_tests
from tests import test_gpu_mesh_raycast as cast_tests

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
COUNTS = (0, 1, 63, 64, 65, 257)
WIDTH, HEIGHT = 16, 12


class Readers(closest_tests.Mesh, project_tests.Mesh):
    """the ray cast's scene with the closest-point query and the projection beside its cast: one mesh, one blob"""


@functools.lru_cache(maxsize=None)
def scene(name):
    """(the mesh with its tree, 257 points, 257 rays from them, their own temperatures, three cameras, their photos): not to be written to"""
    pos, tri = R.cube_lattice(1) if name == "cube" else cast_tests.deep_chain()
    assert name != "cube" or len(tri) == 12
    temp, col = R.attributes(len(pos), 12)
    points = C.query_points(pos, tri, max(COUNTS), 31)
    centres = pos[tri].astype(D).mean(axis=1)
    origins = points.copy()
    origins[4::5, 0] = np.nan  # every fifth ray is unusable: a miss, the NaN that the sums count +0.0 and the extremes leave out
    directions = (centres[np.arange(len(points)) % len(tri)] - points.astype(D)).astype(F)
    own = closest_tests.own_temperature(len(points), 5)
    own[7::11] = np.nan
    eyes = [(3.0, 0.4, 0.6), (0.5, -2.5, 0.7), (0.3, 0.6, 3.5)]
    cameras = np.stack([P.camera_record(R.look_at(eye, (0.5, 0.5, 0.5), up=(0.0, 0.1, 1.0)), 10.0, 10.0, WIDTH / 2.0, HEIGHT / 2.0) for eye in eyes])
    images = np.random.default_rng(17).integers(0, 256, (len(eyes), HEIGHT, WIDTH)).astype(np.uint8)
    return Readers(pos, temp, col, tri), points, origins, directions, own, cameras, images


def cast_stats_of(hit_temperature):
    """float64 [3] from the cast's own output: SUM2 over all rays (a miss counts +0.0), the extremes over the hits in the numbers' order"""
    has = ~np.isnan(hit_temperature)
    shown = hit_temperature[has]
    low = D(shown[np.argmin(R.ord32(shown))]) if has.any() else math.inf
    high = D(shown[np.argmax(R.ord32(shown))]) if has.any() else -math.inf
    return np.array([R.sum2(np.where(has, hit_temperature.astype(D), 0.0)), low, high], D)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", ["cube", "chain"])
def test_three_readers_of_one_blob(name, count):
    mesh, points, origins, directions, own, cameras, images = scene(name)
    q, o, d, own = points[:count], origins[:count], directions[:count], own[:count]

    got = cast_tests.Scene.cast(mesh, o, d)
    cast_tests._same(got, R.raycast(*mesh.host, o, d))
    misses = int(np.isnan(got["hit_temperature"]).sum())
    assert misses >= count // 5 and got["counts"][0] == count - misses and (count == 0 or got["counts"][0] > 0)
    assert got["stats"].view(np.uint64).tolist() == cast_stats_of(got["hit_temperature"]).view(np.uint64).tolist(), \
        ("the cast's stats are not those of its own hit_temperature", got["stats"], cast_stats_of(got["hit_temperature"]))

    want = C.closest(*mesh.host, q, point_temperature=own)
    got = mesh.closest(q, own)
    closest_tests._same(got, want)
    stats = np.array(C.stats_of(want["closest_distance"]) + C.stats_of(want["difference"]), D)
    assert got["stats"].view(np.uint64).tolist() == stats.view(np.uint64).tolist(), ("closest stats", got["stats"], stats)
    assert got["counts"].tolist() == [count, count, mesh.t, 0]

    call = dict(points=q, normals=None, cameras=cameras, images=images, t_lo=10.0, t_hi=40.0, point_temperature=own)
    want = P.project(*(mesh.host[k] for k in (0, 1, 3)), **call)
    got = mesh.project(**call)
    project_tests._same(got, want)
    stats = P.stats_of(want["difference"], want["spread"], want["measured"])
    assert got["stats"].view(np.uint64).tolist() == stats.view(np.uint64).tolist(), ("projection stats", got["stats"], stats)
    assert got["counts"][5] == 0 and (count < 63 or 0 < got["counts"][0])
    assert name != "cube" or count < 63 or got["counts"][4] < got["counts"][3], "the cube hides some of the pairs that reach the occlusion test"
