"""tn_mesh_project on the device against tests/mesh_project_reference.py, exactly — every integer and every float bit pattern (a NaN by
its bits), no tolerance anywhere — through the raw entry into guarded buffers with the inputs unchanged afterwards: the crafted
scenes (pixel centres, the image's border to the ulp, cos == min_cos, behind the camera and at the eye, equal weights, a wall hidden
behind another, unusable points and cameras, calls without a camera, a point, a face or a vertex, 600 points across the statistics'
blocks), a random room with a box in it under six cameras, the occlusion verdict against ``visible_from``, determinism, absent outputs,
and the Python layer with its PLY files."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from tests import mesh_project_reference as P
from tests.test_gpu_mesh_raycast import Scene, _buffer, _device, _untouched
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (CameraView, ThermalMesh, build_mesh_bvh, mesh_measurement, project_images, read_mesh_ply, vertex_normals,
                                    visible_from, write_mesh_ply)

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
OUT = {"measured": torch.float32, "views": torch.int32, "best_camera": torch.int32, "spread": torch.float32, "difference": torch.float32}
assert tuple(OUT) == P.OUTPUTS


class Mesh(Scene):
    """the ray cast's scene — a mesh on the device with its tree, built through the raw entry into guarded buffers — and the projection"""

    def project(self, points, normals, cameras, images, t_lo, t_hi, point_temperature=None, min_cos=0.2, near=0.0, two_sided=False, absent=()):
        """tn_mesh_project into guarded buffers (``absent``: the outputs passed as NULL): host copies of what was written"""
        points = np.ascontiguousarray(points, F).reshape(-1, 3)
        cameras, images = np.ascontiguousarray(cameras, F).reshape(-1, 16), np.ascontiguousarray(images, np.uint8)
        n, k = len(points), len(cameras)
        height, width = images.shape[1:]
        given = {"points": points, "cameras": cameras, "images": images}
        if normals is not None:
            given["normals"] = np.ascontiguousarray(normals, F).reshape(-1, 3)
        if point_temperature is not None:
            given["point_temperature"] = np.ascontiguousarray(point_temperature, F).reshape(-1)
        inputs = {name: _device(a) for name, a in given.items()}
        missing = set(absent) | ({"difference"} if point_temperature is None else set())
        buffers = {name: None if name in missing else _buffer(n, dtype) for name, dtype in OUT.items()}
        counts = None if "counts" in absent else _buffer(6, torch.int64)
        stats = None if "stats" in absent else _buffer(8, torch.float64)
        params = _hip.tn_project_params(t_lo, t_hi, min_cos, near, width, height, 1 if two_sided else 0, 0)
        p, t, tri = self.pointers()
        work = self.v > 0 and self.t > 0

        def address(name, need):
            return inputs[name].data_ptr() if name in inputs and need else None

        _hip.check(_hip.load().tn_mesh_project(
            p if work else None, t if work else None, tri, self.v, self.t, self.blob.data_ptr(), self.blob_bytes, address("points", n),
            address("normals", n), address("point_temperature", n), n, address("cameras", k), address("images", k), k, params,
            *[_hip.ptr(buffers[name]) for name in OUT], _hip.ptr(counts), _hip.ptr(stats), _hip.current_stream()), "tn_mesh_project")
        torch.cuda.synchronize()
        out = {}
        for name, buf in list(buffers.items()) + [("counts", counts), ("stats", stats)]:
            if buf is None:
                out[name] = None
                continue
            size = {"counts": 6, "stats": 8}.get(name, n)
            _untouched(buf, size, name)
            out[name] = buf[:size].cpu().numpy()
        self.unchanged()
        for name, before in given.items():
            assert before.tobytes() == inputs[name].cpu().numpy().tobytes(), f"{name} was written"
        return out


def _same(got, want):
    if got["counts"] is not None:
        assert got["counts"].tolist() == want["counts"].tolist(), ("counts", got["counts"], want["counts"])
    for name in OUT:
        if got[name] is not None:
            assert want[name] is not None and got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
            differ = np.flatnonzero(got[name].view(np.uint32) != want[name].view(np.uint32))
            assert len(differ) == 0, (name, len(differ), "first differing element", int(differ[0]), got[name][differ[0]], want[name][differ[0]])
    if got["stats"] is not None:
        stats = P.stats_of(*[None if got[name] is None else want[name] for name in ("difference", "spread", "measured")])
        assert got["stats"].view(np.uint64).tolist() == stats.view(np.uint64).tolist(), ("stats", got["stats"], stats)


def _split(scene):
    mesh = Mesh(scene["positions"], scene["temperature"], None, scene["triangles"])
    return mesh, {k: v for k, v in scene.items() if k not in ("positions", "temperature", "triangles")}


@functools.lru_cache(maxsize=None)
def random_mesh():
    scene, want = P.random_reference()
    mesh, call = _split(scene)
    return mesh, call, want


# ---- the crafted scenes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(P.crafted()))
def test_crafted_scene_bit_for_bit(name):
    scene = P.crafted()[name]
    want = P.project(**scene)
    mesh, call = _split(scene)
    got = mesh.project(**call)
    _same(got, want)
    if name == "wall":
        assert got["views"].tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 1] and got["measured"][[1, 2]].tolist() == [40.0, 10.0]
    if name == "cos-equal":
        assert got["views"].tolist() == [1]
    if name == "cos-above":
        assert got["views"].tolist() == [0] and got["best_camera"].tolist() == [-1]
    if name == "equal-weights":
        # cameras 0 and 1 are one camera: the lower index; at the image's corners the camera twice as far looks down more steeply
        # (cos / dist2 = 8 / 136^1.5 against 4 / 88^1.5) and wins
        assert got["best_camera"][:4].tolist() == [0, 2, 2, 0] and got["views"][:4].tolist() == [3, 3, 3, 3]
    if name == "two-walls":
        assert got["views"].tolist() == [1, 2, 2, 1, 1] and got["best_camera"][0] == 1 and got["counts"].tolist() == [5, 5, 2, 10, 7, 0]
    if name == "blocks":
        assert got["counts"].tolist() == [597, 600, 2, 1194, 1194, 0]


# ---- the random scene ---------------------------------------------------------------------------------------------------------------------

def test_random_room_bit_for_bit():
    mesh, call, want = random_mesh()
    P.conditions(want)
    assert len(call["points"]) % 64 == 37 and len(call["points"]) > 512
    got = mesh.project(**call)
    _same(got, want)
    assert got["counts"][5] == 0, "a walk reached the stack limit"
    again = mesh.project(**call)
    for name in list(OUT) + ["counts", "stats"]:
        assert got[name].tobytes() == again[name].tobytes(), f"two calls differ in {name}"


def test_occlusion_verdict_is_that_of_visible_from():
    """without normals and with min_cos out of the way a pair is accepted iff the point is in the image and ``visible_from`` sees it:
    with one camera per call, views is that mask"""
    mesh, call, _ = random_mesh()
    bvh = mesh.bvh()
    points = _device(call["points"])
    usable = P.usable_points(call["points"], None)
    rejected = 0
    for k, camera in enumerate(call["cameras"]):
        g = P.pair_geometry(camera, call["points"], None, 32, 24)
        in_image = usable & g["depth"] & g["pixel"]
        seen = visible_from(bvh, points, [float(x) for x in camera[[3, 7, 11]]]).cpu().numpy()
        got = mesh.project(call["points"], None, camera[None], call["images"][k][None], 0.0, 255.0, min_cos=1e-300,
                           absent=("measured", "best_camera", "spread", "stats"))
        assert got["views"].tolist() == (in_image & seen).astype(np.int32).tolist(), k
        rejected += int((in_image & ~seen).sum())
    assert rejected > 100, "the box and the walls hide many points that lie in the image"


@pytest.mark.parametrize("absent", [(name,) for name in list(OUT) + ["counts", "stats"]] + [tuple(OUT) + ("stats",), tuple(OUT) + ("counts",)])
def test_absent_outputs_leave_the_others_unchanged(absent):
    mesh, call, want = random_mesh()
    _same(mesh.project(**call, absent=absent), want)


def test_two_sided_near_and_no_normals_on_the_random_room():
    mesh, call, _ = random_mesh()
    scene, _ = P.random_reference()
    for change in (dict(two_sided=True, min_cos=0.5), dict(near=1.5), dict(normals=None, point_temperature=None)):
        want = P.project(**dict(scene, **change))
        assert 0 < want["counts"][4] < want["pairs"] and want["hidden"] > 0
        _same(mesh.project(**dict(call, **change)), want)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------

def _views(cameras, width, height):
    return [CameraView(c[:12].reshape(3, 4).astype(D), float(c[12]), float(c[13]), float(c[14]), float(c[15]), width, height) for c in cameras]


def test_project_images_reads_once_and_agrees_with_the_reference():
    mesh, call, want = random_mesh()
    bvh = mesh.bvh()
    got = project_images(bvh, _device(call["points"]), _device(call["normals"]), _views(call["cameras"], 32, 24), _device(call["images"]),
                         (call["t_lo"], call["t_hi"]), point_temperature=_device(call["point_temperature"]), min_cos=call["min_cos"])
    for name in OUT:
        assert getattr(got, name).cpu().numpy().view(np.uint32).tolist() == want[name].view(np.uint32).tolist(), name
    count = len(call["points"])
    assert [got.seen, got.usable_points, got.usable_cameras, got.tested_pairs, got.accepted_pairs, got.stack_limit_pairs] == want["counts"].tolist()
    matched = int((~np.isnan(want["difference"])).sum())
    s = want["stats"]
    assert got.matched == matched == got.seen and got.seen_share == got.seen / count and got.mean_views == got.accepted_pairs / count
    assert got.mean_difference == s[0] / matched and got.rms_difference == math.sqrt(s[1] / matched)
    assert (got.min_difference, got.max_difference, got.max_spread) == (s[2], s[3], s[5]) and got.mean_spread == s[4] / got.seen
    assert got.mean_measured == s[6] / got.seen
    plain = project_images(bvh, _device(call["points"]), None, _views(call["cameras"], 32, 24), _device(call["images"]), (call["t_lo"], call["t_hi"]))
    assert plain.difference is None and plain.mean_difference is None and plain.seen > got.seen
    with pytest.raises(ValueError, match="like the views"):
        project_images(bvh, _device(call["points"]), None, _views(call["cameras"], 32, 24), _device(call["images"][:, :, :31]), (0.0, 1.0))


def test_mesh_measurement_of_photos_rendered_from_the_mesh_itself(tmp_path):
    """a room whose vertex temperature is a function of the position, under photos that the reference rendered from that very
    temperature (one closest-hit ray per pixel centre): the residual is the reference's, bit for bit, and small where it should be;
    both meshes survive the PLY writer"""
    pos, temp, tri, cameras, images = P.self_photographed_room()
    scene = {"cameras": cameras, "images": images}
    host = Mesh(pos, temp, np.zeros((len(pos), 3), np.uint8), tri)
    mesh = ThermalMesh(host.pos, host.col, host.temp, None, host.tri, (10.0, 40.0))
    bvh = build_mesh_bvh(mesh)
    normals = vertex_normals(host.pos, host.tri).cpu().numpy()
    want = P.project(pos, temp, tri, pos, normals, cameras, images, 10.0, 40.0, point_temperature=temp)
    assert want["counts"][0] > 300 and want["hidden"] > 100
    # bilinear sampling errs by at most the field's variation over the 2 x 2 pixels around the vertex: away from a silhouette that is
    # the gradient (4.5 degrees per unit) times a pixel's footprint (distance / fx: about 0.25 units at 3 units) — about one degree —
    # plus half a byte (0.06 degrees); at a silhouette the photo shows another surface.  The median vertex is not at a silhouette.
    assert float(np.nanmedian(np.abs(want["difference"]))) < 1.0
    got = mesh_measurement(mesh, bvh, _views(scene["cameras"], 32, 24), _device(scene["images"]), (10.0, 40.0))
    assert got.residual.temperature.cpu().numpy().view(np.uint32).tolist() == want["difference"].view(np.uint32).tolist()
    assert got.measured.temperature.cpu().numpy().view(np.uint32).tolist() == want["measured"].view(np.uint32).tolist()
    assert got.seen == int(want["counts"][0]) and got.seen_share == got.seen / len(pos) and got.projected.stack_limit_pairs == 0
    m = max(abs(got.min_difference), abs(got.max_difference))
    assert got.residual.temperature_bounds == (-m, m) and got.measured.temperature_bounds == (10.0, 40.0) and m == float(np.nanmax(np.abs(want["difference"])))
    for name, shown in (("measured", got.measured), ("residual", got.residual)):
        path = write_mesh_ply(tmp_path / f"{name}.ply", shown)
        back = read_mesh_ply(path)
        assert back["temperature"].view(np.uint32).tolist() == shown.temperature.cpu().numpy().view(np.uint32).tolist(), name
        assert back["positions"].tobytes() == pos.tobytes() and back["triangles"].tobytes() == tri.tobytes()
        assert any(line.startswith("temperature_bounds") for line in back["comments"]), name


# ---- the command line ---------------------------------------------------------------------------------------------------------------------

def test_command_line_on_a_small_dataset_tree(tmp_path, capsys):
    import importlib.util
    import json
    import os

    from PIL import Image

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mesh_project_tool", os.path.join(root, "tools", "mesh_project.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pos, temp, tri, cameras, images = P.self_photographed_room()
    host = Mesh(pos, temp, np.zeros((len(pos), 3), np.uint8), tri)
    ply = write_mesh_ply(tmp_path / "mesh.ply", ThermalMesh(host.pos, host.col, host.temp, None, host.tri, (10.0, 40.0)))
    (tmp_path / "data" / "thermal").mkdir(parents=True)
    frames = []
    for k, c in enumerate(cameras):
        split = "eval" if k == 2 else "train"
        Image.fromarray(images[k], "L").save(tmp_path / "data" / "thermal" / f"frame_{split}_{k:05d}.PNG")
        pose = np.concatenate([c[:12].reshape(3, 4).astype(D), [[0.0, 0.0, 0.0, 1.0]]]).tolist()
        frames.append({"file_path": f"images/frame_{split}_{k:05d}.jpg", "thermal_file_path": f"thermal/frame_{split}_{k:05d}.PNG",
                       "transform_matrix": pose, "fl_x": float(c[12]), "fl_y": float(c[13]), "cx": float(c[14]), "cy": float(c[15])})
    (tmp_path / "data" / "transforms.json").write_text(json.dumps({"camera_model": "OPENCV", "w": 32, "h": 24, "frames": frames}))
    normals = vertex_normals(host.pos, host.tri).cpu().numpy()
    base = [str(ply), "--transforms", str(tmp_path / "data" / "transforms.json"), "--output", str(tmp_path / "measured.ply")]
    assert tool.main(base + ["--residual", str(tmp_path / "residual.ply"), "--report", str(tmp_path / "project.json"), "--min-change", "2.0"]) == 0
    printed = capsys.readouterr().out.splitlines()
    want = P.project(pos, temp, tri, pos, normals, cameras, images, 10.0, 40.0, point_temperature=temp)
    assert printed[0].startswith(f"{ply} under 6 photos: {len(pos)} vertices, {int(want['counts'][0])} seen")
    report = json.loads((tmp_path / "project.json").read_text())
    assert report["counts"]["seen_vertices"] == int(want["counts"][0]) and report["counts"]["accepted_pairs"] == int(want["counts"][4])
    assert report["counts"]["frames"] == 6 and report["temperature_bounds"] == [10.0, 40.0] and report["image"] == {"width": 32, "height": 24}
    assert report["residual"]["min"] == float(np.nanmin(want["difference"])) and report["residual"]["max"] == float(np.nanmax(want["difference"]))
    assert report["spread"]["max"] == float(np.nanmax(want["spread"])) and report["min_change"] == 2.0
    assert {"model_above", "model_below", "compared_area"} <= set(report) and report["compared_area"] > 0.0
    assert len([line for line in printed if line.startswith("model_")]) == len(report["model_above"]["regions"]) + len(report["model_below"]["regions"])
    measured, residual = read_mesh_ply(tmp_path / "measured.ply"), read_mesh_ply(tmp_path / "residual.ply")
    assert measured["temperature"].view(np.uint32).tolist() == want["measured"].view(np.uint32).tolist()
    assert residual["temperature"].view(np.uint32).tolist() == want["difference"].view(np.uint32).tolist()
    # the eval split alone: one photo; bounds from the command line in the training command's MAX MIN order
    assert tool.main(base + ["--frames", "eval", "--temperature-bounds", "40", "10", "--report", str(tmp_path / "eval.json")]) == 0
    one = P.project(pos, temp, tri, pos, normals, cameras[2:3], images[2:3], 10.0, 40.0, point_temperature=temp)
    assert json.loads((tmp_path / "eval.json").read_text())["counts"]["seen_vertices"] == int(one["counts"][0]) > 0
    assert read_mesh_ply(tmp_path / "measured.ply")["temperature"].view(np.uint32).tolist() == one["measured"].view(np.uint32).tolist()
