"""The yardstick of the scalar smoothing and the surface gradient (tests/mesh_gradient_reference.py) against results known by hand and
against the identities of the gradient of a linear interpolant, the new entries in header, ctypes table, Makefile and library, the
refusals that need no device, and the command line's arguments.  No GPU."""
from __future__ import annotations

import ctypes
import importlib.util
import math
import os
import re
import types

import numpy as np
import pytest

from tests import mesh_gradient_reference as R
from tests.mesh_smooth_reference import brute_force_lists
from thermo_nerf_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _gradient(pos, values, tri):
    return R.gradient(pos, values, tri, R.incidence(tri, len(pos)))


def test_right_triangle_and_the_same_scaled_by_two():
    pos, tri = R.RIGHT_TRIANGLE
    got = _gradient(pos, np.array([0, 1, 0], F), tri)
    assert R.bits(got["face_gradient"]).tolist() == [R.bits(np.array([1.0, 0.0, 0.0])).tolist()]  # +0.0, too
    assert got["vertex_gradient"].tolist() == [[1.0, 0.0, 0.0]] * 3 and got["vertex_magnitude"].tolist() == [1.0] * 3
    assert got["totals"].tolist() == [1.0, 1.0, 1.0, 1.0]  # one face, twice its area, times |g| = 1
    double = _gradient(pos * F(2), np.array([0, 1, 0], F), tri)
    assert double["face_gradient"].tolist() == [[0.5, 0.0, 0.0]] and double["vertex_magnitude"].tolist() == [0.5] * 3
    assert double["totals"].tolist() == [1.0, 4.0, 2.0, 0.5]


def test_constant_field_has_gradient_plus_zero():
    pos, tri = R.lattice(5, 5)
    got = _gradient(pos, np.full(len(pos), 21.5, F), tri)
    assert (got["face_gradient"] == 0.0).all()
    # a vertex sum starts from +0.0, and add(+0.0, mul(w, -0.0)) is +0.0: the vertices are +0.0 to the bit
    assert not R.bits(got["vertex_gradient"]).any() and not R.bits(got["vertex_magnitude"]).any()
    assert got["totals"].tolist() == [32.0, 32.0, 0.0, 0.0]
    assert not R.bits(_gradient(*R.RIGHT_TRIANGLE[:1], np.full(3, 7, F), R.RIGHT_TRIANGLE[1])["face_gradient"]).any()


def test_integer_lattice_with_a_linear_field_is_exact():
    pos, tri = R.lattice(5, 5)
    values = (3 * pos[:, 0] - 2 * pos[:, 1]).astype(F)
    got = _gradient(pos, values, tri)
    assert len(tri) == 32 and (got["faces"]["n"] == [0, 0, 1]).all(), "n2 is 1"
    assert (got["face_gradient"] == [3, -2, 0]).all() and (got["vertex_gradient"] == [3, -2, 0]).all()
    assert R.bits(got["vertex_magnitude"]).tolist() == [int(R.bits(np.array([math.sqrt(13.0)], F))[0])] * 25
    assert got["totals"].tolist() == [32.0, 32.0, R.sum2([math.sqrt(13.0)] * 32), math.sqrt(13.0)]


def test_identities_of_the_gradient_on_random_faces():
    """g . e1 = a, g . e2 = b, g . n = 0 with a = u1 - u0, b = u2 - u0, to within 32 u s |x| for the dot product with x, where
    u = 2^-53 and s = (|a| |e2| + |b| |e1|) / |n| is the face's own scale of |g| (|g| <= s by the triangle inequality).  Where the
    bound comes from, the computed edges e1, e2 and face vector n' taken as data and every term to first order in u:
      * a component of A = e2 x n' or B = n' x e1 is fl(fl(.) - fl(.)): off by at most 3 u |e2| |n'| (3 u |e1| |n'|); the numerator
        fl(fl(a A_c) + fl(b B_c)) adds 2 u (|a| |A_c| + |b| |B_c|); n2, a sum of three rounded squares, is off by 3 u n2; the quotient
        adds u: a component of g is off by at most (3 + 2 + 3 + 1) u s = 9 u s, the vector by sqrt(3) 9 u s < 15.6 u s, its dot
        product with x by that times |x|;
      * the dot product the test takes in fp64 is itself off by at most 3 u |g| |x| <= 3 u s |x|;
      * the identities hold for the exact n = e1 x e2, the kernel has n' = n + d with |d_c| <= 3 u |e1| |e2|: (e2 x n') . e1 / (n' . n')
        = n' . n / (n' . n') = 1 - d . n' / (n' . n'), off from 1 by at most 3 sqrt(3) u |e1| |e2| / |n'|, times |a| this is at most
        5.2 u s |e1| (likewise for e2 with b; g . n' = 0 holds for ANY n', so the third identity has no such term).
    15.6 + 3 + 5.2 < 24; the test allows 32, the next power of two, for the higher orders.  Faces with |n| >= 0.05 |e1| |e2|."""
    rng = np.random.default_rng(11)
    pos = rng.uniform(-1.0, 1.0, (3000, 3)).astype(F)
    tri = np.arange(3000, dtype=np.int32).reshape(-1, 3)
    values = rng.uniform(14.0, 33.0, 3000).astype(F)
    faces = R.face_gradients(pos, values, tri)
    e1, e2, n, g = faces["e1"], faces["e2"], faces["n"], faces["g"]
    norm = lambda x: np.sqrt((x * x).sum(axis=1))  # noqa: E731
    keep = faces["usable"] & (norm(n) >= 0.05 * norm(e1) * norm(e2))
    assert keep.sum() > 900
    u0, u1, u2 = (values[tri[:, k]].astype(D) for k in range(3))
    a, b = u1 - u0, u2 - u0
    scale = (np.abs(a) * norm(e2) + np.abs(b) * norm(e1)) / np.where(keep, norm(n), 1.0)
    bound = 32 * 2.0 ** -53
    for x, want in ((e1, a), (e2, b), (n, np.zeros_like(a))):
        deviation = np.abs((g * x).sum(axis=1) - want)
        assert (deviation[keep] <= bound * scale[keep] * norm(x)[keep]).all(), float((deviation[keep] / (scale * norm(x))[keep]).max() / 2.0 ** -53)
    assert (norm(g)[keep] <= scale[keep] * (1 + 1e-12)).all()


def test_unusable_faces_and_vertices_get_the_stated_nan():
    pos, tri = R.lattice(3, 3)
    values = np.arange(9, dtype=F)
    for spoil in ("nan", "inf", "position", "collinear"):
        p, x, t = pos.copy(), values.copy(), tri.copy()
        if spoil == "nan":
            x[0] = np.nan
        elif spoil == "inf":
            x[0] = -np.inf
        elif spoil == "position":
            p[0, 1] = np.inf
        else:
            p[0] = p[1]  # the corner's two faces lose their area: (1,0) (1,0) (1,1) and (1,0) (1,1) (0,1) has one still
        got = _gradient(p, x, t)
        bad = (t == 0).any(axis=1) if spoil != "collinear" else np.array([True] + [False] * 7)
        assert got["faces"]["usable"].tolist() == (~bad).tolist(), spoil
        assert (R.bits(got["face_gradient"][bad]) == R.NAN64_BITS).all() and np.isfinite(got["face_gradient"][~bad]).all()
        if spoil != "collinear":  # vertex 0 has no usable face left
            assert R.bits(got["vertex_gradient"][0]).tolist() == [R.NAN32_BITS] * 3 and R.bits(got["vertex_magnitude"][:1]).tolist() == [R.NAN32_BITS]
            assert np.isfinite(got["vertex_gradient"][1:]).all()
        assert got["totals"][0] == (~bad).sum()
    # a vertex in no triangle, a repeated index, an index outside the vertices
    tri = np.array([(0, 1, 3), (1, 1, 3), (0, 1, 9)], np.int32)
    got = _gradient(pos[:5], values[:5], tri)
    assert got["faces"]["usable"].tolist() == [True, False, False]
    assert R.bits(got["vertex_magnitude"][[2, 4]]).tolist() == [R.NAN32_BITS] * 2 and np.isfinite(got["vertex_magnitude"][[0, 1, 3]]).all()


def test_the_rounds_walk_the_brute_force_lists_and_clip_a_foreign_index():
    from tests.mesh_components_reference import random_mesh

    tri = random_mesh(4, 40, 90, invalid=0.1)
    index = R.incidence(tri, 40)
    walked = [[] for _ in range(40)]
    for vs, cs in R.rounds(index, 3 * len(tri)):
        for v, c in zip(vs.tolist(), cs.tolist()):
            walked[v].append(c)
    assert walked == brute_force_lists(tri, 40)
    foreign = dict(offsets=np.array([-5, 2, 2, 400], np.int32), corners=np.array([0, 99, -1, 5, 7, 2], np.int32))
    assert [(vs.tolist(), cs.tolist()) for vs, cs in R.rounds(foreign, 6)] == [([0], [0]), ([2], [5]), ([], []), ([2], [2])]


def test_smoothing_passes_by_hand():
    pos, tri = R.RIGHT_TRIANGLE
    index = R.incidence(tri, 3)
    # every vertex has one corner, its partners are the other two
    assert R.smooth_pass(np.array([0, 2, 4], F), tri, index, 0.5, False).tolist() == [1.5, 2.0, 2.5]
    assert R.smooth(np.array([0, 2, 4], F), tri, index, 1, 0.5, 0.0).tolist() == [1.5, 2.0, 2.5]
    assert R.smooth(np.array([0, 2, 4], F), tri, index, 1, 0.5, -1.0).tolist() == [0.75, 2.0, 3.25]  # then p - (m - p)
    # a NaN is no partner; it stays with fill off, takes the mean of the finite partners with fill on; an odd payload keeps its bits
    odd = np.array([0x7fc12345, 0x40000000, 0x40800000], np.uint32).view(F)  # NaN, 2, 4
    kept = R.smooth_pass(odd, tri, index, 0.5, False)
    assert R.bits(kept).tolist() == [0x7fc12345, 0x40400000, 0x40400000]  # 2 -> 3 <- 4: each sees the other alone
    filled = R.smooth_pass(odd, tri, index, 0.0, True)
    assert filled.tolist() == [3.0, 2.0, 4.0]
    assert R.bits(R.smooth_pass(np.array([np.nan, np.inf, -np.inf], F), tri, index, 0.5, True)).tolist() == R.bits(np.array([np.nan, np.inf, -np.inf], F)).tolist()


def test_a_hole_of_three_by_three_closes_by_one_ring_per_pass():
    pos, tri = R.lattice(9, 9)
    index = R.incidence(tri, len(pos))
    hole = R.hole(9, 9, 3, 3, 3)
    values = R.random_values(3, 81)
    values[hole] = np.nan
    one = R.smooth(values, tri, index, 1, 0.0, 0.0, fill=True)
    centre = np.zeros(81, bool)
    centre[4 * 9 + 4] = True
    assert np.isnan(one).tolist() == centre.tolist()
    two = R.smooth(values, tri, index, 2, 0.0, 0.0, fill=True)
    assert np.isfinite(two).all()
    assert R.bits(two[~hole]).tolist() == R.bits(values[~hole]).tolist() == R.bits(one[~hole]).tolist()
    assert R.bits(R.smooth(values, tri, index, 2, 0.5, 0.0, fill=False)[hole]).tolist() == R.bits(values[hole]).tolist()


def test_sum2_is_the_regions_yardsticks_sum2():
    from tests.mesh_regions_reference import sum2

    rng = np.random.default_rng(5)
    for n in (0, 1, 255, 256, 257, 513, 70000):
        x = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
        assert R.sum2(x) == sum2(x), n


def test_header_makefile_ctypes_table_and_library_agree_on_the_new_entries():
    header = open(os.path.join(ROOT, "include", "thermonerf_hip.h")).read()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(_hip.lib_path())
    for name in ("tn_mesh_scalar_smooth", "tn_mesh_scalar_gradient", "tn_mesh_scalar_gradient_workspace_bytes"):
        assert name in declared and name in _hip.SIGNATURES and hasattr(lib, name), name
    assert len(_hip.SIGNATURES["tn_mesh_scalar_smooth"][1]) == 13 and len(_hip.SIGNATURES["tn_mesh_scalar_gradient"][1]) == 14
    assert len(_hip.SIGNATURES["tn_mesh_scalar_gradient_workspace_bytes"][1]) == 2
    makefile = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "Makefile")).read()
    assert " tn_mesh_gradient.hip " in makefile and " tn_mesh_lists.h " in makefile and " ../../include/thermonerf_hip.h" in makefile
    # the face is tn_group_sum.h's, the lists' helpers tn_mesh_lists.h's: the new source restates neither
    code = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_mesh_gradient.hip")).read()
    assert '#include "tn_group_sum.h"' in code and "load_face(" in code and "join_run<" in code and "Face load_face(" not in code
    for source in ("tn_mesh_gradient.hip", "tn_mesh_smooth.hip"):
        code = open(os.path.join(ROOT, "thermo_nerf_amd", "csrc", source)).read()
        assert '#include "tn_mesh_lists.h"' in code and "void list_of(" not in code and "Tri load_triangle(" not in code, source


def test_workspace_size_and_the_error_codes_that_need_no_device():
    load = _hip.load()
    size = load.tn_mesh_scalar_gradient_workspace_bytes
    limit = (2 ** 31 - 1) // 3
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(2 ** 31, 0) == 0 and size(8, limit + 1) == 0
    assert size(0, 0) > 0 and size(8, 12) > 0 and size(2 ** 31 - 1, limit) > 0
    assert size(8, 12) >= 12 * 32 + 32 and size(5, 70000) >= 70000 * 32 + 274 * 32
    assert load.tn_mesh_scalar_gradient(None, None, None, 12, 8, None, None, None, None, None, None, None, 0, None) == -1  # TN_ERR_NULL
    assert load.tn_mesh_scalar_smooth(None, None, 12, 8, None, None, 1, 0.5, 0.0, 0, None, None, None) == -1
    assert load.tn_mesh_scalar_smooth(None, None, 0, -1, None, None, 1, 0.5, 0.0, 0, None, None, None) == -2  # TN_ERR_SHAPE
    assert load.tn_mesh_scalar_smooth(None, None, 0, 0, None, None, -1, 0.5, 0.0, 0, None, None, None) == -2
    assert load.tn_mesh_scalar_smooth(None, None, 0, 0, None, None, 1, math.nan, 0.0, 0, None, None, None) == -3  # TN_ERR_UNSUPPORTED
    assert load.tn_mesh_scalar_smooth(None, None, 0, 0, None, None, 1, 0.5, math.inf, 0, None, None, None) == -3
    assert load.tn_mesh_scalar_smooth(None, None, 0, 0, None, None, 1, 0.5, 0.0, 0, None, None, None) == 0  # no vertices: nothing to do


def test_python_layer_exports_and_refuses_before_it_reaches_a_kernel():
    import torch

    from thermo_nerf_amd import export
    from thermo_nerf_amd.export import ThermalMesh

    for name in ("smooth_values", "smooth_temperature", "fill_temperature", "scalar_gradient", "thermal_gradient", "MeshGradient"):
        assert hasattr(export, name), name
    assert {"face_gradient", "vertex_gradient", "mesh", "usable_faces", "mean_magnitude", "max_magnitude"} == \
        {f.name for f in __import__("dataclasses").fields(export.MeshGradient)}
    pos, tri = torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    mesh = ThermalMesh(pos, torch.zeros((3, 3), dtype=torch.uint8), torch.zeros(3), None, tri)
    for call in (lambda: export.smooth_values(mesh.temperature, tri, 3, -1), lambda: export.smooth_temperature(mesh, -1),
                 lambda: export.thermal_gradient(mesh, smooth_iterations=-1), lambda: export.fill_temperature(mesh, -1)):
        with pytest.raises(ValueError, match="iterations"):
            call()
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError, match="finite"):
            export.smooth_values(mesh.temperature, tri, 3, 1, lambda_=bad)
        with pytest.raises(ValueError, match="finite"):
            export.thermal_gradient(mesh, 1, mu=bad)
    with pytest.raises(ValueError, match="no triangles"):
        export.thermal_gradient(types.SimpleNamespace(triangles=None))
    for call in (lambda: export.thermal_gradient(mesh), lambda: export.smooth_temperature(mesh, 1), lambda: export.fill_temperature(mesh, 1),
                 lambda: export.scalar_gradient(pos, mesh.temperature, tri)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_gradient_tool", os.path.join(ROOT, "tools", "mesh_gradient.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_arguments_and_help(capsys):
    tool = _tool()
    args = tool.parse(["mesh.ply", "--output", "g.ply", "--report", "g.json"])
    assert (args.smooth_iterations, args.lambda_, args.mu, args.fill, args.min_gradient, args.length_scale, args.smoothed) == \
        (0, 0.5, 0.0, 0, None, 1.0, None)
    args = tool.parse(["mesh.ply", "--output", "g.ply", "--report", "g.json", "--smooth-iterations", "5", "--lambda", "0.4", "--mu", "-0.43",
                       "--fill", "8", "--min-gradient", "5", "--min-area", "0.25", "--top", "3", "--length-scale", "0.5", "--smoothed", "s.ply"])
    assert (args.smooth_iterations, args.lambda_, args.mu, args.fill, args.min_gradient, args.min_area, args.top, args.length_scale) == \
        (5, 0.4, -0.43, 8, 5.0, 0.25, 3, 0.5) and str(args.smoothed) == "s.ply"
    base = ["mesh.ply", "--output", "g.ply", "--report", "g.json"]
    for bad in (["--smooth-iterations", "-1"], ["--fill", "-1"], ["--lambda", "nan"], ["--mu", "inf"], ["--min-gradient", "-1"],
                ["--min-area", "1"], ["--top", "2"], ["--length-scale", "0"], ["--min-gradient", "1", "--top", "-1"]):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
    with pytest.raises(SystemExit):
        tool.parse(["mesh.ply", "--report", "g.json"])  # --output is required
    capsys.readouterr()
    with pytest.raises(SystemExit) as stop:
        tool.parse(["--help"])
    assert stop.value.code == 0 and "--min-gradient" in capsys.readouterr().out


def test_report_scales_gradients_by_the_length_scale():
    tool = _tool()
    args = tool.parse(["mesh.ply", "--output", "g.ply", "--report", "g.json", "--length-scale", "0.5", "--fill", "2"])
    gradient = types.SimpleNamespace(usable_faces=7, mean_magnitude=3.0, max_magnitude=8.0)
    report = tool.build_report(gradient, None, 9, 8, 4, 1, args)
    assert report["mean_gradient"] == 6.0 and report["max_gradient"] == 16.0 and report["nan_vertices"] == {"before": 4, "after": 1}
    assert report["counts"] == {"vertices": 9, "faces": 8, "usable_faces": 7} and "steep" not in report
    nothing = tool.build_report(types.SimpleNamespace(usable_faces=0, mean_magnitude=math.nan, max_magnitude=math.nan), None, 9, 8, 9, 9, args)
    assert nothing["mean_gradient"] is None and nothing["max_gradient"] is None
