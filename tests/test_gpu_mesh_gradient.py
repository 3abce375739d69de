"""tn_mesh_scalar_smooth / tn_mesh_scalar_gradient on the device against tests/mesh_gradient_reference.py, exactly (integers, float and
double bit patterns), into guarded buffers: the cases known by hand, sizes around the block, the long list of a fan, the faces and
vertices that are not usable, the smoothing passes with holes, the totals over one and two levels of blocks, empty meshes, the error
codes, a foreign index, the Python layer and the command line."""
from __future__ import annotations

import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_gradient_reference as R
from tests import mesh_reference, mesh_smooth_reference
from tests.mesh_closest_reference import plane_grid
from tests.mesh_components_reference import random_mesh
from thermo_nerf_amd import _hip
from thermo_nerf_amd.export import (MeshIncidence, ThermalMesh, build_mesh_bvh, fill_temperature, fit_view, mesh_difference, mesh_incidence,
                                    mesh_thermogram, read_mesh_ply, scalar_gradient, smooth_temperature, smooth_values, thermal_gradient,
                                    thermal_regions, write_mesh_ply)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
GUARD = 96  # elements behind every output buffer that must keep their pattern
FLOAT_FILL, BYTE_FILL = -777.0, 0xEE


def _buffer(n, dtype=torch.float32):
    return torch.full((n + GUARD,), FLOAT_FILL, dtype=dtype, device=DEV)


def _guard_kept(buf, used, name):
    assert bool((buf.reshape(-1)[used:] == FLOAT_FILL).all()), f"{name} was written beyond element {used}"


def _same_bits(got, want, name):
    got, want = R.bits(got.cpu().numpy()).reshape(-1), R.bits(np.asarray(want)).reshape(-1)
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, f"{name}: {len(wrong)} of {len(want)} differ, the first at {wrong[:5].tolist()}"


def indexed(tri, v):
    """(device triangles, the device index, the yardstick's index) of one mesh"""
    dev_tri = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)).to(DEV)
    return dev_tri, mesh_incidence(dev_tri, v), R.incidence(tri, v)


def run_gradient(pos, values, tri, dev_tri, index, want_index, with_faces=True, want=None):
    """tn_mesh_scalar_gradient into guarded buffers, compared to the yardstick bit for bit; returns the yardstick's result"""
    v, t = len(pos), len(tri)
    dev_pos, dev_val = torch.from_numpy(pos).to(DEV), torch.from_numpy(values).to(DEV)
    face, vertex, magnitude, totals = _buffer(3 * t, torch.float64), _buffer(3 * v), _buffer(v), _buffer(4, torch.float64)
    lib = _hip.load()
    need = lib.tn_mesh_scalar_gradient_workspace_bytes(v, t)
    workspace = torch.full((need + 64,), BYTE_FILL, dtype=torch.uint8, device=DEV)
    _hip.check(lib.tn_mesh_scalar_gradient(dev_pos.data_ptr() if v else None, dev_val.data_ptr() if v else None,
                                           dev_tri.data_ptr() if t else None, t, v, index.offsets.data_ptr(),
                                           index.corners.data_ptr() if t else None, face.data_ptr() if with_faces else None,
                                           vertex.data_ptr(), magnitude.data_ptr(), totals.data_ptr(), workspace.data_ptr(), need,
                                           _hip.current_stream()), "tn_mesh_scalar_gradient")
    want = R.gradient(pos, values, tri, want_index) if want is None else want
    if with_faces:
        _same_bits(face[:3 * t], want["face_gradient"], "face_gradient")
    _guard_kept(face, 3 * t if with_faces else 0, "face_gradient")
    _same_bits(vertex[:3 * v], want["vertex_gradient"], "vertex_gradient")
    _same_bits(magnitude[:v], want["vertex_magnitude"], "vertex_magnitude")
    _same_bits(totals[:4], want["totals"], "totals")
    for buf, used, name in ((vertex, 3 * v, "vertex_gradient"), (magnitude, v, "vertex_magnitude"), (totals, 4, "totals")):
        _guard_kept(buf, used, name)
    assert bool((workspace[need:] == BYTE_FILL).all()), "written beyond the workspace"
    if v:
        _same_bits(dev_pos, pos, "positions (an input was written)")
        _same_bits(dev_val, values, "values (an input was written)")
    return want


def run_smooth(values, tri, dev_tri, index, want_index, iterations, lambda_=0.5, mu=0.0, fill=False, in_place=False, want=None):
    v, t = len(values), len(tri)
    out, scratch = _buffer(v), _buffer(v)
    if in_place:
        out[:v] = torch.from_numpy(values).to(DEV)
        dev_val = out
    else:
        dev_val = torch.from_numpy(values).to(DEV)
    _hip.check(_hip.load().tn_mesh_scalar_smooth(dev_val.data_ptr() if v else None, dev_tri.data_ptr() if t else None, t, v,
                                                 index.offsets.data_ptr(), index.corners.data_ptr() if t else None, iterations, lambda_, mu,
                                                 1 if fill else 0, out.data_ptr(), scratch.data_ptr(), _hip.current_stream()),
               "tn_mesh_scalar_smooth")
    want = R.smooth(values, tri, want_index, iterations, lambda_, mu, fill) if want is None else want
    _same_bits(out[:v], want, f"values after {iterations} iterations (lambda {lambda_}, mu {mu}, fill {fill}, in place {in_place})")
    _guard_kept(out, v, "values_out")
    _guard_kept(scratch, v, "scratch")
    if not in_place and v:
        _same_bits(dev_val, values, "values_in was written")
    return want


def spoiled_values(seed, n, share=0.05):
    """degrees with a few NaNs and infinities among them"""
    rng = np.random.default_rng(seed + 1000)
    values = R.random_values(seed, n)
    bad = rng.uniform(size=n) < share
    values[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), size=int(bad.sum()))
    return values


def check_mesh(pos, values, tri):
    """the gradient and two smoothing runs of one mesh, each exact"""
    dev_tri, index, want_index = indexed(tri, len(pos))
    run_gradient(pos, values, tri, dev_tri, index, want_index)
    run_smooth(values, tri, dev_tri, index, want_index, 1, fill=True)
    run_smooth(values, tri, dev_tri, index, want_index, 2, mu=-0.53)
    return dev_tri, index, want_index


# ---- the cases known by hand --------------------------------------------------------------------------------------------------------------

def test_right_triangle_and_the_same_scaled_by_two():
    pos, tri = R.RIGHT_TRIANGLE
    values = np.array([0, 1, 0], F)
    for scale, slope in ((1.0, 1.0), (2.0, 0.5)):
        p = (pos * F(scale)).astype(F)
        dev_tri, index, want_index = indexed(tri, 3)
        want = run_gradient(p, values, tri, dev_tri, index, want_index)
        assert want["face_gradient"].tolist() == [[slope, 0.0, 0.0]] and want["vertex_gradient"].tolist() == [[slope, 0.0, 0.0]] * 3
        run_gradient(p, values, tri, dev_tri, index, want_index, with_faces=False)  # face_gradient may be NULL


def test_constant_field_and_the_linear_field_on_the_integer_lattice():
    pos, tri = R.lattice(5, 5)
    dev_tri, index, want_index = indexed(tri, 25)
    want = run_gradient(pos, np.full(25, 21.5, F), tri, dev_tri, index, want_index)
    assert (want["face_gradient"] == 0.0).all() and not R.bits(want["vertex_gradient"]).any() and not R.bits(want["vertex_magnitude"]).any()
    want = run_gradient(pos, (3 * pos[:, 0] - 2 * pos[:, 1]).astype(F), tri, dev_tri, index, want_index)
    assert (want["face_gradient"] == [3, -2, 0]).all() and (want["vertex_gradient"] == [3, -2, 0]).all()
    assert (want["vertex_magnitude"] == F(math.sqrt(13.0))).all() and want["totals"][0] == 32 and want["totals"][3] == math.sqrt(13.0)


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_face_and_vertex_counts_around_the_block(n):
    strip = mesh_smooth_reference.strip(n + 2)  # T = n
    assert len(strip) == n
    check_mesh(mesh_smooth_reference.random_positions(n, n + 2), spoiled_values(n, n + 2), strip)
    check_mesh(mesh_smooth_reference.random_positions(n + 1, n), spoiled_values(n + 1, n), random_mesh(n, n, 2 * n))  # V = n
    check_mesh(mesh_smooth_reference.random_positions(n + 2, 2 * n), spoiled_values(n + 2, 2 * n), random_mesh(n + 7, 2 * n, n))  # T = n


def test_fan_of_a_thousand_triangles_the_long_list():
    t = 1000
    tri = mesh_smooth_reference.fan(t)
    _, _, want_index = check_mesh(mesh_smooth_reference.random_positions(2, t + 2), R.random_values(2, t + 2), tri)
    assert int(want_index["offsets"][1]) == t, "vertex 0 lists a corner of every triangle"


def test_random_sparse_mesh_with_invalid_and_repeated_indices():
    v, t = 3000, 9000
    tri = random_mesh(23, v, t, invalid=0.05)
    pos = mesh_smooth_reference.random_positions(23, v)
    pos[::97, 1] = np.nan
    check_mesh(pos, spoiled_values(23, v), tri)
    assert bool((tri[:, 0] == tri[:, 1]).any()) and bool((tri < 0).any())


# ---- what is not usable -------------------------------------------------------------------------------------------------------------------

def test_unusable_faces_and_vertices_get_the_stated_nan():
    pos, tri = R.lattice(3, 3)
    values = np.arange(9, dtype=F)
    dev_tri, index, want_index = indexed(tri, 9)
    for spoil in (np.nan, np.inf, -np.inf):
        x = values.copy()
        x[0] = spoil
        want = run_gradient(pos, x, tri, dev_tri, index, want_index)
        assert want["faces"]["usable"].tolist() == [False, False] + [True] * 6
        assert R.bits(want["vertex_magnitude"][:1]).tolist() == [R.NAN32_BITS] and R.bits(want["face_gradient"][0]).tolist() == [R.NAN64_BITS] * 3
    p = pos.copy()
    p[0, 2] = -np.inf  # a coordinate that is not finite
    assert run_gradient(p, values, tri, dev_tri, index, want_index)["totals"][0] == 6
    p = pos.copy()
    p[0] = p[1]  # collinear corners: face 0 has no area, face 1 keeps one
    want = run_gradient(p, values, tri, dev_tri, index, want_index)
    assert want["faces"]["usable"].tolist() == [False] + [True] * 7 and np.isfinite(want["vertex_magnitude"]).all()
    # a vertex in no triangle (2, 4), a repeated index, an index outside the vertices
    other = np.array([(0, 1, 3), (1, 1, 3), (0, 1, 9)], np.int32)
    dev_tri, index, want_index = indexed(other, 5)
    want = run_gradient(pos[:5], values[:5], other, dev_tri, index, want_index)
    assert np.isnan(want["vertex_magnitude"]).tolist() == [False, False, True, False, True] and want["totals"][0] == 1


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------------

def test_smoothing_iterations_factors_in_place_and_out_of_place():
    mesh = mesh_reference.sphere_mesh()[1]
    tri, values = mesh["triangles"], np.ascontiguousarray(mesh["temperature"], F)
    dev_tri, index, want_index = indexed(tri, len(values))
    for mu in (0.0, -0.53):
        last = None
        for k in (0, 1, 2, 5):
            last = run_smooth(values, tri, dev_tri, index, want_index, k, 0.5, mu)
            run_smooth(values, tri, dev_tri, index, want_index, k, 0.5, mu, in_place=True, want=last)
        assert not np.array_equal(last, values)
    run_smooth(values, tri, dev_tri, index, want_index, 0, want=values)
    # the Python layer: the same values, a new tensor, the input left alone
    dev_val = torch.from_numpy(values).to(DEV)
    got = smooth_values(dev_val, dev_tri, len(values), 5, mu=-0.53, incidence=index)
    _same_bits(got, last, "smooth_values")
    _same_bits(dev_val, values, "smooth_values wrote its input")
    assert torch.equal(got, smooth_values(dev_val, dev_tri, len(values), 5, mu=-0.53))


def test_a_hole_closes_by_one_ring_per_pass_and_an_island_without_values_stays_empty():
    pos, tri = R.lattice(9, 9)
    island = (np.array([(0, 1, 2), (1, 3, 2)], np.int32) + 81)  # four more vertices, all NaN, joined to nothing else
    tri = np.concatenate([tri, island])
    hole = np.concatenate([R.hole(9, 9, 3, 3, 3), np.zeros(4, bool)])
    values = np.concatenate([R.random_values(3, 81), np.full(4, np.nan, F)])
    values[hole] = np.array([0x7fc00123], np.uint32).view(F)[0]  # a NaN with a payload
    dev_tri, index, want_index = indexed(tri, 85)
    one = run_smooth(values, tri, dev_tri, index, want_index, 1, 0.0, 0.0, fill=True)
    centre = np.zeros(85, bool)
    centre[4 * 9 + 4] = True
    assert np.isnan(one[:81]).tolist() == centre[:81].tolist(), "after one pass exactly the ring next to finite vertices is finite"
    two = run_smooth(values, tri, dev_tri, index, want_index, 2, 0.0, 0.0, fill=True)
    assert np.isfinite(two[:81]).all() and np.isnan(two[81:]).all()
    run_smooth(values, tri, dev_tri, index, want_index, 2, 0.0, 0.0, fill=True, in_place=True, want=two)
    kept = run_smooth(values, tri, dev_tri, index, want_index, 2, 0.5, -0.53, fill=False)
    assert R.bits(kept[hole]).tolist() == [0x7fc00123] * 9, "fill off leaves the input's bits"
    run_smooth(values, tri, dev_tri, index, want_index, 3, 0.5, 0.0, fill=True)
    # fill_temperature: the finite vertices keep their bits, one read says what remains
    positions = np.concatenate([pos, pos[:4] + F(20)])
    mesh = ThermalMesh(torch.from_numpy(positions).to(DEV), torch.zeros((85, 3), dtype=torch.uint8, device=DEV),
                       torch.from_numpy(values).to(DEV), torch.zeros((85, 3), dtype=torch.uint8, device=DEV), dev_tri, (14.0, 33.0))
    for passes, remain in ((1, 5), (2, 4), (6, 4)):
        filled, remaining = fill_temperature(mesh, passes)
        assert remaining == remain
        _same_bits(filled.temperature[:81][torch.from_numpy(~hole[:81]).to(DEV)], values[:81][~hole[:81]], "a finite vertex was moved")
    _same_bits(filled.temperature, two, "fill_temperature")
    assert filled.thermal_colors is None and filled.temperature_bounds == (14.0, 33.0) and filled.positions is mesh.positions
    assert filled.triangles is mesh.triangles and filled.colors is mesh.colors and mesh.thermal_colors is not None
    smoothed = smooth_temperature(mesh, 3, fill=True)
    _same_bits(smoothed.temperature, R.smooth(values, tri, want_index, 3, 0.5, 0.0, True), "smooth_temperature")
    assert smoothed.thermal_colors is None and smoothed.temperature_bounds == (14.0, 33.0)


# ---- the totals -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 256, 257, 70000])
def test_totals_over_one_and_two_levels_of_blocks(t):
    tri = mesh_smooth_reference.strip(t + 2)
    pos = mesh_smooth_reference.random_positions(t, t + 2)
    values = spoiled_values(t, t + 2, share=0.01)
    dev_tri, index, want_index = indexed(tri, t + 2)
    want = run_gradient(pos, values, tri, dev_tri, index, want_index)
    assert 0 < want["totals"][0] <= t and want["totals"][2] > 0.0 and (t < 70000 or want["totals"][0] < t)


# ---- empty meshes and the error codes ---------------------------------------------------------------------------------------------------

def test_no_vertices_or_no_triangles():
    none = np.zeros((0, 3), np.int32)
    for v, tri in ((0, none), (300, none), (0, np.array([[0, 1, 2], [3, 4, 5]], np.int32))):
        pos, values = mesh_smooth_reference.random_positions(5, v), R.random_values(5, v)
        dev_tri, index, want_index = indexed(tri, v)
        want = run_gradient(pos, values, tri, dev_tri, index, want_index)
        assert want["totals"].tolist() == [0.0] * 4 and np.isnan(want["vertex_magnitude"]).all()
        assert (R.bits(want["face_gradient"]) == R.NAN64_BITS).all()
        for k in (0, 2):
            run_smooth(values, tri, dev_tri, index, want_index, k, fill=True, want=values)


def test_error_codes_without_a_launch():
    lib = _hip.load()
    v, t = 700, 900
    tri_host = random_mesh(3, v, t)
    dev_tri, index, _ = indexed(tri_host, v)
    pos = torch.from_numpy(mesh_smooth_reference.random_positions(3, v)).to(DEV)
    values = torch.from_numpy(R.random_values(3, v)).to(DEV)
    stream = _hip.current_stream()
    out, scratch = _buffer(v), _buffer(v)
    face, vertex, magnitude, totals = _buffer(3 * t, torch.float64), _buffer(3 * v), _buffer(v), _buffer(4, torch.float64)
    need = lib.tn_mesh_scalar_gradient_workspace_bytes(v, t)
    ws = torch.full((need + 8,), BYTE_FILL, dtype=torch.uint8, device=DEV)
    limit = (2 ** 31 - 1) // 3
    shared = dict(triangles=dev_tri.data_ptr(), num_triangles=t, num_vertices=v, offsets=index.offsets.data_ptr(), corners=index.corners.data_ptr())

    smooth_names = ("values_in", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "iterations", "lambda_", "mu", "fill",
                    "values_out", "scratch")
    smooth_good = dict(shared, values_in=values.data_ptr(), iterations=2, lambda_=0.5, mu=-0.53, fill=1, values_out=out.data_ptr(),
                       scratch=scratch.data_ptr())

    def smooth(**change):
        args = dict(smooth_good, **change)
        return lib.tn_mesh_scalar_smooth(*[args[k] for k in smooth_names], stream)

    gradient_names = ("positions", "values", "triangles", "num_triangles", "num_vertices", "offsets", "corners", "face_gradient",
                      "vertex_gradient", "vertex_magnitude", "totals", "workspace", "workspace_bytes")
    gradient_good = dict(shared, positions=pos.data_ptr(), values=values.data_ptr(), face_gradient=face.data_ptr(),
                         vertex_gradient=vertex.data_ptr(), vertex_magnitude=magnitude.data_ptr(), totals=totals.data_ptr(),
                         workspace=ws.data_ptr(), workspace_bytes=need)

    def gradient(**change):
        args = dict(gradient_good, **change)
        return lib.tn_mesh_scalar_gradient(*[args[k] for k in gradient_names], stream)

    for call, good, pointers, wide in ((smooth, smooth_good, ("values_in", "triangles", "offsets", "corners", "values_out", "scratch"), ()),
                                       (gradient, gradient_good, ("positions", "values", "triangles", "offsets", "corners", "vertex_gradient",
                                                                  "vertex_magnitude", "totals", "workspace"), ("face_gradient", "totals", "workspace"))):
        for k in pointers:
            assert call(**{k: None}) == -1, k  # TN_ERR_NULL
        for k in pointers:
            if k not in wide:
                assert call(**{k: good[k] + 2}) == -2, k  # TN_ERR_SHAPE: not 4-byte aligned
        for k in wide:
            assert call(**{k: good[k] + 4}) == -2, k  # not 8-byte aligned
        assert call(num_vertices=-1) == -2 and call(num_vertices=2 ** 31) == -2
        assert call(num_triangles=-1) == -2 and call(num_triangles=limit + 1) == -2
    assert smooth(iterations=-1) == -2 and smooth(iterations=2 ** 30) == -2
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert smooth(lambda_=bad) == -3 and smooth(mu=bad) == -3  # TN_ERR_UNSUPPORTED
    assert smooth(scratch=out.data_ptr()) == -2 and smooth(scratch=values.data_ptr()) == -2  # scratch overlaps an end of the chain
    assert smooth(scratch=out.data_ptr() + 4 * (v - 1)) == -2 and smooth(values_out=values.data_ptr() + 4) == -2
    assert gradient(workspace_bytes=need - 1) == -4 and gradient(workspace_bytes=0) == -4  # TN_ERR_WORKSPACE
    torch.cuda.synchronize()
    for buf in (out, scratch, face, vertex, magnitude, totals):
        assert bool((buf == FLOAT_FILL).all()), "a refused call launched something"
    assert bool((ws == BYTE_FILL).all())
    assert smooth(lambda_=-0.5, mu=0.5) == 0 and gradient(face_gradient=None) == 0  # any finite pair; the rows are optional
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        smooth_values(values, dev_tri, v, 1, incidence=MeshIncidence(index.offsets[:-1], index.corners))
    with pytest.raises(ValueError):
        smooth_values(values[:-1], dev_tri, v, 1)
    with pytest.raises(ValueError):
        scalar_gradient(pos, values.reshape(-1, 1), dev_tri)
    with pytest.raises(TypeError):
        scalar_gradient(pos, values.double(), dev_tri)
    with pytest.raises(ValueError):
        scalar_gradient(pos, values, dev_tri, workspace=ws[:16])


def test_a_foreign_index_gives_other_numbers_and_writes_nothing_outside_the_arrays():
    v, t = 600, 1500
    tri, other = random_mesh(31, v, t), random_mesh(32, v, t)
    pos, values = mesh_smooth_reference.random_positions(31, v), spoiled_values(31, v)
    dev_tri, index, want_index = indexed(tri, v)
    _, foreign, want_foreign = indexed(other, v)
    own = run_gradient(pos, values, tri, dev_tri, index, want_index)
    got = run_gradient(pos, values, tri, dev_tri, foreign, want_foreign)
    assert not np.array_equal(R.bits(own["vertex_gradient"]), R.bits(got["vertex_gradient"]))
    _same_bits(torch.from_numpy(got["face_gradient"]), own["face_gradient"], "the faces do not read the lists")
    own = run_smooth(values, tri, dev_tri, index, want_index, 2, fill=True)
    got = run_smooth(values, tri, dev_tri, foreign, want_foreign, 2, fill=True)
    assert not np.array_equal(R.bits(own), R.bits(got))
    # lists that point outside the corners: offsets below 0 and beyond 3T, corners that do not exist
    wild = dict(offsets=want_foreign["offsets"].copy(), corners=want_foreign["corners"].copy())
    wild["offsets"][::7] = -3
    wild["offsets"][3::11] = 3 * t + 1000
    wild["corners"][::5] = 3 * t + 5
    wild["corners"][1::9] = -2
    dev_wild = MeshIncidence(torch.from_numpy(wild["offsets"]).to(DEV), torch.from_numpy(wild["corners"]).to(DEV))
    run_gradient(pos, values, tri, dev_tri, dev_wild, wild)
    run_smooth(values, tri, dev_tri, dev_wild, wild, 2, fill=True)


# ---- the Python layer and the command line ----------------------------------------------------------------------------------------------

def _sphere():
    mesh = mesh_reference.sphere_mesh()[1]
    pos, tri, temperature = mesh["positions"], mesh["triangles"], np.ascontiguousarray(mesh["temperature"], F)
    device_mesh = ThermalMesh(torch.from_numpy(pos).to(DEV), torch.zeros((len(pos), 3), dtype=torch.uint8, device=DEV),
                              torch.from_numpy(temperature).to(DEV), torch.zeros((len(pos), 3), dtype=torch.uint8, device=DEV),
                              torch.from_numpy(tri).to(DEV), (14.0, 33.0))
    return device_mesh, pos, tri, temperature


def test_thermal_gradient_of_the_sphere_mesh_feeds_regions_and_thermograms():
    mesh, pos, tri, temperature = _sphere()
    want_index = R.incidence(tri, len(pos))
    want = R.gradient(pos, temperature, tri, want_index)
    g = thermal_gradient(mesh)
    _same_bits(g.face_gradient, want["face_gradient"], "face_gradient")
    _same_bits(g.vertex_gradient, want["vertex_gradient"], "vertex_gradient")
    _same_bits(g.mesh.temperature, want["vertex_magnitude"], "the gradient mesh's temperature")
    count, weight, weighted, steepest = want["totals"].tolist()
    assert (g.usable_faces, g.mean_magnitude, g.max_magnitude) == (int(count), weighted / weight, steepest) and count == len(tri)
    assert g.mesh.temperature_bounds == (0.0, steepest) and g.mesh.thermal_colors is None and mesh.thermal_colors is not None
    assert g.mesh.positions is mesh.positions and g.mesh.colors is mesh.colors and g.mesh.triangles is mesh.triangles
    raw = scalar_gradient(mesh.positions, mesh.temperature, mesh.triangles)
    assert torch.equal(raw.vertex_magnitude, g.mesh.temperature) and torch.equal(raw.totals.cpu(), torch.from_numpy(want["totals"]))
    smoothed = thermal_gradient(mesh, smooth_iterations=3, lambda_=0.5, mu=-0.53)
    values = R.smooth(temperature, tri, want_index, 3, 0.5, -0.53)
    _same_bits(smoothed.mesh.temperature, R.gradient(pos, values, tri, want_index)["vertex_magnitude"], "the gradient of the smoothed degrees")
    # where it changes faster than the mean: regions of the gradient mesh; the gradient image
    steep = thermal_regions(g.mesh, min_temperature=g.mean_magnitude)
    assert steep.usable_faces == len(tri) and 0 < steep.selected_faces < len(tri) and len(steep) > 0
    assert all(row["min_temperature"] >= F(g.mean_magnitude) for row in steep.regions)
    image = mesh_thermogram(g.mesh, fit_view(mesh.positions, (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), width=48))
    shown = image.pixel_temperature[image.pixel_face >= 0]
    assert image.covered == shown.numel() > 100 and image.temperature_bounds == (0.0, steepest)
    assert bool((shown >= 0.0).all()) and float(shown.max()) <= steepest  # a vertex has the mean of its faces, a pixel of its vertices
    # nothing usable: no bounds, NaN statistics
    flat = ThermalMesh(mesh.positions, mesh.colors, torch.full_like(mesh.temperature, math.nan), None, mesh.triangles, (14.0, 33.0))
    none = thermal_gradient(flat)
    assert none.usable_faces == 0 and none.mesh.temperature_bounds is None and math.isnan(none.mean_magnitude) and math.isnan(none.max_magnitude)


def test_the_holes_of_a_difference_mesh_are_filled():
    pos, temperature, tri = plane_grid(8, 0.0, 20.0)
    colors = torch.zeros((len(pos), 3), dtype=torch.uint8, device=DEV)
    survey = ThermalMesh(torch.from_numpy(pos).to(DEV), colors, torch.from_numpy(temperature).to(DEV), None, torch.from_numpy(tri).to(DEV), (20.0, 40.0))
    centre = pos[tri.astype(np.int64)].mean(axis=1)
    outside = (np.abs(centre[:, 0] - 2.0) > 1.0) | (np.abs(centre[:, 1] - 2.0) > 1.0)  # the reference lacks the middle 4 x 4 cells
    reference = ThermalMesh(survey.positions, colors, torch.from_numpy((temperature + F(1.5)).astype(F)).to(DEV), None,
                            torch.from_numpy(np.ascontiguousarray(tri[outside])).to(DEV), (20.0, 40.0))
    delta = mesh_difference(survey, build_mesh_bvh(reference), max_distance=0.125).mesh
    missing = torch.isnan(delta.temperature).cpu().numpy()
    assert int(missing.sum()) == 9, "the 3 x 3 vertices inside the hole have no counterpart"
    touched = int(missing[tri.astype(np.int64)].any(axis=1).sum())
    before = thermal_regions(delta, max_temperature=0.0)
    assert touched > 0 and before.usable_faces == len(tri) - touched
    filled, remaining = fill_temperature(delta, 4)
    got, had = filled.temperature.cpu().numpy(), delta.temperature.cpu().numpy()
    assert remaining == 0 and R.bits(got[~missing]).tolist() == R.bits(had[~missing]).tolist()
    assert (got[missing] >= had[~missing].min()).all() and (got[missing] <= had[~missing].max()).all()  # means of what surrounds them
    after = thermal_regions(filled, max_temperature=0.0)
    assert after.usable_faces == len(tri) and after.mesh_area == 16.0 and len(after) == 1
    assert filled.temperature_bounds == delta.temperature_bounds


def _tool():
    spec = importlib.util.spec_from_file_location("mesh_gradient_tool", os.path.join(ROOT, "tools", "mesh_gradient.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_end_to_end_on_a_small_ply(tmp_path, capsys):
    pos, tri = R.lattice(9, 9)
    hole = R.hole(9, 9, 3, 3, 3)
    values = (20 + 3 * pos[:, 0] - 2 * pos[:, 1]).astype(F)
    values[pos[:, 0] >= 7] += F(40.0)  # a step of 40 degrees between x = 6 and x = 7
    spoiled = values.copy()
    spoiled[hole] = np.nan
    source = tmp_path / "mesh.ply"
    write_mesh_ply(source, ThermalMesh(torch.from_numpy(pos), torch.zeros((81, 3), dtype=torch.uint8), torch.from_numpy(spoiled), None,
                                       torch.from_numpy(tri), (14.0, 33.0)))
    tool = _tool()
    report_file, output, smoothed = tmp_path / "out" / "gradient.json", tmp_path / "gradient.ply", tmp_path / "smoothed.ply"
    common = [str(source), "--output", str(output), "--report", str(report_file), "--device", DEV]
    assert tool.main(common + ["--fill", "3", "--min-gradient", "10", "--smoothed", str(smoothed)]) == 0
    printed = capsys.readouterr().out
    print(printed)
    report = json.loads(report_file.read_text())
    assert {"mesh", "length_scale", "smooth_iterations", "lambda", "mu", "fill_passes", "counts", "nan_vertices", "mean_gradient",
            "max_gradient", "min_gradient", "steep", "mesh_area"} == set(report)
    assert report["counts"] == {"vertices": 81, "faces": 128, "usable_faces": 128} and report["nan_vertices"] == {"before": 9, "after": 0}
    index = R.incidence(tri, 81)
    degrees = R.smooth(spoiled, tri, index, 3, 0.0, 0.0, fill=True)
    want = R.gradient(pos, degrees, tri, index)
    assert report["max_gradient"] == want["totals"][3] and report["mean_gradient"] == want["totals"][2] / want["totals"][1]
    assert report["mesh_area"] == 64.0 and len(report["steep"]["regions"]) == 1 and report["steep"]["regions"][0]["max_gradient"] > 20.0
    assert "vertices without a temperature 9 -> 0" in printed and "steep 0:" in printed
    got = read_mesh_ply(output)
    assert R.bits(got["temperature"]).tolist() == R.bits(want["vertex_magnitude"]).tolist()
    assert got["positions"].tobytes() == pos.tobytes() and got["triangles"].tobytes() == tri.tobytes()
    assert R.bits(read_mesh_ply(smoothed)["temperature"]).tolist() == R.bits(degrees).tolist()
    # half a metre per unit: the gradients double, the areas are a quarter, the threshold is in degrees per metre
    assert tool.main(common + ["--fill", "3", "--min-gradient", "20", "--length-scale", "0.5"]) == 0
    scaled = json.loads(report_file.read_text())
    assert scaled["max_gradient"] == 2 * report["max_gradient"] and scaled["mean_gradient"] == 2 * report["mean_gradient"]
    assert scaled["mesh_area"] == 16.0 and scaled["steep"]["area"] == report["steep"]["area"] / 4
    assert [r["faces"] for r in scaled["steep"]["regions"]] == [r["faces"] for r in report["steep"]["regions"]]
    assert scaled["steep"]["regions"][0]["max_gradient"] == 2 * report["steep"]["regions"][0]["max_gradient"]
    assert read_mesh_ply(output)["temperature"].tobytes() == got["temperature"].tobytes(), "the mesh is not scaled"
    # without --fill the hole stays: fewer usable faces, the same count before and after
    assert tool.main(common + ["--smooth-iterations", "2"]) == 0
    plain = json.loads(report_file.read_text())
    touched = int(hole[tri.astype(np.int64)].any(axis=1).sum())
    assert plain["nan_vertices"] == {"before": 9, "after": 9} and plain["counts"]["usable_faces"] == 128 - touched < 128 and "steep" not in plain
