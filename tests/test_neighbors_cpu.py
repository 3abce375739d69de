"""CPU: the numpy restatement of the neighbour search, outlier removal and normals (tests/neighbors_reference.py) on an analytic
cloud, the PLY layout with normals, ``ThermalPointCloud.select`` with normals, and the new command-line flags."""
import importlib.util
import os
import struct

import numpy as np
import pytest
import torch

from tests import neighbors_reference as R
from thermo_nerf_amd.export import ThermalPointCloud, read_ply, write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8

PLAIN = ("property float x", "property float y", "property float z", "property uchar red", "property uchar green",
         "property uchar blue", "property float temperature")
WITH_NORMALS = PLAIN[:3] + ("property float nx", "property float ny", "property float nz") + PLAIN[3:]


@pytest.fixture(scope="module")
def sphere():
    """1500 + 9 points, the reference's neighbours at k = 8 and its normals towards viewpoints at 3 x the radial position"""
    cloud = R.sphere_cloud()
    p = cloud["positions"]
    nn = R.knn(p, K)
    view = (3.0 * p.astype(np.float64)).astype(np.float32)
    return dict(cloud, nn=nn, view=view, normals=R.normals(p, nn["index"], view))


def test_reference_rows_are_sorted_exclude_the_point_and_break_ties_by_index(sphere):
    idx, d2 = sphere["nn"]["index"], sphere["nn"]["d2"]
    n = len(idx)
    assert (idx >= 0).all() and (idx != np.arange(n)[:, None]).all()
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    lattice = R.lattice_cloud()
    nn = R.knn(lattice, 6)
    tied = (np.diff(nn["d2"], axis=1) == 0)
    assert tied.any(axis=1).all(), "every row of the lattice has tied distances"
    assert (np.diff(nn["index"], axis=1)[tied] > 0).all(), "a tie goes to the lower index"
    # fewer than k others: the rest of the row is -1 / +inf and there is no mean distance
    few = R.knn(lattice[:4], 6)
    assert (few["index"][:, 3:] == -1).all() and np.isinf(few["d2"][:, 3:]).all() and np.isinf(few["mean_distance"]).all()
    assert (few["index"][:, :3] >= 0).all()


def test_reference_removes_exactly_the_outliers_at_ratio_3(sphere):
    p, outlier = sphere["positions"], sphere["outlier"]
    m = sphere["nn"]["mean_distance"]
    assert outlier.sum() == 9 and np.isfinite(m).all()
    keep = R.outlier_keep(p, K + 1, 3.0, mean_distance=m)
    assert np.array_equal(~keep, outlier)
    assert np.array_equal(~R.outlier_keep(p, K + 1, 1.0, mean_distance=m), outlier)
    loose = R.outlier_keep(p, K + 1, 10.0, mean_distance=m)
    assert 0 < (~loose).sum() <= 9 and not (~loose & ~outlier).any()
    for ratio in (1.0, 3.0, 10.0):  # the band the device test relies on
        tau = R.outlier_threshold(m, ratio)[2]
        assert np.abs(m - tau).min() > 1e-9 * tau
    # fewer finite points than the statistic needs: only the non-finite ones go
    q = p[:6].copy()
    q[2, 1] = np.nan
    assert np.array_equal(R.outlier_keep(q, 20, 3.0), np.arange(6) != 2)


def test_reference_normals_follow_the_sphere_and_point_outward(sphere):
    p, outlier, out = sphere["positions"], sphere["outlier"], sphere["normals"]
    nrm = out["normals"]
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    angle = R.angle_to_radial_deg(p[~outlier], nrm[~outlier])
    print("median angle to the radial direction", float(np.median(angle)), "smallest eigenvalue gap", float(out["gap"].min()))
    assert np.median(angle) <= 3.0
    # viewpoints at 3 x the radial position: every normal points away from the centre
    assert ((nrm.astype(np.float64) * p.astype(np.float64)).sum(axis=1)[~outlier] > 0).all()
    assert (out["s"] > 0).all()
    # without viewpoints the largest component is positive; degenerate rows have no normal
    free = R.normals(p[:200], R.knn(p[:200], K)["index"])["normals"]
    big = np.abs(free).argmax(axis=1)
    assert (free[np.arange(200), big] > 0).all()
    q = p[:200].copy()
    q[1, 0] = np.inf  # a non-finite point: in nobody's row, no normal
    idx = R.knn(q, K)["index"]
    assert (idx[1] == -1).all() and (idx != 1).all()
    idx[0, 1:] = -1   # one valid neighbour: too few
    deg = R.normals(q, idx)["normals"]
    assert (deg[0] == 0).all() and (deg[1] == 0).all() and (np.abs(deg[2:]).max(axis=1) > 0).all()


def _cloud(m, normals, seed=0):
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize(torch.randn((m, 3), generator=g), dim=1) if normals else None
    return ThermalPointCloud(positions=torch.randn((m, 3), generator=g) * 7.0,
                             colors=torch.randint(0, 256, (m, 3), generator=g, dtype=torch.uint8),
                             temperature=torch.rand((m,), generator=g) * 19.5 + 14.0,
                             thermal_colors=torch.randint(0, 256, (m, 3), generator=g, dtype=torch.uint8),
                             source=torch.arange(m, dtype=torch.int64), temperature_bounds=(14.0, 33.5), normals=nrm)


def _header(m, properties):
    return ("\n".join(["ply", "format binary_little_endian 1.0", "comment temperature_unit celsius",
                       "comment temperature_bounds 14.0 33.5", f"element vertex {m}", *properties, "end_header"]) + "\n").encode("ascii")


@pytest.mark.parametrize("m", [0, 1, 257])
def test_ply_round_trip_with_and_without_normals(tmp_path, m):
    with_n, without = _cloud(m, True), _cloud(m, False)
    # without normals: the bytes of the 19-byte layout, built here field by field
    blob = write_ply(tmp_path / "plain.ply", without).read_bytes()
    want = _header(m, PLAIN)
    for i in range(m):
        want += struct.pack("<fffBBBf", *without.positions[i].tolist(), *without.colors[i].tolist(), float(without.temperature[i]))
    assert blob == want
    assert "normals" not in read_ply(tmp_path / "plain.ply")
    # with normals: nx ny nz between z and red, 31 bytes per vertex
    blob = write_ply(tmp_path / "normals.ply", with_n).read_bytes()
    want = _header(m, WITH_NORMALS)
    for i in range(m):
        want += struct.pack("<ffffffBBBf", *with_n.positions[i].tolist(), *with_n.normals[i].tolist(), *with_n.colors[i].tolist(),
                            float(with_n.temperature[i]))
    assert blob == want and len(blob) == len(_header(m, WITH_NORMALS)) + 31 * m
    back = read_ply(tmp_path / "normals.ply")
    assert back["normals"].dtype == np.float32 and back["normals"].shape == (m, 3)
    assert np.array_equal(back["normals"], with_n.normals.numpy())
    assert np.array_equal(back["positions"], with_n.positions.numpy()) and np.array_equal(back["colors"], with_n.colors.numpy())
    assert np.array_equal(back["temperature"], with_n.temperature.numpy())
    assert back["comments"] == ["temperature_unit celsius", "temperature_bounds 14.0 33.5"]
    if m:
        short = tmp_path / "short.ply"
        short.write_bytes(blob[:-1])
        with pytest.raises(ValueError):
            read_ply(short)
        with pytest.raises(ValueError):
            write_ply(tmp_path / "bad.ply", ThermalPointCloud(with_n.positions, with_n.colors, with_n.temperature,
                                                              normals=torch.zeros((m + 1, 3))))


def test_select_carries_normals_and_positional_construction_stays_valid():
    cloud = _cloud(10, True)
    index = torch.tensor([7, 2, 2, 9])
    picked = cloud.select(index)
    assert torch.equal(picked.normals, cloud.normals[index]) and torch.equal(picked.positions, cloud.positions[index])
    assert torch.equal(picked.source, index) and picked.temperature_bounds == (14.0, 33.5)
    assert torch.equal(cloud.select(slice(2, 5)).normals, cloud.normals[2:5])
    assert _cloud(10, False).select(index).normals is None
    # the six fields of before, by position; normals is the seventh
    old = ThermalPointCloud(cloud.positions, cloud.colors, cloud.temperature, cloud.thermal_colors, cloud.source, (1.0, 2.0))
    assert old.normals is None and old.temperature_bounds == (1.0, 2.0) and old.source is cloud.source
    assert [f for f in ThermalPointCloud.__dataclass_fields__][-1] == "normals"


def _tool():
    spec = importlib.util.spec_from_file_location("export_pointcloud", os.path.join(ROOT, "tools", "export_pointcloud.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_outlier_and_normal_flags(capsys):
    tool = _tool()
    base = ["run", "data", "--output", "c.ply"]
    args = tool.parse(base)
    assert args.remove_outliers is False and args.normals is False
    assert args.outlier_neighbors == 20 and args.outlier_std_ratio == 10.0 and args.normal_neighbors == 30
    args = tool.parse(base + ["--remove-outliers", "--outlier-neighbors", "12", "--outlier-std-ratio", "2.5", "--normals",
                              "--normal-neighbors", "16"])
    assert args.remove_outliers and args.normals
    assert args.outlier_neighbors == 12 and args.outlier_std_ratio == 2.5 and args.normal_neighbors == 16
    for bad in (["--outlier-neighbors", "1"], ["--outlier-neighbors", "34"], ["--outlier-neighbors", "many"],
                ["--outlier-std-ratio", "0"], ["--outlier-std-ratio", "-1"], ["--outlier-std-ratio", "nan"],
                ["--normal-neighbors", "1"], ["--normal-neighbors", "33"], ["--remove-outliers", "yes"]):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
    capsys.readouterr()
