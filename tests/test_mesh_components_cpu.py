"""The yardstick of the mesh components kernels (tests/mesh_components_reference.py) checked on its own: hand-written cases with
every expected array written out, a breadth-first search on random sparse meshes, and the command line's new flags.  No GPU."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

from tests import mesh_components_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.LITERAL))
def test_yardstick_on_the_literal_cases(name):
    case = R.LITERAL[name]
    tri, v = R.literal_triangles(case), case["num_vertices"]
    comp = R.components(tri, v)
    assert comp["labels"].dtype == np.int32 and comp["labels"].tolist() == case["labels"]
    assert comp["component_triangles"].dtype == np.int32 and comp["component_triangles"].tolist() == case["component_triangles"]
    assert comp["summary"].dtype == np.int64 and comp["summary"].tolist() == case["summary"]
    for (min_triangles, largest_only), want in case["filters"].items():
        got = R.filter_components(tri, v, comp, min_triangles, largest_only)
        assert got["vertex_source"].tolist() == want["vertex_source"], (min_triangles, largest_only)
        assert got["triangles"].tolist() == want["triangles"], (min_triangles, largest_only)
        assert got["counts"].tolist() == [len(want["vertex_source"]), len(want["triangles"])]


def test_yardstick_equals_a_breadth_first_search_on_random_sparse_meshes():
    rng = np.random.default_rng(5)
    sizes = set()
    for seed in range(300):
        v = int(rng.integers(1, 120))
        t = int(rng.integers(0, 2 * v + 1))
        tri = R.random_mesh(seed, v, t, invalid=0.1)
        comp = R.components(tri, v)
        labels = comp["labels"]
        assert np.array_equal(labels, R.bfs_labels(tri, v)), seed
        # the counts by their definition, one triangle at a time
        count = np.zeros(v, dtype=np.int64)
        for row in tri[R.valid_mask(tri, v)]:
            count[labels[row[0]]] += 1
        assert np.array_equal(comp["component_triangles"], count), seed
        assert comp["summary"].tolist() == [int((labels == np.arange(v)).sum()), int(count.max()), int(np.argmax(count))], seed
        sizes.update(count[count > 0].tolist())
        # the filter: kept triangles, mapped back through vertex_source, are the valid input triangles of kept components, in order
        for min_triangles, largest_only in ((1, False), (3, False), (2, True)):
            got = R.filter_components(tri, v, comp, min_triangles, largest_only)
            src = got["vertex_source"]
            assert np.all(np.diff(src) > 0)
            kept = (count[labels[src]] >= min_triangles) if len(src) else np.zeros(0, dtype=bool)
            assert kept.all() and (not largest_only or (labels[src] == comp["summary"][2]).all())
            want = [row.tolist() for row in tri[R.valid_mask(tri, v)]
                    if count[labels[row[0]]] >= min_triangles and (not largest_only or labels[row[0]] == comp["summary"][2])]
            assert src[got["triangles"]].reshape(-1, 3).tolist() == want, (seed, min_triangles, largest_only)
            assert set(np.unique(got["triangles"]).tolist()) == set(range(len(src))), "a kept vertex belongs to a kept triangle"
    assert len(sizes) > 10, "the random meshes have components of many sizes"


def test_export_mesh_parses_the_component_flags_and_they_default_to_off(capsys):
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(ROOT, "tools", "export_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["run", "data", "--output", "mesh.ply"]
    args = tool.parse(base)
    assert args.min_component_triangles == 0 and args.largest_component is False
    args = tool.parse(base + ["--min-component-triangles", "200", "--largest-component"])
    assert args.min_component_triangles == 200 and args.largest_component is True
    with pytest.raises(SystemExit):
        tool.parse(base + ["--min-component-triangles", "-1"])
    assert "--min-component-triangles" in capsys.readouterr().err
