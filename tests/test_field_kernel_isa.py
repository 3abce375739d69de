"""Static checks on the compiled field kernel (no GPU: hipcc cross-compiles to gfx950 assembly, tools/isa_census.py reads it).

main_mfma_rays_kernel<true, false> (the benchmark's kernel) and <true, true> (its sample-split form) must fit the register file of
two waves per SIMD without scratch, their per-sample loop must hold exactly the matrix work DESIGN.md §5.2 accounts for, and the
phase stamps of tools/field_stamps.py must be absent from the shipped object."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

pytestmark = pytest.mark.skipif(isa_census.hipcc() is None, reason="hipcc not installed")

SOURCE = os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_render_mfma.hip")


@pytest.fixture(scope="module")
def kernels():
    found = isa_census.census(SOURCE, "main_mfma_rays_kernel<true,")
    by_name = {}
    for k in found:
        by_name["split" if "<true, true>" in k["name"] else "whole"] = k
    assert set(by_name) == {"split", "whole"}, [k["name"] for k in found]
    return by_name


@pytest.mark.parametrize("form", ["whole", "split"])
def test_registers_and_scratch(kernels, form):
    k = kernels[form]
    print(form, "vgpr", k["vgpr"], "agpr", k["agpr"], "allocated", k["vgpr_total"], "scratch", k["scratch"])
    assert k["scratch"] == 0
    assert k["vgpr_total"] is not None and k["vgpr_total"] <= 256  # two waves per SIMD share 512 registers


@pytest.mark.parametrize("form", ["whole", "split"])
def test_sample_loop_matrix_work(kernels, form):
    ops = isa_census.sample_loop(kernels[form])["ops"]
    print(form, {op: c for op, c in ops.items() if op.startswith(("v_mfma", "s_memtime", "s_nop", "s_waitcnt"))})
    assert ops.get("v_mfma_f32_32x32x2_f32", 0) == 384
    assert ops.get("v_mfma_f32_16x16x4_f32", 0) == 64
    assert sum(c for op, c in ops.items() if op.startswith("v_mfma")) == 448  # and no other matrix instruction


@pytest.mark.parametrize("form", ["whole", "split"])
def test_no_stamps_in_the_shipped_kernel(kernels, form):
    for lp in kernels[form]["loops"]:
        assert not any(op.startswith(("s_memtime", "s_memrealtime")) for op in lp["ops"]), lp["label"]
