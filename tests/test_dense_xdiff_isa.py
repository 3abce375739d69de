"""Static check (no GPU) that the dense levels' x-differences left the field kernel's sample loop.

The dense re-layout stores e(x+1,y,z) - e(x,y,z) beside every entry, so the first lerp stage of a dense level is one fma per corner
pair.  Before that the per-sample loop of main_mfma_rays_kernel<true, false> held 226 v_sub_f32 (tools/isa_census.py): 8 of them on
each of the 6 dense levels are gone, and the loop's matrix work and the kernel's scratch are what they were."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

pytestmark = pytest.mark.skipif(isa_census.hipcc() is None, reason="hipcc not installed")

SOURCE = os.path.join(ROOT, "thermo_nerf_amd", "csrc", "tn_render_mfma.hip")


def test_sample_loop_subtractions():
    found = isa_census.census(SOURCE, "main_mfma_rays_kernel<true, false>")
    assert len(found) == 1, [k["name"] for k in found]
    k = found[0]
    ops = isa_census.sample_loop(k)["ops"]
    subs = sum(c for op, c in ops.items() if op.startswith("v_sub_f32"))
    mfma = sum(c for op, c in ops.items() if op.startswith("v_mfma"))
    print("v_sub_f32", subs, "mfma", mfma, "scratch", k["scratch"])
    assert subs <= 226 - 8 * 6
    assert mfma == 448
    assert k["scratch"] == 0
