"""Static bar on the compiled gfx950 code of the forward per-Gaussian kernel (csrc/preprocess.hip, hipcc cross-compiles without a GPU): the
two hot instantiations (fused SH, dc / rest) spill no VGPR, use no scratch and fit the three-waves-per-SIMD register budget; the generic
instantiation every other call form runs is still emitted for both SH layouts.  Read from the code-object metadata and the kernel list that
`tools/isa_audit.py preprocess_forward` reports -- no search for particular instructions."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# A SIMD of gfx950 has 512 VGPRs per lane, handed out in granules of 8: three waves get floor(512 / 3 / 8) * 8 = 168 each.  A property of the
# part, not a measurement.
VGPR_BUDGET_3_WAVES = 512 // 3 // 8 * 8


@pytest.fixture(scope="module")
def rows():
    import isa_audit
    return isa_audit.preprocess_forward()


def test_hot_instantiations_fit_three_waves_without_spills(rows):
    assert VGPR_BUDGET_3_WAVES == 168
    hot = [r for r in rows if r["form"] == "hot"]
    assert sorted(r["split_sh"] for r in hot) == [False, True], [r["kernel"] for r in rows]
    for r in hot:
        assert r["vgpr_spill_count"] == 0 and r["scratch_bytes"] == 0, r
        assert 0 < r["vgprs"] + r["agprs"] <= VGPR_BUDGET_3_WAVES, r
        assert r["lds_bytes"] * 3 <= 160 * 1024, r      # three workgroups (one wave per SIMD each) share a CU's LDS


def test_generic_instantiation_is_still_emitted(rows):
    generic = [r for r in rows if r["form"] == "generic"]
    assert sorted(r["split_sh"] for r in generic) == [False, True], [r["kernel"] for r in rows]
    for r in generic:
        assert r["vgpr_spill_count"] == 0 and r["scratch_bytes"] == 0 and 0 < r["vgprs"] <= 256, r
    assert len(rows) == 4, [r["kernel"] for r in rows]
