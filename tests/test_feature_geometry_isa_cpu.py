"""Static properties of the compiled gfx950 code of csrc/feature_geom.hip (the walk behind gsr_render_features_backward_geometry): register and LDS use,
the call of tests/test_features_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md 5.7; the bounds are the
design's: no register spilled to scratch, at most 128 VGPRs (four waves per SIMD stay possible), LDS = the record table (2 KB), the parked sums (2 KB) and the
feature rows of the group (64 rows of 16 NQ bytes)."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# feature_geom_walk<VEC4, NQ>: 4 NQ channels per walk; rows as float4 (VEC4) or float by float
LDS = {(vec, nq): 2048 + 2048 + 64 * 16 * nq for vec in (True, False) for nq in (1, 2, 4)}
VGPRS = {(True, 4): 114, (True, 2): 84, (True, 1): 77, (False, 4): 127, (False, 2): 94, (False, 1): 78}


def kernel(name):
    m = re.match(r"feature_geom_walkILb([01])ELi(\d)E", name)
    assert m, name
    return m.group(1) == "1", int(m.group(2))


def test_feature_geometry_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "feature_geom.hip"), isa_audit.UNITS["feature_geom.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(LDS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        k = kernel(name)
        assert spills == 0, f"feature_geom.hip:{name}: {spills} spilled VGPRs"
        assert lds == LDS[k], (name, lds)
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == VGPRS[k], f"feature_geom.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.7 records {VGPRS[k]}: update both"
