"""Static properties of the compiled gfx950 code of csrc/distortion.hip (the kernels behind gsr_distortion / gsr_distortion_backward): register and LDS
use, the call of tests/test_feature_geometry_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md 5.8; the bounds are
the design's: no register spilled to scratch, at most 128 VGPRs (four waves per SIMD stay possible), LDS = the tables the kernels declare -- the record
table (2 KB) for the forward, the record table and the parked sums (2 KB each) for the walk."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

LDS = {"distortion_map": 2048, "distortion_walk": 2048 + 2048}
VGPRS = {"distortion_map": 52, "distortion_walk": 67}


def kernel(name):
    found = [k for k in LDS if name.startswith(k + "E")]
    assert len(found) == 1, name
    return found[0]


def test_distortion_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "distortion.hip"), isa_audit.UNITS["distortion.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(LDS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        k = kernel(name)
        assert spills == 0, f"distortion.hip:{name}: {spills} spilled VGPRs"
        assert lds == LDS[k], (name, lds)
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == VGPRS[k], f"distortion.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.8 records {VGPRS[k]}: update both"
