"""Static properties of the compiled gfx950 code of csrc/mcmc.hip (the kernels behind gsr_mcmc_inject_noise / gsr_mcmc_relocation): register and LDS
use, the call of tests/test_distortion_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md 5.9; the bounds are
the design's: no register spilled to scratch, no LDS at all (streaming kernels), at most 128 VGPRs (four waves per SIMD stay possible)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

VGPRS = {"mcmc_noise_kernel": 126, "mcmc_relocation_kernel": 38}


def kernel(name):
    found = [k for k in VGPRS if name.startswith(k + "E")]
    assert len(found) == 1, name
    return found[0]


def test_mcmc_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "mcmc.hip"), isa_audit.UNITS["mcmc.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(VGPRS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        k = kernel(name)
        assert spills == 0, f"mcmc.hip:{name}: {spills} spilled VGPRs"
        assert lds == 0, (name, lds)
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == VGPRS[k], f"mcmc.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.9 records {VGPRS[k]}: update both"
