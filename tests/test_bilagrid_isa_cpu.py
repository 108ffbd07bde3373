"""Static properties of the compiled gfx950 code of csrc/bilagrid.hip (the kernels behind gsr_bilagrid_*): register and LDS use, the call of
tests/test_mcmc_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md 5.10; the bounds are the design's: no
register spilled to scratch, at most 128 VGPRs (four waves per SIMD stay possible), LDS no larger than stated there."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel (the start of its mangled name behind the namespace) -> (VGPRs, LDS bytes)
KERNELS = {
    "bilagrid_slice_kernelE": (61, 12288),
    "bilagrid_slice_bwd_kernelILi16ELb1E": (69, 15360),
    "bilagrid_slice_bwd_kernelILi16ELb0E": (56, 12288),
    "bilagrid_slice_bwd_kernelILi64ELb1E": (122, 61440),
    "bilagrid_slice_bwd_kernelILi64ELb0E": (58, 49152),
    "bilagrid_reduce_kernelE": (48, 0),
    "bilagrid_tv_kernelE": (22, 2048),
    "bilagrid_tv_sum_kernelE": (10, 2048),
    "bilagrid_tv_bwd_kernelE": (46, 0),
}


def kernel(name):
    found = [k for k in KERNELS if name.startswith(k)]
    assert len(found) == 1, name
    return found[0]


def test_bilagrid_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "bilagrid.hip"), isa_audit.UNITS["bilagrid.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(KERNELS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert spills == 0, f"bilagrid.hip:{name}: {spills} spilled VGPRs"
        assert lds <= want_lds, f"bilagrid.hip:{name}: {lds} bytes of LDS, DESIGN.md 5.10 states {want_lds}"
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == want_vgpr, f"bilagrid.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.10 records {want_vgpr}: update both"
