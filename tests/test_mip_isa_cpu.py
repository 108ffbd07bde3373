"""Static properties of the compiled gfx950 code of csrc/mip.hip (the kernels behind gsr_mip_filter_3d, gsr_mip_activations and its backward):
register and LDS use, the call of tests/test_normals_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md
5.12; the bounds are the design's: no register spilled to scratch, at most 128 VGPRs (four waves per SIMD stay possible), no LDS at all (the
camera records of the sweep arrive by scalar loads), no serial load chain."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel (the start of its mangled name behind the namespace) -> (VGPRs, LDS bytes)
KERNELS = {
    "mip_sweep_kernelE": (49, 0),
    "mip_fill_kernelE": (8, 0),
    "mip_activations_kernelE": (63, 0),
    "mip_activations_bwd_kernelE": (92, 0),
}


def kernel(name):
    found = [k for k in KERNELS if name.startswith(k)]
    assert len(found) == 1, name
    return found[0]


def test_mip_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "mip.hip"), isa_audit.UNITS["mip.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(KERNELS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert spills == 0, f"mip.hip:{name}: {spills} spilled VGPRs"
        assert lds <= want_lds, f"mip.hip:{name}: {lds} bytes of LDS, DESIGN.md 5.12 states {want_lds}"
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == want_vgpr, f"mip.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.12 records {want_vgpr}: update both"
        assert not chains and nflat == 0, (name, chains, nflat)
