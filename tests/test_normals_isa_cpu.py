"""Static properties of the compiled gfx950 code of csrc/normals.hip (the kernels behind gsr_gaussian_normals, gsr_depth_normals, gsr_normal_loss
and their backwards): register and LDS use, the call of tests/test_bilagrid_isa_cpu.py for one more translation unit.  The counts are the
measured ones of DESIGN.md 5.11; the bounds are the design's: no register spilled to scratch, at most 128 VGPRs (four waves per SIMD stay
possible), LDS no larger than stated there."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel (the start of its mangled name behind the namespace) -> (VGPRs, LDS bytes)
KERNELS = {
    "gaussian_normals_kernelE": (23, 0),
    "gaussian_normals_bwd_kernelE": (27, 0),
    "depth_normals_kernelE": (19, 4752),             # 66 x 18 depths
    "normal_loss_kernelE": (24, 6800),               # the same tile and 256 fp64 partial sums
    "normal_loss_sum_kernelE": (11, 2048),
    "normal_loss_bwd_normals_kernelE": (20, 4752),
    "depth_normals_bwd_kernelILb0E": (28, 24448),    # 68 x 20 depths and 66 x 18 float4 hand-overs
    "depth_normals_bwd_kernelILb1E": (29, 24448),
}


def kernel(name):
    found = [k for k in KERNELS if name.startswith(k)]
    assert len(found) == 1, name
    return found[0]


def test_normals_kernels_registers_and_lds():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "normals.hip"), isa_audit.UNITS["normals.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(KERNELS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert spills == 0, f"normals.hip:{name}: {spills} spilled VGPRs"
        assert lds <= want_lds, f"normals.hip:{name}: {lds} bytes of LDS, DESIGN.md 5.11 states {want_lds}"
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == want_vgpr, f"normals.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.11 records {want_vgpr}: update both"
