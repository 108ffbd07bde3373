"""Static properties of the compiled gfx950 code of csrc/tsdf.hip (the kernels behind gsr_tsdf_integrate, gsr_mesh_count and gsr_mesh_emit): register
and LDS use, the call of tests/test_mip_isa_cpu.py for one more translation unit.  The counts are the measured ones of DESIGN.md 5.14; the bounds
are the design's: no register spilled to scratch, the integrate at no more than 128 VGPRs (four waves per SIMD stay possible; the camera records
arrive by scalar loads and need none), no LDS but the four words of the count's workgroup scan, no serial load chain."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel (the start of its mangled name behind the namespace) -> (VGPRs, LDS bytes)
KERNELS = {
    "tsdf_integrate_kernelILb0E": (62, 0),
    "tsdf_integrate_kernelILb1E": (84, 0),
    "mesh_classify_kernelE": (21, 0),
    "mesh_count_kernelE": (22, 16),
    "mesh_emit_kernelILb0E": (32, 0),
    "mesh_emit_kernelILb1E": (33, 0),
}


def kernel(name):
    found = [k for k in KERNELS if name.startswith(k)]
    assert len(found) == 1, name
    return found[0]


def test_tsdf_kernels_registers_and_lds():
    import isa_audit
    src, flags = os.path.join(isa_audit.CSRC, "tsdf.hip"), isa_audit.UNITS["tsdf.hip"]
    # the code objects' own metadata: a private array that the compiler kept in memory shows as scratch bytes with no spill counted (the kernels hold
    # many small per-lane arrays -- positions, sums, neighbour bytes -- that must all live in registers)
    res = isa_audit.resources(src, flags)
    assert sorted(kernel(n) for n in res) == sorted(KERNELS), list(res)
    for name, r in res.items():
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, f"tsdf.hip:{name}: spills {r}"
        assert r["scratch_bytes"] == 0, f"tsdf.hip:{name}: {r['scratch_bytes']} bytes of scratch per lane"
        assert r["lds_bytes"] == want_lds, f"tsdf.hip:{name}: {r['lds_bytes']} bytes of LDS, DESIGN.md 5.14 records {want_lds}: update both"
        assert r["vgprs"] == want_vgpr, f"tsdf.hip:{name}: {r['vgprs']} VGPRs, DESIGN.md 5.14 records {want_vgpr}: update both"
    rows = isa_audit.audit(src, flags, [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(KERNELS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert spills == 0, f"tsdf.hip:{name}: {spills} spilled VGPRs"
        assert lds <= want_lds, f"tsdf.hip:{name}: {lds} bytes of LDS, DESIGN.md 5.14 states {want_lds}"
        assert 0 < vgpr <= 128, (name, vgpr)
        assert vgpr == want_vgpr, f"tsdf.hip:{name}: {vgpr} VGPRs, DESIGN.md 5.14 records {want_vgpr}: update both"
        assert not chains and nflat == 0, (name, chains, nflat)
