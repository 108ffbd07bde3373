"""Static properties of the compiled gfx950 code of csrc/vq.hip (the kernels behind gsr_vq_assign and gsr_vq_update): register, LDS and scratch
use, the call of tests/test_mip_isa_cpu.py for one more translation unit.  The counts are the measured ones of the table in DESIGN.md 5.13, row by
row; the bounds are the design's: no register spilled and NO SCRATCH AT ALL (a private array the compiler keeps in memory counts no spill: the
prefetched stage of the assignment once made a round trip through scratch in every trip of the sweep), the assignment within 256 VGPRs (two waves
per SIMD: a second workgroup shares the CU), no serial load chain, and the assignment's inner product on the fp32 matrix instruction -- two row
tiles x two centroid tiles x the pair count per stage."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel as DESIGN.md 5.13 names it -> (the start of its mangled name behind the namespace, VGPRs, LDS bytes)
KERNELS = {
    "vq_norms_kernel": ("vq_norms_kernelE", 8, 0),
    "vq_assign_kernel<4>": ("vq_assign_kernelILi4EE", 158, 5632),
    "vq_assign_kernel<8>": ("vq_assign_kernelILi8EE", 166, 9728),
    "vq_assign_kernel<16>": ("vq_assign_kernelILi16EE", 187, 17920),
    "vq_assign_kernel<24>": ("vq_assign_kernelILi24EE", 209, 26112),
    "vq_assign_kernel<32>": ("vq_assign_kernelILi32EE", 231, 34304),
    "vq_keys_kernel": ("vq_keys_kernelE", 26, 0),
    "vq_bounds_kernel": ("vq_bounds_kernelE", 8, 0),
    "vq_scan_kernel": ("vq_scan_kernelE", 26, 1024),
    "vq_chunk_kernel": ("vq_chunk_kernelE", 44, 0),
    "vq_finish_kernel": ("vq_finish_kernelE", 14, 0),
}
MFMA = "v_mfma_f32_32x32x2_f32"


def kernel(name):
    found = [k for k, v in KERNELS.items() if name.startswith(v[0])]
    assert len(found) == 1, name
    return found[0]


def test_vq_kernels_registers_lds_and_scratch():
    import isa_audit
    src, flags = os.path.join(isa_audit.CSRC, "vq.hip"), isa_audit.UNITS["vq.hip"]
    res = isa_audit.resources(src, flags)
    assert sorted(kernel(n) for n in res) == sorted(KERNELS), list(res)
    for name, r in res.items():
        _, want_vgpr, want_lds = KERNELS[kernel(name)]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, f"vq.hip:{name}: spills {r}"
        assert r["scratch_bytes"] == 0, f"vq.hip:{name}: {r['scratch_bytes']} bytes of scratch per lane"
        assert r["lds_bytes"] == want_lds, f"vq.hip:{name}: {r['lds_bytes']} bytes of LDS, DESIGN.md 5.13 records {want_lds}: update both"
        assert 0 < r["vgprs"] <= 256, (name, r["vgprs"])
        assert r["vgprs"] == want_vgpr, f"vq.hip:{name}: {r['vgprs']} VGPRs, DESIGN.md 5.13 records {want_vgpr}: update both"
    for name, vgpr, lds, spills, nloads, chains, nflat in isa_audit.audit(src, flags, []):
        assert not chains and nflat == 0, (name, chains, nflat)


def test_the_assignment_runs_on_the_fp32_matrix_instruction():
    import isa_audit
    counts = isa_audit.instruction_counts(os.path.join(isa_audit.CSRC, "vq.hip"), isa_audit.UNITS["vq.hip"], MFMA)
    for name, n in counts.items():
        k = kernel(name)
        if k.startswith("vq_assign_kernel"):
            pairs = int(k[len("vq_assign_kernel<"):-1])
            assert n == 2 * 2 * pairs, f"vq.hip:{name}: {n} x {MFMA}, the stage loop holds 2 row tiles x 2 centroid tiles x {pairs} pairs"
        else:
            assert n == 0, (name, n)


def test_the_recorded_counts_are_those_of_the_design_document():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("## 5.13"):]
    section = section[:section.index("\n## ", 10)]
    table = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^\s*\| `(vq_\w+(?:<\d+>)?)` \| (\d+) \| (\d+) \|", section, re.M)}
    assert table == {k: (v[1], v[2]) for k, v in KERNELS.items()}, table
