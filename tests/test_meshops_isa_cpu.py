"""Static properties of the compiled gfx950 code of csrc/meshops.hip (the kernels behind gsr_mesh_components, gsr_mesh_compact_count / _emit,
gsr_mesh_vertex_normals and gsr_mesh_smooth): the call of tests/test_mesh_isa_cpu.py for one more translation unit, on the code objects' own resource
metadata.  No register spilled, no scratch memory, and the VGPR and LDS counts recorded in DESIGN.md 5.15 (the only LDS is the four words of a
workgroup scan)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

# kernel (the start of its mangled name behind the namespace) -> (VGPRs, LDS bytes)
KERNELS = {
    "cc_init_kernelE": (6, 0),
    "cc_hook_kernelE": (10, 0),
    "cc_compress_kernelE": (6, 0),
    "cc_face_count_kernelE": (6, 0),
    "compact_clear_kernelE": (3, 0),
    "compact_mark_kernelE": (7, 0),
    "compact_count_kernelE": (8, 16),
    "compact_emit_vertices_kernelILb0E": (12, 16),
    "compact_emit_vertices_kernelILb1E": (15, 16),
    "compact_emit_faces_kernelE": (14, 16),
    "corner_keys_kernelE": (14, 0),
    "corner_bounds_kernelE": (8, 0),
    "zero_start_kernelE": (3, 0),
    "vertex_normals_kernelE": (30, 0),
    "smooth_step_kernelE": (40, 0),
}


def kernel(name):
    found = [k for k in KERNELS if name.startswith(k)]
    assert len(found) == 1, name
    return found[0]


def test_meshops_kernels_registers_and_lds():
    import isa_audit
    src, flags = os.path.join(isa_audit.CSRC, "meshops.hip"), isa_audit.UNITS["meshops.hip"]
    res = isa_audit.resources(src, flags)
    assert sorted(kernel(n) for n in res) == sorted(KERNELS), list(res)
    for name, r in res.items():
        want_vgpr, want_lds = KERNELS[kernel(name)]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, f"meshops.hip:{name}: spills {r}"
        assert r["scratch_bytes"] == 0, f"meshops.hip:{name}: {r['scratch_bytes']} bytes of scratch per lane"
        assert r["lds_bytes"] == want_lds, f"meshops.hip:{name}: {r['lds_bytes']} bytes of LDS, DESIGN.md 5.15 records {want_lds}: update both"
        assert r["vgprs"] == want_vgpr, f"meshops.hip:{name}: {r['vgprs']} VGPRs, DESIGN.md 5.15 records {want_vgpr}: update both"
