"""Static properties of the compiled gfx950 code of the absolute-gradient path: csrc/absgrad.hip (the reduce and the conversion kernel) has no serial
load chain, no register spill, no flat_* access -- the call and the assertions of tests/test_contrib_isa_cpu.py for one more translation unit -- and
csrc/render_bwd.hip holds the four instantiations of the walk kernel, render_bwd_half<HAS_DEPTH, ABS> (tests/test_isa_audit_cpu.py holds every kernel of
that unit, the new instantiations included, to the same three properties)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def test_absgrad_kernels_have_no_serial_load_chains_spills_or_flat_accesses():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "absgrad.hip"), isa_audit.UNITS["absgrad.hip"], [])
    assert sorted(r[0][:14] for r in rows) == ["absgrad_from_r", "absgrad_reduce"], rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        assert not chains, f"absgrad.hip:{name}: serial load chain(s) {chains} (see tools/isa_audit.py)"
        assert spills == 0, f"absgrad.hip:{name}: {spills} spilled VGPRs"
        assert lds <= 160 * 1024 and 0 < vgpr <= 256, (name, vgpr, lds)
        assert nflat == 0, f"absgrad.hip:{name}: {nflat} flat_* instructions: an address space was lost"


def test_the_four_instantiations_of_the_walk_kernel_exist():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "render_bwd.hip"), isa_audit.UNITS["render_bwd.hip"], [])
    walks = {r[0]: r for r in rows if r[0].startswith("render_bwd_halfILb")}
    assert sorted(n[:26] for n in walks) == ["render_bwd_halfILb0ELb0EEE", "render_bwd_halfILb0ELb1EEE", "render_bwd_halfILb1ELb0EEE",
                                              "render_bwd_halfILb1ELb1EEE"], list(walks)
    for name, vgpr, lds, spills, nloads, chains, nflat in walks.values():
        assert not chains and spills == 0 and nflat == 0, (name, chains, spills, nflat)
        assert lds == 6144 and 0 < vgpr <= 128, (name, vgpr, lds)      # the ABS instantiations keep the LDS tables and stay inside 4 waves per SIMD
