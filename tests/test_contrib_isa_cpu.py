"""Static properties of the compiled gfx950 code of csrc/contrib.hip (the contribution-statistics kernels): no serial load chain, no register
spill, no flat_* access -- the call and the assertions of tests/test_isa_audit_cpu.py for one more translation unit."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def test_contrib_kernels_have_no_serial_load_chains_spills_or_flat_accesses():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "contrib.hip"), isa_audit.UNITS["contrib.hip"], [])
    assert sorted(r[0][:14] for r in rows) == ["contrib_reduce", "contrib_walkE9"], rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        assert not chains, f"contrib.hip:{name}: serial load chain(s) {chains} (see tools/isa_audit.py)"
        assert spills == 0, f"contrib.hip:{name}: {spills} spilled VGPRs"
        assert lds <= 160 * 1024 and 0 < vgpr <= 256, (name, vgpr, lds)
        assert nflat == 0, f"contrib.hip:{name}: {nflat} flat_* instructions: an address space was lost"
