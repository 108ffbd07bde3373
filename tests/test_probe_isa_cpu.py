"""Static properties of the compiled gfx950 code of csrc/probe.hip (the per-pixel probe kernel): no serial load chain, no register spill, no flat_*
access -- the call and the assertions of tests/test_contrib_isa_cpu.py for one more translation unit."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def test_probe_kernel_has_no_serial_load_chains_spills_or_flat_accesses():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "probe.hip"), isa_audit.UNITS["probe.hip"], [])
    assert sorted(r[0][:12] for r in rows) == ["probe_walkE9"], rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        assert not chains, f"probe.hip:{name}: serial load chain(s) {chains} (see tools/isa_audit.py)"
        assert spills == 0, f"probe.hip:{name}: {spills} spilled VGPRs"
        assert lds <= 4 * 1024 and 0 < vgpr <= 256, (name, vgpr, lds)      # (a few KB of LDS: two 16-byte and one 8-byte record per survivor)
        assert nflat == 0, f"probe.hip:{name}: {nflat} flat_* instructions: an address space was lost"
