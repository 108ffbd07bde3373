"""Static properties of the compiled gfx950 code of csrc/features.hip (the N-channel feature render and its gradient): no serial load chain, no register
spill, no flat_* access -- the call and the assertions of tests/test_probe_isa_cpu.py for one more translation unit."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

G = 16      # channels per forward walk (csrc/features.hip FEAT_G; tests/test_features_cpu.py sweeps the group edges of this value)
# LDS tables the design names: the compacted survivors (two 16-byte records each, 2 KB) plus, in the forward, their feature rows (4 G bytes each); in the
# gradient walk of 4 NB channels the per-entry sums (NB 16-byte records each); in its reduce NB 16-byte records per instance of a chunk
LDS = {"feature_walk<true>": 2048 + 64 * 4 * G, "feature_walk<false>": 2048 + 64 * 4 * G}
LDS.update({f"feature_grad_walk<{nb}>": 2048 + 1024 * nb for nb in (1, 2, 4)})
LDS.update({f"feature_grad_reduce<{nb}>": 1024 * nb for nb in (1, 2, 4)})


def kernel(name):
    m = re.match(r"(feature_grad_walk|feature_grad_reduce|feature_walk)IL([bi])(\d)E", name)
    assert m, name
    return f"{m.group(1)}<{m.group(3) if m.group(2) == 'i' else 'true' if m.group(3) == '1' else 'false'}>"


def test_feature_kernels_have_no_serial_load_chains_spills_or_flat_accesses():
    import isa_audit
    rows = isa_audit.audit(os.path.join(isa_audit.CSRC, "features.hip"), isa_audit.UNITS["features.hip"], [])
    assert sorted(kernel(r[0]) for r in rows) == sorted(LDS), rows
    for name, vgpr, lds, spills, nloads, chains, nflat in rows:
        assert not chains, f"features.hip:{name}: serial load chain(s) {chains} (see tools/isa_audit.py)"
        assert spills == 0, f"features.hip:{name}: {spills} spilled VGPRs"
        assert lds == LDS[kernel(name)] and 0 < vgpr <= 256, (name, vgpr, lds)
        assert nflat == 0, f"features.hip:{name}: {nflat} flat_* instructions: an address space was lost"
