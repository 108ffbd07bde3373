"""Static properties of the ranking kernels' gfx950 code (tools/isa_audit.py ranking; hipcc cross-compiles here, no GPU) for the instantiations
compiled for a digit width -- emit_scatter<uint32_t, HB, true> for 5..7 bits (8 bits stay generic: that instantiation parks two SGPRs in VGPR
lanes), bucket_scatter<uint32_t, ., LB> for 5..8 bits (ds_scatter keeps its earlier form: the specialised one measured no faster; ds_segsort chooses
its sweep inside the kernel and is covered by the register and scratch bounds):

* no rolled match loop: the match chain's v_bitop3_b32 (truth table 0x90 = mask & ~(ballot ^ bit), two per bit and item) number exactly
  2 x bits x items, and one v_bfe_i32 + the chain is all a bit costs.  In emit_scatter that is every v_bitop3_b32 of the kernel.
  bucket_scatter holds seven more with OTHER truth tables, as it did before (the compiler's own fusions of and / or / xor in the fused scan,
  38 - 32 = 6 in the run-time-width kernel too), so there the count is taken over the chain's table and the others are bounded;
* emit_scatter<uint32_t, ., true> multiplies with v_mul_u32_u24 only: no v_mul_lo_u32;
* no scratch, no spills, at most 128 VGPRs (four waves per SIMD);
* the v_mbcnt pair replaces half of the v_bcnt.
The committed report profiles/isa_ranking.json must state the same numbers as the sources do now."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")

WIDTHS = (5, 6, 7, 8)


@pytest.fixture(scope="module")
def report():
    import isa_audit
    return {r["instantiation"]: r for r in isa_audit.ranking()}


def specialised(report):
    """(row, bits, items per thread) of every width instantiation"""
    out = [(report[f"emit_scatter<uint32_t, {b}, true>"], b, 16) for b in WIDTHS[:-1]]
    out += [(report[f"bucket_scatter<uint32_t, {f}, {b}>"], b, 16) for b in WIDTHS for f in ("true", "false")]
    return out


def test_every_width_has_its_instantiation_and_the_generic_kernels_stay(report):
    assert len(specialised(report)) == 11 and "emit_scatter<uint32_t, 8, true>" not in report
    for name in ("emit_scatter<uint32_t, 0, true>", "emit_scatter<uint32_t, 0, false>", "emit_scatter<uint64_t, 0, false>", "bucket_scatter<uint32_t, true, 0>",
                 "bucket_scatter<uint32_t, false, 0>", "bucket_scatter<uint64_t, true, 0>", "bucket_scatter<uint64_t, false, 0>", "ds_scatter", "ds_segsort"):
        assert name in report, name
    # the run-time-width kernels keep the rolled loop: two v_bitop3_b32 per item
    assert report["emit_scatter<uint32_t, 0, true>"]["v_bitop3_b32_match"] == 2 * 16
    # ds_segsort: the rolled loop of the run-time width (twice: LDS segments and the oversized path) and the two unrolled sweeps of 9 and 8 bits, each
    # at the kernel's two inlined copies of the LDS sort
    assert report["ds_segsort"]["v_bitop3_b32_match"] == 2 * 3 + 2 * 2 * (9 + 8)


def test_no_rolled_match_loop(report):
    for r, bits, items in specialised(report):
        assert r["v_bitop3_b32_match"] == 2 * bits * items, (r["instantiation"], r["v_bitop3_b32_match"])
        if r["kernel"] != "bucket_scatter":
            assert r["v_bitop3_b32"] == 2 * bits * items, (r["instantiation"], r["v_bitop3_b32"])
        else:
            assert r["v_bitop3_b32"] - r["v_bitop3_b32_match"] <= 7, (r["instantiation"], r["v_bitop3_b32"])
        # one bit extraction per bit and item (emit_scatter: plus the 16 of its valid flags, as in the run-time-width kernel)
        assert bits * items <= r["v_bfe_i32"] <= bits * items + 16, (r["instantiation"], r["v_bfe_i32"])


def test_emission_multiplies_are_24_bit(report):
    for b in WIDTHS[:-1] + (0,):
        r = report[f"emit_scatter<uint32_t, {b}, true>"]
        assert r["v_mul_lo_u32"] == 0 and r["v_mul_u32_u24"] == 34, (r["instantiation"], r["v_mul_lo_u32"], r["v_mul_u32_u24"])
    # the 64-bit-word kernel and the kernel for callers outside the fused path's tile bound keep the full multiplies
    assert report["emit_scatter<uint64_t, 0, false>"]["v_mul_lo_u32"] == 34 and report["emit_scatter<uint32_t, 0, false>"]["v_mul_lo_u32"] == 34


def test_four_waves_per_simd_and_no_scratch(report):
    for r in report.values():
        assert r["scratch_bytes"] == 0 and r["vgpr_spill_count"] == 0, r["instantiation"]
        # SGPRs parked in VGPR lanes: none, except in ds_segsort (2 before this report existed, 24 now), whose v_readlane / v_writelane all sit on the
        # path of segments beyond the LDS capacity and in the prologue -- none inside a radix pass
        assert r["sgpr_spill_count"] == 0 or r["kernel"] == "ds_segsort", r["instantiation"]
        if r["kernel"] == "emit_scatter" and "uint64_t" in r["instantiation"]:
            continue      # (42 KB of LDS: three workgroups per CU, as before)
        assert r["vgprs"] <= 128 and r["waves_per_simd"] >= 4, (r["instantiation"], r["vgprs"], r["waves_per_simd"])


def test_ranks_by_mbcnt(report):
    for r, _, items in specialised(report):
        assert r["v_mbcnt"] == 2 * items and r["v_bcnt_u32_b32"] == 2 * items, (r["instantiation"], r["v_mbcnt"], r["v_bcnt_u32_b32"])


def test_committed_report_is_current(report):
    with open(os.path.join(ROOT, "profiles", "isa_ranking.json")) as f:
        committed = {r["instantiation"]: r for r in json.load(f)["instantiations"]}
    assert sorted(committed) == sorted(report)
    for name, r in report.items():
        for k in ("valu", "salu", "v_mov_b32", "v_mul_lo_u32", "v_bitop3_b32", "vgprs", "scratch_bytes", "lds_bytes"):
            assert committed[name][k] == r[k], (name, k, committed[name][k], r[k])
    with open(os.path.join(ROOT, "profiles", "isa_ranking_parent.json")) as f:
        parent = {r["instantiation"]: r for r in json.load(f)["instantiations"]}
    assert parent["emit_scatter<uint32_t>"]["v_mul_lo_u32"] == 34 and parent["emit_scatter<uint32_t>"]["v_bitop3_b32"] == 32
