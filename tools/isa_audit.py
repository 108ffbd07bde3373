#!/usr/bin/env python
"""Static audit of the gfx950 ISA of every kernel in csrc/ (no GPU needed): registers, LDS, spills, and the pattern that cost
this project the most wall-clock per line of source -- SERIAL LOAD CHAINS.

    python tools/isa_audit.py [file.hip ...]          # default: every translation unit of build.py

A "chain" is a run of  global_load -> s_waitcnt vmcnt(0)  pairs: every load is waited for before the next one is issued, so the
kernel pays one full memory round trip (~1-2 us under load on MI355X) per element instead of one per batch.  hipcc produces
it from perfectly innocent source:

    for (k...) if (in_range(k)) lds[k] = global[k];           // load inside a branch      -> load, wait, ds_write, repeat
    for (k...) v[k] = global[k];  for (k...) if (c(k)) lds[k] = v[k];   // conditional USE -> the load is sunk into the branch

The cure used throughout csrc/: unconditional loads from a clamped (always valid) address into registers, THEN unconditional
LDS writes (surplus lanes write into spare rows).  Round 2 found and removed chains of 12 (SH block of the per-Gaussian
backward: 141 -> 126 us), 15 (SSIM halo staging), 4-6 (scan kernels) and IPT (rectangle gather of the depth sort's last pass).
The output lists, per kernel: VGPRs, LDS bytes, spilled VGPRs, number of vector loads, flat_* instructions (an LDS access and a
global access merged into one generic-pointer access: emit_scatter read its LDS records with four flat_load_dword per instance
until the two sources got separate loops) and the lengths of all chains >= 3."""
from __future__ import annotations

import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian-splatting_amd", "csrc")


def _build_units():
    """The per-unit compiler flags of gaussian-splatting_amd/build.py (its UNITS table, loaded by path: the one place they are written down)."""
    spec = importlib.util.spec_from_file_location("gsr_build_units", os.path.join(ROOT, "gaussian-splatting_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {src: list(flags) for src, flags in mod.UNITS if src.endswith(".hip")}


UNITS = _build_units()


def demangle_short(name: str) -> str:
    name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)
    name = re.sub(r"^_Z\d+", "", name)
    return name[:46]


def audit(path: str, flags, extra):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
               "-S", "--cuda-device-only", "-o", out, path] + flags + extra
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        s = open(out).read()
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.vgpr_count:\s*(\d+)\s*\n\s*\.vgpr_spill_count:\s*(\d+)", s, re.S):
        meta[m.group(2)] = (int(m.group(3)), int(m.group(1)), int(m.group(4)))
    rows = []
    for m in re.finditer(r"^(_Z\w+): ; @.*?\n(.*?)^\.Lfunc_end", s, re.S | re.M):
        seq = []
        for line in m.group(2).split("\n"):
            t = line.strip().split()
            if not t:
                continue
            if t[0].startswith(("global_load", "flat_load", "buffer_load")):
                seq.append("L")
            elif t[0] == "s_waitcnt" and "vmcnt(0)" in line:
                seq.append("0")
            elif t[0] == "s_waitcnt" and "vmcnt" in line:
                seq.append("w")
        st = "".join(seq)
        chains = [len(c) // 2 for c in re.findall(r"(?:L0){3,}", st)]
        v, lds, sp = meta.get(m.group(1), (-1, -1, -1))
        # flat_* = the compiler lost the address space (e.g. it merged an LDS read and a global read into one pointer
        # select): such a load goes down both memory paths and waits on both counters
        nflat = len(re.findall(r"^\s+flat_(?:load|store|atomic)", m.group(2), re.M))
        rows.append((demangle_short(m.group(1)), v, lds, sp, st.count("L"), chains, nflat))
    return rows


def resources(path: str, flags, extra=()):
    """{kernel (demangle_short): {"vgprs", "agprs", "sgprs", "lds_bytes", "scratch_bytes", "vgpr_spill_count", "sgpr_spill_count"}} from the code-object
    metadata of one translation unit.  scratch_bytes > 0 with no spill counted is a private array the compiler kept in memory."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
               "-o", out, path] + list(flags) + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        s = open(out).read()
    rows = {}
    for entry in re.split(r"^  - (?=\.)", s[s.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s*(\S+)\s*$", entry, re.M))
        rows[demangle_short(f["name"])] = {
            "vgprs": int(f["vgpr_count"]), "agprs": int(f.get("agpr_count", 0)), "sgprs": int(f["sgpr_count"]), "lds_bytes": int(f["group_segment_fixed_size"]),
            "scratch_bytes": int(f["private_segment_fixed_size"]), "vgpr_spill_count": int(f["vgpr_spill_count"]), "sgpr_spill_count": int(f["sgpr_spill_count"])}
    return rows


def instruction_counts(path: str, flags, mnemonic: str, extra=()):
    """{kernel (demangle_short): how often `mnemonic` (e.g. v_mfma_f32_32x32x2_f32) occurs in its gfx950 code} for every kernel of one translation unit."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
               "-o", out, path] + list(flags) + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        s = open(out).read()
    return {demangle_short(m.group(1)): len(re.findall(r"^\s+" + re.escape(mnemonic) + r"\s", m.group(2), re.M))
            for m in re.finditer(r"^(_Z\w+): ; @.*?\n(.*?)^\.Lfunc_end", s, re.S | re.M)}


def forward_walk_step(extra=()):
    """Instruction mix of ONE step of the forward blend's survivor walk in the inference build (render_fwd_wave_bf<true, 1, false>): the first unrolled
    copy of the inner loop's body, from the loop header to its closing branch -> {"valu": n, "salu": n, "ds": n}.  The kernel is bound by issue slots
    (DESIGN 4), so this count IS its cost model; tests/test_isa_audit_cpu.py pins it for the shipped form and for the candidate forms."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
               "-o", out, os.path.join(CSRC, "render_fwd.hip")] + UNITS["render_fwd.hip"] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        s = open(out).read()
    m = re.search(r"^_ZN12_GLOBAL__N_118render_fwd_wave_bfILb1ELi1ELb0EEE\w+: ; @.*?\n(.*?)^\.Lfunc_end", s, re.S | re.M)
    if not m:
        raise RuntimeError("render_fwd_wave_bf<true, 1, false> not found")
    body = m.group(1)
    body = body[body.index("This Inner Loop Header"):]
    mix = {"valu": 0, "salu": 0, "ds": 0}
    seen_fma = 0
    for line in body.split("\n")[1:]:
        t = line.strip().split()
        if not t or t[0].startswith((";", ".")):
            continue
        op = t[0]
        if op.startswith("v_"):
            mix["valu"] += 1
            seen_fma += op.startswith("v_fmac_f32")
        elif op.startswith("ds_"):
            mix["ds"] += 1
        elif op.startswith("s_") and op not in ("s_waitcnt", "s_nop"):
            mix["salu"] += 1
            if op.startswith("s_cbranch") and seen_fma >= 6:      # the branch that closes the step (two FMAs of the exponent, four of the accumulators)
                break
    return mix


def preprocess_forward(source=None, extra=()):
    """Every instantiation of the forward per-Gaussian kernel (csrc/preprocess.hip preprocess_fwd_kernel<SPLIT, FORM>), one dict each:
    from the code-object metadata the VGPRs, the spilled SGPRs (parked in VGPR lanes) and VGPRs (in scratch), scratch and LDS bytes; the
    waves per SIMD the compiler states for that register count and the workgroups per CU the LDS admits; and static counts over the whole
    kernel: VALU, SALU, v_mov_b32, lane moves (v_readlane / v_writelane: the traffic of the parked SGPRs), global loads and stores.
    `source`: another copy of preprocess.hip (the parent's, for the committed before / after pair in profiles/); same flags, same headers.
        python tools/isa_audit.py preprocess_forward [path/to/preprocess.hip]      # prints JSON"""
    src = source or os.path.join(CSRC, "preprocess.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
               "-o", out, src] + UNITS["preprocess.hip"] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        s = open(out).read()
    meta = {}
    for entry in re.split(r"^  - (?=\.)", s[s.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s*(\S+)\s*$", entry, re.M))
        meta[f["name"]] = f
    rows = []
    for m in re.finditer(r"^(_Z\w*preprocess_fwd_kernel\w+): ; @.*?\n(.*?)^\.Lfunc_end\d+:(.*?^; Occupancy:\s*\d+)", s, re.S | re.M):
        name, body, trailer = m.group(1), m.group(2), m.group(3)
        f = meta[name]
        ops = [t[0] for t in (line.strip().split() for line in body.split("\n")) if t and not t[0].startswith((";", ".")) and not t[0].endswith(":")]
        form = re.search(r"GsrPreFormIL(\w+?)EEE", name)
        form = "generic" if form is None or "n1" in form.group(1) and form.group(1).count("n1") == 4 else "hot" if form.group(1) == "i0ELi0ELi1ELi0" else form.group(1)
        occ = re.search(r"; Occupancy:\s*(\d+)", trailer)
        lds = int(f["group_segment_fixed_size"])
        rows.append({
            "kernel": name, "split_sh": "ILb1E" in name, "form": form,
            "vgprs": int(f["vgpr_count"]), "agprs": int(f.get("agpr_count", 0)), "sgprs": int(f["sgpr_count"]),
            "sgpr_spill_count": int(f["sgpr_spill_count"]), "vgpr_spill_count": int(f["vgpr_spill_count"]),
            "scratch_bytes": int(f["private_segment_fixed_size"]), "lds_bytes": lds,
            "waves_per_simd": int(occ.group(1)) if occ else None, "workgroups_per_cu_by_lds": (160 * 1024) // lds if lds else None,
            "valu": sum(o.startswith("v_") for o in ops), "salu": sum(o.startswith("s_") and o not in ("s_waitcnt", "s_nop") for o in ops),
            "v_mov_b32": ops.count("v_mov_b32_e32") + ops.count("v_mov_b32_e64") + ops.count("v_mov_b32"),
            "lane_moves": sum(o.startswith(("v_readlane", "v_writelane")) for o in ops),
            "global_loads": sum(o.startswith("global_load") for o in ops), "global_stores": sum(o.startswith("global_store") for o in ops),
        })
    if not rows:
        raise RuntimeError("no preprocess_fwd_kernel instantiation found")
    return sorted(rows, key=lambda r: (r["form"] != "hot", r["split_sh"]))


RANKING_KERNELS = {"tilesort.hip": ("emit_scatter", "bucket_scatter"), "depthsort.hip": ("ds_scatter", "ds_segsort")}


def _template_args(mangled: str, kernel: str) -> str:
    """'<uint32_t, 6, true>' from the Itanium mangling of an instantiation of `kernel` (j = uint32_t, m = uint64_t, Lb / Li literals)."""
    m = re.search(kernel + r"I((?:[jm]|L[bi]\d+E)+)E", mangled)
    if not m:
        return ""
    out = []
    for a in re.findall(r"[jm]|L[bi]\d+E", m.group(1)):
        out.append({"j": "uint32_t", "m": "uint64_t"}.get(a) or (("true" if a[2:-1] == "1" else "false") if a[1] == "b" else a[2:-1]))
    return "<" + ", ".join(out) + ">"


def ranking(source_dir=None, extra=()):
    """Every instantiation of the four stable-ranking kernels of the binning chain (csrc/tilesort.hip emit_scatter / bucket_scatter, csrc/depthsort.hip
    ds_scatter / ds_segsort), one dict each: static counts over the whole kernel of VALU, SALU, v_mov_b32, v_mul_lo_u32, v_bitop3_b32 (two per
    matched bit and item: an unrolled match chain of BITS bits over ITEMS items shows as 2 x BITS x ITEMS, a rolled one as 2), v_bcnt / v_mbcnt;
    from the code-object metadata VGPRs, spills, scratch and LDS bytes, and the waves per SIMD the compiler states.
    `source_dir`: another copy of csrc/ (the parent's, for the committed before / after pair in profiles/).
        python tools/isa_audit.py ranking [dir]      # prints JSON"""
    rows = []
    for unit, kernels in RANKING_KERNELS.items():
        src = os.path.join(source_dir or CSRC, unit)
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k.s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + (source_dir or CSRC), "-S",
                   "--cuda-device-only", "-o", out, src] + UNITS[unit] + list(extra)
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            s = open(out).read()
        meta = {}
        for entry in re.split(r"^  - (?=\.)", s[s.index("amdhsa.kernels:"):], flags=re.M)[1:]:
            f = dict(re.findall(r"^\s*\.(\w+):\s*(\S+)\s*$", entry, re.M))
            meta[f["name"]] = f
        for m in re.finditer(r"^(_Z\w+): ; @.*?\n(.*?)^\.Lfunc_end\d+:(.*?^; Occupancy:\s*\d+)", s, re.S | re.M):
            name, body, trailer = m.group(1), m.group(2), m.group(3)
            kernel = next((k for k in kernels if re.search(r"\d" + k + r"[IE]", name)), None)
            if kernel is None or name not in meta:
                continue
            f = meta[name]
            ops = [t[0] for t in (line.strip().split() for line in body.split("\n")) if t and not t[0].startswith((";", ".")) and not t[0].endswith(":")]
            occ = re.search(r"; Occupancy:\s*(\d+)", trailer)
            # the truth tables of the kernel's v_bitop3_b32: 0x90 = a & ~(b ^ c) is match_digit's; the compiler forms others from plain and / or / xor
            tables = [x.lower() for x in re.findall(r"^\s+v_bitop3_b32\s.*?bitop3:(0x[0-9a-fA-F]+)", body, re.M)]
            inst, pad_last = kernel + _template_args(name, kernel), None
            if unit == "tilesort.hip" and inst.count(",") == 3:
                # the fourth argument is PAD (option ranking_pad_last): the default form keeps the three-argument name it had before the option existed
                # (the parent's rows and the tests name it so), the per-item-validity form is marked
                inst, pad = inst[:-1].rsplit(", ", 1)
                pad_last = int(pad == "true")
                inst += ">" if pad_last else "> pad_last=0"
            rows.append({
                "unit": unit, "kernel": kernel, "instantiation": inst, "symbol": name, "pad_last": pad_last,
                "valu": sum(o.startswith("v_") for o in ops), "salu": sum(o.startswith("s_") and o not in ("s_waitcnt", "s_nop") for o in ops),
                "v_mov_b32": sum(o.startswith("v_mov_b32") for o in ops), "v_mul_lo_u32": sum(o.startswith("v_mul_lo_u32") for o in ops),
                "v_mul_u32_u24": sum(o.startswith(("v_mul_u32_u24", "v_mad_u32_u24")) for o in ops),
                "v_bitop3_b32": sum(o.startswith("v_bitop3_b32") for o in ops), "v_bitop3_b32_match": tables.count("0x90"),
                "v_bfe_i32": sum(o.startswith("v_bfe_i32") for o in ops),
                "v_bcnt_u32_b32": sum(o.startswith("v_bcnt_u32_b32") for o in ops), "v_mbcnt": sum(o.startswith("v_mbcnt") for o in ops),
                "s_nop": ops.count("s_nop"), "branches": sum(o.startswith(("s_cbranch", "s_branch")) for o in ops),
                "vgprs": int(f["vgpr_count"]), "agprs": int(f.get("agpr_count", 0)), "sgprs": int(f["sgpr_count"]),
                "vgpr_spill_count": int(f["vgpr_spill_count"]), "sgpr_spill_count": int(f["sgpr_spill_count"]),
                "scratch_bytes": int(f["private_segment_fixed_size"]), "lds_bytes": int(f["group_segment_fixed_size"]),
                "waves_per_simd": int(occ.group(1)) if occ else None,
            })
    if not rows:
        raise RuntimeError("no ranking kernel found")
    return sorted(rows, key=lambda r: (r["unit"] != "tilesort.hip", r["kernel"], r["instantiation"]))


def main():
    if sys.argv[1:2] == ["ranking"]:
        import json
        dirs = [a for a in sys.argv[2:] if not a.startswith("-")]
        print(json.dumps({"units": {u: UNITS[u] for u in RANKING_KERNELS}, "items_per_thread": {"emit_scatter": 16, "bucket_scatter": 16, "ds_scatter": 8, "ds_segsort": 1},
                          "instantiations": ranking(dirs[0] if dirs else None, [a for a in sys.argv[2:] if a.startswith("-")])}, indent=1))
        return
    if sys.argv[1:2] == ["preprocess_forward"]:
        import json
        srcs = [a for a in sys.argv[2:] if not a.startswith("-")]
        print(json.dumps({"unit": "preprocess.hip", "flags": UNITS["preprocess.hip"], "instantiations": preprocess_forward(srcs[0] if srcs else None, [a for a in sys.argv[2:] if a.startswith("-")])}, indent=1))
        return
    files = [a for a in sys.argv[1:] if a.endswith(".hip")]
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    if not files:
        files = list(UNITS)
    bad = 0
    for f in files:
        base = os.path.basename(f)
        print(f"== {base}")
        for name, v, lds, sp, nl, chains, nflat in audit(os.path.join(CSRC, base), UNITS.get(base, []), extra):
            flag = "   <-- serial load chain" if chains else ""
            spill = f" SPILLS {sp}" if sp > 0 else ""
            flat = f"  FLAT {nflat}" if nflat else ""
            print(f"  {name:46s} vgpr {v:3d}  lds {lds:6d}{spill}  loads {nl:3d}{flat}  chains {chains}{flag}")
            bad += len(chains)
    print(f"{bad} serial load chain(s) of length >= 3")


if __name__ == "__main__":
    main()
