#!/bin/bash
# round-end measurement bundle: rocprofv3 kernel trace + PMC passes (FETCH_SIZE / WRITE_SIZE / SQ, each in its own run), summarised ON the
# GPU machine (the raw counter files are too large to copy back), then the full bench line (bench.py --full) -- taken last, so that its
# roofline.traffic / valu_* fields come from THIS run's counter passes (profiles/pmc_latest.json is replaced before bench.py reads it)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT="${OUT:-out}"      # where the logs go (the scripts this one calls write there too)
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
R="$PWD"
TAG="${ROUND_TAG:-r04}"
B="--full --no-cpu-baseline --no-other-configs --no-in-flight --no-pmc --densify-iters 0 --min-warm-seconds 0.2"
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -o r1 -- python "$R/bench.py" --steps 30 --warmup 5 --train-steps 15 $B > "$OUT/p_prof_stats.log" 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/prof_fetch" -o r1 -- python "$R/bench.py" --steps 10 --warmup 2 --train-steps 5 $B > "$OUT/p_prof_fetch.log" 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/prof_write" -o r1 -- python "$R/bench.py" --steps 10 --warmup 2 --train-steps 5 $B > "$OUT/p_prof_write.log" 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_ANY --output-format csv -d "$OUT/prof_sq" -o r1 -- python "$R/bench.py" --steps 6 --warmup 2 --train-steps 4 $B > "$OUT/p_prof_sq.log" 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_SALU --output-format csv -d "$OUT/prof_sq2" -o r1 -- python "$R/bench.py" --steps 6 --warmup 2 --train-steps 4 $B > "$OUT/p_prof_sq2.log" 2>&1
cd "$R"
# steady-state per-kernel statistics (median / p10 / p90, warm-up dispatches dropped) from the per-dispatch trace, before it is deleted
python tools/kernel_trace_stats.py $OUT/prof_stats $OUT/kernel_stats_steady.csv 0.25
python tools/collect_profiles.py "$TAG" "$OUT/profiles_$TAG"
rm -rf $OUT/prof_stats $OUT/prof_fetch $OUT/prof_write $OUT/prof_sq $OUT/prof_sq2
cp "$OUT/profiles_$TAG/pmc_latest.json" profiles/pmc_latest.json
( time timeout 1200 python bench.py --full ) > $OUT/p_bench_default.log 2>&1
python - "$TAG" <<'PY'
import json, os, sys
tag = sys.argv[1]
line = [ln for ln in open(os.path.join(os.environ["OUT"], "p_bench_default.log")) if ln.startswith("{")][-1]
d = json.loads(line)
open(os.path.join(os.environ["OUT"], f"profiles_{tag}", f"{tag}_bench_default.json"), "w").write(line)
print("bench:", d["value"], "Mpix/s", d["ms_per_step"], "ms; train", d.get("train_iters_per_s"), "it/s; full loop", d.get("train_iters_per_s_full_loop_configs2"))
PY
tail -4 $OUT/p_bench_default.log | cut -c1-300
