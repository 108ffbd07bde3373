#!/bin/bash
# A/B of library options on ONE box (box-to-box variance is larger than most single-kernel gains):
#   gpurun -- 'bash tools/gpu_ab.sh "depth_sort_mode=1" "depth_sort_mode=2"'            (options of the measurement build)
#   GSR_LIB=gaussian-splatting_amd/lib_ab/libgsr_hip.so is set automatically when a lib_ab build exists.
# Each configuration runs bench.py twice, interleaved; one line per run: Mpix/s, ms/frame, train it/s, stage table.
#   LIBS="lib lib_prev" bash tools/gpu_ab.sh          compares LIBRARIES instead (tools/build_prev_lib.sh builds lib_prev from
#                                                       an earlier revision); REPS (3) interleaved runs each, arguments BENCH_ARGS
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
OUT="${OUT:-out}"      # where the logs go
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
if [ -n "$LIBS" ]; then
  # REPS alternations (default 3).  BENCH_ARGS: the arguments of every run; default = the context legs with the train step.  BENCH_ARGS=" " runs
  # plain `python bench.py` (the headline frame only: seconds per run, so more alternations fit a GPU call).  A run that fails ends the script:
  # nothing more is started on a GPU that has just faulted or hung.
  BENCH_ARGS="${BENCH_ARGS:---full --no-other-configs --no-cpu-baseline --no-in-flight --no-pmc --densify-iters 0}"
  for rep in $(seq 1 "${REPS:-3}"); do
    for lib in $LIBS; do
      GSR_LIB="$PWD/gaussian-splatting_amd/$lib/libgsr_hip.so" timeout -k 10 300 python bench.py $BENCH_ARGS > $OUT/ab_${lib}_$rep.log 2>&1 || { echo "$lib rep $rep: bench.py failed ($?)"; tail -5 $OUT/ab_${lib}_$rep.log; exit 1; }
      python - "$lib" "$rep" "$OUT/ab_${lib}_$rep.log" <<'PY' || exit 1
import json, sys
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
print(f"{sys.argv[1]} rep {sys.argv[2]}:", d["value"], d["ms_per_step"], d.get("train_iters_per_s"), d.get("stage_ms"))
PY
    done
  done
  exit 0
fi
[ -f gaussian-splatting_amd/lib_ab/libgsr_hip.so ] && export GSR_LIB="$PWD/gaussian-splatting_amd/lib_ab/libgsr_hip.so"
for rep in 1 2; do
  i=0
  for cfg in "$@"; do
    i=$((i+1))
    opts=""; for o in ${cfg//,/ }; do opts="$opts --opt $o"; done
    timeout 300 python bench.py --full --no-other-configs --no-cpu-baseline --no-in-flight --no-pmc --densify-iters 0 $opts > $OUT/ab_${i}_$rep.log 2>&1
    python - "$cfg" "$rep" "$OUT/ab_${i}_$rep.log" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
print(f"{sys.argv[1]} rep {sys.argv[2]}:", d["value"], d["ms_per_step"], d["train_iters_per_s"], d["stage_ms"])
PY
  done
done
