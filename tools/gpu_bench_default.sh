#!/bin/bash
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
export OUT="${OUT:-out}"      # where the logs go (the scripts this one calls write there too)
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"
export TMPDIR=/tmp
( time timeout 1200 python bench.py --full ) > $OUT/bench_default.log 2>&1
tail -c 3000 $OUT/bench_default.log | tail -5 | cut -c1-1500
