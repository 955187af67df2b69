#!/bin/bash
# Main-leg kernel-trace summary per value of an environment variable: bash scripts/gpu_trace_env.sh TAG VAR v1 v2 ...
R=${GRAFT_REPO_ROOT:-$(pwd)}
# every output goes under $NEUS_OUT_DIR (an absolute path; default: bench_out/ in the repository)
OUT=${NEUS_OUT_DIR:-$R/bench_out}
cd "$R" && mkdir -p "$OUT"
TAG=$1; VAR=$2; shift 2
for V in "$@"; do
  (cd /tmp && export TMPDIR=/tmp && export "$VAR=$V" && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_${TAG}_$V" -o run -- python3 "$R/bench.py" --full \
     --steps 20 --warmup 5 --cpu-baseline 0 --psnr-steps 0 --mc-res 0 --l16 0 --early 0 ${BENCH_ARGS:-} > "$OUT/prof_${TAG}_$V.log" 2>&1) || { echo "PROF_FAIL $V"; exit 1; }
  python3 scripts/prof_summary.py $OUT/prof_${TAG}_$V $OUT/prof_${TAG}_${V}_summary.md --last-steps 20 > /dev/null && rm -rf $OUT/prof_${TAG}_$V
  echo "== $VAR=$V"; head -24 $OUT/prof_${TAG}_${V}_summary.md
done
echo TRACE_OK
