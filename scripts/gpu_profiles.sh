#!/bin/bash
# rocprofv3 kernel-trace summaries of the driver-shaped bench and of a steady-state run (main config only: --l16 0).
# Usage: bash scripts/gpu_profiles.sh TAG
R=${GRAFT_REPO_ROOT:-$(pwd)}
# every output goes under $NEUS_OUT_DIR (an absolute path; default: bench_out/ in the repository)
OUT=${NEUS_OUT_DIR:-$R/bench_out}
mkdir -p "$OUT"
TAG=$1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --cpu-baseline 0 --psnr-steps 0 --mc-res 0 --l16 0 > "$OUT/prof_$TAG.log" 2>&1 || { echo PROF_FAIL; exit 1; }
python3 "$R/scripts/prof_summary.py" "$OUT/prof_$TAG" "$OUT/prof_${TAG}_drv_summary.md" --last-steps 20 > /dev/null && rm -rf "$OUT/prof_$TAG"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run -- python3 "$R/bench.py" --full --steps 50 --warmup 800 --cpu-baseline 0 --psnr-steps 0 --mc-res 0 --l16 0 > "$OUT/prof_${TAG}_steady.log" 2>&1 || { echo PROF2_FAIL; exit 1; }
python3 "$R/scripts/prof_summary.py" "$OUT/prof_$TAG" "$OUT/prof_${TAG}_steady_summary.md" --last-steps 50 > /dev/null && rm -rf "$OUT/prof_$TAG"
echo PROF_OK
