#!/bin/bash
# One GPU-box pass: parity tests, the default bench, and a rocprofv3 kernel-trace summary of the bench.
# Usage (from the repo root on the box): bash scripts/gpu_check.sh [tag] [bench steps] [bench warmup]
R=${GRAFT_REPO_ROOT:-$(pwd)}
# every output goes under $NEUS_OUT_DIR (an absolute path; default: bench_out/ in the repository)
OUT=${NEUS_OUT_DIR:-$R/bench_out}
cd "$R" && mkdir -p "$OUT"
TAG=${1:-run}; STEPS=${2:-200}; WARM=${3:-800}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -5 $OUT/pytest_$TAG.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup $WARM --cpu-steps 6 > $OUT/bench_$TAG.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -2 $OUT/bench_$TAG.log
if [ $rc -ne 0 ]; then exit $rc; fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run -- python3 "$R/bench.py" --full --steps 20 --warmup 800 --cpu-baseline 0 > "$OUT/prof_$TAG.log" 2>&1
rc=$?; echo "rocprof rc=$rc"
[ $rc -eq 0 ] && python3 "$R/scripts/prof_summary.py" "$OUT/prof_$TAG" --last-steps 16 > "$OUT/prof_${TAG}_summary.md" && rm -rf "$OUT/prof_$TAG"
exit $rc
