#!/bin/bash
R=${GRAFT_REPO_ROOT:-$(pwd)}
# every output goes under $NEUS_OUT_DIR (an absolute path; default: bench_out/ in the repository)
OUT=${NEUS_OUT_DIR:-$R/bench_out}
cd "$R" && mkdir -p "$OUT"
timeout -k 10 120 python -u scripts/diag_overhead.py > $OUT/diag_overhead5.log 2>&1 || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_m" -o run -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --cpu-baseline 0 --psnr-steps 0 --mc-res 0 > "$OUT/prof_m.log" 2>&1 || exit 1
python3 "$R/scripts/prof_summary.py" "$OUT/prof_m" "$OUT/prof_m_summary.md" --last-steps 20 > /dev/null
python3 - "$OUT/prof_m" <<'PY'
import sqlite3, glob, sys
db = glob.glob(sys.argv[1] + "/**/*.db", recursive=True)[0]
con = sqlite3.connect(db)
tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
print([t for t in tabs if 'kernel' in t.lower()][:10])
PY
rm -rf "$OUT/prof_m"
