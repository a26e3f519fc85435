#!/bin/bash
# One GPU session: headline bench line (with the --full measurements) +
# rocprofv3 kernel stats, the -m gpu parity suite, then the L (LSTM) bench
# line + kernel stats, all under $OUT (default bench_out).  Stops at the first
# step that faults / aborts / times out (exit status other than 0 or 1).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
step() {
    local name=$1 to=$2
    shift 2
    timeout -k 10 "$to" "$@" > "$O/$name.log" 2>&1
    local rc=$?
    echo "$name rc=$rc" | tee -a "$O/steps.txt"
    tail -n 3 "$O/$name.log"
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
}
rm -f "$O/steps.txt"
step bench_b1 420 python bench.py --full --steps 20 --warmup 3
step prof_b1 420 rocprofv3 --kernel-trace --stats -d "$O/prof_b1" -o run --output-format csv -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline
step pytest_gpu 600 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread
step bench_lstm 300 python bench.py --config lstm --steps 10 --warmup 3 --no-cpu-baseline
step prof_lstm 300 rocprofv3 --kernel-trace --stats -d "$O/prof_lstm" -o run --output-format csv -- python bench.py --config lstm --steps 5 --warmup 2 --no-cpu-baseline --no-roofline
exit 0
