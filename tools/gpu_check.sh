#!/bin/bash
# One GPU-box pass: parity tests, smoke, bench, rocprof kernel stats of the bench.
# Usage (from the repo root on the box): bash tools/gpu_check.sh [tag]
# NO_BENCH=1: tests and smoke only; ONLY_BENCH=1: the bench line only.
set -o pipefail
tag=${1:-run}
out=gpurun_out/$tag
mkdir -p $out
export TMPDIR=/tmp
if [ -z "$ONLY_BENCH" ]; then
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > $out/pytest_gpu.log 2>&1 || { echo "gpu tests failed"; tail -40 $out/pytest_gpu.log; exit 1; }
tail -3 $out/pytest_gpu.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1 || { echo "smoke failed"; tail -30 $out/smoke.log; exit 1; }
tail -1 $out/smoke.log
fi
[ -n "$NO_BENCH" ] && exit 0
# the bench line with every secondary line and baseline (--full)
timeout -k 10 600 python -u bench.py --full > $out/bench.json 2> $out/bench.err || { echo "bench failed"; tail -30 $out/bench.err; exit 1; }
cat $out/bench.json
