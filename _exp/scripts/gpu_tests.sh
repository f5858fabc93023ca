#!/bin/bash
# GPU tests + optional extra bench configs
set -o pipefail
O=${OUT:-build/gpu_tests}; mkdir -p $O
export TMPDIR=/tmp
TAG=${1:-r01}
shift
timeout -k 10 600 python -u -m pytest tests -x -v --timeout 120 --timeout-method thread -m gpu > $O/gputests_$TAG.log 2>&1
rc=$?
tail -40 $O/gputests_$TAG.log
[ $rc -ne 0 ] && { echo "gpu tests failed rc=$rc"; exit 1; }
for cfg in "$@"; do
  timeout -k 10 400 python -u bench.py --full --config $cfg --steps 2 --warmup 1 --no-cpu-baseline > $O/bench_${TAG}_$cfg.json 2> $O/bench_${TAG}_$cfg.err || { echo "bench $cfg failed"; tail -20 $O/bench_${TAG}_$cfg.err; exit 1; }
  cat $O/bench_${TAG}_$cfg.json
done
