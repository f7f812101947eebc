#!/bin/bash
# Round evidence on the GPU box: GPU tests, smoke, the headline bench (with the
# CPU baseline), a rocprofv3 kernel-trace summary of the headline workload, and
# separate PMC passes (FETCH_SIZE / WRITE_SIZE / TCC_EA0_ATOMIC) for the C3
# headline and the C4 / C5 per-GPU shapes, merged into $OUT/traffic.json
# by workload.  Every GPU step has its own time limit; the script stops at the
# first failure.
set -u
OUT=${OUT:-bench_out}     # where the logs and JSON lines go
mkdir -p "$OUT"
TAG=${1:-r}
# keep $OUT small (under 64 MiB), whatever step ends the
# script: the per-dispatch traces and counter rows are reduced on the box
# (kernel stats, traffic_*.json)
trap "find $OUT -name '*kernel_trace.csv' -delete; find $OUT -name '*counter_collection.csv' -delete" EXIT
export TMPDIR=/tmp
timeout -k 10 700 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/tests_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $OUT/tests_$TAG.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || exit $?
Q="--cpu-rays 0 --dropin-step 0 --train-step 0 --density-update 0 --test-time-rays 0"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --full $Q --steps 10 --warmup 3 > $OUT/prof_$TAG.log 2>&1 || exit $?
cp profiles/traffic.json $OUT/traffic.json
pmc() {   # $1 = name, rest = bench args
  local n=$1; shift
  timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmcf_${n}_$TAG -o run --output-format csv -- python3 bench.py --full $Q --steps 3 --warmup 1 "$@" > $OUT/pmcf_${n}_$TAG.log 2>&1 || return $?
  timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmcw_${n}_$TAG -o run --output-format csv -- python3 bench.py --full $Q --steps 3 --warmup 1 "$@" > $OUT/pmcw_${n}_$TAG.log 2>&1 || return $?
  timeout -k 10 300 rocprofv3 --pmc TCC_EA0_ATOMIC_sum -d $OUT/pmca_${n}_$TAG -o run --output-format csv -- python3 bench.py --full $Q --steps 3 --warmup 1 "$@" > $OUT/pmca_${n}_$TAG.log 2>&1 || return $?
  python tools/pmc_traffic.py $OUT/pmcf_${n}_$TAG $OUT/pmcw_${n}_$TAG $OUT/pmca_${n}_$TAG --merge $OUT/traffic.json > $OUT/traffic_${n}_$TAG.json
}
pmc c3 || exit $?
pmc c4 --models 4 --scale 16 --rays 4096 || exit $?
pmc c5 --models 8 --scale 16 --rays 8192 || exit $?
# the headline line (with the CPU baseline) against this code's own PMC figures
timeout -k 10 500 python bench.py --full --traffic-json $OUT/traffic.json > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
# the C4 / C5 per-GPU shapes with their own PMC figures (not the headline)
timeout -k 10 300 python bench.py --full --models 4 --scale 16 --rays 4096 --cpu-rays 0 --dropin-step 0 --traffic-json $OUT/traffic.json > $OUT/bench_c4_$TAG.json 2> $OUT/bench_c4_$TAG.err || exit $?
timeout -k 10 300 python bench.py --full --models 8 --scale 16 --rays 8192 --cpu-rays 0 --dropin-step 0 --traffic-json $OUT/traffic.json > $OUT/bench_c5_$TAG.json 2> $OUT/bench_c5_$TAG.err || exit $?
