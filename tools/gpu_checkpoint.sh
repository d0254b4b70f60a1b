# Checkpoint on one MI355X: the whole -m gpu suite, smoke, the default --full
# bench (C2 + 64 GiB target sub-record, PMC traffic, CPU baselines), the C1
# line, and C3 / C4 / C5 bench lines with their rocprofv3 kernel summaries.
#   TAG=r03x bash tools/gpu_checkpoint.sh            (outputs $OUT/*_$TAG*, OUT defaults to run_out)
#   SKIP_TESTS=1 ... to skip the test suite; CONFIGS="C3 C5" to choose configs
set -o pipefail
export TMPDIR=/tmp
T=${TAG:-r03}
OUT=${OUT:-run_out}
CONFIGS=${CONFIGS:-"C3 C4 C5"}
mkdir -p $OUT
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q --maxfail=30 -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/gpu_tests_$T.log 2>&1 || { echo TESTS_FAIL; tail -40 $OUT/gpu_tests_$T.log; exit 1; }
  tail -2 $OUT/gpu_tests_$T.log
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$T.log 2>&1 || { echo SMOKE_FAIL; tail $OUT/smoke_$T.log; exit 1; }
  cat $OUT/smoke_$T.log
fi
timeout -k 10 900 python bench.py --full --detail $OUT/bench_${T}_C2_detail.json > $OUT/bench_${T}_C2.json 2> $OUT/bench_${T}_C2.err || { echo BENCH_FAIL; tail $OUT/bench_${T}_C2.err; exit 1; }
cat $OUT/bench_${T}_C2.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T}_C2 -o run --output-format csv -- python bench.py --steps 10 --warmup 2 --full --no-cpu-baseline --no-pmc --no-target64 --detail $OUT/prof_${T}_C2_detail.json > $OUT/prof_${T}_C2.log 2>&1 || { echo PROF_FAIL; exit 1; }
timeout -k 10 600 python bench.py --config C1 --full --detail $OUT/bench_${T}_C1_detail.json > $OUT/bench_${T}_C1.json 2> $OUT/bench_${T}_C1.err || { echo BENCH_C1_FAIL; tail $OUT/bench_${T}_C1.err; exit 1; }
cat $OUT/bench_${T}_C1.json
for c in $CONFIGS; do
  timeout -k 10 900 python bench.py --config $c --steps 5 --warmup 1 --full --detail $OUT/bench_${T}_${c}_detail.json > $OUT/bench_${T}_$c.json 2> $OUT/bench_${T}_$c.err || { echo BENCH_${c}_FAIL; tail $OUT/bench_${T}_$c.err; exit 1; }
  cat $OUT/bench_${T}_$c.json
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${T}_$c -o run --output-format csv -- python bench.py --config $c --steps 5 --warmup 1 --full --no-cpu-baseline --no-pmc --detail $OUT/prof_${T}_${c}_detail.json > $OUT/prof_${T}_$c.log 2>&1 || { echo PROF_${c}_FAIL; exit 1; }
done
echo ALL_OK
