# bench.py's N>1 path rehearsed on one GPU: 2 ranks on cuda:0 over gloo
# (host-staged exchanges), the default C2 --full run and C1 -- the code path
# of the driver's scaling run, not a measurement of it (outputs in $OUT,
# run_out by default)
set -o pipefail
export TMPDIR=/tmp
export BOLT_AMD_BENCH_BACKEND=gloo BOLT_AMD_BENCH_DEVICE=0
T=${TAG:-r02}
OUT=${OUT:-run_out}
mkdir -p $OUT
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 3 --warmup 1 --full --detail $OUT/bench_n2_rehearsal_${T}_detail.json > $OUT/bench_n2_rehearsal_$T.json 2> $OUT/bench_n2_rehearsal_$T.err || { echo FAIL; tail -20 $OUT/bench_n2_rehearsal_$T.err; exit 1; }
cat $OUT/bench_n2_rehearsal_$T.json
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29534 bench.py --gpus 2 --steps 3 --warmup 1 --config C1 --full --detail $OUT/bench_n2_rehearsal_${T}_c1_detail.json > $OUT/bench_n2_rehearsal_${T}_c1.json 2> $OUT/bench_n2_rehearsal_${T}_c1.err || { echo FAIL_C1; tail -20 $OUT/bench_n2_rehearsal_${T}_c1.err; exit 1; }
cat $OUT/bench_n2_rehearsal_${T}_c1.json
echo ALL_OK
