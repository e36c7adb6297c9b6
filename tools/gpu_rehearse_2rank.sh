#!/bin/bash
# 2-rank rehearsal of bench.py's N>1 path on ONE GPU (both ranks on device 0,
# the LM's reductions through the gloo host reducer instead of RCCL, which
# needs one GPU per rank): strong scaling (C5 = C4 point-sharded), iterative
# LM.  Usage: bash tools/gpu_rehearse_2rank.sh <tag>
set -o pipefail
T=${1:-rehearse}
OUT=${OUT:-out}
mkdir -p $OUT
export MI_BA_BENCH_BACKEND=gloo
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29533 bench.py --gpus 2 --full --steps 5 --warmup 2 --lm-iters 3 --no-cpu-baseline \
  > $OUT/${T}_2rank.json 2> $OUT/${T}_2rank.err || { echo "2-rank failed"; tail -20 $OUT/${T}_2rank.err; exit 1; }
grep '^{' $OUT/${T}_2rank.json | tail -c 1500
