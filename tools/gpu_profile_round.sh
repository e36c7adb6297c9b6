#!/bin/bash
# Round measurement of HEAD: GPU suite, default bench line, C4 linearization
# trace + PMC (tools/profile.sh), LM kernel trace, Schur-pair PMC passes
# (tools/pmc_lm.sh), semantic-kernel PMC passes (tools/pmc_semantic.sh).
# Usage: bash tools/gpu_profile_round.sh <tag>
set -o pipefail
T=${1:-r3}
OUT=${OUT:-out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest -v --timeout 400 --timeout-method thread -m gpu tests > $OUT/${T}_tests.log 2>&1
echo "tests rc $?"
tail -3 $OUT/${T}_tests.log
timeout -k 10 600 python -u bench.py --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || { echo "bench failed"; exit 1; }
tail -c 400 $OUT/${T}_bench.json
timeout -k 10 900 bash tools/profile.sh $OUT/${T}_prof C4 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_lm -o run -- python3 bench.py --full --steps 2 --warmup 1 --lm-iters 3 --no-cpu-baseline > $OUT/${T}_lm.log 2>&1 || exit 1
echo "lm trace done"
timeout -k 10 900 bash tools/pmc_lm.sh $OUT/${T}_pmclm schur_pairs || exit 1
timeout -k 10 900 bash tools/pmc_semantic.sh $OUT/${T}_pmcs || exit 1
