set -o pipefail
# Round-end check on one MI355X: the GPU test suite, smoke() and the bench
# line, product library only (bash tools/gpu_round_final.sh).
OUT=${OUT:-out}
mkdir -p $OUT/r5final4
timeout -k 10 1100 python -u -m pytest -v --timeout 400 --timeout-method thread -m gpu tests > $OUT/r5final4/tests.log 2>&1 &&
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/r5final4/smoke.log 2>&1 &&
timeout -k 10 600 python -u bench.py --full > $OUT/r5final4/bench.json 2> $OUT/r5final4/bench.err
