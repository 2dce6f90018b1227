#!/bin/bash
# On the GPU box: GPU tests -> smoke -> full bench (with the checked CPU leg), each step under
# its own time limit, stopping at the first failing step.  Logs go to $CHECK_OUT (default
# check_out/).  Usage: tools/gpu_check.sh [bench args...]
OUT=${CHECK_OUT:-check_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?
echo "pytest rc=$rc" >> $OUT/gpu_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 150 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || exit $?
timeout -k 10 700 python -u bench.py --full "$@" > $OUT/bench.json 2> $OUT/bench.err
