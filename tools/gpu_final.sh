#!/bin/bash
# Round-end check on one GPU box: every GPU test, smoke(), then the default bench line
set -o pipefail
O=${KMPC_OUT:-kmpc_out}   # where the logs go
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gputests.log 2>&1 || exit $?
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 || exit $?
timeout -k 10 600 python -u bench.py --full > $O/bench.log 2>&1 || exit $?
echo "exit 0"
