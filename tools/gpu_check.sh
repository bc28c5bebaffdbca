#!/bin/bash
# GPU parity tests + smoke + default bench (no profiler passes) [+ f64 peak probe].
set -o pipefail
O=${KMPC_OUT:-kmpc_out}   # where the logs go
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 700 python -u -m pytest ${1:-tests} -m gpu -x -v --timeout 180 --timeout-method thread > $O/gputests.log 2>&1 &&
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 &&
timeout -k 10 400 python bench.py --full > $O/bench.log 2>$O/bench.err &&
{ [ ! -x tools/dev/f64_peak ] || timeout -k 10 60 tools/dev/f64_peak > $O/f64_peak.log 2>&1; }
echo "exit $?"
