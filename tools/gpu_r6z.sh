#!/bin/bash
# Round-6 GPU session Z: REFINE_RTOL 1e-4 alone (REFINE_MU stays 1e-6) — the GPU suite, then the
# default bench line
set -o pipefail
O=${KMPC_OUT:-kmpc_out}   # where the logs go
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > $O/gputests_z.log 2>&1 || exit $?
timeout -k 10 600 python -u bench.py --full --cpu-seconds 0 > $O/bench_z.log 2> $O/bench_z.err || exit $?
echo "exit 0"
