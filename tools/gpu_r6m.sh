#!/bin/bash
# Round-6 GPU session M: the one-GPU rate against the batch a rank solves at N = 1 / 8 / 4 / 2
# (65,536 / 131,072 / 262,144 / 524,288 windows of the bench stream; headline line only)
set -o pipefail
O=${KMPC_OUT:-kmpc_out}   # where the logs go
mkdir -p $O
: > $O/r6m.log
for G in 65536 131072 262144 524288; do
  echo "== $G" >> $O/r6m.log
  timeout -k 10 400 python -u bench.py --full --headline-only --steps 3 --warmup 1 --global-windows $G >> $O/r6m.log 2>>$O/r6m.err || exit $?
done
echo "exit 0"
