"""The golden of the C3 solve's outputs (tests/test_c3_newton_gpu.py):
``python tests/golden/make_c3_newton_golden.py PATH/TO/libkmpc.so`` writes
tests/golden/c3_newton_parent.npz — W0, value, status and iters of the batches of
tests/c3_newton_cases.py (N = 65, 100, 103; 64 windows each) in mixed and float64-only precision.
The library named is one built at the commit whose results are to be kept bit for bit (the committed
file: the parent of the change that moved the Schur triangular solves' broadcast into the FMA), never
the code under test. Needs a GPU.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from koopman_mpc_portfolio_rebalancing_amd import _lib  # noqa: E402

import c3_newton_cases as cases  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    _lib._lib = _lib.load(os.path.abspath(sys.argv[1]))
    out = {}
    for N in cases.SIZES:
        wp, y = cases.batch(N)
        for prec in cases.PRECISIONS:
            r = cases.solve(wp, y, prec)
            for f in cases.FIELDS:
                out[cases.key(N, prec, f)] = r[f]
            print(f"N = {N} {prec}: statuses {np.bincount(r['status'], minlength=5).tolist()}, "
                  f"iterations {r['iters'].mean():.2f}")
    path = os.path.join(HERE, "c3_newton_parent.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
