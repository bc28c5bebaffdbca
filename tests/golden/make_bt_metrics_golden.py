"""The golden of the metrics kernel's finite histories (tests/test_bt_metrics_gpu.py):
``python tests/golden/make_bt_metrics_golden.py PATH/TO/libkmpc.so`` writes
tests/golden/bt_metrics_parent.npz — the five metrics of tests/bt_metrics_cases.golden_hist(S) for
S = 40 and 4096 (35 paths each, no NaN, no zero peak), as kmpc_backtest_metrics of the library named
returns them. That library is one built at the commit whose results are to be kept bit for bit (the
committed file: the parent of the change that made the kernel's running peak and running minimum
propagate NaN), never the code under test. Needs a GPU.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from koopman_mpc_portfolio_rebalancing_amd import _lib  # noqa: E402

import bt_metrics_cases as cases  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    _lib._lib = _lib.load(os.path.abspath(sys.argv[1]))
    out = {}
    for S in cases.GOLDEN_S:
        hist = cases.golden_hist(S)
        assert np.isfinite(hist).all()
        out[f"S{S}"] = cases.device_metrics(hist)
        assert np.isfinite(out[f"S{S}"]).all()
        print(f"S = {S}: {out[f'S{S}'].shape}, Sharpe {out[f'S{S}'][:, 0].min():.3f} .. {out[f'S{S}'][:, 0].max():.3f}, "
              f"drawdown {out[f'S{S}'][:, 1].min():.3f} .. {out[f'S{S}'][:, 1].max():.3f}")
    path = os.path.join(HERE, "bt_metrics_parent.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
