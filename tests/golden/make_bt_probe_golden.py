"""The golden of the persistent backtest's return codes (tests/bt_probe.py):
``python tests/golden/make_bt_probe_golden.py PATH/TO/libkmpc.so`` writes
tests/golden/bt_probe_codes.npz — the grid's axes and the int8 codes of kmpc_backtest_run and
kmpc_backtest_sweep over it. The library named is one built at the commit whose behaviour is to be
kept (the committed file: the parent of the change that gave both entry points one host path),
never the code under test. CPU only: the probes launch nothing.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bt_probe  # noqa: E402
from koopman_mpc_portfolio_rebalancing_amd import _lib  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    lib = _lib.load(os.path.abspath(sys.argv[1]))
    t0 = time.time()
    run, sweep = bt_probe.probe_codes(lib)
    out = os.path.join(HERE, "bt_probe_codes.npz")
    np.savez_compressed(out, run=run, sweep=sweep, n_cfg=np.int32(bt_probe.N_CFG),
                        **{"axis_" + k: np.asarray(v) for k, v in bt_probe.AXES.items()})
    differ = int((run != sweep).sum())
    print(f"{out}: {run.size} cells in {time.time() - t0:.1f} s, {differ} where the two entry points differ, "
          f"codes run {sorted(set(run.ravel().tolist()))} sweep {sorted(set(sweep.ravel().tolist()))}")


if __name__ == "__main__":
    main()
