"""The return codes of kmpc_backtest_run and kmpc_backtest_sweep over a grid of shapes, by their
shape probe (n_steps = 0: every rule of the C boundary and of the host plan, no launch, no GPU).
The two entry points do not accept the same calls — the sweep rejects KMPC_PRECISION_MIXED where the
run's plan never takes the mixed pair, the run rejects the C3 shapes whose batch AUTO sends to the
mixed pair, and only the run reads the descriptor's cost_coeff and max_turnover — and
tests/golden/bt_probe_codes.npz (tests/golden/make_bt_probe_golden.py) pins both, cell for cell.
"""
import ctypes
import itertools

import numpy as np

from koopman_mpc_portfolio_rebalancing_amd import _lib

# the axes of the grid, in the order of the code arrays' dimensions
AXES = {
    "N": [1, 8, 10, 11, 16, 17, 32, 33, 64, 65, 103, 104, 128, 129, 215, 216, 256, 257, 1024],
    "H": [1, 2, 3, 5, 7, 10, 11, 21],
    "P": [1, 4, 512, 513, 2047, 2048],
    "allow_short": [0, 1],
    "return_full_W": [0, 1],
    "path": [0, 1, 2, 3],
    "precision": [0, 1, 2],
    "cost_turnover": [(1e-3, 0.2), (0.0, 0.2), (1e-3, 0.0), (0.0, 0.0)],
}
N_CFG = 1


def probe_codes(lib, axes=AXES):
    """-> (run, sweep): int8 arrays over the grid of axes, the code of each entry point's probe"""
    shape = tuple(len(v) for v in axes.values())
    run = np.empty(shape, np.int8).reshape(-1)
    sweep = np.empty(shape, np.int8).reshape(-1)
    sd = _lib.SolveDesc()
    bt = _lib.BacktestDesc(0, 0, 20, 1e-3)
    psd, pbt = ctypes.byref(sd), ctypes.byref(bt)
    f_run, f_sweep = lib.kmpc_backtest_run, lib.kmpc_backtest_sweep
    nul = (None,) * 6
    for i, (N, H, P, sh, full, path, prec, (c, tau)) in enumerate(itertools.product(*axes.values())):
        sd.N, sd.H, sd.allow_short, sd.return_full_W, sd.path, sd.precision = N, H, sh, full, path, prec
        sd.cost_coeff, sd.max_turnover = c, tau
        bt.P, bt.N = P, N
        run[i] = f_run(pbt, psd, 0, 0, None, None, 0, *nul, None)
        sweep[i] = f_sweep(pbt, psd, N_CFG, None, None, None, 0, 0, None, None, 0, *nul, None)
    return run.reshape(shape), sweep.reshape(shape)
