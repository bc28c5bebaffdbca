"""Histories of the metrics-kernel tests (tests/test_bt_metrics_gpu.py) and of their golden
(tests/golden/make_bt_metrics_golden.py), and the one call of kmpc_backtest_metrics both make.

history(kind, S, rng): the step returns of one path.
    normal    r ~ N(3e-4, 0.01)
    const     one constant (sd is rounding noise: the 1e-8 floor of the Sharpe ratio decides)
    zero      all 0
    up        all positive (drawdown 0, the peak at the end)
    peak0     all negative (the peak at k = 0 only)
    wipeout   a -100 % step in the middle (cum = 0 afterwards: drawdown -1, total return -1)
    below     up to three returns below -1 (cum changes sign)
    nan0 / nanmid / nanend   one NaN return at k = 0, in the middle, at the end
    first100  a first step of exactly -100 % (peak 0: 0 / 0)
FINITE: the kinds without NaN and with non-zero peaks; NANS: the others.

golden_hist(S): GOLDEN_P histories whose every number comes from integer arithmetic and one float64
multiply-add, so that the file is the same wherever it is generated.
"""
from __future__ import annotations

import ctypes

import numpy as np

FINITE = ("normal", "const", "zero", "up", "peak0", "wipeout", "below")
NANS = ("nan0", "nanmid", "nanend", "first100")
KINDS = FINITE + NANS
GOLDEN_P = 35
GOLDEN_S = (40, 4096)


def history(kind, S, rng):
    r = rng.normal(3e-4, 0.01, S)
    if kind == "const":
        r[:] = 0.01
    elif kind == "zero":
        r[:] = 0.0
    elif kind == "up":
        r = np.abs(r) + 1e-5
    elif kind == "peak0":
        r = -np.abs(r) - 1e-5
    elif kind == "wipeout":
        r[S // 2] = -1.0
    elif kind == "below":
        r[rng.choice(S, min(S, 3), replace=False)] = (-1.5, -2.5, -1.25)[:min(S, 3)]
    elif kind == "nan0":
        r[0] = np.nan
    elif kind == "nanmid":
        r[S // 2] = np.nan
    elif kind == "nanend":
        r[-1] = np.nan
    elif kind == "first100":
        r[0] = -1.0
    elif kind != "normal":
        raise ValueError(kind)
    return r


def assemble(returns, turnover):
    """hist [P, S, 4] float64: value = 1e4 cumprod(1 + r), return, turnover, cost 0."""
    returns = np.asarray(returns, dtype=np.float64)
    hist = np.zeros(returns.shape + (4,))
    with np.errstate(all="ignore"):
        hist[..., 0] = 1e4 * np.cumprod(1 + returns, axis=-1)
    hist[..., 1] = returns
    hist[..., 2] = turnover
    return hist


def paths(P, S, seed, kinds=KINDS):
    """P histories of S steps, path p of kind kinds[p % len(kinds)], each with draws of its own."""
    rng = np.random.default_rng([seed, P, S])
    r = np.stack([history(kinds[p % len(kinds)], S, rng) for p in range(P)])
    return assemble(r, rng.uniform(0, 0.4, (P, S)))


def golden_hist(S):
    p, k = np.meshgrid(np.arange(GOLDEN_P, dtype=np.uint64), np.arange(S, dtype=np.uint64), indexing="ij")
    h = (k * np.uint64(2654435761) + p * np.uint64(40503) + np.uint64(12345)) % np.uint64(65536)
    r = h.astype(np.float64) / 65536.0 * 0.04 - 0.0197           # in [-0.0197, 0.0203)
    h2 = (k * np.uint64(40503) + p * np.uint64(2654435761) + np.uint64(7)) % np.uint64(65536)
    r[5::7, S // 2] = -1.0                                       # five wiped-out paths
    r[6::7, S // 3] = -1.5                                       # five whose cum changes sign
    r[4::7] = -np.abs(r[4::7]) - 2.0 ** -20                      # five with the peak at k = 0
    return assemble(r, h2.astype(np.float64) / 65536.0 * 0.4)


def device_metrics(hist, S=None):
    """kmpc_backtest_metrics over hist [P, S, 4] through the loaded library: [P, 5] float64."""
    import torch
    from koopman_mpc_portfolio_rebalancing_amd import _lib
    P = hist.shape[0]
    S = hist.shape[1] if S is None else S
    d = _lib.BacktestDesc(P, 4, S, 1e-3)
    h = torch.tensor(np.ascontiguousarray(hist), dtype=torch.float64, device="cuda")
    met = torch.empty((P, 5), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().kmpc_backtest_metrics(ctypes.byref(d), h.data_ptr(), met.data_ptr(), None))
    torch.cuda.synchronize()
    return met.cpu().numpy()
