"""One bookkeeping step of run_backtest (backtest.py:173-217) and calculate_metrics
(backtest.py:221-249) in np.longdouble — TEST INFRASTRUCTURE ONLY.

The float32 parts are taken exactly as the reference forms them, with numpy's own float32
operations, and only then widened:

    r = np.exp(y32) - np.float32(1)        (the realized simple return)
    g = np.float32(1) + r                  (the drift's growth factor)

Everything else is long double: turnover, cost, value, port, the 1e-8 guard, the drift, and the five
metrics, with NaN propagating as numpy's sum / maximum.accumulate / min do. tests/test_bt_step_ref_cpu.py
pins this file to oracle/backtest_ref (float64 numpy) at rtol 1e-13.

step_bars gives the error bars of one device step (kmpc_bt_step.h) around this reference; they are
derived in tests/test_bt_step_gpu.py's docstring.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53          # float64 unit roundoff
GUARD = LD(1e-8)            # the float64 constant of the guard, widened
METRICS = ("Sharpe Ratio", "Max Drawdown", "Avg Turnover", "Final Value", "Total Return")


def f32_returns(y):
    """(r, g) as float32 arrays: np.exp(y32) - 1 and 1 + r, numpy float32 operations."""
    y32 = np.asarray(y, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = np.exp(y32) - np.float32(1)
        g = np.float32(1) + r
    assert r.dtype == np.float32 and g.dtype == np.float32
    return r, g


def step(target, w, value, y, c):
    """One step from the state (w, value) under `target`; y: the float32 log-return row of t + 1,
    or None where the panel has none (no market move). Returns (w, value, row, sum_abs_dw,
    sum_abs_tr): the new weights [N] and value, row = (value, return, turnover, cost), and the two
    absolute sums sum_i |tg_i - w_i| and sum_i |tg_i r_i| (0 without a row) the bars need."""
    tg = np.asarray(target, dtype=LD)
    w = np.asarray(w, dtype=LD)
    value, c = LD(value), LD(c)
    with np.errstate(all="ignore"):
        sum_abs_dw = np.sum(np.abs(tg - w))
        turnover = sum_abs_dw
        cost = c * turnover * value
        value = value - cost
        port, sum_abs_tr = LD(0), LD(0)
        if y is None:
            w_new = tg.copy()
        else:
            r32, g32 = f32_returns(y)
            r, g = r32.astype(LD), g32.astype(LD)
            port = np.sum(tg * r)
            sum_abs_tr = np.sum(np.abs(tg * r))
            value = value * (LD(1) + port)
            denom = LD(1) + port
            if np.abs(denom) < GUARD:
                denom = GUARD
            w_new = tg * g / denom
    row = np.array([value, port, turnover, cost], dtype=LD)
    return w_new, value, row, sum_abs_dw, sum_abs_tr


def guard_fires(target, y):
    """(fires, |1 + port|) of the step's guard in long double."""
    r32, _ = f32_returns(y)
    with np.errstate(all="ignore"):
        d = np.abs(LD(1) + np.sum(np.asarray(target, dtype=LD) * r32.astype(LD)))
    return bool(d < GUARD), d


def step_bars(target, w, value, y, c):
    """Bars of a device step around step(...): (bar_w [N], bar_row [4]) in the row's order (value,
    return, turnover, cost). A bar whose quantity is not finite in the reference is 0: there the
    device must give the same inf or a NaN, nothing is measured."""
    tg = np.asarray(target, dtype=LD)
    w_new, v_new, row, A, B = step(target, w, value, y, c)
    value, c = LD(value), LD(c)
    with np.errstate(all="ignore"):
        e_t = 16 * U * A
        e_p = 16 * U * B
        bar_cost = np.abs(c * value) * e_t + 4 * U * np.abs(row[3])
        v1 = value - row[3]
        if y is None:
            bar_value = bar_cost + 4 * U * np.abs(v_new)
            bar_w = np.zeros(tg.shape, dtype=LD)             # a copy of the target
        else:
            one_p = LD(1) + row[1]
            bar_value = np.abs(one_p) * bar_cost + np.abs(v1) * e_p + 4 * U * np.abs(v_new)
            fires, _ = guard_fires(target, y)
            if fires or not np.isfinite(row[1]):
                bar_w = 4 * U * np.abs(w_new)                # denom exact: 1e-8, or the same inf
            else:
                bar_w = np.abs(w_new) * e_p / np.abs(one_p) + 4 * U * np.abs(w_new)
        bar_row = np.array([bar_value, e_p, e_t, bar_cost], dtype=LD)
    bar_row = np.where(np.isfinite(row) & np.isfinite(bar_row), bar_row, LD(0))
    bar_w = np.where(np.isfinite(w_new) & np.isfinite(bar_w), bar_w, LD(0))
    return bar_w, bar_row


def error_ratio(dev, ref, bar):
    """Asserts that dev has ref's NaNs and infinities in ref's places, and returns the largest
    |dev - ref| / bar over the finite entries (0 / 0 counts as 0, x / 0 as inf)."""
    dev = np.atleast_1d(np.asarray(dev, dtype=LD))
    ref = np.atleast_1d(np.asarray(ref, dtype=LD))
    bar = np.broadcast_to(np.atleast_1d(np.asarray(bar, dtype=LD)), ref.shape)
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), ("NaN positions", np.flatnonzero(np.isnan(dev) != nan)[:8])
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(dev), inf) and np.array_equal(dev[inf], ref[inf]), "infinities"
    fin = ~(nan | inf)
    if not fin.any():
        return 0.0
    err = np.abs(dev[fin] - ref[fin])
    b = bar[fin]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, LD(0), np.where(b > 0, err / np.where(b > 0, b, LD(1)), LD(np.inf)))
    return float(ratio.max())


def metrics(returns, turnover, portfolio_value):
    """calculate_metrics in long double: the five metrics in METRICS' order. numpy's rules: a NaN
    return makes the Sharpe ratio and the drawdown NaN (sum, maximum.accumulate and min propagate
    it); a zero running peak divides 0 by 0."""
    r = np.asarray(returns, dtype=LD)
    t = np.asarray(turnover, dtype=LD)
    pv = np.asarray(portfolio_value, dtype=LD)
    S = len(r)
    assert S > 0
    with np.errstate(all="ignore"):
        mean = np.sum(r) / S
        sd = np.sqrt(np.sum((r - mean) * (r - mean)) / S)
        sharpe = np.sqrt(LD(252)) * mean / (sd + GUARD)
        cum = np.cumprod(LD(1) + r)
        peak = np.maximum.accumulate(cum)
        mdd = np.min((cum - peak) / peak)
        out = np.array([sharpe, mdd, np.sum(t) / S, pv[-1], pv[-1] / pv[0] - LD(1)], dtype=LD)
    return out
