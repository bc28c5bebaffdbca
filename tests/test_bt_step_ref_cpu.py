"""tests/bt_step_ref.py (long double) pinned to oracle/backtest_ref.py (float64 numpy) at rtol 1e-13:
the step chained over a run against run_backtest, the metrics against calculate_metrics — on the
three cases of test_backtest_gpu.test_step_kernel_replays_reference_bookkeeping, on the stress
recipes of tests/bt_step_cases.py, and on one hand-built case per edge whose float64 run is exact or
well conditioned (dyadic targets where 1 + port cancels: there a float64 sum's last bit would
otherwise be the whole result). NaN and infinity positions must coincide.
"""
import warnings

import numpy as np
import pytest

import bt_step_cases as cases
import bt_step_ref as ref
from oracle import backtest_ref

RTOL = 1e-13
LD = ref.LD


def chain(targets, rows, c, capital, w0=None):
    """bt_step_ref.step chained over the targets; rows[k] is the realized row of step k or absent."""
    S, N = targets.shape
    w = np.full(N, 1.0 / N) if w0 is None else w0
    w, value = np.asarray(w, dtype=LD), LD(capital)
    hist = np.empty((S, 4), dtype=LD)
    for k in range(S):
        w, value, hist[k], _, _ = ref.step(targets[k], w, value, rows[k] if k < len(rows) else None, c)
    return hist, w


def oracle_run(targets, rows, c, capital):
    """run_backtest from 1 / N: step t reads all_returns[t + 1], so rows shift down by one."""
    S, N = targets.shape
    allr = np.concatenate([np.zeros((1, N), np.float32), np.asarray(rows, np.float32).reshape(-1, N)])
    it = iter(targets)
    seen = []

    def rebalance(t, w):
        seen.append(w)
        return next(it)

    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        h = backtest_ref.run_backtest(rebalance, allr, S + 1, 1, N, capital, 1, c)
    return np.array([[x["portfolio_value"], x["return"], x["turnover"], x["cost"]] for x in h]), seen


def assert_pinned(targets, rows, c, capital=10000.0):
    hist, w = chain(targets, rows, c, capital)
    want, _ = oracle_run(targets, rows, c, capital)
    assert hist.shape == want.shape
    np.testing.assert_allclose(hist.astype(np.float64), want, rtol=RTOL, atol=0, equal_nan=True)
    return hist, want


def assert_metrics_pinned(r, t, pv):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        m = backtest_ref.calculate_metrics(np.asarray(r, float), np.asarray(t, float), np.asarray(pv, float))
    got = ref.metrics(r, t, pv).astype(np.float64)
    want = np.array([m[k] for k in ref.METRICS])
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, equal_nan=True)
    return got, want


@pytest.mark.parametrize("N,S,tail", [(7, 11, True), (1, 6, False), (300, 8, True)])
def test_existing_cases(N, S, tail):
    rng = np.random.default_rng(N + S)
    P, capital, cost = 5, 10000.0, 1e-3
    realized = rng.normal(5e-4, 0.02, (P, S if tail else S + 1, N)).astype(np.float32)
    targets = rng.dirichlet(np.ones(N), (P, S)) if N > 1 else np.ones((P, S, 1))
    for p in range(P):
        hist, want = assert_pinned(targets[p], realized[p][1:], cost, capital)
        if tail:
            assert hist[-1, 1] == 0
        assert_metrics_pinned(want[:, 1], want[:, 2], want[:, 0])


# the recipes whose float64 run is well conditioned: A2 and B1 hold a row where 1 + port cancels to
# 1e-16 or 1e-6, whose float64 value carries the sum's rounding at 1e-10 relative or worse — those
# edges are taken below with dyadic targets, where float64 is exact
@pytest.mark.parametrize("c", [0.0, 1e-3, 2.0])
@pytest.mark.parametrize("N", [1, 2, 7, 65, 257])
@pytest.mark.parametrize("name", ["A0", "A1", "B0", "B2"])
def test_recipes(name, N, c):
    targets, rows, _, tags = cases.make_path(name, N, 0)
    hist, _ = assert_pinned(targets, rows, c)
    if name == "A1":
        assert np.isnan(hist[2, 0]) and np.isnan(hist[2, 1]) and np.isfinite(hist[2, 2:]).all()
        assert np.isfinite(hist[:2]).all() and np.isnan(hist[3, 2])
    if c == 2.0 and name == "A0" and N > 2:
        assert hist[0, 3] > 10000.0 - hist[0, 3]      # the cost exceeds what is left of the value


def test_all_crash_fires_the_guard():
    tg = np.array([[0.5, 0.25, 0.125, 0.125], [0.25, 0.25, 0.25, 0.25]])
    rows = np.full((1, 4), -110.0, np.float32)
    fires, d = ref.guard_fires(tg[0], rows[0])
    assert fires and d == 0
    hist, _ = assert_pinned(tg, rows, 1e-3)
    assert hist[0, 1] == -1 and hist[0, 0] == 0
    _, w = chain(tg[:1], rows, 1e-3, 1e4)
    assert (w == 0).all()                              # tg * (1f + -1f) / 1e-8
    assert hist[1, 2] == 1                             # the next step starts from w = 0


@pytest.mark.parametrize("t,sign", [(1.0, 1), (1.0 + 2.0 ** -19, -1)])
def test_near_guard_does_not_fire(t, sign):
    """r = -1 + 17 * 2^-24 in float32; with t = 1 or 1 + 2^-19 every product and sum is exact in
    float64: 1 + port = 17 * 2^-24 = 1.01e-6, or -15 * 2^-24 + 17 * 2^-43 = -8.9e-7."""
    y = np.array([[np.log(17 * 2.0 ** -24)]], np.float32)
    r, g = ref.f32_returns(y[0])
    assert r[0] == np.float32(-1 + 17 * 2.0 ** -24) and g[0] == np.float32(17 * 2.0 ** -24)
    tg = np.array([[t], [1.0]])
    fires, d = ref.guard_fires(tg[0], y[0])
    assert not fires and 8e-7 < d < 1.1e-6
    hist, _ = assert_pinned(tg, y, 1e-3)
    assert np.sign(1 + hist[0, 1]) == sign


def test_one_asset_crash_and_overflow():
    rng = np.random.default_rng(5)
    N = 6
    tg = rng.dirichlet(np.ones(N), 3)
    tg[1, 2] = 0.0
    rows = rng.normal(0, 0.5, (2, N)).astype(np.float32)
    rows[0, 4] = -110.0
    for j, expect in ((2, "nan"), (3, "inf")):          # y = 89 on a target of 0: 0 * inf; on a positive one: inf
        rr = rows.copy()
        rr[1, j] = 89.0
        hist, _ = assert_pinned(tg, rr, 1e-3)
        _, w = chain(tg[:1], rr[:1], 1e-3, 1e4)
        assert w[4] == 0 and (np.delete(w, 4) > 0).all()
        assert np.isnan(hist[1, 1]) if expect == "nan" else hist[1, 1] == np.inf
        _, w = chain(tg[:2], rr, 1e-3, 1e4)
        assert np.isnan(w).all() if expect == "nan" else (np.isnan(w[j]) and (np.delete(w, j) == 0).all())


def histories():
    rng = np.random.default_rng(11)
    out = {"S1": np.array([0.0123]), "S2": np.array([0.01, -0.03]), "S40": rng.normal(3e-4, 0.01, 40),
           "S4096": rng.normal(3e-4, 0.01, 4096), "zero": np.zeros(9), "up": np.abs(rng.normal(0, 0.01, 12)) + 1e-4,
           "peak0": -np.abs(rng.normal(0, 0.01, 12)) - 1e-4, "wipeout": np.array([0.02, -0.01, -1.0, 0.03, 0.01]),
           "below": np.array([0.02, -1.5, 0.1, -2.5, 0.3, 0.05])}
    return out


@pytest.mark.parametrize("name", list(histories()))
def test_metrics(name):
    r = histories()[name]
    rng = np.random.default_rng(len(r))
    got, _ = assert_metrics_pinned(r, rng.uniform(0, 0.4, len(r)), 1e4 * np.cumprod(1 + r))
    if name == "up":
        assert got[1] == 0
    if name == "wipeout":
        assert got[1] == -1 and got[4] == -1


def test_metrics_constant_returns():
    """A dyadic constant (2^-7: the float64 mean is exact, so sd = 0 on both sides; with 0.01 the
    float64 sd is rounding noise of 1e-18, 1e-10 of the floor): the 1e-8 floor alone decides."""
    r = np.full(30, 2.0 ** -7)
    got, _ = assert_metrics_pinned(r, np.full(30, 0.1), 1e4 * np.cumprod(1 + r))
    assert got[0] == pytest.approx(np.sqrt(252) * 2.0 ** -7 / 1e-8, rel=1e-14)


@pytest.mark.parametrize("r", [[np.nan, 0.01, -0.02], [0.01, -0.02, np.nan, 0.03], [0.01, -0.02, 0.03, np.nan],
                               [-1.0, 0.01, 0.02]])
def test_metrics_nan_rules(r):
    """A NaN return anywhere, or a first step of exactly -100 % (peak 0, 0 / 0): the reference's Max
    Drawdown is NaN, and so is the restatement's."""
    r = np.array(r)
    with np.errstate(all="ignore"):
        got, want = assert_metrics_pinned(r, np.full(len(r), 0.1), 1e4 * np.cumprod(1 + r))
    assert np.isnan(want[1]) and np.isnan(got[1])
    assert np.array_equal(np.isnan(got), np.isnan(want))
