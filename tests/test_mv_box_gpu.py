"""The per-asset position limit of the mean-variance solve on the device (kmpc_solve_mv_box,
MPCConfig.max_weight through solve_mpc_mean_variance[_batched], MarkowitzStrategy(max_weight=...)),
in both storage variants of the box kernel: LDS (H N <= 128) and workspace (up to H N = 1024).

Bars (tests/mv_box_ref.py): the objective against the dense reference within 1e-9 + 1e-7 |f*| (the
project's mean-variance bar); the LP certificate gap within that plus what the kernel's stopping
rule allows, sc tol (mcon + 60 H); feasibility: budget and bounds 1e-9. W itself is compared entry
by entry only through the strong-concavity bound (the optimum has flat directions once N >= 43
with a 60-sample Sigma). tests/test_mv_box_cpu.py holds the kernel's algorithm, restated in numpy,
to the same bars on the same inputs.

Shapes (N, H): (4, 1), (10, 1) part of one wave; (64, 2) n = 128, the last LDS shape; (129, 1),
(43, 3) n = 129, the first workspace shape; (16, 8) many periods; (300, 2) ten waves; (512, 2),
(64, 16) n = 1024, the upper edge, and H = KMPC_MV_MAX_H."""
import ctypes
import functools
import glob
import os
from unittest.mock import MagicMock

import numpy as np
import pandas as pd
import pytest
import torch

import mv_box_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, MPCConfig, run_backtest, solve_mpc_mean_variance,
                                                   solve_mpc_mean_variance_batched, _lib)
from koopman_mpc_portfolio_rebalancing_amd.backtest import Strategy
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy, rolling_moments
from oracle import mv_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "mvbox_*.npz")))
DEV = torch.device("cuda", 0)


def _solve(wp, mu, S, gamma, c, u, full=True):
    """A batch through the Python entry point: (W, status, value, iters) as numpy."""
    mu = np.asarray(mu, np.float64)
    cfg = MPCConfig(horizon=mu.shape[1], gamma=float(gamma), cost_coeff=float(c), max_weight=float(u))
    out = solve_mpc_mean_variance_batched(torch.tensor(np.asarray(wp, np.float64), device=DEV), torch.tensor(mu, device=DEV),
                                          torch.tensor(np.asarray(S, np.float64), device=DEV), cfg, return_full=full,
                                          with_iters=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _one(wp, mu, S, gamma, c, u):
    W, st, val, it = _solve(wp[None], mu[None], S, gamma, c, u)
    return W[0], int(st[0]), float(val[0]), int(it[0])


def _held(tag, W, val, wp, mu, S, gamma, c, u, fref=None):
    """One solved window against the bars; returns the measured certificate gap."""
    assert not ref.violated(W, u), (tag, ref.violated(W, u))
    f = mv_ref.mv_objective(W, wp, mu, S, gamma, c)
    assert abs(val - f) <= 1e-12 * (1 + abs(f)), (tag, val, f)        # the reported value is f(W), to rounding
    gp = ref.gap(W, wp, mu, S, gamma, c, u)
    bar = ref.certificate_bar(f, mu, S, gamma, c)
    print(f"{tag}: gap {gp:.3e} (bar {bar:.3e})" +
          ("" if fref is None else f", |f - f*| {abs(val - fref):.3e} (bar {ref.objective_bar(fref):.3e})"))
    assert gp <= bar, (tag, gp, bar)
    if fref is not None:
        assert abs(val - fref) <= ref.objective_bar(fref), (tag, val, fref)
    return gp


@functools.lru_cache(maxsize=None)
def _golden(path):
    g = np.load(path)
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p) for p in FILES])
def test_goldens_on_device(path):
    g = _golden(path)
    gamma, c, u = (float(v) for v in g["config"])
    W, st, val, it = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, u)
    assert (st == 0).all(), st
    print(f"{os.path.basename(path)}: iterations {it.tolist()}")
    for b in range(len(W)):
        S = g["sigma"] if g["sigma"].ndim == 2 else g["sigma"][b]
        _held(f"{os.path.basename(path)} window {b}", W[b], val[b], g["w_prev"][b], g["mu"][b], S, gamma, c, u, g["obj"][b])
        # W through the strong-concavity bound (gamma lambda_min(Sigma)-strongly concave in each w_t)
        if gamma > 0:
            m = gamma * np.linalg.eigvalsh(S)[0]
            df = abs(g["obj"][b] - mv_ref.mv_objective(W[b], g["w_prev"][b], g["mu"][b], S, gamma, c)) + 1e-13
            assert np.abs(W[b] - g["W"][b]).max() < max(1e-5, 2 * np.sqrt(2 * df / m))
    W0, st0, val0, _ = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, u, full=False)
    assert np.array_equal(W0, W[:, 0]) and np.array_equal(st0, st) and np.array_equal(val0, val)
    W2, st2, val2, it2 = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, u)            # a relaunch
    assert np.array_equal(W2, W) and np.array_equal(val2, val) and np.array_equal(it2, it)


@pytest.mark.parametrize("case", ref.SEEDED, ids=[f"N{c[0]}_H{c[1]}" for c in ref.SEEDED])
def test_seeded_large_shapes(case):
    N, H, gamma, c, u, B = case
    wp, mu, S = ref.seeded(case)
    W, st, val, it = _solve(wp, mu, S, gamma, c, u)
    assert (st == 0).all(), st
    print(f"N={N} H={H}: iterations {it.tolist()}")
    assert W.max() > u - 1e-6          # the limit binds
    for b in range(B):
        fref = None
        if N * H <= 600:
            Wd, sd = ref.dense_mv_box_ipm(wp[b], mu[b], S[b], gamma, c, u)
            assert sd == "optimal"
            fref = mv_ref.mv_objective(Wd, wp[b], mu[b], S[b], gamma, c)
        _held(f"N={N} H={H} window {b}", W[b], val[b], wp[b], mu[b], S[b], gamma, c, u, fref)


def test_limit_that_cannot_bind():
    N, H, gamma, c, u, wp, mu, S = ref.cannot_bind()
    W, st, val, _ = _solve(wp, mu, S, gamma, c, u)
    assert (st == 0).all(), st
    for b in range(len(wp)):
        Wo, so = mv_ref.mv_dense_ipm(wp[b], mu[b], S[b], gamma, c)
        assert so == "optimal" and Wo.max() < u - 1e-3
        _held(f"cannot bind, window {b}", W[b], val[b], wp[b], mu[b], S[b], gamma, c, u,
              mv_ref.mv_objective(Wo, wp[b], mu[b], S[b], gamma, c))


@pytest.mark.parametrize("name", ["mvbox_N10_H1.npz", "mvbox_N43_H3.npz"])
def test_inactive_limit_is_the_plain_solve_python(name):
    g = _golden(os.path.join(GOLD, name))
    gamma, c, _ = (float(v) for v in g["config"])
    a = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, 1.0)
    b = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, 0.0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[0].max() > float(g["config"][2]) + 1e-3     # (and it is not the limited answer)


def _c_call(fn_box, g, u=None):
    """kmpc_solve_mv_box (u given) or kmpc_solve_mv_ws (u None) by hand, full W."""
    L = _lib.load()
    gamma, c, _ = (float(v) for v in g["config"])
    B, H, N = g["mu"].shape
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff, d.allow_short, d.max_iter, d.tol, d.return_full_W = B, N, H, gamma, c, 0, 100, 1e-10, 1
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float64), device=DEV)
    mu, S, wp = t(g["mu"]), t(g["sigma"]), t(g["w_prev"])
    W = torch.zeros((B, H, N), dtype=torch.float64, device=DEV)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    val = torch.zeros(B, dtype=torch.float64, device=DEV)
    it = torch.zeros(B, dtype=torch.int32, device=DEV)
    nws = int(L.kmpc_mv_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    stride = 0 if g["sigma"].ndim == 2 else N * N
    tail = (mu.data_ptr(), S.data_ptr(), stride, wp.data_ptr(), W.data_ptr(), st.data_ptr(), val.data_ptr(), it.data_ptr(),
            ws.data_ptr(), nws, _lib.stream_handle(DEV))
    with torch.cuda.device(DEV):
        rc = L.kmpc_solve_mv_box(ctypes.byref(d), u, *tail) if fn_box else L.kmpc_solve_mv_ws(ctypes.byref(d), *tail)
    torch.cuda.synchronize()
    assert rc == 0
    return W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy()


@pytest.mark.parametrize("name", ["mvbox_N20_H1.npz", "mvbox_N43_H3.npz"])
def test_inactive_limit_is_the_plain_solve_c(name):
    g = _golden(os.path.join(GOLD, name))
    a = _c_call(True, g, 1.0)
    b = _c_call(False, g)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert (a[1] == 0).all()
    # ... and with an active limit the same call is the Python entry point's answer
    gamma, c, u = (float(v) for v in g["config"])
    a = _c_call(True, g, u)
    b = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, u)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["mvbox_N10_H1.npz", "mvbox_N43_H3.npz"])   # LDS / workspace
def test_nan_window_between_solved_ones(name):
    g = _golden(os.path.join(GOLD, name))
    gamma, c, u = (float(v) for v in g["config"])
    wp, mu, S = g["w_prev"][:3].copy(), g["mu"][:3].copy(), g["sigma"][:3].copy()
    H = mu.shape[1]
    mu[1, 0, 1] = np.nan
    W, st, val, _ = _solve(wp, mu, S, gamma, c, u)
    assert st.tolist() == [0, 4, 0]
    assert np.array_equal(W[1], np.tile(wp[1], (H, 1))) and np.isnan(val[1])
    for b in (0, 2):
        Wb, sb, vb, _ = _solve(wp[b:b + 1], mu[b:b + 1], S[b:b + 1], gamma, c, u)
        assert np.array_equal(Wb[0], W[b]) and vb[0] == val[b] and sb[0] == 0


@pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")   # the dense reference's last iterations at c = 10
def test_edges():
    for name, wp, mu, S, gamma, c, u in ref.edge_cases():
        W, st, val, it = _one(wp, mu, S, gamma, c, u)
        assert st == 0, (name, st)
        Wd, sd = ref.dense_mv_box_ipm(wp, mu, S, gamma, c, u)
        assert sd == "optimal", name
        _held(f"{name} ({it} iterations)", W, val, wp, mu, S, gamma, c, u, mv_ref.mv_objective(Wd, wp, mu, S, gamma, c))
        if name == "c = 10, w_prev inside":
            print(f"{name}: movement {np.abs(W - wp).max():.3e}")
            assert np.abs(W - wp).max() <= 1e-8


def test_closed_forms():
    wp, mu, S, gamma, c, u = ref.WATER
    W, st, val, _ = _one(wp, mu, S, gamma, c, u)
    assert st == 0
    _held("water-filling", W, val, wp, mu, S, gamma, c, u, mv_ref.mv_objective(ref.WATER_W, wp, mu, S, gamma, c))
    assert np.abs(W - ref.WATER_W).max() <= 1e-6      # strong concavity: 2 sqrt(2 * 1e-9 / 1e-2) < 1e-3; measured far below
    wp, mu, S, gamma, c, u, G = ref.greedy_case()
    W, st, val, _ = _one(wp, mu, S, gamma, c, u)
    assert st == 0
    _held("greedy fill", W, val, wp, mu, S, gamma, c, u, mv_ref.mv_objective(G, wp, mu, S, gamma, c))
    print(f"greedy fill: |W - G| {np.abs(W - G).max():.3e}")
    assert np.abs(W - G).max() <= 1e-8
    wp, mu, S, gamma, c, u = ref.FLAT
    W, st, val, _ = _one(wp, mu, S, gamma, c, u)
    assert st == 0 and not ref.violated(W, u)
    print(f"flat mu: value {val:.12e}")
    assert abs(val - ref.FLAT_VALUE) <= 1e-8          # the value only: the optimum is not unique


def test_drop_in_api_holds_the_limit():
    """The test that fails without the feature: the limit was ignored."""
    g = _golden(os.path.join(GOLD, "mvbox_N5_H3.npz"))
    gamma, c, u = (float(v) for v in g["config"])
    cfg = MPCConfig(horizon=3, gamma=gamma, cost_coeff=c, max_weight=u)
    W, info = solve_mpc_mean_variance(g["w_prev"][0], g["mu"][0], g["sigma"][0], cfg)
    assert W.shape == (3, 5) and W.dtype == np.float64 and set(info) == {"status", "value"}
    assert info["status"] == "optimal"
    assert W.max() <= u + 1e-9
    assert abs(info["value"] - g["obj"][0]) <= ref.objective_bar(g["obj"][0])
    W1, info1 = solve_mpc_mean_variance(g["w_prev"][0], g["mu"][0], g["sigma"][0],
                                        MPCConfig(horizon=3, gamma=gamma, cost_coeff=c, max_weight=0.0))
    assert info1["status"] == "optimal" and W1.max() > u + 1e-3 and info1["value"] > info["value"]
    with pytest.raises(ValueError):
        solve_mpc_mean_variance(g["w_prev"][0], g["mu"][0], g["sigma"][0], MPCConfig(horizon=3, max_weight=0.2))
    with pytest.raises(ValueError):
        solve_mpc_mean_variance(g["w_prev"][0], g["mu"][0], g["sigma"][0], MPCConfig(horizon=3, max_weight=0.5, allow_short=True))


class _Env:
    """The FinanceEnv surface MarkowitzStrategy and run_backtest touch, over the first `rows` rows
    of the markowitz_N10 panel."""
    n_assets = 10

    def __init__(self, d, rows=None):
        z = d["z"] if rows is None else d["z"][:rows]
        self.mean, self.std = d["mean"], d["std"]
        self.stats = MagicMock()
        self.stats.mean, self.stats.std = d["mean"].astype(np.float64), d["std"].astype(np.float64)
        self.test_dataset = MagicMock()
        self.test_dataset.data = torch.tensor(z)
        self.test_dataset.dates = pd.date_range("2021-01-01", periods=len(z))
        self.test_dataset.__len__.return_value = len(z)

    def extract_current_returns(self, x):
        return x[..., :10]

    def destandardize_returns(self, x):
        return x * torch.tensor(self.std) + torch.tensor(self.mean)


class _Recording(Strategy):
    def __init__(self, inner):
        self.inner, self.targets = inner, []

    def rebalance(self, t, current_weights, env, lookback_window=60):
        w = self.inner.rebalance(t, current_weights, env, lookback_window)
        self.targets.append(np.array(w))
        return w


def test_markowitz_under_the_limit():
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    u = 0.2
    env = _Env(d)
    ts = list(d["ts"])
    W0, st, val, valid = MarkowitzStrategy(risk_aversion=1.0, cost_coeff=1e-3, max_weight=u).rebalance_batch(
        ts, d["w_prev"], env, return_info=True)
    hold = valid == 0
    assert np.array_equal(valid, d["valid"]) and hold.any() and (~hold).any()
    assert np.array_equal(W0[hold], d["w_prev"][hold])
    assert (st[~hold] == 0).all() and W0[~hold].max() <= u + 1e-9
    assert np.abs(W0[~hold].sum(1) - 1).max() <= 1e-9 and W0.min() >= -1e-9
    free = MarkowitzStrategy(risk_aversion=1.0, cost_coeff=1e-3).rebalance_batch(ts, d["w_prev"], env)
    assert np.abs(free - W0).max() > 1e-3 and free.max() > u + 1e-3
    # rolling_moments followed by kmpc_solve_mv_box by hand, bit for bit
    mu, S, v = rolling_moments(torch.tensor(d["z"], device=DEV), ts, 60, 10, d["mean"], d["std"])
    g = {"mu": mu.unsqueeze(1).cpu().numpy(), "sigma": S.cpu().numpy(), "w_prev": d["w_prev"], "config": np.array([1.0, 1e-3, u])}
    Wh, sth, valh, _ = _c_call(True, g, u)
    assert np.array_equal(Wh[~hold, 0], W0[~hold]) and np.array_equal(valh[~hold], val[~hold])
    for b in np.flatnonzero(~hold):       # ... and it is the optimum of the limited program on those moments
        wp, m, Sb = d["w_prev"][b], g["mu"][b], g["sigma"][b]
        Wd, sd = ref.dense_mv_box_ipm(wp, m, Sb, 1.0, 1e-3, u)
        assert sd == "optimal"
        _held(f"markowitz window {b}", Wh[b], valh[b], wp, m, Sb, 1.0, 1e-3, u, mv_ref.mv_objective(Wd, wp, m, Sb, 1.0, 1e-3))
    # a 12-step run_backtest: every target the strategy hands over is within the limit
    rec = _Recording(MarkowitzStrategy(risk_aversion=1.0, cost_coeff=1e-3, max_weight=u))
    df = run_backtest(rec, _Env(d, rows=14), BacktestConfig(horizon=2), verbose=False)
    assert len(df) == 12 == len(rec.targets)
    T = np.array(rec.targets)
    assert T.max() <= u + 1e-9 and np.abs(T.sum(1) - 1).max() <= 1e-9
    assert np.abs(T[5:] - 0.1).max() > 1e-3 and df["turnover"].values[5:].max() > 0      # it does trade
