"""The covariance estimators on the device (kmpc_rolling_cov / _paths: Ledoit-Wolf, OAS, EWMA on the
float64 matrix cores) against the numpy restatement ``cov_ref`` of tests/test_cov_cpu.py, and the
strategies and backtests that read them.

Tolerances: Sigma within 1e-11 max|Sigma| and rho within 1e-10 absolute. Both sides are float64 sums of
at most 250 N terms per entry (worst-case relative error about rows 2^-53 = 3e-14; the EWMA weights are a
running product on the device, one more rounding per row), and rho divides a difference of such sums.
mu and valid are the existing kernel's, bit for bit; Sigma is bitwise symmetric.

Shapes: N in {3, 10, 16, 17, 33, 100} (below a tile, a full tile, one past it, three blocks, the headline),
lookback in {5, 7, 60, 64} and test rows from 0, so windows of 1 .. 64 rows, multiples of the k-step of 4 and
not; N = 100 with 250 rows (more than LDS would hold) and N = 1024 (64 x 64 blocks, 520 tiles per wave).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, MPCConfig, _lib, run_koopman_mv_lockstep,
                                                   run_koopman_mv_sweep, run_markowitz_lockstep, run_markowitz_sweep,
                                                   solve_mpc_mean_variance_batched)
from koopman_mpc_portfolio_rebalancing_amd.backtest import METRIC_NAMES
from koopman_mpc_portfolio_rebalancing_amd.baselines import (KoopmanMVStrategy, MarkowitzStrategy, dmd_model_spec, fit_dmd,
                                                             rolling_moments)
from koopman_mpc_portfolio_rebalancing_amd.mpc import solve_mpc_mean_variance_banded_batched
from oracle import mv_ref
from test_cov_cpu import cov_ref, window_returns

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COLS = ("portfolio_value", "return", "turnover", "cost")
HZ = 5   # BacktestConfig.horizon: n_rows = T + HZ, so the steps run to the panel's last row
TS = [0, 3, 4, 5, 20, 58, 59, 60, 69]
ESTS = [("ledoit_wolf", 0.94), ("oas", 0.94), ("ewma", 0.94), ("ewma", 0.5), ("ewma", 1.0)]
EST_IDS = ["ledoit_wolf", "oas", "ewma0.94", "ewma0.5", "ewma1"]
SIGMA_TOL, RHO_TOL = 1e-11, 1e-10


@functools.lru_cache(maxsize=None)
def panel(N, T=70, P=1, seed=0):
    """P standardized three-factor panels z [P, T, 2 N] float32 (the first N columns are the current
    returns) with their float32 de-standardisation (a non-trivial mean and std per asset)."""
    rng = np.random.default_rng(100 * N + T + seed)
    load = rng.normal(0, 1, (3, N))
    R = rng.normal(0, 1, (P, T, 3)) @ load * 0.01 + rng.normal(0, 0.005, (P, T, N))
    mean = rng.normal(5e-4, 2e-4, N).astype(np.float32)
    std = rng.uniform(0.01, 0.02, N).astype(np.float32)
    z = np.concatenate([R / std, rng.normal(0, 1, (P, T, N))], axis=-1).astype(np.float32)
    return z, mean, std


def device_cov(z2d, ts, lookback, N, mean, std, est, lam):
    mu, S, valid, rho = rolling_moments(torch.tensor(z2d, device=DEV), ts, lookback, N, mean, std, estimator=est,
                                        ewma_lambda=lam, return_shrinkage=True)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), S.cpu().numpy(), valid.cpu().numpy(), rho.cpu().numpy()


def check_against_ref(z2d, ts, lookback, N, mean, std, est, lam):
    mu, S, valid, rho = device_cov(z2d, ts, lookback, N, mean, std, est, lam)
    mu0, _, valid0 = rolling_moments(torch.tensor(z2d, device=DEV), ts, lookback, N, mean, std)
    T = z2d.shape[0]
    assert np.array_equal(valid, [int(t + 1 >= 5 and t < T) for t in ts]) and np.array_equal(valid, valid0.cpu().numpy())
    assert np.array_equal(mu, mu0.cpu().numpy())                       # mu: the existing kernel's, for every estimator
    worst_s = worst_r = 0.0
    for b, t in enumerate(ts):
        Sr, rr = cov_ref(window_returns(z2d, mean, std, t, lookback, N), est, lam)
        assert np.array_equal(S[b], S[b].T), (t, "Sigma is not bitwise symmetric")
        assert np.isfinite(S[b]).all() and np.isfinite(rho[b])
        ds, dr = np.abs(S[b] - Sr).max() / np.abs(Sr).max(), abs(rho[b] - rr)
        worst_s, worst_r = max(worst_s, ds), max(worst_r, dr)
        assert ds <= SIGMA_TOL, (t, ds)
        assert dr <= RHO_TOL, (t, rho[b], rr)
        if est == "ewma":
            assert rho[b] == 0.0
    print(f"{est} lam={lam} N={N} lookback={lookback}: |dSigma| / max|Sigma| <= {worst_s:.2e}, |drho| <= {worst_r:.2e}, rho {rho}")


@pytest.mark.parametrize("est,lam", ESTS, ids=EST_IDS)
@pytest.mark.parametrize("lookback", [5, 7, 60, 64])
@pytest.mark.parametrize("N", [3, 10, 16, 17, 33, 100])
def test_parity_with_cov_ref(N, lookback, est, lam):
    z, mean, std = panel(N)
    check_against_ref(z[0], TS, lookback, N, mean, std, est, lam)


@pytest.mark.parametrize("est,lam", ESTS[:3], ids=EST_IDS[:3])
@pytest.mark.parametrize("N,lookback,T", [(100, 250, 260), (1024, 60, 70)])
def test_streaming_and_limits(N, lookback, T, est, lam):
    """A window larger than LDS (250 rows of 100 assets: 200 KB of float64) and the largest N."""
    z, mean, std = panel(N, T)
    check_against_ref(z[0], [T - 1], lookback, N, mean, std, est, lam)


def c_moments(entry, zt, ts, lookback, N, mean, std, tail=()):
    """kmpc_rolling_moments / kmpc_rolling_cov on one panel zt [T, ld], through the C ABI."""
    L = _lib.load()
    B = len(ts)
    m, sd = torch.tensor(mean, device=DEV), torch.tensor(std, device=DEV)
    tt = torch.tensor(ts, dtype=torch.int32, device=DEV)
    mu = torch.full((B, N), np.nan, dtype=torch.float64, device=DEV)
    S = torch.full((B, N, N), np.nan, dtype=torch.float64, device=DEV)
    valid = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(getattr(L, entry)(B, zt.shape[0], N, lookback, zt.data_ptr(), zt.shape[1], m.data_ptr(), sd.data_ptr(),
                                 tt.data_ptr(), mu.data_ptr(), S.data_ptr(), valid.data_ptr(), *tail, None))
    torch.cuda.synchronize()
    return mu, S, valid


@pytest.mark.parametrize("N,lookback", [(17, 7), (100, 60)])
def test_sample_is_the_existing_kernel(N, lookback):
    z, mean, std = panel(N)
    zt = torch.tensor(z[0], device=DEV)
    old = c_moments("kmpc_rolling_moments", zt, TS, lookback, N, mean, std)
    rho = torch.full((len(TS),), np.nan, dtype=torch.float64, device=DEV)
    new = c_moments("kmpc_rolling_cov", zt, TS, lookback, N, mean, std, (0, 0.94, rho.data_ptr()))
    norho = c_moments("kmpc_rolling_cov", zt, TS, lookback, N, mean, std, (0, float("nan"), None))   # (lambda: EWMA's alone)
    for a, b, c in zip(old, new, norho):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert bool((rho == 0).all())
    # the Python surface: the defaults are the existing call, "sample" by name too, with a zero shrinkage
    dflt = rolling_moments(zt, TS, lookback, N, mean, std)
    named = rolling_moments(zt, TS, lookback, N, mean, std, estimator="sample", return_shrinkage=True)
    assert len(dflt) == 3 and len(named) == 4 and bool((named[3] == 0).all())
    for a, b, c in zip(old, dflt, named):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("est,lam", ESTS[:4], ids=EST_IDS[:4])
@pytest.mark.parametrize("N,lookback", [(17, 7), (100, 60)])
def test_paths_and_determinism(N, lookback, est, lam):
    """P = 3 panels in one launch equal three single-panel calls, and a second launch the first, bit for bit."""
    P, T = 3, 70
    z, mean, std = panel(N, T, P)
    L = _lib.load()
    code = _lib.COV_ESTIMATOR[est]
    zt = torch.tensor(z, device=DEV)
    m, sd = torch.tensor(mean, device=DEV), torch.tensor(std, device=DEV)
    tt = torch.tensor(TS, dtype=torch.int32, device=DEV)
    n = len(TS)

    def launch():
        mu = torch.full((n, P, N), np.nan, dtype=torch.float64, device=DEV)
        S = torch.full((n, P, N, N), np.nan, dtype=torch.float64, device=DEV)
        valid = torch.full((n, P), -1, dtype=torch.int32, device=DEV)
        rho = torch.full((n, P), np.nan, dtype=torch.float64, device=DEV)
        _lib.check(L.kmpc_rolling_cov_paths(P, n, T, N, lookback, zt.data_ptr(), zt.shape[2], m.data_ptr(), sd.data_ptr(),
                                            tt.data_ptr(), mu.data_ptr(), S.data_ptr(), valid.data_ptr(), code, lam,
                                            rho.data_ptr(), None))
        torch.cuda.synchronize()
        return mu, S, valid, rho

    first, again = launch(), launch()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for p in range(P):
        rho1 = torch.full((n,), np.nan, dtype=torch.float64, device=DEV)
        one = c_moments("kmpc_rolling_cov", zt[p], TS, lookback, N, mean, std, (code, lam, rho1.data_ptr())) + (rho1,)
        for a, b in zip(first, one):
            assert torch.equal(a[:, p], b), p
    assert not torch.equal(first[1][:, 0], first[1][:, 1])   # (the panels differ)


@pytest.mark.parametrize("N,lookback", [(10, 60), (17, 7)])
def test_degenerate_windows(N, lookback):
    """A constant panel: X = 0, so Sigma = 1e-6 I exactly, rho = 0 (Ledoit-Wolf: beta = 0) or 1 (OAS: den = 0)."""
    _, mean, std = panel(N)
    z = np.full((70, 2 * N), np.float32(0.37))
    eye = 1e-6 * np.eye(N)
    for est, want in (("ledoit_wolf", 0.0), ("oas", 1.0)):
        _, S, _, rho = device_cov(z, TS, lookback, N, mean, std, est, 0.94)
        assert np.isfinite(S).all() and np.isfinite(rho).all()
        assert (rho == want).all(), (est, rho)
        for b in range(len(TS)):
            assert np.array_equal(S[b], eye), (est, TS[b])
    _, S, _, rho = device_cov(z, TS, lookback, N, mean, std, "ewma", 0.94)   # (the weighted mean rounds: X is a few ulp)
    assert np.isfinite(S).all() and (rho == 0).all() and np.abs(S - eye).max() <= 1e-11 * 1e-6


class _Env:
    """The FinanceEnv surface the strategies touch, over rows z [T, 2 N]."""

    def __init__(self, z, mean, std):
        from unittest.mock import MagicMock
        self.n_assets = len(mean)
        self.stats = MagicMock()
        self.stats.mean, self.stats.std = mean.astype(np.float64), std.astype(np.float64)
        self.test_dataset = MagicMock()
        self.test_dataset.data = torch.tensor(z)


STRAT_TS = [2, 4, 9, 30, 69]


@pytest.mark.parametrize("est,lam", [("ledoit_wolf", 0.94), ("ewma", 0.9)])
def test_markowitz_strategy_reads_the_estimator(est, lam):
    N = 10
    z, mean, std = panel(N)
    env = _Env(z[0], mean, std)
    s = MarkowitzStrategy(risk_aversion=2.0, cost_coeff=1e-3, cov_estimator=est, cov_ewma_lambda=lam)
    wp = np.random.default_rng(3).dirichlet(np.ones(N), len(STRAT_TS))
    W0, st, _, valid = s.rebalance_batch(STRAT_TS, wp, env, return_info=True)
    zt, wt = torch.tensor(z[0], device=DEV), torch.tensor(wp, device=DEV)
    mu, sigma, v = rolling_moments(zt, STRAT_TS, 60, N, mean, std, estimator=est, ewma_lambda=lam)
    Wd, _, _ = solve_mpc_mean_variance_batched(wt, mu.unsqueeze(1), sigma, s.mpc_config)
    Wd = torch.where((v == 0).unsqueeze(1), wt, Wd).cpu().numpy()
    assert np.array_equal(W0, Wd) and np.array_equal(valid, v.cpu().numpy())
    plain = MarkowitzStrategy(risk_aversion=2.0, cost_coeff=1e-3).rebalance_batch(STRAT_TS, wp, env)
    for b, t in enumerate(STRAT_TS):
        if t + 1 < 5:
            assert np.array_equal(W0[b], wp[b])
            continue
        Sr, _ = cov_ref(window_returns(z[0], mean, std, t, 60, N), est, lam)
        Wr, info = mv_ref.solve_mpc_mean_variance_ref(wp[b], mu[b].cpu().numpy()[None], Sr, 2.0, 1e-3)
        print(f"t = {t}: |W0 - oracle| {np.abs(W0[b] - Wr[0]).max():.2e}, |W0 - sample's| {np.abs(W0[b] - plain[b]).max():.2e}")
        assert info["status"] == "optimal" and st[b] == 0
        assert np.abs(W0[b] - Wr[0]).max() < 1e-5                       # tests/test_mv_gpu.py's tolerance
    assert not np.array_equal(W0, plain)                                 # the estimator reaches the solve


@pytest.mark.parametrize("est,lam", [("ledoit_wolf", 0.94), ("ewma", 0.9)])
def test_koopman_mv_strategy_reads_the_estimator(est, lam):
    N, H = 12, 3
    z, mean, std = panel(N)
    env = _Env(z[0], mean, std)
    cfg = MPCConfig(horizon=H, gamma=2.0, cost_coeff=1e-3)
    s = KoopmanMVStrategy(dmd_model_spec(fit_dmd(torch.tensor(z[0]))), cfg, cov_estimator=est, cov_ewma_lambda=lam)
    km = s.device_model()
    wp = np.random.default_rng(4).dirichlet(np.ones(N), len(STRAT_TS))
    W0, st, _, valid = s.rebalance_batch(STRAT_TS, wp, env, return_info=True)
    zt, wt = torch.tensor(z[0], device=DEV), torch.tensor(wp, device=DEV)
    yhat = km.rollout(zt[torch.tensor(STRAT_TS, device=DEV)], mean.astype(np.float64), std.astype(np.float64), H, N)
    _, sigma, v = rolling_moments(zt, STRAT_TS, 60, N, mean, std, estimator=est, ewma_lambda=lam)
    Wd, _, _ = solve_mpc_mean_variance_banded_batched(wt, yhat, sigma, cfg)
    Wd = torch.where((v == 0).unsqueeze(1), wt, Wd).cpu().numpy()
    assert np.array_equal(W0, Wd) and np.array_equal(valid, v.cpu().numpy())
    plain = KoopmanMVStrategy(km, cfg).rebalance_batch(STRAT_TS, wp, env)
    y = yhat.cpu().numpy().astype(np.float64)
    for b, t in enumerate(STRAT_TS):
        if t + 1 < 5:
            assert np.array_equal(W0[b], wp[b])
            continue
        Sr, _ = cov_ref(window_returns(z[0], mean, std, t, 60, N), est, lam)
        Wr, info = mv_ref.solve_mpc_mean_variance_ref(wp[b], y[b], Sr, 2.0, 1e-3)
        print(f"t = {t}: |W0 - oracle| {np.abs(W0[b] - Wr[0]).max():.2e}, |W0 - sample's| {np.abs(W0[b] - plain[b]).max():.2e}")
        assert info["status"] == "optimal" and st[b] == 0
        assert np.abs(W0[b] - Wr[0]).max() < 1e-5
    assert not np.array_equal(W0, plain)


# ---- backtests: each run against the per-step loop written out ---------------------------------

def assert_same(a, b, what):
    for k in COLS + ("weights",):
        assert torch.equal(a[k], b[k]), (what, k)
    for k, v in a["metrics"].items():
        assert torch.equal(v, b["metrics"][k]), (what, k)


def realized_of(z, mean, std, N):
    return (z[:, :, :N] * std + mean).astype(np.float32)


def hand_loop(solve, est, lam, z, mean, std, realized, N, bt_cost=1e-3, capital=10000.0):
    """Per step: the rolling covariance of every path under the estimator (one single-panel call each),
    solve(k, w, mu, sigma) -> W0 [P, N], the hold select, kmpc_backtest_step; then the metrics."""
    L = _lib.load()
    P, T = z.shape[:2]
    zt, rt = torch.tensor(z, device=DEV), torch.tensor(realized, device=DEV)
    f64 = dict(dtype=torch.float64, device=DEV)
    w = torch.full((P, N), 1.0 / N, **f64)
    value = torch.full((P,), capital, **f64)
    hist = torch.empty((P, T, 4), **f64)
    met = torch.empty((P, 5), **f64)
    bd = _lib.BacktestDesc(P, N, T, bt_cost)
    for t in range(T):
        mom = [rolling_moments(zt[p], [t], 60, N, mean, std, estimator=est, ewma_lambda=lam) for p in range(P)]
        mu, sigma, valid = (torch.cat([m[i] for m in mom]).contiguous() for i in range(3))
        W0 = solve(t, w, mu, sigma)
        tg = torch.where((valid == 0).unsqueeze(1), w, W0).contiguous()
        rn = rt[:, t + 1].contiguous() if t + 1 < T else None
        _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), t, tg.data_ptr(), rn.data_ptr() if rn is not None else None,
                                        w.data_ptr(), value.data_ptr(), hist.data_ptr(), _lib.stream_handle(DEV)))
    _lib.check(L.kmpc_backtest_metrics(ctypes.byref(bd), hist.data_ptr(), met.data_ptr(), _lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    out = {k: hist[..., i] for i, k in enumerate(COLS)}
    out["weights"] = w
    out["metrics"] = {name: met[:, j] for j, name in enumerate(METRIC_NAMES)}
    return out


def markowitz(N, H, est, lam, gamma=1.0, cost=1e-3):
    s = MarkowitzStrategy(risk_aversion=gamma, cost_coeff=cost, cov_estimator=est, cov_ewma_lambda=lam)
    s.mpc_config.horizon = H   # (H > 1: the rolling mean in every period)
    return s


def markowitz_loop(s, est, lam, z, mean, std, realized, N, H, bt_cost=1e-3):
    P = z.shape[0]
    solve = lambda t, w, mu, sigma: solve_mpc_mean_variance_batched(
        w, mu[:, None, :].expand(P, H, N).contiguous(), sigma, s.mpc_config)[0]
    return hand_loop(solve, est, lam, z, mean, std, realized, N, bt_cost)


def koopman_loop(km, cfg, est, lam, z, mean, std, realized, N, H, bt_cost=1e-3):
    P, T = z.shape[:2]
    zt = torch.tensor(z, device=DEV)
    y = km.rollout(zt.transpose(0, 1).reshape(T * P, -1), mean, std, H, N).reshape(T, P, H, N)
    solve = lambda t, w, mu, sigma: solve_mpc_mean_variance_banded_batched(w, y[t].contiguous(), sigma, cfg)[0]
    return hand_loop(solve, est, lam, z, mean, std, realized, N, bt_cost)


BT_ESTS = [("ledoit_wolf", 0.94), ("ewma", 0.9)]
BT_T, BT_P = 40, 3


@pytest.mark.parametrize("est,lam", BT_ESTS, ids=["ledoit_wolf", "ewma"])
@pytest.mark.parametrize("N,H", [(10, 1), (12, 3)])
def test_markowitz_lockstep_is_the_loop(N, H, est, lam):
    z, mean, std = panel(N, BT_T, BT_P)
    realized = realized_of(z, mean, std, N)
    s = markowitz(N, H, est, lam)
    bt = BacktestConfig(horizon=HZ)
    run = lambda st, **kw: run_markowitz_lockstep(st, z, realized, bt, mean, std, n_rows=BT_T + HZ, **kw)
    per = run(s, persistent=True)
    hand = markowitz_loop(s, est, lam, z, mean, std, realized, N, H)
    assert per["return"].shape == (BT_P, BT_T)
    assert_same(per, hand, "persistent vs the loop written out")
    assert_same(per, run(s, persistent=False), "persistent vs persistent=False")
    assert not torch.equal(per["portfolio_value"], run(markowitz(N, H, "sample", 0.94))["portfolio_value"])


@pytest.mark.parametrize("est,lam", BT_ESTS, ids=["ledoit_wolf", "ewma"])
@pytest.mark.parametrize("N,H", [(10, 3), (12, 3)])
def test_koopman_mv_lockstep_is_the_loop(N, H, est, lam):
    z, mean, std = panel(N, BT_T, BT_P)
    realized = realized_of(z, mean, std, N)
    cfg = MPCConfig(horizon=H, gamma=2.0, cost_coeff=1e-3)
    s = KoopmanMVStrategy(dmd_model_spec(fit_dmd(torch.tensor(z[0]))), cfg, cov_estimator=est, cov_ewma_lambda=lam)
    km = s.device_model()
    bt = BacktestConfig(horizon=HZ)
    run = lambda st, **kw: run_koopman_mv_lockstep(st, z, realized, bt, mean, std, n_rows=BT_T + HZ, **kw)
    hand = koopman_loop(km, cfg, est, lam, z, mean, std, realized, N, H)
    per = run(s, persistent=True)
    assert per["return"].shape == (BT_P, BT_T)
    assert_same(per, hand, "persistent=True vs the loop written out")
    assert_same(run(s, persistent=False), hand, "persistent=False vs the loop written out")
    assert not torch.equal(per["portfolio_value"], run(KoopmanMVStrategy(km, cfg))["portfolio_value"])


def config_rows(sw, j):
    out = {k: sw[k][j] for k in COLS + ("weights",)}
    out["metrics"] = {k: v[j] for k, v in sw["metrics"].items()}
    return out


@pytest.mark.parametrize("est,lam", BT_ESTS, ids=["ledoit_wolf", "ewma"])
@pytest.mark.parametrize("N,H", [(10, 1), (12, 3)])
def test_markowitz_sweep_rows_are_the_loop(N, H, est, lam):
    z, mean, std = panel(N, BT_T, BT_P)
    realized = realized_of(z, mean, std, N)
    bt = BacktestConfig(horizon=HZ)
    gammas, costs = [1.0, 4.0], [1e-3, 2e-3]
    sw = run_markowitz_sweep(markowitz(N, H, est, lam), z, realized, bt, mean, std, gammas, costs, n_rows=BT_T + HZ)
    assert sw["return"].shape == (2, BT_P, BT_T)
    for j in range(2):
        sj = markowitz(N, H, est, lam, gammas[j], costs[j])
        assert_same(config_rows(sw, j), markowitz_loop(sj, est, lam, z, mean, std, realized, N, H), f"config {j}")
    assert not torch.equal(sw["weights"][0], sw["weights"][1])


@pytest.mark.parametrize("est,lam", BT_ESTS, ids=["ledoit_wolf", "ewma"])
@pytest.mark.parametrize("N,H", [(10, 3), (12, 3)])
def test_koopman_mv_sweep_rows_are_the_loop(N, H, est, lam):
    z, mean, std = panel(N, BT_T, BT_P)
    realized = realized_of(z, mean, std, N)
    cfgs = [MPCConfig(horizon=H, gamma=1.0, cost_coeff=1e-3), MPCConfig(horizon=H, gamma=4.0, cost_coeff=2e-3)]
    s = KoopmanMVStrategy(dmd_model_spec(fit_dmd(torch.tensor(z[0]))), cfgs[0], cov_estimator=est, cov_ewma_lambda=lam)
    km = s.device_model()
    bt = BacktestConfig(horizon=HZ)
    sw = run_koopman_mv_sweep(s, z, realized, bt, mean, std, cfgs, n_rows=BT_T + HZ)
    assert sw["return"].shape == (2, BT_P, BT_T)
    for j in range(2):
        assert_same(config_rows(sw, j), koopman_loop(km, cfgs[j], est, lam, z, mean, std, realized, N, H), f"config {j}")
    assert not torch.equal(sw["weights"][0], sw["weights"][1])
