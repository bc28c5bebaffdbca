"""The Markowitz strategy and its device backtest under the L1 turnover cap
(MarkowitzStrategy(max_turnover=...), kmpc_markowitz_run_cap, kmpc_markowitz_sweep_cap): the cap holds
at every recorded step, the persistent kernel equals the per-step loop bit for bit, launches resume
each other's state, an infeasible step (under a limit, after drift) holds and the path goes on, and
the sweep's rows equal single runs. Helpers (panels, tolerances) are tests/test_markowitz_bt_gpu.py's."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mv_cap_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, _lib, run_backtest, run_markowitz_lockstep,
                                                   run_markowitz_sweep, sweep_backtest_markowitz)
from koopman_mpc_portfolio_rebalancing_amd import baselines
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy
from test_markowitz_bt_gpu import COLS, HZ, _Env, assert_config_rows, assert_same, close_to, golden_paths, panel
from test_mv_box_gpu import _Env as _GoldenEnv, _Recording

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAU = 0.2


def capped(N, H=1, tau=TAU, limit=0.0, gamma=1.0, cost=1e-3, short=False):
    s = MarkowitzStrategy(gamma, cost, short, max_weight=limit, max_turnover=tau)
    s.mpc_config.horizon = H
    return s


def test_max_turnover_keyword_holds_the_cap_at_every_step():
    """The test that fails without the feature (TypeError: no such keyword): a 12-step run_backtest
    on the first 14 rows of the markowitz_N10 panel. Uncapped, steps 4 and 6 turn over 1.59 and 1.79
    (tests/test_mv_cap_cpu.py, the oracle); capped, no step passes 0.2 plus the cap bar."""
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    cfg = BacktestConfig(horizon=2)
    rec = _Recording(MarkowitzStrategy(1.0, 1e-3, max_turnover=TAU))
    df = run_backtest(rec, _GoldenEnv(d, rows=14), cfg, verbose=False)
    free = run_backtest(MarkowitzStrategy(1.0, 1e-3), _GoldenEnv(d, rows=14), cfg, verbose=False)
    to = df["turnover"].values
    print(f"turnover per step, capped: {np.round(to, 12).tolist()}; excess {to.max() - TAU:.3e} (bar {ref.cap_bar(10):.3e})")
    print(f"turnover per step, uncapped: {np.round(free['turnover'].values, 3).tolist()}")
    assert len(df) == 12 == len(rec.targets)
    assert to.max() <= TAU + ref.cap_bar(10)
    assert to.max() >= TAU - 1e-6 and (to[:4] == 0).all()                  # it binds; the first four steps hold
    assert free["turnover"].values.max() > 1.0
    T = np.array(rec.targets)
    assert np.abs(T.sum(1) - 1).max() <= 1e-9 and T.min() >= -1e-9
    # rebalance_batch carries the cap too: the stored windows, each from its own w_prev
    W0, st, val, valid = MarkowitzStrategy(1.0, 1e-3, max_turnover=TAU).rebalance_batch(
        list(d["ts"]), d["w_prev"], _GoldenEnv(d), return_info=True)
    ok = valid == 1
    assert (st[ok] == 0).all() and np.abs(W0[ok] - d["w_prev"][ok]).sum(1).max() <= TAU + ref.cap_bar(10)
    assert np.array_equal(W0[~ok], d["w_prev"][~ok])


@pytest.mark.parametrize("N,H,P,limit", [(10, 1, 3, 0.0), (43, 3, 3, 0.0), (10, 1, 3, 0.25)])
def test_persistent_equals_the_per_step_loop(N, H, P, limit, monkeypatch):
    """kmpc_markowitz_run_cap against the per-step loop (kmpc_solve_mv_cap, the hold select,
    kmpc_backtest_step), bit for bit, over the valid == 0 hold steps; a relaunch and a run split into
    launches of 5 steps are identical; the cap holds at every step and binds at some."""
    steps = 12
    z, mean, std, realized = panel(N, P, steps)
    cfg = BacktestConfig(horizon=HZ)
    s = capped(N, H, limit=limit)
    per = run_markowitz_lockstep(s, z, realized, cfg, mean, std, n_rows=steps + HZ, persistent=True)
    loop = run_markowitz_lockstep(s, z, realized, cfg, mean, std, n_rows=steps + HZ, persistent=False)
    assert per["return"].shape == (P, steps)
    assert_same(per, loop, "persistent vs per-step loop")
    assert_same(per, run_markowitz_lockstep(s, z, realized, cfg, mean, std, n_rows=steps + HZ), "default, relaunch")
    to = per["turnover"].cpu().numpy()
    print(f"N = {N}, H = {H}: largest turnover - tau {to.max() - TAU:.3e} (bar {ref.cap_bar(N):.3e})")
    assert to.max() <= TAU + ref.cap_bar(N) and to.max() >= TAU - 1e-6
    assert (to[:, :4] == 0).all() and (to[:, 4:] > 0).any()                # fewer than 5 rows: hold
    free = run_markowitz_lockstep(capped(N, H, 0.0, limit), z, realized, cfg, mean, std, n_rows=steps + HZ)
    assert float(free["turnover"].max()) > 2 * TAU                          # tau = 0: the uncapped run trades more
    monkeypatch.setattr(baselines, "MARKOWITZ_CHUNK", 5)
    assert_same(per, run_markowitz_lockstep(s, z, realized, cfg, mean, std, n_rows=steps + HZ, persistent=True), "chunks")


def test_zero_cap_is_the_existing_run_bit_for_bit():
    N, P, steps = 10, 3, 12
    z, mean, std, realized = panel(N, P, steps)
    cfg = BacktestConfig(horizon=HZ)
    a = run_markowitz_lockstep(MarkowitzStrategy(1.0, 1e-3, max_turnover=0.0), z, realized, cfg, mean, std, n_rows=steps + HZ)
    b = run_markowitz_lockstep(MarkowitzStrategy(1.0, 1e-3), z, realized, cfg, mean, std, n_rows=steps + HZ)
    assert_same(a, b, "max_turnover = 0")


def _moments(z, mean, std, ts):
    """kmpc_rolling_moments_paths at the test rows ts of the P panels z: (mu [S, P, N], sigma, valid)."""
    L = _lib.load()
    dev = torch.device("cuda")
    P, T, ld = z.shape
    N = len(mean)
    f64 = dict(dtype=torch.float64, device=dev)
    zt = torch.tensor(z, device=dev)
    tt = torch.tensor(ts, dtype=torch.int32, device=dev)
    mu, sigma = torch.empty((len(ts), P, N), **f64), torch.empty((len(ts), P, N, N), **f64)
    valid = torch.empty((len(ts), P), dtype=torch.int32, device=dev)
    m, sd = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    _lib.check(L.kmpc_rolling_moments_paths(P, len(ts), T, N, 60, zt.data_ptr(), ld, m.data_ptr(), sd.data_ptr(),
                                            tt.data_ptr(), mu.data_ptr(), sigma.data_ptr(), valid.data_ptr(), None))
    return mu, sigma, valid


def test_an_infeasible_step_holds_and_the_path_goes_on():
    """u = 0.25 with three assets on the limit and tau = 0.004: whenever the drift carries more than
    E = tau / 2 above the limit the step's window is infeasible (d0 = 2E > tau): status 2, the target is
    the drifted weights, turnover 0, and the next step solves or holds on its own. One launch per step
    shows every step's status; one launch of all steps gives the same history and weights."""
    N, P, steps, u, tau = 10, 3, 10, 0.25, 0.004
    z, mean, std, realized = panel(N, P, steps + 6)
    ts = list(range(5, 5 + steps))
    mu, sigma, valid = _moments(z, mean, std, ts)
    assert bool((valid == 1).all())
    L = _lib.load()
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    rt = torch.tensor(realized, device=dev).transpose(0, 1)[6:6 + steps].contiguous()     # row t + 1 of each step
    w0 = torch.tensor([0.25, 0.25, 0.25, 0.05, 0.05, 0.05, 0.04, 0.03, 0.02, 0.01], **f64).repeat(P, 1)
    bd = _lib.BacktestDesc(P, N, steps, 1e-3)
    md = _lib.MvDesc()
    md.N, md.H, md.gamma, md.cost_coeff = N, 1, 1.0, 1e-3

    def launch(k, n, w, value, hist, target, st, obj):
        _lib.check(L.kmpc_markowitz_run_cap(ctypes.byref(bd), ctypes.byref(md), u, tau, k, n, mu[k].data_ptr(),
                                            sigma[k].data_ptr(), valid[k].data_ptr(), rt[k].data_ptr(), n, w.data_ptr(),
                                            value.data_ptr(), hist.data_ptr(), target.data_ptr(), st.data_ptr(),
                                            obj.data_ptr(), None, 0, None))

    def state():
        return (w0.clone(), torch.full((P,), 1e4, **f64), torch.zeros((P, steps, 4), **f64), torch.empty((P, N), **f64),
                torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P,), **f64))

    w, value, hist, target, st, obj = state()
    seen = {0: 0, 2: 0}
    for k in range(steps):
        before = w.cpu().numpy()
        launch(k, 1, w, value, hist, target, st, obj)
        tg, sk, ok = target.cpu().numpy(), st.cpu().numpy(), obj.cpu().numpy()
        for p in range(P):
            d0 = ref.cap_distance(before[p], u)
            assert sk[p] in (0, 2), (k, p, sk[p])
            seen[int(sk[p])] += 1
            if sk[p] == 2:
                assert d0 > tau and np.array_equal(tg[p], before[p]) and np.isnan(ok[p])
                assert float(hist[p, k, 2]) == 0.0 and float(hist[p, k, 3]) == 0.0
            else:
                assert d0 <= tau and not ref.violated(tg[p][None], before[p], tau, u)
    print(f"statuses over {steps} steps of {P} paths: {seen}")
    assert seen[0] >= 3 and seen[2] >= 3
    assert bool(torch.isfinite(hist).all()) and bool((hist[:, :, 0] > 0).all())
    w1, value1, hist1, target1, st1, obj1 = state()
    launch(0, steps, w1, value1, hist1, target1, st1, obj1)               # every step in one launch
    assert torch.equal(hist1, hist) and torch.equal(w1, w) and torch.equal(value1, value)
    w2, value2, hist2, target2, st2, obj2 = state()
    launch(0, 4, w2, value2, hist2, target2, st2, obj2)                   # split into two launches
    launch(4, steps - 4, w2, value2, hist2, target2, st2, obj2)
    assert torch.equal(hist2, hist) and torch.equal(w2, w)


@pytest.mark.parametrize("N", [10, 129])     # LDS / workspace
def test_sweep_rows_equal_single_runs_and_a_bad_cap_holds_alone(N):
    P, steps = 2, 8
    z, mean, std, realized = panel(N, P, steps)
    cfg = BacktestConfig(horizon=HZ)
    g, c = [1.0, 5.0, 0.5, 1.0, 1.0], [1e-3, 1e-2, 0.0, 1e-3, 1e-3]
    caps = [0.2, 0.05, 0.5, float("nan"), 0.0]
    sw = run_markowitz_sweep(capped(N), z, realized, cfg, mean, std, g, c, n_rows=steps + HZ, max_turnovers=caps)
    assert sw["return"].shape == (5, P, steps)
    for j in range(3):
        one = run_markowitz_lockstep(capped(N, 1, caps[j], 0.0, g[j], c[j]), z, realized, cfg, mean, std, n_rows=steps + HZ)
        assert_config_rows(sw, j, one, "capped sweep")
        assert float(sw["turnover"][j].max()) <= caps[j] + ref.cap_bar(N)
        assert sw["status"][j].tolist() == [0] * P
    for j in (3, 4):                                                       # not finite / not > 0: solver error, hold
        assert bool((sw["turnover"][j] == 0).all()) and sw["status"][j].tolist() == [4] * P
        assert bool(torch.isfinite(sw["portfolio_value"][j]).all())
    # the default: the strategy's cap for every config
    dflt = run_markowitz_sweep(capped(N, 1, 0.05), z, realized, cfg, mean, std, g[:2], c[:2], n_rows=steps + HZ)
    one = run_markowitz_lockstep(capped(N, 1, 0.05, 0.0, g[1], c[1]), z, realized, cfg, mean, std, n_rows=steps + HZ)
    assert_config_rows(dflt, 1, one, "the strategy's cap")


def test_sweep_backtest_markowitz_frames():
    """The env-level sweep with strategies that differ in max_turnover: frames equal to
    run_markowitz_sweep's columns bit for bit and to run_backtest per strategy at the lock-step vs
    sequential tolerances; capped and uncapped strategies do not mix."""
    z, mean, std, realized, T = golden_paths(1)
    env = _Env(z[0], mean, std)
    cfg = BacktestConfig(horizon=HZ)
    strats = [MarkowitzStrategy(1.0, 1e-3, max_turnover=0.2), MarkowitzStrategy(5.0, 1e-2, max_turnover=0.05),
              MarkowitzStrategy(0.5, 0.0, max_turnover=0.5)]
    frames = sweep_backtest_markowitz(env, cfg, strats)
    sw = run_markowitz_sweep(strats[0], z[:1], realized[:1], cfg, mean, std, [s.risk_aversion for s in strats],
                             [s.cost_coeff for s in strats], n_rows=T + HZ, max_turnovers=[s.max_turnover for s in strats])
    assert len(frames) == 3
    for j, df in enumerate(frames):
        assert list(df.columns) == ["date", "portfolio_value", "return", "turnover", "cost"] and len(df) == 12
        for k in COLS:
            assert np.array_equal(df[k].values, sw[k][j, 0].cpu().numpy()), (j, k)
        assert df["turnover"].values.max() <= strats[j].max_turnover + ref.cap_bar(10)
        seq = run_backtest(strats[j], env, cfg, verbose=False)
        close_to({k: df[k].values[None] for k in COLS}, 0, {k: seq[k].values for k in COLS}, f"run_backtest, strategy {j}")
    with pytest.raises(ValueError):
        sweep_backtest_markowitz(env, cfg, [strats[0], MarkowitzStrategy(1.0, 1e-3)])
