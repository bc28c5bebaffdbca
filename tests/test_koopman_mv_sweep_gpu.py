"""The sweep of the mean-variance Koopman-MPC backtest on the device: kmpc_koopman_mv_sweep (C configs
over shared forecasts and covariances, one workgroup per (config, path)) against the run it repeats,
kmpc_koopman_mv_run, bit for bit — they run the same item loop and the same window body.

Model, panel and mock env are tests/test_koopman_mv_gpu.py's (path 0 of the panel carries the jump in
asset 0 after step 0 and its reversal after step 5, which makes limit + cap steps infeasible). Shapes
(N, H): (4, 3) LDS with n < 64, one partial wave; (10, 5) LDS; (61, 2) LDS without the cap, the slab with
it; (62, 2) the first slab shape; (100, 10) the headline shape on the slab (P = 2, 6 steps). The storage
side of every shape is asserted through kmpc_mv_band_workspace_bytes. Ten steps from t = 0 elsewhere: the
first four have fewer than 5 rows and hold. The lock-step run of a config is computed once per
(shape, config) and shared by the tests.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_koopman_mv_gpu as base
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, KoopmanMVStrategy, MPCConfig, _lib, run_backtest,
                                                   run_koopman_mv_lockstep, run_koopman_mv_sweep,
                                                   sweep_backtest_koopman_mv)
from koopman_mpc_portfolio_rebalancing_amd import baselines

pytestmark = pytest.mark.gpu
DEV = base.DEV
HZ = base.HZ
OPTIMAL, INFEASIBLE, SOLVER_ERROR = 0, 2, 4
NAN = float("nan")

#              N,  H, P, steps, slab without the cap, slab with it
SHAPES = [(4, 3, 2, 10, False, False), (10, 5, 2, 10, False, False), (61, 2, 2, 10, False, True),
          (62, 2, 2, 10, True, True), (100, 10, 2, 6, True, True)]
IDS = [f"N{s[0]}_H{s[1]}" for s in SHAPES]


def storage(N, H, B):
    """(slab without the cap, slab with it) of the band kernels for B windows of [H, N]."""
    d = _lib.MvDesc()
    d.B, d.N, d.H = B, N, H
    q = _lib.load().kmpc_mv_band_workspace_bytes
    return int(q(ctypes.byref(d), 0)) > 0, int(q(ctypes.byref(d), 1)) > 0


def cfg_of(H, gamma, cost, u=0.0, tau=0.0):
    return MPCConfig(horizon=H, gamma=gamma, cost_coeff=cost, max_weight=u, mv_max_turnover=tau)


@functools.lru_cache(maxsize=None)
def lockstep(N, H, P, steps, gamma, cost, u, tau, btc, freq=1):
    """run_koopman_mv_lockstep of one config on the panel: the reference of every sweep row."""
    z, mean, std, realized = base.panel(N, P, steps)
    bt = BacktestConfig(horizon=HZ, cost_coeff=btc, rebalance_freq=freq)
    s = KoopmanMVStrategy(base.model(N), cfg_of(H, gamma, cost, u, tau))
    return run_koopman_mv_lockstep(s, z, realized, bt, mean, std, n_rows=steps + HZ)


def sweep(N, H, P, steps, rows, freq=1):
    """run_koopman_mv_sweep of the configs rows = [(gamma, cost, u, tau, bt cost)]."""
    z, mean, std, realized = base.panel(N, P, steps)
    bt = BacktestConfig(horizon=HZ, rebalance_freq=freq)
    s = KoopmanMVStrategy(base.model(N), cfg_of(H, 1.0, 1e-3))
    return run_koopman_mv_sweep(s, z, realized, bt, mean, std, [cfg_of(H, *r[:4]) for r in rows],
                                bt_cost_coeffs=[r[4] for r in rows], n_rows=steps + HZ)


def assert_rows(out, N, H, P, steps, rows, what, freq=1):
    """Config j of the sweep equals the lock-step run of config j: every history column, the weights
    and the metrics, bit for bit."""
    assert out["return"].shape[:2] == (len(rows), P) and out["status"].shape == (len(rows), P)
    for j, r in enumerate(rows):
        one = lockstep(N, H, P, steps, *r, freq)
        for k in base.COLS + ("weights",):
            assert torch.equal(out[k][j], one[k]), (what, j, k)
        for k, v in one["metrics"].items():
            assert torch.equal(out["metrics"][k][j], v), (what, j, k)


def two_chunks(monkeypatch, P, N, steps):
    """The byte cap of the covariance buffer at half the steps, as tests/test_koopman_mv_gpu.py does."""
    half = (steps + 1) // 2
    monkeypatch.setattr(baselines, "MARKOWITZ_SIGMA_BYTES", half * P * N * N * 8)
    assert baselines._markowitz_chunk(P, N) == half


def limits(N):
    """Two active limits for N assets, the tighter one tests/test_koopman_mv_gpu.py's."""
    return base.limit_for(N), min(0.95, 4.0 / N)


@pytest.mark.parametrize("N,H,P,steps,slab,slab_cap", SHAPES, ids=IDS)
def test_sweep_equals_the_runs_without_constraints(N, H, P, steps, slab, slab_cap, monkeypatch):
    """(a) gamma, the solve's cost and the bookkeeping's cost vary; no limit, no cap: one launch per chunk."""
    rows = [(0.5, 1e-3, 0.0, 0.0, 1e-3), (2.0, 5e-4, 0.0, 0.0, 2e-3), (10.0, 0.0, 0.0, 0.0, 0.0)]
    assert storage(N, H, len(rows) * P) == (slab, slab_cap)
    out = sweep(N, H, P, steps, rows)
    assert_rows(out, N, H, P, steps, rows, "one chunk")
    assert bool((out["status"] == OPTIMAL).all())
    assert not torch.equal(out["weights"][0], out["weights"][1])            # (the configs do differ)
    two_chunks(monkeypatch, P, N, steps)                                    # (c) ... and through step0
    assert_rows(sweep(N, H, P, steps, rows), N, H, P, steps, rows, "two chunks")


@pytest.mark.parametrize("N,H,P,steps,slab,slab_cap", SHAPES, ids=IDS)
def test_sweep_equals_the_runs_with_the_four_groups_mixed(N, H, P, steps, slab, slab_cap, monkeypatch):
    """(b) all four (limit, cap) groups in one call, interleaved, with a different limit and cap per config
    inside a group: four launches per chunk over the same forecasts and covariances, scattered back. At
    (100, 10) one config per group, elsewhere two in the limit + cap group and two in the cap group."""
    u0, u1 = limits(N)
    rows = [(1.0, 1e-3, u0, base.TAU, 1e-3), (0.5, 1e-3, 0.0, 0.0, 1e-3), (2.0, 5e-4, u1, 0.0, 2e-3),
            (1.0, 0.0, 0.0, 0.3, 0.0)]
    if N < 100:
        rows += [(3.0, 1e-3, u1, 0.4, 1e-3), (1.0, 2e-3, 1.5, base.TAU, 1e-3)]   # (u >= 1: no limit, the cap group)
    assert storage(N, H, 2 * P) == (slab, slab_cap)
    out = sweep(N, H, P, steps, rows)
    assert_rows(out, N, H, P, steps, rows, "one chunk")
    # the jump path under the tight limit and cap ends infeasible where the run stops before the reversal
    assert int(out["status"][0, 0]) == (INFEASIBLE if steps <= 6 else OPTIMAL)
    assert bool((out["turnover"][0, 0, 4:6] == 0).all()) and bool((out["turnover"][1, 0, 4:6] > 0).all())
    two_chunks(monkeypatch, P, N, steps)                                    # (c)
    assert_rows(sweep(N, H, P, steps, rows), N, H, P, steps, rows, "two chunks")


def test_more_items_than_slots():
    """(62, 2) on the slab with C = 9, P = 58: 522 work items on 512 workgroups, so ten workgroups walk on
    to a second item (q += gridDim.x) whose config is q / P = 8. All nine configs in the limit + cap group
    (one launch), each with its own five parameters. Three steps, t = 0, 4, 8: the last two are solved."""
    N, H, P, C, T, freq = 62, 2, 58, 9, 9, 4
    u0, u1 = limits(N)
    rows = [(0.5 + 0.5 * j, 1e-3 * (j % 3), u0 if j % 2 else u1, 0.05 + 0.05 * j, 5e-4 * (j % 4)) for j in range(C)]
    assert C * P > 512 and storage(N, H, C * P) == (True, True)
    out = sweep(N, H, P, T, rows, freq)
    assert out["return"].shape == (C, P, 3)
    assert_rows(out, N, H, P, T, rows, "522 items", freq)
    assert bool((out["turnover"][:, :, 0] == 0).all()) and bool((out["turnover"][:, 1:, 1:] > 0).all())


def test_configs_are_separate_under_limit_and_cap():
    """Two configs on the jump panel that differ in the cap alone. Under the tight one path 0 starts the
    steps between the jump and its reversal further above the limit than the cap allows back: infeasible,
    hold. Under the loose one the same steps trade."""
    N, H, P = 10, 5, 2
    u = base.limit_for(N)
    rows = [(1.0, 1e-3, u, base.TAU, 1e-3), (1.0, 1e-3, u, 1.0, 1e-3)]
    out = sweep(N, H, P, 10, rows)
    assert_rows(out, N, H, P, 10, rows, "ten steps")
    tight, loose = out["turnover"][0], out["turnover"][1]
    assert bool((tight[0, 4:6] == 0).all()) and bool((tight[0, 6:] > 0).all()) and bool((tight[1, 4:] > 0).all())
    assert bool((loose[:, 4:] > 0).all())
    assert float(tight.max()) <= base.TAU + base.ref.cap_bar(N) and float(loose[0, 4]) > base.TAU
    short = sweep(N, H, P, 6, rows)                                          # ... stopped before the reversal
    assert_rows(short, N, H, P, 6, rows, "six steps")
    assert short["status"].tolist() == [[INFEASIBLE, OPTIMAL], [OPTIMAL, OPTIMAL]]


# ---- the device-side guards, through the C ABI (Python rejects these values) -------------------------

class _Chunk:
    """One chunk of N = 10, H = 5, P = 2, eight steps from t = 0: forecasts, covariances, valid and the
    realized rows on the device, as run_koopman_mv_lockstep prepares them."""
    N, H, P, S = 10, 5, 2, 8

    def __init__(self):
        N, H, P, S = self.N, self.H, self.P, self.S
        L = _lib.load()
        z, mean, std, realized = base.panel(N, P, S)
        zt = torch.tensor(z, device=DEV)
        self.y = base.model(N).rollout(zt.transpose(0, 1).reshape(S * P, -1), mean, std, H, N).contiguous()
        m, sd = torch.tensor(mean, device=DEV), torch.tensor(std, device=DEV)
        ts = torch.arange(S, dtype=torch.int32, device=DEV)
        mu = torch.empty((S, P, N), dtype=torch.float64, device=DEV)
        self.sigma = torch.empty((S, P, N, N), dtype=torch.float64, device=DEV)
        self.valid = torch.empty((S, P), dtype=torch.int32, device=DEV)
        _lib.check(L.kmpc_rolling_moments_paths(P, S, S, N, 60, zt.data_ptr(), 2 * N, m.data_ptr(), sd.data_ptr(),
                                                ts.data_ptr(), mu.data_ptr(), self.sigma.data_ptr(),
                                                self.valid.data_ptr(), _lib.stream_handle(DEV)))
        self.rr = torch.tensor(realized, device=DEV).transpose(0, 1)[1:S].contiguous()   # step t realizes row t + 1
        self.md = _lib.MvDesc()
        self.md.B, self.md.N, self.md.H, self.md.gamma, self.md.cost_coeff = 0, N, H, NAN, NAN   # (the sweep reads neither)
        self.md.max_iter, self.md.tol = 100, 1e-10

    def state(self, items):
        f64 = dict(dtype=torch.float64, device=DEV)
        N, S = self.N, self.S
        return dict(weights=torch.full((items, N), 1.0 / N, **f64), value=torch.full((items,), 1e4, **f64),
                    hist=torch.zeros((items, S, 4), **f64), target=torch.zeros((items, N), **f64),
                    status=torch.full((items,), -1, dtype=torch.int32, device=DEV), obj=torch.zeros((items,), **f64))

    def _tail(self, s):
        return (0, self.S, self.y.data_ptr(), self.sigma.data_ptr(), self.valid.data_ptr(), self.rr.data_ptr(),
                self.S - 1, s["weights"].data_ptr(), s["value"].data_ptr(), s["hist"].data_ptr(), s["target"].data_ptr(),
                s["status"].data_ptr(), s["obj"].data_ptr(), None, 0, _lib.stream_handle(DEV))

    def sweep(self, gamma, cost, btc, limit=None, cap=None):
        """kmpc_koopman_mv_sweep of the configs' lists (limit / cap None: a NULL array) -> rows [C, P, ...]."""
        C, P = len(gamma), self.P
        dev = lambda v: None if v is None else torch.tensor(v, dtype=torch.float64, device=DEV)
        par = [dev(v) for v in (gamma, cost, btc, limit, cap)]
        s = self.state(C * P)
        bd = _lib.BacktestDesc(P, self.N, self.S, NAN)
        _lib.check(_lib.load().kmpc_koopman_mv_sweep(ctypes.byref(bd), ctypes.byref(self.md), C,
                                                     *(None if t is None else t.data_ptr() for t in par), *self._tail(s)))
        torch.cuda.synchronize()
        return {k: v.reshape(C, P, *v.shape[1:]) for k, v in s.items()}

    def run(self, gamma, cost, btc, u=0.0, tau=0.0):
        """kmpc_koopman_mv_run of one config's five scalars -> rows [P, ...]."""
        md = _lib.MvDesc()
        md.B, md.N, md.H, md.gamma, md.cost_coeff, md.max_iter, md.tol = 0, self.N, self.H, gamma, cost, 100, 1e-10
        s = self.state(self.P)
        bd = _lib.BacktestDesc(self.P, self.N, self.S, btc)
        _lib.check(_lib.load().kmpc_koopman_mv_run(ctypes.byref(bd), ctypes.byref(md), u, tau, *self._tail(s)))
        torch.cuda.synchronize()
        return s


@functools.lru_cache(maxsize=None)
def chunk():
    return _Chunk()


def assert_guarded(ck, out, good, bad, scalars):
    """The bad configs hold at every step (turnover 0: the target is the current weights; cost 0) and end
    KMPC_STATUS_SOLVER_ERROR; the good ones equal kmpc_koopman_mv_run with their scalars, every array."""
    valid = ck.valid.cpu().numpy().astype(bool)
    assert not valid[:4].any() and valid[4:].all()                          # (the last step is a solved one)
    for j in bad:
        assert out["status"][j].tolist() == [SOLVER_ERROR] * ck.P, j
        assert bool((out["hist"][j, :, :, 2:] == 0).all()), j
        assert bool((out["hist"][j, :, :-1, 0] != 1e4).all())               # (the path still moves with the market)
    for j in good:
        one = ck.run(*scalars(j))
        assert one["status"].tolist() == [OPTIMAL] * ck.P
        for k, v in one.items():
            assert torch.equal(out[k][j], v), (j, k)
        assert bool((out["hist"][j, :, 4:, 2] > 0).all()), j


def test_device_guards_on_gamma_and_cost():
    ck = chunk()
    gamma, cost, btc = [1.0, -1.0, 3.0, 1.0, NAN, 1.0], [1e-3, 1e-3, 0.0, NAN, 1e-3, -1e-3], [1e-3, 1e-3, 2e-3, 1e-3, 1e-3, 1e-3]
    out = ck.sweep(gamma, cost, btc)
    assert_guarded(ck, out, [0, 2], [1, 3, 4, 5], lambda j: (gamma[j], cost[j], btc[j]))


def test_device_guards_on_the_cap():
    ck = chunk()
    cap = [0.05, 0.0, 0.5, NAN, -0.1]
    gamma, cost, btc = [1.0] * 5, [1e-3] * 5, [1e-3] * 5
    out = ck.sweep(gamma, cost, btc, cap=cap)
    assert_guarded(ck, out, [0, 2], [1, 3, 4], lambda j: (1.0, 1e-3, 1e-3, 0.0, cap[j]))


def test_device_guards_on_the_limit():
    """N * u <= 1, u >= 1 and a non-finite u never reach the window's start point (which assumes
    1 / N < u < 1): the config holds; its neighbours run under their own limits."""
    ck = chunk()
    N = ck.N
    limit = [0.25, 1.0 / N, 1.0, NAN, 0.5, float("inf"), 0.05, -0.25]
    C = len(limit)
    gamma, cost, btc = [1.0] * C, [1e-3] * C, [1e-3] * C
    out = ck.sweep(gamma, cost, btc, limit=limit)
    assert_guarded(ck, out, [0, 4], [1, 2, 3, 5, 6, 7], lambda j: (1.0, 1e-3, 1e-3, limit[j], 0.0))
    assert float(out["target"][0].max()) <= 0.25 and float(out["target"][4].max()) <= 0.5
    # ... and in the limit + cap form (a cap wide enough for the jump path to come back under 0.25)
    both = ck.sweep(gamma, cost, btc, limit=limit, cap=[1.0] * C)
    assert_guarded(ck, both, [0, 4], [1, 2, 3, 5, 6, 7], lambda j: (1.0, 1e-3, 1e-3, limit[j], 1.0))


# ---- the env-level call ------------------------------------------------------------------------------

class _Env(base._Env):
    """... whose de-standardisation also takes the rollout's device tensor (the env without stats)."""

    def destandardize_returns(self, r):
        r = torch.as_tensor(r)
        return r * torch.tensor(self.std, device=r.device) + torch.tensor(self.mean, device=r.device)


def _env_case():
    N, H, steps = 10, 5, 10
    z, mean, std, realized = base.panel(N, 1, steps)
    env = _Env(z[0], mean, std, realized[0])          # (the env realizes its own current returns: no jump)
    u = base.limit_for(N)
    cfgs = [cfg_of(H, 1.0, 1e-3), cfg_of(H, 4.0, 5e-4, u, base.TAU), cfg_of(H, 0.5, 1e-3, 0.0, 0.2)]
    return env, cfgs, steps, BacktestConfig(horizon=HZ)


def test_sweep_backtest_equals_run_backtest():
    env, cfgs, steps, bt = _env_case()
    km = base.model(10)
    dfs = sweep_backtest_koopman_mv(KoopmanMVStrategy(km, cfgs[0]), env, bt, cfgs)
    assert len(dfs) == len(cfgs)
    for j, (df, c) in enumerate(zip(dfs, cfgs)):
        one = run_backtest(KoopmanMVStrategy(km, c), env, bt, verbose=False)
        assert list(df.columns) == list(one.columns) == ["date", "portfolio_value", "return", "turnover", "cost"]
        assert len(df) == len(one) == steps and list(df["date"]) == list(one["date"])
        # the tolerances of tests/test_koopman_mv_gpu.py for the lock-step run against run_backtest
        for k, kw in (("portfolio_value", dict(rtol=1e-6)), ("return", dict(rtol=0, atol=3e-7)),
                      ("turnover", dict(rtol=1e-6, atol=1e-6)), ("cost", dict(rtol=1e-6, atol=1e-6))):
            print(f"config {j} {k}: max abs difference {np.abs(df[k].values - one[k].values).max():.3e}")
            np.testing.assert_allclose(df[k].values, one[k].values, **kw)
    assert not np.allclose(dfs[0]["turnover"].values, dfs[1]["turnover"].values)


def test_sweep_backtest_without_stats_falls_back(monkeypatch):
    env, cfgs, steps, bt = _env_case()
    env.stats = None

    def no_sweep(*a, **kw):
        raise AssertionError("an env without stats runs run_backtest per config")
    monkeypatch.setattr(baselines, "run_koopman_mv_sweep", no_sweep)
    km = base.model(10)
    dfs = sweep_backtest_koopman_mv(KoopmanMVStrategy(km, cfgs[0]), env, bt, cfgs[:2])
    for df, c in zip(dfs, cfgs[:2]):
        one = run_backtest(KoopmanMVStrategy(km, c), env, bt, verbose=False)
        assert len(df) == steps and df.equals(one)
