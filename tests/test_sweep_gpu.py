"""The sweep backtest (kmpc_backtest_sweep, run_backtest_sweep, sweep_backtest) on the device: C MPC
configs over shared forecasts in one launch, against the existing engine run once per config.

The sweep kernel runs the window body and the bookkeeping of the path-persistent kernel on the same
forecasts (the rollout is the same batch of P paths), with the config's parameters read from device
arrays: config j's rows are bit-identical (torch.equal) to run_backtest_lockstep(persistent=True)
with that config. The env-level frames are compared with the sequential run_backtest at the
tolerances of test_lockstep_paths_match_sequential_and_reference_runs (another rollout batch).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, KoopmanModelSpec, KoopmanMPCStrategy, MPCConfig,
                                                   calculate_metrics, run_backtest, run_backtest_lockstep,
                                                   run_backtest_sweep, sweep_backtest, _lib)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

P = 3
# (mpc_cost, max_turnover, bt_cost); the last repeats the first
CONFIGS = [(1e-3, 0.2, 1e-3), (0.0, 0.2, 0.0), (1e-2, 0.05, 1e-3), (10.0, 2.0, 1e-3), (1e-3, 0.2, 1e-3)]
KEYS = ("portfolio_value", "return", "turnover", "cost", "weights")


def _inputs(N, H):
    import bench
    dev = torch.device("cuda")
    obs_n, T = N * 20, H + 9
    spec = KoopmanModelSpec.from_state_dict(bench.make_state_dict(obs_n, 256, 1024, seed=0), bench.MODEL_CFG)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(P, T, obs_n, generator=g).to(dev)
    r = (torch.randn(P, T, N, generator=g) * 0.015 + 5e-4).to(dev)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    return spec, x, r, mean, std


def _mpc(H, path, c, tau):
    return MPCConfig(horizon=H, cost_coeff=c, max_turnover=tau, solver_path=path)


@functools.lru_cache(maxsize=None)
def _runs(N, H, path, chunk):
    """(the sweep of CONFIGS, the existing engine's run of each config); computed once per shape and
    not modified by the tests."""
    from koopman_mpc_portfolio_rebalancing_amd import backtest as bt
    spec, x, r, mean, std = _inputs(N, H)
    saved = bt.PREROLL_CHUNK
    if chunk:
        bt.PREROLL_CHUNK = chunk
    try:
        strat = KoopmanMPCStrategy(spec, _mpc(H, path, 1e-3, 0.2), device="cuda")
        sweep = run_backtest_sweep(strat, x, r, BacktestConfig(horizon=H), mean, std,
                                   [_mpc(H, path, c, tau) for c, tau, _ in CONFIGS], [b for _, _, b in CONFIGS])
        refs = [run_backtest_lockstep(KoopmanMPCStrategy(strat.device_model(), _mpc(H, path, c, tau), device="cuda"),
                                      x, r, BacktestConfig(horizon=H, cost_coeff=b), mean, std, persistent=True)
                for c, tau, b in CONFIGS]
    finally:
        bt.PREROLL_CHUNK = saved
    return sweep, refs


# 9 steps: PREROLL_CHUNK = 9 windows is 3 steps of the 3 paths per rollout, so 3 launches
@pytest.mark.parametrize("N,H,path,chunk", [
    (10, 5, 1, None), (16, 5, 1, None),      # 16-lane groups, 11 and 16 cold slots; C P = 15: a ragged
                                             # last block, different configs in one wave
    (30, 5, 1, None), (20, 10, 1, None),     # 32-lane groups
    (8, 2, 0, None),
    (10, 5, 0, None),                        # one per wave under AUTO
    (50, 10, 0, None),                       # 64 threads
    (100, 5, 0, None),                       # 128 threads
    (150, 10, 0, None),                      # 256 threads, LDL^T arrays in LDS
    (200, 5, 0, None),                       # 256 threads
    (120, 10, 0, None), (230, 10, 0, None),  # H = 10 past the LDS-array strides: plain 128 and 256 threads
    (100, 10, 0, None),                      # the C3 unit
    (10, 5, 1, 9), (100, 10, 0, 9)])         # several launches, each resuming the state
def test_sweep_equals_existing_engine_per_config(N, H, path, chunk):
    sweep, refs = _runs(N, H, path, chunk)
    C = len(CONFIGS)
    assert sweep["in_kernel"].tolist() == [True] * C      # (no fallback hiding a kernel failure)
    assert sweep["return"].shape == (C, P, 9) and sweep["weights"].shape == (C, P, N)
    for j, ref in enumerate(refs):
        for k in KEYS:
            assert torch.equal(sweep[k][j], ref[k]), (j, k)
        for name, v in ref["metrics"].items():
            assert sweep["metrics"][name].shape == (C, P)
            assert torch.equal(sweep["metrics"][name][j], v), (j, name)
    for k in KEYS:                                         # the repeated config
        assert torch.equal(sweep[k][4], sweep[k][0]), k
    for name in sweep["metrics"]:
        assert torch.equal(sweep["metrics"][name][4], sweep["metrics"][name][0]), name
    # a cost of 10 per unit of turnover: the config holds
    assert sweep["turnover"][3][:, 1:].max().item() <= 1e-6
    # the configs do differ (a sweep that ignored its parameters would still pass the above only if
    # the references did too)
    assert not torch.equal(sweep["portfolio_value"][0], sweep["portfolio_value"][2])


def test_sweep_fallback_for_configs_outside_the_kernel_case():
    """max_turnover = 0 is another constraint case (no cap): that config runs as its own
    run_backtest_lockstep call and is reported in_kernel = False; the others are unchanged."""
    N, H, path = 10, 5, 1
    sweep, _ = _runs(N, H, path, None)
    spec, x, r, mean, std = _inputs(N, H)
    strat = KoopmanMPCStrategy(spec, _mpc(H, path, 1e-3, 0.2), device="cuda")
    cfgs = [_mpc(H, path, c, tau) for c, tau, _ in CONFIGS]
    btc = [b for _, _, b in CONFIGS]
    cfgs.insert(2, _mpc(H, path, 1e-3, 0.0))
    btc.insert(2, 2e-3)
    out = run_backtest_sweep(strat, x, r, BacktestConfig(horizon=H), mean, std, cfgs, btc)
    assert out["in_kernel"].tolist() == [True, True, False, True, True, True]
    own = run_backtest_lockstep(KoopmanMPCStrategy(strat.device_model(), cfgs[2], device="cuda"), x, r,
                                BacktestConfig(horizon=H, cost_coeff=2e-3), mean, std)
    keep = [0, 1, 3, 4, 5]
    for k in KEYS:
        assert torch.equal(out[k][2], own[k]), k
        assert torch.equal(out[k][keep], sweep[k]), k
    for name, v in own["metrics"].items():
        assert torch.equal(out["metrics"][name][2], v), name
        assert torch.equal(out["metrics"][name][keep], sweep["metrics"][name]), name
    assert out["turnover"][2].max().item() > 1e-3      # (no cap, cost 1e-3: it trades)


def _abi_sweep(N, H, Pn, S, y, rr, mpc_cost, tau, bt_cost):
    L = _lib.load()
    C = len(tau)
    f64 = dict(dtype=torch.float64, device="cuda")
    sd = _lib.SolveDesc()
    sd.B, sd.N, sd.H, sd.path = 0, N, H, _lib.PATH_REGISTER      # (packs at any batch size)
    d = _lib.BacktestDesc(Pn, N, S, 0.0)
    w = torch.full((C, Pn, N), 1.0 / N, **f64)
    value = torch.full((C, Pn), 1e4, **f64)
    hist = torch.zeros((C, Pn, S, 4), **f64)
    target = torch.empty((C * Pn, N), **f64)
    status = torch.full((C * Pn,), -1, dtype=torch.int32, device="cuda")
    obj = torch.empty((C * Pn,), **f64)
    pc, pt, pb = (torch.tensor(v, **f64) for v in (mpc_cost, tau, bt_cost))
    _lib.check(L.kmpc_backtest_sweep(ctypes.byref(d), ctypes.byref(sd), C, pc.data_ptr(), pt.data_ptr(), pb.data_ptr(),
                                     0, S, y.data_ptr(), rr.data_ptr(), S, w.data_ptr(), value.data_ptr(),
                                     hist.data_ptr(), target.data_ptr(), status.data_ptr(), obj.data_ptr(),
                                     _lib.stream_handle(torch.device("cuda"))))
    torch.cuda.synchronize()
    return w, value, hist, status.reshape(C, Pn)


def test_abi_config_outside_case_is_poisoned_alone():
    """kmpc_backtest_sweep with max_turnover = [0.2, 0, 0.2] (device values the host cannot check):
    config 1 ends every step solver_error with the hold fallback — no turnover, no cost, the weights
    1/N drifted by the market alone — and configs 0 and 2 equal a two-config run without it."""
    N, H, Pn, S = 10, 5, 2, 6
    g = torch.Generator().manual_seed(7)
    y = (torch.randn(S, Pn, H, N, generator=g) * 0.01).cuda().contiguous()
    rr = (torch.randn(S, Pn, N, generator=g) * 0.015 + 5e-4).cuda().contiguous()
    w, value, hist, status = _abi_sweep(N, H, Pn, S, y, rr, [1e-3, 1e-3, 2e-3], [0.2, 0.0, 0.2], [1e-3, 1e-3, 1e-3])
    assert status[1].tolist() == [4, 4]
    assert status[0].max().item() <= 1 and status[2].max().item() <= 1
    assert torch.count_nonzero(hist[1, :, :, 2]).item() == 0 and torch.count_nonzero(hist[1, :, :, 3]).item() == 0
    # buy and hold from 1/N: w <- w (1 + r) / (1 + w . r) with the float32 r = exp(y) - 1 (the
    # device evaluates numpy's float32 exp; torch's differs by an ulp of float32, 6e-8, at most: 1e-6
    # per step, 6 steps)
    r32 = torch.exp(rr) - 1.0
    g32 = (1.0 + r32).double()
    r32 = r32.double()
    wh = torch.full((Pn, N), 1.0 / N, dtype=torch.float64, device="cuda")
    vh = torch.full((Pn,), 1e4, dtype=torch.float64, device="cuda")
    for k in range(S):
        port = (wh * r32[k]).sum(-1, keepdim=True)
        wh = wh * g32[k] / (1.0 + port)
        vh = vh * (1.0 + port[:, 0])
    np.testing.assert_allclose(w[1].cpu().numpy(), wh.cpu().numpy(), rtol=1e-6)
    np.testing.assert_allclose(value[1].cpu().numpy(), vh.cpu().numpy(), rtol=1e-6)
    w2, value2, hist2, status2 = _abi_sweep(N, H, Pn, S, y, rr, [1e-3, 2e-3], [0.2, 0.2], [1e-3, 1e-3])
    for a, b in ((w, w2), (value, value2), (hist, hist2), (status, status2)):
        assert torch.equal(a[[0, 2]], b)
    assert hist[0, :, :, 2].max().item() > 1e-3          # (the healthy configs trade)


def test_sweep_backtest_on_the_golden_env():
    """sweep_backtest: the reference's single-environment call for C configs — each frame against
    the sequential run_backtest with that config, the golden config's against the reference's
    recorded run."""
    from test_backtest_cpu import GoldenEnv
    g = np.load(os.path.join(GOLD, "backtest_koopman_mpc.npz"))
    meta = json.loads(str(g["meta"]))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    spec = KoopmanModelSpec.from_state_dict(sd, meta["config"])
    env = GoldenEnv(g)
    base, bcfg = MPCConfig(**meta["mpc"]), BacktestConfig(**meta["backtest"])
    import dataclasses
    cfgs = [base, dataclasses.replace(base, cost_coeff=1e-2, max_turnover=0.05),
            dataclasses.replace(base, cost_coeff=0.0, max_turnover=0.5)]
    bts = [bcfg, dataclasses.replace(bcfg, cost_coeff=5e-3), dataclasses.replace(bcfg, cost_coeff=0.0)]
    strat = KoopmanMPCStrategy(spec, base)
    frames = sweep_backtest(strat, env, bcfg, cfgs, bts)
    assert len(frames) == 3
    np.testing.assert_allclose(frames[0]["portfolio_value"].values, g["df_value"], rtol=1e-6)
    for df, c, b in zip(frames, cfgs, bts):
        assert list(df.columns) == ["date", "portfolio_value", "return", "turnover", "cost"]
        ref = run_backtest(KoopmanMPCStrategy(strat.device_model(), c), env, b, verbose=False)
        assert list(df["date"]) == list(ref["date"])
        np.testing.assert_allclose(df["portfolio_value"].values, ref["portfolio_value"].values, rtol=1e-6)
        np.testing.assert_allclose(df["return"].values, ref["return"].values, rtol=0, atol=3e-7)
        np.testing.assert_allclose(df["turnover"].values, ref["turnover"].values, rtol=1e-6, atol=1e-6)
        m = calculate_metrics(df)
        assert set(m) == {"Sharpe Ratio", "Max Drawdown", "Avg Turnover", "Final Value", "Total Return"}
        assert np.isfinite(list(m.values())).all()
