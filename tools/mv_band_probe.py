"""Dev probe: the band form of the mean-variance solve (kmpc_solve_mv_band) against the dense kernel
(kmpc_solve_mv_ws) on the same windows — float32-representable forecasts, shared over both — and the
mean-variance Koopman-MPC backtest in its persistent form (kmpc_koopman_mv_run) against the per-step
loop. One process; the C call alone between device events, the two sides alternated, median (and
range) of 3 after a warm-up of each. Per iteration: the time of a batch over the mean iteration count
of its windows (the counts of the two forms are printed and must agree to within 1 per window).
python tools/mv_band_probe.py [--skip-backtest]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, DeviceKoopman, KoopmanModelSpec, KoopmanMVStrategy,
                                                   MPCConfig, _lib, run_koopman_mv_lockstep)

dev = torch.device("cuda", 0)
REPS = 3
f64 = dict(dtype=torch.float64, device=dev)
SHAPES = [(10, 5, 4096), (30, 5, 4096), (100, 10, 64), (100, 10, 512), (64, 16, 64), (100, 1, 4096)]


def inputs(N, H, B):
    """B windows: 64 seeded ones, repeated."""
    rng = np.random.default_rng(1000 * N + H)
    B, reps = min(B, 64), max(1, B // 64)
    y = rng.normal(5e-4, 0.01, (B, H, N)).astype(np.float32)
    F = rng.normal(0, 0.01, (B, N + 5, N))
    S = np.einsum("bki,bkj->bij", F, F) / (N + 5) + 1e-6 * np.eye(N)
    wp = rng.dirichlet(np.ones(N), B)
    return tuple(torch.tensor(np.tile(a, (reps,) + (1,) * (a.ndim - 1)), device=dev) for a in (y, S, wp))


def runner(band, N, H, B, y, S, wp):
    L = _lib.load()
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff, d.max_iter, d.tol = B, N, H, 1.0, 1e-3, 100, 1e-10
    nws = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(d), 0) if band else L.kmpc_mv_workspace_bytes(ctypes.byref(d)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
    W, obj = torch.empty((B, N), **f64), torch.empty((B,), **f64)
    st, it = torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    y64 = y.double().contiguous()

    def call():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if band:
            rc = L.kmpc_solve_mv_band(ctypes.byref(d), y.data_ptr(), S.data_ptr(), 1, wp.data_ptr(), 0.0, 0.0, W.data_ptr(),
                                      st.data_ptr(), obj.data_ptr(), it.data_ptr(), ws.data_ptr(), nws, None)
        else:
            rc = L.kmpc_solve_mv_ws(ctypes.byref(d), y64.data_ptr(), S.data_ptr(), N * N, wp.data_ptr(), W.data_ptr(),
                                    st.data_ptr(), obj.data_ptr(), it.data_ptr(), ws.data_ptr(), nws, None)
        b.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return a.elapsed_time(b), (st.clone(), it.clone(), obj.clone())
    return call


def cell(t, per):
    return f"{np.median(t) / per:.4f} ({min(t) / per:.4f} - {max(t) / per:.4f})"


def solves():
    print(f"gamma = 1, c = 1e-3, long-only, no limit, no cap; median (min - max) of {REPS}, alternating, after a warm-up of each")
    print("| N | H | B | storage (band) | dense ms / window | band ms / window | dense us / window-iteration | "
          "band us / window-iteration | band / dense | iterations dense | iterations band | largest |difference| per window | "
          "statuses equal | max |obj difference| |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for N, H, B in SHAPES:
        y, S, wp = inputs(N, H, B)
        dense, band = runner(False, N, H, B, y, S, wp), runner(True, N, H, B, y, S, wp)
        dense(), band()
        td, tb = [], []
        for _ in range(REPS):
            t, rd = dense()
            td.append(t)
            t, rb = band()
            tb.append(t)
        itd, itb = rd[1].float().mean().item(), rb[1].float().mean().item()
        md, mb = float(np.median(td)), float(np.median(tb))
        q = _lib.MvDesc()
        q.B, q.N, q.H = B, N, H
        lds = int(_lib.load().kmpc_mv_band_workspace_bytes(ctypes.byref(q), 0)) == 0
        print(f"| {N} | {H} | {B} | {'LDS' if lds else 'workspace'} | {cell(td, B)} | {cell(tb, B)} | "
              f"{1e3 * md / B / itd:.3f} | {1e3 * mb / B / itb:.3f} | {mb / md:.3f} | {itd:.2f} | {itb:.2f} | "
              f"{(rd[1] - rb[1]).abs().max().item()} | {torch.equal(rd[0], rb[0])} | {(rd[2] - rb[2]).abs().max().item():.3e} |",
              flush=True)


def model(N):
    obs, hid, Ld = 2 * N, 64, 32
    g = torch.Generator().manual_seed(N)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale
    enc = [(rnd(hid, obs, scale=obs ** -0.5), rnd(hid, scale=obs ** -0.5)), (rnd(Ld, hid, scale=hid ** -0.5), rnd(Ld, scale=hid ** -0.5))]
    q, _ = torch.linalg.qr(torch.randn(Ld, Ld, generator=g, dtype=torch.float64))
    return DeviceKoopman(KoopmanModelSpec(kind="generic", encoder=enc, kmat=(0.95 * q).float(),
                                          decoder=[(rnd(obs, Ld, scale=Ld ** -0.5), None)]), dev)


def backtests():
    P, STEPS = 64, 64
    print(f"\nrun_koopman_mv_lockstep, P = {P} paths, {STEPS + 5} steps of which the first four hold; wall clock of the call "
          f"(rollout and moments included in both), ms per step: median (min - max) of {REPS}, alternating")
    print("| N | H | persistent ms / step | per-step loop ms / step | loop / persistent | same history |")
    print("|---|---|---|---|---|---|")
    for N, H in ((10, 5), (100, 10)):
        rng = np.random.default_rng(N)
        T = STEPS + 5
        z = rng.normal(0, 1, (P, T, 2 * N)).astype(np.float32)
        mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
        realized = z[:, :, :N] * std + mean
        s = KoopmanMVStrategy(model(N), MPCConfig(horizon=H, gamma=1.0, cost_coeff=1e-3))
        bt = BacktestConfig(horizon=5)

        def run(persistent):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run_koopman_mv_lockstep(s, z, realized, bt, mean, std, n_rows=T + 5, persistent=persistent)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), out["portfolio_value"]
        run(True), run(False)
        tp, tl = [], []
        for _ in range(REPS):
            t, hp = run(True)
            tp.append(t)
            t, hl = run(False)
            tl.append(t)
        print(f"| {N} | {H} | {cell(tp, T)} | {cell(tl, T)} | {np.median(tl) / np.median(tp):.3f} | {torch.equal(hp, hl)} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-backtest", action="store_true")
    args = ap.parse_args()
    solves()
    if not args.skip_backtest:
        backtests()
