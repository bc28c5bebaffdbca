"""Dev probe: the Markowitz device backtest under the turnover cap (kmpc_markowitz_run_cap) against
the uncapped one (kmpc_markowitz_run) on the same moments, and — with --other LIB, a libkmpc.so built
from another commit — this tree's kmpc_markowitz_run against that library's. The C call alone between
device events, the state (weights, value, history) reset before every call, the two sides
alternated, median (and range) of 5 after a warm-up of each. Iterations per solve come from the
per-step loop (kmpc_solve_mv_ws / kmpc_solve_mv_cap with the iteration output, kmpc_backtest_step).
python tools/mv_cap_probe.py [--other path/to/libkmpc.so]"""
import argparse
import ctypes
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, _lib, solve_mpc_mean_variance_batched

dev = torch.device("cuda", 0)
REPS, P, STEPS, TAU = 5, 64, 40, 0.2
f64 = dict(dtype=torch.float64, device=dev)


def inputs(N):
    """STEPS steps (test rows 5 .. 5 + STEPS - 1) of P seeded panels: the moments and the realized rows."""
    rng = np.random.default_rng(N)
    T = STEPS + 6
    z = rng.normal(0, 1, (P, T, N)).astype(np.float32)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    L = _lib.load()
    zt, m, sd = torch.tensor(z, device=dev), torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    ts = torch.arange(5, 5 + STEPS, dtype=torch.int32, device=dev)
    mu, sigma = torch.empty((STEPS, P, N), **f64), torch.empty((STEPS, P, N, N), **f64)
    valid = torch.empty((STEPS, P), dtype=torch.int32, device=dev)
    _lib.check(L.kmpc_rolling_moments_paths(P, STEPS, T, N, 60, zt.data_ptr(), N, m.data_ptr(), sd.data_ptr(), ts.data_ptr(),
                                            mu.data_ptr(), sigma.data_ptr(), valid.data_ptr(), None))
    rt = torch.tensor(z * std + mean, device=dev).transpose(0, 1)[6:6 + STEPS].contiguous()
    return mu, sigma, valid, rt


def runner(L, N, mu, sigma, valid, rt, tau):
    """One call of kmpc_markowitz_run (tau = 0) or kmpc_markowitz_run_cap of library L over all steps."""
    bd = _lib.BacktestDesc(P, N, STEPS, 1e-3)
    md = _lib.MvDesc()
    md.B, md.N, md.H, md.gamma, md.cost_coeff = P, N, 1, 1.0, 1e-3
    query = L.kmpc_mv_cap_workspace_bytes if tau else L.kmpc_mv_workspace_bytes
    query.restype, query.argtypes = ctypes.c_size_t, [ctypes.POINTER(_lib.MvDesc)]
    nws = int(query(ctypes.byref(md)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
    w, value, hist = torch.empty((P, N), **f64), torch.empty((P,), **f64), torch.empty((P, STEPS, 4), **f64)
    target, obj = torch.empty((P, N), **f64), torch.empty((P,), **f64)
    st = torch.empty((P,), dtype=torch.int32, device=dev)
    name = "kmpc_markowitz_run_cap" if tau else "kmpc_markowitz_run"
    fn = getattr(L, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    head = (ctypes.byref(bd), ctypes.byref(md), 0.0) + ((tau,) if tau else ())

    def call():
        w.fill_(1.0 / N)
        value.fill_(1e4)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*head, 0, STEPS, mu.data_ptr(), sigma.data_ptr(), valid.data_ptr(), rt.data_ptr(), STEPS, w.data_ptr(),
                value.data_ptr(), hist.data_ptr(), target.data_ptr(), st.data_ptr(), obj.data_ptr(), ws.data_ptr(), nws, None)
        b.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return a.elapsed_time(b), hist.clone()
    return call


def loop_iterations(N, mu, sigma, rt, tau):
    """Mean iterations per solve over the per-step loop, and its history for the bit-identity check."""
    L = _lib.load()
    cfg = MPCConfig(horizon=1, gamma=1.0, cost_coeff=1e-3, mv_max_turnover=tau)
    bd = _lib.BacktestDesc(P, N, STEPS, 1e-3)
    w, value, hist = torch.full((P, N), 1.0 / N, **f64), torch.full((P,), 1e4, **f64), torch.empty((P, STEPS, 4), **f64)
    its, bad = [], 0
    for k in range(STEPS):
        W0, st, _, it = solve_mpc_mean_variance_batched(w, mu[k].unsqueeze(1).contiguous(), sigma[k], cfg, with_iters=True)
        its.append(it.float().mean().item())
        bad += int((st != 0).sum().item())
        _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), k, W0.data_ptr(), rt[k].data_ptr(), w.data_ptr(), value.data_ptr(),
                                        hist.data_ptr(), None))
    torch.cuda.synchronize()
    return float(np.mean(its)), bad, hist


def alternate(a, b):
    a(), b()
    ta, tb = [], []
    for _ in range(REPS):
        t, ha = a()
        ta.append(t)
        t, hb = b()
        tb.append(t)
    return ta, tb, ha, hb


def cell(t):
    return f"{np.median(t) / STEPS:.3f} ({min(t) / STEPS:.3f} - {max(t) / STEPS:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="a libkmpc.so of another commit: its kmpc_markowitz_run against this tree's")
    args = ap.parse_args()
    L = _lib.load()
    print(f"P = {P} paths, {STEPS} steps, H = 1, gamma = 1, c = 1e-3, tau = {TAU}; ms per step: median (min - max) of {REPS}")
    print("| N | uncapped ms / step | iterations / solve | capped ms / step | iterations / solve | capped / uncapped | "
          "per iteration | non-optimal solves | largest turnover | persistent == loop |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for N in (100, 30):
        mu, sigma, valid, rt = inputs(N)
        tp, tc, hp, hc = alternate(runner(L, N, mu, sigma, valid, rt, 0.0), runner(L, N, mu, sigma, valid, rt, TAU))
        ip, bp, lp = loop_iterations(N, mu, sigma, rt, 0.0)
        ic, bc, lc = loop_iterations(N, mu, sigma, rt, TAU)
        mp, mc = float(np.median(tp)), float(np.median(tc))
        print(f"| {N} | {cell(tp)} | {ip:.2f} | {cell(tc)} | {ic:.2f} | {mc / mp:.3f} | {(mc / ic) / (mp / ip):.3f} | "
              f"{bp} / {bc} | {hp[..., 2].max().item():.3f} / {hc[..., 2].max().item():.9f} | "
              f"{torch.equal(hp, lp)} / {torch.equal(hc, lc)} |", flush=True)
    if args.other:
        O = ctypes.CDLL(args.other)
        print(f"\nkmpc_markowitz_run (uncapped), this tree against {os.path.basename(os.path.dirname(args.other)) or 'the other library'}")
        print("| N | other ms / step | this tree ms / step | this / other | same history |")
        print("|---|---|---|---|---|")
        for N in (100, 30):
            mu, sigma, valid, rt = inputs(N)
            to, tt, ho, ht = alternate(runner(O, N, mu, sigma, valid, rt, 0.0), runner(L, N, mu, sigma, valid, rt, 0.0))
            print(f"| {N} | {cell(to)} | {cell(tt)} | {np.median(tt) / np.median(to):.3f} | {torch.equal(ho, ht)} |", flush=True)


if __name__ == "__main__":
    main()
