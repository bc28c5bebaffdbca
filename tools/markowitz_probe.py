"""Dev probe (GPU): path-steps/s of the Markowitz backtest, three forms in one process:
  (a) run_markowitz_lockstep(persistent=True): every step of a path in kmpc_markowitz_run launches;
  (b) run_markowitz_lockstep(persistent=False): the per-step loop (kmpc_solve_mv_ws over the P
      windows, the hold select, kmpc_backtest_step);
  (c) run_backtest(MarkowitzStrategy) looped over paths: the sequential product path, the only
      way before the device backtest — the baseline. It is timed over the first SEQ_PATHS paths (its
      rate does not depend on how many follow one another).
Shapes: N = 10 and N = 100 at P = 64 paths, H = 1; and a sweep of C = 16 configs at P = 1:
  (a) run_markowitz_sweep, (b) 16 run_markowitz_lockstep(P = 1) calls, (c) 16 run_backtest calls.
Wall time around a device synchronise, the median of REPS runs after a warm-up of every form and
shape, the forms alternating. The three forms' histories are compared first (a against b bit for
bit, against c to 1e-6).

    python tools/markowitz_probe.py [--out profiles/markowitz_bt.md]
"""
import argparse
import os
import statistics
import sys
import time
from unittest.mock import MagicMock

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pandas as pd
import torch

from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, run_backtest, run_markowitz_lockstep,
                                                   run_markowitz_sweep)
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy

REPS = 3
T, HZ = 69, 5           # 64 steps per path
SEQ_PATHS = 8


class Env:
    def __init__(self, z, mean, std):
        self.n_assets = z.shape[1]
        self.stats = MagicMock()
        self.stats.mean, self.stats.std = mean.astype(np.float64), std.astype(np.float64)
        self.test_dataset = MagicMock()
        self.test_dataset.data = torch.tensor(z)
        self.test_dataset.dates = pd.date_range("2021-01-01", periods=len(z))
        self.test_dataset.__len__.return_value = len(z)
        self._m, self._s = torch.tensor(mean), torch.tensor(std)

    def extract_current_returns(self, x):
        return x[..., :self.n_assets]

    def destandardize_returns(self, r):
        return r * self._s + self._m


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def medians(fns, reps=REPS):
    for f in fns:
        f()   # warm-up of each form at this shape
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            ts[i].append(timed(f))
    return [statistics.median(t) for t in ts], [(min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--configs", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S = T - HZ
    cfg = BacktestConfig(horizon=HZ)
    print(torch.cuda.get_device_name(0), flush=True)
    lines = ["| shape | work | (a) persistent ms | (a) path-steps/s | (b) per-step loop ms | (b) path-steps/s | "
             "(c) run_backtest ms | (c) path-steps/s | (a)/(b) | (a)/(c) | spread min-max ms (a; b; c) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]

    def row(name, work, n, med, spread, nc=None):
        a, b, c = med
        c = c * n / (nc or n)   # (the baseline's time scaled to the same work)
        sp = "; ".join(f"{lo * 1e3:.1f}-{hi * 1e3:.1f}" for lo, hi in spread)
        r = (f"| {name} | {work} | {a * 1e3:.2f} | {n / a:,.0f} | {b * 1e3:.2f} | {n / b:,.0f} | {c * 1e3:.2f} | "
             f"{n / c:,.0f} | {b / a:.2f} | {c / a:.2f} | {sp} |")
        print(r, flush=True)
        lines.append(r)

    for N in (10, 100):
        rng = np.random.default_rng(N)
        P = args.paths
        z = rng.normal(0, 1, (P, T, N)).astype(np.float32)
        mean = rng.normal(5e-4, 1e-4, N).astype(np.float32)
        std = rng.uniform(0.01, 0.02, N).astype(np.float32)
        zd = torch.tensor(z, device=dev)
        rd = zd * torch.tensor(std, device=dev) + torch.tensor(mean, device=dev)
        s = MarkowitzStrategy(1.0, 1e-3)
        envs = [Env(z[p], mean, std) for p in range(P)]

        def a():
            return run_markowitz_lockstep(s, zd, rd, cfg, mean, std, persistent=True)

        def b():
            return run_markowitz_lockstep(s, zd, rd, cfg, mean, std, persistent=False)

        def c():
            return [run_backtest(s, e, cfg, verbose=False) for e in envs[:SEQ_PATHS]]

        oa, ob, oc = a(), b(), c()
        assert torch.equal(oa["portfolio_value"], ob["portfolio_value"]) and torch.equal(oa["turnover"], ob["turnover"])
        va = oa["portfolio_value"].cpu().numpy()
        for p in range(len(oc)):
            np.testing.assert_allclose(va[p], oc[p]["portfolio_value"].values, rtol=1e-6)
        med, spread = medians([a, b, c])
        row(f"N = {N}, H = 1, {S} steps", f"P = {P} paths", P * S, med, spread, min(P, SEQ_PATHS) * S)

        C = args.configs
        gam = list(np.logspace(-1, 1, C))
        cost = [1e-3 if j % 2 else 1e-4 for j in range(C)]
        z1, r1 = zd[:1].contiguous(), rd[:1].contiguous()
        strats = [MarkowitzStrategy(float(g), float(k)) for g, k in zip(gam, cost)]

        def sa():
            return run_markowitz_sweep(s, z1, r1, cfg, mean, std, gam, cost)

        def sb():
            return [run_markowitz_lockstep(x, z1, r1, cfg, mean, std) for x in strats]

        def sc():
            return [run_backtest(x, envs[0], cfg, verbose=False) for x in strats]

        wa, wb = sa(), sb()
        for j in range(C):
            assert torch.equal(wa["portfolio_value"][j], wb[j]["portfolio_value"])
        med, spread = medians([sa, sb, sc])
        row(f"N = {N}, H = 1, {S} steps", f"sweep of C = {C} configs, P = 1", C * S, med, spread)

    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"`python tools/markowitz_probe.py` on {torch.cuda.get_device_name(0)}: median of {REPS} runs after a "
                    "warm-up of every form, wall time with a device synchronise, the forms alternating. (a)/(b) and "
                    "(a)/(c) are ratios of path-steps/s (config-steps/s in the sweep rows). In the sweep rows (a) is "
                    "run_markowitz_sweep, (b) one run_markowitz_lockstep(P = 1) call per config, (c) one run_backtest "
                    "call per config. In the P-paths rows (c) is timed over the first "
                    f"{SEQ_PATHS} paths and its time scaled to P (its spread column is of the paths timed). {S} steps per "
                    "path, gamma = 1, cost 1e-3, no limit.\n\n" + text)


if __name__ == "__main__":
    main()
