"""Dev probe (GPU): a hyper-parameter sweep of one environment (P = 1 path) over C = 1, 8, 64, 256
configs, at configs[0]'s shape (N = 10, H = 5) and at the C3 shape (N = 100, H = 10). Three ways:
  (a) run_backtest_sweep: the C configs in kmpc_backtest_sweep launches over shared forecasts;
  (b) C sequential run_backtest_lockstep(P = 1) calls, one per config (a sweep without the kernel);
  (c) run_backtest_lockstep at P = C paths (the environment and C - 1 more random ones, one config):
      the same number of window solves in one persistent launch, but C forecasts rolled out per step
      instead of one.
Reports ms per backtest step and config-steps/s (C x steps / wall time, synchronised), the median of
REPS runs after a warm-up of each shape, the variants alternating. The sweep's configs are a grid of
cost_coeff x max_turnover. A persistent launch lasts as long as its slowest work item's sum of window
times, and the windows of (a) and (c) differ (other configs there, other paths here), so two more
variants solve exactly the same windows: (a=) the sweep of C copies of one config and (c=) the
lock-step run of C copies of the one path — their ratio is the sweep kernel's own overhead.

With --spread C (default 64) every config of (a) and every path of (c) is also timed alone.

    python tools/sweep_probe.py [--out profiles/sweep_probe.md]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, KoopmanModelSpec, KoopmanMPCStrategy, MPCConfig,
                                                   run_backtest_lockstep, run_backtest_sweep)

REPS = 3
SHAPES = [("configs[0] model", 10, 128, 5, 130, 10), ("C3 model", 100, 256, 10, 70, 0)]   # name, N, L, H, T, seed


def grid(C, H):
    """C configs: cost_coeff 1e-4 .. 1e-2 (log) x max_turnover 0.05 .. 0.5, all in the kernel's case."""
    nc = max(1, int(round(C ** 0.5)))
    costs = np.logspace(-4, -2, nc) if nc > 1 else np.array([1e-3])
    taus = np.linspace(0.05, 0.5, (C + nc - 1) // nc) if C > 1 else np.array([0.2])
    out = [MPCConfig(horizon=H, cost_coeff=float(c), max_turnover=float(t)) for t in taus for c in costs]
    return out[:C]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cs", default="1,8,64,256")
    ap.add_argument("--spread", type=int, default=64, help="at this C also time every config and path alone (0: skip)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = ["| model | C | (a) sweep ms/step | (a) config-steps/s | (b) sequential ms/step | (b) config-steps/s | "
             "(c) P = C ms/step | (c) config-steps/s | (a)/(c) | (a)/(b) | (a=) ms/step | (c=) ms/step | (a=)/(c=) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    print(torch.cuda.get_device_name(0), flush=True)
    for name, N, L, H, T, seed in SHAPES:
        obs = N * 20
        spec = KoopmanModelSpec.from_state_dict(bench.make_state_dict(obs, L, 1024, seed=seed), bench.MODEL_CFG)
        g = torch.Generator().manual_seed(0)
        CMAX = max(int(c) for c in args.cs.split(","))
        xall = torch.randn(CMAX, T, obs, generator=g).to(dev)
        rall = (torch.randn(CMAX, T, N, generator=g) * 0.015 + 5e-4).to(dev)
        x, r = xall[:1].contiguous(), rall[:1].contiguous()   # the environment
        mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
        bcfg = BacktestConfig(horizon=H)
        S = T - H
        base = KoopmanMPCStrategy(spec, MPCConfig(horizon=H, cost_coeff=1e-3, max_turnover=0.2), device=str(dev))
        km = base.device_model()
        for C in [int(c) for c in args.cs.split(",")]:
            cfgs = grid(C, H)
            strats = [KoopmanMPCStrategy(km, c, device=str(dev)) for c in cfgs]
            xc, rc = xall[:C].contiguous(), rall[:C].contiguous()
            xe, re = x.expand(C, T, obs).contiguous(), r.expand(C, T, N).contiguous()
            same = [cfgs[0]] * C

            def a():
                out = run_backtest_sweep(base, x, r, bcfg, mean, std, cfgs)
                assert bool(out["in_kernel"].all())

            def b():
                for s in strats:
                    run_backtest_lockstep(s, x, r, bcfg, mean, std)

            def c():
                run_backtest_lockstep(base, xc, rc, bcfg, mean, std, persistent=True)

            def a_same():
                run_backtest_sweep(base, x, r, bcfg, mean, std, same)

            def c_same():
                run_backtest_lockstep(strats[0], xe, re, bcfg, mean, std, persistent=True)

            a(), c(), run_backtest_lockstep(strats[0], x, r, bcfg, mean, std)   # warm-up of each shape
            ta, tb, tc, tas, tcs = [], [], [], [], []
            for rep in range(REPS):
                ta.append(timed(a))
                tc.append(timed(c))
                tas.append(timed(a_same))
                tcs.append(timed(c_same))
                if rep == 0 or C <= 64:   # (C = 256 sequential runs take seconds: once)
                    tb.append(timed(b))
            ma, mb, mc, mas, mcs = (statistics.median(t) for t in (ta, tb, tc, tas, tcs))
            row = (f"| {name} (N = {N}, H = {H}, {S} steps) | {C} | {ma / S * 1e3:.3f} | {C * S / ma:,.0f} | "
                   f"{mb / S * 1e3:.3f} | {C * S / mb:,.0f} | {mc / S * 1e3:.3f} | {C * S / mc:,.0f} | "
                   f"{mc / ma:.2f} | {mb / ma:.2f} | {mas / S * 1e3:.3f} | {mcs / S * 1e3:.3f} | {mcs / mas:.2f} |")
            print(row, flush=True)
            lines.append(row)
            if args.spread and C == args.spread:
                # each config and each path alone: a persistent launch lasts as long as its slowest work item
                pa = [min(timed(lambda: run_backtest_sweep(base, x, r, bcfg, mean, std, [cf])) for _ in range(2)) / S * 1e3
                      for cf in cfgs]
                pc = []
                for p in range(C):
                    xp, rp = xall[p:p + 1].contiguous(), rall[p:p + 1].contiguous()
                    pc.append(min(timed(lambda: run_backtest_lockstep(base, xp, rp, bcfg, mean, std, persistent=True))
                                  for _ in range(2)) / S * 1e3)
                k = int(np.argmax(pa))
                note = (f"{name}, C = {C}, ms per step alone: the configs of (a) min {min(pa):.3f} median "
                        f"{statistics.median(pa):.3f} max {max(pa):.3f} (cost {cfgs[k].cost_coeff:.1e}, cap "
                        f"{cfgs[k].max_turnover:.3f}); the paths of (c) min {min(pc):.3f} median {statistics.median(pc):.3f} "
                        f"max {max(pc):.3f}")
                print(note, flush=True)
                notes.append(note)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"`tools/sweep_probe.py` on {torch.cuda.get_device_name(0)}: one environment (P = 1), C configs; "
                    f"median of {REPS} runs, wall time with a device synchronise. (a)/(c) and (a)/(b) are ratios "
                    "of config-steps/s; (a=) / (c=): identical windows (C copies of one config, C copies of the "
                    "path).\n\n" + text + "\n" + "\n\n".join(notes) + "\n")


if __name__ == "__main__":
    main()
