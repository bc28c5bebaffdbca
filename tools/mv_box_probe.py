"""Dev probe: the mean-variance solve with a position limit (kmpc_solve_mv_box) against the plain
solve (kmpc_solve_mv_ws) on the same Markowitz windows. Solve only, device events, the two solves
alternated, median (and range) of 5 after a warm-up of each. python tools/mv_box_probe.py"""
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, solve_mpc_mean_variance_batched
from koopman_mpc_portfolio_rebalancing_amd.baselines import rolling_moments

dev = torch.device("cuda", 0)
REPS = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


print("| windows | N | u | plain ms (min - max) | iters | box ms (min - max) | iters | box / plain | per iteration | status (plain / box) | max w |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for B, N, u in ((65536, 20, 0.1), (4096, 100, 0.03), (1024, 300, 0.01)):
    T = 4096
    rng = np.random.default_rng(0)
    z = torch.tensor(rng.normal(0, 1, (T, N)).astype(np.float32), device=dev)
    ts = rng.integers(60, T, B)
    wp = torch.tensor(rng.dirichlet(np.ones(N), B), device=dev)
    mu, S, _ = rolling_moments(z, ts, 60, N, np.full(N, 5e-4), np.full(N, 0.015))
    mu = mu.unsqueeze(1).contiguous()
    plain = MPCConfig(horizon=1, gamma=1.0, cost_coeff=1e-3)
    box = dataclasses.replace(plain, max_weight=u)
    solve = lambda cfg: solve_mpc_mean_variance_batched(wp, mu, S, cfg, with_iters=True)
    solve(plain), solve(box)
    torch.cuda.synchronize()
    tp, tb = [], []
    for _ in range(REPS):
        t, (Wp, sp, _, ip) = timed(lambda: solve(plain))
        tp.append(t)
        t, (Wb, sb, _, ib) = timed(lambda: solve(box))
        tb.append(t)
    mp, mb = float(np.median(tp)), float(np.median(tb))
    ip, ib = ip.float().mean().item(), ib.float().mean().item()
    cnt = lambda s: np.bincount(s.cpu().numpy(), minlength=5).tolist()
    print(f"| {B} | {N} | {u} | {mp:.2f} ({min(tp):.2f} - {max(tp):.2f}) | {ip:.2f} | {mb:.2f} ({min(tb):.2f} - {max(tb):.2f}) | "
          f"{ib:.2f} | {mb / mp:.3f} | {(mb / ib) / (mp / ip):.3f} | {cnt(sp)} / {cnt(sb)} | {Wb.max().item():.6f} |", flush=True)
