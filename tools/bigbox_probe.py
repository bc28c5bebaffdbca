"""Dev probe: the large-window solve with a position limit (kmpc_solve_box_ws, the BOX form of
ipm_big) against the plain large-window solve (kmpc_solve, path = KMPC_PATH_LARGE) of the same
inputs. Solve only, one process, device events, the two solves alternated, median (and range) of 5
after a warm-up of each; max_weight = 2.5 / N, w_prev = 0.2 Dirichlet + 0.8 / N (every window feasible).
python tools/bigbox_probe.py  (prints the table of profiles/bigbox.md)"""
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, solve_mpc_log_utility_batched, _lib

dev = torch.device("cuda", 0)
REPS = 5
# (N, H, B): BASELINE configs[4]'s shape at two batch sizes, then the other large-window shapes
SHAPES = ((500, 20, 512), (500, 20, 4096), (500, 10, 4096), (300, 15, 4096), (100, 20, 4096))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


print("| N | H | windows | u | plain ms (min - max) | iters | box ms (min - max) | iters | box / plain | per iteration | "
      "status (plain / box) | max w |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for N, H, B in SHAPES:
    u = 2.5 / N
    rng = np.random.default_rng(1000 * N + H)
    wp = torch.tensor(0.2 * rng.dirichlet(np.ones(N), B) + 0.8 / N, device=dev)
    assert (2 * (wp - u).clamp_min(0).sum(-1) <= 0.2 - 0.02).all()   # every window feasible, off the edge
    y = torch.tensor(rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32), device=dev)
    plain = MPCConfig(horizon=H, cost_coeff=1e-3, max_turnover=0.2, solver_path=_lib.PATH_LARGE)
    box = dataclasses.replace(plain, max_weight=u)
    solve = lambda cfg: solve_mpc_log_utility_batched(wp, y, cfg, with_iters=True)
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
    print(f"| {N} | {H} | {B} | {u:.5f} | {mp:.2f} ({min(tp):.2f} - {max(tp):.2f}) | {ip:.2f} | "
          f"{mb:.2f} ({min(tb):.2f} - {max(tb):.2f}) | {ib:.2f} | {mb / mp:.3f} | {(mb / ib) / (mp / ip):.3f} | "
          f"{cnt(sp)} / {cnt(sb)} | {Wb.max().item():.6f} |", flush=True)
