"""Dev probe: one kmpc_rolling_cov_paths call per estimator against kmpc_rolling_moments_paths (the scalar
sample kernel) at the Markowitz backtest's chunk shape: P = 64 paths, N = 100 assets, lookback 60, 52 steps
(the chunk MARKOWITZ_SIGMA_BYTES gives), every window full (test rows 59 .. 110). The C call alone between
device events, the sides alternated within each round, median (and range) of REPS rounds after a warm-up of
each; each round times INNER back-to-back calls and reports one call. Also the Ledoit-Wolf Sigma against the
sample one on the same windows (condition numbers, in numpy).
python tools/rolling_cov_probe.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from koopman_mpc_portfolio_rebalancing_amd import _lib

dev = torch.device("cuda", 0)
REPS, INNER, P, N, LOOKBACK, STEPS = 9, 20, 64, 100, 60, 52
f64 = dict(dtype=torch.float64, device=dev)


def main():
    rng = np.random.default_rng(0)
    T = LOOKBACK + STEPS
    load = rng.normal(0, 1, (3, N))
    z = (rng.normal(0, 1, (P, T, 3)) @ load * 0.6 + rng.normal(0, 0.4, (P, T, N))).astype(np.float32)
    L = _lib.load()
    zt = torch.tensor(z, device=dev)
    m, sd = torch.full((N,), 5e-4, device=dev), torch.full((N,), 0.015, device=dev)
    ts = torch.arange(LOOKBACK - 1, LOOKBACK - 1 + STEPS, dtype=torch.int32, device=dev)
    mu, sigma = torch.empty((STEPS, P, N), **f64), torch.empty((STEPS, P, N, N), **f64)
    valid = torch.empty((STEPS, P), dtype=torch.int32, device=dev)
    rho = torch.empty((STEPS, P), **f64)
    head = (P, STEPS, T, N, LOOKBACK, zt.data_ptr(), N, m.data_ptr(), sd.data_ptr(), ts.data_ptr(), mu.data_ptr(),
            sigma.data_ptr(), valid.data_ptr())

    def side(name):
        def call():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                if name == "sample (rolling_moments_kernel)":
                    rc = L.kmpc_rolling_moments_paths(*head, None)
                else:
                    rc = L.kmpc_rolling_cov_paths(*head, _lib.COV_ESTIMATOR[name], 0.94, rho.data_ptr(), None)
                assert rc == 0, rc
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / INNER
        return call

    names = ["sample (rolling_moments_kernel)", "ledoit_wolf", "oas", "ewma"]
    sides = {n: side(n) for n in names}
    for f in sides.values():
        f()
    times = {n: [] for n in names}
    for _ in range(REPS):
        for n in names:
            times[n].append(sides[n]())
    base = float(np.median(times[names[0]]))
    print(f"P = {P}, N = {N}, lookback {LOOKBACK}, {STEPS} steps ({P * STEPS} windows); ms per call: median (min - max) "
          f"of {REPS} alternated rounds of {INNER} calls")
    print("| estimator | ms / call | against the sample kernel |")
    print("|---|---|---|")
    for n in names:
        t = times[n]
        print(f"| {n} | {np.median(t):.3f} ({min(t):.3f} - {max(t):.3f}) | {np.median(t) / base:.3f} |")
    L.kmpc_rolling_moments_paths(*head, None)
    s0 = sigma[-1, 0].cpu().numpy()
    L.kmpc_rolling_cov_paths(*head, _lib.COV_ESTIMATOR["ledoit_wolf"], 0.94, rho.data_ptr(), None)
    torch.cuda.synchronize()
    s1 = sigma[-1, 0].cpu().numpy()
    print(f"\nlast window of path 0: cond(Sigma) sample {np.linalg.cond(s0):.3e}, ledoit_wolf {np.linalg.cond(s1):.3e} "
          f"(rho {rho[-1, 0].item():.4f})")


if __name__ == "__main__":
    main()
