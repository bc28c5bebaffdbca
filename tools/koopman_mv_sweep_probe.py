"""Dev probe (GPU): the sweep of the mean-variance Koopman-MPC backtest against the runs it replaces.

For C = 16 configs (a gamma grid, an efficient frontier) over the same P paths:
  (a) run_koopman_mv_sweep: one rollout and one moments pass per chunk, every (config, path) in one
      kmpc_koopman_mv_sweep launch per chunk;
  (b) the same C configs as C run_koopman_mv_lockstep calls one after the other (each with its own
      rollout, moments and kmpc_koopman_mv_run launches) — the only way before the sweep.
Cases (N, H, P): (10, 5) and (100, 10), each at P = 1 and P = 64. Per case one process: the histories of
(a) and (b) are compared bit for bit, then wall time around a device synchronise, the two alternating,
median of REPS after a warm-up of each, with the spread (min - max).

    python tools/koopman_mv_sweep_probe.py [--out profiles/koopman_mv_sweep.md]     every case, each in a
                                            child process of its own under a time limit; stops at the first
                                            case that fails
    python tools/koopman_mv_sweep_probe.py --case N,H,P,STEPS                       one case, one row
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
C = 16
HZ = 5
#         N,  H,  P, steps (of which the first four hold), the child's time limit in seconds
CASES = [(10, 5, 1, 64, 300), (10, 5, 64, 64, 300), (100, 10, 1, 16, 900), (100, 10, 64, 16, 900)]
HEAD = ["| N | H | P | steps | items | (a) sweep ms | (b) " + str(C) + " runs ms | (b) / (a) | spread (a) ms | spread (b) ms | "
        "spread of the ratio | same history |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]


def model(N, dev):
    """The generic Koopman model of tools/mv_band_probe.py over 2 N observables."""
    import torch
    from koopman_mpc_portfolio_rebalancing_amd import DeviceKoopman, KoopmanModelSpec
    obs, hid, Ld = 2 * N, 64, 32
    g = torch.Generator().manual_seed(N)
    rnd = lambda *s, scale=1.0: (torch.rand(*s, generator=g) * 2 - 1) * scale
    enc = [(rnd(hid, obs, scale=obs ** -0.5), rnd(hid, scale=obs ** -0.5)), (rnd(Ld, hid, scale=hid ** -0.5), rnd(Ld, scale=hid ** -0.5))]
    q, _ = torch.linalg.qr(torch.randn(Ld, Ld, generator=g, dtype=torch.float64))
    return DeviceKoopman(KoopmanModelSpec(kind="generic", encoder=enc, kmat=(0.95 * q).float(),
                                          decoder=[(rnd(obs, Ld, scale=Ld ** -0.5), None)]), dev)


def case(N, H, P, steps):
    import numpy as np
    import torch
    from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, KoopmanMVStrategy, MPCConfig,
                                                       run_koopman_mv_lockstep, run_koopman_mv_sweep)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(N)
    z = rng.normal(0, 1, (P, steps, 2 * N)).astype(np.float32)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    zd = torch.tensor(z, device=dev)
    rd = (zd[:, :, :N] * torch.tensor(std, device=dev) + torch.tensor(mean, device=dev)).contiguous()
    km = model(N, dev)
    bt = BacktestConfig(horizon=HZ)
    cfgs = [MPCConfig(horizon=H, gamma=float(g), cost_coeff=1e-3) for g in np.logspace(-1, 2, C)]
    strats = [KoopmanMVStrategy(km, c) for c in cfgs]
    kw = dict(n_rows=steps + HZ)

    def a():
        return run_koopman_mv_sweep(strats[0], zd, rd, bt, mean, std, cfgs, **kw)

    def b():
        return [run_koopman_mv_lockstep(s, zd, rd, bt, mean, std, **kw) for s in strats]

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    oa, ob = a(), b()   # (the warm-up of each)
    same = all(torch.equal(oa[k][j], ob[j][k]) for j in range(C) for k in ("portfolio_value", "turnover", "weights"))
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(timed(a))
        tb.append(timed(b))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(f"| {N} | {H} | {P} | {steps} | {C * P} | {ma:.2f} | {mb:.2f} | {mb / ma:.2f} | {min(ta):.2f} - {max(ta):.2f} | "
          f"{min(tb):.2f} - {max(tb):.2f} | {min(tb) / max(ta):.2f} - {max(tb) / min(ta):.2f} | {same} |", flush=True)
    print("device: " + torch.cuda.get_device_name(0), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, metavar="N,H,P,STEPS")
    args = ap.parse_args()
    if args.case:
        return case(*(int(v) for v in args.case.split(",")))
    rows, device = [], ""
    for N, H, P, steps, limit in CASES:   # a fresh process per case, under its own time limit; nothing after a failure
        print(f"case N = {N}, H = {H}, P = {P}, {steps} steps (limit {limit} s) ...", flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", f"{N},{H},{P},{steps}"],
                           capture_output=True, text=True, timeout=limit)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print(f"case {(N, H, P, steps)} ended with status {r.returncode}: stopping", flush=True)
            return 1
        rows += [ln for ln in r.stdout.splitlines() if ln.startswith("| ")]
        device = next((ln[8:] for ln in r.stdout.splitlines() if ln.startswith("device: ")), device)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"`python tools/koopman_mv_sweep_probe.py` on {device}: (a) run_koopman_mv_sweep of C = {C} configs "
                    f"(gamma = 0.1 .. 100 on a log grid, cost 1e-3, no limit, no cap) against (b) the same configs as {C} "
                    "run_koopman_mv_lockstep calls one after the other, over the same P paths. One process per case; wall "
                    "time of the whole call (rollout and moments included) around a device synchronise, the two alternating, "
                    f"median of {REPS} after a warm-up of each; spread: min - max of the {REPS}; spread of the ratio: "
                    "fastest (b) over slowest (a) - slowest (b) over fastest (a). The first four steps of a path hold "
                    "(fewer than 5 rows). Same history: portfolio value, turnover and final weights of every config "
                    "bit for bit.\n\n" + "\n".join(HEAD + rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
