"""Goldens of the log-utility MPC solve with a per-asset position limit (kmpc_solve_box):
``python tests/golden/make_box_golden.py`` writes tests/golden/box_N{N}_H{H}.npz, every case or,
with arguments ``N,H ...``, those files only (the others stay as committed). A one-off on the
CPU (a few minutes: the dense interior point of tests/box_ref.py); nothing on the GPU side runs it.

Per file: w_prev [B, N], yhat [B, H, N] float32, config = (c, tau, u), feasible [B] bool
(box_ref.feasible), W [B, H, N] and obj [B] (oracle.dense_ipm.reference_objective at W) of the
dense reference — tile(w_prev) and NaN on the infeasible windows.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import box_ref  # noqa: E402

# (N, H, c, tau, u, B)
CASES = [
    (3, 2, 1e-3, 0.2, 0.5, 4),       # HM = 2, 64 threads; one infeasible window
    (10, 5, 1e-3, 0.2, 0.25, 6),     # HM = 5, BASELINE configs[0]'s shape
    (13, 4, 1e-3, 0.0, 0.2, 4),      # ragged H, cost without cap
    (16, 5, 0.0, 0.3, 0.15, 6),      # cap without cost
    (30, 5, 0.0, 0.0, 0.1, 4),       # no turnover terms
    (65, 6, 1e-3, 0.3, 0.05, 3),     # HM = 10 ragged, 128 threads
    (100, 10, 1e-3, 0.2, 0.03, 2),   # the C3 shape; one infeasible window
    (129, 2, 1e-3, 0.3, 0.02, 2),    # HM = 2, 256 threads
    (200, 10, 1e-3, 0.2, 0.02, 1),   # HM = 10, 256 threads
    (256, 5, 1e-3, 0.3, 0.01, 1),    # HM = 5, 256 threads, N at its bound
    # one or more per kernel and dispatch edge the ten above do not reach
    (64, 10, 1e-3, 0.2, 0.05, 3),    # HM = 10, 64 threads, exact H, no inactive lane
    (40, 8, 0.0, 0.3, 0.06, 3),      # HM = 10, 64 threads, ragged H, cap without cost
    (120, 10, 1e-3, 0.15, 0.02, 2),  # HM = 10, 128 threads at the 128-lane stride (box arrays in registers);
                                     # one infeasible window
    (104, 7, 1e-3, 0.3, 0.03, 3),    # first N of the 128-lane stride, ragged H
    (103, 10, 1e-3, 0.2, 0.03, 2),   # last N of the 104-lane stride
    (96, 5, 1e-3, 0.2, 0.03, 3),     # HM = 5, 128 threads
    (128, 3, 1e-3, 0.0, 0.02, 3),    # HM = 5, 128 threads, full block, ragged H, cost without cap
    (70, 2, 1e-3, 0.3, 0.04, 3),     # HM = 2, 128 threads
    (128, 1, 0.0, 0.0, 0.02, 3),     # HM = 2, 128 threads, H = 1, no turnover terms
]


def inputs(N, H, B):
    rng = np.random.default_rng(1000 * N + H)
    w_prev = rng.dirichlet(np.ones(N), B)
    yhat = rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32)
    return w_prev, yhat


def main(argv):
    only = {tuple(int(v) for v in a.split(",")) for a in argv}   # N,H ...: write these files only
    unknown = only - {(N, H) for N, H, *_ in CASES}
    if unknown:
        raise SystemExit(f"no such case: {sorted(unknown)}")
    for N, H, c, tau, u, B in CASES:
        if only and (N, H) not in only:
            continue
        t0 = time.time()
        w_prev, yhat = inputs(N, H, B)
        feas = np.array([box_ref.feasible(w_prev[b], H, N, tau, u) for b in range(B)])
        W = np.empty((B, H, N))
        obj = np.full(B, np.nan)
        note = []
        for b in range(B):
            if not feas[b]:
                W[b] = np.tile(w_prev[b], (H, 1))
                continue
            W[b], ok, it = box_ref.dense_box_ipm(w_prev[b], yhat[b], c, tau, u)
            if not ok:
                raise RuntimeError(f"N={N} H={H} window {b}: the dense reference did not converge")
            obj[b] = box_ref.reference_objective(W[b], w_prev[b], yhat[b], c)
            g = box_ref.gap(W[b], w_prev[b], yhat[b], c, tau, u)
            note.append((it, g, float(W[b].max())))
        np.savez(os.path.join(HERE, f"box_N{N}_H{H}.npz"), w_prev=w_prev, yhat=yhat,
                 config=np.array([c, tau, u]), feasible=feas, W=W, obj=obj)
        print(f"N={N} H={H} u={u}: feasible {feas.tolist()}, iterations <= {max(n[0] for n in note)}, "
              f"gap <= {max(n[1] for n in note):.2e}, max w {max(n[2] for n in note):.6f}, {time.time() - t0:.1f} s",
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
