"""Goldens of the mean-variance MPC solve with a per-asset position limit (kmpc_solve_mv_box):
``python tests/golden/make_mvbox_golden.py`` writes tests/golden/mvbox_N{N}_H{H}.npz. A one-off on
the CPU (the dense interior point of tests/mv_box_ref.py and numpy only); nothing on the GPU side
runs it.

Per file: w_prev [B, N] (Dirichlet draws, 1/N in window 1, a vertex e_b — far above the limit — in
window 2), mu [B, H, N], sigma [B, N, N] (a 60-sample covariance plus 1e-6 I per window; one file
stores a single shared [N, N]), config = (gamma, c, u), W [B, H, N] and obj [B]
(oracle.mv_ref.mv_objective at W) of the dense reference.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mv_box_ref  # noqa: E402

# (N, H, gamma, c, u, B, shared Sigma)
CASES = [
    (4, 1, 1.0, 0.0, 0.6, 8, False),       # part of one wave, no cost rows
    (10, 1, 1.0, 1e-3, 0.25, 8, False),    # the Markowitz shape
    (20, 1, 10.0, 1e-2, 0.2, 8, True),     # one Sigma shared by the batch (sigma_stride 0)
    (5, 3, 0.5, 1e-3, 0.4, 8, False),      # several periods
    (8, 2, 0.0, 1e-3, 0.3, 8, False),      # no curvature: a linear program
    (16, 8, 1.0, 1e-3, 0.15, 6, False),    # n = 128 over many periods, the D'ED coupling
    (64, 2, 1.0, 1e-3, 0.05, 4, False),    # n = 128, the last LDS shape
    (43, 3, 2.0, 0.0, 0.1, 4, False),      # n = 129, the first workspace shape; N u = 4.3
]


def main():
    for N, H, gamma, c, u, B, shared in CASES:
        t0 = time.time()
        wp, mu, S = mv_box_ref.inputs(7000 + 100 * N + H, B, N, H)
        if shared:
            S = S[:1]
        W = np.empty((B, H, N))
        obj = np.empty(B)
        gaps = []
        for b in range(B):
            Sb = S[0] if shared else S[b]
            W[b], st = mv_box_ref.dense_mv_box_ipm(wp[b], mu[b], Sb, gamma, c, u)
            if st != "optimal":
                raise RuntimeError(f"N={N} H={H} window {b}: the dense reference ended {st}")
            obj[b] = mv_box_ref.mv_objective(W[b], wp[b], mu[b], Sb, gamma, c)
            gaps.append(mv_box_ref.gap(W[b], wp[b], mu[b], Sb, gamma, c, u))
        np.savez_compressed(os.path.join(HERE, f"mvbox_N{N}_H{H}.npz"), w_prev=wp, mu=mu, sigma=S[0] if shared else S,
                            config=np.array([gamma, c, u]), W=W, obj=obj)
        print(f"N={N} H={H} u={u}: gap <= {max(gaps):.2e}, max w {W.max():.9f}, {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
