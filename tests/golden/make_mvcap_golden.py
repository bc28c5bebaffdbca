"""Goldens of the mean-variance MPC solve with an L1 turnover cap (kmpc_solve_mv_cap):
``python tests/golden/make_mvcap_golden.py`` writes tests/golden/mvcap_N{N}_H{H}.npz. A one-off on
the CPU (the dense interior point of tests/mv_cap_ref.py and numpy only); nothing on the GPU side
runs it.

Per file: the windows of one case of mv_cap_ref.CASES (w_prev [B, N], mu [B, H, N], sigma [B, N, N]
from mv_cap_ref.case_inputs), config = (gamma, c, tau, u or 0, allow_short), W [B, H, N] and obj [B]
(oracle.mv_ref.mv_objective at W) of the dense reference.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mv_cap_ref  # noqa: E402

# the cases of mv_cap_ref.CASES stored as files, by id, and the windows kept of each
STORED = {"N10_H1_c0.001_tau0.2": 4, "N10_H1_c0_tau0.2": 4, "N10_H3_c0.001_tau0.2_short": 4,
          "N16_H8_c0.001_tau0.2": 3, "N43_H3_c0.001_tau0.05": 2}


def file_name(case) -> str:
    N, H, gamma, c, tau, u, short, B = case
    return f"mvcap_N{N}_H{H}" + ("_c0" if c == 0 else "") + ("_short" if short else "") + ".npz"


def main():
    for case in mv_cap_ref.CASES:
        if mv_cap_ref.case_id(case) not in STORED:
            continue
        N, H, gamma, c, tau, u, short, _ = case
        B = STORED[mv_cap_ref.case_id(case)]
        t0 = time.time()
        wp, mu, S = (a[:B] for a in mv_cap_ref.case_inputs(case))
        W = np.empty((B, H, N))
        obj = np.empty(B)
        gaps, to = [], []
        for b in range(B):
            W[b], st = mv_cap_ref.dense_mv_cap_ipm(wp[b], mu[b], S[b], gamma, c, tau, u, short)
            if st != "optimal":
                raise RuntimeError(f"{mv_cap_ref.case_id(case)} window {b}: the dense reference ended {st}")
            obj[b] = mv_cap_ref.mv_objective(W[b], wp[b], mu[b], S[b], gamma, c)
            gaps.append(mv_cap_ref.gap(W[b], wp[b], mu[b], S[b], gamma, c, tau, u, short))
            to.append(mv_cap_ref.turnover(W[b], wp[b]).max())
        np.savez_compressed(os.path.join(HERE, file_name(case)), w_prev=wp, mu=mu, sigma=S,
                            config=np.array([gamma, c, tau, u or 0.0, float(short)]), W=W, obj=obj)
        print(f"{mv_cap_ref.case_id(case)}: gap <= {max(gaps):.2e}, turnover - tau <= {max(to) - tau:.2e}, "
              f"{time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
