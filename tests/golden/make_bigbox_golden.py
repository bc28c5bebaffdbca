"""Goldens of the log-utility MPC solve with a per-asset position limit on the large-window box
kernel (kmpc_solve_box_ws: N > 256, H > 10 or KMPC_PATH_LARGE):
``python tests/golden/make_bigbox_golden.py`` writes tests/golden/bigbox_N{N}_H{H}.npz, every case
or, with arguments ``N,H ...``, those files only (the others stay as committed). A one-off on the
CPU (several minutes: the dense interior point of tests/box_ref.py; N = 260, H = 11 alone takes
about two); nothing on the GPU side runs it.

The format and the seeding are make_box_golden.py's. Per file: w_prev [B, N], yhat [B, H, N]
float32, config = (c, tau, u), feasible [B] bool (box_ref.feasible), W [B, H, N] and obj [B]
(oracle.dense_ipm.reference_objective at W) of the dense reference — tile(w_prev) and NaN on the
infeasible windows.

The generator raises where a window expected feasible is not (or the reverse), or where the dense
reference does not converge. HM = 21 at 1024 threads has no dense golden (N >= 513 with H >= 11 is
a 1 GB KKT matrix): tests/test_bigbox_gpu.py covers that kernel with the LP certificate.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import box_ref  # noqa: E402
from make_box_golden import inputs  # noqa: E402

# (N, H, c, tau, u, B, infeasible windows)
CASES = [
    (300, 3, 1e-3, 0.3, 0.01, 2, ()),     # HM = 10, 512 threads
    (513, 2, 1e-3, 0.3, 0.006, 2, ()),    # HM = 10, 1024 threads
    (1024, 1, 0.0, 0.0, 0.003, 2, ()),    # HM = 10, 1024 threads, N at its bound, no turnover terms
    (13, 21, 0.0, 0.3, 0.2, 3, ()),       # HM = 21, 256 threads, H at its bound, cap without cost
    (40, 11, 1e-3, 0.3, 0.1, 3, ()),      # HM = 21, 256 threads, first H past 10
    (70, 21, 1e-3, 0.2, 0.04, 2, ()),     # HM = 21, 256 threads
    (100, 20, 1e-3, 0.2, 0.03, 2, ()),    # HM = 21, 256 threads
    (260, 11, 1e-3, 0.3, 0.01, 1, ()),    # HM = 21, 512 threads
    # an infeasible window between feasible ones: the seeded Dirichlet w_prev carries more weight above
    # u than tau lets go in the first period; its neighbours start below the limit (holding is feasible)
    (40, 12, 1e-3, 0.2, 0.06, 3, (1,)),   # HM = 21, 256 threads
]


def case_inputs(N, H, B, infeasible):
    w_prev, yhat = inputs(N, H, B)
    if infeasible:
        for b in range(B):
            if b not in infeasible:
                w_prev[b] = 0.3 * w_prev[b] + 0.7 / N
    return w_prev, yhat


def main(argv):
    only = {tuple(int(v) for v in a.split(",")) for a in argv}   # N,H ...: write these files only
    unknown = only - {(N, H) for N, H, *_ in CASES}
    if unknown:
        raise SystemExit(f"no such case: {sorted(unknown)}")
    for N, H, c, tau, u, B, infeasible in CASES:
        if only and (N, H) not in only:
            continue
        t0 = time.time()
        w_prev, yhat = case_inputs(N, H, B, infeasible)
        feas = np.array([box_ref.feasible(w_prev[b], H, N, tau, u) for b in range(B)])
        want = np.array([b not in infeasible for b in range(B)])
        if (feas != want).any():
            raise RuntimeError(f"N={N} H={H}: feasible {feas.tolist()}, expected {want.tolist()}")
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
            note.append((it, g, float(W[b].max()), int((W[b] > u - 1e-7).sum())))
        np.savez(os.path.join(HERE, f"bigbox_N{N}_H{H}.npz"), w_prev=w_prev, yhat=yhat,
                 config=np.array([c, tau, u]), feasible=feas, W=W, obj=obj)
        print(f"N={N} H={H} u={u}: feasible {feas.tolist()}, iterations {min(n[0] for n in note)}..{max(n[0] for n in note)}, "
              f"gap <= {max(n[1] for n in note):.2e}, max w {max(n[2] for n in note):.6f}, "
              f"at the limit {[n[3] for n in note]}, {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
