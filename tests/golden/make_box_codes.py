"""Record the return codes of every entry that takes a position limit, over the whole grid of the
rules that are decided before any launch -> tests/golden/box_codes.npz.

    python tests/golden/make_box_codes.py [--lib PATH/libkmpc.so] [--commit HASH]

Run once against the library of the commit whose behaviour is to be kept (HASH, default the checked
out HEAD, is written into the file); tests/test_box_codes_cpu.py replays the file's rows against the
built library with solve_codes / mv_codes below and demands equality. Null arrays and n_steps = 0
keep every row ahead of a launch, so no GPU is needed.

The solve family (kmpc_solve_desc with cost_coeff = 1e-3, max_turnover = 0.2), per row: kmpc_solve_box;
kmpc_solve_box_workspace_bytes; kmpc_solve_box_ws with a non-null workspace of 2^62 bytes and with
null / 0; kmpc_backtest_run_box and kmpc_backtest_sweep_box with P = B, S = 20, n_cfg = 3, n_steps = 0.
The mean-variance pair, on a grid of its own: kmpc_solve_mv_box; kmpc_markowitz_run and _sweep with
P = B, S = 20, n_cfg = 3, n_steps = 0."""
import argparse
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from koopman_mpc_portfolio_rebalancing_amd import _lib  # noqa: E402

OUT = os.path.join(HERE, "box_codes.npz")
NS = (2, 10, 32, 33, 100, 256, 257, 300, 1024, 1025)
# max_weight as (kind, factor): the value is factor, or factor / N for kind 1
US = ((0, float("nan")), (0, -0.1), (0, 0.0), (1, 1.0), (1, 2.5), (0, 1.0), (0, 3.0))
SOLVE_COLS = ("N", "H", "path", "precision", "allow_short", "return_full_W", "B", "u")
MV_COLS = ("N", "H", "allow_short", "return_full_W", "B", "u")
S, N_CFG = 20, 3

_BUF = ctypes.create_string_buffer(64)
_P = ctypes.cast(_BUF, ctypes.c_void_p)   # a non-null pointer that no rule reads


def _grid(names, *axes):
    rows = []
    for r in itertools.product(*axes):
        *head, (kind, f) = r
        rows.append(tuple(head) + (f / head[0] if kind else f,))
    a = np.array(rows, dtype=np.float64)
    return {n: (a[:, i] if n == "u" else a[:, i].astype(np.int32)) for i, n in enumerate(names)}


def solve_grid():
    return _grid(SOLVE_COLS, NS, (1, 5, 10, 11, 21, 22), (0, 1, 2, 3), (0, 1, 2), (0, 1), (0, 1), (0, 4), US)


def mv_grid():
    return _grid(MV_COLS, NS, (1, 5, 16, 17), (0, 1), (0, 1), (0, 4), US)


def solve_codes(lib, g):
    """The six recorded answers for every row of the solve family's grid g (columns SOLVE_COLS)"""
    n = len(g["N"])
    out = {k: np.zeros(n, np.int64) for k in ("box", "ws_bytes", "ws_big", "ws_null", "bt_run", "bt_sweep")}
    d, bd, z = _lib.SolveDesc(), _lib.BacktestDesc(), None
    d.cost_coeff, d.max_turnover = 1e-3, 0.2
    for i in range(n):
        d.N, d.H, d.path, d.precision = int(g["N"][i]), int(g["H"][i]), int(g["path"][i]), int(g["precision"][i])
        d.allow_short, d.return_full_W, d.B = int(g["allow_short"][i]), int(g["return_full_W"][i]), int(g["B"][i])
        bd.P, bd.N, bd.S, bd.cost_coeff = d.B, d.N, S, 1e-3
        u, pd, pb = float(g["u"][i]), ctypes.byref(d), ctypes.byref(bd)
        out["box"][i] = lib.kmpc_solve_box(pd, u, z, z, z, z, z, z, None)
        out["ws_bytes"][i] = lib.kmpc_solve_box_workspace_bytes(pd, u)
        out["ws_big"][i] = lib.kmpc_solve_box_ws(pd, u, z, z, z, z, z, z, _P, 1 << 62, None)
        out["ws_null"][i] = lib.kmpc_solve_box_ws(pd, u, z, z, z, z, z, z, None, 0, None)
        out["bt_run"][i] = lib.kmpc_backtest_run_box(pb, pd, u, 0, 0, z, z, 0, z, z, z, z, z, z, None)
        out["bt_sweep"][i] = lib.kmpc_backtest_sweep_box(pb, pd, u, N_CFG, z, z, z, 0, 0, z, z, 0, z, z, z, z, z, z, None)
    return out


def mv_codes(lib, g):
    """The three recorded answers for every row of the mean-variance grid g (columns MV_COLS)"""
    n = len(g["N"])
    out = {k: np.zeros(n, np.int64) for k in ("mv_box", "mk_run", "mk_sweep")}
    d, bd, z = _lib.MvDesc(), _lib.BacktestDesc(), None
    d.gamma, d.cost_coeff = 1.0, 1e-3
    for i in range(n):
        d.N, d.H, d.B = int(g["N"][i]), int(g["H"][i]), int(g["B"][i])
        d.allow_short, d.return_full_W = int(g["allow_short"][i]), int(g["return_full_W"][i])
        bd.P, bd.N, bd.S, bd.cost_coeff = d.B, d.N, S, 1e-3
        u, pd, pb = float(g["u"][i]), ctypes.byref(d), ctypes.byref(bd)
        out["mv_box"][i] = lib.kmpc_solve_mv_box(pd, u, z, z, 0, z, z, z, z, z, None, 0, None)
        out["mk_run"][i] = lib.kmpc_markowitz_run(pb, pd, u, 0, 0, z, z, z, z, 0, z, z, z, z, z, z, None, 0, None)
        out["mk_sweep"][i] = lib.kmpc_markowitz_sweep(pb, pd, u, N_CFG, z, z, z, 0, 0, z, z, z, z, 0, z, z, z, z, z, z,
                                                      None, 0, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                        text=True).stdout.strip()
    lib = _lib.load(a.lib)
    sg, mg = solve_grid(), mv_grid()
    sc, mc = solve_codes(lib, sg), mv_codes(lib, mg)
    data = {"commit": np.array(commit), "version": np.array(lib.kmpc_version().decode())}
    data.update({"solve_" + k: v for k, v in sg.items()})
    data.update({"solve_" + k: (v if k == "ws_bytes" else v.astype(np.int8)) for k, v in sc.items()})
    data.update({"mv_" + k: v for k, v in mg.items()})
    data.update({"mv_" + k: v.astype(np.int8) for k, v in mc.items()})
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: commit {commit}, {len(sg['N'])} solve rows, {len(mg['N'])} mean-variance rows, "
          f"{os.path.getsize(OUT)} bytes")
    for k, v in {**sc, **mc}.items():
        if k != "ws_bytes":
            print(f"  {k}: codes {dict(zip(*(x.tolist() for x in np.unique(v, return_counts=True))))}")
    print(f"  rows with a non-zero workspace: {int((sc['ws_bytes'] > 0).sum())}")


if __name__ == "__main__":
    main()
