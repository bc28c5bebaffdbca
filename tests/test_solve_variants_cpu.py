"""The matrix of tests/solve_variants.py without a GPU: it names every kernel of kmpc_solve and every
edge of the dispatch, its mirror of the dispatch (kernel_of) agrees with the library wherever the
library can be asked without a launch, and its inputs have the conditions the GPU suite relies on."""
import ctypes
import os
import re

import numpy as np
import pytest

import solve_variants as sv
from koopman_mpc_portfolio_rebalancing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARR = 21   # per-(t, i) arrays of a large-window slab (kmpc_solve_big.h), next to two 64-wide Schur blocks


def _cases_seen():
    seen = {k: set() for k in sv.KERNELS}
    for _, N, H, name, path in sv.MATRIX:
        seen[sv.cell_kernel(N, H, name, path)].add(sv.case_of(*sv.CASES[name]))
    return seen


def test_the_matrix_names_all_62_kernels():
    assert (sv.PATH_AUTO, sv.PATH_REGISTER, sv.PATH_LARGE, sv.PATH_REGISTER_UNPACKED, sv.PACK_MIN_B, sv.MIXED_MIN_B) == \
        (_lib.PATH_AUTO, _lib.PATH_REGISTER, _lib.PATH_LARGE, _lib.PATH_REGISTER_UNPACKED, _lib.PACK_MIN_B, _lib.MIXED_MIN_B)
    assert len(sv.KERNELS) == 62 == len(set(sv.KERNELS))
    assert len([k for k in sv.KERNELS if k.startswith("big_")]) == 12
    assert len([k for k in sv.KERNELS if k.startswith("pack_")]) == 17
    assert len([k for k in sv.KERNELS if k.startswith("case_")]) == 12
    assert len([k for k in sv.KERNELS if k.startswith("gen_")]) == 20
    assert {sv.cell_kernel(N, H, name, path) for _, N, H, name, path in sv.MATRIX} | {"simplex"} == set(sv.KERNELS)
    # the presolve is what AUTO runs in case 1; the matrix sends that case to the interior point
    assert sv.kernel_of(64, 5, 0.0, 0.0, False) == "simplex"
    assert all(sv.cell_kernel(N, H, name, path) != "simplex" for _, N, H, name, path in sv.MATRIX)
    ids = [sv.cell_id(N, H, name, path) for _, N, H, name, path in sv.MATRIX]
    assert len(set(ids)) == len(ids)                      # one test id per cell
    # every shape runs all six cases, on six windows
    assert len(sv.MATRIX) == 6 * (2 * len(sv.SMALL) + len(sv.REGISTER) + len(sv.FORCED_LARGE) + len(sv.LARGE))
    assert [sv.case_of(*v) for v in sv.CASES.values()] == [7, 7, 3, 1, 6, 2]


def test_every_run_time_case_kernel_sees_each_case_it_can_get():
    """A kernel that reads the constraint case at run time sees every case its dispatch can send it:
    all five where the horizon is ragged or H <= 2 (no constant-case rung takes H = 1..4, 6..9);
    without 7 where a constant-case rung takes case 7 first (the large-window kernels, exact-H
    256-thread blocks); without 7 and 1 where one also takes case 1 (exact H = 5 / 10, N <= 128).
    A constant-case kernel sees its own."""
    for name, cases in _cases_seen().items():
        if name == "simplex":
            want = set()
        elif "_k7" in name:
            want = {7}
        elif name.endswith("_k1"):
            want = {1}
        elif name.startswith("big_") or name in ("gen_hm5_256_exact", "gen_hm10_256_exact"):
            want = {1, 2, 3, 6}
        elif name.startswith("gen_hm") and name.endswith("_exact") and "hm2" not in name:
            want = {2, 3, 6}
        else:   # ragged H, HM = 2, and the packed generic kernels (one kernel for ragged and exact H)
            want = {1, 2, 3, 6, 7}
        assert cases == want, (name, cases)


def test_every_dispatch_edge_is_a_shape():
    Ns = {N for N, _ in sv.SHAPES}
    Hs = {H for _, H in sv.SHAPES}
    assert {10, 11, 16, 17, 32, 33, 64, 65, 103, 104, 128, 129, 192, 193, 215, 216, 256, 257, 512, 513, 1024} <= Ns
    assert {2, 3, 5, 6, 10, 11, 21} <= Hs
    # ... and on the side of the edge that matters: the QL strides at H = 10, the block sizes on
    # the register and on the large-window side
    for N, H in ((103, 10), (104, 10), (215, 10), (216, 10), (192, 10), (193, 8), (256, 10), (257, 10), (512, 12),
                 (513, 11), (1024, 2), (20, 11), (256, 21)):
        assert (N, H) in sv.SHAPES


def _desc(N, H, name, path, B):
    c, tau, short = sv.CASES[name]
    d = _lib.SolveDesc()
    d.B, d.N, d.H, d.cost_coeff, d.max_turnover, d.allow_short, d.path = B, N, H, c, tau, int(short), path
    return d


@pytest.mark.parametrize("B", [sv.B, 800])
def test_mirror_agrees_with_the_workspace_query(B):
    """kmpc_workspace_bytes is non-zero exactly where kernel_of names a large-window kernel, and is
    then min(B, slots) slabs of (21 HM + 128) 64 ceil(N / 64) doubles at that kernel's HM."""
    lib = _lib.load()
    for _, N, H, name, path in sv.MATRIX:
        k = sv.kernel_of(N, H, *sv.CASES[name], path=path, B=B)
        hm = sv.big_hm(k)
        slots = min(B, sv.BIG_SLOTS_SMALL if N <= 256 else sv.BIG_SLOTS)
        want = 8 * (N_ARR * hm + 128) * 64 * ((N + 63) // 64) * slots if hm else 0
        assert lib.kmpc_workspace_bytes(None, ctypes.byref(_desc(N, H, name, path, B))) == want, (N, H, name, path, k)


def test_header_states_the_workspace_formula():
    """include/kmpc.h documents the slab size the library reports (it said 22 HM after the slab
    lost an array)."""
    hdr = open(os.path.join(ROOT, "include", "kmpc.h")).read()
    big = open(os.path.join(ROOT, "koopman_mpc_portfolio_rebalancing_amd", "csrc", "kmpc_solve_big.h")).read()
    assert re.search(r"\((\d+) HM \+ 128\)", hdr).group(1) == str(N_ARR)
    arrays = re.search(r"enum : int \{([^}]*)N_ARR \}", big).group(1)
    assert len([a for a in arrays.split(",") if a.strip()]) == N_ARR


def test_mirror_agrees_with_the_backtest_shape_probe():
    """kmpc_backtest_run's n_steps = 0 probe (tests/bt_probe.py) accepts a call exactly where
    kmpc_solve runs a case-7 exact-H packed or constant-case kernel on the same batch."""
    lib = _lib.load()
    n_ok = 0
    for _, N, H, name, path in sv.MATRIX:
        d = _desc(N, H, name, path, sv.B)
        bt = _lib.BacktestDesc(sv.B, N, 20, 1e-3)
        rc = lib.kmpc_backtest_run(ctypes.byref(bt), ctypes.byref(d), 0, 0, None, None, 0, *([None] * 6), None)
        k = sv.cell_kernel(N, H, name, path)
        assert rc == (_lib.KMPC_OK if sv.persistent(k) else _lib.KMPC_ERR_UNSUPPORTED), (N, H, name, path, k, rc)
        n_ok += rc == _lib.KMPC_OK
    assert n_ok >= 30


# one shape per family
SAMPLE = [(10, 5), (65, 5), (104, 7), (40, 3), (257, 10)]


@pytest.mark.parametrize("name", list(sv.CASES))
@pytest.mark.parametrize("N,H", SAMPLE, ids=[f"N{N}_H{H}" for N, H in SAMPLE])
def test_inputs_have_the_intended_statuses(N, H, name):
    c, tau, short = sv.CASES[name]
    wp, y, W, st, val, it = sv.reference(N, H, name)
    assert wp.shape == (sv.B, N) and y.shape == (sv.B, H, N) and y.dtype == np.float32
    assert np.isnan(y[sv.NAN_WINDOW, H - 1, N // 2]) and np.isnan(y).sum() == 1
    want = sv.intended_status(N, H, name)
    assert want[sv.NAN_WINDOW] == 4 and (want[sv.INFEASIBLE_WINDOW] == 2) == (tau > 0)
    assert not any((N, H, name, b) in sv.ORACLE_INACCURATE for b in range(sv.B))
    assert np.array_equal(st, want), (st, want)
    rest = [b for b in range(sv.B) if want[b] == 0]
    assert np.allclose(wp[rest].sum(-1), 1.0, atol=1e-12)
    assert short or wp[rest].min() >= 0
    if tau > 0:
        assert wp[sv.INFEASIBLE_WINDOW].sum() == 3.0 and wp[sv.INFEASIBLE_WINDOW, 0] == 3.0
    assert np.isfinite(val[rest]).all() and np.isnan(val[want != 0]).all()
    # the oracle applies the fallback too
    for b in np.flatnonzero(want):
        assert np.array_equal(W[b], np.tile(wp[b], (H, 1)))


def test_the_oracle_exceptions_are_cells_of_the_matrix():
    for N, H, name, b in sv.ORACLE_INACCURATE:
        assert (N, H) in sv.SHAPES and name == "k2" and sv.intended_status(N, H, name)[b] == 0
