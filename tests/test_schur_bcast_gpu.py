"""GPU checks of the Schur LDL^T column broadcast in registers (factor(), kmpc_solve_kernel.h:
KMPC_SCHUR_BCAST_F32 / _F64). The whole-wave kernels (one window per workgroup, GL = 64) keep the
K = 3 H rows of G on lanes 0 .. K - 1 of wave 0 and broadcast each step's column inside the wave:
a permlane16 swap for the two 16-lane DPP rows, then row_newbcast inside the FMAs. Shapes are the
ones at which that can go wrong, not the workload's size: K = 30 on two DPP rows (float32 phase +
float64 finish and float64 alone), a one-wave window, K = 15 inside one DPP row, K = 6, and identity
rows (ragged H < HM, no cap). Every shape: statuses, objective, W[0] and iteration counts against the
long-double oracle at the bars of test_solver_gpu.py, and a second launch bit-identical.

Also the retry of warm starts that do not end optimal (kmpc_ipm_body.inc, PH = 3), with a handoff
deep enough that the pass has windows to solve.
"""
import numpy as np
import pytest
import torch

from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, _lib, solve_mpc_log_utility_batched
from oracle import solver as oracle

pytestmark = pytest.mark.gpu


def _solve(wp, y, cfg):
    W, st, val, it = solve_mpc_log_utility_batched(torch.as_tensor(wp, device="cuda"), torch.as_tensor(y, device="cuda"),
                                                   cfg, with_iters=True)
    return W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy().astype(np.int64)


def _batch(N, H, B, seed):
    rng = np.random.default_rng(seed)
    return rng.dirichlet(np.ones(N), B), rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32)


# N, H, c, tau, solver path, windows
SHAPES = [
    pytest.param(100, 10, 1e-3, 0.2, _lib.PATH_AUTO, 64, id="K30-two-dpp-rows-N100"),
    pytest.param(65, 10, 1e-3, 0.2, _lib.PATH_AUTO, 64, id="K30-N65-mixed-range-low"),
    pytest.param(103, 10, 1e-3, 0.2, _lib.PATH_AUTO, 64, id="K30-N103-mixed-range-high"),
    pytest.param(64, 10, 1e-3, 0.2, _lib.PATH_AUTO, 32, id="K30-one-wave-window"),
    pytest.param(10, 5, 1e-3, 0.2, _lib.PATH_REGISTER_UNPACKED, 32, id="K15-one-dpp-row-unpacked"),
    pytest.param(40, 2, 1e-3, 0.2, _lib.PATH_REGISTER, 32, id="K6-H2"),
    pytest.param(90, 7, 1e-3, 0.2, _lib.PATH_AUTO, 32, id="ragged-H7-identity-rows"),
    pytest.param(100, 10, 1e-3, 0.0, _lib.PATH_AUTO, 32, id="no-cap-v-rows-unused"),
]


@pytest.mark.parametrize("N,H,c,tau,path,B", SHAPES)
def test_register_column_broadcast_matches_oracle(N, H, c, tau, path, B):
    wp, y = _batch(N, H, B, 1000 * N + H)
    # the oracle at the kernels' stopping tolerance, as test_iteration_counts_follow_the_oracle
    Wo, sto, valo, ito = oracle.solve_batch(wp, y, c, tau, tol=1e-9, precision="ld")
    ito = ito.astype(np.int64)
    assert (sto == 0).all()
    bar = 1e-6 + 1e-5 * np.abs(valo).max()
    it64 = None
    # "mixed" is the float32 phase + float64 finish where the shape has the pair (H = 10,
    # 64 < N < 104 with cost or cap), the float64 solve elsewhere
    for precision in ("f64", "mixed"):
        cfg = MPCConfig(horizon=H, cost_coeff=c, max_turnover=tau, solver_path=path, precision=precision)
        W, st, val, it = _solve(wp, y, cfg)
        W2, st2, val2, it2 = _solve(wp, y, cfg)
        assert np.array_equal(W, W2) and np.array_equal(st, st2) and np.array_equal(val, val2) and np.array_equal(it, it2)
        print(precision, "iterations device", it.mean(), "oracle", ito.mean(), "max |d|", np.abs(it - ito).max(),
              "objective err", np.abs(val - valo).max(), "W0 err", np.abs(W - Wo[:, 0]).max())
        assert (st == 0).all()
        assert np.abs(val - valo).max() <= bar
        assert np.abs(W - Wo[:, 0]).max() < 1e-3
        if precision == "f64":
            it64 = it
            assert abs(it.mean() - ito.mean()) <= 0.5
            assert np.abs(it - ito).max() <= 2
        else:
            # float32 + float64 iterations: about the float64-only count (test_mixed_gpu.py's bar)
            assert abs(it.mean() - it64.mean()) < 2.0


def test_retry_of_warm_starts_that_do_not_end_optimal():
    """A handoff at mu <= 2e-5 is deep enough that some float64 finishes do not reach `optimal` from
    the float32 iterate; those windows are solved again from the usual initial point, so no status
    is worse than the float64-only solve's. A retried window reports the iterations of all three
    solves: the float64-only count (the retry is that solve) plus its whole warm attempt — the
    float32 phase, which needs 8 or so iterations to bring mu from the initial point's ~0.5 down
    to 2e-5, and a float64 finish. A window that finished from its warm start took about the
    float64-only count in total (test_mixed_gpu.py: the means within 2). So an excess of 8 or more
    over the float64-only count is more than the float32 phase can account for: a retry.
    Measured with this batch: 28 of 2,048 windows retried, each at twice its float64-only count
    plus 0 to 2, and no other window more than 2 over its float64-only count. The parent commit's
    code (the retry as a launch of its own, the LDL^T column through LDS) runs the same arithmetic:
    its `iters` are byte-identical on the benchmark's 65,536 windows, two retried ones among them."""
    N, H, B, c, tau = 100, 10, 2048, 1e-3, 0.2
    wp, y = _batch(N, H, B, 20)
    W64, st64, val64, it64 = _solve(wp, y, MPCConfig(horizon=H, cost_coeff=c, max_turnover=tau, precision="f64"))
    cfg = MPCConfig(horizon=H, cost_coeff=c, max_turnover=tau, precision="mixed", mu_handoff=2e-5)
    W, st, val, it = _solve(wp, y, cfg)
    W2, st2, val2, it2 = _solve(wp, y, cfg)
    assert np.array_equal(W, W2) and np.array_equal(st, st2) and np.array_equal(val, val2) and np.array_equal(it, it2)
    retried = it - it64 >= 8
    print("retried windows", int(retried.sum()), "of", B, "iterations", it[retried], "float64-only", it64[retried],
          "largest excess of the others", (it - it64)[~retried].max())
    assert (st <= st64).all()
    assert np.abs(val - val64).max() <= 1e-6 + 1e-5 * np.abs(val64).max()
    assert np.abs(W - W64).max() < 1e-3
    assert retried.any()
