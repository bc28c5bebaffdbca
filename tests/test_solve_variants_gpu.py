"""Every kernel of the plain solve (kmpc_solve) under every constraint case, against the long-double
oracle: the matrix of tests/solve_variants.py, one test per (shape, case, path).

Each cell solves six windows — a NaN window and, where the case has a cap, an infeasible one between
solved ones — and holds every window to the project's bars: status; objective within
1e-6 + 1e-5 |f*| of the oracle and value == reference_objective(W) to 1e-12; budget and turnover
1e-8, bounds 1e-9; W[0] within 1e-3 where the optimum is unique (cost, no shorting); without shorting
the LP certificate of oracle/certificate.py on the device's own W, a reference that shares no code
with the interior point; a second launch, the solved windows launched alone and return_full=False
bit-identical; packed windows against their one-per-wave twin. Then the unbounded program, slot reuse
under the run-time-case large-window kernel, and AUTO's packing threshold.

One cell found a defect: N9_H9-k7-pack_hm10_g32_gen, window 5, ended optimal_inaccurate where the
long-double oracle is optimal, every other bar met. At iteration 9 the window has mu = 1.135e-06, just
above KMPC_REFINE_MU, so that corrector ran unrefined; its step takes mu to 5.9e-09 and left a dual
residual of 2.2e-07 (long double: 4.0e-10) that later refinement no longer removed. The kernels now
also refine a corrector that aims that far below the threshold (KMPC_REFINE_SMU, kmpc_solve_kernel.h;
profiles/solve_variants_parity.md).
"""
import numpy as np
import pytest
import torch

import solve_variants as sv
from oracle import certificate, dense_ipm, solver as oracle
from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, _lib, solve_mpc_log_utility_batched

pytestmark = pytest.mark.gpu


def _solve(wp, y, name, path, full=True):
    c, tau, short = sv.ALL_CASES[name]
    cfg = MPCConfig(horizon=y.shape[1], cost_coeff=c, max_turnover=tau, allow_short=short, solver_path=path)
    try:
        W, st, val, it = solve_mpc_log_utility_batched(torch.tensor(wp, device="cuda"), torch.tensor(y, device="cuda"),
                                                       cfg, return_full=full, with_iters=True)
        torch.cuda.synchronize()
        return W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy()
    except RuntimeError as e:
        if isinstance(e, _lib.KmpcError):   # a return code of the library: this test's failure
            raise
        # an error of the HIP runtime (a fault in a kernel): the device context is gone, and 500 more
        # cells would only launch on a faulted GPU
        pytest.exit(f"{sv.kernel_of(wp.shape[1], y.shape[1], c, tau, short, path, len(wp))}: {e}", returncode=3)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _bar(f):
    return 1e-6 + 1e-5 * np.abs(f)


def _feasible(W, wp, tau, short, tol=1e-8):
    """The bars of _feasible in test_solver_gpu.py for one window W [H, N]."""
    ok = np.allclose(W.sum(-1), 1.0, atol=tol)
    if not short:
        ok &= bool((W >= -1e-9).all())
    if tau > 0:
        ok &= bool((np.abs(np.diff(np.vstack([wp[None], W]), axis=0)).sum(-1) <= tau + tol).all())
    return bool(ok)


def _is_fallback(W, st, val, wp, b, status):
    return st[b] == status and np.array_equal(W[b], np.tile(wp[b], (W.shape[1], 1))) and np.isnan(val[b])


def _hold_to_oracle(W, st, val, wp, y, name, ref, windows):
    """The status, objective, value, feasibility and W[0] bars on the given windows against
    ref = (Wo, sto, valo) of the same windows. Returns (failures, worst objective error over its bar's
    scale, worst W[0] error, count of shorting windows the device calls inaccurate where the oracle
    says optimal)."""
    c, tau, short = sv.ALL_CASES[name]
    Wo, sto, valo = ref
    fails, n_inacc, w0 = [], 0, 0.0
    err = np.abs(val[windows] - valo[windows])
    for b in windows:
        if st[b] > 1 or (st[b] == 1 and sto[b] == 0 and not short):
            fails.append(f"window {b}: status {st[b]} against the oracle's {sto[b]}")
            continue
        n_inacc += int(st[b] == 1 and sto[b] == 0)
        if not abs(val[b] - valo[b]) <= _bar(valo[b]):
            fails.append(f"window {b}: objective {val[b]!r} against {valo[b]!r}, bar {_bar(valo[b]):.3e}")
        f = dense_ipm.reference_objective(W[b], wp[b], y[b], c)
        if not abs(val[b] - f) <= 1e-12:
            fails.append(f"window {b}: value {val[b]!r} but f(W) = {f!r}")
        if not _feasible(W[b], wp[b], tau, short):
            fails.append(f"window {b}: W is not feasible")
        if c > 0 and not short:
            w0 = max(w0, np.abs(W[b, 0] - Wo[b, 0]).max())
            if not np.abs(W[b, 0] - Wo[b, 0]).max() < 1e-3:
                fails.append(f"window {b}: W[0] off by {np.abs(W[b, 0] - Wo[b, 0]).max():.3e}")
    return fails, float(np.nanmax(err)) if np.isfinite(err).any() else float("nan"), float(w0), n_inacc


CELLS = [(N, H, name, path) for _, N, H, name, path in sv.MATRIX]


@pytest.mark.parametrize("N,H,name,path", CELLS, ids=[sv.cell_id(*c) for c in CELLS])
def test_kernel_matches_the_long_double_oracle(N, H, name, path):
    c, tau, short = sv.CASES[name]
    kernel = sv.cell_kernel(N, H, name, path)
    wp, y, Wo, sto, valo, ito = sv.reference(N, H, name)
    want = sv.intended_status(N, H, name)
    solved = [b for b in range(sv.B) if want[b] == 0]
    # the input conditions: the oracle reports the intended statuses (three known windows inaccurate)
    assert [int(s) for s in sto] == [1 if (N, H, name, b) in sv.ORACLE_INACCURATE else int(want[b]) for b in range(sv.B)]

    W, st, val, it = out = _solve(wp, y, name, path)
    fails, err, w0, n_inacc = _hold_to_oracle(W, st, val, wp, y, name, (Wo, sto, valo), solved)
    for b in range(sv.B):
        if want[b] and not _is_fallback(W, st, val, wp, b, want[b]):
            fails.append(f"window {b}: status {st[b]}, wanted {want[b]} and the fallback")

    # the LP certificate on the device's own W: the first and the last window at least
    gap = float("nan")
    if not short:
        gaps = []
        for b in (solved[0], solved[-1]):
            if st[b] > 1:
                continue
            r = certificate.certify(W[b], wp[b], y[b], c, tau)
            gaps.append(r["gap"])
            if not (r["violation"] <= 1e-8 and -1e-12 <= r["gap"] <= _bar(r["f"])):
                fails.append(f"window {b}: certificate {r}")
            if not abs(-r["f"] - val[b]) <= 1e-12:
                fails.append(f"window {b}: value {val[b]!r} but the certificate's f = {-r['f']!r}")
        gap = max(gaps, default=gap)
    print(f"KERNEL {kernel} N={N} H={H} {name} path={path}: status {st.tolist()} oracle {sto.tolist()} "
          f"objective error {err:.3e} gap {gap:.3e} W0 error {w0:.3e} iterations {it[solved].min()}..{it[solved].max()} "
          f"oracle {ito[solved].min()}..{ito[solved].max()} inaccurate {n_inacc}")
    assert not fails, fails

    assert _same(out, _solve(wp, y, name, path))                 # a second launch is bit-identical
    # the NaN and the infeasible window do not touch their neighbours
    alone = _solve(wp[solved], y[solved], name, path)
    assert _same(alone, (W[solved], st[solved], val[solved], it[solved]))
    W0, st0, val0, it0 = _solve(wp, y, name, path, full=False)
    assert W0.shape == (sv.B, N) and np.array_equal(W0, W[:, 0])
    assert _same((st0, val0, it0), (st, val, it))
    if path == sv.PATH_REGISTER and N <= 32:                     # packed against its one-per-wave twin
        assert kernel.startswith("pack_")
        Wu, stu, valu, _ = _solve(wp, y, name, sv.PATH_REGISTER_UNPACKED)
        assert not sv.cell_kernel(N, H, name, sv.PATH_REGISTER_UNPACKED).startswith("pack_")
        assert np.array_equal(stu <= 1, st <= 1)
        assert (np.abs(val[solved] - valu[solved]) <= _bar(valo[solved])).all()


@pytest.mark.parametrize("N,H,path", sv.UNBOUNDED_SHAPES,
                         ids=[f"N{N}_H{H}-k0-{sv.kernel_of(N, H, 0.0, 0.0, True, p)}" for N, H, p in sv.UNBOUNDED_SHAPES])
def test_unbounded_program(N, H, path):
    """Shorting without cost or cap: sum_t log(R_t . w_t) has no maximum on 1'w = 1. The oracle says
    unbounded (status 3) before its first iteration; every kernel that reads the case at run time does
    too, with the fallback, next to the NaN window."""
    wp, y, Wo, sto, valo, ito = sv.reference(N, H, "k0")
    assert sto.tolist() == [3, 4, 3, 3, 3, 3] and (ito == 0).all()
    W, st, val, it = _solve(wp, y, "k0", path)
    print(f"KERNEL {sv.kernel_of(N, H, 0.0, 0.0, True, path)} N={N} H={H} k0 path={path}: status {st.tolist()} "
          f"iterations {it.tolist()}")
    for b in range(sv.B):
        assert _is_fallback(W, st, val, wp, b, 4 if b == sv.NAN_WINDOW else 3), (b, st[b])


def test_slot_reuse_under_the_run_time_case_large_kernel():
    """800 windows of (30, 11) with shorting and a cap (case 6) on big_hm21_256_gen's 768 slots: the
    windows a reused workgroup solves second equal the same windows solved alone, bit for bit, and
    three of them meet the oracle's bars."""
    N, H, B, name = 30, 11, 800, "k6"
    c, tau, short = sv.CASES[name]
    assert sv.kernel_of(N, H, c, tau, short, sv.PATH_AUTO, B) == "big_hm21_256_gen" and B > sv.BIG_SLOTS_SMALL
    rng = np.random.default_rng(100000 * N + 100 * H + B)
    wp = rng.dirichlet(np.ones(N), B) * 1.5 - 0.5 / N
    y = rng.normal(5e-4, 0.02, (B, H, N)).astype(np.float32)
    W, st, val, it = _solve(wp, y, name, sv.PATH_AUTO)
    assert (st <= 1).all(), np.bincount(st)
    for b in (0, 767, 768, 799):
        one = _solve(wp[b:b + 1], y[b:b + 1], name, sv.PATH_AUTO)
        assert _same(one, (W[b:b + 1], st[b:b + 1], val[b:b + 1], it[b:b + 1])), b
    idx = np.array([1, 768, 799])
    Wo, sto, valo, _ = oracle.solve_batch(wp[idx], y[idx], c, tau, allow_short=short)
    assert (sto == 0).all(), sto
    fails, err, _, n_inacc = _hold_to_oracle(W[idx], st[idx], val[idx], wp[idx], y[idx], name, (Wo, sto, valo), range(3))
    print(f"KERNEL big_hm21_256_gen N={N} H={H} {name} B={B}: status {np.bincount(st).tolist()} objective error {err:.3e} "
          f"iterations {it.min()}..{it.max()} inaccurate {n_inacc}")
    assert not fails, fails


def test_auto_packs_small_windows_past_512():
    """(10, 5) in case 7 under PATH_AUTO: 512 windows run one per wave, 513 packed four per wave. Both
    meet the oracle's bars on a 16-window sample, and agree to the objective bar on every window."""
    N, H, name = 10, 5, "k7"
    c, tau, short = sv.CASES[name]
    k512, k513 = (sv.kernel_of(N, H, c, tau, short, sv.PATH_AUTO, B) for B in (512, 513))
    assert (k512, k513) == ("case_hm5_64_k7", "pack_hm5_g16_k7s11")
    rng = np.random.default_rng(100000 * N + 100 * H + 513)
    wp = rng.dirichlet(np.ones(N), 513)
    y = rng.normal(5e-4, 0.02, (513, H, N)).astype(np.float32)
    one = _solve(wp[:512], y[:512], name, sv.PATH_AUTO)
    packed = _solve(wp, y, name, sv.PATH_AUTO)
    idx = np.arange(0, 512, 32)
    Wo, sto, valo, _ = oracle.solve_batch(wp[idx], y[idx], c, tau)
    assert (sto == 0).all(), sto
    for kernel, (W, st, val, it) in ((k512, one), (k513, packed)):
        assert (st == 0).all(), np.bincount(st)
        fails, err, w0, _ = _hold_to_oracle(W[idx], st[idx], val[idx], wp[idx], y[idx], name, (Wo, sto, valo), range(16))
        print(f"KERNEL {kernel} N={N} H={H} {name} B={len(st)}: objective error {err:.3e} W0 error {w0:.3e} "
              f"iterations {it.min()}..{it.max()}")
        assert not fails, fails
    assert (np.abs(one[2] - packed[2][:512]) <= _bar(one[2])).all()
    assert np.abs(one[0][:, 0] - packed[0][:512, 0]).max() < 1e-3
