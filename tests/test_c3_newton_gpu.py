"""GPU tests of the C3 solve's Newton step (kmpc_solve_c3.hip: H = 10, no short, cost and cap, N < 104)
after the Schur triangular solves of lsolve() moved from v_readlane + FMA to the blocked DPP chain
(kmpc_solve_kernel.h, trisolve_fwd_dpp / trisolve_bwd_dpp): wave 0's lanes 0..29 own the rows of
G = L D L^T, so what is checked does not depend on N except through the reductions that feed the
right-hand side — N = 65 (wave 1 holds one asset) and N = 103 (the last size of the rung) are the
edges, N = 100 the C3 size. 64 windows each (tests/c3_newton_cases.py).

  parity        mixed against float64-only at the project's bar (tests/test_mixed_gpu.py): objective
                within 1e-6 + 1e-5 |f*|, equal statuses; both against the long-double oracle at the
                solver tests' bars: the same objective bar, W0 within 1e-3
  non-finite    the N = 100 batch's NaN window and underflowed period end as the float64-only solve
                ends them (statuses, fallback outputs), and every finite window equals, bit for bit,
                the same window of the batch without them
  bit identity  W0, value, status, iters of every batch, mixed and float64-only, equal byte for byte
                those recorded from the parent's library (tests/golden/c3_newton_parent.npz,
                tests/golden/make_c3_newton_golden.py)
"""
import functools
import os

import numpy as np
import pytest

import c3_newton_cases as cases
from oracle import solver as oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3_newton_parent.npz")


@functools.lru_cache(maxsize=None)
def _device(N, precision, nonfinite=None):
    wp, y = cases.batch(N, nonfinite)
    r = cases.solve(wp, y, precision)
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _oracle(N):
    wp, y = cases.batch(N)
    Wo, sto, valo, _ = oracle.solve_batch(wp, y, cases.C, cases.TAU, precision="ld")
    return Wo[:, 0], sto, valo


@pytest.mark.parametrize("N", [65, 103])
def test_mixed_f64_and_oracle_agree_at_the_rung_edges(N):
    m, d = _device(N, "mixed"), _device(N, "f64")
    W0o, sto, valo = _oracle(N)
    assert (sto == 0).all()
    bar = 1e-6 + 1e-5 * np.abs(valo).max()
    dmd = np.abs(m["value"] - d["value"]).max()
    print(f"N = {N}: |f_mixed - f_f64| max {dmd:.3e} (bar {1e-6 + 1e-5 * np.abs(d['value']).max():.3e})")
    assert np.array_equal(m["status"], d["status"])
    assert dmd <= 1e-6 + 1e-5 * np.abs(d["value"]).max()
    for name, r in (("mixed", m), ("f64", d)):
        dv = np.abs(r["value"] - valo).max()
        dw = np.abs(r["W0"] - W0o).max()
        print(f"N = {N} {name}: |f - f*| max {dv:.3e} (bar {bar:.3e}), |W0 - W0*| max {dw:.3e} (bar 1e-3)")
        assert np.array_equal(r["status"], sto)
        assert dv <= bar
        assert dw < 1e-3


def test_non_finite_windows_end_as_in_float64_and_leave_the_others_alone():
    N = 100
    wp, _ = cases.batch(N)
    m, d = _device(N, "mixed"), _device(N, "f64")
    bad = [cases.NAN_WINDOW, cases.UNDERFLOW_WINDOW]
    ok = np.ones(cases.B, bool)
    ok[bad] = False
    assert np.array_equal(m["status"], d["status"])
    assert d["status"][cases.NAN_WINDOW] == 4 and d["status"][cases.UNDERFLOW_WINDOW] == 2
    assert (d["status"][ok] == 0).all()
    for r in (m, d):
        for b in bad:
            assert np.array_equal(r["W0"][b], wp[b]) and np.isnan(r["value"][b])
    assert np.abs(m["value"][ok] - d["value"][ok]).max() <= 1e-6 + 1e-5 * np.abs(d["value"][ok]).max()
    for prec, r in (("mixed", m), ("f64", d)):
        clean = _device(N, prec, False)
        for f in cases.FIELDS:
            assert r[f][ok].tobytes() == clean[f][ok].tobytes(), (prec, f)


@pytest.mark.parametrize("precision", cases.PRECISIONS)
@pytest.mark.parametrize("N", cases.SIZES)
def test_outputs_equal_the_parents_byte_for_byte(N, precision):
    g = np.load(GOLDEN)
    r = _device(N, precision)
    for f in cases.FIELDS:
        want = g[cases.key(N, precision, f)]
        assert r[f].dtype == want.dtype and r[f].shape == want.shape, f
        assert r[f].tobytes() == want.tobytes(), f
