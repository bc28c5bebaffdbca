"""The L1 turnover cap of the mean-variance solve (MPCConfig.mv_max_turnover, kmpc_solve_mv_cap,
kmpc_markowitz_run_cap / _sweep_cap, MarkowitzStrategy(max_turnover=...)) without a GPU: the symbols
and the unchanged ABI version, every return-code rule of the C functions (decided before any
launch), the Python plumbing and its ValueErrors, the goldens pinned by an LP certificate, the
infeasibility rule d0 > tau against the LP's feasibility, and the kernel's algorithm restated in
numpy (mv_cap_ref.reduced_mv_cap_ipm) held to the device tests' bars on the device tests' inputs."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import mv_cap_ref as ref
import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import BacktestConfig, _lib
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy, sweep_backtest_markowitz
from koopman_mpc_portfolio_rebalancing_amd.mpc import MPCConfig, _box_limit, _mv_turnover_cap
from oracle import mv_ref
from test_markowitz_bt_cpu import markowitz_backtest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "mvcap_*.npz")))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NEW = ("kmpc_mv_cap_workspace_bytes", "kmpc_solve_mv_cap", "kmpc_markowitz_run_cap", "kmpc_markowitz_sweep_cap")
NAN = float("nan")


def test_symbols_and_version():
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmpc.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"


def _desc(B=0, N=10, H=1, gamma=1.0, c=1e-3, short=0, full=0):
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff, d.allow_short, d.return_full_W = B, N, H, gamma, c, short, full
    return d


def _cap(d, u, tau, p=None, ws=None, nws=0):
    return _lib.load().kmpc_solve_mv_cap(ctypes.byref(d), u, tau, p, p, 0, p, p, p, p, None, ws, nws, None)


def _box(d, u, p=None, ws=None, nws=0):
    return _lib.load().kmpc_solve_mv_box(ctypes.byref(d), u, p, p, 0, p, p, p, p, None, ws, nws, None)


def _plain(d, p=None, ws=None, nws=0):
    return _lib.load().kmpc_solve_mv_ws(ctypes.byref(d), p, p, 0, p, p, p, p, None, ws, nws, None)


def test_solve_return_codes_need_no_gpu():
    L = _lib.load()
    assert L.kmpc_solve_mv_cap(None, 0.0, 0.2, None, None, 0, None, None, None, None, None, None, 0, None) == INVALID
    assert _cap(_desc(H=0), 0.0, 0.2) == INVALID
    assert _cap(_desc(B=-1), 0.0, 0.2) == INVALID
    assert _cap(_desc(H=17), 0.0, 0.2) == UNSUPPORTED
    assert _cap(_desc(N=65, H=16), 0.0, 0.2) == UNSUPPORTED
    # the cap itself, before the limit
    for tau in (NAN, -0.1, -float("inf")):
        assert _cap(_desc(), 0.0, tau) == INVALID
        assert _cap(_desc(short=1), 0.5, tau) == INVALID
    assert _cap(_desc(), 0.0, float("inf")) == OK
    # no cap: the existing calls, with their rules
    assert _cap(_desc(), 0.0, 0.0) == OK == _plain(_desc())
    assert _cap(_desc(B=3), 0.0, 0.0) == INVALID == _plain(_desc(B=3))
    assert _cap(_desc(short=1), 0.0, 0.0) == OK
    for u in (0.5, 1.0, 0.1, -0.1, NAN):
        for short in (0, 1):
            assert _cap(_desc(short=short), u, 0.0) == _box(_desc(short=short), u), (u, short)
    # the limit under a cap: 0 none (shorting allowed), else kmpc_solve_mv_box's rules in its order
    assert _cap(_desc(short=1), 0.0, 0.2) == OK
    assert _cap(_desc(), 0.0, 0.2) == OK
    for u in (NAN, -0.1):
        assert _cap(_desc(), u, 0.2) == INVALID
    assert _cap(_desc(short=1), 0.5, 0.2) == UNSUPPORTED
    assert _cap(_desc(short=1), 1.0, 0.2) == UNSUPPORTED
    assert _cap(_desc(short=1, N=10), 0.1, 0.2) == UNSUPPORTED
    assert _cap(_desc(), 1.0, 0.2) == OK and _cap(_desc(), 7.0, 0.2) == OK
    assert _cap(_desc(N=10), 0.1, 0.2) == INVALID and _cap(_desc(N=4), 0.25, 0.2) == INVALID
    # the rules come before the B == 0 return and before the null-array check
    assert _cap(_desc(B=0, N=10), 0.1, 0.2) == INVALID
    assert _cap(_desc(B=5), 0.5, 0.2) == INVALID
    for N, H in ((2, 1), (4, 1), (10, 1), (64, 2), (8, 16), (129, 1), (43, 3), (16, 8), (300, 2), (512, 2), (64, 16), (1024, 1)):
        assert _cap(_desc(N=N, H=H), 0.6, 0.2) == OK == _cap(_desc(N=N, H=H), 0.0, 0.2), (N, H)
    # the workspace: its own query, the CAP slab n (n + 1) / 2 + 2 H n per window in flight
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = lambda d: L.kmpc_mv_cap_workspace_bytes(ctypes.byref(d))
    assert q(_desc(B=4, N=64, H=2)) == 0 == q(_desc(B=4, N=8, H=16)) == q(_desc(B=0, N=129))
    d = _desc(B=4, N=129, H=1)
    need = q(d)
    assert need == 8 * 4 * (129 * 130 // 2 + 2 * 129) > L.kmpc_mv_workspace_bytes(ctypes.byref(d))
    assert q(_desc(B=4, N=43, H=3)) == 8 * 4 * (129 * 130 // 2 + 6 * 129)
    assert q(_desc(B=600, N=129, H=1)) == 8 * 512 * (129 * 130 // 2 + 2 * 129)      # at most 512 windows in flight
    assert _cap(d, 0.0, 0.2, p) == WORKSPACE == _cap(d, 0.5, 0.2, p)
    assert _cap(d, 0.0, 0.2, p, p, need - 1) == WORKSPACE
    assert _cap(d, 0.0, 0.2, p, p, L.kmpc_mv_workspace_bytes(ctypes.byref(d))) == WORKSPACE      # the plain query is too small
    assert _cap(d, 0.0, 0.0, p, p, L.kmpc_mv_workspace_bytes(ctypes.byref(d)) - 1) == WORKSPACE  # no cap: the plain rule


def _run(bd, md, u, tau, step0=0, n_steps=0, a=None, ws=None, nws=0):
    return _lib.load().kmpc_markowitz_run_cap(ctypes.byref(bd), ctypes.byref(md), u, tau, step0, n_steps, a, a, a, a, 0,
                                              a, a, a, a, a, a, ws, nws, None)


def _run0(bd, md, u, step0=0, n_steps=0, a=None, ws=None, nws=0):
    return _lib.load().kmpc_markowitz_run(ctypes.byref(bd), ctypes.byref(md), u, step0, n_steps, a, a, a, a, 0,
                                          a, a, a, a, a, a, ws, nws, None)


def _sweep(bd, md, u, n_cfg, step0=0, n_steps=0, a=None, cap=None, ws=None, nws=0):
    return _lib.load().kmpc_markowitz_sweep_cap(ctypes.byref(bd), ctypes.byref(md), u, n_cfg, a, a, a, cap, step0,
                                                n_steps, a, a, a, a, 0, a, a, a, a, a, a, ws, nws, None)


def test_backtest_return_codes_need_no_gpu():
    L = _lib.load()
    bd = _lib.BacktestDesc(3, 10, 12, 1e-3)
    assert _run(bd, _desc(), 0.0, 0.2) == OK                                # the shape probe
    assert _run(bd, _desc(short=1), 0.0, 0.2) == OK
    assert _run(bd, _desc(N=11), 0.0, 0.2) == INVALID
    assert _run(bd, _desc(full=1), 0.0, 0.2) == INVALID
    assert _run(bd, _desc(), 0.0, 0.2, 10, 3) == INVALID                    # past the history
    assert _run(_lib.BacktestDesc(3, 65, 12, 1e-3), _desc(N=65, H=16), 0.0, 0.2) == UNSUPPORTED
    for tau in (NAN, -1.0):
        assert _run(bd, _desc(), 0.0, tau) == INVALID
    for u in (0.5, 1.0, 0.1, -0.1, NAN, 0.0):                               # tau = 0 is kmpc_markowitz_run
        for short in (0, 1):
            assert _run(bd, _desc(short=short), u, 0.0) == _run0(bd, _desc(short=short), u), (u, short)
    assert _run(bd, _desc(short=1), 0.5, 0.2) == UNSUPPORTED
    assert _run(bd, _desc(), 0.1, 0.2) == INVALID and _run(bd, _desc(), 0.25, 0.2) == OK
    assert _run(_lib.BacktestDesc(0, 10, 12, 1e-3), _desc(), 0.0, 0.2, 0, 5) == OK     # P = 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _run(bd, _desc(), 0.0, 0.2, 0, 5) == INVALID                     # null arrays
    big = _lib.BacktestDesc(3, 129, 12, 1e-3)
    md = _desc(B=3, N=129)
    need = L.kmpc_mv_cap_workspace_bytes(ctypes.byref(md))
    assert _run(big, md, 0.0, 0.2, 0, 5, p) == WORKSPACE
    assert _run(big, md, 0.0, 0.2, 0, 5, p, p, need - 1) == WORKSPACE
    assert _run(big, md, 0.0, 0.2, 0, 5, p, p, L.kmpc_mv_workspace_bytes(ctypes.byref(md))) == WORKSPACE
    # the sweep: caps live on the device, so only the pointer is looked at
    assert _sweep(bd, _desc(), 0.0, 3) == OK and _sweep(bd, _desc(short=1), 0.0, 3) == OK
    assert _sweep(bd, _desc(), 0.0, 0) == INVALID
    assert _sweep(bd, _desc(short=1), 0.5, 3) == UNSUPPORTED
    assert _sweep(bd, _desc(), 0.0, 3, 0, 5, p, None) == INVALID            # a null cap array
    md = _desc(B=9, N=129)
    assert _sweep(big, md, 0.0, 3, 0, 5, p, p) == WORKSPACE
    assert _sweep(big, md, 0.0, 3, 0, 5, p, p, p, L.kmpc_mv_cap_workspace_bytes(ctypes.byref(md)) - 1) == WORKSPACE


def test_python_plumbing_and_value_errors():
    assert MPCConfig().mv_max_turnover == 0.0 and MPCConfig().max_turnover == 0.2
    assert _mv_turnover_cap(MPCConfig()) == 0.0                             # max_turnover is not read
    assert _mv_turnover_cap(MPCConfig(mv_max_turnover=0.3)) == 0.3
    for bad in (-0.1, NAN):
        with pytest.raises(ValueError):
            _mv_turnover_cap(MPCConfig(mv_max_turnover=bad))
    s = MarkowitzStrategy(max_turnover=0.2)
    assert s.max_turnover == 0.2 and s.mpc_config.mv_max_turnover == 0.2 and s.max_weight == 0.0
    assert s.mpc_config.max_turnover == 0.2 == MarkowitzStrategy().mpc_config.max_turnover      # the reference's field
    assert MarkowitzStrategy().max_turnover == 0.0 == MarkowitzStrategy(2.0, 0.01, False).mpc_config.mv_max_turnover
    s = MarkowitzStrategy(1.0, 1e-3, max_weight=0.25, max_turnover=0.1)
    assert (s.max_weight, s.max_turnover) == (0.25, 0.1) and _box_limit(s.mpc_config, 10) == 0.25
    s.set_max_turnover(0.0)
    assert s.mpc_config.mv_max_turnover == 0.0
    with pytest.raises(TypeError):
        MarkowitzStrategy(1.0, 0.001, False, 0.25, 0.2)                     # keywords only
    assert _mv_turnover_cap(MarkowitzStrategy(allow_short=True, max_turnover=0.2).mpc_config) == 0.2
    # the sweep's checks come before any device work (no GPU here: a device call would raise KmpcError)
    cfg = BacktestConfig(horizon=5)
    z, r = np.zeros((1, 8, 4), np.float32), np.zeros((1, 8, 4), np.float32)
    args = (z, r, cfg, np.zeros(4), np.ones(4))
    with pytest.raises(ValueError):
        pkg.run_markowitz_sweep(MarkowitzStrategy(), *args, [1.0, 2.0], [1e-3, 1e-3], max_turnovers=[0.2])
    for bad in (-0.1, NAN):
        with pytest.raises(ValueError):
            pkg.run_markowitz_sweep(MarkowitzStrategy(max_turnover=bad), *args, [1.0], [1e-3])
        with pytest.raises(ValueError):
            pkg.run_markowitz_lockstep(MarkowitzStrategy(max_turnover=bad), *args)
    with pytest.raises(ValueError, match="turnover cap"):
        sweep_backtest_markowitz(None, cfg, [MarkowitzStrategy(max_turnover=0.2), MarkowitzStrategy()])
    with pytest.raises(ValueError, match="max_weight"):
        sweep_backtest_markowitz(None, cfg, [MarkowitzStrategy(max_turnover=0.2), MarkowitzStrategy(max_turnover=0.1, max_weight=0.5)])


# ---- the references ----

def test_dense_reference_closed_form():
    """gamma = 0, c = 0, H = 1, w_prev = 1/N: tau / 2 into the best-mu asset from the worst in order."""
    for N, tau in ((8, 0.2), (8, 0.6), (5, 0.05)):
        wp, mu, S, Wc = ref.closed_form(N, tau)
        assert abs(ref.turnover(Wc, wp)[0] - tau) <= 1e-15 and abs(Wc.sum() - 1) <= 1e-15
        W, st = ref.dense_mv_cap_ipm(wp, mu, S, 0.0, 0.0, tau)
        print(f"N = {N}, tau = {tau}: dense |W - closed form| {np.abs(W - Wc).max():.3e}")
        assert st == "optimal" and np.abs(W - Wc).max() <= 1e-10     # (an LP vertex: the device is held to 1e-8)
        assert ref.gap(Wc, wp, mu, S, 0.0, 0.0, tau) <= 1e-15
    assert (Wc[0] == 0).sum() == 0 and (ref.closed_form(8, 0.6)[3][0] == 0).sum() >= 2      # 0.6: more than one donor


def test_dense_reference_is_the_project_oracle_where_the_cap_cannot_bind():
    N, H, gamma, c, tau, wp, mu, S = ref.cannot_bind()
    for b in range(len(wp)):
        W, st = ref.dense_mv_cap_ipm(wp[b], mu[b], S[b], gamma, c, tau)
        Wo, so = mv_ref.mv_dense_ipm(wp[b], mu[b], S[b], gamma, c)
        assert st == so == "optimal"
        f, fo = (ref.mv_objective(V, wp[b], mu[b], S[b], gamma, c) for V in (W, Wo))
        assert abs(f - fo) <= 1e-11


def test_infeasibility_rule_against_the_lp():
    """d0 <= tau iff the LP over the capped set has a point: long-only, under a limit, with shorting."""
    rng = np.random.default_rng(3)
    wp, u, d0 = ref.INFEASIBLE
    assert abs(ref.cap_distance(wp, u) - d0) <= 1e-15
    cases = [(wp, u, False), (np.array([0.7, 0.5, -0.2, 0.1]), None, False), (np.array([0.7, 0.5, -0.2, 0.1]), 0.6, False),
             (np.array([0.5, 0.6, -0.3, 0.1]), None, True), (rng.dirichlet(np.ones(6)), 0.2, False),
             (rng.dirichlet(np.ones(6)) * 1.1, None, False), (rng.dirichlet(np.ones(6)), None, False)]
    for wp, u, short in cases:
        d0 = ref.cap_distance(wp, u, short)
        for H in (1, 3):
            assert ref.feasible(wp, H, d0 + 1e-6, u, short), (wp, u, short)
            if d0 > 1e-6:
                assert not ref.feasible(wp, H, d0 - 1e-6, u, short), (wp, u, short)
        if d0 > 1e-6:
            W, st, it, f = ref.reduced_mv_cap_ipm(wp, np.zeros((1, len(wp))), np.eye(len(wp)), 1.0, 1e-3, 0.9 * d0, u, short)
            assert st == 2 and it == 0 and np.isnan(f) and np.array_equal(W[0], wp)
    assert ref.cap_distance(np.full(5, 0.2)) == 0.0                          # on the simplex, no limit: never infeasible


def _windows(path):
    g = np.load(path)
    gamma, c, tau, u, short = (float(v) for v in g["config"])
    for b in range(g["mu"].shape[0]):
        yield b, g["w_prev"][b], g["mu"][b], g["sigma"][b], gamma, c, tau, (u or None), bool(short), g["W"][b], float(g["obj"][b])


def test_goldens_are_the_stored_cases():
    have = {os.path.basename(p) for p in FILES}
    assert have == {"mvcap_N10_H1.npz", "mvcap_N10_H1_c0.npz", "mvcap_N10_H3_short.npz", "mvcap_N16_H8.npz", "mvcap_N43_H3.npz"}
    for p in FILES:
        assert os.path.getsize(p) < 64 * 1024


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p) for p in FILES])
def test_goldens_pinned(path):
    binds = False
    for b, wp, mu, S, gamma, c, tau, u, short, W, obj in _windows(path):
        assert not ref.violated(W, wp, tau, u, short)
        to = ref.turnover(W, wp)
        assert np.abs(W.sum(1) - 1).max() <= 1e-12 and to.max() <= tau + 1e-12 and (short or W.min() >= -1e-12)
        assert obj == mv_ref.mv_objective(W, wp, mu, S, gamma, c)
        gp = ref.gap(W, wp, mu, S, gamma, c, tau, u, short)
        print(f"{os.path.basename(path)} window {b}: gap {gp:.3e}, turnover - tau {to.max() - tau:.3e}")
        assert gp <= 1e-10
        binds = binds or abs(to[0] - tau) <= 1e-9
    assert binds          # the cap binds at exactly tau somewhere in every file


def test_certificate_rejects_a_suboptimal_portfolio_and_the_helper_holds_the_cap_bar():
    b, wp, mu, S, gamma, c, tau, u, short, W, obj = next(_windows(os.path.join(GOLD, "mvcap_N10_H1.npz")))
    V = 0.5 * W + 0.5 * wp[None, :]                                         # half the trade: feasible, worse
    assert not ref.violated(V, wp, tau, u, short)
    f = mv_ref.mv_objective(V, wp, mu, S, gamma, c)
    bad = ref.gap(V, wp, mu, S, gamma, c, tau, u, short)
    assert bad > 10 * ref.certificate_bar(f, mu, S, gamma, c, u, short) and bad >= obj - f - 1e-12
    i = int(np.argmax(W[0] - wp))
    j = int(np.argmax(np.where(W[0] - wp < -1e-3, W[0], -np.inf)))            # a seller that keeps some weight
    assert W[0, j] > 1e-3
    V = W.copy()
    V[0, i] += 1e-8
    V[0, j] -= 1e-8                                                         # 2e-8 past the cap: bar 1.1e-8
    assert any(s.startswith("turnover") for s in ref.violated(V, wp, tau, u, short))
    V[0, i] -= 0.9e-8
    V[0, j] += 0.9e-8
    assert ref.violated(V, wp, tau, u, short) == []
    assert abs(ref.cap_bar(10) - 1.1e-8) <= 1e-20
    # mcon counts the H cap rows: n sign rows + 2n |d| rows (+ n limit rows) + H
    assert ref._mcon(3, 10, None, False) == 93 and ref._mcon(3, 10, 0.5, False) == 123 and ref._mcon(3, 10, None, True) == 63


# ---- the kernel's algorithm, in numpy, on the inputs of the device tests ----

def _held(tag, wp, mu, S, gamma, c, tau, u, short, fref=None, max_it=25):
    """reduced_mv_cap_ipm on one window, held to the device tests' bars."""
    W, st, it, f = ref.reduced_mv_cap_ipm(wp, mu, S, gamma, c, tau, u, short)
    gp = ref.gap(W, wp, mu, S, gamma, c, tau, u, short)
    bar = ref.certificate_bar(f, mu, S, gamma, c, u, short)
    ex = ref.turnover(W, wp).max() - tau
    print(f"{tag}: status {st}, {it} iterations, turnover - tau {ex:.3e} (bar {ref.cap_bar(len(wp)):.3e}), gap {gp:.3e} "
          f"(bar {bar:.3e})" + ("" if fref is None else f", |f - f*| {abs(f - fref):.3e} (bar {ref.objective_bar(fref):.3e})"))
    assert st == 0 and it <= max_it
    assert not ref.violated(W, wp, tau, u, short), ref.violated(W, wp, tau, u, short)
    assert gp <= bar
    if fref is not None:
        assert abs(f - fref) <= ref.objective_bar(fref)
    return W, f


def _dense_value(wp, mu, S, gamma, c, tau, u, short):
    Wd, sd = ref.dense_mv_cap_ipm(wp, mu, S, gamma, c, tau, u, short)
    assert sd == "optimal"
    return mv_ref.mv_objective(Wd, wp, mu, S, gamma, c), Wd


def test_reduced_iteration_reaches_the_bars_on_the_goldens():
    for path in FILES:
        for b, wp, mu, S, gamma, c, tau, u, short, W, obj in _windows(path):
            _held(f"{os.path.basename(path)} window {b}", wp, mu, S, gamma, c, tau, u, short, obj)


@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_reduced_iteration_reaches_the_bars_on_the_device_cases(case):
    N, H, gamma, c, tau, u, short, B = case
    wp, mu, S = ref.case_inputs(case)
    binds = 0
    for b in range(B):
        fref = _dense_value(wp[b], mu[b], S[b], gamma, c, tau, u, short)[0] if N * H <= 600 else None
        W, f = _held(f"{ref.case_id(case)} window {b}", wp[b], mu[b], S[b], gamma, c, tau, u, short, fref)
        binds += abs(ref.turnover(W, wp[b])[0] - tau) <= 1e-6
        if u:
            assert W.max() <= u + 1e-9
    assert binds >= B - 1          # (a vertex start may already sit on the best asset)


def test_reduced_iteration_on_the_edges_and_closed_forms():
    for name, wp, mu, S, gamma, c, tau, u, short in ref.edge_cases():
        fref, Wd = _dense_value(wp, mu, S, gamma, c, tau, u, short)
        W, f = _held(name, wp, mu, S, gamma, c, tau, u, short, fref)
        assert abs(ref.turnover(Wd, wp)[0] - tau) <= 1e-9, name              # the cap binds at exactly tau
        if tau == 1e-6:
            assert np.abs(W[0] - wp).max() <= tau and ref.turnover(W, wp).max() <= tau + ref.cap_bar(len(wp))
    N, H, gamma, c, tau, wp, mu, S = ref.cannot_bind()
    for b in range(len(wp)):
        Wo, so = mv_ref.mv_dense_ipm(wp[b], mu[b], S[b], gamma, c)
        assert so == "optimal"
        _held(f"cannot bind, window {b}", wp[b], mu[b], S[b], gamma, c, tau, None, False,
              mv_ref.mv_objective(Wo, wp[b], mu[b], S[b], gamma, c))
    for N, tau in ((8, 0.2), (8, 0.6)):
        wp, mu, S, Wc = ref.closed_form(N, tau)
        W, f = _held(f"closed form, tau = {tau}", wp, mu, S, 0.0, 0.0, tau, None, False)
        print(f"closed form, tau = {tau}: |W - closed form| {np.abs(W - Wc).max():.3e}")
        assert np.abs(W - Wc).max() <= 1e-8
    for name in ("mvcap_N10_H1.npz", "mvcap_N43_H3.npz"):
        wp, mu, S, gamma, c, tau, u = ref.neighbour_windows(os.path.join(GOLD, name))
        for b in (0, 2, 4):
            _held(f"{name} neighbour {b}", wp[b], mu[b], S[b], gamma, c, tau, u, False)
        assert ref.reduced_mv_cap_ipm(wp[3], mu[3], S[3], gamma, c, tau, u)[1] == 2
        E = 0.6 * tau
        _held(f"{name} window 3 under tau = 2E + 1e-3", wp[3], mu[3], S[3], gamma, c, 2 * E + 1e-3, u, False)
    g = np.load(os.path.join(GOLD, "mvcap_N10_H3_short.npz"))
    assert g["W"][0].min() < -1e-3                                              # (the drop-in test's window does short)


def test_reduced_iteration_on_the_markowitz_windows_and_the_uncapped_run_trades_more():
    """The stored moments of markowitz_N10.npz under tau = 0.2 (gamma = 1, c = 1e-3), as
    MarkowitzStrategy(max_turnover=0.2) solves them; and the uncapped 12-step backtest on the first
    14 rows of that panel (the device test's run) has steps far above 0.2."""
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    rows = np.flatnonzero(d["valid"] == 1)
    assert len(rows) >= 4
    for b in rows:
        wp, mu, S = d["w_prev"][b], d["mu"][b][None], d["sigma"][b]
        fref, Wd = _dense_value(wp, mu, S, 1.0, 1e-3, 0.2, None, False)
        _held(f"markowitz window {b}", wp, mu, S, 1.0, 1e-3, 0.2, None, False, fref)
    hist, _ = markowitz_backtest_ref(d["z"][:14], d["mean"], d["std"], 14, 2)
    assert len(hist) == 12
    print(f"uncapped turnover per step: {np.round(hist[:, 2], 3).tolist()}")
    assert hist[:, 2].max() > 1.0 and (hist[:, 2] > 0.2).sum() >= 2
