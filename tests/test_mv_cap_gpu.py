"""The L1 turnover cap of the mean-variance solve on the device (kmpc_solve_mv_cap,
MPCConfig.mv_max_turnover through solve_mpc_mean_variance[_batched]), in both storage variants of
the CAP kernels: LDS (H N <= 128) and workspace (up to H N = 1024), with and without the position
limit and shorting, at c > 0 and c = 0.

Bars (tests/mv_cap_ref.py): the objective against the dense reference within 1e-9 + 1e-7 |f*| (the
project's mean-variance bar; the dense reference where n <= 600); the LP certificate gap within that
plus what the kernel's stopping rule allows, sc tol (mcon + 60 H), on every window; feasibility:
budget and bounds 1e-9, the cap tau + 10 tol (N + 1). tests/test_mv_cap_cpu.py holds the kernel's
algorithm, restated in numpy, to the same bars on the same inputs.

Shapes (N, H): (4, 1), (10, 1) part of one wave; (64, 2) n = 128, the last LDS shape; (8, 16) n = 128
at KMPC_MV_MAX_H (the 32 x 32 Schur system, the largest LDS footprint); (129, 1), (43, 3) the first
workspace shape; (16, 8) many periods; (300, 2); (512, 2), (64, 16) n = 1024."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import mv_cap_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import MPCConfig, solve_mpc_mean_variance, solve_mpc_mean_variance_batched, _lib
from oracle import mv_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "mvcap_*.npz")))
DEV = torch.device("cuda", 0)


def _solve(wp, mu, S, gamma, c, tau, u=None, short=False, full=True):
    """A batch through the Python entry point: (W, status, value, iters) as numpy."""
    mu = np.asarray(mu, np.float64)
    cfg = MPCConfig(horizon=mu.shape[1], gamma=float(gamma), cost_coeff=float(c), max_weight=float(u or 0.0),
                    allow_short=bool(short), mv_max_turnover=float(tau))
    out = solve_mpc_mean_variance_batched(torch.tensor(np.asarray(wp, np.float64), device=DEV), torch.tensor(mu, device=DEV),
                                          torch.tensor(np.asarray(S, np.float64), device=DEV), cfg, return_full=full,
                                          with_iters=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _one(wp, mu, S, gamma, c, tau, u=None, short=False):
    W, st, val, it = _solve(wp[None], mu[None], S[None], gamma, c, tau, u, short)
    return W[0], int(st[0]), float(val[0]), int(it[0])


def _held(tag, W, val, wp, mu, S, gamma, c, tau, u, short, fref=None):
    """One solved window against the bars, the measured figures first."""
    f = mv_ref.mv_objective(W, wp, mu, S, gamma, c)
    gp = ref.gap(W, wp, mu, S, gamma, c, tau, u, short)
    bar = ref.certificate_bar(f, mu, S, gamma, c, u, short)
    ex = ref.turnover(W, wp).max() - tau
    print(f"{tag}: turnover - tau {ex:.3e} (bar {ref.cap_bar(len(wp)):.3e}), gap {gp:.3e} (bar {bar:.3e})" +
          ("" if fref is None else f", |f - f*| {abs(val - fref):.3e} (bar {ref.objective_bar(fref):.3e})"))
    assert not ref.violated(W, wp, tau, u, short), (tag, ref.violated(W, wp, tau, u, short))
    assert abs(val - f) <= 1e-12 * (1 + abs(f)), (tag, val, f)        # the reported value is f(W), to rounding
    assert gp <= bar, (tag, gp, bar)
    if fref is not None:
        assert abs(val - fref) <= ref.objective_bar(fref), (tag, val, fref)


@functools.lru_cache(maxsize=None)
def _dense_value(key):
    """f* of one window of a case (the dense reference, n <= 600), computed once."""
    ci, b = key
    N, H, gamma, c, tau, u, short, B = ref.CASES[ci]
    wp, mu, S = ref.case_inputs(ref.CASES[ci])
    Wd, sd = ref.dense_mv_cap_ipm(wp[b], mu[b], S[b], gamma, c, tau, u, short)
    assert sd == "optimal"
    return mv_ref.mv_objective(Wd, wp[b], mu[b], S[b], gamma, c)


@pytest.mark.parametrize("ci", range(len(ref.CASES)), ids=[ref.case_id(c) for c in ref.CASES])
def test_every_shape_and_constraint_set(ci):
    case = ref.CASES[ci]
    N, H, gamma, c, tau, u, short, B = case
    wp, mu, S = ref.case_inputs(case)
    W, st, val, it = _solve(wp, mu, S, gamma, c, tau, u, short)
    print(f"{ref.case_id(case)}: status {st.tolist()}, iterations {it.tolist()}")
    assert (st == 0).all(), st
    binds = 0
    for b in range(B):
        fref = _dense_value((ci, b)) if N * H <= 600 else None
        _held(f"{ref.case_id(case)} window {b}", W[b], val[b], wp[b], mu[b], S[b], gamma, c, tau, u, short, fref)
        binds += abs(ref.turnover(W[b], wp[b])[0] - tau) <= 1e-6
    assert binds >= B - 1          # tau = 0.2 (0.05) binds; a vertex start may already sit on the best asset
    W0, st0, val0, _ = _solve(wp, mu, S, gamma, c, tau, u, short, full=False)           # return_full off
    assert np.array_equal(W0, W[:, 0]) and np.array_equal(st0, st) and np.array_equal(val0, val)
    W2, st2, val2, it2 = _solve(wp, mu, S, gamma, c, tau, u, short)                     # a relaunch
    assert np.array_equal(W2, W) and np.array_equal(val2, val) and np.array_equal(it2, it)


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p) for p in FILES])
def test_goldens_on_device(path):
    g = np.load(path)
    gamma, c, tau, u, short = (float(v) for v in g["config"])
    u, short = (u or None), bool(short)
    W, st, val, it = _solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, tau, u, short)
    assert (st == 0).all(), st
    for b in range(len(W)):
        _held(f"{os.path.basename(path)} window {b}", W[b], val[b], g["w_prev"][b], g["mu"][b], g["sigma"][b], gamma, c,
              tau, u, short, float(g["obj"][b]))


def test_edges():
    """A vertex of lowest mu, zeros in w_prev, tau = 1e-6 (long-only, a vertex, shorting), w_prev on
    and past the limit."""
    for name, wp, mu, S, gamma, c, tau, u, short in ref.edge_cases():
        W, st, val, it = _one(wp, mu, S, gamma, c, tau, u, short)
        assert st == 0, (name, st)
        Wd, sd = ref.dense_mv_cap_ipm(wp, mu, S, gamma, c, tau, u, short)
        assert sd == "optimal", name
        _held(f"{name} ({it} iterations)", W, val, wp, mu, S, gamma, c, tau, u, short, mv_ref.mv_objective(Wd, wp, mu, S, gamma, c))
        if tau == 1e-6:
            print(f"{name}: |W_0 - w_prev| {np.abs(W[0] - wp).max():.3e}")
            assert np.abs(W[0] - wp).max() <= tau


def test_cap_that_cannot_bind_is_the_plain_optimum():
    N, H, gamma, c, tau, wp, mu, S = ref.cannot_bind()
    W, st, val, _ = _solve(wp, mu, S, gamma, c, tau)
    assert (st == 0).all(), st
    Wp, stp, valp, _ = _solve(wp, mu, S, gamma, c, 0.0)                    # the plain solve on the device
    for b in range(len(wp)):
        Wo, so = mv_ref.mv_dense_ipm(wp[b], mu[b], S[b], gamma, c)
        assert so == "optimal"
        fo = mv_ref.mv_objective(Wo, wp[b], mu[b], S[b], gamma, c)
        _held(f"cannot bind, window {b}", W[b], val[b], wp[b], mu[b], S[b], gamma, c, tau, None, False, fo)
        assert abs(val[b] - valp[b]) <= 2 * ref.objective_bar(fo)


def test_closed_form():
    """gamma = 0, c = 0, H = 1, w_prev = 1/N: tau / 2 into the best-mu asset from the worst in order."""
    for N, tau in ((8, 0.2), (8, 0.6)):
        wp, mu, S, Wc = ref.closed_form(N, tau)
        W, st, val, _ = _one(wp, mu, S, 0.0, 0.0, tau)
        print(f"closed form N = {N}, tau = {tau}: |W - closed form| {np.abs(W - Wc).max():.3e}")
        assert st == 0
        _held("closed form", W, val, wp, mu, S, 0.0, 0.0, tau, None, False, mv_ref.mv_objective(Wc, wp, mu, S, 0.0, 0.0))
        assert np.abs(W - Wc).max() <= 1e-8


def _c_call(g, u, tau, entry="cap"):
    """kmpc_solve_mv_cap / kmpc_solve_mv_box / kmpc_solve_mv_ws by hand, full W, each with its own
    workspace query."""
    L = _lib.load()
    gamma, c = float(g["config"][0]), float(g["config"][1])
    B, H, N = g["mu"].shape
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff, d.allow_short, d.max_iter, d.tol, d.return_full_W = B, N, H, gamma, c, 0, 100, 1e-10, 1
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float64), device=DEV)
    mu, S, wp = t(g["mu"]), t(g["sigma"]), t(g["w_prev"])
    W = torch.zeros((B, H, N), dtype=torch.float64, device=DEV)
    st = torch.zeros(B, dtype=torch.int32, device=DEV)
    val = torch.zeros(B, dtype=torch.float64, device=DEV)
    it = torch.zeros(B, dtype=torch.int32, device=DEV)
    nws = int((L.kmpc_mv_cap_workspace_bytes if entry == "cap" and tau else L.kmpc_mv_workspace_bytes)(ctypes.byref(d)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=DEV)
    tail = (mu.data_ptr(), S.data_ptr(), N * N, wp.data_ptr(), W.data_ptr(), st.data_ptr(), val.data_ptr(), it.data_ptr(),
            ws.data_ptr(), nws, _lib.stream_handle(DEV))
    with torch.cuda.device(DEV):
        if entry == "cap":
            rc = L.kmpc_solve_mv_cap(ctypes.byref(d), u, tau, *tail)
        elif entry == "box":
            rc = L.kmpc_solve_mv_box(ctypes.byref(d), u, *tail)
        else:
            rc = L.kmpc_solve_mv_ws(ctypes.byref(d), *tail)
    torch.cuda.synchronize()
    assert rc == 0
    return W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy()


@pytest.mark.parametrize("name", ["mvcap_N10_H1.npz", "mvcap_N43_H3.npz"])   # LDS / workspace
def test_no_cap_is_the_existing_call_bit_for_bit(name):
    g = np.load(os.path.join(GOLD, name))
    plain = _c_call(g, 0.0, 0.0, "ws")
    for x, y in zip(_c_call(g, 0.0, 0.0), plain):                                      # kmpc_solve_mv_ws
        assert np.array_equal(x, y)
    u = 0.3 if g["mu"].shape[2] == 10 else 0.1
    gb = {k: (np.minimum(g[k], u) if k == "w_prev" else g[k]) for k in g.files}
    for x, y in zip(_c_call(gb, u, 0.0), _c_call(gb, u, 0.0, "box")):                  # kmpc_solve_mv_box
        assert np.array_equal(x, y)
    gamma, c, tau = (float(v) for v in g["config"][:3])
    for x, y in zip(_solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, 0.0), plain):   # mv_max_turnover = 0 in Python
        assert np.array_equal(x, y)
    capped = _c_call(g, 0.0, tau)
    for x, y in zip(_solve(g["w_prev"], g["mu"], g["sigma"], gamma, c, tau), capped):  # ... and the cap, both ways
        assert np.array_equal(x, y)
    assert np.abs(capped[0] - plain[0]).max() > 1e-3                                   # (and it is not the plain answer)


@pytest.mark.parametrize("name", ["mvcap_N10_H1.npz", "mvcap_N43_H3.npz"])   # LDS / workspace
def test_nan_and_infeasible_windows_between_solved_ones(name):
    """Window 1 carries a NaN (status 4), window 3 starts past the limit with 2E > tau (status 2: the
    fallback, value NaN); their neighbours are bit-identical to solving them alone."""
    wp, mu, S, gamma, c, tau, u = ref.neighbour_windows(os.path.join(GOLD, name))
    H, E = mu.shape[1], 0.6 * tau
    assert abs(ref.cap_distance(wp[3], u) - 2 * E) <= 1e-12 and 2 * E > tau and wp[[0, 1, 2, 4]].max() <= u
    W, st, val, _ = _solve(wp, mu, S, gamma, c, tau, u)
    assert st.tolist() == [0, 4, 0, 2, 0], st
    for b in (1, 3):
        assert np.array_equal(W[b], np.tile(wp[b], (H, 1))) and np.isnan(val[b])
    for b in (0, 2, 4):
        Wb, sb, vb, _ = _solve(wp[b:b + 1], mu[b:b + 1], S[b:b + 1], gamma, c, tau, u)
        assert np.array_equal(Wb[0], W[b]) and vb[0] == val[b] and sb[0] == 0
        assert not ref.violated(W[b], wp[b], tau, u)
    # the same start is feasible under a cap of 2E and a little: the solve moves it inside the limit
    W3, s3, v3, _ = _one(wp[3], mu[3], S[3], gamma, c, 2 * E + 1e-3, u)
    assert s3 == 0 and not ref.violated(W3, wp[3], 2 * E + 1e-3, u)


def test_drop_in_api_holds_the_cap():
    g = np.load(os.path.join(GOLD, "mvcap_N10_H3_short.npz"))
    gamma, c, tau = (float(v) for v in g["config"][:3])
    wp, mu, S = g["w_prev"][0], g["mu"][0], g["sigma"][0]
    cfg = MPCConfig(horizon=3, gamma=gamma, cost_coeff=c, allow_short=True, mv_max_turnover=tau)
    W, info = solve_mpc_mean_variance(wp, mu, S, cfg)
    assert W.shape == (3, 10) and info["status"] == "optimal" and set(info) == {"status", "value"}
    assert ref.turnover(W, wp).max() <= tau + ref.cap_bar(10) and W.min() < 0
    assert abs(info["value"] - g["obj"][0]) <= ref.objective_bar(g["obj"][0])
    W1, info1 = solve_mpc_mean_variance(wp, mu, S, MPCConfig(horizon=3, gamma=gamma, cost_coeff=c, allow_short=True))
    assert ref.turnover(W1, wp).max() > tau + 1e-2 and info1["value"] > info["value"]      # max_turnover alone: unread
    Wi, infoi = solve_mpc_mean_variance(wp * 1.5, mu, S, cfg)                              # |1 - sum| = 0.5 > tau
    assert infoi == {"status": "infeasible"} and np.array_equal(Wi, np.tile(wp * 1.5, (3, 1)))
    with pytest.raises(ValueError):
        solve_mpc_mean_variance(wp, mu, S, MPCConfig(horizon=3, mv_max_turnover=-0.1))
