"""The band form of the mean-variance solve on the device (kmpc_solve_mv_band through
solve_mpc_mean_variance_banded[_batched]): every shape of mv_band_ref.SHAPES under every constraint
set of mv_band_ref.SETS — the four (BOX, CAP) instantiations in both storage variants — with shared
and per-window Sigma, against the project's mean-variance bars.

Bars: the objective within 1e-9 + 1e-7 |f*| (mv_cap_ref.objective_bar) of the dense numpy reference
where it runs (n <= 600), and of the dense kernel (solve_mpc_mean_variance_batched: kmpc_solve_mv_ws /
_box / _cap) on the same float32-representable forecasts at every shape — within twice that bar past
n = 600, where the dense kernel is the only reference; budget and bounds 1e-9; the cap within
mv_cap_ref.cap_bar; the reported value equal to f(W) to 1e-12 relative; every window's status equal
to the dense kernel's."""
import functools

import numpy as np
import pytest
import torch

import mv_band_ref as band
import mv_box_ref
import mv_cap_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import (MPCConfig, solve_mpc_mean_variance, solve_mpc_mean_variance_banded,
                                                   solve_mpc_mean_variance_banded_batched,
                                                   solve_mpc_mean_variance_batched)
from oracle import mv_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _cfg(H, gamma, c, tau, u, short):
    return MPCConfig(horizon=H, gamma=float(gamma), cost_coeff=float(c), max_weight=float(u or 0.0),
                     allow_short=bool(short), mv_max_turnover=float(tau))


def _band(wp, y, S, gamma, c, tau, u=None, short=False, full=True):
    """A batch through the band entry: (W, status, value, iters) as numpy. S [B, N, N] or [N, N]."""
    y = np.asarray(y, np.float32)
    out = solve_mpc_mean_variance_banded_batched(
        torch.tensor(np.asarray(wp, np.float64), device=DEV), torch.tensor(y, device=DEV),
        torch.tensor(np.asarray(S, np.float64), device=DEV), _cfg(y.shape[1], gamma, c, tau, u, short),
        return_full=full, with_iters=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _dense(wp, y, S, gamma, c, tau, u=None, short=False, full=True):
    """The same batch through the dense kernels, on the forecasts widened to float64."""
    y = np.asarray(y, np.float32).astype(np.float64)
    out = solve_mpc_mean_variance_batched(
        torch.tensor(np.asarray(wp, np.float64), device=DEV), torch.tensor(y, device=DEV),
        torch.tensor(np.asarray(S, np.float64), device=DEV), _cfg(y.shape[1], gamma, c, tau, u, short),
        return_full=full, with_iters=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def _numpy_value(shape, name, b, shared):
    """f* of one window by the dense numpy reference of its constraint set (n <= 600), once."""
    N, H, gamma, c, tau, u, short, B = cs = band.case(shape, name)
    wp, y, S = band.case_inputs(cs)
    mu, Sb = y[b].astype(np.float64), S[0 if shared else b]
    if tau:
        Wd, sd = ref.dense_mv_cap_ipm(wp[b], mu, Sb, gamma, c, tau, u, short)
    elif u:
        Wd, sd = mv_box_ref.dense_mv_box_ipm(wp[b], mu, Sb, gamma, c, u)
    else:
        Wd, sd = mv_ref.mv_dense_ipm(wp[b], mu, Sb, gamma, c, allow_short=short)
    assert sd == "optimal", (shape, name, b, sd)
    return mv_ref.mv_objective(Wd, wp[b], mu, Sb, gamma, c)


def _feasible(tag, W, wp, tau, u, short):
    if tau:
        assert not ref.violated(W, wp, tau, u, short), (tag, ref.violated(W, wp, tau, u, short))
        return
    assert np.isfinite(W).all(), tag
    assert np.abs(W.sum(1) - 1).max() <= 1e-9, (tag, np.abs(W.sum(1) - 1).max())
    if not short:
        assert W.min() >= -1e-9, (tag, W.min())
    if u:
        assert W.max() <= u + 1e-9, (tag, W.max() - u)


CASES = [(s, n) for s in band.SHAPES for n in band.SETS]


@pytest.mark.parametrize("shape,name", CASES, ids=[f"N{s[0]}_H{s[1]}_{n}" for s, n in CASES])
def test_every_shape_and_constraint_set(shape, name):
    N, H, gamma, c, tau, u, short, B = cs = band.case(shape, name)
    wp, y, S = band.case_inputs(cs)
    shared = (CASES.index((shape, name)) % 2) == 0        # shared and per-window Sigma take turns
    Sin = S[0] if shared else S
    W, st, val, it = _band(wp, y, Sin, gamma, c, tau, u, short)
    Wd, std, vald, itd = _dense(wp, y, Sin, gamma, c, tau, u, short)
    print(f"N{N}_H{H}_{name}: storage {'LDS' if band.in_lds(N, H, bool(tau)) else 'workspace'}, "
          f"{'shared' if shared else 'per-window'} Sigma, status {st.tolist()} (dense {std.tolist()}), "
          f"iterations {it.tolist()} (dense {itd.tolist()}), max |f - f_dense| {np.abs(val - vald).max():.3e}")
    assert np.array_equal(st, std), (st, std)
    assert (st == 0).all(), st
    assert np.abs(it - itd).max() <= 1, (it, itd)
    for b in range(B):
        tag = f"N{N}_H{H}_{name} window {b}"
        mu, Sb = y[b].astype(np.float64), S[0 if shared else b]
        f = mv_ref.mv_objective(W[b], wp[b], mu, Sb, gamma, c)
        assert abs(val[b] - f) <= 1e-12 * (1 + abs(f)), (tag, val[b], f)     # the reported value is f(W)
        _feasible(tag, W[b], wp[b], tau, u, short)
        bar = ref.objective_bar(vald[b])
        assert abs(val[b] - vald[b]) <= (bar if N * H <= 600 else 2 * bar), (tag, val[b], vald[b])
        if N * H <= 600:
            fref = _numpy_value(shape, name, b, shared)
            print(f"{tag}: |f - f*| {abs(val[b] - fref):.3e} (bar {ref.objective_bar(fref):.3e})")
            assert abs(val[b] - fref) <= ref.objective_bar(fref), (tag, val[b], fref)
    W0, st0, val0, _ = _band(wp, y, Sin, gamma, c, tau, u, short, full=False)            # return_full off
    assert np.array_equal(W0, W[:, 0]) and np.array_equal(st0, st) and np.array_equal(val0, val)


@pytest.mark.parametrize("shape", [(10, 5, 4), (65, 2, 3)], ids=["lds", "workspace"])
def test_shared_sigma_is_the_per_window_call_with_it_repeated(shape):
    cs = band.case(shape, "limit_cap")
    N, H, gamma, c, tau, u, short, B = cs
    wp, y, S = band.case_inputs(cs)
    one = _band(wp, y, S[0], gamma, c, tau, u)
    rep = _band(wp, y, np.repeat(S[:1], B, 0), gamma, c, tau, u)
    for a, b in zip(one, rep):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", [(10, 5, 4), (62, 2, 3)], ids=["lds", "workspace"])
@pytest.mark.parametrize("where", ["yhat", "sigma", "w_prev"])
def test_a_nan_window_reports_solver_error_and_leaves_its_neighbours(shape, where):
    cs = band.case(shape, "cap")
    N, H, gamma, c, tau, u, short, B = cs
    wp, y, S = band.case_inputs(cs)
    wp, y, S = wp.copy(), y.copy(), S.copy()
    {"yhat": y, "sigma": S, "w_prev": wp}[where][(1,) + (0,) * ({"yhat": 2, "sigma": 2, "w_prev": 1}[where])] = np.nan
    W, st, val, _ = _band(wp, y, S, gamma, c, tau)
    _, std, _, _ = _dense(wp, y, S, gamma, c, tau)
    assert np.array_equal(st, std) and st[1] == 4 and (np.delete(st, 1) == 0).all(), (st, std)
    assert np.array_equal(W[1], np.tile(wp[1], (H, 1)), equal_nan=True) and np.isnan(val[1])
    for b in (0, 2):
        Wb, sb, vb, _ = _band(wp[b:b + 1], y[b:b + 1], S[b:b + 1], gamma, c, tau)
        assert np.array_equal(Wb[0], W[b]) and vb[0] == val[b] and sb[0] == 0


@pytest.mark.parametrize("H,N_pad", [(2, 2), (4, 96)], ids=["lds", "workspace"])
def test_d0_past_the_cap_under_a_limit_is_infeasible_and_holds(H, N_pad):
    """w_prev = [0.5, 0.3, 0.1, 0.1] under u = 0.25: d0 = 0.6 > tau = 0.2 (mv_cap_ref.INFEASIBLE),
    between two feasible windows; padded with zero-weight assets (N u > 1; the workspace variant)."""
    w_bad, u, d0 = ref.INFEASIBLE
    N = len(w_bad) + N_pad
    rng = np.random.default_rng(7)
    y = rng.normal(5e-4, 0.01, (3, H, N)).astype(np.float32)
    A = rng.normal(0, 0.01, (N + 5, N))
    S = A.T @ A / (N + 5) + 1e-6 * np.eye(N)
    ok = np.full(N, 1.0 / N)
    wp = np.stack([ok, np.concatenate([w_bad, np.zeros(N_pad)]), ok])
    assert abs(ref.cap_distance(wp[1], u) - d0) <= 1e-12 and (not band.in_lds(N, H, True)) == (N_pad > 2)
    W, st, val, _ = _band(wp, y, S, 1.0, 1e-3, 0.2, u)
    _, std, _, _ = _dense(wp, y, S, 1.0, 1e-3, 0.2, u)
    assert st.tolist() == [0, 2, 0] and np.array_equal(st, std), (st, std)
    assert np.array_equal(W[1], np.tile(wp[1], (H, 1))) and np.isnan(val[1])
    for b in (0, 2):
        assert not ref.violated(W[b], wp[b], 0.2, u)


def test_no_curvature_no_cost_shorting_is_unbounded_or_flat():
    N, H = 6, 3
    rng = np.random.default_rng(3)
    y = rng.normal(0, 0.01, (2, H, N)).astype(np.float32)
    y[1] = np.float32(2e-3) * np.arange(1, H + 1, dtype=np.float32)[:, None]     # flat inside every period
    wp = np.stack([np.full(N, 1.0 / N), np.linspace(0.3, 0.1, N) / np.linspace(0.3, 0.1, N).sum()])
    S = np.eye(N) * 1e-4
    W, st, val, _ = _band(wp, y, S, 0.0, 0.0, 0.0, None, True)
    Wd, std, vald, _ = _dense(wp, y, S, 0.0, 0.0, 0.0, None, True)
    assert st.tolist() == [3, 0] and np.array_equal(st, std), (st, std)
    assert np.array_equal(W[0], np.tile(wp[0], (H, 1))) and np.isnan(val[0])
    assert np.array_equal(W[1], Wd[1]) and val[1] == vald[1]


def test_drop_in_api():
    cs = band.case((10, 5, 4), "limit_cap")
    N, H, gamma, c, tau, u, short, B = cs
    wp, y, S = band.case_inputs(cs)
    cfg = _cfg(H, gamma, c, tau, u, short)
    W, info = solve_mpc_mean_variance_banded(wp[0], y[0].astype(np.float64), S[0], cfg)       # float64 in: rounded
    Wd, infod = solve_mpc_mean_variance(wp[0], y[0].astype(np.float64), S[0], cfg)
    assert W.shape == (H, N) and W.dtype == np.float64 and set(info) == {"status", "value"}
    assert info["status"] == infod["status"] == "optimal"
    assert abs(info["value"] - infod["value"]) <= ref.objective_bar(infod["value"])
    Wb, stb, vb = solve_mpc_mean_variance_banded(wp, y, S, cfg)                                   # batched inputs
    assert tuple(Wb.shape) == (B, H, N) and np.array_equal(Wb[0].cpu().numpy(), W) and float(vb[0]) == info["value"]
    w_bad, ub, _ = ref.INFEASIBLE
    w_bad = np.concatenate([w_bad, np.zeros(2)])                                                  # (N u > 1)
    Wi, infoi = solve_mpc_mean_variance_banded(w_bad, y[0, :2, :6], S[0][:6, :6], _cfg(2, 1.0, 1e-3, 0.2, ub, False))
    assert infoi == {"status": "infeasible"} and np.array_equal(Wi, np.tile(w_bad, (2, 1)))
    cfg2 = _cfg(H, gamma, c, tau, u, short)
    cfg2.max_turnover = 1e-9                                                                     # the log-utility solve's: unread
    W2, info2 = solve_mpc_mean_variance_banded(wp[0], y[0], S[0], cfg2)
    assert np.array_equal(W2, W) and info2 == info
