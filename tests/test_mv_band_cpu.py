"""The band form of the mean-variance solve without a GPU.

* Band structure: on M built as the kernel builds it the dense Cholesky factor has nothing outside
  the band (relative to ||L||), and the numpy restatement of the kernel's band-clipped factorization
  and solves (tests/mv_band_ref.py) equals numpy.linalg.cholesky / solve to 1e-12 relative.
* Iteration parity: the kernel's reduced iteration (mv_cap_ref.reduced_mv_cap_ipm,
  mv_box_ref.reduced_mv_box_ipm) with its linear algebra replaced by the band restatement meets the
  device bars against the dense references on the inputs of tests/test_mv_band_gpu.py.
* The C boundary: the three symbols and every return-code rule of include/kmpc.h, each decided before
  a launch; the workspace query.
* Python: the exports (this part fails before the band form existed) and the ValueErrors, raised
  before any device work.
"""
import ctypes

import numpy as np
import pytest
import torch

import koopman_mpc_portfolio_rebalancing_amd as pkg
import mv_band_ref as band
import mv_box_ref
import mv_cap_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import _lib
from oracle import mv_ref

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NAN = float("nan")


# ---- exports ---------------------------------------------------------------------------------------

def test_exports_and_symbols():
    for name in ("solve_mpc_mean_variance_banded", "KoopmanMVStrategy", "run_koopman_mv_lockstep"):
        assert hasattr(pkg, name), name
    lib = _lib.load()
    for name in ("kmpc_mv_band_workspace_bytes", "kmpc_solve_mv_band", "kmpc_koopman_mv_run"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"
    from koopman_mpc_portfolio_rebalancing_amd.compat import baselines as cb, mpc as cm
    assert cm.solve_mpc_mean_variance_banded is pkg.solve_mpc_mean_variance_banded
    assert cb.KoopmanMVStrategy is pkg.KoopmanMVStrategy and cb.run_koopman_mv_lockstep is pkg.run_koopman_mv_lockstep


# ---- band structure --------------------------------------------------------------------------------

def _newton(N, H, seed):
    """M as the kernel assembles it, from a random covariance and positive barrier terms spread over
    several decades (as late interior-point iterations have them)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 1, (N + 3, N))
    S = A.T @ A / (N + 3) + 1e-3 * np.eye(N)
    diag = 10.0 ** rng.uniform(-3, 4, (H, N))
    E = 10.0 ** rng.uniform(-3, 4, (H, N))
    return band.newton_matrix(S, H, 2.0, diag, E)


@pytest.mark.parametrize("N,H", [(2, 2), (3, 16), (10, 5), (65, 2)])
def test_band_structure_and_the_restated_factorization(N, H):
    n = N * H
    M = _newton(N, H, 100 * N + H)
    assert band.bandwidth(M) == (N if H > 1 else N - 1)
    L = np.linalg.cholesky(M)
    r, c = np.indices((n, n))
    outside = np.abs(L[(r - c) > N]).max() if ((r - c) > N).any() else 0.0
    print(f"N{N}_H{H}: largest |L| outside the band {outside:.3e} of ||L|| {np.linalg.norm(L):.3e}")
    assert outside <= 1e-14 * np.linalg.norm(L)
    Lb, ok = band.band_cholesky(band.to_band(M, N), N)
    assert ok
    assert np.abs(band.from_band(Lb, N) - L).max() <= 1e-12 * np.abs(L).max()
    rng = np.random.default_rng(N)
    b = rng.normal(0, 1, (n, 3))
    x, xr = band.band_solve(Lb, N, b), np.linalg.solve(M, b)
    assert np.abs(x - xr).max() <= 1e-12 * np.abs(xr).max()
    x1 = band.band_solve(Lb, N, b[:, 0])
    assert np.array_equal(x1, x[:, 0])


def test_band_factorization_flags_a_lost_pivot():
    M = _newton(3, 4, 1)
    M[5, 5] = -1.0
    with np.errstate(all="ignore"):
        assert not band.band_cholesky(band.to_band(M, 3), 3)[1]


# ---- iteration parity ------------------------------------------------------------------------------

PARITY_SHAPES = [(2, 2, 4), (3, 16, 3), (10, 5, 4), (10, 1, 4), (13, 10, 3)]
PARITY = [(s, n, b) for s in PARITY_SHAPES for n in band.SETS for b in (0, 1)] + \
         [((65, 2, 3), n, 0) for n in ("plain", "limit_cap")]


@pytest.mark.parametrize("shape,name,b", PARITY, ids=[f"N{s[0]}_H{s[1]}_{n}_w{b}" for s, n, b in PARITY])
def test_band_iteration_meets_the_device_bars(shape, name, b):
    """One window of the device test's inputs (float32-rounded forecasts) through the kernel's reduced
    iteration with the band linear algebra. The sets without a cap run the capped restatement at
    tau = 2 long-only (no two points of the simplex are further apart: the cap cannot bind), "limit"
    the BOX restatement; "short" has no uncapped restatement and runs under tau = 0.2 against the
    capped dense reference."""
    N, H, gamma, c, tau, u, short, B = cs = band.case(shape, name)
    wp, y, S = band.case_inputs(cs)
    w0, mu, Sb = wp[b], y[b].astype(np.float64), S[b]
    log = []
    with band.banded_linalg(N, log):
        if name == "limit":
            W, st, it, f = mv_box_ref.reduced_mv_box_ipm(w0, mu, Sb, gamma, c, u)[:4]
        else:
            t = tau if tau else (0.2 if short else 2.0)
            W, st, it, f = ref.reduced_mv_cap_ipm(w0, mu, Sb, gamma, c, t, u, short)
    assert st == 0 and log.count(N * H) >= it, (st, it, log[:3])           # every Newton matrix went through the band
    if name == "limit":
        Wd, sd = mv_box_ref.dense_mv_box_ipm(w0, mu, Sb, gamma, c, u)
        assert not mv_box_ref.violated(W, u)
    elif name == "short":
        Wd, sd = ref.dense_mv_cap_ipm(w0, mu, Sb, gamma, c, 0.2, None, True)
        assert not ref.violated(W, w0, 0.2, None, True)
    elif tau:
        Wd, sd = ref.dense_mv_cap_ipm(w0, mu, Sb, gamma, c, tau, u, short)
        assert not ref.violated(W, w0, tau, u, short)
    else:
        Wd, sd = mv_ref.mv_dense_ipm(w0, mu, Sb, gamma, c)
        assert not ref.violated(W, w0, 2.0)
    assert sd == "optimal"
    fref = mv_ref.mv_objective(Wd, w0, mu, Sb, gamma, c)
    fW = mv_ref.mv_objective(W, w0, mu, Sb, gamma, c)
    print(f"{it} iterations, |f - f*| {abs(f - fref):.3e} (bar {ref.objective_bar(fref):.3e})")
    assert abs(f - fW) <= 1e-12 * (1 + abs(fW))
    assert abs(f - fref) <= ref.objective_bar(fref)


def test_band_and_dense_linear_algebra_take_the_same_iterations():
    cs = band.case((10, 5, 4), "limit_cap")
    N, H, gamma, c, tau, u, short, B = cs
    wp, y, S = band.case_inputs(cs)
    for b in range(B):
        mu = y[b].astype(np.float64)
        Wd, sd, itd, fd = ref.reduced_mv_cap_ipm(wp[b], mu, S[b], gamma, c, tau, u)
        with band.banded_linalg(N):
            Wb, sb, itb, fb = ref.reduced_mv_cap_ipm(wp[b], mu, S[b], gamma, c, tau, u)
        assert sb == sd == 0 and abs(itb - itd) <= 1 and abs(fb - fd) <= ref.objective_bar(fd)


# ---- the C boundary --------------------------------------------------------------------------------

_HOST = (ctypes.c_double * 4)()   # never read: every call here returns before a launch
_PTR = ctypes.addressof(_HOST)


def _md(N=40, H=5, B=4, **kw):
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff = B, N, H, 1.0, 1e-3
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _solve(d, u=0.0, tau=0.0, arrays=True, ws=None, nws=0, iters=True):
    p = _PTR if arrays else None
    return _lib.load().kmpc_solve_mv_band(ctypes.byref(d) if d is not None else None, p, p, 1, p, u, tau, p, p, p,
                                          p if iters else None, ws, nws, None)


def _run(bd, d, u=0.0, tau=0.0, step0=0, n_steps=0, arrays=False, n_real=0, ws=None, nws=0):
    p = _PTR if arrays else None
    ref_ = lambda x: ctypes.byref(x) if x is not None else None
    return _lib.load().kmpc_koopman_mv_run(ref_(bd), ref_(d), u, tau, step0, n_steps, p, p, p, p, n_real, p, p, p, p, p, p,
                                           ws, nws, None)


def test_workspace_query():
    L = _lib.load()
    q = lambda d, cap: int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(d), cap))
    for N, H in ((10, 5), (30, 5), (13, 10), (2, 2), (3, 16), (61, 2)):
        assert q(_md(N, H), 0) == 0 and band.in_lds(N, H, False), (N, H)
    for N, H, cap in ((10, 5, 1), (13, 10, 1), (3, 16, 1)):
        assert q(_md(N, H), cap) == 0 and band.in_lds(N, H, True)
    for N, H, B in ((62, 2, 4), (65, 2, 3), (129, 1, 4), (100, 10, 64), (100, 10, 4096), (64, 16, 2), (512, 2, 1)):
        n, slots = N * H, min(B, 512)
        assert not band.in_lds(N, H, False)
        assert q(_md(N, H, B), 0) == 8 * slots * (n * (N + 1) + H * n), (N, H)
        assert q(_md(N, H, B), 1) == 8 * slots * (n * (N + 1) + 2 * H * n), (N, H)
    assert q(_md(61, 2, 3), 1) == 8 * 3 * (122 * 62 + 4 * 122)              # the cap's columns push (61, 2) out of LDS
    assert band.lds_bytes(61, 2, False) <= 65536 < band.lds_bytes(62, 2, False)
    assert q(_md(100, 10, 0), 0) == 0 and int(L.kmpc_mv_band_workspace_bytes(None, 0)) == 0
    assert q(_md(100, 17), 0) == 0 and q(_md(1025, 1), 0) == 0              # no kernel for the shape: nothing to size


def test_solve_return_codes_in_order():
    assert _solve(None) == INVALID
    for kw in (dict(B=-1), dict(N=0), dict(H=0)):
        assert _solve(_md(**kw)) == INVALID, kw
    for N, H in ((64, 17), (1025, 1), (103, 10)):
        assert _solve(_md(N, H)) == UNSUPPORTED, (N, H)
    assert _solve(_md(64, 17), tau=NAN) == UNSUPPORTED                      # the shape before the cap
    for tau in (NAN, -0.1):
        assert _solve(_md(), tau=tau) == INVALID
        assert _solve(_md(), u=NAN, tau=tau) == INVALID
    for u in (NAN, -0.1):
        assert _solve(_md(), u=u) == INVALID
    assert _solve(_md(allow_short=1), u=0.1) == UNSUPPORTED                 # mv_box_limit's order: shorting ...
    assert _solve(_md(allow_short=1), u=1.5) == UNSUPPORTED                 # ... before the inactive bound
    assert _solve(_md(), u=1.0 / 40) == INVALID and _solve(_md(), u=0.01) == INVALID     # N u <= 1
    assert _solve(_md(B=0), u=0.1, tau=0.2, arrays=False) == OK             # nothing to do, after the rules
    assert _solve(_md(B=0), u=0.01, arrays=False) == INVALID
    assert _solve(_md(), arrays=False) == INVALID                           # null arrays with work to do
    # past the LDS variant: the workspace, asked for before any launch
    d = _md(100, 10, 2)
    need = int(_lib.load().kmpc_mv_band_workspace_bytes(ctypes.byref(d), 0))
    assert need == 8 * 2 * (1000 * 101 + 10 * 1000)
    assert _solve(d) == WORKSPACE and _solve(d, ws=_PTR, nws=need - 1) == WORKSPACE
    assert _solve(d, tau=0.2, ws=_PTR, nws=need) == WORKSPACE               # the cap's slab is larger
    assert _solve(d, u=1.5, ws=None) == WORKSPACE                           # an inactive bound: the plain band solve


def test_run_return_codes_in_order():
    S = 20
    bd = _lib.BacktestDesc(4, 40, S, 1e-3)
    d = _md()
    assert _run(bd, d) == OK                                                # the n_steps = 0 shape probe
    assert _run(None, d) == INVALID and _run(bd, None) == INVALID
    assert _run(bd, d, step0=15, n_steps=6) == INVALID and _run(bd, d, step0=-1) == INVALID
    assert _run(bd, d, n_steps=2, n_real=3) == INVALID
    assert _run(_lib.BacktestDesc(4, 41, S, 1e-3), d) == INVALID            # descriptors that disagree in N
    assert _run(bd, _md(return_full_W=1)) == INVALID
    assert _run(_lib.BacktestDesc(4, 40, S, 1e-3), _md(40, 17)) == UNSUPPORTED
    assert _run(_lib.BacktestDesc(4, 103, S, 1e-3), _md(103, 10)) == UNSUPPORTED
    for tau in (NAN, -1.0):
        assert _run(bd, d, tau=tau) == INVALID
    assert _run(bd, d, u=NAN) == INVALID and _run(bd, d, u=0.02) == INVALID
    assert _run(bd, _md(allow_short=1), u=0.1) == UNSUPPORTED
    assert _run(bd, _md(allow_short=1), tau=0.2) == OK                      # shorting under the cap alone
    assert _run(bd, d, u=0.1, tau=0.2) == OK and _run(bd, d, u=2.0) == OK
    assert _run(_lib.BacktestDesc(0, 40, S, 1e-3), d, n_steps=2) == OK      # no paths: nothing run
    assert _run(bd, d, n_steps=2) == INVALID                                # null arrays with work to do
    big = _lib.BacktestDesc(2, 100, S, 1e-3)
    assert _run(big, _md(100, 10), n_steps=2, arrays=True) == WORKSPACE
    assert _run(big, _md(100, 10)) == OK                                    # the probe needs no workspace


# ---- Python: errors before any device work ---------------------------------------------------------

def _no_device(cfg):
    """A KoopmanMVStrategy whose model and device must not be touched: the config checks come first."""
    class _NoDevice(pkg.KoopmanMVStrategy):
        def device_model(self):
            raise AssertionError("device work before the config checks")

        def _device(self):
            raise AssertionError("device work before the config checks")
    return _NoDevice(None, cfg)


class _Env:
    n_assets = 4


BAD_CONFIGS = [
    (dict(gamma=-1.0), "gamma"), (dict(gamma=NAN), "gamma"), (dict(gamma=float("inf")), "gamma"),
    (dict(max_weight=-0.1), "max_weight"), (dict(max_weight=0.25), "max_weight"),      # N u <= 1 at N = 4
    (dict(max_weight=0.5, allow_short=True), "allow_short"), (dict(mv_max_turnover=-0.1), "mv_max_turnover"),
    (dict(mv_max_turnover=NAN), "mv_max_turnover"), (dict(horizon=17), "exceeds"),
]


@pytest.mark.parametrize("fields,match", BAD_CONFIGS, ids=[m + str(i) for i, (_, m) in enumerate(BAD_CONFIGS)])
def test_python_config_errors(fields, match):
    cfg = pkg.MPCConfig(**{"horizon": 3, "gamma": 1.0, **fields})
    H, N = cfg.horizon, 4
    with pytest.raises(ValueError, match=match):
        pkg.solve_mpc_mean_variance_banded(np.full(N, 0.25), np.zeros((H, N)), np.eye(N), cfg)
    with pytest.raises(ValueError, match=match):
        pkg.solve_mpc_mean_variance_banded(np.full((2, N), 0.25), np.zeros((2, H, N)), np.eye(N), cfg)
    with pytest.raises(ValueError, match=match):
        pkg.solve_mpc_mean_variance_banded_batched(torch.full((2, N), 0.25), torch.zeros(2, H, N), torch.eye(N), cfg)
    s = _no_device(cfg)
    with pytest.raises(ValueError, match=match):
        s.rebalance(7, np.full(N, 0.25), _Env())
    with pytest.raises(ValueError, match=match):
        pkg.run_koopman_mv_lockstep(s, torch.zeros(2, 12, 8), torch.zeros(2, 12, N), pkg.BacktestConfig(horizon=5),
                                    [0.0] * N, [1.0] * N)


def test_python_shape_errors():
    cfg = pkg.MPCConfig(horizon=3, gamma=1.0)
    with pytest.raises(ValueError, match="exceeds"):
        pkg.solve_mpc_mean_variance_banded(np.full(600, 1 / 600), np.zeros((2, 600)), np.eye(600), cfg)
    with pytest.raises(ValueError, match=r"\[H, N\]"):
        pkg.solve_mpc_mean_variance_banded(np.full(4, 0.25), np.zeros(4), np.eye(4), cfg)
    with pytest.raises(ValueError, match="current_weights"):
        pkg.solve_mpc_mean_variance_banded_batched(torch.zeros(3, 4), torch.zeros(2, 3, 4), torch.eye(4), cfg)
    with pytest.raises(ValueError, match="cov_matrix"):
        pkg.solve_mpc_mean_variance_banded_batched(torch.zeros(2, 4), torch.zeros(2, 3, 4), torch.eye(5), cfg)
    s = _no_device(cfg)
    bt, m, sd = pkg.BacktestConfig(horizon=5), [0.0] * 4, [1.0] * 4
    for obs, real in ((torch.zeros(2, 12, 8), torch.zeros(3, 12, 4)), (torch.zeros(2, 12, 8), torch.zeros(2, 11, 4)),
                      (torch.zeros(2, 12, 3), torch.zeros(2, 12, 4)), (torch.zeros(12, 8), torch.zeros(12, 4))):
        with pytest.raises(ValueError, match="obs must be"):
            pkg.run_koopman_mv_lockstep(s, obs, real, bt, m, sd)
    with pytest.raises(ValueError, match="mean and std"):
        pkg.run_koopman_mv_lockstep(s, torch.zeros(2, 12, 8), torch.zeros(2, 12, 4), bt, [0.0] * 3, sd)
