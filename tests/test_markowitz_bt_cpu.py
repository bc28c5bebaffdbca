"""The Markowitz device backtest (kmpc_rolling_moments_paths, kmpc_markowitz_run, kmpc_markowitz_sweep;
run_markowitz_lockstep / run_markowitz_sweep / sweep_backtest_markowitz) without a GPU: the symbols,
the argument and shape rules of the C ABI (every one returns before any launch), the argument checks
of the Python entries (raised before any device work), and the independent numpy restatement of the
whole loop that tests/test_markowitz_bt_gpu.py compares the device against, pinned here on the stored
windows of tests/golden/markowitz_N10.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import _lib
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy
from oracle import mv_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("kmpc_rolling_moments_paths", "kmpc_markowitz_run", "kmpc_markowitz_sweep")


# ---- the numpy restatement (the GPU file's independent reference) -------------------------------

def markowitz_target(R, t, w, gamma, cost, lookback=60):
    """MarkowitzStrategy.rebalance (baselines.py:48-106) on the float32 return history R [T, N]:
    rows [0, t], hold with fewer than 5 (baselines.py:76-78), else the moments of the last `lookback`
    rows (baselines.py:81-88) and W[0] of the H = 1 mean-variance program (oracle/mv_ref.py).
    Returns (target, moments or None)."""
    m = mv_ref.rolling_moments(R[:t + 1], lookback)
    if m is None:
        return np.asarray(w, np.float64), None
    W, _ = mv_ref.solve_mpc_mean_variance_ref(w, m[0].reshape(1, -1), m[1], gamma, cost)
    return W[0], m


def markowitz_backtest_ref(z, mean, std, n_rows, horizon, freq=1, capital=10000.0, bt_cost=1e-3, gamma=1.0,
                           cost=1e-3, lookback=60):
    """run_backtest (backtest.py:133-219) with a MarkowitzStrategy on one panel: z [T, N] float32
    standardized rows, r = z * std + mean in float32 (data_finance.py:740-742) both the strategy's
    history and the realized log-returns. Returns (hist [S, 4]: portfolio_value, return, turnover,
    cost; targets [S, N])."""
    R = np.asarray(z, np.float32) * np.asarray(std, np.float32) + np.asarray(mean, np.float32)
    N = R.shape[1]
    w = np.ones(N) / N
    value = float(capital)
    hist, targets = [], []
    for t in range(0, n_rows - horizon, freq):
        target, _ = markowitz_target(R, t, w, gamma, cost, lookback)
        turnover = np.sum(np.abs(target - w))
        c = bt_cost * turnover * value
        w = target
        value -= c
        port = 0.0
        if t + 1 < len(R):
            rr = np.exp(R[t + 1]) - 1.0
            port = np.sum(w * rr)
            value *= (1.0 + port)
            denom = 1.0 + port
            if abs(denom) < 1e-8:
                denom = 1e-8
            w = w * (1.0 + rr) / denom
        hist.append([value, port, turnover, c])
        targets.append(target)
    return np.array(hist), np.array(targets)


def test_restatement_on_the_golden_windows():
    """The restatement's window against the stored mu / sigma / valid / W0 of markowitz_N10.npz, at
    tests/test_mv_cpu.py's tolerances (mu exact, Sigma 1e-18, the optimum 1e-9)."""
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    R = d["z"] * d["std"] + d["mean"]
    assert R.dtype == np.float32
    for b, t in enumerate(d["ts"]):
        target, m = markowitz_target(R, int(t), d["w_prev"][b], 1.0, 1e-3)
        assert (m is not None) == bool(d["valid"][b])
        if m is None:
            assert np.array_equal(target, d["w_prev"][b])
            continue
        assert m[0].dtype == np.float32 and np.array_equal(m[0].astype(np.float64), d["mu"][b])
        assert np.allclose(m[1], d["sigma"][b], rtol=0, atol=1e-18)
        assert np.abs(target - d["W0"][b]).max() < 1e-9


def test_restatement_loop_holds_then_trades():
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    T, hz = 12, 5
    hist, targets = markowitz_backtest_ref(d["z"][:T], d["mean"], d["std"], T + hz, hz)
    assert hist.shape == (T, 4) and targets.shape == (T, 10)
    assert np.array_equal(hist[:4, 2], np.zeros(4)) and np.array_equal(hist[:4, 3], np.zeros(4))   # t + 1 < 5: hold
    assert hist[4, 2] > 1e-3 and hist[4, 3] == pytest.approx(1e-3 * hist[4, 2] * hist[3, 0], rel=1e-12)
    assert hist[-1, 1] == 0.0                              # the last step has no t + 1
    assert np.abs(targets.sum(1) - 1).max() < 1e-9 and targets.min() > -1e-9
    h2, _ = markowitz_backtest_ref(d["z"][:23], d["mean"], d["std"], 23 + hz, hz, freq=2)
    assert len(h2) == 12 and np.array_equal(h2[:2, 2], np.zeros(2)) and h2[2, 2] > 1e-3


# ---- the C ABI ------------------------------------------------------------------------------------

def test_symbols_exported_and_versions():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"
    for name in ("run_markowitz_lockstep", "run_markowitz_sweep", "sweep_backtest_markowitz"):
        assert callable(getattr(pkg, name))
    from koopman_mpc_portfolio_rebalancing_amd.compat import baselines as shim
    assert shim.run_markowitz_lockstep is pkg.run_markowitz_lockstep


def _descs(N=10, H=1, P=4, S=20, **kw):
    md = _lib.MvDesc()
    md.B, md.N, md.H, md.gamma, md.cost_coeff = 0, N, H, 1.0, 1e-3
    for k, v in kw.items():
        setattr(md, k, v)
    return _lib.BacktestDesc(P, N, S, 1e-3), md


_HOST = (ctypes.c_double * 8)()   # never read: every call below returns before a launch
_PTR = ctypes.addressof(_HOST)


def _run(bd, md, u=0.0, step0=0, n_steps=0, arrays=False, ws=None, ws_bytes=0):
    lib = _lib.load()
    a = _PTR if arrays else None
    byref = lambda x: ctypes.byref(x) if x is not None else None
    return lib.kmpc_markowitz_run(byref(bd), byref(md), u, step0, n_steps, a, a, a, a, 0, a, a, a, a, a, a, ws,
                                  ws_bytes, None)


def _sweep(bd, md, n_cfg, u=0.0, step0=0, n_steps=0, arrays=False, params=True):
    lib = _lib.load()
    a = _PTR if arrays else None
    p = _PTR if params else None
    byref = lambda x: ctypes.byref(x) if x is not None else None
    return lib.kmpc_markowitz_sweep(byref(bd), byref(md), u, n_cfg, p, p, p, step0, n_steps, a, a, a, a, 0, a, a, a, a,
                                    a, a, None, 0, None)


def test_run_argument_errors():
    bd, md = _descs()
    assert _run(bd, md) == 0                                   # the n_steps = 0 probe
    assert _run(None, md) == -1 and _run(bd, None) == -1       # null descriptors
    assert _run(bd, _descs(return_full_W=1)[1]) == -1
    assert _run(bd, _descs(N=11)[1]) == -1                     # the two descs disagree on N
    assert _run(bd, md, step0=15, n_steps=6) == -1             # step0 + n_steps > S
    assert _run(bd, md, n_steps=2) == -1                       # null arrays with work to do
    bd0, _ = _descs(P=0)
    assert _run(bd0, md, n_steps=2) == 0                       # no paths: nothing to do


@pytest.mark.parametrize("N,H,expect", [(1024, 1, 0), (1025, 1, -2), (64, 16, 0), (60, 17, -2), (128, 1, 0),
                                        (129, 1, 0), (40, 2, 0), (300, 1, 0)])
def test_shape_probe(N, H, expect):
    bd, md = _descs(N=N, H=H)
    assert _run(bd, md) == expect
    assert _sweep(bd, md, 3) == expect


def test_sweep_argument_errors():
    bd, md = _descs()
    assert _sweep(bd, md, 3) == 0
    assert _sweep(bd, md, 0) == -1 and _sweep(bd, md, -2) == -1   # n_cfg < 1
    assert _sweep(bd, md, 1 << 30) == -1                          # n_cfg * P past an int
    assert _sweep(None, md, 3) == -1 and _sweep(bd, None, 3) == -1
    assert _sweep(bd, _descs(return_full_W=1)[1], 3) == -1
    assert _sweep(bd, md, 3, n_steps=2, arrays=True, params=False) == -1   # null parameter arrays
    assert _sweep(bd, md, 0, u=float("nan")) == -1


def test_max_weight_rules_in_solve_mv_box_order():
    """0: none. Otherwise kmpc_solve_mv_box's order: the desc, then NaN / <= 0 invalid, then
    allow_short unsupported, then >= 1 inactive, then N u <= 1 invalid."""
    lib = _lib.load()
    bd, md = _descs(N=10)
    short = _descs(N=10, allow_short=1)[1]
    big = _descs(N=1025)[1]
    bdb = _lib.BacktestDesc(4, 1025, 20, 1e-3)
    for call in (_run, lambda b, m, u: _sweep(b, m, 3, u=u)):
        assert call(bd, md, 0.0) == 0 and call(bd, short, 0.0) == 0
        assert call(bd, md, float("nan")) == -1 and call(bd, md, -0.5) == -1
        assert call(bdb, big, float("nan")) == -2          # the shape comes first
        assert call(bd, short, float("nan")) == -1         # invalid before unsupported
        assert call(bd, short, 0.5) == -2 and call(bd, short, 2.0) == -2
        assert call(bd, md, 1.0) == 0 and call(bd, md, 7.0) == 0
        assert call(bd, md, 0.1) == -1 and call(bd, md, 0.05) == -1   # N u <= 1
        assert call(bd, md, 0.1000001) == 0 and call(bd, md, 0.2) == 0
    # the same codes as kmpc_solve_mv_box itself gives (B = 0: before any launch there too)
    for m, u in ((md, float("nan")), (md, -0.5), (short, 0.5), (md, 0.1), (md, 0.2), (md, 1.0)):
        box = lib.kmpc_solve_mv_box(ctypes.byref(m), u, None, None, 0, None, None, None, None, None, None, 0, None)
        assert _run(bd, m, u) == box


def test_workspace_rule():
    """Past H * N = 128 the Newton matrix lives in a workspace slab: KMPC_ERR_WORKSPACE without one or
    with one too small, decided before the launch; none is needed up to 128."""
    lib = _lib.load()
    bd, md = _descs(N=129)
    assert _run(bd, md, n_steps=2, arrays=True) == -3
    md.B = bd.P
    need = lib.kmpc_mv_workspace_bytes(ctypes.byref(md))
    assert need == 8 * (129 * 130 // 2 + 129) * 4
    assert _run(bd, md, n_steps=2, arrays=True, ws=_PTR, ws_bytes=need - 1) == -3
    assert _run(bd, md, u=0.2, n_steps=2, arrays=True) == -3
    assert _sweep(bd, md, 3, n_steps=2, arrays=True) == -3


def test_rolling_moments_paths_argument_errors():
    lib = _lib.load()

    def call(P=2, n_ts=3, T=20, N=4, lookback=60, ldz=4, arrays=True):
        a = _PTR if arrays else None
        return lib.kmpc_rolling_moments_paths(P, n_ts, T, N, lookback, a, ldz, a, a, a, a, a, a, None)

    assert call(P=0) == 0 and call(n_ts=0) == 0
    assert call(P=-1) == -1 and call(n_ts=-1) == -1 and call(N=0) == -1 and call(lookback=0) == -1
    assert call(ldz=3) == -1                      # rows narrower than N
    assert call(arrays=False) == -1
    assert call(P=1 << 20, n_ts=1 << 12) == -1    # P * n_ts past an int


# ---- the Python entries: errors before any device work -------------------------------------------

class _NoDevice(MarkowitzStrategy):
    def _device(self):
        raise AssertionError("device work before the argument checks")


def test_python_shape_errors():
    s = _NoDevice()
    cfg = pkg.BacktestConfig(horizon=5)
    m, sd = [0.0] * 4, [1.0] * 4
    for obs, real in ((torch.zeros(2, 12, 8), torch.zeros(3, 12, 4)),    # P differs
                      (torch.zeros(2, 12, 8), torch.zeros(2, 11, 4)),    # T differs
                      (torch.zeros(2, 12, 3), torch.zeros(2, 12, 4)),    # obs narrower than N
                      (torch.zeros(12, 8), torch.zeros(12, 4))):         # no path axis
        with pytest.raises(ValueError, match="obs must be"):
            pkg.run_markowitz_lockstep(s, obs, real, cfg, m, sd)
        with pytest.raises(ValueError, match="obs must be"):
            pkg.run_markowitz_sweep(s, obs, real, cfg, m, sd, [1.0], [1e-3])
    bad = _NoDevice(max_weight=0.2)   # N u <= 1 at N = 4
    with pytest.raises(ValueError, match="max_weight"):
        pkg.run_markowitz_lockstep(bad, torch.zeros(2, 12, 8), torch.zeros(2, 12, 4), cfg, m, sd)


def test_python_sweep_list_errors():
    s = _NoDevice()
    args = (s, torch.zeros(1, 12, 8), torch.zeros(1, 12, 4), pkg.BacktestConfig(horizon=5), [0.0] * 4, [1.0] * 4)
    with pytest.raises(ValueError, match="cost_coeffs"):
        pkg.run_markowitz_sweep(*args, [1.0, 2.0], [1e-3])
    with pytest.raises(ValueError, match="empty"):
        pkg.run_markowitz_sweep(*args, [], [])
    with pytest.raises(ValueError, match="bt_cost_coeffs"):
        pkg.run_markowitz_sweep(*args, [1.0, 2.0], [1e-3, 1e-3], bt_cost_coeffs=[1e-3])


def test_python_strategies_must_share_the_constraint_set():
    cfg = pkg.BacktestConfig()
    a = _NoDevice(1.0, 1e-3)
    with pytest.raises(ValueError, match="allow_short"):
        pkg.sweep_backtest_markowitz(None, cfg, [a, _NoDevice(2.0, 1e-3, allow_short=True)])
    with pytest.raises(ValueError, match="max_weight"):
        pkg.sweep_backtest_markowitz(None, cfg, [a, _NoDevice(2.0, 1e-2, max_weight=0.3)])
    with pytest.raises(ValueError, match="empty"):
        pkg.sweep_backtest_markowitz(None, cfg, [])
