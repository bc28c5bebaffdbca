"""The sweep of the mean-variance Koopman-MPC backtest without a GPU.

* Exports: run_koopman_mv_sweep and sweep_backtest_koopman_mv in the package and the compat module, the
  symbol kmpc_koopman_mv_sweep in the library (this part fails before the sweep existed).
* The C boundary: every return-code rule of include/kmpc.h in its order, each decided before a launch.
* Python: the ValueErrors, raised before any device work.
* Grouping: the configs' (limit, cap) forms, and the scatter back into the configs' order.
"""
import ctypes

import pytest
import torch

import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import _lib, baselines

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NAN = float("nan")


def test_exports_and_symbol():
    for name in ("run_koopman_mv_sweep", "sweep_backtest_koopman_mv"):
        assert hasattr(pkg, name), name
    from koopman_mpc_portfolio_rebalancing_amd.compat import baselines as cb
    assert cb.run_koopman_mv_sweep is pkg.run_koopman_mv_sweep
    assert cb.sweep_backtest_koopman_mv is pkg.sweep_backtest_koopman_mv
    assert "run_koopman_mv_sweep" in baselines.__all__ and "sweep_backtest_koopman_mv" in baselines.__all__
    lib = _lib.load()
    assert "kmpc_koopman_mv_sweep" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "kmpc_koopman_mv_sweep")
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__                  # a new function within the ABI
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"


# ---- the C boundary --------------------------------------------------------------------------------

_HOST = (ctypes.c_double * 4)()   # never read: every call here returns before a launch
_PTR = ctypes.addressof(_HOST)


def _md(N=40, H=5, **kw):
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff = 0, N, H, 1.0, 1e-3
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _sweep(bd, d, n_cfg=3, cfg=True, limit=False, cap=False, step0=0, n_steps=0, arrays=False, n_real=0, ws=None,
           nws=0, **null):
    """kmpc_koopman_mv_sweep with host placeholders for the arrays it must not read. cfg / arrays: the
    three config arrays / the data arrays set; limit / cap: the two optional config arrays set; null:
    names of single arrays to pass as NULL."""
    ref = lambda x: ctypes.byref(x) if x is not None else None
    c, a = (_PTR if cfg else None), (_PTR if arrays else None)
    p = dict(gamma=c, mv_cost=c, bt_cost=c, yhat=a, sigma=a, valid=a, realized=a, weights=a, value=a, hist=a,
             target=a, status=a, obj=a)
    for k in null:
        p[k] = None
    return _lib.load().kmpc_koopman_mv_sweep(
        ref(bd), ref(d), n_cfg, p["gamma"], p["mv_cost"], p["bt_cost"], _PTR if limit else None, _PTR if cap else None,
        step0, n_steps, p["yhat"], p["sigma"], p["valid"], p["realized"], n_real, p["weights"], p["value"], p["hist"],
        p["target"], p["status"], p["obj"], ws, nws, None)


def test_return_codes_in_order():
    S = 20
    bd = _lib.BacktestDesc(4, 40, S, 1e-3)
    d = _md()
    assert _sweep(bd, d) == OK                                               # the n_steps = 0 shape probe
    assert _sweep(bd, d, limit=True, cap=True) == OK
    # the descriptor rules of kmpc_koopman_mv_run
    assert _sweep(None, d) == INVALID and _sweep(bd, None) == INVALID
    assert _sweep(bd, d, step0=15, n_steps=6) == INVALID and _sweep(bd, d, step0=-1) == INVALID
    assert _sweep(bd, d, n_steps=2, n_real=3) == INVALID
    assert _sweep(_lib.BacktestDesc(4, 41, S, 1e-3), d) == INVALID           # descriptors that disagree in N
    assert _sweep(bd, _md(return_full_W=1)) == INVALID
    assert _sweep(bd, _md(40, 17)) == UNSUPPORTED
    assert _sweep(_lib.BacktestDesc(4, 103, S, 1e-3), _md(103, 10)) == UNSUPPORTED
    assert _sweep(bd, _md(40, 17), n_cfg=0) == UNSUPPORTED                   # the shape before the config count
    # the config count
    assert _sweep(bd, d, n_cfg=0) == INVALID and _sweep(bd, d, n_cfg=-2) == INVALID
    assert _sweep(_lib.BacktestDesc(1 << 20, 40, S, 1e-3), d, n_cfg=1 << 11) == INVALID   # n_cfg * P = 2^31
    assert _sweep(_lib.BacktestDesc(1 << 20, 40, S, 1e-3), d, n_cfg=(1 << 11) - 1) == OK
    assert _sweep(bd, _md(allow_short=1), n_cfg=0, limit=True) == INVALID    # ... before the limit's rule
    # a limit array with allow_short; shorting under the cap alone is a program
    assert _sweep(bd, _md(allow_short=1), limit=True) == UNSUPPORTED
    assert _sweep(bd, _md(allow_short=1), limit=True, cap=True, n_steps=2) == UNSUPPORTED   # ... before the arrays
    assert _sweep(bd, _md(allow_short=1), cap=True) == OK and _sweep(bd, _md(allow_short=1)) == OK
    # nothing to do, after the rules and before the arrays
    assert _sweep(bd, d, cfg=False) == OK                                    # the probe reads no array
    assert _sweep(_lib.BacktestDesc(0, 40, S, 1e-3), d, n_steps=2) == OK     # no paths: nothing run
    # null arrays with work to do, the three config arrays included
    assert _sweep(bd, d, n_steps=2) == INVALID
    # (at a slab shape and without a workspace, so that a call with every array set would end at
    # KMPC_ERR_WORKSPACE: nothing here can reach a launch)
    for name in ("gamma", "mv_cost", "bt_cost", "yhat", "sigma", "valid", "weights", "value", "hist", "target",
                 "status", "obj"):
        assert _sweep(_big(), _md(100, 10), n_steps=2, arrays=True, **{name: None}) == INVALID, name
    assert _sweep(_big(), _md(100, 10), n_steps=2, n_real=1, arrays=True, realized=None) == INVALID
    assert _sweep(_big(), _md(100, 10), n_steps=2, arrays=True, cfg=False) == INVALID


def _big():
    return _lib.BacktestDesc(2, 100, 20, 1e-3)


def test_workspace_rule_at_a_slab_shape():
    """(100, 10) is past the LDS variant: the workspace is that of B = n_cfg * P items, the cap's slab is
    larger, and one byte short is KMPC_ERR_WORKSPACE — decided before the launch."""
    L = _lib.load()
    big, d = _big(), _md(100, 10)
    q = _md(100, 10)
    q.B = 3 * 2
    need = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(q), 0))
    need_cap = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(q), 1))
    assert need == 8 * 6 * (1000 * 101 + 10 * 1000) and need_cap == 8 * 6 * (1000 * 101 + 20 * 1000)
    assert _sweep(big, d, n_steps=2, arrays=True) == WORKSPACE               # none given
    assert _sweep(big, d, n_steps=2, arrays=True, ws=_PTR, nws=need - 1) == WORKSPACE
    assert _sweep(big, d, n_steps=2, arrays=True, limit=True, ws=_PTR, nws=need - 1) == WORKSPACE
    assert _sweep(big, d, n_steps=2, arrays=True, cap=True, ws=_PTR, nws=need) == WORKSPACE
    assert _sweep(big, d, n_steps=2, arrays=True, cap=True, ws=_PTR, nws=need_cap - 1) == WORKSPACE
    assert _sweep(big, d, n_steps=2, arrays=True, ws=None, nws=need) == WORKSPACE
    q.B = 2                                                                  # the run's size does not do for 3 configs
    assert _sweep(big, d, n_steps=2, arrays=True, ws=_PTR,
                  nws=int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(q), 0))) == WORKSPACE
    assert _sweep(big, d) == OK                                              # the probe needs no workspace


# ---- Python: errors before any device work ---------------------------------------------------------

class _NoDevice(pkg.KoopmanMVStrategy):
    """A strategy whose model and device must not be touched: the config checks come first."""

    def __init__(self):
        super().__init__(None, pkg.MPCConfig(horizon=3, gamma=1.0))

    def device_model(self):
        raise AssertionError("device work before the config checks")

    def _device(self):
        raise AssertionError("device work before the config checks")


class _Env:
    n_assets = 4


def _cfg(**kw):
    return pkg.MPCConfig(**{"horizon": 3, "gamma": 1.0, **kw})


def _both(cfgs, match, **kw):
    N, bt = 4, pkg.BacktestConfig(horizon=5)
    with pytest.raises(ValueError, match=match):
        pkg.run_koopman_mv_sweep(_NoDevice(), torch.zeros(2, 12, 8), torch.zeros(2, 12, N), bt, [0.0] * N, [1.0] * N,
                                 cfgs, **kw)
    if not kw:
        with pytest.raises(ValueError, match=match):
            pkg.sweep_backtest_koopman_mv(_NoDevice(), _Env(), bt, cfgs)


def test_python_errors_before_device_work():
    _both([], "empty")
    _both([_cfg(), _cfg(horizon=4)], r"mpc_configs\[1\].*horizon")
    _both([_cfg(), _cfg(gamma=2.0), _cfg(allow_short=True)], r"mpc_configs\[2\].*allow_short")
    _both([_cfg(), _cfg(max_turnover=0.5)], r"max_turnover")               # the log-utility solve's cap is no sweep axis
    _both([_cfg(), _cfg(gamma=-1.0)], r"mpc_configs\[1\].*gamma")
    _both([_cfg(gamma=NAN)], r"mpc_configs\[0\].*gamma")
    _both([_cfg(), _cfg(max_weight=0.25)], r"mpc_configs\[1\].*max_weight")  # N u <= 1 at N = 4
    _both([_cfg(max_weight=-0.5)], "max_weight")
    _both([_cfg(), _cfg(mv_max_turnover=-0.1)], "mv_max_turnover")
    _both([_cfg(cost_coeff=-1e-3)], "cost_coeff")
    _both([_cfg(allow_short=True, max_weight=0.5)] * 2, "allow_short")
    _both([_cfg(horizon=17)], "exceeds")
    _both([_cfg(), _cfg(gamma=2.0)], "bt_cost_coeffs has 3 entries for 2 configs", bt_cost_coeffs=[1e-3] * 3)
    bt, s = pkg.BacktestConfig(horizon=5), _NoDevice()
    with pytest.raises(ValueError, match="obs must be"):
        pkg.run_koopman_mv_sweep(s, torch.zeros(2, 12, 3), torch.zeros(2, 12, 4), bt, [0.0] * 4, [1.0] * 4, [_cfg()])
    with pytest.raises(ValueError, match="mean and std"):
        pkg.run_koopman_mv_sweep(s, torch.zeros(2, 12, 8), torch.zeros(2, 12, 4), bt, [0.0] * 3, [1.0] * 4, [_cfg()])


def test_the_four_free_fields_pass_the_config_check():
    cfgs = [_cfg(), _cfg(gamma=0.0, cost_coeff=0.0, mv_max_turnover=0.1, max_weight=0.5)]
    got, programs = baselines._mv_sweep_configs(cfgs, 4)
    assert got == cfgs and programs == [(0.0, 0.0), (0.5, 0.1)]


# ---- grouping --------------------------------------------------------------------------------------

def test_groups_and_scatter():
    """Six configs with (u, tau) in {0, u0} x {0, tau0} (two of them repeated with other values), plus one
    with an inactive limit u >= 1, which _mv_band_program reports as no limit."""
    N, u0, tau0 = 10, 0.25, 0.05
    spec = [(0.0, tau0), (u0, 0.0), (0.0, 0.0), (u0, tau0), (0.3, 0.0), (0.4, 0.2), (1.5, tau0)]
    cfgs = [_cfg(max_weight=u, mv_max_turnover=t, gamma=1.0 + j) for j, (u, t) in enumerate(spec)]
    _, programs = baselines._mv_sweep_configs(cfgs, N)
    assert programs[6] == (0.0, tau0) and programs[:6] == spec[:6]
    groups = baselines._mv_sweep_groups(programs)
    assert groups == [(False, False, [2]), (False, True, [0, 6]), (True, False, [1, 4]), (True, True, [3, 5])]
    assert sorted(j for _, _, idx in groups for j in idx) == list(range(7))
    # every group's rows carry their config's number: the scatter puts row j at j
    parts = [torch.tensor(idx, dtype=torch.float64)[:, None, None].expand(len(idx), 2, 3).contiguous() for _, _, idx in groups]
    full = baselines._mv_sweep_scatter(parts, groups, 7)
    assert full.shape == (7, 2, 3)
    assert torch.equal(full, torch.arange(7, dtype=torch.float64)[:, None, None].expand(7, 2, 3))
    # one form only: one group, the order kept
    assert baselines._mv_sweep_groups([(0.0, 0.0)] * 3) == [(False, False, [0, 1, 2])]
