"""kmpc_backtest_sweep (ABI 0.7.0) and run_backtest_sweep without a GPU: the symbol, the argument
and shape checks of the C ABI (an n_steps = 0 call is the shape probe: no launch), and the config
checks of the Python entry, which raise before any device work."""
import ctypes
import dataclasses

import pytest
import torch

import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import _lib


def test_symbol_exported_and_versions():
    lib = _lib.load()
    assert "kmpc_backtest_sweep" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "kmpc_backtest_sweep")
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"
    assert callable(pkg.run_backtest_sweep) and callable(pkg.sweep_backtest)


def _descs(N=100, H=10, P=4, S=20):
    sd = _lib.SolveDesc()
    sd.B, sd.N, sd.H, sd.cost_coeff, sd.max_turnover = 0, N, H, -5.0, -1.0   # (ignored by the sweep)
    return _lib.BacktestDesc(P, N, S, 1e-3), sd


def _call(lib, bt, sd, n_cfg, params, step0, n_steps, arrays=None):
    a = arrays if arrays is not None else [None] * 8
    byref = lambda x: ctypes.byref(x) if x is not None else None
    return lib.kmpc_backtest_sweep(byref(bt), byref(sd), n_cfg, *params, step0, n_steps, a[0], a[1], 0, *a[2:], None)


def test_argument_errors():
    lib = _lib.load()
    bt, sd = _descs()
    host = (ctypes.c_double * 3)(1e-3, 1e-3, 1e-3)   # never read: every call below returns before a launch
    p = [ctypes.addressof(host)] * 3
    assert _call(lib, bt, sd, 3, p, 0, 0) == 0                   # the C3 shape: supported
    assert _call(lib, None, sd, 3, p, 0, 0) == -1                # null desc
    assert _call(lib, bt, None, 3, p, 0, 0) == -1
    assert _call(lib, bt, sd, 0, p, 0, 0) == -1                  # n_cfg = 0
    assert _call(lib, bt, sd, -2, p, 0, 0) == -1
    assert _call(lib, bt, sd, 3, p, 0, 2) == -1                  # null arrays with work to do
    assert _call(lib, bt, sd, 3, [None] * 3, 0, 2, [ctypes.addressof(host)] * 8) == -1   # null parameter arrays
    assert _call(lib, bt, sd, 3, p, 15, 6) == -1                 # step0 + n_steps > S
    assert _call(lib, bt, sd, 1 << 30, p, 0, 0) == -1            # n_cfg * P past an int


@pytest.mark.parametrize("change,expect", [
    ({}, 0), ({"H": 5}, 0), ({"N": 20, "H": 5}, 0), ({"N": 8, "H": 2}, 0), ({"N": 200}, 0), ({"precision": 1}, 0),
    ({"H": 3}, -2), ({"N": 20, "H": 3}, -2), ({"allow_short": 1}, -2), ({"precision": 2}, -2), ({"N": 300}, -2),
    ({"return_full_W": 1}, -2), ({"path": 2}, -2)])
def test_shape_probe(change, expect):
    lib = _lib.load()
    bt, sd = _descs()
    for k, v in change.items():
        setattr(sd, k, v)
    bt.N = sd.N
    assert _call(lib, bt, sd, 5, [None] * 3, 0, 0) == expect


class _NoDevice:
    """A strategy whose model must not be touched: the config checks come first."""

    def device_model(self):
        raise AssertionError("device work before the config checks")


@pytest.mark.parametrize("field,value", [("horizon", 10), ("tol", 1e-6), ("allow_short", True), ("solver_path", 1)])
def test_sweep_rejects_configs_differing_elsewhere(field, value):
    base = pkg.MPCConfig(horizon=5)
    cfgs = [base, dataclasses.replace(base, cost_coeff=1e-2, max_turnover=0.1), dataclasses.replace(base, **{field: value})]
    x, r = torch.zeros(1, 12, 40), torch.zeros(1, 12, 4)
    with pytest.raises(ValueError, match=field):
        pkg.run_backtest_sweep(_NoDevice(), x, r, pkg.BacktestConfig(horizon=5), [0.0] * 4, [1.0] * 4, cfgs)


def test_sweep_rejects_negative_cost_and_bad_lengths():
    base = pkg.MPCConfig(horizon=5)
    x, r = torch.zeros(1, 12, 40), torch.zeros(1, 12, 4)
    args = (_NoDevice(), x, r, pkg.BacktestConfig(horizon=5), [0.0] * 4, [1.0] * 4)
    with pytest.raises(ValueError, match="cost_coeff"):
        pkg.run_backtest_sweep(*args, [base, dataclasses.replace(base, cost_coeff=-1e-3)])
    with pytest.raises(ValueError):
        pkg.run_backtest_sweep(*args, [])
    with pytest.raises(ValueError, match="bt_cost_coeffs"):
        pkg.run_backtest_sweep(*args, [base, base], bt_cost_coeffs=[1e-3])
    with pytest.raises(ValueError, match="bt_configs"):
        pkg.sweep_backtest(_NoDevice(), None, pkg.BacktestConfig(), [base], [pkg.BacktestConfig(horizon=7)])
