"""kmpc_backtest_run_box and kmpc_backtest_sweep_box (the path-persistent backtest and its sweep with
a per-asset position limit; added within ABI 0.7.0) without a GPU: the symbols, and the return codes
of the C boundary, every one decided before a launch. The expected codes are written out from the
table of include/kmpc.h, rule by rule and in its order — not recorded from the library:

  1. what kmpc_backtest_run / _sweep rejects before it looks at the shape's kernel: the same code;
  2. max_weight NaN or <= 0: INVALID;
  3. max_weight >= 1 without shorting: the plain entry point's own code;
  4. N * max_weight <= 1: INVALID;
  5. allow_short, N > 256, H > 10, path LARGE, precision MIXED, return_full_W, N <= 32: UNSUPPORTED;
  6. P == 0 or n_steps == 0: OK.

(N, H) = (10, 5) at the default limit 0.1 falls under rule 4 (10 * 0.1 == 1.0 in float64, as in
kmpc_solve_box and MPCConfig.max_weight), which comes before rule 5: INVALID. The N <= 32 rule is
checked at (10, 5) with max_weight = 0.25 and at (32, 5).
"""
import ctypes
import dataclasses

import pytest
import torch

import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -2
P, S, C, TAU, U, N_CFG = 4, 20, 1e-3, 0.2, 0.1, 3
NAN = float("nan")


def test_symbols_exported_and_version_unchanged():
    lib = _lib.load()
    for name in ("kmpc_backtest_run_box", "kmpc_backtest_sweep_box"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"


def _descs(N=40, H=5, paths=P, c=C, tau=TAU, **kw):
    sd = _lib.SolveDesc()
    sd.B, sd.N, sd.H, sd.cost_coeff, sd.max_turnover = 0, N, H, c, tau
    for k, v in kw.items():
        setattr(sd, k, v)
    return _lib.BacktestDesc(paths, N, S, 1e-3), sd


_HOST = (ctypes.c_double * 3)(1e-3, 0.2, 1e-3)   # never read: every call here returns before a launch
_PAR = [ctypes.addressof(_HOST)] * 3


def _ref(x):
    return ctypes.byref(x) if x is not None else None


def _box(sweep, bt, sd, u, step0=0, n_steps=0, n_cfg=N_CFG, par=_PAR, arrays=None):
    a = arrays if arrays is not None else [None] * 8
    lib = _lib.load()
    if sweep:
        return lib.kmpc_backtest_sweep_box(_ref(bt), _ref(sd), u, n_cfg, *par, step0, n_steps, a[0], a[1], 0, *a[2:], None)
    return lib.kmpc_backtest_run_box(_ref(bt), _ref(sd), u, step0, n_steps, a[0], a[1], 0, *a[2:], None)


def _plain(sweep, bt, sd, step0=0, n_steps=0, n_cfg=N_CFG, par=_PAR, arrays=None):
    a = arrays if arrays is not None else [None] * 8
    lib = _lib.load()
    if sweep:
        return lib.kmpc_backtest_sweep(_ref(bt), _ref(sd), n_cfg, *par, step0, n_steps, a[0], a[1], 0, *a[2:], None)
    return lib.kmpc_backtest_run(_ref(bt), _ref(sd), step0, n_steps, a[0], a[1], 0, *a[2:], None)


SWEEP = pytest.mark.parametrize("sweep", [False, True], ids=["run", "sweep"])


@SWEEP
@pytest.mark.parametrize("N,H,u,expect", [
    (40, 5, U, OK), (33, 1, U, OK), (256, 10, U, OK), (40, 7, U, OK),
    (32, 5, U, UNSUPPORTED), (10, 5, 0.25, UNSUPPORTED), (257, 5, U, UNSUPPORTED), (40, 11, U, UNSUPPORTED),
    (10, 5, U, INVALID),   # rule 4 before rule 5: 10 * 0.1 == 1.0
])
def test_shapes(sweep, N, H, u, expect):
    bt, sd = _descs(N, H)
    assert _box(sweep, bt, sd, u) == expect


@SWEEP
@pytest.mark.parametrize("field,value", [("allow_short", 1), ("path", _lib.PATH_LARGE), ("precision", _lib.PRECISION_MIXED),
                                         ("return_full_W", 1)])
def test_each_unsupported_option_alone(sweep, field, value):
    bt, sd = _descs(**{field: value})
    assert _box(sweep, bt, sd, U) == UNSUPPORTED


@SWEEP
def test_the_limit_itself(sweep):
    bt, sd = _descs()
    for u in (NAN, 0.0, -0.1):
        assert _box(sweep, bt, sd, u) == INVALID
    bt, sd = _descs(64, 5)
    for u in (1.0 / 64, 1.0 / 128):
        assert _box(sweep, bt, sd, u) == INVALID
    # the order: the limit's own validity comes before the unsupported options
    bt, sd = _descs(allow_short=1)
    assert _box(sweep, bt, sd, NAN) == INVALID


@SWEEP
@pytest.mark.parametrize("N,H", [(100, 10), (40, 7)])
@pytest.mark.parametrize("u", [1.0, 1.5])
def test_inactive_bound_is_the_plain_entry_point(sweep, N, H, u):
    bt, sd = _descs(N, H)
    plain = _plain(sweep, bt, sd)
    # (the plain kernels: the C3 shape has one, H = 7 has none)
    assert plain == (OK if (N, H) == (100, 10) else UNSUPPORTED)
    assert _box(sweep, bt, sd, u) == plain


def test_run_takes_a_program_without_turnover_terms():
    bt, sd = _descs(c=0.0, tau=0.0)
    assert _box(False, bt, sd, U) == OK


@SWEEP
def test_argument_errors_are_those_of_the_plain_entry_points(sweep):
    bt, sd = _descs()
    host = [ctypes.addressof(_HOST)] * 8
    calls = [
        dict(bt=None, sd=sd), dict(bt=bt, sd=None),                  # null descriptors
        dict(bt=bt, sd=sd, step0=15, n_steps=6),                     # step0 + n_steps > S
        dict(bt=bt, sd=sd, n_steps=2),                               # null arrays with work to do
    ]
    if sweep:
        calls += [dict(bt=bt, sd=sd, n_cfg=0),
                  dict(bt=bt, sd=sd, n_steps=2, par=[None] * 3, arrays=host)]   # null parameter arrays
    for kw in calls:
        b, s = kw.pop("bt"), kw.pop("sd")
        assert _box(sweep, b, s, U, **kw) == INVALID, kw
        assert _plain(sweep, b, s, **kw) == INVALID, kw
    # descriptors that disagree in N
    bt2, _ = _descs(41, 5)
    assert _box(sweep, bt2, sd, U) == INVALID == _plain(sweep, bt2, sd)


@SWEEP
def test_no_paths_is_ok_with_nothing_run(sweep):
    bt, sd = _descs(paths=0)
    assert _box(sweep, bt, sd, U, n_steps=2) == OK


class _NoDevice:
    """A strategy whose model must not be touched: the config checks come first."""

    def device_model(self):
        raise AssertionError("device work before the config checks")


def test_sweep_still_rejects_configs_that_differ_in_the_limit():
    base = pkg.MPCConfig(horizon=5, max_weight=0.1)
    cfgs = [base, dataclasses.replace(base, cost_coeff=1e-2), dataclasses.replace(base, max_weight=0.2)]
    x, r = torch.zeros(1, 12, 160), torch.zeros(1, 12, 40)
    with pytest.raises(ValueError, match="max_weight"):
        pkg.run_backtest_sweep(_NoDevice(), x, r, pkg.BacktestConfig(horizon=5), [0.0] * 40, [1.0] * 40, cfgs)
