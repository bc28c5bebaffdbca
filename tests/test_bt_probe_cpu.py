"""kmpc_backtest_run and kmpc_backtest_sweep share one host path and one argument check but do not
accept the same calls: the return code of each entry point's shape probe over the grid of
tests/bt_probe.py equals the recorded one (tests/golden/bt_probe_codes.npz, written from the library
as it was before the two paths became one), cell for cell. No GPU: a probe launches nothing."""
import os

import numpy as np

import bt_probe
from koopman_mpc_portfolio_rebalancing_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bt_probe_codes.npz")


def test_probe_codes_equal_golden():
    g = np.load(GOLDEN)
    for k, v in bt_probe.AXES.items():   # the fixture was written over this grid
        assert np.array_equal(g["axis_" + k], np.asarray(v)), k
    assert int(g["n_cfg"]) == bt_probe.N_CFG
    run, sweep = bt_probe.probe_codes(_lib.load())
    assert run.shape == g["run"].shape == sweep.shape == g["sweep"].shape
    for name, got in (("run", run), ("sweep", sweep)):
        bad = np.argwhere(got != g[name])
        assert bad.size == 0, f"kmpc_backtest_{name}: {len(bad)} cells differ, the first at index {bad[0].tolist()}"


def test_golden_holds_the_known_differences():
    """The fixture itself: at cost_coeff = 1e-3, max_turnover = 0.2 the 660 calls only the run accepts
    all ask for KMPC_PRECISION_MIXED, and the 6 only the sweep accepts are the C3 shapes N = 65 and
    103, H = 10 at P = 2048 with KMPC_PRECISION_AUTO; max_turnover = 0 is KMPC_ERR_UNSUPPORTED for
    the run everywhere and changes nothing for the sweep."""
    g = np.load(GOLDEN)
    run, sweep = g["run"][..., 0], g["sweep"][..., 0]
    only_run = np.argwhere((run == 0) & (sweep != 0))
    only_sweep = np.argwhere((run != 0) & (sweep == 0))
    assert len(only_run) == 660 and (g["axis_precision"][only_run[:, 6]] == 2).all()
    assert len(only_sweep) == 6
    assert set(g["axis_N"][only_sweep[:, 0]]) == {65, 103} and set(g["axis_H"][only_sweep[:, 1]]) == {10}
    assert set(g["axis_P"][only_sweep[:, 2]]) == {2048} and set(g["axis_precision"][only_sweep[:, 6]]) == {0}
    assert (g["run"][..., 2] == -2).all() and (g["run"][..., 3] == -2).all()
    for j in (1, 2, 3):
        assert np.array_equal(g["sweep"][..., j], g["sweep"][..., 0])
