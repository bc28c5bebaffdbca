"""Every rule of the position limit that is decided before a launch, over the whole grid, against the
codes recorded from the library of an earlier commit (tests/golden/box_codes.npz, written once by
tests/golden/make_box_codes.py, which names the commit in the file): kmpc_solve_box,
kmpc_solve_box_workspace_bytes, kmpc_solve_box_ws with and without a workspace, kmpc_backtest_run_box
and kmpc_backtest_sweep_box, and on a grid of their own kmpc_solve_mv_box, kmpc_markowitz_run and
kmpc_markowitz_sweep. Nothing is regenerated here: the file's rows are replayed against the built
library (null arrays and n_steps = 0: no launch, no GPU) and every answer must be equal."""
import importlib.util
import os

import numpy as np

from koopman_mpc_portfolio_rebalancing_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_box_codes", os.path.join(GOLD, "make_box_codes.py"))
codes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(codes)
REC = np.load(os.path.join(GOLD, "box_codes.npz"))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


def _mismatch(grid, got, want, key):
    bad = np.flatnonzero(got != want)
    return "" if not len(bad) else "%s: %d rows differ, first %s -> %d, recorded %d" % (
        key, len(bad), {k: v[bad[0]].item() for k, v in grid.items()}, got[bad[0]], want[bad[0]])


def test_the_file_names_its_commit_and_covers_the_grid():
    assert len(str(REC["commit"])) == 40 and str(REC["version"]) == "kmpc 0.7.0 (gfx950)"
    for cols, prefix, grid in ((codes.SOLVE_COLS, "solve_", codes.solve_grid()), (codes.MV_COLS, "mv_", codes.mv_grid())):
        for c in cols:   # the recorded rows are the grid's, NaN limits included
            assert np.array_equal(REC[prefix + c], grid[c], equal_nan=True), c
    assert len(REC["solve_N"]) == 40320
    for k in ("box", "ws_big", "ws_null", "bt_run", "bt_sweep"):
        assert set(np.unique(REC["solve_" + k]).tolist()) <= {OK, INVALID, UNSUPPORTED, WORKSPACE}
    assert set(np.unique(REC["solve_ws_null"]).tolist()) == {OK, INVALID, UNSUPPORTED, WORKSPACE}
    assert int((REC["solve_ws_bytes"] > 0).sum()) == 1178
    # the one input the two rules answer differently: allow_short with N * max_weight <= 1
    one = (REC["mv_allow_short"] == 1) & (REC["mv_u"] == 1.0 / REC["mv_N"]) & (REC["mv_H"] == 1) & (REC["mv_N"] <= 1024)
    assert one.sum() > 0 and (REC["mv_mv_box"][one] == UNSUPPORTED).all()
    same = ((REC["solve_allow_short"] == 1) & (REC["solve_u"] == 1.0 / REC["solve_N"]) & (REC["solve_H"] == 1) &
            (REC["solve_N"] <= 1024) & (REC["solve_N"] > 2))
    assert same.sum() > 0 and (REC["solve_box"][same] == INVALID).all()


def test_solve_family_codes_equal_the_recorded_ones():
    grid = {c: REC["solve_" + c] for c in codes.SOLVE_COLS}
    got = codes.solve_codes(_lib.load(), grid)
    bad = [m for k, v in got.items() for m in [_mismatch(grid, v, REC["solve_" + k].astype(np.int64), k)] if m]
    assert not bad, "\n".join(bad)


def test_mean_variance_codes_equal_the_recorded_ones():
    grid = {c: REC["mv_" + c] for c in codes.MV_COLS}
    got = codes.mv_codes(_lib.load(), grid)
    bad = [m for k, v in got.items() for m in [_mismatch(grid, v, REC["mv_" + k].astype(np.int64), k)] if m]
    assert not bad, "\n".join(bad)
