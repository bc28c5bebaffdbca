"""What the rollout's host path answers before any launch, against the answers recorded from the library
of an earlier commit (tests/golden/host_codes_rollout.npz, written once by
tests/golden/make_rollout_host_codes.py, which names the commit in the file): the workspace size, the
return code of kmpc_rollout with B = 0, and with the workspace one byte short. Nothing is regenerated
here: the file's rows are replayed against the built library (no launch, no GPU) and every answer
must be equal."""
import importlib.util
import os

import numpy as np

from koopman_mpc_portfolio_rebalancing_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_rollout_host_codes", os.path.join(GOLD, "make_rollout_host_codes.py"))
codes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(codes)
REC = np.load(os.path.join(GOLD, "host_codes_rollout.npz"))
OK, INVALID, WORKSPACE = 0, -1, -3


def test_the_file_names_its_commit_and_covers_the_grid():
    assert len(str(REC["commit"])) == 40 and str(REC["version"]) == "kmpc 0.7.0 (gfx950)"
    g = codes.grid()
    for c in codes.COLS:
        assert np.array_equal(REC[c], g[c]), c
    assert len(REC["B"]) == 69120
    # the grid as the issue states it, both sides of 8,192 windows, of L % 32 and of L <= 512
    assert set(REC["B"].tolist()) == {0, 1, 300, 8191, 8192, 70000}
    assert set(REC["L"].tolist()) == {16, 48, 128, 256, 544}
    assert set(REC["N"].tolist()) == {1, 33, 100} and set(REC["H"].tolist()) == {1, 10}
    assert set(REC["enc_hidden"].tolist()) == {0, 1024} and set(REC["dec_layers"].tolist()) == {1, 2}
    assert set(REC["kind"].tolist()) == {0, 1}
    assert set(REC["dtype"].tolist()) == {0, 1, 2, 7} and set(REC["latent"].tolist()) == {0, 1, 2, 3}
    assert ((REC["obs_ld"] == 0) | (REC["obs_ld"] == REC["N"]) | (REC["obs_ld"] == REC["N"] - 1)).all()
    # what was recorded: B = 0 passes exactly where the descriptor is valid; a short workspace is
    # refused there, and the size rule stands ahead of the obs_ld, dtype and latent_unfused rules
    valid = (REC["dtype"] != 7) & (REC["latent"] != 3) & ((REC["obs_ld"] == 0) | (REC["obs_ld"] >= REC["N"]))
    assert np.array_equal(REC["rc_b0"] == OK, valid) and (REC["rc_b0"][~valid] == INVALID).all()
    assert (REC["rc_short"] == WORKSPACE).all()
    assert (REC["ws_bytes"] > 0).all() and (REC["ws_bytes"] % 256 == 0).all()


def test_host_answers_equal_the_recorded_ones():
    g = {c: REC[c] for c in codes.COLS}
    got = codes.host_codes(_lib.load(), g)
    bad = []
    for k, v in got.items():
        want = REC[k].astype(np.int64)
        i = np.flatnonzero(v != want)
        if len(i):
            bad.append("%s: %d rows differ, first %s -> %d, recorded %d" % (
                k, len(i), {c: g[c][i[0]].item() for c in codes.COLS}, v[i[0]], want[i[0]]))
    assert not bad, "\n".join(bad)
