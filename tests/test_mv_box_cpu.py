"""The per-asset position limit of the mean-variance solve (MPCConfig.max_weight,
kmpc_solve_mv_box, MarkowitzStrategy(max_weight=...)) without a GPU: the symbol and the unchanged
ABI version, every return-code rule of the C function (decided before any launch), the Python
plumbing, the goldens pinned by an LP certificate, and the kernel's algorithm restated in numpy
(mv_box_ref.reduced_mv_box_ipm) held to the device tests' bars on the device tests' inputs."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import mv_box_ref as ref
import koopman_mpc_portfolio_rebalancing_amd as pkg
from koopman_mpc_portfolio_rebalancing_amd import _lib
from koopman_mpc_portfolio_rebalancing_amd.baselines import MarkowitzStrategy
from koopman_mpc_portfolio_rebalancing_amd.mpc import MPCConfig, _box_limit
from oracle import mv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "mvbox_*.npz")))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


def test_symbol_and_version():
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmpc.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kmpc_solve_mv_box\s*\(", hdr)
    assert "kmpc_solve_mv_box" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "kmpc_solve_mv_box")
    assert _lib.ABI_VERSION == "0.7.0" == pkg.__version__
    assert lib.kmpc_version().decode() == "kmpc 0.7.0 (gfx950)"


def _desc(B=0, N=10, H=1, gamma=1.0, c=1e-3, short=0):
    d = _lib.MvDesc()
    d.B, d.N, d.H, d.gamma, d.cost_coeff, d.allow_short = B, N, H, gamma, c, short
    return d


def _box(d, u, p=None, ws=None, nws=0):
    return _lib.load().kmpc_solve_mv_box(ctypes.byref(d), u, p, p, 0, p, p, p, p, None, ws, nws, None)


def _plain(d, p=None, ws=None, nws=0):
    return _lib.load().kmpc_solve_mv_ws(ctypes.byref(d), p, p, 0, p, p, p, p, None, ws, nws, None)


def test_return_codes_need_no_gpu():
    L = _lib.load()
    # desc is checked as for kmpc_solve_mv_ws
    assert L.kmpc_solve_mv_box(None, 0.5, None, None, 0, None, None, None, None, None, None, 0, None) == INVALID
    assert _box(_desc(H=0), 0.5) == INVALID
    assert _box(_desc(N=0), 0.5) == INVALID
    assert _box(_desc(B=-1), 0.5) == INVALID
    assert _box(_desc(H=17), 0.5) == UNSUPPORTED
    assert _box(_desc(N=1025), 0.5) == UNSUPPORTED
    assert _box(_desc(N=65, H=16), 0.5) == UNSUPPORTED
    # the limit itself
    for u in (float("nan"), 0.0, -0.1, -float("inf")):
        assert _box(_desc(), u) == INVALID
    # no shorting with a limit, active or not
    assert _box(_desc(short=1), 0.5) == UNSUPPORTED
    assert _box(_desc(short=1), 1.0) == UNSUPPORTED
    assert _box(_desc(short=1, N=10), 0.1) == UNSUPPORTED      # (comes before the N u rule)
    # an inactive bound is kmpc_solve_mv_ws with the same arguments
    assert _box(_desc(), 1.0) == OK == _plain(_desc())
    assert _box(_desc(), 7.0) == OK
    assert _box(_desc(B=3), 1.0) == INVALID == _plain(_desc(B=3))          # its null-array check
    assert _box(_desc(N=10), 1.0) == OK                                    # N u <= 1 is not asked of it
    # N u <= 1: empty set, or the single point 1/N
    assert _box(_desc(N=10), 0.1) == INVALID
    assert _box(_desc(N=10), 0.05) == INVALID
    assert _box(_desc(N=4), 0.25) == INVALID
    assert _box(_desc(N=1024), 1.0 / 1024) == INVALID
    # the rules come before the B == 0 return and before the null-array check
    assert _box(_desc(B=0, N=10), 0.1) == INVALID
    assert _box(_desc(B=5), 0.5) == INVALID                                # null arrays
    assert _box(_desc(B=0), 0.5) == OK
    # every supported shape probe
    for N, H in ((2, 1), (4, 1), (10, 1), (64, 2), (129, 1), (43, 3), (16, 8), (300, 2), (512, 2), (64, 16), (1024, 1)):
        assert _box(_desc(N=N, H=H), 0.6) == OK, (N, H)
    assert _box(_desc(c=0.0, gamma=0.0), 0.5) == OK
    # the workspace rule of kmpc_solve_mv_ws (non-null arrays, never read: decided before any launch)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _desc(B=4, N=129, H=1)
    assert _box(d, 0.5, p) == WORKSPACE == _plain(d, p)                    # H N = 129 without a workspace
    assert _box(d, 1.0, p) == WORKSPACE
    need = L.kmpc_mv_workspace_bytes(ctypes.byref(d))
    assert need == 8 * 4 * (129 * 130 // 2 + 129)                          # the box call's workspace: unchanged
    assert _box(d, 0.5, p, p, need - 1) == WORKSPACE == _plain(d, p, p, need - 1)
    assert _box(_desc(B=4, N=43, H=3), 0.1, p) == WORKSPACE
    assert L.kmpc_mv_workspace_bytes(ctypes.byref(_desc(B=4, N=64, H=2))) == 0


def test_python_plumbing():
    assert MPCConfig().max_weight == 0.0
    s = MarkowitzStrategy(max_weight=0.25)
    assert s.max_weight == 0.25 and s.mpc_config.max_weight == 0.25
    assert s.mpc_config.horizon == 1 and s.mpc_config.gamma == 1.0 and s.mpc_config.cost_coeff == 0.001
    assert MarkowitzStrategy().max_weight == 0.0 and MarkowitzStrategy().mpc_config.max_weight == 0.0
    assert MarkowitzStrategy(2.0, 0.01, False).mpc_config.max_weight == 0.0    # the reference's three arguments
    with pytest.raises(TypeError):
        MarkowitzStrategy(1.0, 0.001, False, 0.25)                             # keyword only
    assert _box_limit(s.mpc_config, 10) == 0.25
    assert _box_limit(MarkowitzStrategy(max_weight=1.0).mpc_config, 10) == 0.0
    # the _box_limit errors surface from the strategy's config
    for kw, N in ((dict(max_weight=0.1), 10), (dict(max_weight=0.25), 4), (dict(max_weight=-0.1), 10),
                  (dict(max_weight=float("nan")), 10), (dict(max_weight=0.5, allow_short=True), 10)):
        with pytest.raises(ValueError):
            _box_limit(MarkowitzStrategy(**kw).mpc_config, N)


def test_dense_reference_closed_form_water_filling():
    """mu = [0.03, 0.02, 0.01, -0.01], Sigma = 1e-2 I, gamma = 1, c = 0: w_i = (mu_i - nu) / (2 gamma s)
    clipped to [0, u]. Unlimited: nu = 0.015, w = [0.75, 0.25, 0, 0]; with u = 0.6 the first asset
    caps and the second takes the rest."""
    wp, mu, S, gamma, c, u = ref.WATER
    W, st = ref.dense_mv_box_ipm(wp, mu, S, gamma, c, u)
    assert st == "optimal" and np.abs(W - ref.WATER_W).max() <= 1e-9
    W1, st = ref.dense_mv_box_ipm(wp, mu, S, gamma, c, 1.0)
    assert st == "optimal" and np.abs(W1 - [[0.75, 0.25, 0, 0]]).max() <= 1e-9
    assert ref.gap(ref.WATER_W, wp, mu, S, gamma, c, u) <= 1e-12


def test_dense_reference_matches_the_project_oracle_when_the_bound_is_inactive():
    d = np.load(os.path.join(GOLD, "mv_N20_H1_g1_c1e-3.npz"))
    for b in range(4):
        W, st = ref.dense_mv_box_ipm(d["w_prev"][b], d["mu"][b], d["sigma"][b], 1.0, 1e-3, 1.0)
        Wo, so = mv_ref.mv_dense_ipm(d["w_prev"][b], d["mu"][b], d["sigma"][b], 1.0, 1e-3)
        assert st == so == "optimal"
        f, fo = (mv_ref.mv_objective(V, d["w_prev"][b], d["mu"][b], d["sigma"][b], 1.0, 1e-3) for V in (W, Wo))
        assert abs(f - fo) <= 1e-12 and abs(f - d["obj"][b]) <= 1e-12


def _windows(path):
    g = np.load(path)
    gamma, c, u = (float(v) for v in g["config"])
    for b in range(g["mu"].shape[0]):
        S = g["sigma"] if g["sigma"].ndim == 2 else g["sigma"][b]
        yield b, g["w_prev"][b], g["mu"][b], S, gamma, c, u, g["W"][b], float(g["obj"][b])


def test_every_issue_case_has_a_golden():
    have = {os.path.basename(p) for p in FILES}
    assert have == {f"mvbox_N{N}_H{H}.npz" for N, H in ((4, 1), (10, 1), (20, 1), (5, 3), (8, 2), (16, 8), (64, 2), (43, 3))}
    assert np.load(os.path.join(GOLD, "mvbox_N20_H1.npz"))["sigma"].ndim == 2     # the shared-Sigma file
    for p in FILES:
        assert os.path.getsize(p) < 128 * 1024


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p) for p in FILES])
def test_goldens_pinned(path):
    active = False
    n = 0
    for b, wp, mu, S, gamma, c, u, W, obj in _windows(path):
        assert mu.shape[1] * u > 1
        assert not ref.violated(W, u)
        assert np.abs(W.sum(1) - 1).max() <= 1e-12 and W.min() >= -1e-12 and W.max() <= u + 1e-12
        assert obj == mv_ref.mv_objective(W, wp, mu, S, gamma, c)
        gp = ref.gap(W, wp, mu, S, gamma, c, u)
        print(f"{os.path.basename(path)} window {b}: gap {gp:.3e}")
        assert gp <= 1e-10
        active = active or W.max() > u - 1e-6
        n += 1
    assert 4 <= n <= 8
    assert active   # the limit binds somewhere in every file
    g = np.load(path)
    assert np.allclose(g["w_prev"][1], 1.0 / g["mu"].shape[2]) and g["w_prev"][2].max() == 1.0   # 1/N, a vertex


@pytest.mark.parametrize("name", ["mvbox_N10_H1.npz", "mvbox_N16_H8.npz", "mvbox_N43_H3.npz"])
def test_certificate_rejects_a_suboptimal_portfolio(name):
    """1e-2 of weight moved in period 0 from a capped asset to the asset of lowest mu: still
    feasible, about 1e-2 times the spread of mu (sd 0.01) worse, and the certificate must say so by
    ten times its bar at the least. It bounds the true loss from above."""
    b, wp, mu, S, gamma, c, u, W, obj = next(_windows(os.path.join(GOLD, name)))
    hi = int(np.argmax(np.where(W[0] > u - 1e-6, mu[0], -np.inf)))
    lo = int(np.argmin(mu[0]))
    assert W[0, hi] > u - 1e-6 and W[0, lo] + 1e-2 <= u and hi != lo
    V = W.copy()
    V[0, hi] -= 1e-2
    V[0, lo] += 1e-2
    assert not ref.violated(V, u)
    f = mv_ref.mv_objective(V, wp, mu, S, gamma, c)
    bar = ref.certificate_bar(f, mu, S, gamma, c)
    good, bad = ref.gap(W, wp, mu, S, gamma, c, u), ref.gap(V, wp, mu, S, gamma, c, u)
    print(f"{name}: gap {good:.3e} at the golden, {bad:.3e} after the move, bar {bar:.3e}")
    assert good <= 1e-10
    assert bad > 10 * bar
    assert bad >= obj - f - 1e-12


def test_feasibility_helper_holds_each_bar():
    b, wp, mu, S, gamma, c, u, W, obj = next(_windows(os.path.join(GOLD, "mvbox_N10_H1.npz")))
    assert ref.violated(W, u) == []
    i, j = int(np.argmax(W[0])), int(np.argmin(W[0]))
    V = W.copy()
    V[0, i] += 1e-8
    V[0, j] -= 1e-8
    bad = ref.violated(V, u)
    assert any(s.startswith("max w - u") for s in bad) and any(s.startswith("min w") for s in bad), bad
    V = W.copy()
    V[0, j] += 1e-8
    assert any(s.startswith("budget") for s in ref.violated(V, u))
    V[0, 0] = np.nan
    assert ref.violated(V, u) == ["non-finite W"]


# ---- the kernel's algorithm, in numpy, on the inputs of tests/test_mv_box_gpu.py ----

def _held(tag, wp, mu, S, gamma, c, u, fref=None):
    """reduced_mv_box_ipm on one window, held to the device tests' bars."""
    W, st, it, f = ref.reduced_mv_box_ipm(wp, mu, S, gamma, c, u)
    gp = ref.gap(W, wp, mu, S, gamma, c, u)
    bar = ref.certificate_bar(f, mu, S, gamma, c)
    print(f"{tag}: status {st}, {it} iterations, gap {gp:.3e} (bar {bar:.3e})" +
          ("" if fref is None else f", |f - f*| {abs(f - fref):.3e} (bar {ref.objective_bar(fref):.3e})"))
    assert st == 0 and it <= 20
    assert not ref.violated(W, u)
    assert gp <= bar
    if fref is not None:
        assert abs(f - fref) <= ref.objective_bar(fref)
    return W, f


def test_reduced_iteration_reaches_the_bars_on_the_goldens():
    for path in FILES:
        for b, wp, mu, S, gamma, c, u, W, obj in _windows(path):
            _held(f"{os.path.basename(path)} window {b}", wp, mu, S, gamma, c, u, obj)


@pytest.mark.parametrize("case", ref.SEEDED, ids=[f"N{c[0]}_H{c[1]}" for c in ref.SEEDED])
def test_reduced_iteration_reaches_the_bars_on_the_seeded_shapes(case):
    N, H, gamma, c, u, B = case
    wp, mu, S = ref.seeded(case)
    for b in range(B):
        fref = None
        if N * H <= 600:
            Wd, st = ref.dense_mv_box_ipm(wp[b], mu[b], S[b], gamma, c, u)
            assert st == "optimal"
            fref = mv_ref.mv_objective(Wd, wp[b], mu[b], S[b], gamma, c)
        _held(f"N={N} H={H} window {b}", wp[b], mu[b], S[b], gamma, c, u, fref)


@pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")   # the dense reference's last iterations at c = 10
def test_reduced_iteration_on_the_edges_and_closed_forms():
    for name, wp, mu, S, gamma, c, u in ref.edge_cases():
        Wd, st = ref.dense_mv_box_ipm(wp, mu, S, gamma, c, u)
        assert st == "optimal", name
        W, f = _held(name, wp, mu, S, gamma, c, u, mv_ref.mv_objective(Wd, wp, mu, S, gamma, c))
        if name == "c = 10, w_prev inside":
            assert np.abs(W - wp).max() <= 1e-8
    N, H, gamma, c, u, wp, mu, S = ref.cannot_bind()
    for b in range(len(wp)):
        Wo, so = mv_ref.mv_dense_ipm(wp[b], mu[b], S[b], gamma, c)
        assert so == "optimal" and Wo.max() < u - 1e-3
        _held(f"cannot bind, window {b}", wp[b], mu[b], S[b], gamma, c, u, mv_ref.mv_objective(Wo, wp[b], mu[b], S[b], gamma, c))
    W, f = _held("water-filling", *ref.WATER)
    assert np.abs(W - ref.WATER_W).max() <= 1e-8
    wp, mu, S, gamma, c, u, G = ref.greedy_case()
    W, f = _held("greedy fill", wp, mu, S, gamma, c, u)
    print(f"greedy fill: |W - G| {np.abs(W - G).max():.3e}")
    assert np.abs(W - G).max() <= 1e-8
    W, f = _held("flat mu", *ref.FLAT)
    print(f"flat mu: value {f:.12e}")
    assert abs(f - ref.FLAT_VALUE) <= 1e-8


def test_reduced_iteration_on_the_markowitz_windows():
    """The stored moments of markowitz_N10.npz under u = 0.2 (gamma = 1, c = 1e-3), as
    MarkowitzStrategy(max_weight=0.2) solves them on the device."""
    d = np.load(os.path.join(GOLD, "markowitz_N10.npz"))
    rows = np.flatnonzero(d["valid"] == 1)
    assert len(rows) >= 4
    for b in rows:
        wp, mu, S = d["w_prev"][b], d["mu"][b][None], d["sigma"][b]
        Wd, st = ref.dense_mv_box_ipm(wp, mu, S, 1.0, 1e-3, 0.2)
        assert st == "optimal" and Wd.max() > 0.2 - 1e-6
        _held(f"markowitz window {b}", wp, mu, S, 1.0, 1e-3, 0.2, mv_ref.mv_objective(Wd, wp, mu, S, 1.0, 1e-3))
