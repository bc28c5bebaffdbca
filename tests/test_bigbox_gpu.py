"""The position limit on the large-window kernel (kmpc_solve_box_ws; MPCConfig.solver_path = 2 with
max_weight) on the device.

The box form of ipm_big has six kernels: HM in {10, 21} x 256 / 512 / 1024 threads (kernel_of
below restates big::launch's dispatch). Each is run here

* on goldens of the dense reference (tests/box_ref.py, pinned in test_bigbox_cpu.py): the nineteen
  register-box files through the HM = 10 / 256-thread kernel, and the bigbox_* files,
* against the plain large-window solve where the limit cannot bind,
* in a sweep over the four constraint cases with the limit binding, a non-finite and an infeasible
  window between solved ones, held to the LP certificate box_ref.gap,

then BASELINE configs[4]'s shape, slab reuse past the slot count, the C entry's own rules, and
the layers that turn an MPCConfig into a solve. The bars are the project's:
objective 1e-6 + 1e-5 |f|, W[0] 1e-3 where c > 0, budget and turnover 1e-8, bounds 1e-9
(box_ref.violated), value == reference_objective(W) to 1e-12.
"""
import ctypes
import dataclasses
import functools
import glob
import os

import numpy as np
import pytest
import torch

import box_ref
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, MPCConfig, run_backtest_lockstep,
                                                   solve_mpc_log_utility_batched, _lib)
from koopman_mpc_portfolio_rebalancing_amd.mpc import _solve_desc, log_utility_value_batched
from test_box_gpu import H_, KEYS, N_, P_, S_, U_, _Env, _layers, _strat
from test_box_variants_gpu import CONSTRAINT_CASES

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOX_FILES = sorted(glob.glob(os.path.join(GOLD, "box_N*_H*.npz")))
BIG_FILES = sorted(glob.glob(os.path.join(GOLD, "bigbox_N*_H*.npz")))
LARGE = _lib.PATH_LARGE
KERNELS = {f"hm{hm}_{t}" for hm in (10, 21) for t in (256, 512, 1024)}
# one shape per kernel for the inactive-limit and the certificate tests
SHAPES = [(200, 10), (300, 5), (600, 3), (100, 12), (300, 11), (520, 11)]


def kernel_of(N, H):
    """The box kernel big::launch<HM, true> sends an (N, H) window to (kmpc_solve_big.h)."""
    assert 1 <= H <= 21 and 2 <= N <= 1024
    hm = 10 if H <= 10 else 21
    threads = 64 * -(-N // 64)
    return f"hm{hm}_{256 if threads <= 256 else 512 if threads <= 512 else 1024}"


def _shape_of(path):
    n, h = os.path.basename(path)[:-4].split("_")[1:]
    return int(n[1:]), int(h[1:])


def _id(N, H):
    return f"N{N}_H{H}-{kernel_of(N, H)}"


def _cfg(H, c, tau, u, path=LARGE, **kw):
    return MPCConfig(horizon=H, cost_coeff=c, max_turnover=tau, max_weight=u, solver_path=path, **kw)


def _solve(wp, y, cfg, full=True):
    dev = torch.device("cuda")
    W, st, val, it = solve_mpc_log_utility_batched(torch.as_tensor(wp, device=dev), torch.as_tensor(y, device=dev), cfg,
                                                   return_full=full, with_iters=True)
    torch.cuda.synchronize()
    return W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy()


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _bar(f):
    return 1e-6 + 1e-5 * abs(f)


def _is_fallback(W, st, val, wp, b, status):
    return st[b] == status and np.array_equal(W[b], np.tile(wp[b], (W.shape[1], 1))) and np.isnan(val[b])


def _certified(W, wp, y, c, tau, u, val):
    """One solved window: feasible at the bars, value = f(W) to 1e-12, certificate at the objective
    bar. Returns the certificate gap."""
    assert not box_ref.violated(W, wp, tau, u)
    f = box_ref.reference_objective(W, wp, y, c)
    assert abs(val - f) <= 1e-12, (val, f)
    gp = box_ref.gap(W, wp, y, c, tau, u)
    assert gp <= _bar(f), (gp, _bar(f))
    return gp


def test_the_cases_reach_every_kernel():
    assert len(BOX_FILES) == 19 and len(BIG_FILES) == 9
    assert {kernel_of(*_shape_of(p)) for p in BOX_FILES} == {"hm10_256"}
    golden = {kernel_of(*_shape_of(p)) for p in BIG_FILES}
    # (hm10_256: the register goldens above; hm21_1024 has no dense golden: a 1 GB KKT matrix)
    assert golden == KERNELS - {"hm10_256", "hm21_1024"}
    assert [kernel_of(N, H) for N, H in SHAPES] == ["hm10_256", "hm10_512", "hm10_1024", "hm21_256", "hm21_512",
                                                    "hm21_1024"]
    assert golden | {kernel_of(N, H) for N, H in SHAPES} == KERNELS
    assert kernel_of(500, 20) == "hm21_512" and kernel_of(12, 11) == "hm21_256"
    # the edges of the dispatch
    for (N, H), k in {(256, 10): "hm10_256", (257, 10): "hm10_512", (512, 11): "hm21_512", (513, 10): "hm10_1024",
                      (1024, 21): "hm21_1024"}.items():
        assert kernel_of(N, H) == k


# ---- (a), (b) the goldens ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _golden_run(path):
    """(golden, the device's (W, status, value, iters)); computed once per file, not modified."""
    g = np.load(path)
    c, tau, u = (float(v) for v in g["config"])
    H = g["yhat"].shape[1]
    return g, _solve(g["w_prev"], g["yhat"], _cfg(H, c, tau, u))


def _check_golden(path):
    g, (W, st, val, it) = _golden_run(path)
    c, tau, u = (float(v) for v in g["config"])
    B, H, N = g["yhat"].shape
    feas = g["feasible"].astype(bool)
    print(f"KERNEL {kernel_of(N, H)} {os.path.basename(path)}: status {st.tolist()} iterations {it.tolist()}")
    for b in range(B):
        wp, y = g["w_prev"][b], g["yhat"][b]
        if not feas[b]:
            assert st[b] == 2
            assert np.array_equal(W[b], np.tile(wp, (H, 1)))
            assert np.isnan(val[b])
            continue
        assert st[b] == 0, (b, st[b])
        assert np.abs(W[b].sum(1) - 1).max() <= 1e-8
        assert W[b].min() >= -1e-9
        assert W[b].max() <= u + 1e-9
        if tau > 0:
            assert box_ref.turnover(W[b], wp).max() <= tau + 1e-8
        f = box_ref.reference_objective(W[b], wp, y, c)
        gp = box_ref.gap(W[b], wp, y, c, tau, u)
        print(f"  window {b}: objective error {abs(val[b] - g['obj'][b]):.3e}, gap {gp:.3e}, "
              f"W0 error {np.abs(W[b, 0] - g['W'][b, 0]).max():.3e}, value - f(W) {abs(val[b] - f):.1e}")
        assert abs(val[b] - g["obj"][b]) <= 1e-6 + 1e-5 * abs(g["obj"][b])
        assert gp <= 1e-6 + 1e-5 * abs(f)
        assert abs(val[b] - f) <= 1e-12
        if c > 0:
            assert np.abs(W[b, 0] - g["W"][b, 0]).max() < 1e-3
    # a second launch is bit-identical
    W2, st2, val2, it2 = _solve(g["w_prev"], g["yhat"], _cfg(H, c, tau, u))
    assert np.array_equal(W, W2) and np.array_equal(st, st2) and np.array_equal(val, val2, equal_nan=True)
    assert np.array_equal(it, it2)
    if not feas.all():   # the infeasible windows do not touch their neighbours
        Wf, stf, valf, _ = _solve(g["w_prev"][feas], g["yhat"][feas], _cfg(H, c, tau, u))
        assert np.array_equal(Wf, W[feas]) and np.array_equal(stf, st[feas]) and np.array_equal(valf, val[feas])
    return feas


@pytest.mark.parametrize("path", BOX_FILES, ids=[os.path.basename(p)[:-4] for p in BOX_FILES])
def test_register_goldens_through_the_large_window_kernel(path):
    _check_golden(path)


@pytest.mark.parametrize("path", BIG_FILES, ids=[_id(*_shape_of(p)) for p in BIG_FILES])
def test_goldens(path):
    feas = _check_golden(path)
    assert feas.all() == (os.path.basename(path) != "bigbox_N40_H12.npz")


# ---- (c) every kernel against the plain large-window solve where the limit cannot bind ---------------

@pytest.mark.parametrize("N,H", SHAPES, ids=[_id(N, H) for N, H in SHAPES])
def test_inactive_limit_matches_the_plain_large_window_solve(N, H):
    """u = 0.9 with tau = 0.05: a period moves at most tau / 2 into one asset, so with
    max(w_prev) + H tau / 2 < u - 1e-3 the limit cannot bind and the two programs share their
    optimum. Not bit-identical: l5 is live, so the iterates differ."""
    B, c, tau, u = 3, 1e-3, 0.05, 0.9
    rng = np.random.default_rng(7000 * N + H)
    wp = rng.dirichlet(np.ones(N), B)
    y = rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32)
    assert wp.max() + H * tau / 2 < u - 1e-3
    W, st, val, it = out = _solve(wp, y, _cfg(H, c, tau, u))
    Wp, stp, valp, itp = _solve(wp, y, _cfg(H, c, tau, 0.0))
    err = np.abs(val - valp)
    print(f"KERNEL {kernel_of(N, H)} inactive N={N} H={H}: status {st.tolist()} / plain {stp.tolist()} objective error "
          f"{err.max():.3e} W0 error {np.abs(W[:, 0] - Wp[:, 0]).max():.3e} iterations {it.tolist()} / plain {itp.tolist()}")
    assert np.array_equal(st, stp) and (st == 0).all(), (st, stp)
    assert (err <= 1e-6 + 1e-5 * np.abs(valp)).all(), err
    assert np.abs(W[:, 0] - Wp[:, 0]).max() < 1e-3
    assert W.max() < u
    for b in range(B):
        assert not box_ref.violated(W[b], wp[b], tau, u), b
        assert abs(val[b] - box_ref.reference_objective(W[b], wp[b], y[b], c)) <= 1e-12
    assert _same(out, _solve(wp, y, _cfg(H, c, tau, u)))


# ---- (d) certificate sweep with the limit binding --------------------------------------------------

def sweep_inputs(N, H, k):
    """w_prev [5, N], yhat [5, H, N]: windows 0, 2, 4 half Dirichlet, half uniform (little weight
    above the limit), window 1 with a NaN in its last period, window 3 all in asset 0."""
    rng = np.random.default_rng(1000 * N + 10 * H + k)
    wp = 0.5 * rng.dirichlet(np.ones(N), 5) + 0.5 / N
    wp[3] = 0.0
    wp[3, 0] = 1.0
    y = rng.normal(5e-4, 0.02, (5, H, N)).astype(np.float32)
    y[1, H - 1, N // 2] = np.nan
    return wp, y


SWEEP = [(N, H, k) for N, H in SHAPES for k in range(4)]


@pytest.mark.parametrize("N,H,k", SWEEP, ids=[f"{_id(N, H)}-case{k}" for N, H, k in SWEEP])
def test_certificate_sweep_with_the_limit_binding(N, H, k):
    c, tau = CONSTRAINT_CASES[k]
    u = 2.5 / N
    wp, y = sweep_inputs(N, H, k)
    B = 5
    # period 0 has to trade 2 E, E = sum_i max(w_prev_i - u, 0), to get under the limit: a window is
    # feasible iff 2 E <= tau (test_box_variants_gpu.py holds this rule against the LP)
    E = np.maximum(wp - u, 0.0).sum(-1)
    feas = 2 * E <= tau if tau > 0 else np.ones(B, bool)
    if tau > 0:   # no window near the boundary an interior point cannot resolve
        assert (np.abs(2 * E - tau) >= 0.02).all(), 2 * E - tau
    assert feas[[0, 1, 2, 4]].all() and feas[3] == (tau == 0)
    solved = [b for b in range(B) if b != 1 and feas[b]]
    cfg = _cfg(H, c, tau, u)
    W, st, val, it = _solve(wp, y, cfg)
    print(f"KERNEL {kernel_of(N, H)} sweep N={N} H={H} c={c} tau={tau} u={u:.5f}: feasible {feas.tolist()} "
          f"status {st.tolist()} iterations {it.tolist()}")
    gaps = []
    for b in range(B):
        if b == 1:
            assert _is_fallback(W, st, val, wp, b, 4), (b, st[b])
        elif not feas[b]:
            assert _is_fallback(W, st, val, wp, b, 2), (b, st[b])
        else:
            assert st[b] == 0, (b, st[b])
            gaps.append(_certified(W[b], wp[b], y[b], c, tau, u, val[b]))
    print(f"KERNEL {kernel_of(N, H)} sweep N={N} H={H} case {k}: gap {max(gaps):.3e} "
          f"iterations {it[solved].min()}..{it[solved].max()}")
    assert W[solved].max() > u - 1e-6                        # the limit binds
    # the non-finite and the infeasible windows do not touch their neighbours
    alone = _solve(wp[solved], y[solved], cfg)
    assert _same(alone, (W[solved], st[solved], val[solved], it[solved]))


# ---- (e) BASELINE configs[4]'s shape ---------------------------------------------------------------

def test_properties_at_the_c5_shape():
    B, N, H, c, tau, u = 4, 500, 20, 1e-3, 0.2, 0.01
    rng = np.random.default_rng(7)
    wp = 0.2 * rng.dirichlet(np.ones(N), B) + 0.8 / N
    assert wp.max() < u   # holding is feasible
    y = rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32)
    cfg = _cfg(H, c, tau, u)
    W, st, val, it = _solve(wp, y, cfg)
    print(f"KERNEL {kernel_of(N, H)} C5 shape: status {st.tolist()} iterations {it.tolist()}")
    assert (st == 0).all()
    for b in range(B):
        assert not box_ref.violated(W[b], wp[b], tau, u), b
        assert abs(val[b] - box_ref.reference_objective(W[b], wp[b], y[b], c)) <= 1e-12
        hold = box_ref.reference_objective(np.tile(wp[b], (H, 1)), wp[b], y[b], c)
        assert val[b] >= hold - 1e-9
    assert W.max() > u - 1e-6   # the limit binds
    for b in (0, B - 1):
        gp = _certified(W[b], wp[b], y[b], c, tau, u, val[b])
        print(f"  window {b}: gap {gp:.3e}")
    assert _same((W, st, val, it), _solve(wp, y, cfg))


# ---- (f) more windows than slabs ---------------------------------------------------------------------

def test_slab_reuse_past_the_slot_count():
    """B = 800 windows on 768 slabs: the windows past the first round start in a slab another
    window left behind (a stale L5 or RC5 would show), and must equal themselves solved in a batch
    of 8, bit for bit."""
    B, N, H, c, tau = 800, 12, 11, 1e-3, 0.3
    u = 2.5 / N
    rng = np.random.default_rng(12011)
    wp = 0.5 * rng.dirichlet(np.ones(N), B) + 0.5 / N
    y = rng.normal(5e-4, 0.02, (B, H, N)).astype(np.float32)
    # every window is feasible, away from the edge: period 0 can trade the excess above the limit
    assert (2 * np.maximum(wp - u, 0.0).sum(-1) <= tau - 0.02).all()
    cfg = _cfg(H, c, tau, u)
    W, st, val, it = _solve(wp, y, cfg)
    print(f"KERNEL {kernel_of(N, H)} slab reuse: status {np.bincount(st).tolist()} iterations {it.min()}..{it.max()}")
    assert (st == 0).all()
    assert W.max() > u - 1e-6 and W.max() <= u + 1e-9
    for b0 in (0, 392, 760, 768, 776, 792):
        s = slice(b0, b0 + 8)
        assert _same(_solve(wp[s], y[s], cfg), (W[s], st[s], val[s], it[s])), b0
    for b in (3, 770, 799):
        _certified(W[b], wp[b], y[b], c, tau, u, val[b])


# ---- (g) the C entry ------------------------------------------------------------------------------------

def _ws_c(wp, y, cfg, u, full=True, ws="query", short_by=0, iters=True, entry="kmpc_solve_box_ws"):
    """kmpc_solve_box_ws (or kmpc_solve / kmpc_solve_box) itself. Outputs are pre-filled with
    sentinels. Returns (rc, W, status, value, iters)."""
    dev = torch.device("cuda")
    L = _lib.load()
    yt = torch.as_tensor(y, device=dev).contiguous()
    wt = torch.as_tensor(wp, device=dev).contiguous()
    B, H, N = yt.shape
    W = torch.full((B, H, N) if full else (B, N), -7.0, dtype=torch.float64, device=dev)
    st = torch.full((B,), -7, dtype=torch.int32, device=dev)
    val = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
    it = torch.full((B,), -7, dtype=torch.int32, device=dev)
    d = _solve_desc(B, N, H, cfg, full)
    sh = _lib.stream_handle(dev)
    ip = it.data_ptr() if iters else None
    if entry == "kmpc_solve_box":
        rc = L.kmpc_solve_box(ctypes.byref(d), u, yt.data_ptr(), wt.data_ptr(), W.data_ptr(), st.data_ptr(),
                              val.data_ptr(), ip, sh)
    else:
        need = int(L.kmpc_solve_box_workspace_bytes(ctypes.byref(d), u)) if entry == "kmpc_solve_box_ws" else \
            int(L.kmpc_workspace_bytes(None, ctypes.byref(d)))
        buf = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        p = None if ws is None else buf.data_ptr()
        if entry == "kmpc_solve_box_ws":
            rc = L.kmpc_solve_box_ws(ctypes.byref(d), u, yt.data_ptr(), wt.data_ptr(), W.data_ptr(), st.data_ptr(),
                                     val.data_ptr(), ip, p, need - short_by, sh)
        else:
            rc = L.kmpc_solve(ctypes.byref(d), yt.data_ptr(), wt.data_ptr(), W.data_ptr(), st.data_ptr(),
                              val.data_ptr(), ip, p, need, sh)
    torch.cuda.synchronize()
    return rc, W.cpu().numpy(), st.cpu().numpy(), val.cpu().numpy(), it.cpu().numpy()


def _c_inputs(N, H, B, seed):
    rng = np.random.default_rng(seed)
    return 0.5 * rng.dirichlet(np.ones(N), B) + 0.5 / N, rng.normal(5e-4, 0.015, (B, H, N)).astype(np.float32)


def test_c_workspace_rule_writes_nothing():
    wp, y = _c_inputs(300, 5, 2, 1)
    cfg = _cfg(5, 1e-3, 0.2, 0.0, path=0)
    for kw in (dict(ws=None), dict(short_by=1)):
        rc, W, st, val, it = _ws_c(wp, y, cfg, 2.5 / 300, **kw)
        assert rc == -3, kw
        assert (W == -7).all() and (st == -7).all() and (val == -7).all() and (it == -7).all()
    rc, W, st, val, it = _ws_c(wp, y, cfg, 2.5 / 300)
    assert rc == 0 and (st == 0).all() and W.max() <= 2.5 / 300 + 1e-9 and (it > 0).all()


def test_c_register_shape_is_kmpc_solve_box_bit_for_bit():
    g = np.load(os.path.join(GOLD, "box_N100_H10.npz"))
    c, tau, u = (float(v) for v in g["config"])
    cfg = _cfg(10, c, tau, 0.0, path=0)
    a = _ws_c(g["w_prev"], g["yhat"], cfg, u, ws=None)   # (the workspace is not read)
    b = _ws_c(g["w_prev"], g["yhat"], cfg, u, entry="kmpc_solve_box")
    assert a[0] == b[0] == 0 and _same(a[1:], b[1:])
    assert (a[2] == [0 if f else 2 for f in g["feasible"]]).all()


def test_c_inactive_bound_is_kmpc_solve_with_the_workspace_bit_for_bit():
    wp, y = _c_inputs(300, 5, 3, 2)
    cfg = _cfg(5, 1e-3, 0.2, 0.0, path=0)
    for u in (1.0, 3.0):
        a = _ws_c(wp, y, cfg, u)
        b = _ws_c(wp, y, cfg, u, entry="kmpc_solve")
        assert a[0] == b[0] == 0 and _same(a[1:], b[1:])
        assert (a[2] == 0).all()


def test_c_iters_may_be_null_and_w0_is_the_first_period():
    wp, y = _c_inputs(300, 11, 3, 3)
    cfg = _cfg(11, 1e-3, 0.2, 0.0, path=0)
    u = 2.5 / 300
    full = _ws_c(wp, y, cfg, u)
    noit = _ws_c(wp, y, cfg, u, iters=False)
    assert full[0] == noit[0] == 0 and _same(full[1:4], noit[1:4]) and (noit[4] == -7).all()
    first = _ws_c(wp, y, cfg, u, full=False)
    assert first[0] == 0 and first[1].shape == (3, 300)
    assert np.array_equal(first[1], full[1][:, 0]) and _same(first[2:], full[2:])
    assert (full[2] == 0).all() and full[1].max() > u - 1e-6


# ---- (h) the layers: N = 10, H = 5, P = 4 paths, 12 steps on the large-window box kernel ----------------

def test_window_and_rebalance_batch_carry_the_limit_on_the_large_path():
    km, x, r, mean, std = _layers()
    cfg = _cfg(H_, 1e-3, 0.2, U_)
    reg = dataclasses.replace(cfg, solver_path=0)
    env = _Env(x[0].cpu().numpy(), N_, mean, std)
    ts = list(range(S_))
    wp = np.random.default_rng(3).dirichlet(np.ones(N_), S_)
    wp = np.minimum(wp, 0.2)
    wp /= wp.sum(1, keepdims=True)
    W0, st, val = _strat(cfg).rebalance_batch(ts, wp, env, return_info=True)
    assert (st == 0).all() and W0.max() <= U_ + 1e-9 and np.abs(W0.sum(1) - 1).max() <= 1e-8
    assert W0.max() > U_ - 1e-6                                # the limit binds
    Wr, str_, valr = _strat(reg).rebalance_batch(ts, wp, env, return_info=True)
    assert (str_ == 0).all()
    assert (np.abs(val - valr) <= 1e-6 + 1e-5 * np.abs(valr)).all()
    assert np.abs(W0 - Wr).max() < 1e-3
    # = kmpc_rollout, then kmpc_solve_box_ws, bit for bit
    y = km.rollout(x[0][:S_], mean, std, H_, N_)
    rc, Wc, stc, valc, _ = _ws_c(wp, y.cpu().numpy(), cfg, U_, full=False)
    assert rc == 0
    assert np.array_equal(W0, Wc) and np.array_equal(st, stc) and np.array_equal(val, valc)
    # DeviceKoopman.window with yhat and iterations kept
    Ww, stw, valw, yw, itw = km.window(x[0][:S_], torch.as_tensor(wp).cuda(), mean, std, N_, cfg, keep_yhat=True,
                                       with_iters=True)
    assert torch.equal(yw, y) and np.array_equal(Ww.cpu().numpy(), W0) and itw.shape == (S_,)
    assert np.array_equal(valw.cpu().numpy(), val)


def test_lockstep_backtest_carries_the_limit_on_the_large_path():
    km, x, r, mean, std = _layers()
    cfg = _cfg(H_, 1e-3, 0.2, U_)
    out = run_backtest_lockstep(_strat(cfg), x, r, BacktestConfig(horizon=H_), mean, std)
    assert out["portfolio_value"].shape == (P_, S_)
    # the per-step loop by hand: one rollout of the S x P windows, then kmpc_solve_box_ws and
    # kmpc_backtest_step per step
    dev = x.device
    L = _lib.load()
    xt, rt = x.transpose(0, 1).contiguous(), r.transpose(0, 1).contiguous()
    T = x.shape[1]
    y = km.rollout(xt[:S_].reshape(S_ * P_, -1), mean, std, H_, N_).reshape(S_, P_, H_, N_)
    w = torch.full((P_, N_), 1.0 / N_, dtype=torch.float64, device=dev)
    value = torch.full((P_,), float(BacktestConfig().initial_capital), dtype=torch.float64, device=dev)
    hist = torch.empty((P_, S_, 4), dtype=torch.float64, device=dev)
    bd = _lib.BacktestDesc(P_, N_, S_, float(BacktestConfig().cost_coeff))
    sd = _solve_desc(P_, N_, H_, cfg, False)
    W0 = torch.empty((P_, N_), dtype=torch.float64, device=dev)
    st = torch.empty(P_, dtype=torch.int32, device=dev)
    ob = torch.empty(P_, dtype=torch.float64, device=dev)
    nws = int(L.kmpc_solve_box_workspace_bytes(ctypes.byref(sd), U_))
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    sh = _lib.stream_handle(dev)
    wmax, first = 0.0, None
    for k in range(S_):
        assert L.kmpc_solve_box_ws(ctypes.byref(sd), U_, y[k].data_ptr(), w.data_ptr(), W0.data_ptr(), st.data_ptr(),
                                   ob.data_ptr(), None, ws.data_ptr(), nws, sh) == 0
        assert (st == 0).all()
        wmax = max(wmax, float(W0.max()))
        if k == 0:
            first = (W0.cpu().numpy().copy(), ob.cpu().numpy().copy())
        rn = rt[k + 1] if k + 1 < T else None
        assert L.kmpc_backtest_step(ctypes.byref(bd), k, W0.data_ptr(), rn.data_ptr() if rn is not None else None,
                                    w.data_ptr(), value.data_ptr(), hist.data_ptr(), sh) == 0
    torch.cuda.synchronize()
    assert U_ - 1e-6 < wmax <= U_ + 1e-9                       # every step's target under the limit, which binds
    for j, k in enumerate(KEYS[:4]):
        assert torch.equal(out[k], hist[..., j]), k
    assert torch.equal(out["weights"], w)
    # the register-box run of the same config: the first step's windows (the same inputs) at the
    # objective bar, the final value to 1e-6 relative
    reg = dataclasses.replace(cfg, solver_path=0)
    w1 = np.full((P_, N_), 1.0 / N_)
    Wr, str_, valr, _ = _solve(w1, y[0].cpu().numpy(), reg, full=False)
    assert (str_ == 0).all()
    assert (np.abs(first[1] - valr) <= 1e-6 + 1e-5 * np.abs(valr)).all()
    assert np.abs(first[0] - Wr).max() < 1e-3
    ref = run_backtest_lockstep(_strat(reg), x, r, BacktestConfig(horizon=H_), mean, std)
    a, b = out["portfolio_value"][:, -1], ref["portfolio_value"][:, -1]
    print(f"final value, large vs register box: relative difference {((a - b).abs() / b.abs()).max().item():.3e}")
    assert ((a - b).abs() <= 1e-6 * b.abs()).all()
    # no persistent kernel carries the limit on this path
    with pytest.raises(ValueError):
        run_backtest_lockstep(_strat(cfg), x, r, BacktestConfig(horizon=H_), mean, std, persistent=True)
