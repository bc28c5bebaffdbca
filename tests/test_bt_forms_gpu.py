"""Stress rows through the two forms of the bookkeeping step that cannot be called alone: the wide
form (bt_step_body(..., nt) inside mv_bt_kernel and mv_band_bt_kernel) and the lane-group form
(bt_step_group<16 / 32> inside the packed persistent kernels), and through the block form inside the
register persistent kernels. The realized rows are an input independent of the forecasts, so every
persistent run is driven with engineered rows and held to what the project guarantees: bit identity
with the per-step loop of the solve call and kmpc_backtest_step, on every history column, the final
weights, the metrics and the last step's solve outputs.

Row schedule, S = 10 steps, P = 3 paths (step k reads realized row k + 1; steps 0-3 hold in the
mean-variance families, which need 5 past rows):

    k = 0..3  benign, y ~ N(5e-4, 0.015)
    k = 4     y ~ N(0, 0.3)
    k = 5     benign with one asset (another per path) at y = -110: R = 0, the asset's weight drifts
              to exactly 0 and the next window's w_prev holds a zero
    k = 6, 7  benign
    k = 8     every asset at y = -110: port = -1, the guard fires inside the persistent kernel, the
              weights become exactly 0 and the last window starts from w_prev = 0
    k = 9     no realized row

Beyond bit identity: every solve up to and including step 8's ends optimal (where the family reports
statuses), the crashed asset's weight is exactly 0 before step 6, step 8's return is within 1e-12 of
-1 and the weights after it are exactly 0. For the two Markowitz shapes whose solve block is wider
than the bookkeeping's, the loop's per-step targets are replayed through tests/bt_step_ref.step from
the loop's own pre-step state, and the persistent run's history is held to the bars of
tests/test_bt_step_gpu.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bt_step_ref as ref
import test_koopman_mv_gpu as kmv
import test_markowitz_bt_gpu as mk
from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, KoopmanMVStrategy, _lib, run_koopman_mv_lockstep,
                                                   run_markowitz_lockstep)
from koopman_mpc_portfolio_rebalancing_amd.backtest import METRIC_NAMES

pytestmark = pytest.mark.gpu
P, S = 3, 10
K_WIDE, K_ONE, K_ALL = 4, 5, 8
C, TAU, BTC, V0 = 1e-3, 0.2, 1e-3, 10000.0
COLS = ("portfolio_value", "return", "turnover", "cost")


def crashed_asset(p, N):
    return (1 + 3 * p) % N


@functools.lru_cache(maxsize=None)
def realized_rows(N):
    """[P, S, N] float32: the row step k reads is [:, k + 1] (row 0 is never read)."""
    rng = np.random.default_rng(31 * N + 7)
    r = rng.normal(5e-4, 0.015, (P, S, N)).astype(np.float32)
    r[:, K_WIDE + 1] = rng.normal(0.0, 0.3, (P, N)).astype(np.float32)
    for p in range(P):
        r[p, K_ONE + 1, crashed_asset(p, N)] = -110.0
    r[:, K_ALL + 1] = -110.0
    return r


def same_bits(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_metrics(hist):
    met = torch.empty((P, 5), dtype=torch.float64, device="cuda")
    d = _lib.BacktestDesc(P, 4, S, BTC)
    _lib.check(_lib.load().kmpc_backtest_metrics(ctypes.byref(d), hist.data_ptr(), met.data_ptr(), None))
    torch.cuda.synchronize()
    return met


def assert_stress_outcomes(what, N, hist, w_pre, statuses):
    """hist [P, S, 4], w_pre [S + 1, P, N] (the weights before each step and after the last),
    statuses [S, P] with -1 where the step held without a solve."""
    hist, w_pre = np.asarray(hist), np.asarray(w_pre)
    if statuses is not None:
        solved = statuses[:K_ALL + 1]
        print(f"{what}: statuses per step {statuses.T.tolist()}")
        assert ((solved == 0) | (solved == -1)).all(), statuses      # a window that is not optimal is a finding
        assert (statuses[K_WIDE:K_ALL + 1] == 0).all()
    assert np.isfinite(hist[:, :K_ALL + 1]).all()
    assert (hist[:, K_WIDE:K_ALL + 1, 2] > 0).all()                  # the solved steps trade
    for p in range(P):
        assert w_pre[K_ONE + 1, p, crashed_asset(p, N)] == 0         # exactly 0 into the next window
        assert (np.delete(w_pre[K_ONE + 1, p], crashed_asset(p, N)) > 0).any()
    print(f"{what}: all-crash return + 1 = {(hist[:, K_ALL, 1] + 1).tolist()}")
    assert (np.abs(hist[:, K_ALL, 1] + 1) <= 1e-12).all()
    assert (w_pre[K_ALL + 1] == 0).all()                             # the guard fired: tg * 0f / 1e-8
    assert (hist[:, S - 1, 1] == 0).all()                            # no realized row at the end


# ---- log-utility: kmpc_backtest_run / kmpc_backtest_run_box against kmpc_solve(_box) + kmpc_backtest_step ----

def _sdesc(N, H, path):
    sd = _lib.SolveDesc()
    sd.B, sd.N, sd.H, sd.cost_coeff, sd.max_turnover, sd.path = P, N, H, C, TAU, path
    return sd


class _State:
    def __init__(self, N):
        f64 = dict(dtype=torch.float64, device="cuda")
        self.w = torch.full((P, N), 1.0 / N, **f64)
        self.value = torch.full((P,), V0, **f64)
        self.hist = torch.zeros((P, S, 4), **f64)
        self.target = torch.zeros((P, N), **f64)
        self.status = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        self.obj = torch.zeros((P,), **f64)

    def tail(self):
        return (self.w.data_ptr(), self.value.data_ptr(), self.hist.data_ptr(), self.target.data_ptr(),
                self.status.data_ptr(), self.obj.data_ptr(), _lib.stream_handle(self.w.device))


def forecasts(N, H):
    rng = np.random.default_rng(1000 * N + H)
    return torch.as_tensor(rng.normal(5e-4, 0.015, (S, P, H, N)).astype(np.float32)).cuda()


def log_utility_loop(N, H, path, u):
    L = _lib.load()
    y, r = forecasts(N, H), torch.as_tensor(realized_rows(N)).cuda().transpose(0, 1).contiguous()   # r [S, P, N]
    st = _State(N)
    bd, sd = _lib.BacktestDesc(P, N, S, BTC), _sdesc(N, H, path)
    sh = _lib.stream_handle(y.device)
    w_pre, statuses = [], []
    for k in range(S):
        w_pre.append(st.w.clone())
        io = (y[k].data_ptr(), st.w.data_ptr(), st.target.data_ptr(), st.status.data_ptr(), st.obj.data_ptr())
        if u:
            _lib.check(L.kmpc_solve_box(ctypes.byref(sd), u, *io, None, sh))
        else:
            _lib.check(L.kmpc_solve(ctypes.byref(sd), *io, None, None, 0, sh))
        statuses.append(st.status.clone())
        rn = r[k + 1].data_ptr() if k < S - 1 else None
        _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), k, st.target.data_ptr(), rn, st.w.data_ptr(),
                                        st.value.data_ptr(), st.hist.data_ptr(), sh))
    torch.cuda.synchronize()
    w_pre.append(st.w.clone())
    return st, torch.stack(w_pre).cpu().numpy(), torch.stack(statuses).cpu().numpy()


def log_utility_run(N, H, path, u):
    L = _lib.load()
    y, r = forecasts(N, H), torch.as_tensor(realized_rows(N)).cuda().transpose(0, 1).contiguous()
    rr = r[1:S].contiguous()                                     # the rows of steps 0 .. S - 2
    st = _State(N)
    bd, sd = _lib.BacktestDesc(P, N, S, BTC), _sdesc(N, H, path)
    if u:
        rc = L.kmpc_backtest_run_box(ctypes.byref(bd), ctypes.byref(sd), u, 0, S, y.data_ptr(), rr.data_ptr(), S - 1, *st.tail())
    else:
        rc = L.kmpc_backtest_run(ctypes.byref(bd), ctypes.byref(sd), 0, S, y.data_ptr(), rr.data_ptr(), S - 1, *st.tail())
    _lib.check(rc)
    torch.cuda.synchronize()
    return st


LOG_UTILITY = [(10, 5, 1, False, "bt_step_group<16>, lanes 10..15 off"), (20, 10, 1, False, "bt_step_group<32>"),
               (100, 10, 0, False, "C3 block form"), (230, 10, 0, False, "256-thread block"),
               (40, 5, 0, True, "box run kernel")]


@pytest.mark.parametrize("N,H,path,box,form", LOG_UTILITY, ids=[f"N{c[0]}_H{c[1]}{'_box' if c[3] else ''}" for c in LOG_UTILITY])
def test_log_utility_run_equals_the_loop(N, H, path, box, form):
    u = 2.5 / N if box else 0.0
    loop, w_pre, statuses = log_utility_loop(N, H, path, u)
    run = log_utility_run(N, H, path, u)
    for k in ("hist", "w", "value", "target", "status", "obj"):
        assert same_bits(getattr(loop, k), getattr(run, k)), (form, k)
    assert same_bits(device_metrics(loop.hist), device_metrics(run.hist))
    assert_stress_outcomes(f"N = {N}, H = {H} ({form})", N, run.hist.cpu().numpy(), w_pre, statuses)
    print(f"last window, from w_prev = 0: statuses {run.status.tolist()}")


# ---- Markowitz: kmpc_markowitz_run against the four C calls per step ----------------------------------------

def markowitz_loop(z, mean, std, realized, N, H):
    """test_markowitz_bt_gpu.hand_loop, keeping each step's target, status and pre-step state."""
    L = _lib.load()
    dev = torch.device("cuda")
    T = z.shape[1]
    zt, rt = torch.tensor(z, device=dev), torch.tensor(realized, device=dev)
    m, sd = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    w, value = torch.full((P, N), 1.0 / N, **f64), torch.full((P,), V0, **f64)
    hist, met = torch.empty((P, S, 4), **f64), torch.empty((P, 5), **f64)
    mu, sigma = torch.empty((P, N), **f64), torch.empty((P, N, N), **f64)
    valid = torch.empty((P,), dtype=torch.int32, device=dev)
    W0, obj = torch.empty((P, N), **f64), torch.empty((P,), **f64)
    st = torch.empty((P,), dtype=torch.int32, device=dev)
    md = _lib.MvDesc()
    md.B, md.N, md.H, md.gamma, md.cost_coeff, md.max_iter, md.tol = P, N, H, 1.0, 1e-3, 100, 1e-10
    nws = int(L.kmpc_mv_workspace_bytes(ctypes.byref(md)))
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
    bd = _lib.BacktestDesc(P, N, S, BTC)
    targets, statuses, w_pre, v_pre = [], [], [], []
    for k in range(S):
        tt = torch.tensor([k], dtype=torch.int32, device=dev)
        for p in range(P):
            _lib.check(L.kmpc_rolling_moments(1, T, N, 60, zt[p].data_ptr(), zt.shape[2], m.data_ptr(), sd.data_ptr(),
                                              tt.data_ptr(), mu[p].data_ptr(), sigma[p].data_ptr(),
                                              valid[p:].data_ptr(), None))
        muH = mu[:, None, :].expand(P, H, N).contiguous()
        _lib.check(L.kmpc_solve_mv_ws(ctypes.byref(md), muH.data_ptr(), sigma.data_ptr(), N * N, w.data_ptr(), W0.data_ptr(),
                                      st.data_ptr(), obj.data_ptr(), None, ws.data_ptr(), nws, None))
        tg = torch.where((valid == 0).unsqueeze(1), w, W0)
        targets.append(tg.clone())
        statuses.append(torch.where(valid == 0, torch.full_like(st, -1), st))
        w_pre.append(w.clone())
        v_pre.append(value.clone())
        rn = rt[:, k + 1].contiguous() if k + 1 < T else None
        _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), k, tg.data_ptr(), rn.data_ptr() if rn is not None else None,
                                        w.data_ptr(), value.data_ptr(), hist.data_ptr(), None))
    _lib.check(L.kmpc_backtest_metrics(ctypes.byref(bd), hist.data_ptr(), met.data_ptr(), None))
    torch.cuda.synchronize()
    w_pre.append(w.clone())
    out = {k: hist[..., i] for i, k in enumerate(COLS)}
    out["weights"] = w
    out["metrics"] = {name: met[:, j] for j, name in enumerate(METRIC_NAMES)}
    rec = {k: torch.stack(v).cpu().numpy() for k, v in (("targets", targets), ("statuses", statuses), ("w_pre", w_pre),
                                                        ("v_pre", v_pre))}
    return out, rec


def assert_same_run(a, b, what):
    for k in COLS + ("weights",):
        assert same_bits(a[k], b[k]), (what, k)
    for k, v in a["metrics"].items():
        assert same_bits(v, b["metrics"][k]), (what, k)


def hist_of(out):
    return np.stack([out[k].cpu().numpy() for k in COLS], axis=-1)


MARKOWITZ = [(10, 1, False, "block = bookkeeping width"), (40, 2, True, "128-thread solve over a 64-thread bookkeeping"),
             (129, 1, False, "slab, 192 bookkeeping threads"), (300, 1, True, "320 threads over 256 that stride")]


@pytest.mark.parametrize("N,H,chain,form", MARKOWITZ, ids=[f"N{c[0]}_H{c[1]}" for c in MARKOWITZ])
def test_markowitz_run_equals_the_loop(N, H, chain, form):
    z, mean, std, _ = mk.panel(N, P, S)
    realized = realized_rows(N)
    cfg = BacktestConfig(horizon=mk.HZ)
    per = run_markowitz_lockstep(mk.strategy(N, H), z, realized, cfg, mean, std, n_rows=S + mk.HZ, persistent=True)
    loop, rec = markowitz_loop(z, mean, std, realized, N, H)
    assert per["return"].shape == (P, S)
    assert_same_run(per, loop, form)
    hist = hist_of(per)
    assert_stress_outcomes(f"Markowitz N = {N}, H = {H} ({form})", N, hist, rec["w_pre"], rec["statuses"])
    assert (rec["statuses"][:4] == -1).all() and (hist[:, :4, 2] == 0).all()      # fewer than 5 rows: hold
    if not chain:
        return
    # closing the chain to the reference: the wide form's history within the block form's bars
    worst = 0.0
    w_last = per["weights"].cpu().numpy()
    for k in range(S):
        for p in range(P):
            y = realized[p, k + 1] if k + 1 < S else None
            args = (rec["targets"][k, p], rec["w_pre"][k, p], rec["v_pre"][k, p], y, BTC)
            w_ref, _, row_ref, _, _ = ref.step(*args)
            bar_w, bar_row = ref.step_bars(*args)
            worst = max(worst, ref.error_ratio(hist[p, k], row_ref, bar_row))
            w_dev = rec["w_pre"][k + 1, p] if k + 1 < S else w_last[p]
            worst = max(worst, ref.error_ratio(w_dev, w_ref, bar_w))
    print(f"Markowitz N = {N}, H = {H}: largest error / bar against the long-double step {worst:.3f}")
    assert worst <= 1.0


# ---- Koopman mean-variance band run: kmpc_koopman_mv_run against kmpc_solve_mv_band + kmpc_backtest_step ----

@pytest.mark.parametrize("N,H", [(10, 5), (65, 2)])
def test_koopman_mv_run_equals_the_loop(N, H):
    z, mean, std, _ = kmv.panel(N, P, S)
    realized = realized_rows(N)
    km, cfg = kmv.model(N), kmv.config(N, H, False)
    per = run_koopman_mv_lockstep(KoopmanMVStrategy(km, cfg), z, realized, BacktestConfig(horizon=kmv.HZ), mean, std,
                                  n_rows=S + kmv.HZ, persistent=True)
    loop, statuses = kmv.hand_loop(km, cfg, z, mean, std, realized, N, H, S)
    assert per["return"].shape == (P, S)
    assert_same_run(per, loop, "band run")
    # the weights before steps 6 and 9: the loop over the first 6 and the first 9 steps (every one with its row)
    w_pre = np.zeros((S + 1, P, N))
    w_pre[K_ONE + 1] = kmv.hand_loop(km, cfg, z, mean, std, realized, N, H, K_ONE + 1)[0]["weights"].cpu().numpy()
    w_pre[K_ALL + 1] = kmv.hand_loop(km, cfg, z, mean, std, realized, N, H, K_ALL + 1)[0]["weights"].cpu().numpy()
    assert_stress_outcomes(f"Koopman-MV N = {N}, H = {H}", N, hist_of(per), w_pre, statuses)
