"""kmpc_backtest_metrics (bt_metrics_kernel, one thread per path, sequential sums) against
calculate_metrics in long double (tests/bt_step_ref.metrics).

Bars (u = 2^-53, e = (S + 4) u: a sequential sum of S terms, each after at most 3 roundings of its
own, is within e sum|term| of the exact one; tests/test_bt_metrics_gpu.metric_bars):

    mean = sum r / S                 e_mean = e sum|r_k| / S
    var  = sum (r_k - mean)^2 / S    e_var  = (e sum d_k^2 + 2 e_mean sum|d_k|) / S + e_mean^2, d_k = r_k - mean
                                     (the last term is second order: with constant returns every d_k
                                     is 0 in the reference and the first-order terms vanish, while the
                                     device's d_k is its mean's error)
    sd   = sqrt(var)                 e_sd   = min(e_var / (2 sd), sqrt(e_var))   (|sqrt a - sqrt b| <= sqrt|a - b|)
    Sharpe = sqrt(252) mean / (sd + 1e-8):
                                     sqrt(252) (e_mean / (sd + 1e-8) + |mean| e_sd / (sd + 1e-8)^2) + 4 u |Sharpe|
    Avg Turnover = sum t / S         e sum|t_k| / S
    Final Value                      0 (a copy)
    Total Return = last / first - 1  4 u (|last / first| + 1)
    Max Drawdown = min (cum_k - peak_k) / peak_k, cum_k = prod_{j<=k} (1 + r_j): cum_k carries 2 k
        roundings (one per 1 + r_j, one per product), so cum_k and peak_k are each within 2 S u
        relative, their difference within 2 S u (|cum_k| + |peak_k|), and with the subtraction's and the
        division's own roundings          (4 S + 4) u max_k (|cum_k / peak_k| + 1)
        (min and max are 1-Lipschitz in the sup norm, so a tie broken the other way costs no more).

NaN rule: numpy's maximum.accumulate and min propagate NaN; so must the kernel's running peak and
running minimum. NaN-ness of every metric equals the reference's.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import bt_metrics_cases as cases
import bt_step_ref as ref
from koopman_mpc_portfolio_rebalancing_amd import _lib

pytestmark = pytest.mark.gpu
LD = ref.LD
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def metric_bars(r, t, pv):
    r, t, pv = (np.asarray(x, dtype=LD) for x in (r, t, pv))
    S = len(r)
    u, e = ref.U, (S + 4) * ref.U
    with np.errstate(all="ignore"):
        mean = np.sum(r) / S
        e_mean = e * np.sum(np.abs(r)) / S
        d = r - mean
        e_var = (e * np.sum(d * d) + 2 * e_mean * np.sum(np.abs(d))) / S + e_mean * e_mean
        sd = np.sqrt(np.sum(d * d) / S)
        e_sd = min(e_var / (2 * sd), np.sqrt(e_var)) if sd > 0 else np.sqrt(e_var)
        den = sd + ref.GUARD
        sharpe = np.sqrt(LD(252)) * mean / den
        b_sharpe = np.sqrt(LD(252)) * (e_mean / den + np.abs(mean) * e_sd / (den * den)) + 4 * u * np.abs(sharpe)
        cum = np.cumprod(1 + r)
        peak = np.maximum.accumulate(cum)
        b_mdd = (4 * S + 4) * u * np.max(np.abs(cum / peak) + 1)
        b_turn = e * np.sum(np.abs(t)) / S
        b_tr = 4 * u * (np.abs(pv[-1] / pv[0]) + 1)
    bars = np.array([b_sharpe, b_mdd, b_turn, LD(0), b_tr], dtype=LD)
    return np.where(np.isfinite(bars), bars, LD(0))


def compare(hist, met):
    """Every path against the reference; returns the largest error / bar per metric."""
    worst = np.zeros(5)
    for p in range(hist.shape[0]):
        want = ref.metrics(hist[p, :, 1], hist[p, :, 2], hist[p, :, 0])
        bars = metric_bars(hist[p, :, 1], hist[p, :, 2], hist[p, :, 0])
        for j, name in enumerate(ref.METRICS):
            assert np.isnan(met[p, j]) == np.isnan(want[j]), (p, name, met[p, j], want[j])
            worst[j] = max(worst[j], ref.error_ratio(met[p, j], want[j], bars[j]))
    return worst


def report(what, worst):
    print(what + ": largest error / bar " + ", ".join(f"{n} {w:.3f}" for n, w in zip(ref.METRICS, worst)))
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("P", [1, 255, 256, 257])
@pytest.mark.parametrize("S", [1, 2, 40, 4096])
def test_finite_histories(S, P):
    """Path p has kind FINITE[p % 7] and draws of its own: a wrong path stride or a ragged last block
    of the 256-thread launch shows as another path's metrics. (At S = 1 the wipeout kind is a first
    step of -100 %: NaN on both sides.)"""
    hist = cases.paths(P, S, 1, cases.FINITE)
    report(f"S = {S}, P = {P}", compare(hist, cases.device_metrics(hist)))


@pytest.mark.parametrize("kind", cases.FINITE)
def test_each_kind_alone(kind):
    """One kind per launch at S = 40, so that a failure names it; what each was built for holds."""
    hist = cases.paths(9, 40, 2, (kind,))
    met = cases.device_metrics(hist)
    report(kind, compare(hist, met))
    if kind == "zero":
        assert (met[:, 1] == 0).all()
    if kind == "up":
        # every step is a new peak. The compiler contracts cum - peak into fma(cum', 1 + r, -peak), the
        # product's rounding residual, so the device's drawdown there is within u of 0, not 0 itself
        assert (met[:, 1] <= 0).all() and (met[:, 1] >= -2.0 ** -53).all()
    if kind == "peak0":
        assert (met[:, 1] < 0).all() and np.argmax(hist[0, :, 0]) == 0
    if kind == "wipeout":
        assert (met[:, 1] == -1).all() and (met[:, 4] == -1).all() and (met[:, 3] == 0).all()
    if kind == "below":
        assert (np.cumprod(1 + hist[:, :, 1], axis=1).min(axis=1) < 0).all()
    if kind == "const":
        assert np.allclose(met[:, 0], np.sqrt(252) * 0.01 / 1e-8, rtol=1e-6)


@pytest.mark.parametrize("S", [2, 40])
@pytest.mark.parametrize("kind", cases.NANS)
def test_nan_and_zero_peak(kind, S):
    """A NaN return at k = 0, in the middle or at the end, and a first step of exactly -100 %: the
    reference's Max Drawdown is NaN (np.maximum.accumulate, np.min; 0 / 0), and the kernel's must be."""
    hist = cases.paths(5, S, 3, (kind,))
    met = cases.device_metrics(hist)
    want = ref.metrics(hist[0, :, 1], hist[0, :, 2], hist[0, :, 0])
    assert np.isnan(want[1])
    print(f"{kind}, S = {S}: device Max Drawdown {met[:, 1].tolist()}")
    report(f"{kind}, S = {S}", compare(hist, met))
    assert np.isnan(met[:, 1]).all()


def test_nan_paths_leave_their_neighbours_alone():
    """All eleven kinds side by side over the block edge: the NaN paths' neighbours are measured."""
    hist = cases.paths(257, 40, 4)
    report("mixed, P = 257", compare(hist, cases.device_metrics(hist)))


def test_no_steps():
    """S = 0 through the C call: five NaNs per path, and nothing else written."""
    P, pad = 257, 1024
    buf = torch.full((P * 5 + 2 * pad,), -7.25e77, dtype=torch.float64, device="cuda")
    hist = torch.zeros(8, dtype=torch.float64, device="cuda")
    d = _lib.BacktestDesc(P, 4, 0, 1e-3)
    _lib.check(_lib.load().kmpc_backtest_metrics(ctypes.byref(d), hist.data_ptr(), buf[pad:].data_ptr(), None))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.isnan(out[pad:pad + P * 5]).all()
    assert (out[:pad] == -7.25e77).all() and (out[pad + P * 5:] == -7.25e77).all()


def test_metrics_outputs_are_fenced():
    """P = 257, S = 40 inside a sentinel: exactly the [P, 5] metrics are written."""
    P, pad = 257, 1024
    hist = cases.paths(P, 40, 5, cases.FINITE)
    buf = torch.full((P * 5 + 2 * pad,), -7.25e77, dtype=torch.float64, device="cuda")
    h = torch.tensor(hist, device="cuda")
    d = _lib.BacktestDesc(P, 4, 40, 1e-3)
    _lib.check(_lib.load().kmpc_backtest_metrics(ctypes.byref(d), h.data_ptr(), buf[pad:].data_ptr(), None))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:pad] == -7.25e77).all() and (out[pad + P * 5:] == -7.25e77).all()
    assert np.array_equal(out[pad:pad + P * 5].reshape(P, 5), cases.device_metrics(hist))
    assert np.array_equal(h.cpu().numpy(), hist)


@pytest.mark.parametrize("S", cases.GOLDEN_S)
def test_finite_metrics_keep_the_parent_bits(S):
    """tests/golden/bt_metrics_parent.npz: the metrics of golden_hist(S) from the library before the
    NaN rule changed. Histories without NaN and with non-zero peaks keep every bit."""
    g = np.load(os.path.join(GOLD, "bt_metrics_parent.npz"))
    hist = cases.golden_hist(S)
    assert np.isfinite(hist).all()
    met = cases.device_metrics(hist)
    assert np.isfinite(met).all()
    assert met.tobytes() == g[f"S{S}"].tobytes()
    report(f"golden S = {S}", compare(hist, met))
