"""Baselines on the device: DMD and Markowitz.

Mirrors ``DMDStrategy`` of the reference (baselines.py:127-187): the operator A of x_{t+1} = A x_t
is fitted once on the host exactly as the reference does (``X' @ scipy.linalg.pinv(X)`` on the
float32 training embeddings, baselines.py:145-166 — a one-off fit, not on the path); the rollout
x <- A x over the horizon, the extraction of the first N entries, the de-standardisation and the
log-utility MPC solve run on the device. The rollout is the Koopman kernel chain with an identity
encoder / decoder and the latent operator A^T (row-vector convention, z <- z @ A^T), so DMD shares
``kmpc_window`` with the Koopman strategy.

Mirrors ``MarkowitzStrategy`` (baselines.py:24-106): the rolling 60-row mean / covariance of the
de-standardized current returns (kmpc_rolling_moments) and the H = 1 mean-variance solve
(kmpc_solve_mv, mpc.py:119-184; kmpc_solve_mv_box under a per-asset position limit,
kmpc_solve_mv_cap under an L1 turnover cap) run on the
device, for one window (``rebalance``) or many (``rebalance_batch``). A whole Markowitz backtest of P
paths runs on the device too (``run_markowitz_lockstep``: every step of a path in one
kmpc_markowitz_run launch), as does a sweep of the baseline's two hyper-parameters over shared
moments (``run_markowitz_sweep`` / ``sweep_backtest_markowitz``: kmpc_markowitz_sweep). The rolling
covariance the mean-variance strategies read has a choice of estimator (``cov_estimator``: the
reference's sample covariance, Ledoit-Wolf, OAS or EWMA; kmpc_rolling_cov), routed in one place.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Any, Dict, Optional, Sequence

import numpy as np
import pandas as pd
import torch

from . import _lib
from .backtest import (METRIC_NAMES, PREROLL_CHUNK, BacktestConfig, KoopmanMPCStrategy, Strategy, _cache_hit,
                       _cache_key, _env_stats, _prepare_paths, _sweep_fields, run_backtest)
from .koopman import KoopmanModelSpec
from .mpc import (MPCConfig, _box_limit, _mv_band_program, _mv_desc, _mv_turnover_cap, _workspace,
                  solve_mpc_mean_variance_banded_batched, solve_mpc_mean_variance_batched)


def fit_dmd(train_data) -> np.ndarray:
    """A = X' pinv(X) with X = data[:-1]^T, X' = data[1:]^T (baselines.py:145-166), float32 in,
    computed by scipy.linalg.pinv as in the reference."""
    from scipy.linalg import pinv
    data = train_data.cpu().numpy() if torch.is_tensor(train_data) else np.asarray(train_data)
    X = data[:-1].T
    X_prime = data[1:].T
    return X_prime @ pinv(X)


def dmd_model_spec(A: np.ndarray) -> KoopmanModelSpec:
    """The DMD rollout as a Koopman model: identity encoder, latent operator A^T, identity decoder."""
    n = A.shape[0]
    eye = torch.eye(n, dtype=torch.float32)
    return KoopmanModelSpec(kind="generic", encoder=[(eye, None)], kmat=torch.as_tensor(A, dtype=torch.float32).t().contiguous(),
                            decoder=[(eye, None)], enc_act="relu", enc_last_relu=False, norm_fn="id")


class DMDStrategy(KoopmanMPCStrategy):
    """Dynamic Mode Decomposition strategy (baselines.py:127-187) on the device window path.

    Args:
        train_data: [samples, obs_size] training embeddings (env.train_dataset.data).
        mpc_config: MPCConfig for the log-utility solve.
        device: as KoopmanMPCStrategy ('cpu' selects the current GPU; there is no CPU path).
    """

    def __init__(self, train_data: Any, mpc_config: MPCConfig, device: str = "cpu"):
        self.K = fit_dmd(train_data)
        self.n_assets = None
        super().__init__(dmd_model_spec(self.K), mpc_config, device)


COV_ESTIMATORS = tuple(_lib.COV_ESTIMATOR)   # "sample", "ledoit_wolf", "oas", "ewma"


def _cov_estimator(estimator: str = "sample", ewma_lambda: float = 0.94) -> tuple:
    """(KMPC_COV_* code, lambda) of a covariance estimator's name; ValueError on an unknown name or,
    for "ewma", a lambda outside (0, 1] (the rules of kmpc_rolling_cov, before any device work)."""
    if estimator not in _lib.COV_ESTIMATOR:
        raise ValueError(f"unknown covariance estimator {estimator!r}: one of {', '.join(COV_ESTIMATORS)}")
    lam = float(ewma_lambda)
    if estimator == "ewma" and not (0.0 < lam <= 1.0):
        raise ValueError(f"ewma_lambda must lie in (0, 1] (got {ewma_lambda})")
    return _lib.COV_ESTIMATOR[estimator], lam


def _strategy_cov(strategy) -> tuple:
    """The (code, lambda) of a strategy's cov_estimator / cov_ewma_lambda ("sample" where it has none)."""
    return _cov_estimator(getattr(strategy, "cov_estimator", "sample"), getattr(strategy, "cov_ewma_lambda", 0.94))


def _rolling_cov_paths(cov: tuple, P: int, n: int, T: int, N: int, lookback: int, z, m, sd, ts, mu, sigma, valid,
                       sh) -> None:
    """The covariances of n test rows ts of the P panels z [P, T, ld] under the estimator cov
    (_cov_estimator) into mu [n, P, N], sigma [n, P, N, N], valid [n, P]: the one place the backtests
    route the estimator. "sample" is kmpc_rolling_moments_paths, the others kmpc_rolling_cov_paths."""
    L = _lib.load()
    head = (P, n, T, N, int(lookback), z.data_ptr(), int(z.shape[2]), m.data_ptr(), sd.data_ptr(), ts.data_ptr(),
            mu.data_ptr(), sigma.data_ptr(), valid.data_ptr())
    if cov[0] == _lib.COV_ESTIMATOR["sample"]:
        _lib.check(L.kmpc_rolling_moments_paths(*head, sh))
    else:
        _lib.check(L.kmpc_rolling_cov_paths(*head, cov[0], cov[1], None, sh))


def rolling_moments(z: torch.Tensor, ts, lookback: int, n_assets: int, mean=None, std=None,
                    estimator: str = "sample", ewma_lambda: float = 0.94, return_shrinkage: bool = False):
    """Markowitz moments on the device (baselines.py:70-88) for the windows t in ``ts``.

    Args:
        z: [T, >= N] float32 device tensor of standardized test rows (the first N columns are the
            current returns, data_finance.py:717-729).
        ts: test indices; window t uses rows max(0, t + 1 - lookback) .. t.
        mean, std: [N] de-standardization (data_finance.py:740-742); None -> identity.
        estimator: the covariance's estimator — "sample" (np.cov, the reference's), "ledoit_wolf",
            "oas" (shrinkage towards tr(S) / N I, as sklearn.covariance) or "ewma" (exponentially
            weighted with decay ``ewma_lambda`` in (0, 1]); kmpc_rolling_cov. mu does not depend on it.
            ValueError on an unknown name or a bad lambda, before any device work.
        return_shrinkage: also return the shrinkage rho [B] float64 (0 for "sample" and "ewma").

    Returns:
        mu [B, N] float64 (float32-rounded mean), sigma [B, N, N] float64 (the estimate + 1e-6 I),
        valid [B] int32 (t + 1 >= 5).
    """
    cov = _cov_estimator(estimator, ewma_lambda)
    _lib.require_gpu(z)
    dev = z.device
    N = int(n_assets)
    z = z.to(torch.float32)
    if z.dim() != 2 or z.shape[1] < N or z.stride(1) != 1:
        z = z.reshape(z.shape[0], -1).contiguous()
    T = int(z.shape[0])
    m = torch.zeros(N, dtype=torch.float32, device=dev) if mean is None else \
        torch.as_tensor(np.asarray(mean, np.float64).astype(np.float32), device=dev)
    sd = torch.ones(N, dtype=torch.float32, device=dev) if std is None else \
        torch.as_tensor(np.asarray(std, np.float64).astype(np.float32), device=dev)
    tt = torch.as_tensor(np.asarray(ts, np.int64).astype(np.int32), device=dev)
    B = int(tt.numel())
    mu = torch.empty((B, N), dtype=torch.float64, device=dev)
    sigma = torch.empty((B, N, N), dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    L = _lib.load()
    head = (B, T, N, int(lookback), z.data_ptr(), int(z.stride(0)), m.data_ptr(), sd.data_ptr(), tt.data_ptr(),
            mu.data_ptr(), sigma.data_ptr(), valid.data_ptr())
    rho = torch.empty(B, dtype=torch.float64, device=dev) if return_shrinkage else None
    with torch.cuda.device(dev):
        if estimator == "sample" and rho is None:
            rc = L.kmpc_rolling_moments(*head, _lib.stream_handle(dev))
        else:
            rc = L.kmpc_rolling_cov(*head, cov[0], cov[1], rho.data_ptr() if rho is not None else None,
                                    _lib.stream_handle(dev))
    _lib.check(rc)
    return (mu, sigma, valid, rho) if return_shrinkage else (mu, sigma, valid)


class _LimitKeyword(type(Strategy)):
    """``MarkowitzStrategy(..., max_weight=u, max_turnover=tau)``: the keywords are taken by the
    class call and applied with ``set_max_weight`` / ``set_max_turnover`` — ``__init__`` keeps the
    reference's three arguments exactly (baselines.py:33-37), as the drop-in surface promises."""

    def __call__(cls, *args, max_weight: float = 0.0, max_turnover: float = 0.0, cov_estimator: str = "sample",
                 cov_ewma_lambda: float = 0.94, **kwargs):
        _cov_estimator(cov_estimator, cov_ewma_lambda)   # (ValueError before the strategy exists)
        obj = super().__call__(*args, **kwargs)
        obj.set_max_weight(max_weight)
        obj.set_max_turnover(max_turnover)
        obj.set_cov_estimator(cov_estimator, cov_ewma_lambda)
        return obj


class MarkowitzStrategy(Strategy, metaclass=_LimitKeyword):
    """Classic mean-variance strategy (baselines.py:24-106) on the device.

    Same constructor and ``mpc_config`` (H = 1, gamma = risk_aversion, baselines.py:39-45);
    ``rebalance`` follows baselines.py:48-106 (hold when fewer than 5 past rows, rolling moments
    of the last ``lookback_window`` rows, W[0] of the mean-variance solve). ``max_weight`` (keyword,
    not in the reference) is the per-asset position limit of ``MPCConfig.max_weight``: every target
    keeps w <= max_weight (long-only, N * max_weight > 1; 0: none), so the baseline runs under the
    same limit as the MPC strategies. ``max_turnover`` (keyword, not in the reference either) is
    the L1 turnover cap of ``MPCConfig.mv_max_turnover``: every target keeps
    ||w - current_weights||_1 <= max_turnover (0: none, the reference's program), the cap the MPC
    strategies trade under (MPCConfig.max_turnover). A step whose current weights lie further than
    the cap from the feasible set (under a position limit only) holds them. ``cov_estimator`` and
    ``cov_ewma_lambda`` (keywords, not in the reference; ``set_cov_estimator``) choose the estimator of
    the rolling covariance: "sample" (the reference's np.cov, the default), "ledoit_wolf", "oas" or
    "ewma" (rolling_moments); the rolling mean does not depend on it.
    """

    def __init__(self, risk_aversion: float = 1.0, cost_coeff: float = 0.001, allow_short: bool = False):
        self.risk_aversion = risk_aversion
        self.cost_coeff = cost_coeff
        self.allow_short = allow_short
        self.max_weight = 0.0
        self.max_turnover = 0.0
        self.cov_estimator = "sample"
        self.cov_ewma_lambda = 0.94
        self.mpc_config = MPCConfig(horizon=1, gamma=risk_aversion, cost_coeff=cost_coeff,
                                    allow_short=allow_short, solver="ECOS")
        self._dev = None
        self._cache = (None, None)

    def set_max_weight(self, max_weight: float) -> None:
        """Set the per-asset position limit on the strategy and in its ``mpc_config``."""
        self.max_weight = max_weight
        self.mpc_config.max_weight = max_weight

    def set_max_turnover(self, max_turnover: float) -> None:
        """Set the L1 turnover cap on the strategy and in its ``mpc_config`` (mv_max_turnover)."""
        self.max_turnover = max_turnover
        self.mpc_config.mv_max_turnover = max_turnover

    def set_cov_estimator(self, cov_estimator: str = "sample", cov_ewma_lambda: float = 0.94) -> None:
        """Set the covariance estimator of the rolling moments ("sample", "ledoit_wolf", "oas" or
        "ewma" with its decay); ValueError on an unknown name or a lambda outside (0, 1]."""
        _cov_estimator(cov_estimator, cov_ewma_lambda)
        self.cov_estimator = cov_estimator
        self.cov_ewma_lambda = float(cov_ewma_lambda)

    def _device(self) -> torch.device:
        if self._dev is None:
            if not torch.cuda.is_available():
                raise _lib.KmpcError("MarkowitzStrategy runs on the gfx950 kernels and needs a GPU")
            self._dev = torch.device("cuda", torch.cuda.current_device())
        return self._dev

    def _returns(self, env):
        """(rows [T, >= N] float32 on the device, mean, std, N): the env's test rows with its stats,
        or — for envs with custom extract / destandardize callables — the de-standardized
        current returns computed by those callables (baselines.py:71-73)."""
        data = env.test_dataset.data
        if not _cache_hit(self._cache[0], data):
            dev = self._device()
            st = _env_stats(env)
            n = getattr(env, "n_assets", None)
            if st is not None and n is not None:
                entry = (torch.as_tensor(data).to(dev, torch.float32).contiguous(), st[0], st[1], int(n))
            else:
                r = env.destandardize_returns(env.extract_current_returns(torch.as_tensor(data)))
                r = torch.as_tensor(r).to(dev, torch.float32).contiguous()
                entry = (r, None, None, int(r.shape[-1]))
            self._cache = (_cache_key(data), entry)
        return self._cache[1]

    def rebalance_batch(self, ts: Sequence[int], current_weights, env, lookback_window: int = 60,
                        return_info: bool = False):
        """Independent windows t in ts with their own current weights [B, N] -> W[0] [B, N] float64."""
        self._device()   # no GPU -> KmpcError (there is no CPU path)
        z, mean, std, N = self._returns(env)
        dev = z.device
        wp = torch.as_tensor(np.asarray(current_weights, np.float64), device=dev).reshape(len(ts), N)
        mu, sigma, valid = rolling_moments(z, ts, lookback_window, N, mean, std, estimator=self.cov_estimator,
                                           ewma_lambda=self.cov_ewma_lambda)
        W0, status, value = solve_mpc_mean_variance_batched(wp, mu.unsqueeze(1), sigma, self.mpc_config)
        hold = valid == 0   # fewer than 5 past rows: keep the current weights (baselines.py:76-78)
        W0 = torch.where(hold.unsqueeze(1), wp, W0)
        W0 = W0.cpu().numpy()
        if return_info:
            return W0, status.cpu().numpy(), value.cpu().numpy(), valid.cpu().numpy()
        return W0

    def rebalance(self, t, current_weights, env, lookback_window: int = 60) -> np.ndarray:
        W0 = self.rebalance_batch([t], np.asarray(current_weights, np.float64).reshape(1, -1), env,
                                  lookback_window)
        return W0[0]


# ---- the Markowitz backtest on the device ------------------------------------------------------

# Steps per chunk of run_markowitz_lockstep / run_markowitz_sweep: each chunk is one
# kmpc_rolling_moments_paths and one kmpc_markowitz_run (or _sweep), and holds the chunk's Sigma,
# chunk * P * N^2 * 8 bytes. At most MARKOWITZ_CHUNK steps, and fewer where that buffer would pass
# MARKOWITZ_SIGMA_BYTES (256 MiB: P = 64 paths of N = 100 assets run 52 steps per chunk).
MARKOWITZ_CHUNK = 1024
MARKOWITZ_SIGMA_BYTES = 256 << 20


def _markowitz_chunk(P: int, N: int) -> int:
    return max(1, min(int(MARKOWITZ_CHUNK), int(MARKOWITZ_SIGMA_BYTES) // max(1, P * N * N * 8)))


def _markowitz_paths(strategy, obs, realized, config: BacktestConfig, mean, std, n_rows: Optional[int]):
    """The P paths of a Markowitz device backtest: the shape checks (ValueError before any device
    work), then z [P, T, ld] and the realized rows [T, P, N] on the device, the steps' test indices,
    the float32 de-standardisation and the solve's descriptor fields."""
    from types import SimpleNamespace
    x, r = torch.as_tensor(obs), torch.as_tensor(realized)
    if x.dim() != 3 or r.dim() != 3 or x.shape[:2] != r.shape[:2] or x.shape[2] < r.shape[2]:
        raise ValueError("obs must be [P, T, >= N] and realized [P, T, N]")
    P, T, N = (int(v) for v in r.shape)
    H = int(strategy.mpc_config.horizon)
    u = _box_limit(strategy.mpc_config, N)
    tau = _mv_turnover_cap(strategy.mpc_config)
    cov = _strategy_cov(strategy)
    n_rows = T if n_rows is None else int(n_rows)
    steps = list(range(0, n_rows - config.horizon, config.rebalance_freq))
    dev = strategy._device()
    z = x.to(dev, torch.float32).contiguous()
    rt = r.to(dev, torch.float32).transpose(0, 1).contiguous()
    m = torch.as_tensor(np.asarray(mean, np.float64).astype(np.float32), device=dev)
    sd = torch.as_tensor(np.asarray(std, np.float64).astype(np.float32), device=dev)
    if m.numel() != N or sd.numel() != N:
        raise ValueError(f"mean and std must have {N} entries")
    return SimpleNamespace(z=z, rt=rt, P=P, T=T, N=N, H=H, u=u, tau=tau, steps=steps, S=len(steps), dev=dev, m=m, sd=sd,
                           cov=cov, ts=torch.as_tensor(steps, dtype=torch.int32, device=dev))


def _markowitz_chunks(pp, lookback: int):
    """Per chunk of steps: (k0, n, mu [n, P, H, N], sigma [n, P, N, N], valid [n, P], the realized rows
    [n_real, P, N] of the steps' t + 1 or None, n_real). One kmpc_rolling_moments_paths per chunk
    (kmpc_rolling_cov_paths under the strategy's estimator: _rolling_cov_paths); a
    horizon above 1 repeats the rolling mean in every period (the reference's strategy has H = 1)."""
    P, T, N, H, dev = pp.P, pp.T, pp.N, pp.H, pp.dev
    sc = _markowitz_chunk(P, N)
    for k0 in range(0, pp.S, sc):
        n = min(sc, pp.S - k0)
        mu = torch.empty((n, P, N), dtype=torch.float64, device=dev)
        sigma = torch.empty((n, P, N, N), dtype=torch.float64, device=dev)
        valid = torch.empty((n, P), dtype=torch.int32, device=dev)
        ts = pp.ts[k0:k0 + n]
        _rolling_cov_paths(pp.cov, P, n, T, N, lookback, pp.z, pp.m, pp.sd, ts, mu, sigma, valid, _lib.stream_handle(dev))
        mu = mu[:, :, None, :].expand(n, P, H, N).contiguous()
        tn = [t + 1 for t in pp.steps[k0:k0 + n] if t + 1 < T]   # (steps increase: a prefix has a t + 1)
        rr = pp.rt[torch.as_tensor(tn, dtype=torch.long, device=dev)].contiguous() if tn else None
        yield k0, n, mu, sigma, valid, rr, len(tn)


def _markowitz_out(hist, w, metrics, S: int, lead: tuple) -> Dict[str, Any]:
    hist = hist[..., :S, :]
    out = {k: hist[..., i] for i, k in enumerate(("portfolio_value", "return", "turnover", "cost"))}
    out["weights"] = w
    metrics = metrics.reshape(*lead, 5)
    out["metrics"] = {name: metrics[..., i] for i, name in enumerate(METRIC_NAMES)} if S else {}
    return out


def run_markowitz_lockstep(strategy: "MarkowitzStrategy", obs, realized, config: BacktestConfig, mean, std,
                           n_rows: Optional[int] = None, lookback_window: int = 60,
                           persistent: Optional[bool] = None) -> Dict[str, Any]:
    """P independent Markowitz backtests of the reference loop (backtest.py:133-219 with
    MarkowitzStrategy.rebalance, baselines.py:48-106) on the device: path p reproduces
    run_backtest(strategy, env, config) on an env whose test rows are obs[p] and whose de-standardized
    realized log-returns are realized[p]. Arguments and the returned dict as run_backtest_lockstep.

    Args:
        strategy: a MarkowitzStrategy (risk_aversion, cost_coeff, allow_short, max_weight,
            max_turnover; the horizon of its mpc_config, 1 in the reference).
        obs: [P, T, >= N] float32 standardized test rows; the first N columns are the current returns.
        realized: [P, T, N] float32 de-standardized log-returns (the reference's all_returns).
        mean, std: [N] de-standardisation of the moments (env.stats).
        n_rows: len(env.test_dataset) (default T); steps range(0, n_rows - config.horizon,
            config.rebalance_freq), step t realizing row t + 1.
        persistent: every step of a path in one launch per chunk of steps (kmpc_markowitz_run: the
            step's solve or hold, then its bookkeeping, back to back in one workgroup per path).
            False: the per-step loop — kmpc_solve_mv_ws / kmpc_solve_mv_box (kmpc_solve_mv_cap under
            a turnover cap, where the persistent kernel is kmpc_markowitz_run_cap) over the P windows, the
            hold select, kmpc_backtest_step. Default: the persistent kernel wherever the C ABI has it
            (H * N <= 1,024). The two are bit-identical.
    The steps go in chunks of _markowitz_chunk(P, N), one kmpc_rolling_moments_paths each.
    Returns: dict of device tensors — portfolio_value / return / turnover / cost [P, S], weights
        [P, N] (after the last step), metrics {name: [P]}.
    """
    pp = _markowitz_paths(strategy, obs, realized, config, mean, std, n_rows)
    P, N, H, S, dev = pp.P, pp.N, pp.H, pp.S, pp.dev
    f64 = dict(dtype=torch.float64, device=dev)
    w = torch.full((P, N), 1.0 / N, **f64)       # backtest.py:161
    value = torch.full((P,), float(config.initial_capital), **f64)
    hist = torch.empty((P, max(S, 1), 4), **f64)
    metrics = torch.empty((P, 5), **f64)
    L = _lib.load()
    bd = _lib.BacktestDesc(P, N, max(S, 1), float(config.cost_coeff))
    md = _mv_desc(P, N, H, strategy.mpc_config, False)
    with torch.cuda.device(dev):
        sh = _lib.stream_handle(dev)
        # under a turnover cap the _cap entry with its cap ahead of the steps, and its workspace query
        run, head, query = L.kmpc_markowitz_run, (ctypes.byref(bd), ctypes.byref(md), pp.u), L.kmpc_mv_workspace_bytes
        if pp.tau:
            run, head, query = L.kmpc_markowitz_run_cap, head + (pp.tau,), L.kmpc_mv_cap_workspace_bytes
        if persistent is None or persistent:
            rc = run(*head, 0, 0, None, None, None, None, 0,
                     None, None, None, None, None, None, None, 0, sh)   # (shape check only)
            if rc == _lib.KMPC_ERR_UNSUPPORTED and persistent is None:
                persistent = False
            elif rc == _lib.KMPC_ERR_UNSUPPORTED:
                raise ValueError("persistent=True: no persistent Markowitz kernel for this shape")
            else:
                _lib.check(rc)
                persistent = True
        if persistent and P and S:
            target = torch.empty((P, N), **f64)
            status = torch.zeros((P,), dtype=torch.int32, device=dev)
            objv = torch.empty((P,), **f64)
            nws = int(query(ctypes.byref(md)))
            ws = _workspace(dev, nws) if nws else None
            for k0, n, mu, sigma, valid, rr, n_real in _markowitz_chunks(pp, lookback_window):
                _lib.check(run(
                    *head, k0, n, mu.data_ptr(), sigma.data_ptr(), valid.data_ptr(),
                    rr.data_ptr() if rr is not None else None, n_real, w.data_ptr(), value.data_ptr(), hist.data_ptr(),
                    target.data_ptr(), status.data_ptr(), objv.data_ptr(), ws.data_ptr() if ws is not None else None,
                    nws, sh))
        elif P and S:
            for k0, n, mu, sigma, valid, rr, n_real in _markowitz_chunks(pp, lookback_window):
                for k in range(n):
                    W0, _, _ = solve_mpc_mean_variance_batched(w, mu[k], sigma[k], strategy.mpc_config)
                    W0 = torch.where((valid[k] == 0).unsqueeze(1), w, W0)   # baselines.py:76-78: hold
                    _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), k0 + k, W0.data_ptr(),
                                                    rr[k].data_ptr() if k < n_real else None, w.data_ptr(),
                                                    value.data_ptr(), hist.data_ptr(), sh))
        if P and S:
            _lib.check(L.kmpc_backtest_metrics(ctypes.byref(bd), hist.data_ptr(), metrics.data_ptr(), sh))
    return _markowitz_out(hist, w, metrics, S, (P,))


def run_markowitz_sweep(strategy: "MarkowitzStrategy", obs, realized, config: BacktestConfig, mean, std,
                        risk_aversions: Sequence[float], cost_coeffs: Sequence[float],
                        bt_cost_coeffs: Optional[Sequence[float]] = None, n_rows: Optional[int] = None,
                        lookback_window: int = 60, max_turnovers: Optional[Sequence[float]] = None) -> Dict[str, Any]:
    """A hyper-parameter sweep of run_markowitz_lockstep: C configs (risk_aversion, the strategy's
    cost_coeff, BacktestConfig.cost_coeff) over the same P paths, every step of every (config, path)
    in kmpc_markowitz_sweep launches, one workgroup each. The moments depend on the path only: they
    are computed once per chunk for the P paths and shared by the configs.

    Args:
        strategy: its allow_short, max_weight and horizon are used, equal across the configs; its
            risk_aversion and cost_coeff are not.
        obs, realized, config, mean, std, n_rows, lookback_window: as run_markowitz_lockstep.
        risk_aversions, cost_coeffs: [C] each (ValueError on unequal lengths or none).
        bt_cost_coeffs: the bookkeeping's cost_coeff per config (default config.cost_coeff for all).
        max_turnovers: the turnover cap per config [C] (kmpc_markowitz_sweep_cap). Default: the
            strategy's cap for every config (none: the uncapped sweep). Given, every config is a
            capped one: a cap that is not finite or not > 0 holds, as below.
    A config with a negative or non-finite risk_aversion or cost_coeff holds its weights at every
    step (turnover and cost 0); the others are not affected. Config j's rows equal
    run_markowitz_lockstep with that config's parameters bit for bit.
    Returns: the run_markowitz_lockstep dict with a leading config axis — portfolio_value / return /
        turnover / cost [C, P, S], weights [C, P, N], metrics {name: [C, P]} — and "status" [C, P]
        int32, the last step's solve status of each work item (0 after a held step).
    """
    ga =[float(v) for v in risk_aversions]
    mc = [float(v) for v in cost_coeffs]
    C = len(ga)
    if C < 1:
        raise ValueError("risk_aversions is empty")
    if len(mc) != C:
        raise ValueError(f"cost_coeffs has {len(mc)} entries for {C} risk_aversions")
    btc = [float(config.cost_coeff)] * C if bt_cost_coeffs is None else [float(v) for v in bt_cost_coeffs]
    if len(btc) != C:
        raise ValueError(f"bt_cost_coeffs has {len(btc)} entries for {C} configs")
    caps = None if max_turnovers is None else [float(v) for v in max_turnovers]
    if caps is not None and len(caps) != C:
        raise ValueError(f"max_turnovers has {len(caps)} entries for {C} configs")
    pp = _markowitz_paths(strategy, obs, realized, config, mean, std, n_rows)
    P, N, H, S, dev = pp.P, pp.N, pp.H, pp.S, pp.dev
    f64 = dict(dtype=torch.float64, device=dev)
    w = torch.full((C, P, N), 1.0 / N, **f64)
    value = torch.full((C, P), float(config.initial_capital), **f64)
    hist = torch.empty((C, P, max(S, 1), 4), **f64)
    metrics = torch.empty((C * P, 5), **f64)
    L = _lib.load()
    bd = _lib.BacktestDesc(P, N, max(S, 1), 0.0)
    md = _mv_desc(C * P, N, H, strategy.mpc_config, False)
    if P and S:
        with torch.cuda.device(dev):
            sh = _lib.stream_handle(dev)
            pg, pc, pb = (torch.tensor(v, **f64) for v in (ga, mc, btc))
            if caps is None and pp.tau:
                caps = [pp.tau] * C
            sweep, head, query = L.kmpc_markowitz_sweep, (pg.data_ptr(), pc.data_ptr(), pb.data_ptr()), \
                L.kmpc_mv_workspace_bytes
            if caps is not None:
                pt = torch.tensor(caps, **f64)
                sweep, head, query = L.kmpc_markowitz_sweep_cap, head + (pt.data_ptr(),), L.kmpc_mv_cap_workspace_bytes
            target = torch.empty((C * P, N), **f64)
            status = torch.zeros((C * P,), dtype=torch.int32, device=dev)
            objv = torch.empty((C * P,), **f64)
            nws = int(query(ctypes.byref(md)))
            ws = _workspace(dev, nws) if nws else None
            for k0, n, mu, sigma, valid, rr, n_real in _markowitz_chunks(pp, lookback_window):
                _lib.check(sweep(
                    ctypes.byref(bd), ctypes.byref(md), pp.u, C, *head, k0, n,
                    mu.data_ptr(), sigma.data_ptr(), valid.data_ptr(), rr.data_ptr() if rr is not None else None,
                    n_real, w.data_ptr(), value.data_ptr(), hist.data_ptr(), target.data_ptr(), status.data_ptr(),
                    objv.data_ptr(), ws.data_ptr() if ws is not None else None, nws, sh))
            dm = _lib.BacktestDesc(C * P, N, max(S, 1), 0.0)
            _lib.check(L.kmpc_backtest_metrics(ctypes.byref(dm), hist.data_ptr(), metrics.data_ptr(), sh))
    out = _markowitz_out(hist, w, metrics, S, (C, P))
    out["status"] = status.reshape(C, P) if P and S else torch.zeros((C, P), dtype=torch.int32, device=dev)
    return out


def sweep_backtest_markowitz(env: Any, config: BacktestConfig, strategies: Sequence["MarkowitzStrategy"]) -> list:
    """run_backtest(strategies[j], env, config) for C Markowitz strategies on one environment in one
    sweep (run_markowitz_sweep with P = 1): the env-level counterpart of sweep_backtest. The
    strategies may differ in risk_aversion, cost_coeff and max_turnover only, must be all capped
    or all uncapped and must share their covariance estimator (ValueError otherwise, before any device work). Returns C DataFrames with the reference's columns (date, portfolio_value, return,
    turnover, cost), the rebalance_freq quirk kept. An env without stats (custom de-standardisation)
    runs run_backtest per strategy."""
    strats = list(strategies)
    if not strats:
        raise ValueError("strategies is empty")
    s0 = strats[0]
    for j, s in enumerate(strats):
        for name in ("allow_short", "max_weight"):
            if getattr(s, name) != getattr(s0, name):
                raise ValueError(f"strategies[{j}] differs from strategies[0] in {name}: a sweep varies "
                                 "risk_aversion, cost_coeff and max_turnover only")
        if bool(_mv_turnover_cap(s.mpc_config)) != bool(_mv_turnover_cap(s0.mpc_config)):
            raise ValueError(f"strategies[{j}] and strategies[0]: one has a turnover cap and one has none; a sweep "
                             "runs capped strategies or uncapped ones")
        if int(s.mpc_config.horizon) != int(s0.mpc_config.horizon):
            raise ValueError(f"strategies[{j}] differs from strategies[0] in horizon: a sweep varies "
                             "risk_aversion, cost_coeff and max_turnover only")
        cj, c0 = _strategy_cov(s), _strategy_cov(s0)
        if cj[0] != c0[0] or (s0.cov_estimator == "ewma" and cj[1] != c0[1]):
            raise ValueError(f"strategies[{j}] differs from strategies[0] in cov_estimator: the covariances are "
                             "computed once and shared; a sweep varies risk_aversion, cost_coeff and max_turnover only")
    st = _env_stats(env)
    n = getattr(env, "n_assets", None)
    if st is None or n is None:
        return [run_backtest(s, env, config, verbose=False) for s in strats]
    data = env.test_dataset.data
    rets = env.destandardize_returns(env.extract_current_returns(data))
    n_rows = len(env.test_dataset)
    out = run_markowitz_sweep(s0, torch.as_tensor(data)[None], torch.as_tensor(rets)[None], config, st[0], st[1],
                              [s.risk_aversion for s in strats], [s.cost_coeff for s in strats], n_rows=n_rows,
                              max_turnovers=[s.max_turnover for s in strats] if s0.max_turnover else None)
    steps = range(0, n_rows - config.horizon, config.rebalance_freq)
    dates = [env.test_dataset.dates[t] for t in steps]
    cols = {k: out[k][:, 0].cpu().numpy() for k in ("portfolio_value", "return", "turnover", "cost")}
    return [pd.DataFrame({"date": dates, **{k: v[j] for k, v in cols.items()}}) for j in range(len(strats))]


# ---- mean-variance Koopman-MPC: the forecast sequence in the mean-variance program ---------------

class KoopmanMVStrategy(KoopmanMPCStrategy):
    """The risk-aware form of KoopmanMPCStrategy: the multi-period mean-variance program
    (mpc.py:119-184) with mu_t = yhat_t, the forecast sequence of the same rollout as
    KoopmanMPCStrategy, and Sigma the rolling covariance MarkowitzStrategy uses (the last
    ``lookback_window`` de-standardized rows, np.cov + 1e-6 I; fewer than 5 past rows: hold), solved
    by the band kernels (kmpc_solve_mv_band). ``rebalance`` returns W[0].

    Args:
        model: whatever KoopmanMPCStrategy accepts; ``dmd_model_spec(fit_dmd(train))`` gives the DMD
            variant.
        mpc_config: MPCConfig — horizon, gamma, cost_coeff, allow_short, max_weight and
            mv_max_turnover are read (max_turnover is the log-utility solve's and is not).
        device: as KoopmanMPCStrategy.
        cov_estimator, cov_ewma_lambda: the estimator of the rolling covariance, as MarkowitzStrategy's
            ("sample", "ledoit_wolf", "oas", "ewma"; ValueError on an unknown name or a lambda outside
            (0, 1]). The lock-step run and the sweep read it from the strategy: one estimator for all configs.
    A run_backtest(strategy, env, config) drives it as any Strategy; run_koopman_mv_lockstep runs P
    such backtests on the device.
    """

    def __init__(self, model: Any, mpc_config: MPCConfig, device: str = "cpu", cov_estimator: str = "sample",
                 cov_ewma_lambda: float = 0.94):
        _cov_estimator(cov_estimator, cov_ewma_lambda)
        super().__init__(model, mpc_config, device)
        self.cov_estimator = cov_estimator
        self.cov_ewma_lambda = float(cov_ewma_lambda)
        self._ret_cache = (None, None)

    def _returns(self, env):
        """(rows [T, >= N] float32 on the device, mean, std): what the rolling covariance reads, as
        MarkowitzStrategy._returns."""
        data = env.test_dataset.data
        if not _cache_hit(self._ret_cache[0], data):
            st = _env_stats(env)
            if st is not None:
                entry = (self._test_data(env), st[0], st[1])
            else:
                r = env.destandardize_returns(env.extract_current_returns(torch.as_tensor(data)))
                entry = (torch.as_tensor(r).to(self._device(), torch.float32).contiguous(), None, None)
            self._ret_cache = (_cache_key(data), entry)
        return self._ret_cache[1]

    def rebalance_batch(self, ts: Sequence[int], current_weights, env, lookback_window: int = 60,
                        return_info: bool = False):
        """Independent windows t in ts with their own current weights [B, N] -> W[0] [B, N] float64."""
        N, H = int(env.n_assets), int(self.mpc_config.horizon)
        _mv_band_program(self.mpc_config, N, H)   # (config errors before any device work)
        km = self.device_model()
        data = self._test_data(env)
        obs = data.index_select(0, torch.as_tensor(np.asarray(ts, np.int64), device=km.device))
        wp = torch.as_tensor(np.asarray(current_weights, np.float64), device=km.device).reshape(len(ts), N)
        st = _env_stats(env)
        if st is not None:
            yhat = km.rollout(obs, st[0], st[1], H, N)
        else:   # (custom de-standardisation: as KoopmanMPCStrategy.rebalance_batch)
            y_std = km.rollout(obs, np.zeros(N), np.ones(N), H, N)
            yhat = torch.as_tensor(env.destandardize_returns(y_std), device=km.device, dtype=torch.float32)
        z, mean, std = self._returns(env)
        _, sigma, valid = rolling_moments(z, ts, lookback_window, N, mean, std, estimator=self.cov_estimator,
                                          ewma_lambda=self.cov_ewma_lambda)
        W0, status, value = solve_mpc_mean_variance_banded_batched(wp, yhat, sigma, self.mpc_config)
        W0 = torch.where((valid == 0).unsqueeze(1), wp, W0)   # fewer than 5 past rows: hold
        W0 = W0.cpu().numpy()
        if return_info:
            return W0, status.cpu().numpy(), value.cpu().numpy(), valid.cpu().numpy()
        return W0

    def rebalance(self, t, current_weights, env, lookback_window: int = 60) -> np.ndarray:
        W0 = self.rebalance_batch([t], np.asarray(current_weights, np.float64).reshape(1, -1), env, lookback_window)
        return W0[0]


def run_koopman_mv_lockstep(strategy: "KoopmanMVStrategy", obs, realized, config: BacktestConfig, mean, std,
                            lookback_window: int = 60, n_rows: Optional[int] = None,
                            persistent: Optional[bool] = None) -> Dict[str, Any]:
    """P independent backtests of KoopmanMVStrategy on the device: path p reproduces
    run_backtest(strategy, env, config) on an env whose test rows are obs[p] and whose de-standardized
    realized log-returns are realized[p]. Arguments as run_backtest_lockstep (obs [P, T, obs_size],
    its first N columns the current returns; realized [P, T, N]; mean, std [N]) with the covariance's
    lookback_window; the returned dict as run_markowitz_lockstep.

    The steps go in chunks: one rollout of the chunk's windows (as the log-utility lock-step
    pre-rolls them), one kmpc_rolling_moments_paths for its covariances (within MARKOWITZ_SIGMA_BYTES),
    then one kmpc_koopman_mv_run — every step of a path, solve or hold then bookkeeping, in one
    workgroup — and kmpc_backtest_metrics at the end. persistent=False runs the per-step loop of
    kmpc_solve_mv_band, the hold select and kmpc_backtest_step instead; the two are bit-identical.
    Config and shape errors raise ValueError before any device work."""
    x, r = torch.as_tensor(obs), torch.as_tensor(realized)
    if x.dim() != 3 or r.dim() != 3 or x.shape[:2] != r.shape[:2] or x.shape[2] < r.shape[2]:
        raise ValueError("obs must be [P, T, >= N] and realized [P, T, N]")
    P, T, N = (int(v) for v in r.shape)
    cfg = strategy.mpc_config
    H = int(cfg.horizon)
    u, tau = _mv_band_program(cfg, N, H)
    cov = _strategy_cov(strategy)
    if len(np.atleast_1d(np.asarray(mean))) < N or len(np.atleast_1d(np.asarray(std))) < N:
        raise ValueError(f"mean and std must have {N} entries")
    km = strategy.device_model()
    pp = _prepare_paths(km, x, r, config, mean, std, n_rows)
    S, dev = pp.S, km.device
    z = pp.x.contiguous()
    ts32 = pp.steps_t.to(torch.int32)
    f64 = dict(dtype=torch.float64, device=dev)
    w = torch.full((P, N), 1.0 / N, **f64)       # backtest.py:161
    value = torch.full((P,), float(config.initial_capital), **f64)
    hist = torch.empty((P, max(S, 1), 4), **f64)
    metrics = torch.empty((P, 5), **f64)
    L = _lib.load()
    bd = _lib.BacktestDesc(P, N, max(S, 1), float(config.cost_coeff))
    md = _mv_desc(P, N, H, cfg, False)
    with torch.cuda.device(dev):
        sh = _lib.stream_handle(dev)
        if persistent is None or persistent:
            _lib.check(L.kmpc_koopman_mv_run(ctypes.byref(bd), ctypes.byref(md), u, tau, 0, 0, None, None, None, None, 0,
                                             None, None, None, None, None, None, None, 0, sh))   # (shape check only)
            persistent = True
        if P and S:
            target = torch.empty((P, N), **f64)
            status = torch.zeros((P,), dtype=torch.int32, device=dev)
            objv = torch.empty((P,), **f64)
            nws = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(md), int(bool(tau)))) if persistent else 0
            ws = _workspace(dev, nws) if nws else None
            sc = max(1, min(_markowitz_chunk(P, N), PREROLL_CHUNK // P))
            for k0 in range(0, S, sc):
                n = min(sc, S - k0)
                y = km.rollout(pp.xt[pp.steps_t[k0:k0 + n]].reshape(n * P, -1), pp.m, pp.sd, H, N).contiguous()
                mu = torch.empty((n, P, N), **f64)   # (the rolling mean: not read, mu is the forecast)
                sigma = torch.empty((n, P, N, N), **f64)
                valid = torch.empty((n, P), dtype=torch.int32, device=dev)
                _rolling_cov_paths(cov, P, n, T, N, lookback_window, z, pp.m, pp.sd, ts32[k0:k0 + n], mu, sigma, valid, sh)
                tn = pp.steps_t[k0:k0 + n] + 1
                n_real = int((tn < T).sum().item())   # (steps increase: the rows with a t + 1 are a prefix)
                rr = pp.rt[tn[:n_real]].contiguous() if n_real else None
                if persistent:
                    _lib.check(L.kmpc_koopman_mv_run(
                        ctypes.byref(bd), ctypes.byref(md), u, tau, k0, n, y.data_ptr(), sigma.data_ptr(),
                        valid.data_ptr(), rr.data_ptr() if rr is not None else None, n_real, w.data_ptr(),
                        value.data_ptr(), hist.data_ptr(), target.data_ptr(), status.data_ptr(), objv.data_ptr(),
                        ws.data_ptr() if ws is not None else None, nws, sh))
                    continue
                y = y.reshape(n, P, H, N)
                for k in range(n):
                    W0, _, _ = solve_mpc_mean_variance_banded_batched(w, y[k], sigma[k], cfg)
                    W0 = torch.where((valid[k] == 0).unsqueeze(1), w, W0)   # hold
                    _lib.check(L.kmpc_backtest_step(ctypes.byref(bd), k0 + k, W0.data_ptr(),
                                                    rr[k].data_ptr() if k < n_real else None, w.data_ptr(),
                                                    value.data_ptr(), hist.data_ptr(), sh))
            _lib.check(L.kmpc_backtest_metrics(ctypes.byref(bd), hist.data_ptr(), metrics.data_ptr(), sh))
    return _markowitz_out(hist, w, metrics, S, (P,))


# ---- the sweep of the mean-variance Koopman-MPC backtest -----------------------------------------

_MV_SWEEP_FREE = ("gamma", "cost_coeff", "mv_max_turnover", "max_weight")   # the kernel's per-config parameters


def _mv_sweep_configs(mpc_configs, N: int) -> tuple:
    """The configs of a mean-variance sweep and their programs [(u, tau)] (_mv_band_program, for N
    assets): the configs may differ in gamma, cost_coeff, mv_max_turnover and max_weight only, and each
    must be a program of the band solve with cost_coeff >= 0. Raises ValueError, no device work."""
    cfgs = list(mpc_configs)
    if not cfgs:
        raise ValueError("mpc_configs is empty")
    f0 = _sweep_fields(cfgs[0], _MV_SWEEP_FREE)
    for j, c in enumerate(cfgs):
        fj = _sweep_fields(c, _MV_SWEEP_FREE)
        if fj != f0:
            diff = sorted(k for k in set(f0) | set(fj) if f0.get(k) != fj.get(k))
            raise ValueError(f"mpc_configs[{j}] differs from mpc_configs[0] in {diff}: a sweep varies "
                             "gamma, cost_coeff, mv_max_turnover and max_weight only")
    H = int(cfgs[0].horizon)
    programs = []
    for j, c in enumerate(cfgs):
        try:
            programs.append(_mv_band_program(c, N, H))
            cc = float(c.cost_coeff)
            if not np.isfinite(cc) or cc < 0.0:
                raise ValueError(f"cost_coeff must be finite and >= 0 (got {c.cost_coeff})")
        except ValueError as e:
            raise ValueError(f"mpc_configs[{j}]: {e}") from None
    return cfgs, programs


def _mv_sweep_groups(programs: Sequence[tuple]) -> list:
    """The launches of a mean-variance sweep: the limit and the cap are compile-time forms of the kernel,
    so the configs go in up to four groups by (has an active limit, has a cap) of their programs
    [(u, tau)] (u = 0: none — _box_limit gives 0 for an inactive max_weight >= 1). Returns
    [(has_limit, has_cap, [config indices, increasing])] for the non-empty groups, every config in one."""
    groups = {}
    for j, (u, tau) in enumerate(programs):
        groups.setdefault((bool(u), bool(tau)), []).append(j)
    return [(box, cap, groups[(box, cap)]) for box in (False, True) for cap in (False, True) if (box, cap) in groups]


def _mv_sweep_scatter(parts: Sequence[torch.Tensor], groups: list, C: int) -> torch.Tensor:
    """The groups' rows [C_g, ...] back in the configs' order: [C, ...]."""
    full = parts[0].new_empty((C,) + tuple(parts[0].shape[1:]))
    for part, (_, _, idx) in zip(parts, groups):
        full[torch.as_tensor(idx, device=part.device)] = part
    return full


def run_koopman_mv_sweep(strategy: "KoopmanMVStrategy", obs, realized, config: BacktestConfig, mean, std,
                         mpc_configs: Sequence[MPCConfig], bt_cost_coeffs: Optional[Sequence[float]] = None,
                         lookback_window: int = 60, n_rows: Optional[int] = None) -> Dict[str, Any]:
    """A hyper-parameter sweep of run_koopman_mv_lockstep: C configs (MPCConfig.gamma, cost_coeff,
    mv_max_turnover and max_weight; BacktestConfig.cost_coeff) over the same P paths, every step of
    every (config, path) in kmpc_koopman_mv_sweep launches, one workgroup each — an efficient frontier
    (a gamma grid) at P = 1 fills C compute units where C lock-step runs keep one busy, one after the
    other. The forecasts and the rolling covariances depend on the path only: per chunk of steps they are
    rolled out and computed once for the P paths (chunked as run_koopman_mv_lockstep, within
    MARKOWITZ_SIGMA_BYTES and PREROLL_CHUNK) and shared by the configs.

    Args:
        strategy: its model is used; the solve's program comes from mpc_configs.
        obs, realized, config, mean, std, lookback_window, n_rows: as run_koopman_mv_lockstep
            (config.cost_coeff is the default of bt_cost_coeffs).
        mpc_configs: C MPCConfigs that differ in gamma, cost_coeff, mv_max_turnover and max_weight only;
            each a program of the band solve (_mv_band_program) with cost_coeff >= 0. ValueError
            otherwise, before any device work.
        bt_cost_coeffs: the bookkeeping's cost_coeff per config (default config.cost_coeff for all).
    The position limit and the turnover cap are compile-time forms of the kernel: the configs run in up
    to four launches per chunk, grouped by (has an active limit, has a cap) (_mv_sweep_groups), each over
    the same forecasts and covariances, with the limit and the cap per config inside a group. Config j's
    rows equal run_koopman_mv_lockstep with that config (and its bt_cost_coeff) bit for bit.
    Returns: the run_koopman_mv_lockstep dict with a leading config axis — portfolio_value / return /
        turnover / cost [C, P, S], weights [C, P, N], metrics {name: [C, P]} — and "status" [C, P]
        int32, the last step's solve status of each work item (0 after a held step).
    """
    x, r = torch.as_tensor(obs), torch.as_tensor(realized)
    if x.dim() != 3 or r.dim() != 3 or x.shape[:2] != r.shape[:2] or x.shape[2] < r.shape[2]:
        raise ValueError("obs must be [P, T, >= N] and realized [P, T, N]")
    P, T, N = (int(v) for v in r.shape)
    cfgs, programs = _mv_sweep_configs(mpc_configs, N)
    cov = _strategy_cov(strategy)   # (the strategy's estimator, shared by the configs)
    C, H = len(cfgs), int(cfgs[0].horizon)
    btc = [float(config.cost_coeff)] * C if bt_cost_coeffs is None else [float(v) for v in bt_cost_coeffs]
    if len(btc) != C:
        raise ValueError(f"bt_cost_coeffs has {len(btc)} entries for {C} configs")
    if len(np.atleast_1d(np.asarray(mean))) < N or len(np.atleast_1d(np.asarray(std))) < N:
        raise ValueError(f"mean and std must have {N} entries")
    groups = _mv_sweep_groups(programs)
    km = strategy.device_model()
    pp = _prepare_paths(km, x, r, config, mean, std, n_rows)
    S, dev = pp.S, km.device
    z = pp.x.contiguous()
    ts32 = pp.steps_t.to(torch.int32)
    f64 = dict(dtype=torch.float64, device=dev)
    L = _lib.load()
    bd = _lib.BacktestDesc(P, N, max(S, 1), 0.0)
    state = []   # per group: the descriptor, the configs' device arrays and the work items' rows
    with torch.cuda.device(dev):
        sh = _lib.stream_handle(dev)
        for box, cap, idx in groups:
            Cg = len(idx)
            g = SimpleNamespace(md=_mv_desc(Cg * P, N, H, cfgs[0], False), C=Cg)
            g.par = [torch.tensor([float(getattr(cfgs[j], name)) for j in idx], **f64) for name in ("gamma", "cost_coeff")]
            g.par.append(torch.tensor([btc[j] for j in idx], **f64))
            g.par.append(torch.tensor([programs[j][0] for j in idx], **f64) if box else None)
            g.par.append(torch.tensor([programs[j][1] for j in idx], **f64) if cap else None)
            g.head = (ctypes.byref(bd), ctypes.byref(g.md), Cg) + tuple(t.data_ptr() if t is not None else None for t in g.par)
            _lib.check(L.kmpc_koopman_mv_sweep(*g.head, 0, 0, None, None, None, None, 0, None, None, None, None, None,
                                               None, None, 0, sh))   # (shape check only)
            g.w = torch.full((Cg, P, N), 1.0 / N, **f64)       # backtest.py:161
            g.value = torch.full((Cg, P), float(config.initial_capital), **f64)
            g.hist = torch.empty((Cg, P, max(S, 1), 4), **f64)
            g.target = torch.empty((Cg * P, N), **f64)
            g.status = torch.zeros((Cg, P), dtype=torch.int32, device=dev)
            g.obj = torch.empty((Cg * P,), **f64)
            g.nws = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(g.md), int(cap)))
            state.append(g)
        metrics = torch.empty((C * P, 5), **f64)
        if P and S:
            nws = max(g.nws for g in state)
            ws = _workspace(dev, nws) if nws else None   # (one buffer: the groups' launches follow each other on the stream)
            sc = max(1, min(_markowitz_chunk(P, N), PREROLL_CHUNK // P))
            for k0 in range(0, S, sc):
                n = min(sc, S - k0)
                y = km.rollout(pp.xt[pp.steps_t[k0:k0 + n]].reshape(n * P, -1), pp.m, pp.sd, H, N).contiguous()
                mu = torch.empty((n, P, N), **f64)   # (the rolling mean: not read, mu is the forecast)
                sigma = torch.empty((n, P, N, N), **f64)
                valid = torch.empty((n, P), dtype=torch.int32, device=dev)
                _rolling_cov_paths(cov, P, n, T, N, lookback_window, z, pp.m, pp.sd, ts32[k0:k0 + n], mu, sigma, valid, sh)
                tn = pp.steps_t[k0:k0 + n] + 1
                n_real = int((tn < T).sum().item())   # (steps increase: the rows with a t + 1 are a prefix)
                rr = pp.rt[tn[:n_real]].contiguous() if n_real else None
                for g in state:
                    _lib.check(L.kmpc_koopman_mv_sweep(
                        *g.head, k0, n, y.data_ptr(), sigma.data_ptr(), valid.data_ptr(),
                        rr.data_ptr() if rr is not None else None, n_real, g.w.data_ptr(), g.value.data_ptr(),
                        g.hist.data_ptr(), g.target.data_ptr(), g.status.data_ptr(), g.obj.data_ptr(),
                        ws.data_ptr() if ws is not None and g.nws else None, g.nws, sh))
        hist = _mv_sweep_scatter([g.hist for g in state], groups, C)
        w = _mv_sweep_scatter([g.w for g in state], groups, C)
        status = _mv_sweep_scatter([g.status for g in state], groups, C)
        if P and S:
            dm = _lib.BacktestDesc(C * P, N, max(S, 1), 0.0)
            _lib.check(L.kmpc_backtest_metrics(ctypes.byref(dm), hist.data_ptr(), metrics.data_ptr(), sh))
    out = _markowitz_out(hist, w, metrics, S, (C, P))
    out["status"] = status
    return out


def sweep_backtest_koopman_mv(strategy: "KoopmanMVStrategy", env: Any, config: BacktestConfig,
                              mpc_configs: Sequence[MPCConfig], lookback_window: int = 60) -> list:
    """run_backtest(KoopmanMVStrategy(model, mpc_configs[j]), env, config) for C configs on one
    environment in one sweep (run_koopman_mv_sweep with P = 1): the env-level counterpart of
    sweep_backtest_markowitz for the risk-aware row — a gamma grid gives the efficient frontier. The
    configs may differ in gamma, cost_coeff, mv_max_turnover and max_weight only (ValueError otherwise,
    and on a config that is no program of the band solve, before any device work). Returns C DataFrames
    with the reference's columns (date, portfolio_value, return, turnover, cost), the rebalance_freq
    quirk kept. An env without stats (custom de-standardisation) runs run_backtest per config."""
    cfgs, _ = _mv_sweep_configs(mpc_configs, int(env.n_assets))
    st = _env_stats(env)
    if st is None:
        km = strategy.device_model()
        cov = dict(cov_estimator=getattr(strategy, "cov_estimator", "sample"),
                   cov_ewma_lambda=getattr(strategy, "cov_ewma_lambda", 0.94))
        return [run_backtest(KoopmanMVStrategy(km, c, **cov), env, config, verbose=False) for c in cfgs]
    data = env.test_dataset.data
    rets = env.destandardize_returns(env.extract_current_returns(data))
    n_rows = len(env.test_dataset)
    out = run_koopman_mv_sweep(strategy, torch.as_tensor(data)[None], torch.as_tensor(rets)[None], config, st[0], st[1],
                               cfgs, lookback_window=lookback_window, n_rows=n_rows)
    steps = range(0, n_rows - config.horizon, config.rebalance_freq)
    dates = [env.test_dataset.dates[t] for t in steps]
    cols = {k: out[k][:, 0].cpu().numpy() for k in ("portfolio_value", "return", "turnover", "cost")}
    return [pd.DataFrame({"date": dates, **{k: v[j] for k, v in cols.items()}}) for j in range(len(cfgs))]


__all__: Sequence[str] = ("DMDStrategy", "MarkowitzStrategy", "fit_dmd", "dmd_model_spec",
                          "rolling_moments", "Strategy", "run_markowitz_lockstep", "run_markowitz_sweep",
                          "sweep_backtest_markowitz", "KoopmanMVStrategy", "run_koopman_mv_lockstep",
                          "run_koopman_mv_sweep", "sweep_backtest_koopman_mv")
