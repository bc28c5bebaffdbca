"""MPC solve — the reference's ``mpc.py`` API on the gfx950 solver kernel.

Mirrors ``MPCConfig`` (mpc.py:17-25) field for field and ``solve_mpc_log_utility``
(mpc.py:27-117) signature, return shapes/dtypes and failure semantics: solver failure is never
raised; a status outside {"optimal", "optimal_inaccurate"} returns ``tile(current_weights)`` and
``{"status": s, "value": None}`` (mpc.py:113-115).

``solve_mpc_log_utility_batched`` is the batched entry point (torch device tensors in and out)
that the strategies and the benchmark use. ``solve_mpc_mean_variance`` (mpc.py:119-184) and its
batched form run the mean-variance QP kernel (kmpc_solve_mv) with the same conventions.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib


@dataclass
class MPCConfig:
    """Configuration for MPC solver (mpc.py:17-25)."""
    horizon: int = 5
    gamma: float = 0.0  # Risk aversion (0.0 = log utility maximization); unused by log utility
    cost_coeff: float = 0.001  # Transaction cost coefficient (e.g. 10bps)
    max_turnover: float = 0.2  # Maximum turnover per step
    allow_short: bool = False
    solver: str = "ECOS"  # accepted for compatibility; the gfx950 interior-point kernel solves
    # extra (defaulted) knobs of the device solver
    max_iter: int = 80
    tol: float = 1e-9
    n_refine: int = 0  # 0 -> kernel default
    solver_path: int = 0  # kmpc_solve_desc.path: 0 by shape, 1 register IPM (no presolve), 2 large-window IPM, 3 register IPM without lane-group packing
    precision: str = "auto"  # kmpc_solve_desc.precision: "mixed" (float32 warm-start phase + float64 finish where available), "f64", or "auto" (mixed from 2,048 windows per call, else f64)
    mu_handoff: float = 0.0  # float32 -> float64 handoff at mu <= mu_handoff (0 -> kernel default 3e-5)
    max_weight: float = 0.0  # per-asset position limit w <= max_weight of the log-utility (kmpc_solve_box) and the mean-variance (kmpc_solve_mv_box) solves; 0 or >= 1: none
    mv_max_turnover: float = 0.0  # L1 turnover cap ||w_t - w_{t-1}||_1 <= mv_max_turnover of the mean-variance solve (kmpc_solve_mv_cap); 0: none, the reference's program (max_turnover above is the log-utility solve's and stays unread there)


def _box_limit(config: MPCConfig, N: int) -> float:
    """The active per-asset position limit of `config` for N assets, or 0.0 when it has none
    (max_weight 0, or >= 1: the simplex already bounds every weight by 1). kmpc_solve_desc cannot
    carry the limit, so every caller that turns an MPCConfig into a solve goes through here and
    then through kmpc_solve_box (kmpc_mv_desc cannot either: kmpc_solve_mv_box). Raises ValueError where no program exists: a negative or NaN
    limit, N * max_weight <= 1 (empty set, or the single point 1/N), or together with allow_short."""
    u = float(getattr(config, "max_weight", 0.0))
    if u != u or u < 0.0:
        raise ValueError(f"max_weight must be >= 0 (got {u})")
    if u == 0.0 or u >= 1.0:
        return 0.0
    if bool(config.allow_short):
        raise ValueError("max_weight is a long-only position limit: not available with allow_short")
    if int(N) * u <= 1.0:
        raise ValueError(f"max_weight = {u} leaves no room with N = {int(N)} assets (N * max_weight must exceed 1)")
    return u


def _mv_turnover_cap(config: MPCConfig) -> float:
    """The active L1 turnover cap of the mean-variance solve of `config`, or 0.0 when it has none
    (mv_max_turnover 0: the reference's program; MPCConfig.max_turnover is the log-utility solve's
    and is not read here). kmpc_mv_desc cannot carry the cap, so every caller that turns an
    MPCConfig into a mean-variance solve goes through here and then through kmpc_solve_mv_cap.
    Raises ValueError on a negative or NaN cap."""
    tau = float(getattr(config, "mv_max_turnover", 0.0))
    if tau != tau or tau < 0.0:
        raise ValueError(f"mv_max_turnover must be >= 0 (got {tau})")
    return tau


def _solve_desc(B: int, N: int, H: int, config: MPCConfig, full: bool) -> _lib.SolveDesc:
    d = _lib.SolveDesc()
    d.B, d.N, d.H = int(B), int(N), int(H)
    d.cost_coeff = float(config.cost_coeff)
    d.max_turnover = float(config.max_turnover)
    d.allow_short = int(bool(config.allow_short))
    d.max_iter = int(getattr(config, "max_iter", 80))
    d.tol = float(getattr(config, "tol", 1e-9))
    d.return_full_W = int(bool(full))
    d.n_refine = int(getattr(config, "n_refine", 0))
    d.path = int(getattr(config, "solver_path", 0))
    prec = getattr(config, "precision", "auto")
    if prec not in ("auto", "f64", "mixed"):
        raise ValueError(f"precision must be 'auto', 'f64' or 'mixed' (got {prec!r})")
    d.precision = {"auto": _lib.PRECISION_AUTO, "f64": _lib.PRECISION_F64, "mixed": _lib.PRECISION_MIXED}[prec]
    d.mu_handoff = float(getattr(config, "mu_handoff", 0.0))
    if d.cost_coeff < 0:
        # -c ||dw||_1 with c < 0 is not concave: the reference's cvxpy problem fails DCP and raises
        raise ValueError(f"cost_coeff must be >= 0 (got {config.cost_coeff}): the problem is not convex")
    return d


def _box_route(d: _lib.SolveDesc) -> str:
    """Which entry solves `d` under an active position limit: "large" (kmpc_solve_box_ws, the
    large-window box kernel: MPCConfig.solver_path = 2, at every shape) or "register"
    (kmpc_solve_box: N <= 256, H <= 10). The default path does not route by shape: a limit on a
    larger window raises KmpcError, as kmpc_solve_box answers it with KMPC_ERR_UNSUPPORTED."""
    if d.path == _lib.PATH_LARGE:
        return "large"
    if d.N > 256 or d.H > 10:
        raise _lib.KmpcError(f"libkmpc call failed: unsupported shape ({_lib.KMPC_ERR_UNSUPPORTED}): the register box "
                             f"kernels stop at N <= 256, H <= 10 (got N = {d.N}, H = {d.H}); set "
                             f"MPCConfig.solver_path = 2 for the large-window box kernel")
    return "register"


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """A device buffer of at least nbytes for one call, from torch's caching allocator on the
    current stream: the block returns to the pool when the caller drops it and is handed out again
    only in stream order, so concurrent streams never share scratch and nothing is held between calls."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def solve_mpc_log_utility_batched(
    current_weights: torch.Tensor,
    predicted_log_returns: torch.Tensor,
    config: MPCConfig,
    return_full: bool = False,
    with_iters: bool = False,
):
    """Batched solve on the device.

    Args:
        current_weights: [B, N] (float64; other dtypes are converted) device tensor.
        predicted_log_returns: [B, H, N] float32 device tensor (the reference feeds float32 yhat).
        config: MPCConfig.
        return_full: return W [B, H, N] instead of W[:, 0] [B, N].

    Returns:
        (W, status, value[, iters]): W float64, status int32 [B] (see _lib.STATUS_NAMES),
        value float64 [B] (NaN where the fallback was applied).
    """
    y = predicted_log_returns
    _lib.require_gpu(y)
    if y.dim() != 3:
        raise ValueError("predicted_log_returns must be [B, H, N]")
    B, H, N = y.shape
    y = y.to(torch.float32).contiguous()
    wp = current_weights.to(device=y.device, dtype=torch.float64).contiguous()
    if wp.shape != (B, N):
        raise ValueError(f"current_weights must be [{B}, {N}], got {tuple(wp.shape)}")
    if H > _lib.KMPC_MAX_H or N > _lib.KMPC_MAX_N:
        raise _lib.KmpcError(f"shape H={H}, N={N} exceeds the kernel limits "
                             f"(H <= {_lib.KMPC_MAX_H}, N <= {_lib.KMPC_MAX_N})")
    W = torch.empty((B, H, N) if return_full else (B, N), dtype=torch.float64, device=y.device)
    status = torch.empty(B, dtype=torch.int32, device=y.device)
    value = torch.empty(B, dtype=torch.float64, device=y.device)
    iters = torch.empty(B, dtype=torch.int32, device=y.device)
    d = _solve_desc(B, N, H, config, return_full)
    L = _lib.load()
    u = _box_limit(config, N)
    # The entry, its arguments ahead of the arrays and its workspace query: kmpc_solve; under a limit
    # kmpc_solve_box (the box case of the float64 register kernels: no workspace argument) or
    # kmpc_solve_box_ws (the large-window box kernel, its slabs in a workspace)
    arrays = (y.data_ptr(), wp.data_ptr(), W.data_ptr(), status.data_ptr(), value.data_ptr(), iters.data_ptr())
    if not u:
        entry, head, query = L.kmpc_solve, (ctypes.byref(d),), lambda: L.kmpc_workspace_bytes(None, ctypes.byref(d))
    elif _box_route(d) == "large":
        entry, head = L.kmpc_solve_box_ws, (ctypes.byref(d), u)
        query = lambda: L.kmpc_solve_box_workspace_bytes(ctypes.byref(d), u)
    else:
        entry, head, query = L.kmpc_solve_box, (ctypes.byref(d), u), None
    with torch.cuda.device(y.device):
        tail = ()
        if query is not None:
            nws = int(query())
            ws = _workspace(y.device, nws) if nws or u else None   # (kmpc_solve_box_ws: never a null workspace)
            tail = (ws.data_ptr() if ws is not None else None, nws)
        rc = entry(*head, *arrays, *tail, _lib.stream_handle(y.device))
    _lib.check(rc)
    if with_iters:
        return W, status, value, iters
    return W, status, value


def gross_returns(predicted_log_returns: torch.Tensor) -> torch.Tensor:
    """R = np.exp(yhat) on the float32 yhat (mpc.py:55), bit for bit as numpy evaluates it
    (kmpc_gross_returns), as a float32 device tensor of the same shape."""
    y = predicted_log_returns
    _lib.require_gpu(y)
    y = y.to(torch.float32).contiguous()
    R = torch.empty_like(y)
    L = _lib.load()
    with torch.cuda.device(y.device):
        rc = L.kmpc_gross_returns(y.numel(), y.data_ptr(), R.data_ptr(), _lib.stream_handle(y.device))
    _lib.check(rc)
    return R


def log_utility_value_batched(W: torch.Tensor, current_weights: torch.Tensor,
                              predicted_log_returns: torch.Tensor, cost_coeff: float) -> torch.Tensor:
    """problem.value of the reference program (mpc.py:66-103) at given weights: for each window,
    sum_t log(R_t . w_t) - c sum_t ||w_t - w_{t-1}||_1 (w_{-1} = current_weights), R = np.exp(yhat)
    in float32, sums in float64. W [B, H, N], current_weights [B, N], yhat [B, H, N] -> [B] float64.
    Evaluates any W (e.g. a decision taken on another forecast) in the program of `yhat`."""
    R = gross_returns(predicted_log_returns).double()
    W = W.to(torch.float64)
    wp = current_weights.to(device=W.device, dtype=torch.float64)
    D = torch.diff(torch.cat([wp[:, None, :], W], 1), dim=1)
    return torch.log((R * W).sum(-1)).sum(-1) - cost_coeff * D.abs().sum((-1, -2))


def _default_device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.KmpcError("solve_mpc_log_utility runs on the gfx950 kernel and needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


def solve_mpc_log_utility(
    current_weights: np.ndarray,
    predicted_log_returns: np.ndarray,
    config: MPCConfig,
) -> Tuple[np.ndarray, Dict]:
    """Drop-in for mpc.py:27-117: returns (W [H, N] float64, {"status", "value"})."""
    y = np.asarray(predicted_log_returns)
    H, N = y.shape
    dev = _default_device()
    yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32), device=dev).reshape(1, H, N)
    wt = torch.as_tensor(np.asarray(current_weights, dtype=np.float64), device=dev).reshape(1, N)
    W, status, value = solve_mpc_log_utility_batched(wt, yt, config, return_full=True)
    st = _lib.STATUS_NAMES.get(int(status.item()), "solver_error")
    W_np = W[0].cpu().numpy()
    if st not in ("optimal", "optimal_inaccurate"):
        return np.tile(np.asarray(current_weights, dtype=np.float64), (H, 1)), {"status": st, "value": None}
    return W_np, {"status": st, "value": float(value.item())}


# ---- mean-variance MPC (mpc.py:119-184) ------------------------------------------------------

def _mv_desc(B: int, N: int, H: int, config: MPCConfig, full: bool) -> _lib.MvDesc:
    d = _lib.MvDesc()
    d.B, d.N, d.H = int(B), int(N), int(H)
    d.gamma = float(config.gamma)
    d.cost_coeff = float(config.cost_coeff)
    d.allow_short = int(bool(config.allow_short))
    d.max_iter = int(getattr(config, "mv_max_iter", 100))
    d.tol = float(getattr(config, "mv_tol", 1e-10))
    d.return_full_W = int(bool(full))
    return d


def solve_mpc_mean_variance_batched(
    current_weights: torch.Tensor,
    mu: torch.Tensor,
    cov_matrix: torch.Tensor,
    config: MPCConfig,
    return_full: bool = False,
    with_iters: bool = False,
):
    """Batched mean-variance solve on the device (kmpc_solve_mv_ws; kmpc_solve_mv_box with a
    position limit; kmpc_solve_mv_cap with a turnover cap).

    Args:
        current_weights: [B, N] device tensor (float64; other dtypes are converted).
        mu: [B, H, N] expected returns (the reference passes predicted log-returns / the rolling
            mean as mu, mpc.py:150-155); computed in float64.
        cov_matrix: [B, N, N] per-window covariance, or one shared [N, N] (mpc.py:123).
        config: MPCConfig (gamma, cost_coeff, allow_short, and max_weight: the per-asset position
            limit w <= max_weight, long-only, N * max_weight > 1 — ValueError otherwise; 0 or >= 1:
            none; max_turnover is not part of this program in the reference either;
            mv_max_turnover: the L1 turnover cap of every period, 0: none — a window whose w_prev
            lies further than the cap from the feasible set reports "infeasible" and the fallback).
        return_full: return W [B, H, N] instead of W[:, 0].

    Returns:
        (W, status, value[, iters]) as solve_mpc_log_utility_batched; value is problem.value
        (mpc.py:172, maximize form), NaN where the fallback was applied.
    """
    _lib.require_gpu(mu)
    if mu.dim() != 3:
        raise ValueError("mu must be [B, H, N]")
    B, H, N = mu.shape
    dev = mu.device
    mu64 = mu.to(torch.float64).contiguous()
    wp = current_weights.to(device=dev, dtype=torch.float64).contiguous()
    if wp.shape != (B, N):
        raise ValueError(f"current_weights must be [{B}, {N}], got {tuple(wp.shape)}")
    S = torch.as_tensor(cov_matrix).to(device=dev, dtype=torch.float64).contiguous()
    if S.dim() == 2:
        if S.shape != (N, N):
            raise ValueError(f"cov_matrix must be [{N}, {N}] or [{B}, {N}, {N}]")
        stride = 0
    elif S.shape == (B, N, N):
        stride = N * N
    else:
        raise ValueError(f"cov_matrix must be [{N}, {N}] or [{B}, {N}, {N}], got {tuple(S.shape)}")
    if H > _lib.KMPC_MV_MAX_H or H * N > _lib.KMPC_MV_MAX_HN:
        raise _lib.KmpcError(f"mean-variance shape H={H}, N={N} exceeds the kernel limits "
                             f"(H <= {_lib.KMPC_MV_MAX_H}, H*N <= {_lib.KMPC_MV_MAX_HN})")
    W = torch.empty((B, H, N) if return_full else (B, N), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    value = torch.empty(B, dtype=torch.float64, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    d = _mv_desc(B, N, H, config, return_full)
    L = _lib.load()
    u = _box_limit(config, N)
    tau = _mv_turnover_cap(config)
    with torch.cuda.device(dev):
        nws = int((L.kmpc_mv_cap_workspace_bytes if tau else L.kmpc_mv_workspace_bytes)(ctypes.byref(d)))
        ws = _workspace(dev, nws) if nws else None
        # (the position limit: the BOX form of the same kernels, same workspace; the turnover cap:
        # their CAP form, with or without the limit, and its larger workspace)
        if tau:
            entry, head = L.kmpc_solve_mv_cap, (ctypes.byref(d), u, tau)
        else:
            entry, head = (L.kmpc_solve_mv_box, (ctypes.byref(d), u)) if u else (L.kmpc_solve_mv_ws, (ctypes.byref(d),))
        rc = entry(*head, mu64.data_ptr(), S.data_ptr(), stride, wp.data_ptr(),
                   W.data_ptr(), status.data_ptr(), value.data_ptr(), iters.data_ptr(),
                   ws.data_ptr() if ws is not None else None, nws, _lib.stream_handle(dev))
    _lib.check(rc)
    if with_iters:
        return W, status, value, iters
    return W, status, value


def solve_mpc_mean_variance(
    current_weights: np.ndarray,
    predicted_log_returns: np.ndarray,
    cov_matrix: np.ndarray,
    config: MPCConfig,
) -> Tuple[np.ndarray, Dict]:
    """Drop-in for mpc.py:119-184: returns (W [H, N] float64, info). On a non-optimal status the
    reference returns tile(current_weights) and {"status": s} without a "value" key (mpc.py:180-181)."""
    y = np.asarray(predicted_log_returns)
    H, N = y.shape
    dev = _default_device()
    mu = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64), device=dev).reshape(1, H, N)
    wt = torch.as_tensor(np.asarray(current_weights, dtype=np.float64), device=dev).reshape(1, N)
    S = torch.as_tensor(np.asarray(cov_matrix, dtype=np.float64), device=dev)
    W, status, value = solve_mpc_mean_variance_batched(wt, mu, S, config, return_full=True)
    st = _lib.STATUS_NAMES.get(int(status.item()), "solver_error")
    if st not in ("optimal", "optimal_inaccurate"):
        return np.tile(np.asarray(current_weights, dtype=np.float64), (H, 1)), {"status": st}
    return W[0].cpu().numpy(), {"status": st, "value": float(value.item())}


# ---- mean-variance MPC, band form: the multi-period solve for a forecast sequence -------------

def _mv_band_program(config: MPCConfig, N: int, H: int) -> Tuple[float, float]:
    """(u, tau) of the band solve of `config` for [H, N] windows: the active position limit
    (_box_limit) and turnover cap (_mv_turnover_cap), 0.0 where there is none. Raises ValueError
    where no program exists or the kernels have no shape for it — gamma negative or not finite, the
    _box_limit and _mv_turnover_cap rules, H > KMPC_MV_MAX_H or H * N > KMPC_MV_MAX_HN — so that
    every caller fails before any device work."""
    g = float(config.gamma)
    if not np.isfinite(g) or g < 0.0:
        raise ValueError(f"gamma must be finite and >= 0 (got {config.gamma})")
    if int(H) < 1 or int(N) < 1:
        raise ValueError(f"the window must have H >= 1 periods and N >= 1 assets (got H = {H}, N = {N})")
    if int(H) > _lib.KMPC_MV_MAX_H or int(H) * int(N) > _lib.KMPC_MV_MAX_HN:
        raise ValueError(f"mean-variance shape H={H}, N={N} exceeds the kernel limits "
                         f"(H <= {_lib.KMPC_MV_MAX_H}, H*N <= {_lib.KMPC_MV_MAX_HN})")
    return _box_limit(config, N), _mv_turnover_cap(config)


def solve_mpc_mean_variance_banded_batched(
    current_weights: torch.Tensor,
    predicted_log_returns: torch.Tensor,
    cov_matrix: torch.Tensor,
    config: MPCConfig,
    return_full: bool = False,
    with_iters: bool = False,
):
    """Batched multi-period mean-variance solve on the band kernels (kmpc_solve_mv_band): the
    program of solve_mpc_mean_variance_batched with mu_t = yhat_t, the forecast sequence, and the
    Newton matrix kept and factored as the band matrix it is (half-bandwidth N).

    Args:
        current_weights: [B, N] device tensor (float64; other dtypes are converted).
        predicted_log_returns: [B, H, N] forecasts, read by the kernel as float32 — the rollout's
            yhat goes in as it is; any other dtype is rounded to float32 first.
        cov_matrix: [B, N, N] per-window covariance, or one shared [N, N].
        config: MPCConfig — gamma, cost_coeff, allow_short, max_weight and mv_max_turnover are read
            (max_turnover is not: it is the log-utility solve's, as everywhere in the mean-variance
            solve). ValueError before any device work on gamma < 0 or not finite, the max_weight /
            mv_max_turnover rules, or a shape past H <= 16, H * N <= 1,024.
        return_full: return W [B, H, N] instead of W[:, 0].

    Returns:
        (W, status, value[, iters]) as solve_mpc_mean_variance_batched.
    """
    y = predicted_log_returns
    if y.dim() != 3:
        raise ValueError("predicted_log_returns must be [B, H, N]")
    B, H, N = (int(v) for v in y.shape)
    u, tau = _mv_band_program(config, N, H)
    if tuple(current_weights.shape) != (B, N):
        raise ValueError(f"current_weights must be [{B}, {N}], got {tuple(current_weights.shape)}")
    S = torch.as_tensor(cov_matrix)
    if S.dim() == 2 and tuple(S.shape) == (N, N):
        per_window = 0
    elif tuple(S.shape) == (B, N, N):
        per_window = 1
    else:
        raise ValueError(f"cov_matrix must be [{N}, {N}] or [{B}, {N}, {N}], got {tuple(S.shape)}")
    _lib.require_gpu(y)
    dev = y.device
    y = y.to(torch.float32).contiguous()
    wp = current_weights.to(device=dev, dtype=torch.float64).contiguous()
    S = S.to(device=dev, dtype=torch.float64).contiguous()
    W = torch.empty((B, H, N) if return_full else (B, N), dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    value = torch.empty(B, dtype=torch.float64, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    d = _mv_desc(B, N, H, config, return_full)
    L = _lib.load()
    with torch.cuda.device(dev):
        nws = int(L.kmpc_mv_band_workspace_bytes(ctypes.byref(d), int(bool(tau))))
        ws = _workspace(dev, nws) if nws else None
        rc = L.kmpc_solve_mv_band(ctypes.byref(d), y.data_ptr(), S.data_ptr(), per_window, wp.data_ptr(), u, tau,
                                  W.data_ptr(), status.data_ptr(), value.data_ptr(), iters.data_ptr(),
                                  ws.data_ptr() if ws is not None else None, nws, _lib.stream_handle(dev))
    _lib.check(rc)
    if with_iters:
        return W, status, value, iters
    return W, status, value


def solve_mpc_mean_variance_banded(
    current_weights: np.ndarray,
    predicted_log_returns: np.ndarray,
    cov_matrix: np.ndarray,
    config: MPCConfig,
) -> Tuple[np.ndarray, Dict]:
    """solve_mpc_mean_variance (same signature and return convention) on the band kernels, for a
    forecast sequence predicted_log_returns [H, N]: returns (W [H, N] float64, info). The forecasts
    are read as float32 — a float64 input is rounded to float32 (the rollout's yhat is float32
    already) — so the optimum is that of solve_mpc_mean_variance on the rounded forecasts. Reads
    gamma, cost_coeff, allow_short, max_weight and mv_max_turnover of `config`; max_turnover is
    ignored, as the mean-variance solve ignores it everywhere. The band form pays from H = 2 on
    (profiles/mv_band.md: 4 to 8 times the dense kernel's rate at H = 5 and 10); at H = 1 it is the
    slower of the two (2.5 times at N = 100) and solve_mpc_mean_variance is the call to use.

    Batched inputs — current_weights [B, N], predicted_log_returns [B, H, N], cov_matrix [B, N, N]
    or [N, N], arrays or tensors — go to solve_mpc_mean_variance_banded_batched and return its
    (W [B, H, N], status, value) device tensors."""
    y = predicted_log_returns
    if (torch.is_tensor(y) and y.dim() == 3) or (not torch.is_tensor(y) and np.ndim(y) == 3):
        if not torch.is_tensor(y):
            _mv_band_program(config, int(np.shape(y)[2]), int(np.shape(y)[1]))   # (errors first)
            y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32), device=_default_device())
        wt = current_weights if torch.is_tensor(current_weights) else torch.as_tensor(np.asarray(current_weights, np.float64))
        St = cov_matrix if torch.is_tensor(cov_matrix) else torch.as_tensor(np.asarray(cov_matrix, np.float64))
        return solve_mpc_mean_variance_banded_batched(wt, y, St, config, return_full=True)
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError("predicted_log_returns must be [H, N] (or [B, H, N])")
    H, N = y.shape
    _mv_band_program(config, N, H)
    dev = _default_device()
    yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32), device=dev).reshape(1, H, N)
    wt = torch.as_tensor(np.asarray(current_weights, dtype=np.float64), device=dev).reshape(1, N)
    S = torch.as_tensor(np.asarray(cov_matrix, dtype=np.float64), device=dev)
    W, status, value = solve_mpc_mean_variance_banded_batched(wt, yt, S, config, return_full=True)
    st = _lib.STATUS_NAMES.get(int(status.item()), "solver_error")
    if st not in ("optimal", "optimal_inaccurate"):
        return np.tile(np.asarray(current_weights, dtype=np.float64), (H, 1)), {"status": st}
    return W[0].cpu().numpy(), {"status": st, "value": float(value.item())}
