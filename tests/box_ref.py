"""Reference for the log-utility MPC program with a per-asset position limit — a test helper,
not a test.

The program (MPCConfig.max_weight = u, kmpc_solve_box), per window:

    maximize_W  sum_t log(R_t . w_t) - c sum_t ||w_t - w_{t-1}||_1      R = np.exp(yhat) in float32
    s.t.        1'w_t = 1,  0 <= w_t,i <= u,  ||w_t - w_{t-1}||_1 <= tau  (if tau > 0),  w_{-1} = w_prev

* :func:`dense_box_ipm` — the textbook dense Mehrotra interior point of ``oracle.dense_ipm`` with
  the rows ``u - w >= 0`` appended to its constraint matrix (``oracle.dense_ipm._build``), started
  from ``w = 1/N``. It writes the goldens (tests/golden/make_box_golden.py), on the CPU only.
* :func:`feasible` — LP feasibility of the lifted constraint set (scipy HiGHS dual simplex).
* :func:`gap` — a linearisation certificate: an upper bound of ``p(W) - p*`` for ANY feasible W,
  whatever produced it, from one LP.
* :func:`violated` — the feasibility bars (budget and turnover 1e-8, bounds 1e-9) in one place.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.dense_ipm import _build, gross_returns, reference_objective  # noqa: E402,F401


def dense_box_ipm(w_prev, y, c, tau, u, iters=100, tol=1e-12):
    """Dense-KKT Mehrotra IPM of the capped program. Returns (W [H, N], converged, iterations);
    not converged: W is the iterate with the smallest max(mu, residuals) the loop reached."""
    from scipy.linalg import lu_factor, lu_solve
    from scipy.sparse import csr_matrix, diags

    wp = np.asarray(w_prev, np.float64)
    m = gross_returns(y) - 1.0   # log(R.w) == log(1 + m.w) on sum(w) = 1
    H, N = np.asarray(y).shape
    G, h, A, b, cvec, nw = _build(wp, np.asarray(y, np.float64), c, tau, False)
    nx = G.shape[1]
    Gu = np.zeros((nw, nx))
    Gu[np.arange(nw), np.arange(nw)] = -1.0          # u - w >= 0  as  G x - h >= 0
    G = np.vstack([G, Gu])
    h = np.concatenate([h, np.full(nw, -float(u))])
    Gs = csr_matrix(G)
    mi = G.shape[0]
    x = np.zeros(nx)
    x[:nw] = 1.0 / N
    if nx > nw:
        d = np.diff(np.vstack([wp, x[:nw].reshape(H, N)]), axis=0)
        x[nw:] = np.abs(d).ravel() + 0.01
    z = np.maximum(G @ x - h, 1e-2)
    lam = np.ones(mi)
    nu = np.zeros(H)
    best, Wbest = np.inf, x[:nw].reshape(H, N).copy()
    for it in range(iters):
        g = cvec.copy()
        Hf = np.zeros((nx, nx))
        for t in range(H):
            wt = x[t * N:(t + 1) * N]
            den = 1.0 + m[t] @ wt
            g[t * N:(t + 1) * N] -= m[t] / den
            Hf[t * N:(t + 1) * N, t * N:(t + 1) * N] += np.outer(m[t], m[t]) / den ** 2
        rd = g - Gs.T @ lam + A.T @ nu
        rp = A @ x - b
        rg = Gs @ x - h - z
        mu = (z @ lam) / mi
        if mu < tol and np.abs(rd).max() < 10 * tol and np.abs(rp).max() < 10 * tol and np.abs(rg).max() < 10 * tol:
            return x[:nw].reshape(H, N), True, it
        # (the loop has no safeguards: past the dense solve's noise floor — the dual residual stalls
        # near 1e-11 while mu keeps falling — the KKT matrix turns singular. The best iterate so far is
        # returned then, not converged; the callers judge it by its objective.)
        merit = max(mu, np.abs(rd).max(), np.abs(rp).max(), np.abs(rg).max())
        if not np.isfinite(merit):
            break
        if merit < best:
            best, Wbest = merit, x[:nw].reshape(H, N).copy()
        Wd = lam / z
        M = Hf + (Gs.T @ diags(Wd) @ Gs).toarray()
        K = np.block([[M, A.T], [A, np.zeros((H, H))]])
        if not np.isfinite(K).all():
            break
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lu = lu_factor(K, check_finite=False)

        def solve(rc):
            rhs1 = -rd - Gs.T @ (Wd * rg + rc / z)
            sol = lu_solve(lu, np.concatenate([rhs1, -rp]), check_finite=False)
            dx, dnu = sol[:nx], sol[nx:]
            dz = Gs @ dx + rg
            dlam = -Wd * dz - rc / z
            return dx, dnu, dlam, dz

        def maxstep(v, dv):
            neg = dv < 0
            return min(1.0, float(np.min(-v[neg] / dv[neg]))) if neg.any() else 1.0

        dx, dnu, dlam, dz = solve(z * lam)
        if not np.isfinite(dx).all():
            break
        a = min(maxstep(z, dz), maxstep(lam, dlam))
        mua = (z + a * dz) @ (lam + a * dlam) / mi
        sig = (mua / mu) ** 3
        dx, dnu, dlam, dz = solve(z * lam + dz * dlam - sig * mu)
        a = 0.99 * min(maxstep(z, dz), maxstep(lam, dlam))
        if not (np.isfinite(dx).all() and np.isfinite(dlam).all()):
            break
        x += a * dx
        nu += a * dnu
        lam += a * dlam
        z += a * dz
    return Wbest, False, it


def _lifted(w_prev, H, N, tau, u):
    """The constraint set in (V, S), S >= |V_t - V_{t-1}|: (A_ub, b_ub, A_eq, b_eq, bounds)."""
    from scipy.sparse import eye, hstack, kron, vstack, csr_matrix

    wp = np.asarray(w_prev, np.float64)
    n = H * N
    D = eye(n, format="csr") - eye(n, k=-N, format="csr")     # V_t - V_{t-1} (t >= 1), V_0 (t = 0)
    wp0 = np.concatenate([wp, np.zeros(n - N)])
    In = eye(n, format="csr")
    blocks = [hstack([D, -In]), hstack([-D, -In])]
    rhs = [wp0, -wp0]
    if tau > 0:
        blocks.append(hstack([csr_matrix((H, n)), kron(eye(H), np.ones((1, N)))]))
        rhs.append(np.full(H, float(tau)))
    A_eq = hstack([kron(eye(H), np.ones((1, N))), csr_matrix((H, n))])
    bounds = [(0.0, float(u))] * n + [(0.0, None)] * n
    return vstack(blocks).tocsr(), np.concatenate(rhs), A_eq.tocsr(), np.ones(H), bounds


def feasible(w_prev, H, N, tau, u) -> bool:
    """Whether the capped program has a feasible point (LP, HiGHS dual simplex)."""
    from scipy.optimize import linprog

    A_ub, b_ub, A_eq, b_eq, bounds = _lifted(w_prev, H, N, tau, u)
    r = linprog(np.zeros(2 * H * N), A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds")
    return r.status == 0


def turnover(W, w_prev):
    """||w_t - w_{t-1}||_1 per period, [H]."""
    return np.abs(np.diff(np.vstack([np.asarray(w_prev, np.float64), np.asarray(W, np.float64)]), axis=0)).sum(1)


def violated(W, w_prev, tau, u) -> list:
    """The project's feasibility bars on one window's W [H, N]: budget and turnover 1e-8, bounds
    1e-9. Returns the bars W misses as text (empty: feasible), so ``assert not violated(...)``
    names them."""
    W = np.asarray(W, np.float64)
    bad = []
    if not np.isfinite(W).all():
        return ["non-finite W"]
    e = np.abs(W.sum(1) - 1).max()
    if not e <= 1e-8:
        bad.append(f"budget off by {e:.3e}")
    if not W.min() >= -1e-9:
        bad.append(f"min w {W.min():.3e}")
    if not W.max() <= u + 1e-9:
        bad.append(f"max w - u {W.max() - u:.3e}")
    if tau > 0:
        t = turnover(W, w_prev).max()
        if not t <= tau + 1e-8:
            bad.append(f"turnover - tau {t - tau:.3e}")
    return bad


def gap(W, w_prev, y, c, tau, u) -> float:
    """An upper bound of p(W) - p*, p = phi + c sum_t ||d_t||_1 the program in minimisation form
    with phi(W) = -sum_t log(R_t . w_t). phi is convex, so over the feasible set
        p* >= min_V [phi(W) + grad phi(W).(V - W) + c sum_t ||d_t(V)||_1],
    an LP in (V, S). Returns p(W) minus that bound (inf if the LP fails)."""
    from scipy.optimize import linprog

    W = np.asarray(W, np.float64)
    H, N = W.shape
    R = gross_returns(y)
    rw = np.einsum("hn,hn->h", R, W)
    phi = -float(np.log(rw).sum())
    grad = -(R / rw[:, None]).ravel()
    pW = phi + c * float(turnover(W, w_prev).sum())
    A_ub, b_ub, A_eq, b_eq, bounds = _lifted(w_prev, H, N, tau, u)
    cost = np.concatenate([grad, np.full(H * N, float(c))])
    r = linprog(cost, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds")
    if r.status != 0:
        return float("inf")
    bound = phi - float(grad @ W.ravel()) + float(r.fun)
    return pW - bound
