"""Reference for the mean-variance MPC program with a per-asset position limit — a test helper,
not a test.

The program (MPCConfig.max_weight = u, kmpc_solve_mv_box), per window:

    maximize_W  sum_t [ w_t . mu_t - gamma w_t' Sigma w_t ] - c sum_t ||w_t - w_{t-1}||_1
    s.t.        1'w_t = 1,  0 <= w_t,i <= u,  w_{-1} = w_prev          (no turnover cap)

* :func:`dense_mv_box_ipm` — the textbook dense-KKT Mehrotra interior point of
  ``oracle.mv_ref.mv_dense_ipm`` restated with the rows ``u - w >= 0`` appended, started from
  ``w = 1/N``, tight to 1e-13. It writes the goldens (tests/golden/make_mvbox_golden.py).
* :func:`reduced_mv_box_ipm` — the kernel's own reduced iteration (csrc/kmpc_mv.hip, BOX form) in
  numpy, float64, tol 1e-10: it shows on the CPU which bars the algorithm itself reaches on the
  inputs the device tests use.
* :func:`gap` — a linearisation certificate: an upper bound of ``f* - f(W)`` for ANY feasible W,
  whatever produced it, from one LP.
* :func:`violated` — the feasibility bars (budget 1e-9, bounds 1e-9) in one place.
* :func:`objective_bar`, :func:`certificate_bar` — the two bars the tests hold.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.mv_ref import mv_objective  # noqa: E402,F401


def scale(mu, sigma, gamma, cost) -> float:
    """The kernel's objective scale sc = max(|mu|, 2 gamma |Sigma|, c) (1 when that is 0)."""
    sc = max(float(np.abs(mu).max()), 2.0 * gamma * float(np.abs(sigma).max()), float(cost))
    return sc if sc > 0 and np.isfinite(sc) else 1.0


def objective_bar(f) -> float:
    """The project's mean-variance objective bar (tests/test_mv_gpu.py)."""
    return 1e-9 + 1e-7 * abs(f)


def certificate_bar(f, mu, sigma, gamma, cost, tol=1e-10) -> float:
    """What the kernel's stopping rule allows, in objective units: in units of sc, mu_c < tol is a
    duality gap of up to mcon tol (mcon = 4n constraints, 3n at c = 0), and residuals below 10 tol
    act on at most 6H of L1 distance (w, s and the two |d| slacks of H budget simplices)."""
    H, N = np.asarray(mu).shape
    n = H * N
    mcon = 4 * n if cost > 0 else 3 * n
    return objective_bar(f) + scale(mu, sigma, gamma, cost) * tol * (mcon + 60 * H)


def dense_mv_box_ipm(w_prev, mu, sigma, gamma, cost, u, iters=200, tol=1e-13):
    """Dense-KKT Mehrotra IPM on the epigraph form (variables w [HN], s [HN] when cost > 0) of the
    capped program. Returns (W [H, N], status) with status "optimal", "optimal_inaccurate" or
    "solver_error" (then W is the iterate of the smallest merit)."""
    from scipy.sparse import coo_matrix

    wp = np.asarray(w_prev, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = mu.shape
    n = H * N
    use_s = cost > 0
    nx = n + (n if use_s else 0)
    # inequality rows G x - h >= 0: w >= 0; s -+ (w_t - w_{t-1}) >= 0; u - w >= 0
    rows, cols, vals, h = [], [], [], []
    r = 0
    for k in range(n):
        rows.append(r); cols.append(k); vals.append(1.0); h.append(0.0); r += 1
    if use_s:
        for t in range(H):
            for i in range(N):
                for sgn in (-1.0, 1.0):
                    rows.append(r); cols.append(n + t * N + i); vals.append(1.0)
                    rows.append(r); cols.append(t * N + i); vals.append(sgn)
                    rhs = 0.0
                    if t > 0:
                        rows.append(r); cols.append((t - 1) * N + i); vals.append(-sgn)
                    else:
                        rhs = sgn * wp[i]
                    h.append(rhs); r += 1
    for k in range(n):
        rows.append(r); cols.append(k); vals.append(-1.0); h.append(-float(u)); r += 1
    m = r
    G = coo_matrix((vals, (rows, cols)), shape=(m, nx)).tocsr()
    h = np.array(h)
    A = np.zeros((H, nx))
    for t in range(H):
        A[t, t * N:(t + 1) * N] = 1.0
    b = np.ones(H)
    Q = np.zeros((nx, nx))
    for t in range(H):
        Q[t * N:(t + 1) * N, t * N:(t + 1) * N] = 2.0 * gamma * S
    q = np.zeros(nx)
    q[:n] = -mu.ravel()
    if use_s:
        q[n:] = cost
    sc = max(np.abs(q).max(), np.abs(Q).max(), 1e-300)
    Q, q = Q / sc, q / sc
    x = np.zeros(nx)
    x[:n] = 1.0 / N
    if use_s:
        d = np.diff(np.vstack([wp, x[:n].reshape(H, N)]), axis=0)
        x[n:] = np.abs(d).ravel() + 1.0 / N
    z = np.maximum(G @ x - h, 1e-2)
    lam = np.ones(m)
    nu = np.zeros(H)
    status = "solver_error"
    best, best_x = np.inf, x.copy()
    for _ in range(iters):
        rd = Q @ x + q - G.T @ lam + A.T @ nu
        rp = A @ x - b
        rg = G @ x - h - z
        mu_c = (z @ lam) / m
        merit = max(mu_c, np.abs(rd).max(), np.abs(rp).max(), np.abs(rg).max())
        if not np.isfinite(merit):
            break
        if merit < best:
            best, best_x = merit, x.copy()
        if mu_c < tol and np.abs(rd).max() < 10 * tol and np.abs(rp).max() < 10 * tol and np.abs(rg).max() < 10 * tol:
            status = "optimal"
            break
        Wd = lam / z
        M = Q + (G.T @ G.multiply(Wd[:, None])).toarray()
        K = np.block([[M, A.T], [A, np.zeros((H, H))]])

        def solve(rc):
            rhs1 = -rd - G.T @ (Wd * rg + rc / z)
            try:
                sol = np.linalg.solve(K, np.concatenate([rhs1, -rp]))
            except np.linalg.LinAlgError:
                return None
            dx, dnu = sol[:nx], sol[nx:]
            dz = G @ dx + rg
            dlam = -(lam * dz + rc) / z
            return dx, dnu, dlam, dz

        def maxstep(v, dv):
            neg = dv < 0
            return min(1.0, float(np.min(-v[neg] / dv[neg]))) if neg.any() else 1.0

        r = solve(z * lam)
        if r is None:
            break
        dx, dnu, dlam, dz = r
        a = min(maxstep(z, dz), maxstep(lam, dlam))
        mua = (z + a * dz) @ (lam + a * dlam) / m
        sig = (mua / mu_c) ** 3
        r = solve(z * lam + dz * dlam - sig * mu_c)
        if r is None:
            break
        dx, dnu, dlam, dz = r
        a = min(1.0, 0.99 * min(maxstep(z, dz), maxstep(lam, dlam)))
        x += a * dx
        nu += a * dnu
        lam += a * dlam
        z += a * dz
    if status != "optimal":
        x = best_x
        status = "optimal" if best <= 1e-9 else ("optimal_inaccurate" if best <= 1e-6 else "solver_error")
    return x[:n].reshape(H, N), status


def reduced_mv_box_ipm(w_prev, mu, sigma, gamma, cost, u, max_iter=100, tol=1e-10):
    """The kernel's reduced Mehrotra iteration with the barrier on x5 = u - w (multiplier l5), line
    for line in numpy. Returns (W [H, N], status, iterations, objective): status 0 / 1 / 4 as
    KMPC_STATUS_*, W and the objective those of the best iterate."""
    from scipy.linalg import cho_factor, cho_solve

    wp = np.asarray(w_prev, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = mu.shape
    n = H * N
    hs = cost > 0
    sc = scale(mu, S, gamma, cost)
    g2, cs, mus = 2.0 * gamma / sc, cost / sc, mu / sc

    def prev(v, first):
        return np.vstack([first[None, :], v[:-1]])

    def nxt(v):
        return np.vstack([v[1:], np.zeros((1, N))])

    def to_bound(v, dv, a):
        neg = dv < 0
        return min(a, float(np.min(-v[neg] / dv[neg]))) if neg.any() else a

    zero = np.zeros((H, N))
    w = np.tile(np.minimum(0.5 * np.maximum(wp, 0.0) + 0.5 / N, 0.5 * (u + 1.0 / N)), (H, 1))
    wm = prev(w, wp)
    s = np.abs(w - wm) + 1.0 / N if hs else zero.copy()
    z2 = np.maximum(s - (w - wm), 1e-2) if hs else np.ones((H, N))
    z3 = np.maximum(s + (w - wm), 1e-2) if hs else np.ones((H, N))
    l1 = np.ones((H, N))
    l2 = np.ones((H, N)) if hs else zero.copy()
    l3 = l2.copy()
    l5 = np.ones((H, N))
    nu = np.zeros(H)
    mcon = n + (2 * n if hs else 0) + n
    A = np.kron(np.eye(H), np.ones((1, N)))          # [H, n]
    best, best_obj, best_W = 1e300, np.nan, np.tile(wp, (H, 1))
    it = 0
    for it in range(max_iter):
        wm = prev(w, wp)
        Sw = w @ S
        d = w - wm
        rg2 = (s - d) - z2 if hs else zero
        rg3 = (s + d) - z3 if hs else zero
        eta = l2 - l3
        rp = w.sum(1) - 1.0
        prmax = np.abs(rp).max()
        x5 = u - w
        rw = -mus + g2 * Sw - l1 + eta - nxt(eta) + nu[:, None] + l5
        rs = cs - l2 - l3 if hs else zero
        mu_c = float((w * l1 + z2 * l2 + z3 * l3 + x5 * l5).sum()) / mcon
        rd = max(np.abs(rw).max(), np.abs(rs).max(), np.abs(rg2).max(), np.abs(rg3).max())
        merit = max(mu_c, rd, prmax)
        if not np.isfinite(merit):
            break
        if merit < best:
            best = merit
            best_obj = float((mu * w - gamma * w * Sw - cost * np.abs(d)).sum())
            best_W = w.copy()
        if mu_c < tol and rd < 10 * tol and prmax < 10 * tol:
            break
        W1 = l1 / w + l5 / x5
        al = l2 / z2 if hs else zero
        be = l3 / z3 if hs else zero
        P = 1.0 / (al + be) if hs else zero
        E = 4.0 * al * be * P
        En = nxt(E)
        M = g2 * np.kron(np.eye(H), S) + np.diag((W1 + E + En).ravel())
        for k in range(n - N):
            M[k + N, k] -= En.ravel()[k]
            M[k, k + N] -= En.ravel()[k]
        try:
            cf = cho_factor(M, lower=True)
        except np.linalg.LinAlgError:
            break
        Y = cho_solve(cf, A.T)                         # [n, H]
        Sm = A @ Y
        rc1, rc2, rc3, rc5 = w * l1, z2 * l2, z3 * l3, x5 * l5
        for pas in range(2):
            p2, p3 = rc2 / z2 + al * rg2, rc3 / z3 + be * rg3
            qs = -rs - p2 - p3 if hs else zero
            v = (be - al) * P * qs + p3 - p2 if hs else zero
            rhs = -rw - rc1 / w + rc5 / x5 - (v - nxt(v))
            x = cho_solve(cf, rhs.ravel())
            dnu = np.linalg.solve(Sm, A @ x + rp)
            dw = (x - Y @ dnu).reshape(H, N)
            dd = dw - prev(dw, np.zeros(N))
            ds = P * (qs - (be - al) * dd) if hs else zero
            dz2, dz3 = ds - dd + rg2, ds + dd + rg3
            dl1 = -(l1 * dw + rc1) / w
            dl2 = -(l2 * dz2 + rc2) / z2 if hs else zero
            dl3 = -(l3 * dz3 + rc3) / z3 if hs else zero
            dl5 = (-rc5 + l5 * dw) / x5
            am = to_bound(l1, dl1, to_bound(w, dw, 1e300))
            if hs:
                for a_, b_ in ((z2, dz2), (z3, dz3), (l2, dl2), (l3, dl3)):
                    am = to_bound(a_, b_, am)
            am = to_bound(l5, dl5, to_bound(x5, -dw, am))
            if pas == 1:
                step = min(1.0, 0.99 * am)
                break
            ap = min(1.0, am)
            mua = float(((w + ap * dw) * (l1 + ap * dl1) + (z2 + ap * dz2) * (l2 + ap * dl2) +
                         (z3 + ap * dz3) * (l3 + ap * dl3) + (x5 - ap * dw) * (l5 + ap * dl5)).sum()) / mcon
            smu = (mua / mu_c) ** 3 * mu_c
            rc1 = w * l1 + dw * dl1 - smu
            if hs:
                rc2, rc3 = z2 * l2 + dz2 * dl2 - smu, z3 * l3 + dz3 * dl3 - smu
            rc5 = x5 * l5 - dw * dl5 - smu
        w = w + step * dw
        s = s + step * ds
        if hs:
            z2 = z2 + step * dz2
            z3 = z3 + step * dz3
        l1 = l1 + step * dl1
        l2 = l2 + step * dl2
        l3 = l3 + step * dl3
        l5 = l5 + step * dl5
        nu = nu + step * dnu
    status = 0 if best <= 1e-7 else (1 if best <= 1e-4 else 4)
    return best_W, status, it, best_obj


def _lifted(w_prev, H, N, u):
    """The feasible set in (V, S), S >= |V_t - V_{t-1}|: (A_ub, b_ub, A_eq, b_eq, bounds)."""
    from scipy.sparse import csr_matrix, eye, hstack, kron, vstack

    wp = np.asarray(w_prev, np.float64)
    n = H * N
    D = eye(n, format="csr") - eye(n, k=-N, format="csr")     # V_t - V_{t-1} (t >= 1), V_0 (t = 0)
    wp0 = np.concatenate([wp, np.zeros(n - N)])
    In = eye(n, format="csr")
    A_ub = vstack([hstack([D, -In]), hstack([-D, -In])]).tocsr()
    b_ub = np.concatenate([wp0, -wp0])
    A_eq = hstack([kron(eye(H), np.ones((1, N))), csr_matrix((H, n))]).tocsr()
    bounds = [(0.0, float(u))] * n + [(0.0, None)] * n
    return A_ub, b_ub, A_eq, np.ones(H), bounds


def gap(W, w_prev, mu, sigma, gamma, cost, u) -> float:
    """An upper bound of f* - f(W), f = q - c sum_t ||d_t||_1 the program in its maximize form with
    q(W) = sum_t [w_t . mu_t - gamma w_t' Sigma w_t]. q is concave, so over the feasible set
        f* <= max_V [q(W) + grad q(W).(V - W) - c sum_t ||d_t(V)||_1],
    an LP in (V, S). Returns that bound minus f(W) (inf if the LP fails)."""
    from scipy.optimize import linprog

    W = np.asarray(W, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = W.shape
    SW = W @ S
    q = float((W * mu).sum()) - gamma * float((W * SW).sum())
    grad = (mu - 2.0 * gamma * SW).ravel()
    A_ub, b_ub, A_eq, b_eq, bounds = _lifted(w_prev, H, N, u)
    lp = np.concatenate([-grad, np.full(H * N, float(cost))])
    r = linprog(lp, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds")
    if r.status != 0:
        return float("inf")
    bound = q - float(grad @ W.ravel()) - float(r.fun)
    return bound - mv_objective(W, w_prev, mu, S, gamma, cost)


def violated(W, u) -> list:
    """The mean-variance feasibility bars on one window's W [H, N]: budget 1e-9, bounds 1e-9.
    Returns the bars W misses as text (empty: feasible), so ``assert not violated(...)`` names them."""
    W = np.asarray(W, np.float64)
    if not np.isfinite(W).all():
        return ["non-finite W"]
    bad = []
    e = np.abs(W.sum(1) - 1).max()
    if not e <= 1e-9:
        bad.append(f"budget off by {e:.3e}")
    if not W.min() >= -1e-9:
        bad.append(f"min w {W.min():.3e}")
    if not W.max() <= u + 1e-9:
        bad.append(f"max w - u {W.max() - u:.3e}")
    return bad


def inputs(seed, B, N, H, vertex=True):
    """Seeded windows of the shape the goldens use: mu ~ N(5e-4, 0.01), Sigma a 60-sample covariance
    plus 1e-6 I per window, w_prev a mix of Dirichlet draws, 1/N (window 1) and a vertex (window 2)."""
    rng = np.random.default_rng(seed)
    wp = rng.dirichlet(np.ones(N), B)
    if B > 1:
        wp[1] = 1.0 / N
    if B > 2 and vertex:
        wp[2] = 0.0
        wp[2, int(rng.integers(N))] = 1.0
    mu = rng.normal(5e-4, 0.01, (B, H, N))
    X = rng.normal(5e-4, 0.015, (B, 60, N))
    S = np.stack([np.cov(x, rowvar=False).reshape(N, N) + 1e-6 * np.eye(N) for x in X])
    return wp, mu, S


# ---- the inputs of tests/test_mv_box_gpu.py, here so that tests/test_mv_box_cpu.py can show on
# the CPU that the kernel's algorithm (reduced_mv_box_ipm) reaches the bars on these very inputs ----

# (N, H, gamma, c, u, B): shapes past the goldens, seeded not stored
SEEDED = [
    (129, 1, 1.0, 1e-3, 0.02, 4),     # n = 129: the first workspace shape, 192 threads
    (300, 2, 1.0, 1e-3, 0.01, 3),     # ten waves
    (512, 2, 1.0, 1e-3, 0.005, 2),    # n = 1024, the upper edge
    (64, 16, 1.0, 1e-3, 0.05, 2),     # n = 1024 at H = KMPC_MV_MAX_H
]


def seeded(case):
    """(w_prev [B, N], mu [B, H, N], sigma [B, N, N]) of one SEEDED case."""
    N, H, gamma, c, u, B = case
    return inputs(9000 + 10 * N + H, B, N, H)


def cannot_bind():
    """u = 0.95 with gamma = 10 and a return spread of 2e-4: the risk term spreads the portfolio far
    below the limit (mu is scaled down, not Sigma up, so that the scale sc stays near |f|).
    (N, H, gamma, c, u, w_prev, mu, sigma), 4 windows, no vertex start."""
    N, H = 12, 2
    wp, mu, S = inputs(4242, 4, N, H, vertex=False)
    return N, H, 10.0, 1e-3, 0.95, wp, mu * 0.02, S


def edge_cases():
    """One window each: (name, w_prev [N], mu [H, N], sigma [N, N], gamma, c, u)."""
    out = []
    for name, N, H, Nu in (("N u = 1.05", 20, 1, 1.05), ("N u = 1.01", 20, 1, 1.01), ("N u = 1.01, H = 5", 10, 5, 1.01)):
        wp, mu, S = inputs(5000 + N + H, 1, N, H)
        out.append((name, wp[0], mu[0], S[0], 1.0, 1e-3, Nu / N))
    wp, mu, S = inputs(5100, 1, 10, 2)
    z = wp[0].copy()
    z[[1, 4, 7]] = 0.0
    out.append(("zeros in w_prev", z / z.sum(), mu[0], S[0], 1.0, 1e-3, 0.3))
    on = np.array([0.25, 0.25, 0.25, 0.05, 0.05, 0.05, 0.04, 0.03, 0.02, 0.01])
    out.append(("w_prev on the limit", on, mu[0], S[0], 1.0, 1e-3, 0.25))
    e0 = np.zeros(10)
    e0[0] = 1.0
    out.append(("w_prev = e_0", e0, mu[0], S[0], 1.0, 1e-3, 0.25))
    out.append(("c = 10, w_prev inside", wp[0] * 0.5 + 0.05, mu[0], S[0], 1.0, 10.0, 0.6))
    out.append(("c = 10, w_prev = e_0", e0, mu[0], S[0], 1.0, 10.0, 0.25))
    return out


WATER = (np.full(4, 0.25), np.array([[0.03, 0.02, 0.01, -0.01]]), 1e-2 * np.eye(4), 1.0, 0.0, 0.6)
WATER_W = np.array([[0.6, 0.4, 0.0, 0.0]])          # (the unlimited optimum is [0.75, 0.25, 0, 0])
FLAT = (np.array([0.5, 0.3, 0.1, 0.1]), np.zeros((1, 4)), 1e-4 * np.eye(4), 0.0, 1e-3, 0.4)
FLAT_VALUE = -2e-4   # -2 c E with E = 0.1, the excess of w_prev over the limit (the optimum is not unique)


def greedy_case():
    """gamma = 0, c = 0: a linear program over the capped simplex per period, solved by filling the
    assets in order of mu up to u. (w_prev, mu, sigma, 0, 0, u, G [H, N])."""
    rng = np.random.default_rng(77)
    N, H, u = 7, 2, 0.3
    mu = rng.normal(5e-4, 0.01, (H, N))
    G = np.zeros((H, N))
    for t in range(H):
        left = 1.0
        for i in np.argsort(-mu[t]):
            G[t, i] = min(u, left)
            left -= G[t, i]
    return np.full(N, 1.0 / N), mu, 1e-4 * np.eye(N), 0.0, 0.0, u, G
