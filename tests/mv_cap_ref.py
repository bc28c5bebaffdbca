"""Reference for the mean-variance MPC program with an L1 turnover cap — a test helper, not a test.

The program (MPCConfig.mv_max_turnover = tau, kmpc_solve_mv_cap), per window:

    maximize_W  sum_t [ w_t . mu_t - gamma w_t' Sigma w_t ] - c sum_t ||w_t - w_{t-1}||_1
    s.t.        1'w_t = 1,  ||w_t - w_{t-1}||_1 <= tau,  w_{-1} = w_prev,
                w_t >= 0 unless allow_short,  w_t <= u under a position limit (long-only)

* :func:`dense_mv_cap_ipm` — ``mv_box_ref.dense_mv_box_ipm`` with the rows ``tau - sum_i s_t,i >= 0``
  appended (s present at c = 0 too), the bounds optional. It writes the goldens
  (tests/golden/make_mvcap_golden.py).
* :func:`reduced_mv_cap_ipm` — the kernel's own reduced iteration (csrc/kmpc_mv.hip, CAP form) in
  numpy, line for line: it shows on the CPU which bars the algorithm itself reaches on the inputs
  the device tests use.
* :func:`cap_distance` — d0, the L1 distance from w_prev to the feasible set of period 0: the
  program is feasible iff d0 <= tau.
* :func:`gap` — the LP certificate of mv_box_ref with the cap rows in the lifted set.
* :func:`violated` — budget 1e-9, bounds 1e-9 and the cap ||w_t - w_{t-1}||_1 <= tau + 10 tol (N + 1):
  the stopping rule lets each s -+ d row (N of them bind per period) and the cap row be off by 10 tol.
* :func:`certificate_bar` — mv_box_ref's bar with mcon counting the H cap rows.
"""
from __future__ import annotations

import numpy as np

import mv_box_ref
from mv_box_ref import inputs, mv_objective, objective_bar, scale  # noqa: F401


def _mcon(H, N, u, allow_short) -> int:
    n = H * N
    return (0 if allow_short else n) + 2 * n + (n if u else 0) + H


def certificate_bar(f, mu, sigma, gamma, cost, u=None, allow_short=False, tol=1e-10) -> float:
    """mv_box_ref.certificate_bar with the constraint count of the capped program: mu_c < tol is a
    duality gap of up to mcon tol in units of sc (mcon: n sign rows unless shorting, 2n |d| rows —
    present at c = 0 too —, n limit rows under u, H cap rows), the residuals as there."""
    H, N = np.asarray(mu).shape
    return objective_bar(f) + scale(mu, sigma, gamma, cost) * tol * (_mcon(H, N, u, allow_short) + 60 * H)


def cap_distance(w_prev, u=None, allow_short=False) -> float:
    """d0: the L1 distance from w_prev to {w: 1'w = 1, w >= 0 unless allow_short, w <= u}."""
    wp = np.asarray(w_prev, np.float64)
    if allow_short:
        return abs(1.0 - wp.sum())
    hi = float(u) if u else np.inf
    clip = np.minimum(np.maximum(wp, 0.0), hi)
    return float(np.maximum(-wp, 0.0).sum() + np.maximum(wp - hi, 0.0).sum()) + abs(1.0 - clip.sum())


def dense_mv_cap_ipm(w_prev, mu, sigma, gamma, cost, tau, u=None, allow_short=False, iters=200, tol=1e-13):
    """Dense-KKT Mehrotra IPM on the epigraph form (variables w [HN], s [HN], at c = 0 too) of the
    capped program. Returns (W [H, N], status) with status "optimal", "optimal_inaccurate" or
    "solver_error" (then W is the iterate of the smallest merit; best <= 1e-9 is "optimal")."""
    from scipy.sparse import coo_matrix

    wp = np.asarray(w_prev, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = mu.shape
    n = H * N
    nx = 2 * n
    # inequality rows G x - h >= 0: w >= 0; s -+ (w_t - w_{t-1}) >= 0; u - w >= 0; tau - sum_i s_t,i >= 0
    rows, cols, vals, h = [], [], [], []
    r = 0
    if not allow_short:
        for k in range(n):
            rows.append(r); cols.append(k); vals.append(1.0); h.append(0.0); r += 1
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
    if u:
        for k in range(n):
            rows.append(r); cols.append(k); vals.append(-1.0); h.append(-float(u)); r += 1
    for t in range(H):
        for i in range(N):
            rows.append(r); cols.append(n + t * N + i); vals.append(-1.0)
        h.append(-float(tau)); r += 1
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
    q[n:] = cost
    sc = max(np.abs(q).max(), np.abs(Q).max(), 1e-300)
    Q, q = Q / sc, q / sc
    x = np.zeros(nx)
    w0, s0 = start_point(wp, H, tau, u, allow_short)
    x[:n], x[n:] = w0.ravel(), s0.ravel()
    z = np.maximum(G @ x - h, 1e-2 * min(1.0, tau))
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


def start_point(w_prev, H, tau, u=None, allow_short=False):
    """The kernel's start (W [H, N], s [H, N]): every period at w0 = p + theta (c - p), p the
    projection of w_prev on the bounds, c the plain start 0.5 p + 0.5 / N (under a limit at most
    0.5 (u + 1 / N)), and theta = min(1, 0.5 (tau - out) / ||c - p||_1) with out = ||p - w_prev||_1,
    so that D0 = ||w0 - w_prev||_1 <= out + 0.5 (tau - out) < tau whenever out <= d0 < tau. s is |d|
    plus the same share delta = 0.5 (tau - D0) / N in every element of a period: sum_i s_0,i =
    D0 + 0.5 (tau - D0) < tau and sum_i s_t,i = 0.5 (tau - D0) later on."""
    wp = np.asarray(w_prev, np.float64)
    N = len(wp)
    p = wp.copy() if allow_short else np.maximum(wp, 0.0)
    if u:
        p = np.minimum(p, u)
    c = 0.5 * p + 0.5 / N
    if u:
        c = np.minimum(c, 0.5 * (u + 1.0 / N))
    out = float(np.abs(p - wp).sum())
    dist = float(np.abs(c - p).sum())
    theta = min(1.0, 0.5 * (tau - out) / dist) if dist > 0.0 else 1.0
    w0 = p + theta * (c - p)
    D0 = float(np.abs(w0 - wp).sum())
    delta = 0.5 * (tau - D0) / N
    W = np.tile(w0, (H, 1))
    d = W - np.vstack([wp[None, :], W[:-1]])
    return W, np.abs(d) + delta


def reduced_mv_cap_ipm(w_prev, mu, sigma, gamma, cost, tau, u=None, allow_short=False, max_iter=100, tol=1e-10):
    """The kernel's reduced Mehrotra iteration of the CAP form, line for line in numpy: the BOX
    iteration of mv_box_ref.reduced_mv_box_ipm (the bounds optional) with one more inequality per
    period, x6_t = tau - sum_i s_t,i (a slack variable) and its multiplier l6_t. Eliminating s
    leaves (al + be) ds + (be - al) dd + dl6_t = qs, so dl6 enters the w equation through
    C' = -D' diag((be - al) P) (one column per period) and the cap row reads C dw - kap dl6 = r3,
    kap_t = x6_t / l6_t + sum_i P_t,i, r3_t = -sum_i P qs + rg6_t + rc6_t / l6_t:
        M dw + A' dnu + C' dl6 = r1,  A dw = -rp,  C dw - kap dl6 = r3,
    solved by the Cholesky of M and the 2H x 2H Schur system [A; C] M^-1 [A' C'] + diag(0, kap).
    Returns (W [H, N], status, iterations, objective): status 0 / 1 / 2 / 4 as KMPC_STATUS_*
    (2: d0 > tau, then W = tile(w_prev) and the objective NaN)."""
    from scipy.linalg import cho_factor, cho_solve

    wp = np.asarray(w_prev, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = mu.shape
    n = H * N
    hw, box = not allow_short, bool(u)
    sc = scale(mu, S, gamma, cost)
    g2, cs, mus = 2.0 * gamma / sc, cost / sc, mu / sc
    if cap_distance(wp, u, allow_short) > tau:
        return np.tile(wp, (H, 1)), 2, 0, np.nan

    def prev(v, first):
        return np.vstack([first[None, :], v[:-1]])

    def nxt(v):
        return np.vstack([v[1:], np.zeros((1, N))])

    def to_bound(v, dv, a):
        neg = dv < 0
        return min(a, float(np.min(-v[neg] / dv[neg]))) if neg.any() else a

    def Cmul(g, y):
        """C y [H]: -sum_i g (y_t - y_{t-1})."""
        return -(g * (y - prev(y, np.zeros(N)))).sum(1)

    zero = np.zeros((H, N))
    w, s = start_point(wp, H, tau, u, allow_short)
    wm = prev(w, wp)
    zlo = 1e-2 * min(1.0, tau)
    z2 = np.maximum(s - (w - wm), zlo)
    z3 = np.maximum(s + (w - wm), zlo)
    x6 = np.maximum(tau - s.sum(1), zlo)
    l1 = np.ones((H, N)) if hw else zero.copy()
    l2 = np.ones((H, N))
    l3 = l2.copy()
    l5 = np.ones((H, N)) if box else zero.copy()
    l6 = np.ones(H)
    nu = np.zeros(H)
    mcon = _mcon(H, N, u, allow_short)
    A = np.kron(np.eye(H), np.ones((1, N)))          # [H, n]
    best, best_obj, best_W = 1e300, np.nan, np.tile(wp, (H, 1))
    it = 0
    for it in range(max_iter):
        wm = prev(w, wp)
        Sw = w @ S
        d = w - wm
        rg2 = (s - d) - z2
        rg3 = (s + d) - z3
        rg6 = (tau - s.sum(1)) - x6
        eta = l2 - l3
        rp = w.sum(1) - 1.0
        prmax = np.abs(rp).max()
        x5 = (u - w) if box else np.ones((H, N))
        rw = -mus + g2 * Sw - l1 + eta - nxt(eta) + nu[:, None] + l5
        rs = cs - l2 - l3 + l6[:, None]
        mu_c = (float((w * l1 + z2 * l2 + z3 * l3 + x5 * l5).sum()) + float(x6 @ l6)) / mcon
        rd = max(np.abs(rw).max(), np.abs(rs).max(), np.abs(rg2).max(), np.abs(rg3).max(), np.abs(rg6).max())
        merit = max(mu_c, rd, prmax)
        if not np.isfinite(merit):
            break
        if merit < best:
            best = merit
            best_obj = float((mu * w - gamma * w * Sw - cost * np.abs(d)).sum())
            best_W = w.copy()
        if mu_c < tol and rd < 10 * tol and prmax < 10 * tol:
            break
        W1 = (l1 / w if hw else zero) + (l5 / x5 if box else zero)
        al = l2 / z2
        be = l3 / z3
        P = 1.0 / (al + be)
        g = (be - al) * P
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
        # the columns of [A' C']: C'_{:, t} = -(g 1[period t] - next period's g 1[period t + 1])
        Ct = np.zeros((n, H))
        for t in range(H):
            e = np.zeros((H, N))
            e[t] = g[t]
            Ct[:, t] = -(e - nxt(e)).ravel()
        Y = cho_solve(cf, np.hstack([A.T, Ct]))        # [n, 2H]
        kap = x6 / l6 + P.sum(1)
        Sm = np.zeros((2 * H, 2 * H))
        for q in range(2 * H):
            yq = Y[:, q].reshape(H, N)
            Sm[:H, q] = yq.sum(1)
            Sm[H:, q] = Cmul(g, yq)
        Sm[H:, H:] += np.diag(kap)
        try:
            cs2 = cho_factor(Sm, lower=True)
        except np.linalg.LinAlgError:
            break
        rc1, rc2, rc3, rc5, rc6 = w * l1, z2 * l2, z3 * l3, x5 * l5, x6 * l6
        for pas in range(2):
            p2, p3 = rc2 / z2 + al * rg2, rc3 / z3 + be * rg3
            qs = -rs - p2 - p3
            v = g * qs + p3 - p2
            rhs = -rw - (rc1 / w if hw else zero) + (rc5 / x5 if box else zero) - (v - nxt(v))
            r3 = -(P * qs).sum(1) + rg6 + rc6 / l6
            x = cho_solve(cf, rhs.ravel())
            xm = x.reshape(H, N)
            sol = cho_solve(cs2, np.concatenate([xm.sum(1) + rp, Cmul(g, xm) - r3]))
            dnu, dl6 = sol[:H], sol[H:]
            dw = (x - Y @ sol).reshape(H, N)
            dd = dw - prev(dw, np.zeros(N))
            ds = P * (qs - (be - al) * dd - dl6[:, None])
            dz2, dz3 = ds - dd + rg2, ds + dd + rg3
            dx6 = -ds.sum(1) + rg6
            dl1 = -(l1 * dw + rc1) / w if hw else zero
            dl2 = -(l2 * dz2 + rc2) / z2
            dl3 = -(l3 * dz3 + rc3) / z3
            dl5 = (-rc5 + l5 * dw) / x5 if box else zero
            am = 1e300
            if hw:
                am = to_bound(l1, dl1, to_bound(w, dw, am))
            for a_, b_ in ((z2, dz2), (z3, dz3), (l2, dl2), (l3, dl3)):
                am = to_bound(a_, b_, am)
            if box:
                am = to_bound(l5, dl5, to_bound(x5, -dw, am))
            am = to_bound(l6, dl6, to_bound(x6, dx6, am))
            if pas == 1:
                step = min(1.0, 0.99 * am)
                break
            ap = min(1.0, am)
            mua = (float(((w + ap * dw) * (l1 + ap * dl1) + (z2 + ap * dz2) * (l2 + ap * dl2) +
                          (z3 + ap * dz3) * (l3 + ap * dl3) + (x5 - ap * dw) * (l5 + ap * dl5)).sum()) +
                   float((x6 + ap * dx6) @ (l6 + ap * dl6))) / mcon
            smu = (mua / mu_c) ** 3 * mu_c
            if hw:
                rc1 = w * l1 + dw * dl1 - smu
            rc2, rc3 = z2 * l2 + dz2 * dl2 - smu, z3 * l3 + dz3 * dl3 - smu
            if box:
                rc5 = x5 * l5 - dw * dl5 - smu
            rc6 = x6 * l6 + dx6 * dl6 - smu
        w = w + step * dw
        s = s + step * ds
        z2 = z2 + step * dz2
        z3 = z3 + step * dz3
        x6 = x6 + step * dx6
        l1 = l1 + step * dl1
        l2 = l2 + step * dl2
        l3 = l3 + step * dl3
        l5 = l5 + step * dl5
        l6 = l6 + step * dl6
        nu = nu + step * dnu
    status = 0 if best <= 1e-7 else (1 if best <= 1e-4 else 4)
    if status == 4:
        return np.tile(wp, (H, 1)), 4, it, np.nan
    return best_W, status, it, best_obj


def _lifted(w_prev, H, N, tau, u=None, allow_short=False):
    """mv_box_ref._lifted with the cap rows sum_i S_t,i <= tau and the optional bounds."""
    from scipy.sparse import csr_matrix, eye, hstack, kron, vstack

    A_ub, b_ub, A_eq, b_eq, _ = mv_box_ref._lifted(w_prev, H, N, 1.0)
    n = H * N
    cap = hstack([csr_matrix((H, n)), kron(eye(H), np.ones((1, N)))]).tocsr()
    A_ub = vstack([A_ub, cap]).tocsr()
    b_ub = np.concatenate([b_ub, np.full(H, float(tau))])
    bounds = [(None if allow_short else 0.0, float(u) if u else None)] * n + [(0.0, None)] * n
    return A_ub, b_ub, A_eq, b_eq, bounds


def feasible(w_prev, H, tau, u=None, allow_short=False) -> bool:
    """Whether the capped feasible set is non-empty, by the LP itself (a zero objective)."""
    from scipy.optimize import linprog

    N = len(w_prev)
    A_ub, b_ub, A_eq, b_eq, bounds = _lifted(w_prev, H, N, tau, u, allow_short)
    r = linprog(np.zeros(2 * H * N), A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds")
    return r.status == 0


def gap(W, w_prev, mu, sigma, gamma, cost, tau, u=None, allow_short=False) -> float:
    """mv_box_ref.gap over the capped set: an upper bound of f* - f(W) from one LP (inf if it fails)."""
    from scipy.optimize import linprog

    W = np.asarray(W, np.float64)
    mu = np.asarray(mu, np.float64)
    S = np.asarray(sigma, np.float64)
    H, N = W.shape
    SW = W @ S
    q = float((W * mu).sum()) - gamma * float((W * SW).sum())
    grad = (mu - 2.0 * gamma * SW).ravel()
    A_ub, b_ub, A_eq, b_eq, bounds = _lifted(w_prev, H, N, tau, u, allow_short)
    lp = np.concatenate([-grad, np.full(H * N, float(cost))])
    r = linprog(lp, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs-ds")
    if r.status != 0:
        return float("inf")
    bound = q - float(grad @ W.ravel()) - float(r.fun)
    return bound - mv_objective(W, w_prev, mu, S, gamma, cost)


def turnover(W, w_prev):
    """||w_t - w_{t-1}||_1 per period [H]."""
    W = np.asarray(W, np.float64)
    return np.abs(np.diff(np.vstack([np.asarray(w_prev, np.float64)[None, :], W]), axis=0)).sum(1)


def cap_bar(N, tol=1e-10) -> float:
    """What the stopping rule lets the cap be missed by: 10 tol in each of the N binding s -+ d rows
    of a period and in the cap row itself."""
    return 10.0 * tol * (N + 1)


def violated(W, w_prev, tau, u=None, allow_short=False, tol=1e-10) -> list:
    """The feasibility bars on one window's W [H, N]: budget 1e-9, bounds 1e-9 (the project's) and
    the cap tau + cap_bar(N). Returns the bars W misses as text (empty: feasible)."""
    W = np.asarray(W, np.float64)
    if not np.isfinite(W).all():
        return ["non-finite W"]
    bad = []
    e = np.abs(W.sum(1) - 1).max()
    if not e <= 1e-9:
        bad.append(f"budget off by {e:.3e}")
    if not allow_short and not W.min() >= -1e-9:
        bad.append(f"min w {W.min():.3e}")
    if u and not W.max() <= u + 1e-9:
        bad.append(f"max w - u {W.max() - u:.3e}")
    ex = float(turnover(W, w_prev).max() - tau)
    if not ex <= cap_bar(W.shape[1], tol):
        bad.append(f"turnover - tau {ex:.3e}")
    return bad


# ---- the inputs of tests/test_mv_cap_gpu.py, here so that tests/test_mv_cap_cpu.py can show on the
# CPU that the kernel's algorithm (reduced_mv_cap_ipm) reaches the bars on these very inputs ----

# (N, H, gamma, c, tau, u, allow_short, B): every shape of the device tests, at most 4 windows each
CASES = [
    (4, 1, 1.0, 1e-3, 0.2, None, False, 4),
    (10, 1, 1.0, 1e-3, 0.2, None, False, 4),
    (10, 1, 1.0, 0.0, 0.2, None, False, 4),
    (64, 2, 1.0, 1e-3, 0.2, 0.05, False, 4),      # n = 128: the last LDS shape
    (8, 16, 1.0, 1e-3, 0.2, None, False, 3),      # n = 128 at KMPC_MV_MAX_H: the 32 x 32 Schur system
    (129, 1, 1.0, 1e-3, 0.2, None, False, 4),     # the first workspace shape
    (43, 3, 1.0, 1e-3, 0.05, None, False, 4),
    (10, 3, 1.0, 1e-3, 0.2, None, True, 4),       # shorting
    (16, 8, 1.0, 1e-3, 0.2, None, False, 3),      # many periods
    (16, 8, 1.0, 0.0, 0.2, 0.3, False, 3),
    (300, 2, 1.0, 1e-3, 0.2, None, False, 2),
    (512, 2, 1.0, 1e-3, 0.2, 0.005, False, 2),    # n = 1024 (the dense reference stops at n = 600)
    (64, 16, 1.0, 0.0, 0.2, None, False, 2),      # n = 1024 at H = KMPC_MV_MAX_H
]


def case_id(case) -> str:
    N, H, gamma, c, tau, u, short, B = case
    return f"N{N}_H{H}_c{c:g}_tau{tau:g}" + (f"_u{u:g}" if u else "") + ("_short" if short else "")


def case_inputs(case):
    """(w_prev [B, N], mu [B, H, N], sigma [B, N, N]) of one case: window 1 starts at 1/N, window 2
    at a vertex (long-only without a limit; under a limit the vertex lies outside it and is the
    infeasible-window test's), and with shorting the weights carry negative entries."""
    N, H, gamma, c, tau, u, short, B = case
    wp, mu, S = inputs(11001 + 10 * N + H, B, N, H, vertex=not u)
    if short:
        rng = np.random.default_rng(N + H)
        wp = wp + rng.normal(0.0, 0.05, wp.shape)
        wp[0] /= wp[0].sum()          # window 0 on the budget plane, the others off it by a little
        wp[1:] /= (wp[1:].sum(1, keepdims=True) * (1.0 + 0.02 * rng.random((B - 1, 1))))
    if u:
        wp = np.minimum(wp, u)
        wp = wp + (1.0 - wp.sum(1, keepdims=True)) * (u - wp) / (u - wp).sum(1, keepdims=True)
    return wp, mu, S


def edge_cases():
    """One window each: (name, w_prev [N], mu [H, N], sigma [N, N], gamma, c, tau, u, allow_short)."""
    out = []
    wp, mu, S = inputs(5100, 1, 10, 2)
    worst = np.zeros(10)
    worst[int(np.argmin(mu[0, 0]))] = 1.0
    out.append(("w_prev = the vertex of lowest mu", worst, mu[0], S[0], 1.0, 1e-3, 0.2, None, False))
    out.append(("the same vertex, c = 0", worst, mu[0], S[0], 1.0, 0.0, 0.2, None, False))
    z = wp[0].copy()
    z[[1, 4, 7]] = 0.0
    out.append(("zeros in w_prev", z / z.sum(), mu[0], S[0], 1.0, 1e-3, 0.2, None, False))
    out.append(("zeros in w_prev, u = 0.3", np.minimum(z / z.sum(), 0.3) / np.minimum(z / z.sum(), 0.3).sum(),
                mu[0], S[0], 1.0, 1e-3, 0.2, 0.3, False))
    out.append(("tau = 1e-6", wp[0], mu[0], S[0], 1.0, 1e-3, 1e-6, None, False))
    out.append(("tau = 1e-6, c = 0, vertex", worst, mu[0], S[0], 1.0, 0.0, 1e-6, None, False))
    out.append(("tau = 1e-6, shorting", wp[0] * 1.5 - 0.05, mu[0], S[0], 1.0, 1e-3, 1e-6, None, True))
    on = np.array([0.25, 0.25, 0.25, 0.05, 0.05, 0.05, 0.04, 0.03, 0.02, 0.01])
    out.append(("w_prev on the limit", on, mu[0], S[0], 1.0, 1e-3, 0.2, 0.25, False))
    over = np.array([0.30, 0.25, 0.20, 0.05, 0.05, 0.05, 0.04, 0.03, 0.02, 0.01])
    out.append(("w_prev past the limit, 2E = 0.1 < tau", over, mu[0], S[0], 1.0, 1e-3, 0.2, 0.25, False))
    return out


def cannot_bind():
    """tau = 2 long-only: no two points of the simplex are further apart, so the cap cannot bind and
    the optimum is the plain program's. (N, H, gamma, c, tau, w_prev [4, N], mu, sigma)."""
    N, H = 12, 2
    wp, mu, S = inputs(4242, 4, N, H)
    return N, H, 1.0, 1e-3, 2.0, wp, mu, S


def neighbour_windows(path):
    """Five windows of a golden file under a limit u = 4 / N, for the device test of a NaN window and
    an infeasible one between solved ones: windows 0, 2 and 4 are solved; window 1 carries a NaN in mu;
    window 3 starts E = 0.6 tau above the limit in asset 0, so d0 = 2E > tau.
    (w_prev [5, N], mu, sigma, gamma, c, tau, u)."""
    g = np.load(path)
    gamma, c, tau = (float(v) for v in g["config"][:3])
    N = g["mu"].shape[2]
    idx = [0, 1, 0, 1, 1]
    wp, mu, S = g["w_prev"][idx].copy(), g["mu"][idx].copy(), g["sigma"][idx].copy()
    u = 4.0 / N
    wp = np.minimum(np.abs(wp), u)
    wp = wp + (1.0 - wp.sum(1, keepdims=True)) * (u - wp) / (u - wp).sum(1, keepdims=True)
    mu[1, 0, 1] = np.nan
    E = 0.6 * tau
    wp[3, 1:] *= (1.0 - u - E) / wp[3, 1:].sum()
    wp[3, 0] = u + E
    return wp, mu, S, gamma, c, tau, u


# w_prev = [0.5, 0.3, 0.1, 0.1] under u = 0.25: E = 0.3 leaves the limit, d0 = 2E = 0.6
INFEASIBLE = (np.array([0.5, 0.3, 0.1, 0.1]), 0.25, 0.6)


def closed_form(N=8, tau=0.2, seed=5):
    """gamma = 0, c = 0, H = 1, w_prev = 1/N: a linear program whose optimum moves tau / 2 into the
    best-mu asset, taken from the worst-mu assets in order (each gives at most its 1/N).
    (w_prev, mu [1, N], sigma, W [1, N])."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(5e-4, 0.01, (1, N))
    wp = np.full(N, 1.0 / N)
    W = wp.copy()
    W[int(np.argmax(mu[0]))] += tau / 2
    left = tau / 2
    for i in np.argsort(mu[0]):
        take = min(left, W[i])
        W[i] -= take
        left -= take
        if left <= 0:
            break
    return wp, mu, 1e-4 * np.eye(N), W[None, :]
