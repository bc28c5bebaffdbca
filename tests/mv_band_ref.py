"""The band form of the mean-variance Newton system — a test helper, not a test.

The Newton matrix of the multi-period mean-variance program (csrc/kmpc_mv.hip),

    M = 2 gamma (I_H (x) Sigma) + diag(.) + D' diag(E) D,

is block tridiagonal with diagonal off-diagonal blocks: half-bandwidth N, no fill outside the band in
its Cholesky factor. The band kernels (kmpc_solve_mv_band) keep row r's columns r - N .. r and clip
the dense kernel's right-looking, panel-blocked factorization and its triangular solves to the band.

* :func:`newton_matrix` — M as the kernel assembles it, from given barrier terms.
* :func:`band_cholesky` / :func:`band_solve` — the kernel's band-clipped loops restated in numpy on
  the band layout (row r, column c at [r, c - r + N]).
* :func:`banded_linalg` — a context in which ``scipy.linalg.cho_factor`` / ``cho_solve`` ARE the band
  restatement, so that the reduced iterations of tests/mv_cap_ref.py and tests/mv_box_ref.py (which
  import the two inside the function) run the band linear algebra and everything else unchanged.
* CASES — the shapes and constraint sets of tests/test_mv_band_gpu.py, here so that the CPU tests
  can run the restated iteration on the same inputs.
"""
from __future__ import annotations

import contextlib

import numpy as np

import mv_cap_ref

PB = 8   # the kernel's panel width


def newton_matrix(S, H, gamma_scaled, diag, E):
    """M [n, n] for Sigma S [N, N]: g2 (I_H (x) S) + diag(diag + E + E_next) with -E_next on the
    N-th sub- and super-diagonal (D' diag(E) D, D differencing consecutive periods). diag, E: [H, N]."""
    N = S.shape[0]
    n = H * N
    En = np.vstack([E[1:], np.zeros((1, N))])
    M = gamma_scaled * np.kron(np.eye(H), S) + np.diag((diag + E + En).ravel())
    for k in range(n - N):
        M[k + N, k] -= En.ravel()[k]
        M[k, k + N] -= En.ravel()[k]
    return M


def to_band(M, N):
    """The lower band of M [n, n] in the band layout [n, N + 1]: (r, c) at [r, c - r + N]; the
    slots of columns < 0 are NaN (the kernel never reads them)."""
    n = M.shape[0]
    Bd = np.full((n, N + 1), np.nan)
    for r in range(n):
        lo = max(0, r - N)
        Bd[r, lo - r + N:] = M[r, lo:r + 1]
    return Bd


def from_band(Bd, N):
    """The lower-triangular [n, n] matrix of a band array (zero outside the band)."""
    n = Bd.shape[0]
    L = np.zeros((n, n))
    for r in range(n):
        lo = max(0, r - N)
        L[r, lo:r + 1] = Bd[r, lo - r + N:]
    return L


def band_cholesky(Bd, N):
    """The kernel's factorization on the band array, in place on a copy: panels of PB columns; inside
    a panel column j is scaled over rows j + 1 .. min(n - 1, j + N) and updates the panel's remaining
    columns q <= min(k, je - 1, j + N) of those rows; then the trailing update of rows je .. je - 1 + N,
    columns je .. k, with the panel entries outside a row's band taken as zero. Returns (band L, ok):
    ok False where a pivot is not positive (the kernel's flag)."""
    L = np.array(Bd, np.float64)
    n = L.shape[0]
    at = lambda r, c: (r, c - r + N)
    ok = True
    for jb in range(0, n, PB):
        je = min(jb + PB, n)
        for j in range(jb, je):
            dj = L[at(j, j)]
            if not (dj > 0.0) or not (dj < 1e300):
                ok = False
            lj = np.sqrt(max(dj, 1e-300))
            L[at(j, j)] = lj
            hi = min(n - 1, j + N)
            for k in range(j + 1, hi + 1):
                L[at(k, j)] *= 1.0 / lj
            for k in range(j + 1, hi + 1):
                lkj = L[at(k, j)]
                for q in range(j + 1, min(k, je - 1, j + N) + 1):
                    L[at(k, q)] -= lkj * L[at(q, j)]
        for k in range(je, min(n, je + N)):
            lk = [L[at(k, p)] if p >= k - N else 0.0 for p in range(jb, je)]
            for c in range(je, k + 1):
                v = L[at(k, c)]
                for i, p in enumerate(range(jb, je)):
                    if p >= c - N:
                        v -= lk[i] * L[at(c, p)]
                L[at(k, c)] = v
    return L, ok


def band_solve(L, N, b):
    """x = (L L')^-1 b on the band factor, the kernel's two substitutions: column j of the forward
    pass reaches rows j + 1 .. j + N, column j of the backward pass rows j - N .. j - 1. b [n] or
    [n, m]."""
    n = L.shape[0]
    x = np.array(b, np.float64)
    for j in range(n):
        x[j] = x[j] / L[j, N]
        hi = min(n - 1, j + N)
        for r in range(j + 1, hi + 1):
            x[r] = x[r] - L[r, j - r + N] * x[j]
    for j in range(n - 1, -1, -1):
        x[j] = x[j] / L[j, N]
        for r in range(max(0, j - N), j):
            x[r] = x[r] - L[j, r - j + N] * x[j]
    return x


def bandwidth(M) -> int:
    """The half-bandwidth of a symmetric matrix: the largest |r - c| of a non-zero entry."""
    r, c = np.nonzero(M)
    return int(np.abs(r - c).max()) if len(r) else 0


@contextlib.contextmanager
def banded_linalg(N, log=None):
    """Within the context scipy.linalg.cho_factor(M, lower=True) factors every matrix that has nothing
    outside half-bandwidth N — the n x n Newton matrix — by band_cholesky and cho_solve solves with it
    by band_solve; a matrix with entries past the band (the dense Schur system where 2 H > N + 1) keeps
    scipy's. log, a list, receives the order of every matrix factored in the band form."""
    import scipy.linalg as sl
    f0, s0 = sl.cho_factor, sl.cho_solve

    class _Band:
        def __init__(self, L):
            self.L = L

    def cho_factor(M, lower=False, **kw):
        M = np.asarray(M, np.float64)
        if bandwidth(M) > N:   # (the dense Schur system; a matrix inside the band is the band form's in any case)
            return f0(M, lower=lower, **kw)
        L, ok = band_cholesky(to_band(M, N), N)
        if not ok:
            raise np.linalg.LinAlgError("band Cholesky: non-positive pivot")
        if log is not None:
            log.append(M.shape[0])
        return _Band(L), True

    def cho_solve(cf, b, **kw):
        if isinstance(cf[0], _Band):
            return band_solve(cf[0].L, N, b)
        return s0(cf, b, **kw)

    sl.cho_factor, sl.cho_solve = cho_factor, cho_solve
    try:
        yield
    finally:
        sl.cho_factor, sl.cho_solve = f0, s0


# ---- the inputs of tests/test_mv_band_gpu.py ----------------------------------------------------

def limit_for(N) -> float:
    """The position limit of the "limit" constraint sets: 2.5 / N, at most 0.8 (N u > 1 at every N)."""
    return min(0.8, 2.5 / N)


# (N, H, B): every shape of the device tests. The LDS variant holds a window while its LDS footprint
# stays within KMPC_MV_BAND_LDS_BYTES = 65,536: at H = 2 without the cap (61, 2) is the last shape
# that fits (64,656 bytes) and (62, 2) the first that does not; under the cap (61, 2) is past it too.
SHAPES = [
    (2, 2, 4),
    (3, 16, 3),
    (10, 5, 4),       # well inside the LDS variant
    (10, 1, 4),       # H = 1: the band is the full triangle
    (13, 10, 3),      # n = 130: just past the dense kernels' LDS edge, still in LDS here
    (61, 2, 3),       # at the LDS threshold (the last shape that fits at H = 2)
    (62, 2, 3),       # past it: the first workspace shape at H = 2
    (65, 2, 3),       # band rows cross a wave boundary
    (129, 1, 3),
    (100, 10, 2),     # the headline shape
    (64, 16, 2),      # n = 1024 at KMPC_MV_MAX_H
    (512, 2, 2),      # n = 1024, N = 512
]
# name -> (c, tau, limit?, allow_short)
SETS = {
    "plain": (1e-3, 0.0, False, False),
    "short": (1e-3, 0.0, False, True),
    "c0": (0.0, 0.0, False, False),
    "limit": (1e-3, 0.0, True, False),
    "cap": (1e-3, 0.2, False, False),
    "limit_cap": (1e-3, 0.2, True, False),
}
GAMMA = 1.0


def case(shape, name):
    """The mv_cap_ref case tuple (N, H, gamma, c, tau, u, allow_short, B) of a shape and a set."""
    N, H, B = shape
    c, tau, lim, short = SETS[name]
    return (N, H, GAMMA, c, tau, limit_for(N) if lim else None, short, B)


def case_inputs(cs):
    """(w_prev [B, N], yhat [B, H, N] float32, sigma [B, N, N]) of a case: mv_cap_ref.case_inputs with
    the forecasts rounded to float32, as the band kernel reads them."""
    wp, mu, S = mv_cap_ref.case_inputs(cs)
    return wp, mu.astype(np.float32), S


def lds_bytes(N, H, cap) -> int:
    """The band kernels' LDS footprint of one window (csrc/kmpc_mv.hip: mv_band_lds_bytes)."""
    n = N * H
    small = (2 * n + 4 * H * H + 13 * H + 18) if cap else (2 * n + H * H + 4 * H + 18)
    return 8 * (small + n * ((N | 1) + 1) + (2 if cap else 1) * H * n)


def in_lds(N, H, cap) -> bool:
    return N * H <= 256 and lds_bytes(N, H, cap) <= 65536
