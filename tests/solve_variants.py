"""The kernels of the plain solve (kmpc_solve) and the matrix of shapes, constraint cases and paths
that reaches each of them: shared by test_solve_variants_cpu.py (the matrix names every kernel; the
mirror below is pinned to the library) and test_solve_variants_gpu.py (every cell against the
long-double oracle).

kmpc_solve sends a call to one of 62 kernels:

* the closed-form presolve (kmpc_solve_simplex.hip);
* the large-window ipm_big<HM, MAXT, FL> (kmpc_solve_big.h): HM 10 / 21 x 256 / 512 / 1024 threads x
  case 7 / the constraint case read at run time;
* 17 packed rungs (visit_packed, kmpc_solve_args.h): HM 2 and 5 on 16- and 32-lane groups, HM 10 on
  32-lane groups; case 7 (and at N <= 10 on 16 lanes its 11-slot form), case 1 and the generic one;
* 12 constant-case rungs (visit_case): H = 5 / 10, case 7 at 64 / 128 / 256 threads, case 1 at 64 /
  128, and at H = 10 the two forms with the LDL^T arrays in LDS (104-lane stride, the C3 rung, and
  216-lane stride);
* 20 generic register kernels (launch_ipm): HM 2 / 5 / 10 x 64 / 128 / 256 threads x exact / ragged
  H, and at HM 10 the two 104-stride forms for 64 < N < 104.

kernel_of is a hand mirror of that dispatch (solve_plan in kmpc_solve.hip and the launchers it calls)
in float64: precision AUTO below KMPC_MIXED_MIN_B windows, where the C3 rung runs its float64 kernel.
"""
import functools

import numpy as np

PATH_AUTO, PATH_REGISTER, PATH_LARGE, PATH_REGISTER_UNPACKED = 0, 1, 2, 3   # include/kmpc.h
PACK_MIN_B, MIXED_MIN_B = 512, 2048
QL_CS, QL_CS256 = 104, 216          # kmpc_solve_args.h
BIG_SLOTS_SMALL, BIG_SLOTS = 768, 512   # kmpc_solve_big.h: window slots for N <= 256, past it
B = 6                               # windows per cell of the matrix

# name -> (cost_coeff, max_turnover, allow_short)
CASES = {"k7": (1e-3, 0.2, False), "k7c0": (0.0, 0.3, False), "k3": (1e-3, 0.0, False), "k1": (0.0, 0.0, False),
         "k6": (5e-3, 0.5, True), "k2": (5e-3, 0.0, True)}

# shorting without turnover terms (case 0): the program is unbounded; not a cell of the matrix
UNBOUNDED = {"k0": (0.0, 0.0, True)}
ALL_CASES = {**CASES, **UNBOUNDED}
# one shape per family for the unbounded program: (N, H, path)
UNBOUNDED_SHAPES = [(10, 5, PATH_REGISTER), (65, 5, PATH_AUTO), (110, 10, PATH_AUTO), (200, 3, PATH_AUTO),
                    (40, 3, PATH_LARGE), (257, 10, PATH_AUTO), (20, 11, PATH_AUTO)]


def case_of(c, tau, short):
    """case_of of kmpc_solve_args.h: 1 = no short, 2 = turnover terms (cost or cap), 4 = cap."""
    return (0 if short else 1) | (2 if c > 0 or tau > 0 else 0) | (4 if tau > 0 else 0)


def _threads(N):
    return 64 * ((N + 63) // 64)


def _hm(H):
    return 2 if H <= 2 else 5 if H <= 5 else 10


def _fl(fl):
    return {7: "k7", 1: "k1"}.get(fl, "gen")


def _big(N, H, fl):
    """big::launch<HM> -> launch_t<HM, MAXT>: case 7 has its own kernel, every other case the generic."""
    assert 1 <= N <= 1024 and 1 <= H <= 21
    nt = _threads(N)
    return f"big_hm{10 if H <= 10 else 21}_{256 if nt <= 256 else 512 if nt <= 512 else 1024}_{_fl(fl if fl == 7 else -1)}"


def _packed(N, H, fl):
    """visit_packed<HM>: N <= 32, H <= 10 (3 HM <= 32 holds for HM = 2, 5, 10)."""
    hm = _hm(H)
    exact = H == hm
    if 3 * hm <= 16 and N <= 16:
        if exact and fl == 7:
            return f"pack_hm{hm}_g16_k7s11" if N <= 10 else f"pack_hm{hm}_g16_k7"
        return f"pack_hm{hm}_g16_{_fl(fl if exact else -1)}"
    return f"pack_hm{hm}_g32_{_fl(fl if exact else -1)}"


def _case(N, H, fl):
    """visit_case<H>: the constant-case rung of an H = 5 / 10 window of N <= 256, or None."""
    nt = _threads(N)
    if H not in (5, 10) or nt > 256:
        return None
    if fl == 7:
        if H == 10 and nt == 128 and N < QL_CS:
            return "case_hm10_128_k7_ql104"           # the C3 rung
        if H == 10 and nt == 256 and N < QL_CS256:    # 193 <= N < 216: a 192-thread block (N <= 192)
            return "case_hm10_256_k7_ql216"           # runs the plain 256-thread kernel below
        return f"case_hm{H}_{64 if nt <= 64 else 128 if nt <= 128 else 256}_k7"
    if fl == 1 and nt <= 128:
        return f"case_hm{H}_{64 if nt <= 64 else 128}_k1"
    return None


def _generic(N, H):
    """launch_ipm<HM>: one workgroup of 64 ceil(N / 64) threads, the case read at run time."""
    hm, nt = _hm(H), _threads(N)
    assert nt <= 256 and H <= 10
    ex = "exact" if H == hm else "ragged"
    if nt <= 64:
        return f"gen_hm{hm}_64_{ex}"
    if hm == 10 and nt == 128 and N < QL_CS:
        return f"gen_hm10_128ql_{ex}"
    return f"gen_hm{hm}_{128 if nt <= 128 else 256}_{ex}"


def kernel_of(N, H, c, tau, short, path=PATH_AUTO, B=B):
    """The kernel kmpc_solve runs B windows of (N, H) on, in the order of solve_plan."""
    fl = case_of(c, tau, short)
    if path == PATH_AUTO and fl == 1:                                     # simplex_case
        return "simplex"
    if path == PATH_LARGE or (path == PATH_AUTO and (N > 256 or H > 10)):   # use_big
        return _big(N, H, fl)
    assert N <= 256 and H <= 10, "the register paths have no kernel past 256 assets or 10 periods"
    if path != PATH_REGISTER_UNPACKED and N <= 32 and (path != PATH_AUTO or B > PACK_MIN_B or H <= 2):   # pack_small
        return _packed(N, H, fl)
    rung = _case(N, H, fl)
    if rung is not None:
        assert rung != "case_hm10_128_k7_ql104" or B < MIXED_MIN_B, "AUTO takes the mixed pair from 2,048 windows"
        return rung
    return _generic(N, H)


def persistent(name):
    """Whether kmpc_backtest_run has a path-persistent form of the kernel: a case-7 exact-H packed
    or constant-case rung (Plan::persistent in kmpc_solve.hip)."""
    return name.startswith(("pack_", "case_")) and "_k7" in name


def big_hm(name):
    """The compiled horizon bound of a large-window kernel, None for any other."""
    return int(name.split("_")[1][2:]) if name.startswith("big_") else None


# all 62, from the template parameter ranges
KERNELS = (["simplex"]
           + [f"big_hm{hm}_{t}_{fl}" for hm in (10, 21) for t in (256, 512, 1024) for fl in ("k7", "gen")]
           + [f"pack_hm{hm}_g16_{fl}" for hm in (2, 5) for fl in ("k7s11", "k7", "k1", "gen")]
           + [f"pack_hm{hm}_g32_{fl}" for hm in (2, 5, 10) for fl in ("k7", "k1", "gen")]
           + [f"case_hm{hm}_{t}_k7" for hm in (5, 10) for t in (64, 128, 256)]
           + [f"case_hm{hm}_{t}_k1" for hm in (5, 10) for t in (64, 128)]
           + ["case_hm10_128_k7_ql104", "case_hm10_256_k7_ql216"]
           + [f"gen_hm{hm}_{t}_{ex}" for hm in (2, 5, 10) for t in (64, 128, 256) for ex in ("exact", "ragged")]
           + ["gen_hm10_128ql_exact", "gen_hm10_128ql_ragged"])

# ---- the matrix -----------------------------------------------------------------------------------

SMALL = [(N, H) for N in (10, 11, 16, 17, 32) for H in (2, 1, 5, 3)] + [(1, 10), (20, 10), (32, 10), (32, 6), (9, 9)]
REGISTER = [(33, 2), (64, 1), (65, 2), (128, 1), (129, 2), (256, 1), (192, 2),
            (33, 5), (64, 3), (65, 5), (128, 4), (104, 5), (129, 5), (256, 3), (193, 5),
            (33, 10), (64, 6), (65, 10), (103, 9), (103, 10), (104, 10), (128, 10), (104, 7), (129, 10), (192, 10),
            (215, 10), (216, 10), (256, 10), (193, 8), (256, 6)]
FORCED_LARGE = [(40, 3), (100, 10), (256, 10)]
LARGE = [(257, 10), (512, 3), (513, 10), (1024, 2), (20, 11), (256, 21), (100, 15), (257, 11), (512, 12), (300, 21),
         (513, 11), (700, 12)]

# (family, N, H, path, path of case k1): under PATH_AUTO case k1 would run the presolve, so it goes
# on the path that names the interior point of the same family
_ROWS = ([("packed", N, H, PATH_REGISTER, PATH_REGISTER) for N, H in SMALL]
         + [("unpacked", N, H, PATH_REGISTER_UNPACKED, PATH_REGISTER_UNPACKED) for N, H in SMALL]
         + [("register", N, H, PATH_AUTO, PATH_REGISTER) for N, H in REGISTER]
         + [("forced_large", N, H, PATH_LARGE, PATH_LARGE) for N, H in FORCED_LARGE]
         + [("large", N, H, PATH_AUTO, PATH_LARGE) for N, H in LARGE])
# every cell: (family, N, H, case name, path)
MATRIX = [(fam, N, H, name, k1_path if name == "k1" else path)
          for fam, N, H, path, k1_path in _ROWS for name in CASES]
SHAPES = sorted({(N, H) for _, N, H, _, _ in MATRIX})


def cell_kernel(N, H, name, path):
    return kernel_of(N, H, *CASES[name], path=path, B=B)


def cell_id(N, H, name, path):
    return f"N{N}_H{H}-{name}-{cell_kernel(N, H, name, path)}"


NAN_WINDOW, INFEASIBLE_WINDOW = 1, 4


def inputs(N, H, name):
    """w_prev [6, N] float64 and yhat [6, H, N] float32 of one (shape, case): window 1 has a NaN in
    its last period; where the case has a cap (and N > 1) window 4 starts from w_prev = 3 e_0, whose
    sum the cap keeps from reaching the budget."""
    c, tau, short = ALL_CASES[name]
    rng = np.random.default_rng(100000 * N + 100 * H + sum(map(ord, name)))
    wp = rng.dirichlet(np.ones(N), B)
    if short:
        wp = wp * 1.5 - 0.5 / N
    y = rng.normal(5e-4, 0.02, (B, H, N)).astype(np.float32)
    y[NAN_WINDOW, H - 1, N // 2] = np.nan
    if tau > 0 and N > 1:
        wp[INFEASIBLE_WINDOW] = 0.0
        wp[INFEASIBLE_WINDOW, 0] = 3.0
    return wp, y


def intended_status(N, H, name):
    """The status each window is built to have: 0, 4 at the NaN window, 2 at the infeasible one."""
    st = np.zeros(B, np.int32)
    st[NAN_WINDOW] = 4
    if ALL_CASES[name][1] > 0 and N > 1:
        st[INFEASIBLE_WINDOW] = 2
    return st


# the (N, H, case, window) where the long-double oracle itself ends optimal_inaccurate (status 1)
ORACLE_INACCURATE = {(17, 2, "k2", 2), (32, 2, "k2", 0), (193, 5, "k2", 0)}


@functools.lru_cache(maxsize=None)
def reference(N, H, name):
    """(w_prev, yhat, W, status, value, iterations) of the long-double oracle on inputs(N, H, name):
    computed once per input, shared by the cells and paths that use it, read-only."""
    from oracle import solver as oracle
    c, tau, short = ALL_CASES[name]
    wp, y = inputs(N, H, name)
    out = (wp, y) + tuple(oracle.solve_batch(wp, y, c, tau, allow_short=short))
    for a in out:
        a.setflags(write=False)
    return out
