// kmpc_mv.hip — batched mean-variance MPC solve (replaces solve_mpc_mean_variance, mpc.py:119-184),
// the Markowitz rolling moments (MarkowitzStrategy.rebalance, baselines.py:70-88), their covariance
// under a shrinkage or an exponentially weighted estimator (rolling_cov_kernel) and the Markowitz
// backtest of P paths, every step of a path in one workgroup (mv_bt_kernel, further down).
//
// Program per window (mpc.py:128, 145-172):
//   maximize  sum_t [ w_t . mu_t - gamma w_t' Sigma w_t ] - c sum_t ||w_t - w_{t-1}||_1
//   s.t.      1'w_t = 1, w_t >= 0 unless allow_short          (no turnover cap), w_{-1} = w_prev;
//             with a position limit (kmpc_solve_mv_box, the BOX kernels) also w_t <= u, long-only;
//             with a turnover cap (kmpc_solve_mv_cap, the CAP kernels) also ||w_t - w_{t-1}||_1 <= tau.
// One workgroup per window, one element (t, i) of W per thread (n = H N <= 1024). Algorithm:
// Mehrotra predictor-corrector primal-dual interior point on the epigraph form (s_ti >= |d_ti|,
// d = w_t - w_{t-1}), float64, objective scaled by max(|mu|, 2 gamma |Sigma|, c). The s rows and
// all multipliers are eliminated per element, leaving the dense SPD system
//   M dw + A' dnu = r,  A dw = r2,   M = 2 gamma (I_H (x) Sigma) + diag(l1 / w) + D' diag(E) D
// (D: differencing in t, E = 4 alpha beta / (alpha + beta) from the two |d| rows), solved with a
// right-looking Cholesky of M in LDS (thread r owns row r) and the H x H Schur complement
// S = A M^{-1} A' for the budget multipliers. Test-side restatement: oracle/mv_ref.py.
// Storage: M (n x n) and M^{-1} A' sit in LDS while they fit (n <= 128); past that in a per-block
// slab of the caller's workspace (L2-resident: 2 MB at n = 500), with a persistent grid of
// min(B, MV_SLOTS) blocks walking the windows.
// Band form (kmpc_solve_mv_band, kmpc_koopman_mv_run; the BAND flag of mv_window): M is block
// tridiagonal with diagonal off-diagonal blocks, so its half-bandwidth is N and its Cholesky factor
// has no fill outside the band. Row r keeps columns r - N .. r (N + 1 doubles), the factorization and
// the solves are the dense ones with every loop clipped to the band, and mu is the rollout's float32
// yhat, widened on read. Everything else of the window is the dense form's.
//
// Status / fallback as mpc.py:180-181: non-optimal -> W = tile(w_prev), obj = NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "kmpc_internal.h"
#include "kmpc_bt_step.h"

namespace kmpc {
namespace {

struct MvArgs {
    int B, N, H;
    double gamma, c;
    int allow_short, max_iter, return_full;
    double tol;
    union {                 // (one slot: the dense kernels' argument block keeps its layout)
        const double* mu;   // [B, H, N]
        const float* muf;   // BAND kernels: [B, H, N] float32 (the rollout's yhat), read in place of mu
    };
    const double* sigma;    // [B, N, N], or one [N, N] when sigma_stride == 0
    size_t sigma_stride;    // elements between consecutive windows' Sigma
    const double* wp;       // [B, N]
    double* wout;           // [B, N] or [B, H, N]
    int* status;
    double* obj;
    int* iters;
    double* ws;             // workspace slabs (global-M variant)
    size_t slab;            // doubles per slab
    double max_weight;      // BOX kernels: the per-asset position limit u (w <= u), N u > 1
    double max_turnover;    // CAP kernels: the turnover cap tau (||w_t - w_{t-1}||_1 <= tau), > 0
};

constexpr int MV_SLOTS = 512;   // windows in flight of the global-M variant

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
// block reductions (<= 2 waves): wave reduce, one slot per wave, fixed summation order
__device__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) s += red[q];
    return s;
}
__device__ double block_max(double v, double* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q) s = fmax(s, red[q]);
    return s;
}
__device__ double block_min(double v, double* red) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q) s = fmin(s, red[q]);
    return s;
}
// value of element k - N (previous period) / k + N (next period) of a per-thread vector
__device__ double prev_period(double v, double* vec, int k, int n, int N, double first) {
    __syncthreads();
    if (k < n) vec[k] = v;
    __syncthreads();
    return (k < n && k >= N) ? vec[k - N] : first;
}
__device__ double next_period(double v, double* vec, int k, int n, int N) {
    __syncthreads();
    if (k < n) vec[k] = v;
    __syncthreads();
    return (k + N < n) ? vec[k + N] : 0.0;
}
// per-period sums of a per-thread vector into pv[H] (visible to all threads on return)
__device__ void period_sums(double v, double* vec, double* pv, int k, int n, int N, int H) {
    __syncthreads();
    if (k < n) vec[k] = v;
    __syncthreads();
    if (k < H) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += vec[k * N + j];
        pv[k] = s;
    }
    __syncthreads();
}
__device__ __forceinline__ double to_bound(double v, double dv, double a) {
    return dv < 0.0 ? fmin(a, -v / dv) : a;
}

// M and its factor L are stored packed lower-triangular, row r at r (r + 1) / 2: the factorization
// and the solves only touch entries (r, c <= r), and the packed window fits three per CU at n = 100.
__device__ __forceinline__ size_t tri(int r, int c) { return (size_t)r * (r + 1) / 2 + c; }

// x = M^{-1} b with M = L L' (lower factor in place, packed); thread r owns row r. (A
// single-wave variant with the vector in registers and v_readlane broadcasts measured no faster at
// n = 100 and 11% slower at n = 300: the factorization, not the solves, bounds this kernel.)
__device__ double chol_solve(const double* M, int n, double b, double* vec) {
    const int r = threadIdx.x;
    double x = b;
    for (int j = 0; j < n; ++j) {
        if (r == j) vec[j] = x / M[tri(j, j)];
        __syncthreads();
        if (r > j && r < n) x -= M[tri(r, j)] * vec[j];
    }
    double y = r < n ? vec[r] : 0.0;
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        if (r == j) vec[j] = y / M[tri(j, j)];
        __syncthreads();
        if (r < j) y -= M[tri(j, r)] * vec[j];
    }
    const double out = r < n ? vec[r] : 0.0;
    __syncthreads();
    return out;
}

// Band storage of M and its factor L: row r keeps columns r - N .. r, N + 1 doubles at pitch cs + 1,
// column c at offset c - (r - N): entry (r, c) at r cs + N + c. cs is the distance between the rows of
// one column, which is what the lanes of a wave stride by: N in the workspace slab (rows packed,
// n (N + 1) doubles), N | 1 in LDS (odd, so an even N does not fold a column onto a few banks; one
// pad double per row then). Rows r < N leave their first N - r slots unused. bnd(r, 0) is the row's
// base for indexing by column.
__device__ __forceinline__ size_t bnd(int r, int c, int N, int cs) { return (size_t)r * cs + (size_t)(N + c); }

// chol_solve on the band factor: row r reads L[r, r - N .. r - 1] going forward and L[r + 1 .. r + N, r]
// going back; the entries it skips are the zeros the dense form multiplies by.
__device__ double chol_solve_band(const double* M, int n, int N, int bcs, double b, double* vec) {
    const int r = threadIdx.x;
    double x = b;
    for (int j = 0; j < n; ++j) {
        if (r == j) vec[j] = x / M[bnd(j, j, N, bcs)];
        __syncthreads();
        if (r > j && r < n && r <= j + N) x -= M[bnd(r, j, N, bcs)] * vec[j];
    }
    double y = r < n ? vec[r] : 0.0;
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        if (r == j) vec[j] = y / M[bnd(j, j, N, bcs)];
        __syncthreads();
        if (r < j && r >= j - N) y -= M[bnd(j, r, N, bcs)] * vec[j];
    }
    const double out = r < n ? vec[r] : 0.0;
    __syncthreads();
    return out;
}

// CAP kernels: feasibility of period 0 and the start point; returns the iteration bound. p is w_prev clipped
// to the bounds, out = ||p - w_prev||_1 and d0 = out + |1 - 1'p| the L1 distance from w_prev to the
// feasible set: d0 > tau has no feasible point (-1: infeasible), and a tau outside the program (not
// finite, not > 0: only the sweep can carry one) runs no iteration (0: solver error). Else the plain
// start w (on entry) is pulled towards p, w = p + theta (w - p) with
// theta = min(1, 0.5 (tau - out) / ||w - p||_1), so that ||w - w_prev||_1 <= out + 0.5 (tau - out) < tau.
template <bool BOX>
__device__ __forceinline__ int capped_start(const MvArgs& a, double wpi, bool act, int k, double* red, double& w) {
    const int N = a.N;
    const double tau = a.max_turnover;
    double p = a.allow_short ? wpi : fmax(wpi, 0.0);
    if constexpr (BOX) p = fmin(p, a.max_weight);
    const double out = block_sum(k < N ? fabs(p - wpi) : 0.0, red);
    const double d0 = out + fabs(1.0 - block_sum(k < N ? p : 0.0, red));
    const double dist = block_sum(k < N ? fabs(w - p) : 0.0, red);
    const double theta = dist > 0.0 ? fmin(1.0, 0.5 * (tau - out) / dist) : 1.0;
    if (act) w = p + theta * (w - p);
    if (!(tau > 0.0) || !isfinite(tau)) return 0;
    return d0 > tau ? -1 : a.max_iter;
}

// One window. GM: M and Y in the block's workspace slab (else in LDS after the small arrays).
// BOX: the position limit w <= u (long-only callers), one more barrier on w treated as w >= 0 is:
// slack x5 = u - w taken from the iterate (no slack variable), multiplier l5 in a register.
// CAP: the turnover cap, one more inequality per period on the s rows (present at c = 0 too):
// slack x6_t = tau - sum_i s_t,i kept as a variable (as z2, z3), multiplier l6_t, both in LDS (lane
// t < H works on period t's). Eliminating s leaves (al + be) ds + (be - al) dd + dl6_t = qs, so dl6
// enters the w equation through C' = -D' diag(g), g = (be - al) P (one column per period), and the
// cap row reads C dw - kap dl6 = r3 with kap_t = x6_t / l6_t + sum_i P_t,i and
// r3_t = -sum_i P qs + rg6_t + rc6_t / l6_t:
//   M dw + A' dnu + C' dl6 = r,  A dw = r2,  C dw - kap dl6 = r3
// M and its Cholesky are the same; Y grows to [A' C'] (2H columns) and the Schur system to the SPD
// 2H x 2H matrix [A; C] M^{-1} [A' C'] + diag(0, kap) (dnu then holds [dnu; dl6]). Period 0 is
// feasible iff d0 <= tau, d0 the L1 distance from w_prev to the budget plane within the bounds
// (later periods can always hold): d0 > tau is KMPC_STATUS_INFEASIBLE before any iteration.
// The statements the CAP = false forms run are left word for word as they were and the CAP form
// overrides them under if constexpr (the start's s, z2, z3; the loop bound): even a local for 1 / N
// changed which of two products the compiler fuses there, and with it the uncapped results' last bits.
// BAND: M and L in the band layout (bnd), n (N + 1) doubles; the assembly of M, the factorization and
// chol_solve clipped to the band; mu read from a.muf (float32). Orthogonal to BOX (M's diagonal only)
// and CAP (columns of Y, rows of the Schur system). The BAND = false forms keep their statements, as
// above; the factorization's skipped terms are exact zeros there, so on the same mu the band form
// repeats the dense form's arithmetic.
template <bool GM, bool BOX, bool CAP, bool BAND = false>
__device__ __forceinline__ void mv_window(const MvArgs& a, int b, double* lds) {
    const int N = a.N, H = a.H, n = N * H;
    constexpr int SH = CAP ? 2 : 1, XH = CAP ? 13 : 4;   // Schur rows per period; H-vectors after Sm
    const int H2 = SH * H;
    double* vec = lds;                      // [n] broadcast vector
    double* Sm = vec + n;                   // [H2][H2] the Schur complement, then its Cholesky factor
    double* idg = Sm + H2 * H2 + XH * H + 18;  // [n] 1 / L_jj of the Cholesky factor
    double* M = GM ? a.ws + (size_t)blockIdx.x * a.slab : idg + n;   // packed lower: M, then L
    const int bcs = GM ? N : (N | 1);       // BAND: the rows of a column are bcs doubles apart (bnd)
    double* Y = M + (BAND ? (size_t)n * (bcs + 1) : tri(n, 0));   // [H2][n] M^{-1} A' (CAP: M^{-1} [A' C'])
    double* pv = Sm + H2 * H2;              // [H] period sums (after Sm in LDS, both variants)
    double* nu = pv + H;                    // [H] budget multipliers
    double* dnu = nu + H;                   // [H2] (CAP: dl6 after dnu)
    double* rpv = dnu + H2;                 // [H] primal residuals 1'w_t - 1
    double* red = rpv + H;                  // [16] reduction slots (one per wave)
    int* flag = (int*)(red + 16);
    // CAP only, [H] each after the flag's slot: the cap rows' slack, multiplier, complementarity
    // target, residual, slack step, kap, a second set of period sums, the Schur right-hand side
    double* x6 = red + 18;
    double* l6 = x6 + H;
    double* rc6 = l6 + H;
    double* rg6 = rc6 + H;
    double* dx6 = rg6 + H;
    double* kap = dx6 + H;
    double* pc = kap + H;
    double* cx = pc + H;

    const int k = threadIdx.x;
    const bool act = k < n;
    const int t = act ? k / N : 0, i = act ? k - (k / N) * N : 0;
    const double* Sig = a.sigma + a.sigma_stride * (size_t)b;
    const double* wpv = a.wp + (size_t)b * N;
    const double* muv = a.mu + (size_t)b * n;
    const bool hw = !a.allow_short, hs = a.c > 0.0 || CAP;
    const double wpi = act ? wpv[i] : 0.0;
    double mk_;
    if constexpr (BAND) mk_ = act ? (double)a.muf[(size_t)b * n + k] : 0.0;   // (float32 -> float64: exact)
    else mk_ = act ? muv[k] : 0.0;
    const double mk = mk_;
    double* wout = a.wout + (size_t)b * (a.return_full ? n : N);
    const int nout = a.return_full ? n : N;

    // scale and finiteness
    double smax = 0.0;
    bool finite = isfinite(mk) && isfinite(wpi);
    for (int j = k; j < N * N; j += blockDim.x) {
        const double v = Sig[j];
        finite = finite && isfinite(v);
        smax = fmax(smax, fabs(v));
    }
    const double nonfinite = block_max(finite ? 0.0 : 1.0, red);
    double sc = block_max(fmax(fabs(mk), 2.0 * a.gamma * smax), red);
    sc = fmax(sc, a.c);
    if (!(sc > 0.0) || !isfinite(sc)) sc = 1.0;
    const double g2 = 2.0 * a.gamma / sc, cs = a.c / sc, mus = mk / sc;

    int status = KMPC_STATUS_SOLVER_ERROR, it = 0;
    double best = 1e300, best_obj = __builtin_nan("");
    bool unbounded = false;

    if (nonfinite == 0.0 && isfinite(a.gamma) && isfinite(a.c) && !hw && !hs && !(a.gamma > 0.0)) {
        // no bounds, no cost, no curvature: a linear program over the budget planes, unbounded
        // unless every period's returns are flat (then any budget point is optimal: w_prev scaled)
        period_sums(mk, vec, pv, k, n, N, H);
        const double spread = block_max(act ? fabs(mk - pv[t] / N) : 0.0, red);
        if (spread == 0.0) {
            const double swp = block_sum(k < N ? wpi : 0.0, red);
            const double w = swp != 0.0 ? wpi / swp : 1.0 / N;
            best_obj = block_sum(act ? mk * w : 0.0, red);
            if (act && k < nout) wout[k] = w;
            status = KMPC_STATUS_OPTIMAL;
        } else {
            status = KMPC_STATUS_UNBOUNDED;
        }
    } else if (nonfinite == 0.0 && isfinite(a.gamma) && isfinite(a.c)) {
        double w = act ? 0.5 * (hw ? fmax(wpi, 0.0) : wpi) + 0.5 / N : 0.0;
        if constexpr (BOX) w = fmin(w, 0.5 * (a.max_weight + 1.0 / N));   // strictly inside: 1 / N < u
        int cap_iter = 0;   // CAP: the iteration bound of capped_start
        double sfl = 0.0;   // CAP: s above |d| at the start
        if constexpr (CAP) {
            // s_t,i = |d_t,i| + half of what the start leaves of tau, shared equally: sum_i s_t,i < tau
            cap_iter = capped_start<BOX>(a, wpi, act, k, red, w);
            const double D0 = block_sum(k < N ? fabs(w - wpi) : 0.0, red);
            sfl = 0.5 * (a.max_turnover - D0) / N;
        }
        double wm = prev_period(w, vec, k, n, N, wpi);
        double s = (act && hs) ? fabs(w - wm) + 1.0 / N : 0.0;
        // slacks of the two |d| rows kept as variables (no cancellation in s -+ d near the optimum)
        double z2 = (act && hs) ? fmax(s - (w - wm), 1e-2) : 1.0, z3 = (act && hs) ? fmax(s + (w - wm), 1e-2) : 1.0;
        if constexpr (CAP) {   // ... and the slacks' floor scaled to a small tau
            const double zlo = 1e-2 * fmin(1.0, a.max_turnover);
            s = act ? fabs(w - wm) + sfl : 0.0;
            z2 = act ? fmax(s - (w - wm), zlo) : 1.0;
            z3 = act ? fmax(s + (w - wm), zlo) : 1.0;
            period_sums(s, vec, pv, k, n, N, H);
            if (k < H) { x6[k] = fmax(a.max_turnover - pv[k], zlo); l6[k] = 1.0; }
        }
        double l1 = (act && hw) ? 1.0 : 0.0, l2 = (act && hs) ? 1.0 : 0.0, l3 = l2;
        double l5 = 0.0, x5 = 1.0;   // BOX only (l5 stays 0 on the inactive lanes)
        if constexpr (BOX) l5 = act ? 1.0 : 0.0;
        if (k < H) nu[k] = 0.0;
        const int mcon = (hw ? n : 0) + (hs ? 2 * n : 0) + (BOX ? n : 0) + (CAP ? H : 0);
        const double inv_m = 1.0 / (mcon > 0 ? mcon : 1);

        for (it = 0; it < a.max_iter; ++it) {
            if constexpr (CAP) {
                if (it >= cap_iter) break;   // (no iteration where the window is infeasible or tau outside the program)
            }
            // ---- residuals ----
            wm = prev_period(w, vec, k, n, N, wpi);   // vec holds w afterwards
            double Sw = 0.0;
            if (act)
            {   // Sigma w per element: column i (= row i, symmetric: coalesced across the block),
                // four partial sums so the L2 loads of a group are in flight together
                double s4[4] = {0.0, 0.0, 0.0, 0.0};
                int j = 0;
                for (; j + 4 <= N; j += 4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) s4[e] += Sig[(size_t)(j + e) * N + i] * vec[t * N + j + e];
                }
                for (; j < N; ++j) s4[0] += Sig[(size_t)j * N + i] * vec[t * N + j];
                Sw = (s4[0] + s4[1]) + (s4[2] + s4[3]);
            }
            const double d = w - wm;
            const double rg2 = (act && hs) ? (s - d) - z2 : 0.0, rg3 = (act && hs) ? (s + d) - z3 : 0.0;
            const double eta = l2 - l3;
            const double etan = next_period(eta, vec, k, n, N);
            if constexpr (CAP) {
                period_sums(s, vec, pv, k, n, N, H);
                if (k < H) rg6[k] = (a.max_turnover - pv[k]) - x6[k];
            }
            period_sums(w, vec, pv, k, n, N, H);
            if (k < H) rpv[k] = pv[k] - 1.0;
            double prmax = 0.0;
            for (int q = 0; q < H; ++q) prmax = fmax(prmax, fabs(pv[q] - 1.0));
            double rw = act ? -mus + g2 * Sw - l1 + eta - etan + nu[t] : 0.0;
            double rs = (act && hs) ? cs - l2 - l3 : 0.0;
            double comp = act ? w * l1 + z2 * l2 + z3 * l3 : 0.0;
            double r6 = 0.0;   // CAP: |rg6| of the lane's period
            if constexpr (CAP) {
                if (act) rs += l6[t];
                if (k < H) { comp += x6[k] * l6[k]; r6 = fabs(rg6[k]); }
            }
            if constexpr (BOX) {
                x5 = a.max_weight - w;
                rw += l5;
                comp += x5 * l5;
            }
            const double mu_c = block_sum(comp, red) * inv_m;
            double rdl = fmax(fmax(fabs(rw), fabs(rs)), fmax(fabs(rg2), fabs(rg3)));
            if constexpr (CAP) rdl = fmax(rdl, r6);
            const double rd = block_max(rdl, red);
            const double wabs = block_max(act ? fabs(w) : 0.0, red);
            const double merit = fmax(mu_c, fmax(rd, prmax));
            if (!isfinite(merit)) break;
            if (wabs > 1e7) { unbounded = true; break; }
            if (merit < best) {
                best = merit;
                // problem.value (mpc.py:172) in the reference's maximize form, unscaled
                const double f = block_sum(act ? mk * w - a.gamma * w * Sw - a.c * fabs(d) : 0.0, red);
                best_obj = f;
                if (act && k < nout) wout[k] = w;
            }
            if (mu_c < a.tol && rd < 10.0 * a.tol && prmax < 10.0 * a.tol) break;

            // ---- factor: M = 2 gamma (I (x) Sigma) + diag(W1) + D' diag(E) D ----
            double W1 = (act && hw) ? l1 / w : 0.0;
            if constexpr (BOX) W1 += l5 / x5;
            const double al = (act && hs) ? l2 / z2 : 0.0, be = (act && hs) ? l3 / z3 : 0.0;
            const double P = (act && hs) ? 1.0 / (al + be) : 0.0;
            const double E = 4.0 * al * be * P;
            const double En = next_period(E, vec, k, n, N);
            if constexpr (BAND) {
                if (act) {   // column k, rows k .. k + N (the band's)
                    const int le = k + N < n - 1 ? k + N : n - 1;
                    for (int l = k; l <= le; ++l) {
                        const int tl = l / N, j = l - tl * N;
                        double v = (tl == t) ? g2 * Sig[(size_t)j * N + i] : 0.0;
                        if (l == k) v += W1 + E + En;
                        if (l == k + N) v -= En;
                        M[bnd(l, k, N, bcs)] = v;
                    }
                }
            } else
            if (act) {   // column k, rows l >= k (M symmetric): lanes write consecutive entries
                for (int l = k; l < n; ++l) {
                    const int tl = l / N, j = l - tl * N;
                    double v = (tl == t) ? g2 * Sig[(size_t)j * N + i] : 0.0;
                    if (l == k) v += W1 + E + En;
                    if (l == k + N) v -= En;
                    M[tri(l, k)] = v;
                }
            }
            if (k == 0) *flag = 0;
            __syncthreads();
            // right-looking Cholesky in panels of PB columns (thread k owns row k): inside a panel
            // column by column (pivot, scale, update of the panel's remaining columns); then the
            // trailing matrix at once, M[k][c] -= L[k][panel] . L[c][panel] with row k's panel in
            // registers — one read-modify-write per entry per panel instead of per column
            constexpr int PB = 8;
            if constexpr (BAND) {
                // the same, clipped to the band: column j reaches rows j + 1 .. j + N, row k's update
                // columns >= k - N; a panel's trailing update the N rows under it
                for (int jb = 0; jb < n; jb += PB) {
                    const int je = jb + PB < n ? jb + PB : n;
                    for (int j = jb; j < je; ++j) {
                        if (k == j) {
                            const double dj = M[bnd(j, j, N, bcs)];
                            if (!(dj > 0.0) || !(dj < 1e300)) *flag = 1;
                            const double lj = sqrt(fmax(dj, 1e-300));
                            M[bnd(j, j, N, bcs)] = lj;
                            idg[j] = 1.0 / lj;
                        }
                        __syncthreads();
                        const bool below = k > j && k < n && k <= j + N;   // (one value for both halves)
                        if (below) M[bnd(k, j, N, bcs)] *= idg[j];
                        __syncthreads();   // column j of L complete before any row reads it
                        if (below) {
                            double* mr = M + bnd(k, 0, N, bcs);
                            const double lkj = mr[j];
                            int qe = k < je - 1 ? k : je - 1;   // the panel's columns in row k ...
                            if (qe > j + N) qe = j + N;         // ... whose rows column j reaches
                            for (int q = j + 1; q <= qe; ++q) mr[q] = fma(-lkj, M[bnd(q, j, N, bcs)], mr[q]);
                        }
                    }
                    __syncthreads();
                    if (k >= je && k < n && k - N < je) {
                        double* mr = M + bnd(k, 0, N, bcs);
                        double lk[PB];
#pragma unroll
                        for (int p = 0; p < PB; ++p) lk[p] = (jb + p < je && jb + p >= k - N) ? mr[jb + p] : 0.0;
                        for (int c = je; c <= k; ++c) {
                            const double* mc = M + bnd(c, jb, N, bcs);
                            double lc[PB];
#pragma unroll
                            for (int p = 0; p < PB; ++p) lc[p] = (jb + p < je && jb + p >= c - N) ? mc[p] : 0.0;
                            double v = mr[c];
#pragma unroll
                            for (int p = 0; p < PB; ++p) v = fma(-lk[p], lc[p], v);
                            mr[c] = v;
                        }
                    }
                    __syncthreads();
                }
            } else
            for (int jb = 0; jb < n; jb += PB) {
                const int je = jb + PB < n ? jb + PB : n;
                for (int j = jb; j < je; ++j) {
                    if (k == j) {
                        const double dj = M[tri(j, j)];
                        if (!(dj > 0.0) || !(dj < 1e300)) *flag = 1;
                        const double lj = sqrt(fmax(dj, 1e-300));
                        M[tri(j, j)] = lj;
                        idg[j] = 1.0 / lj;
                    }
                    __syncthreads();
                    if (k > j && k < n) M[tri(k, j)] *= idg[j];
                    __syncthreads();   // column j of L complete before any row reads it
                    if (k > j && k < n) {
                        double* mr = M + tri(k, 0);
                        const double lkj = mr[j];
                        const int qe = k < je - 1 ? k : je - 1;   // the panel's columns in row k
                        for (int q = j + 1; q <= qe; ++q) mr[q] = fma(-lkj, M[tri(q, j)], mr[q]);
                    }
                }
                __syncthreads();
                if (k >= je && k < n) {
                    double* mr = M + tri(k, 0);
                    double lk[PB];
#pragma unroll
                    for (int p = 0; p < PB; ++p) lk[p] = jb + p < je ? mr[jb + p] : 0.0;
                    for (int c = je; c <= k; ++c) {
                        const double* mc = M + tri(c, jb);
                        double lc[PB];
#pragma unroll
                        for (int p = 0; p < PB; ++p) lc[p] = jb + p < je ? mc[p] : 0.0;
                        double v = mr[c];
#pragma unroll
                        for (int p = 0; p < PB; ++p) v = fma(-lk[p], lc[p], v);
                        mr[c] = v;
                    }
                }
                __syncthreads();
            }
            __syncthreads();
            if (*flag) break;
            // Y = M^{-1} A' (one column per period) and S = A Y; CAP: Y = M^{-1} [A' C'] and
            // S = [A; C] Y + diag(0, kap), with (C y)_t = -sum_i g (y_t - y_{t-1})
            double g = 0.0, gn = 0.0;
            if constexpr (CAP) {
                g = (be - al) * P;
                gn = next_period(g, vec, k, n, N);
                period_sums(P, vec, pv, k, n, N, H);
                if (k < H) kap[k] = x6[k] / l6[k] + pv[k];
            }
            for (int q = 0; q < H2; ++q) {
                double bq = (act && t == q) ? 1.0 : 0.0;
                if constexpr (CAP) {
                    if (q >= H) bq = act ? (t + 1 == q - H ? gn : 0.0) - (t == q - H ? g : 0.0) : 0.0;
                }
                double yq;
                if constexpr (BAND) yq = chol_solve_band(M, n, N, bcs, bq, vec);
                else yq = chol_solve(M, n, bq, vec);
                if (act) Y[(size_t)q * n + k] = yq;
                period_sums(yq, vec, pv, k, n, N, H);
                if (k < H) Sm[k * H2 + q] = pv[k];
                __syncthreads();
                if constexpr (CAP) {
                    const double ym = prev_period(yq, vec, k, n, N, 0.0);
                    period_sums(act ? -g * (yq - ym) : 0.0, vec, pv, k, n, N, H);
                    if (k < H) Sm[(H + k) * H2 + q] = pv[k] + (q == H + k ? kap[k] : 0.0);
                    __syncthreads();
                }
            }
            if (k == 0) {   // Cholesky of the H2 x H2 Schur complement
                for (int j = 0; j < H2; ++j) {
                    double dj = Sm[j * H2 + j];
                    for (int q = 0; q < j; ++q) dj -= Sm[j * H2 + q] * Sm[j * H2 + q];
                    if (!(dj > 0.0) || !isfinite(dj)) *flag = 1;
                    dj = sqrt(fmax(dj, 1e-300));
                    Sm[j * H2 + j] = dj;
                    for (int r = j + 1; r < H2; ++r) {
                        double v = Sm[r * H2 + j];
                        for (int q = 0; q < j; ++q) v -= Sm[r * H2 + q] * Sm[j * H2 + q];
                        Sm[r * H2 + j] = v / dj;
                    }
                }
            }
            __syncthreads();
            if (*flag) break;

            // ---- predictor (pass 0) / corrector (pass 1) ----
            double rc1 = (act && hw) ? w * l1 : 0.0, rc2 = (act && hs) ? z2 * l2 : 0.0;
            double rc3 = (act && hs) ? z3 * l3 : 0.0;
            double dw = 0.0, ds = 0.0, dl1 = 0.0, dl2 = 0.0, dl3 = 0.0, step = 0.0, prev_dw = 0.0;
            double rc5 = 0.0, dl5 = 0.0;
            if constexpr (BOX) rc5 = x5 * l5;
            if constexpr (CAP) {
                if (k < H) rc6[k] = x6[k] * l6[k];
            }
            for (int pass = 0; pass < 2; ++pass) {
                const double p2 = rc2 / z2 + al * rg2, p3 = rc3 / z3 + be * rg3;
                const double qs = (act && hs) ? -rs - p2 - p3 : 0.0;
                const double v = (act && hs) ? (be - al) * P * qs + p3 - p2 : 0.0;
                const double vn = next_period(v, vec, k, n, N);
                double rhs = act ? -rw - (hw ? rc1 / w : 0.0) - (v - vn) : 0.0;
                if constexpr (BOX) rhs += rc5 / x5;
                double r3 = 0.0;   // CAP: the cap row's right-hand side of the lane's period
                if constexpr (CAP) {
                    period_sums(P * qs, vec, pv, k, n, N, H);
                    if (k < H) r3 = -pv[k] + rg6[k] + rc6[k] / l6[k];
                }
                double x;
                if constexpr (BAND) x = chol_solve_band(M, n, N, bcs, rhs, vec);
                else x = chol_solve(M, n, rhs, vec);
                if constexpr (CAP) {
                    const double xm = prev_period(x, vec, k, n, N, 0.0);
                    period_sums(act ? -g * (x - xm) : 0.0, vec, pc, k, n, N, H);
                    if (k < H) cx[k] = pc[k] - r3;
                }
                period_sums(x, vec, pv, k, n, N, H);
                if (k == 0) {   // dnu = S^{-1} (A x + r_p); CAP: [dnu; dl6] = S^{-1} [A x + r_p; C x - r3]
                    for (int j = 0; j < H2; ++j) {
                        double u = (!CAP || j < H) ? pv[j] + rpv[j] : cx[j - H];
                        for (int q = 0; q < j; ++q) u -= Sm[j * H2 + q] * dnu[q];
                        dnu[j] = u / Sm[j * H2 + j];
                    }
                    for (int j = H2 - 1; j >= 0; --j) {
                        double u = dnu[j];
                        for (int q = j + 1; q < H2; ++q) u -= Sm[q * H2 + j] * dnu[q];
                        dnu[j] = u / Sm[j * H2 + j];
                    }
                }
                __syncthreads();
                dw = x;
                if (act)
                    for (int q = 0; q < H2; ++q) dw -= Y[(size_t)q * n + k] * dnu[q];
                const double dwm = prev_period(dw, vec, k, n, N, 0.0);
                prev_dw = dwm;
                const double dd = dw - dwm;
                ds = (act && hs) ? P * (qs - (be - al) * dd) : 0.0;
                if constexpr (CAP) {
                    if (act) ds -= P * dnu[H + t];
                    period_sums(ds, vec, pv, k, n, N, H);
                    if (k < H) dx6[k] = -pv[k] + rg6[k];
                }
                const double dz2 = ds - dd + rg2, dz3 = ds + dd + rg3;
                dl1 = (act && hw) ? -(l1 * dw + rc1) / w : 0.0;
                dl2 = (act && hs) ? -(l2 * dz2 + rc2) / z2 : 0.0;
                dl3 = (act && hs) ? -(l3 * dz3 + rc3) / z3 : 0.0;
                if constexpr (BOX) dl5 = (-rc5 + l5 * dw) / x5;
                double am = 1e300;
                if (act && hw) { am = to_bound(w, dw, am); am = to_bound(l1, dl1, am); }
                if (act && hs) {
                    am = to_bound(z2, dz2, am); am = to_bound(z3, dz3, am);
                    am = to_bound(l2, dl2, am); am = to_bound(l3, dl3, am);
                }
                if constexpr (BOX) {
                    if (act) { am = to_bound(x5, -dw, am); am = to_bound(l5, dl5, am); }
                }
                if constexpr (CAP) {
                    if (k < H) { am = to_bound(x6[k], dx6[k], am); am = to_bound(l6[k], dnu[H + k], am); }
                }
                am = block_min(am, red);
                if (pass == 1) { step = fmin(1.0, 0.99 * am); break; }
                const double ap = fmin(1.0, am);
                double compa = act ? (w + ap * dw) * (l1 + ap * dl1) + (z2 + ap * dz2) * (l2 + ap * dl2) +
                                         (z3 + ap * dz3) * (l3 + ap * dl3) : 0.0;
                if constexpr (BOX) compa += (x5 - ap * dw) * (l5 + ap * dl5);
                if constexpr (CAP) {
                    if (k < H) compa += (x6[k] + ap * dx6[k]) * (l6[k] + ap * dnu[H + k]);
                }
                const double mua = block_sum(compa, red) * inv_m;
                double sg = mua / mu_c;
                sg = sg * sg * sg;
                const double smu = sg * mu_c;
                if (act && hw) rc1 = w * l1 + dw * dl1 - smu;
                if (act && hs) { rc2 = z2 * l2 + dz2 * dl2 - smu; rc3 = z3 * l3 + dz3 * dl3 - smu; }
                if constexpr (BOX) {
                    if (act) rc5 = x5 * l5 - dw * dl5 - smu;
                }
                if constexpr (CAP) {
                    if (k < H) rc6[k] = x6[k] * l6[k] + dx6[k] * dnu[H + k] - smu;
                }
            }
            w += step * dw;
            s += step * ds;
            if (act && hs) {
                z2 += step * (ds - (dw - prev_dw) + rg2);
                z3 += step * (ds + (dw - prev_dw) + rg3);
            }
            l1 += step * dl1;
            l2 += step * dl2;
            l3 += step * dl3;
            if constexpr (BOX) l5 += step * dl5;
            __syncthreads();
            if (k < H) nu[k] += step * dnu[k];
            if constexpr (CAP) {
                if (k < H) { x6[k] += step * dx6[k]; l6[k] += step * dnu[H + k]; }
            }
            __syncthreads();
        }
        if (unbounded) status = KMPC_STATUS_UNBOUNDED;
        else if (best <= 1e-7) status = KMPC_STATUS_OPTIMAL;
        else if (best <= 1e-4) status = KMPC_STATUS_OPTIMAL_INACCURATE;
        else status = KMPC_STATUS_SOLVER_ERROR;
        if constexpr (CAP) {
            if (cap_iter < 0) status = KMPC_STATUS_INFEASIBLE;   // d0 > tau (capped_start)
        }
    }
    __syncthreads();
    const bool ok = status == KMPC_STATUS_OPTIMAL || status == KMPC_STATUS_OPTIMAL_INACCURATE;
    if (!ok && k < nout) wout[k] = wpv[k % N];   // tile(current_weights), mpc.py:180-181
    if (k == 0) {
        a.obj[b] = ok ? best_obj : __builtin_nan("");
        a.status[b] = status;
        if (a.iters) a.iters[b] = it;
    }
}

template <int MAXT, bool GM, bool BOX, bool CAP>
__global__ void __launch_bounds__(MAXT) mv_ipm_kernel(MvArgs a) {
    extern __shared__ double lds[];
    if (GM) {
        for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
            mv_window<true, BOX, CAP>(a, b, lds);
            __syncthreads();
        }
    } else {
        mv_window<false, BOX, CAP>(a, blockIdx.x, lds);
    }
}

// The Markowitz backtest (kmpc_markowitz_run / kmpc_markowitz_sweep; run_backtest with a
// MarkowitzStrategy, backtest.py:133-219 and baselines.py:48-106, for P independent paths): one
// workgroup per work item runs every step of its path back to back — the step's window
// (mv_window, or the hold of baselines.py:76-78 where the step has fewer than 5 past rows) then the
// step's bookkeeping (kmpc_bt_step.h, as kmpc_backtest_step) — as bt_kernel (kmpc_bt_run.h) does for
// the log-utility rows. Work item q = j P + p (config j, path p; j = 0 in the run form): its state
// rows are q's, the step's moments and realized row are read at the path p (shared by the configs).
struct MvBt {
    int P;                    // paths
    int items;                // work items: P, or configs x P
    int n_steps;              // steps run by this launch
    int n_real;               // steps k < n_real have a realized row (later ones: no market move)
    int nbt;                  // threads of the bookkeeping: bt_step_kernel's block size for this N
    union {                   // (one slot, as MvArgs')
        const double* mu;     // [n_steps, P, H, N]
        const float* muf;     // BAND kernels: [n_steps, P, H, N] float32 forecasts, read in place of mu
    };
    const double* sigma;      // [n_steps, P, N, N]
    const int* valid;         // [n_steps, P]
    const float* realized;    // [n_steps, P, N] log-returns of each step's t + 1
    const double* gamma;      // SWEEP: [C] device, the solve's gamma
    const double* mv_cost;    // SWEEP: [C] device, the solve's cost_coeff
    const double* bt_cost;    // SWEEP: [C] device, the bookkeeping's cost_coeff
    const double* max_turnover;   // SWEEP of the CAP kernels: [C] device, the solve's turnover cap
    bt::StepArgs st;          // st.k = the first step's history row; st.target = the W0 rows [items, N]
    const double* max_weight; // SWEEP of the BAND BOX kernels: [C] device, the solve's position limit (null: a0's).
                              // After st: every field above keeps its offset
};

// a0: the solve's program; a0.wp = the weights [items, N] (each step's w_prev: the item's current,
// drifted weights), a0.wout = r.st.target, a0.status / a0.obj [items]. Every window is solved as
// window 0 of a per-item copy whose pointers are the item's rows. A held step reports status
// optimal and obj NaN. SWEEP: a config outside the program (gamma < 0, cost_coeff < 0 or a
// non-finite value; the host cannot see the values) gets a NaN parameter, which mv_window answers
// with KMPC_STATUS_SOLVER_ERROR and the hold fallback at every step; so does a cap that is not
// finite or not > 0 (CAP kernels), and a per-config limit outside 1 / N < u < 1 (band BOX sweep).
template <bool GM, bool BOX, bool CAP, bool SWEEP, bool BAND = false>
__device__ __forceinline__ void mv_bt_item(const MvArgs& a0, const MvBt& r, int q, double* lds, double* red) {
    const int N = a0.N, n = a0.N * a0.H;
    int p = q;
    double gj = a0.gamma, cj = a0.c, cb = r.st.c;
    if constexpr (SWEEP) {
        const int j = q / r.P;
        p = q - j * r.P;
        gj = r.gamma[j], cj = r.mv_cost[j];
        if (!(gj >= 0.0) || !isfinite(gj)) gj = __builtin_nan("");
        if (!(cj >= 0.0) || !isfinite(cj)) cj = __builtin_nan("");
        cb = r.bt_cost[j];
    }
    double tj = a0.max_turnover;
    if constexpr (SWEEP && CAP) tj = r.max_turnover[q / r.P];
    // The config's own position limit (the band sweep alone: the dense sweeps have one limit per launch
    // and keep their instruction streams). mv_window's start assumes 1 / N < u < 1: a limit outside
    // that, or a non-finite one, never reaches it: the config's gamma becomes NaN, as a bad gamma[j].
    double uj = a0.max_weight;
    if constexpr (SWEEP && BOX && BAND) {
        if (r.max_weight) {
            const double v = r.max_weight[q / r.P];
            if (isfinite(v) && v < 1.0 && N * v > 1.0) uj = v;
            else gj = __builtin_nan("");
        }
    }
    const size_t PN = (size_t)r.P * N;
    for (int k = 0; k < r.n_steps; ++k) {
        const size_t kp = (size_t)k * r.P + p;
        if (r.valid[kp]) {   // (one value per workgroup: mv_window's barriers stay uniform)
            MvArgs a = a0;
            a.gamma = gj; a.c = cj;
            if constexpr (CAP) a.max_turnover = tj;
            if constexpr (SWEEP && BOX && BAND) a.max_weight = uj;
            a.return_full = 0;
            if constexpr (BAND) a.muf = r.muf + kp * n;   // (the forecasts: float32, a0.mu unused)
            else a.mu = r.mu + kp * n;
            a.sigma = r.sigma + kp * N * N;
            a.wp = a0.wp + (size_t)q * N;
            a.wout = a0.wout + (size_t)q * N;
            a.status = a0.status + q;
            a.obj = a0.obj + q;
            a.iters = nullptr;
            mv_window<GM, BOX, CAP, BAND>(a, 0, lds);
        } else {
            for (int i = threadIdx.x; i < N; i += blockDim.x) a0.wout[(size_t)q * N + i] = a0.wp[(size_t)q * N + i];
            if (threadIdx.x == 0) {
                a0.status[q] = KMPC_STATUS_OPTIMAL;
                a0.obj[q] = __builtin_nan("");
            }
        }
        __syncthreads();   // W0 (st.target) of every thread, and the solve's LDS, done
        bt::StepArgs st = r.st;
        st.k = r.st.k + k;
        st.c = cb;
        st.realized = k < r.n_real ? r.realized + k * PN : nullptr;
        bt::bt_step_body(st, q, p, red, r.nbt);
        __syncthreads();   // the drifted weights are the next solve's w_prev
    }
}

template <int MAXT, bool GM, bool BOX, bool CAP, bool SWEEP>
__global__ void __launch_bounds__(MAXT) mv_bt_kernel(MvArgs a0, MvBt r) {
    extern __shared__ double lds[];
    __shared__ double red[4];   // the bookkeeping's reduction slots (nbt <= 256: four waves)
    if (GM) {
        for (int q = blockIdx.x; q < r.items; q += gridDim.x) mv_bt_item<true, BOX, CAP, SWEEP>(a0, r, q, lds, red);
    } else {
        mv_bt_item<false, BOX, CAP, SWEEP>(a0, r, blockIdx.x, lds, red);
    }
}

// The band forms (kmpc_solve_mv_band; kmpc_koopman_mv_run and, with SWEEP, kmpc_koopman_mv_sweep): the
// same window body and the same item loop with BAND set, under kernel names of their own so that the dense
// instantiations above keep their symbols. MAXT: 256 for the LDS variant (n <= 256 there), else 1024.
template <int MAXT, bool GM, bool BOX, bool CAP>
__global__ void __launch_bounds__(MAXT) mv_band_ipm_kernel(MvArgs a) {
    extern __shared__ double lds[];
    if (GM) {
        for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
            mv_window<true, BOX, CAP, true>(a, b, lds);
            __syncthreads();
        }
    } else {
        mv_window<false, BOX, CAP, true>(a, blockIdx.x, lds);
    }
}

template <int MAXT, bool GM, bool BOX, bool CAP, bool SWEEP>
__global__ void __launch_bounds__(MAXT) mv_band_bt_kernel(MvArgs a0, MvBt r) {
    extern __shared__ double lds[];
    __shared__ double red[4];   // the bookkeeping's reduction slots (nbt <= 256: four waves)
    if (GM) {
        for (int q = blockIdx.x; q < r.items; q += gridDim.x) mv_bt_item<true, BOX, CAP, SWEEP, true>(a0, r, q, lds, red);
    } else {
        mv_bt_item<false, BOX, CAP, SWEEP, true>(a0, r, blockIdx.x, lds, red);
    }
}

// Markowitz moments (baselines.py:70-88) for window b = s P + p: test index t = ts[s] of panel p of
// z [P, T, ldz] (kmpc_rolling_moments: P = 1, so b = s; kmpc_rolling_moments_paths: outputs
// [n_ts, P, ...]): r_s = z_s * std + mean (float32, data_finance.py:740-742) for the rows s of the
// last `lookback` of [0, t] of that panel; mu = mean (float32, as np.mean of the float32 history),
// Sigma = np.cov (float64, ddof 1) + 1e-6 I; valid[b] = (t + 1 >= 5) (baselines.py:76-78).
__global__ void rolling_moments_kernel(int P, int T, int N, int lookback, const float* zp, int ldz,
                                       const float* mean, const float* stdv, const int* ts,
                                       double* mu, double* sigma, int* valid) {
    extern __shared__ double ml[];   // [N] float64 means
    const int b = blockIdx.x;
    const int sb = b / P;
    const float* z = zp + (size_t)(b - sb * P) * T * ldz;
    const int t = ts[sb];
    const int hi = min(t + 1, T), lo = max(0, hi - lookback), rows = hi - lo;
    if (threadIdx.x == 0) valid[b] = (t + 1 >= 5 && t < T) ? 1 : 0;
    // z * std + mean as two float32 roundings (torch's mul then add): no FMA contraction here
    auto ret = [&](int s, int j) -> float {
#pragma clang fp contract(off)
        const float p = z[(size_t)s * ldz + j] * stdv[j];
        return p + mean[j];
    };
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        double acc = 0.0;
        for (int s = lo; s < hi; ++s) acc += (double)ret(s, j);
        const double m = rows > 0 ? acc / rows : 0.0;
        ml[j] = m;
        mu[(size_t)b * N + j] = (double)(float)m;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < N * N; q += blockDim.x) {
        const int r = q / N, c = q - r * N;
        double acc = 0.0;
        for (int s = lo; s < hi; ++s) acc += ((double)ret(s, r) - ml[r]) * ((double)ret(s, c) - ml[c]);
        double v = rows > 1 ? acc / (rows - 1) : 0.0;
        if (r == c) v += 1e-6;
        sigma[(size_t)b * N * N + q] = v;
    }
}

// The covariance estimators of kmpc_rolling_cov (Ledoit-Wolf, OAS, EWMA) for the windows of
// rolling_moments_kernel — same grid (window b = s P + p), same rows lo .. hi - 1, same valid, same
// float32 returns r = z * std + mean and the same mu (the float32-rounded plain mean) — with the Gram
// matrix on v_mfma_f64_16x16x4_f64. With x_s = r_s - mean (float64; EWMA: the omega-weighted mean):
//   Ledoit-Wolf / OAS:  G = X'X, S = G / n, m = tr(S) / p, Sigma = (1 - rho) S + (rho m + 1e-6) I with
//                       rho from tr(S), ||G||_F^2 and sum_s ||x_s||^4 (include/kmpc.h has the formulas);
//   EWMA:               Sigma = sum_s omega_s x_s x_s' + 1e-6 I, omega_s = lambda^(hi-1-s) / sum_k lambda^k.
// Passes, all over the float32 panel (nothing of the window is staged, so any lookback runs):
//   1. the means, one column per thread, into LDS;
//   2. (shrinkage only) sum_s ||x_s||^2 and sum_s ||x_s||^4, one row per wave at a time;
//   3. (shrinkage only) the Gram tiles once for ||G||_F^2 alone — rho scales every entry, and the tiles of
//      N = 1024 do not fit the registers, so they are formed again in pass 4 rather than stored raw, read
//      back and stored again (the same instructions on the same operands: the same bits as the norm saw);
//   4. the Gram tiles again, scaled and stored.
// A wave takes the 16 x 16 tiles (I <= J) of the upper block triangle round-robin and walks the window
// from its last row back in k-steps of 4 (lane l: column l & 15 of the tile, row l >> 4 of the step), so
// the EWMA weight is a running product that may underflow to 0 only where the weight is 0; each return
// is formed once per element per tile pass. Operands are 0 past the window and past column N. The A
// operand carries omega for EWMA, so (i, j) and (j, i) would round differently: only i <= j is taken from
// the accumulators and the mirror is that same value — off-diagonal tiles through a per-wave LDS
// transpose (both stores run along a row of Sigma), diagonal tiles entry by entry. Every sum has a fixed
// order (sequential, butterfly, then the waves' slots in order): the same window gives the same bits in
// any batch.
typedef double cov_d4 __attribute__((ext_vector_type(4)));
constexpr int COV_THREADS = 256, COV_WAVES = COV_THREADS / 64, COV_TLD = 17;   // (tile rows padded: 17 doubles)
constexpr int COV_KU = 4;   // k-steps (of 4 rows) per trip of the Gram loop

__host__ __device__ inline size_t cov_lds_doubles(int N) {
    return (size_t)N + (size_t)COV_WAVES * 16 * COV_TLD + 3 * COV_WAVES;
}

__global__ void __launch_bounds__(COV_THREADS)
rolling_cov_kernel(int P, int T, int N, int lookback, const float* zp, int ldz, const float* mean,
                   const float* stdv, const int* ts, double* mu, double* sigma, int* valid, int estimator,
                   double lambda, double* shrinkage) {
    extern __shared__ double cl[];
    double* ml = cl;                                  // [N] the centring means
    double* tbuf = cl + N;                            // [COV_WAVES][16][COV_TLD] the waves' transpose tiles
    double* red = tbuf + COV_WAVES * 16 * COV_TLD;    // [3][COV_WAVES] reduction slots
    const int b = blockIdx.x;
    const int sb = b / P;
    const float* z = zp + (size_t)(b - sb * P) * T * ldz;
    const int t = ts[sb];
    const int hi = min(t + 1, T), lo = max(0, hi - lookback), rows = max(hi - lo, 0);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool ew = estimator == KMPC_COV_EWMA;
    if (threadIdx.x == 0) valid[b] = (t + 1 >= 5 && t < T) ? 1 : 0;
    auto ret = [&](int s, int j) -> float {
#pragma clang fp contract(off)
        const float p = z[(size_t)s * ldz + j] * stdv[j];
        return p + mean[j];
    };
    // sum_k lambda^k over the window's rows (every thread: the same sequence, the same bits)
    double wsum = 0.0;
    if (ew) {
        double pw = 1.0;
        for (int k = 0; k < rows; ++k) { wsum += pw; pw *= lambda; }
    }
    const double winv = (ew && rows > 0) ? 1.0 / wsum : 0.0;
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        double acc = 0.0;
        for (int s = lo; s < hi; ++s) acc += (double)ret(s, j);
        const double m = rows > 0 ? acc / rows : 0.0;
        mu[(size_t)b * N + j] = (double)(float)m;
        if (ew) {
            double wa = 0.0, pw = 1.0;
            for (int s = hi - 1; s >= lo; --s) { wa += pw * (double)ret(s, j); pw *= lambda; }
            ml[j] = wa * winv;
        } else {
            ml[j] = m;
        }
    }
    __syncthreads();

    const int NB = (N + 15) / 16, ntile = NB * (NB + 1) / 2;
    const int cl16 = lane & 15, kk = lane >> 4;
    const double l4 = (lambda * lambda) * (lambda * lambda);
    const double w0 = (kk == 0 ? 1.0 : kk == 1 ? lambda : kk == 2 ? lambda * lambda : lambda * lambda * lambda) * winv;
    auto tile_of = [&](int q, int& I, int& J) {
        int rem = q;
        I = 0;
        while (rem >= NB - I) { rem -= NB - I; ++I; }
        J = I + rem;
    };
    // tile (I, J) of sum_s [omega_s] x_s x_s': rows (lane >> 4) + 4 r, column lane & 15 in acc[r]
    auto gram_tile = [&](int I, int J) -> cov_d4 {
        const int ca = 16 * I + cl16, cb = 16 * J + cl16;
        const bool ina = ca < N, inb = cb < N;
        const float sa = ina ? stdv[ca] : 0.f, ma = ina ? mean[ca] : 0.f;
        const float sb_ = inb ? stdv[cb] : 0.f, mb = inb ? mean[cb] : 0.f;
        const double ca_m = ina ? ml[ca] : 0.0, cb_m = inb ? ml[cb] : 0.0;
        const float* za = z + (ina ? ca : 0);
        const float* zb = z + (inb ? cb : 0);
        cov_d4 acc = {0.0, 0.0, 0.0, 0.0};
        double w = w0;
        // four k-steps per trip: their eight loads go out together, ahead of the first MFMA (a wave waits
        // on the panel, not on the matrix core); a step past the window adds 0 * 0 and changes nothing
        for (int k0 = 0; k0 < rows; k0 += 4 * COV_KU) {
            float fa[COV_KU], fb[COV_KU];
#pragma unroll
            for (int u = 0; u < COV_KU; ++u) {
                const int k = k0 + 4 * u + kk;
                const size_t off = (size_t)(k < rows ? hi - 1 - k : lo) * ldz;   // (lo: a row of the window, not used)
                fa[u] = za[off];
                fb[u] = zb[off];
            }
#pragma unroll
            for (int u = 0; u < COV_KU; ++u) {
#pragma clang fp contract(off)
                const bool in = k0 + 4 * u + kk < rows;
                const float pa = fa[u] * sa, pb = fb[u] * sb_;
                const float ra = pa + ma, rb = pb + mb;
                double a = (in && ina) ? (double)ra - ca_m : 0.0;
                const double bb = (in && inb) ? (double)rb - cb_m : 0.0;
                if (ew) { a = a * w; w = w * l4; }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc, 0, 0, 0);
            }
        }
        return acc;
    };

    double rho = 0.0, sc = 1.0, dg = 1e-6;   // Sigma = sc G + dg I
    if (!ew) {
        // pass 2: q_s = ||x_s||^2 per row (a wave per row, butterfly sum), then sum q and sum q^2
        double t1 = 0.0, t2 = 0.0;
        for (int s = lo + wv; s < hi; s += COV_WAVES) {
            double q = 0.0;
            for (int j = lane; j < N; j += 64) {
                const double x = (double)ret(s, j) - ml[j];
                q += x * x;
            }
            q = wave_sum(q);
            t1 += q;
            t2 += q * q;
        }
        // pass 3: ||G||_F^2 from the tiles, those off the diagonal twice; in a diagonal tile row < col twice
        double fr = 0.0;
        for (int q = wv; q < ntile; q += COV_WAVES) {
            int I, J;
            tile_of(q, I, J);
            const cov_d4 acc = gram_tile(I, J);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kk + 4 * r;
                const double g2 = acc[r] * acc[r];
                if (I != J || row < cl16) fr += 2.0 * g2;
                else if (row == cl16) fr += g2;
            }
        }
        fr = wave_sum(fr);
        if (lane == 0) { red[wv] = t1; red[COV_WAVES + wv] = t2; red[2 * COV_WAVES + wv] = fr; }
        __syncthreads();
        double trG = 0.0, q4 = 0.0, fro = 0.0;
        for (int w = 0; w < COV_WAVES; ++w) { trG += red[w]; q4 += red[COV_WAVES + w]; fro += red[2 * COV_WAVES + w]; }
        if (rows > 0) {
#pragma clang fp contract(off)
            const double n = (double)rows, p = (double)N;
            const double trS = trG / n, m = trS / p, delta_ = fro / (n * n);
            if (estimator == KMPC_COV_LEDOIT_WOLF) {
                double beta = (q4 / n - delta_) / (p * n);
                const double delta = (delta_ - 2.0 * m * trS + p * (m * m)) / p;
                beta = fmin(beta, delta);
                rho = (beta == 0.0 || delta == 0.0) ? 0.0 : beta / delta;
            } else {   // KMPC_COV_OAS
                const double alpha = delta_ / (p * p);
                const double num = alpha + m * m, den = (n + 1.0) * (alpha - (m * m) / p);
                rho = den == 0.0 ? 1.0 : fmin(num / den, 1.0);
            }
            sc = (1.0 - rho) / n;
            dg = rho * m + 1e-6;
        } else {
            rho = estimator == KMPC_COV_OAS ? 1.0 : 0.0;
            sc = 0.0;
        }
    }
    if (threadIdx.x == 0 && shrinkage) shrinkage[b] = rho;

    // pass 4: the tiles again, scaled, stored with their mirror
    double* out = sigma + (size_t)b * N * N;
    double* tb = tbuf + wv * 16 * COV_TLD;
    for (int q = wv; q < ntile; q += COV_WAVES) {
        int I, J;
        tile_of(q, I, J);
        const cov_d4 acc = gram_tile(I, J);
        if (I == J) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kk + 4 * r, i = 16 * I + row, j = 16 * I + cl16;
                if (row <= cl16 && j < N) {   // (i <= j < N)
#pragma clang fp contract(off)
                    double v = acc[r] * sc;
                    if (i == j) v += dg;
                    out[(size_t)i * N + j] = v;
                    if (i != j) out[(size_t)j * N + i] = v;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma clang fp contract(off)
                const int row = kk + 4 * r, i = 16 * I + row, j = 16 * J + cl16;   // (i < 16 J <= j: never the diagonal)
                const double v = acc[r] * sc;
                tb[row * COV_TLD + cl16] = v;
                if (i < N && j < N) out[(size_t)i * N + j] = v;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // the mirror: Sigma[16 J + c][16 I + lane & 15] = tile[lane & 15][c]
                const int c = kk + 4 * r, i = 16 * I + cl16, j = 16 * J + c;
                if (i < N && j < N) out[(size_t)j * N + i] = tb[cl16 * COV_TLD + c];
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace

// LDS of the small arrays (vec, Sm, pv, nu, dnu, rpv, red, flag, idg) and, for the LDS variant, M and Y
size_t mv_small_bytes(int N, int H) {
    return sizeof(double) * (2 * (size_t)N * H + (size_t)H * H + 4 * (size_t)H + 18);
}
size_t mv_lds_bytes(int N, int H) {
    const size_t n = (size_t)N * H;
    return mv_small_bytes(N, H) + sizeof(double) * (n * (n + 1) / 2 + H * n);
}
static bool mv_in_lds(int N, int H) { return (size_t)N * H <= 128 && mv_lds_bytes(N, H) <= 160 * 1024; }
static size_t mv_slab(int N, int H) {
    const size_t n = (size_t)N * H;
    return n * (n + 1) / 2 + H * n;
}
size_t mv_workspace_bytes(const kmpc_mv_desc* d) {
    if (!d || d->B <= 0 || mv_in_lds(d->N, d->H)) return 0;
    const size_t slots = d->B < MV_SLOTS ? d->B : MV_SLOTS;
    return sizeof(double) * mv_slab(d->N, d->H) * slots;
}
// ... and of the CAP form: Sm [2H][2H], thirteen H-vectors (mv_window: pv, nu, dnu [2H], rpv and the
// eight of the cap rows), Y [2H][n]. The LDS variant holds every n <= 128 (110,864 bytes at n = 128,
// H = 16).
size_t mv_cap_small_bytes(int N, int H) {
    return sizeof(double) * (2 * (size_t)N * H + 4 * (size_t)H * H + 13 * (size_t)H + 18);
}
size_t mv_cap_lds_bytes(int N, int H) {
    const size_t n = (size_t)N * H;
    return mv_cap_small_bytes(N, H) + sizeof(double) * (n * (n + 1) / 2 + 2 * H * n);
}
static bool mv_cap_in_lds(int N, int H) { return (size_t)N * H <= 128 && mv_cap_lds_bytes(N, H) <= 160 * 1024; }
static size_t mv_cap_slab(int N, int H) {
    const size_t n = (size_t)N * H;
    return n * (n + 1) / 2 + 2 * H * n;
}
size_t mv_cap_workspace_bytes(const kmpc_mv_desc* d) {
    if (!d || d->B <= 0 || mv_cap_in_lds(d->N, d->H)) return 0;
    const size_t slots = d->B < MV_SLOTS ? d->B : MV_SLOTS;
    return sizeof(double) * mv_cap_slab(d->N, d->H) * slots;
}

// ... and of the band forms: the small arrays of the dense forms; M in the band layout, n (cs + 1)
// doubles (cs = N | 1 in LDS, N in the slab: bnd), then Y. LDS variant while a window's LDS stays
// within KMPC_MV_BAND_LDS_BYTES (64 KiB: two windows per CU; n <= 256 follows, since
// n (N + 1 + H) >= n (2 sqrt(n) + 1) doubles). Past that the slab, n (N + 1) + SH H n doubles.
static size_t mv_band_lds_bytes(int N, int H, bool cap) {
    const size_t n = (size_t)N * H;
    return (cap ? mv_cap_small_bytes(N, H) : mv_small_bytes(N, H)) +
           sizeof(double) * (n * ((size_t)(N | 1) + 1) + (cap ? 2 : 1) * H * n);
}
static bool mv_band_in_lds(int N, int H, bool cap) {
    return (size_t)N * H <= 256 && mv_band_lds_bytes(N, H, cap) <= KMPC_MV_BAND_LDS_BYTES;
}
static size_t mv_band_slab(int N, int H, bool cap) {
    const size_t n = (size_t)N * H;
    return n * ((size_t)N + 1) + (cap ? 2 : 1) * H * n;
}
size_t mv_band_workspace_bytes(const kmpc_mv_desc* d, bool cap) {
    if (!d || d->B <= 0 || d->N < 1 || d->H < 1 || mv_band_in_lds(d->N, d->H, cap)) return 0;
    const size_t slots = d->B < MV_SLOTS ? d->B : MV_SLOTS;
    return sizeof(double) * mv_band_slab(d->N, d->H, cap) * slots;
}

// kmpc_solve_mv_band (max_weight, max_turnover: 0 or the active value), kmpc_koopman_mv_run (bd set:
// the batch is its P paths) and kmpc_koopman_mv_sweep (bd set and n_cfg > 0: the batch is n_cfg x P work
// items, config-major; the five cfg_ arrays [n_cfg] are device memory, cfg_max_weight / cfg_max_turnover
// non-null pick the BOX / CAP form and the two scalars are not read): the arguments are checked by the
// C ABI; here the storage variant, the workspace and the launch.
int mv_band_launch(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, double max_turnover,
                   const float* yhat, const double* sigma, size_t sigma_stride, const double* w_prev,
                   double* w_out, int* status, double* obj, int* iters, int step0, int n_steps, const int* valid,
                   const float* realized, int n_real, double* value, double* hist, void* ws, size_t ws_bytes,
                   hipStream_t stream, int n_cfg, const double* cfg_gamma, const double* cfg_mv_cost,
                   const double* cfg_bt_cost, const double* cfg_max_weight, const double* cfg_max_turnover) {
    const bool sweep = bd && n_cfg > 0;
    const int items = sweep ? n_cfg * bd->P : bd ? bd->P : d->B;
    kmpc_mv_desc di = *d;
    di.B = items;
    const bool box = sweep ? cfg_max_weight != nullptr : max_weight > 0.0;
    const bool cap = sweep ? cfg_max_turnover != nullptr : max_turnover > 0.0;
    if (sweep) {   // (the configs' own: a0's limit is what a config with a bad limit is handed, inside 1 / N < u < 1)
        max_weight = box ? 0.5 * (1.0 + 1.0 / d->N) : 0.0;
        max_turnover = 0.0;
    }
    MvArgs a;
    a.B = items; a.N = d->N; a.H = d->H;
    a.gamma = d->gamma; a.c = d->cost_coeff;
    a.allow_short = d->allow_short;
    a.max_iter = d->max_iter > 0 ? d->max_iter : 100;
    a.tol = d->tol > 0.0 ? d->tol : 1e-10;
    a.return_full = bd ? 0 : d->return_full_W;
    a.muf = yhat; a.sigma = sigma; a.sigma_stride = sigma_stride; a.wp = w_prev;
    a.wout = w_out; a.status = status; a.obj = obj; a.iters = iters;
    a.ws = (double*)ws; a.slab = mv_band_slab(d->N, d->H, cap);
    a.max_weight = max_weight;
    a.max_turnover = max_turnover;
    MvBt r;
    r.P = sweep ? bd->P : items; r.items = items; r.n_steps = n_steps; r.n_real = n_real;
    r.nbt = d->N >= 256 ? 256 : 64 * ((d->N + 63) / 64);   // (backtest_step_launch's block)
    r.muf = yhat; r.sigma = sigma; r.valid = valid; r.realized = realized;
    r.gamma = cfg_gamma; r.mv_cost = cfg_mv_cost; r.bt_cost = cfg_bt_cost; r.max_turnover = cfg_max_turnover;
    r.max_weight = cfg_max_weight;
    r.st.P = items; r.st.N = d->N; r.st.S = bd ? bd->S : 0; r.st.k = step0;
    r.st.c = bd && !sweep ? bd->cost_coeff : 0.0;   // (sweep: the config's bt_cost)
    r.st.target = w_out; r.st.realized = nullptr; r.st.w = const_cast<double*>(w_prev); r.st.value = value; r.st.hist = hist;
    const int n = d->N * d->H;
    const int nt = 64 * ((n + 63) / 64);   // >= r.nbt
    const bool in_lds = mv_band_in_lds(d->N, d->H, cap);
    const size_t small = cap ? mv_cap_small_bytes(d->N, d->H) : mv_small_bytes(d->N, d->H);
    if (!in_lds) {
        if (n > 1024 || small > 160 * 1024) return KMPC_ERR_UNSUPPORTED;
        if (!ws || ws_bytes < mv_band_workspace_bytes(&di, cap)) return KMPC_ERR_WORKSPACE;
    }
    const dim3 grid(in_lds ? items : (items < MV_SLOTS ? items : MV_SLOTS));
    const size_t lds = in_lds ? mv_band_lds_bytes(d->N, d->H, cap) : small;
    const auto launch = [&](auto bx, auto cp) {
        constexpr bool BX = decltype(bx)::value, CP = decltype(cp)::value;
        if (sweep) {
            if (in_lds) hipLaunchKernelGGL((mv_band_bt_kernel<256, false, BX, CP, true>), grid, dim3(nt), lds, stream, a, r);
            else hipLaunchKernelGGL((mv_band_bt_kernel<1024, true, BX, CP, true>), grid, dim3(nt), lds, stream, a, r);
        } else if (bd) {
            if (in_lds) hipLaunchKernelGGL((mv_band_bt_kernel<256, false, BX, CP, false>), grid, dim3(nt), lds, stream, a, r);
            else hipLaunchKernelGGL((mv_band_bt_kernel<1024, true, BX, CP, false>), grid, dim3(nt), lds, stream, a, r);
        } else {
            if (in_lds) hipLaunchKernelGGL((mv_band_ipm_kernel<256, false, BX, CP>), grid, dim3(nt), lds, stream, a);
            else hipLaunchKernelGGL((mv_band_ipm_kernel<1024, true, BX, CP>), grid, dim3(nt), lds, stream, a);
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    if (box) { if (cap) launch(T{}, T{}); else launch(T{}, F{}); }
    else     { if (cap) launch(F{}, T{}); else launch(F{}, F{}); }
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

int mv_solve_launch(const kmpc_mv_desc* d, const double* mu, const double* sigma, size_t sigma_stride,
                    const double* w_prev, double* w_out, int* status, double* obj, int* iters,
                    void* ws, size_t ws_bytes, hipStream_t stream, double max_weight, double max_turnover) {
    MvArgs a;
    a.B = d->B; a.N = d->N; a.H = d->H;
    a.gamma = d->gamma; a.c = d->cost_coeff;
    a.allow_short = d->allow_short;
    a.max_iter = d->max_iter > 0 ? d->max_iter : 100;
    a.tol = d->tol > 0.0 ? d->tol : 1e-10;
    a.return_full = d->return_full_W;
    a.mu = mu; a.sigma = sigma; a.sigma_stride = sigma_stride; a.wp = w_prev;
    a.wout = w_out; a.status = status; a.obj = obj; a.iters = iters;
    a.ws = (double*)ws; a.slab = mv_slab(d->N, d->H);
    a.max_weight = max_weight;
    a.max_turnover = max_turnover;
    const bool box = max_weight > 0.0;   // kmpc_solve_mv_box (long-only, N u > 1, u < 1); else the plain kernels
    const int n = d->N * d->H;
    const int nt = 64 * ((n + 63) / 64);
    if (max_turnover > 0.0) {   // kmpc_solve_mv_cap: the CAP kernels, their own LDS and slab sizes
        a.slab = mv_cap_slab(d->N, d->H);
        if (mv_cap_in_lds(d->N, d->H)) {
            const size_t lds = mv_cap_lds_bytes(d->N, d->H);
            if (box)
                hipLaunchKernelGGL((mv_ipm_kernel<128, false, true, true>), dim3(d->B), dim3(nt), lds, stream, a);
            else
                hipLaunchKernelGGL((mv_ipm_kernel<128, false, false, true>), dim3(d->B), dim3(nt), lds, stream, a);
        } else {
            const size_t lds = mv_cap_small_bytes(d->N, d->H);
            if (n > 1024 || lds > 160 * 1024) return KMPC_ERR_UNSUPPORTED;
            if (!ws || ws_bytes < mv_cap_workspace_bytes(d)) return KMPC_ERR_WORKSPACE;
            const int grid = d->B < MV_SLOTS ? d->B : MV_SLOTS;
            if (box)
                hipLaunchKernelGGL((mv_ipm_kernel<1024, true, true, true>), dim3(grid), dim3(nt), lds, stream, a);
            else
                hipLaunchKernelGGL((mv_ipm_kernel<1024, true, false, true>), dim3(grid), dim3(nt), lds, stream, a);
        }
    } else if (mv_in_lds(d->N, d->H)) {
        if (box)
            hipLaunchKernelGGL((mv_ipm_kernel<128, false, true, false>), dim3(d->B), dim3(nt), mv_lds_bytes(d->N, d->H), stream, a);
        else
            hipLaunchKernelGGL((mv_ipm_kernel<128, false, false, false>), dim3(d->B), dim3(nt), mv_lds_bytes(d->N, d->H), stream, a);
    } else {
        if (n > 1024 || mv_small_bytes(d->N, d->H) > 160 * 1024) return KMPC_ERR_UNSUPPORTED;
        if (!ws || ws_bytes < mv_workspace_bytes(d)) return KMPC_ERR_WORKSPACE;
        const int grid = d->B < MV_SLOTS ? d->B : MV_SLOTS;
        if (box)
            hipLaunchKernelGGL((mv_ipm_kernel<1024, true, true, false>), dim3(grid), dim3(nt), mv_small_bytes(d->N, d->H), stream, a);
        else
            hipLaunchKernelGGL((mv_ipm_kernel<1024, true, false, false>), dim3(grid), dim3(nt), mv_small_bytes(d->N, d->H), stream, a);
    }
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

// kmpc_markowitz_run (n_cfg = 0) / kmpc_markowitz_sweep: the arguments are checked by the C ABI;
// here the storage variant, the workspace and the launch. cap: the CAP kernels (kmpc_markowitz_run_cap
// / _sweep_cap), their cap max_turnover (run) or the configs' caps [n_cfg] (sweep, device).
int mv_bt_launch(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, bool cap,
                 double max_turnover, const double* cfg_turnover, int n_cfg,
                 const double* gamma, const double* mv_cost, const double* bt_cost, int step0, int n_steps,
                 const double* mu, const double* sigma, const int* valid, const float* realized, int n_real,
                 double* weights, double* value, double* hist, double* target, int* status, double* obj,
                 void* ws, size_t ws_bytes, hipStream_t stream) {
    const bool sweep = n_cfg > 0;
    const int items = sweep ? n_cfg * bd->P : bd->P;
    kmpc_mv_desc di = *d;
    di.B = items;
    MvArgs a;
    a.B = items; a.N = d->N; a.H = d->H;
    a.gamma = d->gamma; a.c = d->cost_coeff;
    a.allow_short = d->allow_short;
    a.max_iter = d->max_iter > 0 ? d->max_iter : 100;
    a.tol = d->tol > 0.0 ? d->tol : 1e-10;
    a.return_full = 0;
    a.mu = mu; a.sigma = sigma; a.sigma_stride = (size_t)d->N * d->N; a.wp = weights;
    a.wout = target; a.status = status; a.obj = obj; a.iters = nullptr;
    a.ws = (double*)ws; a.slab = cap ? mv_cap_slab(d->N, d->H) : mv_slab(d->N, d->H);
    a.max_weight = max_weight;
    a.max_turnover = max_turnover;
    MvBt r;
    r.P = bd->P; r.items = items; r.n_steps = n_steps; r.n_real = n_real;
    r.nbt = d->N >= 256 ? 256 : 64 * ((d->N + 63) / 64);   // (backtest_step_launch's block)
    r.mu = mu; r.sigma = sigma; r.valid = valid; r.realized = realized;
    r.gamma = gamma; r.mv_cost = mv_cost; r.bt_cost = bt_cost; r.max_turnover = cfg_turnover;
    r.max_weight = nullptr;   // (the dense sweeps: one limit per launch, a.max_weight)
    r.st.P = items; r.st.N = d->N; r.st.S = bd->S; r.st.k = step0; r.st.c = sweep ? 0.0 : bd->cost_coeff;
    r.st.target = target; r.st.realized = nullptr; r.st.w = weights; r.st.value = value; r.st.hist = hist;
    const bool box = max_weight > 0.0;
    const int n = d->N * d->H;
    const int nt = 64 * ((n + 63) / 64);   // >= r.nbt
    const bool in_lds = cap ? mv_cap_in_lds(d->N, d->H) : mv_in_lds(d->N, d->H);
    const size_t small = cap ? mv_cap_small_bytes(d->N, d->H) : mv_small_bytes(d->N, d->H);
    if (!in_lds) {
        if (n > 1024 || small > 160 * 1024) return KMPC_ERR_UNSUPPORTED;
        if (!ws || ws_bytes < (cap ? mv_cap_workspace_bytes(&di) : mv_workspace_bytes(&di))) return KMPC_ERR_WORKSPACE;
    }
    const dim3 grid(in_lds ? items : (items < MV_SLOTS ? items : MV_SLOTS));
    const size_t lds = !in_lds ? small : cap ? mv_cap_lds_bytes(d->N, d->H) : mv_lds_bytes(d->N, d->H);
    const auto launch = [&](auto bx, auto cp, auto sw) {
        if (in_lds)
            hipLaunchKernelGGL((mv_bt_kernel<128, false, decltype(bx)::value, decltype(cp)::value, decltype(sw)::value>), grid, dim3(nt), lds, stream, a, r);
        else
            hipLaunchKernelGGL((mv_bt_kernel<1024, true, decltype(bx)::value, decltype(cp)::value, decltype(sw)::value>), grid, dim3(nt), lds, stream, a, r);
    };
    using T = std::true_type;
    using F = std::false_type;
    const auto by_cap = [&](auto bx, auto sw) { if (cap) launch(bx, T{}, sw); else launch(bx, F{}, sw); };
    if (box) { if (sweep) by_cap(T{}, T{}); else by_cap(T{}, F{}); }
    else     { if (sweep) by_cap(F{}, T{}); else by_cap(F{}, F{}); }
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

int rolling_moments_paths_launch(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                                 const float* mean, const float* stdv, const int* ts, double* mu, double* sigma,
                                 int* valid, hipStream_t stream) {
    hipLaunchKernelGGL(rolling_moments_kernel, dim3((unsigned)(n_ts * P)), dim3(256), sizeof(double) * N, stream, P,
                       T, N, lookback, z, ldz, mean, stdv, ts, mu, sigma, valid);
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

int rolling_moments_launch(int B, int T, int N, int lookback, const float* z, int ldz, const float* mean,
                           const float* stdv, const int* ts, double* mu, double* sigma, int* valid,
                           hipStream_t stream) {
    return rolling_moments_paths_launch(1, B, T, N, lookback, z, ldz, mean, stdv, ts, mu, sigma, valid, stream);
}

// kmpc_rolling_cov (P = 1) / kmpc_rolling_cov_paths: the arguments are checked by the C ABI. The sample
// estimator IS rolling_moments_kernel (its bits are pinned), with the shrinkage zeroed on the stream.
int rolling_cov_paths_launch(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                             const float* mean, const float* stdv, const int* ts, double* mu, double* sigma,
                             int* valid, int estimator, double lambda, double* shrinkage, hipStream_t stream) {
    if (estimator == KMPC_COV_SAMPLE) {
        if (shrinkage && hipMemsetAsync(shrinkage, 0, sizeof(double) * (size_t)n_ts * P, stream) != hipSuccess)
            return KMPC_ERR_LAUNCH;
        return rolling_moments_paths_launch(P, n_ts, T, N, lookback, z, ldz, mean, stdv, ts, mu, sigma, valid, stream);
    }
    hipLaunchKernelGGL(rolling_cov_kernel, dim3((unsigned)(n_ts * P)), dim3(COV_THREADS),
                       sizeof(double) * cov_lds_doubles(N), stream, P, T, N, lookback, z, ldz, mean, stdv, ts, mu,
                       sigma, valid, estimator, lambda, shrinkage);
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

}  // namespace kmpc
