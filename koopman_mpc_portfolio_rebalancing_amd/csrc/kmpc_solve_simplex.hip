// kmpc_solve_simplex.hip — the closed-form presolve of the batched MPC solve. Without turnover terms
// (c = tau = 0) and without shorting the program decouples into one problem per period,
// max log(R_t . w_t) over the simplex, whose optimum is exact in closed form — BASELINE configs[1],
// "no-short simplex projection only". kmpc_solve.hip decides when it applies (simplex_case).
#include "kmpc_internal.h"
#include "kmpc_npexp.h"
#include "kmpc_solve_args.h"

namespace kmpc {

namespace {

// c = tau = 0, w >= 0: per period t, log(R_t . w_t) with R = exp(yhat) > 0 is maximized over the
// simplex exactly on the face of the assets with the largest R_t; the returned point is that
// face's centre (equal weights over exact ties: the analytic centre an interior-point method
// converges to, and the vertex e_argmax otherwise). problem.value as the IPM kernels report it
// (mpc.py:103): sum_t log(R_t . w_t) - c sum_t ||w_t - w_{t-1}||_1 (c <= 0 here). One wave per
// window, lanes over the assets (coalesced loads, wave butterflies for max / tie count / sums).
// Non-finite inputs -> solver_error and tile(w_prev).
__device__ __forceinline__ float wmaxf(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wsum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wsumi(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
constexpr int SIMPLEX_WAVES = 4;   // waves per 256-thread block
constexpr int SIMPLEX_HR = 16;     // register fast path: N <= 64 assets, H <= 16 periods
// butterflies within aligned groups of G lanes (G = 32 or 64)
template <int G>
__device__ __forceinline__ float gmaxf(float v) {
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
template <int G>
__device__ __forceinline__ int gsumi(int v) {
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// N <= G (G = 32: two windows per wave; G = 64: one), H <= 16 (BASELINE configs[1]: N = 30, H = 5):
// lane i of the window's lane group holds R_t,i of its asset for every period in registers (one
// pass over yhat, one np_expf per element), and each group reduction runs over all periods at once
// (H independent butterflies interleaved, instead of H dependent rounds). Same arithmetic and order
// as the general loop below (a group butterfly over G lanes adds zeros where the wave-wide one did):
// bit-identical results.
// HR: the period bound; HX = H known at compile time (BASELINE configs[1]: H = 5 — no period guards)
template <int G, int HR = SIMPLEX_HR, bool HX = false>
__device__ __forceinline__ void simplex_regs(const SolveArgs& a, int b, int lane) {
    const int N = a.N, H = HX ? HR : a.H, tw = a.return_full ? H : 1;
    const float* y = a.yhat + (size_t)b * H * N;
    const double* wp = a.wp + (size_t)b * N;
    double* wout = a.wout + (size_t)b * tw * N;
    const bool act = lane < N;
    const double wpi = act ? wp[lane] : 0.0;
    float R[HR];
    int bad = !(isfinite(a.c) && isfinite(a.tau)) || (act && !isfinite(wpi));
#pragma unroll
    for (int t = 0; t < HR; ++t) {
        R[t] = 0.0f;
        if (t < H && act) {
            R[t] = np_expf(y[(size_t)t * N + lane]);
            bad |= !isfinite(R[t]);
        }
    }
    if (gsumi<G>(bad)) {
        if (act)
            for (int t = 0; t < tw; ++t) wout[(size_t)t * N + lane] = wpi;   // mpc.py:113-115
        if (lane == 0) {
            a.status[b] = KMPC_STATUS_SOLVER_ERROR;
            a.obj[b] = __builtin_nan("");
            if (a.iters) a.iters[b] = 0;
        }
        return;
    }
    float rm[HR];
    int cnt[HR];
#pragma unroll
    for (int t = 0; t < HR; ++t) rm[t] = R[t];
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int t = 0; t < HR; ++t)
            if (t < H) rm[t] = fmaxf(rm[t], __shfl_xor(rm[t], o));
    // a period whose every R underflowed to 0 (yhat <= -103.97): R_t . w_t = 0 on the whole simplex
    // and the reference's exp cone exp(u) <= R_t . w_t has no solution (cvxpy: infeasible) —
    // infeasible and the fallback, as the interior-point kernels report it
    bool flat0 = false;
#pragma unroll
    for (int t = 0; t < HR; ++t) flat0 |= t < H && !(rm[t] > 0.0f);
    if (flat0) {
        if (act)
            for (int t = 0; t < tw; ++t) wout[(size_t)t * N + lane] = wpi;   // mpc.py:113-115
        if (lane == 0) {
            a.status[b] = KMPC_STATUS_INFEASIBLE;
            a.obj[b] = __builtin_nan("");
            if (a.iters) a.iters[b] = 0;
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < HR; ++t) cnt[t] = (t < H && act && R[t] == rm[t]) ? 1 : 0;
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int t = 0; t < HR; ++t)
            if (t < H) cnt[t] += __shfl_xor(cnt[t], o);
    double rw[HR], l1[HR];
    double wprev = wpi;
#pragma unroll
    for (int t = 0; t < HR; ++t) {
        rw[t] = l1[t] = 0.0;
        if (t < H) {
            const double w = 1.0 / cnt[t];
            const double wi = (act && R[t] == rm[t]) ? w : 0.0;
            rw[t] = (double)R[t] * wi;
            l1[t] = act ? fabs(wi - wprev) : 0.0;
            if (act && t < tw) wout[(size_t)t * N + lane] = wi;
            wprev = wi;
        }
    }
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int t = 0; t < HR; ++t)
            if (t < H) { rw[t] += __shfl_xor(rw[t], o); l1[t] += __shfl_xor(l1[t], o); }
    if (lane == 0) {
        double f = 0.0;
#pragma unroll
        for (int t = 0; t < HR; ++t)
            if (t < H) f += log(rw[t]) - a.c * l1[t];
        a.status[b] = KMPC_STATUS_OPTIMAL;
        a.obj[b] = f;
        if (a.iters) a.iters[b] = 0;
    }
}

__global__ void __launch_bounds__(64 * SIMPLEX_WAVES) simplex_kernel(SolveArgs a) {
    const int lane = threadIdx.x & 63;
    if (a.N <= 32 && a.H <= SIMPLEX_HR) {
        // two windows per wave, one per 32-lane half
        const int b = (blockIdx.x * SIMPLEX_WAVES + (threadIdx.x >> 6)) * 2 + (lane >> 5);
        if (b < a.B) {   // (whole lane groups)
            if (a.H == 5) simplex_regs<32, 5, true>(a, b, lane & 31);
            else simplex_regs<32>(a, b, lane & 31);
        }
        return;
    }
    const int b = blockIdx.x * SIMPLEX_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;   // (whole waves)
    if (a.N <= 64 && a.H <= SIMPLEX_HR) {
        simplex_regs<64>(a, b, lane);
        return;
    }
    const int N = a.N, H = a.H, tw = a.return_full ? H : 1;
    const float* y = a.yhat + (size_t)b * H * N;
    const double* wp = a.wp + (size_t)b * N;
    double* wout = a.wout + (size_t)b * tw * N;
    int bad = !(isfinite(a.c) && isfinite(a.tau));
    for (int i = lane; i < N; i += 64) bad |= !isfinite(wp[i]);
    for (int k = lane; k < H * N; k += 64) bad |= !isfinite(np_expf(y[k]));
    // a period whose every R underflowed to 0: infeasible (see simplex_regs)
    int zero = 0;
    for (int t = 0; t < H; ++t) {
        float rm = 0.0f;
        for (int i = lane; i < N; i += 64) rm = fmaxf(rm, np_expf(y[(size_t)t * N + i]));
        zero |= !(wmaxf(rm) > 0.0f);
    }
    bad = wsumi(bad);
    if (bad || zero) {
        for (int k = lane; k < tw * N; k += 64) wout[k] = wp[k % N];   // mpc.py:113-115
        if (lane == 0) {
            a.status[b] = bad ? KMPC_STATUS_SOLVER_ERROR : KMPC_STATUS_INFEASIBLE;
            a.obj[b] = __builtin_nan("");
            if (a.iters) a.iters[b] = 0;
        }
        return;
    }
    // the face is that of the largest float32 R = np.exp(yhat) (mpc.py:55): distinct yhat can
    // round to the same R, and the program the reference solves only sees R
    double f = 0.0;
    float prm = 0.0f;
    double pw = 0.0;   // the previous period's face weight
    for (int t = 0; t < H; ++t) {
        const float* yt = y + (size_t)t * N;
        float rm = 0.0f;
        for (int i = lane; i < N; i += 64) rm = fmaxf(rm, np_expf(yt[i]));
        rm = wmaxf(rm);
        int cnt = 0;
        for (int i = lane; i < N; i += 64) cnt += np_expf(yt[i]) == rm;
        cnt = wsumi(cnt);
        const double w = 1.0 / cnt;
        double rw = 0.0, l1 = 0.0;
        for (int i = lane; i < N; i += 64) {
            const float ri = np_expf(yt[i]);
            const double wi = ri == rm ? w : 0.0;
            rw += (double)ri * wi;
            const double wprev = t == 0 ? wp[i] : (np_expf(y[(size_t)(t - 1) * N + i]) == prm ? pw : 0.0);
            l1 += fabs(wi - wprev);
            if (t < tw) wout[(size_t)t * N + i] = wi;
        }
        f += log(wsum(rw)) - a.c * wsum(l1);
        prm = rm;
        pw = w;
    }
    if (lane == 0) {
        a.status[b] = KMPC_STATUS_OPTIMAL;
        a.obj[b] = f;
        if (a.iters) a.iters[b] = 0;
    }
}

}  // namespace

int simplex_launch(const SolveArgs& a, hipStream_t stream) {
    const int per_block = SIMPLEX_WAVES * ((a.N <= 32 && a.H <= SIMPLEX_HR) ? 2 : 1);
    hipLaunchKernelGGL(simplex_kernel, dim3((a.B + per_block - 1) / per_block), dim3(64 * SIMPLEX_WAVES), 0,
                       stream, a);
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

}  // namespace kmpc
