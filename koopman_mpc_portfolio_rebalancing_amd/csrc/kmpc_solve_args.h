// kmpc_solve_args.h — arguments of the batched MPC solve kernel, the ladder from a shape to the
// kernel variant it gets, and the per-horizon launchers.
#pragma once
#include <hip/hip_runtime.h>

#include "kmpc_internal.h"

namespace kmpc {

struct SolveArgs {
    int B, N, H;
    double c, tau;
    int allow_short, max_iter, return_full, n_refine;
    int path;        // kmpc_solve_desc.path (KMPC_PATH_*)
    double tol;
    const float* yhat;
    const double* wp;
    double* wout;
    int* status;
    double* obj;
    int* iters;
    double* trace;   // debug: per-iteration (mu, rd, pr, step) of problem 0, or null
    // mixed precision (kmpc_solve_c3.hip): one warm record per window, or null
    float* warm;
    size_t warm_floats;   // floats per window in warm (mixed_warm_floats)
    // the float32 phase hands its iterate over at mu <= mu_handoff. The box kernels (kmpc_solve_box:
    // float64 only, no float32 phase) read the per-asset position limit from the same slot, so the
    // struct — the kernel argument of every solve kernel — keeps its size and offsets.
    union {
        double mu_handoff;
        double max_weight;
    };
};

// A period whose gross returns R = np.exp(yhat) sum below this is solved on R / sum(R) (the same
// program up to the constant log sum(R); 1 + m = R would lose R's digits): every kernel and the oracle
constexpr double TINY_PERIOD = 0x1p-16;

// Warm record of one window of the mixed-precision pair (kmpc_solve_c3.hip): a 64 B header — int
// flag (1 = warm iterate handed over, 0 = cold: start over, 3 = retried), int float32 iterations,
// padding to WARM_HEAD floats. The fused kernel (the default) hands the iterate over on chip and
// the record is the header alone; the three-launch pair appends w, s, l1, l2, l3 as [5][H][N] and
// z4, l4, nu as [3][H] (float32), padded to 64 B.
constexpr int WARM_HEAD = 16;
__host__ __device__ inline size_t warm_stride(int H, int N) {
    return ((size_t)WARM_HEAD + 5 * (size_t)H * N + 3 * (size_t)H + 15) / 16 * 16;
}
// floats per window of the C3 mixed launcher's record (kmpc_solve_c3.hip: its form decides)
size_t mixed_warm_floats(int H, int N);

// ---- The variant ladder: which ipm_kernel<HM, MAXT, EXACT, FL, CS, QL, GL> a shape gets. ----
// Written once and visited by kmpc_solve (launch_ipm_packed / launch_ipm_case), by the
// path-persistent backtest in its run and sweep forms (kmpc_bt_run.h), each with its own launch as
// the callable, and by the host plan (kmpc_solve.hip) with a probe: the backtest kernels run the
// window body of exactly the variant kmpc_solve picks for the same batch.
constexpr int WAVE = 64;
constexpr int QL_CS = 104;      // cold-array stride of the 128-thread QL variant (N < QL_CS assets)
constexpr int QL_CS256 = 216;   // ... and of the 256-thread one
#ifndef KMPC_PACK_NS   // cold-array slots per 16-lane window of the packed N <= 10 launch
#define KMPC_PACK_NS 11
#endif
// one asset per lane, whole waves: the workgroup of an unpacked window
constexpr int block_threads(int N) { return WAVE * ((N + WAVE - 1) / WAVE); }
// constraint case: 1 = no short, 2 = turnover terms (cost or cap), 4 = turnover cap
__host__ __device__ constexpr int case_of(bool hw, bool hs, bool ht) { return (hw ? 1 : 0) | (hs ? 2 : 0) | (ht ? 4 : 0); }
inline int case_of(const SolveArgs& a) { return case_of(!a.allow_short, a.c > 0.0 || a.tau > 0.0, a.tau > 0.0); }

template <int HM_, int MAXT_, bool EXACT_, int FL_, int CS_ = MAXT_, bool QL_ = false, int GL_ = 64>
struct Variant {
    static constexpr int HM = HM_, MAXT = MAXT_, FL = FL_, CS = CS_, GL = GL_;
    static constexpr bool EXACT = EXACT_, QL = QL_;
    // the C3 rung: its kernels are built in units of their own (kmpc_solve_c3.hip, kmpc_solve_c3sw.hip)
    static constexpr bool C3 = HM == 10 && MAXT == 128 && FL == 7 && QL;
};

// Packed rungs: windows of N <= 32 assets (3 H <= GL) run 64 / GL per one-wave block, each on its
// own lane group (GL = 16 for N <= 16 when 3 HM <= 16, else 32). Constant-case variants for H == HM
// in the two common cases (FL = 7, FL = 1), the generic one otherwise. Calls f(Variant<...>{}) and
// returns its result, or KMPC_ERR_UNSUPPORTED outside that range without calling it.
template <int HM, class F>
int visit_packed(const SolveArgs& a, F&& f) {
    if (a.H > HM || a.N > 32 || 3 * HM > 32) return KMPC_ERR_UNSUPPORTED;
    const int fl = case_of(a);
    const bool exact = a.H == HM;
    if constexpr (3 * HM <= 16) {
        if (a.N <= 16) {
            // N <= 10 (BASELINE configs[0]): the cold arrays at 11 slots per window instead of 16
            // (44 per block): 29 -> 24 KB of LDS per block, six blocks per CU instead of five
            if (exact && fl == 7 && a.N <= KMPC_PACK_NS - 1) return f(Variant<HM, 64, true, 7, 4 * KMPC_PACK_NS, false, 16>{});
            if (exact && fl == 7) return f(Variant<HM, 64, true, 7, 64, false, 16>{});
            if (exact && fl == 1) return f(Variant<HM, 64, true, 1, 64, false, 16>{});
            return f(Variant<HM, 64, false, -1, 64, false, 16>{});
        }
    }
    if constexpr (3 * HM <= 32) {
        if (exact && fl == 7) return f(Variant<HM, 64, true, 7, 64, false, 32>{});
        if (exact && fl == 1) return f(Variant<HM, 64, true, 1, 64, false, 32>{});
        return f(Variant<HM, 64, false, -1, 64, false, 32>{});
    }
    return KMPC_ERR_UNSUPPORTED;
}

// Constant-case rungs (H == HM, N <= 128; case 7 up to 256): the constraint case is a template
// argument, so every predicate on it folds away. Cases: 7 = no short + cost + cap (the benchmark's),
// 1 = no short only (c = tau = 0: the simplex program of BASELINE configs[1]). KMPC_ERR_UNSUPPORTED
// for any other case (kmpc_solve then takes the generic kernel, launch_ipm).
template <int HM, class F>
int visit_case(const SolveArgs& a, F&& f) {
    const int nt = block_threads(a.N);
    const int fl = case_of(a);
    if (a.H != HM || nt > 256) return KMPC_ERR_UNSUPPORTED;
    if (fl == 7) {
        if constexpr (HM == 10) {
            // N <= 103 at H = 10 (BASELINE configs[2..3]: N = 100), the C3 rung: the per-asset LDL^T
            // arrays (iDd, Lr) join the cold arrays in LDS with a 104-lane stride (two windows per CU
            // still fit): 40 VGPRs of live state less, 132 -> 107 spilled dwords, C3 solve +4.5% (r02)
            if (nt == 128 && a.N < QL_CS) return f(Variant<HM, 128, true, 7, QL_CS, true>{});
            // 256-thread windows (one per CU): the 8 cold arrays at a 216-lane stride fit 160 KB
            // (151 -> 108 spilled dwords; N = 200 +6.7%, measured r02)
            if (nt == 256 && a.N < QL_CS256) return f(Variant<HM, 256, true, 7, QL_CS256, true>{});
        }
        return nt <= 64 ? f(Variant<HM, 64, true, 7>{}) : (nt <= 128 ? f(Variant<HM, 128, true, 7>{}) : f(Variant<HM, 256, true, 7>{}));
    }
    if (nt > 128) return KMPC_ERR_UNSUPPORTED;
    if (fl == 1) return nt <= 64 ? f(Variant<HM, 64, true, 1>{}) : f(Variant<HM, 128, true, 1>{});
    return KMPC_ERR_UNSUPPORTED;
}

// ipm_kernel launchers, one translation unit per compile-time horizon bound HM (kmpc_solve_h*.hip)
template <int HM>
int launch_ipm(const SolveArgs& a, hipStream_t stream);
// ... of the box case (a.max_weight: per-asset position limit; kmpc_solve_hbox*.hip)
template <int HM>
int launch_ipm_box(const SolveArgs& a, hipStream_t stream);
// the closed-form presolve (kmpc_solve_simplex.hip: c = tau = 0, no short)
int simplex_launch(const SolveArgs& a, hipStream_t stream);
// large-window kernel (kmpc_solve_big.hip): workspace it needs, and the launch
size_t big_ws_bytes(const SolveArgs& a);
int big_launch(const SolveArgs& a, void* ws, size_t ws_size, hipStream_t stream);
// ... and its box form (a.max_weight: the position limit; kmpc_solve_bigbox.hip): two more slab arrays
size_t big_box_ws_bytes(const SolveArgs& a);
int big_box_launch(const SolveArgs& a, void* ws, size_t ws_size, hipStream_t stream);
// constant-case kernels (kmpc_solve_h*_case.hip); KMPC_ERR_UNSUPPORTED if the case has none
template <int HM>
int launch_ipm_case(const SolveArgs& a, hipStream_t stream);
// the C3 kernel (H = 10, FL = 7, 128 threads, LDL^T arrays in LDS) in its own -O2 unit
// (kmpc_solve_c3.hip): float64, or with a.warm set the mixed-precision pair
int launch_ipm_c3(const SolveArgs& a, hipStream_t stream);
// One launch of the path-persistent backtest kernel (kmpc_bt_run.h) in its two forms. The run
// (kmpc_backtest_run): a.B = P paths, a.wout the [P, N] W0 scratch, a.status / a.obj [P] scratch,
// cost the bookkeeping's cost_coeff, the three per-config arrays null. The sweep
// (kmpc_backtest_sweep): a.B = C P work items (config-major), the scratch sized for them; a.c, a.tau
// and cost are not read (the kernel takes them per config from the device arrays). Always case 7.
struct BtLaunch {
    int P, n_steps, n_real, step0, S;                  // n_steps steps from history row step0 of S
    double cost;
    const double *mpc_cost, *max_turnover, *bt_cost;   // [C] device
    const float *yhat, *realized;                      // [n_steps, P, H, N], [n_steps, P, N]
    double *weights, *value, *hist;                    // [C P, N], [C P], [C P, S, 4]
};
// ... of the C3 shape (the run: kmpc_solve_c3.hip, the sweep: kmpc_solve_c3sw.hip), the constant-case
// shapes H = HM (kmpc_solve_hbt*.hip, kmpc_solve_hsw*.hip) and the packed shapes (N <= 32, H = HM, one
// lane group per work item; kmpc_solve_p*.hip, kmpc_solve_psw*.hip); KMPC_ERR_UNSUPPORTED elsewhere
template <bool SWEEP>
int launch_bt_c3(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
template <int HM, bool SWEEP>
int launch_bt_case(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
template <int HM, bool SWEEP>
int launch_bt_packed(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
// ... and of the box case (a.max_weight: the position limit, one value for every work item): the
// kernel launch_ipm_box<HM> picks for the same N (kmpc_solve_hbtbox*.hip, kmpc_solve_hswbox*.hip). The
// sweep's a.c and a.tau come per config from the device arrays here too; the constraint case is read
// at run time (the generic kernel).
template <int HM, bool SWEEP>
int launch_bt_box(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
// packed small-window kernels, 64 / GL windows per wave (kmpc_solve_p*.hip); KMPC_ERR_UNSUPPORTED
// outside N <= 32, 3 H <= 32
template <int HM>
int launch_ipm_packed(const SolveArgs& a, hipStream_t stream);

}  // namespace kmpc
