// kmpc_bt_run.h — the path-persistent backtest kernel (kmpc_backtest_run; run_backtest,
// backtest.py:133-219, for P independent paths): one workgroup per path runs every step of its path
// back to back — the step's window solve (the body of ipm_kernel, kmpc_ipm_body.inc) then the
// step's bookkeeping (kmpc_bt_step.h, as kmpc_backtest_step) — with no launch and no lock step
// between steps: a path never waits for the slowest window of a batch. The same kernel has a sweep
// form (kmpc_backtest_sweep): C MPC configs (cost_coeff, max_turnover, the backtest's cost_coeff)
// over the same P paths in one launch, one work item per (config j, path p), state index
// q = j P + p (config-major), the step's forecast and realized row read at the path p, so the
// forecasts are rolled out once for the P paths and not per config.
// Instantiated next to the ipm_kernel it mirrors, in a unit with the same compile options: the run
// in kmpc_solve_c3.hip (the C3 kernel), kmpc_solve_hbt*.hip (the constant-case kernels of
// kmpc_solve_h*_case.hip) and kmpc_solve_p*.hip (the packed ones); the sweep in units of its own
// (kmpc_solve_c3sw.hip, kmpc_solve_hsw*.hip, kmpc_solve_psw*.hip) with the options of those.
// The box form (kmpc_backtest_run_box, kmpc_backtest_sweep_box: a per-asset position limit) wraps the
// body of the box kernels of kmpc_solve_box (launch_ipm_box) the same way, in kmpc_solve_hbtbox*.hip
// (the run) and kmpc_solve_hswbox*.hip (the sweep), built with the options of kmpc_solve_hbox*.hip.
#pragma once
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_step.h"

namespace kmpc {

struct BtRun {
    int n_steps;             // steps run by this launch
    int n_real;              // steps k < n_real have a realized row (later ones: no market move)
    const float* yhat;       // [n_steps, P, H, N] forecasts
    const float* realized;   // [n_steps, P, N] log-returns of each step's t + 1
    bt::StepArgs st;         // bookkeeping: st.k = the first step's history row; st.target = W0 scratch
};

struct BtSweep {
    int P;                        // paths (a0.B = C P work items)
    const double* mpc_cost;       // [C] device: the solve's cost_coeff
    const double* max_turnover;   // [C] device: the solve's turnover cap
    const double* bt_cost;        // [C] device: the bookkeeping's cost_coeff
};

template <class T>
__device__ __forceinline__ const T& first_of(const T& t) { return t; }

// One workgroup per work item (window index b = q), or for the packed kernels (GL < 64: N <= 32)
// one GL-lane group per work item, 64 / GL of them per one-wave workgroup. The per-step solve is the
// float64 kernel ipm_kernel<HM, MAXT, EXACT, FL, CS, QL, GL, 0> (the one kmpc_solve picks for a batch
// of P < KMPC_MIXED_MIN_B such windows), so every step's W0 matches the lock-step run's. The work
// items of one packed wave step together (one whose window has converged waits, masked, for its
// wave's slowest), but never for the rest of the batch.
// Sw... is empty (the run: a work item is a path, its parameters a0's) or BtSweep (the sweep); an
// empty pack adds no kernel argument, so the run kernel keeps its kernarg layout. The sweep's kernels
// are the constant case 7 (no short, turnover terms, cap): a config outside it (max_turnover <= 0,
// mpc_cost < 0, or either NaN) gets a NaN parameter, which the window body answers with
// KMPC_STATUS_SOLVER_ERROR and the hold fallback (W0 = w_prev) at every step. In the packed form the
// lane groups of one wave hold different configs: c and tau are per-lane values.
// BOX (shadows the namespace constant the window body reads by name): the per-step solve is the box
// kernel ipm_kernel<HM, MAXT, false, -1, CS, false, 64, 0, true> of launch_ipm_box, the limit in
// a0.max_weight (one value for every work item). That kernel is the generic one: it reads the
// constraint case, c and tau at run time, so its sweep form needs no constant case; a poisoned
// config's NaN parameter ends in the same KMPC_STATUS_SOLVER_ERROR hold.
template <int HM, int MAXT, bool EXACT, int FL, int CS, bool QL, int GL, int PH, bool BOX, class... Sw>
__global__ void __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(HM <= KMPC_WPE2_HM ? 2 : 1)))
bt_kernel(SolveArgs a0, BtRun r, Sw... sw_) {
    constexpr bool SWEEP = sizeof...(Sw) == 1;
    static_assert(PH == 0, "float64 windows");
    static_assert(!SWEEP || FL == 7 || BOX, "per-config parameters stay inside one constant case, or the generic box kernel");
    static_assert(!BOX || (FL == -1 && !EXACT && GL == 64 && !QL), "box kernels: generic float64, whole waves");
    static_assert(GL == 64 || MAXT == 64, "lane groups pack one-wave blocks");
    using Real = double;
    constexpr int NWM = MAXT / WAVE;
    constexpr int WPB = GL == 64 ? 1 : 64 / GL;   // work items per block
    static_assert(sizeof(Shared<HM, NWM, Real>) * WPB + sizeof(double) * NWM +
                      cold_bytes<HM, MAXT, CS, QL, GL, FL, Real, BOX>() <= 160 * 1024, "LDS of one workgroup");
    __shared__ Shared<HM, NWM, Real> shv[WPB];
    __shared__ double red[NWM];
    auto& sh = shv[grp<GL>()];
    const int q = blockIdx.x * WPB + grp<GL>();
    if constexpr (GL < 64) {
        if (q >= a0.B) return;   // (whole groups of the last block)
    }
    // (assigned in the two branches, not defaulted and overwritten: that form reordered the moves at
    // the head of every sweep kernel)
    int p, P;
    double cj, tj, cb;
    if constexpr (SWEEP) {
        const BtSweep& sw = first_of(sw_...);
        const int j = q / sw.P;
        p = q - j * sw.P;
        P = sw.P;
        cj = sw.mpc_cost[j], tj = sw.max_turnover[j];
        if (!(cj >= 0.0)) cj = __builtin_nan("");
        if (!(tj > 0.0)) tj = __builtin_nan("");
        cb = sw.bt_cost[j];
    } else {
        p = q; P = a0.B; cj = a0.c; tj = a0.tau; cb = r.st.c;
    }
    const size_t PHN = (size_t)P * a0.H * a0.N, PN = (size_t)P * a0.N;
    for (int k = 0; k < r.n_steps; ++k) {
        {
            SolveArgs args = a0;
            args.yhat = r.yhat + k * PHN;
            if constexpr (SWEEP) {
                args.c = cj;
                args.tau = tj;
            }
            // (laundering b and the argument fields every step — nothing derived from them hoisted
            // out of the loop — cut the scratch from 512 to 448 B per lane but ran slower: P = 64
            // 0.898 -> 0.913 ms per step, P = 1,024 1.92 -> 1.98 ms)
            const int b = q;
            const int yb = p;
            Handoff<HM, false> hand;
#include "kmpc_ipm_body.inc"
        }
        __syncthreads();   // W0 (st.target) of every lane, and the solve's LDS, done
        bt::StepArgs st = r.st;
        st.k = r.st.k + k;
        if constexpr (SWEEP) st.c = cb;
        st.realized = k < r.n_real ? r.realized + k * PN : nullptr;
        if constexpr (GL == 64)
            bt::bt_step_body(st, q, p, red);
        else
            bt::bt_step_group<GL>(st, q, p, gvt<GL>());
        __syncthreads();   // the drifted weights are the next solve's w_prev
    }
}

// the launch (BtLaunch: kmpc_solve_args.h)
template <bool SWEEP, int HM, int MAXT, bool EXACT, int FL, int CS = MAXT, bool QL = false, int GL = 64, bool BOX = false>
int launch_bt_one(const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    BtRun r;
    r.n_steps = l.n_steps;
    r.n_real = l.n_real;
    r.yhat = l.yhat;
    r.realized = l.realized;
    r.st.P = a.B; r.st.N = a.N; r.st.S = l.S; r.st.k = l.step0; r.st.c = SWEEP ? 0.0 : l.cost;
    r.st.target = a.wout; r.st.realized = nullptr; r.st.w = l.weights; r.st.value = l.value; r.st.hist = l.hist;
    SolveArgs s = a;
    s.wp = l.weights;   // each step's w_prev: the work item's current (drifted) weights
    const size_t lds = cold_bytes<HM, MAXT, CS, QL, GL, FL, double, BOX>();
    constexpr int WPB = GL == 64 ? 1 : 64 / GL;
    const auto launch = [&](auto... sw) {
        hipLaunchKernelGGL((bt_kernel<HM, MAXT, EXACT, FL, CS, QL, GL, 0, BOX, decltype(sw)...>), dim3((a.B + WPB - 1) / WPB),
                           dim3(GL == 64 ? block_threads(a.N) : 64), lds, stream, s, r, sw...);
    };
    if constexpr (SWEEP)
        launch(BtSweep{l.P, l.mpc_cost, l.max_turnover, l.bt_cost});
    else
        launch();
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

// launch_bt_one of a rung of the ladder (kmpc_solve_args.h). The persistent kernels exist for the
// float64 constant case 7 with H = HM: KMPC_ERR_UNSUPPORTED on any other rung (a ragged H or another
// case runs the generic kernel: no persistent form) and on the C3 rung, whose kernel is
// launch_bt_c3's (kmpc_solve_c3.hip, kmpc_solve_c3sw.hip).
template <bool SWEEP, class V>
int launch_bt_variant(V, const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    if constexpr (V::FL == 7 && V::EXACT && !V::C3)
        return launch_bt_one<SWEEP, V::HM, V::MAXT, true, 7, V::CS, V::QL, V::GL>(a, l, stream);
    else
        return KMPC_ERR_UNSUPPORTED;
}

// The packed and the constant-case shapes: the rung launch_ipm_packed<HM> / launch_ipm_case<HM>
// takes for the same batch.
template <int HM, bool SWEEP>
int launch_bt_packed(const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    return visit_packed<HM>(a, [&](auto v) { return launch_bt_variant<SWEEP>(v, a, l, stream); });
}
template <int HM, bool SWEEP>
int launch_bt_case(const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    return visit_case<HM>(a, [&](auto v) { return launch_bt_variant<SWEEP>(v, a, l, stream); });
}
// The C3 rung (the ladder leaves it to units of its own)
template <bool SWEEP>
int launch_bt_c3(const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    return launch_bt_one<SWEEP, 10, 128, true, 7, QL_CS, true>(a, l, stream);
}
// The box form (a.max_weight set): the kernel launch_ipm_box<HM> takes for the same N, H <= HM read
// at run time
template <int HM, bool SWEEP>
int launch_bt_box(const SolveArgs& a, const BtLaunch& l, hipStream_t stream) {
    const int nt = block_threads(a.N);
    if (a.H > HM || nt > 256) return KMPC_ERR_UNSUPPORTED;
#if KMPC_BOX_QLCS
    if constexpr (HM == 10)
        if (nt == 128 && a.N < QL_CS) return launch_bt_one<SWEEP, HM, 128, false, -1, QL_CS, false, 64, true>(a, l, stream);
#endif
    if (nt <= 64) return launch_bt_one<SWEEP, HM, 64, false, -1, 64, false, 64, true>(a, l, stream);
    if (nt <= 128) return launch_bt_one<SWEEP, HM, 128, false, -1, 128, false, 64, true>(a, l, stream);
    return launch_bt_one<SWEEP, HM, 256, false, -1, 256, false, 64, true>(a, l, stream);
}

}  // namespace kmpc
