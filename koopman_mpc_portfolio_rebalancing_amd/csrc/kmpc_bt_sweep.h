// kmpc_bt_sweep.h — the sweep form of the path-persistent backtest kernel (kmpc_backtest_sweep):
// C MPC configs (cost_coeff, max_turnover, the backtest's cost_coeff) over the same P paths in one
// launch. bt_run_kernel (kmpc_bt_run.h) with per-workgroup parameters: one workgroup — one lane
// group in the packed form — per (config j, path p), state index q = j P + p (config-major), the
// step's forecast and realized row read at the path p, so the forecasts are rolled out once for
// the P paths and not per config. Instantiated in units of their own (kmpc_solve_*sw*.hip) with the
// compile options of the units whose kernels they mirror.
#pragma once
#include "kmpc_bt_run.h"

namespace kmpc {

struct BtSweep {
    int P;                        // paths (a0.B = C P work items)
    const double* mpc_cost;       // [C] device: the solve's cost_coeff
    const double* max_turnover;   // [C] device: the solve's turnover cap
    const double* bt_cost;        // [C] device: the bookkeeping's cost_coeff
};

// The kernels are the constant case 7 (no short, turnover terms, cap): a config outside it
// (max_turnover <= 0, mpc_cost < 0, or either NaN) gets a NaN parameter, which the window body
// answers with KMPC_STATUS_SOLVER_ERROR and the hold fallback (W0 = w_prev) at every step. In the
// packed form the lane groups of one wave hold different configs: c and tau are per-lane values.
template <int HM, int MAXT, bool EXACT, int FL, int CS, bool QL, int GL, int PH>
__global__ void __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(HM <= KMPC_WPE2_HM ? 2 : 1)))
bt_sweep_kernel(SolveArgs a0, BtRun r, BtSweep sw) {
    static_assert(PH == 0, "float64 windows");
    static_assert(FL == 7, "per-config parameters stay inside one constant case");
    static_assert(GL == 64 || MAXT == 64, "lane groups pack one-wave blocks");
    using Real = double;
    constexpr int NWM = MAXT / WAVE;
    constexpr int WPB = GL == 64 ? 1 : 64 / GL;   // work items per block
    __shared__ Shared<HM, NWM, Real> shv[WPB];
    __shared__ double red[NWM];
    auto& sh = shv[grp<GL>()];
    const int q = blockIdx.x * WPB + grp<GL>();
    if constexpr (GL < 64) {
        if (q >= a0.B) return;   // (whole groups of the last block)
    }
    const int j = q / sw.P, p = q - j * sw.P;
    double cj = sw.mpc_cost[j], tj = sw.max_turnover[j];
    if (!(cj >= 0.0)) cj = __builtin_nan("");
    if (!(tj > 0.0)) tj = __builtin_nan("");
    const double cb = sw.bt_cost[j];
    const size_t PHN = (size_t)sw.P * a0.H * a0.N, PN = (size_t)sw.P * a0.N;
    for (int k = 0; k < r.n_steps; ++k) {
        {
            SolveArgs args = a0;
            args.yhat = r.yhat + k * PHN;
            args.c = cj;
            args.tau = tj;
            const int b = q;
            const int yb = p;
            Handoff<HM, false> hand;
#include "kmpc_ipm_body.inc"
        }
        __syncthreads();   // W0 (st.target) of every lane, and the solve's LDS, done
        bt::StepArgs st = r.st;
        st.k = r.st.k + k;
        st.c = cb;
        st.realized = k < r.n_real ? r.realized + k * PN : nullptr;
        if constexpr (GL == 64)
            bt::bt_step_body(st, q, p, red);
        else
            bt::bt_step_group<GL>(st, q, p, gvt<GL>());
        __syncthreads();   // the drifted weights are the next solve's w_prev
    }
}

// the launch (SweepLaunch: kmpc_solve_args.h)
template <int HM, int MAXT, bool EXACT, int FL, int CS = MAXT, bool QL = false, int GL = 64>
int launch_bt_sweep_one(const SolveArgs& a, const SweepLaunch& l, hipStream_t stream) {
    BtRun r;
    r.n_steps = l.n_steps;
    r.n_real = l.n_real;
    r.yhat = l.yhat;
    r.realized = l.realized;
    r.st.P = a.B; r.st.N = a.N; r.st.S = l.S; r.st.k = l.step0; r.st.c = 0.0;
    r.st.target = a.wout; r.st.realized = nullptr; r.st.w = l.weights; r.st.value = l.value; r.st.hist = l.hist;
    BtSweep sw;
    sw.P = l.P; sw.mpc_cost = l.mpc_cost; sw.max_turnover = l.max_turnover; sw.bt_cost = l.bt_cost;
    SolveArgs s = a;
    s.wp = l.weights;   // each step's w_prev: the work item's current (drifted) weights
    const size_t lds = cold_bytes<HM, MAXT, CS, QL, GL, FL, double>();
    constexpr int WPB = GL == 64 ? 1 : 64 / GL;
    hipLaunchKernelGGL((bt_sweep_kernel<HM, MAXT, EXACT, FL, CS, QL, GL, 0>), dim3((a.B + WPB - 1) / WPB),
                       dim3(GL == 64 ? block_threads(a.N) : 64), lds, stream, s, r, sw);
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

// launch_bt_sweep_one of a rung of the ladder, as launch_bt_run_variant (the C3 rung's kernel is
// launch_bt_sweep_c3's, kmpc_solve_c3sw.hip)
template <class V>
int launch_bt_sweep_variant(V, const SolveArgs& a, const SweepLaunch& l, hipStream_t stream) {
    if constexpr (V::FL == 7 && V::EXACT && !V::C3)
        return launch_bt_sweep_one<V::HM, V::MAXT, true, 7, V::CS, V::QL, V::GL>(a, l, stream);
    else
        return KMPC_ERR_UNSUPPORTED;
}

// the packed and the constant-case shapes, as launch_bt_run_packed<HM> and launch_bt_run_case<HM>
template <int HM>
int launch_bt_sweep_packed(const SolveArgs& a, const SweepLaunch& l, hipStream_t stream) {
    return visit_packed<HM>(a, [&](auto v) { return launch_bt_sweep_variant(v, a, l, stream); });
}
template <int HM>
int launch_bt_sweep_case(const SolveArgs& a, const SweepLaunch& l, hipStream_t stream) {
    return visit_case<HM>(a, [&](auto v) { return launch_bt_sweep_variant(v, a, l, stream); });
}

}  // namespace kmpc
