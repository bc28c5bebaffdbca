// kmpc_solve_c3.hip — the BASELINE C3 kernel (H = 10, no short + cost + cap, N < 104: 128 threads,
// the per-asset LDL^T arrays in LDS) in its own translation unit, built at -O2: measured 0.6% ahead
// of -Os for this kernel (bit-identical results), while the 256-thread variant of the constant-case
// unit loses 4% at -O2.
//
// Also the mixed-precision form of this kernel (ipm_mixed_kernel below: a float32 phase, the float64
// finish and the retry in one launch) and the path-persistent backtest kernel of this shape
// (kmpc_bt_run.h, kmpc_backtest_run).
#ifndef KMPC_SCHUR_BCAST_F32   // the Schur LDL^T column in registers, both precisions
#define KMPC_SCHUR_BCAST_F32 1
#endif
#ifndef KMPC_SCHUR_BCAST_F64
#define KMPC_SCHUR_BCAST_F64 1
#endif
#ifndef KMPC_RS_ASM_F32   // the float32 phase's reduce-scatter exchanges written out
#define KMPC_RS_ASM_F32 1
#endif
#ifndef KMPC_TRISOLVE_DPP_F32   // the Schur triangular solves' broadcast inside the FMA
#define KMPC_TRISOLVE_DPP_F32 1
#endif
#ifndef KMPC_TRISOLVE_DPP_F64
#define KMPC_TRISOLVE_DPP_F64 1
#endif
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_run.h"

namespace kmpc {
namespace {
// The mixed pair in one launch: each workgroup runs its window's float32 phase and then its float64
// finish (the window body with PH = 1, then PH = 2: kmpc_ipm_body.inc), one launch tail instead of
// two. The float32 phase's iterate goes to the finish on chip, in registers (hand: each lane's w, s,
// l1..l3 for its asset and the period owners' z4, l4, nu, live across the phase boundary; 12 more
// spilled VGPRs in the finish); only the window's 64 B header (warm flag, float32 iterations)
// goes through args.warm. The other forms this kernel had — the iterate through the 20 KB record in
// HBM or through LDS, the retry as a launch of its own — measured behind and are gone.
// One wave per SIMD: the float32 phase's whole state, cold arrays included, then fits the registers
// without spills (424 of 512): measured against two waves per SIMD with the cold arrays in LDS (87
// spilled VGPRs) — C3 mixed solve 85.8 -> 83.5 ms (tools/ab_mixed.sh).
template <int HM, int MAXT, bool EXACT, int FL, int CS, bool QL, int GL>
__global__ void __launch_bounds__(MAXT) __attribute__((amdgpu_waves_per_eu(1))) ipm_mixed_kernel(SolveArgs args) {
    constexpr int NWM = MAXT / WAVE;
    __shared__ union U {
        Shared<HM, NWM, float> f;
        Shared<HM, NWM, double> d;
    } shu;
    const int b = blockIdx.x;
    if (b >= args.B) return;
    const int yb = b;
    float hand_w[HM], hand_s[HM], hand_l1[HM], hand_l2[HM], hand_l3[HM];
    float hand_z4 = 1.0f, hand_l4 = 0.0f, hand_nu = 0.0f;
    bool hand_flag = false, retry_flag = false;
    Handoff<HM, true> hand{hand_w, hand_s, hand_l1, hand_l2, hand_l3, hand_z4, hand_l4, hand_nu, hand_flag, retry_flag};
    [&]() __attribute__((always_inline)) {
        constexpr int PH = 1;
        using Real = float;
        auto& sh = shu.f;
#include "kmpc_ipm_body.inc"
    }();
    __syncthreads();   // the window's header written; the LDS structure reused
    [&]() __attribute__((always_inline)) {
        constexpr int PH = 2;
        using Real = double;
        auto& sh = shu.d;
#include "kmpc_ipm_body.inc"
    }();
    // a warm start that did not end optimal (about two windows in 65,536 at the default handoff):
    // the retry pass by the window's own workgroup, among the other resident windows, instead of
    // a launch of its own on an otherwise empty GPU
    if (!hand.retry) return;
    __syncthreads();
    [&]() __attribute__((always_inline)) {
        constexpr int PH = 3;
        using Real = double;
        auto& sh = shu.d;
#include "kmpc_ipm_body.inc"
    }();
}
}  // namespace

// 1: the three phases in one launch (ipm_mixed_kernel); 0: the three-launch pair, the iterate through
// the full warm record. The pair is kept because its three standalone kernels, compiled in this
// unit, are part of what fixes ipm_mixed_kernel's instruction stream: without them the compiler
// inlines the unit's device functions in another order and the fused kernel's register allocation
// moves (profiles/dispatch_refactor.md, 1a).
#ifndef KMPC_MIXED_FUSED
#define KMPC_MIXED_FUSED 1
#endif

size_t mixed_warm_floats(int H, int N) { return KMPC_MIXED_FUSED ? (size_t)WARM_HEAD : warm_stride(H, N); }

int launch_ipm_c3(const SolveArgs& a, hipStream_t stream) {
    if (a.warm && KMPC_MIXED_FUSED) {
        const size_t lds = cold_bytes<10, 128, QL_CS, true, 64, 7, double>();
        hipLaunchKernelGGL((ipm_mixed_kernel<10, 128, true, 7, QL_CS, true, 64>), dim3(a.B), dim3(128), lds, stream, a);
        return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
    }
    if (a.warm) {   // mixed precision: the float32 phase, then the float64 finish from its iterates
        int rc = launch_one<10, 128, true, 7, QL_CS, true, 64, 1>(a, stream);
        if (rc == KMPC_OK) rc = launch_one<10, 128, true, 7, QL_CS, true, 64, 2>(a, stream);
        // (the retry of warm starts that did not end optimal: most workgroups exit at once)
        if (rc == KMPC_OK) rc = launch_one<10, 128, true, 7, QL_CS, true, 64, 3>(a, stream);
        return rc;
    }
    return launch_one<10, 128, true, 7, QL_CS, true>(a, stream);
}

template int launch_bt_c3<false>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc

#ifdef KMPC_STATS
extern "C" int kmpc_debug_stats_c3(unsigned long long* out, int reset) { return kmpc::debug_stats_tu(out, reset); }
#endif
