// kmpc_solve.hip — host dispatch of the batched MPC solve (replaces solve_mpc_log_utility,
// mpc.py:27-117): no device code here. One plan (solve_plan) maps a call to its kernel family:
//   simplex presolve (kmpc_solve_simplex.hip): c = tau = 0 without shorting, exact in closed form;
//   ipm_big (kmpc_solve_big.h): the state in a workspace slab, streamed per phase, the Schur matrix
//     on the f64 MFMA — for larger windows (N > 256 or H > 10), which need workspace;
//   ipm_kernel (kmpc_solve_kernel.h): a window's state in the registers of one workgroup, one asset
//     per lane — for N <= 256 assets and H <= 10 periods, in the packed, mixed-precision C3,
//     constant-case and generic forms; each horizon bound HM is instantiated in its own translation
//     unit (kmpc_solve_h*.hip, kmpc_solve_p*.hip), the variant by the ladder of kmpc_solve_args.h.
// A call with a per-asset position limit (kmpc_solve_box, kmpc_solve_box_ws) has two families of its
// own: the box case of the generic ipm_kernel and the box form of ipm_big, at the same shape edges.
// kmpc_solve, kmpc_solve_box(_ws) and their workspace queries consume the plan; kmpc_backtest_run and
// kmpc_backtest_sweep and their box forms read from it whether a path-persistent kernel runs the
// body of the kernel the solve would pick.
#include <type_traits>

#include "kmpc_internal.h"
#include "kmpc_solve_args.h"

namespace kmpc {

namespace {

// float32 -> float64 handoff of the mixed-precision pair. Measured on the oracle's iteration
// (tools/f32phase_probe.py, 512 C3 windows of the bench's distribution: float32 to mu <= 5e-5 takes
// 7.9 of the 15.9 iterations, every window optimal, float64 finish 8.0 iterations; 2e-5 left 1% of
// the windows optimal_inaccurate) and on MI355X (tools/ab_mixed.sh, 65,536 windows, retry pass in:
// bench yhat 83.3 ms at 1e-4, 82.0 ms at 5e-5; random yhat 91.1 / 90.7 ms, same statuses as float64).
// 3e-5 since round 6's step / sigma rules (tools/gpu_r6v.sh, twice: bench yhat 74.80 / 74.70 ms at
// 5e-5, 74.43 / 74.24 at 3e-5, 74.11 / 73.94 at 2e-5; random yhat 77.92 / 77.75, 77.64 / 77.45,
// 78.88 / 78.69 — 2e-5 loses on random yhat; statuses as float64 at every threshold)
constexpr double MU_HANDOFF = 3e-5;

// max_weight: the active per-asset position limit the caller (kmpc_capi.hip) has validated (no short,
// 1 / N < max_weight < 1), or 0.0 for none — here and in every function below that takes it
SolveArgs make_args(const kmpc_solve_desc* d, double max_weight) {
    SolveArgs a;
    a.B = d->B; a.N = d->N; a.H = d->H;
    a.c = d->cost_coeff;
    a.tau = d->max_turnover > 0.0 ? d->max_turnover : 0.0;
    a.allow_short = d->allow_short;
    a.max_iter = d->max_iter > 0 ? d->max_iter : 80;
    a.tol = d->tol > 0.0 ? d->tol : 1e-9;
    a.return_full = d->return_full_W;
    a.n_refine = d->n_refine > 0 ? d->n_refine : (d->n_refine < 0 ? 0 : 3);
    a.path = d->path;
    a.warm = nullptr;
    a.warm_floats = 0;
    a.mu_handoff = d->mu_handoff > 0.0 ? d->mu_handoff : MU_HANDOFF;
    // (the limit shares mu_handoff's slot: the box kernels have no float32 phase, and the large-window
    // kernel does not read the handoff)
    if (max_weight > 0.0) a.max_weight = max_weight;
    return a;
}

// per-call solver path (kmpc_solve_desc.path): KMPC_PATH_AUTO by shape, KMPC_PATH_REGISTER =
// interior point in the register kernels whenever they support the shape (no presolve),
// KMPC_PATH_LARGE = the large-window kernel, KMPC_PATH_REGISTER_UNPACKED = the register kernels
// with one window per wave even for small windows (no lane-group packing, no presolve); AUTO and
// REGISTER pack small windows (pack_small: AUTO from KMPC_PACK_MIN_B windows, REGISTER always)
bool simplex_case(const SolveArgs& a) {
    return a.path == KMPC_PATH_AUTO && !(a.c > 0.0) && !(a.tau > 0.0) && !a.allow_short;
}

bool use_big(const SolveArgs& a) {
    if (a.path == KMPC_PATH_REGISTER || a.path == KMPC_PATH_REGISTER_UNPACKED) return false;
    if (a.path == KMPC_PATH_LARGE) return true;
    // measured on MI355X (tools/path_ab.py): the register kernels win up to 256 assets at
    // H <= 10 (N = 192: 76k vs 41k windows/s); the large-window kernel wins past 10 periods at any
    // N (N = 100, H = 20: 36k vs 24k) and past 256 assets (N = 500, H = 10: 23k vs 13k)
    return a.N > 256 || a.H > 10;
}

// Lane-group packing of small windows (N <= 32: 2-4 windows per wave) is a throughput layout. For
// a batch that cannot fill the GPU a window's latency decides, and one window per wave is faster:
// AUTO packs only from KMPC_PACK_MIN_B (include/kmpc.h) windows per call (H > 2), or at any batch
// size for H <= 2.
// Measured (tools/pack_cross_probe.py, solve only, packed / one-per-wave ms): N = 10, H = 5:
// B = 256 0.341 / 0.292, 1,024 0.361 / 0.342, 2,048 0.374 / 0.426, 65,536 3.41 / 9.08; N = 20,
// H = 10: B = 256 0.965 / 0.774, 1,024 1.03 / 1.39; N = 8, H = 2: packed ahead at every B. In the
// path-persistent backtest (P = 64, N = 10, H = 5): 0.297 -> 0.239 ms per step.
bool pack_small(const SolveArgs& a) {
    if (a.path == KMPC_PATH_REGISTER_UNPACKED || a.N > 32 || a.H > 10) return false;
    return a.path != KMPC_PATH_AUTO || a.B > KMPC_PACK_MIN_B || a.H <= 2;
}

// The mixed-precision pair exists for the C3 rung of the ladder. AUTO takes it from KMPC_MIXED_MIN_B
// windows: below it a launch is latency-bound (the slowest window's iterations), and float64 alone
// measured faster — lock-step backtest, C3 model, path-steps/s (tools/lockstep_probe.py): P = 64
// 53.7 k mixed vs 56.1 k float64, P = 256 191 k vs 206 k, P = 1,024 404 k vs 430 k, P = 4,096 539 k
// vs 513 k
bool mixed_precision(const SolveArgs& a, int precision) {
    return precision == KMPC_PRECISION_MIXED || (precision == KMPC_PRECISION_AUTO && a.B >= KMPC_MIXED_MIN_B);
}

// f(the horizon bound HM, as an integral_constant) of the unit whose kernels run H periods
template <class F>
int by_horizon(int H, F&& f) {
    if (H <= 2) return f(std::integral_constant<int, 2>{});
    if (H <= 5) return f(std::integral_constant<int, 5>{});
    if (H <= 10) return f(std::integral_constant<int, 10>{});
    return KMPC_ERR_UNSUPPORTED;   // H > 10: the large-window kernel
}

// BOX, LARGE_BOX: the two families of a call with a position limit; NONE: no kernel runs it
enum class Family { SIMPLEX, LARGE, PACKED, MIXED_C3, CASE, GENERIC, BOX, LARGE_BOX, NONE };
struct Plan {
    Family family;
    // PACKED, CASE: the rung is the C3 one, and the path-persistent backtest kernels have a form of
    // it (float64, case 7, H = HM: launch_bt_variant; one step's W0 only). BOX: persistent past the
    // packed shapes (N > 32: the box case has no packed form), at every H, one step's W0 only
    // (launch_bt_box)
    bool c3 = false, persistent = false;
};

// The kernel family kmpc_solve runs a call on, for the precision asked (kmpc_solve_desc.precision),
// and under a limit the family of kmpc_solve_box / kmpc_solve_box_ws
Plan solve_plan(const SolveArgs& a, int precision, double max_weight) {
    Plan p{Family::GENERIC};
    if (max_weight > 0.0) {
        // One family per side at every batch size, float64 only: no presolve (the capped simplex has
        // no closed form here), no packing, no mixed pair. The box case of the generic register
        // kernels (launch_ipm_box, no workspace) where the register kernels run; elsewhere the box
        // form of the large-window kernel (big_box_launch), which the register paths cannot ask for.
        if (precision == KMPC_PRECISION_MIXED) return Plan{Family::NONE};
        if (a.N <= 256 && a.H <= 10 && a.path != KMPC_PATH_LARGE) {
            p.family = Family::BOX;
            p.persistent = a.N > 32 && !a.return_full;
            return p;
        }
        const bool reg = a.path == KMPC_PATH_REGISTER || a.path == KMPC_PATH_REGISTER_UNPACKED;
        return Plan{reg ? Family::NONE : Family::LARGE_BOX};
    }
    if (simplex_case(a)) return Plan{Family::SIMPLEX};
    if (use_big(a)) return Plan{Family::LARGE};
    const auto rung = [&](auto v) -> int {
        using V = decltype(v);
        p.c3 = V::C3;
        p.persistent = V::FL == 7 && V::EXACT && !a.return_full;
        return KMPC_OK;
    };
    // N <= 32: several windows per wave on lane groups (every such shape has a packed rung today; a
    // shape without one goes on to one window per wave)
    if (pack_small(a) && by_horizon(a.H, [&](auto hm) { return visit_packed<decltype(hm)::value>(a, rung); }) == KMPC_OK) {
        p.family = Family::PACKED;
        return p;
    }
    // H == 5 / 10 with N <= 128 in the two common constraint cases (case 7: N <= 256):
    // constant-case kernels, and on the C3 rung the float32 phase + float64 finish
    if ((a.H == 10 && visit_case<10>(a, rung) == KMPC_OK) || (a.H == 5 && visit_case<5>(a, rung) == KMPC_OK)) {
        p.family = Family::CASE;
        if (p.c3 && mixed_precision(a, precision)) p = Plan{Family::MIXED_C3};
    }
    return p;
}

// Windows per launch: one workgroup of up to 256 threads per window (the register kernels), so a
// grid of at most 2^22 stays below a dispatch's 2^32 work-items; larger batches go as equal launches
// of at most LAUNCH_MAX_B windows: each is past every batch threshold (KMPC_MIXED_MIN_B,
// KMPC_PACK_MIN_B), so AUTO takes the same kernels as for the whole batch.
constexpr int LAUNCH_MAX_B = 1 << 22;
struct SolveIO {
    const float* yhat;
    const double* w_prev;
    double *w_out;
    int* status;
    double* obj;
    int* iters;
};
// launch(desc of one launch, its windows' arrays, whether it is the first)
template <class F>
int for_each_launch(const kmpc_solve_desc* d, const SolveIO& io, F&& launch) {
    if (d->B <= LAUNCH_MAX_B) return launch(*d, io, true);
    const int nch = (int)(((size_t)d->B + LAUNCH_MAX_B - 1) / LAUNCH_MAX_B);
    const int per = (int)(((size_t)d->B + nch - 1) / nch);
    const size_t HN = (size_t)d->H * d->N, wo = d->return_full_W ? HN : (size_t)d->N;
    kmpc_solve_desc c = *d;
    for (int b0 = 0; b0 < d->B; b0 += per) {
        c.B = d->B - b0 < per ? d->B - b0 : per;
        const SolveIO s = {io.yhat + (size_t)b0 * HN, io.w_prev + (size_t)b0 * d->N, io.w_out + (size_t)b0 * wo,
                           io.status + b0, io.obj + b0, io.iters ? io.iters + b0 : nullptr};
        const int rc = launch(c, s, b0 == 0);
        if (rc != KMPC_OK) return rc;
    }
    return KMPC_OK;
}

SolveArgs make_args(const kmpc_solve_desc& d, double max_weight, const SolveIO& io) {
    SolveArgs a = make_args(&d, max_weight);
    a.yhat = io.yhat; a.wp = io.w_prev; a.wout = io.w_out; a.status = io.status; a.obj = io.obj; a.iters = io.iters;
    a.trace = nullptr;
    return a;
}

// One warm record per window of the mixed pair: its 64 B header alone with the fused kernel (the
// whole batch in one launch), else the full record, in chunks of at most WARM_CHUNK windows.
constexpr int WARM_CHUNK = 131072;
int warm_chunk(const SolveArgs& a) {
    const int cap = mixed_warm_floats(a.H, a.N) == (size_t)WARM_HEAD ? LAUNCH_MAX_B : WARM_CHUNK;
    return a.B < cap ? a.B : cap;
}
size_t warm_bytes(const SolveArgs& a) { return sizeof(float) * mixed_warm_floats(a.H, a.N) * (size_t)warm_chunk(a); }

// the mixed pair (float32 phase + float64 finish), chunk by chunk
int mixed_launch(const SolveArgs& a, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!ws || ws_bytes < warm_bytes(a)) return KMPC_ERR_WORKSPACE;
    SolveArgs c = a;
    c.warm = (float*)ws;
    c.warm_floats = mixed_warm_floats(a.H, a.N);
    const size_t HN = (size_t)a.H * a.N;
    const int chunk = warm_chunk(a);
    for (int b0 = 0; b0 < a.B; b0 += chunk) {
        c.B = a.B - b0 < chunk ? a.B - b0 : chunk;
        c.yhat = a.yhat + (size_t)b0 * HN;
        c.wp = a.wp + (size_t)b0 * a.N;
        c.wout = a.wout + (size_t)b0 * (a.return_full ? HN : (size_t)a.N);
        c.status = a.status + b0;
        c.obj = a.obj + b0;
        c.iters = a.iters ? a.iters + b0 : nullptr;
        c.trace = b0 == 0 ? a.trace : nullptr;
        const int rc = launch_ipm_c3(c, stream);
        if (rc != KMPC_OK) return rc;
    }
    return KMPC_OK;
}

}  // namespace

BoxFamily box_family(const kmpc_solve_desc* d, double max_weight) {
    switch (solve_plan(make_args(d, max_weight), d->precision, max_weight).family) {
        case Family::BOX: return BoxFamily::REGISTER;
        case Family::LARGE_BOX: return BoxFamily::LARGE;
        default: return BoxFamily::NONE;
    }
}

size_t solve_workspace_bytes(const kmpc_solve_desc* d, double max_weight) {
    if (!d || d->B <= 0) return 0;
    const SolveArgs a = make_args(d, max_weight);
    switch (solve_plan(a, d->precision, max_weight).family) {
        case Family::LARGE: return big_ws_bytes(a);
        case Family::LARGE_BOX: return big_box_ws_bytes(a);   // two more slab arrays
        case Family::MIXED_C3: return warm_bytes(a);
        default: return 0;
    }
}

int solve_launch(const kmpc_solve_desc* d, double max_weight, const float* yhat, const double* w_prev,
                 double* w_out, int* status, double* obj, int* iters, void* ws, size_t ws_bytes,
                 hipStream_t stream, double* trace) {
    const SolveIO io = {yhat, w_prev, w_out, status, obj, iters};
    return for_each_launch(d, io, [&](const kmpc_solve_desc& c, const SolveIO& s, bool first) -> int {
        SolveArgs a = make_args(c, max_weight, s);
        a.trace = first ? trace : nullptr;
        if (a.B == 0) return KMPC_OK;
        switch (solve_plan(a, c.precision, max_weight).family) {
            case Family::SIMPLEX: return simplex_launch(a, stream);
            case Family::LARGE: return big_launch(a, ws, ws_bytes, stream);
            case Family::PACKED:
                return by_horizon(a.H, [&](auto hm) { return launch_ipm_packed<decltype(hm)::value>(a, stream); });
            case Family::MIXED_C3: return mixed_launch(a, ws, ws_bytes, stream);
            case Family::CASE: return a.H == 10 ? launch_ipm_case<10>(a, stream) : launch_ipm_case<5>(a, stream);
            case Family::BOX:
                return by_horizon(a.H, [&](auto hm) { return launch_ipm_box<decltype(hm)::value>(a, stream); });
            // (one launch per LAUNCH_MAX_B windows over the same slabs: the launches are ordered on the stream)
            case Family::LARGE_BOX: return big_box_launch(a, ws, ws_bytes, stream);
            case Family::NONE: return KMPC_ERR_UNSUPPORTED;
            case Family::GENERIC: break;
        }
        return by_horizon(a.H, [&](auto hm) { return launch_ipm<decltype(hm)::value>(a, stream); });
    });
}

// kmpc_backtest_run (n_cfg = 0) and kmpc_backtest_sweep (n_cfg >= 1 configs over the same bd->P
// paths), one launch of the path-persistent kernel (kmpc_bt_run.h) in its run or sweep form. The
// kernel exists where kmpc_solve sends the batch of sd->B windows (the caller has set it: P for the
// run, n_cfg P for the sweep) to a float64 constant-case register kernel of case 7 (no short, cost
// and cap): H = 10 or 5 with 32 < N <= 256, one window per workgroup, and the packed N <= 32 kernels
// with H = 2, 5 or 10, one work item per lane group — not the mixed pair. It runs that kernel's
// window body, so the steps match it. The run plans with the caller's precision, cost_coeff and
// max_turnover. The sweep's parameters are device arrays, so the constraint case cannot depend on
// them: always the constant case 7 (the caller has set sd's cost_coeff and max_turnover to it) in
// float64 — no mixed pair at any batch size, and none to ask for.
// With a position limit (kmpc_backtest_run_box, kmpc_backtest_sweep_box) every step's solve is
// kmpc_solve_box's, the window body that of the box kernel it runs for the shape (launch_bt_box);
// the sweep's constraint case is read at run time there (the generic kernel).
int backtest_launch(const kmpc_backtest_desc* bd, const kmpc_solve_desc* sd, double max_weight, int n_cfg,
                    const BtLaunch& l, double* target, int* status, double* obj, hipStream_t stream) {
    const bool sweep = n_cfg > 0;
    SolveArgs a = make_args(sd, max_weight);
    if (sweep && sd->precision == KMPC_PRECISION_MIXED) return KMPC_ERR_UNSUPPORTED;
    // (the kernel kmpc_solve, or under a limit kmpc_solve_box, picks for this batch)
    const Plan p = solve_plan(a, sweep ? KMPC_PRECISION_F64 : sd->precision, max_weight);
    if (!p.persistent) return KMPC_ERR_UNSUPPORTED;
    if (bd->P == 0 || l.n_steps == 0) return KMPC_OK;
    a.wout = target; a.status = status; a.obj = obj; a.iters = nullptr; a.trace = nullptr;
    a.yhat = l.yhat; a.wp = l.weights;
    const auto run = [&](auto sw) {
        constexpr bool SW = decltype(sw)::value;
        if (p.family == Family::BOX)
            return by_horizon(a.H, [&](auto hm) { return launch_bt_box<decltype(hm)::value, SW>(a, l, stream); });
        if (p.family == Family::PACKED)
            return by_horizon(a.H, [&](auto hm) { return launch_bt_packed<decltype(hm)::value, SW>(a, l, stream); });
        if (p.c3) return launch_bt_c3<SW>(a, l, stream);
        return a.H == 5 ? launch_bt_case<5, SW>(a, l, stream) : launch_bt_case<10, SW>(a, l, stream);
    };
    return sweep ? run(std::true_type{}) : run(std::false_type{});
}

}  // namespace kmpc
