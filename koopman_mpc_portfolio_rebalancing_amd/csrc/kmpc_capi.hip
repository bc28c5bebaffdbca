// kmpc_capi.hip — the extern "C" boundary of libkmpc.so (declared in include/kmpc.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kmpc_internal.h"
#include "kmpc_solve_args.h"

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int check_solve(const kmpc_solve_desc* d) {
    if (!d) return KMPC_ERR_INVALID;
    if (d->B < 0 || d->N < 1 || d->H < 1) return KMPC_ERR_INVALID;
    if (d->N > KMPC_MAX_N || d->H > KMPC_MAX_H) return KMPC_ERR_UNSUPPORTED;
    if (d->H > 21) return KMPC_ERR_UNSUPPORTED;   // Schur system (3H) must fit one wavefront
    // c < 0 makes -c ||dw||_1 concave in the maximization: not DCP, cvxpy raises (mpc.py:66-103)
    if (d->cost_coeff < 0.0) return KMPC_ERR_INVALID;
    if (d->path < KMPC_PATH_AUTO || d->path > KMPC_PATH_REGISTER_UNPACKED) return KMPC_ERR_INVALID;
    if (d->precision < KMPC_PRECISION_AUTO || d->precision > KMPC_PRECISION_MIXED) return KMPC_ERR_INVALID;
    if (!(d->mu_handoff < 1.0)) return KMPC_ERR_INVALID;   // (NaN too)
    return KMPC_OK;
}

// The argument checks kmpc_backtest_run (the batch is the paths), kmpc_backtest_sweep (the batch is
// configs x paths; the configs carry c and tau, sdesc's are not read) and their box forms share. l: the
// caller's arguments; P, S and cost come from desc. sd: the solve descriptor of the launch's batch.
int backtest_check(bool sweep, const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, int n_cfg,
                   kmpc::BtLaunch& l, const double* target, const int* status, const double* obj, kmpc_solve_desc& sd) {
    if (!desc || !sdesc || desc->P < 0 || desc->N < 1 || desc->S < 1 || l.step0 < 0 || l.n_steps < 0 ||
        l.step0 + l.n_steps > desc->S || l.n_real < 0 || l.n_real > l.n_steps || sdesc->N != desc->N)
        return KMPC_ERR_INVALID;
    if (sweep && (n_cfg < 1 || (long long)n_cfg * desc->P > 0x7fffffffLL)) return KMPC_ERR_INVALID;
    sd = *sdesc;
    sd.B = sweep ? n_cfg * desc->P : desc->P;
    if (sweep) {
        sd.cost_coeff = 0.0;
        sd.max_turnover = 1.0;
    }
    const int rc = check_solve(&sd);
    if (rc) return rc;
    if (desc->P > 0 && l.n_steps > 0 &&
        (!l.yhat || !l.weights || !l.value || !l.hist || !target || !status || !obj || (l.n_real > 0 && !l.realized) ||
         (sweep && (!l.mpc_cost || !l.max_turnover || !l.bt_cost))))
        return KMPC_ERR_INVALID;
    l.P = desc->P; l.S = desc->S; l.cost = desc->cost_coeff;
    return KMPC_OK;
}

// The position limit's own rule for the log-utility solve family (kmpc_solve_box, kmpc_solve_box_ws and
// its workspace query, kmpc_backtest_run_box / _sweep_box), after the descriptor's checks: an error
// code; or KMPC_OK with u = 0.0, an inactive bound (the plain entry runs); or KMPC_OK with the active
// limit u. Which kernel family runs an active limit is the plan's answer (kmpc::box_family).
// The one input this rule and mv_box_limit answer differently is allow_short with N * max_weight <= 1:
// INVALID here (the empty set is found first), UNSUPPORTED there.
int box_limit(const kmpc_solve_desc& d, double max_weight, double& u) {
    u = 0.0;
    if (!(max_weight > 0.0)) return KMPC_ERR_INVALID;                   // (NaN too)
    if (max_weight >= 1.0 && !d.allow_short) return KMPC_OK;            // an inactive bound
    if (!((double)d.N * max_weight > 1.0)) return KMPC_ERR_INVALID;     // empty set or a single point
    if (d.allow_short) return KMPC_ERR_UNSUPPORTED;
    u = max_weight;
    return KMPC_OK;
}

// ... and for the mean-variance pair (kmpc_solve_mv_box; kmpc_markowitz_run / _sweep, where a
// max_weight of 0 means none and does not come here), with the same three answers. Its order is its
// own, shorting before the inactive bound: allow_short with N * max_weight <= 1 is UNSUPPORTED here
// and INVALID in box_limit, and allow_short with max_weight >= 1 is UNSUPPORTED here, inactive there.
int mv_box_limit(const kmpc_mv_desc& d, double max_weight, double& u) {
    u = 0.0;
    if (!(max_weight > 0.0)) return KMPC_ERR_INVALID;                   // (NaN too)
    if (d.allow_short) return KMPC_ERR_UNSUPPORTED;
    if (max_weight >= 1.0) return KMPC_OK;                              // an inactive bound
    if (!((double)d.N * max_weight > 1.0)) return KMPC_ERR_INVALID;     // empty set or a single point
    u = max_weight;
    return KMPC_OK;
}

// The four kmpc_backtest_* entries; max_weight is null for the plain two. Every rule is decided before
// any launch, the limit's (box_limit) before the P == 0 / n_steps == 0 return; an inactive bound IS the
// plain call. Under a limit the plan has a persistent kernel for 32 < N <= 256, H <= 10, float64, W0
// only, path != LARGE (N <= 32 has no box form: those shapes' persistent kernels are the packed ones).
int backtest_entry(bool sweep, const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, const double* max_weight,
                   int n_cfg, kmpc::BtLaunch l, double* target, int* status, double* obj, void* stream) {
    kmpc_solve_desc sd;
    int rc = backtest_check(sweep, desc, sdesc, n_cfg, l, target, status, obj, sd);
    if (rc) return rc;
    double u = 0.0;
    if (max_weight && (rc = box_limit(sd, *max_weight, u))) return rc;
    return kmpc::backtest_launch(desc, &sd, u, sweep ? n_cfg : 0, l, target, status, obj, (hipStream_t)stream);
}

// the caller's arrays of a kmpc_backtest_* entry (P, S and cost: backtest_check)
kmpc::BtLaunch bt_args(int step0, int n_steps, const float* yhat, const float* realized, int n_real, double* weights,
                       double* value, double* hist, const double* mpc_cost = nullptr,
                       const double* max_turnover = nullptr, const double* bt_cost = nullptr) {
    return {/* P */ 0, n_steps, n_real, step0, /* S, cost */ 0, 0.0, mpc_cost, max_turnover, bt_cost,
            yhat, realized, weights, value, hist};
}

}  // namespace

extern "C" {

const char* kmpc_version(void) { return "kmpc 0.7.0 (gfx950)"; }

const char* kmpc_strerror(int code) {
    switch (code) {
        case KMPC_OK: return "ok";
        case KMPC_ERR_INVALID: return "invalid argument";
        case KMPC_ERR_UNSUPPORTED: return "unsupported shape";
        case KMPC_ERR_WORKSPACE: return "workspace too small";
        case KMPC_ERR_LAUNCH: return "HIP launch failed";
        case 100 + KMPC_STATUS_OPTIMAL: return "optimal";
        case 100 + KMPC_STATUS_OPTIMAL_INACCURATE: return "optimal_inaccurate";
        case 100 + KMPC_STATUS_INFEASIBLE: return "infeasible";
        case 100 + KMPC_STATUS_UNBOUNDED: return "unbounded";
        case 100 + KMPC_STATUS_SOLVER_ERROR: return "solver_error";
        default: return "unknown";
    }
}

size_t kmpc_workspace_bytes(const kmpc_rollout_desc* rdesc, const kmpc_solve_desc* sdesc) {
    size_t bytes = 0;
    if (rdesc) bytes += kmpc::rollout_workspace_bytes(rdesc);
    if (rdesc && sdesc) bytes += align256(sizeof(float) * (size_t)rdesc->B * rdesc->H * rdesc->N);
    if (sdesc && check_solve(sdesc) == KMPC_OK) bytes += align256(kmpc::solve_workspace_bytes(sdesc, 0.0));
    return bytes;
}

int kmpc_solve(const kmpc_solve_desc* desc, const float* yhat, const double* w_prev, double* w_out,
               int* status, double* obj, int* iters, void* workspace, size_t ws_bytes,
               void* stream) {
    int rc = check_solve(desc);
    if (rc) return rc;
    if (desc->B == 0) return KMPC_OK;
    if (!yhat || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    if (ws_bytes < kmpc::solve_workspace_bytes(desc, 0.0)) return KMPC_ERR_WORKSPACE;
    return kmpc::solve_launch(desc, 0.0, yhat, w_prev, w_out, status, obj, iters, workspace, ws_bytes,
                              (hipStream_t)stream);
}

// The three limited solve entries decide every rule before any launch (and before the B == 0 return):
// the descriptor, the limit (box_limit), then the family the plan names for an active limit.
int kmpc_solve_box(const kmpc_solve_desc* desc, double max_weight, const float* yhat, const double* w_prev,
                   double* w_out, int* status, double* obj, int* iters, void* stream) {
    int rc = check_solve(desc);
    if (rc) return rc;
    double u;
    if ((rc = box_limit(*desc, max_weight, u))) return rc;
    // an inactive bound: the plain solve, without a workspace (KMPC_ERR_WORKSPACE if it needs one)
    if (u == 0.0) return kmpc_solve(desc, yhat, w_prev, w_out, status, obj, iters, nullptr, 0, stream);
    // (the large family needs the workspace only kmpc_solve_box_ws can hand over)
    if (kmpc::box_family(desc, u) != kmpc::BoxFamily::REGISTER) return KMPC_ERR_UNSUPPORTED;
    if (desc->B == 0) return KMPC_OK;
    if (!yhat || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::solve_launch(desc, u, yhat, w_prev, w_out, status, obj, iters, nullptr, 0, (hipStream_t)stream);
}

size_t kmpc_solve_box_workspace_bytes(const kmpc_solve_desc* desc, double max_weight) {
    double u;
    if (check_solve(desc) || box_limit(*desc, max_weight, u)) return 0;
    if (u == 0.0) return kmpc_workspace_bytes(nullptr, desc);
    return kmpc::solve_workspace_bytes(desc, u);   // (0 for the register family, and for none)
}

int kmpc_solve_box_ws(const kmpc_solve_desc* desc, double max_weight, const float* yhat, const double* w_prev,
                      double* w_out, int* status, double* obj, int* iters, void* workspace, size_t ws_bytes,
                      void* stream) {
    int rc = check_solve(desc);
    if (rc) return rc;
    double u;
    if ((rc = box_limit(*desc, max_weight, u))) return rc;
    if (u == 0.0) return kmpc_solve(desc, yhat, w_prev, w_out, status, obj, iters, workspace, ws_bytes, stream);
    switch (kmpc::box_family(desc, u)) {
        case kmpc::BoxFamily::NONE: return KMPC_ERR_UNSUPPORTED;
        case kmpc::BoxFamily::REGISTER:
            return kmpc_solve_box(desc, max_weight, yhat, w_prev, w_out, status, obj, iters, stream);
        case kmpc::BoxFamily::LARGE: break;
    }
    if (!workspace || ws_bytes < kmpc::solve_workspace_bytes(desc, u)) return KMPC_ERR_WORKSPACE;
    if (desc->B == 0) return KMPC_OK;
    if (!yhat || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::solve_launch(desc, u, yhat, w_prev, w_out, status, obj, iters, workspace, ws_bytes,
                              (hipStream_t)stream);
}

/* Debug entry (not part of include/kmpc.h): kmpc_solve plus a per-iteration trace of problem 0,
   trace[4 * it + {0,1,2,3}] = (mu, dual residual, primal residual, step length). */
int kmpc_solve_trace(const kmpc_solve_desc* desc, const float* yhat, const double* w_prev,
                     double* w_out, int* status, double* obj, int* iters, double* trace,
                     void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_solve(desc);
    if (rc) return rc;
    if (desc->B == 0) return KMPC_OK;
    if (ws_bytes < kmpc::solve_workspace_bytes(desc, 0.0)) return KMPC_ERR_WORKSPACE;
    return kmpc::solve_launch(desc, 0.0, yhat, w_prev, w_out, status, obj, iters, workspace, ws_bytes,
                              (hipStream_t)stream, trace);
}

int kmpc_rollout(const kmpc_rollout_desc* desc, const float* obs, float* yhat, void* workspace,
                 size_t ws_bytes, void* stream) {
    return kmpc::rollout_launch(desc, obs, yhat, workspace, ws_bytes, (hipStream_t)stream);
}

int kmpc_window(const kmpc_rollout_desc* rdesc, const kmpc_solve_desc* sdesc, const float* obs,
                const double* w_prev, float* yhat, double* w_out, int* status, double* obj,
                int* iters, void* workspace, size_t ws_bytes, void* stream) {
    if (!rdesc || !sdesc) return KMPC_ERR_INVALID;
    int rc = check_solve(sdesc);
    if (rc) return rc;
    if (rdesc->B != sdesc->B || rdesc->N != sdesc->N || rdesc->H != sdesc->H) return KMPC_ERR_INVALID;
    if (ws_bytes < kmpc_workspace_bytes(rdesc, sdesc)) return KMPC_ERR_WORKSPACE;
    const size_t rbytes = kmpc::rollout_workspace_bytes(rdesc);
    const size_t ybytes = align256(sizeof(float) * (size_t)rdesc->B * rdesc->H * rdesc->N);
    float* y = yhat ? yhat : (float*)((char*)workspace + rbytes);
    rc = kmpc::rollout_launch(rdesc, obs, y, workspace, rbytes, (hipStream_t)stream);
    if (rc) return rc;
    if (sdesc->B == 0) return KMPC_OK;
    return kmpc::solve_launch(sdesc, 0.0, y, w_prev, w_out, status, obj, iters, (char*)workspace + rbytes + ybytes,
                              ws_bytes - rbytes - ybytes, (hipStream_t)stream);
}

int kmpc_gross_returns(size_t n, const float* yhat, float* R, void* stream) {
    if (n == 0) return KMPC_OK;
    if (!yhat || !R) return KMPC_ERR_INVALID;
    return kmpc::gross_returns_launch(n, yhat, R, (hipStream_t)stream);
}

}  // extern "C"

extern "C" {

int kmpc_backtest_step(const kmpc_backtest_desc* desc, int step, const double* target,
                       const float* realized_next, double* weights, double* value, double* hist,
                       void* stream) {
    if (!desc || desc->P < 0 || desc->N < 1 || desc->S < 1 || step < 0 || step >= desc->S)
        return KMPC_ERR_INVALID;
    if (desc->P > 0 && (!target || !weights || !value || !hist)) return KMPC_ERR_INVALID;
    return kmpc::backtest_step_launch(desc, step, target, realized_next, weights, value, hist,
                                      (hipStream_t)stream);
}

int kmpc_backtest_run(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, int step0, int n_steps,
                      const float* yhat, const float* realized, int n_real, double* weights, double* value,
                      double* hist, double* target, int* status, double* obj, void* stream) {
    return backtest_entry(false, desc, sdesc, nullptr, 0, bt_args(step0, n_steps, yhat, realized, n_real, weights, value, hist),
                          target, status, obj, stream);
}

int kmpc_backtest_sweep(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, int n_cfg,
                        const double* mpc_cost, const double* max_turnover, const double* bt_cost, int step0,
                        int n_steps, const float* yhat, const float* realized, int n_real, double* weights,
                        double* value, double* hist, double* target, int* status, double* obj, void* stream) {
    return backtest_entry(true, desc, sdesc, nullptr, n_cfg,
                          bt_args(step0, n_steps, yhat, realized, n_real, weights, value, hist, mpc_cost, max_turnover, bt_cost),
                          target, status, obj, stream);
}

int kmpc_backtest_run_box(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, double max_weight, int step0,
                          int n_steps, const float* yhat, const float* realized, int n_real, double* weights,
                          double* value, double* hist, double* target, int* status, double* obj, void* stream) {
    return backtest_entry(false, desc, sdesc, &max_weight, 0, bt_args(step0, n_steps, yhat, realized, n_real, weights, value, hist),
                          target, status, obj, stream);
}

int kmpc_backtest_sweep_box(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, double max_weight, int n_cfg,
                            const double* mpc_cost, const double* max_turnover, const double* bt_cost, int step0,
                            int n_steps, const float* yhat, const float* realized, int n_real, double* weights,
                            double* value, double* hist, double* target, int* status, double* obj, void* stream) {
    return backtest_entry(true, desc, sdesc, &max_weight, n_cfg,
                          bt_args(step0, n_steps, yhat, realized, n_real, weights, value, hist, mpc_cost, max_turnover, bt_cost),
                          target, status, obj, stream);
}

int kmpc_standardize(int T, int N, const double* log_returns, const double* mean, const double* std,
                     float* z, void* stream) {
    if (T < 0 || N < 1) return KMPC_ERR_INVALID;
    if ((size_t)T * N > 0 && (!log_returns || !mean || !std || !z)) return KMPC_ERR_INVALID;
    return kmpc::standardize_launch(T, N, log_returns, mean, std, z, (hipStream_t)stream);
}

int kmpc_backtest_metrics(const kmpc_backtest_desc* desc, const double* hist, double* metrics,
                          void* stream) {
    if (!desc || desc->P < 0 || desc->S < 0) return KMPC_ERR_INVALID;
    if (desc->P > 0 && (!hist || !metrics)) return KMPC_ERR_INVALID;
    return kmpc::backtest_metrics_launch(desc, hist, metrics, (hipStream_t)stream);
}

}  // extern "C"

extern "C" {

int kmpc_solve_mv(const kmpc_mv_desc* desc, const double* mu, const double* sigma, size_t sigma_stride,
                  const double* w_prev, double* w_out, int* status, double* obj, int* iters,
                  void* stream) {
    return kmpc_solve_mv_ws(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, nullptr, 0,
                            stream);
}

size_t kmpc_mv_workspace_bytes(const kmpc_mv_desc* desc) { return kmpc::mv_workspace_bytes(desc); }

int kmpc_solve_mv_ws(const kmpc_mv_desc* desc, const double* mu, const double* sigma, size_t sigma_stride,
                     const double* w_prev, double* w_out, int* status, double* obj, int* iters,
                     void* workspace, size_t ws_bytes, void* stream) {
    if (!desc || desc->B < 0 || desc->N < 1 || desc->H < 1) return KMPC_ERR_INVALID;
    if (desc->H > KMPC_MV_MAX_H || desc->N * desc->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (desc->B == 0) return KMPC_OK;
    if (!mu || !sigma || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::mv_solve_launch(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, workspace,
                                 ws_bytes, (hipStream_t)stream);
}

int kmpc_solve_mv_box(const kmpc_mv_desc* desc, double max_weight, const double* mu, const double* sigma,
                      size_t sigma_stride, const double* w_prev, double* w_out, int* status, double* obj,
                      int* iters, void* workspace, size_t ws_bytes, void* stream) {
    // every rule is decided before any launch (and before the B == 0 return): the descriptor as
    // kmpc_solve_mv_ws, then the limit in mv_box_limit's order (not kmpc_solve_box's)
    if (!desc || desc->B < 0 || desc->N < 1 || desc->H < 1) return KMPC_ERR_INVALID;
    if (desc->H > KMPC_MV_MAX_H || desc->N * desc->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    double u;
    const int rc = mv_box_limit(*desc, max_weight, u);
    if (rc) return rc;
    if (u == 0.0)   // an inactive bound: the plain solve
        return kmpc_solve_mv_ws(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, workspace,
                                ws_bytes, stream);
    if (desc->B == 0) return KMPC_OK;
    if (!mu || !sigma || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::mv_solve_launch(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, workspace,
                                 ws_bytes, (hipStream_t)stream, u);
}

size_t kmpc_mv_cap_workspace_bytes(const kmpc_mv_desc* desc) { return kmpc::mv_cap_workspace_bytes(desc); }

int kmpc_solve_mv_cap(const kmpc_mv_desc* desc, double max_weight, double max_turnover, const double* mu,
                      const double* sigma, size_t sigma_stride, const double* w_prev, double* w_out, int* status,
                      double* obj, int* iters, void* workspace, size_t ws_bytes, void* stream) {
    // every rule is decided before any launch (and before the B == 0 return): the descriptor as
    // kmpc_solve_mv_ws, the cap, then the limit (0: none) in mv_box_limit's order
    if (!desc || desc->B < 0 || desc->N < 1 || desc->H < 1) return KMPC_ERR_INVALID;
    if (desc->H > KMPC_MV_MAX_H || desc->N * desc->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (!(max_turnover >= 0.0)) return KMPC_ERR_INVALID;                // (NaN too)
    if (max_turnover == 0.0) {   // no cap: the existing call
        if (max_weight == 0.0)
            return kmpc_solve_mv_ws(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, workspace,
                                    ws_bytes, stream);
        return kmpc_solve_mv_box(desc, max_weight, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters,
                                 workspace, ws_bytes, stream);
    }
    double u = 0.0;
    if (max_weight != 0.0) {   // (0: none, and then allow_short is allowed)
        const int rc = mv_box_limit(*desc, max_weight, u);
        if (rc) return rc;
    }
    if (desc->B == 0) return KMPC_OK;
    if (!mu || !sigma || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::mv_solve_launch(desc, mu, sigma, sigma_stride, w_prev, w_out, status, obj, iters, workspace,
                                 ws_bytes, (hipStream_t)stream, u, max_turnover);
}

size_t kmpc_mv_band_workspace_bytes(const kmpc_mv_desc* desc, int with_cap) {
    if (!desc || desc->N < 1 || desc->H < 1 || desc->H > KMPC_MV_MAX_H || (long long)desc->N * desc->H > KMPC_MV_MAX_HN)
        return 0;
    return kmpc::mv_band_workspace_bytes(desc, with_cap != 0);
}

int kmpc_solve_mv_band(const kmpc_mv_desc* desc, const float* yhat, const double* sigma, int sigma_per_window,
                       const double* w_prev, double max_weight, double max_turnover, double* w_out, int* status,
                       double* obj, int* iters, void* workspace, size_t ws_bytes, void* stream) {
    // every rule is decided before any launch (and before the B == 0 return): the descriptor as
    // kmpc_solve_mv_ws, the cap, then the limit (0: none) in mv_box_limit's order
    if (!desc || desc->B < 0 || desc->N < 1 || desc->H < 1) return KMPC_ERR_INVALID;
    if (desc->H > KMPC_MV_MAX_H || (long long)desc->N * desc->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (!(max_turnover >= 0.0)) return KMPC_ERR_INVALID;                // (NaN too)
    double u = 0.0;
    if (max_weight != 0.0) {   // (0: none, and then allow_short is allowed)
        const int rc = mv_box_limit(*desc, max_weight, u);
        if (rc) return rc;
    }
    if (desc->B == 0) return KMPC_OK;
    if (!yhat || !sigma || !w_prev || !w_out || !status || !obj) return KMPC_ERR_INVALID;
    return kmpc::mv_band_launch(nullptr, desc, u, max_turnover, yhat, sigma,
                                sigma_per_window ? (size_t)desc->N * desc->N : 0, w_prev, w_out, status, obj, iters,
                                0, 0, nullptr, nullptr, 0, nullptr, nullptr, workspace, ws_bytes, (hipStream_t)stream);
}

int kmpc_koopman_mv_run(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, double max_turnover,
                        int step0, int n_steps, const float* yhat, const double* sigma, const int* valid,
                        const float* realized, int n_real, double* weights, double* value, double* hist,
                        double* target, int* status, double* obj, void* workspace, size_t ws_bytes, void* stream) {
    // the rules of kmpc_markowitz_run_cap in its order, all before any launch
    if (!bd || !d || bd->P < 0 || bd->N < 1 || bd->S < 1 || step0 < 0 || n_steps < 0 ||
        step0 + n_steps > bd->S || n_real < 0 || n_real > n_steps || d->N != bd->N || d->H < 1 ||
        d->return_full_W)
        return KMPC_ERR_INVALID;
    if (d->H > KMPC_MV_MAX_H || (long long)d->N * d->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (!(max_turnover >= 0.0)) return KMPC_ERR_INVALID;   // (NaN too)
    double u = 0.0;   // the active limit (0: none)
    if (max_weight != 0.0) {
        const int rc = mv_box_limit(*d, max_weight, u);
        if (rc) return rc;
    }
    if (bd->P == 0 || n_steps == 0) return KMPC_OK;
    if (!yhat || !sigma || !valid || !weights || !value || !hist || !target || !status || !obj ||
        (n_real > 0 && !realized))
        return KMPC_ERR_INVALID;
    return kmpc::mv_band_launch(bd, d, u, max_turnover, yhat, sigma, (size_t)d->N * d->N, weights, target, status,
                                obj, nullptr, step0, n_steps, valid, realized, n_real, value, hist, workspace,
                                ws_bytes, (hipStream_t)stream);
}

int kmpc_koopman_mv_sweep(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, int n_cfg, const double* gamma,
                          const double* mv_cost, const double* bt_cost, const double* max_weight,
                          const double* max_turnover, int step0, int n_steps, const float* yhat, const double* sigma,
                          const int* valid, const float* realized, int n_real, double* weights, double* value,
                          double* hist, double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                          void* stream) {
    // kmpc_koopman_mv_run's rules in its order, all before any launch; the limits and the caps are device
    // values (checked per config in the kernel), so of their rules only allow_short is decided here
    if (!bd || !d || bd->P < 0 || bd->N < 1 || bd->S < 1 || step0 < 0 || n_steps < 0 ||
        step0 + n_steps > bd->S || n_real < 0 || n_real > n_steps || d->N != bd->N || d->H < 1 ||
        d->return_full_W)
        return KMPC_ERR_INVALID;
    if (d->H > KMPC_MV_MAX_H || (long long)d->N * d->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (n_cfg < 1 || (long long)n_cfg * bd->P > 0x7fffffffLL) return KMPC_ERR_INVALID;
    if (max_weight && d->allow_short) return KMPC_ERR_UNSUPPORTED;
    if (bd->P == 0 || n_steps == 0) return KMPC_OK;
    if (!gamma || !mv_cost || !bt_cost || !yhat || !sigma || !valid || !weights || !value || !hist || !target ||
        !status || !obj || (n_real > 0 && !realized))
        return KMPC_ERR_INVALID;
    return kmpc::mv_band_launch(bd, d, 0.0, 0.0, yhat, sigma, (size_t)d->N * d->N, weights, target, status, obj,
                                nullptr, step0, n_steps, valid, realized, n_real, value, hist, workspace, ws_bytes,
                                (hipStream_t)stream, n_cfg, gamma, mv_cost, bt_cost, max_weight, max_turnover);
}

int kmpc_rolling_moments(int B, int T, int N, int lookback, const float* z, int ldz,
                         const float* mean, const float* std, const int* ts,
                         double* mu, double* sigma, int* valid, void* stream) {
    if (B < 0 || T < 0 || N < 1 || lookback < 1 || ldz < N) return KMPC_ERR_INVALID;
    if (B == 0) return KMPC_OK;
    if (!z || !mean || !std || !ts || !mu || !sigma || !valid) return KMPC_ERR_INVALID;
    return kmpc::rolling_moments_launch(B, T, N, lookback, z, ldz, mean, std, ts, mu, sigma, valid,
                                        (hipStream_t)stream);
}

int kmpc_rolling_moments_paths(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                               const float* mean, const float* std, const int* ts,
                               double* mu, double* sigma, int* valid, void* stream) {
    if (P < 0 || n_ts < 0 || T < 0 || N < 1 || lookback < 1 || ldz < N) return KMPC_ERR_INVALID;
    if ((long long)P * n_ts > 0x7fffffffLL) return KMPC_ERR_INVALID;
    if (P == 0 || n_ts == 0) return KMPC_OK;
    if (!z || !mean || !std || !ts || !mu || !sigma || !valid) return KMPC_ERR_INVALID;
    return kmpc::rolling_moments_paths_launch(P, n_ts, T, N, lookback, z, ldz, mean, std, ts, mu, sigma, valid,
                                              (hipStream_t)stream);
}

// kmpc_rolling_cov / _paths: the estimator's rules after the shape rules, all before any launch
static int rolling_cov_rules(int N, int estimator, double ewma_lambda) {
    if (estimator < KMPC_COV_SAMPLE || estimator > KMPC_COV_EWMA) return KMPC_ERR_INVALID;
    if (estimator == KMPC_COV_EWMA && !(ewma_lambda > 0.0 && ewma_lambda <= 1.0)) return KMPC_ERR_INVALID;   // (NaN too)
    if (estimator != KMPC_COV_SAMPLE && N > KMPC_MAX_N) return KMPC_ERR_UNSUPPORTED;
    return KMPC_OK;
}

int kmpc_rolling_cov(int B, int T, int N, int lookback, const float* z, int ldz, const float* mean,
                     const float* std, const int* ts, double* mu, double* sigma, int* valid, int estimator,
                     double ewma_lambda, double* shrinkage, void* stream) {
    if (B < 0 || T < 0 || N < 1 || lookback < 1 || ldz < N) return KMPC_ERR_INVALID;
    if (const int rc = rolling_cov_rules(N, estimator, ewma_lambda)) return rc;
    if (B == 0) return KMPC_OK;
    if (!z || !mean || !std || !ts || !mu || !sigma || !valid) return KMPC_ERR_INVALID;
    return kmpc::rolling_cov_paths_launch(1, B, T, N, lookback, z, ldz, mean, std, ts, mu, sigma, valid, estimator,
                                          ewma_lambda, shrinkage, (hipStream_t)stream);
}

int kmpc_rolling_cov_paths(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz, const float* mean,
                           const float* std, const int* ts, double* mu, double* sigma, int* valid, int estimator,
                           double ewma_lambda, double* shrinkage, void* stream) {
    if (P < 0 || n_ts < 0 || T < 0 || N < 1 || lookback < 1 || ldz < N) return KMPC_ERR_INVALID;
    if ((long long)P * n_ts > 0x7fffffffLL) return KMPC_ERR_INVALID;
    if (const int rc = rolling_cov_rules(N, estimator, ewma_lambda)) return rc;
    if (P == 0 || n_ts == 0) return KMPC_OK;
    if (!z || !mean || !std || !ts || !mu || !sigma || !valid) return KMPC_ERR_INVALID;
    return kmpc::rolling_cov_paths_launch(P, n_ts, T, N, lookback, z, ldz, mean, std, ts, mu, sigma, valid, estimator,
                                          ewma_lambda, shrinkage, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// kmpc_markowitz_run (the batch is the paths) and kmpc_markowitz_sweep (configs x paths; the configs
// carry gamma and the two cost coefficients, the descs' are not read). Every rule is decided before
// any launch, the position limit's in kmpc_solve_mv_box's order. cap: the _cap entries — the run's
// max_turnover (NaN or < 0 invalid; 0 is the plain run) or the sweep's per-config caps (device).
int markowitz_entry(bool sweep, const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, bool cap,
                    double max_turnover, const double* cfg_turnover, int n_cfg, const double* gamma, const double* mv_cost, const double* bt_cost, int step0, int n_steps,
                    const double* mu, const double* sigma, const int* valid, const float* realized, int n_real,
                    double* weights, double* value, double* hist, double* target, int* status, double* obj,
                    void* workspace, size_t ws_bytes, void* stream) {
    if (!bd || !d || bd->P < 0 || bd->N < 1 || bd->S < 1 || step0 < 0 || n_steps < 0 ||
        step0 + n_steps > bd->S || n_real < 0 || n_real > n_steps || d->N != bd->N || d->H < 1 ||
        d->return_full_W)
        return KMPC_ERR_INVALID;
    if (sweep && (n_cfg < 1 || (long long)n_cfg * bd->P > 0x7fffffffLL)) return KMPC_ERR_INVALID;
    if (d->H > KMPC_MV_MAX_H || (long long)d->N * d->H > KMPC_MV_MAX_HN) return KMPC_ERR_UNSUPPORTED;
    if (cap && !sweep) {
        if (!(max_turnover >= 0.0)) return KMPC_ERR_INVALID;   // (NaN too)
        cap = max_turnover > 0.0;                                // 0: kmpc_markowitz_run
    }
    double u = 0.0;   // the active limit (0: the plain kernels)
    if (max_weight != 0.0) {   // (0: none, for these two entries only)
        const int rc = mv_box_limit(*d, max_weight, u);
        if (rc) return rc;
    }
    if (bd->P == 0 || n_steps == 0) return KMPC_OK;
    if (!mu || !sigma || !valid || !weights || !value || !hist || !target || !status || !obj ||
        (n_real > 0 && !realized) || (sweep && (!gamma || !mv_cost || !bt_cost)) || (sweep && cap && !cfg_turnover))
        return KMPC_ERR_INVALID;
    return kmpc::mv_bt_launch(bd, d, u, cap, max_turnover, cfg_turnover, sweep ? n_cfg : 0, gamma, mv_cost, bt_cost, step0, n_steps, mu, sigma, valid,
                              realized, n_real, weights, value, hist, target, status, obj, workspace, ws_bytes,
                              (hipStream_t)stream);
}

}  // namespace

extern "C" {

int kmpc_markowitz_run(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight, int step0,
                       int n_steps, const double* mu, const double* sigma, const int* valid, const float* realized,
                       int n_real, double* weights, double* value, double* hist, double* target, int* status,
                       double* obj, void* workspace, size_t ws_bytes, void* stream) {
    return markowitz_entry(false, bdesc, mvdesc, max_weight, false, 0.0, nullptr, 0, nullptr, nullptr, nullptr, step0,
                           n_steps, mu, sigma, valid, realized, n_real, weights, value, hist, target, status, obj,
                           workspace, ws_bytes, stream);
}

int kmpc_markowitz_run_cap(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                           double max_turnover, int step0, int n_steps, const double* mu, const double* sigma,
                           const int* valid, const float* realized, int n_real, double* weights, double* value,
                           double* hist, double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                           void* stream) {
    return markowitz_entry(false, bdesc, mvdesc, max_weight, true, max_turnover, nullptr, 0, nullptr, nullptr, nullptr,
                           step0, n_steps, mu, sigma, valid, realized, n_real, weights, value, hist, target, status,
                           obj, workspace, ws_bytes, stream);
}

int kmpc_markowitz_sweep(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight, int n_cfg,
                         const double* gamma, const double* mv_cost, const double* bt_cost, int step0, int n_steps,
                         const double* mu, const double* sigma, const int* valid, const float* realized, int n_real,
                         double* weights, double* value, double* hist, double* target, int* status, double* obj,
                         void* workspace, size_t ws_bytes, void* stream) {
    return markowitz_entry(true, bdesc, mvdesc, max_weight, false, 0.0, nullptr, n_cfg, gamma, mv_cost, bt_cost, step0,
                           n_steps, mu, sigma, valid, realized, n_real, weights, value, hist, target, status, obj,
                           workspace, ws_bytes, stream);
}

int kmpc_markowitz_sweep_cap(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                             int n_cfg, const double* gamma, const double* mv_cost, const double* bt_cost,
                             const double* max_turnover, int step0, int n_steps, const double* mu,
                             const double* sigma, const int* valid, const float* realized, int n_real,
                             double* weights, double* value, double* hist, double* target, int* status, double* obj,
                             void* workspace, size_t ws_bytes, void* stream) {
    return markowitz_entry(true, bdesc, mvdesc, max_weight, true, 0.0, max_turnover, n_cfg, gamma, mv_cost, bt_cost,
                           step0, n_steps, mu, sigma, valid, realized, n_real, weights, value, hist, target, status,
                           obj, workspace, ws_bytes, stream);
}

}  // extern "C"
