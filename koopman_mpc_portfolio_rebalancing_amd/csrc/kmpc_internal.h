// kmpc_internal.h — launch entry points shared by the kernels and the C ABI (kmpc_capi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kmpc.h"

namespace kmpc {

// kmpc_solve.hip
// max_weight, here and below: the active per-asset position limit, validated by the caller (no short,
// 1 / N < max_weight < 1), or 0.0 for none. The box family that runs d under a limit: the register
// box kernels (no workspace), the large-window box kernel (solve_workspace_bytes), or none.
enum class BoxFamily { NONE, REGISTER, LARGE };
BoxFamily box_family(const kmpc_solve_desc* d, double max_weight);
size_t solve_workspace_bytes(const kmpc_solve_desc* d, double max_weight);
int solve_launch(const kmpc_solve_desc* d, double max_weight, const float* yhat, const double* w_prev,
                 double* w_out, int* status, double* obj, int* iters, void* ws, size_t ws_bytes,
                 hipStream_t stream, double* trace = nullptr);

// the path-persistent backtest: the run (n_cfg = 0) or the sweep of n_cfg configs (BtLaunch:
// kmpc_solve_args.h); KMPC_ERR_UNSUPPORTED where the plan has no persistent kernel
struct BtLaunch;
int backtest_launch(const kmpc_backtest_desc* bd, const kmpc_solve_desc* sd, double max_weight, int n_cfg,
                    const BtLaunch& l, double* target, int* status, double* obj, hipStream_t stream);

// kmpc_backtest.hip
int gross_returns_launch(size_t n, const float* yhat, float* R, hipStream_t stream);
int backtest_step_launch(const kmpc_backtest_desc* d, int step, const double* target,
                         const float* realized_next, double* weights, double* value, double* hist,
                         hipStream_t stream);
int backtest_metrics_launch(const kmpc_backtest_desc* d, const double* hist, double* metrics,
                            hipStream_t stream);

// kmpc_rollout.hip
size_t rollout_workspace_bytes(const kmpc_rollout_desc* d);
int rollout_launch(const kmpc_rollout_desc* d, const float* obs, float* yhat, void* ws,
                   size_t ws_bytes, hipStream_t stream);
int standardize_launch(int T, int N, const double* y, const double* mean, const double* stdv, float* z,
                       hipStream_t stream);

// kmpc_mv.hip
size_t mv_lds_bytes(int N, int H);
size_t mv_workspace_bytes(const kmpc_mv_desc* d);
size_t mv_cap_workspace_bytes(const kmpc_mv_desc* d);   // the CAP kernels' slabs (0 while H N <= 128)
int mv_solve_launch(const kmpc_mv_desc* d, const double* mu, const double* sigma, size_t sigma_stride,
                    const double* w_prev, double* w_out, int* status, double* obj, int* iters,
                    void* ws, size_t ws_bytes, hipStream_t stream, double max_weight = 0.0,   // > 0: the BOX kernels
                    double max_turnover = 0.0);   // > 0: the CAP kernels (workspace: mv_cap_workspace_bytes)
// the band forms (BAND kernels): the workspace (0 in the LDS case) and the launch of kmpc_solve_mv_band
// (bd null) or of kmpc_koopman_mv_run (bd set: w_prev = the weights, w_out = the target rows) or of
// kmpc_koopman_mv_sweep (bd set, n_cfg > 0: n_cfg x P rows; the configs' device arrays [n_cfg], the last
// two null or set for the whole launch: the BOX / CAP form; max_weight and max_turnover are not read)
size_t mv_band_workspace_bytes(const kmpc_mv_desc* d, bool cap);
int mv_band_launch(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, double max_turnover,
                   const float* yhat, const double* sigma, size_t sigma_stride, const double* w_prev,
                   double* w_out, int* status, double* obj, int* iters, int step0, int n_steps, const int* valid,
                   const float* realized, int n_real, double* value, double* hist, void* ws, size_t ws_bytes,
                   hipStream_t stream, int n_cfg = 0, const double* cfg_gamma = nullptr,
                   const double* cfg_mv_cost = nullptr, const double* cfg_bt_cost = nullptr,
                   const double* cfg_max_weight = nullptr, const double* cfg_max_turnover = nullptr);
int rolling_moments_launch(int B, int T, int N, int lookback, const float* z, int ldz, const float* mean,
                           const float* stdv, const int* ts, double* mu, double* sigma, int* valid,
                           hipStream_t stream);
int rolling_moments_paths_launch(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                                 const float* mean, const float* stdv, const int* ts, double* mu, double* sigma,
                                 int* valid, hipStream_t stream);
// kmpc_rolling_cov (P = 1) / kmpc_rolling_cov_paths: KMPC_COV_SAMPLE is rolling_moments_paths_launch,
// the others rolling_cov_kernel; shrinkage [n_ts, P] may be null
int rolling_cov_paths_launch(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                             const float* mean, const float* stdv, const int* ts, double* mu, double* sigma,
                             int* valid, int estimator, double lambda, double* shrinkage, hipStream_t stream);
// the Markowitz backtest: the run (n_cfg = 0) or the sweep of n_cfg configs; cap: the CAP kernels with
// the run's max_turnover or the sweep's per-config caps cfg_turnover [n_cfg] (device)
int mv_bt_launch(const kmpc_backtest_desc* bd, const kmpc_mv_desc* d, double max_weight, bool cap,
                 double max_turnover, const double* cfg_turnover, int n_cfg,
                 const double* gamma, const double* mv_cost, const double* bt_cost, int step0, int n_steps,
                 const double* mu, const double* sigma, const int* valid, const float* realized, int n_real,
                 double* weights, double* value, double* hist, double* target, int* status, double* obj,
                 void* ws, size_t ws_bytes, hipStream_t stream);

}  // namespace kmpc
