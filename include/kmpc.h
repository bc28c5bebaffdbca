/*
 * kmpc.h — C ABI of the MI355X-native Koopman-MPC window engine (libkmpc.so).
 *
 * This is the drop-in boundary for the per-window hot path of the reference
 * (yli421/koopman-mpc-portfolio-rebalancing):
 *
 *   KoopmanMPCStrategy.rebalance            backtest.py:80-131
 *     encode -> H x (step_latent, decode, extract[:N], destandardize)
 *                                           backtest.py:99-121, model.py:756-797,839-850,
 *                                           data_finance.py:717-742
 *     solve_mpc_log_utility(w_prev, yhat)   mpc.py:27-117
 *
 * Conventions
 *   - Every pointer argument of kmpc_rollout / kmpc_solve / kmpc_window is a DEVICE pointer owned
 *     by the caller (e.g. torch tensor storage). Arrays are row-major and contiguous.
 *   - Calls are stream-ordered on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *     allocate nothing, hold no global state and are re-entrant per device.
 *   - Return value: KMPC_OK (0) or a negative KMPC_ERR_* code (argument / launch errors).
 *     Per-problem solver outcome is reported in status[] (KMPC_STATUS_*), never as an error:
 *     this mirrors mpc.py:107-117, where solver failure is not raised but reported through
 *     problem.status and answered with the "hold current weights" fallback.
 *   - No torch types cross this boundary.
 */
#ifndef KMPC_H
#define KMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ------------------------------------------------------------------------- */
#define KMPC_OK               0
#define KMPC_ERR_INVALID     -1   /* bad descriptor / null pointer                              */
#define KMPC_ERR_UNSUPPORTED -2   /* shape outside what the kernels were built for             */
#define KMPC_ERR_WORKSPACE   -3   /* ws_bytes smaller than kmpc_workspace_bytes()              */
#define KMPC_ERR_LAUNCH      -4   /* a HIP launch failed (hipGetLastError)                     */

/* ---- per-problem solver status (maps to cvxpy status strings, mpc.py:113) ----------------- */
#define KMPC_STATUS_OPTIMAL            0  /* "optimal"                                         */
#define KMPC_STATUS_OPTIMAL_INACCURATE 1  /* "optimal_inaccurate"                              */
#define KMPC_STATUS_INFEASIBLE         2  /* "infeasible"                                      */
#define KMPC_STATUS_UNBOUNDED          3  /* "unbounded"                                       */
#define KMPC_STATUS_SOLVER_ERROR       4  /* "solver_error" (non-finite inputs, breakdown)     */

/* Maximum horizon / asset count the solver kernels are instantiated for. */
#define KMPC_MAX_H 21   /* the 3H x 3H Schur system is factored by one 64-lane wavefront */
#define KMPC_MAX_N 1024

/* ---- MPC solve: replaces solve_mpc_log_utility (mpc.py:27-117) ---------------------------- */
/*
 * For each problem b (one rolling window):
 *   maximize_W  sum_t log(R_t . w_t) - c * sum_t ||w_t - w_{t-1}||_1        (mpc.py:66-103)
 *   s.t.        1^T w_t = 1;  w_t >= 0 unless allow_short;                  (mpc.py:83-86)
 *               ||w_t - w_{t-1}||_1 <= tau  if tau > 0, w_{-1} = w_prev     (mpc.py:94-100)
 *   with R_t = np.exp(yhat_t) (mpc.py:55) evaluated in float32 exactly as numpy does it
 *   (kmpc_gross_returns below) and then used in float64, as cvxpy receives it; W in [H, N].
 * Inputs:  yhat [B, H, N] float32 (predicted log-returns, the reference passes float32 here,
 *          backtest.py:121), w_prev [B, N] float64 (current_weights).
 * Outputs: w_out [B, N] (W[0], what rebalance() applies, backtest.py:131) or [B, H, N] when
 *          return_full_W != 0; status [B]; obj [B] (problem.value, NaN when not optimal);
 *          iters [B] (may be NULL; interior-point iterations taken, 0 for windows solved by the
 *          closed-form presolve: cost_coeff = 0, max_turnover <= 0, no shorting, where the
 *          program separates into H simplex problems with a vertex optimum).
 * Failure fallback (mpc.py:113-115) is applied in-kernel: w_out = tile(w_prev), obj = NaN.
 *          Non-finite yhat / w_prev, or an R that overflows float32 (yhat >= 88.72), give
 *          solver_error and the fallback.
 * Errors:  cost_coeff < 0 -> KMPC_ERR_INVALID: the reference program is then not convex
 *          and cvxpy raises (DCPError) instead of returning a status.
 * Workspace: always size it with kmpc_workspace_bytes(NULL, desc). It is 0 for windows of
 *          N <= 256 assets and H <= 10 periods (solved in registers); otherwise the large-window
 *          kernel keeps each window's interior-point state there: (21 HM + 128) (64 ceil(N / 64))
 *          doubles per window slot, HM = 10 for H <= 10 and 21 past it (the compiled horizon
 *          bound, not H), for min(B, 768) slots when N <= 256, min(B, 512) otherwise.
 *          The mixed-precision pair (AUTO at >= KMPC_MIXED_MIN_B windows, MIXED) keeps a 64 B record
 *          header per window, B x 64 bytes (ABI 0.6.0: the float32 iterate goes to the float64
 *          finish on chip; 0.5.0 kept a (5 H N + 3 H + 16)-float record per window).
 *          Too little -> KMPC_ERR_WORKSPACE.
 */
#define KMPC_PATH_AUTO     0   /* kernel chosen by shape and batch (and the closed-form presolve);
                                  small windows (N <= 32) are packed 2-4 per wave from
                                  KMPC_PACK_MIN_B windows per call (ABI 0.6.0; any batch for
                                  H <= 2), one per wave below it — the faster form at each size */
#define KMPC_PACK_MIN_B    512
#define KMPC_PATH_REGISTER 1   /* interior point in the register kernels where the shape fits them
                                  (small windows packed at any batch size)                         */
#define KMPC_PATH_LARGE    2   /* interior point in the large-window (workspace) kernel            */
#define KMPC_PATH_REGISTER_UNPACKED 3   /* register kernels, one window per wave even for N <= 32
                                           (no lane-group packing); for A/B and tests             */
/* Arithmetic of the interior point. MIXED: where a mixed-precision kernel pair exists (H = 10,
 * 64 < N < 104, no short, c > 0 or tau > 0 with a cap: BASELINE configs[2..3]) the first iterations
 * run in float32 (the whole state in registers, no spills) until mu <= mu_handoff, and the float64
 * kernel finishes from that iterate to the same tolerance and status rules as F64; elsewhere
 * float64. AUTO: MIXED from KMPC_MIXED_MIN_B windows per call (a throughput win), F64 below it
 * (a latency-bound batch: the lock-step backtest's few paths finish sooner in float64 alone).
 * F64: float64 throughout. The answer's accuracy is that of the float64 finish either way. */
#define KMPC_PRECISION_AUTO  0
#define KMPC_PRECISION_F64   1
#define KMPC_PRECISION_MIXED 2
#define KMPC_MIXED_MIN_B 2048
typedef struct kmpc_solve_desc {
    int    B;              /* number of independent problems (windows); past 2^22
                              the solve runs as equal launches of <= 2^22 windows
                              (same kernels, same results as one launch)          */
    int    N;              /* assets,  1 <= N <= KMPC_MAX_N                       */
    int    H;              /* horizon, 1 <= H <= KMPC_MAX_H                       */
    double cost_coeff;     /* MPCConfig.cost_coeff   (mpc.py:22)                  */
    double max_turnover;   /* MPCConfig.max_turnover (mpc.py:23); <= 0 disables   */
    int    allow_short;    /* MPCConfig.allow_short  (mpc.py:24)                  */
    int    max_iter;       /* interior-point iteration cap (0 -> default 80)      */
    double tol;            /* complementarity tolerance (<= 0 -> default 1e-9)    */
    int    return_full_W;  /* 0: w_out is [B,N] (W[0]); 1: w_out is [B,H,N]       */
    int    n_refine;       /* max iterative-refinement steps per Newton solve; refinement stops once
                              ||r||_inf <= 1e-7 ||b||_inf (<0 -> none, 0 -> default 3)             */
    int    path;           /* KMPC_PATH_* (0 = by shape). Per call: no process-wide switches      */
    int    precision;      /* KMPC_PRECISION_* (ABI 0.3.0; MIXED 0.4.0)                           */
    double mu_handoff;     /* mixed precision: the float32 phase hands its iterate to the float64
                              solve once the scaled complementarity mu <= mu_handoff
                              (<= 0 -> default 3e-5)                                               */
} kmpc_solve_desc;

int kmpc_solve(const kmpc_solve_desc* desc,
               const float*  yhat,     /* [B,H,N] */
               const double* w_prev,   /* [B,N]   */
               double*       w_out,    /* [B,N] or [B,H,N] */
               int*          status,   /* [B] */
               double*       obj,      /* [B] */
               int*          iters,    /* [B] or NULL */
               void* workspace, size_t ws_bytes, void* stream);

/* ---- MPC solve with a per-asset position limit (added within ABI 0.7.0, see the version note
 * at the end): the program of kmpc_solve with one more constraint, w_t,i <= max_weight for every
 * period and asset (0 <= w <= max_weight, no shorting). Arrays, statuses and the fallback are
 * those of kmpc_solve; a window whose w_prev sits above the limit where the turnover cap does not
 * let it come down reports KMPC_STATUS_INFEASIBLE and holds. The limit is one more barrier inside
 * the interior point of the float64 register kernels; the call takes no workspace.
 * Return codes, all decided before any launch (and before the B == 0 return):
 *   - desc is checked as for kmpc_solve;
 *   - max_weight NaN or <= 0: KMPC_ERR_INVALID;
 *   - max_weight >= 1 without shorting is an inactive bound: the call IS kmpc_solve(desc, ...,
 *     workspace = NULL, 0) — bit-identical results — and returns KMPC_ERR_WORKSPACE where that
 *     solve needs a workspace (the large-window kernel, the mixed pair): call kmpc_solve there;
 *   - N * max_weight <= 1 (an empty feasible set, or the single point 1/N): KMPC_ERR_INVALID;
 *   - KMPC_ERR_UNSUPPORTED: allow_short != 0; N > 256 or H > 10; path == KMPC_PATH_LARGE;
 *     precision == KMPC_PRECISION_MIXED.
 * KMPC_PRECISION_AUTO and _F64 both run float64 at every batch size; batches past 2^22 windows go
 * as equal launches, as in kmpc_solve. */
int kmpc_solve_box(const kmpc_solve_desc* desc, double max_weight,
                   const float*  yhat,     /* [B,H,N] */
                   const double* w_prev,   /* [B,N]   */
                   double*       w_out,    /* [B,N] or [B,H,N] */
                   int*          status,   /* [B] */
                   double*       obj,      /* [B] */
                   int*          iters,    /* [B] or NULL */
                   void* stream);

/* ---- ... at every shape kmpc_solve takes (added within ABI 0.7.0, see the version note at the
 * end): kmpc_solve_box with a workspace, so that the limit reaches the windows the large-window
 * kernel solves (N > 256 or H > 10, and path == KMPC_PATH_LARGE at any shape; N <= 1024, H <= 21).
 * There the limit is the same barrier inside the large-window interior point — two more arrays in
 * each window's workspace slab (the multiplier, the corrector's target); same arrays, statuses,
 * stopping and fallback rules as kmpc_solve on that kernel. The relation to kmpc_solve_box is that
 * of kmpc_solve_mv_ws to kmpc_solve_mv.
 * Return codes, all decided before any launch (and before the B == 0 return), in this order:
 *   - desc is checked as for kmpc_solve;
 *   - max_weight NaN or <= 0: KMPC_ERR_INVALID;
 *   - max_weight >= 1 without shorting is an inactive bound: the call IS kmpc_solve(desc, ...,
 *     workspace, ws_bytes) — bit-identical results; the workspace is handed on, so an inactive
 *     bound works at every shape;
 *   - N * max_weight <= 1: KMPC_ERR_INVALID;
 *   - allow_short != 0 or precision == KMPC_PRECISION_MIXED: KMPC_ERR_UNSUPPORTED;
 *   - N <= 256, H <= 10 and path != KMPC_PATH_LARGE: the call IS kmpc_solve_box(desc, max_weight,
 *     ...) — bit-identical results, the workspace is not read;
 *   - path == KMPC_PATH_REGISTER or _REGISTER_UNPACKED with N > 256 or H > 10: KMPC_ERR_UNSUPPORTED;
 *   - else the large-window box kernel: KMPC_ERR_WORKSPACE where workspace is NULL or ws_bytes is
 *     below kmpc_solve_box_workspace_bytes(desc, max_weight); then B == 0 returns KMPC_OK; then NULL
 *     arrays (iters may be NULL) are KMPC_ERR_INVALID.
 * kmpc_solve_box_workspace_bytes returns 0 for an invalid descriptor or limit and for the
 * unsupported combinations, kmpc_workspace_bytes(NULL, desc) for an inactive bound, 0 where
 * kmpc_solve_box runs, and otherwise 8 (23 HM + 128) 64 ceil(N / 64) min(B, slots) bytes, HM = 10
 * for H <= 10 and 21 past it, slots = 768 windows in flight for N <= 256 and 512 past it (the plain
 * solve's slab of 21 arrays plus two). kmpc_workspace_bytes and kmpc_solve do not change. */
size_t kmpc_solve_box_workspace_bytes(const kmpc_solve_desc* desc, double max_weight);
int kmpc_solve_box_ws(const kmpc_solve_desc* desc, double max_weight,
                      const float*  yhat,     /* [B,H,N] */
                      const double* w_prev,   /* [B,N]   */
                      double*       w_out,    /* [B,N] or [B,H,N] */
                      int*          status,   /* [B] */
                      double*       obj,      /* [B] */
                      int*          iters,    /* [B] or NULL */
                      void* workspace, size_t ws_bytes, void* stream);

/* ---- gross returns: R = np.exp(yhat) on float32, bit for bit as numpy 2.x evaluates it on x86-64
 * (mpc.py:55; the realized returns np.exp(r) - 1 of backtest.py:188 use the same function).
 * yhat and R are device arrays of n floats. */
int kmpc_gross_returns(size_t n, const float* yhat, float* R, void* stream);

/* ---- Koopman rollout: replaces backtest.py:99-121 (+ model.py encode/step/decode) ---------- */
#define KMPC_MODEL_GENERIC 0   /* GenericKM / SparseKM (model.py:701-797)                      */
#define KMPC_MODEL_LISTA   1   /* LISTAKM              (model.py:801-870)                      */
#define KMPC_ACT_RELU 0
#define KMPC_ACT_TANH 1
#define KMPC_ACT_GELU 2
#define KMPC_NORM_ID   0
#define KMPC_NORM_BALL 1
#define KMPC_MAX_LAYERS 8
#define KMPC_DTYPE_F32  0   /* fp32 arithmetic (the reference's). The GEMMs run on the bf16 MFMA with
                               each fp32 operand split exactly into three bf16 planes and the six
                               leading plane products accumulated in fp32: an fp32 GEMM in accuracy
                               (error against a float64 restatement equal to the f32-input MFMA's,
                               DESIGN.md §3.1), 2.7x the f32-input MFMA's peak rate               */
#define KMPC_DTYPE_BF16 1   /* GEMM operands rounded to bf16 (BASELINE configs[4])               */
#define KMPC_DTYPE_F32_F32MFMA 2   /* fp32 arithmetic on the f32-input MFMA (v_mfma_f32_32x32x2_f32,
                                      the round-4 GEMMs; A/B and tests)                          */
/*
 * An MLP (model.py:67-117, MLPCoder): n_layers Linear layers with dims[0] -> dims[1] -> ... ->
 * dims[n_layers]; activation `act` after every layer but the last; ReLU after the last one when
 * last_relu. weights[l] is the nn.Linear weight [dims[l+1], dims[l]] (row-major, [out, in]),
 * bias[l] is [dims[l+1]] or NULL.
 */
typedef struct kmpc_mlp {
    int n_layers;
    int dims[KMPC_MAX_LAYERS + 1];
    int act;
    int last_relu;
    const float* weight[KMPC_MAX_LAYERS];
    const float* bias[KMPC_MAX_LAYERS];
} kmpc_mlp;

#define KMPC_LATENT_AUTO       0   /* kmpc_rollout_desc.latent_unfused */
#define KMPC_LATENT_UNFUSED    1
#define KMPC_LATENT_SEQUENTIAL 2

typedef struct kmpc_rollout_desc {
    int B;            /* windows                                                  */
    int N;            /* assets (first N outputs of the decoder, data_finance.py:729) */
    int H;            /* horizon                                                  */
    int L;            /* latent size (MODEL.TARGET_SIZE)                          */
    int obs;          /* observation size N * EMBEDDING_DIM                       */
    int model_kind;   /* KMPC_MODEL_*                                             */
    int norm_fn;      /* KMPC_NORM_* (GenericKM only, model.py:740-754)           */
    /* encoder: GenericKM MLP encoder, or LISTA's We (MLP, or 1 linear layer)      */
    kmpc_mlp encoder;
    /* LISTA (model.py:190-209): z = shrink(We x, thr); loops x z = shrink(z S + c, thr) */
    const float* lista_S;     /* [L, L]   */
    int   lista_loops;
    float lista_thresh;       /* alpha / L */
    /* Koopman matrix, z <- z @ K (row-vector convention, model.py:311-321) */
    const float* kmat;        /* [L, L]   */
    /* decoder (GenericKM: MLP decoder; LISTAKM: one linear layer = normalised dictionary^T).
       Only the first N outputs of the last layer are evaluated. For a 1-layer decoder
       decoder.weight[0] may point at the first N rows of the [obs, L] weight (ld = L).   */
    kmpc_mlp decoder;
    const float* mean;        /* [N] de-standardisation (data_finance.py:740-742) */
    const float* std;         /* [N] */
    int obs_ld;               /* row stride of obs in floats (0 -> obs). With obs_ld = N, obs may
                                 point into a standardized [T, N] return panel: window i reads the
                                 rows i .. i+d-1 (kmpc_standardize below) — the time-delay
                                 embedding without materialising it; the first encoder layer's
                                 column blocks must then be in oldest-lag-first order.          */
    int dtype;                /* KMPC_DTYPE_F32 (0, the reference's fp32 arithmetic), KMPC_DTYPE_BF16
                                 (1: GEMM operands rounded to bf16 on MFMA, fp32 accumulation and
                                 epilogues; BASELINE configs[4]) or KMPC_DTYPE_F32_F32MFMA (2)   */
    int latent_unfused;       /* the H-step latent loop (KMPC_LATENT_*, same fp32 arithmetic up to
                                 summation order; A/B and tests):
                                 0 AUTO: the library's choice — from 8,192 windows (LATPOW_MINB)
                                   with a linear latent step (norm 'id', LISTA) one GEMM of z_0 against
                                   the latent powers D_N (K^T)^t, else one fused launch;
                                 1 UNFUSED: one GEMM launch per step;
                                 2 SEQUENTIAL: the fused step-by-step loop at every batch size
                                   (ABI 0.6.0; the three-plane latent_steps_x3_kernel at L = 256) */
} kmpc_rollout_desc;

int kmpc_rollout(const kmpc_rollout_desc* desc,
                 const float* obs,    /* [B, obs] standardized time-delay embedding */
                 float*       yhat,   /* [B, H, N] */
                 void* workspace, size_t ws_bytes, void* stream);

/* ---- data format before the path: standardize a log-return panel (data_finance.py:243-260, 331) */
/* z[t, n] = (float)((log_returns[t, n] - mean[n]) / std[n]), float64 arithmetic then float32, as
 * the reference standardizes in pandas and casts with .astype(np.float32). */
int kmpc_standardize(int T, int N, const double* log_returns, const double* mean, const double* std,
                     float* z, void* stream);

/* ---- fused window: rollout -> solve on one stream (KoopmanMPCStrategy.rebalance) ---------- */
int kmpc_window(const kmpc_rollout_desc* rdesc, const kmpc_solve_desc* sdesc,
                const float*  obs,      /* [B, obs] */
                const double* w_prev,   /* [B, N]   */
                float*        yhat,     /* [B, H, N] (written; may be NULL -> kept in workspace) */
                double*       w_out, int* status, double* obj, int* iters,
                void* workspace, size_t ws_bytes, void* stream);

/* ---- lock-step backtest bookkeeping for P paths: run_backtest / calculate_metrics ------------ */
/*
 * Replaces the per-step body of run_backtest (backtest.py:173-217) for P independent paths run in
 * lock step (each path's target weights come from kmpc_window / kmpc_solve), and calculate_metrics
 * (backtest.py:221-249) per path. History layout: hist [P, S, 4] float64 rows
 * (portfolio_value, return, turnover, cost) — the reference DataFrame columns.
 */
typedef struct kmpc_backtest_desc {
    int    P;            /* paths run in lock step                                   */
    int    N;            /* assets                                                   */
    int    S;            /* history rows per path                                    */
    double cost_coeff;   /* BacktestConfig.cost_coeff (backtest.py:28)               */
} kmpc_backtest_desc;

/* Step `step` (history row) for every path: cost from the turnover to `target` [P,N] f64, the
 * realized float32 log-returns of t+1 `realized_next` [P,N] (NULL when t+1 is past the data:
 * no market move), value [P] and weights [P,N] updated in place (drift with the 1e-8 guard). */
int kmpc_backtest_step(const kmpc_backtest_desc* desc, int step, const double* target,
                       const float* realized_next, double* weights, double* value, double* hist,
                       void* stream);

/* A whole run_backtest per path in ONE launch (ABI 0.5.0): steps step0 .. step0 + n_steps - 1 of
 * every path, each the kmpc_solve of that step's window then the kmpc_backtest_step bookkeeping,
 * run back to back by one workgroup per path — no per-step launches, and no path waits for the
 * slowest window of the step (the lock-step loop's bound at small P). The results are bit-identical
 * to that loop (kmpc_solve of the P windows + kmpc_backtest_step per step): the same window solve
 * and the same bookkeeping code.
 *   sdesc:    the solve's program (B is ignored: the batch is desc->P; return_full_W must be 0).
 *   yhat:     [n_steps, P, H, N] float32 forecasts of the steps (kmpc_rollout of their windows).
 *   realized: [n_steps, P, N] float32 log-returns of each step's t + 1; steps k >= n_real have none
 *             (realized_next = NULL in kmpc_backtest_step).
 *   weights [P,N] f64, value [P] f64, hist [P,S,4]: as kmpc_backtest_step, updated in place.
 *   target [P,N] f64, status [P] int, obj [P] f64: scratch (on return: the last step's W0, status,
 *             objective).
 * KMPC_ERR_UNSUPPORTED unless kmpc_solve would solve a batch of P such windows with a float64
 * register kernel of the constant case (no short, cost and cap) — one window per workgroup for
 * H = 10 or 5 and 32 < N <= 256 (the BASELINE C3 shape among them), or (ABI 0.6.0) the packed
 * kernels for N <= 32 and H = 2, 5 or 10 (BASELINE configs[0]'s 10 assets, H = 5: one path per
 * lane group, 64 / GL paths per wave) — and not the mixed pair, i.e. float64 for this batch size;
 * the caller then runs the lock-step loop. */
int kmpc_backtest_run(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, int step0, int n_steps,
                      const float* yhat, const float* realized, int n_real, double* weights, double* value,
                      double* hist, double* target, int* status, double* obj, void* stream);

/* A hyper-parameter sweep of kmpc_backtest_run in ONE launch (ABI 0.7.0): n_cfg configs — each an
 * MPCConfig.cost_coeff, an MPCConfig.max_turnover and a BacktestConfig.cost_coeff — over the same
 * desc->P paths, one workgroup (one lane group in the packed form) per (config j, path p). Results
 * are config-major: row j * P + p of weights / value / hist / target / status / obj. The forecasts
 * and the realized returns depend on the path only and are shared by the configs, not replicated.
 *   desc:     P = paths; cost_coeff is ignored (bt_cost[j] instead).
 *   sdesc:    the solve's program; cost_coeff, max_turnover and B are ignored; allow_short and
 *             return_full_W must be 0.
 *   mpc_cost, max_turnover, bt_cost: [n_cfg] float64 DEVICE arrays. The kernels are the constant
 *             case "no short, cost and cap": a config with max_turnover[j] <= 0, mpc_cost[j] < 0 or
 *             a non-finite parameter is outside it, and since the host cannot see the values, every
 *             step of that config ends KMPC_STATUS_SOLVER_ERROR with the hold fallback (W0 = w_prev:
 *             turnover and cost 0); the other configs are not affected. Callers run such configs
 *             through kmpc_backtest_run / the lock-step loop instead.
 *   yhat:     [n_steps, P, H, N] float32, realized: [n_steps, P, N] float32, n_real: as kmpc_backtest_run.
 *   weights [n_cfg,P,N] f64, value [n_cfg,P] f64, hist [n_cfg,P,S,4]: updated in place.
 *   target [n_cfg*P,N] f64, status [n_cfg*P] int, obj [n_cfg*P] f64: scratch, as kmpc_backtest_run.
 * Argument rules and return codes as kmpc_backtest_run (n_steps = 0 is the shape probe); n_cfg < 1
 * is KMPC_ERR_INVALID. Always float64, at every batch size: precision AUTO or F64; MIXED is
 * KMPC_ERR_UNSUPPORTED. Shapes: those of kmpc_backtest_run (H = 10 or 5 with 32 < N <= 256; N <= 32
 * with H = 2, 5 or 10, packed or one per wave as kmpc_solve would run a batch of n_cfg * P windows),
 * KMPC_ERR_UNSUPPORTED elsewhere. Config j's rows are bit-identical to kmpc_backtest_run with that
 * config's parameters wherever both pick the same kernel. kmpc_backtest_metrics takes the result
 * with desc.P = n_cfg * P. */
int kmpc_backtest_sweep(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, int n_cfg,
                        const double* mpc_cost, const double* max_turnover, const double* bt_cost,
                        int step0, int n_steps, const float* yhat, const float* realized, int n_real,
                        double* weights, double* value, double* hist, double* target, int* status,
                        double* obj, void* stream);

/* kmpc_backtest_run and kmpc_backtest_sweep with a per-asset position limit (added within ABI 0.7.0,
 * see the version note at the end): every step's solve is kmpc_solve_box(sdesc, max_weight, ...)
 * instead of kmpc_solve, run by the same path-persistent kernel around the box kernels' window body.
 * The results are bit-identical to the loop of kmpc_solve_box and kmpc_backtest_step per step.
 * max_weight is one value for every path and config. Arrays, layouts, n_real, chunked calls
 * through step0 and the n_steps = 0 shape probe are those of kmpc_backtest_run / kmpc_backtest_sweep;
 * the sweep's rule for a config with max_turnover[j] <= 0, mpc_cost[j] < 0 or a non-finite parameter
 * (KMPC_STATUS_SOLVER_ERROR and the hold at every step) is kept, so both sweeps take the same
 * configs; the run takes any cost_coeff >= 0 and max_turnover kmpc_solve_box takes.
 * Return codes, all decided before any launch, in this order:
 *   - whatever kmpc_backtest_run / _sweep rejects before looking at the shape's kernel (NULL
 *     descriptors, P / S / the step range / n_real, sdesc->N != desc->N, n_cfg, sdesc as for
 *     kmpc_solve, NULL arrays with work to do): the same code;
 *   - max_weight NaN or <= 0: KMPC_ERR_INVALID;
 *   - max_weight >= 1 without shorting is an inactive bound: the call IS kmpc_backtest_run / _sweep
 *     with the same arguments (its return code, bit-identical results);
 *   - N * max_weight <= 1 (an empty feasible set, or the single point 1/N): KMPC_ERR_INVALID;
 *   - KMPC_ERR_UNSUPPORTED: allow_short != 0; N > 256 or H > 10; path == KMPC_PATH_LARGE;
 *     precision == KMPC_PRECISION_MIXED; return_full_W != 0; N <= 32 (the box case has no packed
 *     form: run the lock-step loop there);
 *   - P == 0 or n_steps == 0: KMPC_OK, nothing run.
 * Shapes: 32 < N <= 256 and every H from 1 to 10; float64 at every batch size. */
int kmpc_backtest_run_box(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, double max_weight,
                          int step0, int n_steps, const float* yhat, const float* realized, int n_real,
                          double* weights, double* value, double* hist,
                          double* target, int* status, double* obj, void* stream);
int kmpc_backtest_sweep_box(const kmpc_backtest_desc* desc, const kmpc_solve_desc* sdesc, double max_weight,
                            int n_cfg, const double* mpc_cost, const double* max_turnover, const double* bt_cost,
                            int step0, int n_steps, const float* yhat, const float* realized, int n_real,
                            double* weights, double* value, double* hist,
                            double* target, int* status, double* obj, void* stream);

/* metrics [P,5]: Sharpe Ratio, Max Drawdown, Avg Turnover, Final Value, Total Return. */
int kmpc_backtest_metrics(const kmpc_backtest_desc* desc, const double* hist, double* metrics,
                          void* stream);

/* ---- mean-variance MPC: replaces solve_mpc_mean_variance (mpc.py:119-184) ------------------ */
/*
 * For each problem b:
 *   maximize_W  sum_t [ w_t . mu_t - gamma w_t' Sigma w_t ] - c sum_t ||w_t - w_{t-1}||_1
 *   s.t.        1' w_t = 1;  w_t >= 0 unless allow_short  (mpc.py:145-169; no turnover cap)
 * with w_{-1} = w_prev. mu [B,H,N] float64 (the reference passes predicted log-returns / the
 * Markowitz rolling mean as mu), Sigma [B,N,N] float64 (sigma_stride = N*N) or one shared [N,N]
 * (sigma_stride = 0). Outputs as kmpc_solve; failure fallback tile(w_prev), obj = NaN
 * (mpc.py:180-181). Shapes: H*N <= KMPC_MV_MAX_HN, H <= KMPC_MV_MAX_H. Past H*N = 128 the
 * dense Newton matrix leaves LDS for a workspace slab (kmpc_mv_workspace_bytes; use
 * kmpc_solve_mv_ws — kmpc_solve_mv, which has no workspace argument, then returns
 * KMPC_ERR_WORKSPACE).
 */
#define KMPC_MV_MAX_HN 1024
#define KMPC_MV_MAX_H  16
typedef struct kmpc_mv_desc {
    int    B, N, H;
    double gamma;          /* MPCConfig.gamma (risk aversion, mpc.py:20)        */
    double cost_coeff;     /* MPCConfig.cost_coeff                              */
    int    allow_short;    /* MPCConfig.allow_short                             */
    int    max_iter;       /* interior-point iteration cap (0 -> 100)           */
    double tol;            /* complementarity tolerance (<= 0 -> 1e-10)         */
    int    return_full_W;  /* 0: w_out [B,N] (W[0]); 1: [B,H,N]                  */
} kmpc_mv_desc;

int kmpc_solve_mv(const kmpc_mv_desc* desc,
                  const double* mu,        /* [B,H,N] */
                  const double* sigma,     /* [B,N,N] or [N,N] */
                  size_t sigma_stride,     /* elements between windows' Sigma (0: shared) */
                  const double* w_prev,    /* [B,N] */
                  double* w_out, int* status, double* obj, int* iters, void* stream);
/* kmpc_solve_mv with a caller-provided workspace of kmpc_mv_workspace_bytes(desc) bytes */
size_t kmpc_mv_workspace_bytes(const kmpc_mv_desc* desc);
int kmpc_solve_mv_ws(const kmpc_mv_desc* desc, const double* mu, const double* sigma, size_t sigma_stride,
                     const double* w_prev, double* w_out, int* status, double* obj, int* iters,
                     void* workspace, size_t ws_bytes, void* stream);

/* ---- mean-variance MPC with a per-asset position limit (added within ABI 0.7.0, see the version
 * note at the end): the program of kmpc_solve_mv_ws with one more constraint, w_t,i <= max_weight
 * for every period and asset (0 <= w <= max_weight, no shorting). Arrays, statuses, the fallback
 * and the workspace (kmpc_mv_workspace_bytes, unchanged) are those of kmpc_solve_mv_ws. The program
 * has no turnover cap, so it is never infeasible: a w_prev above the limit trades down and pays the
 * cost, and no new status appears. The limit is one more barrier inside the same interior point
 * (slack max_weight - w from the iterate, its multiplier in a register), in both storage variants.
 * Return codes, all decided before any launch (and before the B == 0 return), in this order:
 *   - desc is checked as for kmpc_solve_mv_ws;
 *   - max_weight NaN or <= 0: KMPC_ERR_INVALID;
 *   - allow_short != 0: KMPC_ERR_UNSUPPORTED;
 *   - max_weight >= 1 is an inactive bound: the call IS kmpc_solve_mv_ws with the same arguments,
 *     bit-identical results;
 *   - N * max_weight <= 1 (an empty feasible set, or the single point 1/N): KMPC_ERR_INVALID;
 *   - then the workspace rule of kmpc_solve_mv_ws (KMPC_ERR_WORKSPACE past H*N = 128 without one).
 * This order is not kmpc_solve_box's: shorting is looked at before the inactive bound here, so
 * allow_short with N * max_weight <= 1 is KMPC_ERR_UNSUPPORTED here and KMPC_ERR_INVALID there, and
 * allow_short with max_weight >= 1 is KMPC_ERR_UNSUPPORTED here and the plain solve there. */
int kmpc_solve_mv_box(const kmpc_mv_desc* desc, double max_weight, const double* mu, const double* sigma,
                      size_t sigma_stride, const double* w_prev, double* w_out, int* status, double* obj,
                      int* iters, void* workspace, size_t ws_bytes, void* stream);

/* ---- mean-variance MPC with an L1 turnover cap (added within ABI 0.7.0, see the version note at
 * the end): the program of kmpc_solve_mv_ws (of kmpc_solve_mv_box where max_weight is given) with one
 * more constraint per period, sum_i |w_t,i - w_{t-1},i| <= max_turnover (w_{-1} = w_prev), with or
 * without allow_short. Arrays, statuses and the fallback are those of kmpc_solve_mv_ws. The cap is one
 * more inequality per period on the epigraph rows s >= |d| (kept at cost_coeff = 0 too) inside the
 * same interior point: slack and multiplier per period, the same Cholesky, a 2H x 2H Schur system.
 * Unlike the uncapped programs this one can be infeasible: period 0 needs d0 <= max_turnover, d0 the
 * L1 distance from w_prev to the feasible set — the mass of w_prev outside its bounds (below 0 when
 * long-only, above max_weight under a limit) plus the budget gap |1 - sum clip(w_prev)| of the clipped
 * vector; with allow_short just |1 - sum w_prev|. d0 > max_turnover reports KMPC_STATUS_INFEASIBLE
 * for that window, before any iteration, with the fallback (tile(w_prev), obj NaN); the other windows
 * are not affected. A w_prev on the simplex under no limit has d0 = 0.
 * The workspace is kmpc_mv_cap_workspace_bytes(desc): the CAP kernels' slab per window in flight
 * (n (n + 1) / 2 + 2 H n doubles, n = H*N), 0 up to H*N = 128. kmpc_mv_workspace_bytes is too small.
 * Return codes, all decided before any launch (and before the B == 0 return), in this order:
 *   - desc is checked as for kmpc_solve_mv_ws;
 *   - max_turnover NaN or < 0: KMPC_ERR_INVALID;
 *   - max_turnover == 0 (no cap): the call IS kmpc_solve_mv_ws (max_weight == 0) or
 *     kmpc_solve_mv_box (otherwise) with the same arguments, their rules and workspace, bit-identical
 *     results;
 *   - max_weight == 0: no position limit (and allow_short is allowed); otherwise the rules of
 *     kmpc_solve_mv_box in its order (NaN or < 0 KMPC_ERR_INVALID, allow_short KMPC_ERR_UNSUPPORTED,
 *     >= 1 an inactive bound, N * max_weight <= 1 KMPC_ERR_INVALID);
 *   - then KMPC_ERR_WORKSPACE past H*N = 128 without kmpc_mv_cap_workspace_bytes(desc) bytes. */
size_t kmpc_mv_cap_workspace_bytes(const kmpc_mv_desc* desc);
int kmpc_solve_mv_cap(const kmpc_mv_desc* desc, double max_weight, double max_turnover, const double* mu,
                      const double* sigma, size_t sigma_stride, const double* w_prev, double* w_out, int* status,
                      double* obj, int* iters, void* workspace, size_t ws_bytes, void* stream);

/* ---- Markowitz rolling moments: MarkowitzStrategy.rebalance (baselines.py:70-88) ------------ */
/* For window b at test row t = ts[b]: returns r_s = z_s * std + mean (float32, as
 * destandardize_returns, data_finance.py:740-742) of the standardized rows z [T, ldz] (first N
 * columns = extract_current_returns), s in the last `lookback` rows of [0, t]; mu[b] = mean
 * (rounded to float32 as the reference's float32 np.mean), sigma[b] = np.cov (ddof 1, float64)
 * + 1e-6 I; valid[b] = 1 when t + 1 >= 5 (else the strategy holds its weights). */
int kmpc_rolling_moments(int B, int T, int N, int lookback, const float* z, int ldz,
                         const float* mean, const float* std, const int* ts,
                         double* mu, double* sigma, int* valid, void* stream);

/* The moments of kmpc_rolling_moments for n_ts test rows of P panels in one launch (added within
 * ABI 0.7.0): z [P, T, ldz] holds P standardized panels of T rows each, and window (s, p) is the one
 * kmpc_rolling_moments computes at test row ts[s] of panel p — its rows stay inside that panel.
 * Outputs are step-major: mu [n_ts, P, N], sigma [n_ts, P, N, N], valid [n_ts, P] (the layout
 * kmpc_markowitz_run reads). Same kernel arithmetic: with P = 1 the results equal
 * kmpc_rolling_moments(B = n_ts) bit for bit. P * n_ts must fit an int. */
int kmpc_rolling_moments_paths(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                               const float* mean, const float* std, const int* ts,
                               double* mu, double* sigma, int* valid, void* stream);

/* ---- Rolling covariance with a choice of estimator (added within ABI 0.7.0) ------------------- */
/* kmpc_rolling_moments / _paths with the covariance estimator chosen by the caller: the same windows
 * (rows lo .. hi - 1 of panel p for test row ts[s], n = hi - lo rows, p = N assets), the same float32
 * returns r_s = z_s * std + mean widened to float64, the same mu (the float32-rounded plain mean, for
 * every estimator) and the same valid; a window with valid = 0 is still filled from the rows it has.
 * Every estimator returns its Sigma + 1e-6 I, exactly symmetric (sigma == sigma^T bit for bit).
 *   KMPC_COV_SAMPLE       np.cov (ddof 1): the call IS kmpc_rolling_moments / _paths, bit for bit.
 *   KMPC_COV_LEDOIT_WOLF  x_s = r_s - mean(r) (float64), G = X'X, S = G / n, m = tr(S) / p,
 *                         beta_ = sum_s (||x_s||^2)^2, delta_ = ||G||_F^2 / n^2,
 *                         beta = (beta_ / n - delta_) / (p n), delta = (delta_ - 2 m tr(S) + p m^2) / p,
 *                         beta <- min(beta, delta), rho = 0 if beta == 0 (or delta == 0) else beta / delta,
 *                         Sigma = (1 - rho) S + rho m I      (sklearn.covariance.ledoit_wolf).
 *   KMPC_COV_OAS          the same S and m; alpha = ||S||_F^2 / p^2, num = alpha + m^2,
 *                         den = (n + 1) (alpha - m^2 / p), rho = 1 if den == 0 else min(num / den, 1),
 *                         Sigma = (1 - rho) S + rho m I      (sklearn.covariance.oas).
 *   KMPC_COV_EWMA         omega_s = lambda^(hi-1-s) / sum_k lambda^k, m_w = sum_s omega_s r_s,
 *                         Sigma = sum_s omega_s (r_s - m_w)(r_s - m_w)'
 *                         (np.cov(aweights = omega, ddof = 0); lambda = 1: the 1/n sample covariance).
 * A window of n <= 1 rows or of constant rows gives Sigma = 1e-6 I (rho = 0 for Ledoit-Wolf, 1 for OAS),
 * never a NaN. The Gram matrix runs on the float64 matrix cores from the float32 panel, so any lookback
 * runs; every sum has a fixed order: a window's bits do not depend on the batch around it.
 *   estimator:   KMPC_COV_*; another value is KMPC_ERR_INVALID.
 *   ewma_lambda: read by KMPC_COV_EWMA alone: outside (0, 1] or NaN is KMPC_ERR_INVALID.
 *   shrinkage:   [B] (or [n_ts, P]) float64, rho per window (0 for SAMPLE and EWMA); may be NULL.
 * Rules, each decided before any launch: the shape rules of kmpc_rolling_moments / _paths
 * (KMPC_ERR_INVALID), then the estimator, then lambda, then N > KMPC_MAX_N with an estimator other than
 * SAMPLE (KMPC_ERR_UNSUPPORTED), then an empty batch (KMPC_OK), then null arrays (KMPC_ERR_INVALID). */
enum kmpc_cov_estimator {
    KMPC_COV_SAMPLE = 0,
    KMPC_COV_LEDOIT_WOLF = 1,
    KMPC_COV_OAS = 2,
    KMPC_COV_EWMA = 3
};
int kmpc_rolling_cov(int B, int T, int N, int lookback, const float* z, int ldz,
                     const float* mean, const float* std, const int* ts,
                     double* mu, double* sigma, int* valid,
                     int estimator, double ewma_lambda, double* shrinkage, void* stream);
int kmpc_rolling_cov_paths(int P, int n_ts, int T, int N, int lookback, const float* z, int ldz,
                           const float* mean, const float* std, const int* ts,
                           double* mu, double* sigma, int* valid,
                           int estimator, double ewma_lambda, double* shrinkage, void* stream);

/* ---- Markowitz backtest: run_backtest(MarkowitzStrategy(...)) for P paths in ONE launch -------- */
/* (added within ABI 0.7.0) Steps step0 .. step0 + n_steps - 1 of every path, each the strategy's
 * window — kmpc_solve_mv_ws (kmpc_solve_mv_box under a limit) of that step's moments from the path's
 * current weights where valid, else the hold (target = current weights, baselines.py:76-78) — then
 * the kmpc_backtest_step bookkeeping, run back to back by one workgroup per path, as
 * kmpc_backtest_run does for the log-utility solve. The results are bit-identical to the per-step
 * loop of those calls: the same window solve and the same bookkeeping sums.
 *   bdesc:      P paths, N assets, S history rows, cost_coeff (as kmpc_backtest_run).
 *   mvdesc:     the solve's program; B is ignored (the batch is bdesc->P), N must equal bdesc->N,
 *               return_full_W must be 0 (KMPC_ERR_INVALID otherwise).
 *   max_weight: 0: no position limit. Otherwise the rules of kmpc_solve_mv_box in its order: NaN or
 *               < 0 KMPC_ERR_INVALID; allow_short KMPC_ERR_UNSUPPORTED; >= 1 an inactive bound (the
 *               plain kernels); N * max_weight <= 1 KMPC_ERR_INVALID.
 *   mu [n_steps, P, H, N] f64, sigma [n_steps, P, N, N] f64, valid [n_steps, P] int: the steps'
 *               moments (kmpc_rolling_moments_paths for H = 1).
 *   realized [n_steps, P, N] f32, n_real, weights [P,N], value [P], hist [P,S,4]: as kmpc_backtest_run.
 *   target [P,N] f64, status [P] int, obj [P] f64: scratch (on return the last step's W0, status,
 *               objective; a held step reports optimal and NaN).
 *   workspace:  kmpc_mv_workspace_bytes of mvdesc with B = P (0 up to H*N = 128).
 * Return codes, all decided before any launch: the argument rules above; KMPC_ERR_UNSUPPORTED past
 * H*N = KMPC_MV_MAX_HN or H > KMPC_MV_MAX_H; then n_steps = 0 (the shape probe) or P = 0 return
 * KMPC_OK; null arrays KMPC_ERR_INVALID; KMPC_ERR_WORKSPACE as kmpc_solve_mv_ws. */
int kmpc_markowitz_run(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                       int step0, int n_steps, const double* mu, const double* sigma, const int* valid,
                       const float* realized, int n_real, double* weights, double* value, double* hist,
                       double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                       void* stream);

/* A sweep of kmpc_markowitz_run over the baseline's hyper-parameters in ONE launch (added within
 * ABI 0.7.0): n_cfg configs — a risk aversion gamma[j], the solve's cost_coeff mv_cost[j] and the
 * bookkeeping's cost_coeff bt_cost[j], float64 DEVICE arrays — over the same bdesc->P paths, one
 * workgroup per (config j, path p). Rows are config-major, as kmpc_backtest_sweep: row j * P + p of
 * weights / value / hist / target / status / obj; the moments and the realized returns depend on the
 * path only and are shared by the configs. mvdesc's gamma and cost_coeff and bdesc's cost_coeff are
 * ignored; there is one max_weight (and one allow_short) per launch. A config with gamma[j] < 0,
 * mv_cost[j] < 0 or a non-finite one ends every step KMPC_STATUS_SOLVER_ERROR with the hold
 * fallback (turnover and cost 0); the other configs are not affected. n_cfg < 1 (or n_cfg * P past
 * an int) is KMPC_ERR_INVALID; every other rule as kmpc_markowitz_run, the workspace that of mvdesc
 * with B = n_cfg * P. Config j's rows are bit-identical to kmpc_markowitz_run with its parameters. */
int kmpc_markowitz_sweep(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                         int n_cfg, const double* gamma, const double* mv_cost, const double* bt_cost,
                         int step0, int n_steps, const double* mu, const double* sigma, const int* valid,
                         const float* realized, int n_real, double* weights, double* value, double* hist,
                         double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                         void* stream);

/* kmpc_markowitz_run / kmpc_markowitz_sweep under the turnover cap of kmpc_solve_mv_cap (added within
 * ABI 0.7.0): every valid step's window is kmpc_solve_mv_cap's, from the path's current (drifted)
 * weights; a step whose window is infeasible (under a limit, weights drifted above it by more than the
 * cap allows back: d0 > max_turnover) reports KMPC_STATUS_INFEASIBLE, holds, and the path goes on.
 * Results are bit-identical to the per-step loop of kmpc_solve_mv_cap and kmpc_backtest_step.
 *   max_turnover (run): NaN or < 0 KMPC_ERR_INVALID; 0: the call IS kmpc_markowitz_run with the
 *               same arguments (its workspace rule too), bit-identical results.
 *   max_turnover (sweep): [n_cfg] float64 DEVICE array, one cap per config. A config whose cap is not
 *               finite or not > 0 ends every step KMPC_STATUS_SOLVER_ERROR with the hold fallback, as
 *               one with a bad gamma[j] does: the host cannot see device values. A null pointer is
 *               KMPC_ERR_INVALID with the other null arrays.
 *   max_weight: as kmpc_markowitz_run (0: none, and then allow_short is allowed under the cap too).
 *   workspace:  kmpc_mv_cap_workspace_bytes of mvdesc with B = P (sweep: n_cfg * P), 0 up to H*N = 128.
 * Every other argument and rule, the n_steps = 0 shape probe and the P = 0 return as
 * kmpc_markowitz_run / kmpc_markowitz_sweep. */
int kmpc_markowitz_run_cap(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                           double max_turnover, int step0, int n_steps, const double* mu, const double* sigma,
                           const int* valid, const float* realized, int n_real, double* weights, double* value,
                           double* hist, double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                           void* stream);
int kmpc_markowitz_sweep_cap(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                             int n_cfg, const double* gamma, const double* mv_cost, const double* bt_cost,
                             const double* max_turnover /* [n_cfg], device */, int step0, int n_steps,
                             const double* mu, const double* sigma, const int* valid, const float* realized,
                             int n_real, double* weights, double* value, double* hist, double* target, int* status,
                             double* obj, void* workspace, size_t ws_bytes, void* stream);

/* ---- mean-variance MPC, band form: the multi-period solve for a forecast sequence (added within
 * ABI 0.7.0, see the version note at the end). The program is kmpc_solve_mv_cap's (mean-variance,
 * optional position limit, optional turnover cap) with mu_t = yhat_t, the rollout's float32 forecast
 * [B,H,N] exactly as kmpc_rollout writes it (widened to float64 in the kernel, which is exact; no
 * float64 copy). The Newton matrix M = 2 gamma (I_H (x) Sigma) + diag + D' diag(E) D is block
 * tridiagonal with diagonal off-diagonal blocks: half-bandwidth N, and its Cholesky factor has no fill
 * outside the band. These kernels keep N + 1 doubles per row of M (columns r - N .. r) and clip the
 * factorization and the triangular solves to the band; the interior point around them, the statuses
 * (KMPC_STATUS_INFEASIBLE for d0 > max_turnover, SOLVER_ERROR for non-finite input, UNBOUNDED) and the
 * fallback (tile(w_prev), obj NaN) are those of the dense kernels, which every other kmpc_solve_mv*
 * and kmpc_markowitz_* entry keeps using. On the same (float32-representable) mu a window ends with
 * the dense kernel's status and optimum. At H = 1 the band is the full triangle.
 * Storage: a window's M and Y sit in LDS while the window's LDS footprint is at most
 * KMPC_MV_BAND_LDS_BYTES (e.g. N = 10, H = 5; N = 30, H = 5; N = 61, H = 2 without the cap); past that
 * in a slab of the workspace, n (N + 1) + SH H n doubles per window in flight (n = H*N; SH = 1, or 2
 * with the cap; at most 512 windows in flight): kmpc_mv_band_workspace_bytes(desc, with_cap), 0 in the
 * LDS case. with_cap != 0: the size for a call with max_turnover > 0.
 *   sigma_per_window: 0: one shared Sigma [N,N]; otherwise Sigma [B,N,N].
 *   max_weight:   0: no limit. Otherwise the rules of kmpc_solve_mv_box in its order (NaN or < 0
 *                 KMPC_ERR_INVALID, allow_short KMPC_ERR_UNSUPPORTED, >= 1 an inactive bound,
 *                 N * max_weight <= 1 KMPC_ERR_INVALID).
 *   max_turnover: 0: no cap. NaN or < 0: KMPC_ERR_INVALID.
 * Return codes, all decided before any launch (and before the B == 0 return), in this order: desc as
 * kmpc_solve_mv_ws (KMPC_ERR_INVALID; KMPC_ERR_UNSUPPORTED past H <= KMPC_MV_MAX_H,
 * H*N <= KMPC_MV_MAX_HN); max_turnover; max_weight; B == 0 returns KMPC_OK; null arrays (iters may be
 * NULL) KMPC_ERR_INVALID; KMPC_ERR_WORKSPACE without kmpc_mv_band_workspace_bytes bytes. */
#define KMPC_MV_BAND_LDS_BYTES 65536
size_t kmpc_mv_band_workspace_bytes(const kmpc_mv_desc* desc, int with_cap);
int kmpc_solve_mv_band(const kmpc_mv_desc* desc, const float* yhat /* [B,H,N] f32 */, const double* sigma,
                       int sigma_per_window, const double* w_prev, double max_weight, double max_turnover,
                       double* w_out, int* status, double* obj, int* iters, void* workspace, size_t ws_bytes,
                       void* stream);

/* The mean-variance Koopman-MPC backtest for P paths in ONE launch (added within ABI 0.7.0): steps
 * step0 .. step0 + n_steps - 1 of every path, each the window of kmpc_solve_mv_band — that step's
 * forecast yhat and covariance, from the path's current (drifted) weights — where valid, else the
 * hold, then the kmpc_backtest_step bookkeeping, one workgroup per path. A step whose window does not
 * end optimal (infeasible under limit and cap, non-finite input) holds and the path goes on. The
 * results are bit-identical to the per-step loop of kmpc_solve_mv_band and kmpc_backtest_step: the
 * same window body and the same bookkeeping sums.
 *   yhat [n_steps, P, H, N] f32, sigma [n_steps, P, N, N] f64, valid [n_steps, P] int.
 *   max_weight, max_turnover: as kmpc_solve_mv_band.
 *   workspace: kmpc_mv_band_workspace_bytes of mvdesc with B = P.
 * Every other array and rule — bdesc, mvdesc (B ignored, return_full_W = 0), realized, n_real, weights,
 * value, hist, target, status, obj, chunking through step0, the n_steps = 0 shape probe and the P = 0
 * return — as kmpc_markowitz_run_cap. */
int kmpc_koopman_mv_run(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, double max_weight,
                        double max_turnover, int step0, int n_steps, const float* yhat, const double* sigma,
                        const int* valid, const float* realized, int n_real, double* weights, double* value,
                        double* hist, double* target, int* status, double* obj, void* workspace, size_t ws_bytes,
                        void* stream);

/* A sweep of kmpc_koopman_mv_run over the program's hyper-parameters in ONE launch (added within ABI
 * 0.7.0): n_cfg configs — a risk aversion gamma[j], the solve's cost_coeff mv_cost[j], the
 * bookkeeping's cost_coeff bt_cost[j], a position limit max_weight[j] and a turnover cap
 * max_turnover[j], float64 DEVICE arrays [n_cfg] — over the same bdesc->P paths, one workgroup per work
 * item (config j, path p) (past the LDS variant at most 512 in flight, the others following in the same
 * workgroups). Rows are config-major, as kmpc_markowitz_sweep: row j * P + p of weights / target
 * [n_cfg * P, N], value / status / obj [n_cfg * P] and hist [n_cfg * P, S, 4]. The forecasts, the
 * covariances, valid and the realized returns depend on the path only and are shared by the configs:
 * yhat [n_steps, P, H, N] f32, sigma [n_steps, P, N, N], valid [n_steps, P], realized [n_real, P, N].
 * mvdesc's gamma and cost_coeff and bdesc's cost_coeff are not read.
 *   max_weight:   NULL: no limit in any config. Otherwise every config runs the limit's kernel form
 *                 under its own max_weight[j], 1 / N < max_weight[j] < 1; with allow_short
 *                 KMPC_ERR_UNSUPPORTED.
 *   max_turnover: NULL: no cap in any config. Otherwise every config runs the cap's kernel form under
 *                 its own max_turnover[j] > 0.
 * The host cannot see device values: a config with gamma[j] < 0, mv_cost[j] < 0, a max_weight[j] with
 * N * max_weight[j] <= 1 or >= 1, a max_turnover[j] not > 0, or any of them not finite, ends every
 * valid step KMPC_STATUS_SOLVER_ERROR with the hold fallback (target = the current weights, turnover
 * and cost 0); the other configs are not affected.
 *   workspace: kmpc_mv_band_workspace_bytes of mvdesc with B = n_cfg * P, with_cap = (max_turnover !=
 *              NULL).
 * Return codes, all decided before any launch, in this order: the descriptor rules of
 * kmpc_koopman_mv_run (KMPC_ERR_INVALID, then KMPC_ERR_UNSUPPORTED past the shape limits); n_cfg < 1
 * or n_cfg * P past an int KMPC_ERR_INVALID; max_weight non-NULL with allow_short
 * KMPC_ERR_UNSUPPORTED; P == 0 or n_steps == 0 (the shape probe) KMPC_OK; null arrays (gamma, mv_cost
 * and bt_cost included) KMPC_ERR_INVALID; KMPC_ERR_WORKSPACE. Chunking through step0 as
 * kmpc_koopman_mv_run. Config j's rows are bit-identical to kmpc_koopman_mv_run with that config's five
 * scalars (bt_cost[j] as bdesc->cost_coeff; no limit / no cap where the array is NULL). */
int kmpc_koopman_mv_sweep(const kmpc_backtest_desc* bdesc, const kmpc_mv_desc* mvdesc, int n_cfg,
                          const double* gamma, const double* mv_cost, const double* bt_cost,
                          const double* max_weight   /* [n_cfg] device, or NULL: no limit */,
                          const double* max_turnover /* [n_cfg] device, or NULL: no cap   */,
                          int step0, int n_steps, const float* yhat, const double* sigma, const int* valid,
                          const float* realized, int n_real, double* weights, double* value, double* hist,
                          double* target, int* status, double* obj, void* workspace, size_t ws_bytes, void* stream);

/* Workspace needed by kmpc_rollout / kmpc_solve / kmpc_window (either desc may be NULL; with both,
   the sum for kmpc_window: rollout scratch + yhat + the solve's). */
size_t kmpc_workspace_bytes(const kmpc_rollout_desc* rdesc, const kmpc_solve_desc* sdesc);

/* Human-readable text for a return code or (status + 100) for a per-problem status. */
const char* kmpc_strerror(int code);

/* Library version string, "kmpc <ABI> (gfx950)". ABI 0.2.0 appended kmpc_solve_desc.path and
   kmpc_rollout_desc.latent_unfused; 0.3.0 appended kmpc_solve_desc.precision and .mu_handoff:
   callers built against an older ABI must rebuild. 0.4.0 added enum values only
   (KMPC_PRECISION_MIXED, KMPC_DTYPE_F32_F32MFMA; AUTO precision now float64 below KMPC_MIXED_MIN_B
   windows; KMPC_DTYPE_F32's GEMMs on three bf16 planes), no layout change. 0.5.0 added a function
   (kmpc_backtest_run), no layout change. 0.6.0 added enum values only (KMPC_LATENT_SEQUENTIAL) and
   kmpc_backtest_run's packed shapes, no layout change. 0.7.0 added a function
   (kmpc_backtest_sweep), no layout change. kmpc_solve_box was added within 0.7.0: a new function
   only — no struct, enum or existing function changed, so every caller built against 0.7.0 keeps
   working unchanged and the version string did not move; a caller that needs the function checks
   for the symbol (dlsym) rather than for a version. kmpc_solve_mv_box was added within 0.7.0 in the
   same way: a new function only, kmpc_mv_desc and every existing function unchanged.
   kmpc_rolling_moments_paths, kmpc_markowitz_run and kmpc_markowitz_sweep were added within 0.7.0 in
   the same way: three new functions, no struct, enum or existing function changed.
   kmpc_backtest_run_box and kmpc_backtest_sweep_box were added within 0.7.0 in the same way: two new
   functions, no struct, enum or existing function changed.
   kmpc_solve_box_workspace_bytes and kmpc_solve_box_ws were added within 0.7.0 in the same way: two
   new functions, no struct, enum or existing function changed (kmpc_solve_box keeps every return
   code it had).
   kmpc_mv_cap_workspace_bytes, kmpc_solve_mv_cap, kmpc_markowitz_run_cap and kmpc_markowitz_sweep_cap
   were added within 0.7.0 in the same way: four new functions, no struct, enum or existing function
   changed.
   kmpc_mv_band_workspace_bytes, kmpc_solve_mv_band and kmpc_koopman_mv_run were added within 0.7.0 in
   the same way: three new functions (and the constant KMPC_MV_BAND_LDS_BYTES), no struct, enum or
   existing function changed.
   kmpc_koopman_mv_sweep was added within 0.7.0 in the same way: one new function, no struct, enum or
   existing function changed.
   kmpc_rolling_cov and kmpc_rolling_cov_paths were added within 0.7.0 in the same way: two new
   functions and the new enum kmpc_cov_estimator, no struct, existing enum or existing function changed. */
const char* kmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMPC_H */
