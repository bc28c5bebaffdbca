// kmpc_rollout.hip — batched Koopman rollout on gfx950 (replaces backtest.py:99-121).
//
//   z  = encode(obs)                       GenericKM: MLPCoder (model.py:108-117) + norm_fn
//                                          LISTAKM:   LISTA (model.py:190-209)
//   for k in 0..H-1:
//     z = z @ K  (+ norm_fn)               model.py:311-321 / 787-797 (row-vector convention)
//     yhat[:, k, :] = decode(z)[:, :N] * std + mean      model.py:768-777 / 839-850,
//                                          data_finance.py:729 (slice), :740-742 (de-standardize)
//
// Every dense contraction is one fp32 GEMM — the arithmetic type of the reference's torch fp32
// path — on the bf16 MFMA with each fp32 operand split exactly into three bf16 planes
// (gemm_nt_x3_kernel; desc->dtype = KMPC_DTYPE_F32, the default) or on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32, KMPC_DTYPE_F32_F32MFMA); or, with KMPC_DTYPE_BF16, a bf16 MFMA GEMM
// (operands rounded to bf16, fp32 accumulation; BASELINE configs[4]) — with a fused epilogue
// (bias + activation, LISTA shrink, de-standardize-and-scatter). Only the first N decoder rows are
// evaluated. Weights in the reference's nn.Linear [out, in] layout are consumed as-is ("NT");
// K and S (right-multiplied, [in, out]) are transposed once per call into the workspace.
#include <algorithm>

#include "kmpc_rollout_gemm.h"
#include "kmpc_rollout_latent.h"

namespace kmpc {

// shrink in place (LISTA initial z = shrink(c, thr), model.py:203)
__global__ void shrink_kernel(const float* x, float* y, size_t n, float thr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float v = x[i];
        const float av = fabsf(v) - thr;
        y[i] = (av > 0.0f) ? copysignf(av, v) : 0.0f * v;
    }
}

// x / ||x||_2 per row (norm_fn 'ball', model.py:750-751); one wave per row
__global__ void ball_norm_kernel(float* x, int M, int L) {
    const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (row >= M) return;
    float* p = x + (size_t)row * L;
    float s = 0.0f;
    for (int j = lane; j < L; j += 64) s += p[j] * p[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    const float nrm = sqrtf(s);
    for (int j = lane; j < L; j += 64) p[j] = p[j] / nrm;
}

// out[j][i] = in[i][j]  (L x L)
__global__ void transpose_kernel(const float* in, float* out, int R, int Cc) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 8 rows per pass
    for (int r = ty; r < 32; r += 8) {
        const int i = by + r, j = bx + tx;
        if (i < R && j < Cc) tile[r][tx] = in[(size_t)i * Cc + j];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = bx + r, i = by + tx;
        if (i < R && j < Cc) out[(size_t)j * R + i] = tile[tx][r];
    }
}

__global__ void tile_epilogue_kernel(int H, int N, const float* bias, const float* mean, const float* stdv,
                                     float* tb, float* tm, float* ts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * N) return;
    const int n = i % N;
    tb[i] = bias ? bias[n] : 0.0f;
    tm[i] = mean[n];
    ts[i] = stdv[n];
}

// ---- the route of one GEMM (tests/rollout_variants.py: gemm() is its mirror) ----------------------
constexpr int BIG_TILES = 512;          // 128-square tiles from which 8 waves of 32 x 64 beat 16 of 32 x 32
constexpr int SPLIT_TILES64 = 256;      // fewer 64-square tiles than CUs: a long K is split (configs[1])
constexpr int BF16_FEW = 256;           // fewer 128-square tiles than CUs: bf16 takes the 64-square tile or splits
constexpr int F32_SPLITK = 4;           // K slices of the fp32 split, from K >= 128 per slice (8 measured no faster)
constexpr int BF16_SPLIT_MINK = 2048;   // bf16 splits only a long K (the LISTA encoder's obs = 10,000)
constexpr int SPLITK_BUF = 8;           // slices the partial buffer holds (the bf16 split uses all 8)
constexpr size_t SPLITK_ELEMS = (size_t)256 * 64 * 64;   // most outputs a split GEMM has: 256 tiles of 64 x 64
static_assert(F32_SPLITK >= 2 && F32_SPLITK <= SPLITK_BUF, "split-K slices");

enum GemmTile : int {
    TILE_64,       // 64 x 64: 2 x 2 waves of 32 x 32 (gemm_nt_kernel<1, 1>; bf16: gemm_nt_bf16_kernel<1>)
    TILE_128_44,   // 128 x 128: 4 x 4 waves of 32 x 32 (fp32)
    TILE_128_42,   // 128 x 128: 4 x 2 waves of 32 x 64 (fp32)
    TILE_128,      // 128 x 128: 2 x 2 waves of 64 x 64 (gemm_nt_bf16_kernel<2>)
};
enum GemmTail : int {
    TAIL_NONE,      // the GEMM's own fused epilogue
    TAIL_EPILOGUE,  // split K: splitk_epilogue_kernel sums the slices, then the epilogue
    TAIL_RAW,       // split K: the raw partials are handed on (latent_z0 sums them)
};
struct GemmRoute {
    int dtype;       // KMPC_DTYPE_*: three bf16 planes, bf16 operands, f32-input MFMA
    GemmTile tile;
    int ksplit;      // 1, or the K slices (blockIdx.z)
    GemmTail tail;
};

// raw_ok: the caller can take raw partials and the GEMM has no epilogue (EPI_NONE)
static GemmRoute route_gemm(int M, int N, int K, int dtype, bool have_part, bool raw_ok) {
    const size_t t128 = (size_t)((N + 127) / 128) * ((M + 127) / 128);
    const size_t t64 = (size_t)((N + 63) / 64) * ((M + 63) / 64);
    if (dtype == KMPC_DTYPE_BF16) {
        const bool few = t128 < BF16_FEW;
        if (few && have_part && K >= BF16_SPLIT_MINK && (size_t)M * N <= SPLITK_ELEMS)
            return {dtype, TILE_128, SPLITK_BUF, TAIL_EPILOGUE};
        return {dtype, few ? TILE_64 : TILE_128, 1, TAIL_NONE};
    }
    if (t128 < BIG_TILES) {
        if (have_part && t64 < SPLIT_TILES64 && K >= 128 * F32_SPLITK)
            return {dtype, TILE_64, F32_SPLITK, raw_ok ? TAIL_RAW : TAIL_EPILOGUE};
        return {dtype, TILE_128_44, 1, TAIL_NONE};
    }
    return {dtype, TILE_128_42, 1, TAIL_NONE};
}

template <int WM, int WN, int GM, int GN>
static void launch_f32(dim3 grid, hipStream_t s, const GemmArgs& g) {
    if (g.bf16 == 2)
        hipLaunchKernelGGL((gemm_nt_x3_kernel<WM, WN, GM, GN>), grid, dim3(64 * GM * GN), 0, s, g);
    else
        hipLaunchKernelGGL((gemm_nt_kernel<WM, WN, BK, GM, GN>), grid, dim3(64 * GM * GN), 0, s, g);
}

// launch a routed GEMM and its tail; part holds the partials of a split
static int launch_gemm(const GemmRoute& r, GemmArgs g, float* part, hipStream_t s) {
    // GemmArgs::bf16: 2 = three bf16 planes (fp32 arithmetic), 1 = bf16 operands, 0 = f32-input MFMA
    g.bf16 = r.dtype == KMPC_DTYPE_F32 ? 2 : r.dtype == KMPC_DTYPE_BF16 ? 1 : 0;
    g.ksplit = r.ksplit;
    if (r.ksplit > 1) g.part = part;
    const int t = r.tile == TILE_64 ? 64 : 128;
    const dim3 grid((g.N + t - 1) / t, (g.M + t - 1) / t, r.ksplit);
    if (g.bf16 == 1) {
        if (r.tile == TILE_64) hipLaunchKernelGGL(gemm_nt_bf16_kernel<1>, grid, dim3(256), 0, s, g);
        else hipLaunchKernelGGL(gemm_nt_bf16_kernel<2>, grid, dim3(256), 0, s, g);
    } else if (r.tile == TILE_64) {
        launch_f32<1, 1, 2, 2>(grid, s, g);
    } else if (r.tile == TILE_128_44) {
        launch_f32<1, 1, 4, 4>(grid, s, g);
    } else {
        launch_f32<1, 2, 4, 2>(grid, s, g);
    }
    if (r.tail == TAIL_EPILOGUE) {
        const size_t n = (size_t)g.M * g.N;
        hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g);
    }
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

// what every GEMM of one rollout shares: the dtype, the stream and the scratch buffers
struct GemmCtx {
    int dtype;
    hipStream_t s;
    float* ping; float* pong; int wmax;   // [B, wmax] activations of the hidden layers
    float* part;                          // split-K partials
};

// nparts (optional): a split GEMM with no epilogue leaves its raw partials in part and reports the
// slice count instead of summing them
static int gemm(const GemmCtx& c, const GemmArgs& g, int* nparts = nullptr) {
    if (nparts) *nparts = 0;
    if (g.M <= 0 || g.N <= 0) return KMPC_OK;
    const GemmRoute r = route_gemm(g.M, g.N, g.K, c.dtype, c.part != nullptr, nparts && g.epi == EPI_NONE);
    if (r.tail == TAIL_RAW) *nparts = r.ksplit;
    return launch_gemm(r, g, c.part, c.s);
}

static GemmArgs linear(int M, int N, int K, const float* A, int lda, const float* W, const float* bias,
                       float* C, int ldc) {
    GemmArgs g = {};
    g.M = M; g.N = N; g.K = K; g.A = A; g.lda = lda; g.B = W; g.ldb = K; g.bias = bias;
    g.C = C; g.ldc = ldc; g.epi = EPI_NONE;
    return g;
}

// run an MLP on X [B, dims[0]] -> out [B, dims[n]] (only the first `last_cols` outputs of the last
// layer, written with row stride ldo)
static int run_mlp(const GemmCtx& c, const kmpc_mlp& m, int Bn, const float* X, int ldx, float* out, int ldo,
                   int last_cols, int last_epi, const float* mean, const float* stdv, int* last_nparts = nullptr) {
    const float* cur = X;
    int ldc = ldx;
    for (int l = 0; l < m.n_layers; ++l) {
        const bool last = (l == m.n_layers - 1);
        const int nout = last ? last_cols : m.dims[l + 1];
        float* dst = last ? out : ((l & 1) ? c.pong : c.ping);
        GemmArgs g = linear(Bn, nout, m.dims[l], cur, ldc, m.weight[l], m.bias[l], dst, last ? ldo : c.wmax);
        if (!last) { g.epi = EPI_ACT; g.act = m.act; }
        else if (last_epi == EPI_DESTD) { g.epi = EPI_DESTD; g.mean = mean; g.stdv = stdv; }
        else if (m.last_relu) { g.epi = EPI_ACT; g.act = KMPC_ACT_RELU; }
        int rc = gemm(c, g, last ? last_nparts : nullptr);
        if (rc) return rc;
        cur = dst;
        ldc = c.wmax;
    }
    return KMPC_OK;
}

// ---- the route of one rollout (tests/rollout_variants.py: plan_stages() is its mirror) ------------
constexpr int FUSE_L_MULT = 32;         // a fused loop works on whole 32-column tiles of z K
constexpr int FUSE_L_MAX = 512;         // and keeps 2 x 32 rows of z in LDS: 132 KB at L = 512
constexpr int LAT16_MAXB = 256 * 32;    // below this 32-row blocks would leave CUs idle: the 16-row loop
constexpr int LAT16_WAVES = 8;          // waves of the 16-row loop; it runs at any batch while L <= 16 of them
constexpr int LAT32_WAVES = 4;          // waves of the 32-row loop
constexpr int LATPOW_MINB = 8192;       // the latent-powers GEMM from here (at 4,096 the 16-row loop is faster)
constexpr int LATX3_L = 256;            // the three-plane loop is built for this latent alone (the C3 model)

enum LoopKind : int {
    LOOP_STEPS,        // per step: one GEMM z K, the ball norm if any, the decoder MLP
    LOOP_POWERS,       // latent_powers_kernel, then one GEMM of z0 against [W_1; ..; W_H]
    LOOP_LAT16_KDIR,   // latent_steps16_kernel reading K in place
    LOOP_LAT16_KT,     // latent_steps16_kernel reading K^T
    LOOP_LATX3,        // latent_steps_x3_kernel
    LOOP_LAT32,        // latent_steps_kernel
};
struct RolloutPlan {
    bool ball;       // GenericKM with the ball norm after the encoder and every step
    bool fused;      // one of the four fused H-step loops (they sum z0's raw partials: latent_z0)
    LoopKind loop;
    bool need_kt;    // K^T is formed in the workspace
    bool zfuse;      // the last encoder layer may hand z0 over as raw split-K partials
};

// A fused H-step loop takes: fp32, one decoder layer, L % 32 == 0 and <= 512, decoder rows read with
// 16-byte loads (16-byte aligned base), the identity or the ball norm; latent_unfused =
// KMPC_LATENT_UNFUSED forces the per-step launches, KMPC_LATENT_SEQUENTIAL a step-by-step loop even
// where the latent powers would run (A/B and the GPU tests)
static bool latent_fusable(const kmpc_rollout_desc* d) {
    return d->latent_unfused != KMPC_LATENT_UNFUSED && d->dtype != KMPC_DTYPE_BF16 && d->decoder.n_layers == 1 &&
           d->L % FUSE_L_MULT == 0 && d->L <= FUSE_L_MAX && ((uintptr_t)d->decoder.weight[0] & 15) == 0 &&
           !(d->model_kind == KMPC_MODEL_GENERIC && d->norm_fn != KMPC_NORM_ID && d->norm_fn != KMPC_NORM_BALL);
}

static RolloutPlan plan_rollout(const kmpc_rollout_desc* d) {
    RolloutPlan p;
    const int B = d->B, L = d->L;
    p.ball = d->model_kind == KMPC_MODEL_GENERIC && d->norm_fn == KMPC_NORM_BALL;
    const bool fus = latent_fusable(d);
    // the powers need a linear step; they read K^T
    const bool latpow = d->latent_unfused == KMPC_LATENT_AUTO && fus && B >= LATPOW_MINB && !p.ball;
    // 16 windows per block: twice the blocks of the 32-row kernel for small batches, and one z K
    // column tile per wave at L <= 128 (65,536 windows, L = 128: 263 -> 184 us; at L = 256 the
    // 32-row kernel stays ahead: 1,346 vs 1,575 us)
    const bool lat16 = fus && (B < LAT16_MAXB || L <= 16 * LAT16_WAVES);
    // small batches read K in place and skip the transpose launch (configs[1]: 0.194 -> 0.190 ms per
    // step); at 65,536 windows the in-place read costs the loop more than the launch
    const bool kdir = lat16 && B < LAT16_MAXB;
    p.loop = latpow ? LOOP_POWERS : !fus ? LOOP_STEPS : lat16 ? (kdir ? LOOP_LAT16_KDIR : LOOP_LAT16_KT)
             : d->dtype == KMPC_DTYPE_F32 && !p.ball && L == LATX3_L ? LOOP_LATX3 : LOOP_LAT32;
    p.fused = p.loop != LOOP_STEPS && p.loop != LOOP_POWERS;
    p.need_kt = p.loop != LOOP_LAT16_KDIR;
    // z0 may stay unwritten only where a loop that sums the partials follows at once: the ball norm
    // and the LISTA loops read z0 first
    p.zfuse = p.fused && d->model_kind == KMPC_MODEL_GENERIC && !p.ball;
    return p;
}

// ---- the workspace: every region once, in order --------------------------------------------------
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static int max_width(const kmpc_mlp& m) {
    int w = 0;
    for (int l = 0; l <= m.n_layers; ++l) w = m.dims[l] > w ? m.dims[l] : w;
    return w;
}

struct RolloutWs {   // byte offsets
    int wmax, dpad;  // widest activation; the decoder's first N rows padded to whole 32-row tiles
    size_t Kt, St;          // K^T, S^T (LISTA): [L, L]
    size_t ping, pong, z0, z1;   // [B, wmax] activations; [B, L]: z; c (LISTA) / z next
    size_t part;            // split-K partials: SPLITK_BUF slices of at most SPLITK_ELEMS outputs
    size_t Kp, Dp;          // bf16 planes [3][L][L] of K^T and [3][dpad][L] of the decoder rows
    size_t Wpow, tiled;     // latent powers [H N, L]; the tiled bias / mean / std [3][H N]
    size_t total;
};

static RolloutWs layout(const kmpc_rollout_desc* d) {
    RolloutWs w;
    const size_t B = (size_t)d->B;
    w.wmax = std::max(d->L, std::max(max_width(d->encoder), max_width(d->decoder)));
    w.dpad = 32 * ((d->N + 31) / 32);
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    w.Kt = take(sizeof(float) * (size_t)d->L * d->L);
    w.St = take(sizeof(float) * (size_t)d->L * d->L);
    w.ping = take(sizeof(float) * B * w.wmax);
    w.pong = take(sizeof(float) * B * w.wmax);
    w.z0 = take(sizeof(float) * B * d->L);
    w.z1 = take(sizeof(float) * B * d->L);
    w.part = take(sizeof(float) * SPLITK_BUF * (B * (size_t)w.wmax < SPLITK_ELEMS ? B * (size_t)w.wmax : SPLITK_ELEMS));
    const size_t kplanes = sizeof(__bf16) * 3 * (size_t)d->L * d->L, wpow = sizeof(float) * (size_t)d->H * d->N * d->L;
    w.Kp = take(kplanes + sizeof(__bf16) * 3 * (size_t)w.dpad * d->L);
    w.Dp = w.Kp + kplanes;
    w.Wpow = take(wpow + sizeof(float) * 3 * (size_t)d->H * d->N);
    w.tiled = w.Wpow + wpow;
    w.total = off;
    return w;
}

size_t rollout_workspace_bytes(const kmpc_rollout_desc* d) { return d ? layout(d).total : 0; }

int rollout_launch(const kmpc_rollout_desc* d, const float* obs, float* yhat, void* ws,
                   size_t ws_bytes, hipStream_t s) {
    if (!d || !obs || !yhat || !d->kmat || !d->mean || !d->std) return KMPC_ERR_INVALID;
    if (d->B < 0 || d->N < 1 || d->H < 1 || d->L < 1 || d->obs < d->N) return KMPC_ERR_INVALID;
    if (d->encoder.n_layers < 1 || d->encoder.n_layers > KMPC_MAX_LAYERS) return KMPC_ERR_INVALID;
    if (d->decoder.n_layers < 1 || d->decoder.n_layers > KMPC_MAX_LAYERS) return KMPC_ERR_INVALID;
    if (d->encoder.dims[0] != d->obs || d->encoder.dims[d->encoder.n_layers] != d->L) return KMPC_ERR_INVALID;
    if (d->decoder.dims[0] != d->L || d->decoder.dims[d->decoder.n_layers] < d->N) return KMPC_ERR_INVALID;
    if (d->model_kind == KMPC_MODEL_LISTA && !d->lista_S) return KMPC_ERR_INVALID;
    const RolloutWs w = layout(d);
    if (ws_bytes < w.total || (!ws && ws_bytes)) return KMPC_ERR_WORKSPACE;
    if (d->obs_ld < 0 || (d->obs_ld > 0 && d->obs_ld < d->N)) return KMPC_ERR_INVALID;
    if (d->dtype != KMPC_DTYPE_F32 && d->dtype != KMPC_DTYPE_BF16 && d->dtype != KMPC_DTYPE_F32_F32MFMA)
        return KMPC_ERR_INVALID;
    if (d->latent_unfused < KMPC_LATENT_AUTO || d->latent_unfused > KMPC_LATENT_SEQUENTIAL) return KMPC_ERR_INVALID;
    if (d->B == 0) return KMPC_OK;
    const int Bn = d->B, L = d->L, N = d->N, H = d->H;
    const int obs_ld = d->obs_ld > 0 ? d->obs_ld : d->obs;
    const bool generic = d->model_kind == KMPC_MODEL_GENERIC;
    const RolloutPlan plan = plan_rollout(d);
    char* const base = (char*)ws;
    float *Kt = (float*)(base + w.Kt), *St = (float*)(base + w.St), *z0 = (float*)(base + w.z0), *z1 = (float*)(base + w.z1);
    const GemmCtx c = {d->dtype, s, (float*)(base + w.ping), (float*)(base + w.pong), w.wmax, (float*)(base + w.part)};
    int rc;

    dim3 tg((L + 31) / 32, (L + 31) / 32);
    if (plan.need_kt) hipLaunchKernelGGL(transpose_kernel, tg, dim3(256), 0, s, d->kmat, Kt, L, L);
    if (!generic) hipLaunchKernelGGL(transpose_kernel, tg, dim3(256), 0, s, d->lista_S, St, L, L);
    if (hipGetLastError() != hipSuccess) return KMPC_ERR_LAUNCH;

    // ---- encode ----
    // znparts > 0: the last encoder layer left z0 UNWRITTEN — its raw split-K partials sit in
    // c.part, and the fused latent loop rebuilds z0 from them (same slice order and bias). Only
    // plan.zfuse allows it, and then nothing is launched between that layer and the loop
    // (tests/test_rollout_gpu.py::test_fused_z0_is_never_read fills the workspace with NaN).
    int znparts = 0;
    if (generic) {
        rc = run_mlp(c, d->encoder, Bn, obs, obs_ld, z0, L, L, EPI_NONE, nullptr, nullptr, plan.zfuse ? &znparts : nullptr);
        if (rc) return rc;
        if (plan.ball) hipLaunchKernelGGL(ball_norm_kernel, dim3((Bn + 3) / 4), dim3(256), 0, s, z0, Bn, L);
    } else {
        // c = We(x) (z1 holds c), z = shrink(c); loops: z = shrink(z S + c)   (model.py:200-209)
        rc = run_mlp(c, d->encoder, Bn, obs, obs_ld, z1, L, L, EPI_NONE, nullptr, nullptr);
        if (rc) return rc;
        const size_t n = (size_t)Bn * L;
        hipLaunchKernelGGL(shrink_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z1, z0, n,
                           d->lista_thresh);
        float* zc = z0;
        float* zn = c.ping;   // ping is [B, wmax] >= [B, L]
        for (int it = 0; it < d->lista_loops; ++it) {
            GemmArgs g = linear(Bn, L, L, zc, L, St, nullptr, zn, L);
            g.epi = EPI_SHRINK; g.R = z1; g.ldr = L; g.thr = d->lista_thresh;
            if ((rc = gemm(c, g))) return rc;
            float* t = zc; zc = zn; zn = t;
        }
        if (zc != z0 && hipMemcpyAsync(z0, zc, sizeof(float) * n, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return KMPC_ERR_LAUNCH;
    }
    if (hipGetLastError() != hipSuccess) return KMPC_ERR_LAUNCH;

    // ---- H x (step_latent, decode[:N], destandardize) ----
    if (plan.loop == LOOP_POWERS) {
        const int HN = H * N;
        float* Wpow = (float*)(base + w.Wpow);
        float* tb = (float*)(base + w.tiled);
        float* tm = tb + HN;
        float* ts = tm + HN;
        // W_1 = D_N K^T, W_t = W_{t-1} K^T (float64 chains per row, fp32 W_t)
        hipLaunchKernelGGL(latent_powers_kernel, dim3(N), dim3(64 * ((L + 63) / 64)), sizeof(double) * L, s,
                           d->decoder.weight[0], Kt, L, N, H, Wpow);
        hipLaunchKernelGGL(tile_epilogue_kernel, dim3((HN + 255) / 256), dim3(256), 0, s, H, N, d->decoder.bias[0],
                           d->mean, d->std, tb, tm, ts);
        GemmArgs g = linear(Bn, HN, L, z0, L, Wpow, tb, yhat, HN);   // yhat [B, H, N] = [B, H N]
        g.epi = EPI_DESTD; g.mean = tm; g.stdv = ts;
        return gemm(c, g);
    }
    if (plan.fused) {
        LatentArgs la;
        la.B = Bn; la.L = L; la.N = N; la.H = H; la.z0 = z0; la.Kt = Kt; la.K = d->kmat; la.D = d->decoder.weight[0];
        la.zparts = c.part; la.nparts = znparts;
        la.zbias = d->encoder.bias[d->encoder.n_layers - 1];
        la.bias = d->decoder.bias[0]; la.mean = d->mean; la.stdv = d->std; la.yhat = yhat;
        la.ball = plan.ball;
        auto blocks = [Bn](int rows) { return dim3((Bn + rows - 1) / rows); };   // windows per block -> grid
        if (plan.loop == LOOP_LAT16_KDIR || plan.loop == LOOP_LAT16_KT) {
            const size_t lds = sizeof(float) * 2 * LAT16 * (L + 4);
            if (plan.loop == LOOP_LAT16_KDIR)
                hipLaunchKernelGGL((latent_steps16_kernel<LAT16_WAVES, true>), blocks(LAT16), dim3(64 * LAT16_WAVES), lds,
                                   s, la);
            else
                hipLaunchKernelGGL((latent_steps16_kernel<LAT16_WAVES, false>), blocks(LAT16), dim3(64 * LAT16_WAVES), lds,
                                   s, la);
        } else if (plan.loop == LOOP_LATX3) {
            __bf16* Kp = (__bf16*)(base + w.Kp);
            __bf16* Dp = (__bf16*)(base + w.Dp);
            const size_t nk = (size_t)L * L, nd = (size_t)w.dpad * L;
            hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, Kt, L, L, L, L, Kp);
            hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, s, la.D, N, w.dpad, L,
                               L, Dp);
            const size_t lds = sizeof(__bf16) * 3 * LATX3_ROWS * (L + 8);
            hipLaunchKernelGGL((latent_steps_x3_kernel<8, LATX3_L>), blocks(LATX3_ROWS), dim3(512), lds, s, la,
                               (const __bf16*)Kp, (const __bf16*)Dp, w.dpad);
        } else {
            const size_t lds = sizeof(float) * 2 * LAT_ROWS * (L + 4);
            hipLaunchKernelGGL(latent_steps_kernel<LAT32_WAVES>, blocks(LAT_ROWS), dim3(64 * LAT32_WAVES), lds, s, la);
        }
        return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
    }
    float* zc = z0;
    float* zn = z1;
    for (int k = 0; k < H; ++k) {
        if ((rc = gemm(c, linear(Bn, L, L, zc, L, Kt, nullptr, zn, L)))) return rc;
        if (plan.ball) hipLaunchKernelGGL(ball_norm_kernel, dim3((Bn + 3) / 4), dim3(256), 0, s, zn, Bn, L);
        // decoder: hidden layers full width, last layer first-N rows + destandardize into yhat[:, k, :]
        rc = run_mlp(c, d->decoder, Bn, zn, L, yhat + (size_t)k * N, H * N, N, EPI_DESTD, d->mean, d->std);
        if (rc) return rc;
        float* t = zc; zc = zn; zn = t;
    }
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

// z = f32((y - mean) / std): float64 arithmetic, one rounding to float32 (data_finance.py:243-260, 331)
__global__ void standardize_kernel(int T, int N, const double* y, const double* mean, const double* stdv,
                                   float* z) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)T * N) return;
    const int n = (int)(i % N);
    z[i] = (float)((y[i] - mean[n]) / stdv[n]);
}

int standardize_launch(int T, int N, const double* y, const double* mean, const double* stdv, float* z,
                       hipStream_t s) {
    const size_t n = (size_t)T * N;
    if (n == 0) return KMPC_OK;
    hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, N, y, mean,
                       stdv, z);
    return hipGetLastError() == hipSuccess ? KMPC_OK : KMPC_ERR_LAUNCH;
}

}  // namespace kmpc
