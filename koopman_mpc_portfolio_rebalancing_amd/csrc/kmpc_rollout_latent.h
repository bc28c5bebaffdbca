// kmpc_rollout_latent.h — the H-step latent loops of the rollout (kmpc_rollout.hip): LatentArgs, the
// four fused loops, plane splitting and the latent-powers kernel.
#pragma once
#include "kmpc_rollout_gemm.h"

namespace kmpc {

// Fused latent steps (fp32, single-layer decoder): the whole H-step loop of backtest.py:101-119
// in one launch. A block owns 32 windows; their z rows stay in LDS for all H steps (ping-pong
// tiles), each step computes z <- z K on v_mfma_f32_32x32x2_f32 (K^T rows streamed from L2, the
// next 32-k chunk prefetched under the current one), the ball norm if any (model.py:750-751),
// then decode rows 0..N-1 with bias + de-standardize straight into yhat[:, k, :]
// (model.py:768-777, data_finance.py:729-742). Same k order per MFMA lane as gemm_nt_kernel (lane
// (r, h) consumes k = k0 + 16 h + s); the chunks alternate between two accumulators, so the
// fp32 sums are regrouped (not bit-identical to the unfused launches; within the rollout tests'
// 1e-4 of the reference). Replaces 2H small GEMM launches that are latency-bound at small batch.
struct LatentArgs {
    int B, L, N, H;
    const float* z0;     // [B, L]
    // z0 as the raw split-K partials of the last encoder layer (nparts > 0): z0 = sum of the parts in
    // slice order + zbias, as splitk_epilogue_kernel would have formed it (bit-identical)
    const float* zparts; int nparts; const float* zbias;
    const float* Kt;     // [L, L]: row j = column j of K (32-row kernel)
    const float* K;      // [L, L] row-major, z <- z K (16-row kernel: read in place, no transpose launch)
    const float* D;      // decoder rows 0..N-1, [N, L]
    const float* bias;   // [N] or null
    const float* mean; const float* stdv;
    float* yhat;         // [B, H, N]
    int ball;
};
constexpr int LAT_ROWS = 32;

__device__ __forceinline__ float latent_z0(const LatentArgs& a, int m, int col) {
    const size_t i = (size_t)m * a.L + col;
    if (a.nparts == 0) return a.z0[i];
    float v = a.zparts[i];
    for (int z = 1; z < a.nparts; ++z) v += a.zparts[(size_t)z * a.B * a.L + i];
    return v + (a.zbias ? a.zbias[col] : 0.0f);
}

// acc (+)= A[32 rows of As, stride lda] . B[32 rows of Bg, stride L]^T over k in [0, L)
__device__ __forceinline__ void tile_dot(const float* As, int lda, const float* Bg, int L, bool brow_ok,
                                         int lane, f32x16& acc) {
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc1[i] = 0.0f;
    const float* pa = As + r * lda + 16 * h;
    const float* pb = Bg + (size_t)r * L + 16 * h;
    f32x4 bn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bn[q] = brow_ok ? *(const f32x4*)(pb + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < L; k0 += 32) {
        float af[16], bf[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 x = *(const f32x4*)(pa + k0 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) { af[4 * q + e] = x[e]; bf[4 * q + e] = bn[q][e]; }
        }
        if (k0 + 32 < L) {   // next chunk of B under this chunk's MFMAs
#pragma unroll
            for (int q = 0; q < 4; ++q) bn[q] = brow_ok ? *(const f32x4*)(pb + k0 + 32 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if ((k0 >> 5) & 1) {
#pragma unroll
            for (int s = 0; s < 16; ++s) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc1, 0, 0, 0);
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += acc1[i];
}

template <int NWV>
__global__ void __launch_bounds__(64 * NWV) latent_steps_kernel(LatentArgs a) {
    extern __shared__ float zs[];   // [2][32][L + 4]
    const int L = a.L, LS = L + 4, N = a.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5;
    const int m0 = blockIdx.x * LAT_ROWS;
    float* zc = zs;
    float* zn = zs + LAT_ROWS * LS;
    for (int idx = tid; idx < LAT_ROWS * L; idx += 64 * NWV) {
        const int row = idx / L, col = idx - row * L;
        zc[row * LS + col] = (m0 + row < a.B) ? latent_z0(a, m0 + row, col) : 0.0f;
    }
    __syncthreads();
    const int nct = L / 32, ndt = (N + 31) / 32;
    for (int k = 0; k < a.H; ++k) {
        // z <- z K: output column tiles ct = wv, wv + NWV, ...
        for (int ct = wv; ct < nct; ct += NWV) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            tile_dot(zc, LS, a.Kt + (size_t)ct * 32 * L, L, true, lane, acc);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                zn[((i & 3) + 8 * (i >> 2) + 4 * h) * LS + ct * 32 + (lane & 31)] = acc[i];
        }
        __syncthreads();
        if (a.ball) {   // x / ||x||_2 per row: 8 threads per row (the first 256 threads)
            if (tid < 8 * LAT_ROWS) {
                const int row = tid >> 3, part = tid & 7;
                float sq = 0.0f;
                for (int j = part; j < L; j += 8) sq += zn[row * LS + j] * zn[row * LS + j];
                sq += __shfl_xor(sq, 1, 64);
                sq += __shfl_xor(sq, 2, 64);
                sq += __shfl_xor(sq, 4, 64);
                const float nrm = sqrtf(sq);
                for (int j = part; j < L; j += 8) zn[row * LS + j] = zn[row * LS + j] / nrm;
            }
            __syncthreads();
        }
        // decode rows 0..N-1 (+ bias), de-standardize into yhat[:, k, :]
        for (int ct = wv; ct < ndt; ct += NWV) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            const int nrow = ct * 32 + (lane & 31);
            tile_dot(zn, LS, a.D + (size_t)ct * 32 * L, L, nrow < N, lane, acc);
            if (nrow < N) {
                const float bias = a.bias ? a.bias[nrow] : 0.0f, mu = a.mean[nrow], sd = a.stdv[nrow];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (m < a.B) a.yhat[((size_t)m * a.H + k) * N + nrow] = destandardize(acc[i] + bias, sd, mu);
                }
            }
        }
        float* t = zc; zc = zn; zn = t;
        __syncthreads();
    }
}

// Small window batches (fewer than 8,192 windows: 32-row blocks would leave CUs idle, BASELINE
// configs[1] has 4,096 -> 128 blocks): the same H-step loop with 16 windows per block on
// v_mfma_f32_16x16x4_f32 (A[l&15][k], B[k][l&15], k = 4 (l>>4) + e over a 16-k chunk; C/D
// col = l&15, row = 4 (l>>4) + i). z <- z K: L / 16 column tiles over the 4 waves; decode: the
// ceil(N / 16) decoder row tiles. One accumulator per tile (exact fp32, the k order of a chunk is
// the same for both operands).
constexpr int LAT16 = 16;
__device__ __forceinline__ void tile_dot16(const float* As, int lda, const float* Bg, int L, bool brow_ok, int lane,
                                           f32x4& acc) {
    const int r = lane & 15, kq = lane >> 4;
    const float* pa = As + r * lda + 4 * kq;
    const float* pb = Bg + (size_t)r * L + 4 * kq;
    f32x4 bn = brow_ok ? *(const f32x4*)pb : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < L; k0 += 16) {
        const f32x4 av = *(const f32x4*)(pa + k0);
        const f32x4 bv = bn;
        if (k0 + 16 < L) bn = brow_ok ? *(const f32x4*)(pb + k0 + 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
    }
}

// tile_dot16 with B = columns col0.. col0 + 15 of the row-major K read in place: lane (r, kq) loads
// K[k0 + 4 kq + e][col0 + r], e = 0..3 (16 lanes cover 64 contiguous bytes of a K row; K is L2
// resident). Same values and k order as tile_dot16 on K^T, so the sums are bit-identical.
__device__ __forceinline__ void tile_dot16_k(const float* As, int lda, const float* K, int col0, int L, int lane,
                                             f32x4& acc) {
    const int r = lane & 15, kq = lane >> 4;
    const float* pa = As + r * lda + 4 * kq;
    const float* pb = K + (size_t)(4 * kq) * L + col0 + r;
    f32x4 bn = {pb[0], pb[L], pb[2 * L], pb[3 * L]};
    for (int k0 = 0; k0 < L; k0 += 16) {
        const f32x4 av = *(const f32x4*)(pa + k0);
        const f32x4 bv = bn;
        if (k0 + 16 < L) {
            const float* q = pb + (size_t)(k0 + 16) * L;
            bn = f32x4{q[0], q[L], q[2 * L], q[3 * L]};
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
    }
}

// NWV waves per block: the L / 16 column tiles of z K spread over them (8 waves: one tile each at
// L = 128, two waves per SIMD at configs[1]'s 256 blocks)
template <int NWV, bool KDIR>
__global__ void __launch_bounds__(64 * NWV) latent_steps16_kernel(LatentArgs a) {
    extern __shared__ float zs[];   // [2][16][L + 4]
    const int L = a.L, LS = L + 4, N = a.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * LAT16;
    float* zc = zs;
    float* zn = zs + LAT16 * LS;
    for (int idx = tid; idx < LAT16 * L; idx += 64 * NWV) {
        const int row = idx / L, col = idx - row * L;
        zc[row * LS + col] = (m0 + row < a.B) ? latent_z0(a, m0 + row, col) : 0.0f;
    }
    __syncthreads();
    const int nct = L / 16, ndt = (N + 15) / 16;
    const int c = lane & 15, rq = 4 * (lane >> 4);
    for (int k = 0; k < a.H; ++k) {
        for (int ct = wv; ct < nct; ct += NWV) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (KDIR) tile_dot16_k(zc, LS, a.K, ct * 16, L, lane, acc);
            else tile_dot16(zc, LS, a.Kt + (size_t)ct * 16 * L, L, true, lane, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) zn[(rq + i) * LS + ct * 16 + c] = acc[i];
        }
        __syncthreads();
        if (a.ball) {   // x / ||x||_2 per row: 16 threads per row (the first 256 threads)
            if (tid < 16 * LAT16) {
                const int row = tid >> 4, part = tid & 15;
                float sq = 0.0f;
                for (int j = part; j < L; j += 16) sq += zn[row * LS + j] * zn[row * LS + j];
                sq += __shfl_xor(sq, 1, 64);
                sq += __shfl_xor(sq, 2, 64);
                sq += __shfl_xor(sq, 4, 64);
                sq += __shfl_xor(sq, 8, 64);
                const float nrm = sqrtf(sq);
                for (int j = part; j < L; j += 16) zn[row * LS + j] = zn[row * LS + j] / nrm;
            }
            __syncthreads();
        }
        for (int ct = wv; ct < ndt; ct += NWV) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int nrow = ct * 16 + c;
            tile_dot16(zn, LS, a.D + (size_t)ct * 16 * L, L, nrow < N, lane, acc);
            if (nrow < N) {
                const float bias = a.bias ? a.bias[nrow] : 0.0f, mu = a.mean[nrow], sd = a.stdv[nrow];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + rq + i;
                    if (m < a.B) a.yhat[((size_t)m * a.H + k) * N + nrow] = destandardize(acc[i] + bias, sd, mu);
                }
            }
        }
        float* t = zc; zc = zn; zn = t;
        __syncthreads();
    }
}

// The H-step loop with the fp32 products on the bf16 MFMA in three exact planes (dtype
// KMPC_DTYPE_F32 at L = 256 — the C3 latent — identity norm; other shapes keep the f32-input
// kernels). 64 windows per block: z lives in LDS as its three bf16 planes (hi + mid + lo = z
// exactly; [3][64][L + 8], 101 KB, one block of 8 waves per CU), K^T and the decoder rows are split
// into planes once per call (split_planes_kernel, [3][rows][L] in the workspace, L2 resident) and
// read straight into the B fragments with 16-byte loads, two 16-k steps ahead; each B fragment
// feeds both 32-row tiles (half the L2 stream of 32-row blocks: a 32-row version of this kernel
// measured 1.54 ms against the f32-input kernel's 1.46 ms at C3, bound by that stream). Per 16-k
// step and tile six v_mfma_f32_32x32x16_bf16 (192 cycles) against eight v_mfma_f32_32x32x2_f32
// (512). One z buffer: each wave keeps its z K tiles in accumulators, a barrier, then the tiles are
// split into the buffer.
__global__ void __launch_bounds__(256) split_planes_kernel(const float* src, int R, int Rp, int L, int ld,
                                                           __bf16* dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)Rp * L;
    if (i >= n) return;
    const int row = (int)(i / L), col = (int)(i % L);
    const float x = row < R ? src[(size_t)row * ld + col] : 0.0f;
    __bf16 h, m, l;
    split3(x, h, m, l);
    dst[i] = h;
    dst[n + i] = m;
    dst[2 * n + i] = l;
}

constexpr int LATX3_ROWS = 64;
// acc0 / acc1 += rows 0..31 / 32..63 of the z planes . B[32 plane rows at Bp, row stride L, plane
// stride PS]^T over k in [0, L); the six plane products per 16-k step, small pairs first
template <int L, int LSP, int PL>
__device__ __forceinline__ void tile_x3_2(const __bf16* zp, const __bf16* Bp, size_t PS, int lane, f32x16& acc0,
                                         f32x16& acc1) {
    const int r = lane & 31, h = lane >> 5;
    const __bf16* pa = zp + r * LSP + 8 * h;
    const __bf16* pb = Bp + (size_t)r * L + 8 * h;
    bf16x8 b0[3], b1[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        b0[p] = *(const bf16x8*)(pb + p * PS);
        b1[p] = *(const bf16x8*)(pb + p * PS + 16);
    }
#pragma unroll 2
    for (int k0 = 0; k0 < L; k0 += 16) {
        bf16x8 bf[3], a0[3], a1[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            bf[p] = b0[p];
            b0[p] = b1[p];
            if (k0 + 32 < L) b1[p] = *(const bf16x8*)(pb + p * PS + k0 + 32);
            a0[p] = *(const bf16x8*)(pa + p * PL + k0);
            a1[p] = *(const bf16x8*)(pa + 32 * LSP + p * PL + k0);
        }
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], bf[1], acc0, 0, 0, 0);   // mid.mid
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[1], bf[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[2], bf[0], acc0, 0, 0, 0);   // lo.hi
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[2], bf[0], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bf[2], acc0, 0, 0, 0);   // hi.lo
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bf[2], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[1], bf[0], acc0, 0, 0, 0);   // mid.hi
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[1], bf[0], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bf[1], acc0, 0, 0, 0);   // hi.mid
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bf[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0], bf[0], acc0, 0, 0, 0);   // hi.hi
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], bf[0], acc1, 0, 0, 0);
    }
}

template <int NWV, int L>
__global__ void __launch_bounds__(64 * NWV) latent_steps_x3_kernel(LatentArgs a, const __bf16* Kp,
                                                                   const __bf16* Dp, int Dpad) {
    extern __shared__ __bf16 zp[];   // [3][64][L + 8]
    // L a compile-time constant: the tile write-back's LDS offsets are instruction immediates
    constexpr int LSP = L + 8, PL = LATX3_ROWS * LSP, NCT = L / 32;
    static_assert(NCT <= NWV, "one z K column tile per wave");
    const int N = a.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * LATX3_ROWS;
    for (int idx = tid; idx < LATX3_ROWS * L; idx += 64 * NWV) {
        const int row = idx / L, col = idx - row * L;
        const float x = (m0 + row < a.B) ? latent_z0(a, m0 + row, col) : 0.0f;
        __bf16 p0, p1, p2;
        split3(x, p0, p1, p2);
        zp[row * LSP + col] = p0;
        zp[PL + row * LSP + col] = p1;
        zp[2 * PL + row * LSP + col] = p2;
    }
    __syncthreads();
    const int ndt = (N + 31) / 32;
    const size_t KPS = (size_t)L * L, DPS = (size_t)Dpad * L;
    float* yhat = a.yhat;
    for (int k = 0; k < a.H; ++k) {
        // per-step launder of the base pointers: the addresses derived from them are recomputed
        // each step (scalar work) instead of being hoisted into VGPRs for all H steps
        asm volatile("" : "+s"(Kp), "+s"(Dp), "+s"(yhat));
        // z <- z K: column tile wv of both row tiles, held in registers until every wave has read z
        f32x16 acc0, acc1;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
        if (wv < NCT) tile_x3_2<L, LSP, PL>(zp, Kp + (size_t)wv * 32 * L, KPS, lane, acc0, acc1);
        __syncthreads();
        if (wv < NCT) {
            __bf16* zt = zp + 4 * h * LSP + wv * 32 + r;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int o = ((i & 3) + 8 * (i >> 2)) * LSP;
                __bf16 p0, p1, p2;
                split3(acc0[i], p0, p1, p2);
                zt[o] = p0;
                zt[PL + o] = p1;
                zt[2 * PL + o] = p2;
                split3(acc1[i], p0, p1, p2);
                zt[32 * LSP + o] = p0;
                zt[PL + 32 * LSP + o] = p1;
                zt[2 * PL + 32 * LSP + o] = p2;
            }
        }
        __syncthreads();
        // decode rows 0..N-1 (+ bias), de-standardize into yhat[:, k, :]
        for (int ct = wv; ct < ndt; ct += NWV) {
            f32x16 d0, d1;
#pragma unroll
            for (int i = 0; i < 16; ++i) d0[i] = d1[i] = 0.0f;
            tile_x3_2<L, LSP, PL>(zp, Dp + (size_t)ct * 32 * L, DPS, lane, d0, d1);
            const int nrow = ct * 32 + r;
            if (nrow < N) {
                const float bias = a.bias ? a.bias[nrow] : 0.0f, mu = a.mean[nrow], sd = a.stdv[nrow];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (m < a.B) yhat[((size_t)m * a.H + k) * N + nrow] = destandardize(d0[i] + bias, sd, mu);
                    if (m + 32 < a.B)
                        yhat[((size_t)(m + 32) * a.H + k) * N + nrow] = destandardize(d1[i] + bias, sd, mu);
                }
            }
        }
        // (the next step's z K only reads the planes; its writes follow the barrier after it)
    }
}

// Latent powers (round 5): for a linear latent step (z_t = z_{t-1} K, identity norm) and a one-layer
// decoder, y_t = z_t D_N^T + b = z_0 (D_N (K^T)^t)^T + b, so the whole H-step loop is ONE GEMM of
// z_0 against W = [W_1; ...; W_H], W_t = D_N (K^T)^t = W_{t-1} K^T ([H N, L], latent_powers_kernel
// per call, float64 chains rounded once per W_t): L H N multiply-adds per window instead of
// H (L^2 + L N) — 3.6x fewer at C3 (L = 256, N = 100, H = 10). The same fp32 GEMM arithmetic,
// with the K products taken on the weights instead of the activations (checked against float64:
// tests/test_rollout_gpu.py). From LATPOW_MINB windows (kmpc_rollout.hip).
// W_t rows: one workgroup per decoder row i (rows are independent: W_t[i] = W_{t-1}[i] K^T), one
// thread per column j, the row chain carried in float64 in LDS and each W_t rounded once to fp32;
// Kt = K^T read coalesced (thread j reads Kt[k][j]). ~10 us where H GEMM launches took ~160 us.
__global__ void latent_powers_kernel(const float* __restrict__ D, const float* __restrict__ Kt, int L, int N, int H,
                                     float* __restrict__ W) {
    extern __shared__ double prow[];   // [L]
    const int i = blockIdx.x, j = threadIdx.x;
    if (j < L) prow[j] = (double)D[(size_t)i * L + j];
    __syncthreads();
    for (int t = 0; t < H; ++t) {
        double acc = 0.0;
        if (j < L) {
            // eight independent partial sums, sixteen loads in flight (L % 32 == 0: latent_fusable)
            double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < L; k0 += 16) {
                float kv[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) kv[u] = Kt[(size_t)(k0 + u) * L + j];
#pragma unroll
                for (int u = 0; u < 16; ++u) a[u & 7] = fma(prow[k0 + u], (double)kv[u], a[u & 7]);
            }
            acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        }
        __syncthreads();
        if (j < L) {
            prow[j] = acc;
            W[((size_t)t * N + i) * L + j] = (float)acc;
        }
        __syncthreads();
    }
}

}  // namespace kmpc
