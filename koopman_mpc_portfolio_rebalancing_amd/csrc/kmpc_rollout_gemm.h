// kmpc_rollout_gemm.h — the GEMMs of the rollout (kmpc_rollout.hip): GemmArgs, the fused epilogues, the
// three GEMM kernels (f32-input MFMA, bf16, fp32 as three bf16 planes) and the split-K epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kmpc_internal.h"

namespace kmpc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

enum Epi : int {
    EPI_NONE = 0,        // out = acc (+ bias)
    EPI_ACT = 1,         // out = act(acc + bias)
    EPI_SHRINK = 2,      // out = shrink(acc + R, thr)            (LISTA, model.py:30-40,205-207)
    EPI_DESTD = 3,       // out = acc * std[n] + mean[n]          (data_finance.py:740-742)
};

struct GemmArgs {
    int M, N, K;
    const float* A; int lda;      // [M, K]
    const float* B; int ldb;      // [N, K]  (nn.Linear weight layout)
    const float* bias;            // [N] or null
    float* C; int ldc;            // [M, N] (row stride ldc)
    int epi, act;
    const float* R; int ldr;      // EPI_SHRINK addend [M, N]
    float thr;
    const float* mean; const float* stdv;   // EPI_DESTD [N]
    int bf16;                     // 1: operands rounded to bf16, v_mfma_f32_32x32x16_bf16 (fp32 accumulate);
                                  // 2: fp32 operands as three bf16 planes (gemm_nt_x3_kernel)
    int ksplit;                   // > 1: blockIdx.z takes a K slice, raw partials to part[z][M][N]
    float* part;                  //      (splitk_epilogue_kernel sums them in slice order, then the epilogue)
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__device__ __forceinline__ float apply_act(float x, int act) {
    if (act == KMPC_ACT_RELU) return fmaxf(x, 0.0f);
    if (act == KMPC_ACT_TANH) return tanhf(x);
    return gelu_erf(x);
}

// Tile: GM x GN waves per block, each a (32 WM) x (32 WN) block of 32 x 32 accumulator tiles, BK = 32.
// 128 x 128 as 4 x 2 waves of 32 x 64 (512 threads) for GEMMs with 512 or more such tiles, as 4 x 4
// waves of 32 x 32 (1024 threads) below that (one workgroup per CU); split K for the narrow last
// encoder layer of small batches (configs[1]).
constexpr int BM = 128, BN = 128, BK = 32, LDS_STRIDE = BK + 4;

// C = epi(A . B^T). Each lane of an MFMA consumes 16 contiguous k (k = 16h + s, h = lane >> 5),
// so operand fragments are two ds_read_b128 per row; the k permutation is the same for A and B.
// y * std + mean with two float32 roundings, as the reference's torch mul then add
// (data_finance.py:742): FMA contraction off here so yhat matches it bit for bit.
__device__ __forceinline__ float destandardize(float y, float sd, float mu) {
#pragma clang fp contract(off)
    const float p = y * sd;
    return p + mu;
}

// the epilogue of one output element
__device__ __forceinline__ float epi_value(const GemmArgs& g, int m, int n, float acc) {
    float v = acc + (g.bias ? g.bias[n] : 0.0f);
    if (g.epi == EPI_ACT) {
        v = apply_act(v, g.act);
    } else if (g.epi == EPI_SHRINK) {
        v += g.R[(size_t)m * g.ldr + n];
        const float av = fabsf(v) - g.thr;
        v = (av > 0.0f) ? copysignf(av, v) : 0.0f * v;
    } else if (g.epi == EPI_DESTD) {
        v = destandardize(v, g.stdv[n], g.mean[n]);
    }
    return v;
}

// fused epilogue of a WM x WN block of 32 x 32 accumulator tiles (either MFMA dtype: the C/D
// layout is dtype-independent on gfx950)
template <int WM, int WN>
__device__ __forceinline__ void epilogue(const GemmArgs& g, f32x16 (&acc)[WM][WN], int m0, int n0, int wm, int wn,
                                         int lane) {
    // epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b) {
            const int n = n0 + wn + b * 32 + (lane & 31);
            if (n >= g.N) continue;
            const float bias = g.bias ? g.bias[n] : 0.0f;
            float mu = 0.0f, sd = 1.0f;
            if (g.epi == EPI_DESTD) { mu = g.mean[n]; sd = g.stdv[n]; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= g.M) continue;
                float v = acc[a][b][r] + bias;
                if (g.epi == EPI_ACT) {
                    v = apply_act(v, g.act);
                } else if (g.epi == EPI_SHRINK) {
                    v += g.R[(size_t)m * g.ldr + n];
                    const float av = fabsf(v) - g.thr;
                    v = (av > 0.0f) ? copysignf(av, v) : 0.0f * v;
                } else if (g.epi == EPI_DESTD) {
                    v = destandardize(v, sd, mu);
                }
                g.C[(size_t)m * g.ldc + n] = v;
            }
        }
}

// XCD-aware tile order: the dispatcher deals workgroups round-robin over the 8 XCDs by linear id,
// so neighbouring tiles of one row panel of A would land in 8 different L2s. Renumber so that each
// XCD gets a contiguous run of tiles (same A row panels): id -> (id % 8) * (total / 8) + id / 8.
__device__ __forceinline__ void xcd_tile(int& m0, int& n0, int tm = BM, int tn = BN) {
    const int gx = gridDim.x, total = gridDim.x * gridDim.y;
    int id = blockIdx.y * gx + blockIdx.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    m0 = (id / gx) * tm;
    n0 = (id % gx) * tn;
}

// (the tiles above, and 2 x 2 waves of 32 x 32: the 64-square tile of the split-K GEMMs)
template <int WM, int WN, int BKT = BK, int GM = 2, int GN = 2>
__global__ void __launch_bounds__(64 * GM * GN) gemm_nt_kernel(GemmArgs g) {
    constexpr int NT = 64 * GM * GN;
    constexpr int TM = 32 * GM * WM, TN = 32 * GN * WN;
    constexpr int LS = BKT + 4;   // LDS row stride (floats): conflict-free ds_read_b128 fragments
    __shared__ float As[TM * LS];
    __shared__ float Bs[TN * LS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int m0, n0;
    xcd_tile(m0, n0, TM, TN);
    const int wm = (wv / GN) * 32 * WM, wn = (wv % GN) * 32 * WN;
    f32x16 acc[WM][WN];
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    const bool vec_ok = ((g.lda & 3) == 0) && ((g.ldb & 3) == 0) &&
                        ((((uintptr_t)g.A) & 15) == 0) && ((((uintptr_t)g.B) & 15) == 0);
    // split K: slice blockIdx.z of ksplit (whole BK tiles)
    int kbeg = 0, kend = g.K;
    if (g.ksplit > 1) {
        const int kc = ((g.K + g.ksplit * BKT - 1) / (g.ksplit * BKT)) * BKT;
        kbeg = blockIdx.z * kc;
        kend = min(g.K, kbeg + kc);
    }
    // A tile: TM rows x BKT k = TM BKT / 4 float4, TM BKT / 1024 per thread (B: TN rows). The next
    // k-tile's global loads are issued into registers before this tile's MFMAs (register double
    // buffering: one LDS buffer, the HBM / L2 latency under the math).
    constexpr int QA = TM * BKT / (4 * NT), QB = TN * BKT / (4 * NT);
    static_assert(QA * 4 * NT == TM * BKT && QB * 4 * NT == TN * BKT, "tile loads per thread");
    constexpr int RQ = BKT / 4;                     // float4 per row
    f32x4 va[QA], vb[QB];
    auto fetch_row = [&](const float* P, int ld, int rows, int r0, int row, int kk, f32x4& v) {
        v = f32x4{0.f, 0.f, 0.f, 0.f};
        const int rr = r0 + row;
        if (rr >= rows) return;
        if (vec_ok && kk + 3 < kend) {
            v = *(const f32x4*)(P + (size_t)rr * ld + kk);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (kk + e < kend) v[e] = P[(size_t)rr * ld + kk + e];
        }
    };
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
            const int idx = tid + q * NT;           // 0 .. TM RQ - 1
            fetch_row(g.A, g.lda, g.M, m0, idx / RQ, k0 + (idx % RQ) * 4, va[q]);
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int idx = tid + q * NT;
            fetch_row(g.B, g.ldb, g.N, n0, idx / RQ, k0 + (idx % RQ) * 4, vb[q]);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
            const int idx = tid + q * NT;
            *(f32x4*)(As + (idx / RQ) * LS + (idx % RQ) * 4) = va[q];
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int idx = tid + q * NT;
            *(f32x4*)(Bs + (idx / RQ) * LS + (idx % RQ) * 4) = vb[q];
        }
    };
    auto compute = [&]() {
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int kb = 0; kb < BKT; kb += 32) {   // 32-k sub-steps: lane (r, h) takes k = kb + 16 h + s
            float af[WM][16], bf[WN][16];
#pragma unroll
            for (int a = 0; a < WM; ++a) {
                const float* pa = As + (wm + a * 32 + r) * LS + kb + 16 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 x = *(const f32x4*)(pa + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) af[a][4 * q + e] = x[e];
                }
            }
#pragma unroll
            for (int b = 0; b < WN; ++b) {
                const float* pb = Bs + (wn + b * 32 + r) * LS + kb + 16 * h;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 y = *(const f32x4*)(pb + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bf[b][4 * q + e] = y[e];
                }
            }
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int a = 0; a < WM; ++a)
#pragma unroll
                    for (int b = 0; b < WN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][s], bf[b][s], acc[a][b], 0, 0, 0);
        }
    };
    fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BKT) {
        stage();
        __syncthreads();
        if (k0 + BKT < kend) fetch(k0 + BKT);
        compute();
        __syncthreads();
    }
    if (g.ksplit > 1) {   // raw partial of this K slice
        float* P = g.part + (size_t)blockIdx.z * g.M * g.N;
#pragma unroll
        for (int a = 0; a < WM; ++a)
#pragma unroll
            for (int b = 0; b < WN; ++b) {
                const int n = n0 + wn + b * 32 + (lane & 31);
                if (n >= g.N) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < g.M) P[(size_t)m * g.N + n] = acc[a][b][r];
                }
            }
        return;
    }
    epilogue<WM, WN>(g, acc, m0, n0, wm, wn, lane);
}

// split-K: C = epi(sum of the ksplit partials, in slice order)
__global__ void __launch_bounds__(256) splitk_epilogue_kernel(GemmArgs g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)g.M * g.N) return;
    const int m = (int)(i / g.N), n = (int)(i % g.N);
    float v = g.part[i];
    for (int z = 1; z < g.ksplit; ++z) v += g.part[(size_t)z * g.M * g.N + i];
    g.C[(size_t)m * g.ldc + n] = epi_value(g, m, n, v);
}

// bf16 variant (BASELINE configs[4]: "bf16 MFMA rollout"): the same 128 x 128 tile and epilogues;
// A and B are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) while being staged into LDS, the products
// run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation. Lane (r, h) of a 32x32x16 step holds
// A[row r][k = 8h + j] and B[col r][k = 8h + j], j = 0..7: one ds_read_b128 per operand per step.
constexpr int LDS_STRIDE_H = BK + 8;   // bf16 elements per LDS row (80 B: 16-B aligned fragments)

// WT = 2: 128 x 128 tile (4 waves of 64 x 64); WT = 1: 64 x 64 (4 waves of 32 x 32), for grids with
// fewer 128-tiles than CUs and a short K (configs[4]'s LISTA and latent-step layers)
template <int WT>
__global__ void __launch_bounds__(256) gemm_nt_bf16_kernel(GemmArgs g) {
    constexpr int TM = 64 * WT;
    __shared__ __bf16 As[TM * LDS_STRIDE_H];
    __shared__ __bf16 Bs[TM * LDS_STRIDE_H];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int m0, n0;
    xcd_tile(m0, n0, TM, TM);
    const int wm = (wv >> 1) * 32 * WT, wn = (wv & 1) * 32 * WT;
    f32x16 acc[WT][WT];
#pragma unroll
    for (int a = 0; a < WT; ++a)
#pragma unroll
        for (int b = 0; b < WT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    const bool vec_ok = ((g.lda & 3) == 0) && ((g.ldb & 3) == 0) &&
                        ((((uintptr_t)g.A) & 15) == 0) && ((((uintptr_t)g.B) & 15) == 0);
    // split K: slice blockIdx.z of ksplit (whole BK tiles), raw partials as gemm_nt_kernel
    int kbeg = 0, kend = g.K;
    if (g.ksplit > 1) {
        const int kc = ((g.K + g.ksplit * BK - 1) / (g.ksplit * BK)) * BK;
        kbeg = blockIdx.z * kc;
        kend = min(g.K, kbeg + kc);
    }
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
#pragma unroll
        for (int q = 0; q < 2 * WT; ++q) {
            const int idx = tid + q * 256;          // TM rows x 8 groups of 4 k
            const int row = idx >> 3, c4 = (idx & 7) * 4;
            const int kk = k0 + c4;
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            const int ma = m0 + row, nb = n0 + row;
            if (vec_ok && kk + 3 < kend) {
                if (ma < g.M) va = *(const f32x4*)(g.A + (size_t)ma * g.lda + kk);
                if (nb < g.N) vb = *(const f32x4*)(g.B + (size_t)nb * g.ldb + kk);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (kk + e < kend) {
                        if (ma < g.M) va[e] = g.A[(size_t)ma * g.lda + kk + e];
                        if (nb < g.N) vb[e] = g.B[(size_t)nb * g.ldb + kk + e];
                    }
                }
            }
            bf16x4 ha, hb;
#pragma unroll
            for (int e = 0; e < 4; ++e) { ha[e] = (__bf16)va[e]; hb[e] = (__bf16)vb[e]; }
            *(bf16x4*)(As + row * LDS_STRIDE_H + c4) = ha;
            *(bf16x4*)(Bs + row * LDS_STRIDE_H + c4) = hb;
        }
        __syncthreads();
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int st = 0; st < BK / 16; ++st) {
            bf16x8 af[WT], bfr[WT];
#pragma unroll
            for (int a = 0; a < WT; ++a) {
                af[a] = *(const bf16x8*)(As + (wm + a * 32 + r) * LDS_STRIDE_H + 16 * st + 8 * h);
                bfr[a] = *(const bf16x8*)(Bs + (wn + a * 32 + r) * LDS_STRIDE_H + 16 * st + 8 * h);
            }
#pragma unroll
            for (int a = 0; a < WT; ++a)
#pragma unroll
                for (int b = 0; b < WT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
    if (g.ksplit > 1) {   // raw partial of this K slice
        float* P = g.part + (size_t)blockIdx.z * g.M * g.N;
#pragma unroll
        for (int a = 0; a < WT; ++a)
#pragma unroll
            for (int b = 0; b < WT; ++b) {
                const int n = n0 + wn + b * 32 + (lane & 31);
                if (n >= g.N) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < g.M) P[(size_t)m * g.N + n] = acc[a][b][r];
                }
            }
        return;
    }
    epilogue<WT, WT>(g, acc, m0, n0, wm, wn, lane);
}

// fp32 GEMM as three bf16 planes (round 5): every fp32 operand x is split exactly into
// x = hi + mid + lo, three bf16 numbers (8 significant bits each, 24 in all: hi = bf16(x),
// mid = bf16(x - hi), lo = x - hi - mid, every subtraction exact in fp32), and
//   a . b = sum over the six plane pairs of order <= 2^-16:  hi.hi + hi.mid + mid.hi + hi.lo + lo.hi + mid.mid
// on v_mfma_f32_32x32x16_bf16 (bf16 x bf16 products are exact in fp32, fp32 accumulation). The
// dropped pairs (mid.lo, lo.mid, lo.lo) are below 2^-24 of |a b|: the same order as the one fp32
// rounding of an fp32 product, so the result is an fp32 GEMM in accuracy (measured against an fp64
// reference beside the native f32-input MFMA: tests/test_rollout_gpu.py) at 12 MFMA cycles per k
// instead of 32 (v_mfma_f32_32x32x2_f32: 64 cycles for k = 2; the bf16 form: 32 cycles for k = 16).
// Same tiles, k loop (register double buffering), split-K and epilogues as gemm_nt_kernel; the
// planes are formed while staging into LDS.
// (KMPC_DTYPE_F32 is this form; KMPC_DTYPE_F32_F32MFMA selects gemm_nt_kernel at run time.)
__device__ __forceinline__ void split3(float x, __bf16& hi, __bf16& mid, __bf16& lo) {
    hi = (__bf16)x;
    const float r1 = x - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}

template <int WM, int WN, int GM = 2, int GN = 2, int BKT = BK>
__global__ void __launch_bounds__(64 * GM * GN) gemm_nt_x3_kernel(GemmArgs g) {
    constexpr int NT = 64 * GM * GN;
    constexpr int TM = 32 * GM * WM, TN = 32 * GN * WN;
    constexpr int NS = BKT / 16;               // 16-k MFMA steps per k-tile (BKT = 32: two)
    static_assert(NS * 16 == BKT && NS >= 1, "k-tile of whole 16-k steps");
    constexpr int LS = BKT + 8;                // bf16 elements per LDS row (80 B: aligned ds_read_b128)
    // two buffers when they fit and the workgroup alone holds four waves per SIMD (a smaller one
    // keeps the single buffer: two workgroups per CU share the LDS)
    constexpr bool DB = 2 * 3 * (TM + TN) * LS * 2 <= 160 * 1024 && GM * GN >= 16;
    constexpr int NB = DB ? 2 : 1;
    __shared__ __bf16 As[NB][3][TM * LS];
    __shared__ __bf16 Bs[NB][3][TN * LS];
    static_assert(sizeof(As) + sizeof(Bs) <= 160 * 1024, "LDS");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int m0, n0;
    xcd_tile(m0, n0, TM, TN);
    const int wm = (wv / GN) * 32 * WM, wn = (wv % GN) * 32 * WN;
    f32x16 acc[WM][WN];
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    const bool vec_ok = ((g.lda & 3) == 0) && ((g.ldb & 3) == 0) &&
                        ((((uintptr_t)g.A) & 15) == 0) && ((((uintptr_t)g.B) & 15) == 0);
    int kbeg = 0, kend = g.K;
    if (g.ksplit > 1) {
        const int kc = ((g.K + g.ksplit * BKT - 1) / (g.ksplit * BKT)) * BKT;
        kbeg = blockIdx.z * kc;
        kend = min(g.K, kbeg + kc);
    }
    constexpr int QA = TM * BKT / (4 * NT), QB = TN * BKT / (4 * NT);
    static_assert(QA * 4 * NT == TM * BKT && QB * 4 * NT == TN * BKT, "tile loads per thread");
    constexpr int RQ = BKT / 4;
    f32x4 va[QA], vb[QB];
    auto fetch_row = [&](const float* P, int ld, int rows, int r0, int row, int kk, f32x4& v) {
        v = f32x4{0.f, 0.f, 0.f, 0.f};
        const int rr = r0 + row;
        if (rr >= rows) return;
        if (vec_ok && kk + 3 < kend) {
            v = *(const f32x4*)(P + (size_t)rr * ld + kk);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (kk + e < kend) v[e] = P[(size_t)rr * ld + kk + e];
        }
    };
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < QA; ++q) {
            const int idx = tid + q * NT;
            fetch_row(g.A, g.lda, g.M, m0, idx / RQ, k0 + (idx % RQ) * 4, va[q]);
        }
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            const int idx = tid + q * NT;
            fetch_row(g.B, g.ldb, g.N, n0, idx / RQ, k0 + (idx % RQ) * 4, vb[q]);
        }
    };
    auto put = [&](__bf16* S0, __bf16* S1, __bf16* S2, int idx, const f32x4& v) {
        bf16x4 h, m, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            __bf16 x0, x1, x2;
            split3(v[e], x0, x1, x2);
            h[e] = x0; m[e] = x1; l[e] = x2;
        }
        const int o = (idx / RQ) * LS + (idx % RQ) * 4;
        *(bf16x4*)(S0 + o) = h;
        *(bf16x4*)(S1 + o) = m;
        *(bf16x4*)(S2 + o) = l;
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < QA; ++q) put(As[buf][0], As[buf][1], As[buf][2], tid + q * NT, va[q]);
#pragma unroll
        for (int q = 0; q < QB; ++q) put(Bs[buf][0], Bs[buf][1], Bs[buf][2], tid + q * NT, vb[q]);
    };
    auto substep = [&](int buf, int st) {   // lane (r, h): k = 16 st + 8 h + j
        const int r = lane & 31, h = lane >> 5;
        {
            bf16x8 af[3][WM], bf[3][WN];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int a = 0; a < WM; ++a)
                    af[p][a] = *(const bf16x8*)(As[buf][p] + (wm + a * 32 + r) * LS + 16 * st + 8 * h);
#pragma unroll
                for (int b = 0; b < WN; ++b)
                    bf[p][b] = *(const bf16x8*)(Bs[buf][p] + (wn + b * 32 + r) * LS + 16 * st + 8 * h);
            }
#pragma unroll
            for (int a = 0; a < WM; ++a)
#pragma unroll
                for (int b = 0; b < WN; ++b) {
                    // the small pairs first, hi.hi last (fixed order: deterministic)
                    f32x16 c = acc[a][b];
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][a], bf[1][b], c, 0, 0, 0);   // mid.mid
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2][a], bf[0][b], c, 0, 0, 0);   // lo.hi
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][a], bf[2][b], c, 0, 0, 0);   // hi.lo
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][a], bf[0][b], c, 0, 0, 0);   // mid.hi
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][a], bf[1][b], c, 0, 0, 0);   // hi.mid
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][a], bf[0][b], c, 0, 0, 0);   // hi.hi
                    acc[a][b] = c;
                }
        }
    };
    if constexpr (DB) {
        // one barrier per k-tile: tile k's MFMA steps read buffer k & 1 while tile k + 1 (fetched
        // into registers one iteration earlier) is split into the other buffer between them
        fetch(kbeg);
        stage(0);
        if (kbeg + BKT < kend) fetch(kbeg + BKT);
        __syncthreads();
        int buf = 0;
        for (int k0 = kbeg; k0 < kend; k0 += BKT) {
            substep(buf, 0);
            if (k0 + BKT < kend) {
                stage(buf ^ 1);
                if (k0 + 2 * BKT < kend) fetch(k0 + 2 * BKT);
            }
#pragma unroll
            for (int st = 1; st < NS; ++st) substep(buf, st);
            __syncthreads();
            buf ^= 1;
        }
    } else {
        fetch(kbeg);
        for (int k0 = kbeg; k0 < kend; k0 += BKT) {
            stage(0);
            __syncthreads();
            if (k0 + BKT < kend) fetch(k0 + BKT);
#pragma unroll
            for (int st = 0; st < NS; ++st) substep(0, st);
            __syncthreads();
        }
    }
    if (g.ksplit > 1) {   // raw partial of this K slice
        float* P = g.part + (size_t)blockIdx.z * g.M * g.N;
#pragma unroll
        for (int a = 0; a < WM; ++a)
#pragma unroll
            for (int b = 0; b < WN; ++b) {
                const int n = n0 + wn + b * 32 + (lane & 31);
                if (n >= g.N) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < g.M) P[(size_t)m * g.N + n] = acc[a][b][r];
                }
            }
        return;
    }
    epilogue<WM, WN>(g, acc, m0, n0, wm, wn, lane);
}

}  // namespace kmpc
