// Dev probe: what one step of the Schur triangular solves' substitution chain costs a lone wave on
// gfx950, in the two forms lsolve() can take (kmpc_solve_kernel.h). One wave per SIMD (256-thread
// workgroups, one per CU, waves_per_eu(1)), multipliers in registers, lane r owns row r (r < 30):
//   readlane  29 steps x = fma(-l[j], readlane(x, j), x): v_readlane into SGPRs (one in float32, two
//             in float64) and an FMA that reads them — written in C++, so the compiler places the
//             wait states it needs, as in the product;
//   dpp       29 steps of v_fmac_*_dpp x, x, -l[j] row_newbcast:(j & 15), each behind the two wait
//             states a DPP read needs after a VALU write of its source (s_nop 1): the cost of a chain
//             step alone (the values are those of two separate 16-lane chains);
//   blocked   the chain over DPP rows 0 and 1 as lsolve() runs it: 15 steps inside row 0, a
//             permlane16 swap, 16 block updates of row 1 from the swapped register, 13 steps inside
//             row 1 (44 FMAs for 29 steps).
// Prints clock64 ticks per chain and per step of the 29, float32 and float64.
// Build: hipcc -O3 --offload-arch=gfx950 tools/dev/trisolve_chain_rate.hip -o tools/dev/trisolve_chain_rate
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <utility>

constexpr int K1 = 29;   // steps of a KM = 30 chain

enum Form { READLANE = 0, DPP = 1, BLOCKED = 2 };

__device__ __forceinline__ float rl(float v, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}
__device__ __forceinline__ double rl(double v, int j) {
    const int2 x = __builtin_bit_cast(int2, v);
    return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(x.x, j), __builtin_amdgcn_readlane(x.y, j)));
}
__device__ __forceinline__ void rows(float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(int, a), __builtin_bit_cast(int, b), false, false);
    a = __builtin_bit_cast(float, r[0]);
    b = __builtin_bit_cast(float, r[1]);
}
__device__ __forceinline__ void rows(double& a, double& b) {
    const int2 x = __builtin_bit_cast(int2, a), y = __builtin_bit_cast(int2, b);
    const auto r0 = __builtin_amdgcn_permlane16_swap(x.x, y.x, false, false);
    const auto r1 = __builtin_amdgcn_permlane16_swap(x.y, y.y, false, false);
    a = __builtin_bit_cast(double, make_int2(r0[0], r1[0]));
    b = __builtin_bit_cast(double, make_int2(r0[1], r1[1]));
}

// one step: x = fma(-l, lane LANE of the row of SRC, x) on the DPP rows in RM
template <int LANE, int RM, bool SELF>
__device__ __forceinline__ void step(float& x, float c, float l) {
    if constexpr (SELF) asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %0, -%1 row_newbcast:%2 row_mask:%3 bank_mask:0xf"
                                     : "+v"(x) : "v"(l), "n"(LANE), "n"(RM));
    else asm volatile("v_fmac_f32_dpp %0, %1, -%2 row_newbcast:%3 row_mask:%4 bank_mask:0xf"
                      : "+v"(x) : "v"(c), "v"(l), "n"(LANE), "n"(RM));
}
template <int LANE, int RM, bool SELF>
__device__ __forceinline__ void step(double& x, double c, double l) {
    if constexpr (SELF) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%1 row_newbcast:%2 row_mask:%3 bank_mask:0xf"
                                     : "+v"(x) : "v"(l), "n"(LANE), "n"(RM));
    else asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:%4 bank_mask:0xf"
                      : "+v"(x) : "v"(c), "v"(l), "n"(LANE), "n"(RM));
}
template <int J0, int RM, bool SELF, class T, int... I>
__device__ __forceinline__ void steps(T& x, T c, const T (&l)[K1], std::integer_sequence<int, I...>) {
    (step<(J0 + I) & 15, RM, SELF>(x, c, l[J0 + I]), ...);
}

template <int FORM, class T>
__device__ __forceinline__ void chain(T& x, const T (&l)[K1]) {
    if constexpr (FORM == READLANE) {
#pragma unroll
        for (int j = 0; j < K1; ++j) x = fma(-l[j], rl(x, j), x);
    } else if constexpr (FORM == DPP) {
        steps<0, 0xf, true>(x, x, l, std::make_integer_sequence<int, K1>{});
    } else {
        steps<0, 0x1, true>(x, x, l, std::make_integer_sequence<int, 15>{});
        asm volatile("s_nop 1" : "+v"(x));
        T a = x, b = x;
        rows(a, b);
        asm volatile("s_nop 1" : "+v"(a));
        steps<0, 0x2, false>(x, a, l, std::make_integer_sequence<int, 16>{});
        steps<16, 0x2, true>(x, x, l, std::make_integer_sequence<int, K1 - 16>{});
    }
}

template <int FORM, class T>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k(T* out, long long* cyc, int n, T lv) {
    T l[K1];
    const int r = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < K1; ++j) l[j] = j < r ? lv * (T)(1 + ((j + r) & 3)) : (T)0;   // strictly lower
    T x = (T)1 + (T)r * (T)1e-3;
    const long long t0 = clock64();
    for (int i = 0; i < n; ++i) {
        chain<FORM>(x, l);
        asm volatile("" : "+v"(x));
    }
    const long long t1 = clock64();
    out[blockIdx.x * blockDim.x + threadIdx.x] = x;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

static int g_blocks = 256;

template <int FORM, class T>
void run(const char* name, void* out, long long* cyc, int n) {
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        hipLaunchKernelGGL((k<FORM, T>), dim3(g_blocks), dim3(256), 0, 0, (T*)out, cyc, n, (T)1e-3);
        if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return; }
        static long long h[1024];
        (void)hipMemcpy(h, cyc, sizeof(long long) * g_blocks, hipMemcpyDeviceToHost);
        double m = 0;
        for (int i = 0; i < g_blocks; ++i) m += (double)h[i];
        m /= g_blocks;
        if (m < best) best = m;
    }
    const double per_chain = best / n;
    printf("%-18s %8.1f ticks per chain of %d steps, %6.2f per step\n", name, per_chain, K1, per_chain / K1);
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
    g_blocks = p.multiProcessorCount < 1024 ? p.multiProcessorCount : 1024;   // one workgroup per CU
    void* out; long long* cyc;
    (void)hipMalloc(&out, sizeof(double) * 1024 * 256);
    (void)hipMalloc(&cyc, sizeof(long long) * 1024);
    const int n = 4096;
    printf("%s, %d workgroups of 4 waves (one wave per SIMD), clock64 ticks\n", p.name, g_blocks);
    run<READLANE, float>("f32 readlane", out, cyc, n);   // (first launch: warm-up of the clocks, repeated below)
    run<READLANE, float>("f32 readlane", out, cyc, n);
    run<DPP, float>("f32 dpp", out, cyc, n);
    run<BLOCKED, float>("f32 dpp blocked", out, cyc, n);
    run<READLANE, double>("f64 readlane", out, cyc, n);
    run<DPP, double>("f64 dpp", out, cyc, n);
    run<BLOCKED, double>("f64 dpp blocked", out, cyc, n);
    (void)hipFree(out);
    (void)hipFree(cyc);
    return 0;
}
