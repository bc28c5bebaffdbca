// Dev probe: what a packed float32 instruction costs a lone wave on gfx950. One wave per SIMD
// (256-thread workgroups, one per CU, waves_per_eu(1)), pure VALU stream, operands in registers:
// the float32 phase of the C3 solve kernel runs this way, and the SLP vectoriser packs some of its
// element-wise arithmetic into v_pk_*_f32. Times dependent (1 chain) and independent (8 chains)
// streams of v_fma_f32, v_pk_fma_f32, v_pk_mul_f32 and v_pk_add_f32, written as asm so that each
// line is exactly the instruction named, and prints cycles per instruction and per scalar
// operation (a packed instruction does two).
// Build: hipcc -O3 --offload-arch=gfx950 tools/dev/pk_f32_rate.hip -o tools/dev/pk_f32_rate
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int UNROLL = 16;

enum Kind { FMA = 0, PK_FMA = 1, PK_MUL = 2, PK_ADD = 3 };

template <int KIND, int NCH>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k(float* out, long long* cyc, int n, float af, float bf) {
    f2 x[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) x[c] = f2{1.0f + threadIdx.x * 1e-6f + c, 1.0f - threadIdx.x * 1e-6f + c};
    const f2 a = f2{af, af}, b = f2{bf, bf};
    const long long t0 = clock64();
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if constexpr (KIND == FMA) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(x[c].x) : "v"(af), "v"(bf));
                else if constexpr (KIND == PK_FMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(x[c]) : "v"(a), "v"(b));
                else if constexpr (KIND == PK_MUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(x[c]) : "v"(a));
                else asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(x[c]) : "v"(b));
            }
        }
    }
    const long long t1 = clock64();
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) s += x[c].x + x[c].y;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

static int g_blocks = 256;

template <int KIND, int NCH>
void run(const char* name, float* out, long long* cyc, int n) {
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        hipLaunchKernelGGL((k<KIND, NCH>), dim3(g_blocks), dim3(256), 0, 0, out, cyc, n, 0.999999f, 1e-7f);
        if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); return; }
        static long long h[1024];
        (void)hipMemcpy(h, cyc, sizeof(long long) * g_blocks, hipMemcpyDeviceToHost);
        double m = 0;
        for (int i = 0; i < g_blocks; ++i) m += (double)h[i];
        m /= g_blocks;
        if (m < best) best = m;
    }
    const double per_instr = best / ((double)n * UNROLL * NCH);
    const int ops = KIND == FMA ? 1 : 2;
    printf("%-13s chains %d: %6.2f cycles per instruction, %6.2f per scalar %s\n", name, NCH, per_instr,
           per_instr / ops, KIND == FMA || KIND == PK_FMA ? "FMA" : (KIND == PK_MUL ? "mul" : "add"));
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
    g_blocks = p.multiProcessorCount < 1024 ? p.multiProcessorCount : 1024;   // one workgroup per CU
    float* out; long long* cyc;
    (void)hipMalloc(&out, sizeof(float) * 1024 * 256);
    (void)hipMalloc(&cyc, sizeof(long long) * 1024);
    const int n = 2048;
    printf("%s, %d workgroups of 4 waves (one wave per SIMD), clock64 ticks\n", p.name, g_blocks);
    run<FMA, 1>("v_fma_f32", out, cyc, n);   // (first launch: warm-up of the clocks, repeated below)
    run<FMA, 1>("v_fma_f32", out, cyc, n);
    run<FMA, 8>("v_fma_f32", out, cyc, n);
    run<PK_FMA, 1>("v_pk_fma_f32", out, cyc, n);
    run<PK_FMA, 8>("v_pk_fma_f32", out, cyc, n);
    run<PK_MUL, 1>("v_pk_mul_f32", out, cyc, n);
    run<PK_MUL, 8>("v_pk_mul_f32", out, cyc, n);
    run<PK_ADD, 1>("v_pk_add_f32", out, cyc, n);
    run<PK_ADD, 8>("v_pk_add_f32", out, cyc, n);
    (void)hipFree(out);
    (void)hipFree(cyc);
    return 0;
}
