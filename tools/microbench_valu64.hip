// microbench_valu64.hip -- issue rates of the f64 VALU instructions the f64 all-pairs kernels are made of (kernels_bf64.hip),
// on the whole chip, and the LDS crossbar beside them.  Build: hipcc --offload-arch=gfx950 -O3 tools/microbench_valu64.hip -o ...
// Prints the implied cycles per wave-instruction per SIMD at the clock measured with s_memtime/s_memrealtime (as
// tools/microbench_valu.hip does for fp32).  The ds_bpermute rows chain each bpermute on its own previous result: they
// measure mostly the crossbar's latency, not its issue cost.
#include <hip/hip_runtime.h>
#include <cstdio>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); return 1; } } while (0)

constexpr int ITERS = 2048;

template <int KIND>
__global__ __launch_bounds__(256) void k(double* out, double b, double c, unsigned long long* clk) {
    double a0 = threadIdx.x + 1.0, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    const int src = ((threadIdx.x + 63) & 63) * 4;
    int r0 = threadIdx.x, r1 = r0 + 1, r2 = r0 + 2, r3 = r0 + 3, r4 = r0 + 4, r5 = r0 + 5;
    unsigned long long t0 = __builtin_amdgcn_s_memtime(), q0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < ITERS; ++i) {
        if (KIND == 0) {  // 8 independent v_fma_f64
            asm volatile("v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n v_fma_f64 %3, %3, %8, %9\n"
                         "v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n v_fma_f64 %6, %6, %8, %9\n v_fma_f64 %7, %7, %8, %9\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));
        } else if (KIND == 1) {  // 8 independent v_mul_f64
            asm volatile("v_mul_f64 %0, %0, %8\n v_mul_f64 %1, %1, %8\n v_mul_f64 %2, %2, %8\n v_mul_f64 %3, %3, %8\n"
                         "v_mul_f64 %4, %4, %8\n v_mul_f64 %5, %5, %8\n v_mul_f64 %6, %6, %8\n v_mul_f64 %7, %7, %8\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
        } else if (KIND == 2) {  // 8 independent v_add_f64
            asm volatile("v_add_f64 %0, %0, %8\n v_add_f64 %1, %1, %8\n v_add_f64 %2, %2, %8\n v_add_f64 %3, %3, %8\n"
                         "v_add_f64 %4, %4, %8\n v_add_f64 %5, %5, %8\n v_add_f64 %6, %6, %8\n v_add_f64 %7, %7, %8\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));
        } else if (KIND == 3) {  // 8 independent v_rsq_f64
            asm volatile("v_rsq_f64 %0, %0\n v_rsq_f64 %1, %1\n v_rsq_f64 %2, %2\n v_rsq_f64 %3, %3\n"
                         "v_rsq_f64 %4, %4\n v_rsq_f64 %5, %5\n v_rsq_f64 %6, %6\n v_rsq_f64 %7, %7\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7));
        } else if (KIND == 4) {  // 8 fma : 1 rsq (does the transcendental co-issue with f64 FMAs?)
            asm volatile("v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n v_rsq_f64 %7, %7\n"
                         "v_fma_f64 %3, %3, %8, %9\n v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n v_fma_f64 %6, %6, %8, %9\n"
                         "v_fma_f64 %0, %0, %8, %9\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));
        } else if (KIND == 5) {  // 8 fma beside 6 ds_bpermute_b32 (a k_bf64_sym step's accumulator rotation per 8 f64 ops)
            asm volatile("v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n v_fma_f64 %3, %3, %8, %9\n"
                         "v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n v_fma_f64 %6, %6, %8, %9\n v_fma_f64 %7, %7, %8, %9\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));
            r0 = __builtin_amdgcn_ds_bpermute(src, r0); r1 = __builtin_amdgcn_ds_bpermute(src, r1); r2 = __builtin_amdgcn_ds_bpermute(src, r2);
            r3 = __builtin_amdgcn_ds_bpermute(src, r3); r4 = __builtin_amdgcn_ds_bpermute(src, r4); r5 = __builtin_amdgcn_ds_bpermute(src, r5);
        } else if (KIND == 6) {  // 6 ds_bpermute_b32 alone
            r0 = __builtin_amdgcn_ds_bpermute(src, r0); r1 = __builtin_amdgcn_ds_bpermute(src, r1); r2 = __builtin_amdgcn_ds_bpermute(src, r2);
            r3 = __builtin_amdgcn_ds_bpermute(src, r3); r4 = __builtin_amdgcn_ds_bpermute(src, r4); r5 = __builtin_amdgcn_ds_bpermute(src, r5);
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime(), q1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) { clk[0] = t1 - t0; clk[1] = q1 - q0; }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + double(r0 + r1 + r2 + r3 + r4 + r5);
}

template <int KIND>
int run(const char* name, int instr_per_iter, int waves_per_simd, double* out, unsigned long long* clk) {
    const int blocks = 256 * waves_per_simd;  // 256 CUs x 4 SIMDs x waves_per_simd waves / 4 waves per block
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, out, 1.0001, 0.5, clk);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    const int reps = 5;
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, out, 1.0001, 0.5, clk);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0; CHECK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long h[2]; CHECK(hipMemcpy(h, clk, sizeof(h), hipMemcpyDeviceToHost));
    const double ghz = double(h[0]) / double(h[1]) * 0.1;  // s_memrealtime ticks at 100 MHz
    const double us = ms * 1e3 / reps;
    const double cyc = us * 1e3 * ghz / (double(ITERS) * instr_per_iter * waves_per_simd);
    printf("%-34s waves/SIMD=%d  %8.1f us  clock %.2f GHz  %.2f cycles per wave-instruction per SIMD\n", name, waves_per_simd, us, ghz, cyc);
    return 0;
}

int main() {
    double* out; unsigned long long* clk;
    CHECK(hipMalloc(&out, sizeof(double) * 256 * 8 * 256));
    CHECK(hipMalloc(&clk, 16));
    for (int w : {2, 4}) {
        if (run<0>("v_fma_f64", 8, w, out, clk)) return 1;
        if (run<1>("v_mul_f64", 8, w, out, clk)) return 1;
        if (run<2>("v_add_f64", 8, w, out, clk)) return 1;
        if (run<3>("v_rsq_f64", 8, w, out, clk)) return 1;
        if (run<4>("8 fma : 1 rsq mix (9 instr)", 9, w, out, clk)) return 1;
        if (run<5>("8 fma + 6 ds_bpermute (per fma)", 8, w, out, clk)) return 1;
        if (run<6>("6 ds_bpermute alone (per bpermute)", 6, w, out, clk)) return 1;
    }
    return 0;
}
