// fma_f64_sgpr.hip - does v_fma_f64 pay for a scalar-register operand on gfx950?  (v_fma_f32 does: it issues at half rate with
// one, DESIGN.md.)  The loop of fma_f64_rate.hip twice: both multiplicands in vector registers, and one of them wave-uniform
// (a kernel argument the compiler keeps in a scalar register pair and names as the operand; check with -save-temps that the
// loop reads `v_fma_f64 v[..], s[..], v[..], v[..]`).  The lag kernel of the time correlation functions (molar_amd/csrc/tcf.hip)
// multiplies a wave-uniform origin value by a per-lane window value: this decides whether the origin may sit in scalar registers.
// Prints per (operands, waves per SIMD): wall time (best of five) and wave-wide FMAs per second of the whole device in units of
// 1e12 lane operations.
// Build: hipcc --offload-arch=gfx950 -O3 fma_f64_sgpr.hip -o fma_f64_sgpr
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int ITER = 20000;
constexpr int NACC = 8;

template <bool UNIFORM>
__global__ void __launch_bounds__(1024) k(double *out, double a0, double b0) {
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    const double a = UNIFORM ? a0 : a0 + threadIdx.x * 1e-9, b = b0 - threadIdx.x * 1e-9;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = fma(a, b, acc[i]);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i];
    if (s == 12345.678) out[0] = s;                                               // keeps the accumulators alive
}

template <bool UNIFORM>
int run(int cus, int waves_per_simd) {
    double *out;
    CHECK(hipMalloc(&out, 8));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const dim3 grid(cus), block(256 * waves_per_simd);
    hipLaunchKernelGGL(k<UNIFORM>, grid, block, 0, 0, out, 0.3, 0.7);
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k<UNIFORM>, grid, block, 0, 0, out, 0.3, 0.7);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double lane_fmas = (double)ITER * NACC * waves_per_simd * 4.0 * cus * 64.0;
    printf("operands %s waves_per_simd %d ms %.4f tfma %.3f\n", UNIFORM ? "sgpr_vgpr" : "vgpr_vgpr", waves_per_simd, best, lane_fmas / (best * 1e-3) / 1e12);
    CHECK(hipFree(out));
    return 0;
}

int main() {
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    printf("device %s cus %d\n", p.gcnArchName, p.multiProcessorCount);
    int rc = 0;
    for (int w = 1; w <= 4; w *= 2) {
        rc |= run<false>(p.multiProcessorCount, w);
        rc |= run<true>(p.multiProcessorCount, w);
    }
    return rc;
}
