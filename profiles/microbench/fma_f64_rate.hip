// fma_f64_rate.hip - back-to-back issue rate of v_fma_f64 on gfx950: the roof the lag kernel of the mean-squared displacement
// (molar_amd/csrc/msd.hip) is held against.  One workgroup of 4 * WAVES waves per CU (WAVES waves per SIMD), each wave ITER
// rounds over NACC independent accumulators, operands in registers, nothing else in the loop.  Prints, per (WAVES, NACC): wall
// time (best of five), wave-wide FMAs per second of the whole device in units of 1e12 lane operations, and cycles per
// instruction per SIMD at the clock the runtime reports (the chip may hold a lower one: the rate is the one to compare against).
// Build: hipcc --offload-arch=gfx950 -O3 fma_f64_rate.hip -o fma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

constexpr int ITER = 20000;

template <int NACC>
__global__ void __launch_bounds__(1024) k(double *out, double a0, double b0) {
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    const double a = a0 + threadIdx.x * 1e-9, b = b0 - threadIdx.x * 1e-9;        // random-looking, finite, not zero
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = fma(a, b, acc[i]);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i];
    if (s == 12345.678) out[0] = s;                                               // keeps the accumulators alive
}

template <int NACC>
int run(int cus, int waves_per_simd, double mhz) {
    double *out;
    CHECK(hipMalloc(&out, 8));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const dim3 grid(cus), block(256 * waves_per_simd);
    hipLaunchKernelGGL(k<NACC>, grid, block, 0, 0, out, 0.3, 0.7);
    CHECK(hipDeviceSynchronize());
    float best = 1e30f;
    for (int r = 0; r < 5; ++r) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k<NACC>, grid, block, 0, 0, out, 0.3, 0.7);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    const double insts_per_simd = (double)ITER * NACC * waves_per_simd;
    const double lane_fmas = insts_per_simd * 4.0 * cus * 64.0;
    printf("waves_per_simd %d nacc %d ms %.4f tfma %.3f cycles_per_fma %.2f\n", waves_per_simd, NACC, best, lane_fmas / (best * 1e-3) / 1e12,
           best * 1e-3 * mhz * 1e6 / insts_per_simd);
    CHECK(hipFree(out));
    return 0;
}

int main() {
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const double mhz = p.clockRate / 1000.0;
    printf("device %s cus %d clock_mhz %.0f\n", p.gcnArchName, p.multiProcessorCount, mhz);
    int rc = 0;
    rc |= run<1>(p.multiProcessorCount, 1, mhz);
    rc |= run<8>(p.multiProcessorCount, 1, mhz);
    rc |= run<8>(p.multiProcessorCount, 2, mhz);
    rc |= run<8>(p.multiProcessorCount, 4, mhz);
    return rc;
}
