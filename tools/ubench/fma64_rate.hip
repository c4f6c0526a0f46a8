// Micro-benchmark: the fp64 FMA rate of the whole device - the yardstick of storm_xcorr_lag_rows (tools/align_time.py divides the delay
// search's own FMA count by it).  Every lane runs 8 independent v_fma_f64 chains; 8 waves per SIMD keep every pipe full.
// hipcc --offload-arch=gfx950 -O3 fma64_rate.hip -o fma64_rate; prints "fp64 FMA rate: <x> GFMA/s" (median of 5 launches).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>

__global__ __launch_bounds__(256) void k(double* out, int iters) {
    double v[8];
    for (int i = 0; i < 8; ++i) v[i] = 0.5 + 0.01 * (double)((threadIdx.x & 63) + i);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = fma(v[i], 1.0000001, 1e-9);
    }
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += v[i];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int blocks = p.multiProcessorCount * 8, iters = 20000;       // 8 workgroups of 4 waves per CU
    double* out;
    if (hipMalloc(&out, (size_t)blocks * 256 * sizeof(double)) != hipSuccess) return 1;
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    float ms[6];
    for (int r = 0; r < 6; ++r) {                                      // the first launch is the warm-up
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, out, iters);
        (void)hipEventRecord(b, 0);
        if (hipEventSynchronize(b) != hipSuccess) return 1;
        (void)hipEventElapsedTime(&ms[r], a, b);
    }
    std::sort(ms + 1, ms + 6);
    const double fmas = (double)blocks * 256.0 * 8.0 * (double)iters;
    printf("fp64 FMA rate: %.1f GFMA/s (%d CUs, %.3f ms for %.3e FMAs, median of 5 launches)\n", fmas / (ms[3] * 1e-3) / 1e9, p.multiProcessorCount, ms[3], fmas);
    (void)hipFree(out);
    return 0;
}
