// Long recordings: the stitch of enhanced windows back into their recordings (storm_crossfade_rows) and the host-side design of its ramp
// (storm_crossfade_ramp).  Definitions in include/storm_hip.h.
// A gather: output sample m of recording r reads window k = min(m / H, n_r - 1) at j = m - k H and, in the first V samples of a window that
// has a predecessor, that predecessor at j + H; out = prev + ramp[j] (cur - prev) as three separate fp32 operations.  One workgroup owns
// STORM_CROSSFADE_TILE consecutive outputs of one recording, a thread four consecutive ones.  No atomics, nothing is accumulated and no
// output reads another output: a sample's bits depend on its own recording's windows only, whatever the grid, the launch's other recordings
// or the pool's row order.  Four samples that lie in one window and on one side of the fade's end move as 16-byte loads and one 16-byte
// store where every address allows it - the same operations per sample as the scalar path.
// Included by spectral.hip alone (kernel and entry points live in that translation unit).
#pragma once
#include <math.h>
#include "common.h"

namespace storm {

constexpr int CROSSFADE_TILE = STORM_CROSSFADE_TILE, CROSSFADE_THREADS = 256, CROSSFADE_PER_THREAD = 4;
static_assert(CROSSFADE_THREADS * CROSSFADE_PER_THREAD == CROSSFADE_TILE, "STORM_CROSSFADE_TILE: four outputs per thread of a 256-thread workgroup");

// the three operations of the fade, one statement each: no compiler may contract the product into the sum
__device__ __forceinline__ float crossfade_mix(float prev, float cur, float w) {
    const float d = cur - prev;
    const float p = w * d;
    return prev + p;
}

// pool row of window `slot` of the launch's win_row table, or nullptr for a skipped window (-1; an entry outside the pool reads as one too:
// the host refuses such a table, the kernel must still not read outside the pool)
__device__ __forceinline__ const float* crossfade_row(const float* __restrict__ pool, long long pool_stride, const int* __restrict__ win_row,
                                                      int slot, int N) {
    const int row = win_row[slot];
    return (row >= 0 && row < N) ? pool + (long long)row * pool_stride : nullptr;
}

__global__ void __launch_bounds__(CROSSFADE_THREADS)
crossfade_rows_kernel(const float* __restrict__ pool, long long pool_stride, int N, float* __restrict__ out, long long out_stride, long long width,
                      const int* __restrict__ rec_len, const int* __restrict__ rec_windows, const int* __restrict__ rec_first,
                      const int* __restrict__ win_row, int W, int V, const float* __restrict__ ramp) {
    const int r = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * CROSSFADE_TILE + (long long)CROSSFADE_PER_THREAD * threadIdx.x;
    if (m0 >= width) return;
    const int H = W - V, n = rec_windows[r], first = rec_first[r];
    long long len = n >= 1 ? (long long)rec_len[r] : 0;
    const long long covered = n >= 1 ? (long long)(n - 1) * H + W : 0;         // (a length the host never saw must still not read past a window's end)
    if (len > covered) len = covered;
    if (len > width) len = width;
    float* o = out + (long long)r * out_stride + m0;

    if (m0 + 3 < len) {
        long long kk = m0 / H;
        const int k = (int)(kk < n - 1 ? kk : n - 1), j = (int)(m0 - (long long)k * H);
        const bool fade = k > 0 && j + 3 < V, plain = k == 0 || j >= V;
        const long long k3 = (m0 + 3) / H;
        if ((k3 < n - 1 ? k3 : n - 1) == k && (fade || plain) && ((uintptr_t)o & 15) == 0) {
            const float* pc = crossfade_row(pool, pool_stride, win_row, first + k, N);
            const float* pp = fade ? crossfade_row(pool, pool_stride, win_row, first + k - 1, N) : nullptr;
            const bool ok_c = !pc || ((uintptr_t)(pc + j) & 15) == 0, ok_p = !pp || ((uintptr_t)(pp + j + H) & 15) == 0;
            if (ok_c && ok_p && (!fade || ((uintptr_t)(ramp + j) & 15) == 0)) {
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                float4 c = pc ? *reinterpret_cast<const float4*>(pc + j) : zero;
                if (fade) {
                    const float4 p = pp ? *reinterpret_cast<const float4*>(pp + j + H) : zero;
                    const float4 w = *reinterpret_cast<const float4*>(ramp + j);
                    c = make_float4(crossfade_mix(p.x, c.x, w.x), crossfade_mix(p.y, c.y, w.y), crossfade_mix(p.z, c.z, w.z), crossfade_mix(p.w, c.w, w.w));
                }
                *reinterpret_cast<float4*>(o) = c;
                return;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < CROSSFADE_PER_THREAD; ++e) {
        const long long m = m0 + e;
        if (m >= width) break;
        float v = 0.f;                                                         // samples from the recording's length up to the width
        if (m < len) {
            const long long kk = m / H;
            const int k = (int)(kk < n - 1 ? kk : n - 1), j = (int)(m - (long long)k * H);
            const float* pc = crossfade_row(pool, pool_stride, win_row, first + k, N);
            v = pc ? pc[j] : 0.f;
            if (k > 0 && j < V) {
                const float* pp = crossfade_row(pool, pool_stride, win_row, first + k - 1, N);
                v = crossfade_mix(pp ? pp[j + H] : 0.f, v, ramp[j]);
            }
        }
        o[e] = v;
    }
}

}  // namespace storm

extern "C" int storm_crossfade_ramp(int V, int kind, float* out) {
    STORM_CHECK(out != nullptr, "storm_crossfade_ramp: null pointer");
    STORM_CHECK(V >= 1, "storm_crossfade_ramp: V=%d (at least 1)", V);
    STORM_CHECK(kind == STORM_RAMP_HANN || kind == STORM_RAMP_LINEAR, "storm_crossfade_ramp: kind=%d (0 hann, 1 linear)", kind);
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < V; ++j) {                                              // fp64, rounded to fp32 once
        const double u = (double)(j + 1) / (double)(V + 1);
        if (kind == STORM_RAMP_LINEAR) { out[j] = (float)u; continue; }
        const double s = sin(pi / 2.0 * (double)(j + 1) / (double)(V + 1));
        out[j] = (float)(s * s);
    }
    return STORM_OK;
}

extern "C" int storm_crossfade_rows(const float* pool, int N, long long pool_stride, float* out, int R, long long width, long long out_stride,
                                    const int* rec_len, const int* rec_windows, const int* rec_first, const int* win_row, int W, int V,
                                    const float* ramp, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(pool && out && rec_len && rec_windows && rec_first && win_row && ramp, "storm_crossfade_rows: null pointer");
    STORM_CHECK(W >= 2 && V >= 1 && V <= W / 2, "storm_crossfade_rows: V=%d outside [1, W / 2] for W=%d", V, W);
    STORM_CHECK(N >= 1 && pool_stride >= W, "storm_crossfade_rows: a pool of %d rows with stride %lld for windows of %d", N, pool_stride, W);
    STORM_CHECK(R >= 1 && R <= 65535 && width >= 1 && out_stride >= width, "storm_crossfade_rows: R=%d width=%lld out_stride=%lld", R, width, out_stride);
    const long long tiles = (width + CROSSFADE_TILE - 1) / CROSSFADE_TILE;
    STORM_CHECK(tiles <= 0x7fffffffll, "storm_crossfade_rows: width=%lld", width);
    hipLaunchKernelGGL(crossfade_rows_kernel, dim3((unsigned)tiles, R), dim3(CROSSFADE_THREADS), 0, (hipStream_t)st, pool, pool_stride, N, out, out_stride,
                       width, rec_len, rec_windows, rec_first, win_row, W, V, ramp);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
