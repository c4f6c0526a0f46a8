// Pooled rows after the sampler.  Long recordings: the stitch of enhanced windows back into their recordings (storm_crossfade_rows) and the
// host-side design of its ramp (storm_crossfade_ramp).  Posterior ensembles (below the stitch): K draws per utterance combined into one
// estimate with a per-bin spread and per-row agreement numbers (storm_ensemble_combine_rows).  Definitions in include/storm_hip.h.
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

// ---- posterior ensembles (definition in include/storm_hip.h) --------------------------------------------------------------------------------
// Two launches for the whole batch:
//   ensemble_combine_kernel  a stream.  One workgroup of four waves per STORM_ENSEMBLE_TILE consecutive bins (i = f T + t) of one utterance; a
//                            thread owns the bin pairs l, l + 256, ... of the tile.  Per pair it reads the K draws' two bins as ONE 16-byte
//                            load each (every pool element is read once; scalar loads where a pair is cut by the row's end, by frames[b] or by
//                            a pool row that does not start on 16 bytes - the same values, so the same bits), keeps them in registers, and
//                            works through the two bins one after the other in fp64: back-transform, mean, combined value, spread, and the
//                            bin's terms of E and d_0 .. d_{K-1} added to the thread's K + 1 running sums.  The draw loops are instantiated
//                            for K <= 8 / 16 / 32 and fully unrolled: nothing is indexed at run time, nothing lives in scratch memory.
//                            The tile's K + 1 sums (butterfly, wave order) go to caller-owned scratch.
//   ensemble_rows_kernel     one wave per utterance: lane j adds sum j's tile partials in tile order, lane 0 forms D and the medoid draw.
// No atomics; the cut depends on the bin index only.
constexpr int ENSEMBLE_TILE = STORM_ENSEMBLE_TILE, ENSEMBLE_THREADS = 256, ENSEMBLE_MAX_DRAWS = STORM_ENSEMBLE_MAX_DRAWS;
constexpr int ENSEMBLE_PAIRS = ENSEMBLE_TILE / 2 / ENSEMBLE_THREADS;             // bin pairs per thread
static_assert(ENSEMBLE_PAIRS * 2 * ENSEMBLE_THREADS == ENSEMBLE_TILE, "STORM_ENSEMBLE_TILE: a multiple of two bins per thread of a 256-thread workgroup");
static_assert(ENSEMBLE_MAX_DRAWS == 32, "STORM_ENSEMBLE_MAX_DRAWS: the widest instantiation of the draw loop");

// Batcher's odd-even merge sort for N = 2^q values as a list of compare-exchanges, built at compile time: every index of the network is a
// constant, so the values stay in registers.
template <int N> struct SortNet { int n; unsigned char lo[N * N], hi[N * N]; };
template <int N> constexpr SortNet<N> make_sort_net() {
    SortNet<N> s{};
    for (int p = 1; p < N; p <<= 1)
        for (int k = p; k >= 1; k >>= 1)
            for (int j = k % p; j + k < N; j += 2 * k)
                for (int i = 0; i < k && i + j + k < N; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) { s.lo[s.n] = (unsigned char)(i + j); s.hi[s.n] = (unsigned char)(i + j + k); ++s.n; }
    return s;
}
template <int N, int C = 0> __device__ __forceinline__ void sort_ascending(double (&v)[N]) {
    constexpr SortNet<N> net = make_sort_net<N>();
    if constexpr (C < net.n) {
        const double a = v[net.lo[C]], b = v[net.hi[C]];
        v[net.lo[C]] = fmin(a, b);
        v[net.hi[C]] = fmax(a, b);
        sort_ascending<N, C + 1>(v);
    }
}

// one bin: steps 1 - 4 of the definition and the bin's terms of step 5 (acc[0] += |c|^2, acc[1 + k] += |x_k - c|^2).  Every product and sum is a
// statement of its own kind below and the build does not contract them.
template <int KMAX>
__device__ __forceinline__ void ensemble_bin(const float (&re)[KMAX], const float (&im)[KMAX], int K, double factor, double e, int mode,
                                             double (&acc)[KMAX + 1], float& o_re, float& o_im, float& o_s) {
#pragma clang fp contract(off)
    double xr[KMAX], xi[KMAX], g[KMAX];
    const double inv_e = 1.0 / e, Kd = (double)K;
    double sr = 0.0, si = 0.0, sg = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        xr[k] = 0.0; xi[k] = 0.0; g[k] = HUGE_VAL;                             // (past K: sorted behind every draw, never added)
        if (k < K) {
            const double a = (double)re[k], b = (double)im[k];
            const double aa = a * a, bb = b * b;
            const double r = sqrt(aa + bb);
            double gk = 0.0, gr = 0.0, gi = 0.0;
            if (r != 0.0) {
                const double m = r / factor;
                gk = e == 1.0 ? m : (e == 0.5 ? m * m : pow(m, inv_e));
                const double ur = a / r, ui = b / r;
                gr = gk * ur;
                gi = gk * ui;
            }
            xr[k] = gr; xi[k] = gi; g[k] = gk;
            sr += gr; si += gi; sg += gk;
        }
    }
    const double cr = sr / Kd, ci = si / Kd;
    const double crr = cr * cr, cii = ci * ci;
    const double cn2 = crr + cii;
    acc[0] += cn2;
    double sd = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            const double dr = xr[k] - cr, di = xi[k] - ci;
            const double drr = dr * dr, dii = di * di;
            const double q = drr + dii;
            acc[1 + k] += q;
            sd += q;
        }
    }
    o_s = K > 1 ? (float)sqrt(sd / (double)(K - 1)) : 0.f;
    if (mode == STORM_ENSEMBLE_MEAN) { o_re = (float)cr; o_im = (float)ci; return; }
    double a = sg / Kd;
    if (mode == STORM_ENSEMBLE_MAG_MEDIAN) {
        sort_ascending<KMAX>(g);
        const int lo = (K - 1) / 2, hi = K / 2;
        double vlo = 0.0, vhi = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k == lo) vlo = g[k];
            if (k == hi) vhi = g[k];
        }
        a = lo == hi ? vlo : 0.5 * (vlo + vhi);
    }
    const double n = sqrt(cn2);
    double vr = 0.0, vi = 0.0;
    if (n != 0.0) {
        const double ur = cr / n, ui = ci / n;
        vr = a * ur;
        vi = a * ui;
    }
    o_re = (float)vr; o_im = (float)vi;
}

template <int KMAX>
__global__ void __launch_bounds__(ENSEMBLE_THREADS)
ensemble_combine_kernel(const float2* __restrict__ pool, long long pool_stride, int N, const int* __restrict__ draw_row, float2* __restrict__ out,
                        float* __restrict__ spread, double* __restrict__ part, int K, int F, int T, const int* __restrict__ frames, double factor,
                        double e, int mode) {
    __shared__ double red[KMAX + 1][ENSEMBLE_THREADS / 64];
    const int b = blockIdx.y, l = threadIdx.x;
    const int n = F * T;                                                       // (the host refuses F T >= 2^31)
    int valid = frames ? frames[b] : T;
    if (valid > T) valid = T;                                                  // (a device-side count the host never saw must still not read outside the row)
    const int* rows = draw_row + (long long)b * K;
    float2* orow = out + (long long)b * n;
    float* srow = spread ? spread + (long long)b * n : nullptr;
    double acc[KMAX + 1];
#pragma unroll
    for (int j = 0; j <= KMAX; ++j) acc[j] = 0.0;
    for (int pj = 0; pj < ENSEMBLE_PAIRS; ++pj) {
        const long long i64 = (long long)blockIdx.x * ENSEMBLE_TILE + 2 * (l + ENSEMBLE_THREADS * pj);
        if (i64 >= n) break;                                                   // (ascending: nothing of this thread lies behind it)
        const int i = (int)i64;
        const bool has1 = i + 1 < n;
        const bool in0 = i % T < valid, in1 = has1 && (i + 1) % T < valid;
        float re0[KMAX], im0[KMAX], re1[KMAX], im1[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            re0[k] = im0[k] = re1[k] = im1[k] = 0.f;
            if (k < K) {
                const int row = rows[k];
                const float2* p = (row >= 0 && row < N) ? pool + (long long)row * pool_stride + i : nullptr;
                if (p && in0 && in1 && ((uintptr_t)p & 15) == 0) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    re0[k] = v.x; im0[k] = v.y; re1[k] = v.z; im1[k] = v.w;
                } else if (p) {
                    if (in0) { const float2 v = p[0]; re0[k] = v.x; im0[k] = v.y; }
                    if (in1) { const float2 v = p[1]; re1[k] = v.x; im1[k] = v.y; }
                }
            }
        }
        float o[4] = {0.f, 0.f, 0.f, 0.f}, s[2] = {0.f, 0.f};
        if (in0) ensemble_bin<KMAX>(re0, im0, K, factor, e, mode, acc, o[0], o[1], s[0]);
        if (in1) ensemble_bin<KMAX>(re1, im1, K, factor, e, mode, acc, o[2], o[3], s[1]);
        if (has1 && ((uintptr_t)(orow + i) & 15) == 0) {
            *reinterpret_cast<float4*>(orow + i) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            orow[i] = make_float2(o[0], o[1]);
            if (has1) orow[i + 1] = make_float2(o[2], o[3]);
        }
        if (srow) {
            if (has1 && ((uintptr_t)(srow + i) & 7) == 0) {
                *reinterpret_cast<float2*>(srow + i) = make_float2(s[0], s[1]);
            } else {
                srow[i] = s[0];
                if (has1) srow[i + 1] = s[1];
            }
        }
    }
#pragma unroll
    for (int j = 0; j <= KMAX; ++j) {
        if (j <= K) {                                                          // (uniform in the workgroup)
            const double w = wave_sum_d(acc[j]);
            if ((l & 63) == 0) red[j][l >> 6] = w;
        }
    }
    __syncthreads();
    if (l <= K)
        part[((long long)b * gridDim.x + blockIdx.x) * (K + 1) + l] = ((red[l][0] + red[l][1]) + red[l][2]) + red[l][3];
}

// part[b][tile][K + 1] -> rows_out[b] = (E, D, d_0 .. d_{K-1}) and best[b]: lane j adds sum j's tile partials in tile order from +0
__global__ void __launch_bounds__(64)
ensemble_rows_kernel(const double* __restrict__ part, double* __restrict__ rows_out, int* __restrict__ best, int K, int ntiles) {
    __shared__ double tot[ENSEMBLE_MAX_DRAWS + 1];
    const int b = blockIdx.x, j = threadIdx.x;
    if (j <= K) {
        double s = 0.0;
        for (int x = 0; x < ntiles; ++x) s += part[((long long)b * ntiles + x) * (K + 1) + j];
        tot[j] = s;
    }
    __syncthreads();
    double* o = rows_out + (long long)b * (2 + K);
    if (j == 0) {
        double s = 0.0;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            s += tot[1 + k];
            if (tot[1 + k] < tot[1 + arg]) arg = k;                            // (strictly smaller: the lowest k of a tie stays)
        }
        o[0] = tot[0];
        o[1] = s / (double)K;
        best[b] = arg;
    }
    if (j < K) o[2 + j] = tot[1 + j];
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

extern "C" long long storm_ensemble_scratch_bytes(int B, int F, int T, int K) {
    if (B <= 0 || B > 65535 || F <= 0 || T <= 0 || (long long)F * T > 0x7fffffffll || K < 1 || K > STORM_ENSEMBLE_MAX_DRAWS) return 0;
    const long long tiles = ((long long)F * T + storm::ENSEMBLE_TILE - 1) / storm::ENSEMBLE_TILE;
    return (long long)B * tiles * (K + 1) * (long long)sizeof(double);
}

extern "C" int storm_ensemble_combine_rows(const float* pool, int N, long long pool_stride, const int* draw_row, float* out, float* spread,
                                           double* rows_out, int* best, void* scratch, long long scratch_bytes, int B, int K, int F, int T,
                                           const int* frames, float factor, float exponent, int mode, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(pool && draw_row && out && rows_out && best && scratch, "storm_ensemble_combine_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && F >= 1 && T >= 1 && (long long)F * T <= 0x7fffffffll, "storm_ensemble_combine_rows: B=%d F=%d T=%d", B, F, T);
    STORM_CHECK(K >= 1 && K <= ENSEMBLE_MAX_DRAWS, "storm_ensemble_combine_rows: K=%d outside [1, %d]", K, ENSEMBLE_MAX_DRAWS);
    STORM_CHECK(N >= 1 && pool_stride >= (long long)F * T, "storm_ensemble_combine_rows: a pool of N=%d rows with pool_stride=%lld for rows of %lld bins", N,
                pool_stride, (long long)F * T);
    STORM_CHECK(((uintptr_t)pool & 15) == 0 && ((uintptr_t)out & 15) == 0, "storm_ensemble_combine_rows: pool %p and out %p must be 16-byte aligned",
                (const void*)pool, (void*)out);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= storm_ensemble_scratch_bytes(B, F, T, K),
                "storm_ensemble_combine_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)", scratch, scratch_bytes,
                storm_ensemble_scratch_bytes(B, F, T, K));
    STORM_CHECK(mode == STORM_ENSEMBLE_MEAN || mode == STORM_ENSEMBLE_MAG_MEAN || mode == STORM_ENSEMBLE_MAG_MEDIAN,
                "storm_ensemble_combine_rows: mode=%d (0 mean, 1 mag_mean, 2 mag_median)", mode);
    STORM_CHECK(factor > 0.f && exponent > 0.f, "storm_ensemble_combine_rows: factor=%g exponent=%g (both must be positive)", (double)factor, (double)exponent);
    const int tiles = (int)(((long long)F * T + ENSEMBLE_TILE - 1) / ENSEMBLE_TILE);
    const dim3 grid((unsigned)tiles, B), block(ENSEMBLE_THREADS);
    hipStream_t hs = (hipStream_t)st;
    const float2* p2 = reinterpret_cast<const float2*>(pool);
    float2* o2 = reinterpret_cast<float2*>(out);
    double* part = (double*)scratch;
    const double fd = (double)factor, ed = (double)exponent;
    if (K <= 8)
        hipLaunchKernelGGL(ensemble_combine_kernel<8>, grid, block, 0, hs, p2, pool_stride, N, draw_row, o2, spread, part, K, F, T, frames, fd, ed, mode);
    else if (K <= 16)
        hipLaunchKernelGGL(ensemble_combine_kernel<16>, grid, block, 0, hs, p2, pool_stride, N, draw_row, o2, spread, part, K, F, T, frames, fd, ed, mode);
    else
        hipLaunchKernelGGL(ensemble_combine_kernel<32>, grid, block, 0, hs, p2, pool_stride, N, draw_row, o2, spread, part, K, F, T, frames, fd, ed, mode);
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ensemble_rows_kernel, dim3(B), dim3(64), 0, hs, (const double*)part, rows_out, best, K, tiles);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
