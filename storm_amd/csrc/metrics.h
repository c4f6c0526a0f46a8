// Evaluation metrics of enhanced audio on the device (the reference's util/other.py: si_sdr_components / energy_ratios :21-44, snr_dB :96-100,
// lsd :16-19) - streaming reductions, one pass over the inputs.  Definitions in include/storm_hip.h.
// Both metrics share one structure: a row is cut at FIXED positions (STORM_METRICS_CHUNK samples; LSD_FRAMES x LSD_BINS spectrogram tiles),
// one workgroup sums one piece in fp64 in an order that depends on the position inside the piece only, writes its partial to caller-owned
// scratch, and a second kernel adds a row's partials in index order and forms the numbers.  No atomics; the cut depends on the sample /
// (bin, frame) index only, so a row's results are the same bits at any batch size, batch width, row stride and position in the batch.
// The frame-based measures (segmental SNR, log-likelihood ratio, LPC cepstral distance; the reference has none of them) follow below the
// two: frames cut at fixed positions, per-frame numbers in caller-owned scratch, a row kernel with sums in index order.
// Included by spectral.hip alone (kernels and entry points live in that translation unit).
#pragma once
#include "common.h"

namespace storm {

constexpr int METRICS_THREADS = 256;
constexpr int ENERGY_CHUNK = STORM_METRICS_CHUNK;                      // samples per workgroup
constexpr int ENERGY_GROUPS = ENERGY_CHUNK / 4 / METRICS_THREADS;      // float4 groups per thread: thread t owns groups t, t + 256, ...
constexpr int ENERGY_UNROLL = 4;                                       // groups whose loads are issued before the first is used
constexpr int ENERGY_GRAM = 6;                                         // <h,s> <h,n> <s,s> <n,n> <s,n> <h,h>  (h = s_hat)
static_assert(ENERGY_GROUPS * 4 * METRICS_THREADS == ENERGY_CHUNK && ENERGY_GROUPS % ENERGY_UNROLL == 0, "STORM_METRICS_CHUNK: a multiple of 4096");
constexpr int LSD_FRAMES = 64, LSD_BINS = 32;                          // a workgroup's tile: one lane per frame, 8 bins per wave
constexpr int LSD_BINS_PER_WAVE = LSD_BINS / (METRICS_THREADS / 64);
constexpr double ENERGY_EPS = 1e-10;                                   // si_sdr_components' own default: energy_ratios never passes its eps on (other.py:38)

// four samples of a chunk at offset k (m = the chunk's valid samples): one 16-byte load where the row allows it, zeros past m
__device__ __forceinline__ float4 metrics_load4(const float* __restrict__ p, int k, int m, bool vec) {
    if (vec && k + 3 < m) return *reinterpret_cast<const float4*>(p + k);
    return make_float4(k < m ? p[k] : 0.f, k + 1 < m ? p[k + 1] : 0.f, k + 2 < m ? p[k + 2] : 0.f, k + 3 < m ? p[k + 3] : 0.f);
}

// part[b][chunk][6]: the Gram entries of (s_hat, s, n) over samples [chunk CHUNK, (chunk + 1) CHUNK) below the row's length.  fp32 x fp32 is
// exact in fp64, so every fma adds an exact product; a thread walks its samples in ascending order whatever the alignment (the scalar path of a
// row that does not start on 16 bytes adds the same numbers in the same order), zeros past the length add +0.
__global__ void __launch_bounds__(METRICS_THREADS)
energy_partials_kernel(const float* __restrict__ sh, const float* __restrict__ s, const float* __restrict__ n, double* __restrict__ part,
                       long long L, long long stride_h, long long stride_s, long long stride_n, const int* __restrict__ row_len) {
    __shared__ double red[ENERGY_GRAM][METRICS_THREADS / 64];
    const int b = blockIdx.y, t = threadIdx.x;
    long long len = row_len ? (long long)row_len[b] : L;
    if (len > L) len = L;                                              // (a device-side length the host never saw must still not read outside the row)
    const long long i0 = (long long)blockIdx.x * ENERGY_CHUNK;
    if (i0 >= len) return;                                             // (uniform in the workgroup) a chunk past the row: the row sum never reads its slot
    const int m = (int)(len - i0 < ENERGY_CHUNK ? len - i0 : ENERGY_CHUNK);
    const float* ph = sh + (long long)b * stride_h + i0;
    const float* ps = s + (long long)b * stride_s + i0;
    const float* pn = n + (long long)b * stride_n + i0;
    const bool vec = (((uintptr_t)ph | (uintptr_t)ps | (uintptr_t)pn) & 15) == 0;
    double a[ENERGY_GRAM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < ENERGY_GROUPS; j0 += ENERGY_UNROLL) {
        if (4 * (t + METRICS_THREADS * j0) >= m) break;
        float4 h4[ENERGY_UNROLL], s4[ENERGY_UNROLL], n4[ENERGY_UNROLL];
#pragma unroll
        for (int u = 0; u < ENERGY_UNROLL; ++u) {
            const int k = 4 * (t + METRICS_THREADS * (j0 + u));
            h4[u] = metrics_load4(ph, k, m, vec); s4[u] = metrics_load4(ps, k, m, vec); n4[u] = metrics_load4(pn, k, m, vec);
        }
#pragma unroll
        for (int u = 0; u < ENERGY_UNROLL; ++u) {
            const float hv[4] = {h4[u].x, h4[u].y, h4[u].z, h4[u].w}, sv[4] = {s4[u].x, s4[u].y, s4[u].z, s4[u].w},
                        nv[4] = {n4[u].x, n4[u].y, n4[u].z, n4[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double h = hv[e], x = sv[e], v = nv[e];
                a[0] = fma(h, x, a[0]); a[1] = fma(h, v, a[1]); a[2] = fma(x, x, a[2]);
                a[3] = fma(v, v, a[3]); a[4] = fma(x, v, a[4]); a[5] = fma(h, h, a[5]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < ENERGY_GRAM; ++g) {
        const double w = wave_sum_d(a[g]);
        if ((t & 63) == 0) red[g][t >> 6] = w;
    }
    __syncthreads();
    if (t < ENERGY_GRAM)
        part[((long long)b * gridDim.x + blockIdx.x) * ENERGY_GRAM + t] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
}

// one thread per row: the row's partials in chunk order, then the four numbers from the Gram entries.
//   alpha_s = <h,s> / (eps + <s,s>), alpha_n = <h,n> / (eps + <n,n>)                                   (other.py:23, 27)
//   |s_target|^2 = alpha_s^2 <s,s>,  |e_noise|^2 = alpha_n^2 <n,n>
//   |e_noise + e_art|^2 = |h - alpha_s s|^2 = <h,h> - 2 alpha_s <h,s> + alpha_s^2 <s,s>
//   |e_art|^2 = |h - alpha_s s - alpha_n n|^2 = <h,h> + alpha_s^2 <s,s> + alpha_n^2 <n,n> - 2 alpha_s <h,s> - 2 alpha_n <h,n> + 2 alpha_s alpha_n <s,n>
//   ratio = 10 log10(eps + |s_target|^2 / (eps + |.|^2))                                                 (other.py:40-42)
//   input SNR = 10 log10((<s,s> / len) / (<n,n> / len))                                                  (other.py:96-100)
__global__ void energy_finish_kernel(const double* __restrict__ part, double* __restrict__ out, long long L, const int* __restrict__ row_len,
                                     int nchunks, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    long long len = row_len ? (long long)row_len[b] : L;
    if (len > L) len = L;
    const int nc = len <= 0 ? 0 : (int)((len + ENERGY_CHUNK - 1) / ENERGY_CHUNK);
    double g[ENERGY_GRAM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < ENERGY_GRAM; ++k) g[k] += part[((long long)b * nchunks + c) * ENERGY_GRAM + k];
    const double hs = g[0], hn = g[1], ss = g[2], nn = g[3], sn = g[4], hh = g[5], eps = ENERGY_EPS;
    const double as = hs / (eps + ss), an = hn / (eps + nn);
    const double target = as * as * ss, noise = an * an * nn;
    const double resid = hh - 2.0 * as * hs + target;
    const double art = hh + target + noise - 2.0 * as * hs - 2.0 * an * hn + 2.0 * as * an * sn;
    const double n_samples = (double)len;
    out[4 * b + 0] = 10.0 * log10(eps + target / (eps + resid));
    out[4 * b + 1] = 10.0 * log10(eps + target / (eps + noise));
    out[4 * b + 2] = 10.0 * log10(eps + target / (eps + art));
    out[4 * b + 3] = 10.0 * log10((ss / n_samples) / (nn / n_samples));
}

// part[b][bin tile][frame tile]: sum over the tile's (f, t < frames_b) of |2 ln(eps + |A|) - 2 ln(eps + |S|)| in fp64 (other.py:18-19; the
// magnitudes are formed in fp64 from the complex64 parts, whose squares are exact there).  Lane = frame (a wave reads 512 contiguous bytes of a
// bin's row per load), a wave owns bins w, w + 4, ... of the tile; all of a thread's loads are issued before the first logarithm.
__global__ void __launch_bounds__(METRICS_THREADS)
lsd_partials_kernel(const float* __restrict__ A, const float* __restrict__ S, double* __restrict__ part, int F, int T,
                    const int* __restrict__ row_frames, double eps) {
    __shared__ double red[METRICS_THREADS / 64];
    const int b = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int frames = row_frames ? row_frames[b] : T;
    if (frames > T) frames = T;                                        // (a device-side count the host never saw must still not read outside the row)
    const int t0 = blockIdx.x * LSD_FRAMES;
    if (t0 >= frames) return;                                          // (uniform) a tile of padding frames: the row sum never reads its slot
    const int t = t0 + lane, f0 = blockIdx.y * LSD_BINS + w;
    const float2* pa = reinterpret_cast<const float2*>(A) + (long long)b * F * T + t;
    const float2* ps = reinterpret_cast<const float2*>(S) + (long long)b * F * T + t;
    float2 av[LSD_BINS_PER_WAVE], sv[LSD_BINS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < LSD_BINS_PER_WAVE; ++i) {
        const int f = f0 + 4 * i;
        const bool in = t < frames && f < F;
        av[i] = in ? pa[(long long)f * T] : make_float2(0.f, 0.f);
        sv[i] = in ? ps[(long long)f * T] : make_float2(0.f, 0.f);
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LSD_BINS_PER_WAVE; ++i) {
        if (t < frames && f0 + 4 * i < F) {
            const double ma = sqrt((double)av[i].x * (double)av[i].x + (double)av[i].y * (double)av[i].y);
            const double ms = sqrt((double)sv[i].x * (double)sv[i].x + (double)sv[i].y * (double)sv[i].y);
            acc += fabs(2.0 * log(eps + ma) - 2.0 * log(eps + ms));
        }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        part[((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one thread per row: bin tiles in order, inside each the row's own frame tiles in order; sqrt(sum / (F frames_b))  (other.py:19: ONE mean, then the root)
__global__ void lsd_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int F, int T, const int* __restrict__ row_frames,
                                  int nbt, int nft, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int frames = row_frames ? row_frames[b] : T;
    if (frames > T) frames = T;
    const int nf = frames <= 0 ? 0 : (frames + LSD_FRAMES - 1) / LSD_FRAMES;
    double sum = 0.0;
    for (int y = 0; y < nbt; ++y)
        for (int x = 0; x < nf; ++x) sum += part[((long long)b * nbt + y) * nft + x];
    out[b] = sqrt(sum / ((double)F * (double)frames));
}

// ---- frame-based measures: segmental SNR, log-likelihood ratio, LPC cepstral distance (definition in include/storm_hip.h) -----------------
// Three launches for the whole batch:
//   lpc_frames_kernel   one workgroup of four waves per LPC_TILE consecutive frames of one row (the cut depends on the frame index only).
//                       The strip of both signals that the tile's frames share (they overlap by 3/4) and the window are staged in LDS once;
//                       wave v owns frames v, v + 4, ... of the tile: it writes the windowed frame into its own LDS buffer, lanes stride the
//                       samples, and the 17 lags and the error energy are reduced with wave_sum_d - first the clean frame, then the processed
//                       one through the same buffer.  It writes the segmental SNR and the 2 x 17 lags of every frame to the caller's scratch.
//   lpc_model_kernel    one LANE per frame: Levinson-Durbin, the cepstrum recursion and the quadratic form of both signals in registers, then
//                       LLR and CD (NaN for a void frame).  The recursions are serial chains of dependent fp64 operations: as the tail of the
//                       frames kernel they kept 16 lanes of a workgroup busy and the other 240 waiting (17.8 us per tile and CU on the
//                       MI355X); one lane per frame fills whole waves with them.
//   lpc_rows_kernel     one workgroup per row: the mean of the segmental SNR; the number of frames that are not void; for LLR and for CD the
//                       n_keep-th smallest value T by a bisection over the fp64 bit pattern (63 counting passes, both measures at once - a
//                       non-negative double orders as its bits), then (sum of the values below T + (n_keep - their count) T) / n_keep.
// Every sum: thread t adds its elements t, t + threads, ... in ascending order, wave_sum_d, the four waves' sums in wave order.  No atomics.
constexpr int LPC_TILE = STORM_LPC_TILE;                               // frames per workgroup
constexpr int LPC_MAX_W = 2048, LPC_MAX_P = 16, LPC_LAGS = LPC_MAX_P + 1;
constexpr int LPC_FPW = LPC_TILE / (METRICS_THREADS / 64);             // frames per wave
constexpr int LPC_KEEP = 32;                                           // frames per thread that lpc_rows_kernel keeps in registers
constexpr double LPC_EPS = 2.220446049250313e-16;                      // 2^-52
constexpr double LPC_STOP = 9.094947017729282e-13;                     // 2^-40: Levinson-Durbin stops before an order with E <= 2^-40 r[0]
constexpr double LPC_PI = 3.14159265358979323846;
constexpr double LPC_DB = 4.342944819032518;                           // 10 / ln 10

// W, H, P of a sample rate; false = refused (2 P < W <= 2048)
__host__ __device__ inline bool lpc_shape(int fs, int& W, int& H, int& P) {
    if (fs < 1) return false;
    const long long w = (30ll * fs + 500) / 1000;
    P = fs >= 10000 ? 16 : 10;
    if (w <= 2 * P || w > LPC_MAX_W) return false;
    W = (int)w; H = W / 4;
    return true;
}
__host__ __device__ inline long long lpc_frames(long long len, int W, int H) { return len >= W ? (len - W) / H : 0; }
__device__ __forceinline__ long long lpc_row_len(const int* row_len, int b, long long L) {
    long long len = row_len ? (long long)row_len[b] : L;
    return len > L ? L : len;                                          // (a device-side length the host never saw must still not read outside the row)
}
// v clamped to [lo, hi]; a NaN stays NaN, -0 becomes +0
__device__ __forceinline__ double lpc_clamp(double v, double lo, double hi) { return (v < lo ? lo : (v > hi ? hi : v)) + 0.0; }

// the dynamic LDS of lpc_frames_kernel, doubles first: win[W], buf[4][W + 16]; then the two strips
__host__ __device__ inline int lpc_strip(int W, int H) { return (LPC_TILE - 1) * H + W; }
__host__ __device__ inline int lpc_lds_doubles(int W) { return W + (METRICS_THREADS / 64) * (W + LPC_MAX_P); }
inline int lpc_lds_bytes(int W, int H) { return lpc_lds_doubles(W) * (int)sizeof(double) + 2 * lpc_strip(W, H) * (int)sizeof(float); }

// the 17 lags of the windowed frame in buf[0 .. W) (buf[W .. W + 16) is zero): lane l adds n = l, l + 64, ... ascending, then wave_sum_d.
// Lags past P are computed and not used.
__device__ __forceinline__ void lpc_lags(const double* __restrict__ buf, int W, int lane, double (&r)[LPC_LAGS]) {
#pragma unroll
    for (int k = 0; k < LPC_LAGS; ++k) r[k] = 0.0;
    for (int n = lane; n < W; n += 64) {
        const double v = buf[n];
#pragma unroll
        for (int k = 0; k < LPC_LAGS; ++k) r[k] = fma(v, buf[n + k], r[k]);
    }
#pragma unroll
    for (int k = 0; k < LPC_LAGS; ++k) r[k] = wave_sum_d(r[k]);
}

// One signal of one frame, in registers (every loop is unrolled: all indices are compile-time): Levinson-Durbin on the lags r, the cepstrum
// of 1 / A(z) and the quadratic form a' Toeplitz(rc) a (rows ascending, inside a row the columns ascending).  out[0] = the form,
// out[1 .. P] = the cepstrum.
template <int P>
__device__ __forceinline__ void lpc_model(const double* rl, const double* rcl, double (&out)[LPC_LAGS]) {
    double r[P + 1], a[P + 1], c[P + 1];
#pragma unroll
    for (int j = 0; j <= P; ++j) { r[j] = rl[j]; a[j] = 0.0; c[j] = 0.0; }
    a[0] = 1.0;
    if (r[0] > 0.0) {                                                  // (a void frame: nothing reads its numbers)
        double E = r[0];
        bool go = true;
#pragma unroll
        for (int i = 1; i <= P; ++i) {
            go = go && !(E <= LPC_STOP * r[0]);                        // stops before an order with E <= 2^-40 r[0]: the rest stays 0
            if (go) {
                double acc = r[i];
#pragma unroll
                for (int j = 1; j < i; ++j) acc += a[j] * r[i - j];
                const double k = -acc / E;
#pragma unroll
                for (int j = 1; 2 * j <= i; ++j) {                     // a_j += k a_{i-j} for all j < i at once, in pairs (j, i - j)
                    const double lo = a[j], hi = a[i - j];
                    a[j] = lo + k * hi;
                    if (j != i - j) a[i - j] = hi + k * lo;
                }
                a[i] = k;
                E *= 1.0 - k * k;
            }
        }
#pragma unroll
        for (int n = 1; n <= P; ++n) {
            double acc = 0.0;
#pragma unroll
            for (int k = 1; k < n; ++k) acc += ((double)k / (double)n) * c[k] * a[n - k];
            c[n] = -a[n] - acc;
        }
    }
#pragma unroll
    for (int j = 0; j <= P; ++j) r[j] = rcl[j];
    double form = 0.0;
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        double rowsum = 0.0;
#pragma unroll
        for (int j = 0; j <= P; ++j) rowsum += r[i > j ? i - j : j - i] * a[j];
        form += a[i] * rowsum;
    }
    out[0] = form;
#pragma unroll
    for (int n = 1; n <= P; ++n) out[n] = c[n];
}

// fr[b][m][0] = the segmental SNR of frame m, lags[b][m][s][k] = r[k] of its clean (s = 0) and processed (s = 1) windowed frame
__global__ void __launch_bounds__(METRICS_THREADS)
lpc_frames_kernel(const float* __restrict__ x, const float* __restrict__ y, const double* __restrict__ window, double* __restrict__ fr,
                  double* __restrict__ lags, long long L, long long stride_x, long long stride_y, const int* __restrict__ row_len,
                  long long Mmax, int W, int H) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = lpc_strip(W, H), WB = W + LPC_MAX_P;
    double* const win = reinterpret_cast<double*>(smem);
    double* const bufs = win + W;
    float* const xs = reinterpret_cast<float*>(bufs + (METRICS_THREADS / 64) * WB);
    float* const ys = xs + S;
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long m0 = (long long)blockIdx.x * LPC_TILE;
    const long long M = lpc_frames(lpc_row_len(row_len, b, L), W, H);
    if (m0 >= M) return;                                               // (uniform in the workgroup) a tile past the row's frames
    const int live = (int)(M - m0 < LPC_TILE ? M - m0 : LPC_TILE);     // frames of this tile; its samples end at (m0 + live - 1) H + W <= len
    {
        const float* px = x + (long long)b * stride_x + m0 * H;
        const float* py = y + (long long)b * stride_y + m0 * H;
        const int ns = (live - 1) * H + W;
        for (int i = t; i < ns; i += METRICS_THREADS) { xs[i] = px[i]; ys[i] = py[i]; }
        for (int i = t; i < W; i += METRICS_THREADS) win[i] = window[i];
        if (lane < LPC_MAX_P) bufs[wv * WB + W + lane] = 0.0;
    }
    __syncthreads();
    double* const buf = bufs + wv * WB;
    for (int i = 0; i < LPC_FPW; ++i) {                                // (every wave walks the barriers; a wave without a frame only waits)
        const int f = wv + i * (METRICS_THREADS / 64);
        const bool on = f < live;
        const long long m = (long long)b * Mmax + m0 + f;
        double r[LPC_LAGS];
        double ed = 0.0;
        if (on) {
            const float* fx = xs + f * H;
            const float* fy = ys + f * H;
            for (int n = lane; n < W; n += 64) {
                const double c = win[n] * (double)fx[n], p = win[n] * (double)fy[n], d = c - p;
                ed = fma(d, d, ed);
                buf[n] = c;
            }
        }
        __syncthreads();
        if (on) {
            lpc_lags(buf, W, lane, r);
            ed = wave_sum_d(ed);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < LPC_LAGS; ++k) lags[(m * 2 + 0) * LPC_LAGS + k] = r[k];
                fr[m * 3] = lpc_clamp(10.0 * log10(r[0] / (ed + LPC_EPS) + LPC_EPS), -10.0, 35.0);
            }
        }
        __syncthreads();                                               // (the clean frame is read: the buffer takes the processed one)
        if (on) {
            const float* fy = ys + f * H;
            for (int n = lane; n < W; n += 64) buf[n] = win[n] * (double)fy[n];
        }
        __syncthreads();
        if (on) {
            lpc_lags(buf, W, lane, r);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < LPC_LAGS; ++k) lags[(m * 2 + 1) * LPC_LAGS + k] = r[k];
            }
        }
        __syncthreads();                                               // (the next frame overwrites the buffer)
    }
}

// LLR and CD of a frame from its two rows of lags
template <int P>
__device__ __forceinline__ void lpc_frame_numbers(const double* r, double& llr, double& cd) {
    double oc[LPC_LAGS], op[LPC_LAGS];                                 // [0]: a' R_c a, [1 .. P]: the cepstrum; clean, processed
    lpc_model<P>(r, r, oc);
    lpc_model<P>(r + LPC_LAGS, r, op);
    double d2 = 0.0;
#pragma unroll
    for (int n = 1; n <= P; ++n) { const double d = oc[n] - op[n]; d2 += d * d; }
    llr = lpc_clamp(log(op[0] / oc[0]), 0.0, 2.0);
    cd = lpc_clamp(LPC_DB * sqrt(2.0 * d2), 0.0, 10.0);
}

// fr[b][m][1 .. 2] = (LLR, CD) of frame m, NaN for a void frame; frames_out (optional) gets the frame's three numbers, NaN past the row's own
// frames.  One lane per frame.
__global__ void __launch_bounds__(64)
lpc_model_kernel(const double* __restrict__ lags, double* __restrict__ fr, double* __restrict__ frames_out, long long L,
                 const int* __restrict__ row_len, long long Mmax, int W, int H, int P) {
    const int b = blockIdx.y;
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    if (f >= Mmax) return;
    const long long M = lpc_frames(lpc_row_len(row_len, b, L), W, H);
    const long long o = ((long long)b * Mmax + f) * 3;
    const double nan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    if (f >= M) {
        if (frames_out) { frames_out[o] = nan; frames_out[o + 1] = nan; frames_out[o + 2] = nan; }
        return;
    }
    const double* r = lags + ((long long)b * Mmax + f) * 2 * LPC_LAGS;
    double llr = nan, cd = nan;
    if (r[0] > 0.0 && r[LPC_LAGS] > 0.0) {
        if (P == 16) lpc_frame_numbers<16>(r, llr, cd);
        else lpc_frame_numbers<10>(r, llr, cd);
    }
    fr[o + 1] = llr; fr[o + 2] = cd;
    if (frames_out) { frames_out[o] = fr[o]; frames_out[o + 1] = llr; frames_out[o + 2] = cd; }
}

// the workgroup's sum of one double / two counts per thread: wave sums, then the waves in order (every thread returns the same bits)
__device__ __forceinline__ double lpc_block_sum(double v, double* red, int t) {
    v = wave_sum_d(v);
    __syncthreads();                                                   // (the previous use of red is read)
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ void lpc_block_count2(int& a, int& c, int* red, int t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    __syncthreads();
    if ((t & 63) == 0) { red[2 * (t >> 6)] = a; red[2 * (t >> 6) + 1] = c; }
    __syncthreads();
    a = red[0] + red[2] + red[4] + red[6];
    c = red[1] + red[3] + red[5] + red[7];
}

// out[b] = (mean segmental SNR, trimmed mean LLR, trimmed mean CD), counts[b] = (M, M'): one workgroup per row
__global__ void __launch_bounds__(METRICS_THREADS)
lpc_rows_kernel(const double* __restrict__ fr, double* __restrict__ out, int* __restrict__ counts, long long L, const int* __restrict__ row_len,
                long long Mmax, int W, int H) {
    __shared__ double red[METRICS_THREADS / 64];
    __shared__ int redi[2 * (METRICS_THREADS / 64)];
    const int b = blockIdx.x, t = threadIdx.x;
    const long long M = lpc_frames(lpc_row_len(row_len, b, L), W, H);
    const double* p = fr + (long long)b * Mmax * 3;
    const double nan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    double s = 0.0;
    int nv = 0, unused = 0;
    // the row's first LPC_KEEP x 256 frames (61 s at 16 kHz) stay in this thread's registers as bit patterns, all ones for a void frame or none:
    // the counting passes below read only the frames past them from memory
    unsigned long long k1[LPC_KEEP], k2[LPC_KEEP];
#pragma unroll
    for (int i = 0; i < LPC_KEEP; ++i) {
        const long long m = t + (long long)i * METRICS_THREADS;
        k1[i] = ~0ull; k2[i] = ~0ull;
        if (m < M) {
            const double v1 = p[3 * m + 1], v2 = p[3 * m + 2];
            s += p[3 * m];
            if (v1 == v1) { ++nv; k1[i] = __builtin_bit_cast(unsigned long long, v1); k2[i] = __builtin_bit_cast(unsigned long long, v2); }   // (a void frame's LLR is NaN)
        }
    }
    for (long long m = t + (long long)LPC_KEEP * METRICS_THREADS; m < M; m += METRICS_THREADS) {
        s += p[3 * m];
        nv += p[3 * m + 1] == p[3 * m + 1] ? 1 : 0;
    }
    s = lpc_block_sum(s, red, t);
    lpc_block_count2(nv, unused, redi, t);
    const int keep = nv < 1 ? 0 : ((19 * (long long)nv + 10) / 20 < 1 ? 1 : (int)((19 * (long long)nv + 10) / 20));   // max(1, floor(0.95 M' + 0.5))
    if (t == 0) {
        counts[2 * b] = (int)M; counts[2 * b + 1] = nv;
        out[3 * b] = M > 0 ? s / (double)M : nan;
    }
    if (keep == 0) {                                                   // (uniform in the workgroup)
        if (t == 0) { out[3 * b + 1] = nan; out[3 * b + 2] = nan; }
        return;
    }
    // T = the keep-th smallest bit pattern: bit by bit from the top, a bit is set when fewer than `keep` values lie below the pattern with it
    unsigned long long T1 = 0ull, T2 = 0ull;
    for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long c1 = T1 | (1ull << bit), c2 = T2 | (1ull << bit);
        int n1 = 0, n2 = 0;
#pragma unroll
        for (int i = 0; i < LPC_KEEP; ++i) { n1 += k1[i] < c1 ? 1 : 0; n2 += k2[i] < c2 ? 1 : 0; }
        for (long long m = t + (long long)LPC_KEEP * METRICS_THREADS; m < M; m += METRICS_THREADS) {
            const double v1 = p[3 * m + 1], v2 = p[3 * m + 2];
            if (v1 == v1) {
                n1 += __builtin_bit_cast(unsigned long long, v1) < c1 ? 1 : 0;
                n2 += __builtin_bit_cast(unsigned long long, v2) < c2 ? 1 : 0;
            }
        }
        lpc_block_count2(n1, n2, redi, t);
        if (n1 < keep) T1 = c1;
        if (n2 < keep) T2 = c2;
    }
    const double t1 = __builtin_bit_cast(double, T1), t2 = __builtin_bit_cast(double, T2);
    double s1 = 0.0, s2 = 0.0;
    int n1 = 0, n2 = 0;
#pragma unroll
    for (int i = 0; i < LPC_KEEP; ++i) {
        if (k1[i] < T1) { s1 += __builtin_bit_cast(double, k1[i]); ++n1; }
        if (k2[i] < T2) { s2 += __builtin_bit_cast(double, k2[i]); ++n2; }
    }
    for (long long m = t + (long long)LPC_KEEP * METRICS_THREADS; m < M; m += METRICS_THREADS) {
        const double v1 = p[3 * m + 1], v2 = p[3 * m + 2];
        if (v1 == v1) {
            if (v1 < t1) { s1 += v1; ++n1; }
            if (v2 < t2) { s2 += v2; ++n2; }
        }
    }
    s1 = lpc_block_sum(s1, red, t);
    s2 = lpc_block_sum(s2, red, t);
    lpc_block_count2(n1, n2, redi, t);
    if (t == 0) {
        out[3 * b + 1] = (s1 + (double)(keep - n1) * t1) / (double)keep;
        out[3 * b + 2] = (s2 + (double)(keep - n2) * t2) / (double)keep;
    }
}

}  // namespace storm

extern "C" long long storm_energy_ratios_scratch_bytes(int B, long long L) {
    if (B <= 0 || L <= 0) return 0;
    return (long long)B * ((L + storm::ENERGY_CHUNK - 1) / storm::ENERGY_CHUNK) * storm::ENERGY_GRAM * (long long)sizeof(double);
}

extern "C" int storm_energy_ratios_rows(const float* s_hat, const float* s, const float* n, double* out, void* scratch, long long scratch_bytes,
                                        int B, long long L, long long stride_hat, long long stride_s, long long stride_n, const int* row_len,
                                        storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(s_hat && s && n && out && scratch, "storm_energy_ratios_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && L >= 1 && L <= (1ll << 40), "storm_energy_ratios_rows: B=%d L=%lld", B, L);
    STORM_CHECK(stride_hat >= L && stride_s >= L && stride_n >= L, "storm_energy_ratios_rows: strides %lld %lld %lld for rows of %lld", stride_hat,
                stride_s, stride_n, L);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= storm_energy_ratios_scratch_bytes(B, L),
                "storm_energy_ratios_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)", scratch, scratch_bytes,
                storm_energy_ratios_scratch_bytes(B, L));
    const long long nchunks = (L + ENERGY_CHUNK - 1) / ENERGY_CHUNK;
    hipLaunchKernelGGL(energy_partials_kernel, dim3((unsigned)nchunks, B), dim3(METRICS_THREADS), 0, (hipStream_t)st, s_hat, s, n, (double*)scratch, L,
                       stride_hat, stride_s, stride_n, row_len);
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(energy_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)st, (const double*)scratch, out, L, row_len, (int)nchunks, B);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" long long storm_lsd_scratch_bytes(int B, int F, int T) {
    if (B <= 0 || F <= 0 || T <= 0) return 0;
    return (long long)B * ((F + storm::LSD_BINS - 1) / storm::LSD_BINS) * ((T + storm::LSD_FRAMES - 1) / storm::LSD_FRAMES) * (long long)sizeof(double);
}

extern "C" int storm_lsd_rows(const float* spec_hat, const float* spec, double* out, void* scratch, long long scratch_bytes, int B, int F, int T,
                              const int* row_frames, double eps, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(spec_hat && spec && out && scratch, "storm_lsd_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && F >= 1 && F <= 65535 * LSD_BINS && T >= 1, "storm_lsd_rows: B=%d F=%d T=%d", B, F, T);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= storm_lsd_scratch_bytes(B, F, T),
                "storm_lsd_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)", scratch, scratch_bytes, storm_lsd_scratch_bytes(B, F, T));
    const int nbt = (F + LSD_BINS - 1) / LSD_BINS, nft = (T + LSD_FRAMES - 1) / LSD_FRAMES;
    hipLaunchKernelGGL(lsd_partials_kernel, dim3(nft, nbt, B), dim3(METRICS_THREADS), 0, (hipStream_t)st, spec_hat, spec, (double*)scratch, F, T,
                       row_frames, eps);
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(lsd_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)st, (const double*)scratch, out, F, T, row_frames, nbt, nft, B);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_lpc_window(int fs, double* w, long long capacity) {
    int W, H, P;
    STORM_CHECK(storm::lpc_shape(fs, W, H, P), "storm_lpc_window: fs=%d (the window W = (30 fs + 500) / 1000 must satisfy 2 P < W <= %d)", fs, storm::LPC_MAX_W);
    STORM_CHECK(w != nullptr, "storm_lpc_window: null pointer");
    STORM_CHECK(capacity >= W, "storm_lpc_window: capacity %lld for a window of %d", capacity, W);
    for (int n = 0; n < W; ++n) w[n] = 0.5 * (1.0 - cos(2.0 * storm::LPC_PI * (double)(n + 1) / (double)(W + 1)));
    return W;
}

extern "C" long long storm_lpc_measures_scratch_bytes(int B, long long L, int fs) {
    int W, H, P;
    if (B <= 0 || B > 65535 || L <= 0 || L > (1ll << 30) || !storm::lpc_shape(fs, W, H, P)) return 0;
    return (long long)B * 2 * (long long)sizeof(int) + (long long)B * storm::lpc_frames(L, W, H) * (3 + 2 * storm::LPC_LAGS) * (long long)sizeof(double);
}

extern "C" int storm_lpc_measures_rows(const float* x, const float* y, const double* window, double* out, double* frames_out, void* scratch,
                                       long long scratch_bytes, int B, long long L, long long stride_x, long long stride_y, const int* row_len,
                                       int fs, storm_stream_t st) {
    using namespace storm;
    int W, H, P;
    STORM_CHECK(lpc_shape(fs, W, H, P), "storm_lpc_measures_rows: fs=%d (the window W = (30 fs + 500) / 1000 must satisfy 2 P < W <= %d)", fs, LPC_MAX_W);
    STORM_CHECK(x && y && window && out && scratch, "storm_lpc_measures_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && L >= 1 && L <= (1ll << 30), "storm_lpc_measures_rows: B=%d L=%lld", B, L);
    STORM_CHECK(stride_x >= L && stride_y >= L, "storm_lpc_measures_rows: strides %lld %lld for rows of %lld", stride_x, stride_y, L);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= storm_lpc_measures_scratch_bytes(B, L, fs),
                "storm_lpc_measures_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)", scratch, scratch_bytes,
                storm_lpc_measures_scratch_bytes(B, L, fs));
    const long long Mmax = lpc_frames(L, W, H);
    int* counts = (int*)scratch;
    double* fr = (double*)((char*)scratch + (long long)B * 2 * sizeof(int));            // [B][Mmax][3]
    double* lags = fr + (long long)B * Mmax * 3;                                          // [B][Mmax][2][17]
    hipStream_t hs = (hipStream_t)st;
    if (Mmax > 0) {
        const int lds = lpc_lds_bytes(W, H);
        static int lds_allowed = 64 * 1024;                            // (a window of more than ~1100 samples needs more than the default)
        if (lds > lds_allowed) {
            STORM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lpc_frames_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            lds_allowed = 160 * 1024;
        }
        hipLaunchKernelGGL(lpc_frames_kernel, dim3((unsigned)((Mmax + LPC_TILE - 1) / LPC_TILE), B), dim3(METRICS_THREADS), lds, hs, x, y, window, fr,
                           lags, L, stride_x, stride_y, row_len, Mmax, W, H);
        STORM_LAUNCH_CHECK();
        hipLaunchKernelGGL(lpc_model_kernel, dim3((unsigned)((Mmax + 63) / 64), B), dim3(64), 0, hs, (const double*)lags, fr, frames_out, L, row_len,
                           Mmax, W, H, P);
        STORM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lpc_rows_kernel, dim3(B), dim3(METRICS_THREADS), 0, hs, (const double*)fr, out, counts, L, row_len, Mmax, W, H);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
