// Evaluation metrics of enhanced audio on the device (the reference's util/other.py: si_sdr_components / energy_ratios :21-44, snr_dB :96-100,
// lsd :16-19) - streaming reductions, one pass over the inputs.  Definitions in include/storm_hip.h.
// Both metrics share one structure: a row is cut at FIXED positions (STORM_METRICS_CHUNK samples; LSD_FRAMES x LSD_BINS spectrogram tiles),
// one workgroup sums one piece in fp64 in an order that depends on the position inside the piece only, writes its partial to caller-owned
// scratch, and a second kernel adds a row's partials in index order and forms the numbers.  No atomics; the cut depends on the sample /
// (bin, frame) index only, so a row's results are the same bits at any batch size, batch width, row stride and position in the batch.
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
