// STFT / iSTFT front and back end with the magnitude-compression transform fused in.
// Reference map in include/storm_hip.h.  n_fft = 510 is tiny (<= 0.3 GFLOP per utterance),
// so each frame is a direct real DFT out of LDS: one workgroup per frame, one thread per
// frequency bin (forward) / per output sample (inverse), twiddles from a [n_fft] table,
// products in fp32, sums in fp64.  Semantics are torch.stft / torch.istft with center=True,
// reflect padding, periodic Hann, onesided output, window-envelope normalisation.
#include "common.h"
#define STORM_TASNET_IMPL          // the time-domain network's kernels (ConvTasNet) are compiled with the 1-D signal code
#include "tasnet.h"

namespace storm {

constexpr int MAX_NFFT = 1024;

// frames of torch.stft(center=True) over L samples: the row grows by n_fft / 2 (rounded down) on either side, and every frame needs n_fft
// samples of it.  Even n_fft: 1 + L / hop.  Odd n_fft: 1 + (L - 1) / hop, one frame fewer whenever hop divides L.
__host__ __device__ inline long long stft_frames(long long L, int n_fft, int hop) { return 1 + (L + 2 * (n_fft / 2) - n_fft) / hop; }

// |z| of a spectrogram bin for spec_fwd / spec_back.  sqrtf(re^2 + im^2) wherever the sum of squares is far from fp32's ends (the bits this
// library has always produced); outside that range the squares underflow or overflow where torch.abs does not (a bin of magnitude 1e-30
// came out as 0), so there hypotf takes over.
__device__ inline float spec_abs(float re, float im) {
    const float s = re * re + im * im;
    return (s >= 0x1p-100f && s <= 0x1p+100f) ? sqrtf(s) : hypotf(re, im);
}

__global__ void peak_abs_kernel(const float* __restrict__ wav, float* __restrict__ peak, long long L, long long stride,
                                const int* __restrict__ row_len) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    if (row_len) L = row_len[b];
    const float* p = wav + (long long)b * stride;
    float m = 0.f;
    for (long long i = threadIdx.x; i < L; i += blockDim.x) m = fmaxf(m, fabsf(p[i]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    // (an all-zero utterance: the reference divides 0 / 0 and fills the whole sampler with NaN, model.py:281-284; here its
    // row stays zero - in a batch it would otherwise poison nothing but itself, silently)
    if (threadIdx.x == 0) peak[b] = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), 1e-20f);
}

__global__ void stft_kernel(const float* __restrict__ wav, const float* __restrict__ peak, float* __restrict__ spec,
                            const float* __restrict__ window, const float* __restrict__ tw, long long L,
                            long long stride, int n_fft, int hop, int n_frames, int Tpad, float factor, float expo, const int* __restrict__ row_len) {
    __shared__ float xs[MAX_NFFT];
    __shared__ float2 tws[MAX_NFFT];
    const int frame = blockIdx.x, b = blockIdx.y, F = n_fft / 2 + 1;
    float2* out = reinterpret_cast<float2*>(spec) + (long long)b * F * Tpad;
    if (row_len) { L = row_len[b]; n_frames = (int)stft_frames(L, n_fft, hop); }      // ragged batch: this row's own length / frame count
    if (frame >= n_frames) {                       // pad_spec: zero frames
        for (int f = threadIdx.x; f < F; f += blockDim.x) out[(long long)f * Tpad + frame] = make_float2(0.f, 0.f);
        return;
    }
    const float* x = wav + (long long)b * stride;
    const int pad = n_fft / 2;
    for (int k = threadIdx.x; k < n_fft; k += blockDim.x) {
        long long idx = (long long)frame * hop + k - pad;
        if (idx < 0) idx = -idx;                   // reflect (no edge repeat)
        if (idx >= L) idx = 2 * (L - 1) - idx;
        // a ragged row of <= n_fft / 2 samples is rejected by the host wrappers (torch.stft raises for it); a device-side
        // length the host never saw must still not read outside the row
        idx = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
        const float v = peak ? x[idx] / peak[b] : x[idx];    // y / norm_factor (model.py:284)
        xs[k] = v * window[k];
        tws[k] = reinterpret_cast<const float2*>(tw)[k];
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int k = 0; k < n_fft; ++k) {
            const float2 w = tws[idx];
            re += (double)(xs[k] * w.x);
            im -= (double)(xs[k] * w.y);
            idx += f; if (idx >= n_fft) idx -= n_fft;
        }
        float zr = (float)re, zi = (float)im;
        // spec_fwd: |X|^e exp(j angle X) * factor  (data_module.py:182-186)
        if (expo != 1.0f) {
            const float mag = spec_abs(zr, zi);
            const float sc = mag > 0.f ? powf(mag, expo - 1.0f) : 0.f;
            zr *= sc; zi *= sc;
        }
        out[(long long)f * Tpad + frame] = make_float2(zr * factor, zi * factor);
    }
}

__global__ void istft_frames_kernel(const float* __restrict__ spec, float* __restrict__ frames,
                                    const float* __restrict__ window, const float* __restrict__ tw, int T, int n_fft,
                                    float factor, float expo) {
    __shared__ float2 X[MAX_NFFT / 2 + 1];
    __shared__ float2 tws[MAX_NFFT];
    const int frame = blockIdx.x, b = blockIdx.y, F = n_fft / 2 + 1;
    const float2* in = reinterpret_cast<const float2*>(spec) + (long long)b * F * T;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        float2 z = in[(long long)f * T + frame];
        z.x /= factor; z.y /= factor;                         // spec_back (data_module.py:188-193)
        if (expo != 1.0f) {
            const float mag = spec_abs(z.x, z.y);
            const float sc = mag > 0.f ? powf(mag, 1.0f / expo - 1.0f) : 0.f;
            z.x *= sc; z.y *= sc;
        }
        X[f] = z;
    }
    for (int k = threadIdx.x; k < n_fft; k += blockDim.x) tws[k] = reinterpret_cast<const float2*>(tw)[k];
    __syncthreads();
    const bool even = (n_fft % 2) == 0;
    for (int k = threadIdx.x; k < n_fft; k += blockDim.x) {
        double acc = (double)X[0].x;
        int idx = 0;
        for (int f = 1; f < F; ++f) {
            idx += k; if (idx >= n_fft) idx -= n_fft;
            const float2 w = tws[idx];
            const double term = (double)(X[f].x * w.x) - (double)(X[f].y * w.y);   // Re(X e^{+j 2 pi f k / N})
            acc += (even && f == F - 1) ? term : 2.0 * term;
        }
        frames[((long long)b * T + frame) * n_fft + k] = (float)(acc / n_fft) * window[k];
    }
}

__global__ void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                 const float* __restrict__ peak, float* __restrict__ wav, int T, long long L,
                                 long long stride, int n_fft, int hop, const int* __restrict__ row_len) {
    const int b = blockIdx.y;
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= L) return;
    if (row_len && n >= row_len[b]) { wav[(long long)b * stride + n] = 0.f; return; }   // ragged batch: istft(..., length = this row's)
    const long long m = n + n_fft / 2;
    long long t1 = m / hop; if (t1 > T - 1) t1 = T - 1;
    long long t0 = (m - n_fft + hop) / hop; if (m - n_fft + 1 <= 0) t0 = 0; if (t0 < 0) t0 = 0;
    float y = 0.f, env = 0.f;
    for (long long t = t0; t <= t1; ++t) {
        const long long k = m - t * hop;
        if (k < 0 || k >= n_fft) continue;
        y += frames[((long long)b * T + t) * n_fft + k];
        env += window[k] * window[k];
    }
    float v = env > 1e-11f ? y / env : 0.f;
    if (peak) v *= peak[b];
    wav[(long long)b * stride + n] = v;
}

// standalone spec_fwd / spec_back on a complex tensor (data_module.py:182-193)
__global__ void spec_transform_kernel(const float* __restrict__ in, float* __restrict__ out, long long n,
                                      float factor, float expo, int inverse) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float2 z = reinterpret_cast<const float2*>(in)[i];
        if (inverse) { z.x /= factor; z.y /= factor; }
        if (expo != 1.0f) {
            const float mag = spec_abs(z.x, z.y);
            const float sc = mag > 0.f ? powf(mag, (inverse ? 1.0f / expo : expo) - 1.0f) : 0.f;
            z.x *= sc; z.y *= sc;
        }
        if (!inverse) { z.x *= factor; z.y *= factor; }
        reinterpret_cast<float2*>(out)[i] = z;
    }
}

// ---- rational resampling (storm_resample_poly; definition in include/storm_hip.h) ---------------------------------------------
// y[n] = sum_m T[p][m] x[q - m],  c = n down + half, p = c mod up, q = c div up,  T = the phase-major table of storm_resample_taps.
// One workgroup owns RESAMPLE_TILE consecutive outputs of one row (thread t: outputs t, t + 256, ...: coalesced stores, and for
// the common odd `down` a conflict-free LDS stride).  The input samples its outputs touch are staged through LDS in windows of
// RESAMPLE_WINDOW samples, walked from the highest index down: that is ascending m for every output, so an output is ONE fp32 FMA
// chain over m = 0 .. M_p - 1 whatever the window, tile, batch or grid - its bits depend on its own row's samples only.  (A tile of
// 48 -> 16 kHz or 44.1 -> 16 kHz needs one window; ratios of 8 : 1 and steeper walk several.)  Samples outside [0, len_b) are zero
// and are never loaded; products with them are skipped (they add +0).  The taps stay in global memory: an output's M_p taps are
// contiguous, the table is <= 82 KB and lives in the L2.
constexpr int RESAMPLE_TILE = STORM_RESAMPLE_TILE, RESAMPLE_THREADS = 256, RESAMPLE_PER_THREAD = RESAMPLE_TILE / RESAMPLE_THREADS;
constexpr int RESAMPLE_WINDOW = 8192;            // samples per staged window (32 KB of LDS, a multiple of 4)

__global__ void __launch_bounds__(RESAMPLE_THREADS)
resample_poly_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ taps, long long L_in, long long stride_in,
                     long long L_out, long long stride_out, const int* __restrict__ row_len, int up, int down, int half, int M) {
    __shared__ __attribute__((aligned(16))) float xs[RESAMPLE_WINDOW];
    const int b = blockIdx.y, t = threadIdx.x;
    long long len = row_len ? (long long)row_len[b] : L_in;
    if (len > L_in) len = L_in;                                                      // (a device-side length the host never saw must still not read outside the row)
    const long long n_valid = len <= 0 ? 0 : (len * up + down - 1) / down;           // this row's outputs; the rest of its row is zero
    const long long n0 = (long long)blockIdx.x * RESAMPLE_TILE;
    const float* xr = x + (long long)b * stride_in;
    float* yr = y + (long long)b * stride_out;
    const bool vec = ((uintptr_t)xr & 15) == 0;                                      // 16-byte loads where the row starts on one

    long long q[RESAMPLE_PER_THREAD];
    int Mp[RESAMPLE_PER_THREAD];
    const float* tp[RESAMPLE_PER_THREAD];
    float acc[RESAMPLE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RESAMPLE_PER_THREAD; ++j) {
        const long long n = n0 + j * RESAMPLE_THREADS + t;
        const long long c = n * down + half;
        const int p = (int)(c % up);
        q[j] = c / up;
        Mp[j] = n < n_valid ? (2 * half - p) / up + 1 : 0;                           // taps of phase p: h[p + m up], p + m up <= 2 half
        tp[j] = taps + (long long)p * M;
        acc[j] = 0.f;
    }
    if (n0 < n_valid) {                                                              // (uniform in the workgroup: b and blockIdx only)
        const long long n_last = (n0 + RESAMPLE_TILE < n_valid ? n0 + RESAMPLE_TILE : n_valid) - 1;
        long long hi = (n_last * down + half) / up;                                  // highest sample any output of the tile reads (m = 0)
        if (hi > len - 1) hi = len - 1;
        long long lowest = (n0 * down + half) / up - (M - 1);                        // lowest one (first output, last tap)
        if (lowest < 0) lowest = 0;
        while (hi >= lowest) {
            long long lo = hi - (RESAMPLE_WINDOW - 4);                               // window [lo, hi], lo a multiple of 4: at most WINDOW samples
            if (lo < lowest) lo = lowest;
            lo &= ~3ll;
            const int n4 = (int)((hi - lo) / 4) + 1;
            for (int i = t; i < n4; i += RESAMPLE_THREADS) {
                const long long k = lo + 4ll * i;
                float4 v;
                if (vec && k + 3 < len) v = *reinterpret_cast<const float4*>(xr + k);
                else v = make_float4(k < len ? xr[k] : 0.f, k + 1 < len ? xr[k + 1] : 0.f, k + 2 < len ? xr[k + 2] : 0.f, k + 3 < len ? xr[k + 3] : 0.f);
                *reinterpret_cast<float4*>(xs + 4 * i) = v;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < RESAMPLE_PER_THREAD; ++j) {
                long long m0 = q[j] - hi, m1 = q[j] - lo;                            // the taps whose sample q - m lies in [lo, hi]
                if (m0 < 0) m0 = 0;
                if (m1 > Mp[j] - 1) m1 = Mp[j] - 1;
                if (m0 > m1) continue;
                const int at = (int)(q[j] - lo);                                     // sample q - m sits at xs[at - m]: inside the window for m in [m0, m1]
                float a = acc[j];
                for (int m = (int)m0; m <= (int)m1; ++m) a = fmaf(tp[j][m], xs[at - m], a);
                acc[j] = a;
            }
            __syncthreads();
            hi = lo - 1;
        }
    }
#pragma unroll
    for (int j = 0; j < RESAMPLE_PER_THREAD; ++j) {
        const long long n = n0 + j * RESAMPLE_THREADS + t;
        if (n < L_out) yr[n] = acc[j];
    }
}

}  // namespace storm

using namespace storm;

extern "C" int storm_spec_transform(const float* in, float* out, long long n_complex, float spec_factor,
                                    float spec_abs_exponent, int inverse, storm_stream_t s) {
    STORM_CHECK(in && out && n_complex > 0 && spec_factor != 0.f && spec_abs_exponent != 0.f, "storm_spec_transform: bad arguments");
    long long nb = (n_complex + 255) / 256; if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(spec_transform_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, in, out, n_complex,
                       spec_factor, spec_abs_exponent, inverse);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_peak_abs(const float* wav, float* peak, int B, long long L, long long stride, const int* row_len,
                              storm_stream_t s) {
    STORM_CHECK(wav && peak && B > 0 && L > 0, "storm_peak_abs: bad arguments");
    hipLaunchKernelGGL(peak_abs_kernel, dim3(B), dim3(256), 0, (hipStream_t)s, wav, peak, L, stride, row_len);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_stft(const float* wav, const float* peak, float* spec, const float* window, const float* twiddle,
                          int B, long long L, long long stride, int n_fft, int hop, int n_frames, int Tpad,
                          float spec_factor, float spec_abs_exponent, const int* row_len, storm_stream_t s) {
    STORM_CHECK(wav && spec && window && twiddle && B > 0, "storm_stft: null pointer");
    STORM_CHECK(n_fft >= 2 && n_fft <= MAX_NFFT && hop > 0, "storm_stft: n_fft=%d hop=%d", n_fft, hop);
    STORM_CHECK(L > n_fft / 2, "storm_stft: signal too short for reflect padding (L=%lld)", L);
    STORM_CHECK(n_frames == (int)stft_frames(L, n_fft, hop) && Tpad >= n_frames, "storm_stft: n_frames=%d Tpad=%d L=%lld", n_frames, Tpad, L);
    hipLaunchKernelGGL(stft_kernel, dim3(Tpad, B), dim3(256), 0, (hipStream_t)s, wav, peak, spec, window, twiddle, L, stride,
                       n_fft, hop, n_frames, Tpad, spec_factor, spec_abs_exponent, row_len);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_istft(const float* spec, const float* peak, float* wav, float* frames, const float* window,
                           const float* twiddle, int B, int T, long long L, long long stride, int n_fft, int hop,
                           float spec_factor, float spec_abs_exponent, const int* row_len, storm_stream_t s) {
    STORM_CHECK(spec && wav && frames && window && twiddle && B > 0 && T > 0, "storm_istft: null pointer");
    STORM_CHECK(n_fft >= 2 && n_fft <= MAX_NFFT && hop > 0, "storm_istft: n_fft=%d hop=%d", n_fft, hop);
    STORM_CHECK(L > 0 && L <= (long long)n_fft + (long long)hop * (T - 1) - n_fft / 2, "storm_istft: length %lld not covered by %d frames", L, T);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(istft_frames_kernel, dim3(T, B), dim3(256), 0, st, spec, frames, window, twiddle, T, n_fft, spec_factor, spec_abs_exponent);
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(istft_ola_kernel, dim3(cdiv(L, 256), B), dim3(256), 0, st, frames, window, peak, wav, T, L, stride, n_fft, hop, row_len);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

// ---- resampling: filter design on the host (the single source of the coefficients) and the launch ----
namespace {
int resample_gcd(int a, int b) { while (b) { const int r = a % b; a = b; b = r; } return a; }
// modified Bessel function I0 by its power series sum_k ((x/2)^k / k!)^2, to fp64 convergence
double bessel_i0(double x) {
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}
}  // namespace

extern "C" int storm_resample_num_taps(int up, int down) {
    STORM_CHECK(up >= 1 && down >= 1, "storm_resample: up=%d down=%d (both must be >= 1)", up, down);
    STORM_CHECK(resample_gcd(up, down) == 1, "storm_resample: ratio %d / %d is not reduced (gcd %d)", up, down, resample_gcd(up, down));
    const int R = up > down ? up : down;
    STORM_CHECK(R <= STORM_RESAMPLE_MAX_RATE, "storm_resample: max(up, down) = %d exceeds %d", R, STORM_RESAMPLE_MAX_RATE);
    return 2 * 10 * R + 1;
}

extern "C" int storm_resample_taps(int up, int down, float* taps_phase_major, long long capacity) {
    const int ntaps = storm_resample_num_taps(up, down);
    if (ntaps < 0) return ntaps;
    STORM_CHECK(taps_phase_major != nullptr, "storm_resample_taps: null pointer");
    const int R = up > down ? up : down, half = 10 * R, M = (ntaps + up - 1) / up;
    STORM_CHECK(capacity >= (long long)up * M, "storm_resample_taps: capacity %lld for a table of %d x %d", capacity, up, M);
    // firwin(2 half + 1, 1 / R, window = ('kaiser', 5.0)) * up in fp64: sinc low-pass at 1 / R of Nyquist under a Kaiser window, unit DC gain
    const double beta = 5.0, pi = 3.14159265358979323846, fc = 1.0 / (double)R, i0b = bessel_i0(beta);
    double sum = 0.0;
    const auto tap = [&](int j) {
        const double n = (double)(j - half), r = n / (double)half, arg = pi * (fc * n);     // (fc n first: exact multiples of R land on exact integers)
        const double w = bessel_i0(beta * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / i0b;
        return fc * (j == half ? 1.0 : sin(arg) / arg) * w;
    };
    for (int j = 0; j < ntaps; ++j) sum += tap(j);
    for (int p = 0; p < up; ++p)
        for (int m = 0; m < M; ++m) {
            const int j = p + m * up;
            taps_phase_major[(long long)p * M + m] = j < ntaps ? (float)(tap(j) / sum * (double)up) : 0.f;       // rounded to fp32 once; zero past M_p
        }
    return STORM_OK;
}

extern "C" int storm_resample_poly(const float* x, float* y, const float* taps, int B, long long L_in, long long stride_in, long long L_out,
                                   long long stride_out, const int* row_len, int up, int down, storm_stream_t s) {
    STORM_CHECK(x && y && taps, "storm_resample_poly: null pointer (x=%p y=%p taps=%p)", (const void*)x, (const void*)y, (const void*)taps);
    const int ntaps = storm_resample_num_taps(up, down);
    if (ntaps < 0) return ntaps;
    STORM_CHECK(B >= 1 && B <= 65535 && L_in >= 1 && L_in <= (1ll << 40), "storm_resample_poly: B=%d L_in=%lld", B, L_in);
    STORM_CHECK(L_out == (L_in * up + down - 1) / down, "storm_resample_poly: L_out=%lld, %lld samples at %d / %d give %lld", L_out, L_in, up, down,
                (L_in * up + down - 1) / down);
    STORM_CHECK(stride_in >= L_in && stride_out >= L_out, "storm_resample_poly: stride_in=%lld stride_out=%lld for rows of %lld / %lld", stride_in,
                stride_out, L_in, L_out);
    const long long tiles = (L_out + RESAMPLE_TILE - 1) / RESAMPLE_TILE;
    STORM_CHECK(tiles <= 0x7fffffffll, "storm_resample_poly: L_out=%lld", L_out);
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)tiles, B), dim3(RESAMPLE_THREADS), 0, (hipStream_t)s, x, y, taps, L_in, stride_in, L_out,
                       stride_out, row_len, up, down, (ntaps - 1) / 2, (ntaps + up - 1) / up);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

// ---- evaluation metrics of enhanced audio (storm_energy_ratios_rows, storm_lsd_rows): kernels and entry points ----
#include "metrics.h"

// ---- intelligibility (storm_stoi_rows, storm_stoi_taps, storm_resample_poly_taps): STOI / ESTOI kernels, filter design and entry points ----
#include "stoi.h"

// ---- long recordings (storm_crossfade_rows, storm_crossfade_ramp): the stitch of enhanced windows, kernel and entry points ----
#include "longform.h"

// ---- misaligned audio (storm_xcorr_lag_rows, storm_shift_rows, storm_sosfilt_rows, storm_butter_sos): delay search, shift, biquad cascade ----
#include "align.h"

// ---- BSS-eval SDR (storm_bss_sdr_rows, storm_bss_sdr_scratch_bytes): lag correlations per piece, Levinson-Durbin solve per row ----
#include "bss.h"
