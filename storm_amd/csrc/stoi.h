// Intelligibility of enhanced audio on the device: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) for batches of rows at 10 kHz,
// and the design of their resampling filter.  Definition in include/storm_hip.h (storm_stoi_rows); the reference only calls the pystoi
// package (util/inference.py:65), so that text is the specification.  Five launches for the whole batch:
//   stoi_energy_kernel    one wave per gate frame: 20 log10(|w frame| + EPS) of the clean signal
//   stoi_gate_kernel      one workgroup per row: the loudest frame, the mask, the list of kept frames (an exclusive prefix count); row 0's
//                         also writes the fp64 window and twiddles of the call, once
//   stoi_tob_kernel       one workgroup per spectrogram frame: the frame is rebuilt from the three kept frames that overlap it (the signal
//                         without its silent frames is never written), clean + j processed ride ONE 512-point complex FFT in LDS, then the
//                         15 third-octave band magnitudes
//   stoi_segment_kernel   one wave per 30-frame segment: both normalisations, one partial per measure
//   stoi_finish_kernel    one wave per row: the segment partials in index order (loaded 64 at a time, added by one lane)
// After the fp32 samples are read everything is fp64.  No atomics; every sum runs in an order fixed by indices inside the row, so a row's
// two numbers are the same bits alone, in any batch, at any batch width, row stride and position.
// Included by spectral.hip alone (kernels and entry points live in that translation unit; its bessel_i0 / resample_gcd / resample_poly_kernel
// are used here).
#pragma once
#include "common.h"

namespace storm {

constexpr int STOI_FS = 10000, STOI_FRAME = 256, STOI_HOP = 128, STOI_NFFT = 512, STOI_BANDS = 15, STOI_SEG = 30;
constexpr int STOI_THREADS = 256, STOI_WAVES = STOI_THREADS / 64;
constexpr double STOI_EPS = 2.220446049250313e-16;                      // 2^-52
constexpr double STOI_DYN_RANGE = 40.0;
constexpr double STOI_CLIP = 1.0 + 5.623413251903491;                   // 1 + 10^(-BETA / 20), BETA = -15 dB
constexpr double STOI_TOO_SHORT = 1e-5;                                 // fewer than STOI_SEG spectrogram frames
constexpr double STOI_PI = 3.14159265358979323846;
constexpr int STOI_BIN0 = 7, STOI_BIN1 = 219;                           // the bands cover bins [7, 219)
__device__ const int stoi_band_edge[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// hanning(258)[1:-1][k]
__device__ __forceinline__ double stoi_window(int k) { return 0.5 - 0.5 * cos(2.0 * STOI_PI * (double)(k + 1) / (double)(STOI_FRAME + 1)); }
// gate frames of a row of len samples: starts 0, 128, ... < len - 256
__host__ __device__ inline long long stoi_gate_frames(long long len) { return len > STOI_FRAME ? (len - STOI_FRAME + STOI_HOP - 1) / STOI_HOP : 0; }
__device__ __forceinline__ long long stoi_row_len(const int* row_len, int b, long long L) {
    long long len = row_len ? (long long)row_len[b] : L;
    return len > L ? L : len;                                          // (a device-side length the host never saw must still not read outside the row)
}

// the caller's scratch, cut for (B, L): every piece starts on 8 bytes
struct StoiScratch {
    long long nF, nM, nJ;        // the most gate frames / spectrogram frames / segments a row of L samples can have
    int* counts;                 // [B][4]: gate frames, kept frames, segments, spectrogram frames of every row
    double* energy;              // [B][nF] dB
    double* tob;                 // [2][B][15][nM]: clean, processed
    double* part;                // [B][nJ][2]: STOI, ESTOI sums of every segment
    double* table;               // [3][256]: the window hanning(258)[1:-1], then cos and sin of -2 pi t / 512 (written by the gate kernel)
    int* kept;                   // [B][nF]: the kept frames' indices, ascending
};
// the pieces' byte offsets in that order; returns the total
inline long long stoi_scratch_layout(int B, long long L, StoiScratch& s, long long (&off)[6]) {
    s.nF = stoi_gate_frames(L);
    s.nM = s.nF > 1 ? s.nF - 1 : 0;
    s.nJ = s.nM >= STOI_SEG ? s.nM - STOI_SEG + 1 : 0;
    long long o = 0;
    off[0] = o; o += (long long)B * 4 * sizeof(int);
    off[1] = o; o += (long long)B * s.nF * sizeof(double);
    off[2] = o; o += 2ll * B * STOI_BANDS * s.nM * sizeof(double);
    off[3] = o; o += (long long)B * s.nJ * 2 * sizeof(double);
    off[4] = o; o += 3ll * STOI_FRAME * sizeof(double);
    off[5] = o; o += (long long)B * s.nF * sizeof(int);
    return o;
}
inline StoiScratch stoi_scratch(void* base, int B, long long L) {
    StoiScratch s;
    long long off[6];
    stoi_scratch_layout(B, L, s, off);
    char* p = (char*)base;
    s.counts = (int*)(p + off[0]); s.energy = (double*)(p + off[1]); s.tob = (double*)(p + off[2]); s.part = (double*)(p + off[3]);
    s.table = (double*)(p + off[4]); s.kept = (int*)(p + off[5]);
    return s;
}

// energy[b][k] = 20 log10(sqrt(sum_j (w[j] x[128 k + j])^2) + EPS): one wave per frame, lane l owns samples l, l + 64, l + 128, l + 192
__global__ void __launch_bounds__(STOI_THREADS)
stoi_energy_kernel(const float* __restrict__ x, double* __restrict__ energy, long long L, long long stride, const int* __restrict__ row_len, long long nF) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * STOI_WAVES + (threadIdx.x >> 6);
    if (k >= stoi_gate_frames(stoi_row_len(row_len, b, L))) return;     // (uniform in the wave) frame k ends at 128 k + 255 < len - 1
    const float* p = x + (long long)b * stride + k * STOI_HOP;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < STOI_FRAME / 64; ++j) {
        const double v = stoi_window(lane + 64 * j) * (double)p[lane + 64 * j];
        acc = fma(v, v, acc);
    }
    acc = wave_sum_d(acc);
    if (lane == 0) energy[(long long)b * nF + k] = 20.0 * log10(sqrt(acc) + STOI_EPS);
}

// one workgroup per row: max_k e, keep frame k iff max - 40 - e_k < 0, kept[b][0 .. K) = the kept k ascending, counts[b] = (frames, K, J, M).
// Row 0's workgroup also writes the call's window and twiddle table (the band-spectrum kernel's workgroups read it, not recompute it).
__global__ void __launch_bounds__(STOI_THREADS)
stoi_gate_kernel(const double* __restrict__ energy, int* __restrict__ kept, int* __restrict__ counts, double* __restrict__ table, long long L,
                 const int* __restrict__ row_len, long long nF) {
    __shared__ double red[STOI_WAVES];
    __shared__ int scan[2][STOI_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b == 0) {
        double s, c;
        sincos(-2.0 * STOI_PI * (double)t / (double)STOI_NFFT, &s, &c);
        table[t] = stoi_window(t); table[STOI_FRAME + t] = c; table[2 * STOI_FRAME + t] = s;
    }
    const int frames = (int)stoi_gate_frames(stoi_row_len(row_len, b, L));
    const double* e = energy + (long long)b * nF;
    int* kp = kept + (long long)b * nF;
    double m = -INFINITY;
    for (int k = t; k < frames; k += STOI_THREADS) m = fmax(m, e[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    const double top = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    int base = 0;                                                      // kept frames before this pass (the same in every thread)
    for (int k0 = 0; k0 < frames; k0 += STOI_THREADS) {
        const int k = k0 + t;
        const int keep = k < frames && top - STOI_DYN_RANGE - e[k] < 0.0 ? 1 : 0;
        int cur = 0;                                                   // inclusive prefix sum of `keep` over the pass's 256 frames
        scan[0][t] = keep;
        __syncthreads();
        for (int o = 1; o < STOI_THREADS; o <<= 1) {
            scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (keep) kp[base + scan[cur][t] - 1] = k;
        base += scan[cur][STOI_THREADS - 1];
        __syncthreads();                                               // (the next pass overwrites scan[0])
    }
    if (t == 0) {
        const int M = base > 0 ? base - 1 : 0;
        counts[4 * b + 0] = frames; counts[4 * b + 1] = base; counts[4 * b + 2] = M >= STOI_SEG ? M - STOI_SEG + 1 : 0; counts[4 * b + 3] = M;
    }
}

__device__ __forceinline__ int stoi_bitrev9(int k) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) r |= ((k >> i) & 1) << (8 - i);
    return r;
}

// tob[s][b][i][m], s = 0 clean / 1 processed: spectrogram frame m of the signal without its silent frames.  Samples [128 m, 128 m + 256) of that
// signal are w*frame[kept[m-1]][128:] + w*frame[kept[m]][:128] (first half; the earlier frame first, as an overlap-add in frame order adds them)
// and w*frame[kept[m]][128:] + w*frame[kept[m+1]][:128] (second half; m + 1 <= K - 1 because M = K - 1); times w again, zero padded to 512.
// z = clean + j processed through one radix-2 decimation-in-frequency FFT (thread t: one butterfly per stage, output in bit-reversed order),
// X_k = (Z_k + conj Z_{512-k}) / 2, Y_k = (Z_k - conj Z_{512-k}) / 2j, band sums of |.|^2 in bin order, roots.
__global__ void __launch_bounds__(STOI_THREADS)
stoi_tob_kernel(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ kept, const int* __restrict__ counts,
                const double* __restrict__ table, double* __restrict__ tob, long long stride_x, long long stride_y, long long nF, long long nM, int B) {
    __shared__ double zr[STOI_NFFT], zi[STOI_NFFT], twr[STOI_NFFT / 2], twi[STOI_NFFT / 2], w[STOI_FRAME];
    __shared__ double px[STOI_BIN1], py[STOI_BIN1];
    const int b = blockIdx.y, t = threadIdx.x;
    const long long m = blockIdx.x;
    if (m >= counts[4 * b + 3]) return;                                // (uniform in the workgroup)
    const int* kp = kept + (long long)b * nF;
    const float* xr = x + (long long)b * stride_x;
    const float* yr = y + (long long)b * stride_y;
    w[t] = table[t]; twr[t] = table[STOI_FRAME + t]; twi[t] = table[2 * STOI_FRAME + t];
    __syncthreads();
    {
        // the two kept frames that cover sample t of the frame: `early` holds it in its second half (t < 128) or its first half (t >= 128)
        const bool first = t < STOI_HOP;
        const long long f_early = first ? (m >= 1 ? (long long)kp[m - 1] : -1) : (long long)kp[m];
        const long long f_late = first ? (long long)kp[m] : (long long)kp[m + 1];
        const int j_early = first ? t + STOI_HOP : t, j_late = first ? t : t - STOI_HOP;
        double sx = 0.0, sy = 0.0;
        if (f_early >= 0) {
            sx = w[j_early] * (double)xr[f_early * STOI_HOP + j_early];
            sy = w[j_early] * (double)yr[f_early * STOI_HOP + j_early];
        }
        sx += w[j_late] * (double)xr[f_late * STOI_HOP + j_late];
        sy += w[j_late] * (double)yr[f_late * STOI_HOP + j_late];
        zr[t] = w[t] * sx; zi[t] = w[t] * sy;
        zr[t + STOI_FRAME] = 0.0; zi[t + STOI_FRAME] = 0.0;
    }
    __syncthreads();
    for (int half = STOI_NFFT / 2; half >= 1; half >>= 1) {
        const int j = t & (half - 1), i0 = ((t - j) << 1) + j, i1 = i0 + half;
        const double ar = zr[i0], ai = zi[i0], br = zr[i1], bi = zi[i1];
        const double dr = ar - br, di = ai - bi;
        const int q = j * (STOI_NFFT / 2 / half);                      // W_512^(j 256 / half)
        zr[i0] = ar + br; zi[i0] = ai + bi;
        zr[i1] = dr * twr[q] - di * twi[q]; zi[i1] = dr * twi[q] + di * twr[q];
        __syncthreads();
    }
    if (t >= STOI_BIN0 && t < STOI_BIN1) {
        const int k = stoi_bitrev9(t), kn = stoi_bitrev9(STOI_NFFT - t);
        const double xre = 0.5 * (zr[k] + zr[kn]), xim = 0.5 * (zi[k] - zi[kn]);
        const double yre = 0.5 * (zi[k] + zi[kn]), yim = 0.5 * (zr[kn] - zr[k]);
        px[t] = xre * xre + xim * xim;
        py[t] = yre * yre + yim * yim;
    }
    __syncthreads();
    if (t < 2 * STOI_BANDS) {
        const int s = t / STOI_BANDS, i = t - s * STOI_BANDS;
        const double* p = s ? py : px;
        double acc = 0.0;
        for (int k = stoi_band_edge[i]; k < stoi_band_edge[i + 1]; ++k) acc += p[k];
        tob[(((long long)s * B + b) * STOI_BANDS + i) * nM + m] = sqrt(acc);
    }
}

// part[b][j] = (STOI, ESTOI) sums of segment j (spectrogram frames j .. j + 29): one wave per segment, lane i < 15 owns band i, lane f < 30
// owns frame f, every sum sequential in index order.
//   STOI, per band:  c = |x| / (|y| + EPS), y' = min(c y, x (1 + 10^(15/20))), both minus their means over the frames, each over its norm + EPS,
//                    sum_f x y'
//   ESTOI: every band minus its mean over the frames, over its norm + EPS; then every frame minus its mean over the bands, over its norm + EPS;
//          sum_{i, f} x y
__global__ void __launch_bounds__(STOI_THREADS)
stoi_segment_kernel(const double* __restrict__ tob, const int* __restrict__ counts, double* __restrict__ part, long long nM, long long nJ, int B) {
    __shared__ double xs[STOI_WAVES][STOI_BANDS][STOI_SEG], ys[STOI_WAVES][STOI_BANDS][STOI_SEG];
    __shared__ double band[STOI_WAVES][STOI_BANDS], col[STOI_WAVES][STOI_SEG];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long j = (long long)blockIdx.x * STOI_WAVES + wv;
    const bool live = j < counts[4 * b + 2];                           // (uniform in the wave; every wave walks the barriers below)
    if (live)
        for (int e = lane; e < STOI_BANDS * STOI_SEG; e += 64) {
            const int i = e / STOI_SEG, f = e - i * STOI_SEG;
            xs[wv][i][f] = tob[((long long)b * STOI_BANDS + i) * nM + j + f];
            ys[wv][i][f] = tob[(((long long)B + b) * STOI_BANDS + i) * nM + j + f];
        }
    __syncthreads();
    if (live && lane < STOI_BANDS) {
        double* xb = xs[wv][lane];
        double* yb = ys[wv][lane];
        double nx = 0.0, ny = 0.0;
        for (int f = 0; f < STOI_SEG; ++f) { nx = fma(xb[f], xb[f], nx); ny = fma(yb[f], yb[f], ny); }
        const double c = sqrt(nx) / (sqrt(ny) + STOI_EPS);
        double mx = 0.0, mp = 0.0, my = 0.0;
        for (int f = 0; f < STOI_SEG; ++f) { mx += xb[f]; mp += fmin(c * yb[f], xb[f] * STOI_CLIP); my += yb[f]; }
        mx /= STOI_SEG; mp /= STOI_SEG; my /= STOI_SEG;
        double vx = 0.0, vp = 0.0, vy = 0.0, xp = 0.0;
        for (int f = 0; f < STOI_SEG; ++f) {
            const double dx = xb[f] - mx, dp = fmin(c * yb[f], xb[f] * STOI_CLIP) - mp, dy = yb[f] - my;
            vx = fma(dx, dx, vx); vp = fma(dp, dp, vp); vy = fma(dy, dy, vy);
        }
        const double sx = sqrt(vx) + STOI_EPS, sp = sqrt(vp) + STOI_EPS, sy = sqrt(vy) + STOI_EPS;
        for (int f = 0; f < STOI_SEG; ++f) {
            const double dx = (xb[f] - mx) / sx, dp = (fmin(c * yb[f], xb[f] * STOI_CLIP) - mp) / sp;
            xp = fma(dx, dp, xp);
            xb[f] = dx; yb[f] = (yb[f] - my) / sy;                      // ESTOI's first normalisation, in place
        }
        band[wv][lane] = xp;
    }
    __syncthreads();
    if (live && lane < STOI_SEG) {
        double mx = 0.0, my = 0.0;
        for (int i = 0; i < STOI_BANDS; ++i) { mx += xs[wv][i][lane]; my += ys[wv][i][lane]; }
        mx /= STOI_BANDS; my /= STOI_BANDS;
        double vx = 0.0, vy = 0.0;
        for (int i = 0; i < STOI_BANDS; ++i) {
            const double dx = xs[wv][i][lane] - mx, dy = ys[wv][i][lane] - my;
            vx = fma(dx, dx, vx); vy = fma(dy, dy, vy);
        }
        const double sx = sqrt(vx) + STOI_EPS, sy = sqrt(vy) + STOI_EPS;
        double xy = 0.0;
        for (int i = 0; i < STOI_BANDS; ++i) xy = fma((xs[wv][i][lane] - mx) / sx, (ys[wv][i][lane] - my) / sy, xy);
        col[wv][lane] = xy;
    }
    __syncthreads();
    if (live && lane == 0) {
        double d = 0.0, e = 0.0;
        for (int i = 0; i < STOI_BANDS; ++i) d += band[wv][i];
        for (int f = 0; f < STOI_SEG; ++f) e += col[wv][f];
        part[((long long)b * nJ + j) * 2 + 0] = d;
        part[((long long)b * nJ + j) * 2 + 1] = e;
    }
}

// one wave per row: the segments in order; STOI = sum / (15 J), ESTOI = sum / (30 J); 1e-5 for a row without a segment.  The wave brings 64
// segments' partials into LDS with one load per lane, lane 0 adds them one after the other (a lane that walked the row alone paid one
// global-memory latency per segment: 69 us for the 750 segments of a 10-s file); slots past J hold +0, which changes no bit of a sum.
__global__ void __launch_bounds__(64)
stoi_finish_kernel(const double* __restrict__ part, const int* __restrict__ counts, double* __restrict__ out, long long nJ) {
    __shared__ double pd[64], pe[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int J = counts[4 * b + 2];                                   // (uniform in the workgroup)
    if (J < 1) {
        if (lane == 0) { out[2 * b] = STOI_TOO_SHORT; out[2 * b + 1] = STOI_TOO_SHORT; }
        return;
    }
    const double* p = part + (long long)b * nJ * 2;
    double d = 0.0, e = 0.0;
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        pd[lane] = j < J ? p[2 * j] : 0.0;
        pe[lane] = j < J ? p[2 * j + 1] : 0.0;
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 64; ++i) { d += pd[i]; e += pe[i]; }
        }
        __syncthreads();                                               // (the next pass overwrites pd, pe)
    }
    if (lane == 0) {
        out[2 * b] = d / ((double)STOI_BANDS * (double)J);
        out[2 * b + 1] = e / ((double)STOI_SEG * (double)J);
    }
}

// the filter of the definition's step 1 for fs_sig -> 10 kHz: (up, down) reduced, the half length L; false = refused
inline bool stoi_filter_shape(int fs_sig, int& up, int& down, int& half) {
    if (fs_sig < 1) return false;
    const int g = resample_gcd(STOI_FS, fs_sig);
    up = STOI_FS / g; down = fs_sig / g;
    const int R = up > down ? up : down;
    if (R > STORM_RESAMPLE_MAX_RATE) return false;
    const double fc = 1.0 / (2.0 * (double)R);
    half = (int)ceil((60.0 - 8.0) / (28.714 * (fc / 10.0)));
    return true;
}

}  // namespace storm

extern "C" int storm_stoi_num_taps(int fs_sig) {
    int up, down, half;
    STORM_CHECK(storm::stoi_filter_shape(fs_sig, up, down, half), "storm_stoi_num_taps: fs_sig=%d (>= 1, and 10000 / fs_sig reduced within %d)", fs_sig,
                STORM_RESAMPLE_MAX_RATE);
    return 2 * half + 1;
}

extern "C" int storm_stoi_taps(int fs_sig, float* taps_phase_major, long long capacity) {
    int up, down, half;
    STORM_CHECK(storm::stoi_filter_shape(fs_sig, up, down, half), "storm_stoi_taps: fs_sig=%d (>= 1, and 10000 / fs_sig reduced within %d)", fs_sig,
                STORM_RESAMPLE_MAX_RATE);
    STORM_CHECK(taps_phase_major != nullptr, "storm_stoi_taps: null pointer");
    const int ntaps = 2 * half + 1, M = (ntaps + up - 1) / up, R = up > down ? up : down;
    STORM_CHECK(capacity >= (long long)up * M, "storm_stoi_taps: capacity %lld for a table of %d x %d", capacity, up, M);
    // kaiser(2 half + 1, 0.1102 (60 - 8.7)) * 2 up fc sinc(2 fc (j - half)) in fp64, sum 1, times up (as resample_poly applies a given window)
    const double beta = 0.1102 * (60.0 - 8.7), fc = 1.0 / (2.0 * (double)R), i0b = bessel_i0(beta);
    const auto tap = [&](int j) {
        const double n = (double)(j - half), r = n / (double)half, arg = storm::STOI_PI * (2.0 * fc * n);
        const double w = bessel_i0(beta * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / i0b;
        return w * (2.0 * (double)up * fc * (j == half ? 1.0 : sin(arg) / arg));
    };
    double sum = 0.0;
    for (int j = 0; j < ntaps; ++j) sum += tap(j);
    for (int p = 0; p < up; ++p)
        for (int m = 0; m < M; ++m) {
            const int j = p + m * up;
            taps_phase_major[(long long)p * M + m] = j < ntaps ? (float)(tap(j) / sum * (double)up) : 0.f;      // rounded to fp32 once; zero past M_p
        }
    return STORM_OK;
}

extern "C" int storm_resample_poly_taps(const float* x, float* y, const float* taps, int B, long long L_in, long long stride_in, long long L_out,
                                        long long stride_out, const int* row_len, int up, int down, int num_taps, storm_stream_t s) {
    using namespace storm;
    STORM_CHECK(x && y && taps, "storm_resample_poly_taps: null pointer (x=%p y=%p taps=%p)", (const void*)x, (const void*)y, (const void*)taps);
    STORM_CHECK(up >= 1 && down >= 1 && resample_gcd(up, down) == 1 && up <= STORM_RESAMPLE_MAX_RATE && down <= STORM_RESAMPLE_MAX_RATE,
                "storm_resample_poly_taps: up=%d down=%d (reduced, each in [1, %d])", up, down, STORM_RESAMPLE_MAX_RATE);
    STORM_CHECK(num_taps >= 1 && (num_taps & 1) && num_taps <= (1 << 24), "storm_resample_poly_taps: num_taps=%d (odd, >= 1)", num_taps);
    STORM_CHECK(B >= 1 && B <= 65535 && L_in >= 1 && L_in <= (1ll << 40), "storm_resample_poly_taps: B=%d L_in=%lld", B, L_in);
    STORM_CHECK(L_out == (L_in * up + down - 1) / down, "storm_resample_poly_taps: L_out=%lld, %lld samples at %d / %d give %lld", L_out, L_in, up,
                down, (L_in * up + down - 1) / down);
    STORM_CHECK(stride_in >= L_in && stride_out >= L_out, "storm_resample_poly_taps: stride_in=%lld stride_out=%lld for rows of %lld / %lld", stride_in,
                stride_out, L_in, L_out);
    const long long tiles = (L_out + RESAMPLE_TILE - 1) / RESAMPLE_TILE;
    STORM_CHECK(tiles <= 0x7fffffffll, "storm_resample_poly_taps: L_out=%lld", L_out);
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)tiles, B), dim3(RESAMPLE_THREADS), 0, (hipStream_t)s, x, y, taps, L_in, stride_in, L_out,
                       stride_out, row_len, up, down, (num_taps - 1) / 2, (num_taps + up - 1) / up);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" long long storm_stoi_scratch_bytes(int B, long long L) {
    if (B <= 0 || L <= 0) return 0;
    storm::StoiScratch s;
    long long off[6];
    return storm::stoi_scratch_layout(B, L, s, off);
}

extern "C" int storm_stoi_rows(const float* x, const float* y, double* out, void* scratch, long long scratch_bytes, int B, long long L,
                               long long stride_x, long long stride_y, const int* row_len, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(x && y && out && scratch, "storm_stoi_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && L >= 1 && L <= (1ll << 30), "storm_stoi_rows: B=%d L=%lld", B, L);
    STORM_CHECK(stride_x >= L && stride_y >= L, "storm_stoi_rows: strides %lld %lld for rows of %lld", stride_x, stride_y, L);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= storm_stoi_scratch_bytes(B, L),
                "storm_stoi_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)", scratch, scratch_bytes, storm_stoi_scratch_bytes(B, L));
    const StoiScratch s = stoi_scratch(scratch, B, L);
    hipStream_t hs = (hipStream_t)st;
    if (s.nF > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((s.nF + STOI_WAVES - 1) / STOI_WAVES), B), dim3(STOI_THREADS), 0, hs, x, s.energy, L,
                           stride_x, row_len, s.nF);
        STORM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(stoi_gate_kernel, dim3(B), dim3(STOI_THREADS), 0, hs, (const double*)s.energy, s.kept, s.counts, s.table, L, row_len, s.nF);
    STORM_LAUNCH_CHECK();
    if (s.nJ > 0) {                                                    // (no row of this width can have a segment otherwise)
        hipLaunchKernelGGL(stoi_tob_kernel, dim3((unsigned)s.nM, B), dim3(STOI_THREADS), 0, hs, x, y, (const int*)s.kept, (const int*)s.counts, (const double*)s.table, s.tob,
                           stride_x, stride_y, s.nF, s.nM, B);
        STORM_LAUNCH_CHECK();
        hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)((s.nJ + STOI_WAVES - 1) / STOI_WAVES), B), dim3(STOI_THREADS), 0, hs,
                           (const double*)s.tob, (const int*)s.counts, s.part, s.nM, s.nJ, B);
        STORM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(stoi_finish_kernel, dim3(B), dim3(64), 0, hs, (const double*)s.part, (const int*)s.counts, out, s.nJ);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
