// Alignment and rumble removal of waveform rows on the device (the reference's util/other.py: align :153-157, hp_filter :76-80):
//   storm_xcorr_lag_rows   the lag of the largest full cross-correlation value of every row (two launches),
//   storm_shift_rows       a gather by a per-row shift read from device memory (np.roll, or its zero-filled form),
//   storm_sosfilt_rows     a cascade of biquads per row (scipy.signal.sosfilt with zero initial state),
//   storm_butter_sos       the Butterworth sections of scipy.signal.butter(..., output='sos') for even orders, on the host.
// Definitions in include/storm_hip.h.  No atomics anywhere; whatever is summed is summed in an order that the indices inside the row fix, so a
// row's results are the same bits alone, in any batch, at any batch width, row stride and position.
// Included by spectral.hip alone (kernels and entry points live in that translation unit).
#pragma once
#include <math.h>
#include "common.h"

namespace storm {

// ---- delay search -------------------------------------------------------------------------------------------------------------------------
// A workgroup owns XCORR_TILE consecutive lags and walks the whole n range of the tile: a lag's value is ONE fp64 fma chain in ascending n
// (fp32 x fp32 is exact in fp64, so every fma adds an exact product).  Terms outside a lag's own n range are staged as zeros: the chain
// starts at +0 and never becomes -0, so adding the +-0 product of such a term leaves it as it is (finite samples).  A thread keeps R
// consecutive lags and a window of 2 R ref values in registers: a block of R steps of n reads R new ref values and R values of y (the same
// address in every lane: an LDS broadcast) for R^2 fmas.  Both are staged as fp64 (converted once per tile and chunk, not once per use), so
// the inner loop is 16-byte LDS reads and fmas only.  One CU walks a tile: its time is at least TILE x (n range) fmas at one CU's fp64 rate
// whatever R is, so the tile is kept small (STORM_XCORR_TILE = 512 lags) and the tiles of a launch spread over the device; a launch has
// (lags / R) threads, and R = 8 (64 fmas against eight 16-byte reads, one wave per tile) runs nearest the fp64 rate once every SIMD has a
// wave, while a smaller R gives a launch of few lags (one row, a bounded search) more waves and each thread a shorter walk.  The launcher
// picks the largest R in {8, 4, 2} that still gives every SIMD a wave, else 2 (a tile is 512 / R threads); no bit depends on R - a lag's
// chain is the same chain.
constexpr int XCORR_TILE = STORM_XCORR_TILE, XCORR_CHUNK = 1024, XCORR_MAX_THREADS = XCORR_TILE / 2;
static_assert(XCORR_TILE == 512 && XCORR_CHUNK % 8 == 0, "STORM_XCORR_TILE: 512 / R threads for R = 2, 4, 8 lags per thread");
constexpr long long XCORR_NO_LAG = 0x7fffffffffffffffll;               // the lag of an entry that holds no value (a lane past the row's last lag)

struct XcorrPartial { double peak; long long lag; };
static_assert(sizeof(XcorrPartial) == STORM_XCORR_PARTIAL_BYTES, "STORM_XCORR_PARTIAL_BYTES");

// the row's lag range [dmin, dmax] (ny, nr >= 1)
__host__ __device__ inline void xcorr_range(long long ny, long long nr, long long max_lag, long long& dmin, long long& dmax) {
    dmin = -(ny - 1); dmax = nr - 1;
    if (max_lag >= 0) {
        if (dmin < -max_lag) dmin = -max_lag;
        if (dmax > max_lag) dmax = max_lag;
    }
}

// workgroup k of a row -> its tile, heaviest first: the tile of the lag with the longest overlap (tc), then its neighbours outwards in turn
__host__ __device__ inline long long xcorr_tile_of(long long k, long long T, long long tc) {
    const long long below = tc, above = T - 1 - tc, m = below < above ? below : above;
    if (k <= 2 * m) { const long long h = (k + 1) / 2; return (k & 1) ? tc + h : tc - h; }
    const long long rest = k - 2 * m;
    return below > above ? tc - m - rest : tc + m + rest;
}

// a over b: b replaces a if a holds nothing, if b is larger, or if b is equal at a smaller lag
__device__ __forceinline__ bool xcorr_better(double bc, long long bd, double ac, long long ad) {
    if (bd == XCORR_NO_LAG) return false;
    return ad == XCORR_NO_LAG || bc > ac || (bc == ac && bd < ad);
}

__device__ __forceinline__ long long row_length(const int* __restrict__ row_len, int b, long long width) {
    long long len = row_len ? (long long)row_len[b] : width;
    return len > width ? width : len;                                  // (a device-side length the host never saw must still not read outside the row)
}

struct alignas(16) XcorrPair { double x, y; };                         // one 16-byte LDS read
// R consecutive doubles of LDS (aligned to 16 bytes)
template <int R> __device__ __forceinline__ void xcorr_load(const double* p, double* dst) {
#pragma unroll
    for (int j = 0; j < R; j += 2) {
        const XcorrPair v = *reinterpret_cast<const XcorrPair*>(p + j);
        dst[j] = v.x; dst[j + 1] = v.y;
    }
}

template <int XCORR_R>
__global__ void __launch_bounds__(XCORR_TILE / XCORR_R)
xcorr_tiles_kernel(const float* __restrict__ y, const float* __restrict__ ref, XcorrPartial* __restrict__ part, long long Ny, long long Nr,
                   long long stride_y, long long stride_r, const int* __restrict__ y_len, const int* __restrict__ r_len, long long max_lag,
                   int tiles_max) {
    __shared__ __attribute__((aligned(16))) double ys[XCORR_CHUNK];
    __shared__ __attribute__((aligned(16))) double rs[XCORR_CHUNK + XCORR_TILE + XCORR_R];
    constexpr int XCORR_THREADS = XCORR_TILE / XCORR_R;
    __shared__ double best_c[XCORR_MAX_THREADS];
    __shared__ long long best_d[XCORR_MAX_THREADS];
    const int b = blockIdx.y, t = threadIdx.x;
    const long long ny = row_length(y_len, b, Ny), nr = row_length(r_len, b, Nr);
    if (ny < 1 || nr < 1) return;                                      // (uniform) the finish kernel writes such a row's (0, 0)
    long long dmin, dmax;
    xcorr_range(ny, nr, max_lag, dmin, dmax);
    const long long T = (dmax - dmin) / XCORR_TILE + 1;
    if ((long long)blockIdx.x >= T || T > tiles_max) return;           // (uniform)
    long long dc = (nr - ny) / 2;                                      // the lag of the longest overlap
    dc = dc < dmin ? dmin : (dc > dmax ? dmax : dc);
    const long long tile = xcorr_tile_of(blockIdx.x, T, (dc - dmin) / XCORR_TILE);
    const long long D0 = dmin + tile * XCORR_TILE, Dend = D0 + XCORR_TILE - 1 < dmax ? D0 + XCORR_TILE - 1 : dmax;
    const long long nlo = -Dend > 0 ? -Dend : 0, nhi = ny < nr - D0 ? ny : nr - D0;      // the n range of the tile's lags together
    const float* py = y + (long long)b * stride_y;
    const float* pr = ref + (long long)b * stride_r;
    const int base = t * XCORR_R;
    double acc[XCORR_R];
#pragma unroll
    for (int j = 0; j < XCORR_R; ++j) acc[j] = 0.0;

    for (long long c0 = nlo; c0 < nhi; c0 += XCORR_CHUNK) {
        const int m = (int)(nhi - c0 < XCORR_CHUNK ? nhi - c0 : XCORR_CHUNK), mr = (m + XCORR_R - 1) / XCORR_R * XCORR_R;
        for (int i = t; i < mr; i += XCORR_THREADS) ys[i] = c0 + i < nhi ? (double)py[c0 + i] : 0.0;
        for (int k = t; k < mr + XCORR_TILE + XCORR_R; k += XCORR_THREADS) {
            const long long idx = c0 + D0 + k;
            rs[k] = idx >= 0 && idx < nr ? (double)pr[idx] : 0.0;
        }
        __syncthreads();
        double w[2 * XCORR_R];
        xcorr_load<XCORR_R>(rs + base, w);
        for (int i = 0; i < mr; i += XCORR_R) {
            double yv[XCORR_R];
            xcorr_load<XCORR_R>(rs + i + base + XCORR_R, w + XCORR_R);
            xcorr_load<XCORR_R>(ys + i, yv);                           // (every lane reads the same address)
#pragma unroll
            for (int u = 0; u < XCORR_R; ++u)                          // ascending n; lag base + j reads ref[n + d] = w[u + j]
#pragma unroll
                for (int j = 0; j < XCORR_R; ++j) acc[j] = fma(yv[u], w[u + j], acc[j]);
#pragma unroll
            for (int j = 0; j < XCORR_R; ++j) w[j] = w[XCORR_R + j];
        }
        __syncthreads();
    }

    // the tile's (max, smallest lag): a thread's lags in ascending order, then a tree over the threads
    double bc = 0.0;
    long long bd = XCORR_NO_LAG;
#pragma unroll
    for (int j = 0; j < XCORR_R; ++j) {
        const long long d = D0 + base + j;
        if (d <= Dend && (bd == XCORR_NO_LAG || acc[j] > bc)) { bc = acc[j]; bd = d; }
    }
    best_c[t] = bc; best_d[t] = bd;
    __syncthreads();
    for (int h = XCORR_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h && xcorr_better(best_c[t + h], best_d[t + h], best_c[t], best_d[t])) { best_c[t] = best_c[t + h]; best_d[t] = best_d[t + h]; }
        __syncthreads();
    }
    if (t == 0) {
        XcorrPartial p; p.peak = best_c[0]; p.lag = best_d[0];
        part[(long long)b * tiles_max + tile] = p;
    }
}

// one thread per row: the row's tiles in tile order (ascending lags), replaced on strictly greater only - the smallest lag of the maximum
__global__ void xcorr_finish_kernel(const XcorrPartial* __restrict__ part, int* __restrict__ lag, double* __restrict__ peak, long long Ny,
                                    long long Nr, const int* __restrict__ y_len, const int* __restrict__ r_len, long long max_lag, int tiles_max,
                                    int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long long ny = row_length(y_len, b, Ny), nr = row_length(r_len, b, Nr);
    double bc = 0.0;
    long long bd = 0;
    if (ny >= 1 && nr >= 1) {
        long long dmin, dmax;
        xcorr_range(ny, nr, max_lag, dmin, dmax);
        const long long T = (dmax - dmin) / XCORR_TILE + 1;
        for (long long k = 0; k < T && k < tiles_max; ++k) {
            const XcorrPartial p = part[(long long)b * tiles_max + k];
            if (k == 0 || p.peak > bc) { bc = p.peak; bd = p.lag; }
        }
    }
    lag[b] = (int)bd; peak[b] = bc;
}

// ---- shift --------------------------------------------------------------------------------------------------------------------------------
// One workgroup owns SHIFT_TILE consecutive outputs of one row, a thread four consecutive ones.  Four outputs whose sources are four
// consecutive samples of the row move as one 16-byte load where the source address allows it and one 16-byte store where the destination does;
// the scalar path moves the same values.
constexpr int SHIFT_THREADS = 256, SHIFT_PER_THREAD = 4, SHIFT_TILE = SHIFT_THREADS * SHIFT_PER_THREAD;

__global__ void __launch_bounds__(SHIFT_THREADS)
shift_rows_kernel(const float* __restrict__ x, long long stride_x, float* __restrict__ out, long long stride_o, long long N,
                  const int* __restrict__ shift, const int* __restrict__ row_len, int wrap) {
    const int b = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * SHIFT_TILE + (long long)SHIFT_PER_THREAD * threadIdx.x;
    if (m0 >= N) return;
    long long len = row_length(row_len, b, N);
    if (len < 0) len = 0;
    const long long s = shift[b];
    const long long back = wrap ? (len > 0 ? ((s % len) + len) % len : 0) : s;        // out[m] = x[m - back] (wrap: modulo len)
    const float* px = x + (long long)b * stride_x;
    float* o = out + (long long)b * stride_o + m0;
    if (m0 + 3 < len) {
        long long src = m0 - back;
        if (wrap && src < 0) src += len;
        if (src >= 0 && src + 3 < len) {                               // four consecutive samples of the row
            float4 v;
            if (((uintptr_t)(px + src) & 15) == 0) v = *reinterpret_cast<const float4*>(px + src);
            else v = make_float4(px[src], px[src + 1], px[src + 2], px[src + 3]);
            if (((uintptr_t)o & 15) == 0) *reinterpret_cast<float4*>(o) = v;
            else { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < SHIFT_PER_THREAD; ++e) {
        const long long m = m0 + e;
        if (m >= N) break;
        float v = 0.f;                                                 // samples from the row's length up to the width
        if (m < len) {
            long long src = m - back;
            if (wrap && src < 0) src += len;
            if (src >= 0 && src < len) v = px[src];
        }
        o[e] = v;
    }
}

// ---- cascaded biquads ---------------------------------------------------------------------------------------------------------------------
// The recurrence is serial in n; the sections of a row overlap as a software pipeline across lanes.  One wave is a workgroup; lane g S + s is
// section s of the workgroup's row g (G = min(64 / S, SOS_ROWS) rows).  In stage k a lane runs its section over block k - s of SOS_BLOCK
// samples, which it reads from ITS slot of an LDS buffer and writes to its right neighbour's slot: a section-0 slot is filled with the block of
// x by the whole wave (lane = sample of the block and row parity: coalesced, loaded one stage ahead, converted once), the last section writes
// to its row's output slot, which the whole wave stores to global memory one stage later.  Two buffers in turn, one barrier per stage; a lane
// reads its whole block into registers before it writes its first output, and no read or write is conditional on the section.  Every value is one section's own direct-form-II
// transposed update in fp64, every multiply and add rounded separately (no contraction), so the overlap changes no bit.  fp64 denormals are
// never flushed on gfx950.
constexpr int SOS_LANES = 64, SOS_BLOCK = 32, SOS_ROWS = 16, SOS_Q = SOS_ROWS / 2;     // a lane stages sample lane % 32 of rows lane / 32 + 2 q
static_assert(SOS_LANES == 2 * SOS_BLOCK, "a wave stages two rows of a block at a time");
struct SosTable { double c[STORM_SOS_MAX_SECTIONS][5]; };              // b0 b1 b2 a1 a2 of every section (a0 = 1)

// one sample through one section: scipy.signal.sosfilt's statements, in its order
__device__ __forceinline__ double sos_step(double xc, double b0, double b1, double b2, double a1, double a2, double& z0, double& z1) {
#pragma clang fp contract(off)
    const double xn = b0 * xc + z0;
    z0 = b1 * xc - a1 * xn + z1;
    z1 = b2 * xc - a2 * xn;
    return xn;
}

__global__ void __launch_bounds__(SOS_LANES)
sosfilt_rows_kernel(const float* __restrict__ x, long long stride_x, void* __restrict__ out, long long stride_o, int out_f32, long long L,
                    const int* __restrict__ row_len, SosTable tab, int S, int G, int B) {
    __shared__ double hand[2][SOS_BLOCK][SOS_LANES + SOS_ROWS];        // [stage parity][sample of the block][slot]: slot = reading lane, 64 + g = row g's output
    const int lane = threadIdx.x, g = lane / S, s = lane - g * S;
    const int row0 = blockIdx.x * G;
    const bool mine = g < G && row0 + g < B;
    const long long nblk = (L + SOS_BLOCK - 1) / SOS_BLOCK;
    const int sc = mine ? s : 0;
    const double b0 = tab.c[sc][0], b1 = tab.c[sc][1], b2 = tab.c[sc][2], a1 = tab.c[sc][3], a2 = tab.c[sc][4];
    double z0 = 0.0, z1 = 0.0;
    const int wslot = mine && s == S - 1 ? SOS_LANES + g : lane + 1;   // (lane 63 is never a writer that is not a last section: 64 / S rows fill at most 64 lanes)
    // the wave's share of a block: this lane moves sample si of the rows sg + 2 q of the workgroup
    const int si = lane & (SOS_BLOCK - 1), sg = lane >> 5;
    long long len_q[SOS_Q], lim_q[SOS_Q];                              // the row's length (reads, values) and its width (stores); 0: no such row
#pragma unroll
    for (int q = 0; q < SOS_Q; ++q) {
        const int gg = sg + 2 * q;
        const bool ok = gg < G && row0 + gg < B;
        const long long len = ok ? row_length(row_len, row0 + gg, L) : 0;
        len_q[q] = len > 0 ? len : 0; lim_q[q] = ok ? L : 0;
    }
    const float* px = x + (long long)(row0 + sg) * stride_x + si;
    const long long at0 = (long long)(row0 + sg) * stride_o + si;
    float pre[SOS_Q];
    const auto load_block = [&](long long blk) {
        const long long n = blk * SOS_BLOCK + si;
#pragma unroll
        for (int q = 0; q < SOS_Q; ++q) pre[q] = n < len_q[q] ? px[(long long)(2 * q) * stride_x + blk * SOS_BLOCK] : 0.f;
    };
    const auto stage_block = [&](int parity) {
#pragma unroll
        for (int q = 0; q < SOS_Q; ++q)
            if (sg + 2 * q < G) hand[parity][si][(sg + 2 * q) * S] = (double)pre[q];
    };
    load_block(0);
    stage_block(1);                                                    // (stage 0 reads the buffer of parity 1)
    __syncthreads();
    for (long long k = 0; k < nblk + S; ++k) {
        const int cur = (int)(k & 1), prev = cur ^ 1;
        const bool more = k + 1 < nblk;
        if (more) load_block(k + 1);                                   // (in flight during this stage's arithmetic)
        const long long ob = k - S;                                    // the block the last sections finished one stage ago
        if (ob >= 0) {
            const long long n = ob * SOS_BLOCK + si;
#pragma unroll
            for (int q = 0; q < SOS_Q; ++q) {
                if (n < lim_q[q]) {
                    const double v = n < len_q[q] ? hand[prev][si][SOS_LANES + sg + 2 * q] : 0.0;      // the tail of a row: zeros
                    const long long at = at0 + (long long)(2 * q) * stride_o + ob * SOS_BLOCK;
                    if (out_f32) static_cast<float*>(out)[at] = (float)v;
                    else static_cast<double*>(out)[at] = v;
                }
            }
        }
        const long long blk = k - s;
        if (mine && blk >= 0 && blk < nblk) {
            double in[SOS_BLOCK];                                      // all reads of the block first: one LDS latency, not one per sample
#pragma unroll
            for (int i = 0; i < SOS_BLOCK; ++i) in[i] = hand[prev][i][lane];
#pragma unroll
            for (int i = 0; i < SOS_BLOCK; ++i) hand[cur][i][wslot] = sos_step(in[i], b0, b1, b2, a1, a2, z0, z1);
        }
        if (more) stage_block(cur);                                    // (block k + 1 is read from this stage's buffer in the next stage)
        __syncthreads();
    }
}

// ---- Butterworth design (host) ------------------------------------------------------------------------------------------------------------
struct Cplx { double re, im; };
inline Cplx cmul(Cplx a, Cplx b) { return Cplx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline Cplx cdiv(Cplx a, Cplx b) {
    const double d = b.re * b.re + b.im * b.im;
    return Cplx{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}

}  // namespace storm

extern "C" int storm_butter_sos(int order, double wn, int highpass, double* sos_out) {
    using namespace storm;
    STORM_CHECK(sos_out != nullptr, "storm_butter_sos: null pointer");
    STORM_CHECK(order >= 2 && order % 2 == 0 && order <= 2 * STORM_SOS_MAX_SECTIONS, "storm_butter_sos: order=%d (even, in [2, %d]: an odd order has a first-order section, which this closed form does not design)",
                order, 2 * STORM_SOS_MAX_SECTIONS);
    STORM_CHECK(wn > 0.0 && wn < 1.0, "storm_butter_sos: wn=%g (the cut-off as a fraction of the Nyquist rate, inside (0, 1))", wn);
    const double pi = 3.14159265358979323846, fs2 = 4.0;               // the bilinear transform at fs = 2: 2 fs
    const double warped = fs2 * tan(pi * wn / 2.0);
    const int S = order / 2;
    // the prototype's poles -exp(j pi m / (2 N)), m = -N + 1, -N + 3, ..., N - 1, moved to the cut-off (lp2lp: p wo, lp2hp: wo / p) and through
    // the bilinear transform (4 + p) / (4 - p); the gain is real(4^N or wo^N / prod(4 - p)) over ALL poles in that order
    Cplx den{1.0, 0.0};
    Cplx pz[2 * STORM_SOS_MAX_SECTIONS];
    for (int i = 0; i < order; ++i) {
        const int m = -order + 1 + 2 * i;
        const double th = pi * (double)m / (2.0 * (double)order);
        const Cplx p{-cos(th), -sin(th)};
        const Cplx pa = highpass ? cdiv(Cplx{warped, 0.0}, p) : Cplx{p.re * warped, p.im * warped};
        const Cplx lo{fs2 - pa.re, -pa.im};
        pz[i] = cdiv(Cplx{fs2 + pa.re, pa.im}, lo);
        den = cmul(den, lo);
    }
    const double num = highpass ? pow(fs2, (double)order) : pow(warped, (double)order);
    const double gain = cdiv(Cplx{num, 0.0}, den).re;
    // conjugate pairs: pole i (m < 0) pairs with pole N - 1 - i; the pair nearest the unit circle goes last
    int idx[STORM_SOS_MAX_SECTIONS];
    double dist[STORM_SOS_MAX_SECTIONS];
    for (int i = 0; i < S; ++i) { idx[i] = i; dist[i] = fabs(1.0 - sqrt(pz[i].re * pz[i].re + pz[i].im * pz[i].im)); }
    for (int i = 1; i < S; ++i)                                        // (insertion sort, descending distance, stable)
        for (int j = i; j > 0 && dist[idx[j]] > dist[idx[j - 1]]; --j) { const int t = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = t; }
    for (int k = 0; k < S; ++k) {
        const Cplx p = pz[idx[k]];
        double* o = sos_out + 6 * k;
        const double g = k == 0 ? gain : 1.0;                          // the whole gain in the first section's numerator
        o[0] = g; o[1] = (highpass ? -2.0 : 2.0) * g; o[2] = g;        // zeros at +1 (high-pass) or -1 (low-pass), twice
        o[3] = 1.0; o[4] = -2.0 * p.re; o[5] = p.re * p.re + p.im * p.im;
    }
    return STORM_OK;
}

extern "C" int storm_xcorr_num_partials(long long Ny, long long Nr, int max_lag) {
    if (Ny < 1 || Nr < 1 || Ny > (1ll << 30) || Nr > (1ll << 30)) return 0;
    long long dmin, dmax;
    storm::xcorr_range(Ny, Nr, max_lag, dmin, dmax);
    return (int)((dmax - dmin) / storm::XCORR_TILE + 1);
}

extern "C" int storm_xcorr_lag_rows(const float* y, const float* ref, int* lag, double* peak, void* scratch, long long scratch_bytes, int B,
                                    long long Ny, long long Nr, long long stride_y, long long stride_ref, const int* y_len, const int* ref_len,
                                    int max_lag, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(y && ref && lag && peak && scratch, "storm_xcorr_lag_rows: null pointer");
    STORM_CHECK(B >= 1 && B <= 65535 && Ny >= 1 && Nr >= 1 && Ny <= (1ll << 30) && Nr <= (1ll << 30), "storm_xcorr_lag_rows: B=%d Ny=%lld Nr=%lld", B, Ny, Nr);
    STORM_CHECK(stride_y >= Ny && stride_ref >= Nr, "storm_xcorr_lag_rows: strides %lld %lld for rows of %lld / %lld", stride_y, stride_ref, Ny, Nr);
    const int tiles = storm_xcorr_num_partials(Ny, Nr, max_lag);
    const long long need = (long long)B * tiles * (long long)sizeof(XcorrPartial);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= need, "storm_xcorr_lag_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)",
                scratch, scratch_bytes, need);
    // lags per thread: the largest R that leaves a wave for every SIMD (four per CU), 2 when even that does not
    long long dmin, dmax;
    xcorr_range(Ny, Nr, max_lag, dmin, dmax);
    const long long lags = (long long)B * (dmax - dmin + 1), fill = (long long)device_cus() * 4 * 64;
    int R = switches().xcorr_lags;
    if (R != 2 && R != 4 && R != 8) R = lags >= 8 * fill ? 8 : (lags >= 4 * fill ? 4 : 2);
    const dim3 grid((unsigned)tiles, B);
#define STORM_XCORR_LAUNCH(r) hipLaunchKernelGGL(xcorr_tiles_kernel<r>, grid, dim3(XCORR_TILE / r), 0, (hipStream_t)st, y, ref, (XcorrPartial*)scratch, \
                                                 Ny, Nr, stride_y, stride_ref, y_len, ref_len, (long long)max_lag, tiles)
    if (R == 8) STORM_XCORR_LAUNCH(8);
    else if (R == 4) STORM_XCORR_LAUNCH(4);
    else STORM_XCORR_LAUNCH(2);
#undef STORM_XCORR_LAUNCH
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(xcorr_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)st, (const XcorrPartial*)scratch, lag, peak, Ny, Nr, y_len,
                       ref_len, (long long)max_lag, tiles, B);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_shift_rows(const float* x, float* out, const int* shift, int B, long long N, long long stride_x, long long stride_out,
                                const int* row_len, int wrap, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(x && out && shift, "storm_shift_rows: null pointer");
    STORM_CHECK(x != out, "storm_shift_rows: in place (out == x)");
    STORM_CHECK(B >= 1 && B <= 65535 && N >= 1 && N <= (1ll << 40), "storm_shift_rows: B=%d N=%lld", B, N);
    STORM_CHECK(stride_x >= N && stride_out >= N, "storm_shift_rows: strides %lld %lld for rows of %lld", stride_x, stride_out, N);
    const long long tiles = (N + SHIFT_TILE - 1) / SHIFT_TILE;
    STORM_CHECK(tiles <= 0x7fffffffll, "storm_shift_rows: N=%lld", N);
    hipLaunchKernelGGL(shift_rows_kernel, dim3((unsigned)tiles, B), dim3(SHIFT_THREADS), 0, (hipStream_t)st, x, stride_x, out, stride_out, N, shift,
                       row_len, wrap);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_sosfilt_rows(const float* x, void* out, const double* sos, int S, int B, long long L, long long stride_x, long long stride_out,
                                  const int* row_len, int out_f32, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(x && out && sos, "storm_sosfilt_rows: null pointer");
    STORM_CHECK(S >= 1 && S <= STORM_SOS_MAX_SECTIONS, "storm_sosfilt_rows: S=%d sections (1 to %d)", S, STORM_SOS_MAX_SECTIONS);
    STORM_CHECK(B >= 1 && L >= 1 && L <= (1ll << 40), "storm_sosfilt_rows: B=%d L=%lld", B, L);
    STORM_CHECK(stride_x >= L && stride_out >= L, "storm_sosfilt_rows: strides %lld %lld for rows of %lld", stride_x, stride_out, L);
    SosTable tab;
    for (int s = 0; s < STORM_SOS_MAX_SECTIONS; ++s)
        for (int j = 0; j < 5; ++j) tab.c[s][j] = 0.0;
    for (int s = 0; s < S; ++s) {
        STORM_CHECK(sos[6 * s + 3] == 1.0, "storm_sosfilt_rows: sos[%d][3] = %g (a0 must be 1, as scipy.signal.sosfilt requires)", s, sos[6 * s + 3]);
        tab.c[s][0] = sos[6 * s]; tab.c[s][1] = sos[6 * s + 1]; tab.c[s][2] = sos[6 * s + 2]; tab.c[s][3] = sos[6 * s + 4]; tab.c[s][4] = sos[6 * s + 5];
    }
    const int G = SOS_LANES / S < SOS_ROWS ? SOS_LANES / S : SOS_ROWS;
    hipLaunchKernelGGL(sosfilt_rows_kernel, dim3((unsigned)((B + G - 1) / G)), dim3(SOS_LANES), 0, (hipStream_t)st, x, stride_x, out, stride_out, out_f32, L,
                       row_len, tab, S, G, B);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
