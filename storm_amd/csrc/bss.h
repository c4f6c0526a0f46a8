// BSS-eval SDR of waveform rows on the device (Vincent et al. 2006: the estimate projected onto the span of flen delayed copies of the
// reference; the reference project does not compute it - include/storm_hip.h is the specification):
//   storm_bss_sdr_rows            per row the SDR in dB, optionally the solved filter and the correlations it was solved from (two launches),
//   storm_bss_sdr_scratch_bytes   the scratch the two launches hand their partials through.
// No atomics anywhere; whatever is summed is summed in an order that the indices inside the row fix, so a row's results are the same bits
// alone, in any batch, at any batch width, row stride and position.
// Included by spectral.hip alone (kernels and entry points live in that translation unit).
#pragma once
#include <math.h>
#include "common.h"
#include "align.h"

namespace storm {

// ---- correlations -------------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, piece of STORM_BSS_PIECE samples of the FIRST factor s[n]); it computes G[k] = sum s[n] s[n + k], D[k] = sum s[n]
// e[n + k] (k < flen) and Ee = sum e[n]^2 of the piece together: every one of them ONE fp64 fma chain in ascending n from +0 (fp32 x fp32 is
// exact in fp64, so every fma adds an exact product).  The walk is xcorr_tiles_kernel's: both rows are staged as fp64 in LDS a chunk at a time
// (second factors reach flen - 1 samples past the chunk, into the next piece where the row goes on, zeros from the row's length on: the
// chain starts at +0 and never becomes -0, so the +-0 product of such a term leaves it as it is), a thread keeps R consecutive lags of BOTH
// banks and a sliding register window of 2 R values of each row, and s[n] - which both banks share - is an LDS broadcast: a block of R steps
// of n reads 3 R doubles for 2 R^2 fmas.  The first factor is read from the same LDS image as the second: a chunk ends inside a block of R
// steps only at the row's end (pieces and chunks are multiples of R), where that image holds zeros.  Ee is thread 0's window of e against
// itself (its lag 0 is e[n]); every thread runs that chain on its own window and only thread 0's is written.  A workgroup has
// ceil(flen / R) threads rounded up to whole waves; lanes past flen walk lags nobody asked for and write nothing.  R = 8 has the most fmas
// per LDS read (the delay search measured it nearest the fp64 rate once every SIMD has a wave; this walk was measured at R = 2 only); a
// launch of few pieces (one file, a micro-batch) gets more waves from a smaller R.  The launcher picks the largest R in {8, 4, 2} that still
// gives every SIMD a wave, else 2; no bit depends on R - a chain is the same chain.
// What bounds a piece is issue, not the fp64 pipe or the LDS: a workgroup's waves sit alone on their
// SIMDs, and at R = 2 a step of n is 5 fp64 fmas (two lags of two banks and the Ee chain) in one wave's stream, whatever flen is and
// however many pieces (up to one per CU) the launch has: a third of a millisecond per piece (profiles/r18_bss_sdr.txt).  Reading the next
// block's LDS values ahead of the fmas (8 % slower) and a forced unroll of two blocks per pass (32 % slower; the compiler's own choice is
// four) were measured and not kept.
constexpr int BSS_TAPS = STORM_BSS_MAX_TAPS, BSS_PIECE = STORM_BSS_PIECE, BSS_CHUNK = 1024, BSS_LANES = 64;
static_assert(BSS_PIECE == STORM_METRICS_CHUNK, "STORM_BSS_PIECE: the cut of storm_energy_ratios_rows");
static_assert(BSS_PIECE % BSS_CHUNK == 0 && BSS_CHUNK % 8 == 0 && BSS_TAPS % (8 * BSS_LANES) == 0, "pieces and chunks: whole blocks of R = 2, 4, 8 steps; whole waves");

template <int R>
__global__ void __launch_bounds__(BSS_TAPS / R)
bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est, double* __restrict__ part, long long L, long long stride_r,
                long long stride_e, const int* __restrict__ row_len, int F, int pieces) {
    __shared__ __attribute__((aligned(16))) double sw[BSS_CHUNK + BSS_TAPS + R];
    __shared__ __attribute__((aligned(16))) double ew[BSS_CHUNK + BSS_TAPS + R];
    const int b = blockIdx.y, t = threadIdx.x, T = blockDim.x;
    const long long len = row_length(row_len, b, L);
    const long long p0 = (long long)blockIdx.x * BSS_PIECE;
    if (p0 >= len) return;                                             // (uniform) a piece past the row: the solve never reads its slot
    const long long pend = p0 + BSS_PIECE < len ? p0 + BSS_PIECE : len;
    const float* ps = ref + (long long)b * stride_r;
    const float* pe = est + (long long)b * stride_e;
    const int span = T * R, base = t * R;                              // the lags the workgroup walks (>= F, <= BSS_TAPS)
    double g[R], d[R], ee = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) { g[j] = 0.0; d[j] = 0.0; }

    for (long long c0 = p0; c0 < pend; c0 += BSS_CHUNK) {
        const int m = (int)(pend - c0 < BSS_CHUNK ? pend - c0 : BSS_CHUNK), mr = (m + R - 1) / R * R;
        for (int k = t; k < mr + span + R; k += T) {
            const long long idx = c0 + k;
            const bool in = idx < len;
            sw[k] = in ? (double)ps[idx] : 0.0;
            ew[k] = in ? (double)pe[idx] : 0.0;
        }
        __syncthreads();
        double ws[2 * R], we[2 * R];
        xcorr_load<R>(sw + base, ws);
        xcorr_load<R>(ew + base, we);
        for (int i = 0; i < mr; i += R) {
            double sv[R];
            xcorr_load<R>(sw + i + base + R, ws + R);
            xcorr_load<R>(ew + i + base + R, we + R);
            xcorr_load<R>(sw + i, sv);                                 // (every lane reads the same address)
#pragma unroll
            for (int u = 0; u < R; ++u)                                // ascending n; lag base + j reads s[n + k] = ws[u + j], e[n + k] = we[u + j]
#pragma unroll
                for (int j = 0; j < R; ++j) { g[j] = fma(sv[u], ws[u + j], g[j]); d[j] = fma(sv[u], we[u + j], d[j]); }
#pragma unroll
            for (int u = 0; u < R; ++u) ee = fma(we[u], we[u], ee);    // (every thread, thread 0's is Ee: a test of t costs every lane a select per fma)
#pragma unroll
            for (int j = 0; j < R; ++j) { ws[j] = ws[R + j]; we[j] = we[R + j]; }
        }
        __syncthreads();
    }

    double* o = part + ((long long)b * pieces + blockIdx.x) * (2 * F + 1);
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (base + j < F) { o[base + j] = g[j]; o[F + base + j] = d[j]; }
    if (t == 0) o[2 * F] = ee;
}

// ---- solve --------------------------------------------------------------------------------------------------------------------------------
// One WAVE per row.  Every one of the row's 2 flen + 1 numbers is the sum of its pieces in ascending order from +0.  Then the Levinson-Durbin
// recursion of the header in fp64: 511 dependent orders whose time is latency, so the row stays inside one wave - no multi-wave barrier, no
// LDS tree.  Lane l owns the entries i = l + 64 j (j < 8) of a and C in REGISTERS; G, D and a copy of a live in LDS, where the reversed
// operands G[m - i] and a[m - i] are read (consecutive lanes, consecutive addresses: no bank conflict).  The two dot products of an order are
// taken together: a lane's own terms as one fma chain in ascending j from +0 (terms with i >= m left out), then the xor butterfly over the
// lanes (32, 16, .. 1: addition commutes, so every lane ends with the same bits).  That shape depends on m only.  Every multiply-add of the
// recursion is a fused one, written as such.  The barriers order the LDS copy of a for a workgroup that is a single wave.  An order costs
// about a microsecond whatever m is (two butterflies of six dependent shuffles, two fp64 divisions, two LDS round trips, issued by a lone
// wave); a form that ran the C-half one order behind the a-half, its reductions and divisions side by side, measured 12 % slower
// (profiles/r18_bss_sdr.txt) and was not kept.
__global__ void __launch_bounds__(BSS_LANES)
bss_solve_kernel(const double* __restrict__ part, double* __restrict__ sdr, double* __restrict__ filt, double* __restrict__ parts, long long L,
                 const int* __restrict__ row_len, int F, int pieces) {
    constexpr int J = BSS_TAPS / BSS_LANES;
    __shared__ double Gs[BSS_TAPS], Ds[BSS_TAPS], As[BSS_TAPS], Es;
    const int b = blockIdx.x, l = threadIdx.x, W = 2 * F + 1;
    const long long len = row_length(row_len, b, L);
    const int nc = len <= 0 ? 0 : (int)((len + BSS_PIECE - 1) / BSS_PIECE);
    for (int k = l; k < W; k += BSS_LANES) {
        double v = 0.0;
        for (int c = 0; c < nc; ++c) v += part[((long long)b * pieces + c) * W + k];
        if (k < F) { Gs[k] = v; As[k] = k == 0 ? 1.0 : 0.0; }
        else if (k < 2 * F) Ds[k - F] = v;
        else Es = v;
        if (parts) parts[(long long)b * W + k] = v;
    }
    __syncthreads();
    const double Ee = Es, nan = __builtin_nan("");
    double E = Gs[0];
    bool bad = len < 1 || E == 0.0 || Ee == 0.0 || !(E > 0.0) || !isfinite(E);
    double a[J], c[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { a[j] = 0.0; c[j] = 0.0; }
    if (l == 0 && !bad) { a[0] = 1.0; c[0] = Ds[0] / E; }
    for (int m = 1; m < F && !bad; ++m) {                              // (E, lam, mu are the same bits in every lane: the loop is uniform)
        double da = 0.0, dc = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j < m && i < m) { const double gv = Gs[m - i]; da = fma(a[j], gv, da); dc = fma(c[j], gv, dc); }
        }
        da = wave_sum_d(da); dc = wave_sum_d(dc);
        const double lam = -da / E;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) a[j] = fma(lam, As[m - i], a[j]);
        }
        E = E * fma(-lam, lam, 1.0);
        if (!(E > 0.0) || !isfinite(E)) { bad = true; break; }
        const double mu = (Ds[m] - dc) / E;
        __syncthreads();                                               // every lane has read the old a
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) As[i] = a[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) c[j] = fma(mu, As[m - i], c[j]);
        }
    }
    double P = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int i = l + BSS_LANES * j;
        if (i < F) P = fma(Ds[i], c[j], P);
    }
    P = wave_sum_d(P);
    if (filt) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (i < F) filt[(long long)b * F + i] = bad ? nan : c[j];
        }
    }
    if (l == 0) {
        const double rest = Ee - P, inf = __builtin_inf();
        sdr[b] = bad ? nan : (rest <= 0.0 ? inf : (P > 0.0 ? 10.0 * log10(P / rest) : -inf));
    }
}

inline long long bss_pieces(long long L) { return (L + BSS_PIECE - 1) / BSS_PIECE; }

}  // namespace storm

extern "C" long long storm_bss_sdr_scratch_bytes(int B, long long L, int flen) {
    if (B < 1 || B > 65535 || L < 1 || L > (1ll << 30) || flen < 1 || flen > STORM_BSS_MAX_TAPS) return 0;
    return (long long)B * storm::bss_pieces(L) * (2 * flen + 1) * (long long)sizeof(double);
}

extern "C" int storm_bss_sdr_rows(const float* ref, const float* est, double* sdr, double* filt, double* parts, void* scratch,
                                  long long scratch_bytes, int B, long long L, long long stride_ref, long long stride_est, const int* row_len,
                                  int flen, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(ref && est && sdr && scratch, "storm_bss_sdr_rows: null pointer");
    STORM_CHECK(flen >= 1 && flen <= STORM_BSS_MAX_TAPS, "storm_bss_sdr_rows: flen=%d (1 to %d taps)", flen, STORM_BSS_MAX_TAPS);
    STORM_CHECK(B >= 1 && B <= 65535, "storm_bss_sdr_rows: B=%d (1 to 65535 rows)", B);
    STORM_CHECK(L >= 1 && L <= (1ll << 30), "storm_bss_sdr_rows: L=%lld (1 to 2^30 samples)", L);
    STORM_CHECK(stride_ref >= L && stride_est >= L, "storm_bss_sdr_rows: strides %lld %lld for rows of %lld", stride_ref, stride_est, L);
    const long long need = storm_bss_sdr_scratch_bytes(B, L, flen);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= need, "storm_bss_sdr_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)",
                scratch, scratch_bytes, need);
    const int pieces = (int)bss_pieces(L);
    // lags per thread: the largest R that leaves a wave for every SIMD (four per CU) and whose one wave of 64 R lags is not wider than flen,
    // 2 when even that does not
    const long long chains = (long long)B * pieces * flen, fill = (long long)device_cus() * 4 * 64;
    int R = switches().bss_lags;
    if (R != 2 && R != 4 && R != 8) {
        R = chains >= 8 * fill ? 8 : (chains >= 4 * fill ? 4 : 2);
        while (R > 2 && flen < BSS_LANES * R) R /= 2;
    }
    const int threads = ((flen + R - 1) / R + BSS_LANES - 1) / BSS_LANES * BSS_LANES;
    const dim3 grid((unsigned)pieces, B);
#define STORM_BSS_LAUNCH(r) hipLaunchKernelGGL(bss_corr_kernel<r>, grid, dim3(threads), 0, (hipStream_t)st, ref, est, (double*)scratch, L, stride_ref, \
                                               stride_est, row_len, flen, pieces)
    if (R == 8) STORM_BSS_LAUNCH(8);
    else if (R == 4) STORM_BSS_LAUNCH(4);
    else STORM_BSS_LAUNCH(2);
#undef STORM_BSS_LAUNCH
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(bss_solve_kernel, dim3(B), dim3(BSS_LANES), 0, (hipStream_t)st, (const double*)scratch, sdr, filt, parts, L, row_len, flen, pieces);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
