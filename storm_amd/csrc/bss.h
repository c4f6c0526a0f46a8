// BSS-eval SDR of waveform rows on the device (Vincent et al. 2006: the estimate projected onto the span of flen delayed copies of the
// reference; the reference project does not compute it - include/storm_hip.h is the specification):
//   storm_bss_sdr_rows            per row the SDR in dB, optionally the solved filter and the correlations it was solved from (two launches),
//   storm_bss_sdr_scratch_bytes   the scratch the two launches hand their partials through,
//   storm_bss_eval_rows           per row SDR, SIR and SAR against a target AND a noise row (bss_eval_sources with two sources): the four pairs'
//                                 correlations as one grid, the SDR's solve, a block Levinson recursion for the joint projection (three launches),
//   storm_bss_eval_scratch_bytes  its scratch.
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
__device__ __forceinline__ void bss_corr_piece(const float* __restrict__ ref, const float* __restrict__ est, double* __restrict__ part, long long L,
                                               long long stride_r, long long stride_e, const int* __restrict__ row_len, int F, int pieces) {
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

template <int R>
__global__ void __launch_bounds__(BSS_TAPS / R)
bss_corr_kernel(const float* __restrict__ ref, const float* __restrict__ est, double* __restrict__ part, long long L, long long stride_r,
                long long stride_e, const int* __restrict__ row_len, int F, int pieces) {
    bss_corr_piece<R>(ref, est, part, L, stride_r, stride_e, row_len, F, pieces);
}

// The four pairs of storm_bss_eval_rows as ONE grid: blockIdx.z picks (first factor, second factor) = (s1, e), (s2, e), (s1, s2), (s2, s1)
// and the pair's region of the scratch; a workgroup then walks its piece exactly as above, so every number is the bits of the one-pair
// launch on that pair.  (G11 and G22 are walked twice and three of the four Ee chains are not used: the price of not touching the walk.)
template <int R>
__global__ void __launch_bounds__(BSS_TAPS / R)
bss_corr4_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ e, double* __restrict__ part, long long region,
                 long long L, long long stride_1, long long stride_2, long long stride_e, const int* __restrict__ row_len, int F, int pieces) {
    const int z = blockIdx.z;
    const float* first = (z & 1) ? s2 : s1;
    const long long sf = (z & 1) ? stride_2 : stride_1;
    const float* second = z < 2 ? e : (z == 2 ? s2 : s1);
    const long long ss = z < 2 ? stride_e : (z == 2 ? stride_2 : stride_1);
    bss_corr_piece<R>(first, second, part + z * region, L, sf, ss, row_len, F, pieces);
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
                 const int* __restrict__ row_len, int F, int pieces, double* __restrict__ proj, int sdr_stride) {
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
        sdr[(long long)b * sdr_stride] = bad ? nan : (rest <= 0.0 ? inf : (P > 0.0 ? 10.0 * log10(P / rest) : -inf));
        if (proj) proj[b] = bad ? nan : P;                             // (storm_bss_eval_rows: P1 of its SIR)
    }
}

// ---- joint solve (storm_bss_eval_rows) ----------------------------------------------------------------------------------------------------
// The 2 F x 2 F block-Toeplitz system of the header by the block Levinson recursion (Whittle 1963; Wiggins & Robinson 1965) with 2 x 2
// blocks, one WAVE per row like the solve above and for its reason: F - 1 dependent orders whose time is latency.  That recursion was built
// and not a blocked Cholesky of the dense matrix because it met the bound (tests/test_bss_eval.py: 1e-4 dB against two dense host solvers up to a
// joint condition of 1e8) with 56 KB of LDS and no global scratch, where the Cholesky needs 8 MB per row and multi-wave barriers.
//   forward predictor  A = (I, A_1 .. A_m)      T A = (Ef, 0 .. 0)        backward predictor  B = (B_0 .. B_{m-1}, I)   T B = (0 .. 0, Eb)
// (T the block-Toeplitz matrix of order m, blocks R(k - l), R(-p) = R(p)^T; A_j, B_j, Ef, Eb are 2 x 2.)  The backward predictor is KEPT
// REVERSED, Bt_j = B_{m-j}, so that both updates read their other operand at the mirrored index m - j, as the scalar recursion does:
//   Delta = sum_{j<m} R(m - j) A_j      delta = sum_{j<m} R(m - j) x_j                  (2 x 2 and 2: six reductions, one butterfly pass)
//   Kf = -Eb^-1 Delta    Kb = -Ef^-1 Delta^T                                            (the backward residual is Delta^T: T is symmetric)
//   A_j <- A_j + Bt_{m-j} Kf     Bt_j <- Bt_j + A_{m-j} Kb      (j = 0 .. m, old values on the right, A_m = Bt_m = 0 before)
//   Ef <- Ef + Delta^T Kf        Eb <- Eb + Delta Kb            (the off-diagonal pair averaged: symmetric in exact arithmetic)
//   g = Eb^-1 (d_m - delta)      x_j <- x_j + Bt_{m-j} g        (the new Eb and Bt)
// Block j sits in lane j mod 64: A_j, Bt_j, x_j in registers (80 doubles a lane), the correlations and a copy of A and Bt in LDS, where the
// mirrored operands are read (consecutive lanes, consecutive addresses).  A lane's terms of the six sums are fma chains in ascending j from
// +0, then the xor butterfly: a shape that depends on m only.  A 2 x 2 error matrix is factored as L diag(a, p) L^T (l = b / a, p = c - l b)
// and is refused - the row's sir, sar and filter are NaN - unless a > 0, p > 0 and both are finite: the non-positive pivot of the header.
struct BssLdl { double l, ia, ip; bool ok; };
__device__ inline BssLdl bss_ldl(double a, double b, double c) {
    BssLdl f;
    f.l = b / a;
    const double p = fma(-f.l, b, c);
    f.ia = 1.0 / a;
    f.ip = 1.0 / p;
    f.ok = a > 0.0 && p > 0.0 && isfinite(a) && isfinite(p);
    return f;
}
__device__ inline void bss_ldl_solve(const BssLdl& f, double r0, double r1, double& y0, double& y1) {   // [[a, b], [b, c]] y = r
    y1 = fma(-f.l, r0, r1) * f.ip;
    y0 = fma(-f.l, y1, r0 * f.ia);
}

__global__ void __launch_bounds__(BSS_LANES)
bss_joint_kernel(const double* __restrict__ part, long long region, const double* __restrict__ proj, double* __restrict__ out,
                 double* __restrict__ filt, double* __restrict__ parts, long long L, const int* __restrict__ row_len, int F, int pieces) {
    constexpr int J = BSS_TAPS / BSS_LANES;
    __shared__ double Rs[4][BSS_TAPS];                                 // R(p)[r][c] = Rs[2 r + c][p]: G11, X12, X21, G22
    __shared__ double Ds[2][BSS_TAPS], As[4][BSS_TAPS], Bs[4][BSS_TAPS], Es;
    const int b = blockIdx.x, l = threadIdx.x, W = 2 * F + 1;
    const long long len = row_length(row_len, b, L);
    const int nc = len <= 0 ? 0 : (int)((len + BSS_PIECE - 1) / BSS_PIECE);
    for (int k = l; k < 6 * F + 1; k += BSS_LANES) {                   // the output order G11, D1, G22, D2, X12, X21, Ee
        const int q = k / F, i = k - q * F;                            // (q == 6: Ee)
        const int z = q < 4 ? q >> 1 : (q == 4 ? 2 : (q == 5 ? 3 : 0));                      // the pair's region of the scratch
        const int off = q == 6 ? 2 * F : ((q == 0 || q == 2) ? i : F + i);                   // its first bank, its second bank, its Ee
        const double* src = part + z * region + (long long)b * pieces * W + off;
        double v = 0.0;
        for (int c = 0; c < nc; ++c) v += src[(long long)c * W];
        if (q == 0) Rs[0][i] = v;
        else if (q == 1) Ds[0][i] = v;
        else if (q == 2) Rs[3][i] = v;
        else if (q == 3) Ds[1][i] = v;
        else if (q == 4) Rs[1][i] = v;
        else if (q == 5) Rs[2][i] = v;
        else Es = v;
        if (parts) parts[(long long)b * (6 * F + 1) + k] = v;
    }
    for (int k = l; k < F; k += BSS_LANES)
#pragma unroll
        for (int c = 0; c < 4; ++c) As[c][k] = Bs[c][k] = (k == 0 && (c == 0 || c == 3)) ? 1.0 : 0.0;
    __syncthreads();
    const double Ee = Es, P1 = proj[b], sdr = out[3 * (long long)b], nan = __builtin_nan(""), inf = __builtin_inf();
    double Ef[3] = {Rs[0][0], Rs[1][0], Rs[3][0]}, Eb[3] = {Ef[0], Ef[1], Ef[2]};              // e00, e01 = e10, e11
    BssLdl ef = bss_ldl(Ef[0], Ef[1], Ef[2]), eb = ef;
    // (the same bits in every lane, like every scalar below: the loop is uniform)  len < F + 1: 2 F copies in len + F - 1 dimensions, always dependent
    bool bad = sdr != sdr || len < F + 1 || !(Ef[2] > 0.0) || !ef.ok;
    double a[J][4], bt[J][4], x[J][2];
#pragma unroll
    for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { a[j][c] = 0.0; bt[j][c] = 0.0; }
        x[j][0] = 0.0; x[j][1] = 0.0;
    }
    if (l == 0 && !bad) {
        a[0][0] = a[0][3] = bt[0][0] = bt[0][3] = 1.0;
        bss_ldl_solve(ef, Ds[0][0], Ds[1][0], x[0][0], x[0][1]);
    }
    for (int m = 1; m < F && !bad; ++m) {
        double dl[4] = {0.0, 0.0, 0.0, 0.0}, dx[2] = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j < m && i < m) {
                const int p = m - i;
                const double r00 = Rs[0][p], r01 = Rs[1][p], r10 = Rs[2][p], r11 = Rs[3][p];
                dl[0] = fma(r01, a[j][2], fma(r00, a[j][0], dl[0]));
                dl[1] = fma(r01, a[j][3], fma(r00, a[j][1], dl[1]));
                dl[2] = fma(r11, a[j][2], fma(r10, a[j][0], dl[2]));
                dl[3] = fma(r11, a[j][3], fma(r10, a[j][1], dl[3]));
                dx[0] = fma(r01, x[j][1], fma(r00, x[j][0], dx[0]));
                dx[1] = fma(r11, x[j][1], fma(r10, x[j][0], dx[1]));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                             // wave_sum_d of the six together: their shuffles overlap
#pragma unroll
            for (int c = 0; c < 4; ++c) dl[c] += __shfl_xor(dl[c], o, 64);
            dx[0] += __shfl_xor(dx[0], o, 64);
            dx[1] += __shfl_xor(dx[1], o, 64);
        }
        double kf[4], kb[4];                                           // [r][c] at 2 r + c
        bss_ldl_solve(eb, -dl[0], -dl[2], kf[0], kf[2]);               // Eb Kf = -Delta, a column at a time
        bss_ldl_solve(eb, -dl[1], -dl[3], kf[1], kf[3]);
        bss_ldl_solve(ef, -dl[0], -dl[1], kb[0], kb[2]);               // Ef Kb = -Delta^T
        bss_ldl_solve(ef, -dl[2], -dl[3], kb[1], kb[3]);
        const double f01 = fma(dl[2], kf[3], fma(dl[0], kf[1], Ef[1])), f10 = fma(dl[3], kf[2], fma(dl[1], kf[0], Ef[1]));
        const double b01 = fma(dl[1], kb[3], fma(dl[0], kb[1], Eb[1])), b10 = fma(dl[3], kb[2], fma(dl[2], kb[0], Eb[1]));
        Ef[0] = fma(dl[2], kf[2], fma(dl[0], kf[0], Ef[0]));
        Ef[2] = fma(dl[3], kf[3], fma(dl[1], kf[1], Ef[2]));
        Ef[1] = 0.5 * (f01 + f10);
        Eb[0] = fma(dl[1], kb[2], fma(dl[0], kb[0], Eb[0]));
        Eb[2] = fma(dl[3], kb[3], fma(dl[2], kb[1], Eb[2]));
        Eb[1] = 0.5 * (b01 + b10);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) {
                const int q = m - i;
                const double t0 = Bs[0][q], t1 = Bs[1][q], t2 = Bs[2][q], t3 = Bs[3][q];
                const double u0 = As[0][q], u1 = As[1][q], u2 = As[2][q], u3 = As[3][q];
                a[j][0] = fma(t1, kf[2], fma(t0, kf[0], a[j][0]));
                a[j][1] = fma(t1, kf[3], fma(t0, kf[1], a[j][1]));
                a[j][2] = fma(t3, kf[2], fma(t2, kf[0], a[j][2]));
                a[j][3] = fma(t3, kf[3], fma(t2, kf[1], a[j][3]));
                bt[j][0] = fma(u1, kb[2], fma(u0, kb[0], bt[j][0]));
                bt[j][1] = fma(u1, kb[3], fma(u0, kb[1], bt[j][1]));
                bt[j][2] = fma(u3, kb[2], fma(u2, kb[0], bt[j][2]));
                bt[j][3] = fma(u3, kb[3], fma(u2, kb[1], bt[j][3]));
            }
        }
        ef = bss_ldl(Ef[0], Ef[1], Ef[2]);
        eb = bss_ldl(Eb[0], Eb[1], Eb[2]);
        if (!ef.ok || !eb.ok) { bad = true; break; }
        double g0, g1;
        bss_ldl_solve(eb, Ds[0][m] - dx[0], Ds[1][m] - dx[1], g0, g1);
        __syncthreads();                                               // every lane has read the old A and Bt
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) {
#pragma unroll
                for (int c = 0; c < 4; ++c) { As[c][i] = a[j][c]; Bs[c][i] = bt[j][c]; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (BSS_LANES * j <= m && i <= m) {
                const int q = m - i;
                x[j][0] = fma(Bs[1][q], g1, fma(Bs[0][q], g0, x[j][0]));
                x[j][1] = fma(Bs[3][q], g1, fma(Bs[2][q], g0, x[j][1]));
            }
        }
    }
    double P = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int i = l + BSS_LANES * j;
        if (i < F) P = fma(Ds[1][i], x[j][1], fma(Ds[0][i], x[j][0], P));
    }
    P = wave_sum_d(P);
    if (filt) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int i = l + BSS_LANES * j;
            if (i < F) {
                filt[((long long)b * 2 + 0) * F + i] = bad ? nan : x[j][0];
                filt[((long long)b * 2 + 1) * F + i] = bad ? nan : x[j][1];
            }
        }
    }
    if (l == 0) {
        const double over = P - P1, rest = Ee - P;
        out[3 * (long long)b + 1] = bad ? nan : (over <= 0.0 ? (P1 > 0.0 ? inf : nan) : (P1 > 0.0 ? 10.0 * log10(P1 / over) : -inf));
        out[3 * (long long)b + 2] = bad ? nan : (rest <= 0.0 ? inf : (P > 0.0 ? 10.0 * log10(P / rest) : -inf));
    }
}

inline long long bss_pieces(long long L) { return (L + BSS_PIECE - 1) / BSS_PIECE; }

// lags per thread of a correlation launch of `chains` chains: the largest R that leaves a wave for every SIMD (four per CU) and whose one
// wave of 64 R lags is not wider than flen, 2 when even that does not
inline int bss_lags_per_thread(long long chains, int flen) {
    const long long fill = (long long)device_cus() * 4 * 64;
    int R = switches().bss_lags;
    if (R != 2 && R != 4 && R != 8) {
        R = chains >= 8 * fill ? 8 : (chains >= 4 * fill ? 4 : 2);
        while (R > 2 && flen < BSS_LANES * R) R /= 2;
    }
    return R;
}

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
    const int R = bss_lags_per_thread((long long)B * pieces * flen, flen);
    const int threads = ((flen + R - 1) / R + BSS_LANES - 1) / BSS_LANES * BSS_LANES;
    const dim3 grid((unsigned)pieces, B);
#define STORM_BSS_LAUNCH(r) hipLaunchKernelGGL(bss_corr_kernel<r>, grid, dim3(threads), 0, (hipStream_t)st, ref, est, (double*)scratch, L, stride_ref, \
                                               stride_est, row_len, flen, pieces)
    if (R == 8) STORM_BSS_LAUNCH(8);
    else if (R == 4) STORM_BSS_LAUNCH(4);
    else STORM_BSS_LAUNCH(2);
#undef STORM_BSS_LAUNCH
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(bss_solve_kernel, dim3(B), dim3(BSS_LANES), 0, (hipStream_t)st, (const double*)scratch, sdr, filt, parts, L, row_len, flen, pieces,
                       (double*)nullptr, 1);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" long long storm_bss_eval_scratch_bytes(int B, long long L, int flen) {
    const long long pair = storm_bss_sdr_scratch_bytes(B, L, flen);    // (0: refused)
    return pair == 0 ? 0 : 4 * pair + (long long)B * (long long)sizeof(double);
}

extern "C" int storm_bss_eval_rows(const float* target, const float* noise, const float* est, double* out, double* filt, double* parts, void* scratch,
                                   long long scratch_bytes, int B, long long L, long long stride_t, long long stride_n, long long stride_e,
                                   const int* row_len, int flen, storm_stream_t st) {
    using namespace storm;
    STORM_CHECK(target && noise && est && out && scratch, "storm_bss_eval_rows: null pointer");
    STORM_CHECK(flen >= 1 && flen <= STORM_BSS_MAX_TAPS, "storm_bss_eval_rows: flen=%d (1 to %d taps)", flen, STORM_BSS_MAX_TAPS);
    STORM_CHECK(B >= 1 && B <= 65535, "storm_bss_eval_rows: B=%d (1 to 65535 rows)", B);
    STORM_CHECK(L >= 1 && L <= (1ll << 30), "storm_bss_eval_rows: L=%lld (1 to 2^30 samples)", L);
    STORM_CHECK(stride_t >= L && stride_n >= L && stride_e >= L, "storm_bss_eval_rows: strides %lld %lld %lld for rows of %lld", stride_t, stride_n,
                stride_e, L);
    const long long need = storm_bss_eval_scratch_bytes(B, L, flen);
    STORM_CHECK(((uintptr_t)scratch & 7) == 0 && scratch_bytes >= need, "storm_bss_eval_rows: scratch %p of %lld bytes, %lld needed (8-byte aligned)",
                scratch, scratch_bytes, need);
    const int pieces = (int)bss_pieces(L);
    const long long region = (long long)B * pieces * (2 * flen + 1);   // doubles per pair; then B doubles: P1 of every row
    double* part = (double*)scratch;
    double* proj = part + 4 * region;
    const int R = bss_lags_per_thread(4ll * B * pieces * flen, flen);
    const int threads = ((flen + R - 1) / R + BSS_LANES - 1) / BSS_LANES * BSS_LANES;
    const dim3 grid((unsigned)pieces, B, 4);
#define STORM_BSS_LAUNCH(r) hipLaunchKernelGGL(bss_corr4_kernel<r>, grid, dim3(threads), 0, (hipStream_t)st, target, noise, est, part, region, L, stride_t, \
                                               stride_n, stride_e, row_len, flen, pieces)
    if (R == 8) STORM_BSS_LAUNCH(8);
    else if (R == 4) STORM_BSS_LAUNCH(4);
    else STORM_BSS_LAUNCH(2);
#undef STORM_BSS_LAUNCH
    STORM_LAUNCH_CHECK();
    // the sdr column and P1: round 18's solve on the (target, estimate) region, writing out[b][0]; then the joint solve fills out[b][1 .. 2]
    hipLaunchKernelGGL(bss_solve_kernel, dim3(B), dim3(BSS_LANES), 0, (hipStream_t)st, (const double*)part, out, (double*)nullptr, (double*)nullptr, L,
                       row_len, flen, pieces, proj, 3);
    STORM_LAUNCH_CHECK();
    hipLaunchKernelGGL(bss_joint_kernel, dim3(B), dim3(BSS_LANES), 0, (hipStream_t)st, (const double*)part, region, (const double*)proj, out, filt, parts, L,
                       row_len, flen, pieces);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
