// ConvTasNet (the reference's backbones/convtasnet.py: learnt encoder, TCN separator, learnt decoder) - the 1-D, time-domain
// network of the engine.  Activations are channels-last [B][L][C] in the compute dtype; the TCN's two running sums (`output`,
// `skip_connection`) are fp32 [B][L][BN]; statistics are fp32.  Five kernels:
//   * tasnet_encode      pad_signal (convtasnet.py:75-94) + Conv1d(1, N, win, stride) in one pass, + partial sums for TCN.LN;
//   * tasnet_gln_finalize  per-wave (sum, sumsq) partials of a row -> (mean, rstd) of GroupNorm(1, C, eps) over all of C x L;
//   * tasnet_pointwise   the 1x1 convolutions as MFMA GEMMs (32x32x16 bf16 / f16, 32x32x2 f32) straight from global memory:
//                        A = weight rows, B = activation rows rewritten in registers on load (norm-apply or PReLU), epilogue =
//                        bias (+ scalar PReLU + partials of the next norm), or the fused res_out + skip_out form that adds its two
//                        column halves to `output` and `skip_connection` in place;
//   * tasnet_depthwise   3 taps, dilation d, groups = C: norm-apply on load (the zero padding comes AFTER the norm: an out-of-range
//                        tap adds 0), + bias, PReLU, partials of reg2;
//   * tasnet_decode      sigmoid(mask) * enc and ConvTranspose1d(N, 1, win, stride) as a gather: no atomics, fixed sum order.
// No normalised tensor is ever written.  Every partial-sum slot is written by exactly one wave, so results do not depend on
// scheduling and a row's values do not depend on the batch it is in.
// Included by spectral.hip (which defines STORM_TASNET_IMPL and so owns the kernels) and by abi.hip (declarations only).
#pragma once
#include <type_traits>
#include "common.h"
#include "conv_params.h"

namespace storm {

enum { TASNET_OP_ENCODE = 0, TASNET_OP_POINTWISE = 1, TASNET_OP_DEPTHWISE = 2 };
constexpr int TASNET_PW_ROWS = 128, TASNET_PW_COLS = 64;      // frames x output channels of a pointwise workgroup (4 waves x 32 frames)

struct TasnetPointwise {
    const void* x; const void* w; const float* bias; void* out; float* skip;
    const float* stats; const float* gamma; const float* beta; const float* prelu_in; const float* prelu_out; float* part;
    int L, Cin, Cout, x_f32, out_f32, res_skip;
};

// per-row partial-sum slots ((sum, sumsq) fp32 pairs) the producing kernel of `op` writes for L frames of C output channels
int tasnet_num_partials(int op, int L, int C);
int launch_tasnet_encode(const float* wav, long long wav_stride, const float* wT, void* enc, float* part, int B, long long T, int N,
                         int win, int stride, int L, int dtype, hipStream_t st);
int launch_tasnet_gln_finalize(const float* part, float* stats, int B, int nparts, long long count, float eps, hipStream_t st);
int launch_tasnet_pointwise(const TasnetPointwise& p, int B, int dtype, hipStream_t st);
int launch_tasnet_depthwise(const void* x, const float* w3, const float* bias, const float* stats, const float* gamma, const float* beta,
                            const float* prelu, void* out, float* part, int B, int L, int C, int dilation, int dtype, hipStream_t st);
int launch_tasnet_decode(const void* mask, const void* enc, const float* wd, float* out, int B, int L, int N, int win, int stride,
                         int dtype, hipStream_t st);

#ifdef STORM_TASNET_IMPL

// the value an activation of type T holds after a store of v
template <typename T> __device__ __forceinline__ float tn_round(float v) { T t; from_f32(t, v); return to_f32(t); }

// (sum, sumsq) of a wave's lanes -> slot `slot` of row b; the wave reduction runs in fp64, the slot is fp32
__device__ __forceinline__ void tn_write_partial(float s, float q, float* part, long long slot) {
    const double ds = wave_sum_d((double)s), dq = wave_sum_d((double)q);
    if ((threadIdx.x & 63) == 0) { part[2 * slot] = (float)ds; part[2 * slot + 1] = (float)dq; }
}

template <typename T>
__global__ void __launch_bounds__(256) tasnet_encode_kernel(const float* __restrict__ wav, long long wav_stride, const float* __restrict__ wT,
                                                            T* __restrict__ enc, float* __restrict__ part, long long T_in, int N, int win,
                                                            int stride, int L) {
    const int b = blockIdx.y, ncg = N / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = idx < (long long)L * ncg;
    float s = 0.f, q = 0.f;
    if (valid) {
        const int l = (int)(idx / ncg), c = (int)(idx % ncg) * 8;
        const float* x = wav + (long long)b * wav_stride;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < win; ++k) {
            const long long t = (long long)l * stride + k - stride;      // pad_signal: `stride` zeros in front, zeros past the end
            const float xv = (t >= 0 && t < T_in) ? x[t] : 0.f;
            float w[8];
            load8(wT + (long long)k * N + c, w);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(xv, w[i], acc[i]);
        }
        store8(enc + ((long long)b * L + l) * N + c, acc);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float v = tn_round<T>(acc[i]); s += v; q += v * v; }
    }
    tn_write_partial(s, q, part, ((long long)b * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6));
}

__global__ void __launch_bounds__(64) tasnet_gln_finalize_kernel(const float* __restrict__ part, float* __restrict__ stats, int nparts,
                                                                 long long count, float eps) {
    const int b = blockIdx.x;
    const float* p = part + (long long)b * nparts * 2;
    double s = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) { s += (double)p[2 * i]; q += (double)p[2 * i + 1]; }
    s = wave_sum_d(s); q = wave_sum_d(q);
    if (threadIdx.x == 0) {
        const double mean = s / (double)count;
        double var = q / (double)count - mean * mean;        // biased, as GroupNorm
        if (var < 0.0) var = 0.0;
        stats[2 * b] = (float)mean;
        stats[2 * b + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

template <typename T, int N> __device__ __forceinline__ typename Mma<T>::Frag tn_frag(const float (&v)[N]) {
    typename Mma<T>::Frag f;
    if constexpr (sizeof(T) == 2) { const uint4 r = pack8<T>(v); __builtin_memcpy(&f, &r, 16); }
    else { f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; }
    return f;
}
template <int N, typename S> __device__ __forceinline__ void tn_load(const S* p, float (&v)[N]) {
    if constexpr (N == 8) load8(p, v);
    else { const float4 a = *reinterpret_cast<const float4*>(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
}

// out[b][l][co] = sum_ci W[co][ci] * pre(x[b][l][ci]) + bias[co].  A wave owns 32 frames x 64 output channels: its activation
// fragment (lane = frame, 8 / 4 consecutive channels) is rewritten once per k-step and feeds two MFMAs; D has the frame on the lane
// and 4 consecutive output channels in registers 4g .. 4g+3, so a store is one 8- / 16-byte vector.
template <typename T, bool IN_F32>
__global__ void __launch_bounds__(256) tasnet_pointwise_kernel(TasnetPointwise p) {
    typedef typename Mma<T>::Frag Frag;
    typedef typename std::conditional<IN_F32, float, T>::type TIn;
    constexpr int KS = Elem<T>::PER16;                 // channels of a lane's fragment; a k-step is 2 * KS channels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, L = p.L, Cin = p.Cin, Cout = p.Cout;
    const int l = blockIdx.x * TASNET_PW_ROWS + wave * 32 + r, co0 = blockIdx.y * TASNET_PW_COLS;
    const bool lv = l < L;
    const TIn* xrow = static_cast<const TIn*>(p.x) + ((long long)b * L + (lv ? l : 0)) * Cin;
    const T* w = static_cast<const T*>(p.w);
    float mean = 0.f, rstd = 1.f, slope_in = 1.f;
    if (p.stats) { mean = p.stats[2 * b]; rstd = p.stats[2 * b + 1]; }
    if (p.prelu_in) slope_in = p.prelu_in[0];
    f32x16 acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nt][i] = 0.f;

    for (int k0 = 0; k0 < Cin; k0 += 2 * KS) {
        const int kc = k0 + KS * h;
        const bool kv = kc < Cin;
        float v[KS];
#pragma unroll
        for (int i = 0; i < KS; ++i) v[i] = 0.f;
        if (lv && kv) {
            tn_load<KS>(xrow + kc, v);
            if (p.stats) {                              // (x - mean) * rstd * gamma_c + beta_c
                float g[KS], be[KS];
                tn_load<KS>(p.gamma + kc, g);
                tn_load<KS>(p.beta + kc, be);
#pragma unroll
                for (int i = 0; i < KS; ++i) { const float sc = rstd * g[i]; v[i] = fmaf(v[i], sc, be[i] - mean * sc); }
            } else if (p.prelu_in) {
#pragma unroll
                for (int i = 0; i < KS; ++i) v[i] = v[i] >= 0.f ? v[i] : slope_in * v[i];
            }
        }
        const Frag fb = tn_frag<T, KS>(v);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int co = co0 + 32 * nt + r;
            Frag fa;
            __builtin_memset(&fa, 0, sizeof(fa));
            if (co < Cout && kv) fa = *reinterpret_cast<const Frag*>(w + (long long)co * Cin + kc);
            Mma<T>::run(fa, fb, acc[nt]);
        }
    }

    const float slope_out = p.prelu_out ? p.prelu_out[0] : 1.f;
    const int BN = Cout / 2;
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = co0 + 32 * nt + 8 * g + 4 * h;                 // registers 4g .. 4g+3: rows co .. co+3 of D, column l
            if (!lv || co >= Cout) continue;
            const float4 bi = *reinterpret_cast<const float4*>(p.bias + co);
            float y[4] = {acc[nt][4 * g] + bi.x, acc[nt][4 * g + 1] + bi.y, acc[nt][4 * g + 2] + bi.z, acc[nt][4 * g + 3] + bi.w};
            if (p.res_skip) {                                             // output += res_out(x), skip_connection += skip_out(x)
                float* dst = (co < BN ? static_cast<float*>(p.out) : p.skip) + ((long long)b * L + l) * BN + (co < BN ? co : co - BN);
                float4 o = *reinterpret_cast<float4*>(dst);
                o.x += y[0]; o.y += y[1]; o.z += y[2]; o.w += y[3];
                *reinterpret_cast<float4*>(dst) = o;
                continue;
            }
            if (p.prelu_out) {
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = y[i] >= 0.f ? y[i] : slope_out * y[i];
            }
            const long long o = ((long long)b * L + l) * Cout + co;
            if (sizeof(T) == 4 || p.out_f32) {
                *reinterpret_cast<float4*>(static_cast<float*>(p.out) + o) = make_float4(y[0], y[1], y[2], y[3]);
            } else if constexpr (sizeof(T) == 2) {
                *reinterpret_cast<uint2*>(static_cast<T*>(p.out) + o) = make_uint2(pack2(y[0], y[1], (T*)nullptr), pack2(y[2], y[3], (T*)nullptr));
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = tn_round<T>(y[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { s += y[i]; q += y[i] * y[i]; }
        }
    if (p.part)
        tn_write_partial(s, q, p.part, ((long long)b * gridDim.y * gridDim.x + (long long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave);
}

template <typename T>
__global__ void __launch_bounds__(256) tasnet_depthwise_kernel(const T* __restrict__ x, const float* __restrict__ w3, const float* __restrict__ bias,
                                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ prelu, T* __restrict__ out,
                                                               float* __restrict__ part, int L, int C, int dil) {
    const int b = blockIdx.y, ncg = C / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = idx < (long long)L * ncg;
    float s = 0.f, q = 0.f;
    if (valid) {
        const int l = (int)(idx / ncg), c = (int)(idx % ncg) * 8;
        const float mean = stats[2 * b], rstd = stats[2 * b + 1], slope = prelu[0];
        float sc[8], sh[8], acc[8];
        load8(gamma + c, sc);
        load8(beta + c, sh);
        load8(bias + c, acc);
#pragma unroll
        for (int i = 0; i < 8; ++i) { sc[i] *= rstd; sh[i] -= mean * sc[i]; }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const long long lt = (long long)l + (long long)(t - 1) * dil;
            if (lt < 0 || lt >= L) continue;            // padding of the NORMALISED tensor: the tap adds 0
            float v[8], w[8];
            load8(x + ((long long)b * L + lt) * C + c, v);
            load8(w3 + (long long)t * C + c, w);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(w[i], fmaf(v[i], sc[i], sh[i]), acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = acc[i] >= 0.f ? acc[i] : slope * acc[i];
        store8(out + ((long long)b * L + l) * C + c, acc);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float v = tn_round<T>(acc[i]); s += v; q += v * v; }
    }
    tn_write_partial(s, q, part, ((long long)b * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6));
}

// out[b][t] = sum over the frames l that cover sample t (t - l * stride in [0, win)) and the channels n of
// sigmoid(mask[b][l][n]) * enc[b][l][n] * wd[n][t - l * stride]: frames in rising order, eight channel-interleaved partial sums
template <typename T>
__global__ void __launch_bounds__(256) tasnet_decode_kernel(const T* __restrict__ mask, const T* __restrict__ enc, const float* __restrict__ wd,
                                                            float* __restrict__ out, int L, int N, int win, int stride, long long Tout) {
    const int b = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tout) return;
    long long l_hi = t / stride; if (l_hi > L - 1) l_hi = L - 1;
    const long long l_lo = t - win + 1 <= 0 ? 0 : (t - win + stride) / stride;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long l = l_lo; l <= l_hi; ++l) {
        const int k = (int)(t - l * stride);
        const T* m = mask + ((long long)b * L + l) * N;
        const T* e = enc + ((long long)b * L + l) * N;
        for (int c = 0; c < N; c += 8) {
            float mv[8], ev[8];
            load8(m + c, mv);
            load8(e + c, ev);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(ev[i] / (1.0f + expf(-mv[i])), wd[(long long)(c + i) * win + k], acc[i]);
        }
    }
    out[(long long)b * Tout + t] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

int tasnet_num_partials(int op, int L, int C) {
    if (op == TASNET_OP_POINTWISE) return 4 * cdiv(L, TASNET_PW_ROWS) * cdiv(C, TASNET_PW_COLS);
    return 4 * cdiv((long long)L * (C / 8), 256);
}

int launch_tasnet_encode(const float* wav, long long wav_stride, const float* wT, void* enc, float* part, int B, long long T, int N, int win,
                         int stride, int L, int dtype, hipStream_t st) {
    const dim3 grid(cdiv((long long)L * (N / 8), 256), B);
    if (dtype == STORM_F32) hipLaunchKernelGGL(tasnet_encode_kernel<float>, grid, dim3(256), 0, st, wav, wav_stride, wT, static_cast<float*>(enc), part, T, N, win, stride, L);
    else if (dtype == STORM_BF16) hipLaunchKernelGGL(tasnet_encode_kernel<bf16_t>, grid, dim3(256), 0, st, wav, wav_stride, wT, static_cast<bf16_t*>(enc), part, T, N, win, stride, L);
    else hipLaunchKernelGGL(tasnet_encode_kernel<half_t>, grid, dim3(256), 0, st, wav, wav_stride, wT, static_cast<half_t*>(enc), part, T, N, win, stride, L);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

int launch_tasnet_gln_finalize(const float* part, float* stats, int B, int nparts, long long count, float eps, hipStream_t st) {
    hipLaunchKernelGGL(tasnet_gln_finalize_kernel, dim3(B), dim3(64), 0, st, part, stats, nparts, count, eps);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

int launch_tasnet_pointwise(const TasnetPointwise& p, int B, int dtype, hipStream_t st) {
    const dim3 grid(cdiv(p.L, TASNET_PW_ROWS), cdiv(p.Cout, TASNET_PW_COLS), B);
    if (dtype == STORM_F32) hipLaunchKernelGGL((tasnet_pointwise_kernel<float, false>), grid, dim3(256), 0, st, p);
    else if (dtype == STORM_BF16) {
        if (p.x_f32) hipLaunchKernelGGL((tasnet_pointwise_kernel<bf16_t, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((tasnet_pointwise_kernel<bf16_t, false>), grid, dim3(256), 0, st, p);
    } else {
        if (p.x_f32) hipLaunchKernelGGL((tasnet_pointwise_kernel<half_t, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((tasnet_pointwise_kernel<half_t, false>), grid, dim3(256), 0, st, p);
    }
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

int launch_tasnet_depthwise(const void* x, const float* w3, const float* bias, const float* stats, const float* gamma, const float* beta,
                            const float* prelu, void* out, float* part, int B, int L, int C, int dilation, int dtype, hipStream_t st) {
    const dim3 grid(cdiv((long long)L * (C / 8), 256), B);
    if (dtype == STORM_F32) hipLaunchKernelGGL(tasnet_depthwise_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), w3, bias, stats, gamma, beta, prelu, static_cast<float*>(out), part, L, C, dilation);
    else if (dtype == STORM_BF16) hipLaunchKernelGGL(tasnet_depthwise_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), w3, bias, stats, gamma, beta, prelu, static_cast<bf16_t*>(out), part, L, C, dilation);
    else hipLaunchKernelGGL(tasnet_depthwise_kernel<half_t>, grid, dim3(256), 0, st, static_cast<const half_t*>(x), w3, bias, stats, gamma, beta, prelu, static_cast<half_t*>(out), part, L, C, dilation);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

int launch_tasnet_decode(const void* mask, const void* enc, const float* wd, float* out, int B, int L, int N, int win, int stride, int dtype,
                         hipStream_t st) {
    const long long Tout = (long long)(L - 1) * stride + win;
    const dim3 grid(cdiv(Tout, 256), B);
    if (dtype == STORM_F32) hipLaunchKernelGGL(tasnet_decode_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(mask), static_cast<const float*>(enc), wd, out, L, N, win, stride, Tout);
    else if (dtype == STORM_BF16) hipLaunchKernelGGL(tasnet_decode_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(mask), static_cast<const bf16_t*>(enc), wd, out, L, N, win, stride, Tout);
    else hipLaunchKernelGGL(tasnet_decode_kernel<half_t>, grid, dim3(256), 0, st, static_cast<const half_t*>(mask), static_cast<const half_t*>(enc), wd, out, L, N, win, stride, Tout);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

#endif  // STORM_TASNET_IMPL

}  // namespace storm
