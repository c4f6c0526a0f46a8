// SDE steps of the predictor-corrector sampler on the complex64 state.
// Reference map in include/storm_hip.h.  One fused elementwise kernel per update rule, templated on where row b's
// coefficients come from (Coef: computed in-kernel from t[b] in fp64 and rounded once for OUVE, or read from the caller's
// fp32 tables for any other linear-drift SDE) and on where a generated draw takes its Philox key from (Key: one seed for the
// call, or a key per row); the state update follows the reference's fp32 op order.  Noise is either injected (parity runs)
// or generated in-kernel with Philox4x32-10 + Box-Muller.
#include "common.h"

namespace storm {

// ---- Philox4x32-10 --------------------------------------------------------------------------
__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}
__device__ inline void philox4x32(uint64_t seed, uint64_t idx, uint64_t offset, uint32_t (&c)[4]) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    c[0] = (uint32_t)idx; c[1] = (uint32_t)(idx >> 32); c[2] = (uint32_t)offset; c[3] = (uint32_t)(offset >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) { philox_round(c, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
}
// standard complex normal: re, im ~ N(0, 1/2) independent (torch.randn_like on complex64).  Key = seed (words k0 low, k1 high),
// counter words 0-1 = the element index (low, high), words 2-3 = the offset (low, high); Box-Muller on output words 0 and 1.
__device__ inline float2 complex_normal(uint64_t seed, uint64_t idx, uint64_t offset) {
    uint32_t c[4];
    philox4x32(seed, idx, offset, c);
    // (0,1]: from 2^23 on `+ 0.5f` is a tie that rounds to even, so a top-24-bit value of 0xFFFFFF gives exactly 1.0 - r = 0 (both
    // components +-0) and theta = fl32(2 pi) occur; the smallest value is 2^-25 (|z| = sqrt(25 ln 2), the largest magnitude)
    const float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-logf(u1));                                         // sqrt(-2 ln u / 2)
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    return make_float2(r * cs, r * sn);
}
// Where a generated draw takes its Philox key and counter from.  BatchKey: one seed for the whole call, the counter is the
// element's position in the BATCH (k = b * n + i).  RowKeys: row b has its own key row_seeds[b] and counts from 0 within the
// row, so the row draws what a batch-1 call with seed = row_seeds[b] draws (there b = 0 and k = i) wherever it sits in a batch.
struct BatchKey {
    uint64_t seed;
    __device__ float2 draw(int, long long, long long k, uint64_t offset) const { return complex_normal(seed, (uint64_t)k, offset); }
};
struct RowKeys {
    const uint64_t* row_seeds;                     // device [B]
    __device__ float2 draw(int b, long long i, long long, uint64_t offset) const { return complex_normal(row_seeds[b], (uint64_t)i, offset); }
};
// injected noise z (batch layout) or a generated draw for element i of row b (k = b * n + i)
template <class Key>
__device__ inline float2 get_noise(const float* z, int b, long long i, long long k, Key key, uint64_t offset) {
    return z ? reinterpret_cast<const float2*>(z)[k] : key.draw(b, i, k, offset);
}

// ---- OUVE coefficient helpers (sdes.py:200-231), fp64 then rounded ---------------------------
struct Ouve { double theta, smin, smax, logsig; int N; };
__device__ inline Ouve make_ouve(storm_ouve p) {
    Ouve o; o.theta = p.theta; o.smin = p.sigma_min; o.smax = p.sigma_max; o.logsig = log(o.smax / o.smin); o.N = p.N;
    return o;
}
__device__ inline float ouve_std(const Ouve& o, double t) {
    const double v = o.smin * o.smin * exp(-2.0 * o.theta * t) * (exp(2.0 * (o.theta + o.logsig) * t) - 1.0) * o.logsig /
                     (o.theta + o.logsig);
    return (float)sqrt(v);
}
__device__ inline float ouve_g(const Ouve& o, double t) {
    return (float)(o.smin * pow(o.smax / o.smin, t) * sqrt(2.0 * o.logsig));
}

// Where an update takes row b's coefficients from: a (the drift is a (y - x)), the diffusion g, the perturbation std.  By-value
// kernel arguments like the keys; a kernel evaluates what it needs once per thread, ahead of the element loop.
struct OuveCoef {                                  // derived in-kernel from t[b] (device [B])
    storm_ouve p; const float* t;
    __device__ float a(int) const { return p.theta; }
    __device__ float g(int b) const { return ouve_g(make_ouve(p), (double)t[b]); }
};
struct OuvePriorCoef {                             // the prior is drawn at t = T = 1 whatever the batch
    storm_ouve p;
    __device__ float std(int) const { return ouve_std(make_ouve(p), 1.0); }
};
// coefficient tables (device fp32 [B]; a call hands the ones its kernel reads): any SDE  dx = a(t) (y - x) dt + g(t) dw  (OUVPSDE,
// sdes.py:255-326: a = 1/2 stiffness beta(t), g = sqrt(beta(t))).  The caller evaluates a(t_b), g(t_b), std(t_b) in the reference's
// own fp32 torch expressions; the state update is the same op order for every source (SDE.discretize sdes.py:86-90,
// RSDE.discretize :147-157, rsde_parts :123-145, predictors.py:46-69).
struct TableCoef {
    const float* a_rows; const float* g_rows; const float* std_rows;
    __device__ float a(int b) const { return a_rows[b]; }
    __device__ float g(int b) const { return g_rows[b]; }
    __device__ float std(int b) const { return std_rows[b]; }
};
struct ThetaTableCoef {                            // OUVE's constant drift factor beside a g table (storm_ouve_pf_drift_g)
    float theta; const float* g_rows;
    __device__ float a(int) const { return theta; }
    __device__ float g(int b) const { return g_rows[b]; }
};

// x = y + z * std_b  (OUVESDE.prior_sampling sdes.py:233-237, OUVPSDE.prior_sampling :306-310)
template <class Coef, class Key>
__global__ void prior_kernel(const float* __restrict__ y, const float* __restrict__ z, float* __restrict__ x, long long n,
                             Coef coef, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    const float sd = coef.std(b);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 yy = reinterpret_cast<const float2*>(y)[k];
        const float2 zz = get_noise(z, b, i, k, key, offset);
        reinterpret_cast<float2*>(x)[k] = make_float2(yy.x + zz.x * sd, yy.y + zz.y * sd);
    }
}

template <class Key>
__global__ void ouve_ald_kernel(float* __restrict__ x, float* __restrict__ x_mean, const float* __restrict__ score,
                                const float* __restrict__ z, const float* __restrict__ t, long long n, storm_ouve p,
                                float snr, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    const float std = ouve_std(make_ouve(p), (double)t[b]);
    const float sstd = snr * std;
    const float step = sstd * sstd * 2.0f;                 // correctors.py:87
    const float nscale = sqrtf(step * 2.0f);               // correctors.py:91
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 xx = reinterpret_cast<const float2*>(x)[k];
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        const float2 zz = get_noise(z, b, i, k, key, offset);
        const float2 xm = make_float2(xx.x + step * s.x, xx.y + step * s.y);
        if (x_mean) reinterpret_cast<float2*>(x_mean)[k] = xm;
        reinterpret_cast<float2*>(x)[k] = make_float2(xm.x + zz.x * nscale, xm.y + zz.y * nscale);
    }
}

template <class Coef, class Key>
__global__ void predictor_kernel(float* __restrict__ x, float* __restrict__ x_mean, const float* __restrict__ score,
                                 const float* __restrict__ y, const float* __restrict__ z, long long n, int N, int kind,
                                 int noise_free, Coef coef, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    const float a = coef.a(b), g = coef.g(b);
    const float dt = (float)(1.0 / N);
    const float G = g * sqrtf(dt);            // sdes.py:89 (also g * sqrt(-dt) for euler_maruyama)
    const float G2 = kind == 0 ? G * G : g * g;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 xx = reinterpret_cast<const float2*>(x)[k];
        const float2 yy = reinterpret_cast<const float2*>(y)[k];
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        float2 xm;
        if (kind == 0) {
            // reverse diffusion: f = a (y - x) dt; rev_f = f - G^2 s; x_mean = x - rev_f   (sdes.py:86-90,147-157)
            const float fx = (a * (yy.x - xx.x)) * dt, fy = (a * (yy.y - xx.y)) * dt;
            const float rx = fx - G2 * s.x, ry = fy - G2 * s.y;
            xm = make_float2(xx.x - rx, xx.y - ry);
        } else {
            // Euler-Maruyama: x_mean = x + (a (y - x) - g^2 s) * (-1/N)                    (predictors.py:46-54)
            const float dx = a * (yy.x - xx.x) + (-G2) * s.x, dy = a * (yy.y - xx.y) + (-G2) * s.y;
            xm = make_float2(xx.x + dx * (-dt), xx.y + dy * (-dt));
        }
        if (x_mean) reinterpret_cast<float2*>(x_mean)[k] = xm;
        if (noise_free) {
            reinterpret_cast<float2*>(x)[k] = xm;
        } else {
            const float2 zz = get_noise(z, b, i, k, key, offset);
            reinterpret_cast<float2*>(x)[k] = make_float2(xm.x + G * zz.x, xm.y + G * zz.y);
        }
    }
}

__global__ void batch_l2norm_kernel(const float* __restrict__ v, float* __restrict__ out, long long n2) {
    // one workgroup per batch item; n2 = number of floats per item
    __shared__ double red[4];
    const int b = blockIdx.x;
    const float* p = v + (long long)b * n2;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n2; i += blockDim.x) { const double a = p[i]; acc += a * a; }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[b] = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
}

// mode 0: step from the batch means of the B norms (the reference's semantics for the batch handed to the sampler,
// correctors.py:53-55); mode 1: every row its own step (= B calls with batch 1, what the reference CLI does);
// mode 2: snorm[0] / znorm[0] already hold the means over a LARGER batch (all-reduced over the ranks of a sharded run).
__global__ void langevin_kernel(float* __restrict__ x, float* __restrict__ x_mean, const float* __restrict__ score,
                                const float* __restrict__ z, const float* __restrict__ snorm,
                                const float* __restrict__ znorm, int B, long long n, float snr, int mode) {
    const int b = blockIdx.y;
    float gs, gz;
    if (mode == 1) { gs = snorm[b]; gz = znorm[b]; }
    else if (mode == 2) { gs = snorm[0]; gz = znorm[0]; }
    else {
        gs = 0.f; gz = 0.f;
        for (int i = 0; i < B; ++i) { gs += snorm[i]; gz += znorm[i]; }
        gs /= (float)B; gz /= (float)B;
    }
    const float r = snr * gz / gs;
    const float step = r * r * 2.0f;                       // correctors.py:55
    const float nscale = sqrtf(step * 2.0f);
    const long long base = (long long)b * n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = base + i;
        const float2 xx = reinterpret_cast<const float2*>(x)[k];
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        const float2 zz = reinterpret_cast<const float2*>(z)[k];
        const float2 xm = make_float2(xx.x + step * s.x, xx.y + step * s.y);
        if (x_mean) reinterpret_cast<float2*>(x_mean)[k] = xm;
        reinterpret_cast<float2*>(x)[k] = make_float2(xm.x + zz.x * nscale, xm.y + zz.y * nscale);
    }
}

// z[b][i], n values per row, one row per grid.y (the one-seed form is launched as ONE row holding all the values: k = i there)
template <class Key>
__global__ void complex_randn_kernel(float* __restrict__ z, long long n, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        reinterpret_cast<float2*>(z)[k] = key.draw(b, i, k, offset);
    }
}

// drift of the probability-flow ODE: theta (y - x) - 1/2 g(t)^2 score  (sdes.py:92-121 with probability_flow=True, :203-207)
__global__ void ouve_pf_drift_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ y,
                                     const float* __restrict__ score, const float* __restrict__ t, long long n, storm_ouve p) {
    const int b = blockIdx.y;
    const Ouve o = make_ouve(p);
    const float g = ouve_g(o, (double)t[b]);
    const float hg2 = 0.5f * g * g;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 xx = reinterpret_cast<const float2*>(x)[k];
        const float2 yy = reinterpret_cast<const float2*>(y)[k];
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        reinterpret_cast<float2*>(out)[k] = make_float2(p.theta * (yy.x - xx.x) - hg2 * s.x, p.theta * (yy.y - xx.y) - hg2 * s.y);
    }
}

// the same with the coefficients handed in per row (fp32 [B]): the ODE sampler evaluates g - for OUVE sigma_min (sigma_max /
// sigma_min)^t sqrt(2 logsig) - with the reference's own fp32 torch ops on the host (sdes.py:203-207), so the right-hand side
// is the reference's to the last bit - at rtol = atol = 1e-5 the first steps' error estimates sit at the fp32 noise floor and
// an ulp in g changes which steps RK45 accepts.  (The t form above rounds differently: theta d - (1/2 g^2) s.)
template <class Coef>
__global__ void pf_drift_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ y,
                                const float* __restrict__ score, long long n, Coef coef) {
    const int b = blockIdx.y;
    const float a = coef.a(b), g = coef.g(b);
    const float g2 = g * g;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 xx = reinterpret_cast<const float2*>(x)[k];
        const float2 yy = reinterpret_cast<const float2*>(y)[k];
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        // sde_drift + (-(g^2) * score * 0.5)  in the reference's operation order (sdes.py:129-134)
        reinterpret_cast<float2*>(out)[k] = make_float2(a * (yy.x - xx.x) + (-g2 * s.x) * 0.5f, a * (yy.y - xx.y) + (-g2 * s.y) * 0.5f);
    }
}

// ---- probability-flow ODE (Dormand-Prince RK45, sampling/__init__.py:71-141 runs scipy's on the host) ----------------
// out = x + h * sum_j coef[j] * K[j]  over n floats (one fused pass per stage instead of one pass per term)
struct RkTerms { const float* k[7]; float c[7]; int n; };
__global__ void rk_combine_kernel(float* __restrict__ out, const float* __restrict__ x, RkTerms t, float h, long long n4) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (j < t.n) {
                const float4 k = reinterpret_cast<const float4*>(t.k[j])[i];
                a.x = fmaf(t.c[j], k.x, a.x); a.y = fmaf(t.c[j], k.y, a.y); a.z = fmaf(t.c[j], k.z, a.z); a.w = fmaf(t.c[j], k.w, a.w);
            }
        const float4 xx = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(fmaf(h, a.x, xx.x), fmaf(h, a.y, xx.y), fmaf(h, a.z, xx.z), fmaf(h, a.w, xx.w));
    }
}
// per-block partial of sum_c |v_c|^2 / (atol + max(|xa_c|, |xb_c|) rtol)^2 over complex elements c, where
// v = h * sum_j coef[j] K[j] (t.n > 0) or v = K[0] - K[1] (t.n == -2) or v = K[0] (t.n == -1): scipy's scaled RMS norms
__global__ void rk_scaled_sumsq_kernel(double* __restrict__ part, const float* __restrict__ xa, const float* __restrict__ xb,
                                       RkTerms t, float h, float atol, float rtol, long long nc) {
    __shared__ double red[4];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += (long long)gridDim.x * blockDim.x) {
        float2 v = make_float2(0.f, 0.f);
        if (t.n > 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < t.n) { const float2 k = reinterpret_cast<const float2*>(t.k[j])[i]; v.x = fmaf(t.c[j], k.x, v.x); v.y = fmaf(t.c[j], k.y, v.y); }
            v.x *= h; v.y *= h;
        } else {
            v = reinterpret_cast<const float2*>(t.k[0])[i];
            if (t.n == -2) { const float2 w = reinterpret_cast<const float2*>(t.k[1])[i]; v.x -= w.x; v.y -= w.y; }
        }
        const float2 a = reinterpret_cast<const float2*>(xa)[i];
        float m = sqrtf(a.x * a.x + a.y * a.y);
        if (xb) { const float2 b = reinterpret_cast<const float2*>(xb)[i]; m = fmaxf(m, sqrtf(b.x * b.x + b.y * b.y)); }
        const double sc = (double)atol + (double)m * (double)rtol;
        acc += ((double)v.x * v.x + (double)v.y * v.y) / (sc * sc);
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void sum_partials_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {   // fixed order: deterministic
    if (threadIdx.x == 0 && blockIdx.x == 0) { double s = 0.0; for (int i = 0; i < n; ++i) s += part[i]; out[0] = s; }
}

// ---- per-row forms: B independent utterances advance with their OWN step sizes (the reference integrates one utterance per
// solve_ivp call, model.py:224-244 minibatch = 1, so every utterance has its own accepted / rejected step sequence).  scipy
// keeps the solver state in complex128 (it up-casts the complex64 state it is handed and only the right-hand side runs in
// fp32, sampling/__init__.py:119-123): the state x is fp64 here too, the stages K are the fp32 network outputs, and the
// algebra is fp64 - the accept / reject decisions then follow scipy's to rounding noise of 1e-16, not 1e-7.
// MAXT stages and NE coefficient rows over them (7 x 1: the storm_rk_*_rows entry points; STORM_RK_MAX_TERMS x 1 / x 2: the wide forms)
template <int MAXT, int NE> struct RkTermsN { const float* k[MAXT]; double c[NE][MAXT]; int n; };
using RkTermsD = RkTermsN<7, 1>;
struct alignas(16) Cplx128 { double x, y; };
struct RkRows { double h[STORM_RK_MAX_ROWS]; };
template <int V> using RkFloats = float __attribute__((ext_vector_type(2 * V)));   // V complex64: one 8- or 16-byte access
// a[e][..] = sum_j c[e][j] K_j over the V complex elements from `at`, fp64, the terms in index order: the ONE body of every width,
// so a sum over n terms is the same bits whichever entry point formed it.  Every stage is read once, for all NE rows.
template <int MAXT, int NE, int V>
__device__ __forceinline__ void rk_stage_sums(const RkTermsN<MAXT, NE>& t, long long at, double (&a)[NE][2 * V]) {
#pragma unroll
    for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int q = 0; q < 2 * V; ++q) a[e][q] = 0.0;
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
        if (j < t.n) {
            const RkFloats<V> k = *reinterpret_cast<const RkFloats<V>*>(t.k[j] + 2 * at);
#pragma unroll
            for (int e = 0; e < NE; ++e)
#pragma unroll
                for (int q = 0; q < 2 * V; ++q) a[e][q] = fma(t.c[e][j], (double)k[q], a[e][q]);
        }
}
// out64 = x + h_b * sum_j c_j K_j (complex128, may be NULL); out32 = the same rounded to complex64 (the next network input).
// A thread takes V complex elements at a time (V = 2: 16-byte stage reads; rows of an even length on 16-byte aligned pointers only).
template <int MAXT, int V>
__global__ void rk_combine_rows_kernel(double* __restrict__ out64, float* __restrict__ out32, const double* __restrict__ x,
                                       RkTermsN<MAXT, 1> t, RkRows hr, long long n2) {
    const int b = blockIdx.y;
    const double h = hr.h[b];
    const long long base = (long long)b * n2, nv = n2 / V;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        const long long at = base + i * V;
        double a[1][2 * V];
        rk_stage_sums<MAXT, 1, V>(t, at, a);
        RkFloats<V> o32;
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const Cplx128 xx = reinterpret_cast<const Cplx128*>(x)[at + q];
            const double ox = fma(h, a[0][2 * q], xx.x), oy = fma(h, a[0][2 * q + 1], xx.y);
            if (out64) reinterpret_cast<Cplx128*>(out64)[at + q] = Cplx128{ox, oy};
            o32[2 * q] = (float)ox; o32[2 * q + 1] = (float)oy;
        }
        if (out32) *reinterpret_cast<RkFloats<V>*>(out32 + 2 * at) = o32;
    }
}
// part[e][b][block] = that block's share of row b's scaled sum of squares: sum_c |v_c|^2 / (atol + max(|xa_c|, |xb_c|) rtol)^2 with
// v = h_b * sum_j c[e][j] K_j (t.n > 0; NE = 2: both error estimators of DOP853 in one pass over the stages), K[0] - K[1]
// (t.n == -2), K[0] (t.n == -1) or xa itself (t.n == -3; the three NE = 1 only).  The block count per row depends on the row
// length only, so a row's sum is the same number whatever batch it sits in.
template <int MAXT, int NE>
__global__ void rk_scaled_sumsq_rows_kernel(double* __restrict__ part, const double* __restrict__ xa, const double* __restrict__ xb,
                                            RkTermsN<MAXT, NE> t, RkRows hr, double atol, double rtol, long long nc) {
    __shared__ double red[NE][4];
    const int b = blockIdx.y;
    const double h = hr.h[b];
    const long long base = (long long)b * nc;
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += (long long)gridDim.x * blockDim.x) {
        const Cplx128 a = reinterpret_cast<const Cplx128*>(xa)[base + i];
        double v[NE][2];
        if (t.n > 0) {
            rk_stage_sums<MAXT, NE, 1>(t, base + i, v);
#pragma unroll
            for (int e = 0; e < NE; ++e) { v[e][0] *= h; v[e][1] *= h; }
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e) v[e][0] = v[e][1] = 0.0;
            if (t.n == -3) {
                v[0][0] = a.x; v[0][1] = a.y;
            } else {
                const float2 k = reinterpret_cast<const float2*>(t.k[0])[base + i];
                v[0][0] = k.x; v[0][1] = k.y;
                if (t.n == -2) { const float2 w = reinterpret_cast<const float2*>(t.k[1])[base + i]; v[0][0] -= (double)w.x; v[0][1] -= (double)w.y; }
            }
        }
        double m = sqrt(a.x * a.x + a.y * a.y);
        if (xb) { const Cplx128 q = reinterpret_cast<const Cplx128*>(xb)[base + i]; m = fmax(m, sqrt(q.x * q.x + q.y * q.y)); }
        const double sc = atol + m * rtol;
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] += (v[e][0] * v[e][0] + v[e][1] * v[e][1]) / (sc * sc);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const double w = wave_sum_d(acc[e]);
        if ((threadIdx.x & 63) == 0) red[e][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int e = 0; e < NE; ++e)
            part[((long long)e * gridDim.y + b) * gridDim.x + blockIdx.x] = red[e][0] + red[e][1] + red[e][2] + red[e][3];
}
__global__ void sum_rows_kernel(const double* __restrict__ part, int n, int B, double* __restrict__ out) {   // one thread per row, fixed order
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { double s = 0.0; for (int i = 0; i < n; ++i) s += part[(long long)b * n + i]; out[b] = s; }
}

// SI-SDR of B (reference, estimate) waveform pairs (util/other.py:82-94): alpha = <s_hat, s> / ||s||^2,
// 10 log10((eps +) ||alpha s||^2 / (eps + ||alpha s - s_hat||^2)); sums in fp64, the residual formed per sample.
__global__ void si_sdr_kernel(const float* __restrict__ s, const float* __restrict__ sh, float* __restrict__ out, long long n,
                              long long stride_s, long long stride_h, float eps) {
    __shared__ double red[2][4];
    __shared__ double alpha_sh;
    const int b = blockIdx.x;
    const float* ps = s + (long long)b * stride_s;
    const float* ph = sh + (long long)b * stride_h;
    double dot = 0.0, ss = 0.0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) { const double a = ps[i]; dot += a * (double)ph[i]; ss += a * a; }
    dot = wave_sum_d(dot); ss = wave_sum_d(ss);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = dot; red[1][threadIdx.x >> 6] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) alpha_sh = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    __syncthreads();
    const double alpha = alpha_sh;
    double tgt = 0.0, res = 0.0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = alpha * (double)ps[i], r = a - (double)ph[i];
        tgt += a * a; res += r * r;
    }
    tgt = wave_sum_d(tgt); res = wave_sum_d(res);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = tgt; red[1][threadIdx.x >> 6] = res; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double T = red[0][0] + red[0][1] + red[0][2] + red[0][3], R = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        out[b] = (float)(10.0 * log10((double)eps + T / ((double)eps + R)));
    }
}

// ---- validation loss: forward diffusion and the denoising-score-matching residual (model.py:138-154, 560-595) ----------------
// x_t = mean_b(x0, y) + std_b z on the complex64 state in one pass, no `mean` tensor.  m_rows / std_rows: the mean factor and the
// perturbation std at t_b, device fp32 [B], the SDE's own torch expressions (sdes.py:210-231, 296-306).  The mean in the two
// operation orders of the reference: FORM 0 (OUVESDE._mean, sdes.py:210-213)  m x0 + (1 - m) y, 1 - m formed in fp32 here;
// FORM 1 (OUVPSDE._mean, sdes.py:296-299)  y + m (x0 - y).
template <int FORM, class Key>
__global__ void perturb_kernel(const float* __restrict__ x0, const float* __restrict__ y, const float* __restrict__ z,
                               float* __restrict__ xt, long long n, const float* __restrict__ m_rows,
                               const float* __restrict__ std_rows, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    const float m = m_rows[b], sd = std_rows[b];
    const float om = 1.0f - m;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long k = (long long)b * n + i;
        const float2 xx = reinterpret_cast<const float2*>(x0)[k];
        const float2 yy = reinterpret_cast<const float2*>(y)[k];
        const float2 zz = get_noise(z, b, i, k, key, offset);
        float2 mean;
        if (FORM == 0) mean = make_float2(m * xx.x + om * yy.x, m * xx.y + om * yy.y);
        else mean = make_float2(yy.x + m * (xx.x - yy.x), yy.y + m * (xx.y - yy.y));
        reinterpret_cast<float2*>(xt)[k] = make_float2(mean.x + sd * zz.x, mean.y + sd * zz.y);      // model.py:150
    }
}

// One block's share of a row's loss sum -> part[b][block] (fp64); loss_rows_finish_kernel adds a row's shares in a fixed order.
// The block count per row depends on the row length only and nothing is atomic, so a row's sum is the same number in every run and
// in whatever batch the row sits (as rk_scaled_sumsq_rows_kernel).
__device__ inline void loss_block_partial(double acc, double* __restrict__ part) {
    __shared__ double red[4];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// err = score std_b + z in fp32 (model.py:152); rho = |err|^2 (kind 0, `mse`) or |err| (kind 1, `mae`) and the sum in fp64
// (model.py:113-122, 468-470).  z is the injected tensor or the draw of (key, offset) - the one perturb_kernel made, never stored.
// row_frames: row b counts the elements whose frame i % T lies below row_frames[b] (NULL: all).
template <class Key>
__global__ void dsm_loss_kernel(double* __restrict__ part, const float* __restrict__ score, const float* __restrict__ z,
                                const float* __restrict__ std_rows, const int* __restrict__ row_frames, long long n, int T,
                                int kind, Key key, uint64_t offset) {
    const int b = blockIdx.y;
    const float sd = std_rows[b];
    const int frames = row_frames ? row_frames[b] : 0;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (row_frames && (int)(i % T) >= frames) continue;
        const long long k = (long long)b * n + i;
        const float2 s = reinterpret_cast<const float2*>(score)[k];
        const float2 zz = get_noise(z, b, i, k, key, offset);
        const float ex = s.x * sd + zz.x, ey = s.y * sd + zz.y;
        const double r2 = (double)ex * (double)ex + (double)ey * (double)ey;
        acc += kind == 0 ? r2 : sqrt(r2);
    }
    loss_block_partial(acc, part);
}
// the predictive models' losses (model.py:329-343, 479-481), d = a - b in fp32: kind 0 sum d^2 over the n floats of a row (a complex
// spectrogram through its float view, or a real waveform); kind 1 sum |d| over n complex elements; kind 2 sum |d| over n real samples.
// With row_frames a row of kind 0 / 1 is complex (kind 0: n even) and counts the frames below row_frames[b] only.
__global__ void pair_loss_kernel(double* __restrict__ part, const float* __restrict__ a, const float* __restrict__ b_,
                                 const int* __restrict__ row_frames, long long n, int T, int kind) {
    const int b = blockIdx.y;
    const int frames = row_frames ? row_frames[b] : 0;
    const bool cplx = kind == 1 || (kind == 0 && row_frames);
    const long long ne = (kind == 0 && row_frames) ? n / 2 : n;          // elements of the row the loop walks
    const long long base = (long long)b * ne;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += (long long)gridDim.x * blockDim.x) {
        if (cplx) {
            if (row_frames && (int)(i % T) >= frames) continue;
            const float2 p = reinterpret_cast<const float2*>(a)[base + i], q = reinterpret_cast<const float2*>(b_)[base + i];
            const float dx = p.x - q.x, dy = p.y - q.y;
            const double r2 = (double)dx * (double)dx + (double)dy * (double)dy;
            acc += kind == 0 ? r2 : sqrt(r2);
        } else {
            const float d = a[base + i] - b_[base + i];
            acc += kind == 0 ? (double)d * (double)d : fabs((double)d);
        }
    }
    loss_block_partial(acc, part);
}
__global__ void loss_rows_finish_kernel(const double* __restrict__ part, int nb, int B, float* __restrict__ out) {   // one thread per row, fixed order
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { double s = 0.0; for (int i = 0; i < nb; ++i) s += part[(long long)b * nb + i]; out[b] = (float)(0.5 * s); }
}

static inline int ew_blocks(long long n) { long long b = (n + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }
// blocks per row of the loss reductions: a function of the row length ONLY
static inline int loss_blocks(long long n) { const int b = ew_blocks(n); return b > STORM_RK_ROW_BLOCKS ? STORM_RK_ROW_BLOCKS : b; }

}  // namespace storm

using namespace storm;

// One launch for the "B rows x n elements" kernels: grid.y is the row, grid.x strides over the row's elements.
template <class... P, class... A>
static int launch_rows(void (*kernel)(P...), int B, long long n, storm_stream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3(ew_blocks(n), B), dim3(256), 0, (hipStream_t)s, args...);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

// Every entry point that can generate noise exists twice - one seed for the call (BatchKey) or a key per row (RowKeys, the *_rs
// names; their `seed` argument is not read): its checks, then the update's ONE kernel with the coefficient source and the key chosen.
extern "C" int storm_ouve_prior(const float* y, const float* z, float* x, int B, long long n, storm_ouve p,
                                uint64_t seed, uint64_t offset, storm_stream_t s) {
    STORM_CHECK(y && x && B > 0 && n > 0, "storm_ouve_prior: bad arguments");
    return launch_rows(prior_kernel<OuvePriorCoef, BatchKey>, B, n, s, y, z, x, n, OuvePriorCoef{p}, BatchKey{seed}, offset);
}
extern "C" int storm_ouve_prior_rs(const float* y, const float* z, float* x, int B, long long n, storm_ouve p,
                                   uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_ouve_prior_rs: null row_seeds");
    STORM_CHECK(y && x && B > 0 && n > 0, "storm_ouve_prior_rs: bad arguments");
    return launch_rows(prior_kernel<OuvePriorCoef, RowKeys>, B, n, s, y, z, x, n, OuvePriorCoef{p}, RowKeys{row_seeds}, offset);
}

extern "C" int storm_ouve_ald_step(float* x, float* x_mean, const float* score, const float* z, const float* t, int B,
                                   long long n, storm_ouve p, float snr, uint64_t seed, uint64_t offset,
                                   storm_stream_t s) {
    STORM_CHECK(x && score && t && B > 0 && n > 0, "storm_ouve_ald_step: bad arguments");
    return launch_rows(ouve_ald_kernel<BatchKey>, B, n, s, x, x_mean, score, z, t, n, p, snr, BatchKey{seed}, offset);
}
extern "C" int storm_ouve_ald_step_rs(float* x, float* x_mean, const float* score, const float* z, const float* t, int B,
                                      long long n, storm_ouve p, float snr, uint64_t seed, uint64_t offset,
                                      const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_ouve_ald_step_rs: null row_seeds");
    STORM_CHECK(x && score && t && B > 0 && n > 0, "storm_ouve_ald_step_rs: bad arguments");
    return launch_rows(ouve_ald_kernel<RowKeys>, B, n, s, x, x_mean, score, z, t, n, p, snr, RowKeys{row_seeds}, offset);
}

extern "C" int storm_ouve_predictor_step(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                         const float* t, int B, long long n, storm_ouve p, int kind, int noise_free,
                                         uint64_t seed, uint64_t offset, storm_stream_t s) {
    STORM_CHECK(x && score && y && t && B > 0 && n > 0 && p.N > 0, "storm_ouve_predictor_step: bad arguments");
    STORM_CHECK(kind == 0 || kind == 1, "storm_ouve_predictor_step: kind=%d", kind);
    return launch_rows(predictor_kernel<OuveCoef, BatchKey>, B, n, s, x, x_mean, score, y, z, n, p.N, kind, noise_free, OuveCoef{p, t},
                       BatchKey{seed}, offset);
}
extern "C" int storm_ouve_predictor_step_rs(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                            const float* t, int B, long long n, storm_ouve p, int kind, int noise_free,
                                            uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_ouve_predictor_step_rs: null row_seeds");
    STORM_CHECK(x && score && y && t && B > 0 && n > 0 && p.N > 0, "storm_ouve_predictor_step_rs: bad arguments");
    STORM_CHECK(kind == 0 || kind == 1, "storm_ouve_predictor_step_rs: kind=%d", kind);
    return launch_rows(predictor_kernel<OuveCoef, RowKeys>, B, n, s, x, x_mean, score, y, z, n, p.N, kind, noise_free, OuveCoef{p, t},
                       RowKeys{row_seeds}, offset);
}

extern "C" int storm_batch_l2norm(const float* v, float* out, int B, long long n, storm_stream_t s) {
    STORM_CHECK(v && out && B > 0 && n > 0, "storm_batch_l2norm: bad arguments");
    hipLaunchKernelGGL(batch_l2norm_kernel, dim3(B), dim3(256), 0, (hipStream_t)s, v, out, 2 * n);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_langevin_step(float* x, float* x_mean, const float* score, const float* z, const float* score_norms,
                                   const float* z_norms, int B, long long n, float snr, int mode, storm_stream_t s) {
    STORM_CHECK(x && score && z && score_norms && z_norms && B > 0 && n > 0, "storm_langevin_step: bad arguments");
    STORM_CHECK(mode >= 0 && mode <= 2, "storm_langevin_step: mode=%d", mode);
    return launch_rows(langevin_kernel, B, n, s, x, x_mean, score, z, score_norms, z_norms, B, n, snr, mode);
}

extern "C" int storm_complex_randn(float* z, long long n_complex, uint64_t seed, uint64_t offset, storm_stream_t s) {
    STORM_CHECK(z && n_complex > 0, "storm_complex_randn: bad arguments");
    return launch_rows(complex_randn_kernel<BatchKey>, 1, n_complex, s, z, n_complex, BatchKey{seed}, offset);
}
extern "C" int storm_complex_randn_rs(float* z, int B, long long n_per_row, uint64_t seed, uint64_t offset,
                                      const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(z && B > 0 && n_per_row > 0 && row_seeds, "storm_complex_randn_rs: bad arguments");
    return launch_rows(complex_randn_kernel<RowKeys>, B, n_per_row, s, z, n_per_row, RowKeys{row_seeds}, offset);
}

static int fill_terms(RkTerms& t, const float* const* K, const float* coef, int n_terms) {
    STORM_CHECK(K && n_terms >= -2 && n_terms <= 7 && n_terms != 0, "storm_rk: n_terms=%d", n_terms);
    const int np = n_terms > 0 ? n_terms : -n_terms;
    STORM_CHECK(n_terms < 0 || coef, "storm_rk: null coefficients");
    for (int j = 0; j < 7; ++j) { t.k[j] = j < np ? K[j] : nullptr; t.c[j] = (n_terms > 0 && j < np) ? coef[j] : 0.f; }
    for (int j = 0; j < np; ++j) STORM_CHECK(K[j] != nullptr, "storm_rk: null stage %d", j);
    t.n = n_terms;
    return STORM_OK;
}

extern "C" int storm_rk_combine(float* out, const float* x, const float* const* K, const float* coef, int n_terms, float h,
                                long long n_complex, storm_stream_t s) {
    STORM_CHECK(out && x && n_complex > 0 && n_complex % 2 == 0 && n_terms > 0, "storm_rk_combine: bad arguments");
    RkTerms t;
    if (int rc = fill_terms(t, K, coef, n_terms)) return rc;
    hipLaunchKernelGGL(rk_combine_kernel, dim3(ew_blocks(n_complex / 2)), dim3(256), 0, (hipStream_t)s, out, x, t, h, n_complex / 2);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_rk_scaled_sumsq(double* out, double* scratch, int scratch_len, const float* xa, const float* xb,
                                     const float* const* K, const float* coef, int n_terms, float h, float atol, float rtol,
                                     long long n_complex, storm_stream_t s) {
    STORM_CHECK(out && scratch && xa && n_complex > 0 && scratch_len >= 1, "storm_rk_scaled_sumsq: bad arguments");
    RkTerms t;
    if (int rc = fill_terms(t, K, coef, n_terms)) return rc;
    int nb = ew_blocks(n_complex);
    if (nb > scratch_len) nb = scratch_len;
    hipLaunchKernelGGL(rk_scaled_sumsq_kernel, dim3(nb), dim3(256), 0, (hipStream_t)s, scratch, xa, xb, t, h, atol, rtol, n_complex);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, scratch, nb, out);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

static int fill_rows(RkRows& r, const double* h_rows, int B) {
    STORM_CHECK(B > 0 && B <= STORM_RK_MAX_ROWS, "storm_rk rows: B=%d outside 1..%d", B, STORM_RK_MAX_ROWS);
    for (int b = 0; b < STORM_RK_MAX_ROWS; ++b) r.h[b] = (b < B && h_rows) ? h_rows[b] : (h_rows ? 0.0 : 1.0);
    return STORM_OK;
}
static int fill_terms_d(RkTermsD& t, const float* const* K, const double* coef, int n_terms) {
    STORM_CHECK(n_terms >= -3 && n_terms <= 7 && n_terms != 0, "storm_rk rows: n_terms=%d", n_terms);
    const int np = n_terms > 0 ? n_terms : (n_terms == -3 ? 0 : -n_terms);
    STORM_CHECK(np == 0 || K, "storm_rk rows: null stage list");
    STORM_CHECK(n_terms < 0 || coef, "storm_rk rows: null coefficients");
    for (int j = 0; j < 7; ++j) { t.k[j] = j < np ? K[j] : nullptr; t.c[0][j] = (n_terms > 0 && j < np) ? coef[j] : 0.0; }
    for (int j = 0; j < np; ++j) STORM_CHECK(K[j] != nullptr, "storm_rk rows: null stage %d", j);
    t.n = n_terms;
    return STORM_OK;
}

extern "C" int storm_rk_combine_rows(double* out64, float* out32, const double* x, const float* const* K, const double* coef,
                                     int n_terms, const double* h_rows, int B, long long n_complex_row, storm_stream_t s) {
    STORM_CHECK((out64 || out32) && x && n_complex_row > 0 && n_terms > 0 && h_rows, "storm_rk_combine_rows: bad arguments");
    RkTermsD t; RkRows r;
    if (int rc = fill_terms_d(t, K, coef, n_terms)) return rc;
    if (int rc = fill_rows(r, h_rows, B)) return rc;
    return launch_rows(rk_combine_rows_kernel<7, 1>, B, n_complex_row, s, out64, out32, x, t, r, n_complex_row);
}

extern "C" int storm_rk_scaled_sumsq_rows(double* out, double* scratch, long long scratch_len, const double* xa, const double* xb,
                                          const float* const* K, const double* coef, int n_terms, const double* h_rows, double atol,
                                          double rtol, int B, long long n_complex_row, storm_stream_t s) {
    STORM_CHECK(out && scratch && xa && n_complex_row > 0, "storm_rk_scaled_sumsq_rows: bad arguments");
    RkTermsD t; RkRows r;
    if (int rc = fill_terms_d(t, K, coef, n_terms)) return rc;
    if (int rc = fill_rows(r, h_rows, B)) return rc;
    int nb = ew_blocks(n_complex_row);
    if (nb > STORM_RK_ROW_BLOCKS) nb = STORM_RK_ROW_BLOCKS;           // a function of the row length ONLY (see the kernel)
    STORM_CHECK(scratch_len >= (long long)nb * B, "storm_rk_scaled_sumsq_rows: scratch of %lld doubles < %lld", scratch_len, (long long)nb * B);
    hipLaunchKernelGGL((rk_scaled_sumsq_rows_kernel<7, 1>), dim3(nb, B), dim3(256), 0, (hipStream_t)s, scratch, xa, xb, t, r, atol, rtol, n_complex_row);
    hipLaunchKernelGGL(sum_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)s, scratch, nb, B, out);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

// ---- the wide forms: up to STORM_RK_MAX_TERMS stages (DOP853: 12 in a stage, 13 in its two error estimators) ----
using RkTermsWide = RkTermsN<STORM_RK_MAX_TERMS, 1>;
using RkTermsPair = RkTermsN<STORM_RK_MAX_TERMS, 2>;
template <int NE>
static int fill_terms_wide(RkTermsN<STORM_RK_MAX_TERMS, NE>& t, const float* const* K, const double* const (&coef)[NE], int n_terms) {
    STORM_CHECK(n_terms >= 1 && n_terms <= STORM_RK_MAX_TERMS, "storm_rk wide: n_terms=%d outside 1..%d", n_terms, STORM_RK_MAX_TERMS);
    STORM_CHECK(K, "storm_rk wide: null stage list");
    for (int e = 0; e < NE; ++e) STORM_CHECK(coef[e], "storm_rk wide: null coefficients");
    for (int j = 0; j < STORM_RK_MAX_TERMS; ++j) {
        t.k[j] = j < n_terms ? K[j] : nullptr;
        for (int e = 0; e < NE; ++e) t.c[e][j] = j < n_terms ? coef[e][j] : 0.0;
    }
    for (int j = 0; j < n_terms; ++j) STORM_CHECK(K[j] != nullptr, "storm_rk wide: null stage %d", j);
    t.n = n_terms;
    return STORM_OK;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int storm_rk_combine_rows_wide(double* out64, float* out32, const double* x, const float* const* K, const double* coef,
                                          int n_terms, const double* h_rows, int B, long long n_complex_row, storm_stream_t s) {
    STORM_CHECK((out64 || out32) && x && n_complex_row > 0 && h_rows, "storm_rk_combine_rows_wide: bad arguments");
    RkTermsWide t; RkRows r;
    const double* const cf[1] = {coef};
    if (int rc = fill_terms_wide<1>(t, K, cf, n_terms)) return rc;
    if (int rc = fill_rows(r, h_rows, B)) return rc;
    // two complex elements per thread where every row starts on a 16-byte boundary (complex128 always does)
    bool pair = n_complex_row % 2 == 0 && (!out32 || aligned16(out32));
    for (int j = 0; j < n_terms; ++j) pair = pair && aligned16(K[j]);
    if (pair)
        return launch_rows(rk_combine_rows_kernel<STORM_RK_MAX_TERMS, 2>, B, n_complex_row / 2, s, out64, out32, x, t, r, n_complex_row);
    return launch_rows(rk_combine_rows_kernel<STORM_RK_MAX_TERMS, 1>, B, n_complex_row, s, out64, out32, x, t, r, n_complex_row);
}

extern "C" int storm_rk_error_pair_rows(double* out, double* scratch, long long scratch_len, const double* xa, const double* xb,
                                        const float* const* K, const double* coef_a, const double* coef_b, int n_terms,
                                        const double* h_rows, double atol, double rtol, int B, long long n_complex_row, storm_stream_t s) {
    STORM_CHECK(out && scratch && xa && n_complex_row > 0, "storm_rk_error_pair_rows: bad arguments");
    RkTermsPair t; RkRows r;
    const double* const cf[2] = {coef_a, coef_b};
    if (int rc = fill_terms_wide<2>(t, K, cf, n_terms)) return rc;
    if (int rc = fill_rows(r, h_rows, B)) return rc;
    int nb = ew_blocks(n_complex_row);
    if (nb > STORM_RK_ROW_BLOCKS) nb = STORM_RK_ROW_BLOCKS;           // the geometry of storm_rk_scaled_sumsq_rows: the row length ONLY
    STORM_CHECK(scratch_len >= 2LL * nb * B, "storm_rk_error_pair_rows: scratch of %lld doubles < %lld", scratch_len, 2LL * nb * B);
    hipLaunchKernelGGL((rk_scaled_sumsq_rows_kernel<STORM_RK_MAX_TERMS, 2>), dim3(nb, B), dim3(256), 0, (hipStream_t)s, scratch, xa, xb, t, r,
                       atol, rtol, n_complex_row);
    hipLaunchKernelGGL(sum_rows_kernel, dim3((2 * B + 63) / 64), dim3(64), 0, (hipStream_t)s, scratch, nb, 2 * B, out);   // out[e * B + b]
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

extern "C" int storm_copy_rows(void* dst, const void* src, const int* row_mask, int B, long long row_bytes, storm_stream_t s) {
    STORM_CHECK(dst && src && row_mask && B > 0 && row_bytes > 0, "storm_copy_rows: bad arguments");
    for (int b = 0; b < B; ) {                                        // one device-to-device copy per run of selected rows
        if (!row_mask[b]) { ++b; continue; }
        int e = b;
        while (e < B && row_mask[e]) ++e;
        STORM_HIP(hipMemcpyAsync(static_cast<char*>(dst) + (long long)b * row_bytes, static_cast<const char*>(src) + (long long)b * row_bytes,
                                 (size_t)((long long)(e - b) * row_bytes), hipMemcpyDeviceToDevice, (hipStream_t)s));
        b = e;
    }
    return STORM_OK;
}

extern "C" int storm_ouve_pf_drift(float* out, const float* x, const float* y, const float* score, const float* t, int B,
                                   long long n, storm_ouve p, storm_stream_t s) {
    STORM_CHECK(out && x && y && score && t && B > 0 && n > 0, "storm_ouve_pf_drift: bad arguments");
    return launch_rows(ouve_pf_drift_kernel, B, n, s, out, x, y, score, t, n, p);
}

extern "C" int storm_ouve_pf_drift_g(float* out, const float* x, const float* y, const float* score, const float* g_rows, int B,
                                     long long n, float theta, storm_stream_t s) {
    STORM_CHECK(out && x && y && score && g_rows && B > 0 && n > 0, "storm_ouve_pf_drift_g: bad arguments");
    return launch_rows(pf_drift_kernel<ThetaTableCoef>, B, n, s, out, x, y, score, n, ThetaTableCoef{theta, g_rows});
}

extern "C" int storm_sde_prior_rows(const float* y, const float* z, float* x, const float* std_rows, int B, long long n,
                                    uint64_t seed, uint64_t offset, storm_stream_t s) {
    STORM_CHECK(y && x && std_rows && B > 0 && n > 0, "storm_sde_prior_rows: bad arguments");
    return launch_rows(prior_kernel<TableCoef, BatchKey>, B, n, s, y, z, x, n, TableCoef{nullptr, nullptr, std_rows}, BatchKey{seed}, offset);
}
extern "C" int storm_sde_prior_rows_rs(const float* y, const float* z, float* x, const float* std_rows, int B, long long n,
                                       uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_sde_prior_rows_rs: null row_seeds");
    STORM_CHECK(y && x && std_rows && B > 0 && n > 0, "storm_sde_prior_rows_rs: bad arguments");
    return launch_rows(prior_kernel<TableCoef, RowKeys>, B, n, s, y, z, x, n, TableCoef{nullptr, nullptr, std_rows}, RowKeys{row_seeds}, offset);
}

extern "C" int storm_sde_predictor_step_rows(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                             const float* a_rows, const float* g_rows, int B, long long n, int N, int kind,
                                             int noise_free, uint64_t seed, uint64_t offset, storm_stream_t s) {
    STORM_CHECK(x && score && y && a_rows && g_rows && B > 0 && n > 0 && N > 0, "storm_sde_predictor_step_rows: bad arguments");
    STORM_CHECK(kind == 0 || kind == 1, "storm_sde_predictor_step_rows: kind=%d", kind);
    return launch_rows(predictor_kernel<TableCoef, BatchKey>, B, n, s, x, x_mean, score, y, z, n, N, kind, noise_free,
                       TableCoef{a_rows, g_rows, nullptr}, BatchKey{seed}, offset);
}
extern "C" int storm_sde_predictor_step_rows_rs(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                                const float* a_rows, const float* g_rows, int B, long long n, int N, int kind,
                                                int noise_free, uint64_t seed, uint64_t offset, const uint64_t* row_seeds,
                                                storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_sde_predictor_step_rows_rs: null row_seeds");
    STORM_CHECK(x && score && y && a_rows && g_rows && B > 0 && n > 0 && N > 0, "storm_sde_predictor_step_rows_rs: bad arguments");
    STORM_CHECK(kind == 0 || kind == 1, "storm_sde_predictor_step_rows_rs: kind=%d", kind);
    return launch_rows(predictor_kernel<TableCoef, RowKeys>, B, n, s, x, x_mean, score, y, z, n, N, kind, noise_free,
                       TableCoef{a_rows, g_rows, nullptr}, RowKeys{row_seeds}, offset);
}

extern "C" int storm_sde_pf_drift_rows(float* out, const float* x, const float* y, const float* score, const float* a_rows,
                                       const float* g_rows, int B, long long n, storm_stream_t s) {
    STORM_CHECK(out && x && y && score && a_rows && g_rows && B > 0 && n > 0, "storm_sde_pf_drift_rows: bad arguments");
    return launch_rows(pf_drift_kernel<TableCoef>, B, n, s, out, x, y, score, n, TableCoef{a_rows, g_rows, nullptr});
}

extern "C" int storm_si_sdr(const float* s, const float* s_hat, float* out, int B, long long n, long long stride_s,
                            long long stride_hat, float eps, storm_stream_t st) {
    STORM_CHECK(s && s_hat && out && B > 0 && n > 0, "storm_si_sdr: bad arguments");
    hipLaunchKernelGGL(si_sdr_kernel, dim3(B), dim3(256), 0, (hipStream_t)st, s, s_hat, out, n, stride_s, stride_hat, eps);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}

// ---- validation loss (see the kernels).  The *_rs forms as above; `form` / `kind` are checked here, the kernels trust them.
template <class Key>
static int launch_perturb(const float* x0, const float* y, const float* z, float* xt, const float* m_rows, const float* std_rows,
                          int form, int B, long long n, Key key, uint64_t offset, storm_stream_t s) {
    if (form == 0) return launch_rows(perturb_kernel<0, Key>, B, n, s, x0, y, z, xt, n, m_rows, std_rows, key, offset);
    return launch_rows(perturb_kernel<1, Key>, B, n, s, x0, y, z, xt, n, m_rows, std_rows, key, offset);
}
extern "C" int storm_sde_perturb_rows(const float* x0, const float* y, const float* z, float* xt, const float* m_rows,
                                      const float* std_rows, int form, int B, long long n, uint64_t seed, uint64_t offset,
                                      storm_stream_t s) {
    STORM_CHECK(x0 && y && xt && m_rows && std_rows && B > 0 && n > 0, "storm_sde_perturb_rows: bad arguments");
    STORM_CHECK(form == 0 || form == 1, "storm_sde_perturb_rows: form=%d", form);
    return launch_perturb(x0, y, z, xt, m_rows, std_rows, form, B, n, BatchKey{seed}, offset, s);
}
extern "C" int storm_sde_perturb_rows_rs(const float* x0, const float* y, const float* z, float* xt, const float* m_rows,
                                         const float* std_rows, int form, int B, long long n, uint64_t seed, uint64_t offset,
                                         const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_sde_perturb_rows_rs: null row_seeds");
    STORM_CHECK(x0 && y && xt && m_rows && std_rows && B > 0 && n > 0, "storm_sde_perturb_rows_rs: bad arguments");
    STORM_CHECK(form == 0 || form == 1, "storm_sde_perturb_rows_rs: form=%d", form);
    return launch_perturb(x0, y, z, xt, m_rows, std_rows, form, B, n, RowKeys{row_seeds}, offset, s);
}

extern "C" long long storm_dsm_loss_scratch_bytes(int B, long long n) {
    if (B <= 0 || n <= 0) return 0;
    return (long long)B * loss_blocks(n) * (long long)sizeof(double);
}
static int finish_loss_rows(const double* part, int nb, int B, float* out, storm_stream_t s) {
    hipLaunchKernelGGL(loss_rows_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)s, part, nb, B, out);
    STORM_LAUNCH_CHECK();
    return STORM_OK;
}
template <class Key>
static int launch_dsm_loss(const char* who, const float* score, const float* z, float* out, void* scratch, long long scratch_bytes,
                           const float* std_rows, const int* row_frames, int T, int kind, int B, long long n, Key key,
                           uint64_t offset, storm_stream_t s) {
    STORM_CHECK(score && out && scratch && std_rows && B > 0 && n > 0, "%s: bad arguments", who);
    STORM_CHECK(kind == 0 || kind == 1, "%s: kind=%d", who, kind);
    STORM_CHECK(!row_frames || (T > 0 && n % T == 0), "%s: row_frames with T=%d for rows of %lld elements", who, T, n);
    STORM_CHECK(scratch_bytes >= storm_dsm_loss_scratch_bytes(B, n), "%s: scratch of %lld bytes < %lld", who, scratch_bytes,
                storm_dsm_loss_scratch_bytes(B, n));
    const int nb = loss_blocks(n);
    hipLaunchKernelGGL(dsm_loss_kernel<Key>, dim3(nb, B), dim3(256), 0, (hipStream_t)s, (double*)scratch, score, z, std_rows, row_frames, n, T,
                       kind, key, offset);
    return finish_loss_rows((const double*)scratch, nb, B, out, s);
}
extern "C" int storm_dsm_loss_rows(const float* score, const float* z, float* out, void* scratch, long long scratch_bytes,
                                   const float* std_rows, const int* row_frames, int T, int kind, int B, long long n, uint64_t seed,
                                   uint64_t offset, storm_stream_t s) {
    return launch_dsm_loss("storm_dsm_loss_rows", score, z, out, scratch, scratch_bytes, std_rows, row_frames, T, kind, B, n, BatchKey{seed},
                           offset, s);
}
extern "C" int storm_dsm_loss_rows_rs(const float* score, const float* z, float* out, void* scratch, long long scratch_bytes,
                                      const float* std_rows, const int* row_frames, int T, int kind, int B, long long n, uint64_t seed,
                                      uint64_t offset, const uint64_t* row_seeds, storm_stream_t s) {
    (void)seed;
    STORM_CHECK(row_seeds, "storm_dsm_loss_rows_rs: null row_seeds");
    return launch_dsm_loss("storm_dsm_loss_rows_rs", score, z, out, scratch, scratch_bytes, std_rows, row_frames, T, kind, B, n,
                           RowKeys{row_seeds}, offset, s);
}

extern "C" int storm_pair_loss_rows(const float* a, const float* b, float* out, void* scratch, long long scratch_bytes,
                                    const int* row_frames, int T, int kind, int B, long long n, storm_stream_t s) {
    STORM_CHECK(a && b && out && scratch && B > 0 && n > 0, "storm_pair_loss_rows: bad arguments");
    STORM_CHECK(kind >= 0 && kind <= 2, "storm_pair_loss_rows: kind=%d", kind);
    STORM_CHECK(!row_frames || kind != 2, "storm_pair_loss_rows: row_frames with real samples (kind 2)");
    STORM_CHECK(!row_frames || kind != 0 || n % 2 == 0, "storm_pair_loss_rows: row_frames with an odd float count %lld", n);
    const long long ne = (row_frames && kind == 0) ? n / 2 : n;           // complex elements of a row with frames
    STORM_CHECK(!row_frames || (T > 0 && ne % T == 0), "storm_pair_loss_rows: row_frames with T=%d for rows of %lld elements", T, ne);
    STORM_CHECK(scratch_bytes >= storm_dsm_loss_scratch_bytes(B, n), "storm_pair_loss_rows: scratch of %lld bytes < %lld", scratch_bytes,
                storm_dsm_loss_scratch_bytes(B, n));
    const int nb = loss_blocks(n);
    hipLaunchKernelGGL(pair_loss_kernel, dim3(nb, B), dim3(256), 0, (hipStream_t)s, (double*)scratch, a, b, row_frames, n, T, kind);
    return finish_loss_rows((const double*)scratch, nb, B, out, s);
}
