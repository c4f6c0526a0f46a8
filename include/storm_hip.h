/*
 * libstorm_hip — C ABI of the MI355X-native (gfx950) StoRM reverse-SDE sampling engine.
 *
 * Drop-in boundary for the hot path  ScoreModel.enhance -> get_pc_sampler ->
 * predictor/corrector -> OUVE SDE -> NCSN++ forward  (+ STFT/iSTFT front/back end).
 * The reference (sp-uhh/storm) has no FFI for this path except one pybind op
 * (sgmse/backbones/ncsnpp_utils/op/upfirdn2d.cpp:12-22); its extension points are
 * Python.  Each entry point below therefore names the reference
 * Python/ATen/CUDA interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *  - every function returns 0 (STORM_OK) or a negative error code; the message is
 *    available from storm_last_error() (thread-local);
 *  - nothing allocates: the caller owns every buffer (activations, packed weights,
 *    workspace); all pointers are DEVICE pointers unless a parameter says "host";
 *  - kernels are enqueued on the given HIP stream (pass torch's current stream),
 *    no host synchronisation inside (mirrors upfirdn2d_kernel.cu:213-215);
 *  - activations are NHWC ("[B][F][T][C]", C a multiple of 8) in fp32 or bf16
 *    (dtype argument); the complex spectrogram [B,1,F,T] complex64 of the reference
 *    is bit-identical to NHWC fp32 with C=2 (re, im interleaved);
 *  - thread-compatible: calls from different host threads must use different streams
 *    and buffers.
 */
#ifndef STORM_HIP_H
#define STORM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* storm_stream_t;              /* hipStream_t */

enum { STORM_OK = 0, STORM_ERR_INVALID = -1, STORM_ERR_HIP = -2, STORM_ERR_UNSUPPORTED = -3 };
enum { STORM_F32 = 0, STORM_BF16 = 1, STORM_F16 = 2 };    /* activation / operand dtype (fp32 accumulation always) */

const char* storm_last_error(void);
/* Bumped whenever a public struct changes size or layout (2: storm_conv_args gained splitk_ws / splitk_ws_bytes, storm_op 13 pointer
 * slots).  A host compiled against another header must not call in: check storm_abi_version() == STORM_ABI_VERSION and
 * storm_abi_struct_bytes(0 / 1) == sizeof(storm_conv_args) / sizeof(storm_op) once at load time.  Callers zero-initialise
 * storm_conv_args (memset) before filling it: every optional pointer is "absent" as NULL. */
#define STORM_ABI_VERSION 2
int storm_abi_version(void);
long long storm_abi_struct_bytes(int which);   /* 0: storm_conv_args, 1: storm_op, 2: storm_conv_seg, 3: storm_ncsnpp_config, 4: storm_ncsnpp_config_ex */
/* Test / tool hook, not part of the drop-in surface: the launchers' A/B switches (forced kernel family, pretend-small device for
 * persistent tile walks, ...) are a table filled once from the environment variables of the same names when the library is
 * first used; these two calls read / change an entry afterwards (names: STORM_CONV_VARIANT, STORM_CONV_PIPE128,
 * STORM_CONV_CUS; profiling build also STORM_CONV_PERSIST / _DMA / _ABLATE / _TRACE_PTR).  Production code
 * never calls them and a launch never reads the environment - with ONE exception that is a serving mode, not a test hook:
 * STORM_BATCH_INVARIANT = 1 takes every launch decision that changes a summation order (conv tile by rounds of workgroups,
 * small-call K split, key ranges of the attention) for one image whatever the call holds, so that a row's result does not
 * depend - bit for bit - on what it is batched with (storm_amd.set_batch_invariant). */
int storm_set_switch(const char* name, long long value);
long long storm_get_switch(const char* name);
/* device name / CU count of the current device, for logs; host out-buffers */
int storm_device_info(char* name, int name_len, int* n_cu, size_t* hbm_bytes);

/* ------------------------------------------------------------------------------------------
 * Weight repacking (device -> device).  Replaces nothing in the reference: it is the
 * engine's own weight layout, built once per model from the reference's state_dict tensors.
 *   conv:   src fp32 [Cout][Cin][KH][KW] (nn.Conv2d.weight, layers.py:100-126)
 *           -> dst [KH*KW][CoutP][CinP] (ci contiguous), zero padded
 *   matrix: src fp32 [rows][cols]; transpose!=0 reads src as [cols][rows]
 *           (layers.NIN.W is [Cin][Cout], layers.py:548-557) -> dst [CoutP][CinP]
 * ------------------------------------------------------------------------------------------ */
int storm_pack_conv_weight(const float* src, void* dst, int Cout, int Cin, int ntaps,
                           int CoutP, int CinP, int dtype, storm_stream_t s);
int storm_pack_matrix(const float* src, void* dst, int Cout, int Cin, int transpose,
                      int CoutP, int CinP, int dtype, storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the matrix cores (MFMA 32x32x16 bf16 / 32x32x2 f32).
 * Replaces nn.Conv2d 3x3/1x1 (layers.py:100-126, called from layerspp.py:225-235,260,266,269,
 * ncsnpp.py:183,240,252,108), layers.NIN (layers.py:548-557) and the attention einsums
 * (layerspp.py:82,86) — all are "NT" contractions  out[pix][co] = sum_k X[pix][k] W[co][k].
 *
 * Up to two K-segments accumulate into the same output tile (e.g. Conv_1 3x3 over h plus the
 * Conv_2 1x1 shortcut over x of a BigGAN block, layerspp.py:266-274); a segment may read the
 * channel-concatenation of two tensors (torch.cat([h, hs.pop()], 1), ncsnpp.py:381).
 * Epilogue: out = (acc + bias[co] + tbias[b][co] + skip[pix][co]) * scale.
 * ------------------------------------------------------------------------------------------ */
typedef struct storm_conv_seg {
    const void* src_a;          /* NHWC [B][H][W][Ca]                                   */
    const void* src_b;          /* optional second tensor [B][H][W][Cb] (concat) or NULL  */
    int Ca, Cb;
    long long bstride_a;        /* elements between batches of src_a (H*W*Ca)             */
    long long bstride_b;
    const void* w;              /* packed [ntaps][w_rows_padded][CinP]                    */
    int CinP;                   /* row stride of w (elements)                             */
    int w_rows;                 /* rows of w that may be read (>= Cout valid)             */
    int ntaps;                  /* 9 (3x3, pad 1) or 1                                    */
    long long w_bstride;        /* elements between per-batch weight matrices, 0 = shared */
    long long w_tapstride;      /* elements between taps of w                             */
    const float* gn_ss;         /* optional: fused GroupNorm apply on load: the fp32 (scale, shift) table storm_gn_finalize_ss
                                   writes, [B][(Ca+Cb)/8][2][8] (per 8 channels: their 8 scales, then their 8 shifts);
                                   the conv consumes act(x*scale+shift) (zero padded) instead of x   */
    int gn_silu;                /* apply SiLU after the affine                            */
} storm_conv_seg;

typedef struct storm_conv_args {
    storm_conv_seg seg[2];
    int nseg;
    int B, H, W;                /* 1x1-only calls may pass H=1, W=npix                    */
    void* out;                  /* NHWC [B][H][W][outC]                                   */
    int outC;                   /* channel count of out (multiple of 8)                   */
    int Cout;                   /* valid output channels (<= outC); the rest are written 0+skip */
    long long out_bstride;
    const float* bias;          /* [Cout] or NULL                                         */
    const float* tbias;         /* [B][tbias_stride] per-batch per-channel bias or NULL; rows are read 16 bytes at a time:
                                 * tbias 16-byte aligned, tbias_stride a multiple of 4 (bias: 16-byte aligned)           */
    int tbias_stride;
    const void* skip;           /* NHWC like out (same dtype as activations) or NULL      */
    long long skip_bstride;
    float scale;
    int out_f32;                /* !=0: write fp32 whatever the operand dtype (scores)    */
    int dtype;                  /* STORM_F32 / STORM_BF16 operands + activations          */
    float* gn_part;             /* optional fused GroupNorm statistics: per-tile (sum, sumsq) of
                                   the output, fp32 [B][storm_conv_tiles()][outC][2]; NULL = off */
    void* splitk_ws;            /* optional scratch of storm_conv_splitk_bytes() bytes (16-byte aligned): lets a 3x3 layer with
                                   so few pixel tiles that most CUs would idle split its K loop over workgroups (fp32 slabs,
                                   summed in a fixed order: bit-reproducible).  NULL / too small = the unsplit kernel       */
    long long splitk_ws_bytes;
} storm_conv_args;

int storm_conv(const storm_conv_args* a, storm_stream_t s);
/* The same for P problems that are ONE layer (same weights, channels, taps; own tensors, batch sizes and widths) in ONE launch - the
 * ragged micro-batches of a stream (BASELINE.json configs[4]).  16-bit 3x3 convolutions of the pipelined kernel only
 * (STORM_ERR_UNSUPPORTED otherwise: run them one by one).  A pixel tile computes exactly what storm_conv computes for it with the
 * same tile (bn = 256 or 128 output channels per workgroup; 0 = chosen by the group's tile count); K is never split.  blob: device
 * scratch >= storm_conv_group_blob_bytes (tables of the launch; this convenience entry fills it with a synchronous copy). */
long long storm_conv_group_blob_bytes(const storm_conv_args* a, int P);
int storm_conv_group(const storm_conv_args* a, int P, void* blob, long long blob_bytes, int bn, storm_stream_t s);
/* scratch bytes with which storm_conv would split K for this call; 0 = it would not (most layers).  No counterpart in the
 * reference: a scheduling aid for ddpm_conv3x3 (layers.py:119-126) on the 16 x 64 ... 4 x 16 pixel levels of ncsnpplarge
 * (ncsnpp.py:460-470), where one launch is otherwise a serial K loop on a few workgroups. */
long long storm_conv_splitk_bytes(const storm_conv_args* a);
/* number of pixel tiles per batch item the kernel will use for this call (size of gn_part) */
int storm_conv_tiles(const storm_conv_args* a);
/* name (as rocprofv3 prints it) of the kernel storm_conv launches for these arguments: lets a profiler or
 * bench.py's roofline name the kernel the launcher really picked; static storage */
const char* storm_conv_kernel_name(const storm_conv_args* a);

/* ------------------------------------------------------------------------------------------
 * Fused single-head attention (flash style: online softmax, the [L][L] scores never leave the chip).  Replaces the two
 * einsums and F.softmax of AttnBlockpp.forward (layerspp.py:82-86):
 *   out[b][i][:] = sum_j softmax_j(scale * <q[b][i], k[b][j]>) v[b][j][:] + bias[:]
 * q, k, out: [B][L][C] (C contiguous, = NHWC activations of the NIN projections, layerspp.py:78-80); vT: [B][C][ldv]
 * (v transposed, row stride ldv >= L, a multiple of 8, zero past L); bias = the NIN_2 (v) bias, which passes through the
 * softmax-weighted sum unchanged (rows of the weights sum to one), or NULL.  bf16 / fp16 (P and the output rounded to the
 * operand type) and fp32 (exact-fp32 MFMA: the parity path), C in {32, 64, 128, 256}, any L; other cases return
 * STORM_ERR_UNSUPPORTED (storm_attention_supported tells beforehand) and run as GEMM + storm_softmax_rows.
 * Alignment: the kernels read q, k and vT and write out in 16-byte pieces, so q, k, vT, out (and the scratch of storm_attention_ws) must
 * be 16-byte aligned and the four batch strides - counted in elements, and free otherwise: rows of wider tensors are fine - multiples of
 * 16 bytes (8 elements bf16 / fp16, 4 fp32); the same holds for every pointer of storm_attention_group.  bias has no requirement beyond
 * a float's.  A call outside this is refused (STORM_ERR_INVALID, the argument named in storm_last_error) before anything is launched.
 * ------------------------------------------------------------------------------------------ */
int storm_attention_supported(int C, int dtype);
int storm_attention(const void* q, const void* k, const void* vT, const float* bias, void* out, int B, int L, int C, int ldv,
                    long long q_bstride, long long k_bstride, long long vT_bstride, long long out_bstride, float scale,
                    int dtype, storm_stream_t s);
/* The same with caller scratch: a call whose query blocks leave most CUs idle (one to four utterances) splits the KEY loop into 2 - 8
 * ranges on as many workgroups and merges them in a second launch (fixed order, no atomics).  storm_attention_scratch_bytes = the scratch
 * that call wants (0: it runs unsplit; fp32 never splits); scratch NULL or too small = unsplit.  The merged result differs from the
 * unsplit one by fp32 rounding of the merge (layerspp.py:82-86 computes one softmax over all keys; so does the merge, exactly, in fp32). */
long long storm_attention_scratch_bytes(int B, int L, int C, int dtype);
int storm_attention_ws(const void* q, const void* k, const void* vT, const float* bias, void* out, int B, int L, int C, int ldv,
                       long long q_bstride, long long k_bstride, long long vT_bstride, long long out_bstride, float scale, int dtype,
                       void* scratch, long long scratch_bytes, storm_stream_t s);
/* The same for P problems of one layer in ONE launch (ragged micro-batches of a stream: their own batch sizes and sequence lengths; 16-bit
 * operands; the key loop is never split: the group fills the chip).  q / k / out: P pointers to contiguous [B_p][L_p][C], vT: [B_p][C][ldv_p].
 * A query block computes what the unsplit storm_attention computes for it.  blob: device scratch >= storm_attention_group_blob_bytes. */
long long storm_attention_group_blob_bytes(const int* B, const int* L, int P);
int storm_attention_group(const void* const* q, const void* const* k, const void* const* vT, void* const* out, const int* B, const int* L,
                          const int* ldv, int P, const float* bias, int C, float scale, int dtype, void* blob, long long blob_bytes,
                          storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * GroupNorm(min(C/4,32) groups, eps) [+ SiLU] [+ FIR x2 up / down of BOTH the activated and
 * the raw tensor].  Replaces nn.GroupNorm(eps=1e-6) + nn.SiLU (layerspp.py:219,231,243,264;
 * ncsnpp.py:238,250,392,406; layerspp.py:67,77) and, fused, upsample_2d/downsample_2d on h
 * and x inside ResnetBlockBigGANpp.forward (layerspp.py:245-255).
 * The input may be the channel concat of two tensors.  stats: [B][G][2] doubles (sum, sumsq),
 * must be zero before storm_gn_stats.
 * ------------------------------------------------------------------------------------------ */
int storm_gn_stats(const void* xa, int Ca, const void* xb, int Cb, int B, int HW,
                   int groups, double* stats, int dtype, storm_stream_t s);
/* stats from the per-tile partials a producing storm_conv left in gn_part (no pass over the
 * tensor): channel c < Ca comes from part_a [B][tiles_a][Ca][2], else part_b [B][tiles_b][Cb][2]. */
int storm_gn_finalize(const float* part_a, int Ca, int tiles_a, const float* part_b, int Cb, int tiles_b,
                      int B, int groups, double* stats, storm_stream_t s);
/* Same, and also the per-channel affine of the normalisation for consumers that fuse the apply:
 * scale[c] = rstd*gamma[c], shift[c] = beta[c] - mean*rstd*gamma[c], stored as ss [B][C/8][2][8] (the 8 scales of a channel
 * octet, then its 8 shifts: the order the kernels' packed fp32 math reads them in); count = elements per channel (H*W). */
int storm_gn_finalize_ss(const float* part_a, int Ca, int tiles_a, const float* part_b, int Cb, int tiles_b,
                         int B, int groups, long long count, const float* gamma, const float* beta, float eps,
                         double* stats, float* ss, storm_stream_t s);
/* resample: 0 none, 1 FIR up x2, 2 FIR down x2; the non-FIR members of a network built with fir=False (naive_upsample_2d /
 * naive_downsample_2d in ResnetBlockBigGANpp.forward, layerspp.py:246-258; up_or_down_sampling.py:164-178): 3 nearest up x2,
 * 4 2x2 mean down (mean taken in fp32, rounded once).  out_act gets act(GN(x)) (resampled),
 * out_raw (may be NULL; required non-NULL only if wanted) gets the resampled raw concat. */
int storm_gn_apply(const void* xa, int Ca, const void* xb, int Cb, int B, int H, int W,
                   int groups, const double* stats, const float* gamma, const float* beta,
                   float eps, int silu, int resample, void* out_act, void* out_raw,
                   int dtype, storm_stream_t s);
/* name (as rocprofv3 prints it, without the argument list) of the kernel storm_gn_apply launches for these arguments (C = Ca + Cb):
 * lets a profiler / bench.py's per-op table name what the launcher really picked; static storage */
const char* storm_gn_apply_kernel_name(int C, int B, int H, int W, int silu, int resample, int dtype);

/* FIR resampling with taps [1,3,3,1] (zero boundary), optional "+ add" on the output.
 * Replaces upsample_2d / downsample_2d -> upfirdn2d (up_or_down_sampling.py:195-257,
 * op/upfirdn2d.py:145-156, op/upfirdn2d_kernel.cu:107-207 modes 3 and 5).               */
int storm_fir_up2(const void* x, const void* add, void* out, int B, int H, int W, int C,
                  int dtype, storm_stream_t s);
int storm_fir_down2(const void* x, void* out, int B, int H, int W, int C,
                    int dtype, storm_stream_t s);
/* The reference's one native-op ABI with its own argument list:
 *   upfirdn2d(input[N,H,W,1], kernel[kh,kw], up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1) -> [N,outH,outW,1]
 * (op/upfirdn2d.cpp:12-22 -> upfirdn2d_op, op/upfirdn2d_kernel.cu:209-369; the CPU form is upfirdn2d_native, op/upfirdn2d.py:159-200).
 * input / out: N contiguous planes (the reference reshapes [B,C,H,W] to [B*C,H,W,1]: minor = 1) of `dtype`; kernel: fp32 device taps
 * (the reference always builds it as fp32, up_or_down_sampling.py:223,256); any up / down factors, pads (negative = crop) and kernel
 * size.  out must hold N * outH * outW elements with outH / outW = storm_upfirdn2d_out_size(...) (the caller allocates: at::empty in
 * upfirdn2d_kernel.cu:242-243).  Errors as everywhere: negative code + storm_last_error (TORCH_CHECK in the reference). */
int storm_upfirdn2d(const void* input, const float* kernel, void* out, int N, int H, int W, int kh, int kw,
                    int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                    int dtype, storm_stream_t s);
/* (in * up + pad0 + pad1 - ktaps) / down + 1 (upfirdn2d_kernel.cu:226-227); host arithmetic, no device work */
long long storm_upfirdn2d_out_size(int in, int up, int down, int pad0, int pad1, int ktaps);

/* Row softmax of fp32 scores [rows][ld] (first L columns valid) -> probabilities (activation
 * dtype, same row stride, padding columns written as 0).
 * Replaces F.softmax(w, dim=-1) in AttnBlockpp.forward (layerspp.py:84).                 */
int storm_softmax_rows(const float* scores, void* probs, long long rows, int L, int ld,
                       int dtype, storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Network input / time embedding / output head.
 * ------------------------------------------------------------------------------------------ */
/* complex [B,F,T] tensors (n_in of them) -> NHWC [B][F][T][8] = 2*(re,im..)-1, zero padded.
 * Replaces the real/imag channel packing + "x = 2x - 1" (ncsnpp.py:289-296, 321-323).     */
int storm_pack_input(const float* const* cplx_in /* host array of n_in device ptrs */, int n_in,
                     void* out, int B, int F, int T, int dtype, storm_stream_t s);
/* t[B] -> act_temb[B][4nf] = SiLU(Linear2(SiLU(Linear1(GFP(log t)))))
 * Replaces GaussianFourierProjection + the 2-layer MLP (layerspp.py:39-41, ncsnpp.py:298-317)
 * plus the SiLU that every block applies to temb (layerspp.py:263).                        */
int storm_time_embedding(const float* t, const float* gfp_W, const float* W1, const float* b1,
                         const float* W2, const float* b2, float* act_temb, int B, int nf,
                         storm_stream_t s);
/* out[B][N] = W[N][K] . act_temb[b] + bias[N]  — all blocks' Dense_0 at once (layerspp.py:262-263) */
int storm_dense(const float* x, const float* W, const float* bias, float* out, int B, int N, int K,
                storm_stream_t s);
/* pyramid NHWC [B][F][T][8] -> complex [B,F,T]:  sign * (W[2][cin] . (p / t_b) + b)
 * Replaces "h / used_sigmas", output_layer and view_as_complex (ncsnpp.py:441-449) and the
 * negation in ScoreModel.forward (model.py:131-132) when negate!=0.                        */
int storm_output_head(const void* pyr, const float* t /* NULL: no division */, const float* W,
                      const float* bias, int cin, float* out_cplx, int B, int F, int T,
                      int negate, int dtype, storm_stream_t s);
/* The progressive input pyramid in ONE launch (csrc/pyramid.hip): levels[0] = the packed inputs (exactly storm_pack_input),
 * levels[k] = FIR x2 down of levels[k - 1] (exactly storm_fir_down2), k < n_levels <= 4; levels[k]: NHWC [B][F >> k][T >> k][8].
 * cplx_in == NULL: levels[0] is READ instead of written (the continuation of a pyramid deeper than three steps: ncsnpplarge has six).
 * Replaces the packing above and pyramid_downsample before every Combine (ncsnpp.py:352-355; up_or_down_sampling.py:230-257): the input
 * pyramid depends on the network input alone, so it is built once, ahead of the U-Net.                                            */
int storm_input_pyramid(const float* const* cplx_in /* host array of n_in device ptrs, or NULL */, int n_in,
                        void* const* levels /* host array of n_levels device ptrs */, int n_levels, int B, int F, int T,
                        int dtype, storm_stream_t s);
/* The same with the options of the reference constructor: mean != 0 = the non-FIR pyramid of fir=False, levels[k] = the 2x2 mean of
 * levels[k - 1] (pyramid_downsample = Downsample(fir=False, with_conv=False) -> F.avg_pool2d(x, 2), layerspp.py:151-156); centered != 0 =
 * the inputs are packed as they are, without the 2x - 1 of ncsnpp.py:325-327.  storm_input_pyramid is this call with (0, 0).          */
int storm_input_pyramid_ex(const float* const* cplx_in, int n_in, void* const* levels, int n_levels, int B, int F, int T, int mean,
                           int centered, int dtype, storm_stream_t s);
/* Combine(method='cat') (layerspp.py:44-59; progressive_combine='cat', ncsnpp.py:204-207): out NHWC [npix][2 C] =
 * cat([conv1x1(x) + bias, h], channels) in one pass - x: the 8-channel input-pyramid level [npix][8], w: its packed 1x1 weight
 * [C rows][CinP] (storm_pack_conv_weight), h: [npix][C].  The convolution lands in the channel slice [0, C), h is copied to [C, 2 C). */
int storm_combine_cat(const void* x, const void* w, int CinP, const float* bias, const void* h, void* out, long long npix, int C,
                      int dtype, storm_stream_t s);
/* The progressive output pyramid and the head in ONE launch: p_{L-1} = ph[L-1]; p_k = up2(p_{k+1}) + ph[k] (exactly storm_fir_up2 with
 * its add operand, every level rounded to the storage type); out = storm_output_head(p_0, ...).  ph[k]: NHWC [B][F >> k][T >> k][8], the
 * outputs of the pyramid's 3x3 convolutions, finest first, n_levels <= 8.  Replaces pyramid_upsample + "pyramid = pyramid + pyramid_h"
 * after every decoder level (ncsnpp.py:389-410) and the head (ncsnpp.py:441-449).                                                   */
int storm_output_pyramid(const void* const* ph /* host array of n_levels device ptrs */, int n_levels, const float* t /* NULL: no division */,
                         const float* W, const float* bias, int cin, float* out_cplx, int B, int F, int T, int negate, int dtype,
                         storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * OUVE SDE steps on the complex64 state [B, n] (n = F*T complex per batch item).
 * Replace OUVESDE.prior_sampling/_std/sde, SDE.discretize, RSDE.discretize (sdes.py:73-90,
 * 147-157, 200-237), ReverseDiffusionPredictor / EulerMaruyamaPredictor.update_fn
 * (predictors.py:46-69), AnnealedLangevinDynamics / LangevinCorrector.update_fn
 * (correctors.py:45-93).  z == NULL: standard complex normal noise (variance 1/2 per
 * component, like torch.randn_like on a complex tensor) is generated in-kernel with
 * Philox4x32-10 from (seed, offset).
 * ------------------------------------------------------------------------------------------ */
typedef struct storm_ouve { float theta, sigma_min, sigma_max; int N; } storm_ouve;

int storm_ouve_prior(const float* y, const float* z, float* x, int B, long long n, storm_ouve p,
                     uint64_t seed, uint64_t offset, storm_stream_t s);
int storm_ouve_ald_step(float* x, float* x_mean, const float* score, const float* z, const float* t,
                        int B, long long n, storm_ouve p, float snr,
                        uint64_t seed, uint64_t offset, storm_stream_t s);
/* predictor: kind 0 = reverse_diffusion, 1 = euler_maruyama; noise_free!=0 skips "+ G z" */
int storm_ouve_predictor_step(float* x, float* x_mean, const float* score, const float* y,
                              const float* z, const float* t, int B, long long n, storm_ouve p,
                              int kind, int noise_free, uint64_t seed, uint64_t offset,
                              storm_stream_t s);
/* ---- per-row noise keys (the *_rs forms).  The entry points above draw element i of row b from the Philox counter b * n + i of ONE
 * seed: a row's noise depends on where it sits in the batch.  The *_rs forms take their sibling's argument list plus
 * row_seeds = device uint64 [B] and draw row b from (key row_seeds[b], counter i within the row, offset) - exactly what the
 * sibling called on that row alone (B = 1) with seed = row_seeds[b] and the same offset draws, so a seeded result does not depend on
 * the batch around it.  `seed` is not read; z != NULL injects noise as before; everything after the draw is the sibling's arithmetic.
 * They replace the same reference lines as their siblings, called once per utterance (enhancement.py:66-72: one file per call):
 *   storm_ouve_prior_rs              OUVESDE.prior_sampling (sdes.py:233-237)
 *   storm_ouve_ald_step_rs           AnnealedLangevinDynamics.update_fn (correctors.py:64-93)
 *   storm_ouve_predictor_step_rs     ReverseDiffusionPredictor / EulerMaruyamaPredictor.update_fn (predictors.py:46-69) with
 *                                    SDE.discretize / RSDE.discretize (sdes.py:73-90, 147-157)
 *   storm_sde_prior_rows_rs          OUVPSDE.prior_sampling (sdes.py:306-310)
 *   storm_sde_predictor_step_rows_rs the predictors' update_fn (predictors.py:46-69) over OUVPSDE (sdes.py:286-301, 123-157)
 *   storm_complex_randn_rs           torch.randn_like(x) of LangevinCorrector.update_fn (correctors.py:50-52): z = [B][n_per_row] */
int storm_ouve_prior_rs(const float* y, const float* z, float* x, int B, long long n, storm_ouve p,
                        uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s);
int storm_ouve_ald_step_rs(float* x, float* x_mean, const float* score, const float* z, const float* t,
                           int B, long long n, storm_ouve p, float snr,
                           uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s);
int storm_ouve_predictor_step_rs(float* x, float* x_mean, const float* score, const float* y,
                                 const float* z, const float* t, int B, long long n, storm_ouve p,
                                 int kind, int noise_free, uint64_t seed, uint64_t offset,
                                 const uint64_t* row_seeds, storm_stream_t s);
/* per-batch L2 norms of complex tensors: out[b] = ||v_b||  (correctors.py:53-54) */
int storm_batch_l2norm(const float* v, float* out, int B, long long n, storm_stream_t s);
/* Langevin corrector step; z must be given or generated beforehand (its norm is needed):
 * step = 2 (snr * ||z|| / ||score||)^2 with the norms taken as
 *   mode 0: means over the B rows (correctors.py:53-55 for the batch handed to the sampler),
 *   mode 1: row b's own norms (B independent batch-1 calls: what the reference CLI computes per file),
 *   mode 2: score_norms[0] / z_norms[0] = means over a larger batch (all-reduced over the ranks of a sharded run). */
int storm_langevin_step(float* x, float* x_mean, const float* score, const float* z,
                        const float* score_norms, const float* z_norms, int B, long long n, float snr, int mode,
                        storm_stream_t s);
/* Scale-invariant SDR in dB of B (clean s, estimate s_hat) waveform pairs, fp32 [B][>= n] with row strides (util/other.py:82-94:
 * si_sdr with eps = 0, si_sdr_torch with eps = 1e-10; used by the evaluation loop, util/inference.py:20-72) */
int storm_si_sdr(const float* s, const float* s_hat, float* out, int B, long long n, long long stride_s, long long stride_hat,
                 float eps, storm_stream_t st);
/* drift of the probability-flow ODE, out = theta (y - x) - 1/2 g(t)^2 score  (sdes.py:92-121 with probability_flow, :203-207) */
int storm_ouve_pf_drift(float* out, const float* x, const float* y, const float* score, const float* t, int B,
                        long long n, storm_ouve p, storm_stream_t s);
/* the same with g(t_b) given per row (device fp32 [B]; the ODE sampler computes it with the reference's own fp32 formula,
 * sdes.py:203-207, so the right-hand side matches the reference's to the last bit) */
int storm_ouve_pf_drift_g(float* out, const float* x, const float* y, const float* score, const float* g_rows, int B,
                          long long n, float theta, storm_stream_t s);
/* ---- coefficient-table forms for any SDE  dx = a(t) (y - x) dt + g(t) dw: the second SDE the reference registers, OUVPSDE
 * (sdes.py:255-326: a = 1/2 stiffness beta(t), g = sqrt(beta(t)), beta(t) = beta_min + t (beta_max - beta_min)).  a_rows / g_rows /
 * std_rows = the per-row values at t_b (device fp32 [B]); the host side forms them with the reference's own fp32 expressions
 * (sdes.py:286-301), the kernels do the state-sized work of OUVPSDE.prior_sampling (:306-310), SDE.discretize (:73-90),
 * RSDE.discretize / rsde_parts (:123-157) and the predictors' update_fn (predictors.py:46-69) exactly as the storm_ouve_* ones do.
 * kind / noise_free / z == NULL as in storm_ouve_predictor_step; N = the SDE's discretisation steps (dt = 1 / N). */
int storm_sde_prior_rows(const float* y, const float* z, float* x, const float* std_rows, int B, long long n,
                         uint64_t seed, uint64_t offset, storm_stream_t s);
int storm_sde_predictor_step_rows(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                  const float* a_rows, const float* g_rows, int B, long long n, int N, int kind,
                                  int noise_free, uint64_t seed, uint64_t offset, storm_stream_t s);
/* the same two with per-row noise keys (see storm_ouve_prior_rs) */
int storm_sde_prior_rows_rs(const float* y, const float* z, float* x, const float* std_rows, int B, long long n,
                            uint64_t seed, uint64_t offset, const uint64_t* row_seeds, storm_stream_t s);
int storm_sde_predictor_step_rows_rs(float* x, float* x_mean, const float* score, const float* y, const float* z,
                                     const float* a_rows, const float* g_rows, int B, long long n, int N, int kind,
                                     int noise_free, uint64_t seed, uint64_t offset, const uint64_t* row_seeds,
                                     storm_stream_t s);
/* out = a_b (y - x) - 1/2 g_b^2 score: the probability-flow right-hand side (sdes.py:92-145 with probability_flow=True) */
int storm_sde_pf_drift_rows(float* out, const float* x, const float* y, const float* score, const float* a_rows,
                            const float* g_rows, int B, long long n, storm_stream_t s);
/* ---- validation loss: the reference's `_step`, the number logged as valid_loss (model.py:138-154 ScoreModel, :329-349
 * DiscriminativeModel, :560-595 StochasticRegenerationModel).  Rows as above: complex64 [B][n], one kernel per pass.
 * Forward diffusion  xt[b] = mean_b(x0, y) + std_rows[b] z  (SDE.marginal_prob + model.py:144-150; sdes.py:210-231 OUVESDE,
 * :296-306 OUVPSDE) without a `mean` tensor.  m_rows / std_rows: the mean factor and the std at t_b, device fp32 [B], formed by
 * the caller with the reference's own fp32 expressions.  form 0: m x0 + (1 - m) y (OUVESDE._mean, 1 - m in fp32 in the kernel);
 * form 1: y + m (x0 - y) (OUVPSDE._mean).  z NULL: drawn in the kernel from (seed, offset) as storm_sde_prior_rows does. */
int storm_sde_perturb_rows(const float* x0, const float* y, const float* z, float* xt, const float* m_rows,
                           const float* std_rows, int form, int B, long long n, uint64_t seed, uint64_t offset,
                           storm_stream_t s);
int storm_sde_perturb_rows_rs(const float* x0, const float* y, const float* z, float* xt, const float* m_rows,
                              const float* std_rows, int form, int B, long long n, uint64_t seed, uint64_t offset,
                              const uint64_t* row_seeds, storm_stream_t s);
/* Denoising-score-matching residual per row, out[b] = 0.5 sum_i rho(score[b][i] std_rows[b] + z[b][i]), fp32 [B]: err formed in
 * fp32 (model.py:151-152), rho = |.|^2 (kind 0, `mse`) or |.| (kind 1, `mae`) and the sum in fp64 (ScoreModel._loss model.py:113-122,
 * loss_fn_score :468-470; the caller takes the mean or the sum of the rows).  z NULL: re-drawn in the kernel from the (seed, offset)
 * / row_seeds the perturbation used - the noise never exists in memory.  row_frames (device int [B], may be NULL) with T = frames
 * per row (n % T == 0): row b counts only the elements whose frame index i % T is below row_frames[b] (the zero frames of a ragged
 * or padded batch stay out).  Per-block fp64 partials, then a fixed-order row sum; the block count depends on n only: a row's value
 * is the same in every run and every batch.  scratch: caller-owned, >= storm_dsm_loss_scratch_bytes(B, n) bytes. */
long long storm_dsm_loss_scratch_bytes(int B, long long n);
int storm_dsm_loss_rows(const float* score, const float* z, float* out, void* scratch, long long scratch_bytes,
                        const float* std_rows, const int* row_frames, int T, int kind, int B, long long n, uint64_t seed,
                        uint64_t offset, storm_stream_t s);
int storm_dsm_loss_rows_rs(const float* score, const float* z, float* out, void* scratch, long long scratch_bytes,
                           const float* std_rows, const int* row_frames, int T, int kind, int B, long long n, uint64_t seed,
                           uint64_t offset, const uint64_t* row_seeds, storm_stream_t s);
/* The predictive models' losses per row (DiscriminativeModel._loss model.py:329-343, loss_fn_denoiser :479-481), out[b] fp32, the
 * same reduction: kind 0  0.5 sum (a - b)^2 over the n FLOATS of a row (a complex spectrogram through its float view, or a real
 * waveform); kind 1  0.5 sum |a - b| over n COMPLEX elements; kind 2  the same over n real samples.  row_frames / T as above for
 * complex rows (kinds 0 and 1; kind 0: n even, T divides n / 2).  scratch >= storm_dsm_loss_scratch_bytes(B, n).  (`sisdr`,
 * model.py:341-342, is storm_si_sdr with eps = 1e-10.) */
int storm_pair_loss_rows(const float* a, const float* b, float* out, void* scratch, long long scratch_bytes,
                         const int* row_frames, int T, int kind, int B, long long n, storm_stream_t s);
/* ---- probability-flow ODE sampler (sampling/__init__.py:71-141 hands the state to scipy's RK45 on the host) ----
 * out = x + h * sum_{j<n_terms} coef[j] K[j]   (one Runge-Kutta stage; K = host array of device pointers, <= 7) */
int storm_rk_combine(float* out, const float* x, const float* const* K, const float* coef, int n_terms, float h,
                     long long n_complex, storm_stream_t s);
/* out[0] = sum_c |v_c|^2 / (atol + max(|xa_c|, |xb_c|) rtol)^2 over the complex elements (scipy's scaled norms, squared
 * and un-averaged): v = h * sum coef[j] K[j] (n_terms > 0: the embedded error), K[0] (n_terms = -1) or K[0] - K[1]
 * (n_terms = -2).  xb may be NULL.  scratch: >= 2048 doubles; deterministic (fixed summation order). */
int storm_rk_scaled_sumsq(double* out, double* scratch, int scratch_len, const float* xa, const float* xb,
                          const float* const* K, const float* coef, int n_terms, float h, float atol, float rtol,
                          long long n_complex, storm_stream_t s);
/* Per-row forms for a batch of B independent utterances that advance with their OWN step sizes (the reference calls solve_ivp
 * once per utterance: model.py:224-244, minibatch = 1).  scipy keeps its state in complex128 and only the right-hand side
 * runs in fp32 (sampling/__init__.py:119-123): x / out64 / xa / xb are complex128 [B][n_complex_row], the stages K complex64,
 * coefficients and step sizes fp64, so step decisions follow scipy's to 1e-16.  h_rows: HOST array of B step sizes
 * (B <= STORM_RK_MAX_ROWS, passed in the kernel arguments).
 *   combine_rows:      out[b] = x[b] + h_rows[b] * sum_j coef[j] K[j][b]  -> out64 (complex128) and / or out32 (complex64)
 *   scaled_sumsq_rows: out[b] = row b's sum of |v|^2 / (atol + max(|xa|, |xb|) rtol)^2; v as in storm_rk_scaled_sumsq
 *                      (n_terms = -3: v = xa itself); h_rows NULL = 1.  The partial-sum geometry depends on the row length
 *                      only, so a row's value does not depend on the batch around it; scratch: >= STORM_RK_ROW_BLOCKS * B doubles
 *   copy_rows:         dst[b] = src[b] for the rows with row_mask[b] != 0 (HOST mask): the accepted rows of a step */
enum { STORM_RK_MAX_ROWS = 128, STORM_RK_ROW_BLOCKS = 256 };
int storm_rk_combine_rows(double* out64, float* out32, const double* x, const float* const* K, const double* coef, int n_terms,
                          const double* h_rows, int B, long long n_complex_row, storm_stream_t s);
int storm_rk_scaled_sumsq_rows(double* out, double* scratch, long long scratch_len, const double* xa, const double* xb,
                               const float* const* K, const double* coef, int n_terms, const double* h_rows, double atol,
                               double rtol, int B, long long n_complex_row, storm_stream_t s);
int storm_copy_rows(void* dst, const void* src, const int* row_mask, int B, long long row_bytes, storm_stream_t s);
/* The wide forms: up to STORM_RK_MAX_TERMS stages, for solve_ivp's other explicit methods (sampling/__init__.py:71-141 passes
 * `method` on to scipy: RK23's rows fit the forms above, DOP853 has 12 terms in a stage and 13 in its two error estimators,
 * scipy/integrate/_ivp/rk.py DOP853._step_impl / _estimate_error_norm).  Types, h_rows and B as in the per-row forms above.
 *   combine_rows_wide: storm_rk_combine_rows with n_terms in 1..13; for n_terms <= 7 the same bits.  16-byte stage accesses where
 *                      the row length is even and K / out32 are 16-byte aligned.
 *   error_pair_rows:   ONE pass over the stages for two coefficient rows: out[b] = row b's sum of |va|^2 / scale^2 and out[B + b]
 *                      that of |vb|^2 / scale^2, v = h_rows[b] * sum_j coef[j] K[j][b], scale = atol + max(|xa|, |xb|) rtol
 *                      (xb may be NULL); h_rows NULL = 1 (DOP853 applies |h| to the norm on the host).  The geometry of
 *                      storm_rk_scaled_sumsq_rows (each sum is its bits for n_terms <= 7), no atomics; scratch: >= 2 *
 *                      STORM_RK_ROW_BLOCKS * B doubles, out: 2 * B doubles. */
enum { STORM_RK_MAX_TERMS = 13 };
int storm_rk_combine_rows_wide(double* out64, float* out32, const double* x, const float* const* K, const double* coef, int n_terms,
                               const double* h_rows, int B, long long n_complex_row, storm_stream_t s);
int storm_rk_error_pair_rows(double* out, double* scratch, long long scratch_len, const double* xa, const double* xb,
                             const float* const* K, const double* coef_a, const double* coef_b, int n_terms, const double* h_rows,
                             double atol, double rtol, int B, long long n_complex_row, storm_stream_t s);
/* fills z[B*n] complex with standard complex normal noise (re, im ~ N(0, 1/2)).  Element i is Philox4x32-10 of
 *   key     (k0, k1)         = (low, high 32 bits of seed)
 *   counter (c0, c1, c2, c3) = (low, high 32 bits of i, low, high 32 bits of offset)
 * followed by Box-Muller on the first two output words w0, w1: u = (float(w >> 8) + 0.5f) * 2^-24 in fp32, which lies in (0, 1]
 * (the + 0.5f of 0xFFFFFF rounds to even), z = sqrtf(-logf(u1)) * (cos, sin)(fl32(2 pi) * u2).  Every entry point that takes
 * (seed, offset) draws element i of row b from the same generator at i = b * n + i_in_row; the *_rs forms use key row_seeds[b]
 * and i = i_in_row.  tests/philox_ref.py is an independent reference of this layout. */
int storm_complex_randn(float* z, long long n_complex, uint64_t seed, uint64_t offset,
                        storm_stream_t s);
/* rows form: z[B][n_per_row], row b = storm_complex_randn(n_per_row, row_seeds[b], offset) (see storm_ouve_prior_rs; the draw
 * of torch.randn_like in LangevinCorrector.update_fn, correctors.py:50-52, made per utterance) */
int storm_complex_randn_rs(float* z, int B, long long n_per_row, uint64_t seed, uint64_t offset,
                           const uint64_t* row_seeds, storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Spectral front / back end.  Replace torch.stft / torch.istft as called by
 * SpecsDataModule.stft/istft (data_module.py:195-223: n_fft, hop, periodic Hann, center=True,
 * reflect padding), spec_fwd / spec_back (data_module.py:182-193), pad_spec (util/other.py:
 * 102-109) and the peak normalisation in enhance() (model.py:282-284, 302).
 * ------------------------------------------------------------------------------------------ */
/* out = spec_fwd(in) (inverse==0) or spec_back(in) (inverse!=0) on n complex64 values
 * (data_module.py:182-193): |z|^e e^{j angle z} * factor  /  its inverse.  An exact-zero bin stays exactly zero in both
 * directions.  |z| is sqrtf(re^2 + im^2) while re^2 + im^2 lies in [2^-100, 2^100] and hypotf(re, im) outside, where the squares
 * under- or overflow and torch.abs does not (here, in storm_stft and in storm_istft alike).  */
int storm_spec_transform(const float* in, float* out, long long n_complex, float spec_factor,
                         float spec_abs_exponent, int inverse, storm_stream_t s);
/* Ragged batches (micro-batching of utterances of different lengths that share ONE padded frame count, i.e.
 * roundup(frames(L_b), 64) equal for all rows, frames(L) = 1 + (L + 2 (n_fft / 2) - n_fft) / hop in integer division: torch.stft's
 * count with center=True, which is 1 + L / hop for an even n_fft and 1 + (L - 1) / hop for an odd one; storm_stft takes
 * n_frames = frames(L) and refuses another value): the three front / back end calls take row_len = device int32 [B] with
 * every row's own sample count (NULL = all rows L); wav buffers are [B][L] with L = the longest row, zero filled past a
 * row's length.  Row b then equals the single-utterance call with L_b (the reference pads per utterance,
 * util/other.py:102-109, enhancement.py:66-72).
 * peak[b] = max |wav[b][:L_b]|  (model.py:283) */
int storm_peak_abs(const float* wav, float* peak, int B, long long L, long long stride, const int* row_len,
                   storm_stream_t s);
/* wav [B][L] (row stride `stride`) -> spec complex [B][F][Tpad]; frames >= n_frames are zero.
 * spec = spec_fwd(stft(wav / peak[b])); peak may be NULL (no normalisation).
 * twiddle: fp32 [n_fft][2] = (cos, sin)(2 pi k / n_fft); window: fp32 [n_fft].            */
int storm_stft(const float* wav, const float* peak, float* spec, const float* window,
               const float* twiddle, int B, long long L, long long stride, int n_fft, int hop,
               int n_frames, int Tpad, float spec_factor, float spec_abs_exponent, const int* row_len,
               storm_stream_t s);
/* spec complex [B][F][T] (ALL T frames are inverted, as to_audio does, model.py:258-259,301)
 * -> wav [B][L] = istft(spec_back(spec), length=L) * peak[b].
 * frames: workspace fp32 [B][T][n_fft].                                                    */
int storm_istft(const float* spec, const float* peak, float* wav, float* frames,
                const float* window, const float* twiddle, int B, int T, long long L,
                long long stride, int n_fft, int hop, float spec_factor, float spec_abs_exponent,
                const int* row_len, storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Rational resampling (audio at another rate than the model's 16 kHz): x [B][L_in] at rate sr_in -> y [B][L_out] at sr_out with
 * up / down = sr_out / sr_in REDUCED (g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g), L_out = ceil(L_in up / down):
 *   R = max(up, down), half = 10 R;  h[j], j = 0 .. 2 half: the Kaiser(beta = 5) windowed-sinc low-pass with cut-off 1 / R of
 *   Nyquist, normalised to unit DC gain, times up;
 *   y[n] = sum_k h[n down - k up + half] x[k]        (x = 0 outside [0, L_in), h = 0 outside [0, 2 half])
 * i.e. scipy.signal.resample_poly(x, up, down) with its defaults.  Polyphase: c = n down + half, p = c mod up, q = c div up,
 * y[n] = sum_{m < M_p} T[p][m] x[q - m] with T[p][m] = h[p + m up] - one fp32 FMA chain over m ascending per output, so an
 * output's bits depend on its own row's samples only.  Refused: a ratio that is not reduced, max(up, down) > 1024.
 *
 * storm_resample_num_taps: 2 half + 1 (< 0: refused).  The phase-major table has M = ceil(num_taps / up) taps per phase.
 * storm_resample_taps (host): designs h in fp64 (I0 by its power series), rounds every tap to fp32 once and writes T as
 *   fp32 [up][M], zero past M_p, into the CALLER's host memory of `capacity` floats (>= up M) - the single source of the
 *   coefficients; the caller copies the table to the device.
 * storm_resample_poly: taps = that table on the device.  row_len (optional, device int32 [B]): the rows' own input sample
 *   counts; row b then gets ceil(row_len[b] up / down) outputs, the rest of its output row is zero, and its input samples at
 *   k >= row_len[b] are never read.  One workgroup computes STORM_RESAMPLE_TILE outputs of one row. */
#define STORM_RESAMPLE_MAX_RATE 1024
#define STORM_RESAMPLE_TILE 1024
int storm_resample_num_taps(int up, int down);
int storm_resample_taps(int up, int down, float* taps_phase_major, long long capacity);
int storm_resample_poly(const float* x, float* y, const float* taps, int B, long long L_in, long long stride_in,
                        long long L_out, long long stride_out, const int* row_len, int up, int down, storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Metrics of enhanced audio (the reference's calc_metrics step; definitions in util/other.py).  Both are one streaming pass: a row is cut
 * at FIXED positions, a workgroup sums one piece in fp64 into the caller's scratch, a second kernel adds a row's pieces in index order -
 * no atomics, and a row's numbers are the same bits at any B, batch width, row stride and position in the batch.
 *
 * storm_energy_ratios_rows: s_hat, s, n fp32 [B][L] (row strides in floats) -> out fp64 [B][4] =
 *   (SI-SDR, SI-SIR, SI-SAR) = energy_ratios(s_hat, s, n) (util/other.py:35-44) on the decomposition of si_sdr_components (:21-33), whose
 *   eps is always its own default 1e-10 (energy_ratios does not pass its argument on), and the input SNR snr_dB(s, n) (:96-100).
 *   From the six inner products of (s_hat, s, n), accumulated in fp64 (fp32 x fp32 is exact there) over pieces of STORM_METRICS_CHUNK
 *   samples; |s_hat - alpha_s s|^2 and |s_hat - alpha_s s - alpha_n n|^2 are expanded in them.  row_len (optional, device int32 [B]):
 *   row b is its first row_len[b] samples; the rest is never read.
 * storm_lsd_rows: two complex64 spectrograms [B][F][T] (storm_stft's layout) -> out fp64 [B] =
 *   sqrt(mean_{f, t < frames_b} |2 ln(eps + |spec_hat|) - 2 ln(eps + |spec|)|), lsd of util/other.py:16-19 after its two STFTs (one mean
 *   over all bins, then the root); magnitudes and logarithms in fp64.  row_frames (optional, device int32 [B]): the rows' own frame counts
 *   (padding frames are not counted).
 * scratch: device memory of at least the _scratch_bytes of the same (B, L) / (B, F, T), 8-byte aligned, pure scratch. */
#define STORM_METRICS_CHUNK 16384
long long storm_energy_ratios_scratch_bytes(int B, long long L);
int storm_energy_ratios_rows(const float* s_hat, const float* s, const float* n, double* out, void* scratch, long long scratch_bytes, int B,
                             long long L, long long stride_hat, long long stride_s, long long stride_n, const int* row_len, storm_stream_t st);
long long storm_lsd_scratch_bytes(int B, int F, int T);
int storm_lsd_rows(const float* spec_hat, const float* spec, double* out, void* scratch, long long scratch_bytes, int B, int F, int T,
                   const int* row_frames, double eps, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * Intelligibility of enhanced audio: STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) per row.  The reference
 * never computes them itself (it calls the pystoi package, util/inference.py:65), so THIS TEXT is the specification; the numbers were
 * checked against a float64 restatement of the published algorithm (tests/stoi_cases.py), not against pystoi.
 * Constants: FS = 10000, N_FRAME = 256, HOP = 128, NFFT = 512, 15 third-octave bands from 150 Hz, segments of N = 30 frames,
 * BETA = -15 dB, DYN_RANGE = 40 dB, EPS = 2^-52.  Inputs: x (clean) and y (processed), the row's first `len` samples of each, at fs_sig.
 *  1. Resample (only if fs_sig != FS) both signals by up / down = FS / fs_sig reduced: R = max(up, down), fc = 1 / (2 R),
 *     L = ceil((60 - 8) / (28.714 fc / 10)); h[t], t = 0 .. 2 L: kaiser(2 L + 1, beta = 0.1102 (60 - 8.7))[t] * 2 up fc sinc(2 fc (t - L)),
 *     normalised to sum(h) = 1, applied as scipy.signal.resample_poly(x, up, down, window=h) applies it (times up, centred:
 *     out[n] = sum_k up h[n down - k up + L] in[k]); ceil(len up / down) outputs.  16 kHz: 5 / 8, 581 taps; 48 kHz: 5 / 24, 1741 taps.
 *  2. Silent frames: w = hanning(258)[1:-1]; frames start at i = 0, 128, ... < len - 256 (strict: the frame that would end exactly at the
 *     last sample is not taken); e_k = 20 log10(|w x_frame_k|_2 + EPS); frame k is kept iff max_k(e) - 40 - e_k < 0, and the same mask applies
 *     to y.  The K kept frames, already windowed, are overlap-added at hop 128 into x_sil, y_sil of (K - 1) 128 + 256 samples.
 *  3. STFT: frames of x_sil start at 0, 128, ... < len_sil - 256: M = K - 1 frames; each times w again, zero padded to 512, rfft (257 bins).
 *  4. Bands: band i sums |X_j|^2 over edge_i <= j < edge_{i+1}, edges (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
 *     (the bins nearest to 150 * 2^((2 i -+ 1) / 6) Hz); X_tob = sqrt(band sums) [15][M], likewise Y_tob.
 *  5. M < 30 (rows with len <= 256 included): both results are 1e-5 (pystoi's "not enough frames" value).
 *  6. Segments m = 30 .. M: columns m - 30 .. m - 1, J = M - 29 segments of [15][30].
 *  ESTOI: in each segment, every band minus its mean over the 30 frames, over its 2-norm; then every frame minus its mean over the 15
 *     bands, over its 2-norm; for X and Y; d = sum(Xn Yn) / (30 J).
 *  STOI: in each segment and band c = |x| / (|y| + EPS), y' = min(c y, x (1 + 10^(15/20))); x and y' minus their means over the 30 frames,
 *     each over its norm + EPS; d = sum(x y') / (15 J).
 *  Deviation from pystoi: pystoi adds EPS * randn jitter before each ESTOI normalisation (its last digits are not deterministic); here
 *     there is no jitter and every ESTOI normalisation divides by norm + EPS - a constant band or frame contributes 0, not a random direction.
 *
 * storm_stoi_num_taps / storm_stoi_taps (host): the filter of step 1 for fs_sig, 2 L + 1 taps (< 0: refused - fs_sig < 1 or
 *   max(up, down) > STORM_RESAMPLE_MAX_RATE), designed in fp64 (I0 by its power series), times up, rounded to fp32 once, written in
 *   storm_resample_taps' phase-major layout fp32 [up][M], M = ceil(num_taps / up), into the CALLER's host memory.
 * storm_resample_poly_taps: storm_resample_poly with a table of an explicit num_taps (odd, >= 1; half = (num_taps - 1) / 2) - the same
 *   kernel, the same single fp32 FMA chain per output.
 * storm_stoi_rows: x, y fp32 [B][L] AT 10 kHz (row strides in floats) -> out fp64 [B][2] = (STOI, ESTOI), steps 2 - 6.  row_len (optional,
 *   device int32 [B]): row b is its first row_len[b] samples, the rest is never read.  After the samples are read all arithmetic is fp64;
 *   no atomics, every sum in an order fixed by indices inside the row: a row's two numbers are the same bits alone, in any batch, at any
 *   batch width, row stride and position.  x_sil is never written: spectrogram frame m reads the kept frames m - 1, m, m + 1 of the row.
 *   scratch: at least storm_stoi_scratch_bytes(B, L) bytes of device memory, 8-byte aligned; after the call it begins with int32 [B][4] =
 *   (gate frames, kept frames K, segments J, spectrogram frames M) of every row. */
int storm_stoi_num_taps(int fs_sig);
int storm_stoi_taps(int fs_sig, float* taps_phase_major, long long capacity);
int storm_resample_poly_taps(const float* x, float* y, const float* taps, int B, long long L_in, long long stride_in, long long L_out,
                             long long stride_out, const int* row_len, int up, int down, int num_taps, storm_stream_t s);
long long storm_stoi_scratch_bytes(int B, long long L);
int storm_stoi_rows(const float* x, const float* y, double* out, void* scratch, long long scratch_bytes, int B, long long L,
                    long long stride_x, long long stride_y, const int* row_len, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * Frame-based measures of enhanced audio: segmental SNR, log-likelihood ratio (LLR) and LPC cepstral distance (CD) per row - the family of
 * Quackenbush, Barnwell, Clements 1988 as the evaluation code of Hu, Loizou 2008 and the REVERB challenge use it.  The reference has no
 * such metric, so THIS TEXT is the specification; the numbers were checked against a float64 restatement of it (tests/lpc_cases.py), not
 * against pysepm.  Inputs: x (clean) and y (processed) fp32, the row's first `len` samples of each, at fs Hz; after a sample is read all
 * arithmetic is fp64.
 * Constants: W = (30 fs + 500) / 1000 and H = W / 4 in integer division (16 kHz: 480, 120; 8 kHz: 240, 60; 44.1 kHz: 1323, 330);
 *   P = 16 for fs >= 10000, else 10; EPS = 2^-52.  Refused: fs with W <= 2 P or W > 2048.
 *  1. Frames: M = (len - W) / H by floor division for len >= W, else 0; frame m covers samples m H .. m H + W - 1.  This is the count of the
 *     published MATLAB / pysepm code as recalled here, ONE SHORT of every full frame of the row (the frame that ends at or just before the
 *     last sample is not taken); it is kept so that numbers compare with the literature.
 *  2. Window: w[n] = 0.5 (1 - cos(2 pi (n + 1) / (W + 1))), n = 0 .. W - 1; c = w x_frame, p = w y_frame.
 *  3. Segmental SNR of a frame: 10 log10(sum c^2 / (sum (c - p)^2 + EPS) + EPS) clamped to [-10, 35] dB; defined for every frame (a silent
 *     clean frame gives -10).
 *  4. LPC: r[k] = sum_n v[n] v[n + k], k = 0 .. P, for v = c and v = p.  A frame with r_c[0] <= 0 or r_p[0] <= 0 is VOID for LLR and CD (not
 *     for the segmental SNR).  Levinson-Durbin: a = (1, a_1 .. a_P), E_0 = r[0]; at order i = 1 .. P
 *       k_i = -(r[i] + sum_{j=1}^{i-1} a_j r[i-j]) / E   (j ascending, starting from r[i]),
 *       a_j += k_i a_{i-j} for all j < i at once,  a_i = k_i,  E *= 1 - k_i^2;
 *     the recursion stops before an order whose incoming E <= 2^-40 r[0], the remaining coefficients are 0.
 *  5. LLR of a frame: ln((a_p' R_c a_p) / (a_c' R_c a_c)), R_c = Toeplitz(r_c[0 .. P]), clamped to [0, 2].  A quadratic form is
 *     sum_i a_i (sum_j R_c[i][j] a_j), i and j ascending.
 *  6. CD of a frame: the cepstrum of 1 / A(z), c_1 = -a_1, c_n = -a_n - sum_{k=1}^{n-1} (k / n) c_k a_{n-k} for n <= P (k ascending);
 *     CD = (10 / ln 10) sqrt(2 sum_{n=1}^{P} (c_c[n] - c_p[n])^2) clamped to [0, 10] dB.
 *  7. Row values: the segmental SNR is the mean over the M frames (NaN for M = 0).  LLR and CD are each the mean of the
 *     n_keep = max(1, floor(0.95 M' + 0.5)) SMALLEST values among the M' frames that are not void - the published 95 % trim, n_keep in
 *     integer arithmetic as max(1, (19 M' + 10) / 20) - and NaN for M' = 0.  A clamp leaves a NaN a NaN; a frame whose LLR is NaN counts as void.
 *  Order of every sum (a row's numbers are the same bits alone, in any batch, at any batch width, row stride and position; no atomics):
 *   inside a frame, lane l of a wave of 64 adds the terms n = l, l + 64, ... in ascending order as fused multiply-adds from +0, then the 64
 *   lane sums are added in a butterfly (l with l ^ 32, ^ 16, ... ^ 1);  over a row, thread t of 256 adds the frames t, t + 256, ... in
 *   ascending order, the butterfly adds each wave's 64 sums, and the four wave sums are added in wave order.  The trimmed mean is
 *   (sum of the values below T in that order + (n_keep - their count) T) / n_keep, T the n_keep-th smallest value.  The recursions and the
 *   quadratic forms of steps 4 - 6 run in the order written there, every product and sum rounded on its own (not fused).
 *   One workgroup takes STORM_LPC_TILE consecutive frames of one row: the cut depends on the frame index only.
 *
 * storm_lpc_window (host): w of step 2 for fs in fp64 into the CALLER's host memory of `capacity` doubles; returns W, or < 0 when refused
 *   (fs, null pointer, capacity < W).  The caller copies the table to the device.
 * storm_lpc_measures_rows: x, y fp32 [B][L] at fs (row strides in floats), window = that table on the device -> out fp64 [B][3] =
 *   (segmental SNR, LLR, CD).  frames_out (optional): fp64 [B][M(L)][3], the per-frame values of steps 3, 5, 6; NaN past a row's own M and,
 *   in LLR and CD, for void frames.  row_len (optional, device int32 [B]): row b is its first row_len[b] samples (clipped to L), the rest
 *   is never read.
 *   scratch: at least storm_lpc_measures_scratch_bytes(B, L, fs) bytes of device memory (0: refused arguments), 8-byte aligned; after the
 *   call it begins with int32 [B][2] = (M, M') of every row.  The library allocates nothing. */
#define STORM_LPC_TILE 8
int storm_lpc_window(int fs, double* w, long long capacity);
long long storm_lpc_measures_scratch_bytes(int B, long long L, int fs);
int storm_lpc_measures_rows(const float* x, const float* y, const double* window, double* out, double* frames_out, void* scratch,
                            long long scratch_bytes, int B, long long L, long long stride_x, long long stride_y, const int* row_len, int fs,
                            storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * Long recordings: a recording longer than one window of W samples is enhanced as n overlapping windows (overlap V, 1 <= V <= W / 2, hop
 * H = W - V, window k starts at k H, n = ceil((L - V) / H)) and stitched back.  Output sample m < L of a recording:
 *   k = min(m / H, n - 1), j = m - k H, cur = window_k[j];
 *   k > 0 and j < V:  prev = window_{k-1}[j + H],  out = prev + ramp[j] * (cur - prev)   (three fp32 operations in this order, not contracted)
 *   otherwise:        out = cur.
 * A skipped window reads as zeros; samples from L up to `width` are zero.  Windows cut from a signal therefore stitch back to it bit for bit.
 *
 * storm_crossfade_ramp (host, no device): ramp[j], j = 0 .. V - 1, designed in fp64 and rounded to fp32 once into the CALLER's host memory
 *   of V floats; STORM_RAMP_HANN: sin(pi / 2 (j + 1) / (V + 1))^2, STORM_RAMP_LINEAR: (j + 1) / (V + 1).
 * storm_crossfade_rows: ONE launch stitches R recordings.  pool: the enhanced windows, fp32 [N][W] with row stride pool_stride; out fp32
 *   [R][width] with row stride out_stride; device int32 arrays: rec_len[R] (samples), rec_windows[R] (n_r, with (n_r - 1) H + V < rec_len[r]
 *   <= (n_r - 1) H + W, or n_r = 1 and rec_len[r] <= W), rec_first[R] (index of the recording's first entry in win_row) and
 *   win_row[sum n_r]: the pool row of every window in recording order, -1 for a skipped window; ramp: that table on the device.
 *   One workgroup computes STORM_CROSSFADE_TILE outputs of one recording; no atomics - an output's bits depend on its own recording's
 *   windows only. */
#define STORM_CROSSFADE_TILE 1024
enum { STORM_RAMP_HANN = 0, STORM_RAMP_LINEAR = 1 };
int storm_crossfade_ramp(int V, int kind, float* ramp);
int storm_crossfade_rows(const float* pool, int N, long long pool_stride, float* out, int R, long long width, long long out_stride,
                         const int* rec_len, const int* rec_windows, const int* rec_first, const int* win_row, int W, int V,
                         const float* ramp, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * Posterior ensembles: K draws of the sampler per utterance combined into one estimate, with a per-bin spread and per-row agreement
 * numbers.  The reference has no ensemble, so THIS TEXT is the specification; the numbers were checked against a float64 restatement of
 * it (tests/ensemble_cases.py).
 * pool: complex64 [N][F][T] (T fastest, row stride pool_stride in complex elements), sampler outputs in the model's TRANSFORMED domain.
 * draw_row: device int32 [B][K], the pool row of draw k of utterance b, every entry in [0, N), in any order (an entry outside the pool reads
 *   as zeros: the host cannot see the table, the kernel must still not read outside the pool).
 * frames (optional, device int32 [B]): the row's valid frame count; bins with t >= frames[b] are never read, out and spread are zeros there.
 * 1 <= K <= STORM_ENSEMBLE_MAX_DRAWS.
 * Per bin everything after the fp32 load is fp64, every product and sum rounded on its own (no contraction); |v|^2 of a complex v is
 * v_re v_re + v_im v_im, |v| its square root:
 *  1. Back-transform (data_module.py:188-193) of draw k, z_k = (re, im): r = sqrt(re re + im im); r == 0: x_k = 0.  Otherwise m_k = r / factor,
 *     g = m_k for e == 1, m_k m_k for e == 0.5, else pow(m_k, 1 / e); x_k = (g (re / r), g (im / r)) and |x_k| = g (taken as g, not formed
 *     again from x_k).  factor and e are the data module's fp32 values widened to fp64.
 *  2. Mean: c = (sum_k x_k) / K, k ascending from +0, real and imaginary part each.
 *  3. Combined value by mode - STORM_ENSEMBLE_MEAN: c;  STORM_ENSEMBLE_MAG_MEAN: a c / |c| with a = (sum_k |x_k|) / K (k ascending from +0);
 *     STORM_ENSEMBLE_MAG_MEDIAN: a c / |c| with a the median of the |x_k| - the middle order statistic, for even K half the sum of the two
 *     middle ones (0.5 (lower + upper)).  a c / |c| is (a (c_re / n), a (c_im / n)) with n = |c|; |c| == 0 gives 0 in the two magnitude
 *     modes.  out: complex64 [B][F][T] in the LINEAR STFT domain, rounded to fp32 once.
 *  4. Spread (optional, fp32 [B][F][T]): s = sqrt((sum_k |x_k - c|^2) / (K - 1)), k ascending from +0, as written (not E[x^2] - |c|^2);
 *     0 for K = 1.
 *  5. Row numbers: rows_out fp64 [B][2 + K] = (E, D, d_0 .. d_{K-1}) with E = sum over the valid bins of |c|^2, d_k = sum over the valid
 *     bins of |x_k - c|^2 and D = (sum_k d_k) / K (k ascending from +0).  best[b] (int32) = the k with the smallest d_k, the lowest k on a
 *     tie: the medoid draw.  10 log10(E / D) is the row's agreement in dB.
 *  6. Order of the row sums (a row's bits are the same alone, in any batch, at any pool stride and under any permutation of pool rows; no
 *     atomics): one workgroup takes STORM_ENSEMBLE_TILE consecutive bins of one row in i = f T + t order - the cut depends on the bin index
 *     only.  The tile's bins form pairs (2 p, 2 p + 1); thread l of 256 adds the valid bins of its pairs p = l, l + 256, ... in ascending
 *     bin order from +0 (lane-strided, ascending), the 64 lane sums of a wave are added in a butterfly (l with l ^ 32, ^ 16, ... ^ 1) and
 *     the four wave sums in wave order - the orders of the frame-based measures above.  A second kernel adds a row's tile partials in tile
 *     order from +0.
 *
 * storm_ensemble_combine_rows: out, and optionally spread, as above; scratch: at least storm_ensemble_scratch_bytes(B, F, T, K) bytes of
 *   device memory (0: refused arguments), 8-byte aligned, the tile partials.  pool and out are 16-byte aligned.  Refused: null pointers (spread
 *   and frames may be null), B, F, T, N < 1 (B <= 65535, F T < 2^31), K outside 1 .. STORM_ENSEMBLE_MAX_DRAWS, pool_stride < F T, a pool or
 *   out that is not 16-byte aligned, scratch too small or misaligned, an unknown mode, factor or exponent <= 0.  The library allocates nothing. */
#define STORM_ENSEMBLE_MAX_DRAWS 32
#define STORM_ENSEMBLE_TILE 1024
enum { STORM_ENSEMBLE_MEAN = 0, STORM_ENSEMBLE_MAG_MEAN = 1, STORM_ENSEMBLE_MAG_MEDIAN = 2 };
long long storm_ensemble_scratch_bytes(int B, int F, int T, int K);
int storm_ensemble_combine_rows(const float* pool, int N, long long pool_stride, const int* draw_row, float* out, float* spread,
                                double* rows_out, int* best, void* scratch, long long scratch_bytes, int B, int K, int F, int T,
                                const int* frames, float factor, float exponent, int mode, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * Misaligned audio (the reference's util/other.py: align :153-157, hp_filter :76-80).  Every scoring entry point above assumes that its
 * rows are sample-aligned; these find a delay, undo it and remove rumble without leaving the device.
 *
 * Delay search.  A row is ny samples of y and nr samples of ref (fp32).  The full cross-correlation at lag d is
 *   c[d] = sum_n (double) y[n] * (double) ref[n + d],   n ascending from max(0, -d) to min(ny, nr - d) - 1,
 *   d from max(-(ny - 1), -max_lag) to min(nr - 1, max_lag); max_lag < 0: unbounded (the reference's behaviour).
 * A product of two fp32 values is exact in fp64, and c[d] is ONE fp64 chain in ascending n that starts at +0 (fused or unfused multiply-add:
 * the same bits).  lag = the SMALLEST d at which c[d] is maximal (np.argmax's first index: an all-zero row gives the smallest d of the
 * range), peak = c[lag].  The reference's align() rolls y by l = argmax(fftconvolve(ref, flip(y))) - (nr - 1): entry i of that convolution is
 * c[i - (ny - 1)], so l = lag + ny - nr, which is lag for ny == nr.  Samples are expected finite.
 *
 * storm_xcorr_num_partials: scratch entries per row (STORM_XCORR_PARTIAL_BYTES each) for rows of Ny / Nr samples: the lag tiles of
 *   STORM_XCORR_TILE consecutive lags (0: refused - a width < 1 or > 2^30).
 * storm_xcorr_lag_rows: y fp32 [B][Ny], ref fp32 [B][Nr] (row strides in floats) -> lag int32 [B], peak fp64 [B].  y_len / ref_len (optional,
 *   device int32 [B]): row b is its first y_len[b] / ref_len[b] samples, the rest is never read (a length < 1: lag 0, peak 0).  Two launches:
 *   a workgroup owns one tile of lags and walks the tile's whole n range (no split over n, so no partial sums of a lag exist) and writes
 *   the tile's (max, smallest lag) to scratch - the tiles with the longest overlaps are started first, and a thread keeps 8, 4 or 2
 *   consecutive lags by the size of the launch (no bit depends on that choice); one thread per row then takes the
 *   row's tiles in ascending order, replacing on strictly greater.  No atomics: a row's two outputs are the same bits alone, in any batch,
 *   at any width, stride and position.  scratch: B * storm_xcorr_num_partials(Ny, Nr, max_lag) * STORM_XCORR_PARTIAL_BYTES bytes of device
 *   memory, 8-byte aligned.
 *
 * storm_shift_rows: out[b][n] = x[b][(n - s) mod len] when wrap (np.roll(x, s) of the row's len samples), else x[b][n - s] where
 *   0 <= n - s < len and 0 elsewhere; s = shift[b] is read from DEVICE memory (int32 [B], any value: a lag goes in as it came out);
 *   samples from len up to N are written as zeros.  row_len optional as above.  Not in place.
 *
 * storm_sosfilt_rows: scipy.signal.sosfilt with zero initial state on every row.  sos: HOST fp64 [S][6] = (b0, b1, b2, a0 = 1, a1, a2) per
 *   section, 1 <= S <= STORM_SOS_MAX_SECTIONS.  Per sample n, for each section s in order, xc starting as (double) x[n]:
 *     xn = b0 xc + z0;   z0 = b1 xc - a1 xn + z1;   z1 = b2 xc - a2 xn;   xc = xn
 *   evaluated in exactly that order in fp64, every multiply and add rounded separately (never contracted), subnormals kept.  out: fp64
 *   [B][L], or fp32 (that value rounded once) when out_f32; row strides in elements of their own type; samples from row_len[b] up to L are
 *   written as zeros.  Rows are independent; the sections of a row overlap as a pipeline across lanes, which changes no bit.
 * storm_butter_sos (host, no device): the sections of scipy.signal.butter(order, wn, 'hp' | 'lp', output='sos') for an EVEN order, in closed
 *   form in fp64 into the CALLER's order / 2 * 6 doubles: the prototype's poles -exp(j pi m / (2 order)), pre-warped with 4 tan(pi wn / 2),
 *   lp2hp (highpass != 0) or lp2lp, the bilinear transform at fs = 2, conjugate poles paired, the pair nearest the unit circle last, the
 *   whole gain in the first section's numerator g [1, -2, 1] (low-pass: g [1, 2, 1]).  Agrees with scipy to a few units in the last place
 *   (another libm's tan / cos).  Refused: an odd order, order outside [2, 2 STORM_SOS_MAX_SECTIONS], wn outside (0, 1). */
#define STORM_XCORR_TILE 512
#define STORM_XCORR_PARTIAL_BYTES 16
#define STORM_SOS_MAX_SECTIONS 16
int storm_xcorr_num_partials(long long Ny, long long Nr, int max_lag);
int storm_xcorr_lag_rows(const float* y, const float* ref, int* lag, double* peak, void* scratch, long long scratch_bytes, int B,
                         long long Ny, long long Nr, long long stride_y, long long stride_ref, const int* y_len, const int* ref_len,
                         int max_lag, storm_stream_t st);
int storm_shift_rows(const float* x, float* out, const int* shift, int B, long long N, long long stride_x, long long stride_out,
                     const int* row_len, int wrap, storm_stream_t st);
int storm_sosfilt_rows(const float* x, void* out, const double* sos, int S, int B, long long L, long long stride_x, long long stride_out,
                       const int* row_len, int out_f32, storm_stream_t st);
int storm_butter_sos(int order, double wn, int highpass, double* sos_out);

/* ------------------------------------------------------------------------------------------
 * BSS-eval SDR: the signal-to-distortion ratio that allows the estimate a short linear FILTER of the reference (Vincent, Gribonval,
 * Fevotte 2006; what mir_eval.separation.bss_eval_sources and fast_bss_eval call SDR), where SI-SDR allows a gain and the alignment above a
 * gain and one integer delay.  The reference project does not compute it, so this comment is the specification.
 *
 * Per row: reference s[0..L), estimate e[0..L), both fp32; filter length F = flen, 1 <= F <= STORM_BSS_MAX_TAPS.
 *
 * Correlations.
 *   G[k] = sum_n (double) s[n] * (double) s[n + k],   k = 0 .. F - 1,   n = 0 .. L - 1 - k   (an empty sum is 0)
 *   D[k] = sum_n (double) s[n] * (double) e[n + k]
 *   Ee   = sum_n (double) e[n]^2
 * A product of two fp32 values is exact in fp64.  The order of summation is fixed by the sample index alone: n is cut into pieces of
 * STORM_BSS_PIECE samples (the cut of storm_energy_ratios_rows); a term belongs to the piece of the index of its FIRST factor s[n] (of
 * e[n] for Ee) - s[n + k] / e[n + k] may lie in the next piece; inside a piece every G[k], D[k] and Ee is ONE fp64 chain in ascending n
 * that starts at +0 (fused or unfused multiply-add: the same bits); the pieces are then added in ascending order from +0.  No atomics:
 * these 2 F + 1 numbers are the same bits for a row alone, in any batch, at any width, stride and position, and np.cumsum per lag and
 * piece reproduces them bit for bit.
 *
 * Filter.  C solves Toeplitz(G) C = D by the Levinson-Durbin recursion in fp64 (Golub & Van Loan alg. 4.7.3, the algorithm behind
 * scipy.linalg.solve_toeplitz):
 *   a = [1], E = G[0], C[0] = D[0] / E
 *   for m = 1 .. F - 1:
 *       lam = -(sum_{i<m} a[i] G[m - i]) / E
 *       a[i] <- a[i] + lam a[m - i]      (i = 0 .. m, a[m] = 0 before)
 *       E <- E (1 - lam^2)
 *       mu = (D[m] - sum_{i<m} C[i] G[m - i]) / E
 *       C[i] <- C[i] + mu a[m - i]       (i = 0 .. m, the new a)
 * Every multiply-add is a fused one.  The two dot products of order m are summed in a shape that depends on m only: entry i belongs to
 * lane i mod 64 of one wave, a lane adds its entries i < m as one fma chain in ascending i from +0, and the 64 lane sums are added by the
 * xor butterfly 32, 16, 8, 4, 2, 1.  Fixed, so rows stay batch-independent; NOT pinned to numpy bit for bit.
 *
 * Result.  P = sum_k D[k] C[k] (the same shape) and sdr = 10 log10(P / (Ee - P)): the energy of the projection of the zero-padded estimate
 * onto the span of the F delayed copies of the reference over the energy of what is left of it (||e - proj||^2 = Ee - P: the projection is
 * orthogonal).  This is mir_eval.separation.bss_eval_sources(s[None], e[None])[0] with exact linear correlations; mir_eval takes its
 * correlations from an FFT of length 2^ceil(log2(L + 512)), which wraps for some L - its artefact, not part of this definition.  F = 1 is
 * SI-SDR without its eps.  argmax |C| is the delay the alignment above would find.
 *
 * Edge rules.  Ee - P <= 0: +inf.  Trust range: at an SDR of x dB the difference Ee - P carries a relative error of about
 * 10^(x / 10) * 1e-15, so the number means something up to roughly 100 dB (an exactly filtered row measured Ee - P = -1e-10 at
 * Ee = 5.5e4).  P <= 0 with Ee - P > 0: -inf.  NaN: a row of fewer than 1 sample, G[0] == 0, Ee == 0, or an E that is <= 0 or not finite
 * at some order - a reference whose F delays are numerically dependent; mir_eval falls back to a least-squares solve there, this refuses
 * by NaN.  No diagonal loading is applied (band-limited references down to min E / G[0] = 5e-5 solve to the same SDR as a dense solver).
 * The filter of a NaN row is NaN; the correlations of a row of fewer than 1 sample are zeros.  Samples are expected finite.
 * SIR / SAR against a noise reference: storm_bss_eval_rows below.  Out of scope: a time-varying filter, permutations of several sources.
 *
 * storm_bss_sdr_scratch_bytes: device scratch for rows of L samples: B * ceil(L / STORM_BSS_PIECE) * (2 flen + 1) doubles (0: refused -
 *   B outside 1 .. 65535, L outside 1 .. 2^30, flen outside 1 .. STORM_BSS_MAX_TAPS).
 * storm_bss_sdr_rows: ref, est fp32 [B][L] (row strides in floats) -> sdr fp64 [B]; filt (optional) fp64 [B][flen] = C; parts (optional)
 *   fp64 [B][2 flen + 1] = G, D, Ee.  row_len (optional, device int32 [B]): row b is its first row_len[b] samples, the rest is never read.
 *   Two launches: a workgroup per (row, piece) computes the piece's 2 flen + 1 chains together - a thread keeps 8, 4 or 2 consecutive lags
 *   of both banks by the size of the launch (no bit depends on that choice) - and writes them to scratch; one wave per row then adds the
 *   pieces, runs the recursion and forms the number.  scratch: 8-byte aligned device memory of at least the query's answer. */
#define STORM_BSS_MAX_TAPS 512
#define STORM_BSS_PIECE 16384
long long storm_bss_sdr_scratch_bytes(int B, long long L, int flen);
int storm_bss_sdr_rows(const float* ref, const float* est, double* sdr, double* filt, double* parts, void* scratch, long long scratch_bytes,
                       int B, long long L, long long stride_ref, long long stride_est, const int* row_len, int flen, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * BSS-eval SDR, SIR and SAR with two sources (bss_eval_sources of Vincent, Gribonval, Fevotte 2006 for target and noise): the distortion
 * of an estimate that may be a FILTERED mixture is split into "noise that is left" (SIR) and "what the system invented" (SAR).  This is
 * BSS-eval's split: the projection onto the delayed copies of BOTH sources is JOINT, and SAR's numerator is s_target + e_interf.  It is NOT
 * the reference project's si_sir / si_sar (storm_energy_ratios_rows), which use two separate one-tap projections and put the target alone in
 * SAR's numerator, and so book any filter as interference and artefacts.  The reference project does not compute it: this comment is the
 * specification.
 *
 * Per row: target s1[0..L), interferer s2[0..L), estimate e[0..L), all fp32; F = flen, 1 <= F <= STORM_BSS_MAX_TAPS.
 *
 * Correlations, for k = 0 .. F - 1:
 *   G11[k] = sum s1[n] s1[n + k]     D1[k] = sum s1[n] e[n + k]
 *   G22[k] = sum s2[n] s2[n + k]     D2[k] = sum s2[n] e[n + k]
 *   X12[k] = sum s1[n] s2[n + k]     X21[k] = sum s2[n] s1[n + k]        Ee = sum e[n]^2
 * every one summed exactly as above: exact fp64 products, pieces of STORM_BSS_PIECE samples cut by the index of the FIRST factor, inside a
 * piece one ascending fp64 chain from +0, the pieces added in order, no atomics.  These 6 F + 1 numbers are, bit for bit, what four calls of
 * storm_bss_sdr_rows return as parts: (ref, est) = (s1, e), (s2, e), (s1, s2), (s2, s1).  parts is fp64 [B][6 F + 1] in the order
 * G11, D1, G22, D2, X12, X21, Ee.
 *
 * Joint system.  The unknowns are interleaved, x = (c1[0], c2[0], c1[1], c2[1], ..).  M is 2 F x 2 F, symmetric, block-Toeplitz with 2 x 2
 * blocks:
 *   block(k, l) = R(k - l)     R(m) = [[G11[|m|], c12(m)], [c12(-m), G22[|m|]]]     c12(m) = X12[m] for m >= 0, X21[-m] for m < 0
 * - the Gram matrix of the 2 F zero-padded delayed copies.  d = (D1[0], D2[0], D1[1], ..).  M x = d is solved in fp64 and P12 = d . x.
 * P1 = D1 . C1 with Toeplitz(G11) C1 = D1 is the single-source projection above, by the same recursion in the same summation shape.
 *
 * The solve is the block Levinson recursion (Whittle 1963; Wiggins & Robinson 1965) with 2 x 2 blocks: forward predictor A, backward
 * predictor B (kept reversed, Bt_j = B_{m - j}), symmetric 2 x 2 error matrices Ef, Eb, all starting from I and R(0); x[0] = R(0)^-1 d[0].
 *   for m = 1 .. F - 1:
 *       Delta = sum_{j<m} R(m - j) A_j          delta = sum_{j<m} R(m - j) x_j
 *       Kf = -Eb^-1 Delta                       Kb = -Ef^-1 Delta^T
 *       A_j <- A_j + Bt_{m-j} Kf                Bt_j <- Bt_j + A_{m-j} Kb         (j = 0 .. m, the old values on the right)
 *       Ef <- Ef + Delta^T Kf                   Eb <- Eb + Delta Kb               (the two off-diagonal entries averaged)
 *       g = Eb^-1 (d[m] - delta)                x_j <- x_j + Bt_{m-j} g           (the new Eb and Bt)
 * A 2 x 2 matrix [[a, b], [b, c]] is inverted through l = b / a, p = c - l b (its pivots a and p).  Every multiply-add is a fused one; the
 * six sums of an order have the shape of the recursion above: block j in lane j mod 64 of one wave, a lane's blocks j < m as fma chains in
 * ascending j from +0 (inside a block first the column of s1, then that of s2), then the xor butterfly 32 .. 1.  Fixed, so rows stay
 * batch-independent; pinned by bounds against dense solvers, NOT bit for bit.  This recursion was built, and not a blocked Cholesky of the
 * dense matrix in global scratch, because it meets the bound (1e-4 dB against two dense host solvers up to a joint condition of 1e8) inside
 * one wave's registers and 56 KB of LDS.
 *
 * Numbers (out fp64 [B][3]):
 *   sdr = 10 log10(P1 / (Ee - P1))      the SAME BITS as storm_bss_sdr_rows(s1, e)
 *   sir = 10 log10(P1 / (P12 - P1))
 *   sar = 10 log10(P12 / (Ee - P12))
 * Edge rules.  P12 - P1 <= 0 with P1 > 0: sir = +inf (P1 <= 0 then: NaN; P1 <= 0 otherwise: -inf).  Ee - P12 <= 0: sar = +inf (else
 * P12 <= 0: -inf).  Whatever makes the SDR above NaN makes all three NaN.  G22[0] == 0 (a silent noise row): sir and sar are NaN, sdr is still
 * given.  A joint system that is numerically dependent - a pivot a or p of Ef or Eb that is <= 0 or not finite at some order, e.g. a noise row
 * that is a multiple or a filtered copy of the target - : sir and sar are NaN; no diagonal loading, no least-squares fallback.  A row of
 * fewer than F + 1 samples is always dependent (2 F zero-padded copies in L + F - 1 dimensions) and is refused the same way by its length,
 * not by the rounding of a pivot that is zero in exact arithmetic; its sdr is still given.  filt
 * (optional) fp64 [B][2][F] = c1, c2 of the joint solve, NaN where sir is NaN.  The correlations of a row of no samples are zeros.
 * Out of scope: permutations of several sources, a time-varying filter.
 *
 * storm_bss_eval_scratch_bytes: 4 x storm_bss_sdr_scratch_bytes(B, L, flen) + 8 B bytes (0: refused, as there).
 * storm_bss_eval_rows: three launches - the four pairs' correlations as one grid (a workgroup per (pair, row, piece), the walk of
 *   storm_bss_sdr_rows), that entry's solve for sdr and P1, one wave per row for the joint recursion.  Strides in floats, row_len and scratch
 *   as above. */
long long storm_bss_eval_scratch_bytes(int B, long long L, int flen);
int storm_bss_eval_rows(const float* target, const float* noise, const float* est, double* out, double* filt, double* parts, void* scratch,
                        long long scratch_bytes, int B, long long L, long long stride_t, long long stride_n, long long stride_e,
                        const int* row_len, int flen, storm_stream_t st);

/* ------------------------------------------------------------------------------------------
 * ConvTasNet (backbones/convtasnet.py): the time-domain denoiser.  Activations are channels-last [B][L][C] in `dtype`
 * (C % 8 == 0); the TCN's running sums `output` / `skip_connection` are fp32 [B][L][BN]; statistics are fp32.  A global layer
 * norm (GroupNorm(1, C, eps) over all of C x L of a row) is never materialised: the producing kernel writes per-wave
 * (sum, sumsq) partials, storm_tasnet_gln_finalize turns them into stats[B][2] = (mean, rstd), the consumer applies
 * (x - mean) * rstd * gamma_c + beta_c while it loads its operand.
 * ------------------------------------------------------------------------------------------ */
enum { STORM_TASNET_ENCODE = 0, STORM_TASNET_POINTWISE = 1, STORM_TASNET_DEPTHWISE = 2 };
/* partial-sum slots per row that the kernel `op` (above) writes for L frames of C output channels: part = fp32 [B][slots][2] */
int storm_tasnet_num_partials(int op, int L, int C);
/* pad_signal (convtasnet.py:75-94) + Conv1d(1, N, win, stride = win / 2, bias=False): wav fp32 [B][T] (row stride wav_stride)
 * -> enc [B][L][N], L = storm_tasnet_frames(T, win); wT = the weight transposed, fp32 [win][N]; part: the partials for TCN.LN. */
int storm_tasnet_frames(long long T, int win);
int storm_tasnet_encode(const float* wav, long long wav_stride, const float* wT, void* enc, float* part, int B, long long T,
                        int N, int win, int dtype, storm_stream_t s);
int storm_tasnet_gln_finalize(const float* part, float* stats, int B, int nparts, long long count, float eps, storm_stream_t s);
/* 1x1 convolution as an MFMA GEMM: out[b][l][co] = sum_ci w[co][ci] * pre(x[b][l][ci]) + bias[co].
 *   x: [B][L][Cin] in dtype, or fp32 when x_f32 (a running sum; rounded to dtype as it is loaded); w: [Cout][Cin] in dtype.
 *   pre: norm_stats != NULL: the norm-apply with gamma / beta fp32 [Cin]; else prelu_in != NULL: PReLU with the scalar slope
 *        *prelu_in; else none.
 *   res_skip == 0: out [B][L][Cout] (fp32 when out_f32), after the scalar PReLU *prelu_out when given; part != NULL: partials
 *        of the stored values for the next norm.
 *   res_skip != 0: res_out and skip_out as ONE GEMM, w = cat[res_out.weight, skip_out.weight] ([Cout = 2 BN][Cin]): columns
 *        [0, BN) are added to out = `output`, columns [BN, 2 BN) to skip = `skip_connection`, both fp32 [B][L][BN], in place. */
int storm_tasnet_pointwise(const void* x, int x_f32, const void* w, const float* bias, void* out, int out_f32, float* skip,
                           int res_skip, const float* norm_stats, const float* gamma, const float* beta, const float* prelu_in,
                           const float* prelu_out, float* part, int B, int L, int Cin, int Cout, int dtype, storm_stream_t s);
/* Conv1d(C, C, 3, dilation = padding = d, groups = C) on the norm-applied x, + bias, scalar PReLU, partials of the next norm.
 * w3 = the weight transposed, fp32 [3][C].  The zero padding follows the norm: a tap outside [0, L) adds 0; d >= L leaves the
 * centre tap. */
int storm_tasnet_depthwise(const void* x, const float* w3, const float* bias, const float* norm_stats, const float* gamma,
                           const float* beta, const float* prelu, void* out, float* part, int B, int L, int C, int dilation,
                           int dtype, storm_stream_t s);
/* sigmoid(mask) * enc, then ConvTranspose1d(N, 1, win, stride = win / 2, bias=False) as a gather (no atomics): mask, enc
 * [B][L][N]; wd fp32 [N][win]; out fp32 [B][(L - 1) * stride + win] - the padded length, untrimmed as the reference returns it. */
int storm_tasnet_decode(const void* mask, const void* enc, const float* wd, float* out, int B, int L, int N, int win, int dtype,
                        storm_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Program interpreter: runs a whole NCSN++ forward (or any op list) with one host call.
 * The op list is planned on the host side (csrc/ncsnpp_graph.hip) once per
 * (model, B, F, T, dtype); pointers are offsets into the caller-owned buffers in `bufs`.
 * Replaces the Python op-by-op dispatch of NCSNpp.forward (ncsnpp.py:281-450).
 * ------------------------------------------------------------------------------------------ */
/* The slots of an op by code (csrc/op_fields.h names them; callers that read records by number - bench.py, tools/, tests/ - rely on them):
 * a reference that is absent has buf < 0, an unused integer or float is 0. */
enum {
    STORM_OP_MEMSET = 0,            /* p[0] dst; i = bytes (set to zero) */
    STORM_OP_PACK_INPUT = 1,        /* p[0..2] complex inputs, p[3] out; i = n_in, B, F, T (storm_pack_input) */
    STORM_OP_TEMB = 2,              /* p[0] t, p[1] gfp_W, p[2] W1, p[3] b1, p[4] W2, p[5] b2, p[6] act_temb; i = B, nf (storm_time_embedding) */
    STORM_OP_DENSE = 3,             /* p[0] x, p[1] W, p[2] bias, p[3] out; i = B, N, K (storm_dense) */
    STORM_OP_CONV = 4,              /* p[0..2] segment 0's src_a, src_b, w, p[3..5] segment 1's, p[6] out, p[7] bias, p[8] tbias, p[9] skip, p[10] gn_part,
                                     * p[11] segment 0's gn_ss, p[12] split-K scratch; i = nseg, B, H, W, outC, Cout, tbias_stride, out_f32, then per segment
                                     * (i[8..14], i[15..21]) Ca, Cb, CinP, w_rows, ntaps, w_bstride, w_tapstride, i[22] segment 0's bstride_a (< 0: H W Ca),
                                     * i[23] out_bstride (< 0: H W outC); f = scale, segment 0's gn_silu, fp32 slabs in the scratch (storm_conv) */
    STORM_OP_GN_STATS = 5,          /* p[0] xa, p[1] xb, p[2] stats; i = Ca, Cb, B, HW, groups (storm_gn_stats) */
    STORM_OP_GN_APPLY = 6,          /* p[0] xa, p[1] xb, p[2] stats, p[3] gamma, p[4] beta, p[5] out_act, p[6] out_raw; i = Ca, Cb, B, H, W, groups, silu, resample;
                                     * f = eps (storm_gn_apply) */
    STORM_OP_FIR_UP = 7,            /* p[0] x, p[1] add, p[2] out; i = B, H, W, C (storm_fir_up2) */
    STORM_OP_FIR_DOWN = 8,          /* p[0] x, p[1] out; i = B, H, W, C (storm_fir_down2) */
    STORM_OP_SOFTMAX = 9,           /* p[0] scores, p[1] probs; i = rows, L, ld (storm_softmax_rows) */
    STORM_OP_OUTPUT_HEAD = 10,      /* p[0] pyr, p[1] t, p[2] W, p[3] bias, p[4] out; i = cin, B, F, T, negate (storm_output_head) */
    STORM_OP_GN_FINALIZE = 11,      /* p[0] part_a, p[1] part_b, p[2] stats, p[3] gamma, p[4] beta, p[5] ss; i = Ca, tiles_a, Cb, tiles_b, B, groups, count; f = eps
                                     * (p[5] present: storm_gn_finalize_ss, else storm_gn_finalize, which reads neither gamma, beta, count nor eps) */
    STORM_OP_ATTENTION = 12,        /* p[0] q, p[1] k, p[2] vT, p[3] bias, p[4] out, p[5] scratch; i = B, L, C, ldv, scratch_bytes; f = scale (storm_attention_ws) */
    STORM_OP_INPUT_PYRAMID = 13,    /* p[0..2] complex inputs (or none: level 0 is read), p[3..6] levels; i = n_in, B, F, T, n_levels, mean, centered */
    STORM_OP_OUTPUT_PYRAMID = 14,   /* p[0..7] ph (finest first), p[8] t, p[9] W, p[10] bias, p[11] out; i = cin, B, F, T, negate, n_levels */
    STORM_OP_COMBINE_CAT = 15       /* p[0] x, p[1] w, p[2] bias, p[3] h, p[4] out; i = npix, C, CinP (storm_combine_cat) */
};
#define STORM_OP_NPTR 13
#define STORM_OP_NINT 24
#define STORM_OP_NFLT 4
typedef struct storm_ref { int32_t buf; int32_t pad_; int64_t off; } storm_ref; /* buf<0: NULL; byte offset */
typedef struct storm_op {
    int32_t code;
    int32_t pad_;
    storm_ref p[STORM_OP_NPTR];
    int64_t i[STORM_OP_NINT];
    float f[STORM_OP_NFLT];
} storm_op;

/* ops: host array; bufs: host array of n_bufs device base pointers.                       */
int storm_program_run(const storm_op* ops, int n_ops, void* const* bufs, int n_bufs, int dtype,
                      storm_stream_t s);
/* Same, but brackets every op with HIP events on stream `s`, synchronises, and writes the
 * elapsed milliseconds of each op to the HOST array ms[n_ops] (bench.py's roofline leg).    */
int storm_program_run_timed(const storm_op* ops, int n_ops, void* const* bufs, int n_bufs,
                            int dtype, storm_stream_t s, float* ms);
/* name of the kernel op k of a program launches (STORM_OP_CONV ops; "" otherwise), see storm_conv_kernel_name */
const char* storm_program_kernel_name(const storm_op* ops, int k, int dtype);

/* ------------------------------------------------------------------------------------------
 * Whole-network entry points: NCSN++ as ONE object of the C ABI (a host in any language builds it from the reference's
 * state_dict tensors and evaluates the score with one call; the Python class storm_amd.backbones.NCSNpp is a thin caller).
 * Replaces NCSNpp.__init__ / load_state_dict (ncsnpp.py:38-273) and NCSNpp.forward (ncsnpp.py:281-450) for the
 * configuration family of the StoRM hot path (BigGAN blocks, FIR resampling, output_skip / input_skip pyramids, Fourier
 * time embedding, swish); the _ex forms below take the constructor's other options (fir=False, skip_rescale=False, progressive /
 * progressive_input = 'none', progressive_combine='cat', centered, conditional, scale_by_sigma) and say what stays refused and why.
 * ------------------------------------------------------------------------------------------ */
typedef struct storm_ncsnpp_config {
    int nf;                     /* base width (128)                                                  */
    int n_levels;               /* len(ch_mult)                                                      */
    int ch_mult[8];             /* (1, 2, 2, 2); ncsnpplarge (1, 1, 2, 2, 2, 2, 2)                    */
    int num_res_blocks;
    int n_attn;
    int attn_resolutions[4];    /* frequency heights that get an AttnBlockpp ((0,) = bottleneck only)  */
    int image_size;             /* 256                                                               */
    int input_channels;         /* real channels of the score net input: 4 (x, y) or 6 (x, y, y_den)   */
    int discriminative;         /* predictive denoiser: 2 channels, no time conditioning, no 1/t       */
} storm_ncsnpp_config;
typedef struct storm_ncsnpp storm_ncsnpp;
/* The extended description: the graph-shaping options of the reference constructor (ncsnpp.py:40-147) beyond the StoRM default set.
 * struct_size = sizeof(storm_ncsnpp_config_ex) as the caller compiled it (another size: STORM_ERR_INVALID, nothing is read past it).
 * STORM_NCSNPP_CONFIG_EX_DEFAULTS fills the options with the reference's defaults - with them every _ex entry point below is its plain
 * namesake.  Still refused (STORM_ERR_INVALID at the Python surface: NotImplementedError): resblock_type='ddpm' and progressive /
 * progressive_input = 'residual' (FIR fused into a strided / transposed 3x3 convolution: a kernel family of its own), nonlinearity other
 * than swish (SiLU is fused into the convolutions' operand rewrite), fir_kernel other than [1,3,3,1], spatial_channels other than 1,
 * embedding_type='positional' (the reference's own forward reads self.sigmas, which NCSNpp never defines: ncsnpp.py:304-308), and
 * fir=False together with progressive='output_skip' (the reference itself fails there: layerspp.py:117 passes 'nearest' as scale_factor). */
typedef struct storm_ncsnpp_config_ex {
    int struct_size;
    int nf, n_levels, ch_mult[8], num_res_blocks, n_attn, attn_resolutions[4], image_size, input_channels, discriminative;   /* as above */
    int fir;                    /* 1: FIR [1,3,3,1] resampling; 0: nearest x2 / 2x2 mean (layerspp.py:246-258, 151-156); needs progressive == 0 */
    int skip_rescale;           /* 1: (x + h) / sqrt(2) after the residual adds; 0: x + h (layerspp.py:88-91, 271-274)            */
    int progressive;            /* 1: 'output_skip'; 0: 'none' - head = GroupNorm, act, conv3x3 (ncsnpp.py:258-263, 430-436)       */
    int progressive_input;      /* 1: 'input_skip'; 0: 'none' - no input pyramid, no Combine modules                             */
    int combine_cat;            /* 0: Combine 'sum'; 1: 'cat' - the following widths double (ncsnpp.py:204-207)                   */
    int centered;               /* 1: no 2x - 1 at the input (ncsnpp.py:325-327)                                                 */
    int conditional;            /* 0: no time embedding into the blocks (ncsnpp.py:317-323); forced 0 when discriminative          */
    int scale_by_sigma;         /* 0: no division by t at the head (ncsnpp.py:438-440); forced 0 when discriminative              */
} storm_ncsnpp_config_ex;
#define STORM_NCSNPP_CONFIG_EX_DEFAULTS(c) do { (c)->struct_size = (int)sizeof(storm_ncsnpp_config_ex); (c)->fir = 1; (c)->skip_rescale = 1; \
    (c)->progressive = 1; (c)->progressive_input = 1; (c)->combine_cat = 0; (c)->centered = 0; (c)->conditional = 1; (c)->scale_by_sigma = 1; } while (0)
/* NCSNpp.__init__ / load_state_dict / forward (ncsnpp.py:38-273, 281-450) for every accepted option set: */
int storm_ncsnpp_num_tensors_ex(const storm_ncsnpp_config_ex* cfg);
int storm_ncsnpp_tensor_info_ex(const storm_ncsnpp_config_ex* cfg, int i, char* name, int name_len, int* ndim, long long* shape4);
long long storm_ncsnpp_arena_bytes_ex(const storm_ncsnpp_config_ex* cfg, int dtype);
int storm_ncsnpp_create_ex(const storm_ncsnpp_config_ex* cfg, const void* const* weights, int n_weights, int dtype, void* arena,
                           storm_stream_t s, storm_ncsnpp** out);

/* the reference state_dict of this configuration: count, then (name, shape) of tensor i in the reference's order */
int storm_ncsnpp_num_tensors(const storm_ncsnpp_config* cfg);
int storm_ncsnpp_tensor_info(const storm_ncsnpp_config* cfg, int i, char* name, int name_len, int* ndim, long long* shape4);
long long storm_ncsnpp_arena_bytes(const storm_ncsnpp_config* cfg, int dtype);
/* weights[i] = device pointer to fp32 tensor i of the state_dict (contiguous).  Packs them (stream s) into the engine's
 * layout: arena = caller-owned device buffer of storm_ncsnpp_arena_bytes() or NULL (the handle allocates one). */
int storm_ncsnpp_create(const storm_ncsnpp_config* cfg, const void* const* weights, int n_weights, int dtype, void* arena,
                        storm_stream_t s, storm_ncsnpp** out);
void storm_ncsnpp_destroy(storm_ncsnpp* h);
/* A/B switches of the planner (all on by default): GroupNorm statistics from conv epilogues, GroupNorm apply in conv operand
 * loads, fused attention kernel */
int storm_ncsnpp_set_fusion(storm_ncsnpp* h, int fuse_stats, int fuse_apply, int fused_attention);
/* HIP-graph replay of this handle's evaluations (the reference's own operating point is ONE utterance per
 * call, enhancement.py:66-72, where an evaluation is ~120 short launches): mode 0 = eager launches, 1 = replay, -1 (default) = the
 * library's rule (today: eager - measured on MI355X the launch loop keeps the queue full at every batch size, profiles/r05a_*).  The first call per (shape, workspace address) runs eagerly, the second records the runs
 * of ops that touch only the workspace and the weights, later calls are one hipGraphLaunch per run + the three ops that read the
 * caller's tensors (input packing, time embedding, output head).  A replayed evaluation executes exactly the eager kernels with the
 * eager arguments: results are bit-identical.  A workspace passed to a graph-mode call must stay allocated while the handle lives
 * or until the same address is passed again (the recorded kernels point into it). */
int storm_ncsnpp_set_graph(storm_ncsnpp* h, int mode);
long long storm_ncsnpp_graph_launches(storm_ncsnpp* h);    /* hipGraphLaunch calls this handle has made (diagnostics: 0 = everything ran eagerly) */
/* bytes of scratch one forward at (B, F, T) needs (liveness-planned; 5.2 GB at B = 16, 256 x 512, bf16); -1 on error */
long long storm_ncsnpp_workspace_bytes(storm_ncsnpp* h, int B, int F, int T);
/* out[b] = dnn(cat[parts...], t) (negate != 0: its negative = the score, model.py:131-132).  parts: n device pointers to
 * complex64 [B][F][T]; t fp32 [B] (NULL when discriminative); out complex64 [B][F][T]; ws: >= workspace_bytes, pure scratch
 * (nothing is carried from one call to the next: one buffer sized for the largest shape serves every shape).
 * Threading: a handle may be shared by host threads that call with DIFFERENT streams and workspaces - the per-shape plan
 * cache is locked and bounded (64 shapes, least recently used out), `negate` is a per-call argument, the weights are read
 * only; storm_ncsnpp_set_fusion / _destroy must not race with calls. */
int storm_ncsnpp_forward(storm_ncsnpp* h, const void* const* parts, int n_parts, const float* t, void* out, void* ws,
                         long long ws_bytes, int B, int F, int T, int negate, storm_stream_t s);
/* GROUPED evaluation - P micro-batches of different (B_p, T_p) of one stream in ONE call (BASELINE.json configs[4]: 2 - 10 s utterances
 * bucketed by padded frame count are 2 - 3 rows per micro-batch; the reference processes one file per call, enhancement.py:66-72).  All
 * problems run the same op sequence; op k of every problem shares one launch where a grouped kernel exists (today: the 16-bit 3x3
 * convolutions with > 128 output channels - one persistent walk over all problems' pixel tiles), and runs problem by problem otherwise.
 * Every row computes what its own micro-batch's storm_ncsnpp_forward computes in the kernels that serve it (the tile choice and the K split
 * of few-tile layers follow the GROUP's tile count, so a 16-bit row agrees with its own call to the rounding of its activations; fp32: no
 * grouped kernel, bit-identical).  parts: P * n_parts pointers, problem-major; t / out: P pointers; ws >= _group_workspace_bytes(same list). */
long long storm_ncsnpp_group_workspace_bytes(storm_ncsnpp* h, int P, const int* B, const int* T, int F);
int storm_ncsnpp_forward_group(storm_ncsnpp* h, int P, const int* B, const int* T, int F, const void* const* parts, int n_parts,
                               const float* const* t, void* const* out, void* ws, long long ws_bytes, int negate, storm_stream_t s);
long long storm_ncsnpp_group_launches(storm_ncsnpp* h);    /* grouped kernel launches this handle has made (diagnostics: 0 = every op ran problem by problem) */
/* the planned op list of (B, F, T) (owned by the handle) for storm_program_run_timed / storm_program_kernel_name, the packed
 * arena, and the algorithmic FLOPs of one forward */
int storm_ncsnpp_program(storm_ncsnpp* h, int B, int F, int T, const storm_op** ops, int* n_ops, long long* flops);
/* a program handed out above stays valid (pinned) until the handle is destroyed or the caller releases it: */
int storm_ncsnpp_release_program(storm_ncsnpp* h, const storm_op* ops);
const void* storm_ncsnpp_arena(storm_ncsnpp* h);

#ifdef __cplusplus
}
#endif
#endif /* STORM_HIP_H */
