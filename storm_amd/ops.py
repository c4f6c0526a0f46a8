"""Tensor-level wrappers over the C ABI (one function per entry point of include/storm_hip.h).

Activations are NHWC tensors ``[B, H, W, C]`` (C % 8 == 0) in float32 or bfloat16; complex
spectrograms are complex64 ``[B, F, T]``.  These wrappers only marshal pointers/shapes and
enqueue on torch's current HIP stream; all compute happens in libstorm_hip.
"""
import ctypes as C
import math
import threading

import torch

from . import _lib as L


def _alloc(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------- weights -----------------
def pack_conv_weight(w, dtype, cout_pad=32):
    """nn.Conv2d weight [Cout, Cin, kh, kw] fp32 -> packed [taps][CoutP][CinP]."""
    Cout, Cin, kh, kw = w.shape
    ntaps = kh * kw
    per16 = 4 if dtype == torch.float32 else 8
    CoutP, CinP = round_up(Cout, cout_pad), round_up(Cin, per16 * 2)
    w = w.contiguous().float()
    out = _alloc((ntaps, CoutP, CinP), dtype, w)
    L.check(L.lib().storm_pack_conv_weight(L.ptr(w), L.ptr(out), Cout, Cin, ntaps, CoutP, CinP, L.dt(dtype), L.stream()),
            "storm_pack_conv_weight")
    return out


def pack_matrix(w, dtype, transpose=False, cout_pad=32):
    """[Cout][Cin] fp32 (or [Cin][Cout] with transpose=True, e.g. NIN.W) -> packed [CoutP][CinP]."""
    w = w.contiguous().float()
    Cin, Cout = (w.shape[0], w.shape[1]) if transpose else (w.shape[1], w.shape[0])
    per16 = 4 if dtype == torch.float32 else 8
    CoutP, CinP = round_up(Cout, cout_pad), round_up(Cin, per16 * 2)
    out = _alloc((1, CoutP, CinP), dtype, w)
    L.check(L.lib().storm_pack_matrix(L.ptr(w), L.ptr(out), Cout, Cin, int(transpose), CoutP, CinP, L.dt(dtype), L.stream()),
            "storm_pack_matrix")
    return out


# ---------------------------------------------------------------- conv / gemm -------------
class Seg:
    """One K-segment of storm_conv: activations (optionally the channel concat of two tensors)
    and packed weights [ntaps][rows][CinP] (or a per-batch activation used as the weight matrix)."""

    def __init__(self, src_a, w, ntaps, src_b=None, w_batched=False, src_bstride=None, gn_ss=None, gn_silu=True):
        self.src_a, self.src_b, self.w, self.ntaps = src_a, src_b, w, ntaps
        self.w_batched, self.src_bstride = w_batched, src_bstride
        self.gn_ss, self.gn_silu = gn_ss, gn_silu      # fused GroupNorm apply (+SiLU) on load


def _conv_args(segs, Cout, out=None, outC=None, bias=None, tbias=None, skip=None, scale=1.0, out_f32=False,
               B=None, H=None, W=None):
    """storm_conv_args for a convolution (+ the output tensor it points at)"""
    x = segs[0].src_a
    if B is None:
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
    dtype = x.dtype
    outC = outC if outC is not None else round_up(Cout, 8)
    if out is None:
        out = _alloc((B, H, W, outC), torch.float32 if out_f32 else dtype, x)
    a = L.ConvArgs()
    a.nseg = len(segs)
    for k, s in enumerate(segs):
        g = a.seg[k]
        g.src_a, g.Ca = L.ptr(s.src_a), s.src_a.shape[-1]
        g.bstride_a = s.src_bstride if s.src_bstride is not None else H * W * g.Ca
        if s.src_b is not None:
            g.src_b, g.Cb = L.ptr(s.src_b), s.src_b.shape[-1]
            g.bstride_b = H * W * g.Cb
        g.w, g.ntaps = L.ptr(s.w), s.ntaps
        g.CinP, g.w_rows = s.w.shape[-1], s.w.shape[-2]
        g.w_tapstride = s.w.shape[-1] * s.w.shape[-2]
        g.w_bstride = s.w.shape[-1] * s.w.shape[-2] if s.w_batched else 0
        if s.gn_ss is not None:
            g.gn_ss, g.gn_silu = L.ptr(s.gn_ss), int(s.gn_silu)
    a.B, a.H, a.W = B, H, W
    a.out, a.outC, a.Cout, a.out_bstride = L.ptr(out), outC, Cout, H * W * outC
    a.bias = L.ptr(bias)
    if tbias is not None:
        a.tbias, a.tbias_stride = L.ptr_rows(tbias), tbias.stride(0)
    if skip is not None:
        a.skip, a.skip_bstride = L.ptr(skip), H * W * outC
    a.scale, a.out_f32, a.dtype = scale, int(out_f32), L.dt(dtype)
    return a, out


def conv(segs, Cout, gn_partials=False, **kw):
    """out[b,h,w,co] = (sum_seg conv(seg) + bias + tbias[b] + skip) * scale   (storm_conv)."""
    a, out = _conv_args(segs, Cout, **kw)
    part = None
    if gn_partials:
        tiles = L.lib().storm_conv_tiles(C.byref(a))
        part = torch.zeros((a.B, tiles, a.outC, 2), dtype=torch.float32, device=out.device)
        a.gn_part = L.ptr(part)
    need = L.lib().storm_conv_splitk_bytes(C.byref(a))      # few-tile 3x3 layers: scratch for the split of K over workgroups
    if need > 0:
        ws = torch.empty((need,), dtype=torch.uint8, device=out.device)
        a.splitk_ws, a.splitk_ws_bytes = L.ptr(ws), need
    L.check(L.lib().storm_conv(C.byref(a), L.stream()), "storm_conv")
    return (out, part) if gn_partials else out


def conv_group(problems, Cout, gn_partials=False, bn=0):
    """ONE launch for several problems of one 3x3 layer (storm_conv_group): problems = [(segs, kw), ...] as conv() takes them, every
    problem with its own tensors / batch size / width and the same weights.  Returns the outputs (and GroupNorm partials) per problem."""
    P = len(problems)
    arr = (L.ConvArgs * P)()
    outs, parts, keep = [], [], []
    for p, (segs, kw) in enumerate(problems):
        a, out = _conv_args(segs, Cout, **kw)
        part = None
        if gn_partials:
            tiles = L.lib().storm_conv_tiles(C.byref(a))
            part = torch.zeros((a.B, tiles, a.outC, 2), dtype=torch.float32, device=out.device)
            a.gn_part = L.ptr(part)
        arr[p] = a
        keep.append(a)
        outs.append(out)
        parts.append(part)
    need = L.lib().storm_conv_group_blob_bytes(arr, P)
    blob = torch.empty((need,), dtype=torch.uint8, device=outs[0].device)
    L.check(L.lib().storm_conv_group(arr, P, L.ptr(blob), need, int(bn), L.stream()), "storm_conv_group")
    return (outs, parts) if gn_partials else outs


def conv_kernel_name(segs, Cout, **kw):
    """name of the kernel storm_conv launches for these arguments (storm_conv_kernel_name)"""
    a, _ = _conv_args(segs, Cout, **kw)
    if L.lib().storm_conv_splitk_bytes(C.byref(a)) > 0:     # (as conv() would call it: with the split-K scratch)
        a.splitk_ws, a.splitk_ws_bytes = 16, L.lib().storm_conv_splitk_bytes(C.byref(a))
    return L.lib().storm_conv_kernel_name(C.byref(a)).decode()


def gn_finalize(part_a, part_b=None, gamma=None, beta=None, count=None, eps=1e-6):
    """[B][tiles][C][2] conv-epilogue partials (optionally of two concatenated tensors) -> stats [B][G][2] fp64;
    with gamma/beta/count also the per-channel affine for convs that fuse the apply, ss [B][C/8][2][8] (per channel octet:
    its 8 scales, then its 8 shifts - see pack_gn_ss)."""
    B, ta, Ca, _ = part_a.shape
    tb, Cb = (part_b.shape[1], part_b.shape[2]) if part_b is not None else (0, 0)
    G = gn_groups(Ca + Cb)
    stats = torch.empty((B, G, 2), dtype=torch.float64, device=part_a.device)
    if gamma is None:
        L.check(L.lib().storm_gn_finalize(L.ptr(part_a), Ca, ta, L.ptr(part_b), Cb, tb, B, G, L.ptr(stats), L.stream()),
                "storm_gn_finalize")
        return stats
    ss = torch.empty((B, (Ca + Cb) // 8, 2, 8), dtype=torch.float32, device=part_a.device)
    L.check(L.lib().storm_gn_finalize_ss(L.ptr(part_a), Ca, ta, L.ptr(part_b), Cb, tb, B, G, int(count), L.ptr(gamma),
                                         L.ptr(beta), eps, L.ptr(stats), L.ptr(ss), L.stream()), "storm_gn_finalize_ss")
    return stats, ss


def pack_gn_ss(scale, shift):
    """per-channel (scale, shift) [B, C] -> the table layout the conv kernels read (storm_gn_finalize_ss)"""
    B, Cc = scale.shape
    return torch.stack([scale.reshape(B, Cc // 8, 8), shift.reshape(B, Cc // 8, 8)], 2).contiguous().float()


def attention(q, k, vT, bias, scale):
    """q, k [B, L, C], vT [B, C, ldv] (bf16) -> softmax(scale q k^T) v + bias, [B, L, C] (storm_attention)."""
    B, Lq, Cc = q.shape
    out = torch.empty_like(q)
    need = L.lib().storm_attention_scratch_bytes(B, Lq, Cc, L.dt(q))        # small calls: scratch for the split of the key loop
    ws = torch.empty((need,), dtype=torch.uint8, device=q.device) if need > 0 else None
    L.check(L.lib().storm_attention_ws(L.ptr(q), L.ptr(k), L.ptr(vT), L.ptr(bias), L.ptr(out), B, Lq, Cc, vT.shape[-1], Lq * Cc, Lq * Cc,
                                       Cc * vT.shape[-1], Lq * Cc, float(scale), L.dt(q), L.ptr(ws), need, L.stream()), "storm_attention")
    return out


def attention_group(problems, bias, scale):
    """ONE launch for the fused attention of several problems of one layer (storm_attention_group): problems = [(q, k, vT), ...] as
    attention() takes them (own batch sizes / sequence lengths).  Returns the outputs per problem."""
    P = len(problems)
    Cc = problems[0][0].shape[-1]
    arr = lambda vals: (C.c_void_p * P)(*vals)
    outs = [torch.empty_like(q) for q, _, _ in problems]
    Bs = (C.c_int * P)(*[q.shape[0] for q, _, _ in problems])
    Ls = (C.c_int * P)(*[q.shape[1] for q, _, _ in problems])
    ld = (C.c_int * P)(*[v.shape[-1] for _, _, v in problems])
    need = L.lib().storm_attention_group_blob_bytes(Bs, Ls, P)
    blob = torch.empty((need,), dtype=torch.uint8, device=outs[0].device)
    L.check(L.lib().storm_attention_group(arr([L.ptr(q) for q, _, _ in problems]), arr([L.ptr(k) for _, k, _ in problems]),
                                          arr([L.ptr(v) for _, _, v in problems]), arr([L.ptr(o) for o in outs]), Bs, Ls, ld, P, L.ptr(bias), Cc,
                                          float(scale), L.dt(problems[0][0]), L.ptr(blob), need, L.stream()), "storm_attention_group")
    return outs


# ---------------------------------------------------------------- norm / resample ---------
def gn_groups(C):
    return min(C // 4, 32)


def gn_stats(xa, xb=None):
    B, H, W, Ca = xa.shape
    Cb = xb.shape[-1] if xb is not None else 0
    G = gn_groups(Ca + Cb)
    stats = torch.zeros((B, G, 2), dtype=torch.float64, device=xa.device)
    L.check(L.lib().storm_gn_stats(L.ptr(xa), Ca, L.ptr(xb), Cb, B, H * W, G, L.ptr(stats), L.dt(xa), L.stream()),
            "storm_gn_stats")
    return stats


def gn_apply(xa, stats, gamma, beta, xb=None, silu=True, resample=0, eps=1e-6, want_raw=True):
    """resample: 0 none, 1 / 2 FIR x2 up / down, 3 / 4 the non-FIR members (nearest x2 up / 2x2 mean down, fir=False)"""
    B, H, W, Ca = xa.shape
    Cb = xb.shape[-1] if xb is not None else 0
    Ctot = Ca + Cb
    OH, OW = (2 * H, 2 * W) if resample in (1, 3) else ((H // 2, W // 2) if resample in (2, 4) else (H, W))
    out = _alloc((B, OH, OW, Ctot), xa.dtype, xa)
    raw = _alloc((B, OH, OW, Ctot), xa.dtype, xa) if (resample and want_raw) else None
    L.check(L.lib().storm_gn_apply(L.ptr(xa), Ca, L.ptr(xb), Cb, B, H, W, stats.shape[1], L.ptr(stats),
                                   L.ptr(gamma), L.ptr(beta), eps, int(silu), resample, L.ptr(out), L.ptr(raw),
                                   L.dt(xa), L.stream()), "storm_gn_apply")
    return (out, raw) if resample else out


def fir_up2(x, add=None):
    B, H, W, Cc = x.shape
    out = _alloc((B, 2 * H, 2 * W, Cc), x.dtype, x)
    L.check(L.lib().storm_fir_up2(L.ptr(x), L.ptr(add), L.ptr(out), B, H, W, Cc, L.dt(x), L.stream()), "storm_fir_up2")
    return out


def fir_down2(x):
    B, H, W, Cc = x.shape
    out = _alloc((B, H // 2, W // 2, Cc), x.dtype, x)
    L.check(L.lib().storm_fir_down2(L.ptr(x), L.ptr(out), B, H, W, Cc, L.dt(x), L.stream()), "storm_fir_down2")
    return out


def upfirdn2d(input, kernel, up_x=1, up_y=1, down_x=1, down_y=1, pad_x0=0, pad_x1=0, pad_y0=0, pad_y1=0):
    """The reference's native op with its own argument list (op/upfirdn2d.cpp:12-22): input [N, H, W, 1] contiguous (planes),
    kernel [kh, kw] -> [N, outH, outW, 1]; any factors / pads.  One call of storm_upfirdn2d on torch's current stream."""
    if input.dim() != 4 or input.shape[-1] != 1 or not input.is_contiguous():
        raise ValueError("upfirdn2d: input must be a contiguous [N, H, W, 1] tensor (op/upfirdn2d.cpp:9)")
    N, H, W, _ = input.shape
    kh, kw = kernel.shape
    lib = L.lib()
    OH = lib.storm_upfirdn2d_out_size(H, up_y, down_y, pad_y0, pad_y1, kh)
    OW = lib.storm_upfirdn2d_out_size(W, up_x, down_x, pad_x0, pad_x1, kw)
    out = _alloc((N, max(OH, 0), max(OW, 0), 1), input.dtype, input)
    k32 = kernel.to(device=input.device, dtype=torch.float32).contiguous()
    L.check(lib.storm_upfirdn2d(L.ptr(input), L.ptr(k32), L.ptr(out), N, H, W, kh, kw, up_x, up_y, down_x, down_y,
                                pad_x0, pad_x1, pad_y0, pad_y1, L.dt(input), L.stream()), "storm_upfirdn2d")
    return out


def softmax_rows(scores, dtype, valid=None):
    """softmax over the first `valid` columns of each row (the rest is row padding, written as 0)."""
    ld = scores.shape[-1]
    rows, Lr = scores.numel() // ld, (valid if valid is not None else ld)
    out = _alloc(scores.shape, dtype, scores)
    L.check(L.lib().storm_softmax_rows(L.ptr(scores), L.ptr(out), rows, Lr, ld, L.dt(dtype), L.stream()), "storm_softmax_rows")
    return out


# ---------------------------------------------------------------- network head/tail -------
def pack_input(cplx, dtype):
    """list of complex64 [B,F,T] -> NHWC [B,F,T,8] holding 2*(re,im)-1."""
    B, F, T = cplx[0].shape
    views = [torch.view_as_real(c.contiguous()) for c in cplx]
    arr = (C.c_void_p * len(views))(*[L.ptr(v) for v in views])
    out = _alloc((B, F, T, 8), dtype, views[0])
    L.check(L.lib().storm_pack_input(arr, len(views), L.ptr(out), B, F, T, L.dt(dtype), L.stream()), "storm_pack_input")
    return out


def time_embedding(t, gfp_W, W1, b1, W2, b2):
    B, nf = t.shape[0], gfp_W.shape[0]
    out = _alloc((B, 4 * nf), torch.float32, t)
    L.check(L.lib().storm_time_embedding(L.ptr(t), L.ptr(gfp_W), L.ptr(W1), L.ptr(b1), L.ptr(W2), L.ptr(b2),
                                         L.ptr(out), B, nf, L.stream()), "storm_time_embedding")
    return out


def dense(x, W, bias):
    B, K = x.shape
    N = W.shape[0]
    out = _alloc((B, N), torch.float32, x)
    L.check(L.lib().storm_dense(L.ptr(x), L.ptr(W), L.ptr(bias), L.ptr(out), B, N, K, L.stream()), "storm_dense")
    return out


def output_head(pyr, t, W, bias, negate):
    B, F, T, _ = pyr.shape
    cin = W.shape[1]
    out = torch.empty((B, F, T), dtype=torch.complex64, device=pyr.device)
    W2 = W.reshape(2, cin).contiguous()
    L.check(L.lib().storm_output_head(L.ptr(pyr), L.ptr(t), L.ptr(W2), L.ptr(bias), cin,
                                      L.ptr(torch.view_as_real(out)), B, F, T, int(negate), L.dt(pyr), L.stream()),
            "storm_output_head")
    return out


def input_pyramid(cplx, dtype, n_levels, level0=None):
    """The progressive input pyramid in ONE launch (storm_input_pyramid): level 0 = pack_input(cplx), level k = fir_down2 of level k - 1.
    cplx None: `level0` (NHWC [B,F,T,8]) is read instead.  Returns the list of levels."""
    if cplx is not None:
        B, F, T = cplx[0].shape
        views = [torch.view_as_real(c.contiguous()) for c in cplx]
        arr = (C.c_void_p * len(views))(*[L.ptr(v) for v in views])
        like, n_in = views[0], len(views)
        levels = [_alloc((B, F, T, 8), dtype, like)]
    else:
        B, F, T, _ = level0.shape
        arr, like, n_in = None, level0, 0
        levels = [level0]
    levels += [_alloc((B, F >> k, T >> k, 8), dtype, like) for k in range(1, n_levels)]
    lv = (C.c_void_p * n_levels)(*[L.ptr(v) for v in levels])
    L.check(L.lib().storm_input_pyramid(arr, n_in, lv, n_levels, B, F, T, L.dt(dtype), L.stream()), "storm_input_pyramid")
    return levels


def output_pyramid(phs, t, W, bias, negate):
    """The progressive output pyramid + head in ONE launch (storm_output_pyramid): phs = the pyramid convolutions' outputs NHWC [B, F >> k, T >> k, 8],
    finest first; p = phs[0] + up(phs[1] + up(...)); returns complex64 [B,F,T] = output_head(p, t, W, bias, negate)."""
    B, F, T, _ = phs[0].shape
    cin = W.shape[1]
    out = torch.empty((B, F, T), dtype=torch.complex64, device=phs[0].device)
    W2 = W.reshape(2, cin).contiguous()
    arr = (C.c_void_p * len(phs))(*[L.ptr(v) for v in phs])
    L.check(L.lib().storm_output_pyramid(arr, len(phs), L.ptr(t), L.ptr(W2), L.ptr(bias), cin, L.ptr(torch.view_as_real(out)), B, F, T, int(negate),
                                         L.dt(phs[0]), L.stream()), "storm_output_pyramid")
    return out


# ---------------------------------------------------------------- SDE steps ---------------
def _ouve(sde):
    return L.Ouve(float(sde.theta), float(sde.sigma_min), float(sde.sigma_max), int(sde.N))


def _r(z):
    return None if z is None else torch.view_as_real(z)


def _t32(t):
    """per-batch times as the kernels read them: contiguous float32 (a float64 / strided t would be read as garbage)"""
    return t.to(torch.float32).contiguous()


def _n_per_batch(x):
    return x.numel() // x.shape[0]


def row_seed_table(row_seeds, device):
    """Per-row Philox keys as the *_rs kernels read them: an int64 tensor [B] on `device`, values in [0, 2^63) (the kernels read
    the same 64 bits as unsigned keys).  Takes a sequence of ints or an int64 tensor."""
    if not torch.is_tensor(row_seeds):
        vals = [int(v) for v in row_seeds]
        if any(v < 0 or v >= 2 ** 63 for v in vals):
            raise ValueError("row_seeds must lie in [0, 2^63)")
        row_seeds = torch.tensor(vals, dtype=torch.int64)
    if row_seeds.dtype != torch.int64 or row_seeds.dim() != 1:
        raise ValueError(f"row_seeds must be an int64 tensor [B], got {row_seeds.dtype} {tuple(row_seeds.shape)}")
    return row_seeds.to(device).contiguous()


def _keys(row_seeds, like):
    """the key table of a call on the batch `like` (one key per row), on its device"""
    k = row_seed_table(row_seeds, like.device)
    if k.shape[0] != like.shape[0]:
        raise ValueError(f"row_seeds has {k.shape[0]} keys for a batch of {like.shape[0]} rows")
    return k


def _noise_call(name, args, seed, offset, row_seeds, like):
    """The one call of a noise-drawing entry point: `name` with args (its arguments up to `seed`), seed, offset - or, with row_seeds,
    its per-row-key form name + "_rs": seed 0 (not read) and the key table of the batch `like` after offset."""
    keys = ()
    if row_seeds is not None:
        k = _keys(row_seeds, like)                          # (kept alive in a local: a temporary would be freed before the launch)
        name, seed, keys = name + "_rs", 0, (L.ptr(k),)
    L.check(getattr(L.lib(), name)(*args, seed, offset, *keys, L.stream()), name)


def ouve_prior(sde, y, z=None, seed=0, offset=0, row_seeds=None):
    """row_seeds (here and in every op that takes seed=, offset=): int64 device tensor [B] of per-row Philox keys - row b draws
    what the batch-1 call with seed = row_seeds[b] draws (the storm_*_rs entry points) instead of its share of the stream of `seed`"""
    x = torch.empty_like(y)
    _noise_call("storm_ouve_prior", (L.ptr(_r(y)), L.ptr(_r(z)), L.ptr(_r(x)), y.shape[0], _n_per_batch(y), _ouve(sde)),
                seed, offset, row_seeds, y)
    return x


def ouve_ald_step(sde, x, score, t, snr, z=None, seed=0, offset=0, row_seeds=None):
    """In place on x; returns (x, x_mean)."""
    xm = torch.empty_like(x)
    t = _t32(t)
    _noise_call("storm_ouve_ald_step", (L.ptr(_r(x)), L.ptr(_r(xm)), L.ptr(_r(score)), L.ptr(_r(z)), L.ptr(t), x.shape[0], _n_per_batch(x),
                                        _ouve(sde), float(snr)), seed, offset, row_seeds, x)
    return x, xm


def ouve_predictor_step(sde, x, score, y, t, kind=0, z=None, noise_free=False, seed=0, offset=0, row_seeds=None):
    """In place on x; returns (x, x_mean)."""
    xm = torch.empty_like(x)
    t = _t32(t)
    _noise_call("storm_ouve_predictor_step", (L.ptr(_r(x)), L.ptr(_r(xm)), L.ptr(_r(score)), L.ptr(_r(y)), L.ptr(_r(z)), L.ptr(t), x.shape[0],
                                              _n_per_batch(x), _ouve(sde), kind, int(noise_free)), seed, offset, row_seeds, x)
    return x, xm


def batch_l2norm(v):
    out = _alloc((v.shape[0],), torch.float32, v)
    L.check(L.lib().storm_batch_l2norm(L.ptr(_r(v)), L.ptr(out), v.shape[0], _n_per_batch(v), L.stream()), "storm_batch_l2norm")
    return out


def _all_reduce_sum(t, group):
    """in-place SUM of `t` over a torch.distributed ProcessGroup (RCCL on HIP devices, gloo on CPU tensors).  A ProcessGroup
    has no `all_reduce` method (its `allreduce` returns a Work handle): the functional form is the supported call."""
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def langevin_group_norms(sn, zn, group):
    """(mean ||score||, mean ||z||) over the rows of ALL ranks' batches: the two floats (+ the row count) a sharded `langevin`
    corrector needs to reproduce the unsharded step size (correctors.py:53-55)"""
    tot = torch.stack([sn.sum(), zn.sum(), torch.tensor(float(sn.shape[0]), device=sn.device, dtype=sn.dtype)])
    _all_reduce_sum(tot, group)
    return (tot[0:1] / tot[2]).contiguous(), (tot[1:2] / tot[2]).contiguous()


def langevin_step(x, score, z, snr, per_row=False, group=None):
    """Langevin corrector update, IN PLACE on x (returns (x, x_mean)).  Step size from the batch-mean norms (reference
    semantics, correctors.py:53-55), from every row's own norms (per_row: B independent batch-1 calls), or - with a
    torch.distributed process group - from the means over the batches of all ranks (a 2-float all-reduce per step)."""
    xm = torch.empty_like(x)
    sn, zn = batch_l2norm(score), batch_l2norm(z)
    mode = 1 if per_row else 0
    if group is not None and not per_row:
        (sn, zn), mode = langevin_group_norms(sn, zn, group), 2
    L.check(L.lib().storm_langevin_step(L.ptr(_r(x)), L.ptr(_r(xm)), L.ptr(_r(score)), L.ptr(_r(z)), L.ptr(sn), L.ptr(zn),
                                        x.shape[0], _n_per_batch(x), float(snr), mode, L.stream()), "storm_langevin_step")
    return x, xm


def si_sdr(s, s_hat, eps=0.0):
    """SI-SDR in dB per row of two fp32 waveform batches [B, L] (rows may be strided views)."""
    assert s.dim() == 2 and s_hat.dim() == 2 and s.shape[0] == s_hat.shape[0] and s.stride(1) == 1 and s_hat.stride(1) == 1
    n = min(s.shape[1], s_hat.shape[1])
    out = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
    L.check(L.lib().storm_si_sdr(L.ptr_rows(s), L.ptr_rows(s_hat), L.ptr(out), s.shape[0], n, s.stride(0), s_hat.stride(0), float(eps),
                                 L.stream()), "storm_si_sdr")
    return out


def ouve_pf_drift_g(sde, x, y, score, g_rows):
    """theta (y - x) - 1/2 g_b^2 score with the diffusion coefficient given per row (device fp32 [B])"""
    out = torch.empty_like(x)
    g_rows = g_rows.to(device=x.device, dtype=torch.float32).contiguous()
    L.check(L.lib().storm_ouve_pf_drift_g(L.ptr(_r(out)), L.ptr(_r(x)), L.ptr(_r(y)), L.ptr(_r(score)), L.ptr(g_rows), x.shape[0],
                                          _n_per_batch(x), float(sde.theta), L.stream()), "storm_ouve_pf_drift_g")
    return out


def _rows32(v, like):
    """per-row coefficients as the rows-form kernels read them: device fp32 [B], contiguous"""
    return v.to(device=like.device, dtype=torch.float32).contiguous()


def sde_prior_rows(y, std_rows, z=None, seed=0, offset=0, row_seeds=None):
    """y + z * std_b (OUVPSDE.prior_sampling, sdes.py:306-310); z=None draws in-kernel (Philox)."""
    x = torch.empty_like(y)
    std_rows = _rows32(std_rows, y)
    _noise_call("storm_sde_prior_rows", (L.ptr(_r(y)), L.ptr(_r(z)), L.ptr(_r(x)), L.ptr(std_rows), y.shape[0], _n_per_batch(y)),
                seed, offset, row_seeds, y)
    return x


def sde_predictor_step_rows(sde, x, score, y, t, kind=0, z=None, noise_free=False, seed=0, offset=0, row_seeds=None):
    """Predictor update for an SDE with drift a(t) (y - x) and diffusion g(t) given by its `drift_rows(t)` / `diffusion(t)`
    (fp32 [B], the reference's own expressions).  In place on x; returns (x, x_mean)."""
    xm = torch.empty_like(x)
    a, g = _rows32(sde.drift_rows(t), x), _rows32(sde.diffusion(t), x)
    _noise_call("storm_sde_predictor_step_rows", (L.ptr(_r(x)), L.ptr(_r(xm)), L.ptr(_r(score)), L.ptr(_r(y)), L.ptr(_r(z)), L.ptr(a), L.ptr(g),
                                                  x.shape[0], _n_per_batch(x), int(sde.N), kind, int(noise_free)), seed, offset, row_seeds, x)
    return x, xm


def sde_pf_drift_rows(x, y, score, a_rows, g_rows):
    """a_b (y - x) - 1/2 g_b^2 score: the probability-flow right-hand side with per-row coefficients (device fp32 [B])"""
    out = torch.empty_like(x)
    a, g = _rows32(a_rows, x), _rows32(g_rows, x)
    L.check(L.lib().storm_sde_pf_drift_rows(L.ptr(_r(out)), L.ptr(_r(x)), L.ptr(_r(y)), L.ptr(_r(score)), L.ptr(a), L.ptr(g),
                                            x.shape[0], _n_per_batch(x), L.stream()), "storm_sde_pf_drift_rows")
    return out


# ---------------------------------------------------------------- validation loss ---------
LOSS_KINDS = {"mse": 0, "mae": 1}
PAIR_SQUARE, PAIR_ABS_COMPLEX, PAIR_ABS_REAL = 0, 1, 2


def sde_perturb_rows(x0, y, m_rows, std_rows, form, z=None, seed=0, offset=0, row_seeds=None):
    """x_t = mean_b(x0, y) + std_b z on complex64 [B, ...] in one pass (SDE.marginal_prob + model.py:144-150).  m_rows / std_rows: fp32 [B]
    in the SDE's own expressions; form 0: m x0 + (1 - m) y (OUVESDE._mean), form 1: y + m (x0 - y) (OUVPSDE._mean); z=None draws in-kernel."""
    if x0.shape != y.shape or (z is not None and z.shape != x0.shape):
        raise ValueError(f"sde_perturb_rows: x0 {tuple(x0.shape)}, y {tuple(y.shape)}, z {None if z is None else tuple(z.shape)}")
    x0, y, z = x0.contiguous(), y.contiguous(), (None if z is None else z.contiguous())
    xt = torch.empty_like(x0)
    m, sd = _rows32(m_rows, x0), _rows32(std_rows, x0)
    _noise_call("storm_sde_perturb_rows", (L.ptr(_r(x0)), L.ptr(_r(y)), L.ptr(_r(z)), L.ptr(_r(xt)), L.ptr(m), L.ptr(sd), int(form), x0.shape[0],
                                           _n_per_batch(x0)), seed, offset, row_seeds, x0)
    return xt


def _frames(frames, like):
    """(row_frames device int32 [B] or None, T): `like` is a spectrogram batch [B, ..., T]"""
    rf = _row_len(frames, like)
    if rf is not None and rf.shape[0] != like.shape[0]:
        raise ValueError(f"frames has {rf.shape[0]} entries for a batch of {like.shape[0]} rows")
    return rf, (like.shape[-1] if rf is not None else 0)


def _loss_scratch(B, n, like):
    # per call (the caching allocator makes it cheap), not cached per host thread: ADVICE.md - such a cache is never freed
    return torch.empty((L.lib().storm_dsm_loss_scratch_bytes(B, n),), dtype=torch.uint8, device=like.device)


def dsm_loss_rows(score, std_rows, z=None, kind="mse", frames=None, seed=0, offset=0, row_seeds=None):
    """fp32 [B]: row b's 0.5 sum rho(score std_b + z), rho = |.|^2 ('mse') or |.| ('mae') (model.py:151-153, 113-122).  z=None re-draws
    the noise of the perturbation with the same seed / offset / row_seeds in the kernel.  frames: per-row valid frame counts of
    spectrogram rows [..., T] (the rest of a row is padding and stays out)."""
    score, z = score.contiguous(), (None if z is None else z.contiguous())
    B, n = score.shape[0], _n_per_batch(score)
    out = _alloc((B,), torch.float32, score)
    sd = _rows32(std_rows, score)
    rf, T = _frames(frames, score)
    ws = _loss_scratch(B, n, score)
    _noise_call("storm_dsm_loss_rows", (L.ptr(_r(score)), L.ptr(_r(z)), L.ptr(out), L.ptr(ws), ws.numel(), L.ptr(sd), L.ptr(rf), T,
                                        LOSS_KINDS[kind], B, n), seed, offset, row_seeds, score)
    return out


def pair_loss_rows(a, b, kind="mse", frames=None):
    """fp32 [B]: row b's 0.5 sum |a - b|^2 ('mse') or 0.5 sum |a - b| ('mae') of two complex spectrogram batches or two real waveform
    batches of one shape (DiscriminativeModel._loss model.py:329-343, loss_fn_denoiser :479-481); frames as in dsm_loss_rows (complex only)."""
    if a.shape != b.shape or a.is_complex() != b.is_complex():
        raise ValueError(f"pair_loss_rows: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}")
    cplx = a.is_complex()
    if frames is not None and not cplx:
        raise ValueError("pair_loss_rows: frames count the frames of complex spectrogram rows")
    B = a.shape[0]
    av, bv = (_r(a.contiguous()), _r(b.contiguous())) if cplx else (a.float().contiguous(), b.float().contiguous())
    code = PAIR_SQUARE if LOSS_KINDS[kind] == 0 else (PAIR_ABS_COMPLEX if cplx else PAIR_ABS_REAL)
    n = _n_per_batch(av) if code != PAIR_ABS_COMPLEX else _n_per_batch(a)
    out = _alloc((B,), torch.float32, av)
    rf, T = _frames(frames, a)
    ws = _loss_scratch(B, n, av)
    L.check(L.lib().storm_pair_loss_rows(L.ptr(av), L.ptr(bv), L.ptr(out), L.ptr(ws), ws.numel(), L.ptr(rf), T, code, B, n, L.stream()),
            "storm_pair_loss_rows")
    return out


_rk_scratch = {}


def _kptrs(K):
    arr = (C.c_void_p * len(K))(*[L.ptr(_r(k)) for k in K])
    return arr


RK_MAX_ROWS, RK_ROW_BLOCKS, RK_MAX_TERMS = 128, 256, 13          # include/storm_hip.h: STORM_RK_MAX_ROWS, STORM_RK_ROW_BLOCKS, STORM_RK_MAX_TERMS


def _hrows(h, B):
    if h is None:
        return None
    if len(h) != B or B > RK_MAX_ROWS:
        raise ValueError(f"per-row step sizes: {len(h)} values for {B} rows (at most {RK_MAX_ROWS})")
    return (C.c_double * B)(*[float(v) for v in h])


def rk_combine_rows(x64, K, coef, h_rows, want64=False, entry="storm_rk_combine_rows"):
    """x64[b] + h_rows[b] * sum_j coef[j] K[j][b]: one Runge-Kutta stage of B utterances with their own step sizes.  x64 is
    the complex128 solver state, K complex64 stages; returns the complex64 rounding (the next network input), with
    want64=True (out64, out32)."""
    B = x64.shape[0]
    if B > RK_MAX_ROWS:                      # the kernels take their step sizes as a 128-entry argument array: larger batches in row blocks
        parts = [rk_combine_rows(x64[i:i + RK_MAX_ROWS], [k[i:i + RK_MAX_ROWS] for k in K], coef, h_rows[i:i + RK_MAX_ROWS], want64, entry)
                 for i in range(0, B, RK_MAX_ROWS)]
        return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])) if want64 else torch.cat(parts)
    out32 = torch.empty(x64.shape, dtype=torch.complex64, device=x64.device)
    out64 = torch.empty_like(x64) if want64 else None
    cf = (C.c_double * len(K))(*[float(c) for c in coef])
    L.check(getattr(L.lib(), entry)(L.ptr(_r(out64)) if want64 else None, L.ptr(_r(out32)), L.ptr(_r(x64)), _kptrs(K), cf, len(K),
                                    _hrows(h_rows, B), B, _n_per_batch(x64), L.stream()), entry)
    return (out64, out32) if want64 else out32


def rk_combine_rows_wide(x64, K, coef, h_rows, want64=False):
    """rk_combine_rows for up to RK_MAX_TERMS stages (DOP853's rows have 12): the same bits for up to 7"""
    return rk_combine_rows(x64, K, coef, h_rows, want64, entry="storm_rk_combine_rows_wide")


def _rk_scratch_for(device, need):
    key = (str(device), threading.get_ident())          # (per host thread: grouped micro-batches interleave their launches on one stream)
    if key not in _rk_scratch or _rk_scratch[key].numel() < need:
        _rk_scratch[key] = torch.empty(need, dtype=torch.float64, device=device)
    return _rk_scratch[key]


def rk_error_pair_rows(xa, xb, K, coef_a, coef_b, h_rows, atol, rtol):
    """Device float64 [2, B] from ONE pass over up to RK_MAX_TERMS stages: [0, b] / [1, b] = row b's sum of |v|^2 / (atol + max(|xa|,
    |xb|) rtol)^2 with v = h_b sum coef_a[j] K[j] / h_b sum coef_b[j] K[j] (h_rows None: 1) - DOP853's two error estimators.  Each
    sum is what rk_scaled_sumsq_rows gives for that coefficient row; a row's values do not depend on the other rows of the batch."""
    B = xa.shape[0]
    if B > RK_MAX_ROWS:
        return torch.cat([rk_error_pair_rows(xa[i:i + RK_MAX_ROWS], xb[i:i + RK_MAX_ROWS] if xb is not None else None,
                                             [k[i:i + RK_MAX_ROWS] for k in K], coef_a, coef_b,
                                             h_rows[i:i + RK_MAX_ROWS] if h_rows is not None else None, atol, rtol)
                          for i in range(0, B, RK_MAX_ROWS)], dim=1)
    scratch = _rk_scratch_for(xa.device, 2 * RK_ROW_BLOCKS * B)
    out = torch.empty(2, B, dtype=torch.float64, device=xa.device)
    ca, cb = [(C.c_double * len(K))(*[float(c) for c in cf]) for cf in (coef_a, coef_b)]
    L.check(L.lib().storm_rk_error_pair_rows(L.ptr(out), L.ptr(scratch), scratch.numel(), L.ptr(_r(xa)), L.ptr(_r(xb)) if xb is not None else None,
                                             _kptrs(K) if K else None, ca, cb, len(K), _hrows(h_rows, B), float(atol), float(rtol), B,
                                             _n_per_batch(xa), L.stream()), "storm_rk_error_pair_rows")
    return out


def rk_scaled_sumsq_rows(xa, xb, K, coef, h_rows, atol, rtol, mode=None):
    """Device float64 [B]: row b's sum over its complex elements of |v|^2 / (atol + max(|xa|, |xb|) rtol)^2 with
    v = h_b sum coef[j] K[j] (mode None), K[0] (-1), K[0] - K[1] (-2) or xa itself (-3); xa / xb complex128, K complex64.
    A row's value does not depend on the other rows of the batch."""
    B = xa.shape[0]
    if B > RK_MAX_ROWS:                      # (row blocks, as rk_combine_rows: a row's value does not depend on the others)
        return torch.cat([rk_scaled_sumsq_rows(xa[i:i + RK_MAX_ROWS], xb[i:i + RK_MAX_ROWS] if xb is not None else None,
                                               [k[i:i + RK_MAX_ROWS] for k in K], coef,
                                               h_rows[i:i + RK_MAX_ROWS] if h_rows is not None else None, atol, rtol, mode)
                          for i in range(0, B, RK_MAX_ROWS)])
    scratch = _rk_scratch_for(xa.device, RK_ROW_BLOCKS * B)
    out = torch.empty(B, dtype=torch.float64, device=xa.device)
    n_terms = len(K) if mode is None else mode
    cf = (C.c_double * max(1, len(K)))(*[float(c) for c in (coef if coef is not None else [0.0] * max(1, len(K)))])
    L.check(L.lib().storm_rk_scaled_sumsq_rows(L.ptr(out), L.ptr(scratch), scratch.numel(), L.ptr(_r(xa)),
                                               L.ptr(_r(xb)) if xb is not None else None, _kptrs(K) if K else None, cf, n_terms,
                                               _hrows(h_rows, B), float(atol), float(rtol), B, _n_per_batch(xa), L.stream()),
            "storm_rk_scaled_sumsq_rows")
    return out


def copy_rows(dst, src, mask):
    """dst[b] = src[b] for the rows with mask[b] (host booleans): the rows whose Runge-Kutta step was accepted"""
    B = dst.shape[0]
    m = (C.c_int * B)(*[int(bool(v)) for v in mask])
    L.check(L.lib().storm_copy_rows(L.ptr(dst), L.ptr(src), m, B, dst[0].numel() * dst.element_size(), L.stream()), "storm_copy_rows")
    return dst


def complex_randn(shape, device, seed, offset, row_seeds=None):
    """standard complex normal noise of `shape`; with row_seeds (int64 device [shape[0]]) row b = complex_randn(shape[1:], row_seeds[b], offset)"""
    z = torch.empty(shape, dtype=torch.complex64, device=device)
    rows = (z.numel(),) if row_seeds is None else (z.shape[0], _n_per_batch(z))       # (the one-seed form is ONE row of all the values)
    _noise_call("storm_complex_randn", (L.ptr(_r(z)), *rows), seed, offset, row_seeds, z)
    return z


# ---------------------------------------------------------------- spectral ----------------
_tables = {}


def dft_tables(n_fft, device, window="hann"):
    """(window [n_fft], twiddle [n_fft,2] = (cos, sin)(2 pi k / n_fft)) on `device`, cached."""
    key = (n_fft, str(device), window)
    if key not in _tables:
        if window == "hann":
            w = torch.hann_window(n_fft, periodic=True)
        elif window == "sqrthann":
            w = torch.sqrt(torch.hann_window(n_fft, periodic=True))
        else:
            raise NotImplementedError(f"Window type {window} not implemented!")
        k = torch.arange(n_fft, dtype=torch.float64) * (2.0 * math.pi / n_fft)
        tw = torch.stack([torch.cos(k), torch.sin(k)], dim=1).float().contiguous()
        _tables[key] = (w.to(device).contiguous(), tw.to(device))
    return _tables[key]


def spec_transform(spec, spec_factor, spec_abs_exponent, inverse):
    """spec_fwd (inverse=False) / spec_back (inverse=True) on a complex64 tensor."""
    spec = spec.contiguous()
    out = torch.empty_like(spec)
    L.check(L.lib().storm_spec_transform(L.ptr(_r(spec)), L.ptr(_r(out)), spec.numel(), float(spec_factor),
                                         float(spec_abs_exponent), int(inverse), L.stream()), "storm_spec_transform")
    return out


def _row_len(lengths, like):
    """per-row sample counts of a ragged batch as the kernels read them (device int32 [B]) or None"""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor):
        return lengths.to(device=like.device, dtype=torch.int32).contiguous()
    return torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=like.device)


PEAK_FLOOR = 1e-20                       # storm_peak_abs never returns less (as fp32): the peak of a row whose every sample is zero


def peak_abs(wav, lengths=None):
    """fp32 [B]: max |wav[b]| of a batch whose rows are contiguous (the rows may overlap: a strided view), at least PEAK_FLOOR"""
    B, Lw = wav.shape
    out = _alloc((B,), torch.float32, wav)
    rl = _row_len(lengths, wav)
    L.check(L.lib().storm_peak_abs(L.ptr_rows(wav), L.ptr(out), B, Lw, wav.stride(0), L.ptr(rl), L.stream()), "storm_peak_abs")
    return out


def stft_frames(length, n_fft, hop):
    """frames of torch.stft(center=True) over `length` samples: the signal grows by n_fft // 2 samples on either side and every frame
    needs n_fft samples of it.  Even n_fft: 1 + length // hop; odd n_fft: 1 + (length - 1) // hop."""
    return 1 + (int(length) + 2 * (int(n_fft) // 2) - int(n_fft)) // int(hop)


def stft(wav, peak=None, n_fft=510, hop=128, spec_factor=1.0, spec_abs_exponent=1.0, pad_to=1, window="hann", lengths=None):
    """wav [B, L] fp32 -> complex64 [B, n_fft/2+1, Tpad] = spec_fwd(stft(wav / peak)), zero padded
    in T to a multiple of `pad_to`.  lengths: per-row sample counts of a ragged batch (rows zero filled past them)."""
    B, Lw = wav.shape
    # reflect padding by n_fft // 2 samples needs more samples than that in EVERY row (torch.stft raises otherwise,
    # data_module.py:217-219): a shorter row of a ragged batch would index before its own start
    shortest = Lw if lengths is None else int(min(int(v) for v in lengths))
    if shortest <= n_fft // 2:
        raise ValueError(f"stft: a row of {shortest} samples is too short for reflect padding by n_fft // 2 = {n_fft // 2}")
    if lengths is not None and int(max(int(v) for v in lengths)) > Lw:
        raise ValueError(f"stft: a row length exceeds the batch width {Lw}")
    n_frames = stft_frames(Lw, n_fft, hop)
    Tpad = round_up(n_frames, pad_to)
    win, tw = dft_tables(n_fft, wav.device, window)
    spec = torch.empty((B, n_fft // 2 + 1, Tpad), dtype=torch.complex64, device=wav.device)
    rl = _row_len(lengths, wav)
    L.check(L.lib().storm_stft(L.ptr_rows(wav), L.ptr(peak), L.ptr(_r(spec)), L.ptr(win), L.ptr(tw), B, Lw, wav.stride(0),
                               n_fft, hop, n_frames, Tpad, float(spec_factor), float(spec_abs_exponent), L.ptr(rl), L.stream()),
            "storm_stft")
    return spec


def istft(spec, length, peak=None, n_fft=510, hop=128, spec_factor=1.0, spec_abs_exponent=1.0, window="hann", lengths=None):
    """complex64 [B, F, T] -> wav [B, length] = istft(spec_back(spec)) * peak; with `lengths`, row b is
    istft(..., length=lengths[b]) and zero past it."""
    B, F, T = spec.shape
    spec = spec.contiguous()
    win, tw = dft_tables(n_fft, spec.device, window)
    wav = torch.empty((B, length), dtype=torch.float32, device=spec.device)
    frames = torch.empty((B, T, n_fft), dtype=torch.float32, device=spec.device)
    rl = _row_len(lengths, spec)
    L.check(L.lib().storm_istft(L.ptr(_r(spec)), L.ptr(peak), L.ptr(wav), L.ptr(frames), L.ptr(win), L.ptr(tw), B, T,
                                length, wav.stride(0), n_fft, hop, float(spec_factor), float(spec_abs_exponent), L.ptr(rl),
                                L.stream()), "storm_istft")
    return wav


# ---------------------------------------------------------------- resampling --------------
RESAMPLE_TILE = L.RESAMPLE_TILE          # outputs per workgroup of storm_resample_poly (tests place lengths around it)
_resample_tables = {}


def resample_ratio(up, down):
    """(up, down) reduced by their gcd; the library refuses what is left if it is out of its range"""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"resample: up={up} down={down} (both must be >= 1)")
    g = math.gcd(up, down)
    return up // g, down // g


def resample_length(n, up, down):
    """samples of an n-sample signal after resampling by up / down: ceil(n up / down)"""
    up, down = resample_ratio(up, down)
    return -(-int(n) * up // down)


def _resample_table(up, down, device):
    """the phase-major tap table [up, M] of the reduced ratio on `device`: designed by the library (storm_resample_taps), fetched once"""
    key = (up, down, str(device))
    if key not in _resample_tables:
        n = L.lib().storm_resample_num_taps(up, down)
        if n < 0:
            L.check(n, "storm_resample_num_taps")
        M = -(-n // up)
        host = torch.empty((up, M), dtype=torch.float32)
        L.check(L.lib().storm_resample_taps(up, down, host.data_ptr(), host.numel()), "storm_resample_taps")
        _resample_tables[key] = host.to(device)
    return _resample_tables[key]


def resample_taps(up, down, device="cpu"):
    """The library's filter for the ratio up / down as its kernel reads it: fp32 [up, M], T[p][m] = h[p + m up], zero past the phase's
    last tap (include/storm_hip.h: storm_resample_taps).  A copy: the cached table stays as the library wrote it."""
    up, down = resample_ratio(up, down)
    return _resample_table(up, down, torch.device(device)).clone()


def resample_poly(x, up, down, lengths=None):
    """x [B, L] fp32 (row stride may exceed L) -> [B, ceil(L up / down)]: scipy.signal.resample_poly(x, up, down) with its defaults,
    every output one fp32 FMA chain.  lengths: per-row sample counts of a ragged batch - row b gets ceil(lengths[b] up / down)
    outputs and zeros after them; its samples past lengths[b] are not read.  A ratio of 1 returns x itself (no launch)."""
    up, down = resample_ratio(up, down)
    if up == down:
        return x
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"resample_poly: expected a float32 batch [B, L], got {x.dtype} {tuple(x.shape)}")
    B, Lin = x.shape
    if lengths is not None and (len(lengths) != B or int(max(int(v) for v in lengths)) > Lin):
        raise ValueError(f"resample_poly: lengths {[int(v) for v in lengths]} for a batch {tuple(x.shape)}")
    if x.stride(1) != 1:
        x = x.contiguous()
    Lout = -(-Lin * up // down)
    taps = _resample_table(up, down, x.device)
    y = torch.empty((B, Lout), dtype=torch.float32, device=x.device)
    rl = _row_len(lengths, x)
    stride = x.stride(0) if B > 1 else Lin                       # (a one-row tensor's row stride is whatever its producer left there)
    L.check(L.lib().storm_resample_poly(L.ptr_rows(x), L.ptr(y), L.ptr(taps), B, Lin, stride, Lout, y.stride(0), L.ptr(rl), up, down,
                                        L.stream()), "storm_resample_poly")
    return y


# ---------------------------------------------------------------- long recordings ---------
CROSSFADE_TILE = L.CROSSFADE_TILE        # outputs per workgroup of storm_crossfade_rows (tests place lengths around it)
WINDOW_KEY_STEP = 0x9E3779B97F4A7C15     # window k of a recording draws from key + (k + 1) * this, mod 2^63
_ramps = {}


def _check_overlap(W, V):
    W, V = int(W), int(V)
    if W < 2 or V < 1 or V > W // 2:
        raise ValueError(f"V={V} lies outside [1, W // 2] for windows of W={W} samples")
    return W, V


def window_plan(n_samples, W, V):
    """(n, padded_length) of a recording of n_samples: n = ceil((n_samples - V) / H) windows of W samples at hop H = W - V, the [n, W]
    view of stride H of the recording zero filled to padded_length = (n - 1) H + W.  A recording of at most W samples is not windowed:
    (1, n_samples)."""
    W, V = _check_overlap(W, V)
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"window_plan: a recording of {n_samples} samples")
    if n_samples <= W:
        return 1, n_samples
    H = W - V
    n = -(-(n_samples - V) // H)
    return n, (n - 1) * H + W


def window_key(key, k):
    """the Philox key of window k of a recording with key `key`: (key + (k + 1) * 0x9E3779B97F4A7C15) mod 2^63"""
    return (int(key) + (int(k) + 1) * WINDOW_KEY_STEP) % 2 ** 63


def crossfade_ramp(V, kind="hann", device="cpu"):
    """The fade-in weights of a V-sample overlap as storm_crossfade_rows reads them: fp32 [V] on `device`, designed by the library in fp64
    and rounded once (storm_crossfade_ramp) - 'hann': sin(pi/2 (j + 1) / (V + 1))^2, 'linear': (j + 1) / (V + 1).  Cached per device."""
    V = int(V)
    if V < 1:
        raise ValueError(f"V={V}: an overlap has at least one sample")
    if kind not in L.RAMP_KINDS:
        raise ValueError(f"ramp {kind!r}: one of {sorted(L.RAMP_KINDS)}")
    key = (V, kind, str(torch.device(device)))
    if key not in _ramps:
        host = torch.empty(V, dtype=torch.float32)
        L.check(L.lib().storm_crossfade_ramp(V, L.RAMP_KINDS[kind], host.data_ptr()), "storm_crossfade_ramp")
        _ramps[key] = host.to(device)
    return _ramps[key]


def crossfade_rows(pool, win_row, rec_len, rec_windows, W, V, ramp=None, width=None):
    """The stitch of R recordings in ONE launch (storm_crossfade_rows).  pool: the enhanced windows, fp32 [N, W] (row stride may exceed W);
    win_row: the pool row of every window in (recording, window) order, -1 for a skipped window (it reads as zeros); rec_len / rec_windows:
    every recording's sample count and window count (host ints: rec_windows[r] = window_plan(rec_len[r], W, V)[0]); ramp: fp32 [V] on the
    pool's device (None: crossfade_ramp(V)).  Returns fp32 [R, width] (width None: the longest recording), zero past a recording's length."""
    W, V = _check_overlap(W, V)
    if pool.dim() != 2 or pool.dtype != torch.float32 or pool.shape[1] != W or pool.shape[0] < 1 or pool.stride(1) != 1:
        raise ValueError(f"pool: expected float32 rows [N, W = {W}], got {pool.dtype} {tuple(pool.shape)}")
    N = pool.shape[0]
    win_row, rec_len, rec_windows = [int(v) for v in win_row], [int(v) for v in rec_len], [int(v) for v in rec_windows]
    R, H = len(rec_len), W - V
    if R < 1 or len(rec_windows) != R:
        raise ValueError(f"rec_windows has {len(rec_windows)} entries for {R} recordings in rec_len")
    for r, (n_samples, n) in enumerate(zip(rec_len, rec_windows)):
        if n < 1 or n_samples < 1 or n_samples > (n - 1) * H + W or (n > 1 and n_samples <= (n - 1) * H + V):
            raise ValueError(f"rec_len[{r}] = {n_samples} samples is inconsistent with rec_windows[{r}] = {n} windows of {W} at hop {H}")
    if len(win_row) != sum(rec_windows):
        raise ValueError(f"win_row has {len(win_row)} entries for {sum(rec_windows)} windows in rec_windows")
    if any(v < -1 or v >= N for v in win_row):
        raise ValueError(f"win_row names a row outside the pool of {N} rows (-1 marks a skipped window): {[v for v in win_row if v < -1 or v >= N][:4]}")
    width = max(rec_len) if width is None else int(width)
    if width < max(rec_len):
        raise ValueError(f"width={width} is narrower than the longest recording ({max(rec_len)} samples)")
    if ramp is None:
        ramp = crossfade_ramp(V, "hann", pool.device)
    if ramp.dtype != torch.float32 or tuple(ramp.shape) != (V,) or ramp.device != pool.device:
        raise ValueError(f"ramp: expected float32 [V = {V}] on {pool.device}, got {ramp.dtype} {tuple(ramp.shape)} on {ramp.device}")
    first = [0] * R
    for r in range(1, R):
        first[r] = first[r - 1] + rec_windows[r - 1]
    table = torch.tensor(rec_len + rec_windows + first + win_row, dtype=torch.int32).to(pool.device)       # one upload for the four arrays
    lens, wins, firsts, rows = table[:R], table[R:2 * R], table[2 * R:3 * R], table[3 * R:]
    out = torch.empty((R, width), dtype=torch.float32, device=pool.device)
    stride = pool.stride(0) if N > 1 else W                      # (a one-row tensor's row stride is whatever its producer left there)
    L.check(L.lib().storm_crossfade_rows(L.ptr_rows(pool), N, stride, L.ptr(out), R, width, out.stride(0), L.ptr(lens), L.ptr(wins), L.ptr(firsts),
                                         L.ptr(rows), W, V, L.ptr(ramp.contiguous()), L.stream()), "storm_crossfade_rows")
    return out


# ---------------------------------------------------------------- posterior ensembles -----
ENSEMBLE_TILE = L.ENSEMBLE_TILE          # consecutive bins per workgroup of storm_ensemble_combine_rows (tests place bin counts around it)
ENSEMBLE_MAX_DRAWS = L.ENSEMBLE_MAX_DRAWS
ENSEMBLE_MODES = tuple(L.ENSEMBLE_MODES)                  # "mean", "mag_mean", "mag_median"
DRAW_KEY_STEP = 0xD1B54A32D192ED03       # draw k > 0 of an utterance draws from key + k * this, mod 2^63


def draw_key(key, k):
    """the Philox key of draw k of an utterance with key `key`: the key itself for k = 0 (the single draw of before), else
    (key + k * 0xD1B54A32D192ED03) mod 2^63"""
    key, k = int(key), int(k)
    if k < 0:
        raise ValueError(f"draw_key: k={k}")
    return key if k == 0 else (key + k * DRAW_KEY_STEP) % 2 ** 63


def ensemble_combine(pool, draw_row, factor, exponent, mode="mean", frames=None, spread=False):
    """K draws per utterance combined in ONE launch pair (storm_ensemble_combine_rows; the definition is in include/storm_hip.h).
    pool: sampler outputs in the model's transformed domain, complex64 [N, F, T] (bins contiguous; the row stride may exceed F T);
    draw_row: [B][K] pool rows, host ints or a device int32 tensor [B, K] (draw k of utterance b; any order); factor, exponent: the data
    module's spec_factor and spec_abs_exponent; mode: one of ENSEMBLE_MODES; frames: per-utterance valid frame counts (bins past them are
    not read and come back as zeros).  Returns (out complex64 [B, F, T] in the LINEAR STFT domain, spread fp32 [B, F, T] or None,
    rows fp64 [B, 2 + K] = (E, D, d_0 .. d_{K-1}), best int32 [B] = the medoid draw)."""
    if pool.dim() != 3 or pool.dtype != torch.complex64 or min(pool.shape) < 1:
        raise ValueError(f"ensemble_combine: pool is {pool.dtype} {tuple(pool.shape)}, expected complex64 [N, F, T]")
    if mode not in L.ENSEMBLE_MODES:
        raise ValueError(f"ensemble_combine: mode {mode!r}: one of {list(ENSEMBLE_MODES)}")
    N, F, T = pool.shape
    if pool.stride(2) != 1 or pool.stride(1) != T or (N > 1 and pool.stride(0) < F * T):
        pool = pool.contiguous()
    if pool.data_ptr() % 16:
        pool = pool.clone(memory_format=torch.contiguous_format)               # (a view that starts off a 16-byte boundary: the library refuses it)
    stride = pool.stride(0) if N > 1 else F * T                  # (a one-row tensor's row stride is whatever its producer left there)
    if isinstance(draw_row, torch.Tensor):
        if draw_row.dim() != 2:
            raise ValueError(f"ensemble_combine: draw_row is {tuple(draw_row.shape)}, expected [B, K]")
        table = draw_row.to(device=pool.device, dtype=torch.int32).contiguous()
    else:
        rows = [[int(v) for v in r] for r in draw_row]
        if not rows or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("ensemble_combine: draw_row must be [B][K] with one K for every utterance")
        if any(v < 0 or v >= N for r in rows for v in r):
            raise ValueError(f"ensemble_combine: draw_row names a row outside the pool of {N} rows")
        table = torch.tensor(rows, dtype=torch.int32).reshape(len(rows), len(rows[0])).to(pool.device)
    B, K = table.shape
    if B < 1 or K < 1 or K > ENSEMBLE_MAX_DRAWS:
        raise ValueError(f"ensemble_combine: draw_row is [{B}, {K}]: at least one utterance and 1 <= K <= {ENSEMBLE_MAX_DRAWS} draws")
    _metric_lengths("ensemble_combine", frames, B, T, "frames")
    out = torch.empty((B, F, T), dtype=torch.complex64, device=pool.device)
    sp = torch.empty((B, F, T), dtype=torch.float32, device=pool.device) if spread else None
    rows_out = _alloc((B, 2 + K), torch.float64, pool)
    best = _alloc((B,), torch.int32, pool)
    ws = torch.empty((max(L.lib().storm_ensemble_scratch_bytes(B, F, T, K) // 8, 1),), dtype=torch.float64, device=pool.device)
    fr = _row_len(frames, pool)
    if not L.is_sim() and not pool.is_cuda:
        raise L.StormError("storm_amd ops run on the GPU only: got a CPU tensor (there is no CPU fallback)")
    L.check(L.lib().storm_ensemble_combine_rows(pool.data_ptr(), N, stride, L.ptr(table),
                                                L.ptr(_r(out)), L.ptr(sp), L.ptr(rows_out), L.ptr(best), L.ptr(ws), 8 * ws.numel(), B, K, F, T,
                                                L.ptr(fr), float(factor), float(exponent), L.ENSEMBLE_MODES[mode], L.stream()),
            "storm_ensemble_combine_rows")
    return out, sp, rows_out, best


# ---------------------------------------------------------------- metrics -----------------
METRICS_CHUNK = L.METRICS_CHUNK          # samples per workgroup of storm_energy_ratios_rows (tests place lengths around it)


def _metric_lengths(who, lengths, B, width, what):
    """lengths of a ragged batch checked on the host: one per row, each in [1, width]"""
    if lengths is None:
        return
    vals = [int(v) for v in lengths]
    if len(vals) != B or min(vals) < 1 or max(vals) > width:
        raise ValueError(f"{who}: {what} {vals} for a batch of {B} rows x {width}")


def energy_ratios_rows(s_hat, s, n, lengths=None):
    """fp64 [B, 4] = (SI-SDR, SI-SIR, SI-SAR, input SNR) in dB per row of three fp32 waveform batches [B, L] (rows may be strided views):
    energy_ratios(s_hat, s, n) and snr_dB(s, n) of util/other.py:21-44, 96-100.  lengths: per-row sample counts of a ragged batch (the
    rest of a row is not read).  A row's numbers do not depend on the batch it is in."""
    for name, x in (("s_hat", s_hat), ("s", s), ("n", n)):
        if x.dim() != 2 or x.dtype != torch.float32 or x.shape != s_hat.shape:
            raise ValueError(f"energy_ratios_rows: {name} is {x.dtype} {tuple(x.shape)}, expected float32 [B, L] = {tuple(s_hat.shape)}")
    B, Lw = s_hat.shape
    if B < 1 or Lw < 1:
        raise ValueError(f"energy_ratios_rows: empty batch {tuple(s_hat.shape)}")
    _metric_lengths("energy_ratios_rows", lengths, B, Lw, "lengths")
    rows = [x if x.stride(1) == 1 else x.contiguous() for x in (s_hat, s, n)]
    strides = [x.stride(0) if B > 1 else Lw for x in rows]       # (a one-row tensor's row stride is whatever its producer left there)
    out = _alloc((B, 4), torch.float64, s_hat)
    ws = torch.empty((L.lib().storm_energy_ratios_scratch_bytes(B, Lw),), dtype=torch.uint8, device=s_hat.device)
    rl = _row_len(lengths, s_hat)
    L.check(L.lib().storm_energy_ratios_rows(L.ptr_rows(rows[0]), L.ptr_rows(rows[1]), L.ptr_rows(rows[2]), L.ptr(out), L.ptr(ws), ws.numel(),
                                             B, Lw, strides[0], strides[1], strides[2], L.ptr(rl), L.stream()), "storm_energy_ratios_rows")
    return out


def lsd_rows(S_hat, S, frames=None, eps=1e-10):
    """fp64 [B]: the log-spectral distance sqrt(mean |2 ln(eps + |S_hat|) - 2 ln(eps + |S|)|) per row of two complex64 spectrogram batches
    [B, F, T] (util/other.py:16-19 after its STFTs).  frames: per-row valid frame counts (the padding frames of a row stay out)."""
    if S_hat.shape != S.shape or S_hat.dim() != 3 or S_hat.dtype != torch.complex64 or S.dtype != torch.complex64:
        raise ValueError(f"lsd_rows: {S_hat.dtype} {tuple(S_hat.shape)} against {S.dtype} {tuple(S.shape)}, expected two complex64 [B, F, T]")
    B, F, T = S_hat.shape
    if min(B, F, T) < 1:
        raise ValueError(f"lsd_rows: empty batch {tuple(S_hat.shape)}")
    _metric_lengths("lsd_rows", frames, B, T, "frames")
    S_hat, S = S_hat.contiguous(), S.contiguous()
    out = _alloc((B,), torch.float64, S_hat)
    ws = torch.empty((L.lib().storm_lsd_scratch_bytes(B, F, T),), dtype=torch.uint8, device=S_hat.device)
    rf = _row_len(frames, S_hat)
    L.check(L.lib().storm_lsd_rows(L.ptr(_r(S_hat)), L.ptr(_r(S)), L.ptr(out), L.ptr(ws), ws.numel(), B, F, T, L.ptr(rf), float(eps), L.stream()),
            "storm_lsd_rows")
    return out


# ---------------------------------------------------------------- intelligibility ---------
STOI_FS = 10000                          # the rate STOI / ESTOI are defined at (include/storm_hip.h: storm_stoi_rows)
_stoi_tables = {}


def _stoi_table(fs, device):
    """(taps [up, M] on `device`, num_taps, up, down) of the STOI resampling filter fs -> 10 kHz: designed by the library (storm_stoi_taps),
    fetched once per rate and device"""
    key = (fs, str(device))
    if key not in _stoi_tables:
        n = L.lib().storm_stoi_num_taps(fs)
        if n < 0:
            L.check(n, "storm_stoi_num_taps")
        up, down = resample_ratio(STOI_FS, fs)
        host = torch.empty((up, -(-n // up)), dtype=torch.float32)
        L.check(L.lib().storm_stoi_taps(fs, host.data_ptr(), host.numel()), "storm_stoi_taps")
        _stoi_tables[key] = (host.to(device), n, up, down)
    return _stoi_tables[key]


def stoi_taps(fs, device="cpu"):
    """The library's STOI resampling filter fs -> 10 kHz as its kernel reads it: fp32 [up, M], T[p][m] = up h[p + m up], zero past the
    phase's last tap (include/storm_hip.h: storm_stoi_taps).  A copy: the cached table stays as the library wrote it."""
    return _stoi_table(int(fs), torch.device(device))[0].clone()


def stoi_resample(x, fs, lengths=None):
    """x [B, L] fp32 at `fs` -> [B, ceil(L up / down)] at 10 kHz through the STOI filter (storm_resample_poly_taps); rows past their
    length are zero, as in resample_poly.  fs = 10000 returns x itself (no launch)."""
    fs = int(fs)
    if fs == STOI_FS:
        return x
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"stoi_resample: expected a float32 batch [B, L], got {x.dtype} {tuple(x.shape)}")
    taps, n, up, down = _stoi_table(fs, x.device)
    if x.stride(1) != 1:
        x = x.contiguous()
    B, Lin = x.shape
    Lout = -(-Lin * up // down)
    y = torch.empty((B, Lout), dtype=torch.float32, device=x.device)
    rl = _row_len(lengths, x)
    stride = x.stride(0) if B > 1 else Lin                       # (a one-row tensor's row stride is whatever its producer left there)
    L.check(L.lib().storm_resample_poly_taps(L.ptr_rows(x), L.ptr(y), L.ptr(taps), B, Lin, stride, Lout, y.stride(0), L.ptr(rl), up, down, n,
                                             L.stream()), "storm_resample_poly_taps")
    return y


def stoi_rows(clean, estimate, lengths=None, fs=16000, counts=False):
    """fp64 [B, 2] = (STOI, ESTOI) per row of two fp32 waveform batches [B, L] at `fs` (rows may be strided views): the definition of
    include/storm_hip.h (storm_stoi_rows), 1e-5 for a row with fewer than 30 spectrogram frames.  Unless fs is 10000 both batches are
    resampled on the device first (storm_resample_poly_taps with the STOI filter; row b then has ceil(lengths[b] up / down) samples).
    lengths: per-row sample counts of a ragged batch (the rest of a row is not read).  A row's numbers do not depend on the batch it is in.
    counts=True (tests): also int32 [B, 3] = the row's gate frames, kept frames and segments."""
    for name, x in (("clean", clean), ("estimate", estimate)):
        if x.dim() != 2 or x.dtype != torch.float32 or x.shape != clean.shape:
            raise ValueError(f"stoi_rows: {name} is {x.dtype} {tuple(x.shape)}, expected float32 [B, L] = {tuple(clean.shape)}")
    B, Lw = clean.shape
    if B < 1 or Lw < 1:
        raise ValueError(f"stoi_rows: empty batch {tuple(clean.shape)}")
    _metric_lengths("stoi_rows", lengths, B, Lw, "lengths")
    fs = int(fs)
    if fs != STOI_FS:
        up, down = resample_ratio(STOI_FS, fs)
        clean, estimate = stoi_resample(clean, fs, lengths), stoi_resample(estimate, fs, lengths)
        if lengths is not None:
            lengths = [-(-int(v) * up // down) for v in lengths]
        Lw = clean.shape[1]
    rows = [x if x.stride(1) == 1 else x.contiguous() for x in (clean, estimate)]
    strides = [x.stride(0) if B > 1 else Lw for x in rows]       # (a one-row tensor's row stride is whatever its producer left there)
    out = _alloc((B, 2), torch.float64, clean)
    ws = torch.empty((L.lib().storm_stoi_scratch_bytes(B, Lw) // 4,), dtype=torch.int32, device=clean.device)
    rl = _row_len(lengths, clean)
    L.check(L.lib().storm_stoi_rows(L.ptr_rows(rows[0]), L.ptr_rows(rows[1]), L.ptr(out), L.ptr(ws), 4 * ws.numel(), B, Lw, strides[0],
                                    strides[1], L.ptr(rl), L.stream()), "storm_stoi_rows")
    return (out, ws[:4 * B].reshape(B, 4)[:, :3].clone()) if counts else out


# ---------------------------------------------------------------- frame-based measures ----
LPC_TILE = L.LPC_TILE                    # consecutive frames per workgroup of storm_lpc_measures_rows (tests place frame counts around it)
_lpc_windows = {}


def lpc_shape(fs):
    """(W, H, P) of include/storm_hip.h (storm_lpc_measures_rows) for a sample rate: window, hop and LPC order"""
    fs = int(fs)
    W = (30 * fs + 500) // 1000
    return W, W // 4, 16 if fs >= 10000 else 10


def _lpc_window(fs, device):
    """the analysis window of the frame-based measures at fs, fp64 [W] on `device`: written by the library (storm_lpc_window), fetched once
    per rate and device"""
    key = (fs, str(device))
    if key not in _lpc_windows:
        host = torch.empty((max(lpc_shape(fs)[0], 1),), dtype=torch.float64)
        n = L.lib().storm_lpc_window(fs, host.data_ptr(), host.numel())
        if n < 0:
            L.check(n, "storm_lpc_window")
        _lpc_windows[key] = host[:n].to(device)
    return _lpc_windows[key]


def lpc_window(fs, device="cpu"):
    """The window of the frame-based measures at `fs` as the kernel reads it: fp64 [W], w[n] = 0.5 (1 - cos(2 pi (n + 1) / (W + 1)))
    (include/storm_hip.h: storm_lpc_window).  A copy: the cached table stays as the library wrote it."""
    return _lpc_window(int(fs), torch.device(device)).clone()


def lpc_measures_rows(x, y, lengths=None, fs=16000, frames=False, counts=False):
    """fp64 [B, 3] = (segmental SNR in dB, log-likelihood ratio, LPC cepstral distance in dB) per row of the clean batch x and the processed
    batch y, fp32 [B, L] at `fs` (rows may be strided views): the definition of include/storm_hip.h (storm_lpc_measures_rows).  A row with
    fewer than W + H samples has no frame: three NaN; a row whose frames are all void (a silent signal) has NaN for LLR and CD.
    lengths: per-row sample counts of a ragged batch (the rest of a row is not read).  A row's numbers do not depend on the batch it is in.
    frames=True: also fp64 [B, M(L), 3], the per-frame values (NaN past a row's own frames and, in LLR and CD, for void frames).
    counts=True: also int32 [B, 2] = the row's frames M and those that are not void M'.  Returned in this order: rows, frames, counts."""
    for name, v in (("x", x), ("y", y)):
        if v.dim() != 2 or v.dtype != torch.float32 or v.shape != x.shape:
            raise ValueError(f"lpc_measures_rows: {name} is {v.dtype} {tuple(v.shape)}, expected float32 [B, L] = {tuple(x.shape)}")
    B, Lw = x.shape
    if B < 1 or Lw < 1:
        raise ValueError(f"lpc_measures_rows: empty batch {tuple(x.shape)}")
    _metric_lengths("lpc_measures_rows", lengths, B, Lw, "lengths")
    fs = int(fs)
    win = _lpc_window(fs, x.device)
    W, H, _ = lpc_shape(fs)
    rows = [v if v.stride(1) == 1 else v.contiguous() for v in (x, y)]
    strides = [v.stride(0) if B > 1 else Lw for v in rows]       # (a one-row tensor's row stride is whatever its producer left there)
    out = _alloc((B, 3), torch.float64, x)
    per = _alloc((B, (Lw - W) // H if Lw >= W else 0, 3), torch.float64, x) if frames else None
    ws = torch.empty((L.lib().storm_lpc_measures_scratch_bytes(B, Lw, fs) // 4,), dtype=torch.int32, device=x.device)
    rl = _row_len(lengths, x)
    L.check(L.lib().storm_lpc_measures_rows(L.ptr_rows(rows[0]), L.ptr_rows(rows[1]), L.ptr(win), L.ptr(out), L.ptr(per), L.ptr(ws),
                                            4 * ws.numel(), B, Lw, strides[0], strides[1], L.ptr(rl), fs, L.stream()), "storm_lpc_measures_rows")
    res = (out,) + ((per,) if frames else ()) + ((ws[:2 * B].reshape(B, 2).clone(),) if counts else ())
    return res if len(res) > 1 else out


# ---------------------------------------------------------------- misaligned audio --------
XCORR_TILE = L.XCORR_TILE                # consecutive lags per workgroup of storm_xcorr_lag_rows (tests place delays around its multiples)
SOS_MAX_SECTIONS = L.SOS_MAX_SECTIONS


def _wave_rows(who, name, x):
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: {name} is {x.dtype} {tuple(x.shape)}, expected a float32 batch [B, L]")
    return x if x.stride(1) == 1 else x.contiguous()


def xcorr_lag_rows(y, ref, lengths=None, ref_lengths=None, max_lag=None):
    """(lag int32 [B], peak fp64 [B]) per row of two fp32 waveform batches y [B, Ny] and ref [B, Nr] (rows may be strided views): the
    smallest lag d at which the full cross-correlation c[d] = sum_n y[n] ref[n + d] is largest, and that value (include/storm_hip.h:
    storm_xcorr_lag_rows; every c[d] is one fp64 chain in ascending n).  ref is y delayed by `lag` samples.  lengths / ref_lengths:
    per-row sample counts of a ragged batch (the rest of a row is not read).  max_lag: only |d| <= max_lag is searched (None: every
    lag).  Two launches, no synchronisation; a row's outputs do not depend on the batch it is in."""
    y, ref = _wave_rows("xcorr_lag_rows", "y", y), _wave_rows("xcorr_lag_rows", "ref", ref)
    B, Ny = y.shape
    Nr = ref.shape[1]
    if ref.shape[0] != B:
        raise ValueError(f"xcorr_lag_rows: {tuple(y.shape)} against {tuple(ref.shape)}")
    _metric_lengths("xcorr_lag_rows", lengths, B, Ny, "lengths")
    _metric_lengths("xcorr_lag_rows", ref_lengths, B, Nr, "ref_lengths")
    ml = -1 if max_lag is None else int(max_lag)
    if ml < -1 or ml > 2 ** 30:
        raise ValueError(f"xcorr_lag_rows: max_lag={max_lag} (None or a sample count >= 0)")
    tiles = L.lib().storm_xcorr_num_partials(Ny, Nr, ml)
    if tiles < 1:
        raise ValueError(f"xcorr_lag_rows: rows of {Ny} / {Nr} samples")
    lag, peak = _alloc((B,), torch.int32, y), _alloc((B,), torch.float64, y)
    ws = torch.empty((B * tiles * L.XCORR_PARTIAL_BYTES // 8,), dtype=torch.float64, device=y.device)
    sy, sr = (y.stride(0), ref.stride(0)) if B > 1 else (Ny, Nr)   # (a one-row tensor's row stride is whatever its producer left there)
    yl, rl = _row_len(lengths, y), _row_len(ref_lengths, y)
    L.check(L.lib().storm_xcorr_lag_rows(L.ptr_rows(y), L.ptr_rows(ref), L.ptr(lag), L.ptr(peak), L.ptr(ws), 8 * ws.numel(), B, Ny, Nr, sy, sr,
                                         L.ptr(yl), L.ptr(rl), ml, L.stream()), "storm_xcorr_lag_rows")
    return lag, peak


def shift_rows(x, shift, lengths=None, wrap=True):
    """x fp32 [B, N] moved by a per-row shift that stays on the device: out[b, n] = x[b, (n - s) mod len] (wrap=True: np.roll(row, s)) or
    x[b, n - s] inside the row and 0 outside (wrap=False); s = shift[b], an int32 DEVICE tensor [B] (a list or int is uploaded).  lengths:
    per-row sample counts; samples past them are written as zeros.  One launch (storm_shift_rows)."""
    x = _wave_rows("shift_rows", "x", x)
    B, N = x.shape
    if isinstance(shift, torch.Tensor):
        shift = shift.to(device=x.device, dtype=torch.int32).reshape(-1).contiguous()
    else:
        shift = torch.tensor([int(shift)] * B if isinstance(shift, int) else [int(v) for v in shift], dtype=torch.int32, device=x.device)
    if shift.numel() != B:
        raise ValueError(f"shift_rows: {shift.numel()} shifts for a batch of {B} rows")
    _metric_lengths("shift_rows", lengths, B, N, "lengths")
    out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    rl = _row_len(lengths, x)
    L.check(L.lib().storm_shift_rows(L.ptr_rows(x), L.ptr(out), L.ptr(shift), B, N, x.stride(0) if B > 1 else N, out.stride(0),
                                     L.ptr(rl), int(bool(wrap)), L.stream()), "storm_shift_rows")
    return out


def butter_sos(order, wn, btype="hp"):
    """The second-order sections of scipy.signal.butter(order, wn, btype, output='sos') for an even order: a float64 CPU tensor [order / 2, 6],
    designed by the library in closed form (storm_butter_sos).  wn: the cut-off as a fraction of the Nyquist rate; btype 'hp' or 'lp'."""
    kinds = {"hp": 1, "highpass": 1, "high": 1, "lp": 0, "lowpass": 0, "low": 0}
    if btype not in kinds:
        raise ValueError(f"butter_sos: btype {btype!r} ('hp' or 'lp')")
    order = int(order)
    sos = torch.zeros((max(order // 2, 1), 6), dtype=torch.float64)
    L.check(L.lib().storm_butter_sos(order, float(wn), kinds[btype], sos.data_ptr()), "storm_butter_sos")
    return sos


def sosfilt_rows(x, sos, lengths=None, out_dtype=torch.float64):
    """scipy.signal.sosfilt(sos, row) with zero initial state for every row of x fp32 [B, L]: out_dtype float64 [B, L], or float32 = that value
    rounded once.  sos: [S, 6] (a tensor or array; read on the host as float64, a0 = 1).  lengths: per-row sample counts; the tail of a row is
    zero.  One launch (storm_sosfilt_rows): every multiply and add of the recurrence is rounded separately, in scipy's order."""
    x = _wave_rows("sosfilt_rows", "x", x)
    B, Lw = x.shape
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError(f"sosfilt_rows: out_dtype {out_dtype} (float64 or float32)")
    sos = torch.as_tensor(sos).detach().to("cpu", torch.float64).contiguous()
    if sos.dim() != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= SOS_MAX_SECTIONS:
        raise ValueError(f"sosfilt_rows: sos {tuple(sos.shape)}, expected [S, 6] with 1 <= S <= {SOS_MAX_SECTIONS}")
    _metric_lengths("sosfilt_rows", lengths, B, Lw, "lengths")
    out = torch.empty((B, Lw), dtype=out_dtype, device=x.device)
    rl = _row_len(lengths, x)
    L.check(L.lib().storm_sosfilt_rows(L.ptr_rows(x), L.ptr(out), sos.data_ptr(), sos.shape[0], B, Lw, x.stride(0) if B > 1 else Lw, out.stride(0),
                                       L.ptr(rl), int(out_dtype == torch.float32), L.stream()), "storm_sosfilt_rows")
    return out


# ---------------------------------------------------------------- BSS-eval SDR ------------
BSS_MAX_TAPS = L.BSS_MAX_TAPS            # the longest filter storm_bss_sdr_rows allows the estimate
BSS_PIECE = L.BSS_PIECE                  # samples per workgroup of its correlations (tests place lengths around it)


def bss_sdr_rows(reference, estimate, lengths=None, flen=512, return_filter=False, return_parts=False):
    """fp64 [B]: the BSS-eval SDR in dB per row of two fp32 waveform batches [B, L] (rows may be strided views) - the estimate projected onto
    the span of `flen` delayed copies of the reference, the energy of the projection over the energy of the rest (include/storm_hip.h:
    storm_bss_sdr_rows has the definition and the edge rules: +inf for no rest, NaN for an empty or all-zero row and for a reference whose
    delays are numerically dependent).  lengths: per-row sample counts of a ragged batch (the rest of a row is not read).
    return_filter adds fp64 [B, flen], the solved filter (argmax |filter| is the estimate's delay); return_parts adds fp64 [B, 2 flen + 1] =
    (G, D, Ee), the correlations it was solved from.  Two launches, no synchronisation; a row's outputs do not depend on the batch it is in."""
    ref, est = _wave_rows("bss_sdr_rows", "reference", reference), _wave_rows("bss_sdr_rows", "estimate", estimate)
    B, Lw = ref.shape
    if est.shape != ref.shape:
        raise ValueError(f"bss_sdr_rows: {tuple(ref.shape)} against {tuple(est.shape)}")
    if lengths is not None:                                        # (a row of no samples is allowed here: its SDR is NaN)
        vals = [int(v) for v in lengths]
        if len(vals) != B or min(vals) < 0 or max(vals) > Lw:
            raise ValueError(f"bss_sdr_rows: lengths {vals} for a batch of {B} rows x {Lw}")
    flen = int(flen)
    out = _alloc((B,), torch.float64, ref)
    filt = _alloc((B, max(flen, 1)), torch.float64, ref) if return_filter else None
    parts = _alloc((B, 2 * max(flen, 0) + 1), torch.float64, ref) if return_parts else None
    ws = torch.empty((max(L.lib().storm_bss_sdr_scratch_bytes(B, Lw, flen) // 8, 1),), dtype=torch.float64, device=ref.device)
    sr, se = (ref.stride(0), est.stride(0)) if B > 1 else (Lw, Lw)    # (a one-row tensor's row stride is whatever its producer left there)
    rl = _row_len(lengths, ref)
    L.check(L.lib().storm_bss_sdr_rows(L.ptr_rows(ref), L.ptr_rows(est), L.ptr(out), L.ptr(filt), L.ptr(parts), L.ptr(ws), 8 * ws.numel(), B, Lw,
                                       sr, se, L.ptr(rl), flen, L.stream()), "storm_bss_sdr_rows")
    res = (out,) + ((filt,) if return_filter else ()) + ((parts,) if return_parts else ())
    return res if len(res) > 1 else out


def bss_eval_rows(target, noise, estimate, lengths=None, flen=512, return_filter=False, return_parts=False):
    """fp64 [B, 3] = (sdr, sir, sar) in dB per row of three fp32 waveform batches [B, L] (rows may be strided views): BSS-eval with two
    sources - the estimate projected onto `flen` delayed copies of the target (P1) and, jointly, of target and noise (P12); sdr = P1 / (Ee -
    P1) is bss_sdr_rows(target, estimate) bit for bit, sir = P1 / (P12 - P1), sar = P12 / (Ee - P12) (include/storm_hip.h:
    storm_bss_eval_rows has the definition and the edge rules: NaN sir / sar for a silent noise row and for a noise row whose delays depend
    on the target's).  This is BSS-eval's split, not si_sir / si_sar of energy_ratios_rows.  lengths: per-row sample counts of a ragged batch.
    return_filter adds fp64 [B, 2, flen], the two filters of the joint solve; return_parts adds fp64 [B, 6 flen + 1] = (G11, D1, G22, D2,
    X12, X21, Ee).  Three launches, no synchronisation; a row's outputs do not depend on the batch it is in."""
    tgt, noi, est = (_wave_rows("bss_eval_rows", n, v) for n, v in (("target", target), ("noise", noise), ("estimate", estimate)))
    B, Lw = tgt.shape
    if est.shape != tgt.shape or noi.shape != tgt.shape:
        raise ValueError(f"bss_eval_rows: {tuple(tgt.shape)}, {tuple(noi.shape)} and {tuple(est.shape)}")
    if lengths is not None:                                        # (a row of no samples is allowed here: its numbers are NaN)
        vals = [int(v) for v in lengths]
        if len(vals) != B or min(vals) < 0 or max(vals) > Lw:
            raise ValueError(f"bss_eval_rows: lengths {vals} for a batch of {B} rows x {Lw}")
    flen = int(flen)
    out = _alloc((B, 3), torch.float64, tgt)
    filt = _alloc((B, 2, max(flen, 1)), torch.float64, tgt) if return_filter else None
    parts = _alloc((B, 6 * max(flen, 0) + 1), torch.float64, tgt) if return_parts else None
    ws = torch.empty((max(L.lib().storm_bss_eval_scratch_bytes(B, Lw, flen) // 8, 1),), dtype=torch.float64, device=tgt.device)
    st, sn, se = (tgt.stride(0), noi.stride(0), est.stride(0)) if B > 1 else (Lw, Lw, Lw)
    rl = _row_len(lengths, tgt)
    L.check(L.lib().storm_bss_eval_rows(L.ptr_rows(tgt), L.ptr_rows(noi), L.ptr_rows(est), L.ptr(out), L.ptr(filt), L.ptr(parts), L.ptr(ws),
                                        8 * ws.numel(), B, Lw, st, sn, se, L.ptr(rl), flen, L.stream()), "storm_bss_eval_rows")
    res = (out,) + ((filt,) if return_filter else ()) + ((parts,) if return_parts else ())
    return res if len(res) > 1 else out


# ---------------------------------------------------------------- ConvTasNet --------------
TASNET_ENCODE, TASNET_POINTWISE, TASNET_DEPTHWISE = 0, 1, 2


def tasnet_frames(T, win):
    """frames of a T-sample waveform after pad_signal (convtasnet.py:75-94) under Conv1d(win, stride = win // 2)"""
    n = L.lib().storm_tasnet_frames(int(T), int(win))
    if n <= 0:
        raise L.StormError(f"storm_tasnet_frames({T}, {win}) failed")
    return n


def _tasnet_part(op, B, Lf, Cc, like):
    n = L.lib().storm_tasnet_num_partials(op, Lf, Cc)
    if n <= 0:
        raise L.StormError(f"storm_tasnet_num_partials({op}, {Lf}, {Cc}) failed")
    return _alloc((B, n, 2), torch.float32, like)


def tasnet_encode(wav, wT, dtype):
    """wav [B, T] fp32, wT [win, N] fp32 -> (enc [B, L, N] in dtype, partial sums of enc for TCN.LN)"""
    B, T = wav.shape
    win, N = wT.shape
    Lf = tasnet_frames(T, win)
    enc = _alloc((B, Lf, N), dtype, wav)
    part = _tasnet_part(TASNET_ENCODE, B, Lf, N, wav)
    L.check(L.lib().storm_tasnet_encode(L.ptr_rows(wav), wav.stride(0), L.ptr(wT), L.ptr(enc), L.ptr(part), B, T, N, win, L.dt(dtype),
                                        L.stream()), "storm_tasnet_encode")
    return enc, part


def tasnet_gln_finalize(part, count, eps=1e-8):
    """partials [B, n, 2] of a row's C x L values -> stats [B, 2] = (mean, rstd) of GroupNorm(1, C, eps)"""
    B, n, _ = part.shape
    stats = _alloc((B, 2), torch.float32, part)
    L.check(L.lib().storm_tasnet_gln_finalize(L.ptr(part), L.ptr(stats), B, n, int(count), float(eps), L.stream()), "storm_tasnet_gln_finalize")
    return stats


def tasnet_pointwise(x, w, bias, dtype, norm=None, prelu_in=None, prelu_out=None, out_f32=False, partials=False, res_skip=None):
    """1x1 convolution on the MFMA: x [B, L, Cin] (dtype, or fp32 = a running sum), w [Cout, Cin] in dtype, bias fp32.
    norm = (stats, gamma, beta): norm-apply on load; prelu_in / prelu_out: 1-element slope tensors (PReLU on load / in the epilogue).
    res_skip = (output, skip): the fused res_out + skip_out form - adds to both fp32 [B, L, Cout / 2] tensors in place, returns None.
    Otherwise returns out [B, L, Cout] (and its partial sums with partials=True)."""
    B, Lf, Cin = x.shape
    Cout = w.shape[0]
    if w.dtype != dtype or w.shape[1] != Cin or x.dtype not in (dtype, torch.float32):
        raise L.StormError(f"tasnet_pointwise: x {tuple(x.shape)} {x.dtype}, w {tuple(w.shape)} {w.dtype}, compute dtype {dtype}")
    stats, gamma, beta = norm if norm is not None else (None, None, None)
    if res_skip is not None:
        out, skip = res_skip
        if not (out.dtype == skip.dtype == torch.float32 and tuple(out.shape) == tuple(skip.shape) == (B, Lf, Cout // 2)):
            raise L.StormError("tasnet_pointwise: res_skip needs two fp32 [B, L, Cout / 2] tensors")
        part = None
    else:
        out, skip = _alloc((B, Lf, Cout), torch.float32 if out_f32 else dtype, x), None
        part = _tasnet_part(TASNET_POINTWISE, B, Lf, Cout, x) if partials else None
    L.check(L.lib().storm_tasnet_pointwise(L.ptr(x), int(x.dtype == torch.float32), L.ptr(w), L.ptr(bias), L.ptr(out), int(out.dtype == torch.float32),
                                           L.ptr(skip), int(res_skip is not None), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(prelu_in),
                                           L.ptr(prelu_out), L.ptr(part), B, Lf, Cin, Cout, L.dt(dtype), L.stream()), "storm_tasnet_pointwise")
    if res_skip is not None:
        return None
    return (out, part) if partials else out


def tasnet_depthwise(x, w3, bias, norm, prelu, dilation):
    """x [B, L, C] -> (PReLU(dconv(norm(x)) + bias) [B, L, C], its partial sums); w3 [3, C] fp32; norm = (stats, gamma, beta)"""
    B, Lf, Cc = x.shape
    stats, gamma, beta = norm
    out = torch.empty_like(x)
    part = _tasnet_part(TASNET_DEPTHWISE, B, Lf, Cc, x)
    L.check(L.lib().storm_tasnet_depthwise(L.ptr(x), L.ptr(w3), L.ptr(bias), L.ptr(stats), L.ptr(gamma), L.ptr(beta), L.ptr(prelu), L.ptr(out),
                                           L.ptr(part), B, Lf, Cc, int(dilation), L.dt(x), L.stream()), "storm_tasnet_depthwise")
    return out, part


def tasnet_decode(mask, enc, wd):
    """sigmoid(mask) * enc [B, L, N] through ConvTranspose1d(N, 1, win, stride = win // 2): fp32 [B, (L - 1) * stride + win]; wd [N, win] fp32"""
    B, Lf, N = enc.shape
    win = wd.shape[1]
    out = _alloc((B, (Lf - 1) * (win // 2) + win), torch.float32, enc)
    L.check(L.lib().storm_tasnet_decode(L.ptr(mask), L.ptr(enc), L.ptr(wd), L.ptr(out), B, Lf, N, win, L.dt(enc), L.stream()), "storm_tasnet_decode")
    return out
