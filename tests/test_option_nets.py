"""NCSN++ constructor options beyond the StoRM default set (fir=False, skip_rescale=False, progressive / progressive_input = 'none',
progressive_combine='cat', centered, conditional, scale_by_sigma, dropout): state_dict contract and forward parity against the REFERENCE's
own class (fixture F21, tools/make_golden_options.py), the new kernels alone against torch, the grouped stream, the C ABI's _ex forms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import option_nets as ON
from tests.backend import dev, nchw, nhwc, switch, tol  # noqa: F401
from tests.util import rel_l2

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's bounds for the same comparison on F2 (tests/test_net.py:14-16, 454)
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2, torch.float16: 5e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def q(x, dtype):
    return x.to(dtype).float()


def build(name, dev):
    from storm_amd.backbones.ncsnpp import NCSNpp
    net = NCSNpp(**ON.CASES[name])
    names, vals = ON.fill_module(net)
    return net.to(dev), names, vals


@pytest.mark.parametrize("name", list(ON.CASES))
def test_option_net_has_the_reference_state_dict(golden, name):
    """NCSNpp(**kw) owns the reference class's state_dict - same keys, order and shapes (recorded from the reference in F21) - and loads
    it strictly; the seeded fill reproduces the very weights the reference ran with (hash)."""
    from storm_amd.backbones.ncsnpp import NCSNpp
    g = golden["f21_option_nets"]
    net = NCSNpp(**ON.CASES[name])
    sd = net.state_dict()
    assert list(sd) == [str(s) for s in g[f"{name}_names"]]
    shapes = g[f"{name}_shapes"]
    for k, (key, v) in enumerate(sd.items()):
        assert tuple(v.shape) == tuple(int(s) for s in shapes[k][:v.dim()]), key
    names, vals = ON.fill_module(net)                         # load_state_dict(strict=True)
    assert np.array_equal(ON.sd_hash(vals), g[f"{name}_sdhash"])
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), vals.values()))


@pytest.mark.parametrize("name", list(ON.CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_option_net_forward_vs_reference(dev, golden, name, dtype):
    """forward of every option case against the reference class's output on the same weights and input"""
    g = golden["f21_option_nets"]
    net, _, vals = build(name, dev)
    assert np.array_equal(ON.sd_hash(vals), g[f"{name}_sdhash"])
    net.set_compute_dtype(dtype)
    xkey, _ = ON.case_input(ON.CASES[name])
    y = net(T(g[xkey]).to(dev), T(g["t"]).to(dev))
    err = rel_l2(y.cpu(), g[f"{name}_y"])
    print(f"F21 {name} {dtype}: rel-L2 vs reference {err:.3e}")
    assert err < TOL[dtype], err


@pytest.mark.parametrize("kw,word", [(dict(resblock_type="ddpm"), "resblock_type"), (dict(progressive="residual"), "progressive=residual"),
                                     (dict(progressive_input="residual"), "progressive_input"), (dict(nonlinearity="relu"), "nonlinearity"),
                                     (dict(fir_kernel=(1, 2, 1)), "fir_kernel"), (dict(spatial_channels=2), "spatial_channels"),
                                     (dict(embedding_type="positional"), "embedding_type"), (dict(fir=False), "fir=False")])
def test_refused_options_name_the_option(kw, word):
    from storm_amd.backbones.ncsnpp import NCSNpp
    with pytest.raises(NotImplementedError) as e:
        NCSNpp(nf=8, **kw)
    assert word in str(e.value)


# ---- the new kernels alone ---------------------------------------------------------------------------------------------------------
# shapes: (B, C, H, W) - one and several row strips / column blocks (odd and even counts), ragged channel groups, and the channel counts
# that run with 16 / 32 slots of a pixel per workgroup (both NS paths; STORM_GN_WIDE = 0 forces 8)
NAIVE_SHAPES = [(2, 24, 6, 10), (2, 72, 20, 36), (1, 160, 38, 70), (1, 128, 6, 20), (2, 256, 10, 12)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("resample", [3, 4])
@pytest.mark.parametrize("shape", NAIVE_SHAPES)
def test_groupnorm_naive_resample_fused(dev, dtype, resample, shape, switch):
    """h = resample(SiLU(GN(cat[xa, xb]))) and x = resample(cat[xa, xb]) of a BigGAN up / down block built with fir=False, in one pass:
    nearest x2 (3) / 2 x 2 mean (4).  Tolerances of test_groupnorm_fir_fused (tests/test_ops.py) for the same dtype; the nearest copy of
    the raw tensor is bit-exact in every dtype."""
    from storm_amd import ops
    g = torch.Generator().manual_seed(5)
    B, Cc, H, W = shape
    x = torch.randn(B, Cc, H, W, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    Ca = Cc // 8 // 2 * 8 if Cc >= 16 else Cc                       # two-input form: cat([xa, xb], channel)
    xa = nhwc(x[:, :Ca]).to(dtype).to(dev)
    xb = nhwc(x[:, Ca:]).to(dtype).to(dev) if Ca < Cc else None
    st = ops.gn_stats(xa, xb)
    act, raw = ops.gn_apply(xa, st, gam.to(dev), bet.to(dev), xb=xb, resample=resample)
    xq = q(x, dtype)
    rs = (lambda v: F.interpolate(v, scale_factor=2, mode="nearest")) if resample == 3 else (lambda v: F.avg_pool2d(v, 2))
    want_act = rs(F.silu(F.group_norm(xq, min(Cc // 4, 32), gam, bet, eps=1e-6)))
    e_act, e_raw = rel_l2(nchw(act.float().cpu()), want_act), rel_l2(nchw(raw.float().cpu()), rs(xq))
    print(f"gn_apply resample={resample} {shape} {dtype}: act {e_act:.3e} raw {e_raw:.3e}")
    assert e_act < tol(dtype, 2e-6, 5e-3) and e_raw < tol(dtype, 2e-6, 5e-3)
    if resample == 3:
        assert torch.equal(nchw(raw.cpu()).float(), rs(xq))             # a copy
    switch("STORM_GN_WIDE", 0)
    act8, raw8 = ops.gn_apply(xa, st, gam.to(dev), bet.to(dev), xb=xb, resample=resample)
    assert torch.equal(act, act8) and torch.equal(raw, raw8)
    for rows in (4, 8):                                                # rows per strip: the same bits whatever the strips
        switch("STORM_GN_ROWS", rows)
        actr, rawr = ops.gn_apply(xa, st, gam.to(dev), bet.to(dev), xb=xb, resample=resample)
        assert torch.equal(act, actr) and torch.equal(raw, rawr)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,n_levels,centered", [((2, 16, 24), 3, 0), ((1, 32, 64), 4, 0), ((3, 8, 40), 2, 1), ((1, 64, 64), 4, 1)])
def test_mean_input_pyramid(dev, dtype, shape, n_levels, centered):
    """storm_input_pyramid_ex(mean=1): packing (2x - 1 unless centered) + the avg_pool2d(2) chain of fir=False in one launch, and the
    continuation of a deeper pyramid from a given level 0"""
    from storm_amd import _lib as L
    B, Fq, Tt = shape
    g = torch.Generator().manual_seed(3)
    cplx = [(torch.randn(B, Fq, Tt, dtype=torch.complex64, generator=g) * 0.5).to(dev) for _ in range(2)]
    x = torch.cat([torch.view_as_real(c.cpu()).permute(0, 3, 1, 2) for c in cplx], 1)        # [B, 4, F, T]: (re, im) per input
    if not centered:
        x = 2 * x - 1
    levels = [torch.zeros(B, Fq >> k, Tt >> k, 8, dtype=dtype, device=dev) for k in range(n_levels)]
    views = [torch.view_as_real(c) for c in cplx]
    arr = (C.c_void_p * 2)(*[L.ptr(v) for v in views])
    lv = (C.c_void_p * n_levels)(*[L.ptr(v) for v in levels])
    L.check(L.lib().storm_input_pyramid_ex(arr, 2, lv, n_levels, B, Fq, Tt, 1, centered, L.dt(dtype), L.stream()), "storm_input_pyramid_ex")
    want = q(x, dtype)
    for k in range(n_levels):
        got = nchw(levels[k].float().cpu())
        assert torch.equal(got[:, 4:], torch.zeros_like(got[:, 4:]))
        if dtype == torch.float32 and k == 0:
            assert torch.equal(got[:, :4], want)
        assert rel_l2(got[:, :4], want) < tol(dtype, 2e-6, 5e-3), k
        want = q(F.avg_pool2d(want, 2), dtype)
    # continuation: levels[1] read, two more levels written - the same bits as the one-launch chain
    if n_levels >= 3:
        cont = [levels[1]] + [torch.zeros_like(levels[k]) for k in range(2, n_levels)]
        lc = (C.c_void_p * len(cont))(*[L.ptr(v) for v in cont])
        L.check(L.lib().storm_input_pyramid_ex(None, 0, lc, len(cont), B, Fq >> 1, Tt >> 1, 1, centered, L.dt(dtype), L.stream()), "storm_input_pyramid_ex")
        for a, b in zip(cont[1:], levels[2:]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npix,Cc", [(37, 16), (8 * 25, 64), (1000, 192), (513, 256)])
def test_combine_cat(dev, dtype, npix, Cc):
    """Combine(method='cat'): cat([conv1x1(x) + bias, h], channel) in one pass (storm_combine_cat); the copy of h is bit-exact"""
    from storm_amd import _lib as L
    from storm_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.zeros(1, npix, 1, 8)
    x[..., :6] = torch.randn(1, npix, 1, 6, generator=g)
    w, b = torch.randn(Cc, 6, 1, 1, generator=g) / 6 ** 0.5, 0.1 * torch.randn(Cc, generator=g)
    h = torch.randn(1, npix, 1, Cc, generator=g)
    xd, hd = x.to(dtype).to(dev), h.to(dtype).to(dev)
    per16 = 4 if dtype == torch.float32 else 8
    CinP = -(-6 // (2 * per16)) * 2 * per16
    wp = ops.pack_conv_weight(w.to(dev), dtype)
    out = torch.zeros(1, npix, 1, 2 * Cc, dtype=dtype, device=dev)
    L.check(L.lib().storm_combine_cat(L.ptr(xd), L.ptr(wp), CinP, L.ptr(b.to(dev)), L.ptr(hd), L.ptr(out), npix, Cc, L.dt(dtype), L.stream()), "storm_combine_cat")
    want = torch.cat([F.conv2d(nchw(q(x[..., :6], dtype)), q(w, dtype), b), nchw(q(h, dtype))], 1)
    got = nchw(out.float().cpu())
    assert torch.equal(got[:, Cc:], want[:, Cc:])
    assert rel_l2(got[:, :Cc], want[:, :Cc]) < tol(dtype, 2e-6, 5e-3)


# ---- grouped stream -------------------------------------------------------------------------------------------------------------------
def test_option_net_enhance_stream_equals_own_runs(dev, switch):
    """An option net (fir=False, progressive='none', 'cat', skip_rescale=False) through ScoreModel.enhance_stream: two micro-batches of
    different length meet in grouped network calls (storm_ncsnpp_forward_group: the new ops run problem by problem inside it) and return
    what their own enhance_batch calls return - bit-equal per row in batch-invariant mode, the rule of the existing grouped tests."""
    from oracle import sde_ref as SR
    from storm_amd.model import ScoreModel
    kw = dict(fir=False, progressive="none", progressive_combine="cat", skip_rescale=False)
    m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5, nf=8, **kw)
    ON.fill_module(m.dnn)
    m.eval(no_ema=True)
    m = m.to(dev)
    switch("STORM_BATCH_INVARIANT", 1)
    g = torch.Generator().manual_seed(31)
    lens = [[5003], [9000]] if dev.type == "cpu" else [[5003, 4500], [9000]]
    batches = []
    for bl in lens:
        y = torch.zeros(len(bl), max(bl))
        for k, n in enumerate(bl):
            y[k, :n] = 0.1 * torch.randn(n, generator=g)
        batches.append((y.to(dev), bl if len(set(bl)) > 1 else None))
    frames = [-(-(1 + max(bl) // 128) // 64) * 64 for bl in lens]
    N = 1
    draws = [[SR.complex_randn((len(bl), 1, 256, f), torch.Generator().manual_seed(100 * p + i)).to(dev) for i in range(1 + 2 * N)]
             for p, (bl, f) in enumerate(zip(lens, frames))]
    skw = dict(N=N, corrector="ald", snr=0.5)

    def fns():
        return [(lambda it=iter(d): next(it)) for d in draws]
    own = [m.enhance_batch(yb, lengths=bl, noise_fn=fn, **skw) for (yb, bl), fn in zip(batches, fns())]
    outs = m.enhance_stream(batches, noise_fns=fns(), **skw)
    assert m.last_group_calls is not None and m.last_group_calls[0] >= 1
    for p in range(len(lens)):
        assert torch.isfinite(outs[p]).all()
        assert torch.equal(outs[p], own[p]), p


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_option_net_forward_group(dev, dtype):
    """storm_ncsnpp_forward_group on the wide 'cat' net (16-bit: its 3x3 layers share launches, the non-FIR / cat ops run problem by
    problem): never a failed check, every problem within the 16-bit bound of its own call, fp32 bit for bit"""
    from storm_amd.backbones.ncsnpp import NCSNpp
    net = NCSNpp(**dict(ON.WIDE, progressive_combine="cat", fir=False, progressive="none"))
    ON.fill_module(net)
    net = net.to(dev).set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(5)
    shapes = [(2, 64), (1, 128)] if dev.type != "cpu" else [(1, 32), (1, 64)]
    ins = [[(torch.randn(B, 16, Tt, dtype=torch.complex64, generator=g) * 0.5).to(dev) for _ in range(2)] for B, Tt in shapes]
    ts = [(0.05 + 0.9 * torch.rand(B, generator=g)).to(dev) for B, _ in shapes]
    own = [net.forward_parts(i, t) for i, t in zip(ins, ts)]
    grp = net.forward_parts_group(ins, ts)
    for a, b in zip(grp, own):
        if dtype == torch.float32:
            assert torch.equal(a, b)
        else:
            assert rel_l2(a.cpu(), b.cpu()) < TOL[dtype]


# ---- the C ABI's _ex forms ------------------------------------------------------------------------------------------------------------
def test_create_ex_with_default_options_equals_create(dev):
    """storm_ncsnpp_create_ex with STORM_NCSNPP_CONFIG_EX_DEFAULTS' values = storm_ncsnpp_create: same tensor list, arena size, output bits;
    another struct_size is refused with the ABI's error code"""
    from oracle import ncsnpp_ref as NR
    from storm_amd import _lib as L
    from storm_amd.backbones.ncsnpp import NCSNpp
    lib = L.lib()
    net = NCSNpp(nf=8, input_channels=4)
    net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=7))
    net = net.to(dev)
    c0, c1 = net.c_config(), net.c_config_ex()
    n = lib.storm_ncsnpp_num_tensors(C.byref(c0))
    assert n == lib.storm_ncsnpp_num_tensors_ex(C.byref(c1)) == len(net.state_dict())
    assert lib.storm_ncsnpp_arena_bytes(C.byref(c0), L.F32) == lib.storm_ncsnpp_arena_bytes_ex(C.byref(c1), L.F32)
    nm0, nm1, nd, sh = C.create_string_buffer(128), C.create_string_buffer(128), C.c_int(), (C.c_longlong * 4)()
    for i in range(n):
        L.check(lib.storm_ncsnpp_tensor_info(C.byref(c0), i, nm0, 128, C.byref(nd), sh), "tensor_info")
        L.check(lib.storm_ncsnpp_tensor_info_ex(C.byref(c1), i, nm1, 128, C.byref(nd), sh), "tensor_info_ex")
        assert nm0.value == nm1.value
    sd = [v.detach().to(device=dev, dtype=torch.float32).contiguous() for v in net.state_dict().values()]
    ptrs = (C.c_void_p * n)(*[L.ptr(t) for t in sd])
    g = torch.Generator().manual_seed(2)
    B, Fq, Tt = 1, 32, 32
    xs = [(torch.randn(B, Fq, Tt, dtype=torch.complex64, generator=g) * 0.5).to(dev) for _ in range(2)]
    t = torch.tensor([0.4]).to(dev)
    parts = (C.c_void_p * 2)(*[L.ptr(torch.view_as_real(x)) for x in xs])
    outs = []
    for create, cfg in ((lib.storm_ncsnpp_create, c0), (lib.storm_ncsnpp_create_ex, c1)):
        h = C.c_void_p()
        L.check(create(C.byref(cfg), ptrs, n, L.F32, None, L.stream(), C.byref(h)), "create")
        nb = lib.storm_ncsnpp_workspace_bytes(h, B, Fq, Tt)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.zeros(B, 1, Fq, Tt, dtype=torch.complex64, device=dev)
        L.check(lib.storm_ncsnpp_forward(h, parts, 2, L.ptr(t), L.ptr(torch.view_as_real(out)), L.ptr(ws), nb, B, Fq, Tt, 0, L.stream()), "forward")
        outs.append(out.cpu())
        lib.storm_ncsnpp_destroy(h)
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().sum()) > 0
    bad = net.c_config_ex()
    bad.struct_size -= 4
    h = C.c_void_p()
    assert lib.storm_ncsnpp_num_tensors_ex(C.byref(bad)) == -1
    assert lib.storm_ncsnpp_arena_bytes_ex(C.byref(bad), L.F32) == -1
    rc = lib.storm_ncsnpp_create_ex(C.byref(bad), ptrs, n, L.F32, None, L.stream(), C.byref(h))
    assert rc == -1 and not h.value and b"struct_size" in lib.storm_last_error()
    # fir=False with the output pyramid: refused by the library as well
    bad = net.c_config_ex()
    bad.fir = 0
    assert lib.storm_ncsnpp_num_tensors_ex(C.byref(bad)) == -1 and b"fir=False" in lib.storm_last_error()


def test_default_net_plans_the_same_program(dev):
    """options at their defaults: the planned op list of the _ex path is the one of the plain entry points (the interpreter's new
    fields stay zero)"""
    from storm_amd import _lib as L
    from storm_amd.backbones.ncsnpp import NCSNpp
    from storm_amd.backbones.plan import OP_COMBINE_CAT, OP_GN_APPLY, OP_INPUT_PYRAMID
    net = NCSNpp(nf=8, input_channels=4).to(dev)
    ops, n, _ = net.program(1, 32, 32)
    for k in range(n):
        assert ops[k].code != OP_COMBINE_CAT
        if ops[k].code == OP_GN_APPLY:
            assert ops[k].i[7] in (0, 1, 2)
        if ops[k].code == OP_INPUT_PYRAMID:
            assert ops[k].i[5] == 0 and ops[k].i[6] == 0
    net2 = NCSNpp(nf=8, input_channels=4, fir=False, progressive="none", progressive_combine="cat", centered=True).to(dev)
    ops2, n2, _ = net2.program(1, 32, 32)
    codes = [ops2[k].code for k in range(n2)]
    assert codes.count(OP_COMBINE_CAT) == 3
    assert sorted(ops2[k].i[7] for k in range(n2) if ops2[k].code == OP_GN_APPLY and ops2[k].i[7]) == [3, 3, 3, 4, 4, 4]
    assert all(ops2[k].i[5] == 1 and ops2[k].i[6] == 1 for k in range(n2) if ops2[k].code == OP_INPUT_PYRAMID)
