"""ConvTasNet on the HIP engine: registry and refusals, the reference's state_dict, forward parity against the REFERENCE's own class
(fixture F22, tools/make_golden_convtasnet.py), every kernel of csrc/tasnet.h alone against torch, batch independence, the
DiscriminativeModel path of a time-domain backbone (FORCE_STFT_OUT) and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import convtasnet_cases as CC
from tests import option_nets as ON
from tests.backend import dev, tol  # noqa: F401
from tests.util import rel_l2

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2, torch.float16: 5e-3}          # tests/test_option_nets.py:TOL - the same comparison on NCSN++
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.bfloat16: "bf16", torch.float16: "fp16"}
# A norm's (mean, rstd) from the kernels' partial sums against torch's: a wave's (sum, sumsq) is reduced in fp64 and rounded ONCE to its fp32
# slot (2^-24 relative), the slots are summed in fp64; var = E[x^2] - mean^2 amplifies that by E[x^2] / var, which is < 10 for the data below
# (|mean| < 3 sigma).  torch's own fp32 statistics carry an error of the same order.  2e-6 = the fp32 bound of the kernel tests themselves.
STAT_TOL = 2e-6


def q(x, dtype):
    return x.to(dtype).float()


def build(name, dev):
    from storm_amd.backbones.convtasnet import ConvTasNet
    net = ConvTasNet(**CC.CASES[name])
    names, vals = CC.fill(net)
    return net.to(dev), names, vals


# ---- 1. registry -------------------------------------------------------------------------------------------------------------------------
def test_registry_knows_convtasnet_and_keeps_the_other_two_out():
    from storm_amd.backbones import BackboneRegistry
    from storm_amd.backbones.convtasnet import ConvTasNet
    assert BackboneRegistry.get_by_name("convtasnet") is ConvTasNet
    for name in ("gagnet", "ae-ncsnpp"):
        with pytest.raises(ValueError, match="registered upstream but not built here"):
            BackboneRegistry.get_by_name(name)


@pytest.mark.parametrize("kw,word", [(dict(causal=True), "causal"), (dict(kernel=5), "kernel"), (dict(enc_dim=100), "enc_dim"),
                                     (dict(feature_dim=12), "feature_dim")])
def test_refused_options_name_the_option(kw, word):
    from storm_amd.backbones.convtasnet import ConvTasNet
    with pytest.raises(NotImplementedError) as e:
        ConvTasNet(**kw)
    assert word in str(e.value)


def test_surface_of_the_reference_class():
    from argparse import ArgumentParser

    from storm_amd.backbones.convtasnet import ConvTasNet
    net = ConvTasNet()
    assert net.FORCE_STFT_OUT is True and (net.win, net.stride) == (32, 16)
    assert net.total_receptive_field == 16 * (3 + 2 * sum(2 ** i for s in range(3) for i in range(8) if (s, i) != (0, 0)))    # convtasnet.py:45, 296-300
    assert ConvTasNet.add_argparse_args(ArgumentParser()).parse_args(["--causal"]).causal is True
    with pytest.raises(RuntimeError, match="Input can only be 2 or 3 dimensional."):
        net(torch.zeros(1, 1, 2, 100))


# ---- 2. state_dict -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.CASES))
def test_state_dict_is_the_reference_layout(golden, name):
    from storm_amd.backbones.convtasnet import ConvTasNet
    g = golden["f22_convtasnet"]
    net = ConvTasNet(**CC.CASES[name])
    sd = net.state_dict()
    assert list(sd) == [str(s) for s in g[f"{name}_names"]]
    if name == "default":
        assert len(sd) == 345 and list(sd)[0] == "encoder.weight" and list(sd)[-1] == "decoder.weight"
    shapes = g[f"{name}_shapes"]
    for k, (key, v) in enumerate(sd.items()):
        assert tuple(v.shape) == tuple(int(s) for s in shapes[k][:v.dim()]), key
    names, vals = CC.fill(net)                                # load_state_dict(strict=True)
    assert np.array_equal(ON.sd_hash(vals), g[f"{name}_sdhash"])
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), vals.values()))
    slopes = [v for k, v in vals.items() if CC.is_slope(k)]
    assert slopes and all(0.1 <= float(v) <= 0.4 for v in slopes)


# ---- 3. forward against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,samples", CC.INPUTS)
def test_forward_vs_reference(dev, golden, name, samples, dtype):
    """The reference class's output on the same weights and input.  fp32: the project's 1e-4.  16 bit: max(TOL, 2 x the reference's own
    error when its torch modules run in that dtype, recorded in F22) - the engine rounds its stored activations at other points than torch."""
    g = golden["f22_convtasnet"]
    net, _, vals = build(name, dev)
    assert np.array_equal(ON.sd_hash(vals), g[f"{name}_sdhash"])
    net.set_compute_dtype(dtype)
    want = g[f"{name}_{samples}_y"]
    y = net(T(g[f"x_{samples}"]).to(dev))
    assert y.dtype == torch.float32 and tuple(y.shape) == want.shape        # the padded length, untrimmed
    bound = TOL[dtype] if dtype == torch.float32 else max(TOL[dtype], 2 * float(g[f"{name}_{samples}_referr_{TAG[dtype]}"]))
    err = rel_l2(y.cpu(), want)
    print(f"F22 {name} {samples} {dtype}: rel-L2 vs reference {err:.3e} (bound {bound:.1e})")
    assert err < bound, err
    if samples == 1000:
        assert y.shape[1] == 63 * 16 + 32 and max(b.dilation for b in net.TCN.TCN) >= 64       # 64 frames under a dilation of 128


# ---- 4. each kernel alone against torch --------------------------------------------------------------------------------------------------
def _stats_of(v):
    """torch's (mean, rstd) of GroupNorm(1, C, eps=1e-8) per row of v [B, ...] (fp64)"""
    v = v.double().flatten(1)
    mean = v.mean(1)
    return mean, 1.0 / torch.sqrt(v.var(1, unbiased=False) + 1e-8)


def _check_stats(part, stored, what):
    from storm_amd import ops
    st = ops.tasnet_gln_finalize(part, stored[0].numel()).cpu().double()
    mean, rstd = _stats_of(stored.float().cpu())
    e_mean = float(((st[:, 0] - mean) * rstd).abs().max())          # in units of sigma
    e_rstd = float(((st[:, 1] - rstd) / rstd).abs().max())
    print(f"{what}: mean {e_mean:.2e} sigma, rstd {e_rstd:.2e}")
    assert e_mean < STAT_TOL and e_rstd < STAT_TOL


def _pad_signal(x, win):
    stride = win // 2
    rest = win - (stride + x.shape[1] % win) % win
    return F.pad(x, (stride, rest + stride))[:, None]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Ts,N,win", [(1, 100, 8, 16), (3, 1037, 64, 32), (2, 4000, 256, 32)])
def test_encoder_kernel(dev, dtype, B, Ts, N, win):
    """pad_signal + Conv1d(1, N, win, stride = win / 2) against F.conv1d on the padded input; its partial sums give torch's mean and variance"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(1)
    x = 0.5 * torch.randn(B, Ts, generator=g) + 0.1
    w = torch.randn(N, 1, win, generator=g) / win ** 0.5
    enc, part = ops.tasnet_encode(x.to(dev), w[:, 0].t().contiguous().to(dev), dtype)
    want = F.conv1d(_pad_signal(x, win), w, stride=win // 2).transpose(1, 2)
    assert tuple(enc.shape) == tuple(want.shape) == (B, ops.tasnet_frames(Ts, win), N)
    err = rel_l2(enc.float().cpu(), q(want, dtype))
    print(f"tasnet_encode {(B, Ts, N, win)} {dtype}: rel-L2 {err:.3e}")
    assert err < tol(dtype, 2e-6, 5e-3)
    _check_stats(part, enc, "encoder partials")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc,Lf,d", [(8, 5, 1), (96, 64, 4), (512, 253, 128), (32, 64, 128)])
def test_depthwise_kernel(dev, dtype, Cc, Lf, d):
    """norm-on-load + 3-tap dilated depthwise convolution + bias + PReLU + the partial sums of reg2.  beta != 0 and gamma != 1: padding the
    raw tensor (instead of the normalised one) would add beta_c - mean rstd gamma_c at every out-of-range tap.  (32, 64, 128): d >= L."""
    from storm_amd import ops
    g = torch.Generator().manual_seed(2)
    B = 2
    x = q(1.5 * torch.randn(B, Lf, Cc, generator=g) + 0.7, dtype)
    gam, bet = 1 + 0.3 * torch.randn(Cc, generator=g), 0.5 + 0.3 * torch.randn(Cc, generator=g)
    w, b = torch.randn(Cc, 1, 3, generator=g) / 3 ** 0.5, 0.2 * torch.randn(Cc, generator=g)
    slope = torch.tensor([0.25])
    mean, rstd = _stats_of(x)
    st = torch.stack([mean, rstd], 1).float()
    out, part = ops.tasnet_depthwise(x.to(dtype).to(dev), w[:, 0].t().contiguous().to(dev), b.to(dev), (st.to(dev), gam.to(dev), bet.to(dev)), slope.to(dev), d)
    xn = ((x.double() - mean[:, None, None]) * rstd[:, None, None] * gam.double() + bet.double()).float().transpose(1, 2)
    want = F.prelu(F.conv1d(xn, w, b, padding=d, dilation=d, groups=Cc), slope).transpose(1, 2)
    err = rel_l2(out.float().cpu(), q(want, dtype))
    print(f"tasnet_depthwise {(Cc, Lf, d)} {dtype}: rel-L2 {err:.3e}")
    assert err < tol(dtype, 2e-6, 5e-3)
    _check_stats(part, out, "depthwise partials")


PW_SHAPES = [(8, 32, 7), (128, 512, 253), (512, 256, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("Cin,Cout,Lf", PW_SHAPES)
def test_pointwise_kernel(dev, dtype, Cin, Cout, Lf, fused):
    """the 1x1 convolution on the MFMA, plain (bias only) and with norm-on-load + PReLU epilogue + partial sums"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(3)
    B = 2
    x = q(1.2 * torch.randn(B, Lf, Cin, generator=g) + 0.4, dtype)
    w, b = q(torch.randn(Cout, Cin, generator=g) / Cin ** 0.5, dtype), 0.2 * torch.randn(Cout, generator=g)
    xd, wd, bd = x.to(dtype).to(dev), w.to(dtype).to(dev), b.to(dev)
    if fused:
        gam, bet = 1 + 0.3 * torch.randn(Cin, generator=g), 0.5 + 0.3 * torch.randn(Cin, generator=g)
        slope = torch.tensor([0.3])
        mean, rstd = _stats_of(x)
        st = torch.stack([mean, rstd], 1).float()
        out, part = ops.tasnet_pointwise(xd, wd, bd, dtype, norm=(st.to(dev), gam.to(dev), bet.to(dev)), prelu_out=slope.to(dev), partials=True)
        xn = q(((x.double() - mean[:, None, None]) * rstd[:, None, None] * gam.double() + bet.double()).float(), dtype)      # the MFMA operand
        want = F.prelu(F.conv1d(xn.transpose(1, 2), w[:, :, None], b), slope).transpose(1, 2)
    else:
        out = ops.tasnet_pointwise(xd, wd, bd, dtype)
        want = F.conv1d(x.transpose(1, 2), w[:, :, None], b).transpose(1, 2)
    assert out.dtype == dtype
    err = rel_l2(out.float().cpu(), q(want, dtype))
    print(f"tasnet_pointwise {(Cin, Cout, Lf)} fused={fused} {dtype}: rel-L2 {err:.3e}")
    assert err < tol(dtype, 2e-6, 5e-3)
    if fused:
        _check_stats(part, out, "pointwise partials")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,BN,Lf", [(32, 8, 7), (512, 128, 253), (128, 32, 64)])
def test_pointwise_res_skip(dev, dtype, H, BN, Lf):
    """res_out and skip_out as one GEMM over two consecutive blocks: `output` and `skip_connection` (fp32) accumulate in place, the latter
    from zero; then the next block's conv1d reads the fp32 `output` (rounded on load) and the head applies its PReLU on load of `skip`."""
    from storm_amd import ops
    g = torch.Generator().manual_seed(4)
    B = 2
    output0 = torch.randn(B, Lf, BN, generator=g)
    output, skip = output0.clone().to(dev), torch.zeros(B, Lf, BN).to(dev)
    want_out, want_skip = output0.clone(), torch.zeros(B, Lf, BN)
    for _ in range(2):
        x = q(1.2 * torch.randn(B, Lf, H, generator=g) + 0.4, dtype)
        gam, bet = 1 + 0.3 * torch.randn(H, generator=g), 0.5 + 0.3 * torch.randn(H, generator=g)
        wr, ws = (q(torch.randn(BN, H, generator=g) / H ** 0.5, dtype) for _ in range(2))
        br, bs = 0.2 * torch.randn(BN, generator=g), 0.2 * torch.randn(BN, generator=g)
        mean, rstd = _stats_of(x)
        st = torch.stack([mean, rstd], 1).float()
        assert ops.tasnet_pointwise(x.to(dtype).to(dev), torch.cat([wr, ws]).to(dtype).to(dev), torch.cat([br, bs]).to(dev), dtype,
                                    norm=(st.to(dev), gam.to(dev), bet.to(dev)), res_skip=(output, skip)) is None
        xn = q(((x.double() - mean[:, None, None]) * rstd[:, None, None] * gam.double() + bet.double()).float(), dtype).transpose(1, 2)
        want_out += F.conv1d(xn, wr[:, :, None], br).transpose(1, 2)
        want_skip += F.conv1d(xn, ws[:, :, None], bs).transpose(1, 2)
    e_out, e_skip = rel_l2(output.cpu(), want_out), rel_l2(skip.cpu(), want_skip)
    print(f"tasnet_pointwise res_skip {(H, BN, Lf)} {dtype}: output {e_out:.3e} skip {e_skip:.3e}")
    assert output.dtype == skip.dtype == torch.float32
    assert e_out < tol(dtype, 2e-6, 5e-3) and e_skip < tol(dtype, 2e-6, 5e-3)
    # fp32 operand: conv1d of the next block (PReLU epilogue, partials) and the head (PReLU on load)
    w1, b1 = q(torch.randn(H, BN, generator=g) / BN ** 0.5, dtype), 0.2 * torch.randn(H, generator=g)
    slope = torch.tensor([0.2])
    h, part = ops.tasnet_pointwise(output, w1.to(dtype).to(dev), b1.to(dev), dtype, prelu_out=slope.to(dev), partials=True)
    want = F.prelu(F.conv1d(q(output.cpu(), dtype).transpose(1, 2), w1[:, :, None], b1), slope).transpose(1, 2)
    assert h.dtype == dtype and rel_l2(h.float().cpu(), q(want, dtype)) < tol(dtype, 2e-6, 5e-3)
    _check_stats(part, h, "conv1d partials")
    m = ops.tasnet_pointwise(skip, w1.to(dtype).to(dev), b1.to(dev), dtype, prelu_in=slope.to(dev))
    want = F.conv1d(q(F.prelu(skip.cpu(), slope), dtype).transpose(1, 2), w1[:, :, None], b1).transpose(1, 2)
    e = rel_l2(m.float().cpu(), q(want, dtype))
    print(f"tasnet_pointwise PReLU on load {(BN, H, Lf)} {dtype}: rel-L2 {e:.3e}")
    assert e < tol(dtype, 2e-6, 5e-3)
    bn = ops.tasnet_pointwise(h, w1.t().contiguous().to(dtype).to(dev), b1[:BN].contiguous().to(dev), dtype, out_f32=True)     # the BN form: fp32 out
    want = F.conv1d(h.float().cpu().transpose(1, 2), w1.t()[:, :, None], b1[:BN]).transpose(1, 2)
    assert bn.dtype == torch.float32 and rel_l2(bn.cpu(), want) < tol(dtype, 2e-6, 5e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lf,N,win", [(1, 8, 16), (7, 64, 32), (253, 256, 32)])
def test_decoder_kernel(dev, dtype, Lf, N, win):
    """sigmoid, multiply and ConvTranspose1d(N, 1, win, stride = win / 2) against torch; a gather without atomics: two runs, equal bits"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(5)
    B = 2
    mask, enc = q(2 * torch.randn(B, Lf, N, generator=g), dtype), q(torch.randn(B, Lf, N, generator=g), dtype)
    w = torch.randn(N, 1, win, generator=g) / N ** 0.5
    args = (mask.to(dtype).to(dev), enc.to(dtype).to(dev), w[:, 0].contiguous().to(dev))
    out = ops.tasnet_decode(*args)
    want = F.conv_transpose1d((torch.sigmoid(mask) * enc).transpose(1, 2), w, stride=win // 2)[:, 0]
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape) == (B, (Lf - 1) * (win // 2) + win)
    err = rel_l2(out.cpu(), want)
    print(f"tasnet_decode {(Lf, N, win)} {dtype}: rel-L2 {err:.3e}")
    assert err < tol(dtype, 2e-6, 5e-3)
    assert torch.equal(out, ops.tasnet_decode(*args))


def test_kernel_entry_points_refuse_bad_shapes(dev):
    from storm_amd import _lib as L
    from storm_amd import ops
    x = torch.zeros(1, 4, 12).to(dev)
    with pytest.raises(L.StormError, match="multiples of 8"):
        ops.tasnet_pointwise(x, torch.zeros(8, 12).to(dev), torch.zeros(8).to(dev), torch.float32)


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(dev):
    """the norm statistics are per row: B = 3 rows through forward equal each row's own B = 1 call"""
    net, _, _ = build("small", dev)
    x = 0.1 * torch.randn(3, 1037, generator=torch.Generator().manual_seed(6))
    x[1] *= 5.0                                                # rows of different level: shared statistics would show
    y = net(x.to(dev)).cpu()
    for b in range(3):
        e = rel_l2(y[b], net(x[b:b + 1].to(dev)).cpu()[0])
        assert e < 1e-6, (b, e)
    assert torch.equal(net(x[:, None].to(dev)).cpu(), y)       # [B, 1, T] is [B, T]


# ---- 6. DiscriminativeModel --------------------------------------------------------------------------------------------------------------
def test_discriminative_model_enhance_vs_reference(dev, golden):
    """DiscriminativeModel with a time-domain backbone (model.py:322-370): spectrogram -> iSTFT -> net -> STFT -> to_audio, against the
    reference's own enhance() on the same weights (F22), F9's bound"""
    from storm_amd.model import DiscriminativeModel
    g = golden["f22_convtasnet"]
    m = DiscriminativeModel(backbone="convtasnet", **CC.MODEL_KW, **CC.CASES[CC.ENHANCE_CASE])
    CC.fill(m.dnn)
    m.eval(no_ema=True)
    m = m.to(dev)
    out = m.enhance(T(g["enhance_wav"]).to(dev)).cpu()
    err = rel_l2(out, g["enhance_out"])
    print(f"F22 DiscriminativeModel(convtasnet).enhance: rel-L2 vs reference {err:.3e}")
    assert out.shape == (CC.ENHANCE_SAMPLES,) and err < 1e-4


def test_storm_with_a_convtasnet_denoiser_fails_as_upstream(dev):
    """StochasticRegenerationModel hands its denoiser a spectrogram: the reference's own RuntimeError"""
    from storm_amd.model import StochasticRegenerationModel
    s = StochasticRegenerationModel(backbone_denoiser="convtasnet", backbone_score="ncsnpp", nf=8, **CC.MODEL_KW, **CC.CASES["small"])
    s.eval(no_ema=True)
    s = s.to(dev)
    with pytest.raises(RuntimeError, match="Input can only be 2 or 3 dimensional."):
        s.enhance(0.1 * torch.randn(1, 4000, generator=torch.Generator().manual_seed(7)).to(dev), N=1)


# ---- 7. command line ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_enhancement_cli_denoiser_only(tmp_path):
    """enhancement.py --mode denoiser-only on a ConvTasNet checkpoint, no new flag: the enhanced files have the input lengths and equal
    model.enhance of the same files"""
    from scipy.io import wavfile

    from storm_amd.backbones.convtasnet import ConvTasNet
    from storm_amd.model import DiscriminativeModel
    kw = CC.CASES["small"]
    _, vals = CC.fill(ConvTasNet(**kw))
    path = os.path.join(tmp_path, "tasnet.ckpt")
    torch.save({"state_dict": {"dnn." + k: v for k, v in vals.items()}, "hyper_parameters": dict(backbone="convtasnet", **CC.MODEL_KW, **kw)}, path)
    noisy, out = os.path.join(tmp_path, "noisy"), os.path.join(tmp_path, "enhanced")
    os.makedirs(noisy)
    g = torch.Generator().manual_seed(9)
    wavs = [0.1 * torch.randn(n, generator=g) for n in (6000, 4321)]
    for i, w in enumerate(wavs):
        wavfile.write(os.path.join(noisy, f"u{i}.wav"), 16000, w.numpy().astype(np.float32))
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=ROOT).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "enhancement.py"), "--test_dir", noisy, "--enhanced_dir", out, "--ckpt", path,
                        "--mode", "denoiser-only"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # (no 'ema' entry in this checkpoint)
        m = DiscriminativeModel.load_from_checkpoint(path, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    m.eval(no_ema=False)
    m = m.cuda()
    for i, w in enumerate(wavs):
        sr, x = wavfile.read(os.path.join(out, f"u{i}.wav"))
        assert sr == 16000 and x.shape == (len(w),) and np.isfinite(x).all()
        want = m.enhance(w[None]).cpu()
        assert float(want.abs().max()) > 0 and rel_l2(T(x), want) < 1e-6, i
