"""ConvTasNet - drop-in for sgmse/backbones/convtasnet.py (ConvTasNet :13, TCN :269, DepthConv1d :227): the time-domain predictive
denoiser of ``train.py --backbone convtasnet`` / ``enhancement.py --mode denoiser-only``.

The modules below only HOLD the reference's parameters (same names, order and shapes, so its checkpoints load strictly); the forward
runs on the HIP kernels of csrc/tasnet.h through storm_amd.ops.tasnet_*: encoder (+ pad_signal), the 1x1 convolutions as MFMA GEMMs
with the global layer norms applied on load, the dilated depthwise convolution, and the masking + decoder.  No torch arithmetic.

Refused (NotImplementedError naming the option): causal=True (cLN is a prefix scan over time - not built), kernel != 3 (the
reference's own residual add fails there: the padding stays 2^i, convtasnet.py:293), channel counts that are not multiples of 8.
"""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from .shared import BackboneRegistry


class _Holder(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError("parameter holder: the network runs through ConvTasNet.forward on the HIP engine")


class DepthConv1d(_Holder):
    """convtasnet.py:227-254 (non-causal, skip=True)"""

    def __init__(self, input_channel, hidden_channel, kernel, padding, dilation):
        super().__init__()
        self.dilation = dilation
        self.conv1d = nn.Conv1d(input_channel, hidden_channel, 1)
        self.dconv1d = nn.Conv1d(hidden_channel, hidden_channel, kernel, dilation=dilation, groups=hidden_channel, padding=padding)
        self.res_out = nn.Conv1d(hidden_channel, input_channel, 1)
        self.nonlinearity1 = nn.PReLU()
        self.nonlinearity2 = nn.PReLU()
        self.reg1 = nn.GroupNorm(1, hidden_channel, eps=1e-08)
        self.reg2 = nn.GroupNorm(1, hidden_channel, eps=1e-08)
        self.skip_out = nn.Conv1d(hidden_channel, input_channel, 1)


class TCN(_Holder):
    """convtasnet.py:269-312 (non-causal, dilated, skip=True)"""

    def __init__(self, input_dim, output_dim, BN_dim, hidden_dim, layer, stack, kernel=3):
        super().__init__()
        self.LN = nn.GroupNorm(1, input_dim, eps=1e-8)
        self.BN = nn.Conv1d(input_dim, BN_dim, 1)
        self.receptive_field = 0
        self.TCN = nn.ModuleList([])
        for s in range(stack):
            for i in range(layer):
                self.TCN.append(DepthConv1d(BN_dim, hidden_dim, kernel, padding=2 ** i, dilation=2 ** i))
                self.receptive_field += kernel if (i == 0 and s == 0) else (kernel - 1) * 2 ** i
        self.output = nn.Sequential(nn.PReLU(), nn.Conv1d(BN_dim, output_dim, 1))


@BackboneRegistry.register("convtasnet")
class ConvTasNet(nn.Module):
    def __init__(self, fs=16000, win=2, enc_dim=256, feature_dim=128, layer=8, stack=3, kernel=3, causal=False, **kwargs):
        super().__init__()
        if causal:
            raise NotImplementedError("ConvTasNet(causal=True): cLN (a cumulative norm: prefix scan over time) is not built on this engine")
        if kernel != 3:
            raise NotImplementedError(f"ConvTasNet(kernel={kernel}): only kernel=3 - the reference's own residual add fails otherwise "
                                      "(the padding stays 2^i, convtasnet.py:293)")
        for name, v in (("enc_dim", enc_dim), ("feature_dim", feature_dim)):
            if v <= 0 or v % 8:
                raise NotImplementedError(f"ConvTasNet({name}={v}): channel counts are multiples of 8 (16-byte channel slots)")
        self.num_spk = 1
        self.FORCE_STFT_OUT = True
        self.enc_dim = enc_dim
        self.win = int(fs * win / 1000)
        self.stride = self.win // 2
        if self.win < 2:
            raise NotImplementedError(f"ConvTasNet(fs={fs}, win={win}): a window of {self.win} samples")
        self.encoder = nn.Conv1d(1, self.enc_dim, self.win, bias=False, stride=self.stride)
        self.feature_dim, self.layer, self.stack, self.kernel, self.causal = feature_dim, layer, stack, kernel, causal
        self.TCN = TCN(self.enc_dim, self.num_spk * self.enc_dim, self.feature_dim, self.feature_dim * 4, self.layer, self.stack, self.kernel)
        self.total_receptive_field = self.stride * self.TCN.receptive_field
        self.decoder = nn.ConvTranspose1d(self.enc_dim, 1, self.win, bias=False, stride=self.stride)
        self.compute_dtype = torch.float32
        self._packed = {}
        self.register_load_state_dict_post_hook(lambda m, keys: m.invalidate())

    @staticmethod
    def add_argparse_args(parser):
        parser.add_argument("--causal", action="store_true", default=False)
        return parser

    # ---- engine state ----------------------------------------------------------------------
    def set_compute_dtype(self, dtype):
        """torch.float32 (exact fp32 MFMA) or torch.bfloat16 / torch.float16 (16-bit MFMA operands and activations; fp32 accumulation,
        statistics and running sums of the TCN)"""
        L.dt(dtype)
        self.compute_dtype = dtype
        return self

    def invalidate(self):
        """Call after changing parameters in place (e.g. EMA swap): the weights are re-packed lazily."""
        self._packed = {}

    def _apply(self, fn, *a, **k):
        self.invalidate()
        return super()._apply(fn, *a, **k)

    def _pack(self, dtype, device):
        """the engine's weight layout, built once per (dtype, device): GEMM matrices [Cout, Cin] in dtype, everything else fp32"""
        key = (dtype, str(device))
        if key in self._packed:
            return self._packed[key]

        def f32(p):
            return p.detach().to(device=device, dtype=torch.float32).contiguous()

        def mat(*convs):
            return torch.cat([f32(c.weight)[:, :, 0] for c in convs], 0).to(dtype).contiguous()

        t = self.TCN
        P = dict(enc_wT=f32(self.encoder.weight)[:, 0].t().contiguous(), ln=(f32(t.LN.weight), f32(t.LN.bias)),
                 bn_w=mat(t.BN), bn_b=f32(t.BN.bias), out_slope=f32(t.output[0].weight), out_w=mat(t.output[1]), out_b=f32(t.output[1].bias),
                 dec_w=f32(self.decoder.weight)[:, 0].contiguous(), blocks=[])
        for blk in t.TCN:
            P["blocks"].append(dict(
                w1=mat(blk.conv1d), b1=f32(blk.conv1d.bias), slope1=f32(blk.nonlinearity1.weight), reg1=(f32(blk.reg1.weight), f32(blk.reg1.bias)),
                w3=f32(blk.dconv1d.weight)[:, 0].t().contiguous(), b3=f32(blk.dconv1d.bias), slope2=f32(blk.nonlinearity2.weight),
                reg2=(f32(blk.reg2.weight), f32(blk.reg2.bias)), dilation=blk.dilation,
                w_rs=mat(blk.res_out, blk.skip_out), b_rs=torch.cat([f32(blk.res_out.bias), f32(blk.skip_out.bias)]).contiguous()))
        self._packed[key] = P
        return P

    # ---- forward (convtasnet.py:55-72, TCN.forward :314-339, DepthConv1d.forward :256-267) ------
    def forward(self, input, *args, **ignored_kwargs):
        if input.dim() not in [2, 3]:
            raise RuntimeError("Input can only be 2 or 3 dimensional.")
        if input.dim() == 3:
            if input.size(1) != 1:
                raise RuntimeError(f"ConvTasNet: expected one channel [B, 1, T], got {tuple(input.shape)}")
            input = input[:, 0]
        device, dtype = self.encoder.weight.device, self.compute_dtype
        wav = input.to(device=device, dtype=torch.float32).contiguous()
        P = self._pack(dtype, device)
        B = wav.shape[0]
        enc, part = ops.tasnet_encode(wav, P["enc_wT"], dtype)
        Lf, N = enc.shape[1], enc.shape[2]
        H = 4 * self.feature_dim
        st = ops.tasnet_gln_finalize(part, N * Lf)
        output = ops.tasnet_pointwise(enc, P["bn_w"], P["bn_b"], dtype, norm=(st, *P["ln"]), out_f32=True)
        skip = torch.zeros_like(output)
        for b in P["blocks"]:
            h, part = ops.tasnet_pointwise(output, b["w1"], b["b1"], dtype, prelu_out=b["slope1"], partials=True)
            st = ops.tasnet_gln_finalize(part, H * Lf)
            h, part = ops.tasnet_depthwise(h, b["w3"], b["b3"], (st, *b["reg1"]), b["slope2"], b["dilation"])
            st = ops.tasnet_gln_finalize(part, H * Lf)
            ops.tasnet_pointwise(h, b["w_rs"], b["b_rs"], dtype, norm=(st, *b["reg2"]), res_skip=(output, skip))
        mask = ops.tasnet_pointwise(skip, P["out_w"], P["out_b"], dtype, prelu_in=P["out_slope"])
        return ops.tasnet_decode(mask, enc, P["dec_w"])
