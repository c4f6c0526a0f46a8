"""Validation-loss cases (fixture F23, tests/golden/f23_valid_loss.npz), shared by the generator (tools/make_golden_valid_loss.py, which
runs the REFERENCE's `_step` where the reference exists) and tests/test_valid_loss.py (which reads only the .npz): the constructor
arguments, the seeded weights, the seeded spectrogram batches and the two seeded draws (t, z) of a step."""
import hashlib

import numpy as np
import torch

from oracle import ncsnpp_ref as NR
from tests import convtasnet_cases as CC

B, F, T = 3, 256, 64                                         # one 64-frame bucket of n_fft = 510 spectrograms
OUVE = dict(CC.MODEL_KW, nf=8)
OUVP = dict(sde="ouvp", beta_min=0.1, beta_max=2.0, stiffness=1, spec_factor=0.15, spec_abs_exponent=0.5, nf=8)
# name -> (model class, constructor keywords, seed of the case: weights seed .. seed + 1, inputs seed + 10, draws seed + 20)
CASES = {
    "score_ouve_mse": ("score", dict(OUVE, backbone="ncsnpp", loss_type="mse"), 2300),
    "score_ouve_mae": ("score", dict(OUVE, backbone="ncsnpp", loss_type="mae"), 2310),
    "score_ouvp_mse": ("score", dict(OUVP, backbone="ncsnpp", loss_type="mse"), 2320),
    "disc_ncsnpp_mse": ("disc", dict(OUVE, backbone="ncsnpp", input_channels=2, discriminative=True, loss_type="mse"), 2330),
    "disc_ncsnpp_mae": ("disc", dict(OUVE, backbone="ncsnpp", input_channels=2, discriminative=True, loss_type="mae"), 2340),
    "disc_convtasnet_sisdr": ("disc", dict(CC.MODEL_KW, backbone="convtasnet", loss_type="sisdr", **CC.CASES["small"]), 2350),
    "storm_both_mse_mse": ("storm", dict(OUVE, backbone_denoiser="ncsnpp", backbone_score="ncsnpp", condition="both",
                                         loss_type_score="mse", loss_type_denoiser="mse"), 2360),
    "storm_noisy_none": ("storm", dict(OUVE, backbone_denoiser="ncsnpp", backbone_score="ncsnpp", condition="noisy",
                                       loss_type_score="mse", loss_type_denoiser="none"), 2370),
}
DRAWS = [n for n, (kind, _, _) in CASES.items() if kind != "disc"]         # the cases whose step draws t and z


def build(name, classes, **extra):
    """The case's model from `classes` = {"score": ScoreModel, "disc": DiscriminativeModel, "storm": StochasticRegenerationModel} (the
    reference's or the engine's) with its seeded weights loaded; returns (model in eval(no_ema=True), the weight tensors in load order)."""
    kind, kw, seed = CASES[name]
    m = classes[kind](**dict(kw), **extra)
    if kind == "storm":
        sd_d = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=seed)
        sd_s = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=6 if kw["condition"] == "both" else 4), seed=seed + 1)
        m.denoiser_net.load_state_dict(sd_d)
        m.score_net.load_state_dict(sd_s)
        vals = list(sd_d.values()) + list(sd_s.values())
    elif kw["backbone"] == "convtasnet":
        _, sd = CC.fill(m.dnn, seed=seed)
        vals = list(sd.values())
    else:
        sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2 if kind == "disc" else 4, discriminative=kind == "disc"), seed=seed)
        m.dnn.load_state_dict(sd)
        vals = list(sd.values())
    m._error_loading_ema = True                                # (no EMA state: eval() swaps nothing)
    m.eval(no_ema=True)
    return m, vals


def inputs(name):
    """(x clean, y noisy): complex64 [B, 1, F, T]"""
    g = torch.Generator().manual_seed(CASES[name][2] + 10)
    x = 0.3 * torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g)
    return x, x + 0.2 * torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g)


def draw_seed(name):
    return CASES[name][2] + 20


def draws(name):
    """(u, z): what `torch.rand(B)` and `torch.randn_like(x)` give after torch.manual_seed(draw_seed(name)) (model.py:144, 146) - the
    CPU generator's stream is a function of the seed alone"""
    g = torch.Generator().manual_seed(draw_seed(name))
    u = torch.rand(B, generator=g)
    return u, torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g)


def sha(tensors):
    h = hashlib.sha256()
    for v in tensors:
        v = v.detach().contiguous()
        h.update((torch.view_as_real(v) if v.is_complex() else v).numpy().tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()
