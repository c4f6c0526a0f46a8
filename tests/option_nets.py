"""Option nets (fixture F21, tests/golden/f21_option_nets.npz): NCSN++ built with constructor options beyond the StoRM default set.

Shared by the generator (tools/make_golden_options.py, which runs the REFERENCE's class where the reference exists) and by
tests/test_option_nets.py (which reads only the .npz): the cases, and the rule that fills a state_dict - every tensor, in order, all
non-zero, including the ones init_scale=0 would zero - from one seeded NumPy stream.
"""
import hashlib

import numpy as np
import torch

TINY4 = dict(nf=8, input_channels=4)                              # oracle/make_golden.py:TINY["tiny4"]
WIDE = dict(nf=64, ch_mult=(1, 3), num_res_blocks=1, attn_resolutions=(0,), image_size=16, input_channels=4)   # tests/test_net.py:GROUP_NET
SHAPE = (32, 64)
T_COND = (0.9, 0.05)
SEED = 21

NOFIR = dict(fir=False, progressive="none")
CASES = {
    # each option of the table alone (fir=False always with progressive='none')
    "skip_rescale": dict(TINY4, skip_rescale=False),
    "prog_none": dict(TINY4, progressive="none"),
    "prog_in_none": dict(TINY4, progressive_input="none"),
    "cat": dict(TINY4, progressive_combine="cat"),
    "centered": dict(TINY4, centered=True),
    "nofir": dict(TINY4, **NOFIR),
    "dropout": dict(TINY4, dropout=0.1),
    "uncond": dict(TINY4, conditional=False),
    "no_sigma": dict(TINY4, scale_by_sigma=False),
    # combinations
    "nofir_cat_all": dict(TINY4, **NOFIR, progressive_combine="cat", skip_rescale=False, centered=True),
    "nofir_no_pyramids": dict(TINY4, **NOFIR, progressive_input="none"),
    "disc_nofir": dict(nf=8, input_channels=2, discriminative=True, **NOFIR),        # keeps the avg_pool2d input pyramid
    # doubled widths in the MFMA convolution kernels
    "wide_cat": dict(WIDE, progressive_combine="cat"),
}


def fill_values(names, shapes, seed=SEED):
    """name -> float32 tensor for the given state_dict layout, drawn in order from one stream: GroupNorm scales around 1, biases and
    other vectors 0.1 n (the Fourier frequencies 16 n, their own initialisation), matrices and convolutions n / sqrt(fan_in)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in zip(names, shapes):
        shape = tuple(int(s) for s in shape)
        v = rng.standard_normal(shape).astype(np.float32)
        if len(shape) == 1:
            if name.endswith(".W"):
                v = v * 16.0
            elif name.endswith(".weight"):
                v = 1.0 + 0.1 * v
            else:
                v = 0.1 * v
        else:
            v = v / np.float32(np.sqrt(np.prod(shape[1:])))
        v = np.where(v == 0, np.float32(1e-3), v).astype(np.float32)
        out[name] = torch.from_numpy(v)
    return out


def fill_module(net, seed=SEED):
    """load the seeded values into net (strict); returns (names, state_dict values)"""
    sd0 = net.state_dict()
    names = list(sd0)
    vals = fill_values(names, [tuple(v.shape) for v in sd0.values()], seed)
    net.load_state_dict(vals, strict=True)
    return names, vals


def sd_hash(vals):
    h = hashlib.sha256()
    for v in vals.values():
        h.update(v.detach().contiguous().numpy().astype(np.float32).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def case_input(kw):
    """(fixture key, x): complex64 [2, in/2, 32, 64]; one seeded input per channel count, shared by the cases (the fixture stays small)"""
    n_c = 1 if kw.get("discriminative") else kw["input_channels"] // 2
    g = torch.Generator().manual_seed(1000 + n_c)
    return f"x{2 * n_c}", torch.randn(2, n_c, *SHAPE, dtype=torch.complex64, generator=g) * 0.5
