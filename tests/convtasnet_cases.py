"""ConvTasNet cases (fixture F22, tests/golden/f22_convtasnet.npz), shared by the generator (tools/make_golden_convtasnet.py, which runs
the REFERENCE's class where the reference exists) and tests/test_convtasnet.py (which reads only the .npz): the constructor arguments,
the seeded fill and the seeded inputs."""
import numpy as np
import torch

from tests import option_nets as ON

CASES = {
    "small": dict(enc_dim=64, feature_dim=32, layer=3, stack=2),
    "win16": dict(fs=8000, enc_dim=48, feature_dim=24, layer=2, stack=1),
    "default": dict(),
}
# (case, samples per row): 2 rows each.  default at 1000 samples has 64 frames under dilations up to 128: only the centre tap is left
INPUTS = [("small", 4000), ("win16", 1037), ("default", 4000), ("default", 1000)]
ENHANCE_CASE, ENHANCE_SAMPLES = "small", 5003
MODEL_KW = dict(sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)   # tests/test_model.py:COMMON without nf
SEED = 22


def is_slope(name):
    return "nonlinearity" in name or name == "TCN.output.0.weight"


def fill(net, seed=SEED):
    """option_nets.fill_values for every tensor, then every PReLU slope from a second seeded stream in [0.1, 0.4] (fill_values puts 1-D
    '.weight' tensors near 1, which would make every PReLU an identity); loaded strictly.  Returns (names, values)."""
    sd0 = net.state_dict()
    names = list(sd0)
    vals = ON.fill_values(names, [tuple(v.shape) for v in sd0.values()], seed)
    rng = np.random.default_rng(seed + 1000)
    for n in names:
        if is_slope(n):
            vals[n] = torch.from_numpy((0.1 + 0.3 * rng.random(tuple(vals[n].shape))).astype(np.float32))
    net.load_state_dict(vals, strict=True)
    return names, vals


def case_input(samples):
    return 0.1 * torch.randn(2, samples, generator=torch.Generator().manual_seed(2200 + samples))


def enhance_input():
    return 0.1 * torch.randn(1, ENHANCE_SAMPLES, generator=torch.Generator().manual_seed(2299))
