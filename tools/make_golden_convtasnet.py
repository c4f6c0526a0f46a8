"""Generate tests/golden/f22_convtasnet.npz: the REFERENCE's ConvTasNet for every case of tests/convtasnet_cases.py - state_dict layout
and fill hash, forward outputs, DiscriminativeModel.enhance, and the reference's OWN 16-bit error (its torch modules in bf16 / fp16 on the
CPU against its fp32 output), which bounds the engine's 16-bit tolerance.

Runs only where the reference checkout exists (oracle.ref_import); tests read the .npz alone.

    python tools/make_golden_convtasnet.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import convtasnet_cases as CC  # noqa: E402
from tests import option_nets as ON  # noqa: E402
from tests.util import rel_l2  # noqa: E402


def main():
    ref = import_reference()
    from sgmse.backbones.convtasnet import ConvTasNet as RefNet
    out = {}
    nets = {}
    for name, kw in CC.CASES.items():
        torch.manual_seed(0)
        net = RefNet(**kw)
        names, vals = CC.fill(net)
        net.eval()
        nets[name] = net
        out[f"{name}_names"] = np.array(names)
        out[f"{name}_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in vals.values()], dtype=np.int32)
        out[f"{name}_sdhash"] = ON.sd_hash(vals)
        print(f"{name}: {len(names)} tensors")
    for name, samples in CC.INPUTS:
        net, key = nets[name], f"{name}_{samples}"
        x = CC.case_input(samples)
        with torch.no_grad():
            y = net(x)
            y64 = net.double()(x.double())
            net.float()
        assert torch.isfinite(y).all(), key
        out[f"x_{samples}"] = x.numpy()
        out[f"{key}_y"] = y.numpy()
        line = f"{key}: out {tuple(y.shape)}, fp32 vs fp64 {rel_l2(y, y64):.2e}"
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            with torch.no_grad():
                y16 = net.to(dt)(x.to(dt)).float()
            net.float()
            CC.fill(net)                                   # (the round trip through 16 bits rounded the parameters)
            err = rel_l2(y16, y)
            out[f"{key}_referr_{tag}"] = np.float64(err)
            line += f", reference in {tag} {err:.2e}"
        print(line)
    M, DM = ref["model"], ref["data_module"].SpecsDataModule
    m = M.DiscriminativeModel(backbone="convtasnet", data_module_cls=DM, **CC.MODEL_KW, **CC.CASES[CC.ENHANCE_CASE])
    CC.fill(m.dnn)
    m.eval(no_ema=True)
    wav = CC.enhance_input()
    with torch.no_grad():
        xh = m.enhance(wav.clone())
    assert xh.shape == (CC.ENHANCE_SAMPLES,) and torch.isfinite(xh).all()
    out["enhance_wav"] = wav.numpy()
    out["enhance_out"] = xh.numpy()
    path = os.path.join(ROOT, "tests", "golden", "f22_convtasnet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
