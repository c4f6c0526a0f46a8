"""Generate tests/golden/f21_option_nets.npz: the REFERENCE's NCSNpp(**kw) for every case of tests/option_nets.py.

Runs only where the reference checkout exists (oracle.ref_import); tests read the .npz alone.

    python tools/make_golden_options.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import option_nets as ON  # noqa: E402


def main():
    import_reference()
    from sgmse.backbones.ncsnpp import NCSNpp as RefNCSNpp
    out = {"t": np.array(ON.T_COND, dtype=np.float32)}
    t = torch.tensor(ON.T_COND)
    for name, kw in ON.CASES.items():
        torch.manual_seed(0)
        net = RefNCSNpp(**kw)
        names, vals = ON.fill_module(net)
        net.eval()
        xkey, x = ON.case_input(kw)
        with torch.no_grad():
            y = net(x, t)
        assert torch.isfinite(torch.view_as_real(y)).all(), name
        out[xkey] = x.numpy()
        out[f"{name}_y"] = y.numpy()
        out[f"{name}_names"] = np.array(names)
        out[f"{name}_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in vals.values()], dtype=np.int32)
        out[f"{name}_sdhash"] = ON.sd_hash(vals)
        print(f"{name}: {len(names)} tensors, |y| = {float(y.abs().pow(2).mean().sqrt()):.3e}")
    path = os.path.join(ROOT, "tests", "golden", "f21_option_nets.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
