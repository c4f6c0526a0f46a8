"""Generate tests/golden/f25_ode_methods.npz: the REFERENCE's get_ode_sampler (sampling/__init__.py:71-141, scipy.integrate.solve_ivp on
the host) with method = RK23 and DOP853 on fixture F7's problem, one utterance per call - end state and nfev of every case of
tests/ode_method_cases.py.

Every (method, tolerance) is run twice, with the score in complex64 and in complex128; it is kept only if each utterance needs the same
number of evaluations both times (tests/ode_method_cases.py says why).  Both counts of every run tried are stored.

Runs only where the reference checkout exists (oracle.ref_import); tests read the .npz alone.

    python tools/make_golden_ode_methods.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import ode_method_cases as OC  # noqa: E402


def run(ref, sde, y, z, method, tol, double):
    """the reference's sampler on ONE utterance; its prior draw (torch.randn_like, sdes.py:prior_sampling) replaced by the recorded z"""
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: z.to(x.dtype)
    try:
        sampler = ref["sampling"].get_ode_sampler(sde, OC.make_score(sde, double), y=y, eps=OC.EPS, device="cpu", method=method, rtol=tol, atol=tol)
        x, nfe = sampler()
    finally:
        torch.randn_like = orig
    return x, int(nfe)


def main():
    ref = import_reference()
    sde = ref["sdes"].OUVESDE(**OC.SDE)
    y, z = OC.inputs()
    out = dict(seed=np.array(OC.SEED), input_hash=OC.input_hash(y, z))
    kept, tried = [], []
    for method in OC.METHODS:
        n_kept = 0
        for tol in OC.TOLERANCES:
            if n_kept == OC.CASES_PER_METHOD:
                break
            rows = [(run(ref, sde, y[b:b + 1], z[b:b + 1], method, tol, False), run(ref, sde, y[b:b + 1], z[b:b + 1], method, tol, True))
                    for b in range(y.shape[0])]
            n32, n64 = [r[0][1] for r in rows], [r[1][1] for r in rows]
            keep = n32 == n64
            tried.append((method, tol, n32, n64, keep))
            print(f"{method} rtol = atol = {tol:g}: nfev {n32} (score in complex64) {n64} (complex128): {'kept' if keep else 'dropped'}")
            out[f"tried_{method}_{tol:g}_nfev32"], out[f"tried_{method}_{tol:g}_nfev64"] = np.array(n32), np.array(n64)
            if not keep:
                continue
            n_kept += 1
            kept.append((method, tol))
            for b, ((x, nfe), _) in enumerate(rows):
                assert x.dtype == torch.complex64 and torch.isfinite(torch.view_as_real(x)).all()
                out[OC.key(method, tol, b) + "_out"] = x.numpy()
                out[OC.key(method, tol, b) + "_nfev"] = np.array(nfe)
        if n_kept < OC.CASES_PER_METHOD:
            print(f"{method}: only {n_kept} of {OC.CASES_PER_METHOD} cases pass the robustness condition")
    assert kept == OC.CASES, ("tests/ode_method_cases.py CASES disagrees with the selection", kept)
    path = os.path.join(ROOT, "tests", "golden", "f25_ode_methods.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
