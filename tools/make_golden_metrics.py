"""Fixture F24 (tests/golden/f24_metrics.npz): what the REFERENCE's util/other.py computes on the seeded inputs of tests/metrics_cases.py.

    python tools/make_golden_metrics.py

Needs the reference checkout (oracle.ref_import: STORM_REFERENCE_ROOT); nothing of it is copied - the file holds, per case,
  energy_ref64 / energy_ref32 [cases, 4]  energy_ratios(s_hat, s, n) and snr_dB(s, n) on float64 copies of the float32 inputs / on the float32 inputs,
  lsd_ref64 / lsd_ref32 [cases]           lsd(s_hat, s) likewise (the float64 run with the reference's own window values, as float64),
  *_sha                                   SHA-256 of the float32 inputs (the test regenerates them from the seeds and compares).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import metrics_cases as MC  # noqa: E402


def main():
    other = import_reference()["other"]
    out = {}
    e64, e32, esha = [], [], []
    for case in MC.ENERGY_CASES:
        sh, s, n = MC.energy_inputs(case)
        rows = []
        for cast in (np.float64, np.float32):
            a, b, c = sh.astype(cast), s.astype(cast), n.astype(cast)
            rows.append([float(v) for v in other.energy_ratios(a, b, c)] + [float(other.snr_dB(b, c))])
        assert all(abs(v) < 60.0 for v in rows[0]), (case["name"], rows[0])          # the bound of the test is derived for ratios inside +- 60 dB
        e64.append(rows[0]); e32.append(rows[1]); esha.append(MC.sha256(sh, s, n))
        print(f"{case['name']:>16}: " + " ".join(f"{v:10.5f}" for v in rows[0]) + "   max |f32 - f64| " + f"{max(abs(p - q) for p, q in zip(*rows)):.2e} dB")
    out.update(energy_names=np.array([c["name"] for c in MC.ENERGY_CASES]), energy_ref64=np.array(e64, dtype=np.float64),
               energy_ref32=np.array(e32, dtype=np.float64), energy_sha=np.array(esha))
    l64, l32, lsha = [], [], []
    window32 = other.stft_kwargs["window"]
    for case in MC.LSD_CASES:
        sh, s, _ = MC.lsd_inputs(case)
        other.stft_kwargs["window"] = window32
        v32 = float(other.lsd(sh, s))
        other.stft_kwargs["window"] = window32.double()                             # the same window values: only the arithmetic changes
        v64 = float(other.lsd(sh.astype(np.float64), s.astype(np.float64)))
        other.stft_kwargs["window"] = window32
        l64.append(v64); l32.append(v32); lsha.append(MC.sha256(sh, s))
        print(f"{case['name']:>16}: lsd {v64:.12f}   |f32 - f64| {abs(v32 - v64):.2e}")
    out.update(lsd_names=np.array([c["name"] for c in MC.LSD_CASES]), lsd_ref64=np.array(l64, dtype=np.float64), lsd_ref32=np.array(l32, dtype=np.float64),
               lsd_sha=np.array(lsha))
    path = os.path.join(ROOT, "tests", "golden", "f24_metrics.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
