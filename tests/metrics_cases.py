"""Seeded inputs of fixture F24 (tests/golden/f24_metrics.npz), shared by its generator (tools/make_golden_metrics.py) and its test
(tests/test_metrics.py).  The fixture stores only what the reference computed on these inputs and their SHA-256; the inputs themselves
regenerate from the seeds below.

Energy cases (energy_ratios / snr_dB, util/other.py:21-44, 96-100): s_hat = 0.8 s + g_n n + g_a noise with s, n, noise ~ amp N(0, 1),
rounded to float32.  Lengths sit on the partition boundary of storm_energy_ratios_rows (STORM_METRICS_CHUNK = 16384 samples per
workgroup, +- 1) and at 1, 37 and 48001; the (g_n, g_a) mixes keep every ratio inside +- 60 dB (the generator asserts it).  One sample
(L = 1) is a special geometry: every vector is collinear, the residual of the projection is zero and SI-SDR is |s_target|^2 / eps, so
that case uses amp = 1e-3 to keep 10 log10(|s_hat|^2 / 1e-10) under 60 dB.

LSD cases (lsd, util/other.py:16-19): s_hat = 0.8 s + 0.3 n at amp 0.1; L = 256 is the shortest signal the STFT's reflect padding
accepts; `zero_tail` samples at the end are exact zeros in both signals (whole frames whose every bin sits at eps)."""
import hashlib

import numpy as np

CHUNK = 16384                                       # include/storm_hip.h: STORM_METRICS_CHUNK
MIXES = ((0.3, 0.1), (0.05, 1e-3), (1.0, 1e-3), (0.01, 0.3))


def _energy_cases():
    cases = []
    for i, (L, j) in enumerate(((1, 0), (37, 3), (CHUNK - 1, 1), (CHUNK, 2), (CHUNK + 1, 3), (48001, 1))):
        cases.append(dict(name=f"L{L}_mix{j}", L=L, seed=2400 + i, mix=MIXES[j], amp=1e-3 if L == 1 else 1.0))
    for j in (0, 2, 3):                             # the longest length with every mix (mix 1 is above)
        cases.append(dict(name=f"L48001_mix{j}", L=48001, seed=2410 + j, mix=MIXES[j], amp=1.0))
    return cases


ENERGY_CASES = _energy_cases()
LSD_CASES = [dict(name="L256", L=256, seed=2450, zero_tail=0), dict(name="L300", L=300, seed=2451, zero_tail=0),
             dict(name="L16385", L=16385, seed=2452, zero_tail=0), dict(name="L48001", L=48001, seed=2453, zero_tail=0),
             dict(name="L6000_tail2000", L=6000, seed=2454, zero_tail=2000)]
RAGGED = ("L300", "L16385", "L48001")               # the rows of the ragged-batch tests (LSD cases; their n serves the energy test)


def energy_inputs(case):
    """(s_hat, s, n) float32 [L]"""
    r = np.random.default_rng(case["seed"])
    s, n, noise = (case["amp"] * r.standard_normal(case["L"]) for _ in range(3))
    gn, ga = case["mix"]
    return (0.8 * s + gn * n + ga * noise).astype(np.float32), s.astype(np.float32), n.astype(np.float32)


def lsd_inputs(case):
    """(s_hat, s, n) float32 [L]"""
    r = np.random.default_rng(case["seed"])
    s, n = (0.1 * r.standard_normal(case["L"]) for _ in range(2))
    if case["zero_tail"]:
        s[-case["zero_tail"]:] = 0.0
        n[-case["zero_tail"]:] = 0.0
    return (0.8 * s + 0.3 * n).astype(np.float32), s.astype(np.float32), n.astype(np.float32)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
