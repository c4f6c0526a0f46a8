"""Seeded inputs and numpy restatements for tests/test_align.py and tools/make_golden_align.py (delay search, shift, biquad cascade).

The restatement of the delay search is the definition of include/storm_hip.h word for word: per lag, np.cumsum (sequential, fp64) of the
exact products in ascending n, its last entry, then np.argmax (first index of the maximum)."""
import functools
import hashlib

import numpy as np

TILE = 512                       # STORM_XCORR_TILE (the test asserts that the library says the same)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def lag_range(ny, nr, max_lag=None):
    dmin, dmax = -(ny - 1), nr - 1
    if max_lag is not None:
        dmin, dmax = max(dmin, -max_lag), min(dmax, max_lag)
    return dmin, dmax


def xcorr(y, ref, max_lag=None):
    """(dmin, c fp64 [dmax - dmin + 1]) of two fp32 arrays: c[d] = cumsum(y64[lo:hi] * r64[lo + d:hi + d])[-1]"""
    y64, r64 = y.astype(np.float64), ref.astype(np.float64)
    ny, nr = len(y), len(ref)
    dmin, dmax = lag_range(ny, nr, max_lag)
    c = np.empty(dmax - dmin + 1)
    for d in range(dmin, dmax + 1):
        lo, hi = max(0, -d), min(ny, nr - d)
        c[d - dmin] = np.cumsum(y64[lo:hi] * r64[lo + d:hi + d])[-1]
    return dmin, c


def lag_peak(y, ref, max_lag=None):
    dmin, c = xcorr(y, ref, max_lag)
    i = int(np.argmax(c))
    return dmin + i, c[i]


def delayed(x, d):
    """x delayed by d samples (d < 0: advanced), zero-filled, same length"""
    out = np.zeros_like(x)
    L = len(x)
    if d >= 0:
        out[d:] = x[:L - d]
    else:
        out[:L + d] = x[-d:]
    return out


@functools.lru_cache(maxsize=None)
def planted(L, d, seed=0):
    """(y, ref) fp32 [L]: seeded white noise and the same noise delayed by d (|d| < L), zero-filled.  An overlap shorter than 64 samples
    would leave no clear peak in noise: then y is a single sample at one end and ref a single sample d further."""
    rng = np.random.default_rng(1000 * L + seed)
    y = rng.standard_normal(L).astype(np.float32)
    if L - abs(d) < 64 and d != 0:
        y = np.zeros(L, np.float32)
        y[0 if d > 0 else L - 1] = np.float32(1.5)
        ref = np.zeros(L, np.float32)
        ref[(0 if d > 0 else L - 1) + d] = np.float32(2.25)
        return y, ref
    return y, delayed(y, d)


# (L, true delay): the issue's lengths and delays, the two extremes of every length, both sides of every tile boundary of L = 4097
LENGTHS = (1, 2, 63, 64, 65, 1000, 4097)


def delay_cases():
    cases = []
    for L in LENGTHS:
        ds = {0}
        for d in (1, 37, 500, L - 1):
            if 0 < d < L:
                ds |= {d, -d}
        if L == 4097:
            dmin = -(L - 1)
            for b in range(dmin + TILE, L, TILE):                  # the first lag of every tile but the first
                ds |= {b - 1, b}
        cases += [(L, d) for d in sorted(ds)]
    return cases


# ---- against the reference's align: inputs with a clear peak -----------------------------------------------------------------------------
ALIGN_L = 4097
ALIGN_SHIFTS = (0, 1, -1, 37, -500)


@functools.lru_cache(maxsize=None)
def align_inputs(shift):
    """(y, ref) fp32 [4097]: ref is seeded white noise, y is ref moved by -shift (zero-filled) plus 5 % noise, so align(y, ref) moves y by
    +shift"""
    rng = np.random.default_rng(26000 + shift)
    ref = rng.standard_normal(ALIGN_L).astype(np.float32)
    y = (delayed(ref, -shift) + np.float32(0.05) * rng.standard_normal(ALIGN_L).astype(np.float32)).astype(np.float32)
    return y, ref


# ---- high-pass ---------------------------------------------------------------------------------------------------------------------------
HP_L = 3000


@functools.lru_cache(maxsize=None)
def hp_input():
    """fp32 [3000]: white noise on a 30 Hz rumble and an offset - what the filter is for"""
    rng = np.random.default_rng(2680)
    t = np.arange(HP_L) / 16000.0
    return (0.1 * rng.standard_normal(HP_L) + 0.5 * np.sin(2 * np.pi * 30.0 * t) + 0.25).astype(np.float32)


def sosfilt(sos, x):
    """scipy.signal.sosfilt's recurrence in Python floats (fp64, every operation rounded separately), zero initial state"""
    out = np.empty(len(x))
    z = [[0.0, 0.0] for _ in sos]
    for n, v in enumerate(x):
        xc = float(v)
        for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
            xn = b0 * xc + z[s][0]
            z[s][0] = b1 * xc - a1 * xn + z[s][1]
            z[s][1] = b2 * xc - a2 * xn
            xc = xn
        out[n] = xc
    return out
