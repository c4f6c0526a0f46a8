"""Seeded inputs and the float64 numpy restatement for tests/test_bss_sdr.py (BSS-eval SDR with a short filter, storm_bss_sdr_rows).

The restatement is the definition of include/storm_hip.h word for word: per lag and piece np.cumsum (sequential, fp64) of the exact products in
ascending n from +0, the pieces added in ascending order from +0, the Levinson-Durbin recursion as the header prints it, the edge rules.  Only
the correlations are pinned bit for bit; the recursion's dot products are summed here by np.dot, on the device in the shape the header gives."""
import functools

import numpy as np
import scipy.signal as ss

PIECE = 16384                    # STORM_BSS_PIECE  (the test asserts that the library says the same)
MAX_TAPS = 512                   # STORM_BSS_MAX_TAPS
COLOURS = ("white", "ar2", "lowpass")
# the issue's lengths: tiny rows, both sides of 512 lags, both sides of the piece cut with lags that straddle it, three pieces
LENGTHS = (2, 63, 511, 513, 4097, PIECE, PIECE + 1, PIECE + 511, 33000)
FLENS = (1, 2, 64, 512)


def _chain(prod):
    """one fp64 chain in ascending order from +0"""
    return np.cumsum(np.concatenate(([0.0], prod)))[-1]


def correlations(s, e, F):
    """fp64 [2 F + 1] = G, D, Ee of two fp32 arrays of equal length"""
    s64, e64 = s.astype(np.float64), e.astype(np.float64)
    L = len(s)
    total = np.zeros(2 * F + 1)
    for p0 in range(0, L, PIECE):
        pend = min(p0 + PIECE, L)                                  # the piece of the FIRST factor's index
        part = np.zeros(2 * F + 1)
        for k in range(F):
            hi = min(pend, L - k)
            if hi > p0:
                part[k] = _chain(s64[p0:hi] * s64[p0 + k:hi + k])
                part[F + k] = _chain(s64[p0:hi] * e64[p0 + k:hi + k])
        part[2 * F] = _chain(e64[p0:pend] * e64[p0:pend])
        total = total + part                                       # ascending pieces, from +0
    return total


def levinson(G, D):
    """C with Toeplitz(G) C = D (Golub & Van Loan alg. 4.7.3), or None when E is <= 0 or not finite at some order"""
    F = len(G)
    a, C = np.zeros(F), np.zeros(F)
    E = G[0]
    if not (E > 0 and np.isfinite(E)):
        return None
    a[0], C[0] = 1.0, D[0] / E
    for m in range(1, F):
        lam = -np.dot(a[:m], G[m:0:-1]) / E
        a[:m + 1] = a[:m + 1] + lam * a[m::-1]
        E = E * (1.0 - lam * lam)
        if not (E > 0 and np.isfinite(E)):
            return None
        mu = (D[m] - np.dot(C[:m], G[m:0:-1])) / E
        C[:m + 1] = C[:m + 1] + mu * a[m::-1]
    return C


def sdr_of(parts, C):
    """the header's result and edge rules from G, D, Ee and a solved filter"""
    F = (len(parts) - 1) // 2
    P, Ee = float(np.dot(parts[F:2 * F], C)), float(parts[2 * F])
    if Ee - P <= 0:
        return np.inf
    return 10 * np.log10(P / (Ee - P)) if P > 0 else -np.inf


@functools.lru_cache(maxsize=None)
def restated(colour, L, F, seed=0):
    """(parts, filter or None, sdr) of the seeded pair (colour, L, seed) by the restatement"""
    s, e = pair(colour, L, seed)
    parts = correlations(s, e, F)
    if L < 1 or parts[0] == 0 or parts[2 * F] == 0:
        return parts, None, np.nan
    C = levinson(parts[:F], parts[F:2 * F])
    return parts, C, (np.nan if C is None else sdr_of(parts, C))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
# condition number of Toeplitz(G) at 512 taps: white below 10, AR(2) 2e3 .. 4e3, low-pass 2e5 .. 2e7
def coloured(colour, x):
    if colour == "white":
        return x
    if colour == "ar2":
        return ss.lfilter([1.0], [1.0, -1.6, 0.8], x)
    b, a = ss.butter(4, 0.25)
    return ss.lfilter(b, a, x)


@functools.lru_cache(maxsize=None)
def fir(seed=0):
    """40 taps, decaying, the first the largest"""
    rng = np.random.default_rng(7000 + seed)
    h = 0.5 * rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
    h[0] = 1.0
    return h


def with_noise(x, db, rng):
    """x plus white noise `db` dB below it"""
    n = rng.standard_normal(len(x))
    return x + n * np.sqrt(np.mean(x ** 2) / max(np.mean(n ** 2), 1e-300)) * 10 ** (-db / 20)


@functools.lru_cache(maxsize=None)
def pair(colour, L, seed=0):
    """(reference, estimate) fp32 [L]: a seeded row of the colour, and that row through the 40-tap FIR plus noise at -20 dB"""
    rng = np.random.default_rng(100000 * COLOURS.index(colour) + 10 * L + seed)
    s = coloured(colour, rng.standard_normal(L + 200))[200:].astype(np.float32)       # (past the colouring filter's transient)
    e = with_noise(np.convolve(s.astype(np.float64), fir(seed))[:L], 20.0, rng).astype(np.float32)
    return s, e


def delayed(x, d):
    out = np.zeros_like(x)
    out[d:] = x[:len(x) - d]
    return out
