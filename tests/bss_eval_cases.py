"""Seeded inputs and the float64 numpy restatements for tests/test_bss_eval.py (BSS-eval SDR / SIR / SAR with two sources,
storm_bss_eval_rows).

Two restatements of the definition of include/storm_hip.h, neither of which shares a line with the kernels:
  * the quadratic form: the 2 F x 2 F block-Toeplitz matrix and its right-hand side built from the 6 F + 1 correlations, handed to a dense
    solver of the caller's choice (np.linalg.solve, scipy.linalg.solve) - numbers();
  * the time-domain form, which is mir_eval's formulation: np.linalg.lstsq of the zero-padded estimate onto the zero-padded delayed copies of
    the target alone and of target and noise, then the energies of the projected signals - time_domain().
The correlations themselves are pinned bit for bit through tests/bss_cases.py (correlations: np.cumsum per lag and piece)."""
import functools

import numpy as np

from tests import bss_cases as BC

PAIRS = (("white", "white"), ("ar2", "white"), ("white", "ar2"))
# the ragged batch of the correlation test: tiny rows, both sides of 512 lags, both sides of the piece cut with lags that straddle it, three pieces
LENGTHS = (2, 63, 513, BC.PIECE, BC.PIECE + 1, BC.PIECE + 511, 33000)
FLENS = (1, 2, 64, 512)
ARTEFACTS_DB = 26.0


def split(parts, F):
    """G11, D1, G22, D2, X12, X21 (each [F]) and Ee of one row's parts [6 F + 1]"""
    return tuple(parts[i * F:(i + 1) * F] for i in range(6)) + (float(parts[6 * F]),)


def joint_system(parts, F):
    """(M [2F, 2F], d [2F]) of the header: unknowns interleaved, block(k, l) = R(k - l)"""
    G11, D1, G22, D2, X12, X21, _ = split(parts, F)
    m = np.arange(F)[:, None] - np.arange(F)[None, :]                          # k - l
    c12 = np.where(m >= 0, X12[np.abs(m)], X21[np.abs(m)])                     # c12(m)
    c21 = np.where(m <= 0, X12[np.abs(m)], X21[np.abs(m)])                     # c12(-m)
    M = np.empty((2 * F, 2 * F))
    M[0::2, 0::2], M[0::2, 1::2], M[1::2, 0::2], M[1::2, 1::2] = G11[np.abs(m)], c12, c21, G22[np.abs(m)]
    d = np.empty(2 * F)
    d[0::2], d[1::2] = D1, D2
    return M, d


def toeplitz(G):
    return G[np.abs(np.arange(len(G))[:, None] - np.arange(len(G))[None, :])]


def ratios(P1, P12, Ee):
    """the header's three numbers and their inf rules from the two projections' energies (a NaN row never gets here)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        sdr = np.inf if Ee - P1 <= 0 else (10 * np.log10(P1 / (Ee - P1)) if P1 > 0 else -np.inf)
        sir = (np.inf if P1 > 0 else np.nan) if P12 - P1 <= 0 else (10 * np.log10(P1 / (P12 - P1)) if P1 > 0 else -np.inf)
        sar = np.inf if Ee - P12 <= 0 else (10 * np.log10(P12 / (Ee - P12)) if P12 > 0 else -np.inf)
    return np.array([sdr, sir, sar])


def numbers(parts, F, solve=np.linalg.solve):
    """(sdr, sir, sar), x of the quadratic form with the dense solver `solve(matrix, rhs)`"""
    G11, D1, _, _, _, _, Ee = split(parts, F)
    M, d = joint_system(parts, F)
    x = solve(M, d)
    return ratios(float(D1 @ solve(toeplitz(G11), D1)), float(d @ x), Ee), x


def delayed_copies(s, F):
    """[L + F - 1, F]: column k is s delayed by k samples, zero-padded"""
    L = len(s)
    A = np.zeros((L + F - 1, F))
    for k in range(F):
        A[k:k + L, k] = s
    return A


def time_domain(s1, s2, e, F):
    """mir_eval's formulation: least-squares projections of the zero-padded estimate, then energies of the projected SIGNALS"""
    s1, s2, e = (np.asarray(v, dtype=np.float64) for v in (s1, s2, e))
    ep = np.concatenate([e, np.zeros(F - 1)])
    A1 = delayed_copies(s1, F)
    A12 = np.concatenate([A1, delayed_copies(s2, F)], axis=1)
    p1 = A1 @ np.linalg.lstsq(A1, ep, rcond=None)[0]
    p12 = A12 @ np.linalg.lstsq(A12, ep, rcond=None)[0]
    e_interf, e_artif = p12 - p1, ep - p12
    return np.array([10 * np.log10(np.sum(p1 ** 2) / np.sum((e_interf + e_artif) ** 2)), 10 * np.log10(np.sum(p1 ** 2) / np.sum(e_interf ** 2)),
                     10 * np.log10(np.sum((p1 + e_interf) ** 2) / np.sum(e_artif ** 2))])


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def taps(F, seed):
    """two filters of min(F, 40) taps: the target's (first tap 1) and a weaker one for the noise"""
    n = min(F, 40)
    return BC.fir(seed)[:n].copy(), 0.3 * BC.fir(seed + 1)[:n]


@functools.lru_cache(maxsize=None)
def triple(colours, L, F, seed=0):
    """(target, noise, estimate) fp32 [L]: two independent seeded rows of the two colours, estimate = h1 * target + h2 * noise + white
    artefacts ARTEFACTS_DB below that sum"""
    c1, c2 = colours
    rng = np.random.default_rng(7 + 1000 * BC.COLOURS.index(c1) + 100 * BC.COLOURS.index(c2) + 10 * L + F + seed)
    s1 = BC.coloured(c1, rng.standard_normal(L + 200))[200:].astype(np.float32)
    s2 = BC.coloured(c2, rng.standard_normal(L + 200))[200:].astype(np.float32)
    h1, h2 = taps(F, seed)
    mix = np.convolve(s1.astype(np.float64), h1)[:L] + np.convolve(s2.astype(np.float64), h2)[:L]
    return s1, s2, BC.with_noise(mix, ARTEFACTS_DB, rng).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ragged_triple(L, seed=0):
    """a row of the ragged batch: the round-18 pair of a colour, and a noise row that is correlated with the target ASYMMETRICALLY (half the
    target three samples late, plus white noise), so that X12 != X21"""
    s1, e = BC.pair(BC.COLOURS[L % 3], L, seed)
    rng = np.random.default_rng(555 + L)
    s2 = (0.5 * BC.delayed(s1, min(3, L - 1)) + rng.standard_normal(L)).astype(np.float32)
    return s1, s2, e


@functools.lru_cache(maxsize=None)
def restated_parts(L, F, seed=0):
    """[6 F + 1] of ragged_triple(L) by the np.cumsum restatement of tests/bss_cases.py, one pair at a time"""
    s1, s2, e = ragged_triple(L, seed)
    a, b, c, d = (BC.correlations(u, v, F) for u, v in ((s1, e), (s2, e), (s1, s2), (s2, s1)))
    return np.concatenate([a[:F], a[F:2 * F], b[:F], b[F:2 * F], c[F:2 * F], d[F:2 * F], a[2 * F:]])


def exact_triple(L, F, seed=0):
    """(target, noise, estimate, h1, h2) with an estimate that is EXACTLY h1 * target + h2 * noise as fp32: samples are multiples of 1/8 in
    [-1, 1] and taps multiples of 1/16 in [-1, 1], so every product has at most 9 significant bits and a sum of 2 x min(F, 16) of them fits
    fp32's 24 without rounding; the last 64 samples of both sources are zero, so no tail of the convolution is cut off (round 18's anchor)."""
    rng = np.random.default_rng(9000 + 10 * L + F + seed)
    s1, s2 = (rng.integers(-8, 9, L).astype(np.float64) / 8 for _ in range(2))
    s1[-64:], s2[-64:] = 0.0, 0.0
    n = min(F, 16)
    h1, h2 = (rng.integers(-16, 17, n).astype(np.float64) / 16 for _ in range(2))
    h1[0] = 1.0
    e = np.convolve(s1, h1)[:L] + np.convolve(s2, h2)[:L]
    e32 = e.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), e)
    return s1.astype(np.float32), s2.astype(np.float32), e32, h1, h2
