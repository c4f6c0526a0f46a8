"""Posterior ensembles: the float64 numpy restatement of the definition in include/storm_hip.h (storm_ensemble_combine_rows) and the case
tables of tests/test_ensemble.py.  The restatement follows the header's expressions and orders literally: numpy's float64 +, -, *, /, sqrt
are the IEEE operations the kernel uses, one rounding each, so for the transforms without pow every number is expected bit for bit; pow is
numpy's (a few units in the last place from any other correct implementation)."""
import functools

import numpy as np

TILE, THREADS, MAX_DRAWS = 1024, 256, 32                    # STORM_ENSEMBLE_TILE, the workgroup of the combine kernel, STORM_ENSEMBLE_MAX_DRAWS
PAIRS = TILE // 2 // THREADS
MODES = ("mean", "mag_mean", "mag_median")
TRANSFORMS = ((0.15, 0.5), (0.33, 0.667), (1.0, 1.0))       # (spec_factor, spec_abs_exponent): the StoRM default, a pow, the identity
DRAW_KEY_STEP = 0xD1B54A32D192ED03


def draw_key(key, k):
    return int(key) if k == 0 else (int(key) + int(k) * DRAW_KEY_STEP) % 2 ** 63


def back_transform(z, factor, e):
    """step 1 on a complex64 array: (x_re, x_im, |x|) float64; factor, e are the fp32 values widened"""
    factor, e = np.float64(np.float32(factor)), np.float64(np.float32(e))
    re, im = z.real.astype(np.float64), z.imag.astype(np.float64)
    r = np.sqrt(re * re + im * im)
    nz = r != 0.0
    rs = np.where(nz, r, 1.0)
    m = rs / factor
    with np.errstate(all="ignore"):
        g = m if e == 1.0 else (m * m if e == 0.5 else np.power(m, np.float64(1.0) / e))
    g = np.where(nz, g, 0.0)
    return np.where(nz, g * (re / rs), 0.0), np.where(nz, g * (im / rs), 0.0), g


def _ordered_sum(v, ok):
    """step 6 on v [n] (bin order) with the bins' validity ok [n]: tiles of TILE bins, thread l adds the valid bins of its pairs l, l + 256, ...
    ascending from +0, butterfly per wave, waves in order, tiles in order"""
    n = v.shape[0]
    tiles = -(-n // TILE)
    pad = tiles * TILE - n
    v = np.concatenate([v, np.zeros(pad)]).reshape(tiles, PAIRS, THREADS, 2)
    ok = np.concatenate([ok, np.zeros(pad, dtype=bool)]).reshape(tiles, PAIRS, THREADS, 2)
    lane = np.zeros((tiles, THREADS))
    for pj in range(PAIRS):
        for el in range(2):
            lane = np.where(ok[:, pj, :, el], lane + v[:, pj, :, el], lane)
    idx = np.arange(THREADS)
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, idx ^ o]
    w = lane[:, ::64]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    total = np.float64(0.0)
    for x in range(tiles):
        total = total + part[x]
    return total


def combine(pool, draw_row, factor, e, mode, frames=None):
    """pool complex64 [N, F, T], draw_row [B][K] -> (out complex128 [B, F, T] before its one rounding to fp32, spread float64 [B, F, T],
    rows float64 [B, 2 + K], best [B])"""
    N, F, T = pool.shape
    B, K = len(draw_row), len(draw_row[0])
    out = np.zeros((B, F, T), dtype=np.complex128)
    spread = np.zeros((B, F, T))
    rows = np.zeros((B, 2 + K))
    best = np.zeros(B, dtype=np.int32)
    Kd = np.float64(K)
    for b in range(B):
        valid = T if frames is None else int(frames[b])
        ok = np.broadcast_to(np.arange(T) < valid, (F, T))
        xs = [back_transform(np.where(ok, pool[draw_row[b][k]], 0), factor, e) for k in range(K)]       # (bins past frames[b] are never read)
        sr, si, sg = np.zeros((F, T)), np.zeros((F, T)), np.zeros((F, T))
        for xr, xi, g in xs:
            sr, si, sg = sr + xr, si + xi, sg + g
        cr, ci = sr / Kd, si / Kd
        cn2 = cr * cr + ci * ci
        sd, q = np.zeros((F, T)), []
        for xr, xi, _ in xs:
            dr, di = xr - cr, xi - ci
            q.append(dr * dr + di * di)
            sd = sd + q[-1]
        s = np.sqrt(sd / np.float64(K - 1)) if K > 1 else np.zeros((F, T))
        if mode == "mean":
            vr, vi = cr, ci
        else:
            if mode == "mag_mean":
                a = sg / Kd
            else:
                srt = np.sort(np.stack([g for _, _, g in xs]), axis=0)
                a = srt[(K - 1) // 2] if K % 2 else 0.5 * (srt[K // 2 - 1] + srt[K // 2])
            n = np.sqrt(cn2)
            nz = n != 0.0
            ns = np.where(nz, n, 1.0)
            vr, vi = np.where(nz, a * (cr / ns), 0.0), np.where(nz, a * (ci / ns), 0.0)
        out[b].real, out[b].imag = np.where(ok, vr, 0.0), np.where(ok, vi, 0.0)       # (no complex arithmetic: it would lose a zero's sign)
        spread[b] = np.where(ok, s, 0.0)
        okf = ok.reshape(-1)
        rows[b, 0] = _ordered_sum(cn2.reshape(-1), okf)
        for k in range(K):
            rows[b, 2 + k] = _ordered_sum(q[k].reshape(-1), okf)
        tot = np.float64(0.0)
        for k in range(K):
            tot = tot + rows[b, 2 + k]
        rows[b, 1] = tot / Kd
        arg = 0
        for k in range(K):
            if rows[b, 2 + k] < rows[b, 2 + arg]:
                arg = k
        best[b] = arg
    return out, spread, rows, best


def n_terms(F, T, K, valid=None):
    """the terms behind one number of rows_out: the row's valid bins (the sum), K roundings of the mean and K of D, and 32 for a bin's own
    chain (a square root, quotients, products, a pow of a few units in the last place)"""
    return F * (T if valid is None else valid) + 2 * K + 32


def pool_for(N, F, T, seed):
    """a Gaussian pool whose |z| spans four decades (a per-element scale 10^u, u uniform in [-3, 1]), with a few exact zeros"""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((N, F, T)) + 1j * rng.standard_normal((N, F, T))) * 10.0 ** rng.uniform(-3.0, 1.0, (N, F, T))
    z = z.astype(np.complex64)
    flat = z.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = 0
    return z


# (F, T, K, B, mode, transform index): a covering table.  F in {1, 5, 257}, T in {1, 2, 63, 64, 65, 130}, B in {1, 3}; every K of
# {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32} with an odd T; every mode at K = 2, 5, 32; every transform with every mode; one tile, a cut tile and
# up to 33 tiles (257 x 130 = 33410 bins); odd F T with B = 3 (odd utterances start off a 16-byte boundary in out).
KERNEL_CASES = [
    (5, 63, 1, 1, "mean", 0), (1, 1, 2, 3, "mean", 1), (5, 65, 2, 1, "mag_mean", 0), (257, 1, 2, 1, "mag_median", 2),
    (1, 63, 3, 3, "mag_median", 1), (5, 65, 4, 1, "mag_median", 0), (257, 65, 5, 1, "mean", 1), (5, 63, 5, 3, "mag_mean", 2),
    (1, 65, 5, 1, "mag_median", 0), (5, 63, 8, 1, "mag_median", 1), (5, 65, 9, 3, "mag_median", 0), (257, 63, 16, 1, "mag_mean", 2),
    (5, 65, 17, 1, "mag_median", 1), (1, 63, 31, 3, "mag_median", 0), (5, 65, 32, 1, "mean", 0), (5, 63, 32, 1, "mag_mean", 1),
    (5, 63, 32, 3, "mag_median", 2), (5, 2, 3, 1, "mean", 0), (5, 64, 4, 3, "mag_mean", 1), (257, 130, 3, 1, "mag_median", 0),
    (1, 130, 8, 1, "mean", 2), (1, 2, 16, 3, "mag_median", 1),
]


def case_id(c):
    return "-".join(str(v) for v in c)


def draw_rows(B, K, seed):
    """a [B][K] table over a pool of B K + 2 rows: a seeded permutation, so that no utterance's draws are consecutive pool rows"""
    perm = np.random.default_rng(seed).permutation(B * K + 2)[:B * K]
    return [[int(v) for v in perm[b * K:(b + 1) * K]] for b in range(B)]


@functools.lru_cache(maxsize=None)
def kernel_case(c):
    """(pool, draw_row, reference) of a case of KERNEL_CASES: computed once, shared, never written to"""
    F, T, K, B, mode, tf = c
    seed = 1000 + KERNEL_CASES.index(c)
    pool = pool_for(B * K + 2, F, T, seed)
    rows = draw_rows(B, K, seed)
    ref = combine(pool, rows, *TRANSFORMS[tf], mode)
    pool.setflags(write=False)
    return pool, rows, ref
