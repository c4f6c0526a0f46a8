"""The frame-based measures of include/storm_hip.h (storm_lpc_measures_rows) restated in numpy, frame by frame, in float64 and again in
np.longdouble - the reference of tests/test_lpc_measures.py - and the seeded signals of its cases.  Nothing here is compared with pysepm:
the header's text is the specification."""
import functools

import numpy as np

FS = (16000, 8000, 44100)
EPS = 2.0 ** -52
STOP = 2.0 ** -40
CAP = 0.10                                # a measured case has at most this share of its frames at a clamp (a clamped frame hides its error)
FLOOR = 1e-10                             # three orders above fp64 rounding of 480-term sums, ten below any indexing error


def shape(fs):
    """(W, H, P): window, hop, LPC order"""
    W = (30 * fs + 500) // 1000
    return W, W // 4, 16 if fs >= 10000 else 10


def n_frames(length, fs):
    W, H, _ = shape(fs)
    return (length - W) // H if length >= W else 0


def n_keep(m_valid):
    return max(1, (19 * m_valid + 10) // 20)                                   # floor(0.95 M' + 0.5)


def window(fs, T=np.float64):
    W = shape(fs)[0]
    pi = T(4) * np.arctan(T(1))
    return (T(0.5) * (T(1) - np.cos(T(2) * pi * (np.arange(W).astype(T) + T(1)) / T(W + 1)))).astype(T)


def levinson(r, P, T=np.float64):
    """a = (1, a_1 .. a_P) of the header's step 4"""
    a = np.zeros(P + 1, dtype=T)
    a[0] = T(1)
    E = r[0]
    for i in range(1, P + 1):
        if E <= T(STOP) * r[0]:
            break
        acc = r[i]
        for j in range(1, i):
            acc = acc + a[j] * r[i - j]
        k = -acc / E
        old = a.copy()
        for j in range(1, i):
            a[j] = old[j] + k * old[i - j]
        a[i] = k
        E = E * (T(1) - k * k)
    return a


def cepstrum(a, P, T=np.float64):
    c = np.zeros(P + 1, dtype=T)
    for n in range(1, P + 1):
        acc = T(0)
        for k in range(1, n):
            acc = acc + (T(k) / T(n)) * c[k] * a[n - k]
        c[n] = -a[n] - acc
    return c


def clamp(v, lo, hi, T):
    return min(max(v, T(lo)), T(hi))


def autocorr(v, P):
    return np.array([np.dot(v[:len(v) - k], v[k:]) for k in range(P + 1)], dtype=v.dtype)


def toeplitz_form(a, r, P):
    R = np.array([[r[abs(i - j)] for j in range(P + 1)] for i in range(P + 1)], dtype=a.dtype)
    return np.dot(a, np.dot(R, a))


def frame_values(x, y, fs, T=np.float64):
    """[M, 3] = (segmental SNR, LLR, CD) of every frame of the row (x clean, y processed: 1-D, read as fp32), NaN in LLR and CD for a void
    frame; arithmetic in T"""
    W, H, P = shape(fs)
    x, y = np.asarray(x, dtype=np.float32).astype(T), np.asarray(y, dtype=np.float32).astype(T)
    w = window(fs, T)
    M = n_frames(len(x), fs)
    out = np.full((M, 3), np.nan, dtype=T)
    for m in range(M):
        c, p = w * x[m * H:m * H + W], w * y[m * H:m * H + W]
        d = c - p
        out[m, 0] = clamp(T(10) * np.log10(np.dot(c, c) / (np.dot(d, d) + T(EPS)) + T(EPS)), -10, 35, T)
        rc, rp = autocorr(c, P), autocorr(p, P)
        if rc[0] <= 0 or rp[0] <= 0:
            continue
        ac, ap = levinson(rc, P, T), levinson(rp, P, T)
        out[m, 1] = clamp(np.log(toeplitz_form(ap, rc, P) / toeplitz_form(ac, rc, P)), 0, 2, T)
        dc = cepstrum(ac, P, T)[1:] - cepstrum(ap, P, T)[1:]
        out[m, 2] = clamp(T(10) / np.log(T(10)) * np.sqrt(T(2) * np.dot(dc, dc)), 0, 10, T)
    return out


def row_values(frames):
    """((segmental SNR, LLR, CD), M, M') of a row from its frame values"""
    T = frames.dtype.type
    M = frames.shape[0]
    ok = ~np.isnan(frames[:, 1]) if M else np.zeros(0, dtype=bool)
    Mv = int(ok.sum())
    out = np.full(3, np.nan, dtype=frames.dtype)
    if M:
        out[0] = np.sum(frames[:, 0]) / T(M)
    if Mv:
        k = n_keep(Mv)
        for u in (1, 2):
            out[u] = np.sum(np.sort(frames[ok, u])[:k]) / T(k)
    return out, M, Mv


def reference_xy(x, y, fs):
    """(float64 frames [M, 3], float64 row values [3], M, M', per-unit bounds [3], per-unit share of clamped frames [3]) of one row.  The
    bound of a unit is max(16 x the largest |float64 - longdouble| over the row's frames, FLOOR); where longdouble is no wider than double
    the floor alone applies."""
    f64, fld = frame_values(x, y, fs), frame_values(x, y, fs, np.longdouble)
    row, M, Mv = row_values(f64)
    bound = np.full(3, FLOOR)
    clamped = np.zeros(3)
    if M:
        wider = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
        diff = np.abs(f64.astype(np.longdouble) - fld)
        for u, (lo, hi) in enumerate(((-10.0, 35.0), (0.0, 2.0), (0.0, 10.0))):
            ok = ~np.isnan(f64[:, u])
            if ok.any():
                if wider:
                    bound[u] = max(16.0 * float(diff[ok, u].max()), FLOOR)
                clamped[u] = float(np.mean((f64[ok, u] == lo) | (f64[ok, u] == hi)))
    return f64, row, M, Mv, bound, clamped


@functools.lru_cache(maxsize=None)
def reference(key):
    """reference_xy of the seeded pair key = (fs, snr_db, length); computed once, shared, not to be written to"""
    return reference_xy(*pair(*key), key[0])


# ---- signals ---------------------------------------------------------------------------------------------------------------------------------
def speech_like(fs, length, seed):
    """a noise-excited resonator (two formant-like pole pairs of moderate sharpness) under a slow envelope, fp32, peak 0.5"""
    from scipy.signal import lfilter
    g = np.random.default_rng(seed)
    e = g.standard_normal(length + 256)
    a = np.array([1.0])
    for f, r in ((0.0625 * fs, 0.90), (0.1875 * fs, 0.85)):
        a = np.convolve(a, [1.0, -2.0 * r * np.cos(2.0 * np.pi * f / fs), r * r])
    v = lfilter([1.0], a, e)[256:]
    v = v * (0.6 + 0.4 * np.sin(2.0 * np.pi * np.arange(length) / (0.11 * fs) + 0.3))
    return (0.5 * v / np.abs(v).max()).astype(np.float32)


def add_noise(x, snr_db, seed):
    """x plus white noise at snr_db below the whole row's power, fp32"""
    g = np.random.default_rng(seed)
    n = g.standard_normal(len(x))
    n *= np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(n ** 2)) * 10.0 ** (-snr_db / 20.0)
    return (x.astype(np.float64) + n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(fs, snr_db, length):
    x = speech_like(fs, max(length, 1), 1000 + fs % 997)
    return x, add_noise(x, snr_db, 7 + int(snr_db))


def lowpassed(x):
    """x through a 4th-order Butterworth low-pass at half Nyquist, fp32"""
    from scipy.signal import butter, lfilter
    b, a = butter(4, 0.5)
    return lfilter(b, a, x.astype(np.float64)).astype(np.float32)


def lengths_of(fs):
    W, H, _ = shape(fs)
    return [W - 1, W, W + H - 1, W + H, W + H + 1] + ([4000] if fs == 16000 else []) + [2045]


def candidates():
    return [(fs, snr, L) for fs in FS for snr in (30, 20) for L in lengths_of(fs)]


@functools.lru_cache(maxsize=None)
def measured_cases():
    """the (fs, snr_db, length) that count as measured: every 30 dB case (the test asserts the cap on them) and the 20 dB cases that meet the cap"""
    return tuple(k for k in candidates() if k[1] == 30 or reference(k)[5].max() <= CAP)
