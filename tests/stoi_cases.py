"""Cases and the float64 numpy restatement of STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) as include/storm_hip.h defines them
for storm_stoi_rows.  Nothing here was compared with the `pystoi` package (it is installed on none of the project's machines): the
restatement follows the published algorithm and the header's text, and the ANCHORS are the values the definition's author obtained from
an independent restatement (scipy's resample_poly in float64, no EPS in the ESTOI denominators)."""
import functools
import math

import numpy as np

FS, N_FRAME, HOP, NFFT, NUM_BANDS, MIN_FREQ, N_SEG, BETA, DYN_RANGE = 10000, 256, 128, 512, 15, 150, 30, -15.0, 40.0
EPS = float(np.finfo(np.float64).eps)                                  # 2^-52
TOO_SHORT = 1e-5                                                       # fewer than N_SEG spectrogram frames
BAND_EDGES = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)

# name: (seed, n, fs, snr_db, gaps)
CASES = {
    "a16k": (11, 32000, 16000, 5, [(0.3, 0.45)]),
    "b16k": (12, 16001, 16000, 0, []),
    "c10k": (43, 20000, 10000, 10, [(0, 0.1), (0.6, 0.7)]),
    "d10k_min": (14, 4224, 10000, 3, []),
    "e10k_short": (15, 4096, 10000, 3, []),
    "f8k": (16, 12000, 8000, -5, [(0.5, 0.62)]),
    "g48k": (17, 60000, 48000, 15, []),
}
# name: (ESTOI, STOI, frames, kept frames, segments)
ANCHORS = {
    "a16k": (0.554863220463, 0.891634270393, 155, 133, 103),
    "b16k": (0.413031712860, 0.748459163738, 77, 77, 47),
    "c10k": (0.703308530955, 0.948283164949, 155, 126, 96),
    "d10k_min": (0.356661216474, 0.724027085997, 31, 31, 1),
    "e10k_short": (1e-5, 1e-5, 30, 30, 0),                             # 30 frames, all kept: M = 29 spectrogram frames, no segment
    "f8k": (0.270203715710, 0.510816022568, 116, 104, 74),
    "g48k": (0.984579373931, 0.998761758436, 96, 96, 66),
}


def case(seed, n, fs, snr_db, gaps):
    r = np.random.default_rng(seed); t = np.arange(n) / fs
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + 0.3)
    c = r.standard_normal(n); c = np.convolve(c, np.ones(8) / 8, mode="same") * env
    for a, b in gaps: c[int(a * n):int(b * n)] *= 1e-4
    v = r.standard_normal(n); v *= np.sqrt((c**2).sum() / (v**2).sum()) * 10 ** (-snr_db / 20)
    return c.astype(np.float32), (c + v).astype(np.float32)      # clean, processed


@functools.lru_cache(maxsize=None)
def signals(name):
    """(clean, processed) fp32 of a case; cached - never modify the arrays"""
    c, p = case(*CASES[name])
    c.setflags(write=False)
    p.setflags(write=False)
    return c, p


def ratio(fs_sig):
    g = math.gcd(FS, int(fs_sig))
    return FS // g, int(fs_sig) // g


def resample_filter(fs_sig):
    """h (float64, sum 1) of the definition's step 1: Kaiser windowed sinc with 60 dB rejection, 2 L + 1 taps"""
    up, down = ratio(fs_sig)
    fc = 1.0 / (2 * max(up, down))
    half = int(np.ceil((60.0 - 8.0) / (28.714 * (fc / 10.0))))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2 * up * fc * np.sinc(2 * fc * t))
    return h / np.sum(h)


def resample64(x, fs_sig):
    """step 1 in float64: scipy.signal.resample_poly with the filter above"""
    from scipy.signal import resample_poly
    up, down = ratio(fs_sig)
    x = np.asarray(x, np.float64)
    return x.copy() if up == down else resample_poly(x, up, down, window=resample_filter(fs_sig))


def band_edges():
    """the third-octave band edges as FFT bins, computed as the definition's step 4 does"""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    k = np.arange(NUM_BANDS)
    lo = [int(np.argmin((f - MIN_FREQ * 2.0 ** ((2 * i - 1) / 6)) ** 2)) for i in k]
    hi = [int(np.argmin((f - MIN_FREQ * 2.0 ** ((2 * i + 1) / 6)) ** 2)) for i in k]
    return lo, hi


def _window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_energies(x):
    """(frames [K0, 256] already windowed, energies in dB [K0]) of step 2"""
    w = _window()
    starts = range(0, len(x) - N_FRAME, HOP)
    frames = np.array([w * x[i:i + N_FRAME] for i in starts]).reshape(-1, N_FRAME)
    return frames, 20 * np.log10(np.linalg.norm(frames, axis=1) + EPS)


def _overlap_add(frames):
    out = np.zeros((len(frames) - 1) * HOP + N_FRAME)
    for i, f in enumerate(frames):
        out[i * HOP:i * HOP + N_FRAME] += f
    return out


def _tob(x):
    w = _window()
    frames = np.array([w * x[i:i + N_FRAME] for i in range(0, len(x) - N_FRAME, HOP)]).reshape(-1, N_FRAME)
    spec = np.abs(np.fft.rfft(frames, n=NFFT, axis=1)) ** 2               # [M, 257]
    return np.sqrt(np.array([spec[:, BAND_EDGES[i]:BAND_EDGES[i + 1]].sum(axis=1) for i in range(NUM_BANDS)]))      # [15, M]


def stoi64(x, y, fs_sig):
    """dict(stoi, estoi, frames, kept, segments, margin): the definition in float64 on two equally long 1-D signals.  margin: the smallest
    distance in dB of a frame's energy from the gate threshold (inf without a frame)."""
    x, y = resample64(x, fs_sig), resample64(y, fs_sig)
    out = dict(stoi=TOO_SHORT, estoi=TOO_SHORT, frames=0, kept=0, segments=0, margin=math.inf)
    if len(x) <= N_FRAME:
        return out
    xf, e = frame_energies(x)
    yf, _ = frame_energies(y)
    dist = np.max(e) - DYN_RANGE - e
    mask = dist < 0
    out.update(frames=len(e), kept=int(mask.sum()), margin=float(np.abs(dist).min()))
    X, Y = _tob(_overlap_add(xf[mask])), _tob(_overlap_add(yf[mask]))
    M = X.shape[1]
    if M < N_SEG:
        return out
    xs = np.array([X[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])     # [J, 15, 30]
    ys = np.array([Y[:, m - N_SEG:m] for m in range(N_SEG, M + 1)])
    J = xs.shape[0]

    def row_col_normalize(a):
        a = a - a.mean(axis=2, keepdims=True)
        a = a / (np.linalg.norm(a, axis=2, keepdims=True) + EPS)
        a = a - a.mean(axis=1, keepdims=True)
        return a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
    estoi = float(np.sum(row_col_normalize(xs) * row_col_normalize(ys)) / (N_SEG * J))
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(c * ys, xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xm = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xm = xm / (np.linalg.norm(xm, axis=2, keepdims=True) + EPS)
    stoi = float(np.sum(xm * yp) / (NUM_BANDS * J))
    out.update(stoi=stoi, estoi=estoi, segments=J)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """stoi64 of a case at its own rate (computed once)"""
    c, p = signals(name)
    return stoi64(c, p, CASES[name][2])


@functools.lru_cache(maxsize=None)
def at_10k_fp32(name):
    """(clean, processed) of a case resampled to 10 kHz by scipy in float64 and rounded to fp32 - inputs of the 10 kHz kernel tests"""
    c, p = signals(name)
    fs = CASES[name][2]
    out = resample64(c, fs).astype(np.float32), resample64(p, fs).astype(np.float32)
    for a in out:
        a.setflags(write=False)
    return out
