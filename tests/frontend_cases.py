"""Case tables, seeded inputs and float64 references for tests/test_frontend_edges.py (storm_peak_abs, storm_stft, storm_istft at the
edges of their argument range).

The reference of every case is torch.stft / torch.istft in float64 with the arguments the reference's data module passes: periodic Hann
or its square root, center=True, reflect padding (sgmse/data_module.py:19-25, 217-223).  Every tolerance is measured from that reference
alone: what torch's own float32 transform shows against float64 on the same fp32 samples, times MARGIN.  The kernels accumulate in fp64
from fp32 products and an fp32 twiddle table, so they should be no worse than an fp32 FFT; MARGIN = 4 leaves room for the difference
between the two summation orders and for the device's powf / sqrtf, and nothing for a wrong sample."""
import functools

import torch

MARGIN = 4.0
KEEP = 1e-3                     # inverse: samples whose window envelope is at least KEEP of its maximum are compared unweighted
MAX_LEFT_OUT = 0.10             # ... and they are at least 90 % of every case (the reference envelope alone leaves out at most 7.5 %)

# (n_fft, hop, window): both parities, the table limit (MAX_NFFT = 1024), a hop above n_fft / 2, a hop that does not divide n_fft
SETTINGS = (
    (510, 128, "hann"),
    (510, 128, "sqrthann"),
    (511, 128, "sqrthann"),
    (255, 64, "hann"),
    (254, 64, "hann"),
    (1024, 256, "hann"),
    (510, 256, "sqrthann"),
    (510, 100, "hann"),
    (64, 16, "hann"),
    (7, 3, "sqrthann"),
)
FUSED_SETTINGS = tuple(s for s in SETTINGS if s[0] in (510, 511) and s[1] == 128)
RAGGED_SETTINGS = ((510, 128, "hann"), (511, 128, "sqrthann"))
COMPRESSIONS = ((0.5, 0.15), (0.667, 0.065), (1.0, 1.0))        # (spec_abs_exponent, spec_factor)
BATCH = 2


def setting_id(s):
    return f"{s[0]}-{s[1]}-{s[2]}"


def torch_frames(length, n_fft, hop):
    """frames of torch.stft(center=True), from its definition: the padded signal has length + 2 (n_fft // 2) samples"""
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop


def lengths(n_fft, hop):
    """the edge lengths of one setting, ascending, at most 64 frames each.  A row needs more than p = n_fft // 2 samples (torch.stft
    refuses reflect padding otherwise), so entries of the list that are not longer than p are no cases (2 hop - 1 = p at 510 / 128,
    2 hop + 1 < p at 510 / 100): the refusal test owns them."""
    p = n_fft // 2
    want = (p + 1, p + 2, 2 * hop - 1, 2 * hop, 2 * hop + 1, n_fft - 1, n_fft, n_fft + 1, 5 * hop + hop // 2, 9 * hop - 1, 9 * hop,
            63 * hop + 1, 64 * hop - 1)
    return tuple(sorted({L for L in want if L > p}))


def window(n_fft, kind, dtype=torch.float64):
    w = torch.hann_window(n_fft, periodic=True, dtype=dtype)
    return torch.sqrt(w) if kind == "sqrthann" else w


@functools.lru_cache(maxsize=None)
def signal(L, seed=0):
    """fp32 [BATCH, L]: seeded white noise of standard deviation 0.3"""
    return torch.randn(BATCH, L, generator=torch.Generator().manual_seed(1_000_003 * seed + L)) * 0.3


@functools.lru_cache(maxsize=None)
def spectrum(F, T, even, seed=0):
    """complex64 [BATCH, F, T]: seeded, DC real and (even n_fft) Nyquist real, as the transform of a real signal"""
    g = torch.Generator().manual_seed(7919 * seed + 64 * F + T)
    X = torch.complex(torch.randn(BATCH, F, T, generator=g), torch.randn(BATCH, F, T, generator=g))
    X[:, 0] = X[:, 0].real.to(torch.complex64)
    if even:
        X[:, -1] = X[:, -1].real.to(torch.complex64)
    return X


def stft_t(y, setting, dtype):
    n_fft, hop, kind = setting
    return torch.stft(y.to(dtype), n_fft=n_fft, hop_length=hop, window=window(n_fft, kind, dtype), center=True, return_complex=True)


def istft_t(X, setting, length, dtype):
    n_fft, hop, kind = setting
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    return torch.istft(X.to(cdt), n_fft=n_fft, hop_length=hop, window=window(n_fft, kind, dtype), center=True, length=length)


def spec_fwd_t(spec, e, factor):
    """data_module.py:182-186 in the dtype of `spec`"""
    if e != 1:
        spec = spec.abs() ** e * torch.exp(1j * spec.angle())
    return spec * factor


def frame_err(Y, ref):
    """worst frame of a batch: max over bins of |Y - ref|, divided by that frame's largest |ref| (float64)"""
    d = (Y.to(torch.complex128) - ref).abs().amax(dim=-2)
    m = ref.abs().amax(dim=-2)
    return float((d / m).max())


@functools.lru_cache(maxsize=None)
def stft_case(setting, L, scale=1.0):
    """(y fp32, ref complex128, torch fp32's frame_err) of one forward case"""
    y = signal(L) * scale
    ref = stft_t(y, setting, torch.float64)
    return y, ref, frame_err(stft_t(y, setting, torch.float32), ref)


@functools.lru_cache(maxsize=None)
def fused_case(setting, L, e, factor, scale=1.0):
    """(y fp32, peak fp32 [BATCH], ref complex128 = spec_fwd(stft(y / peak)), torch fp32's frame_err of the same expression)"""
    y = signal(L) * scale
    peak = y.abs().amax(dim=1)
    ref = spec_fwd_t(stft_t(y.double() / peak.double()[:, None], setting, torch.float64), e, factor)
    t32 = spec_fwd_t(stft_t(y / peak[:, None], setting, torch.float32), e, factor)
    return y, peak, ref, frame_err(t32, ref)


def envelope(setting, T, length):
    """float64 [length]: the window envelope sum_t w^2[n + p - t hop] that istft divides by, over the samples it returns"""
    n_fft, hop, kind = setting
    w2 = window(n_fft, kind) ** 2
    env = torch.zeros(n_fft + hop * (T - 1), dtype=torch.float64)
    for t in range(T):
        env[t * hop:t * hop + n_fft] += w2
    return env[n_fft // 2:n_fft // 2 + length]


def istft_lengths(setting, L):
    """output lengths of the inverse of a T-frame spectrum, T = frames of L: L itself, the default hop (T - 1) and the largest covered"""
    n_fft, hop, _ = setting
    T = torch_frames(L, n_fft, hop)
    return T, tuple(sorted({n for n in (L, hop * (T - 1), n_fft + hop * (T - 1) - n_fft // 2) if n > 0}))


def wav_err(x, ref, env):
    """(weighted, kept, share left out) of a batch of inverses [BATCH, length] against float64:
    weighted = max_n |x - ref| env / max env, over the largest |ref| of the row: the error of the overlap-add numerator
    kept     = max |x - ref| over the samples with env >= KEEP max env, over the largest |ref| among them
    (the division by the envelope amplifies rounding without bound where the envelope vanishes: at the last covered sample of a Hann
    window it is 1e-10 of its maximum)"""
    d = (x.double() - ref).abs()
    rel = env / env.max()
    weighted = float(((d * rel).amax(dim=1) / ref.abs().amax(dim=1)).max())
    keep = rel >= KEEP
    kept = float((d[:, keep].amax(dim=1) / ref[:, keep].abs().amax(dim=1)).max())
    return weighted, kept, 1.0 - float(keep.double().mean())


@functools.lru_cache(maxsize=None)
def istft_case(setting, L, length):
    """(X complex64, ref fp64 [BATCH, length], env, torch fp32's wav_err) of one inverse case"""
    n_fft, hop, _ = setting
    T = torch_frames(L, n_fft, hop)
    X = spectrum(n_fft // 2 + 1, T, n_fft % 2 == 0)
    ref = istft_t(X, setting, length, torch.float64)
    env = envelope(setting, T, length)
    return X, ref, env, wav_err(istft_t(X, setting, length, torch.float32), ref, env)


@functools.lru_cache(maxsize=None)
def round_trip_torch32(setting, L):
    """torch fp32's own istft(stft(y), L) against y: (kept error, share left out)"""
    n_fft, hop, _ = setting
    y = signal(L)
    back = istft_t(stft_t(y, setting, torch.float32), setting, L, torch.float32)
    _, kept, out = wav_err(back, y.double(), envelope(setting, torch_frames(L, n_fft, hop), L))
    return kept, out


# ---- ragged batches: frame counts of 63 and 64 under one padded count of 64; 8192 is 65 frames at 510 and 64 at 511 ----------------------
def ragged_lengths(n_fft):
    return (8064, 7937, 8191, 8100) + ((8192,) if n_fft % 2 else ())
