"""Small utilities of sgmse/util/other.py that the hot path and the evaluation loop use:
pad_spec (:102-109), si_sdr / si_sdr_torch (:82-94), and the metrics of the calc_metrics step in batch form on the device:
energy_ratios (:21-44), lsd (:16-19), snr_dB (:96-100); mean_std (:53-57) on the host; stoi: STOI / ESTOI on the device under the
signature of pystoi.stoi, which the reference's evaluation calls; align (:153-157) and hp_filter (:76-80) on the device; sdr: the BSS-eval SDR with a short filter,
which the reference does not have; lpc_measures / seg_snr / llr / cepstral_distance: the frame-based measures, which it does not have either."""
import warnings

import numpy as np
import torch


def pad_spec(Y):
    T = Y.size(3)
    num_pad = 64 - T % 64 if T % 64 != 0 else 0
    return torch.nn.functional.pad(Y, (0, num_pad, 0, 0))


def si_sdr(s, s_hat):
    """numpy, one pair (util/other.py:82-86) - the host-side definition the evaluation loop of the reference uses"""
    alpha = np.dot(s_hat, s) / np.linalg.norm(s) ** 2
    return 10 * np.log10(np.linalg.norm(alpha * s) ** 2 / np.linalg.norm(alpha * s - s_hat) ** 2)


def si_sdr_torch(s, s_hat):
    """one pair of 1-D tensors (util/other.py:88-94, the eps = 1e-10 variant): a 0-d tensor.  On a HIP device the sums run
    in one kernel (storm_si_sdr); CPU tensors (host-side metric code) use the same formula in torch."""
    min_len = min(s.size(-1), s_hat.size(-1))
    s, s_hat = s[..., :min_len], s_hat[..., :min_len]
    if s.is_cuda:
        from .. import ops
        return ops.si_sdr(s.reshape(1, -1).float().contiguous(), s_hat.reshape(1, -1).float().contiguous(), eps=1e-10)[0]
    alpha = torch.dot(s_hat, s) / torch.norm(s) ** 2
    return 10 * torch.log10(1e-10 + torch.norm(alpha * s) ** 2 / (1e-10 + torch.norm(alpha * s - s_hat) ** 2))


def si_sdr_batch(s, s_hat, eps=0.0):
    """[B, L] device tensors -> [B] dB (one launch for the whole evaluation batch)"""
    from .. import ops
    return ops.si_sdr(s.float(), s_hat.float(), eps=eps)


def _rows(x):
    """a waveform or a batch of waveforms as a float32 batch [B, L]"""
    x = x.float()
    return x.reshape(1, -1) if x.dim() == 1 else x


def energy_ratios(s_hat, s, n, lengths=None):
    """(si_sdr, si_sir, si_sar) in dB, fp64 [B]: util/other.py:35-44 for every row of the device batches [B, L] (1-D tensors: one row);
    eps = 1e-10 as si_sdr_components places it.  lengths: per-row sample counts of a ragged batch.  One kernel pair for the batch
    (storm_energy_ratios_rows); a row's numbers do not depend on the batch it is in."""
    from .. import ops
    r = ops.energy_ratios_rows(_rows(s_hat), _rows(s), _rows(n), lengths=lengths)
    return r[:, 0], r[:, 1], r[:, 2]


def snr_dB(s, n, lengths=None):
    """10 log10(mean s^2 / mean n^2) per row, fp64 [B] (util/other.py:96-100)"""
    from .. import ops
    s = _rows(s)
    return ops.energy_ratios_rows(s, s, _rows(n), lengths=lengths)[:, 3]


def lsd(s_hat, s, lengths=None, eps=1e-10):
    """log-spectral distance per row of two waveform batches [B, L], fp64 [B] (util/other.py:16-19): the two STFTs (n_fft = 510, hop = 128,
    periodic Hann, as stft_kwargs :14) are the engine's own, then storm_lsd_rows.  lengths: per-row sample counts; row b counts its own
    1 + lengths[b] // 128 frames.  A row of <= 255 samples is refused by the STFT (reflect padding), as torch.stft refuses it."""
    from .. import ops
    s_hat, s = _rows(s_hat).contiguous(), _rows(s).contiguous()
    if s_hat.shape != s.shape:
        raise ValueError(f"lsd: {tuple(s_hat.shape)} against {tuple(s.shape)}")
    if lengths is not None and len(lengths) != s.shape[0]:
        raise ValueError(f"lsd: {len(lengths)} lengths for a batch of {s.shape[0]} rows")
    S_hat, S = ops.stft(s_hat, lengths=lengths), ops.stft(s, lengths=lengths)
    frames = None if lengths is None else [1 + int(v) // 128 for v in lengths]
    return ops.lsd_rows(S_hat, S, frames=frames, eps=eps)


def stoi(x, y, fs_sig, extended=False, lengths=None):
    """STOI (extended=False) or ESTOI (extended=True) of the processed signal y against the clean x at fs_sig Hz, under pystoi.stoi's
    signature, on the device: resampling to 10 kHz and storm_stoi_rows (include/storm_hip.h has the definition; its numbers were checked
    against a float64 restatement of the published algorithm, not against pystoi).  x, y: 1-D -> a float; [B, L] -> an fp64 tensor [B]
    (lengths: per-row sample counts of a ragged batch).  numpy arrays are moved to the current HIP device; any other dtype (pystoi's callers
    pass float64) is rounded to fp32, which is what the kernels read.  A signal with fewer than 30
    frames left after the silent-frame gate gives 1e-5 and pystoi's RuntimeWarning."""
    from .. import _lib, ops
    dev = None
    for v in (x, y):
        if isinstance(v, torch.Tensor):
            dev = v.device
    if dev is None:
        dev = torch.device("cpu") if _lib.is_sim() else torch.device("cuda", torch.cuda.current_device())
    x, y = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)) for v in (x, y))
    if x.shape != y.shape:
        raise Exception("x and y should have the same length," + f"found {tuple(x.shape)} and {tuple(y.shape)}")      # (pystoi raises this)
    one = x.dim() == 1
    r, counts = ops.stoi_rows(_rows(x).to(dev, torch.float32), _rows(y).to(dev, torch.float32), lengths=lengths, fs=fs_sig, counts=True)
    d = r[:, 1 if extended else 0]
    if bool((counts[:, 2] < 1).any()):
        warnings.warn("Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. Returning 1e-5. "
                      "Please check you wav files", RuntimeWarning)
    return float(d[0]) if one else d


def _device_rows(*xs):
    """the arguments as tensors on one device (numpy arrays are moved to the current HIP device), and whether the first is 1-D"""
    from .. import _lib
    dev = None
    for v in xs:
        if isinstance(v, torch.Tensor):
            dev = v.device
    if dev is None:
        dev = torch.device("cpu") if _lib.is_sim() else torch.device("cuda", torch.cuda.current_device())
    ts = [v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)) for v in xs]
    return [_rows(t.to(dev)) for t in ts], ts[0].dim() == 1


def align(y, ref, lengths=None, max_lag=None, wrap=True):
    """y moved onto ref (util/other.py:153-157) on the device: the arg-max of the full cross-correlation of every row (storm_xcorr_lag_rows:
    two launches, exact fp64 chains instead of the reference's fftconvolve - the two agree wherever the peak is clear), then one gather
    (storm_shift_rows) that reads the lag from device memory.  Nothing is synchronised and the result stays on the device.  y, ref: 1-D or
    [B, L] (fp32 is what the kernels read); lengths: per-row sample counts of a ragged batch, for y and ref alike.  max_lag: search only
    |lag| <= max_lag samples (None: unbounded, as the reference).  wrap=True rolls like the reference's np.roll; wrap=False fills with zeros.
    The shift is the reference's expression l = argmax - (len(ref) - 1) taken literally, which is lag + len(y) - len(ref): the lag itself for
    equal lengths; for unequal lengths that is the reference's own (surprising) choice, reproduced here, and costs one more tiny launch."""
    from .. import ops
    (yr, rr), one = _device_rows(y, ref)
    lag, _ = ops.xcorr_lag_rows(yr, rr, lengths=lengths, ref_lengths=lengths, max_lag=max_lag)
    if lengths is None and yr.shape[1] != rr.shape[1]:
        lag = lag + (yr.shape[1] - rr.shape[1])
    out = ops.shift_rows(yr, lag, lengths=lengths, wrap=wrap)
    return out[0] if one else out


def hp_filter(signal, cut_off=80, order=10, sr=16000, lengths=None):
    """Butterworth high-pass of every row (util/other.py:76-80): the sections of scipy.signal.butter(order, cut_off / sr * 2, 'hp',
    output='sos') as the library designs them (storm_butter_sos: even orders) through storm_sosfilt_rows, which restates scipy.signal.sosfilt
    bit for bit.  signal: [L] or [B, L] (fp32 is what the kernel reads); returns float64 like the reference, on the device."""
    from .. import ops
    (x,), one = _device_rows(signal)
    out = ops.sosfilt_rows(x, ops.butter_sos(order, cut_off / sr * 2, "hp"), lengths=lengths, out_dtype=torch.float64)
    return out[0] if one else out


def sdr(s, s_hat, flen=512, lengths=None):
    """BSS-eval SDR in dB of the estimate s_hat against the clean s, in si_sdr's argument order, on the device: s_hat is allowed any linear
    filter of `flen` taps of s (a delay, a codec's or a resampler's colouring), where si_sdr allows a gain (storm_bss_sdr_rows;
    include/storm_hip.h has the definition - the reference has no such metric, and nothing here was compared with mir_eval).  s, s_hat: 1-D ->
    a float; [B, L] -> an fp64 tensor [B] on the device (lengths: per-row sample counts of a ragged batch).  numpy arrays are moved to the
    current HIP device; fp32 is what the kernels read."""
    from .. import ops
    (sr, er), one = _device_rows(s, s_hat)
    d = ops.bss_sdr_rows(sr, er, lengths=lengths, flen=flen)
    return float(d[0]) if one else d


def bss_eval(s, n, s_hat, flen=512, lengths=None):
    """(sdr, sir, sar) in dB of the estimate s_hat against the clean s and the noise n, in energy_ratios' argument roles, on the device:
    BSS-eval with two sources - s_hat is allowed one linear filter of `flen` taps of s and one of n, solved jointly; sir is what is left of n,
    sar what neither source explains (storm_bss_eval_rows; include/storm_hip.h has the definition - this is BSS-eval's split, not si_sir /
    si_sar, and nothing here was compared with mir_eval).  1-D arguments -> three floats; [B, L] -> three fp64 tensors [B] on the device
    (lengths: per-row sample counts of a ragged batch).  numpy arrays are moved to the current HIP device; fp32 is what the kernels read."""
    from .. import ops
    (sr, nr, er), one = _device_rows(s, n, s_hat)
    d = ops.bss_eval_rows(sr, nr, er, lengths=lengths, flen=flen)
    return tuple(float(d[0, k]) for k in range(3)) if one else (d[:, 0], d[:, 1], d[:, 2])


def lpc_measures(s, s_hat, fs=16000, lengths=None):
    """(seg_snr, llr, cd): segmental SNR in dB, log-likelihood ratio and LPC cepstral distance in dB of the estimate s_hat against the clean
    s, in si_sdr's argument order, on the device - the frame-based measures of the enhancement and dereverberation literature (30 ms frames
    at 3/4 overlap, LPC order 16, or 10 below 10 kHz; LLR and CD are means of the 95 % smallest frame values; storm_lpc_measures_rows;
    include/storm_hip.h has the definition - the reference has no such metric, and nothing here was compared with pysepm).  s, s_hat: 1-D ->
    three floats; [B, L] -> three fp64 tensors [B] on the device (lengths: per-row sample counts of a ragged batch).  A signal shorter than
    37.5 ms gives NaN, a silent one NaN for llr and cd.  numpy arrays are moved to the current HIP device; fp32 is what the kernels read."""
    from .. import ops
    (sr, er), one = _device_rows(s, s_hat)
    d = ops.lpc_measures_rows(sr, er, lengths=lengths, fs=fs)
    return tuple(float(d[0, k]) for k in range(3)) if one else (d[:, 0], d[:, 1], d[:, 2])


def seg_snr(s, s_hat, fs=16000, lengths=None):
    """the segmental SNR of lpc_measures alone"""
    return lpc_measures(s, s_hat, fs=fs, lengths=lengths)[0]


def llr(s, s_hat, fs=16000, lengths=None):
    """the log-likelihood ratio of lpc_measures alone"""
    return lpc_measures(s, s_hat, fs=fs, lengths=lengths)[1]


def cepstral_distance(s, s_hat, fs=16000, lengths=None):
    """the LPC cepstral distance of lpc_measures alone"""
    return lpc_measures(s, s_hat, fs=fs, lengths=lengths)[2]


def mean_std(data):
    """(mean, population std) of the values that are not NaN (util/other.py:53-57); host"""
    data = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data, dtype=np.float64)
    data = data[~np.isnan(data)]
    return np.mean(data), np.std(data)
