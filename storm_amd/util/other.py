"""Small utilities of sgmse/util/other.py that the hot path and the evaluation loop use:
pad_spec (:102-109), si_sdr / si_sdr_torch (:82-94), and the metrics of the calc_metrics step in batch form on the device:
energy_ratios (:21-44), lsd (:16-19), snr_dB (:96-100); mean_std (:53-57) on the host; stoi: STOI / ESTOI on the device under the
signature of pystoi.stoi, which the reference's evaluation calls."""
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


def mean_std(data):
    """(mean, population std) of the values that are not NaN (util/other.py:53-57); host"""
    data = np.asarray(data.detach().cpu() if isinstance(data, torch.Tensor) else data, dtype=np.float64)
    data = data[~np.isnan(data)]
    return np.mean(data), np.std(data)
