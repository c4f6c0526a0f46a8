"""Evaluation loop — drop-in for sgmse/util/inference.py:20-72 (`evaluate_model`), built for the batched engine.

The reference enhances the first `num_eval_files` validation pairs ONE BY ONE (model.enhance) and averages PESQ,
SI-SDR and ESTOI on the host.  Here the pairs are grouped into micro-batches of utterances that share a padded frame
count (storm_amd.distributed.bucket_by_frames: different lengths welcome; every op of the path is per utterance, so a
batched run equals the per-file runs), enhanced with `model.enhance_batch(lengths=...)`, SI-SDR is one HIP launch per batch
(storm_si_sdr), and PESQ / ESTOI are used when the `pesq` / `pystoi` packages are importable (they are CPU reference
implementations of ITU-T P.862 / ESTOI; without them the two averages are NaN).

Pairs come from `model.data_module.valid_set.__getitem__(i, raw=True)` like the reference, or from `pairs=` (a sequence
of (clean [1, L], noisy [1, L]) tensors) since datasets are outside the hot path."""
import inspect
import math

import torch

from ..distributed import bucket_by_frames
from .other import lsd, si_sdr_batch

# Settings of the reference's validation runs (util/inference.py:11-13)
snr = 0.5
N = 50
corrector_steps = 1
MAX_VIS_SAMPLES = 10


def _optional(name, attr):
    try:
        return getattr(__import__(name), attr)
    except Exception:
        return None


METRIC_KEYS = ("si_sdr", "si_sir", "si_sar", "lsd", "isnr")
LPC_KEYS = ("seg_snr", "llr", "cd")          # score_batch(lpc=True)


def score_batch(clean, noisy, estimate, lengths=None, stoi=False, fs=16000, align=False, max_lag=None, hp=None, sdr=False, sdr_taps=512, bss=False,
                bss_taps=512, lpc=False):
    """The calc_metrics numbers of one micro-batch of device waveforms [B, L]: a dict of fp64 [B] tensors si_sdr / si_sir / si_sar
    (energy_ratios(estimate, clean, noisy - clean), util/other.py:35-44), lsd (estimate against clean, :16-19) and isnr (snr_dB(clean,
    noisy - clean), :96-100).  lengths: per-row sample counts of a ragged batch.  One energy launch pair, two STFTs and one LSD launch
    pair; every row's numbers are those of its own one-row call.  stoi=True adds the keys stoi and estoi: ops.stoi_rows(clean, estimate)
    of waveforms at `fs` Hz (resampled to 10 kHz on the device; include/storm_hip.h has the definition).
    hp=HZ: clean, noisy and estimate first pass the reference's hp_filter (order 10 at HZ for waveforms at `fs`; ops.sosfilt_rows, rounded
    to fp32 once).  align=True: the estimate is then moved onto the clean row by the arg-max of their cross-correlation
    (ops.xcorr_lag_rows, |lag| <= max_lag samples when given) and ZERO-FILLED, not rolled - rolled-in samples are unrelated audio that would
    enter every energy - before any metric; the result gains the key lag (int32 [B]): the samples by which the estimate was late.
    sdr=True adds the key sdr: the BSS-eval SDR of the estimate against clean with a filter of sdr_taps taps (ops.bss_sdr_rows), computed on
    what hp= and align= leave.  bss=True adds the keys bss_sdr, bss_sir, bss_sar: BSS-eval with two sources, target clean and noise noisy -
    clean, each allowed a filter of bss_taps taps, solved jointly (ops.bss_eval_rows; BSS-eval's split, not si_sir / si_sar), on the same
    rows.  lpc=True adds the keys seg_snr, llr, cd: the frame-based measures of the estimate against clean at `fs` Hz (ops.lpc_measures_rows;
    include/storm_hip.h has the definition), on the same rows.  Without these keywords nothing changes."""
    from .. import ops
    clean, noisy, estimate = clean.float(), noisy.float(), estimate.float()
    if hp is not None:
        sos = ops.butter_sos(10, float(hp) / fs * 2, "hp")
        clean, noisy, estimate = (ops.sosfilt_rows(v, sos, lengths=lengths, out_dtype=torch.float32) for v in (clean, noisy, estimate))
    lag = None
    if align:
        back, _ = ops.xcorr_lag_rows(estimate, clean, lengths=lengths, ref_lengths=lengths, max_lag=max_lag)
        estimate, lag = ops.shift_rows(estimate, back, lengths=lengths, wrap=False), -back
    r = ops.energy_ratios_rows(estimate, clean, noisy - clean, lengths=lengths)
    out = {"si_sdr": r[:, 0], "si_sir": r[:, 1], "si_sar": r[:, 2], "lsd": lsd(estimate, clean, lengths=lengths), "isnr": r[:, 3]}
    if stoi:
        d = ops.stoi_rows(clean, estimate, lengths=lengths, fs=fs)
        out["stoi"], out["estoi"] = d[:, 0], d[:, 1]
    if sdr:
        out["sdr"] = ops.bss_sdr_rows(clean, estimate, lengths=lengths, flen=sdr_taps)
    if bss:
        d = ops.bss_eval_rows(clean, noisy - clean, estimate, lengths=lengths, flen=bss_taps)
        out["bss_sdr"], out["bss_sir"], out["bss_sar"] = d[:, 0], d[:, 1], d[:, 2]
    if lpc:
        d = ops.lpc_measures_rows(clean, estimate, lengths=lengths, fs=fs)
        out["seg_snr"], out["llr"], out["cd"] = d[:, 0], d[:, 1], d[:, 2]
    if lag is not None:
        out["lag"] = lag
    return out


def evaluate_model(model, num_eval_files, spec=False, audio=False, discriminative=False, pairs=None, batch=16, noise_for=None,
                   metrics=False, estoi=None, lpc=False, draws=1, combine="mean", **enhance_kwargs):
    """Returns (pesq, si_sdr, estoi, [noisy, estimate, clean spectrograms] | None, [noisy, estimate, clean audio] | None),
    the reference's tuple.  `discriminative` is accepted for signature parity (the model class decides the path).
    noise_for(ids) -> noise_fn: injected sampler noise for the micro-batch of files `ids` (parity tests; production runs
    pass seed= and draw in-kernel).  metrics=True appends a sixth element: the means over the evaluated files of score_batch's
    numbers, {si_sdr, si_sir, si_sar, lsd, isnr} as floats, computed on the same micro-batches.
    estoi="device": the third element is the mean over the files of the device ESTOI (ops.stoi_rows at 16 kHz, one call per micro-batch),
    whether or not pystoi imports, and the sixth element gains the means stoi and estoi; None: pystoi on the host, NaN without it.
    lpc=True (with metrics=True): the sixth element gains the means seg_snr, llr and cd of score_batch(lpc=True) at 16 kHz.
    draws=K > 1, combine: every file's estimate is model.enhance_ensemble's (K draws per file combined on the device; its keys come from
    seed=s - file i has the key s + i - or keys=, one per file in the files' order, among the keywords, or are drawn); draws=1 changes nothing."""
    if int(draws) < 1:
        raise ValueError(f"draws={draws}: at least 1")
    if int(draws) > 1 and noise_for is not None:
        raise ValueError("draws > 1 draws its noise in the kernels from per-draw keys: noise_for does not apply")
    if estoi not in (None, "device"):
        raise ValueError(f"estoi={estoi!r}: None (pystoi on the host) or 'device'")
    model.eval()
    pesq, stoi = _optional("pesq", "pesq"), _optional("pystoi", "stoi")
    if pairs is None:
        vs = model.data_module.valid_set
        pairs = [vs.__getitem__(i, raw=True) for i in range(num_eval_files)]
    pairs = [(x if x.dim() == 2 else x.unsqueeze(0), y if y.dim() == 2 else y.unsqueeze(0)) for x, y in list(pairs)[:num_eval_files]]
    n = len(pairs)
    dev = next(model.parameters()).device
    est = [None] * n
    sdr = torch.zeros(n, dtype=torch.float64)
    scores = {k: torch.zeros(n, dtype=torch.float64) for k in METRIC_KEYS + (LPC_KEYS if lpc else ())} if metrics else None
    intel = torch.zeros(n, 2, dtype=torch.float64) if estoi == "device" else None
    hop = model.data_module.hop_length
    batched = hasattr(model, "enhance_batch") and not discriminative
    for ids in bucket_by_frames([p[1].shape[-1] for p in pairs], batch if batched else 1, hop=hop, n_fft=model.data_module.n_fft):
        lens = [pairs[i][1].shape[-1] for i in ids]
        width = max(lens)
        y = torch.zeros(len(ids), width)
        x = torch.zeros(len(ids), width)
        for k, i in enumerate(ids):                                         # first channel only (util/inference.py:44-47)
            y[k, :lens[k]] = pairs[i][1][0]
            x[k, :min(lens[k], pairs[i][0].shape[-1])] = pairs[i][0][0, :lens[k]]
        y, x = y.to(dev), x.to(dev)
        kw = dict(enhance_kwargs)
        if noise_for is not None:
            kw["noise_fn"] = noise_for(ids)
        if int(draws) > 1:
            if kw.get("seed") is not None:                                  # a file's key follows its index, not its place in a micro-batch
                first = int(kw.pop("seed"))
                kw["keys"] = [first + i for i in ids]
            elif kw.get("keys") is not None:                                # keys=: one per file, in the files' order
                kw["keys"] = [int(kw["keys"][i]) for i in ids]
            x_hat = model.enhance_ensemble(y, draws=int(draws), combine=combine, lengths=lens if len(set(lens)) > 1 else None, batch=batch, **kw)
        elif batched:
            x_hat = model.enhance_batch(y, lengths=lens if len(set(lens)) > 1 else None, **kw)
        else:
            x_hat = model.enhance(y[:1], **kw).reshape(1, -1)         # (N / snr / corrector_steps ... reach the model here too: util/inference.py:49)
        x_hat = x_hat.reshape(len(ids), -1).float().to(dev)
        if len(set(lens)) == 1:                                             # one launch for the whole micro-batch
            sdr[ids] = si_sdr_batch(x.contiguous(), x_hat.contiguous()).double().cpu()
        else:                                                               # ragged rows: every file over its own length
            for k, i in enumerate(ids):
                sdr[i] = float(si_sdr_batch(x[k:k + 1, :lens[k]], x_hat[k:k + 1, :lens[k]]))
        if metrics:
            w = min(width, x_hat.shape[1])
            for key, v in score_batch(x[:, :w], y[:, :w], x_hat[:, :w], lengths=[min(v, w) for v in lens], **(dict(lpc=True) if lpc else {})).items():
                scores[key][ids] = v.cpu()
        if intel is not None:
            from .. import ops
            w = min(width, x_hat.shape[1])
            intel[ids] = ops.stoi_rows(x[:, :w], x_hat[:, :w], lengths=[min(v, w) for v in lens], fs=16000).cpu()
        for k, i in enumerate(ids):
            est[i] = x_hat[k, :lens[k]].cpu()
    _pesq = _estoi = float("nan")
    if pesq is not None:
        _pesq = sum(pesq(16000, pairs[i][0][0].numpy(), est[i].numpy(), "wb") for i in range(n)) / n
    if intel is not None:
        _estoi = float(intel[:, 1].mean()) if n else math.nan
    elif stoi is not None:
        _estoi = sum(stoi(pairs[i][0][0].numpy(), est[i].numpy(), 16000, extended=True) for i in range(n)) / n
    specs = audios = None
    if spec:
        k = min(n, MAX_VIS_SAMPLES)
        sp = lambda w: model._stft(w.to(dev)).cpu()
        specs = [[sp(pairs[i][1][0]) for i in range(k)], [sp(est[i]) for i in range(k)], [sp(pairs[i][0][0]) for i in range(k)]]
    if audio:
        k = min(n, MAX_VIS_SAMPLES)
        audios = [[pairs[i][1][0] for i in range(k)], [est[i] for i in range(k)], [pairs[i][0][0] for i in range(k)]]
    out = (_pesq, float(sdr.mean()) if n else math.nan, _estoi, specs, audios)
    if metrics:
        out += ({k: float(v.mean()) if n else math.nan for k, v in scores.items()},)
        if intel is not None:
            out[5].update(stoi=float(intel[:, 0].mean()) if n else math.nan, estoi=float(intel[:, 1].mean()) if n else math.nan)
    return out


def validation_epoch(model, batches, seed=None, row_seeds=None, **loss_kwargs):
    """valid_loss over a validation set: `model.validation_loss` (the reference's `_step` as validation_step logs it, model.py:161-163,
    605-610) on every micro-batch of `batches` = [(x, y) or (x, y, frames), ...] - spectrogram batches complex64 [b,1,F,T], frames the
    rows' valid frame counts - and the mean of the batch losses weighted by their row counts, as Lightning reduces a value logged with
    on_epoch=True and batch_size.  seed: micro-batch k draws from seed + k (as enhance_stream); row_seeds: one key list per micro-batch.
    Returns a float, or for StochasticRegenerationModel the tuple (loss, loss_score, loss_denoiser) of floats (loss_denoiser None for
    loss_type_denoiser 'none')."""
    model.eval()
    batches = list(batches)
    if row_seeds is not None and len(row_seeds) != len(batches):
        raise ValueError(f"row_seeds has {len(row_seeds)} key lists for {len(batches)} micro-batches")
    draws = "seed" in inspect.signature(model.validation_loss).parameters          # (DiscriminativeModel draws nothing)
    totals, rows = None, 0
    for k, batch in enumerate(batches):
        kw = dict(loss_kwargs)
        if len(batch) == 3:
            kw["frames"] = batch[2]
        if draws and row_seeds is not None:
            kw["row_seeds"] = row_seeds[k]
        elif draws and seed is not None:
            kw["seed"] = seed + k
        out = model.validation_loss(batch[0], batch[1], **kw)
        vals = out if isinstance(out, tuple) else (out,)
        b = batch[0].shape[0]
        vals = [None if v is None else float(v) * b for v in vals]
        totals = vals if totals is None else [None if v is None else s + v for s, v in zip(totals, vals)]
        rows += b
    if totals is None:
        return math.nan
    means = tuple(None if s is None else s / rows for s in totals)
    return means if len(means) > 1 else means[0]
