"""Model wrappers — drop-in for the inference surface of sgmse/model.py (ScoreModel :24,
DiscriminativeModel :320, StochasticRegenerationModel :392) without Lightning: ``enhance()``,
``get_pc_sampler()``, ``get_ode_sampler()``, ``forward`` / ``forward_score`` / ``forward_denoiser``,
``to_audio`` / ``_stft`` / ``_istft`` / ``_forward_transform`` / ``_backward_transform``,
``eval(no_ema=False)`` EMA swap and ``load_from_checkpoint``, and ``validation_loss`` - the reference's ``_step`` as
``validation_step`` logs it (valid_loss), forward only.  Training methods are out of scope.

New surface (not in the reference): ``enhance_batch`` (several utterances per call, equal to
per-utterance ``enhance`` calls; also on ``DiscriminativeModel``), ``enhance_long`` (recordings of any lengths as overlapping windows,
pooled into batches of one shape and cross-faded on the device), ``set_precision`` and the ``noise_fn`` / ``seed`` / ``row_seeds`` /
``peak`` knobs.
"""
import time
import warnings
from math import ceil

import torch
import torch.nn as nn

from . import sampling
from .backbones import BackboneRegistry
from .checkpoint import load_checkpoint_file
from .data_module import SpecsDataModule
from .sdes import SDERegistry

_PRECISIONS = {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16,
               "fp16": torch.float16, "float16": torch.float16, "half": torch.float16}


class _EMA:
    """Inference-side mirror of torch_ema.ExponentialMovingAverage (store / copy_to / restore /
    load_state_dict); the shadow parameters come from the checkpoint's ``ema`` entry (model.py:86-108)."""

    def __init__(self, parameters, decay):
        self.decay = decay
        self.shadow_params = None
        self.collected_params = None

    def load_state_dict(self, sd):
        self.decay = sd.get("decay", self.decay)
        self.shadow_params = [p.clone() for p in sd["shadow_params"]]

    def state_dict(self):
        return {"decay": self.decay, "shadow_params": self.shadow_params, "collected_params": self.collected_params}

    def _match(self, parameters):
        params = list(parameters)
        if self.shadow_params is None:
            return None, params
        if len(self.shadow_params) == len(params):
            return self.shadow_params, params
        trainable = [p for p in params if p.requires_grad]
        if len(self.shadow_params) == len(trainable):
            return self.shadow_params, trainable
        raise RuntimeError(f"EMA state has {len(self.shadow_params)} tensors, model has {len(params)} parameters")

    def store(self, parameters):
        self.collected_params = [p.detach().clone() for p in parameters]

    def copy_to(self, parameters):
        shadow, params = self._match(parameters)
        if shadow is None:
            return
        with torch.no_grad():
            for s, p in zip(shadow, params):
                p.copy_(s.to(p.device))

    def restore(self, parameters):
        if self.collected_params is None:
            return
        with torch.no_grad():
            for c, p in zip(self.collected_params, parameters):
                p.copy_(c)
        self.collected_params = None

    def to(self, *a, **k):
        pass


class _Base(nn.Module):
    """Shared inference plumbing of the three model classes."""

    def _init_common(self, sde, t_eps, ema_decay, data_module_cls, kwargs):
        sde_cls = SDERegistry.get_by_name(sde)
        self.sde = sde_cls(**kwargs)
        self.t_eps = t_eps
        self.ema_decay = ema_decay
        self._error_loading_ema = False
        dm_cls = data_module_cls if data_module_cls is not None else SpecsDataModule
        self.data_module = dm_cls(**kwargs, gpu=kwargs.get("gpus", 0) > 0)

    def _backbones(self):
        return [m for m in self.children() if hasattr(m, "set_compute_dtype")]

    def set_precision(self, precision):
        """'fp32': exact-fp32 MFMA path (reference numerics); 'bf16' / 'fp16': 16-bit MFMA operands / activations
        with fp32 accumulation, statistics, time embedding and SDE state."""
        dt = _PRECISIONS[precision] if isinstance(precision, str) else precision
        for m in self._backbones():
            m.set_compute_dtype(dt)
        return self

    # ---- EMA swap (model.py:97-111) ----------------------------------------------------------
    def on_load_checkpoint(self, checkpoint):
        ema = checkpoint.get("ema", None)
        if ema is not None:
            self.ema.load_state_dict(ema)
        else:
            self._error_loading_ema = True
            warnings.warn("EMA state_dict not found in checkpoint!")

    def train(self, mode=True, no_ema=False):
        res = super().train(mode)
        if not self._error_loading_ema:
            if mode is False and not no_ema:
                self.ema.store(self.parameters())
                self.ema.copy_to(self.parameters())
            else:
                if self.ema.collected_params is not None:
                    self.ema.restore(self.parameters())
            for m in self._backbones():
                m.invalidate()
        return res

    def eval(self, no_ema=False):
        return self.train(False, no_ema=no_ema)

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    @property
    def device(self):
        return next(self.parameters()).device

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", **overrides):
        """Lightning-free reader of a pytorch-lightning 1.8 ``.ckpt`` (enhancement.py:56-59): builds the
        model from ``hyper_parameters`` (+ overrides), loads ``state_dict`` and the ``ema`` shadow weights."""
        ckpt = load_checkpoint_file(checkpoint_path, map_location)
        hp = dict(ckpt.get("hyper_parameters", {}))
        hp.update(overrides)
        if not isinstance(hp.get("data_module_cls"), type):
            hp["data_module_cls"] = SpecsDataModule
        model = cls(**hp)
        missing, unexpected = model.load_state_dict(ckpt["state_dict"], strict=False)
        if missing:
            raise RuntimeError(f"checkpoint lacks parameters: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        model.on_load_checkpoint(ckpt)
        return model

    # ---- audio <-> spectrogram (model.py:258-271) ---------------------------------------------
    def to_audio(self, spec, length=None):
        return self._istft(self._backward_transform(spec), length)

    def _forward_transform(self, spec):
        return self.data_module.spec_fwd(spec)

    def _backward_transform(self, spec):
        return self.data_module.spec_back(spec)

    def _stft(self, sig):
        return self.data_module.stft(sig)

    def _istft(self, spec, length=None):
        return self.data_module.istft(spec, length)

    def _prepare(self, y, lengths=None, peak=None):
        """model.py:282-286 for a batch: y [B, L] host/device -> (Y [B,1,F,Tpad], peak [B], L).  lengths: the rows' own sample
        counts when utterances of different lengths share the batch (same padded frame count; rows zero filled).  peak: fp32 [B],
        the rows' normalisation factors from outside instead of their own peaks (the windows of a long recording: enhance_long).
        Rows that are contiguous are read where they lie (the overlapping windows of a recording are a strided view, not a copy)."""
        if y.dim() != 2:
            raise ValueError("expected a waveform batch [B, L]")
        yd = y.to(device=self.device, dtype=torch.float32)
        if yd.stride(1) != 1:
            yd = yd.contiguous()
        Y, peak = self.data_module.wav_to_spec(yd, pad_to=64, lengths=lengths, peak=peak)
        return Y, peak, y.size(1)

    # ---- audio at another rate than the model's (an extension: upstream asserts 16 kHz input, enhancement.py:69) -----------
    def _off_rate(self, sr):
        return sr is not None and int(sr) != self.data_module.sample_rate

    def _to_model_rate(self, y, sr, lengths=None):
        """y [B, L] at rate sr (lengths: the rows' own sample counts) -> (y resampled to the model rate on the device, the rows' counts there)"""
        dm = self.data_module
        if y.dim() != 2:
            raise ValueError("expected a waveform batch [B, L]")
        l16 = None
        if lengths is not None:
            lengths = [int(v) for v in lengths]
            l16 = [-(-v * dm.sample_rate // int(sr)) for v in lengths]
            tp = {dm.padded_frames(v) for v in l16}
            if len(tp) != 1 or max(lengths) != y.shape[1]:
                raise ValueError(f"a ragged batch must share one padded frame count at the model rate of {dm.sample_rate} Hz and be as wide as its longest "
                                 f"row: the rows' {lengths} samples at {int(sr)} Hz are {l16} samples there, padded frame counts {sorted(tp)}")
        return dm.resample(y.to(device=self.device, dtype=torch.float32), int(sr), dm.sample_rate, lengths=lengths), l16

    def _from_model_rate(self, x16, sr, l16, lengths, width):
        """the enhanced batch back at rate sr, every row trimmed to its input sample count (a round trip never comes back shorter:
        ceil(ceil(L u / d) d / u) >= L) and zero past it"""
        x = self.data_module.resample(x16, self.data_module.sample_rate, int(sr), lengths=l16)[:, :width].contiguous()
        if lengths is not None:
            for b, n in enumerate(lengths):
                x[b, int(n):] = 0
        return x

    # ---- validation loss: the reference's `_step` (model.py:138-154, 345-349, 560-595) ------------
    def _loss_draws(self, B, t, z, seed, row_seeds):
        """(t fp32 [B] on the host, noise keywords of the perturbation and the loss kernel).  t = t_eps + (T - t_eps) u (model.py:144)
        with u from a host generator seeded with `seed`, or - row_seeds - one generator per row, so that a row's t does not depend on
        its batch; with neither, torch's global generator gives u and the kernels' seed, as it gives the reference its draws."""
        if sum(v is not None for v in (z, seed, row_seeds)) > 1:
            raise ValueError("z, seed and row_seeds exclude one another")
        if row_seeds is not None:
            row_seeds = [int(v) for v in row_seeds]
            if len(row_seeds) != B:
                raise ValueError(f"row_seeds has {len(row_seeds)} keys for a batch of {B} rows")
        if t is None:
            if row_seeds is not None:
                u = torch.cat([torch.rand(1, generator=torch.Generator().manual_seed(v)) for v in row_seeds])
            else:
                u = torch.rand(B, generator=None if seed is None else torch.Generator().manual_seed(int(seed)))
            t = self.t_eps + (self.sde.T - self.t_eps) * u
        t = t.detach().to(device="cpu", dtype=torch.float32)
        if t.shape != (B,):
            raise ValueError(f"t has shape {tuple(t.shape)} for a batch of {B} rows")
        if z is not None:
            return t, {}
        if row_seeds is not None:
            return t, {"row_seeds": row_seeds}
        return t, {"seed": int(seed) if seed is not None else int(torch.randint(2 ** 62, (1,)))}

    def _score_network(self):
        """the network whose evaluations a grouped stream shares (ScoreModel: dnn; StoRM: score_net - its denoiser runs once per micro-batch)"""
        return getattr(self, "score_net", None) or self.dnn

    def enhance_stream(self, batches, grouped=True, return_nfe=False, seed=None, seeds=None, noise_fns=None, width=None, row_seeds=None,
                       peaks=None, **kwargs):
        """(ScoreModel and StochasticRegenerationModel.)  A stream of ragged micro-batches (BASELINE.json configs[4]) in lockstep: `batches` = [(y [b, L], lengths or None), ...] as
        storm_amd.distributed.bucket_by_frames forms them.  Every micro-batch runs enhance_batch - the same sampler, noise stream and
        (ODE) per-row step control as its own call - but the score evaluations of all micro-batches that are still running share ONE
        grouped network call per step (storm_amd.sampling.grouped, storm_ncsnpp_forward_group): the layers with a grouped kernel see
        the whole stream's pixel tiles in one launch instead of 2 - 3 rows at a time.  grouped=False: one micro-batch after the other.
        seed: micro-batch k draws from the Philox stream seed + k (seeds: one seed per micro-batch; noise_fns: one injected-noise callable per micro-batch instead).
        row_seeds: one list of per-row Philox keys per micro-batch (enhance_batch's row_seeds) instead of seed / seeds / noise_fns: every
        utterance draws what its own batch-1 run with that key draws, whatever micro-batch it is in.
        width: at most this many micro-batches in flight (None = all); a finished one is replaced by the next of the list (storm_amd.sampling.grouped.run_grouped).
        peaks: one entry per micro-batch, enhance_batch's peak (fp32 [b]) or None for the rows' own peaks.
        Returns the list of enhanced batches (and the mean evaluations per utterance with return_nfe); self.last_nfev_stream = the
        evaluations every micro-batch executed."""
        from .sampling.grouped import run_grouped
        if row_seeds is not None:
            if seed is not None or seeds is not None or noise_fns is not None:
                raise ValueError("row_seeds cannot be combined with seed, seeds or noise_fns")
            if len(row_seeds) != len(batches):
                raise ValueError(f"row_seeds has {len(row_seeds)} key lists for {len(batches)} micro-batches")
        if peaks is not None and len(peaks) != len(batches):
            raise ValueError(f"peaks has {len(peaks)} entries for {len(batches)} micro-batches")
        outs = [None] * len(batches)

        def one(k):
            yb, bl = batches[k]
            kw = dict(kwargs)
            if seeds is not None:
                kw["seed"] = seeds[k]
            elif seed is not None:
                kw["seed"] = seed + k
            if noise_fns is not None:
                kw["noise_fn"] = noise_fns[k]                  # (parity runs: the draws of micro-batch k)
            if row_seeds is not None:
                kw["row_seeds"] = row_seeds[k]
            if peaks is not None and peaks[k] is not None:
                kw["peak"] = peaks[k]
            return self.enhance_batch(yb, lengths=bl, return_nfe=True, **kw)
        fns = [(lambda k=k: one(k)) for k in range(len(batches))]
        res, batcher = run_grouped(self._score_network(), fns, device=self.device, width=width) if grouped else ([f() for f in fns], None)
        outs = [r[0] for r in res]
        self.last_nfev_stream = [r[1] for r in res]
        self.last_group_calls = None if batcher is None else (batcher.calls, batcher.rows)
        if return_nfe:
            rows = sum(b[0].shape[0] for b in batches)
            return outs, sum(r[1] * b[0].shape[0] for r, b in zip(res, batches)) / rows
        return outs

    _has_sampler = True                  # (DiscriminativeModel: False - one forward pass, no noise keys)

    def enhance_long(self, recordings, window=65408, overlap=8192, batch=16, ramp="hann", keys=None, seed=None, sr=None,
                     skip_silent=False, grouped=False, return_nfe=False, **sampler_kwargs):
        """Recordings of any lengths (a list of 1-D or [1, L] waveforms, host or device) -> the list of enhanced 1-D waveforms on the
        device, each with its input's sample count.  window / overlap (W, V; 16 kHz samples, 1 <= V <= W // 2, hop H = W - V): a
        recording of more than W samples at 16 kHz becomes n = ceil((L - V) / H) windows starting at k H - the [n, W] view of stride H of
        the recording zero filled to (n - 1) H + W (ops.window_plan).  The windows of ALL such recordings form one pool in (recording,
        window) order; every run of `batch` of them is ONE enhance_batch call of the shape [b, W] with peak = the RECORDING's peak per row
        (the reference normalises the whole input, model.py:282-286, and a training crop by its file's factor, data_module.py:92-114)
        and row_seeds = ops.window_key(recording key, k), so a window's result does not depend on what it is batched with; after the last
        batch ONE ops.crossfade_rows launch cross-fades the windows of all recordings (ramp: 'hann' or 'linear', ops.crossfade_ramp).
        A recording of at most W samples runs as it always did: storm_amd.distributed.bucket_by_frames + enhance_batch(lengths=...,
        row_seeds=[its key]).
        keys: one Philox key per recording; seed=s: recording i has the key s + i; neither: drawn from torch's generator
        (DiscriminativeModel ignores all three).  sr: the recordings' sample rate, one for all or one each - a recording is resampled to
        16 kHz as a whole, windowed there, stitched, resampled back and trimmed to its input sample count.
        skip_silent: windows whose every sample is zero are not sampled and read as zeros in the stitch.
        grouped (ScoreModel, StochasticRegenerationModel): the batches run in lockstep through enhance_stream - True: 8 in flight, an
        int: that many - instead of one after the other.  return_nfe: also the score evaluations of every sampled row, summed.
        sampler_kwargs: enhance_batch's (sampler_type, N, corrector, snr, ...)."""
        from . import ops
        from .distributed import bucket_by_frames
        dm = self.data_module
        W, V = int(window), int(overlap)
        if V < 1 or V > W // 2:
            raise ValueError(f"overlap={V} lies outside [1, window // 2] for window={W}")
        if W <= dm.n_fft // 2:
            raise ValueError(f"window={W} is too short for the STFT's reflect padding by n_fft // 2 = {dm.n_fft // 2} samples")
        if int(batch) < 1:
            raise ValueError(f"batch={batch}")
        for name in ("row_seeds", "lengths", "peak", "noise_fn"):
            if name in sampler_kwargs:
                raise ValueError(f"enhance_long forms {name} itself")
        if keys is not None and seed is not None:
            raise ValueError("keys and seed exclude each other")
        R = len(recordings)
        if keys is not None:
            keys = [int(v) for v in keys]
            if len(keys) != R:
                raise ValueError(f"keys has {len(keys)} entries for {R} recordings")
        elif seed is not None:
            keys = [int(seed) + i for i in range(R)]
        elif self._has_sampler:
            keys = [int(v) for v in torch.randint(2 ** 62, (R,))]
        else:
            keys = [0] * R
        rates = list(sr) if isinstance(sr, (list, tuple)) else [sr] * R
        if len(rates) != R:
            raise ValueError(f"sr has {len(rates)} entries for {R} recordings")
        H = W - V
        with torch.no_grad():
            x16, counts = [], []
            for i, w in enumerate(recordings):
                if w.dim() == 2 and w.shape[0] == 1:
                    w = w[0]
                if w.dim() != 1 or w.numel() < 1:
                    raise ValueError(f"recordings[{i}]: expected a waveform [L] or [1, L], got {tuple(w.shape)}")
                w = w.to(device=self.device, dtype=torch.float32)
                counts.append(w.numel())
                x16.append(dm.resample(w, int(rates[i]), dm.sample_rate) if self._off_rate(rates[i]) else w)
            long_ids = [i for i in range(R) if x16[i].numel() > W]
            short_ids = [i for i in range(R) if x16[i].numel() <= W]
            # ---- the pool: every window of every long recording, in (recording, window) order
            win_row, rec_windows, entries = [], [], []                # entries: (view [n, W], k, peak [1], key) of the windows that are sampled
            for i in long_ids:
                n, padded = ops.window_plan(x16[i].numel(), W, V)
                buf = torch.zeros(padded, dtype=torch.float32, device=self.device)
                buf[:x16[i].numel()] = x16[i]
                view = buf.as_strided((n, W), (H, 1))
                pk = ops.peak_abs(x16[i].reshape(1, -1))
                silent = (ops.peak_abs(view) <= ops.PEAK_FLOOR).tolist() if skip_silent else [False] * n
                rec_windows.append(n)
                for k in range(n):
                    win_row.append(-1 if silent[k] else len(entries))
                    if not silent[k]:
                        entries.append((view, k, pk, ops.window_key(keys[i], k)))
            jobs = []                                                 # (y [b, .], lengths, peak, row_seeds, where its rows go)
            for j0 in range(0, len(entries), int(batch)):
                run = entries[j0:j0 + int(batch)]
                one_view = all(e[0] is run[0][0] for e in run) and [e[1] for e in run] == list(range(run[0][1], run[0][1] + len(run)))
                rows = run[0][0][run[0][1]:run[0][1] + len(run)] if one_view else torch.stack([e[0][e[1]] for e in run])
                jobs.append((rows, None, torch.cat([e[2] for e in run]), [e[3] for e in run], ("pool", j0)))
            lens = [x16[i].numel() for i in short_ids]
            for bucket in bucket_by_frames(lens, int(batch), hop=dm.hop_length, n_fft=dm.n_fft):
                bl = [lens[k] for k in bucket]
                y = torch.zeros(len(bucket), max(bl), dtype=torch.float32, device=self.device)
                for row, k in enumerate(bucket):
                    y[row, :bl[row]] = x16[short_ids[k]]
                jobs.append((y, None if len(set(bl)) == 1 else bl, None, [keys[short_ids[k]] for k in bucket], ("short", [short_ids[k] for k in bucket])))
            # ---- run: one enhance_batch per job, one after the other or in lockstep
            if grouped and self._has_sampler and len(jobs) > 1:
                outs = self.enhance_stream([(j[0], j[1]) for j in jobs], width=8 if grouped is True else int(grouped), row_seeds=[j[3] for j in jobs],
                                           peaks=[j[2] for j in jobs], **sampler_kwargs)
                res = [(x, int(n_eval) * x.shape[0]) for x, n_eval in zip(outs, self.last_nfev_stream)]
            else:
                res = []
                for j in jobs:
                    self.last_nfev_rows = None
                    x, n_eval = self.enhance_batch(j[0], lengths=j[1], peak=j[2], row_seeds=j[3], return_nfe=True, **sampler_kwargs)
                    own = getattr(self, "last_nfev_rows", None)       # (ODE: every row's own count; otherwise all rows take n_eval)
                    res.append((x, sum(int(v) for v in own) if own else int(n_eval) * x.shape[0]))
            pool = torch.zeros((max(len(entries), 1), W), dtype=torch.float32, device=self.device)
            result, nfe = [None] * R, 0
            for (y, bl, _, _, (kind, where)), (x, evals) in zip(jobs, res):
                nfe += evals
                if kind == "pool":
                    pool[where:where + y.shape[0]] = x
                else:
                    for row, i in enumerate(where):
                        result[i] = x[row, :x16[i].numel()].clone()
            # ---- the stitch: all long recordings in one launch
            if long_ids:
                stitched = ops.crossfade_rows(pool, win_row, [x16[i].numel() for i in long_ids], rec_windows, W, V,
                                              ramp=ops.crossfade_ramp(V, ramp, self.device))
                for r, i in enumerate(long_ids):
                    result[i] = stitched[r, :x16[i].numel()]
            for i in range(R):
                if self._off_rate(rates[i]):
                    result[i] = dm.resample(result[i].contiguous(), dm.sample_rate, int(rates[i]))[:counts[i]]
        return (result, nfe) if return_nfe else result

    # the sampler keywords enhance_batch names, with its defaults (StochasticRegenerationModel: its own)
    _sampler_defaults = dict(sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=50, corrector_steps=1, snr=0.5)
    _ENSEMBLE_COMBINES = ("mean", "mag_mean", "mag_median", "medoid")

    def enhance_ensemble(self, y, draws=1, combine="mean", keys=None, seed=None, lengths=None, sr=None, batch=16, return_spread=False,
                         return_stft=False, return_nfe=False, **sampler_kwargs):
        """(ScoreModel and StochasticRegenerationModel.)  `draws` = K samples of the clean-speech posterior per utterance of y [B, L],
        combined on the device (ops.ensemble_combine; the definition is in include/storm_hip.h) -> the combined waveforms fp32 [B, L].
        The (utterance, draw) pairs form a pool in that order; every run of `batch` of them is ONE sampler run (K draws of one utterance
        fill the batch that a single utterance leaves empty), draw k of utterance b with the Philox key ops.draw_key(key_b, k), so a draw
        is what enhance_batch(y[b:b+1], row_seeds=[that key]) samples, whatever it is batched with.  The STFT, the peak (every draw of an
        utterance is normalised by that utterance's peak) and - StoRM - the denoiser run once per utterance; after the last run ONE
        combine launch forms, per bin of the LINEAR spectrogram,
          combine='mean': the mean of the draws;  'mag_mean' / 'mag_median': the mean's phase with the mean / median of the draws' magnitudes;
          'medoid': the draw closest to the mean over the whole utterance (its own spectrogram through the unchanged spec_to_wav: that
          utterance's result is its chosen draw's own result, bit for bit; chosen and gathered on the device).
        draws=1: no combine - enhance_batch(y, row_seeds=keys), bit for bit; the spread is zeros and the agreement +inf.
        keys: one Philox key per utterance; seed=s: utterance i has the key s + i; neither: drawn from torch's generator.  lengths, sr: as
        in enhance_batch.  sampler_kwargs: enhance_batch's (sampler_type, predictor, corrector, N, corrector_steps, snr, ...).
        Returns the waveforms and, in this order: return_spread - the per-bin spread fp32 [B, F, T] (the draws' standard deviation around
        their mean, padded frame count, zeros past an utterance's own frames) and the per-utterance agreement 10 log10(E / D) in dB, fp64
        [B] (E the energy of the mean, D the draws' mean squared distance from it), both over the frames that reach the utterance's samples,
        ceil((length + n_fft // 2) / hop) of them; return_stft - the combined linear spectrogram
        complex64 [B, F, T]; return_nfe - the score evaluations of all (utterance, draw) rows, summed, as enhance_long counts
        them (enhance_batch has one sampler run and returns that run's count; here there are several runs of different widths)."""
        from . import ops
        K = int(draws)
        if K < 1 or K > ops.ENSEMBLE_MAX_DRAWS:
            raise ValueError(f"draws={draws}: between 1 and {ops.ENSEMBLE_MAX_DRAWS}")
        if combine not in self._ENSEMBLE_COMBINES:
            raise ValueError(f"combine={combine!r}: one of {list(self._ENSEMBLE_COMBINES)}")
        if int(batch) < 1:
            raise ValueError(f"batch={batch}")
        for name in ("row_seeds", "peak", "noise_fn", "z"):
            if name in sampler_kwargs:
                raise ValueError(f"enhance_ensemble forms {name} itself")
        if keys is not None and seed is not None:
            raise ValueError("keys and seed exclude each other")
        if y.dim() != 2:
            raise ValueError("expected a waveform batch [B, L]")
        B = y.shape[0]
        if keys is not None:
            keys = [int(v) for v in keys]
            if len(keys) != B:
                raise ValueError(f"keys has {len(keys)} entries for {B} utterances")
        elif seed is not None:
            keys = [int(seed) + i for i in range(B)]
        else:
            keys = [int(v) for v in torch.randint(2 ** 62, (B,))]
        if self._off_rate(sr):
            y16, l16 = self._to_model_rate(y, sr, lengths)
            res = self.enhance_ensemble(y16, K, combine, keys=keys, lengths=l16, batch=batch, return_spread=return_spread, return_stft=return_stft,
                                        return_nfe=return_nfe, **sampler_kwargs)
            res = res if isinstance(res, tuple) else (res,)
            return self._ensemble_result((self._from_model_rate(res[0], sr, l16, lengths, y.shape[1]),) + res[1:])
        dm = self.data_module
        kw = {**self._sampler_defaults, **sampler_kwargs}
        named = [kw.pop(k) for k in ("sampler_type", "predictor", "corrector", "N", "corrector_steps", "snr")]
        with torch.no_grad():
            Y, peak, T_orig = self._prepare(y, lengths)
            F, Tp = Y.shape[2], Y.shape[3]
            # (StoRM: the denoiser's output, once per utterance; one draw: the denoiser runs inside the one sampler run, as in enhance_batch)
            cond = None if K == 1 else self._ensemble_condition(Y, int(batch), kw)
            pairs = [(b, k) for b in range(B) for k in range(K)]
            step = B if K == 1 else int(batch)                            # (one draw: the one sampler run of enhance_batch)
            pool, nfe = [], 0
            for j0 in range(0, len(pairs), step):
                run = pairs[j0:j0 + step]
                whole = [b for b, _ in run] == list(range(B))
                idx = None if whole else torch.tensor([b for b, _ in run], device=Y.device)
                sample, n_eval = self._sample_spec(Y if whole else Y.index_select(0, idx), *named, [ops.draw_key(keys[b], k) for b, k in run], dict(kw),
                                                   **({} if cond is None else {"Y_denoised": cond if whole else cond.index_select(0, idx)}))
                own = getattr(self, "last_nfev_rows", None)               # (ODE: every row's own count; otherwise all rows take n_eval)
                nfe += sum(int(v) for v in own) if own else int(n_eval) * len(run)
                pool.append(sample)
            pool = pool[0] if len(pool) == 1 else torch.cat(pool, dim=0)
            # the frames that reach an utterance's samples (frame t covers t hop +- n_fft // 2): the padding frames behind them are left out
            own_frames = [min(Tp, -(-(int(n) + dm.n_fft // 2) // dm.hop_length)) for n in (lengths if lengths is not None else [T_orig] * B)]
            if K == 1:
                x_hat = dm.spec_to_wav(pool, T_orig, peak, lengths=lengths)
                spread = torch.zeros((B, F, Tp), dtype=torch.float32, device=Y.device) if return_spread else None
                agree = torch.full((B,), float("inf"), dtype=torch.float64, device=Y.device)
                stft = dm.spec_back(pool[:, 0]) if return_stft else None
            else:
                table = torch.arange(B * K, dtype=torch.int32, device=Y.device).reshape(B, K)
                stft, spread, rows, best = ops.ensemble_combine(pool[:, 0], table, dm.spec_factor, dm.spec_abs_exponent,
                                                                mode="mean" if combine == "medoid" else combine, frames=own_frames,
                                                                spread=return_spread)
                agree = 10.0 * torch.log10(rows[:, 0] / rows[:, 1])
                if combine == "medoid":
                    chosen = pool.index_select(0, table.gather(1, best.long().unsqueeze(1)).reshape(-1).long())
                    x_hat = dm.spec_to_wav(chosen, T_orig, peak, lengths=lengths)
                    stft = dm.spec_back(chosen[:, 0]) if return_stft else None
                else:
                    x_hat = ops.istft(stft, int(T_orig), peak, n_fft=dm.n_fft, hop=dm.hop_length, spec_factor=1.0, spec_abs_exponent=1.0,
                                      window=dm.window_type, lengths=lengths)
        return self._ensemble_result((x_hat,) + ((spread, agree) if return_spread else ()) + ((stft,) if return_stft else ())
                                     + ((nfe,) if return_nfe else ()))

    @staticmethod
    def _ensemble_result(res):
        return res if len(res) > 1 else res[0]

    def _ensemble_condition(self, Y, batch, kw):
        """what every draw of an utterance shares besides Y (StochasticRegenerationModel: the denoiser's output); None: nothing"""
        return None

    @staticmethod
    def _slice_keys(kwargs, sl):
        """the sampler keywords of the batch slice `sl`: per-row keys (row_seeds) go with their rows"""
        if kwargs.get("row_seeds") is None:
            return kwargs
        return {**kwargs, "row_seeds": kwargs["row_seeds"][sl]}

    def _sampler_minibatched(self, make, y, minibatch):
        M = y.shape[0]

        def batched_sampling_fn():
            samples, ns = [], []
            for i in range(int(ceil(M / minibatch))):
                sample, n = make(slice(i * minibatch, (i + 1) * minibatch))()
                samples.append(sample)
                ns.append(n)
            return torch.cat(samples, dim=0), ns
        return batched_sampling_fn


class ScoreModel(_Base):
    def __init__(self, backbone: str = "ncsnpp", sde: str = "ouve", lr: float = 1e-4, ema_decay: float = 0.999,
                 t_eps: float = 3e-2, transform: str = "none", nolog: bool = False, num_eval_files: int = 50,
                 loss_type: str = "mse", data_module_cls=None, **kwargs):
        super().__init__()
        dnn_cls = BackboneRegistry.get_by_name(backbone)
        kwargs.update(input_channels=4)                                    # model.py:47
        self.dnn = dnn_cls(**kwargs)
        self._init_common(sde, t_eps, ema_decay, data_module_cls, kwargs)
        self.ema = _EMA(self.parameters(), decay=ema_decay)
        self.lr, self.loss_type, self.num_eval_files, self.nolog = lr, loss_type, num_eval_files, nolog
        self._set_score_sign()

    def _set_score_sign(self):
        if hasattr(self.dnn, "negate_output"):
            self.dnn.negate_output = True          # score = -dnn(...) (model.py:131-132) folded into the output head

    def _raw_dnn_output(self, x, t, y):
        return -self.forward(x, t, y)

    def forward(self, x, t, y, **kwargs):
        """score = -dnn(cat[x, y], t); x, y complex64 [B,1,F,T], t [B]."""
        return self.dnn.forward_parts([x[:, 0], y[:, 0]], t)

    def get_pc_sampler(self, predictor_name, corrector_name, y, N=None, minibatch=None, scale_factor=None, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, **kwargs}
        if minibatch is None:
            return sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y, **kwargs)
        return self._sampler_minibatched(
            lambda sl: sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, y=y[sl], **self._slice_keys(kwargs, sl)),
            y, minibatch)

    def get_ode_sampler(self, y, N=None, minibatch=1, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, **kwargs}
        if minibatch is None:
            return sampling.get_ode_sampler(sde, self, y=y, **kwargs)
        return self._sampler_minibatched(lambda sl: sampling.get_ode_sampler(sde, self, y=y[sl], **self._slice_keys(kwargs, sl)), y, minibatch)

    def enhance_batch(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=50,
                      corrector_steps=1, snr=0.5, return_nfe=False, lengths=None, row_seeds=None, sr=None, peak=None, **kwargs):
        """B equal-length utterances y [B, L] in one sampler run.  Every op on the path is per utterance, the Langevin
        corrector runs with per-row step sizes and the ODE sampler with one Runge-Kutta step controller per row (the
        reference solves one utterance per solve_ivp call), so with INJECTED noise (noise_fn) row b equals enhance(y[b:b+1])
        for every sampler / predictor / corrector.  The in-kernel Philox noise has two forms.  seed=: ONE stream for the call,
        the counter is the position in the batch - rows are independent draws, but a row's draws depend on where it sits.
        row_seeds=[s_0 ... s_{B-1}] (ints in [0, 2^63), instead of seed / noise_fn): row b has its own key and draws exactly
        what enhance(y[b:b+1], seed=s_b) draws, so row b equals that call wherever and with whatever it is batched - to fp32
        rounding, and bit for bit in every precision under storm_amd.set_batch_invariant().
        For sampler_type="ode" the returned nfe is the number of score evaluations executed (= the slowest row's count).
        lengths: ragged micro-batch - rows of different sample counts that share one padded frame count
        (storm_amd.distributed.bucket_by_frames); y is zero filled to the longest row and so is the result.
        sr: the sample rate of y (and of lengths) when it is not the model's 16 kHz - y is resampled to 16 kHz on the device, enhanced as
        a 16 kHz batch, resampled back and every row trimmed to its input sample count; the padded-frame rule of a ragged batch then
        holds for the 16 kHz lengths.
        peak: fp32 [B], the rows' normalisation factors instead of their own peaks (None: as the reference, every row's own peak)."""
        if self._off_rate(sr):
            y16, l16 = self._to_model_rate(y, sr, lengths)
            x16, nfe = self.enhance_batch(y16, sampler_type, predictor, corrector, N, corrector_steps, snr, return_nfe=True, lengths=l16,
                                          row_seeds=row_seeds, peak=peak, **kwargs)
            x_hat = self._from_model_rate(x16, sr, l16, lengths, y.shape[1])
            return (x_hat, nfe) if return_nfe else x_hat
        Y, peak, T_orig = self._prepare(y, lengths, peak)
        sample, nfe = self._sample_spec(Y, sampler_type, predictor, corrector, N, corrector_steps, snr, row_seeds, kwargs)
        x_hat = self.data_module.spec_to_wav(sample, T_orig, peak, lengths=lengths)
        return (x_hat, nfe) if return_nfe else x_hat

    def _sample_spec(self, Y, sampler_type, predictor, corrector, N, corrector_steps, snr, row_seeds, kwargs):
        """enhance_batch from the prepared spectrograms Y [B,1,F,Tpad] to the sampler's output: (sample, score evaluations).  kwargs: the
        caller's remaining sampler keywords (a dict this method may add to)."""
        if row_seeds is not None:
            kwargs["row_seeds"] = row_seeds
        if sampler_type == "pc":
            kwargs.setdefault("langevin_per_row", True)
            sampler = self.get_pc_sampler(predictor, corrector, Y, N=N, corrector_steps=corrector_steps, snr=snr,
                                          intermediate=False, **kwargs)
        elif sampler_type == "ode":
            kwargs.setdefault("per_row", True)       # one RK45 step controller per utterance (model.py:224: minibatch = 1)
            sampler = self.get_ode_sampler(Y, N=N, minibatch=None, **kwargs)
        else:
            raise ValueError("{} is not a valid sampler type!".format(sampler_type))
        sample, nfe = sampler()
        self.last_nfev_rows = getattr(sampler, "nfev_rows", None)     # ODE: the evaluations every row needed on its own
        return sample, nfe

    def validation_loss(self, x, y, t=None, z=None, seed=None, row_seeds=None, frames=None, reduce=True):
        """The reference's `_step` (model.py:138-154), the number it logs as valid_loss, on a spectrogram batch x (clean), y (noisy)
        complex64 [B,1,F,T]: draw t, perturb x towards y (one kernel), ONE score evaluation, the residual loss of `loss_type`
        (one kernel and a row sum).  t / z: injected (parity runs); otherwise t is drawn on the host and the noise in the kernels from
        seed= or row_seeds= (see _loss_draws; with row_seeds row b is its batch-1 call with seed = row_seeds[b]).  frames: the rows'
        valid frame counts - the padding frames of a ragged or padded batch stay out of the sums.  reduce=True: torch.mean of the
        rows as `_loss` takes it (model.py:113-122); reduce=False: the rows, fp32 [B]."""
        from . import ops
        if self.loss_type not in ops.LOSS_KINDS:
            raise NotImplementedError(f"loss_type {self.loss_type!r}: the score loss is 'mse' or 'mae' (model.py:113-122)")
        th, keys = self._loss_draws(x.shape[0], t, z, seed, row_seeds)
        with torch.no_grad():
            x, y = x.to(self.device), y.to(self.device)
            z = None if z is None else z.to(self.device)
            x_t, std = self.sde.marginal_prob_sample(x, th, y, z=z, **keys)
            score = self(x_t, th.to(self.device), y)
            rows = ops.dsm_loss_rows(score, std, z=z, kind=self.loss_type, frames=frames, **keys)
        return torch.mean(rows) if reduce else rows

    def enhance(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=50, corrector_steps=1,
                snr=0.5, timeit=False, scale_factor=None, return_stft=False, sr=None, **kwargs):
        """One-call enhancement of one utterance y [1, L] (model.py:273-310).  sr: y's sample rate when it is not 16 kHz (enhance_batch);
        return_stft=True returns the 16 kHz spectrograms."""
        start = time.time()
        if self._off_rate(sr):
            if return_stft:
                y, sr = self._to_model_rate(y, sr)[0], None
            else:
                kwargs["sr"] = sr
        if return_stft:
            Y, peak, T_orig = self._prepare(y)
            sampler = self.get_pc_sampler(predictor, corrector, Y, N=N, corrector_steps=corrector_steps, snr=snr, **kwargs)
            sample, nfe = sampler()
            return sample.squeeze(), Y.squeeze(), T_orig, float(peak[0])
        x_hat, nfe = self.enhance_batch(y, sampler_type, predictor, corrector, N, corrector_steps, snr,
                                        return_nfe=True, **kwargs)
        x_hat = x_hat.squeeze().cpu()
        end = time.time()
        if timeit:
            rtf = (end - start) / (len(x_hat) / (sr or 16000))
            return x_hat, nfe, rtf
        return x_hat


class DiscriminativeModel(ScoreModel):
    """Predictive denoiser (model.py:320-370): NCSN++ on the spectrogram, or a time-domain backbone (FORCE_STFT_OUT: ConvTasNet)
    between an iSTFT and an STFT."""

    def _set_score_sign(self):
        pass

    def forward(self, y):
        if getattr(self.dnn, "FORCE_STFT_OUT", False):        # a time-domain net (ConvTasNet): it is handed the waveform (model.py:323-324)
            y = self._istft(self._backward_transform(y.squeeze(1)))
        t = torch.ones(y.shape[0], device=y.device)
        return self.dnn(y, t)

    def validation_loss(self, x, y, frames=None, reduce=True):
        """The reference's `_step` / `_loss` (model.py:329-349): Xhat = self(y), then `loss_type` 'mse' / 'mae' / 'sisdr' against x
        (spectrogram batches complex64 [B,1,F,T]).  A time-domain backbone (FORCE_STFT_OUT) returns waveforms: x goes through
        istft(spec_back(x)) first, as upstream; 'sisdr' trims to the shorter length (si_sdr_torch), 'mse' / 'mae' on unequal
        lengths fail as upstream's subtraction does.  reduce=True: torch.mean over the rows; reduce=False: the rows, fp32 [B]."""
        from . import ops
        time_domain = bool(getattr(self.dnn, "FORCE_STFT_OUT", False))
        if self.loss_type not in ("mse", "mae", "sisdr"):
            raise NotImplementedError(f"loss_type {self.loss_type!r}: the predictive loss is 'mse', 'mae' or 'sisdr' (model.py:329-343)")
        with torch.no_grad():
            x, y = x.to(self.device), y.to(self.device)
            x_hat = self(y)
            if time_domain:
                if frames is not None:
                    raise ValueError("frames count spectrogram frames: a time-domain backbone's loss runs on waveforms")
                x = self._istft(self._backward_transform(x.squeeze(1)))
                x_hat = x_hat.reshape(x_hat.shape[0], -1)
            if self.loss_type == "sisdr":
                if not time_domain:
                    raise RuntimeError("loss_type 'sisdr' needs a time-domain backbone (si_sdr_torch takes 1-D signals, util/other.py:88-94)")
                rows = -ops.si_sdr(x.float(), x_hat.float(), eps=1e-10)
            else:
                if x.shape != x_hat.shape:
                    raise RuntimeError(f"The size of tensor a ({x.shape[-1]}) must match the size of tensor b ({x_hat.shape[-1]}) for "
                                       f"loss_type {self.loss_type!r}: target {tuple(x.shape)}, estimate {tuple(x_hat.shape)}")
                rows = ops.pair_loss_rows(x, x_hat, kind=self.loss_type, frames=frames)
        return torch.mean(rows) if reduce else rows

    _has_sampler = False                 # (enhance_long: no noise keys, no grouped sampler stream)

    def enhance_batch(self, y, lengths=None, peak=None, sr=None, return_nfe=False, **ignored_kwargs):
        """The batched form of `enhance`: y [B, L] -> fp32 [B, L] on the device, row b equal to enhance(y[b:b+1]).  lengths, peak and sr as
        in ScoreModel.enhance_batch; sampler keywords (row_seeds among them) are ignored, as `enhance` ignores them.  return_nfe: the one
        network evaluation."""
        if self._off_rate(sr):
            y16, l16 = self._to_model_rate(y, sr, lengths)
            x_hat = self._from_model_rate(self.enhance_batch(y16, lengths=l16, peak=peak), sr, l16, lengths, y.shape[1])
            return (x_hat, 1) if return_nfe else x_hat
        with torch.no_grad():
            Y, peak, T_orig = self._prepare(y, lengths, peak)
            X_hat = self(Y)
            if getattr(self.dnn, "FORCE_STFT_OUT", False):    # a time-domain net: its waveforms go back to spectrograms (model.py:362-363)
                X_hat = self._forward_transform(self._stft(X_hat.reshape(X_hat.shape[0], -1))).unsqueeze(1)
            x_hat = self.data_module.spec_to_wav(X_hat, T_orig, peak, lengths=lengths)
        return (x_hat, 1) if return_nfe else x_hat

    def enhance_ensemble(self, y, draws=1, combine="mean", lengths=None, sr=None, return_spread=False, return_stft=False, return_nfe=False,
                         **ignored_kwargs):
        """A predictive model draws no noise: every draw would be the same output, so draws > 1 is refused.  draws=1: enhance_batch."""
        if int(draws) != 1:
            raise ValueError(f"DiscriminativeModel.enhance_ensemble: draws={draws} - a predictive model has no noise to draw from, its one "
                             f"output is the only draw (draws=1)")
        if return_spread or return_stft:
            raise ValueError("DiscriminativeModel.enhance_ensemble: return_spread and return_stft belong to the sampling models")
        return self.enhance_batch(y, lengths=lengths, sr=sr, return_nfe=return_nfe)

    def enhance(self, y, sr=None, **ignored_kwargs):
        """sr: y's sample rate when it is not 16 kHz - resampled on the device before and after, as in ScoreModel.enhance_batch"""
        if self._off_rate(sr):
            y16, _ = self._to_model_rate(y, sr)
            x16 = self.enhance(y16).reshape(y16.shape[0], -1)
            return self._from_model_rate(x16, sr, None, None, y.shape[1]).squeeze()
        with torch.no_grad():
            Y, peak, T_orig = self._prepare(y)
            X_hat = self(Y)
            if getattr(self.dnn, "FORCE_STFT_OUT", False):    # ... and its waveform goes back to a spectrogram (model.py:362-363)
                X_hat = self._forward_transform(self._stft(X_hat)).unsqueeze(1)
            return self.data_module.spec_to_wav(X_hat, T_orig, peak).squeeze()


class StochasticRegenerationModel(_Base):
    """StoRM: predictive denoiser followed by the score-based sampler around its output (model.py:392-780)."""

    def __init__(self, backbone_denoiser: str = "ncsnpp", backbone_score: str = "ncsnpp", sde: str = "ouve",
                 lr: float = 1e-4, ema_decay: float = 0.999, t_eps: float = 3e-2, nolog: bool = False,
                 num_eval_files: int = 50, loss_type_denoiser: str = "none", loss_type_score: str = "mse",
                 data_module_cls=None, mode="regen-joint-training", condition="both", **kwargs):
        super().__init__()
        kwargs_denoiser = kwargs                                           # same dict on purpose (model.py:416)
        kwargs_denoiser.update(input_channels=2)
        kwargs_denoiser.update(discriminative=True)
        self.denoiser_net = BackboneRegistry.get_by_name(backbone_denoiser)(**kwargs) if backbone_denoiser != "none" else None
        kwargs.update(input_channels=(6 if condition == "both" else 4))
        kwargs_denoiser.update(discriminative=False)
        self.score_net = BackboneRegistry.get_by_name(backbone_score)(**kwargs) if backbone_score != "none" else None
        if self.score_net is not None and hasattr(self.score_net, "negate_output"):
            self.score_net.negate_output = True
        self._init_common(sde, t_eps, ema_decay, data_module_cls, kwargs)
        self.ema = _EMA(self.parameters(), decay=ema_decay)
        self.condition, self.mode = condition, mode
        self.lr, self.num_eval_files, self.nolog = lr, num_eval_files, nolog
        self.loss_type_denoiser, self.loss_type_score = loss_type_denoiser, loss_type_score
        self.weighting_denoiser_to_score = kwargs.get("weighting_denoiser_to_score", .5)       # model.py:438-441

    def forward_score(self, x, t, score_conditioning, sde_input, **kwargs):
        """-score_net(cat[x] + conditioning, t)  (model.py:548-554)"""
        return self.score_net.forward_parts([x[:, 0]] + [c[:, 0] for c in score_conditioning], t)

    def forward_denoiser(self, y, **kwargs):
        return self.denoiser_net(y)

    def get_pc_sampler(self, predictor_name, corrector_name, y, N=None, minibatch=None, scale_factor=None,
                       conditioning=None, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, **kwargs}
        if minibatch is None:
            return sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self.forward_score, y=y,
                                           conditioning=conditioning, **kwargs)
        return self._sampler_minibatched(
            lambda sl: sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self.forward_score,
                                               y=y[sl], conditioning=[c[sl] for c in conditioning], **self._slice_keys(kwargs, sl)),
            y, minibatch)

    def _score_conditioning(self, Y, Y_denoised):
        if self.condition == "noisy":
            return [Y]
        if self.condition == "post_denoiser":
            return [Y_denoised]
        if self.condition == "both":
            return [Y, Y_denoised]
        raise NotImplementedError(f"Don't know the conditioning you have wished for: {self.condition}")

    def validation_loss(self, x, y, t=None, z=None, seed=None, row_seeds=None, frames=None, reduce=True):
        """The reference's `_step` (model.py:560-595): denoiser forward, the forward SDE from x towards y_denoised, `condition`,
        forward_score, then (loss, loss_score, loss_denoiser) with loss = w loss_denoiser + (1 - w) loss_score, w =
        weighting_denoiser_to_score; loss_denoiser is None for loss_type_denoiser 'none'.  Arguments as ScoreModel.validation_loss.
        The reduction is the reference's `_reduce_op`, 0.5 * torch.sum over the WHOLE batch (model.py:449) - the sum of the rows,
        not their mean; reduce=False: the rows, fp32 [B]."""
        from . import ops
        if self.loss_type_score not in ops.LOSS_KINDS:                    # configure_losses (model.py:465-485)
            raise NotImplementedError(f"loss_type_score {self.loss_type_score!r}: 'mse' or 'mae'")
        if self.loss_type_denoiser not in ("mse", "mae", "none"):
            raise NotImplementedError(f"loss_type_denoiser {self.loss_type_denoiser!r}: 'mse', 'mae' or 'none'")
        th, keys = self._loss_draws(x.shape[0], t, z, seed, row_seeds)
        with torch.no_grad():
            x, y = x.to(self.device), y.to(self.device)
            z = None if z is None else z.to(self.device)
            y_denoised = self.forward_denoiser(y)
            x_t, std = self.sde.marginal_prob_sample(x, th, y_denoised, z=z, **keys)
            score = self.forward_score(x_t, th.to(self.device), self._score_conditioning(y, y_denoised), y_denoised)
            ls = ops.dsm_loss_rows(score, std, z=z, kind=self.loss_type_score, frames=frames, **keys)
            ld = None
            if self.loss_type_denoiser != "none":
                ld = ops.pair_loss_rows(y_denoised, x, kind=self.loss_type_denoiser, frames=frames)
            if reduce:
                ls, ld = torch.sum(ls), (None if ld is None else torch.sum(ld))
            w = self.weighting_denoiser_to_score
            loss = ls if ld is None else w * ld + (1 - w) * ls                                  # model.py:533-543
        return loss, ls, ld

    def enhance_batch(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="none", N=30,
                      corrector_steps=1, snr=0.5, denoiser_only=False, return_nfe=False, return_stft=False, lengths=None,
                      row_seeds=None, sr=None, peak=None, **kwargs):
        """row_seeds: one Philox key per row, as in ScoreModel.enhance_batch (row b draws what its batch-1 run with seed = s_b draws);
        sr: the sample rate of y and lengths when it is not 16 kHz, as there (return_stft=True returns the 16 kHz spectrograms);
        peak: fp32 [B], the rows' normalisation factors instead of their own peaks, as there"""
        if self._off_rate(sr):
            y16, l16 = self._to_model_rate(y, sr, lengths)
            out = self.enhance_batch(y16, sampler_type, predictor, corrector, N, corrector_steps, snr, denoiser_only=denoiser_only,
                                     return_nfe=True, return_stft=return_stft, lengths=l16, row_seeds=row_seeds, peak=peak, **kwargs)
            if return_stft:
                return out
            x_hat = self._from_model_rate(out[0], sr, l16, lengths, y.shape[1])
            return (x_hat, out[1]) if return_nfe else x_hat
        Y, peak, T_orig = self._prepare(y, lengths, peak)
        sample, nfe = self._sample_spec(Y, sampler_type, predictor, corrector, N, corrector_steps, snr, row_seeds, kwargs, denoiser_only=denoiser_only)
        if return_stft:                                     # (model.py:766-767; a batch gets every row's normalisation factor)
            norm = float(peak[0]) if sample.shape[0] == 1 else peak.detach().reshape(-1).cpu()
            return sample.squeeze(), Y.squeeze(), T_orig, norm
        x_hat = self.data_module.spec_to_wav(sample, T_orig, peak, lengths=lengths)
        return (x_hat, nfe) if return_nfe else x_hat

    _sampler_defaults = dict(sampler_type="pc", predictor="reverse_diffusion", corrector="none", N=30, corrector_steps=1, snr=0.5)

    def _sample_spec(self, Y, sampler_type, predictor, corrector, N, corrector_steps, snr, row_seeds, kwargs, denoiser_only=False, Y_denoised=None):
        """enhance_batch from the prepared spectrograms Y [B,1,F,Tpad] to the sampler's output: (sample, score evaluations).  kwargs: the
        caller's remaining sampler keywords (a dict this method may add to).  Y_denoised: the denoiser's output for these rows where the
        caller already has it (enhance_ensemble: once per utterance, replicated for its draws); None: forward_denoiser(Y)."""
        denoiser_only = bool(kwargs.pop("denoiser_only", denoiser_only))
        kwargs.setdefault("langevin_per_row", True)
        if row_seeds is not None:
            kwargs["row_seeds"] = row_seeds
        nfe = 0
        with torch.no_grad():
            if Y_denoised is None:
                Y_denoised = self.forward_denoiser(Y) if self.denoiser_net is not None else None
            if self.score_net is not None and not denoiser_only:
                score_conditioning = self._score_conditioning(Y, Y_denoised)
                if sampler_type != "pc":
                    raise NotImplementedError("StoRM supports the PC sampler only (the reference's ODE path drops the "
                                              "conditioning, model.py:671-691)")
                sampler = self.get_pc_sampler(predictor, corrector, Y_denoised, N=N, corrector_steps=corrector_steps,
                                              snr=snr, intermediate=False, conditioning=score_conditioning, **kwargs)
                sample, nfe = sampler()
            else:
                sample = Y_denoised
        return sample, nfe

    def _ensemble_condition(self, Y, batch, kw):
        if self.denoiser_net is None:
            return None
        if Y.shape[0] <= batch:
            return self.forward_denoiser(Y)                               # ONE evaluation for all utterances, none per draw
        return torch.cat([self.forward_denoiser(Y[j0:j0 + batch]) for j0 in range(0, Y.shape[0], batch)], dim=0)

    def enhance(self, y, sampler_type="pc", predictor="reverse_diffusion", corrector="none", N=30, corrector_steps=1,
                snr=0.5, timeit=False, scale_factor=None, return_stft=False, denoiser_only=False, sr=None, **kwargs):
        """model.py:720-780; return_stft=True returns (sample, Y, T_orig, norm_factor) like the reference.  sr: y's sample rate when it is
        not 16 kHz (enhance_batch)."""
        start = time.time()
        if self._off_rate(sr):
            kwargs["sr"] = sr
        out = self.enhance_batch(y, sampler_type, predictor, corrector, N, corrector_steps, snr,
                                 denoiser_only=denoiser_only, return_nfe=True, return_stft=return_stft, **kwargs)
        if return_stft:
            return out
        x_hat, nfe = out
        x_hat = x_hat.squeeze().cpu()
        end = time.time()
        if timeit:
            return x_hat, nfe, (end - start) / (len(x_hat) / (sr or 16000))
        return x_hat
