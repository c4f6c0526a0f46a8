#!/usr/bin/env python
"""Inference CLI — drop-in for the reference enhancement.py (same flags, enhancement.py:28-36):

    python enhancement.py --test_dir noisy/ --enhanced_dir out/ --ckpt model.ckpt --mode storm \
        [--corrector ald --corrector-steps 1 --snr 0.5 --N 50]

Additions: --precision {fp32,bf16}, --batch (equal-length utterances per sampler call), --seed / --utterance-seed, --sampler ode with
--ode-method {RK45,RK23,DOP853} / --ode-rtol / --ode-atol (what the reference hands to scipy.integrate.solve_ivp), --resample /
--output-sr (files of other rates than 16 kHz, resampled on the device), --window / --overlap / --ramp / --skip-silent (long recordings as
overlapping windows, pooled into full batches and cross-faded on the device: enhance_long), --draws / --combine / --spread-dir (several draws of the posterior
per file, combined on the device: enhance_ensemble) and multi-GPU sharding when launched with torchrun (one
process per GPU, files dealt by length; no collectives in the sampler).  WAV I/O uses scipy.io.wavfile (torchaudio is not required)."""
import glob
import hashlib
import os
from argparse import ArgumentParser

import numpy as np
import torch


def read_wav(path):
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.T
    else:
        x = x[None]
    return torch.from_numpy(np.ascontiguousarray(x)), sr


def write_wav(path, x, sr):
    from scipy.io import wavfile
    wavfile.write(path, sr, x.detach().cpu().numpy().astype(np.float32))


def utterance_key(seed, path):
    """--utterance-seed: a file's Philox key from the seed and its NAME only, (S + first 8 bytes of sha256(basename), little endian) mod 2^63"""
    return (seed + int.from_bytes(hashlib.sha256(os.path.basename(path).encode()).digest()[:8], "little")) % 2 ** 63


def main():
    p = ArgumentParser()
    p.add_argument("--test_dir", type=str, required=True, help="Directory containing your corrupted files to enhance.")
    p.add_argument("--enhanced_dir", type=str, required=True, help="Where to write your cleaned files.")
    p.add_argument("--ckpt", type=str, required=True)
    p.add_argument("--mode", required=True, choices=["score-only", "denoiser-only", "storm"])
    p.add_argument("--corrector", type=str, choices=("ald", "langevin", "none"), default="ald")
    p.add_argument("--corrector-steps", type=int, default=1)
    p.add_argument("--snr", type=float, default=0.5)
    p.add_argument("--N", type=int, default=50)
    p.add_argument("--sampler", choices=("pc", "ode"), default="pc", help="(extension) ode: the probability-flow sampler of ScoreModel.enhance(sampler_type='ode') - "
                   "BASELINE.json configs[4]; score-only mode, one step controller per file (the reference integrates one file per solve_ivp call)")
    p.add_argument("--ode-method", choices=("RK45", "RK23", "DOP853"), default=None, help="with --sampler ode: solve_ivp's explicit method (default RK45)")
    p.add_argument("--ode-rtol", type=float, default=None, help="with --sampler ode: relative tolerance of the step controller (default 1e-5)")
    p.add_argument("--ode-atol", type=float, default=None, help="with --sampler ode: absolute tolerance of the step controller (default 1e-5)")
    p.add_argument("--precision", choices=("fp32", "bf16", "fp16"), default="fp32")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--seed", type=int, default=None, help="Philox seed of the sampler noise (default: drawn from torch's RNG, as the reference)")
    p.add_argument("--utterance-seed", type=int, default=None, help="instead of --seed: every file draws from a Philox key of its own, formed from this seed and the file's "
                   "name, so its enhanced wav depends only on (seed, name, samples, precision) - not on the other files of --test_dir, nor on --batch, --group or "
                   "the number of GPUs.  fp32: equal to rounding; bit for bit (and in bf16 / fp16 at all) only together with --batch-invariant")
    p.add_argument("--batch-invariant", action="store_true", help="every utterance's result independent - bit for bit - of what it is batched with "
                   "(storm_amd.set_batch_invariant: launch decisions per image; costs the batch-aware kernel selections)")
    p.add_argument("--group", type=int, default=8, help="score-only and storm modes: this many micro-batches (frame buckets of different lengths) run their samplers in lockstep "
                   "and share the launches of the score network (ScoreModel.enhance_stream); 1 = one micro-batch after the other")
    p.add_argument("--resample", action="store_true", help="(extension) read files of any sample rate: each is resampled to the model's 16 kHz on the device when it is loaded "
                   "(SpecsDataModule.resample, scipy.signal.resample_poly's filter), batching and seeding work on the 16 kHz signals, and every enhanced file is "
                   "resampled back and written at its own rate with its own sample count.  Without it a file of another rate is refused, as upstream")
    p.add_argument("--output-sr", choices=("input", "model"), default="input", help="with --resample: write every file at its own rate (input) or at 16 kHz (model)")
    p.add_argument("--window", type=float, default=None, help="(extension) seconds: a file longer than this is enhanced as overlapping windows of this length, the windows of "
                   "all files pooled into batches of --batch rows of one shape and cross-faded back on the device (enhance_long; 4.088 s = 512 frames is the "
                   "benchmark's shape).  Absent: every file is one row, as upstream")
    p.add_argument("--overlap", type=float, default=0.512, help="with --window: seconds two neighbouring windows share (at most half a window)")
    p.add_argument("--ramp", choices=("hann", "linear"), default="hann", help="with --window: the cross-fade's weights over the overlap")
    p.add_argument("--skip-silent", action="store_true", help="with --window: windows whose every sample is zero are not sampled and come out as zeros")
    p.add_argument("--draws", type=int, default=1, help="(extension) this many samples of the posterior per file, drawn as full batches and combined on the device "
                   "(enhance_ensemble; draw k of a file uses the key ops.draw_key(file key, k)).  1: one draw per file, as upstream")
    p.add_argument("--combine", choices=("mean", "mag_mean", "mag_median", "medoid"), default="mean", help="with --draws: the mean of the draws' linear spectrograms, the mean's "
                   "phase with the mean / median of their magnitudes, or the draw closest to the mean")
    p.add_argument("--spread-dir", type=str, default=None, help="with --draws: write every file's per-bin spread (the draws' standard deviation around their mean, fp32 "
                   "[F, frames]) as <name>.npy into this directory")
    p.add_argument("--dist-world1",action="store_true", help="with ONE rank: form the RCCL process group anyway (dry run of the sharded path on one GPU)")
    args = p.parse_args()
    if args.seed is not None and args.utterance_seed is not None:
        raise SystemExit("--seed and --utterance-seed exclude each other")
    ode_kw = {k: v for k, v in (("method", args.ode_method), ("rtol", args.ode_rtol), ("atol", args.ode_atol)) if v is not None}
    if ode_kw and args.sampler != "ode":
        raise SystemExit("--ode-method / --ode-rtol / --ode-atol: only with --sampler ode")
    if args.draws < 1:
        raise SystemExit(f"--draws {args.draws}: at least 1")
    if args.draws > 1 and args.window is not None:
        raise SystemExit("--draws: not together with --window (a long recording's windows are drawn once)")
    if args.draws > 1 and args.mode == "denoiser-only":
        raise SystemExit("--draws: the denoiser-only mode draws no noise, its one output is the only draw")
    if args.draws == 1 and (args.spread_dir is not None or args.combine != "mean"):
        raise SystemExit("--combine / --spread-dir: only with --draws K, K > 1")
    if args.sampler == "ode" and args.mode != "score-only":
        raise SystemExit("--sampler ode: score-only mode (the reference's StoRM ODE path drops the conditioning, model.py:671-691)")

    from storm_amd import distributed as D
    from storm_amd.model import DiscriminativeModel, ScoreModel, StochasticRegenerationModel
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    rank, world, local = D.init(single_rank_group=args.dist_world1)
    if world > 1:
        D.pin_to_gpu_numa(local)                            # this rank's launch thread next to its GPU
    os.makedirs(args.enhanced_dir, exist_ok=True)
    model_cls = {"storm": StochasticRegenerationModel, "score-only": ScoreModel, "denoiser-only": DiscriminativeModel}[args.mode]
    model = model_cls.load_from_checkpoint(args.ckpt, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    model.eval(no_ema=False)
    model.cuda()
    model.set_precision(args.precision)
    if args.batch_invariant:
        import storm_amd
        storm_amd.set_batch_invariant(True)

    files = sorted(glob.glob(os.path.join(args.test_dir, "*.wav")))
    model_sr = model.data_module.sample_rate
    wavs, lengths, rates, samples = [], [], [], []
    for f in files:
        y, sr = read_wav(f)
        if not args.resample:
            assert sr == 16000, "You need to make sure sample_sr matches model_sr --> resample to 16kHz"
        rates.append(sr)
        samples.append(y.shape[1])                          # the file's own sample count: what its enhanced file has again
        wavs.append(y[:1])
        lengths.append(-(-y.shape[1] * model_sr // sr))     # ... and its count at the model's rate, which the files are dealt and bucketed by

    def write_enhanced(i, x):
        """file i's enhanced 16 kHz signal: back at the file's own rate and sample count (--output-sr input), or as it is"""
        x, sr = x.float().reshape(-1), model_sr
        if rates[i] != model_sr and args.output_sr == "input":
            x, sr = model.data_module.resample(x.to(model.device), model_sr, rates[i])[:samples[i]], rates[i]
        write_wav(os.path.join(args.enhanced_dir, os.path.basename(files[i])), x, sr)
    mine = D.shard_indices(len(files), rank, world, lengths)
    for i in mine:
        if rates[i] != model_sr:                            # --resample: this rank's files to the model's rate, on its device
            wavs[i] = model.data_module.resample(wavs[i].to(model.device), rates[i], model_sr).cpu()
    # micro-batches of utterances that share a padded frame count (different lengths welcome): equal to per-file runs
    def run(batch):
        ids = [mine[k] for k in batch]
        lens = [lengths[i] for i in ids]
        y = torch.zeros(len(ids), max(lens))
        for k, i in enumerate(ids):
            y[k, :lens[k]] = wavs[i][0]
        ragged = None if len(set(lens)) == 1 else lens
        if args.mode == "denoiser-only":
            outs = [model.enhance(wavs[i]) for i in ids]
        else:
            kw = {} if args.seed is None else dict(seed=args.seed + ids[0])     # distinct, reproducible draws per batch
            if args.utterance_seed is not None:
                kw = dict(row_seeds=[keys[i] for i in ids])                     # every file its own draws, whatever it is batched with
            x_hat = model.enhance_batch(y, lengths=ragged, **skw, **kw)
            outs = [x_hat[k, :lens[k]] for k in range(len(ids))]
        return ids, outs

    skw = dict(sampler_type="ode", N=args.N, **ode_kw) if args.sampler == "ode" else dict(corrector=args.corrector, N=args.N, corrector_steps=args.corrector_steps, snr=args.snr)
    keys = None if args.utterance_seed is None else [utterance_key(args.utterance_seed, f) for f in files]
    if args.window is not None:
        # long recordings: this rank's files in ONE enhance_long call - the windows of all files longer than --window pooled into full batches
        # of one shape, cross-faded on the device; shorter files as below.  A file's key: its utterance key, --seed + its index, or drawn.
        file_keys = [keys[i] for i in mine] if keys is not None else (None if args.seed is None else [args.seed + i for i in mine])
        outs = model.enhance_long([wavs[i][0] for i in mine], window=round(args.window * model_sr), overlap=round(args.overlap * model_sr),
                                  batch=args.batch, ramp=args.ramp, keys=file_keys, skip_silent=args.skip_silent,
                                  grouped=args.group if args.mode != "denoiser-only" and args.group > 1 else False, **skw) if mine else []
        for i, x in zip(mine, outs):
            write_enhanced(i, x)
        D.finish()
        return
    buckets = D.bucket_by_frames([lengths[i] for i in mine], args.batch)
    if args.draws > 1:
        # several draws per file: every micro-batch of files is ONE enhance_ensemble call - its (file, draw) pairs run as batches of --batch rows
        # and are combined in one launch.  A file's key: its utterance key, --seed + its index, or drawn.
        if args.spread_dir is not None:
            os.makedirs(args.spread_dir, exist_ok=True)
        dm = model.data_module
        for batch in buckets:
            ids = [mine[k] for k in batch]
            lens = [lengths[i] for i in ids]
            y = torch.zeros(len(ids), max(lens))
            for k, i in enumerate(ids):
                y[k, :lens[k]] = wavs[i][0]
            file_keys = [keys[i] for i in ids] if keys is not None else (None if args.seed is None else [args.seed + i for i in ids])
            res = model.enhance_ensemble(y, draws=args.draws, combine=args.combine, keys=file_keys, lengths=None if len(set(lens)) == 1 else lens,
                                         batch=args.batch, return_spread=args.spread_dir is not None, **skw)
            x_hat = res[0] if args.spread_dir is not None else res
            for k, i in enumerate(ids):
                write_enhanced(i, x_hat[k, :lens[k]])
                if args.spread_dir is not None:
                    frames = 1 + (lens[k] + 2 * (dm.n_fft // 2) - dm.n_fft) // dm.hop_length
                    np.save(os.path.join(args.spread_dir, os.path.splitext(os.path.basename(files[i]))[0] + ".npy"), res[1][k, :, :frames].cpu().numpy())
        buckets = []
    if args.mode in ("score-only", "storm") and args.group > 1 and len(buckets) > 1:
        # a ragged set of files: micro-batches of 2 - 3 rows each - their score evaluations share launches (storm_ncsnpp_forward_group)
        # (--group micro-batches in flight; one that finishes - an ODE micro-batch needs its own number of evaluations - is replaced by the next)
        chunk, metas = [], []
        for batch in buckets:
            ids = [mine[k] for k in batch]
            lens = [lengths[i] for i in ids]
            y = torch.zeros(len(ids), max(lens))
            for k, i in enumerate(ids):
                y[k, :lens[k]] = wavs[i][0]
            chunk.append((y, None if len(set(lens)) == 1 else lens))
            metas.append((ids, lens))
        outs = model.enhance_stream(chunk, width=args.group, seeds=None if args.seed is None else [args.seed + ids[0] for ids, _ in metas],     # (the draws of the one-by-one path)
                                    row_seeds=None if keys is None else [[keys[i] for i in ids] for ids, _ in metas], **skw)
        for (ids, lens), x_hat in zip(metas, outs):
            for k, i in enumerate(ids):
                write_enhanced(i, x_hat[k, :lens[k]])
        buckets = []
    for batch in buckets:
        ids, outs = run(batch)
        for i, x in zip(ids, outs):
            write_enhanced(i, x)
    D.finish()


if __name__ == "__main__":
    main()
