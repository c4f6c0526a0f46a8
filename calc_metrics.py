#!/usr/bin/env python
"""Score a directory of enhanced files against the clean and noisy ones - the reference's calc_metrics step on the device:

    python calc_metrics.py --clean_dir clean/ --noisy_dir noisy/ --enhanced_dir out/ [--batch 16] [--resample] [--stoi]
                           [--align [--max-lag SECONDS]] [--hp-filter [HZ]] [--sdr [TAPS]] [--bss [TAPS]] [--lpc]

Files are matched by basename (every *.wav of --enhanced_dir needs its clean and noisy namesake).  Each triple is trimmed to its
shortest member, the triples are bucketed by frame count and scored as ragged micro-batches (storm_amd.util.inference.score_batch:
SI-SDR / SI-SIR / SI-SAR, LSD and the input SNR, util/other.py:16-44, 96-100); PESQ and ESTOI are added on the host when the `pesq`
/ `pystoi` packages import.  Written into --enhanced_dir:

    _results.csv       Filename,Length,iSNR,si_sdr,si_sir,si_sar,lsd[,pesq,estoi] - one line per file, Length in samples at 16 kHz
                       (--stoi: ...,lsd[,pesq],stoi,estoi; --sdr: then sdr; --bss: then bss_sdr,bss_sir,bss_sar;
                       --lpc: then seg_snr,llr,cd; --align: lag, always last)
    _avg_results.txt   metric: mean ± std of each column (mean_std, NaNs dropped)

A file's line does not depend on --batch nor on the other files.  --resample: files of other rates are resampled to 16 kHz on the
device when they are loaded (SpecsDataModule.resample); without it such a file is refused, as in enhancement.py.  --stoi: STOI and ESTOI
of every file on the device, in the same micro-batches (storm_stoi_rows, defined in include/storm_hip.h and checked against a restatement
of the published algorithm, not against pystoi); host pystoi is then not called, and a pesq column still appears when `pesq` imports.
--hp-filter [HZ]: clean, noisy and enhanced file pass the reference's hp_filter first (Butterworth high-pass of order 10, 80 Hz unless given).
--align: enhanced files that are a few samples off (a codec, a network that pads its input) are moved onto their clean file before any
metric - the arg-max of the cross-correlation, searched within --max-lag seconds when given, zero-filled - and the column lag (last) says
by how many samples at 16 kHz the file was late.  Host PESQ / ESTOI columns, where they appear, still read the files as loaded.
--sdr [TAPS]: the column sdr, the BSS-eval SDR that allows the enhanced file a linear filter of TAPS taps of the clean one (512 unless
given, at most 512) where si_sdr allows a gain: a codec's or a resampler's colouring and a delay below TAPS samples are not booked as
distortion (storm_bss_sdr_rows, defined in include/storm_hip.h; not compared with mir_eval).  It is computed on what --hp-filter and
--align leave; a file that is exactly a filtered clean file prints inf.
--bss [TAPS]: the columns bss_sdr,bss_sir,bss_sar, BSS-eval with two sources: the enhanced file is allowed a filter of TAPS taps of the clean
file AND one of the noise (noisy - clean), solved jointly; bss_sir is the noise that is left, bss_sar what neither explains, where si_sir /
si_sar book any filter as interference and artefacts (storm_bss_eval_rows, defined in include/storm_hip.h; BSS-eval's split, not compared
with mir_eval).  bss_sdr is the column sdr of --sdr at the same TAPS.  Computed on what --hp-filter and --align leave.
--lpc: the columns seg_snr,llr,cd, the frame-based measures of the enhanced file against the clean one: segmental SNR (dB, frames clamped to
[-10, 35]), log-likelihood ratio (frames clamped to [0, 2]) and LPC cepstral distance (dB, frames clamped to [0, 10]) over 30 ms frames at
3/4 overlap with LPC order 16, the last two as means of the 95 % smallest frame values (storm_lpc_measures_rows, defined in
include/storm_hip.h and checked against a restatement of that text, not against pysepm).  Computed on what --hp-filter and --align leave; a
file shorter than 37.5 ms prints nan, and mean_std leaves a nan out of the averages."""
import glob
import os
from argparse import ArgumentParser

import numpy as np
import torch

from enhancement import read_wav

SR = 16000
COLUMNS = ("iSNR", "si_sdr", "si_sir", "si_sar", "lsd")
BSS_COLUMNS = ("bss_sdr", "bss_sir", "bss_sar")
LPC_COLUMNS = ("seg_snr", "llr", "cd")
KEYS = {"iSNR": "isnr", "si_sdr": "si_sdr", "si_sir": "si_sir", "si_sar": "si_sar", "lsd": "lsd"}


def main():
    p = ArgumentParser()
    p.add_argument("--clean_dir", type=str, required=True, help="Directory of the clean files.")
    p.add_argument("--noisy_dir", type=str, required=True, help="Directory of the noisy files.")
    p.add_argument("--enhanced_dir", type=str, required=True, help="Directory of the enhanced files; the results are written here.")
    p.add_argument("--batch", type=int, default=16, help="files per scoring micro-batch")
    p.add_argument("--resample", action="store_true", help="read files of any sample rate: each is resampled to 16 kHz on the device when it is loaded")
    p.add_argument("--stoi", action="store_true", help="append the columns stoi,estoi, computed on the device (pystoi is not needed and not called)")
    p.add_argument("--align", action="store_true", help="move every enhanced file onto its clean file before scoring; appends the column lag (samples)")
    p.add_argument("--max-lag", type=float, default=None, help="with --align: search delays of at most this many seconds (default: any)")
    p.add_argument("--hp-filter", type=float, nargs="?", const=80.0, default=None, metavar="HZ",
                   help="high-pass clean, noisy and enhanced at HZ (80 when no value is given) before scoring")
    p.add_argument("--sdr", type=int, nargs="?", const=512, default=None, metavar="TAPS",
                   help="append the column sdr: the BSS-eval SDR with a filter of TAPS taps (512 when no value is given), on the device")
    p.add_argument("--bss", type=int, nargs="?", const=512, default=None, metavar="TAPS",
                   help="append the columns bss_sdr,bss_sir,bss_sar: BSS-eval against clean and noise with filters of TAPS taps (512 when no value is given), on the device")
    p.add_argument("--lpc", action="store_true",
                   help="append the columns seg_snr,llr,cd: segmental SNR, log-likelihood ratio and LPC cepstral distance, on the device")
    args = p.parse_args()
    if args.sdr is not None and not 1 <= args.sdr <= 512:
        p.error("--sdr TAPS: 1 to 512")
    if args.bss is not None and not 1 <= args.bss <= 512:
        p.error("--bss TAPS: 1 to 512")
    if args.max_lag is not None and (not args.align or args.max_lag < 0):
        p.error("--max-lag SECONDS (>= 0) goes with --align")

    from storm_amd import distributed as D
    from storm_amd.data_module import SpecsDataModule
    from storm_amd.util.inference import _optional, score_batch
    from storm_amd.util.other import mean_std
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))

    def load(path):
        x, sr = read_wav(path)
        if not args.resample:
            assert sr == SR, "You need to make sure sample_sr matches model_sr --> resample to 16kHz"
        return SpecsDataModule.resample(x[0].to(dev), sr, SR)                  # first channel

    names = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(args.enhanced_dir, "*.wav")))]
    triples = []
    for name in names:
        x, y, e = (load(os.path.join(d, name)) for d in (args.clean_dir, args.noisy_dir, args.enhanced_dir))
        n = min(x.shape[0], y.shape[0], e.shape[0])
        triples.append((x[:n], y[:n], e[:n]))
    lengths = [t[0].shape[0] for t in triples]
    device_columns = COLUMNS + (("stoi", "estoi") if args.stoi else ()) + (("sdr",) if args.sdr is not None else ()) + (BSS_COLUMNS if args.bss is not None else ()) + (LPC_COLUMNS if args.lpc else ()) + (("lag",) if args.align else ())
    values = {c: [None] * len(names) for c in device_columns}
    for ids in D.bucket_by_frames(lengths, args.batch):
        lens = [lengths[i] for i in ids]
        rows = torch.zeros(3, len(ids), max(lens), device=dev)
        for k, i in enumerate(ids):
            for j in range(3):
                rows[j, k, :lens[k]] = triples[i][j]
        kw = dict(stoi=True, fs=SR) if args.stoi else {}
        if args.align:
            kw.update(align=True, max_lag=None if args.max_lag is None else int(round(args.max_lag * SR)))
        if args.hp_filter is not None:
            kw.update(hp=args.hp_filter, fs=SR)
        if args.sdr is not None:
            kw.update(sdr=True, sdr_taps=args.sdr)
        if args.bss is not None:
            kw.update(bss=True, bss_taps=args.bss)
        if args.lpc:
            kw.update(lpc=True, fs=SR)
        scores = {k: v.cpu() for k, v in score_batch(rows[0], rows[1], rows[2], lengths=lens, **kw).items()}
        for k, i in enumerate(ids):
            for c in device_columns:
                values[c][i] = float(scores[KEYS.get(c, c)][k])
    columns = list(COLUMNS)
    pesq, stoi = _optional("pesq", "pesq"), _optional("pystoi", "stoi")
    if args.stoi:
        if pesq is not None:
            columns += ["pesq"]
            values["pesq"] = [pesq(SR, x.cpu().numpy(), e.cpu().numpy(), "wb") for x, _, e in triples]
        columns += ["stoi", "estoi"]
    elif pesq is not None and stoi is not None:
        columns += ["pesq", "estoi"]
        values["pesq"] = [pesq(SR, x.cpu().numpy(), e.cpu().numpy(), "wb") for x, _, e in triples]
        values["estoi"] = [stoi(x.cpu().numpy(), e.cpu().numpy(), SR, extended=True) for x, _, e in triples]
    if args.sdr is not None:
        columns += ["sdr"]
    if args.bss is not None:
        columns += list(BSS_COLUMNS)
    if args.lpc:
        columns += list(LPC_COLUMNS)
    if args.align:
        columns += ["lag"]

    table = [[f"{values[c][i]:.0f}" if c == "lag" else f"{values[c][i]:.6f}" for c in columns] for i in range(len(names))]
    with open(os.path.join(args.enhanced_dir, "_results.csv"), "w", encoding="utf-8") as f:
        f.write(",".join(["Filename", "Length"] + columns) + "\n")
        for i, name in enumerate(names):
            f.write(",".join([name, str(lengths[i])] + table[i]) + "\n")
    with open(os.path.join(args.enhanced_dir, "_avg_results.txt"), "w", encoding="utf-8") as f:
        for j, c in enumerate(columns):                                        # (of the printed values: the averages follow from _results.csv alone)
            mean, std = mean_std(np.array([float(row[j]) for row in table]))
            f.write(f"{c}: {mean:.6f} ± {std:.6f}\n")


if __name__ == "__main__":
    main()
