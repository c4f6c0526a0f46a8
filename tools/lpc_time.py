"""Time the frame-based measures (storm_lpc_measures_rows: one workgroup per 8 frames for the lags, one lane per frame for Levinson-Durbin,
quadratic forms and cepstra, one workgroup per row for the mean and the two trimmed means) on the device at the bench batch of 16 x 4 s and at 16 x 60 s, fp32
waveforms at 16 kHz.  Beside each, in the same run and on the same rows:
  (a) the HBM floor: the bytes of the two inputs, 2 B L 4, over the measured rate of a device-to-device copy of as many bytes;
  (b) storm_energy_ratios_rows (one streaming pass over three rows) and storm_stoi_rows (at 10 kHz, as the library defines it: the rows are
      taken as 10 kHz samples, FFTs included) - the two existing scoring kernels that are the yardsticks;
  (c) the three kernels separately, from a kernel trace of its own: run
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/lpc_time.py --trace-loop
      first and hand DIR to --kernel-trace (a profiled run is never compared with an unprofiled one: (c) stands beside the call time, not in it).
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up (as tools/bss_eval_time.py).

    python tools/lpc_time.py [--kernel-trace DIR] [--out profiles/r23_lpc.txt]
"""
import argparse
import csv
import glob
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

FS, SHAPES, TRACE_CALLS = 16000, ((16, 64000), (16, 960000)), 8


def inputs(B, Lw, dev):
    """seeded rows: an AR(2)-coloured clean signal under a slow envelope, white noise at -10 dB, an estimate that keeps a tenth of the noise"""
    import scipy.signal as ss
    rng = np.random.default_rng(23)
    s = ss.lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal((B, Lw)), axis=-1)
    s = 0.1 * s / s.std() * (0.6 + 0.4 * np.sin(2.0 * np.pi * np.arange(Lw) / (0.37 * FS)))
    n = 0.0316 * rng.standard_normal((B, Lw))
    return tuple(torch.from_numpy(v.astype(np.float32)).to(dev) for v in (s, n, s + 0.1 * n))


def caller(s, e):
    B, Lw = s.shape
    lib, st = L.lib(), L.stream()
    win = ops.lpc_window(FS, s.device)
    out = torch.empty(B, 3, dtype=torch.float64, device=s.device)
    ws = torch.empty(lib.storm_lpc_measures_scratch_bytes(B, Lw, FS) // 8, dtype=torch.float64, device=s.device)

    def call():
        L.check(lib.storm_lpc_measures_rows(L.ptr(s), L.ptr(e), L.ptr(win), L.ptr(out), None, L.ptr(ws), 8 * ws.numel(), B, Lw, Lw, Lw, None, FS, st),
                "storm_lpc_measures_rows")
    return call, out


def trace_loop(dev):
    """--trace-loop: TRACE_CALLS calls of every shape in the order of main(), nothing else of the library on the stream"""
    for B, Lw in SHAPES:
        s, _, e = inputs(B, Lw, dev)
        call, _ = caller(s, e)
        for _ in range(TRACE_CALLS):
            call()
        torch.cuda.synchronize()


def kernel_times(d):
    """{shape index: (frames us, model us, rows us)}: medians over the dispatches of a --trace-loop run, in start order"""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    with open(files[0]) as f:
        rd = csv.DictReader(f)
        col = lambda part: next(c for c in rd.fieldnames if part in c.lower())  # noqa: E731
        cs, ce, cn = col("start"), col("end"), col("kernel_name")
        for r in rd:
            if "lpc_" in r[cn]:
                rows.append((int(r[cs]), int(r[ce]) - int(r[cs]), r[cn]))
    rows.sort()
    kinds = [[dur for _, dur, name in rows if k in name] for k in ("lpc_frames_kernel", "lpc_model_kernel", "lpc_rows_kernel")]
    if any(len(k) != len(SHAPES) * TRACE_CALLS for k in kinds):
        return None
    return {i: tuple(statistics.median(k[i * TRACE_CALLS + 2:(i + 1) * TRACE_CALLS]) / 1e3 for k in kinds) for i in range(len(SHAPES))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--trace-loop", action="store_true", help="only call every shape a few times (the program to run under rocprofv3)")
    p.add_argument("--kernel-trace", default=None, metavar="DIR", help="the output directory of a rocprofv3 --kernel-trace run of --trace-loop")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_loop:
        trace_loop(dev)
        return
    kt = kernel_times(args.kernel_trace) if args.kernel_trace else None
    lib, st = L.lib(), L.stream()
    W, H, P = ops.lpc_shape(FS)
    lines = [f"frame-based measures (segmental SNR, LLR, LPC cepstral distance) on the device, fp32 waveforms at {FS} Hz, {torch.cuda.get_device_name(0)}",
             f"all figures measured on that device: median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, "
             "after 5 warm-up calls",
             f"W = {W}, H = {H}, P = {P}; frames kernel: a workgroup of four waves per {ops.LPC_TILE} frames, strip and window staged in LDS, "
             f"{2 * (P + 1)} lags of {W} terms per frame in fp64; model kernel: one lane per frame, both recursions in registers; rows kernel: a workgroup "
             "per row, 63 counting passes for the two trimmed means", ""]
    for si, (B, Lw) in enumerate(SHAPES):
        s, n, e = inputs(B, Lw, dev)
        in_bytes = 2 * B * Lw * 4
        call, out = caller(s, e)
        t = per_launch(call, args.reps)
        M = (Lw - W) // H
        assert torch.equal(out, ops.lpc_measures_rows(s, e, fs=FS))
        cp = copy_time(in_bytes, dev, args.reps)
        floor_us = 1e3 * cp[0] / 2                                             # (the copy reads and writes in_bytes: a read-only pass moves half)
        o = out[0].tolist()
        lines.append(f"B = {B} x {Lw} samples ({B * Lw / FS:.0f} s of audio), {M} frames per row")
        lines.append(row(f"storm_lpc_measures_rows: 3 launches, {B * -(-M // ops.LPC_TILE)} + {B * -(-M // 64)} + {B} workgroups, {2 * 17 * W * M * B:.3e} fp64 FMAs of lags, "
                         f"row 0: seg_snr {o[0]:.3f} dB llr {o[1]:.4f} cd {o[2]:.3f} dB", t, in_bytes))
        lines.append(row(f"(a) device-to-device copy of {in_bytes / 1e6:.2f} MB (read + written); HBM floor of the call = 2 B L 4 = {in_bytes / 1e6:.2f} MB "
                         f"read once at that rate: {floor_us:.1f} us (inputs of this size fit the 256 MiB Infinity Cache: the copy can run above the HBM rate)", cp, 2 * in_bytes))
        eo = torch.empty(B, 4, dtype=torch.float64, device=dev)
        ews = torch.empty(lib.storm_energy_ratios_scratch_bytes(B, Lw), dtype=torch.uint8, device=dev)

        def energy():
            L.check(lib.storm_energy_ratios_rows(L.ptr(e), L.ptr(s), L.ptr(n), L.ptr(eo), L.ptr(ews), ews.numel(), B, Lw, Lw, Lw, Lw, None, st),
                    "storm_energy_ratios_rows")
        so = torch.empty(B, 2, dtype=torch.float64, device=dev)
        sws = torch.empty(lib.storm_stoi_scratch_bytes(B, Lw) // 8 + 1, dtype=torch.float64, device=dev)

        def stoi():
            L.check(lib.storm_stoi_rows(L.ptr(s), L.ptr(e), L.ptr(so), L.ptr(sws), 8 * sws.numel(), B, Lw, Lw, Lw, None, st), "storm_stoi_rows")
        te, ts = per_launch(energy, args.reps), per_launch(stoi, args.reps)
        lines.append(row(f"(b) storm_energy_ratios_rows on the same rows (three rows read once, {12 * B * Lw / 1e6:.2f} MB)", te, 12 * B * Lw))
        lines.append(row("(b) storm_stoi_rows on the same rows taken as 10 kHz samples (5 launches, one 512-point FFT per spectrogram frame)", ts, in_bytes))
        lines.append(f"    lpc / floor {1e3 * t[0] / floor_us:.1f} x; lpc / energy_ratios {t[0] / te[0]:.2f} x; lpc / stoi {t[0] / ts[0]:.2f} x")
        if kt is not None:
            f, m, r = kt[si]
            lines.append(f"    (c) kernel trace (a run of its own, medians of {TRACE_CALLS - 2} dispatches): frames kernel {f:.1f} us, model kernel {m:.1f} us, "
                         f"rows kernel {r:.1f} us")
        else:
            lines.append("    (c) kernel trace: not taken")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
