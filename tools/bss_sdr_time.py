"""Time the BSS-eval SDR (storm_bss_sdr_rows: lag correlations per piece, then a Levinson-Durbin solve per row) on the device at one 10-s row
(B = 1 x 160 000 samples at 16 kHz) and at the bench batch of 16 x 4 s (B = 16 x 64 000), for filters of 512 and of 64 taps.  Beside each:
  (a) a device-to-device copy of the input bytes;
  (b) the correlations' FMA count 2 F L per row divided by the device's fp64 FMA rate - measured by tools/ubench/fma64_rate (built: hipcc
      --offload-arch=gfx950 -O3 tools/ubench/fma64_rate.hip -o tools/ubench/fma64_rate), or given with --fma-rate GFMA/s;
  (c) the restatement on the host for the same rows (np.cumsum correlations of tests/bss_cases.py, scipy.linalg.solve_toeplitz), device <->
      host transfers included: the alternative the kernels remove;
  (d) the two kernels separately, from a kernel trace of its own: run
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bss_sdr_time.py --trace-loop
      first and hand DIR to --kernel-trace (a profiled run is never compared with an unprofiled one: (d) stands beside the call time, not in it).
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up (as tools/time_metrics.py).

    python tools/bss_sdr_time.py [--kernel-trace DIR] [--out profiles/r18_bss_sdr.txt]
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from tools.align_time import fma_rate  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

FS = 16000
SHAPES = ((1, 160000), (16, 64000))     # one 10-s file; the bench batch of 16 x 4 s
FLENS = (512, 64)
TRACE_CALLS = 20                        # calls per configuration of --trace-loop


def inputs(B, Lw, dev):
    """seeded rows: AR(2)-coloured noise, and that row delayed by 37 samples plus noise at -20 dB"""
    import scipy.signal as ss
    rng = np.random.default_rng(18)
    s = ss.lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal((B, Lw)), axis=-1)
    s = (0.1 * s / s.std()).astype(np.float32)
    e = np.roll(s, 37, axis=1) + 0.01 * rng.standard_normal((B, Lw)).astype(np.float32)
    return torch.from_numpy(s).to(dev), torch.from_numpy(e.astype(np.float32)).to(dev)


def caller(s, e, flen):
    B, Lw = s.shape
    lib, st = L.lib(), L.stream()
    out = torch.empty(B, dtype=torch.float64, device=s.device)
    ws = torch.empty(lib.storm_bss_sdr_scratch_bytes(B, Lw, flen) // 8, dtype=torch.float64, device=s.device)

    def call():
        L.check(lib.storm_bss_sdr_rows(L.ptr(s), L.ptr(e), L.ptr(out), None, None, L.ptr(ws), 8 * ws.numel(), B, Lw, Lw, Lw, None, flen, st),
                "storm_bss_sdr_rows")
    return call, out


def host_restatement(s, e, flen, reps):
    """(median, min, max) ms of: rows to the host, the restatement's correlations and scipy's Toeplitz solve per row, the numbers back"""
    import scipy.linalg as sl

    from tests import bss_cases as BC
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sh, eh = s.cpu().numpy(), e.cpu().numpy()
        vals = []
        for k in range(sh.shape[0]):
            parts = BC.correlations(sh[k], eh[k], flen)
            vals.append(BC.sdr_of(parts, sl.solve_toeplitz(parts[:flen], parts[flen:2 * flen])))
        back = torch.tensor(vals, dtype=torch.float64).to(s.device)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return (statistics.median(ms), min(ms), max(ms)), back


def trace_loop(dev):
    """--trace-loop: TRACE_CALLS calls of every configuration in the order of main(), nothing else of the library on the stream"""
    for B, Lw in SHAPES:
        s, e = inputs(B, Lw, dev)
        for flen in FLENS:
            call, _ = caller(s, e, flen)
            for _ in range(TRACE_CALLS):
                call()
            torch.cuda.synchronize()


def kernel_times(d):
    """{(shape index, flen index): (corr us, solve us)}: medians over the dispatches of a --trace-loop run, taken in start order"""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    with open(files[0]) as f:
        rd = csv.DictReader(f)
        col = lambda part: next(c for c in rd.fieldnames if part in c.lower())  # noqa: E731
        cs, ce, cn = col("start"), col("end"), col("kernel_name")
        for r in rd:
            if "bss_" in r[cn]:
                rows.append((int(r[cs]), int(r[ce]) - int(r[cs]), r[cn]))
    rows.sort()
    corr = [dur for _, dur, n in rows if "bss_corr_kernel" in n]
    solve = [dur for _, dur, n in rows if "bss_solve_kernel" in n]
    n = len(SHAPES) * len(FLENS)
    if len(corr) != n * TRACE_CALLS or len(solve) != n * TRACE_CALLS:
        return None
    out = {}
    for i in range(n):
        sl_ = slice(i * TRACE_CALLS + 2, (i + 1) * TRACE_CALLS)                 # (the first two calls of a configuration: warm-up)
        out[divmod(i, len(FLENS))] = (statistics.median(corr[sl_]) / 1e3, statistics.median(solve[sl_]) / 1e3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--fma-rate", type=float, default=None, help="the device's fp64 FMA rate in GFMA/s (default: run tools/ubench/fma64_rate)")
    p.add_argument("--trace-loop", action="store_true", help="only call every configuration a few times (the program to run under rocprofv3)")
    p.add_argument("--kernel-trace", default=None, metavar="DIR", help="the output directory of a rocprofv3 --kernel-trace run of --trace-loop")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_loop:
        trace_loop(dev)
        return
    rate, how = fma_rate(args.fma_rate)
    kt = kernel_times(args.kernel_trace) if args.kernel_trace else None
    lines = [f"BSS-eval SDR with a filter of F taps on the device, fp32 waveforms at {FS} Hz, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls",
             f"correlations: a workgroup per (row, piece of {ops.BSS_PIECE} samples), 8 / 4 / 2 lags of both banks per thread by the launch's chain count; "
             "solve: one wave per row, 8 entries of a and C per lane in registers, xor-butterfly reductions",
             f"fp64 FMA rate of the device: {'unmeasured' if rate is None else f'{rate / 1e9:.1f} GFMA/s'} ({how})", ""]
    for si, (B, Lw) in enumerate(SHAPES):
        s, e = inputs(B, Lw, dev)
        in_bytes = 8 * B * Lw
        cp = copy_time(in_bytes, dev, args.reps)
        lines.append(f"B = {B} x {Lw} samples ({B * Lw / FS:.0f} s of audio)")
        lines.append(row(f"(a) device-to-device copy of the two inputs, {in_bytes / 1e6:.2f} MB (read + written)", cp, 2 * in_bytes))
        for fi, flen in enumerate(FLENS):
            call, out = caller(s, e, flen)
            t = per_launch(call, args.reps)
            fmas = 2 * flen * Lw * B
            pieces = -(-Lw // ops.BSS_PIECE)
            lines.append(row(f"storm_bss_sdr_rows flen = {flen}: 2 launches, {B * pieces} + {B} workgroups, {fmas:.3e} fp64 FMAs, sdr {float(out[0]):.3f} dB", t))
            floor = "fp64 FMA rate unmeasured" if rate is None else f"(b) FMA count / FMA rate {1e6 * fmas / rate:.1f} us, call / that {t[0] * 1e-3 / (fmas / rate):.1f} x"
            lines.append(f"    {floor}; call / copy {t[0] / cp[0]:.1f} x")
            th, back = host_restatement(s, e, flen, 3)
            gap = float((back - out).abs().max())
            lines.append(row("(c) the restatement on the host (np.cumsum correlations, scipy solve_toeplitz), both transfers included, 3 calls", th))
            lines.append(f"    host / device {th[0] / t[0]:.0f} x; largest |device - host| over the rows {gap:.2e} dB")
            if kt is not None:
                c, v = kt[(si, fi)]
                lines.append(f"    (d) kernel trace (a run of its own, medians of {TRACE_CALLS - 2} dispatches): correlations {c:.1f} us, solve {v:.1f} us")
            else:
                lines.append("    (d) kernel trace: not taken")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
