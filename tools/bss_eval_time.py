"""Time BSS-eval SDR / SIR / SAR with two sources (storm_bss_eval_rows: the correlations of four pairs as one grid, round 18's solve for the SDR,
one wave per row for the block Levinson recursion) on the device at one 10-s row (B = 1 x 160 000 samples at 16 kHz) and at the bench batch of
16 x 4 s (B = 16 x 64 000), for filters of 512 and of 64 taps.  Beside each:
  (a) a device-to-device copy of the input bytes;
  (b) storm_bss_sdr_rows on the same target and estimate rows in the same build;
  (c) the restatement on the host for the same rows (np.cumsum correlations of tests/bss_cases.py for the four pairs, np.linalg.solve on the
      joint matrix of tests/bss_eval_cases.py), device <-> host transfers included: the alternative the kernels remove (--host-reps calls);
  (d) the three kernels separately, from a kernel trace of its own: run
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bss_eval_time.py --trace-loop
      first and hand DIR to --kernel-trace (a profiled run is never compared with an unprofiled one: (d) stands beside the call time, not in it).
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up (as tools/bss_sdr_time.py).

    python tools/bss_eval_time.py [--kernel-trace DIR] [--out profiles/r19_bss_eval.txt]
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
from tools import bss_sdr_time as R18  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

FS, SHAPES, FLENS, TRACE_CALLS = R18.FS, R18.SHAPES, R18.FLENS, R18.TRACE_CALLS


def inputs(B, Lw, dev):
    """seeded rows: an AR(2)-coloured target, white noise, and an estimate that is the target delayed by 37 samples plus a third of the noise
    delayed by 5 plus white artefacts at -30 dB"""
    import scipy.signal as ss
    rng = np.random.default_rng(19)
    s = ss.lfilter([1.0], [1.0, -1.6, 0.8], rng.standard_normal((B, Lw)), axis=-1)
    s = (0.1 * s / s.std()).astype(np.float32)
    n = (0.05 * rng.standard_normal((B, Lw))).astype(np.float32)
    e = np.roll(s, 37, axis=1) + 0.3 * np.roll(n, 5, axis=1) + 0.003 * rng.standard_normal((B, Lw)).astype(np.float32)
    return tuple(torch.from_numpy(v.astype(np.float32)).to(dev) for v in (s, n, e))


def caller(s, n, e, flen):
    B, Lw = s.shape
    lib, st = L.lib(), L.stream()
    out = torch.empty(B, 3, dtype=torch.float64, device=s.device)
    ws = torch.empty(lib.storm_bss_eval_scratch_bytes(B, Lw, flen) // 8, dtype=torch.float64, device=s.device)

    def call():
        L.check(lib.storm_bss_eval_rows(L.ptr(s), L.ptr(n), L.ptr(e), L.ptr(out), None, None, L.ptr(ws), 8 * ws.numel(), B, Lw, Lw, Lw, Lw, None, flen,
                                        st), "storm_bss_eval_rows")
    return call, out


def host_restatement(s, n, e, flen, reps):
    """(median, min, max) ms of: rows to the host, the restatement's correlations of the four pairs and a dense solve per row, the numbers back"""
    from tests import bss_cases as BC
    from tests import bss_eval_cases as EC
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sh, nh, eh = s.cpu().numpy(), n.cpu().numpy(), e.cpu().numpy()
        vals = []
        for k in range(sh.shape[0]):
            a, b, c, d = (BC.correlations(u, v, flen) for u, v in ((sh[k], eh[k]), (nh[k], eh[k]), (sh[k], nh[k]), (nh[k], sh[k])))
            F = flen
            parts = np.concatenate([a[:F], a[F:2 * F], b[:F], b[F:2 * F], c[F:2 * F], d[F:2 * F], a[2 * F:]])
            vals.append(EC.numbers(parts, F)[0])
        back = torch.tensor(np.array(vals), dtype=torch.float64).to(s.device)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    return (statistics.median(ms), min(ms), max(ms)), back


def trace_loop(dev):
    """--trace-loop: TRACE_CALLS calls of every configuration in the order of main(), nothing else of the library on the stream"""
    for B, Lw in SHAPES:
        s, n, e = inputs(B, Lw, dev)
        for flen in FLENS:
            call, _ = caller(s, n, e, flen)
            for _ in range(TRACE_CALLS):
                call()
            torch.cuda.synchronize()


def kernel_times(d):
    """{(shape index, flen index): (corr us, sdr solve us, joint solve us)}: medians over the dispatches of a --trace-loop run, in start order"""
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
    kinds = [[dur for _, dur, name in rows if k in name] for k in ("bss_corr4_kernel", "bss_solve_kernel", "bss_joint_kernel")]
    n = len(SHAPES) * len(FLENS)
    if any(len(k) != n * TRACE_CALLS for k in kinds):
        return None
    out = {}
    for i in range(n):
        sl_ = slice(i * TRACE_CALLS + 2, (i + 1) * TRACE_CALLS)                 # (the first two calls of a configuration: warm-up)
        out[divmod(i, len(FLENS))] = tuple(statistics.median(k[sl_]) / 1e3 for k in kinds)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--host-reps", type=int, default=1)
    p.add_argument("--trace-loop", action="store_true", help="only call every configuration a few times (the program to run under rocprofv3)")
    p.add_argument("--kernel-trace", default=None, metavar="DIR", help="the output directory of a rocprofv3 --kernel-trace run of --trace-loop")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_loop:
        trace_loop(dev)
        return
    kt = kernel_times(args.kernel_trace) if args.kernel_trace else None
    lines = [f"BSS-eval SDR / SIR / SAR with two sources and filters of F taps on the device, fp32 waveforms at {FS} Hz, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls",
             f"correlations: the four pairs as one grid, a workgroup per (pair, row, piece of {ops.BSS_PIECE} samples), the walk of storm_bss_sdr_rows; "
             "sdr and P1: that entry's solve; joint solve: one wave per row, block Levinson with 2 x 2 blocks, 8 blocks of A, Bt and x per lane in "
             "registers, six xor-butterfly reductions per order", ""]
    for si, (B, Lw) in enumerate(SHAPES):
        s, n, e = inputs(B, Lw, dev)
        in_bytes = 12 * B * Lw
        cp = copy_time(in_bytes, dev, args.reps)
        lines.append(f"B = {B} x {Lw} samples ({B * Lw / FS:.0f} s of audio)")
        lines.append(row(f"(a) device-to-device copy of the three inputs, {in_bytes / 1e6:.2f} MB (read + written)", cp, 2 * in_bytes))
        for fi, flen in enumerate(FLENS):
            call, out = caller(s, n, e, flen)
            t = per_launch(call, args.reps)
            pieces = -(-Lw // ops.BSS_PIECE)
            o = out[0].tolist()
            lines.append(row(f"storm_bss_eval_rows flen = {flen}: 3 launches, {4 * B * pieces} + {B} + {B} workgroups, {8 * flen * Lw * B:.3e} fp64 FMAs of "
                             f"correlations, sdr {o[0]:.3f} sir {o[1]:.3f} sar {o[2]:.3f} dB", t))
            call18, out18 = R18.caller(s, e, flen)
            t18 = per_launch(call18, args.reps)
            same = bool(torch.equal(out18, out[:, 0]))
            lines.append(row(f"(b) storm_bss_sdr_rows on the same target and estimate (sdr column bit-equal: {same})", t18))
            lines.append(f"    eval / sdr {t[0] / t18[0]:.2f} x; call / copy {t[0] / cp[0]:.1f} x")
            if args.host_reps > 0:
                th, back = host_restatement(s, n, e, flen, args.host_reps)
                gap = float((back - out).abs().max())
                lines.append(row(f"(c) the restatement on the host (np.cumsum correlations of four pairs, np.linalg.solve), both transfers included, "
                                 f"{args.host_reps} call(s)", th))
                lines.append(f"    host / device {th[0] / t[0]:.0f} x; largest |device - host| over the rows and the three numbers {gap:.2e} dB")
            if kt is not None:
                c, v, j = kt[(si, fi)]
                lines.append(f"    (d) kernel trace (a run of its own, medians of {TRACE_CALLS - 2} dispatches): correlations {c:.1f} us, sdr solve {v:.1f} us, "
                             f"joint solve {j:.1f} us ({j / max(flen - 1, 1):.2f} us per order)")
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
