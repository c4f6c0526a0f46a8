"""Time STOI / ESTOI on the device (storm_resample_poly_taps with the STOI filter, then storm_stoi_rows) at one 10-s file (B = 1 x 160 000
samples at 16 kHz) and at the bench batch of 16 x 4 s (B = 16 x 64 000), the resampling and the metric separately, next to the two
yardsticks of tools/time_metrics.py: a device-to-device copy that moves the same input bytes and storm_energy_ratios_rows on the same rows.
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up.  A call of the resampling is 2 launches (clean,
processed), a call of the metric 5 (frame energies, gate, band spectra, segments, row sums).

    python tools/stoi_time.py [--out profiles/r16_stoi.txt]

Per kernel: --kernels B runs nothing but --reps calls of the resampling and of the metric at the shape with B rows (1 or 16), for a kernel
trace around the tool; profiles/r16_stoi_kernels.txt holds the two tables of

    rocprofv3 --kernel-trace --stats -d DIR -o bB --output-format csv -- python tools/stoi_time.py --kernels B --reps 50      (B = 1, 16)

(DIR/.../bB_kernel_stats.csv: calls and average nanoseconds per kernel name).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from tests import stoi_cases as SC  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

FS = 16000
SHAPES = ((1, 160000), (16, 64000))     # one 10-s file; the bench batch of 16 x 4 s


def parity(dev):
    lines = ["parity with the float64 restatement of the definition (tests/stoi_cases.py; NOT pystoi, which no machine of the project has), this device:"]
    for name in SC.CASES:
        c, p = SC.signals(name)
        fs = SC.CASES[name][2]
        got = ops.stoi_rows(torch.from_numpy(c.copy())[None].to(dev), torch.from_numpy(p.copy())[None].to(dev), fs=fs).cpu().numpy()[0]
        r = SC.restated(name)
        lines.append(f"  {name:>10} at {fs:5d} Hz: STOI {got[0]:.12f} ESTOI {got[1]:.12f}, |difference| {abs(got[0] - r['stoi']):.2e} {abs(got[1] - r['estoi']):.2e}")
    return lines + [""]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--kernels", type=int, default=None, choices=[s[0] for s in SHAPES], metavar="B",
                   help="only --reps calls of the resampling and the metric at the shape with B rows (to be run under a kernel trace)")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream()
    g = torch.Generator().manual_seed(16)
    lines = [f"STOI / ESTOI on the device, fp32 waveforms at {FS} Hz, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls", ""]
    if args.kernels is None:
        lines += parity(dev)
    taps, n_taps, up, down = ops._stoi_table(FS, dev)
    for B, Lw in SHAPES:
        if args.kernels not in (None, B):
            continue
        s = (0.1 * torch.randn(B, Lw, generator=g)).to(dev)
        n = (0.05 * torch.randn(B, Lw, generator=g)).to(dev)
        sh = (0.8 * s + 0.3 * n).contiguous()
        L10 = -(-Lw * up // down)
        s10, sh10 = torch.empty(B, L10, device=dev), torch.empty(B, L10, device=dev)
        out = torch.empty(B, 2, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.storm_stoi_scratch_bytes(B, L10), dtype=torch.uint8, device=dev)
        eout = torch.empty(B, 4, dtype=torch.float64, device=dev)
        ews = torch.empty(lib.storm_energy_ratios_scratch_bytes(B, Lw), dtype=torch.uint8, device=dev)

        def resample():
            for x, y in ((s, s10), (sh, sh10)):
                L.check(lib.storm_resample_poly_taps(L.ptr(x), L.ptr(y), L.ptr(taps), B, Lw, Lw, L10, L10, None, up, down, n_taps, st),
                        "storm_resample_poly_taps")

        def metric():
            L.check(lib.storm_stoi_rows(L.ptr(s10), L.ptr(sh10), L.ptr(out), L.ptr(ws), ws.numel(), B, L10, L10, L10, None, st), "storm_stoi_rows")

        def energy():
            L.check(lib.storm_energy_ratios_rows(L.ptr(sh), L.ptr(s), L.ptr(n), L.ptr(eout), L.ptr(ews), ews.numel(), B, Lw, Lw, Lw, Lw, None, st),
                    "storm_energy_ratios_rows")
        if args.kernels is not None:
            for _ in range(args.reps):
                resample()
                metric()
            torch.cuda.synchronize()
            print(f"{args.reps} calls of the resampling (2 launches) and of storm_stoi_rows (5 launches) at B = {B} x {Lw} samples")
            return
        r_bytes, m_bytes, e_bytes = 8 * B * Lw, 8 * B * L10, 12 * B * Lw
        tr, tm, te = per_launch(resample, args.reps), per_launch(metric, args.reps), per_launch(energy, args.reps)
        tw = per_launch(lambda: ops.stoi_rows(s, sh, fs=FS), args.reps)
        cr, cm = copy_time(r_bytes, dev, args.reps), copy_time(m_bytes, dev, args.reps)
        assert torch.equal(out, ops.stoi_rows(s, sh, fs=FS))
        counts = np.frombuffer(ws[:16 * B].cpu().numpy().tobytes(), dtype=np.int32).reshape(B, 4)
        frames, kept, segs = (int(v) for v in counts[0, :3])
        nM = frames - 1                                                      # the band-spectrum grid: the most frames a row of L10 samples can have
        lines += [f"B = {B} x {Lw} samples ({B * Lw / FS:.0f} s of audio) -> {B} x {L10} at 10 kHz; a row has {frames} gate frames, {kept} kept, {segs} segments",
                  row(f"resampling {up}/{down}, {n_taps} taps: 2 signals read once, {r_bytes / 1e6:.2f} MB, 2 launches x {-(-L10 // ops.RESAMPLE_TILE) * B} workgroups",
                      tr, r_bytes),
                  row(f"device-to-device copy of {r_bytes / 1e6:.2f} MB (read + written)", cr, 2 * r_bytes),
                  f"    resampling / copy {tr[0] / cr[0]:.2f} x",
                  row(f"storm_stoi_rows: 2 signals at 10 kHz, {m_bytes / 1e6:.2f} MB, 5 launches ({-(-frames // 4) * B} + {B} + {nM * B} + "
                      f"{-(-(nM - 29) // 4) * B} + {B} workgroups)", tm, m_bytes),
                  row(f"device-to-device copy of {m_bytes / 1e6:.2f} MB (read + written)", cm, 2 * m_bytes),
                  f"    metric / copy {tm[0] / cm[0]:.2f} x, metric per launch {1e3 * tm[0] / 5:.1f} us",
                  row(f"storm_energy_ratios_rows on the same rows at 16 kHz (2 launches, {e_bytes / 1e6:.2f} MB)", te, e_bytes),
                  f"    (resampling + metric) / energy ratios {(tr[0] + tm[0]) / te[0]:.2f} x with 7 launches against 2",
                  row("ops.stoi_rows, wav at 16 kHz in: 2 + 5 launches, host wrapper (allocations, length table) included", tw), ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
