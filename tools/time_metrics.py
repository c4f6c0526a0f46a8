"""Time the metric kernels (storm_energy_ratios_rows, storm_lsd_rows) at one 10-s file (B = 1 x 160 000 samples) and at the bench batch of
16 x 4 s (B = 16 x 64 000), next to the existing storm_si_sdr on the same rows and a device-to-device copy that moves the same bytes, and
print their parity with the reference's float64 values of fixture F24 on this device.  One pair of HIP events per call on the one stream,
median of --reps calls after a warm-up; a call of the energy / LSD entry points is its two launches (partials + row sums).

    python tools/time_metrics.py [--out profiles/r13_metrics.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from storm_amd.util import other as O  # noqa: E402
from tests import metrics_cases as MC  # noqa: E402


def per_launch(fn, reps, warmup=5):
    """(median, min, max) ms of `reps` calls, each between its own two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def copy_time(nbytes, dev, reps):
    """a device-to-device copy of nbytes (reads them and writes as many)"""
    src = torch.empty(max(nbytes // 4, 1), device=dev)
    dst = torch.empty_like(src)
    return per_launch(lambda: dst.copy_(src), reps)


def row(label, t, nbytes=None):
    """nbytes: the bytes the call moves (a kernel: its inputs, read once; a copy: read + written)"""
    rate = "" if nbytes is None else f"   {nbytes / t[0] / 1e9:6.3f} TB/s"
    return f"  {1e3 * t[0]:9.1f} us ({1e3 * t[1]:.1f} .. {1e3 * t[2]:.1f})  {label}{rate}"


def parity(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "f24_metrics.npz"))
    lines = ["parity with the reference's float64 values (fixture F24), this device:"]
    worst = 0.0
    for k, case in enumerate(MC.ENERGY_CASES):
        sh, s, n = (torch.from_numpy(v)[None].to(dev) for v in MC.energy_inputs(case))
        worst = max(worst, float(np.abs(ops.energy_ratios_rows(sh, s, n).cpu().numpy()[0] - g["energy_ref64"][k]).max()))
    lines.append(f"  SI-SDR / SI-SIR / SI-SAR / input SNR over {len(MC.ENERGY_CASES)} cases: largest |difference| {worst:.2e} dB (test bound 1e-4 dB)")
    bound = 4.0 * float(np.max(np.abs(g["lsd_ref32"] - g["lsd_ref64"])))
    for k, case in enumerate(MC.LSD_CASES):
        sh, s, _ = (torch.from_numpy(v)[None].to(dev) for v in MC.lsd_inputs(case))
        lines.append(f"  lsd {case['name']:>15}: |difference| {abs(float(O.lsd(sh, s)[0]) - float(g['lsd_ref64'][k])):.2e} (test bound {bound:.2e})")
    return lines + [""]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=200)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream()
    g = torch.Generator().manual_seed(13)
    lines = [f"metric kernels, fp32 waveforms / complex64 spectrograms, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls", ""]
    lines += parity(dev)
    for B, Lw in ((1, 160000), (16, 64000)):
        s = (0.1 * torch.randn(B, Lw, generator=g)).to(dev)
        n = (0.05 * torch.randn(B, Lw, generator=g)).to(dev)
        sh = (0.8 * s + 0.3 * n).contiguous()
        out = torch.empty(B, 4, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.storm_energy_ratios_scratch_bytes(B, Lw), dtype=torch.uint8, device=dev)
        sdr = torch.empty(B, device=dev)

        def energy():
            L.check(lib.storm_energy_ratios_rows(L.ptr(sh), L.ptr(s), L.ptr(n), L.ptr(out), L.ptr(ws), ws.numel(), B, Lw, Lw, Lw, Lw, None, st),
                    "storm_energy_ratios_rows")

        def si_sdr():
            L.check(lib.storm_si_sdr(L.ptr(s), L.ptr(sh), L.ptr(sdr), B, Lw, Lw, Lw, 0.0, st), "storm_si_sdr")
        A, S = ops.stft(sh), ops.stft(s)
        F, T = A.shape[1:]
        lout = torch.empty(B, dtype=torch.float64, device=dev)
        lws = torch.empty(lib.storm_lsd_scratch_bytes(B, F, T), dtype=torch.uint8, device=dev)
        Ar, Sr = torch.view_as_real(A), torch.view_as_real(S)

        def lsd_rows():
            L.check(lib.storm_lsd_rows(L.ptr(Ar), L.ptr(Sr), L.ptr(lout), L.ptr(lws), lws.numel(), B, F, T, None, 1e-10, st), "storm_lsd_rows")
        e_bytes, d_bytes, l_bytes = 12 * B * Lw, 8 * B * Lw, 16 * B * F * T
        te, td, tl = per_launch(energy, args.reps), per_launch(si_sdr, args.reps), per_launch(lsd_rows, args.reps)
        tw = per_launch(lambda: O.lsd(sh, s), args.reps)
        ce, cl = copy_time(e_bytes, dev, args.reps), copy_time(l_bytes, dev, args.reps)
        assert torch.equal(out, ops.energy_ratios_rows(sh, s, n)) and torch.equal(lout, ops.lsd_rows(A, S))
        assert float((out[:, 0] - sdr.double()).abs().max()) < 2e-3
        lines += [f"B = {B} x {Lw} samples ({B * Lw / 16000:.0f} s of audio); spectrograms {B} x {F} x {T}",
                  row(f"storm_energy_ratios_rows: 3 rows read once, {e_bytes / 1e6:.2f} MB, {-(-Lw // ops.METRICS_CHUNK) * B} workgroups", te, e_bytes),
                  row(f"storm_si_sdr (one 256-thread workgroup per row, 2 rows read twice: {d_bytes / 1e6:.2f} MB once)", td, d_bytes),
                  row(f"device-to-device copy of {e_bytes / 1e6:.2f} MB (read + written)", ce, 2 * e_bytes),
                  f"    energy / copy {te[0] / ce[0]:.2f} x, energy / storm_si_sdr {te[0] / td[0]:.2f} x",
                  row(f"storm_lsd_rows: 2 spectrograms read once, {l_bytes / 1e6:.2f} MB, {-(-T // 64) * -(-F // 32) * B} workgroups", tl, l_bytes),
                  row(f"device-to-device copy of {l_bytes / 1e6:.2f} MB (read + written)", cl, 2 * l_bytes),
                  f"    lsd_rows / copy {tl[0] / cl[0]:.2f} x",
                  row("util.other.lsd, wav in: two storm_stft + storm_lsd_rows (host wrappers included)", tw), ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
