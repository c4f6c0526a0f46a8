"""Time the delay search, the shift and the biquad cascade on the device at one 10-s row (B = 1 x 160 000 samples at 16 kHz) and at the
bench batch of 16 x 4 s (B = 16 x 64 000): storm_xcorr_lag_rows unbounded and with max_lag = 0.5 s, storm_shift_rows, storm_sosfilt_rows
with the reference's five sections.  Beside each stands its yardstick:
  delay search  its own fp64 FMA count (sum over the lags of the overlap lengths) divided by the device's fp64 FMA rate - measured by
                tools/ubench/fma64_rate (built: hipcc --offload-arch=gfx950 -O3 tools/ubench/fma64_rate.hip -o tools/ubench/fma64_rate),
                or given with --fma-rate GFMA/s - and a device-to-device copy of the input bytes;
  shift         that copy;
  cascade       that copy, and scipy.signal.sosfilt on the host for the same rows, device <-> host transfers included: the alternative the
                kernel removes.
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up (as tools/time_metrics.py).

    python tools/align_time.py [--out profiles/r17_align.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

FS = 16000
SHAPES = ((1, 160000), (16, 64000))     # one 10-s file; the bench batch of 16 x 4 s


def fma_rate(given):
    """the device's fp64 FMA rate in FMA/s: --fma-rate, else the micro-benchmark's own line, else None"""
    if given:
        return given * 1e9, "--fma-rate"
    exe = os.path.join(ROOT, "tools", "ubench", "fma64_rate")
    if not os.path.exists(exe):
        return None, "tools/ubench/fma64_rate is not built"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"fp64 FMA rate: ([0-9.]+) GFMA/s", out)
    return (float(m.group(1)) * 1e9, out.strip()) if m else (None, "tools/ubench/fma64_rate printed no rate")


def xcorr_fmas(n, max_lag):
    """FMAs of one row of n against n samples: sum over the lags d of n - |d|"""
    m = n - 1 if max_lag is None else min(max_lag, n - 1)
    return n + 2 * sum(n - d for d in range(1, m + 1))


def host_sosfilt(x, sos, reps):
    """(median, min, max) ms of: rows to the host, scipy.signal.sosfilt in fp64, result back to the device"""
    import scipy.signal as ss
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        y = torch.from_numpy(ss.sosfilt(sos, x.cpu().numpy().astype(np.float64), axis=-1)).to(x.device)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t))
    assert y.shape == x.shape
    return statistics.median(ms), min(ms), max(ms)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--fma-rate", type=float, default=None, help="the device's fp64 FMA rate in GFMA/s (default: run tools/ubench/fma64_rate)")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    lib, st = L.lib(), L.stream()
    rate, how = fma_rate(args.fma_rate)
    g = torch.Generator().manual_seed(17)
    sos = ops.butter_sos(10, 80 / FS * 2)
    lines = [f"delay search, shift and biquad cascade on the device, fp32 waveforms at {FS} Hz, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls",
             f"lag tile STORM_XCORR_TILE = {ops.XCORR_TILE} lags per workgroup, 8 / 4 / 2 lags per thread by the launch's lag count (a wave for every SIMD); "
             "cascade: one wave per min(64 / S, 16) rows, blocks of 32 samples handed from section to section through LDS",
             f"fp64 FMA rate of the device: {'unmeasured' if rate is None else f'{rate / 1e9:.1f} GFMA/s'} ({how})", ""]
    for B, Lw in SHAPES:
        s = (0.1 * torch.randn(B, Lw, generator=g)).to(dev)
        late = torch.roll(s, 37, dims=1).contiguous()
        in_bytes = 8 * B * Lw
        lag, peak = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
        cp = copy_time(in_bytes, dev, args.reps)
        lines.append(f"B = {B} x {Lw} samples ({B * Lw / FS:.0f} s of audio)")
        lines.append(row(f"device-to-device copy of the two inputs, {in_bytes / 1e6:.2f} MB (read + written)", cp, 2 * in_bytes))
        for ml in (None, FS // 2):
            tiles = lib.storm_xcorr_num_partials(Lw, Lw, -1 if ml is None else ml)
            ws = torch.empty(B * tiles * L.XCORR_PARTIAL_BYTES, dtype=torch.uint8, device=dev)

            def search():
                L.check(lib.storm_xcorr_lag_rows(L.ptr(late), L.ptr(s), L.ptr(lag), L.ptr(peak), L.ptr(ws), ws.numel(), B, Lw, Lw, Lw, Lw, None, None,
                                                 -1 if ml is None else ml, st), "storm_xcorr_lag_rows")
            reps = args.reps if ml is not None else max(args.reps // 10, 5)      # (the unbounded search of a 10-s row is milliseconds long)
            t = per_launch(search, reps)
            assert lag.tolist() == [-37] * B
            fmas = B * xcorr_fmas(Lw, ml)
            floor = "fp64 FMA rate unmeasured" if rate is None else f"FMA count / FMA rate {1e6 * fmas / rate:.1f} us, search / that {t[0] * 1e-3 / (fmas / rate):.2f} x"
            lines += [row(f"storm_xcorr_lag_rows {'unbounded' if ml is None else f'max_lag = {ml} ({ml / FS} s)'}: 2 launches, {B * tiles} + 1 workgroups, "
                          f"{fmas:.3e} fp64 FMAs ({reps} calls)", t),
                      f"    {floor}; search / copy {t[0] / cp[0]:.1f} x"]
        sh = torch.full((B,), -37, dtype=torch.int32, device=dev)
        out = torch.empty(B, Lw, device=dev)
        ts = per_launch(lambda: L.check(lib.storm_shift_rows(L.ptr(late), L.ptr(out), L.ptr(sh), B, Lw, Lw, Lw, None, 1, st), "storm_shift_rows"), args.reps)
        assert torch.equal(out, s)
        c1 = copy_time(4 * B * Lw, dev, args.reps)
        lines += [row(f"storm_shift_rows by -37 (wrap): {4 * B * Lw / 1e6:.2f} MB read once", ts, 4 * B * Lw),
                  row(f"device-to-device copy of {4 * B * Lw / 1e6:.2f} MB (read + written)", c1, 8 * B * Lw), f"    shift / copy {ts[0] / c1[0]:.2f} x"]
        o64 = torch.empty(B, Lw, dtype=torch.float64, device=dev)
        reps = max(args.reps // 10, 5)
        tf = per_launch(lambda: L.check(lib.storm_sosfilt_rows(L.ptr(s), L.ptr(o64), sos.data_ptr(), 5, B, Lw, Lw, Lw, None, 0, st), "storm_sosfilt_rows"), reps)
        th = host_sosfilt(s, sos.numpy(), max(reps // 2, 3))
        lines += [row(f"storm_sosfilt_rows, 5 sections, fp64 out: 1 launch, {-(-B // 12)} workgroup(s) of one wave ({reps} calls)", tf, 4 * B * Lw),
                  row("scipy.signal.sosfilt on the host for the same rows, device -> host and host -> device included", th),
                  f"    cascade / copy {tf[0] / c1[0]:.1f} x; host / cascade {th[0] / tf[0]:.2f} x", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
