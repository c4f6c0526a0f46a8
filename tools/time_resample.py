"""Time storm_resample_poly at the bench batch (16 rows x 4 s) for 48 <-> 16 kHz and 44.1 <-> 16 kHz next to a device-to-device copy
that moves the same bytes, and one ScoreModel.enhance_batch at the bench shape (bf16, N = 30, ALD corrector) with and without sr=48000.
The kernel and the copy: one pair of HIP events per launch on the one stream, median of --reps launches after a warm-up.

    python tools/time_resample.py [--out profiles/r12_resample.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import randomize  # noqa: E402
from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from storm_amd.model import ScoreModel  # noqa: E402


def per_launch(fn, reps, warmup=5):
    """(median, min, max) ms of `reps` launches, each between its own two events"""
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--no-model", action="store_true")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    B, seconds = 16, 4
    g = torch.Generator().manual_seed(1)
    lines = [f"storm_resample_poly at the bench batch: {B} rows x {seconds} s, fp32, {torch.cuda.get_device_name(0)}",
             f"median (min .. max) of {args.reps} launches, one pair of HIP events per launch on the one stream, after 5 warm-up launches", ""]
    for sr_in, sr_out in ((48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100)):
        up, down = ops.resample_ratio(sr_out, sr_in)
        x = (0.1 * torch.randn(B, seconds * sr_in, generator=g)).to(dev)
        taps = ops.resample_taps(up, down, device=dev)
        Lin, Lout = x.shape[1], ops.resample_length(x.shape[1], up, down)
        y = torch.empty(B, Lout, device=dev)
        lib, st = L.lib(), L.stream()

        def launch():
            L.check(lib.storm_resample_poly(L.ptr(x), L.ptr(y), L.ptr(taps), B, Lin, Lin, Lout, Lout, None, up, down, st), "storm_resample_poly")
        nbytes = 4 * B * (Lin + Lout)
        src = torch.empty(nbytes // 8, device=dev)                  # a copy reads and writes its size: half the kernel's bytes each way
        dst = torch.empty_like(src)
        k, c = per_launch(launch, args.reps), per_launch(lambda: dst.copy_(src), args.reps)
        assert torch.equal(y, ops.resample_poly(x, up, down))
        lines += [f"{sr_in} -> {sr_out} Hz (up {up}, down {down}, {taps.shape[1]} taps per phase): {B} x {Lin} in, {B} x {Lout} out, {nbytes / 1e6:.2f} MB",
                  f"  {1e3 * k[0]:9.1f} us ({1e3 * k[1]:.1f} .. {1e3 * k[2]:.1f})  storm_resample_poly   {nbytes / k[0] / 1e9:6.3f} TB/s of algorithmic bytes",
                  f"  {1e3 * c[0]:9.1f} us ({1e3 * c[1]:.1f} .. {1e3 * c[2]:.1f})  device-to-device copy of {nbytes / 2e6:.2f} MB (the same bytes moved)",
                  f"  ratio to the copy: {k[0] / c[0]:.2f} x", ""]
    if not args.no_model:
        m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)
        randomize(m, seed=0)
        m._error_loading_ema = True
        m = m.eval().to(dev)
        m.set_precision("bf16")
        kw = dict(N=30, corrector="ald", corrector_steps=1, snr=0.5)
        w16 = (0.1 * torch.randn(B, seconds * 16000, generator=g)).to(dev)
        w48 = (0.1 * torch.randn(B, seconds * 48000, generator=g)).to(dev)

        def wall(fn, reps=3):
            import time
            fn(0)                                                   # warm-up: code objects, graphs, the tap table
            out = []
            for i in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(1 + i)
                torch.cuda.synchronize()
                out.append(time.perf_counter() - t0)
            return statistics.median(out)
        a = wall(lambda i: m.enhance_batch(w16, seed=i, **kw))
        b = wall(lambda i: m.enhance_batch(w48, seed=i, sr=48000, **kw))
        lines += [f"ScoreModel.enhance_batch, {B} x {seconds} s, ncsnpp bf16, N = 30 + ALD (median wall time of 3 calls, host clock around a device synchronise):",
                  f"  {1e3 * a:9.2f} ms  16 kHz input",
                  f"  {1e3 * b:9.2f} ms  48 kHz input, sr=48000 (resample, enhance, resample back, trim)",
                  f"  difference {1e3 * (b - a):.2f} ms = {100 * (b - a) / a:.2f} %", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
