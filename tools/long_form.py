"""Time long recordings on the 27.8 M network with the benchmark's seeded random weights (bf16, 30 PC steps with the ald corrector): one
recording as ONE row against the same recording through enhance_long, four recordings of different lengths through batch-1 calls against
enhance_long, and storm_crossfade_rows alone next to a device-to-device copy of its output bytes.  Every stage is its own process (so that a
launcher can give each its own time limit) and appends its lines to --out; wall-clock medians of --reps runs after one warm-up run, the
device synchronised on both sides.

    for s in header kernel whole windowed files files_long; do timeout 600 python tools/long_form.py --stage $s --out profiles/r15_long_form.txt || break; done
    (whole / windowed take --seconds, 60 by default)
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(N=30, corrector="ald", corrector_steps=1, snr=0.5)
W, V = 65408, 8192


def model(dev):
    import bench
    from storm_amd.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)
    bench.randomize(m, seed=0)
    m._error_loading_ema = True
    m.eval()
    m = m.to(dev)
    m.set_precision("bf16")
    return m


def timed(fn, reps):
    """(median seconds, all, the last result) of `reps` runs after one warm-up run"""
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, out


def fmt(t):
    return f"{t[0]:8.3f} s ({', '.join(f'{v:.3f}' for v in t[1])})"


def recording(seconds, seed, dev):
    return (0.1 * torch.randn(int(seconds * 16000), generator=torch.Generator().manual_seed(seed))).to(dev)


def per_launch(fn, reps, warmup=5):
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
    p.add_argument("--stage", required=True, choices=["header", "whole", "windowed", "files", "files_long", "kernel"])
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--seconds", type=float, default=60.0, help="stages whole / windowed: the recording's duration")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    from storm_amd import ops
    from storm_amd.distributed import bucket_by_frames
    lines = []
    if args.stage == "header":
        lines = [f"long recordings, NCSN++ 27.8 M with seeded random weights, bf16, PC sampler N = 30 + ald, {torch.cuda.get_device_name(0)}",
                 f"window {W} samples (512 frames), overlap {V}; wall-clock median of {args.reps} runs after one warm-up run (all runs in brackets)", ""]
    elif args.stage in ("whole", "windowed"):
        m, x = model(dev), recording(args.seconds, 1, dev)
        if args.stage == "whole":
            t = timed(lambda: m.enhance_batch(x[None], row_seeds=[11], return_nfe=True, **KW), args.reps)
            frames = m.data_module.padded_frames(x.numel())
            lines = [f"one {args.seconds:g}-s recording ({x.numel()} samples)",
                     f"  {fmt(t)}  as ONE row of {frames} frames (enhance_batch, batch 1): {t[2][1]} evaluations of 1 row"]
        else:
            n = ops.window_plan(x.numel(), W, V)[0]
            t = timed(lambda: m.enhance_long([x], window=W, overlap=V, batch=16, keys=[11], return_nfe=True, **KW), args.reps)
            lines = [f"  {fmt(t)}  enhance_long(batch=16): {n} windows in {-(-n // 16)} batches, {t[2][1]} row evaluations in all", ""]
    elif args.stage in ("files", "files_long"):
        m = model(dev)
        recs = [recording(s, 10 + k, dev) for k, s in enumerate((20, 35, 50, 65))]
        keys = [21, 22, 23, 24]
        if args.stage == "files":
            buckets = bucket_by_frames([r.numel() for r in recs], 16)
            t = timed(lambda: [m.enhance_batch(recs[b[0]][None], row_seeds=[keys[b[0]]], **KW) for b in buckets], args.reps)
            lines = ["four recordings of 20 / 35 / 50 / 65 s",
                     f"  {fmt(t)}  one row each: {len(buckets)} frame buckets of one file, one batch-1 enhance_batch call after the other"]
        else:
            n = sum(ops.window_plan(r.numel(), W, V)[0] for r in recs)
            t = timed(lambda: m.enhance_long(recs, window=W, overlap=V, batch=16, keys=keys, return_nfe=True, **KW), args.reps)
            lines = [f"  {fmt(t)}  enhance_long(batch=16): {n} windows in {-(-n // 16)} batches, {t[2][1]} row evaluations in all", ""]
    else:
        g = torch.Generator().manual_seed(3)
        lines = ["storm_crossfade_rows alone: median (min .. max) of 200 calls, one pair of HIP events per call, after 5 warm-up calls"]
        H = W - V
        for recs_n in ([16], [40, 40, 40, 40]):
            N = sum(recs_n)
            pool = torch.randn(N, W, generator=g).to(dev)
            lens = [(n - 1) * H + W - 1234 for n in recs_n]
            ramp = ops.crossfade_ramp(V, "hann", dev)
            out = ops.crossfade_rows(pool, list(range(N)), lens, recs_n, W, V, ramp=ramp)
            nbytes = out.numel() * 4
            from storm_amd import _lib as L
            first = [sum(recs_n[:r]) for r in range(len(recs_n))]
            tab = [torch.tensor(v, dtype=torch.int32).to(dev) for v in (lens, recs_n, first, list(range(N)))]
            raw = torch.empty_like(out)

            def launch():
                L.check(L.lib().storm_crossfade_rows(L.ptr(pool), N, W, L.ptr(raw), len(recs_n), raw.shape[1], raw.stride(0), L.ptr(tab[0]), L.ptr(tab[1]),
                                                     L.ptr(tab[2]), L.ptr(tab[3]), W, V, L.ptr(ramp), L.stream()), "storm_crossfade_rows")
            tr = per_launch(launch, 200)
            assert torch.equal(raw, out)
            tk = per_launch(lambda: ops.crossfade_rows(pool, list(range(N)), lens, recs_n, W, V, ramp=ramp), 200)
            src, dst = torch.empty_like(out), torch.empty_like(out)
            tc = per_launch(lambda: dst.copy_(src), 200)
            lines += [f"  {N} windows in {len(recs_n)} recording(s), output {nbytes / 1e6:.2f} MB, {-(-max(lens) // ops.CROSSFADE_TILE) * len(recs_n)} workgroups",
                      f"    {1e3 * tr[0]:9.1f} us ({1e3 * tr[1]:.1f} .. {1e3 * tr[2]:.1f})  storm_crossfade_rows, the launch alone (tables resident)   "
                      f"{2 * nbytes / tr[0] / 1e9:.3f} TB/s read + written, launch / copy {tr[0] / tc[0]:.2f} x",
                      f"    {1e3 * tk[0]:9.1f} us ({1e3 * tk[1]:.1f} .. {1e3 * tk[2]:.1f})  ops.crossfade_rows (host checks, one int32 table upload, one launch)",
                      f"    {1e3 * tc[0]:9.1f} us ({1e3 * tc[1]:.1f} .. {1e3 * tc[2]:.1f})  device-to-device copy of the same output bytes   crossfade / copy {tk[0] / tc[0]:.2f} x"]
        lines.append("")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "a" if args.stage != "header" else "w").write(text)


if __name__ == "__main__":
    main()
