"""Time the posterior ensembles on the device.
  (1) the combine (storm_ensemble_combine_rows: the combine-and-partials stream and the row kernel) on 16 utterances x 8 draws of 256 x 256
      bins, every mode, with and without the spread.  Beside it, in the same run: a device-to-device copy of as many bytes as the call
      moves at least - 8 N F T read + 12 B F T written (8 B F T without the spread) - and the floor that rate gives.
  (2) end to end: ONE 4 s utterance with draws=16 (one batch of 16 rows, one STFT, one combine, one iSTFT) against 16 separate `enhance`
      calls with the same keys - what a user of the single-draw surface would run - on the benchmark's network with its seeded weights
      (quality is not at stake here: no trained weights).
One pair of HIP events per call on the one stream, median of --reps calls after a warm-up (as tools/lpc_time.py); (2) in wall time around a
synchronize, median of --e2e-reps runs.

    python tools/ensemble_time.py [--out profiles/r24_ensemble.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from storm_amd import _lib as L  # noqa: E402
from storm_amd import ops  # noqa: E402
from tools.time_metrics import copy_time, per_launch, row  # noqa: E402

B, K, F, T = 16, 8, 256, 256


def caller(pool, table, mode, spread):
    lib, st = L.lib(), L.stream()
    N = pool.shape[0]
    out = torch.empty((B, F, T), dtype=torch.complex64, device=pool.device)
    sp = torch.empty((B, F, T), dtype=torch.float32, device=pool.device) if spread else None
    rows = torch.empty((B, 2 + K), dtype=torch.float64, device=pool.device)
    best = torch.empty((B,), dtype=torch.int32, device=pool.device)
    ws = torch.empty(lib.storm_ensemble_scratch_bytes(B, F, T, K) // 8, dtype=torch.float64, device=pool.device)

    def call():
        L.check(lib.storm_ensemble_combine_rows(pool.data_ptr(), N, F * T, L.ptr(table), out.data_ptr(), L.ptr(sp), L.ptr(rows), L.ptr(best), L.ptr(ws),
                                                8 * ws.numel(), B, K, F, T, None, 0.15, 0.5, L.ENSEMBLE_MODES[mode], st), "storm_ensemble_combine_rows")
    return call, (out, sp, rows, best)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def end_to_end(dev, reps, lines):
    from bench import randomize
    from storm_amd.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)
    randomize(m, seed=0)
    m._error_loading_ema = True
    m = m.eval().to(dev)
    m.set_precision("bf16")
    g = torch.Generator().manual_seed(24)
    y = (0.1 * torch.randn(1, 65408, generator=g)).to(dev)
    kw = dict(N=30, corrector="ald", snr=0.5)
    keys = [ops.draw_key(7, k) for k in range(16)]
    one = wall(lambda: m.enhance_ensemble(y, draws=16, combine="mean", keys=[7], batch=16, **kw), reps)
    sep = wall(lambda: [m.enhance(y, seed=k, **kw) for k in keys], reps)
    lines.append(f"end to end, the benchmark's network (ncsnpp, {sum(p.numel() for p in m.parameters()) / 1e6:.1f} M parameters, bench.py's seeded weights), bf16, one "
                 f"utterance of 65408 samples (512 frames), N = 30 + ald (60 evaluations per draw): wall time around a synchronize, median (min .. max) of {reps} runs")
    lines.append(f"  {1e3 * one[0]:9.1f} ms ({1e3 * one[1]:.1f} .. {1e3 * one[2]:.1f})  enhance_ensemble(draws=16, batch=16): one sampler run of 16 rows, one combine, one iSTFT")
    lines.append(f"  {1e3 * sep[0]:9.1f} ms ({1e3 * sep[1]:.1f} .. {1e3 * sep[2]:.1f})  16 separate enhance(seed=draw_key(7, k)) calls (each returns its waveform to the host)")
    lines.append(f"    separate / ensemble {sep[0] / one[0]:.2f} x")
    lines.append("")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--e2e-reps", type=int, default=3)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(24)
    N = B * K
    pool = (torch.view_as_complex(torch.randn(N, F, T, 2, generator=g)) * 10.0 ** (4 * torch.rand(N, F, T, generator=g) - 3)).to(dev)
    table = torch.arange(N, dtype=torch.int32, device=dev).reshape(B, K)
    lines = [f"posterior ensembles on the device, {torch.cuda.get_device_name(0)}",
             f"all figures measured on that device: median (min .. max) of {args.reps} calls, one pair of HIP events per call on the one stream, after 5 warm-up calls",
             f"combine: {B} utterances x {K} draws of {F} x {T} bins, transform (0.15, 0.5); one workgroup of four waves per {ops.ENSEMBLE_TILE} bins, two bins per "
             "lane per draw as one 16-byte load, fp64 after the load; then one wave per utterance for the row numbers", ""]
    for spread in (True, False):
        nbytes = 8 * N * F * T + (12 if spread else 8) * B * F * T
        cp = copy_time(nbytes // 2, dev, args.reps)                            # (a copy of n bytes reads n and writes n: this one moves nbytes in all)
        lines.append(row(f"device-to-device copy that moves {nbytes / 1e6:.1f} MB in all (the floor of a call {'with' if spread else 'without'} spread: "
                         f"8 N F T read + {12 if spread else 8} B F T written)", cp, nbytes))
        for mode in ops.ENSEMBLE_MODES:
            call, res = caller(pool, table, mode, spread)
            t = per_launch(call, args.reps)
            want = ops.ensemble_combine(pool, table, 0.15, 0.5, mode=mode, spread=spread)
            assert torch.equal(torch.view_as_real(res[0]), torch.view_as_real(want[0])) and torch.equal(res[2], want[2]) and torch.equal(res[3], want[3])
            lines.append(row(f"storm_ensemble_combine_rows {mode:>10} {'with' if spread else 'without'} spread: {t[0] / cp[0]:.2f} x the copy", t, nbytes))
        lines.append("")
    if args.e2e_reps > 0:
        end_to_end(dev, args.e2e_reps, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
