"""Measurement (not a test) of the ODE sampler's three methods, in two parts.

    python tools/ode_methods.py [--out profiles/r14_ode_methods.txt] [--skip-network] [--skip-kernels] [--methods DOP853 --tols 1e-5 --max-evals 20000]

1. Evaluations and seconds per utterance of RK45 / RK23 / DOP853 at rtol = atol in {1e-5, 3e-2}: the 27.8 M ncsnpp with bench.py's
   seeded RANDOM weights (bench.randomize, seed 0), bf16, 4 utterances of 256 x 256 bins x frames in one enhance_batch call (per_row:
   one step controller per utterance), wav -> wav.  One warm-up run, then the median of --runs runs of the same seeded input (host
   clock around a call that ends in a device -> host copy).  The weights are random: the counts are those of a noise-driven
   right-hand side, not of a trained model.  A run that needs more than --max-evals evaluations is stopped and reported as such.
2. The wide Runge-Kutta launches beside the 7-term launches on the same element count, as GB/s of the bytes each moves: the library's
   entry points called directly on pre-allocated outputs, --inner launches queued between two device events, the median of --reps such
   windows after a warm-up window.  A stage launch reads 8 B per complex element and stage and 16 B of state and writes 16 + 8 B; an
   error launch reads 8 B per stage and 2 x 16 B of state.  The 7-term entry points timed here are THIS build's (the 7-term
   instantiation of the shared body), not a build of the commit before it.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS, TOLS = ("RK45", "RK23", "DOP853"), (3e-2, 1e-5)
BATCH, SAMPLES = 4, 255 * 128                                           # 1 + 32640 // 128 = 256 frames


class TooManyEvaluations(RuntimeError):
    pass


def network_table(args, emit):
    from bench import randomize
    from storm_amd.model import ScoreModel
    dev = torch.device("cuda:0")
    model = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)
    randomize(model, seed=0)
    model._error_loading_ema = True
    model.eval()
    model = model.to(dev)
    model.set_precision("bf16")
    wav = (0.1 * torch.randn(BATCH, SAMPLES, generator=torch.Generator().manual_seed(1234))).to(dev)
    count = [0]
    forward = model.forward

    def counted(x, t, y, **kw):
        count[0] += 1
        if count[0] > args.max_evals:
            raise TooManyEvaluations()
        return forward(x, t, y, **kw)
    model.forward = counted

    def run(method, tol):
        count[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, nfe = model.enhance_batch(wav, sampler_type="ode", method=method, rtol=tol, atol=tol, seed=7, return_nfe=True)
        out = out.cpu()                                                 # (ends the timed region: device -> host)
        el = time.perf_counter() - t0
        assert out.shape == (BATCH, SAMPLES) and bool(torch.isfinite(out).all())
        return el, nfe, list(model.last_nfev_rows)
    emit(f"# 27.8 M ncsnpp, bench.py's seeded random weights, bf16, {BATCH} x 256 x 256, per_row; one warm-up, median of {args.runs} runs; "
         f"evaluations include the 2 of the initial step, the closing denoising evaluation is one more")
    emit(f"{'method':8s} {'rtol=atol':>9s} {'evaluations per utterance':>34s} {'executed':>9s} {'s / utterance':>14s} {'runs (s / batch)':>28s}")
    for tol in args.tols:
        for method in args.methods:
            try:
                run(method, tol)                                        # warm-up: every shape and launch of this method
                res = [run(method, tol) for _ in range(args.runs)]
            except TooManyEvaluations:
                torch.cuda.synchronize()
                emit(f"{method:8s} {tol:9g} {'stopped: more than %d evaluations' % args.max_evals:>34s}")
                continue
            secs = [r[0] for r in res]
            assert all(r[1:] == res[0][1:] for r in res)                # (the same seeded input: the same step sequence)
            rows = res[0][2]
            emit(f"{method:8s} {tol:9g} {' '.join(str(r) for r in rows) + '  (mean %.1f)' % (sum(rows) / BATCH):>34s} {res[0][1]:9d} "
                 f"{statistics.median(secs) / BATCH:14.3f} {' '.join('%.3f' % s for s in secs):>28s}")
    model.forward = forward


def kernel_table(args, emit):
    from storm_amd import _lib as L
    from storm_amd import ops
    lib, dev = L.lib(), torch.device("cuda:0")
    B, n = args.rows, args.elements
    g = torch.Generator().manual_seed(1)
    x = torch.view_as_complex(torch.randn(B, n, 2, generator=g, dtype=torch.float64)).to(dev)
    xb = x * 1.01
    K = [torch.view_as_complex(torch.randn(B, n, 2, generator=g)).to(dev) for _ in range(13)]
    o64, o32 = torch.empty_like(x), torch.empty(B, n, dtype=torch.complex64, device=dev)
    out, scratch = torch.empty(2, B, dtype=torch.float64, device=dev), torch.empty(2 * ops.RK_ROW_BLOCKS * B, dtype=torch.float64, device=dev)
    cf = (C.c_double * 13)(*[0.1 * (j + 1) for j in range(13)])
    cg = (C.c_double * 13)(*[0.1 * (13 - j) for j in range(13)])
    h = (C.c_double * B)(*[-0.01] * B)
    p, r, st = L.ptr, ops._r, L.stream()

    def combine(entry, nt):
        kp = ops._kptrs(K[:nt])
        return lambda: getattr(lib, entry)(p(r(o64)), p(r(o32)), p(r(x)), kp, cf, nt, h, B, n, st)

    def sumsq(nt):
        kp = ops._kptrs(K[:nt])
        return lambda: lib.storm_rk_scaled_sumsq_rows(p(out), p(scratch), scratch.numel(), p(r(x)), p(r(xb)), kp, cf, nt, h, 1e-5, 1e-5, B, n, st)

    def pair(nt):
        kp = ops._kptrs(K[:nt])
        return lambda: lib.storm_rk_error_pair_rows(p(out), p(scratch), scratch.numel(), p(r(x)), p(r(xb)), kp, cf, cg, nt, None, 1e-5, 1e-5, B, n, st)

    def timed(fn):
        ms = []
        for w in range(args.reps + 1):                                  # (window 0 is the warm-up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                rc = fn()
            b.record()
            b.synchronize()
            assert rc == 0, lib.storm_last_error().decode()
            ms.append(a.elapsed_time(b) / args.inner)
        return statistics.median(ms[1:])
    emit(f"# the Runge-Kutta launches: {B} rows x {n} complex elements, outputs allocated once, {args.inner} launches queued between two device "
         f"events, median of {args.reps} windows; the 7-term entry points are this build's, the commit before was not built or timed")
    emit(f"{'launch':58s} {'us':>9s} {'MB moved':>9s} {'GB/s':>8s}")
    cases = [("storm_rk_combine_rows (7 terms)", combine("storm_rk_combine_rows", 7), 8 * 7 + 40)]
    cases += [(f"storm_rk_combine_rows_wide ({nt} terms)", combine("storm_rk_combine_rows_wide", nt), 8 * nt + 40) for nt in (7, 12, 13)]
    cases += [("storm_rk_scaled_sumsq_rows (7 terms, one sum)", sumsq(7), 8 * 7 + 32)]
    cases += [(f"storm_rk_error_pair_rows ({nt} terms, two sums)", pair(nt), 8 * nt + 32) for nt in (7, 13)]
    for name, fn, per_element in cases:
        ms, nbytes = timed(fn), B * n * per_element
        emit(f"{name:58s} {ms * 1e3:9.1f} {nbytes / 1e6:9.2f} {nbytes / ms / 1e6:8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-evals", type=int, default=2000, help="stop a run of the network table that needs more evaluations than this")
    ap.add_argument("--methods", nargs="+", default=list(METHODS), choices=METHODS)
    ap.add_argument("--tols", nargs="+", type=float, default=list(TOLS))
    ap.add_argument("--rows", type=int, default=BATCH)
    ap.add_argument("--elements", type=int, default=256 * 256)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ode_methods.py measures on the GPU: none found")
    out = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        out = open(args.out, "w")

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    emit(f"# tools/ode_methods.py on {torch.cuda.get_device_name(0)}")
    if not args.skip_kernels:
        kernel_table(args, emit)
    if not args.skip_network:
        network_table(args, emit)


if __name__ == "__main__":
    main()
