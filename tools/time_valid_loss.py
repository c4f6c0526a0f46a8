"""Time ScoreModel.validation_loss at the bench shape (16 x 256 x 256, bf16, the 27.8 M `ncsnpp`) next to ONE score evaluation
(storm_ncsnpp_forward through model.forward) and the two new kernels alone: HIP events around repeated calls after a warm-up.

    python tools/time_valid_loss.py [--out profiles/r11_valid_loss.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import randomize  # noqa: E402
from storm_amd import ops  # noqa: E402
from storm_amd.model import ScoreModel  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps                                  # ms per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=20)
    args = p.parse_args()
    dev = torch.device("cuda:0")
    B, F, T = 16, 256, 256
    m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5)
    randomize(m, seed=0)
    m._error_loading_ema = True
    m = m.eval().to(dev)
    m.set_precision("bf16")
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g)).to(dev)
    y = x + (0.2 * torch.randn(B, 1, F, T, dtype=torch.complex64, generator=g)).to(dev)
    t = torch.linspace(0.05, 0.95, B)
    td = t.to(dev)
    std = m.sde._std(t).to(dev)
    mf = m.sde.mean_factor_rows(t).to(dev)
    score = m(x, td, y)
    n = F * T
    rows = [
        ("one score evaluation (model.forward -> storm_ncsnpp_forward)", timed(lambda: m(x, td, y), args.reps), None),
        ("validation_loss(seed=) (t on the host, perturb, one evaluation, loss)", timed(lambda: m.validation_loss(x, y, seed=3), args.reps), None),
        ("validation_loss(row_seeds=)", timed(lambda: m.validation_loss(x, y, row_seeds=list(range(1, B + 1))), args.reps), None),
        ("sde_perturb_rows, generated noise (reads 16, writes 8 bytes per complex element)",
         timed(lambda: ops.sde_perturb_rows(x, y, mf, std, 0, seed=3), 10 * args.reps), 24 * B * n),
        ("dsm_loss_rows 'mse', generated noise (reads 8 bytes per complex element)",
         timed(lambda: ops.dsm_loss_rows(score, std, kind="mse", seed=3), 10 * args.reps), 8 * B * n),
        ("pair_loss_rows 'mse' (reads 16 bytes per complex element)", timed(lambda: ops.pair_loss_rows(x, y, kind="mse"), 10 * args.reps), 16 * B * n),
    ]
    lines = [f"validation loss at the bench shape: {B} x {F} x {T} complex64, ncsnpp (27.8 M), bf16, {torch.cuda.get_device_name(0)}",
             f"HIP events around {args.reps} calls ({10 * args.reps} for the kernels alone) after 3 warm-up calls; ms per call", ""]
    for name, ms, nbytes in rows:
        bw = "" if nbytes is None else f"   {nbytes / ms / 1e9:7.2f} TB/s of algorithmic bytes (incl. launch and allocation)"
        lines.append(f"{ms:9.4f} ms  {name}{bw}")
    extra = rows[1][1] - rows[0][1]
    lines += ["", f"validation_loss - one evaluation = {extra:.4f} ms = {100 * extra / rows[0][1]:.2f} % of the evaluation"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
