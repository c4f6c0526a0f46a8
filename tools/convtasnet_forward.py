"""One ConvTasNet forward at the default size (27 blocks' worth of kernels on a 4-s utterance) for a profiler to wrap:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o trace -- python tools/convtasnet_forward.py [--precision bf16] [--batch 1]

Seeded weights (tests/convtasnet_cases.py), a few untimed calls, then `--reps` timed ones; prints one JSON line with the mean wall time."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "fp16"])
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--seconds", type=float, default=4.0)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    from storm_amd.backbones.convtasnet import ConvTasNet
    from tests import convtasnet_cases as CC
    net = ConvTasNet()
    CC.fill(net)
    net = net.cuda().set_compute_dtype({"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.precision])
    x = (0.1 * torch.randn(a.batch, int(16000 * a.seconds), generator=torch.Generator().manual_seed(0))).cuda()
    for _ in range(2):
        y = net(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        y = net(x)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.reps * 1e3
    print(json.dumps(dict(what="convtasnet default forward", precision=a.precision, batch=a.batch, seconds=a.seconds, frames=int((y.shape[1] - 32) // 16 + 1),
                          ms_per_forward=round(ms, 3), finite=bool(torch.isfinite(y).all()))))


if __name__ == "__main__":
    main()
