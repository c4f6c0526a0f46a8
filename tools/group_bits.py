#!/usr/bin/env python
"""Fingerprint of the grouped evaluation (storm_ncsnpp_forward_group) for comparing two builds of the library bit for bit: one NCSNpp per case
is driven through forward_parts_group on seeded inputs; per case one line with storm_ncsnpp_group_workspace_bytes, the grouped launches of one
call and the sha256 of every problem's output bytes.  Two builds agree when their outputs diff empty.

    python tools/group_bits.py --sim                         # the host simulator (fp32 and bf16)
    STORM_LIB=/path/to/libstorm_hip.so python tools/group_bits.py   # that library on the GPU (default: the tree's), + the 27.8 M ncsnpp
"""
import ctypes as C
import hashlib
import sys

import torch

sys.path.insert(0, ".")
import storm_amd  # noqa: E402
from oracle import ncsnpp_ref as NR  # noqa: E402  (test infrastructure: seeded weights only)
from storm_amd import _lib as L  # noqa: E402
from storm_amd.backbones.ncsnpp import NCSNpp  # noqa: E402
from tests import option_nets as ON  # noqa: E402  (test infrastructure: seeded weights of the option nets)

GROUP_NET = dict(nf=64, ch_mult=(1, 3), num_res_blocks=1, attn_resolutions=(0,), image_size=16, input_channels=4)   # tests/test_net.py
SHAPES = {"gpu_list": [(2, 64), (1, 128), (3, 32)], "sim_list": [(1, 64), (2, 32), (1, 32)]}                       # test_forward_group_equals_per_problem_forwards
OPTION_SHAPES = {"gpu_list": [(2, 64), (1, 128)], "sim_list": [(1, 32), (1, 64)]}                                  # test_option_net_forward_group
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def seeded(kw, seed, dev):
    m = NCSNpp(**kw)
    m.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(**kw), seed=seed))
    return m.to(dev)


def case(name, m, F, shapes, dtype, dev):
    m.set_compute_dtype(dtype)
    g = torch.Generator().manual_seed(5)
    ins = [[(torch.randn(B, F, Tt, dtype=torch.complex64, generator=g) * 0.5).to(dev) for _ in range(2)] for B, Tt in shapes]
    ts = [(0.05 + 0.9 * torch.rand(B, generator=g)).to(dev) for B, _ in shapes]
    n0 = m.group_launches()
    outs = m.forward_parts_group(ins, ts)
    launches = m.group_launches() - n0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    P = len(shapes)
    Bs, Ts = (C.c_int * P)(*[b for b, _ in shapes]), (C.c_int * P)(*[t for _, t in shapes])
    with m._lock:
        ws = L.lib().storm_ncsnpp_group_workspace_bytes(m._get_handle(L.dt(dtype), dev), P, Bs, Ts, F)
    sha = " ".join(hashlib.sha256(torch.view_as_real(o).cpu().contiguous().numpy().tobytes()).hexdigest()[:16] for o in outs)
    print(f"{name} {NAMES[dtype]} {shapes}: workspace {ws} B, {launches} grouped launches, sha256 {sha}", flush=True)


def main():
    sim = "--sim" in sys.argv
    if sim:
        from tests.sim.simenv import load_sim
        load_sim()
        dev = torch.device("cpu")
    else:
        L.lib()
        dev = torch.device("cuda:0")
        print(f"library: {L.LIB_PATH}", file=sys.stderr)
    dtypes = [torch.float32, torch.bfloat16] if sim else [torch.float32, torch.bfloat16, torch.float16]   # (simulator: bf16 covers the 16-bit kernels)
    net = seeded(GROUP_NET, 9, dev)
    for inv in (0, 1):
        storm_amd.set_batch_invariant(bool(inv))
        for key, shapes in SHAPES.items():
            for dtype in dtypes:
                case(f"group_net invariant={inv} {key}", net, 16, shapes, dtype, dev)
    storm_amd.set_batch_invariant(False)
    cat = NCSNpp(**dict(ON.WIDE, progressive_combine="cat", fir=False, progressive="none"))
    ON.fill_module(cat)
    cat = cat.to(dev)
    for key, shapes in OPTION_SHAPES.items():
        for dtype in (torch.bfloat16, torch.float32):
            case(f"wide_cat {key}", cat, 16, shapes, dtype, dev)
    if not sim:
        full = seeded(dict(input_channels=4), 11, dev)
        for dtype in (torch.bfloat16, torch.float16):
            case("ncsnpp", full, 256, [(2, 256), (1, 512), (3, 320)], dtype, dev)


if __name__ == "__main__":
    main()
