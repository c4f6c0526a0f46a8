"""TEST INFRASTRUCTURE: run the hazard zoo (tests/sim/hazard_zoo.cpp) under the schedule this process was started with.

STORM_SIM_WAVES / STORM_SIM_DMA are fixed per loaded simulator library, so tests/test_sim_schedules.py starts
`python -m tests.sim.zoo` once per combination and reads the JSON it prints: {kernel: {"correct": [...], "broken": [...]}}."""
import ctypes
import json

import numpy as np

NTILES = 4
# kernel -> words of input per tile, words of output
KERNELS = {"raw_below": (64, 64), "raw_below_busy": (64, 64), "raw_above_busy": (64, 64),
           "war_ring": (128, 128), "dma_war": (512, 128), "dma_raw": (512, 128)}


def source(kernel):
    """The kernel's input: distinct positive words, so that a stale, zero or too-new word never equals the right one."""
    words, _ = KERNELS[kernel]
    ntiles = 1 if kernel.startswith("raw") else NTILES
    return (np.arange(1, ntiles * words + 1, dtype=np.int64) * 7919 % 1000003).astype(np.int32).reshape(ntiles, words)


def run(lib, kernel, broken):
    src = source(kernel)
    out = np.zeros(128, dtype=np.uint32)
    rc = lib.storm_sim_zoo(kernel.encode(), int(broken), src.ctypes.data_as(ctypes.c_void_p), src.shape[0], out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, kernel
    return out[:KERNELS[kernel][1]].tolist()


def main():
    from tests.sim.build_sim import build
    lib = ctypes.CDLL(build())
    lib.storm_sim_zoo.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    print(json.dumps({k: {"correct": run(lib, k, False), "broken": run(lib, k, True)} for k in KERNELS}))


if __name__ == "__main__":
    main()
