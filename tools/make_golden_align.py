"""Fixture F26 (tests/golden/f26_align.npz): what the REFERENCE's util/other.py align and hp_filter return on the seeded inputs of
tests/align_cases.py.

    python tools/make_golden_align.py

Needs the reference checkout (oracle.ref_import: STORM_REFERENCE_ROOT); nothing of it is copied - the file holds
  align_shifts [cases]      the planted shifts (tests/align_cases.py: ALIGN_SHIFTS),
  align_l [cases]           the roll the reference applied: argmax(fftconvolve(ref, flip(y))) - (len(ref) - 1),
  align_out_sha [cases]     SHA-256 of the float32 array align(y, ref) returned,
  align_in_sha [cases]      SHA-256 of the float32 inputs (the test regenerates them from the seeds and compares),
  hp_out [3000]             hp_filter(x) with the reference's defaults (80 Hz, order 10, 16 kHz), float64,
  hp_in_sha                 SHA-256 of the float32 input.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402
from tests import align_cases as AC  # noqa: E402


def main():
    other = import_reference()["other"]
    ls, out_sha, in_sha = [], [], []
    for shift in AC.ALIGN_SHIFTS:
        y, ref = AC.align_inputs(shift)
        got = np.asarray(other.align(y.copy(), ref.copy()), dtype=np.float32)
        half = AC.ALIGN_L // 2                                                   # (one period of the roll: a roll by l is a roll by l +- L)
        moved = [l for l in range(-half, AC.ALIGN_L - half) if np.array_equal(got, np.roll(y, l))]
        assert len(moved) == 1, (shift, moved)
        dmin, c = AC.xcorr(y, ref)
        runner_up = np.sort(c)[-2] / c.max()
        print(f"shift {shift:5d}: the reference rolled by {moved[0]:5d}; runner-up of the restatement's c {runner_up:.3f} of the peak")
        ls.append(moved[0]); out_sha.append(AC.sha256(got)); in_sha.append(AC.sha256(y, ref))
    x = AC.hp_input()
    hp = np.asarray(other.hp_filter(x.copy()), dtype=np.float64)
    assert hp.shape == x.shape
    path = os.path.join(ROOT, "tests", "golden", "f26_align.npz")
    np.savez(path, align_shifts=np.array(AC.ALIGN_SHIFTS, dtype=np.int64), align_l=np.array(ls, dtype=np.int64), align_out_sha=np.array(out_sha),
             align_in_sha=np.array(in_sha), hp_out=hp, hp_in_sha=np.array(AC.sha256(x)))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
