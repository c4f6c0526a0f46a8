"""Frame-based measures on the device - segmental SNR, log-likelihood ratio, LPC cepstral distance (storm_lpc_measures_rows, storm_lpc_window
and their Python / command-line surfaces) - against the float64 numpy restatement of the definition in include/storm_hip.h
(tests/lpc_cases.py).  pysepm is installed on none of the project's machines: nothing here was compared with it.

The bound of every comparison with the restatement, per unit (dB, LLR, dB): max(16 x the largest |float64 - longdouble| of the restatement
over the case's frames, 1e-10) - the first term is measured on the host that runs the test, the floor is three orders above fp64 rounding
of 480-term sums and ten or more below any indexing error."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lpc_cases as LC
from tests.backend import dev  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
UNITS = ("seg_snr dB", "llr", "cd dB")


def _same(a, b):
    """bit-equal, NaN in the same places"""
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=-1234.5), torch.nan_to_num(b, nan=-1234.5)) and torch.equal(a.isnan(), b.isnan())


def _one(v, d):
    return T(np.ascontiguousarray(v, dtype=np.float32))[None].to(d)


def _call(x, y, fs, d):
    from storm_amd import ops
    out, fr, cnt = ops.lpc_measures_rows(_one(x, d), _one(y, d), fs=fs, frames=True, counts=True)
    assert out.dtype == fr.dtype == torch.float64 and cnt.dtype == torch.int32 and out.device.type == d.type
    return out[0].cpu().numpy(), fr[0].cpu().numpy(), cnt[0].tolist()


def _check(tag, got_row, got_frames, got_counts, ref):
    """device values against reference_xy's: counts exact, NaN in the same places, every unit within its bound; prints figure / bound"""
    f64, row, M, Mv, bound, _ = ref
    assert got_counts == [M, Mv], (tag, got_counts, M, Mv)
    assert got_frames.shape == f64.shape and (np.isnan(got_frames) == np.isnan(f64)).all(), tag
    assert (np.isnan(got_row) == np.isnan(row)).all(), (tag, got_row, row)
    for u, unit in enumerate(UNITS):
        ef = float(np.nanmax(np.abs(got_frames[:, u] - f64[:, u]))) if M and not np.isnan(f64[:, u]).all() else 0.0
        er = 0.0 if np.isnan(row[u]) else float(abs(got_row[u] - row[u]))
        print(f"lpc {tag} {unit}: frames {ef:.3e} row {er:.3e} / bound {bound[u]:.3e}")
        assert ef <= bound[u] and er <= bound[u], (tag, unit, ef, er, bound[u])


# ---- 1. the restatement's own LPC against an independent solver ----------------------------------------------------------------------------
def test_restatement_lpc_against_solve_toeplitz():
    """Levinson-Durbin of lpc_cases on the frames of the well-conditioned (30 dB) rows against scipy.linalg.solve_toeplitz of the normal
    equations R a = -r"""
    from scipy.linalg import solve_toeplitz
    n = 0
    for fs in LC.FS:
        W, H, P = LC.shape(fs)
        x, y = LC.pair(fs, 30, 2045)
        w = LC.window(fs)
        for m in range(LC.n_frames(2045, fs)):
            for v in (x, y):
                r = LC.autocorr(w * v[m * H:m * H + W].astype(np.float64), P)
                a = LC.levinson(r, P)
                want = solve_toeplitz(r[:P], -r[1:P + 1])
                assert np.abs(a[1:] - want).max() <= 1e-9 * np.abs(want).max(), (fs, m)
                n += 1
    assert n == 2 * (13 + 30 + 2)


def test_trim_count_is_the_published_rounding():
    assert [LC.n_keep(m) for m in (1, 2, 10, 11, 30, 100)] == [1, 2, 10, 10, 29, 95]
    assert all(LC.n_keep(m) == max(1, math.floor(0.95 * m + 0.5 + 1e-9)) for m in range(1, 400))


# ---- 2. measured cases -----------------------------------------------------------------------------------------------------------------------
def test_every_30_db_case_and_some_20_db_cases_are_measured():
    cases = LC.measured_cases()
    assert all(k in cases for k in LC.candidates() if k[1] == 30) and any(k[1] == 20 for k in cases)


@pytest.mark.parametrize("key", LC.measured_cases(), ids=lambda k: "-".join(str(v) for v in k))
def test_measured_cases(dev, key):
    """per-frame and row values of the seeded speech-like row with white noise at 30 / 20 dB, at the edge lengths of every rate, against the
    restatement.  Asserted on the reference before the kernel runs: at most 10 % of the frames sit at a clamp (a clamped frame hides its error)"""
    ref = LC.reference(key)
    assert ref[5].max() <= LC.CAP, (key, ref[5])
    assert ref[2] == LC.n_frames(key[2], key[0])
    x, y = LC.pair(*key)
    _check("-".join(str(v) for v in key), *_call(x, y, key[0], dev), ref)


def test_largest_window(dev):
    """fs = 68266 Hz: W = 2048, the largest window the library takes (the most LDS a workgroup asks for), three frames"""
    fs = 68266
    assert LC.shape(fs) == (2048, 512, 16)
    x = LC.speech_like(fs, 2048 + 3 * 512 + 5, 5)
    y = LC.add_noise(x, 30, 6)
    ref = LC.reference_xy(x, y, fs)
    assert ref[2] == 3 and ref[5].max() <= LC.CAP
    _check("68266-30-3589", *_call(x, y, fs, dev), ref)


# ---- 3. ragged batches and layout ----------------------------------------------------------------------------------------------------------
RAGGED = {16000: [4000, 1703, 599], 8000: [2045, 300, 1000], 44100: [5000, 1653, 3303]}


@pytest.mark.parametrize("fs", LC.FS)
def test_ragged_batch_of_three(dev, fs):
    """a batch of three rows with their own lengths (several tiles, one frame, none) against the restatement; every row is bit-equal to its
    own one-row call, and stays so at another row stride, from a misaligned view and with NaN past lengths[b]"""
    from storm_amd import ops
    lens = RAGGED[fs]
    Lw = max(lens)
    xs = [LC.speech_like(fs, n, 40 + k) for k, n in enumerate(lens)]
    ys = [LC.add_noise(v, 30, 50 + k) for k, v in enumerate(xs)]
    x, y = torch.zeros(3, Lw), torch.zeros(3, Lw)
    for k, n in enumerate(lens):
        x[k, :n], y[k, :n] = T(xs[k]), T(ys[k])
    x, y = x.to(dev), y.to(dev)
    out, fr, cnt = ops.lpc_measures_rows(x, y, lengths=lens, fs=fs, frames=True, counts=True)
    assert fr.shape == (3, LC.n_frames(Lw, fs), 3)
    for k, n in enumerate(lens):
        ref = LC.reference_xy(xs[k], ys[k], fs)
        M = ref[2]
        assert bool(fr[k, M:].isnan().all())                                  # past the row's own frames
        _check(f"{fs}-ragged-{n}", out[k].cpu().numpy(), fr[k, :M].cpu().numpy(), cnt[k].tolist(), ref)
        alone = ops.lpc_measures_rows(x[k:k + 1, :n], y[k:k + 1, :n], fs=fs, frames=True, counts=True)
        assert _same(alone[0][0], out[k]) and _same(alone[1][0], fr[k, :M]) and alone[2][0].tolist() == cnt[k].tolist()
    # another stride and a view that starts 4 bytes off a 16-byte boundary; NaN where no row may be read
    wide_x, wide_y = torch.full((3, Lw + 7), math.nan, device=dev), torch.full((3, Lw + 5), math.nan, device=dev)
    for k, n in enumerate(lens):
        wide_x[k, 1:1 + n], wide_y[k, 3:3 + n] = x[k, :n], y[k, :n]
    again = ops.lpc_measures_rows(wide_x[:, 1:1 + Lw], wide_y[:, 3:3 + Lw], lengths=lens, fs=fs, frames=True, counts=True)
    assert _same(again[0], out) and _same(again[1], fr) and torch.equal(again[2], cnt)
    # the order of the rows and the width of the batch change nothing
    back = ops.lpc_measures_rows(torch.flip(x, [0]), torch.flip(y, [0]), lengths=lens[::-1], fs=fs)
    assert _same(torch.flip(back, [0]), out)


# ---- 4. exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", LC.FS)
def test_identical_signals(dev, fs):
    """y = x: every frame is (35, 0, 0), and so is the row"""
    x = LC.speech_like(fs, RAGGED[fs][0], 3)
    row, fr, cnt = _call(x, x, fs, dev)
    M = LC.n_frames(len(x), fs)
    assert M > LC.shape(fs)[0] // 300 and cnt == [M, M]
    assert (fr == np.array([35.0, 0.0, 0.0])).all() and row.tolist() == [35.0, 0.0, 0.0]


@pytest.mark.parametrize("gain,snr", [(0.5, 20 * math.log10(2.0)), (-1.0, -20 * math.log10(2.0))])
def test_power_of_two_gain(dev, gain, snr):
    """y = 0.5 x and y = -x scale every lag exactly: both recursions are the same bits, LLR and CD are exactly 0; the segmental SNR is
    +6.0206 / -6.0206 dB within the bound"""
    x = LC.speech_like(16000, 2045, 3)
    y = (gain * x).astype(np.float32)
    row, fr, cnt = _call(x, y, 16000, dev)
    ref = LC.reference_xy(x, y, 16000)
    assert cnt == [13, 13] and (fr[:, 1:] == 0.0).all() and row[1] == 0.0 and row[2] == 0.0
    assert np.abs(fr[:, 0] - snr).max() <= ref[4][0] and abs(row[0] - snr) <= ref[4][0] and abs(snr) > 6.02
    _check(f"gain {gain}", row, fr, cnt, ref)


def test_silent_clean_signal(dev):
    """clean all zeros: every frame's segmental SNR is -10, every frame is void, LLR and CD are NaN"""
    y = LC.speech_like(16000, 2045, 3)
    row, fr, cnt = _call(np.zeros_like(y), y, 16000, dev)
    assert cnt == [13, 0] and (fr[:, 0] == -10.0).all() and np.isnan(fr[:, 1:]).all()
    assert row[0] == -10.0 and math.isnan(row[1]) and math.isnan(row[2])
    row, fr, cnt = _call(y, np.zeros_like(y), 16000, dev)                     # a silent estimate: void as well, 0 dB
    assert cnt == [13, 0] and np.isnan(fr[:, 1:]).all() and np.abs(fr[:, 0]).max() <= 1e-10 and math.isnan(row[1])


def test_zeroed_stretch_gives_void_frames(dev):
    """a row whose clean signal is zero over a stretch: the frames inside it are NaN in LLR and CD, counted out of M' (exactly the
    restatement's count) and left out of the trimmed means - a void frame counted as 0 would lower both"""
    x = LC.speech_like(16000, 4000, 3).copy()
    y = LC.add_noise(x, 30, 4)
    x[1000:2500] = 0.0
    ref = LC.reference_xy(x, y, 16000)
    void = np.isnan(ref[0][:, 1])
    assert ref[2] == 29 and 5 <= void.sum() == 29 - ref[3] <= 12 and ref[1][1] > 0.01
    row, fr, cnt = _call(x, y, 16000, dev)
    assert (np.isnan(fr[:, 1]) == void).all() and (fr[void, 0] == -10.0).all()
    _check("zeroed stretch", row, fr, cnt, ref)


def test_single_sample_frame(dev):
    """a clean frame that holds one nonzero sample: a_c = (1, 0, ...) and its cepstrum is 0, so LLR = ln(sum a_p^2) and CD comes from the
    processed signal's cepstrum alone"""
    fs = 16000
    W, H, P = LC.shape(fs)
    y = LC.speech_like(fs, W + H, 3)
    x = np.zeros_like(y)
    x[200] = 0.25
    r = LC.autocorr(LC.window(fs) * y[:W].astype(np.float64), P)
    ap = LC.levinson(r, P)
    cp = LC.cepstrum(ap, P)
    llr = min(max(math.log(float(np.dot(ap, ap))), 0.0), 2.0)
    cd = min(10.0 / math.log(10.0) * math.sqrt(2.0 * float(np.dot(cp[1:], cp[1:]))), 10.0)
    row, fr, cnt = _call(x, y, fs, dev)
    ref = LC.reference_xy(x, y, fs)
    assert cnt == [1, 1] and abs(fr[0, 1] - llr) <= ref[4][1] and abs(fr[0, 2] - cd) <= ref[4][2] and 0.0 < llr and cd > 0.0
    _check("single sample", row, fr, cnt, ref)
    row, fr, cnt = _call(x, (0.5 * x).astype(np.float32), fs, dev)            # against itself at half the gain: exactly 0
    assert cnt == [1, 1] and fr[0, 1] == 0.0 and fr[0, 2] == 0.0


@pytest.mark.parametrize("fs", LC.FS)
def test_row_shorter_than_a_window(dev, fs):
    """L < W: M = 0, three NaN, nothing per frame"""
    x = LC.speech_like(fs, LC.shape(fs)[0] - 1, 3)
    row, fr, cnt = _call(x, x, fs, dev)
    assert cnt == [0, 0] and fr.shape == (0, 3) and np.isnan(row).all()


# ---- 5. clamps and trim ----------------------------------------------------------------------------------------------------------------------
def test_lowpassed_estimate_sits_at_the_clamps(dev):
    """a 4th-order Butterworth low-pass at half Nyquist as the estimate: the LPC envelopes part by more than the clamps allow"""
    x = (0.1 * np.random.default_rng(11).standard_normal(4000)).astype(np.float32)
    y = LC.lowpassed(x)
    ref = LC.reference_xy(x, y, 16000)
    assert (ref[0][:, 1] == 2.0).all() and (ref[0][:, 2] == 10.0).all()
    row, fr, cnt = _call(x, y, 16000, dev)
    assert (fr[:, 1] == 2.0).all() and (fr[:, 2] == 10.0).all() and row[1] == 2.0 and row[2] == 10.0
    _check("lowpassed", row, fr, cnt, ref)


@pytest.mark.parametrize("frames", [1, 10, 11, 30])
def test_trim_edges(dev, frames):
    """rows cut to M' = 1, 10, 11, 30 frames, the rounding edges of n_keep = 1, 10, 10, 29; counts=True returns (M, M')"""
    from storm_amd import ops
    W, H, _ = LC.shape(8000)
    n = W + frames * H + 7
    x = LC.speech_like(8000, n, 21)
    y = LC.add_noise(x, 20, 22)
    ref = LC.reference_xy(x, y, 8000)
    assert ref[2] == ref[3] == frames and LC.n_keep(frames) == {1: 1, 10: 10, 11: 10, 30: 29}[frames]
    row, fr, cnt = _call(x, y, 8000, dev)
    _check(f"trim {frames}", row, fr, cnt, ref)
    if LC.n_keep(frames) < frames:                                            # the trim is seen: the untrimmed mean lies outside the bound
        assert abs(float(np.mean(ref[0][:, 1])) - ref[1][1]) > 1e3 * ref[4][1]
    out, counts = ops.lpc_measures_rows(_one(x, dev), _one(y, dev), fs=8000, counts=True)
    assert counts.tolist() == [[frames, frames]] and out.shape == (1, 3)


def test_long_row_past_the_frames_kept_in_registers(dev):
    """a row of more than 32 x 256 frames (the row kernel keeps that many in registers and reads the rest from memory in every counting pass)
    with a silent stretch: the counts, the mean and the two trimmed means are those of the restatement's row step on the device's own
    per-frame values (their parity is the measured cases' business: 8300 frames of the restatement would take a minute)"""
    from storm_amd import ops
    W, H, _ = LC.shape(8000)
    n = W + 8300 * H + 11
    x = LC.speech_like(8000, n, 31).copy()
    y = LC.add_noise(x, 20, 32)
    x[100000:103000] = 0.0
    out, fr, cnt = ops.lpc_measures_rows(_one(x, dev), _one(y, dev), fs=8000, frames=True, counts=True)
    frames = fr[0].cpu().numpy()
    row, M, Mv = LC.row_values(frames)
    assert cnt.tolist() == [[M, Mv]] and M == 8300 and 8300 - 50 <= Mv < 8300 - 40 and LC.n_keep(Mv) < Mv - 400
    got = out[0].cpu().numpy()
    for u, unit in enumerate(UNITS):
        print(f"lpc long row {unit}: row {abs(got[u] - row[u]):.3e} / bound {LC.FLOOR:.3e}")
        assert abs(got[u] - row[u]) <= LC.FLOOR
    ok = ~np.isnan(frames[:, 1])
    assert abs(float(np.mean(frames[ok, 2])) - row[2]) > 1e-3                 # (the trim is seen)


# ---- 6. the window ---------------------------------------------------------------------------------------------------------------------------
def test_window_table(dev):
    """ops.lpc_window is the header's w[n] (the library's cos against numpy's: a few units in the last place), symmetric and below 1"""
    from storm_amd import _lib, ops
    for fs in LC.FS + (68266,):
        w = ops.lpc_window(fs, dev)
        want = LC.window(fs)
        assert w.dtype == torch.float64 and w.device.type == dev.type and w.shape == (LC.shape(fs)[0],)
        assert np.abs(w.cpu().numpy() - want).max() <= 4 * 2.0 ** -53 and float(w.max()) <= 1.0 and float(w.min()) > 0.0
        w[0] = 7.0                                                            # a copy: the cached table stays as the library wrote it
        assert float(ops.lpc_window(fs, dev)[0]) < 1.0
    lib = _lib.lib()
    buf = torch.full((480,), 7.0, dtype=torch.float64)
    assert lib.storm_lpc_window(16000, buf.data_ptr(), 479) < 0 and "capacity 479" in lib.storm_last_error().decode()
    assert bool((buf == 7.0).all())
    assert lib.storm_lpc_window(16000, None, 480) < 0 and "null pointer" in lib.storm_last_error().decode()
    assert lib.storm_lpc_window(16000, buf.data_ptr(), 480) == 480 and np.abs(buf.numpy() - LC.window(16000)).max() <= 4 * 2.0 ** -53


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument(dev):
    from storm_amd import _lib, ops
    from storm_amd._lib import StormError
    x = torch.zeros(2, 1000, device=dev)
    with pytest.raises(ValueError, match="lpc_measures_rows"):
        ops.lpc_measures_rows(x, x[:, :999])
    with pytest.raises(ValueError, match="y is"):
        ops.lpc_measures_rows(x, x.double())
    with pytest.raises(ValueError, match="lengths"):
        ops.lpc_measures_rows(x, x, lengths=[1000])
    with pytest.raises(ValueError, match="lengths"):
        ops.lpc_measures_rows(x, x, lengths=[1000, 1001])
    for fs in (100, 96000):                                                  # W = 3 <= 2 P;  W = 2880 > 2048
        with pytest.raises(StormError, match=f"fs={fs}"):
            ops.lpc_measures_rows(x, x, fs=fs)
        with pytest.raises(StormError, match=f"fs={fs}"):
            ops.lpc_window(fs)
    lib = _lib.lib()
    q = lib.storm_lpc_measures_scratch_bytes
    assert q(2, 1000, 16000) == 2 * 8 + 2 * 4 * 37 * 8 and q(3, 479, 16000) == 3 * 8 and q(1, 300, 8000) == 8 + 37 * 8     # (3 numbers + 2 x 17 lags per frame)
    assert 0 == q(0, 1000, 16000) == q(65536, 1000, 16000) == q(1, 0, 16000) == q(1, 2 ** 30 + 1, 16000) == q(1, 1000, 100) == q(1, 1000, 96000)
    need = q(2, 1000, 16000)
    out = torch.full((2, 3), 7.0, dtype=torch.float64, device=dev)
    ws = torch.full((need // 8 + 1,), 7.0, dtype=torch.float64, device=dev)
    win = ops.lpc_window(16000, dev)
    p = x.data_ptr()

    def call(a=p, b=p, w=win.data_ptr(), o=out.data_ptr(), s=ws.data_ptr(), bytes_=need, B=2, L=1000, strides=(1000, 1000), fs=16000):
        return lib.storm_lpc_measures_rows(a, b, w, o, None, s, bytes_, B, L, *strides, None, fs, _lib.stream())
    for kw, word in ((dict(a=None), "null pointer"), (dict(b=None), "null pointer"), (dict(w=None), "null pointer"), (dict(o=None), "null pointer"),
                     (dict(s=None), "null pointer"), (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(L=0), "L=0"), (dict(L=2 ** 30 + 1), "L="),
                     (dict(bytes_=need - 8), "scratch"), (dict(s=ws.data_ptr() + 4), "8-byte aligned"), (dict(fs=100), "fs=100"),
                     (dict(fs=96000), "fs=96000"), (dict(strides=(999, 1000)), "strides 999"), (dict(strides=(1000, 999)), "strides 1000 999")):
        assert call(**kw) != 0 and word in lib.storm_last_error().decode(), kw
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all())              # no kernel ran
    assert call() == 0 and out[:, 0].tolist() == [-10.0, -10.0] and bool(out[:, 1:].isnan().all())      # (all-zero rows)
    assert ws[:2].view(torch.int32).tolist() == [4, 0, 4, 0]


# ---- 8. the Python and command-line surfaces ---------------------------------------------------------------------------------------------
def _files(n, seed):
    """(clean, noisy, estimate) of n samples at 16 kHz"""
    s = LC.speech_like(16000, n, seed)
    noisy = LC.add_noise(s, 10, seed + 1)
    return T(s), T(noisy), T(LC.add_noise(s, 25, seed + 2))


def test_util_other_lpc_measures(dev):
    """util.other.lpc_measures in stoi's calling convention: 1-D numpy -> three floats equal to the batch call's row; [B, L] -> three fp64
    tensors; seg_snr / llr / cepstral_distance are its elements"""
    from storm_amd import ops
    from storm_amd.util import other as O
    s, _, e = _files(2045, 30)
    want = ops.lpc_measures_rows(s[None].to(dev), e[None].to(dev))
    got = O.lpc_measures(s.numpy(), e.numpy()) if dev.type == "cpu" else O.lpc_measures(s.numpy(), e.to(dev))
    assert all(isinstance(v, float) for v in got) and list(got) == want[0].tolist() and got[1] > 0.0
    assert (O.seg_snr(s.to(dev), e.to(dev)), O.llr(s.to(dev), e.to(dev)), O.cepstral_distance(s.to(dev), e.to(dev))) == got
    rows = O.lpc_measures(torch.stack([s, e]).to(dev), torch.stack([e, s]).to(dev), lengths=[2045, 700])
    assert len(rows) == 3 and all(r.shape == (2,) and r.dtype == torch.float64 and r.device.type == dev.type for r in rows)
    assert [float(r[0]) for r in rows] == list(got)
    at8k = O.lpc_measures(s.to(dev), e.to(dev), fs=8000)
    assert at8k == tuple(ops.lpc_measures_rows(s[None].to(dev), e[None].to(dev), fs=8000)[0].tolist()) and at8k != got


def test_score_batch_lpc(dev):
    """score_batch(lpc=True): exactly the three extra keys, the separate ops call on (clean, estimate) bit for bit, on what hp= and align=
    leave; every other key keeps its bits and, without the keyword, the key set is the one of before"""
    from storm_amd import ops
    from storm_amd.util.inference import METRIC_KEYS, score_batch
    lens = [2000, 1500]
    x, y, e = (torch.zeros(2, 2000) for _ in range(3))
    for k, n in enumerate(lens):
        x[k, :n], y[k, :n], e[k, :n] = _files(n, 70 + k)
    late = torch.zeros_like(e)
    late[:, 3:] = e[:, :-3]                                                  # three samples late
    x, y, e, late = (v.to(dev) for v in (x, y, e, late))
    keys = ("seg_snr", "llr", "cd")
    cols = lambda d: torch.stack([d[k] for k in keys], dim=1)                # noqa: E731
    plain = score_batch(x, y, e, lengths=lens)
    assert list(plain) == ["si_sdr", "si_sir", "si_sar", "lsd", "isnr"] == list(METRIC_KEYS)
    got = score_batch(x, y, e, lengths=lens, lpc=True)
    assert list(got) == list(plain) + list(keys) and all(_same(got[k], plain[k]) for k in plain)
    assert _same(cols(got), ops.lpc_measures_rows(x, e, lengths=lens))
    assert _same(cols(score_batch(x, y, e, lengths=lens, lpc=True, fs=8000)), ops.lpc_measures_rows(x, e, lengths=lens, fs=8000))
    al = score_batch(x, y, late, lengths=lens, align=True, lpc=True)
    back, _ = ops.xcorr_lag_rows(late, x, lengths=lens, ref_lengths=lens)
    assert al["lag"].tolist() == [3, 3] and list(al)[-4:] == list(keys) + ["lag"]
    assert _same(cols(al), ops.lpc_measures_rows(x, ops.shift_rows(late, back, lengths=lens, wrap=False), lengths=lens))
    sos = ops.butter_sos(10, 80 / 16000 * 2)
    f = [ops.sosfilt_rows(v, sos, lengths=lens, out_dtype=torch.float32) for v in (x, e)]
    assert _same(cols(score_batch(x, y, e, lengths=lens, hp=80, lpc=True)), ops.lpc_measures_rows(f[0], f[1], lengths=lens))


def test_evaluate_model_lpc(dev, golden):
    """evaluate_model(metrics=True, lpc=True) on F10's pairs: the sixth element gains seg_snr, llr, cd, the means of the files' own one-row
    calls (without lpc its keys are the ones of before: tests/test_stoi.py and tests/test_metrics.py hold them)"""
    from oracle import ncsnpp_ref as NR
    from storm_amd import ops
    from storm_amd.model import ScoreModel
    from storm_amd.util.inference import METRIC_KEYS, evaluate_model
    g = golden["f10_eval"]
    m = ScoreModel(backbone="ncsnpp", sde="ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5, spec_factor=0.15, spec_abs_exponent=0.5, nf=8)
    m.dnn.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=51))
    m.eval(no_ema=True)
    m = m.to(dev)
    pairs = [(T(g[f"eval_clean{i}"]), T(g[f"eval_noisy{i}"])) for i in range(3)]
    noises = [T(g[f"eval_noise{i}"]) for i in range(3)]

    def noise_for(ids):
        it = iter(range(noises[0].shape[0]))
        return lambda: torch.cat([noises[i][next(it)] for i in ids], 0).to(dev)
    kw = dict(audio=True, pairs=pairs, batch=2, noise_for=noise_for, N=1)    # (one reverse step: the simulator walks every lane)
    full = evaluate_model(m, 3, metrics=True, lpc=True, **kw)
    assert sorted(full[5]) == sorted(METRIC_KEYS + ("seg_snr", "llr", "cd"))
    each = torch.cat([ops.lpc_measures_rows(pairs[i][0].to(dev), full[4][1][i][None].to(dev)).cpu() for i in range(3)])
    assert not bool(each.isnan().any())
    for u, k in enumerate(("seg_snr", "llr", "cd")):
        assert abs(full[5][k] - float(each[:, u].mean())) <= 1e-12, k


@pytest.mark.gpu
def test_calc_metrics_cli_lpc(tmp_path, monkeypatch):
    """calc_metrics.py --lpc on three short files (its main() under the command line's argv, as tests/test_bss_eval.py runs it): the columns
    seg_snr,llr,cd stand last (before lag), a line does not depend on --batch, the values are score_batch's per file, the averages list
    them, and without the flag the files are the flagless run's byte for byte"""
    from scipy.io import wavfile

    import calc_metrics
    from storm_amd.util.inference import score_batch
    from tests.backend import setup_backend
    setup_backend("hip")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "plain", "plain2", "b1", "b3", "all")}
    for d in dirs.values():
        os.makedirs(d)
    triples = {}
    for name, n in (("a.wav", 6000), ("b.wav", 5700), ("c.wav", 5000)):
        triples[name] = _files(n, n)
        for key, w in [("clean", triples[name][0]), ("noisy", triples[name][1])] + [(k, triples[name][2]) for k in ("plain", "plain2", "b1", "b3", "all")]:
            wavfile.write(os.path.join(dirs[key], name), 16000, w.numpy().astype(np.float32))
    runs = {"plain": [], "plain2": ["--batch", "2"], "b1": ["--lpc", "--batch", "1"], "b3": ["--lpc", "--batch", "3"],
            "all": ["--lpc", "--bss", "64", "--align", "--hp-filter", "--batch", "2"]}
    for key, extra in runs.items():
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs[key]] + extra)
        calc_metrics.main()
    raw = lambda key, f: open(os.path.join(dirs[key], f), "rb").read()      # noqa: E731
    read = lambda key, f="_results.csv": raw(key, f).decode("utf-8").splitlines()    # noqa: E731
    assert raw("plain", "_results.csv") == raw("plain2", "_results.csv") and raw("plain", "_avg_results.txt") == raw("plain2", "_avg_results.txt")
    head = read("plain")[0].split(",")
    assert head[:7] == ["Filename", "Length", "iSNR", "si_sdr", "si_sir", "si_sar", "lsd"] and not any(c in head for c in ("seg_snr", "llr", "cd"))
    assert read("b1") == read("b3") and read("b1")[0].split(",") == head + ["seg_snr", "llr", "cd"]
    assert [ln.split(",")[:-3] for ln in read("b1")[1:]] == [ln.split(",") for ln in read("plain")[1:]]
    assert read("b1", "_avg_results.txt")[:-3] == read("plain", "_avg_results.txt")
    assert [ln.split(":")[0] for ln in read("b1", "_avg_results.txt")[-3:]] == ["seg_snr", "llr", "cd"]
    assert read("all")[0].split(",")[-7:] == ["bss_sdr", "bss_sir", "bss_sar", "seg_snr", "llr", "cd", "lag"]
    dev_ = torch.device("cuda:0")
    for key, kw, at in (("b1", {}, -3), ("all", dict(align=True, hp=80.0), -4)):
        for line in read(key)[1:]:
            cells = line.split(",")
            s, n, e = (w.to(dev_)[None] for w in triples[cells[0]])
            want = score_batch(s, n, e, lpc=True, **kw)
            assert cells[at:at + 3 or None] == [f"{float(want[k][0]):.6f}" for k in ("seg_snr", "llr", "cd")], (key, line)
    vals = np.array([[float(c) for c in ln.split(",")[-3:]] for ln in read("b1")[1:]])
    for u, ln in enumerate(read("b1", "_avg_results.txt")[-3:]):
        assert ln == f"{('seg_snr', 'llr', 'cd')[u]}: {vals[:, u].mean():.6f} ± {vals[:, u].std():.6f}"


# ---- 9. the kernels under the simulator's skewed wave schedules --------------------------------------------------------------------------
SKEWED = ["tests/test_lpc_measures.py::test_measured_cases[sim-44100-30-2045]",         # two frames: two of the four waves have one, > 64 KiB of LDS
          "tests/test_lpc_measures.py::test_measured_cases[sim-16000-30-2045]"]         # 13 frames: a full tile and a tile of five


@pytest.mark.parametrize("waves", ["reverse", "first", "last", "seed:1"])
def test_kernels_under_skewed_wave_schedules(waves):
    """the frame and the row kernel with the simulator's waves run in another order (STORM_SIM_WAVES, read when the simulation is loaded: a
    process of its own, as tests/test_sim_schedules.py runs its selection): the two smallest multi-frame cases pass"""
    env = dict(os.environ, PYTHONPATH=ROOT, STORM_SIM_WAVES=waves, STORM_TEST_WORKERS="2")
    env.pop("STORM_SIM_DMA", None)
    r = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(ROOT, t) for t in SKEWED] + ["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(SKEWED) and "skipped" not in r.stdout, r.stdout[-1000:]
