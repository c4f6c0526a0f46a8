"""Misaligned audio on the device: the delay search (storm_xcorr_lag_rows), the shift (storm_shift_rows), the biquad cascade
(storm_sosfilt_rows), the Butterworth design (storm_butter_sos) and their Python / command-line surfaces - against the numpy restatements
of tests/align_cases.py, scipy.signal and the reference's own align / hp_filter (fixture F26, tools/make_golden_align.py)."""
import os
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

from tests import align_cases as AC
from tests.backend import dev, switch  # noqa: F401

T = torch.from_numpy
ULP2 = float(np.spacing(2.0))                                               # one unit in the last place of 2.0: 4.44e-16
# storm_butter_sos against scipy.signal.butter(order, wn, 'hp', output='sos') over orders {2, 4, 10} x {50, 80, 300 Hz at 16 kHz, 80 Hz at
# 48 kHz}: the largest coefficient difference measured on the build machine is 1.5 units in the last place of 2.0 (order 10 at 50 and 80 Hz,
# order 2 at 80 Hz; most entries 0 to 1).  Host code: the bound is 4 x that, the margin covers another libm's tan / cos.
DESIGN_TOL = 4 * 1.5 * ULP2
# hp_filter end to end (the library's own sections through the kernel, fp64 out) against the reference's hp_filter output of fixture F26,
# relative to the output's largest magnitude: measured 6.34e-14 on the host simulation (the 1.5-ulp coefficient differences through a 10th
# order recursion over 3000 samples; the kernel itself is bit-equal to scipy.signal.sosfilt on equal sections).  The bound is 4 x that.
HP_TOL = 4 * 6.34e-14


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(rows, d, width=None, junk=0.0):
    """fp32 arrays -> a [B, width] batch on d (junk past every row's length) and the lengths"""
    lens = [len(r) for r in rows]
    out = torch.full((len(rows), width or max(lens)), junk, dtype=torch.float32)
    for k, r in enumerate(rows):
        out[k, :lens[k]] = T(np.ascontiguousarray(r))
    return out.to(d), lens


# ---- 1. delay search ----------------------------------------------------------------------------------------------------------------------
def test_tile_size_is_the_header_s():
    from storm_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "storm_hip.h")).read()
    assert f"#define STORM_XCORR_TILE {AC.TILE}\n" in text and _lib.XCORR_TILE == AC.TILE


@pytest.mark.parametrize("L", AC.LENGTHS)
def test_planted_delays(dev, L):
    """every planted delay of this length (0, +-1, +-37, +-500, the two extremes as single samples at the ends, both sides of every lag-tile
    boundary) as ONE batch: lag equals and peak is bit-equal to the restatement, which finds the planted delay"""
    from storm_amd import ops
    delays = [d for (n, d) in AC.delay_cases() if n == L]
    pairs = [AC.planted(L, d) for d in delays]
    y, _ = _batch([p[0] for p in pairs], dev)
    r, _ = _batch([p[1] for p in pairs], dev)
    lag, peak = ops.xcorr_lag_rows(y, r)
    assert lag.dtype == torch.int32 and peak.dtype == torch.float64
    lag, peak = lag.cpu().numpy(), peak.cpu().numpy()
    for k, d in enumerate(delays):
        el, ep = AC.lag_peak(*pairs[k])
        assert el == d, (L, d, el)
        assert lag[k] == el and _bits(peak[k]) == _bits(ep), (L, d, lag[k], peak[k], ep)


@pytest.mark.parametrize("L,d,max_lag", [(1000, 500, 0), (1000, 500, 100), (4097, -500, 37), (4097, 1025, 1024), (65, -37, 64), (65, 1, 1000)])
def test_bounded_search(dev, L, d, max_lag):
    """max_lag = 0, smaller than the true delay (the best lag in range by the restatement), and wider than the row"""
    from storm_amd import ops
    y, r = AC.planted(L, d)
    lag, peak = ops.xcorr_lag_rows(T(y)[None].to(dev), T(r)[None].to(dev), max_lag=max_lag)
    el, ep = AC.lag_peak(y, r, max_lag)
    assert abs(el) <= max_lag and (el == d) == (abs(d) <= max_lag)
    assert int(lag[0]) == el and _bits(peak.cpu().numpy()[0]) == _bits(ep)


def test_tie_zero_row_and_unequal_lengths(dev):
    from storm_amd import ops
    # a tie: ref holds two equal impulses, c[10] == c[40] - the smaller lag wins
    y, r = np.zeros(100, np.float32), np.zeros(100, np.float32)
    y[10], r[20], r[50] = 3.0, 0.5, 0.5
    lag, peak = ops.xcorr_lag_rows(T(y)[None].to(dev), T(r)[None].to(dev))
    dmin, c = AC.xcorr(y, r)
    assert c[10 - dmin] == c[40 - dmin] == c.max() and (int(lag[0]), float(peak[0])) == (10, 1.5)
    # an all-zero row: the smallest lag of the range
    z = torch.zeros(1, 70, device=dev)
    for ml, want in ((None, -69), (5, -5), (0, 0)):
        lag, peak = ops.xcorr_lag_rows(z, z, max_lag=ml)
        assert (int(lag[0]), float(peak[0])) == (want, 0.0)
    # unequal lengths, either way round
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(300).astype(np.float32), np.zeros(1000, np.float32)
    b[417:717] = a
    for y, r in ((a, b), (b, a)):
        lag, peak = ops.xcorr_lag_rows(T(y)[None].to(dev), T(r)[None].to(dev))
        el, ep = AC.lag_peak(y, r)
        assert abs(el) == 417 and int(lag[0]) == el and _bits(peak.cpu().numpy()[0]) == _bits(ep)


@pytest.mark.parametrize("R", [2, 4, 8])
def test_lags_per_thread_change_no_bit(dev, switch, R):
    """the launcher keeps 8, 4 or 2 lags per thread by the size of the launch (here forced through the library's test switch): a lag's
    chain is the same chain, so every choice gives the restatement's bits - tile boundaries, the extremes, a ragged batch"""
    from storm_amd import ops
    switch("STORM_XCORR_LAGS", R)
    for L, delays in ((4097, (0, -500, 1023, 1024, -1025, 4096, -4096)), (65, (0, 1, -37, 64))):
        pairs = [AC.planted(L, d) for d in delays]
        lag, peak = ops.xcorr_lag_rows(_batch([p[0] for p in pairs], dev)[0], _batch([p[1] for p in pairs], dev)[0])
        for k, d in enumerate(delays):
            el, ep = AC.lag_peak(*pairs[k])
            assert int(lag[k]) == el == d and _bits(peak.cpu().numpy()[k]) == _bits(ep), (R, L, d)
    ys, rs = [AC.planted(1000, 37)[0], AC.planted(65, 1)[0]], [AC.planted(1000, 37)[1][:700], AC.planted(65, 1)[1]]
    yb, ylen = _batch(ys, dev, width=1100, junk=7.0)
    rb, rlen = _batch(rs, dev, width=1200, junk=-3.0)
    lag, peak = ops.xcorr_lag_rows(yb, rb, lengths=ylen, ref_lengths=rlen, max_lag=300)
    for k in range(2):
        el, ep = AC.lag_peak(ys[k], rs[k], 300)
        assert int(lag[k]) == el and _bits(peak.cpu().numpy()[k]) == _bits(ep), (R, k)


def test_ragged_batch_equals_one_row_calls(dev):
    """three rows of different lengths (y and ref lengths differ too) in buffers wider than the rows, row strides wider than the batch,
    non-zero junk past every length: every row is bit-equal to its own one-row call on the trimmed row and to the restatement"""
    from storm_amd import ops
    ys = [AC.planted(1000, 37)[0], AC.planted(4097, -500)[0], AC.planted(65, 1)[0]]
    rs = [AC.planted(1000, 37)[1], AC.planted(4097, -500)[1][:3000], np.concatenate([AC.planted(65, 1)[1]] * 2)]
    yb, ylen = _batch(ys, dev, width=4200, junk=7.0)
    rb, rlen = _batch(rs, dev, width=4300, junk=-3.0)
    lag, peak = ops.xcorr_lag_rows(yb[:, :4100], rb[:, :4097], lengths=ylen, ref_lengths=rlen)
    for k in range(3):
        l1, p1 = ops.xcorr_lag_rows(T(ys[k])[None].to(dev), T(rs[k])[None].to(dev))
        el, ep = AC.lag_peak(ys[k], rs[k])
        assert int(lag[k]) == int(l1[0]) == el
        assert _bits(peak.cpu().numpy()[k]) == _bits(p1.cpu().numpy()[0]) == _bits(ep)
    with pytest.raises(ValueError, match="lengths"):
        ops.xcorr_lag_rows(yb, rb, lengths=[1000, 5000, 65])


@pytest.mark.parametrize("shift", AC.ALIGN_SHIFTS)
def test_align_equals_the_reference(dev, golden, shift):
    """util.other.align against the reference's own align (fixture F26) on inputs with a clear peak - its fftconvolve rounds differently, so
    the restatement's runner-up is asserted to be at most half the peak before anything is compared"""
    from storm_amd.util.other import align
    g = golden["f26_align"]
    k = list(g["align_shifts"]).index(shift)
    y, ref = AC.align_inputs(shift)
    assert AC.sha256(y, ref) == str(g["align_in_sha"][k])
    dmin, c = AC.xcorr(y, ref)
    assert np.sort(c)[-2] <= 0.5 * c.max()
    assert int(g["align_l"][k]) == shift == dmin + int(np.argmax(c))
    out = align(T(y).to(dev), T(ref).to(dev))
    assert out.shape == (AC.ALIGN_L,) and out.device.type == dev.type
    assert AC.sha256(out.cpu().numpy()) == str(g["align_out_sha"][k])
    rows = align(T(y)[None].to(dev), T(ref)[None].to(dev), wrap=False, max_lag=600)
    assert np.array_equal(rows.cpu().numpy()[0], AC.delayed(y, shift))


def test_align_unequal_lengths_is_the_reference_s_expression(dev):
    """len(y) != len(ref): the roll is argmax - (len(ref) - 1) = lag + len(y) - len(ref), literally"""
    from storm_amd.util.other import align
    y, ref = AC.align_inputs(37)
    y = y[:3000]
    full = ss.correlate(ref.astype(np.float64), y.astype(np.float64), mode="full", method="direct")       # = fftconvolve(ref, flip(y)) without the FFT
    l = int(np.argmax(full)) - (len(ref) - 1)
    assert l == AC.lag_peak(y, ref)[0] + len(y) - len(ref)
    out = align(T(y).to(dev), T(ref).to(dev))
    assert np.array_equal(out.cpu().numpy(), np.roll(y, l))


# ---- 2. shift -----------------------------------------------------------------------------------------------------------------------------
def _shifted(x, s, wrap, n=None):
    n = len(x) if n is None else n
    out = np.zeros(len(x), np.float32)
    if wrap:
        out[:n] = np.roll(x[:n], s)
    elif abs(s) < n:
        out[:n] = AC.delayed(x[:n], s)
    return out


@pytest.mark.parametrize("N", [5, 1030])
def test_shift_rows(dev, N):
    """np.roll bit for bit (wrap) and the zero-filled form: shifts 0, +-1, +-(N - 1), |s| >= N, a different shift in every row"""
    from storm_amd import ops
    shifts = [0, 1, -1, N - 1, -(N - 1), N, -N, 3 * N + 2, -(2 * N + 3), 2 ** 31 - 1, -2 ** 31]
    x = np.random.default_rng(N).standard_normal((len(shifts), N)).astype(np.float32)
    xd = T(x).to(dev)
    for wrap in (True, False):
        out = ops.shift_rows(xd, torch.tensor(shifts, dtype=torch.int32, device=dev), wrap=wrap).cpu().numpy()
        for k, s in enumerate(shifts):
            assert np.array_equal(out[k], _shifted(x[k], s, wrap)), (N, s, wrap)
    assert np.array_equal(ops.shift_rows(xd, 2).cpu().numpy(), np.roll(x, 2, axis=1))


def test_shift_ragged_and_misaligned(dev):
    """ragged rows (the tail is zero whatever lies in the input) and base pointers off the 16-byte grid on either side: the scalar paths
    of the 16-byte loads and stores move the same values"""
    from storm_amd import _lib, ops
    N, lens, shifts = 1030, [1030, 517, 4, 1], [5, -3, 1, 9]
    x = np.random.default_rng(3).standard_normal((4, N + 8)).astype(np.float32)
    for off in (0, 1, 2, 3):                                                 # the input rows start off * 4 bytes past a 16-byte boundary
        xd = T(x).to(dev)[:, off:off + N]
        for wrap in (True, False):
            out = ops.shift_rows(xd, shifts, lengths=lens, wrap=wrap).cpu().numpy()
            for k in range(4):
                assert np.array_equal(out[k], _shifted(x[k, off:off + N], shifts[k], wrap, lens[k])), (off, wrap, k)
    # a destination off the grid: the raw entry point into a view of a wider buffer
    xd = T(x).to(dev)[:, :N]
    sh = torch.tensor(shifts, dtype=torch.int32, device=dev)
    for off in (1, 2, 4):
        buf = torch.full((4, N + 8), 9.0, device=dev)
        _lib.check(_lib.lib().storm_shift_rows(xd.data_ptr(), buf.data_ptr() + 4 * off, sh.data_ptr(), 4, N, xd.stride(0), buf.stride(0), None, 1,
                                               _lib.stream()), "storm_shift_rows")
        got = buf.cpu().numpy()
        assert np.array_equal(got[:, off:off + N], np.stack([np.roll(x[k, :N], shifts[k]) for k in range(4)]))
        assert (got[:, :off] == 9.0).all() and (got[:, off + N:] == 9.0).all()


# ---- 3. biquad cascade --------------------------------------------------------------------------------------------------------------------
SOS5 = ss.butter(10, 80 / 16000 * 2, "hp", output="sos")                     # the reference's five sections


@pytest.mark.parametrize("S", [1, 5])
def test_sosfilt_equals_scipy(dev, S):
    """bit-equal to scipy.signal.sosfilt in fp64, the fp32 output is that value rounded once; lengths 1, 2, 3, 257, 4099"""
    from storm_amd import ops
    rng = np.random.default_rng(S)
    for L in (1, 2, 3, 257, 4099):
        x = rng.standard_normal((2, L)).astype(np.float32)
        want = ss.sosfilt(SOS5[:S], x.astype(np.float64), axis=-1)
        got = ops.sosfilt_rows(T(x).to(dev), SOS5[:S])
        assert got.dtype == torch.float64 and np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (S, L)
        got32 = ops.sosfilt_rows(T(x).to(dev), T(SOS5[:S].copy()), out_dtype=torch.float32)
        assert got32.dtype == torch.float32 and np.array_equal(got32.cpu().numpy(), want.astype(np.float32)), (S, L)
    if S == 5:
        assert np.array_equal(_bits(AC.sosfilt(SOS5, x[0, :300])), _bits(want[0, :300]))      # the Python restatement of the definition


@pytest.mark.parametrize("S,B", [(5, 14), (1, 35), (3, 22), (8, 9)])
def test_sosfilt_ragged_batch_equals_one_row_calls(dev, S, B):
    """more rows than one workgroup holds (min(64 / S, 16)), ragged, junk past every length, a row stride wider than the batch: every row is
    bit-equal to its one-row call and to scipy, and zero past its length"""
    from storm_amd import ops
    rng = np.random.default_rng(100 + S)
    lens = [int(v) for v in rng.integers(1, 90, size=B)]
    lens[0], lens[-1] = 90, 33
    rows = [rng.standard_normal(n).astype(np.float32) for n in lens]
    xb, _ = _batch(rows, dev, width=100, junk=5.0)
    got = ops.sosfilt_rows(xb[:, :90], SOS5[:S], lengths=lens).cpu().numpy()
    G = min(64 // S, 16)                                                     # rows per workgroup
    for k in (0, 1, B // 2, G - 1, G, B - 1):
        want = ss.sosfilt(SOS5[:S], rows[k].astype(np.float64))
        one = ops.sosfilt_rows(T(rows[k])[None].to(dev), SOS5[:S]).cpu().numpy()[0]
        assert np.array_equal(_bits(got[k, :lens[k]]), _bits(want)) and np.array_equal(_bits(one), _bits(want)), (S, k)
    for k in range(B):
        assert not got[k, lens[k]:].any()
    with pytest.raises(ValueError, match="sos"):
        ops.sosfilt_rows(xb, np.zeros((17, 6)))
    bad = SOS5.copy()
    bad[2, 3] = 2.0
    from storm_amd._lib import StormError
    with pytest.raises(StormError, match="a0"):
        ops.sosfilt_rows(xb, bad)


def test_sosfilt_keeps_subnormals(dev):
    """a 2000-sample burst and 160 000 zeros through the default filter: the state decays through the subnormal range (the reference output
    holds thousands of subnormals) - still bit-equal, so nothing is flushed"""
    from storm_amd import ops
    x = np.zeros((1, 162000), np.float32)
    x[0, :2000] = np.random.default_rng(9).standard_normal(2000).astype(np.float32)
    want = ss.sosfilt(SOS5, x.astype(np.float64), axis=-1)
    tiny = (want != 0) & (np.abs(want) < np.finfo(np.float64).tiny)
    assert tiny.sum() > 1000
    got = ops.sosfilt_rows(T(x).to(dev), SOS5).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))


# ---- 4. design ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4, 10])
def test_butter_sos_equals_scipy(dev, order):
    from storm_amd import ops
    worst = 0.0
    for hz, sr in ((50, 16000), (80, 16000), (300, 16000), (80, 48000)):
        wn = hz / sr * 2
        for btype in ("hp", "lp"):
            got, want = ops.butter_sos(order, wn, btype).numpy(), ss.butter(order, wn, btype, output="sos")
            assert got.shape == want.shape == (order // 2, 6)
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.array_equal(got[:, 3], np.ones(order // 2))
    print(f"storm_butter_sos order {order}: largest coefficient difference {worst / ULP2:.2f} ulp(2.0)")
    assert worst <= DESIGN_TOL


def test_butter_sos_refusals_name_the_argument(dev):
    from storm_amd import ops
    from storm_amd._lib import StormError
    for order in (3, 1, 0, 34):
        with pytest.raises(StormError, match="order"):
            ops.butter_sos(order, 0.01)
    for wn in (0.0, 1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(StormError, match="wn"):
            ops.butter_sos(10, wn)
    with pytest.raises(ValueError, match="btype"):
        ops.butter_sos(10, 0.01, "bandpass")


# ---- 5. hp_filter end to end --------------------------------------------------------------------------------------------------------------
def test_hp_filter_equals_the_reference(dev, golden):
    """util.other.hp_filter (the library's own sections through the kernel) against the reference's hp_filter output (fixture F26); with
    scipy's sections the kernel reproduces the fixture bit for bit"""
    from storm_amd import ops
    from storm_amd.util.other import hp_filter
    g = golden["f26_align"]
    x = AC.hp_input()
    assert AC.sha256(x) == str(g["hp_in_sha"])
    want = g["hp_out"]
    got = hp_filter(T(x).to(dev))
    assert got.dtype == torch.float64 and got.shape == (AC.HP_L,) and got.device.type == dev.type
    err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    print(f"hp_filter vs the reference: max |difference| / max |output| {err:.2e}")
    assert err <= HP_TOL
    assert np.array_equal(_bits(ops.sosfilt_rows(T(x)[None].to(dev), SOS5).cpu().numpy()[0]), _bits(want))
    rows = hp_filter(T(np.stack([x, x[::-1].copy()])).to(dev), lengths=[AC.HP_L, 100])
    assert np.array_equal(_bits(rows.cpu().numpy()[0]), _bits(got.cpu().numpy())) and not rows[1, 100:].any()
    assert float(np.abs(got.cpu().numpy()[2000:]).mean()) < 0.5 * float(np.abs(x[2000:]).mean())         # the rumble and the offset are gone


# ---- 6. surfaces --------------------------------------------------------------------------------------------------------------------------
def _triple(L, seed):
    g = torch.Generator().manual_seed(seed)
    s, n = 0.1 * torch.randn(L, generator=g), 0.05 * torch.randn(L, generator=g)
    return s, s + n, 0.8 * s + 0.3 * n


def test_score_batch_align(dev):
    """an estimate that is 3 samples late: lag == 3 and every metric is bit for bit that of the estimate with its last three samples zeroed
    (what the zero-filled shift back leaves); a ragged batch, lags of either sign; without the keyword keys and bits are as before"""
    from storm_amd import ops
    from storm_amd.util.inference import score_batch
    lens, lags = [2000, 1500], [3, -2]
    x, y, e, late, hand = (torch.zeros(2, 2000) for _ in range(5))
    for k, L in enumerate(lens):
        s, n, est = _triple(L, 40 + k)
        x[k, :L], y[k, :L], e[k, :L] = s, n, est
        late[k, :L] = T(AC.delayed(est.numpy(), lags[k]))
        hand[k, :L] = T(AC.delayed(AC.delayed(est.numpy(), lags[k]), -lags[k]))
    x, y, e, late, hand = (v.to(dev) for v in (x, y, e, late, hand))
    plain = score_batch(x, y, hand, lengths=lens)
    assert set(plain) == {"isnr", "lsd", "si_sdr", "si_sir", "si_sar"}
    got = score_batch(x, y, late, lengths=lens, align=True)
    assert sorted(got) == sorted(list(plain) + ["lag"]) and got["lag"].tolist() == lags
    for k in plain:
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(plain[k].cpu().numpy())), k
    want = ops.energy_ratios_rows(hand, x, y - x, lengths=lens)
    assert np.array_equal(_bits(got["si_sdr"].cpu().numpy()), _bits(want[:, 0].cpu().numpy()))
    assert float(score_batch(x, y, late, lengths=lens)["si_sdr"][0]) < float(got["si_sdr"][0]) - 10.0      # what a 3-sample delay costs unrepaired
    one = score_batch(x[:1], y[:1], late[:1], align=True, max_lag=8)
    assert int(one["lag"][0]) == 3 and _bits(one["si_sdr"].cpu().numpy())[0] == _bits(got["si_sdr"].cpu().numpy())[0]
    assert int(score_batch(x[:1], y[:1], late[:1], align=True, max_lag=0)["lag"][0]) == 0
    # hp: the three signals pass the filter first (fp32, rounded once)
    sos = ops.butter_sos(10, 80 / 16000 * 2)
    f = [ops.sosfilt_rows(v, sos, lengths=lens, out_dtype=torch.float32) for v in (x, y, late)]
    want = score_batch(f[0], f[1], f[2], lengths=lens, align=True)
    got = score_batch(x, y, late, lengths=lens, align=True, hp=80)
    assert got["lag"].tolist() == lags
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k


@pytest.mark.gpu
def test_calc_metrics_cli_align(tmp_path, monkeypatch):
    """calc_metrics.py --align --hp-filter: a directory whose enhanced files are a few samples late scores what the aligned directory
    scores without --align; the lines equal the function calls, do not depend on --batch, the column lag comes last; without the flags the
    files are what the unchanged tool writes"""
    from scipy.io import wavfile

    import calc_metrics
    from storm_amd.util.inference import score_batch
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "good", "late1", "late2", "latehp1", "latehp2", "plain")}
    for d in dirs.values():
        os.makedirs(d)
    triples, lags = {}, {"a.wav": 5, "b.wav": -4}
    for name, L in (("a.wav", 4000), ("b.wav", 3000)):
        s, n, est = _triple(L, L)
        est[:8], est[-8:] = 0.0, 0.0                                         # what leaves the row when it is moved is silence
        late = T(AC.delayed(est.numpy(), lags[name]))
        triples[name] = (s, n, est, late)
        for key, w in [("clean", s), ("noisy", n), ("good", est), ("plain", late)] + [(k, late) for k in dirs if k.startswith("late")]:
            wavfile.write(os.path.join(dirs[key], name), 16000, w.numpy().astype(np.float32))
    runs = {"good": [], "plain": [], "late1": ["--align", "--batch", "1"], "late2": ["--align", "--batch", "2", "--max-lag", "0.001"],
            "latehp1": ["--align", "--hp-filter", "--batch", "1"], "latehp2": ["--align", "--hp-filter", "80", "--batch", "2"]}
    for key, extra in runs.items():
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs[key]] + extra)
        calc_metrics.main()
    read = lambda key, f="_results.csv": open(os.path.join(dirs[key], f), "rb").read().decode("utf-8").splitlines()    # noqa: E731
    assert read("late1") == read("late2") and read("latehp1") == read("latehp2")
    assert read("late1", "_avg_results.txt") == read("late2", "_avg_results.txt")
    good, late = read("good"), read("late1")
    assert late[0].split(",")[-1] == "lag" and late[0].split(",")[:-1] == good[0].split(",") and "lag" not in good[0]
    assert [ln.split(",")[:7] for ln in late[1:]] == [ln.split(",")[:7] for ln in good[1:]]
    assert [ln.split(",")[-1] for ln in late[1:]] == ["5", "-4"]
    assert read("plain")[0] == good[0] and read("plain")[1].split(",")[3] != good[1].split(",")[3]
    assert read("late1", "_avg_results.txt")[-1].startswith("lag: ")
    dev_ = torch.device("cuda:0")
    for line in read("latehp1")[1:]:
        cells = line.split(",")
        s, n, _, latew = (w.to(dev_)[None] for w in triples[cells[0]])
        want = score_batch(s, n, latew, align=True, hp=80.0)
        assert cells[2:7] == [f"{float(want[k][0]):.6f}" for k in ("isnr", "si_sdr", "si_sir", "si_sar", "lsd")] and int(cells[-1]) == lags[cells[0]]
    monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs["good"], "--max-lag", "1"])
    with pytest.raises(SystemExit):
        calc_metrics.main()
