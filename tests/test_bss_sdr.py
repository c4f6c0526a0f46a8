"""BSS-eval SDR with a short filter on the device (storm_bss_sdr_rows: lag correlations per piece, a Levinson-Durbin solve per row) and its
Python / command-line surfaces - against the float64 restatement of tests/bss_cases.py (the correlations bit for bit), two independent CPU
solvers on the device's own correlations, and anchors that need no solver.  include/storm_hip.h is the specification."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl
import torch

from tests import bss_cases as BC
from tests.backend import dev, switch  # noqa: F401

T = torch.from_numpy
DB_TOL = 1e-4                    # the project's bound for dB numbers (tests/test_metrics.py)
# the two CPU solvers must agree with each other to a hundredth of that bound before either is used as the reference (measured: 2e-12 dB)
SOLVERS_AGREE = 1e-6
# filter against scipy.linalg.solve_toeplitz, relative L2, for references of condition below 1e4: condition x order x fp64 epsilon =
# 1e4 x 512 x 1.1e-16 = 6e-10, one order of margin
FILT_TOL = 1e-8
ANCHOR_TOL = 2e-6                # the fp32 bound of the kernel tests: the exact-filter anchor's estimate is rounded to fp32 once


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _batch(rows, d, width=None, junk=0.0, offset=0):
    """fp32 arrays -> a [B, width] view on d (junk past every row's length; the view starts `offset` floats into a wider buffer, so its rows
    are off the 16-byte grid and its stride is wider than the batch) and the lengths"""
    lens = [len(r) for r in rows]
    width = width or max(lens)
    buf = torch.full((len(rows), width + 8), junk, dtype=torch.float32)
    for k, r in enumerate(rows):
        buf[k, offset:offset + lens[k]] = T(np.ascontiguousarray(r))
    return buf.to(d)[:, offset:offset + width], lens


def _cpu_solvers(parts):
    """the SDR of one row from its G, D, Ee by scipy.linalg.solve_toeplitz and by np.linalg.solve on the dense matrix"""
    F = (len(parts) - 1) // 2
    G, D = parts[:F], parts[F:2 * F]
    Ct = sl.solve_toeplitz(G, D)
    Cd = np.linalg.solve(sl.toeplitz(G), D)
    return Ct, BC.sdr_of(parts, Ct), BC.sdr_of(parts, Cd)


def test_constants_are_the_header_s():
    from storm_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "storm_hip.h")).read()
    assert f"#define STORM_BSS_PIECE {BC.PIECE}\n" in text and _lib.BSS_PIECE == BC.PIECE == _lib.METRICS_CHUNK
    assert f"#define STORM_BSS_MAX_TAPS {BC.MAX_TAPS}\n" in text and _lib.BSS_MAX_TAPS == BC.MAX_TAPS


# ---- 1. correlations, bit for bit -----------------------------------------------------------------------------------------------------------
def _ragged_cases():
    return [(BC.COLOURS[k % 3], L) for k, L in enumerate(BC.LENGTHS)]


@pytest.mark.parametrize("flen", BC.FLENS)
def test_correlations_bit_equal(dev, flen):
    """all the lengths (2 .. 33000: both sides of 512 lags, both sides of the piece cut with lags that straddle it, three pieces) as ONE
    ragged batch with junk past every length, rows off the 16-byte grid and a stride wider than the batch: G, D, Ee equal the restatement's
    bits; so does every row alone"""
    from storm_amd import ops
    cases = _ragged_cases()
    pairs = [BC.pair(c, L) for c, L in cases]
    ref, lens = _batch([p[0] for p in pairs], dev, junk=7.0, offset=1)
    est, _ = _batch([p[1] for p in pairs], dev, junk=-3.0, offset=3)
    sdr, parts = ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen, return_parts=True)
    assert sdr.dtype == parts.dtype == torch.float64 and parts.shape == (len(cases), 2 * flen + 1)
    parts = parts.cpu().numpy()
    for k, (c, L) in enumerate(cases):
        want = BC.restated(c, L, flen)[0]
        assert np.array_equal(_bits(parts[k]), _bits(want)), (c, L, flen)
    for k in (0, 3, 7):                                                      # alone, contiguous, no lengths
        one = ops.bss_sdr_rows(T(pairs[k][0])[None].to(dev), T(pairs[k][1])[None].to(dev), flen=flen, return_parts=True)[1]
        assert np.array_equal(_bits(one.cpu().numpy()[0]), _bits(parts[k])), (cases[k], flen)


@pytest.mark.parametrize("R", [2, 4, 8])
def test_lags_per_thread_change_no_bit(dev, switch, R):
    """the launcher keeps 8, 4 or 2 lags per thread by the size of the launch (forced here through the library's test switch): a chain is
    the same chain, so every choice gives the restatement's bits - across the piece cut, for a filter that fills the waves and one that
    does not"""
    from storm_amd import ops
    switch("STORM_BSS_LAGS", R)
    cases = [c for c in _ragged_cases() if c[1] in (513, BC.PIECE + 511)]
    pairs = [BC.pair(c, L) for c, L in cases]
    ref, lens = _batch([p[0] for p in pairs], dev, junk=7.0)
    est, _ = _batch([p[1] for p in pairs], dev, junk=-3.0)
    for flen in (512, 64, 1):
        parts = ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen, return_parts=True)[1].cpu().numpy()
        for k, (c, L) in enumerate(cases):
            assert np.array_equal(_bits(parts[k]), _bits(BC.restated(c, L, flen)[0])), (R, c, L, flen)


# ---- 2. the SDR against two CPU solvers on the device's own correlations; 3. the filter ---------------------------------------------------
SOLVE_CASES = [(c, L, F) for c in BC.COLOURS for (L, F) in ((4097, 512), (BC.PIECE + 511, 512), (4097, 64))]


@pytest.mark.parametrize("colour,L,flen", SOLVE_CASES)
def test_sdr_and_filter_against_cpu_solvers(dev, colour, L, flen):
    """scipy.linalg.solve_toeplitz and np.linalg.solve on the device's G, D, Ee must agree with each other; the device's SDR is then within
    the project's bound for dB numbers of both and of the restatement end to end; the filter of the well-conditioned colours is within
    condition x order x epsilon of solve_toeplitz's"""
    from storm_amd import ops
    s, e = BC.pair(colour, L)
    sdr, filt, parts = (v.cpu().numpy()[0] for v in ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev), flen=flen, return_filter=True,
                                                                      return_parts=True))
    Ct, st, sd = _cpu_solvers(parts)
    assert abs(st - sd) <= SOLVERS_AGREE, (st, sd)
    rest = BC.restated(colour, L, flen)[2]
    gap = max(abs(sdr - st), abs(sdr - sd))
    rel = float(np.linalg.norm(filt - Ct) / np.linalg.norm(Ct))
    print(f"bss_sdr {colour} L={L} F={flen}: {sdr:.6f} dB, |device - CPU solvers| {gap:.2e} dB, |solvers apart| {abs(st - sd):.2e} dB, "
          f"|device - restatement| {abs(sdr - rest):.2e} dB, filter rel. L2 against solve_toeplitz {rel:.2e}")
    assert 15.0 < sdr < 25.0                                                 # (noise at -20 dB; a filter of fewer taps than the FIR loses a little)
    assert gap <= DB_TOL and abs(sdr - rest) <= DB_TOL
    if colour != "lowpass":                                                  # (condition up to 2e7: printed, not asserted)
        assert rel <= FILT_TOL


# ---- 4. anchors that need no solver ---------------------------------------------------------------------------------------------------------
def test_exact_filter_anchor(dev):
    """a white reference whose last 64 samples are zero, the estimate exactly convolve(ref, h)[:L] with 40 taps (no tail is cut off), rounded to
    fp32 once: nothing is left (+inf, or at least 120 dB) and the solved filter is h.  Without the zeroed tail the cut-off tail is real
    residual and the same case scores tens of dB, not hundreds."""
    from storm_amd import ops
    L, h = 4097, BC.fir(1)
    s = BC.pair("white", L, seed=1)[0].copy()
    cut = np.convolve(s.astype(np.float64), h)[:L].astype(np.float32)
    s[-64:] = 0.0
    e = np.convolve(s.astype(np.float64), h)[:L].astype(np.float32)
    sdr, filt = ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev), return_filter=True)
    sdr, filt = float(sdr[0]), filt.cpu().numpy()[0]
    err = float(np.abs(filt[:40] - h).max())
    print(f"exact-filter anchor: sdr {sdr}, max |filt[:40] - h| {err:.2e}, max |filt[40:]| {np.abs(filt[40:]).max():.2e}")
    assert sdr == np.inf or sdr >= 120.0
    assert err <= ANCHOR_TOL and float(np.abs(filt[40:]).max()) <= ANCHOR_TOL
    uncut = float(ops.bss_sdr_rows(T(BC.pair("white", L, seed=1)[0])[None].to(dev), T(cut)[None].to(dev))[0])
    assert 10.0 < uncut < 60.0, uncut


def test_one_tap_is_si_sdr(dev):
    """flen = 1 allows a gain only: SI-SDR without its eps, on a 10-dB case"""
    from storm_amd import ops
    rng = np.random.default_rng(11)
    s = BC.pair("ar2", 4097)[0]
    e = BC.with_noise(s.astype(np.float64), 10.0, rng).astype(np.float32)
    sd, ed = T(s)[None].to(dev), T(e)[None].to(dev)
    got = float(ops.bss_sdr_rows(sd, ed, flen=1)[0])
    want = float(ops.energy_ratios_rows(ed, sd, ed - sd)[0, 0])
    print(f"flen = 1: {got:.6f} dB against SI-SDR {want:.6f} dB")
    assert 9.0 < want < 11.0 and abs(got - want) <= DB_TOL


@pytest.mark.parametrize("d", [0, 1, 37, 500])
def test_delay_anchor(dev, d):
    """a coloured row with a zeroed 512-sample tail, delayed by d, plus noise at -20 dB: argmax |filter| is the delay, which is the negated
    result of the delay search as score_batch signs it; the SDR stays at 20 dB where SI-SDR collapses"""
    from storm_amd import ops
    L = 4097
    s = BC.pair("ar2", L)[0].copy()
    s[-512:] = 0.0
    e = BC.with_noise(BC.delayed(s, d).astype(np.float64), 20.0, np.random.default_rng(500 + d)).astype(np.float32)
    sd, ed = T(s)[None].to(dev), T(e)[None].to(dev)
    sdr, filt = ops.bss_sdr_rows(sd, ed, return_filter=True)
    back, _ = ops.xcorr_lag_rows(ed, sd)
    si = float(ops.energy_ratios_rows(ed, sd, ed - sd)[0, 0])
    print(f"delay {d}: sdr {float(sdr[0]):.3f} dB, SI-SDR {si:.3f} dB")
    assert int(filt[0].abs().argmax()) == d == -int(back[0])
    assert 19.0 < float(sdr[0]) < 22.0
    if d >= 37:
        assert float(sdr[0]) > si + 20.0


# ---- 5. edge rules ------------------------------------------------------------------------------------------------------------------------
def test_edge_rows_are_nan_and_leave_their_neighbours_alone(dev):
    from storm_amd import ops
    L = 700
    a, b = BC.pair("white", L), BC.pair("ar2", L)
    z = np.zeros(L, np.float32)
    refs, ests = [a[0], z, b[0], a[0], b[0]], [a[1], a[1], z, a[1], b[1]]
    lens = [L, L, L, 0, L]                                                   # zero reference, zero estimate, a row of no samples
    ref, _ = _batch(refs, dev, junk=2.0)
    est, _ = _batch(ests, dev, junk=2.0)
    for flen in (64, 512):
        sdr, filt, parts = ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen, return_filter=True, return_parts=True)
        assert torch.isnan(sdr[1:4]).all() and torch.isnan(filt[1:4]).all() and not parts[3].any()
        for k in (0, 4):
            one = ops.bss_sdr_rows(T(refs[k])[None].to(dev), T(ests[k])[None].to(dev), flen=flen, return_filter=True, return_parts=True)
            assert all(torch.equal(got[k], alone[0]) for got, alone in zip((sdr, filt, parts), one)) and bool(torch.isfinite(sdr[k]))
    # one sample: a number (the estimate is a multiple of the reference, so nothing is left), never NaN
    s1, e1 = torch.tensor([[0.5]], device=dev), torch.tensor([[0.25]], device=dev)
    for flen in (1, 512):
        assert not bool(torch.isnan(ops.bss_sdr_rows(s1, e1, flen=flen)).any())


def test_refusals_name_the_argument(dev):
    from storm_amd import _lib, ops
    from storm_amd._lib import StormError
    x = torch.zeros(2, 100, device=dev)
    for flen in (0, -1, 513):
        with pytest.raises(StormError, match="flen"):
            ops.bss_sdr_rows(x, x, flen=flen)
    with pytest.raises(ValueError, match="lengths"):
        ops.bss_sdr_rows(x, x, lengths=[100, 101])
    with pytest.raises(ValueError, match="estimate"):
        ops.bss_sdr_rows(x, x.double())
    lib = _lib.lib()
    assert lib.storm_bss_sdr_scratch_bytes(2, 100, 512) == 2 * 1025 * 8 and lib.storm_bss_sdr_scratch_bytes(2, BC.PIECE + 1, 3) == 2 * 2 * 7 * 8
    assert 0 == lib.storm_bss_sdr_scratch_bytes(0, 100, 8) == lib.storm_bss_sdr_scratch_bytes(1, 0, 8) == lib.storm_bss_sdr_scratch_bytes(1, 2 ** 30 + 1, 8)
    assert 0 == lib.storm_bss_sdr_scratch_bytes(1, 100, 0) == lib.storm_bss_sdr_scratch_bytes(1, 100, 513)
    out, ws = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2 * 1025, dtype=torch.float64, device=dev)

    def call(B=2, L=100, flen=512, bytes_=8 * 2 * 1025):
        return lib.storm_bss_sdr_rows(x.data_ptr(), x.data_ptr(), out.data_ptr(), None, None, ws.data_ptr(), bytes_, B, L, 100, 100, None, flen,
                                      _lib.stream())
    assert call() == 0
    for kw, word in ((dict(B=0), "B=0"), (dict(L=0), "L=0"), (dict(L=2 ** 30 + 1), "L="), (dict(bytes_=8 * 2 * 1025 - 8), "scratch"),
                     (dict(flen=513), "flen=513")):
        assert call(**kw) != 0 and word in lib.storm_last_error().decode(), kw


# ---- 6. batch independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", [64, 512])
def test_a_row_does_not_depend_on_its_batch(dev, flen):
    """a row alone; first and last in a batch of three rows of different lengths and levels; at another stride; with and without the filter:
    sdr, filter and correlations are the same bits"""
    from storm_amd import ops
    L = BC.PIECE + 511
    s, e = BC.pair("ar2", L)
    others = [BC.pair("white", 700), BC.pair("lowpass", 4097)]
    alone = ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev), flen=flen, return_filter=True, return_parts=True)
    for pos, offset in ((0, 0), (2, 3)):
        rows = others.copy()
        rows.insert(pos, (s, e))
        ref, lens = _batch([1000.0 * r[0] if len(r[0]) == 700 else r[0] for r in rows], dev, width=L + 5 * offset, junk=9.0, offset=offset)
        est, _ = _batch([r[1] for r in rows], dev, width=L + 5 * offset, junk=-9.0, offset=offset)
        got = ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen, return_filter=True, return_parts=True)
        assert all(torch.equal(g[pos], a[0]) for g, a in zip(got, alone)), (pos, offset)
        plain = ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, got[0])
        assert torch.equal(ops.bss_sdr_rows(ref, est, lengths=lens, flen=flen, return_parts=True)[1], got[2])


# ---- 7. surfaces --------------------------------------------------------------------------------------------------------------------------
def test_util_other_sdr(dev):
    from storm_amd import ops
    from storm_amd.util.other import sdr
    s, e = BC.pair("ar2", 4097)
    want = ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev))
    got = sdr(T(s).to(dev), T(e).to(dev))
    assert isinstance(got, float) and got == float(want[0])
    if dev.type == "cpu":                                                    # (numpy in: moved to the current device - the simulation's is the host)
        assert sdr(s, e) == got
    rows = sdr(T(np.stack([s, e])).to(dev), T(np.stack([e, s])).to(dev), flen=64, lengths=[4097, 1000])
    assert rows.shape == (2,) and rows.dtype == torch.float64 and rows.device.type == dev.type
    assert float(rows[0]) == float(ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev), flen=64)[0])


@pytest.mark.gpu
def test_util_other_sdr_numpy_on_the_device():
    from tests.backend import setup_backend
    from storm_amd.util.other import sdr
    setup_backend("hip")
    s, e = BC.pair("ar2", 4097)
    got = sdr(s, e)
    assert isinstance(got, float) and got == sdr(T(s).cuda(), T(e).cuda()) and abs(got - BC.restated("ar2", 4097, 512)[2]) <= DB_TOL


def _triple(L, seed):
    g = torch.Generator().manual_seed(seed)
    s, n = 0.1 * torch.randn(L, generator=g), 0.05 * torch.randn(L, generator=g)
    return s, s + n, 0.8 * s + 0.3 * n


def test_score_batch_sdr(dev):
    """score_batch(sdr=True): the key sdr is the separate ops call bit for bit, every other key keeps its bits; it is computed on what hp= and
    align= leave"""
    from storm_amd import ops
    from storm_amd.util.inference import score_batch
    lens = [2000, 1500]
    x, y, e = (torch.zeros(2, 2000) for _ in range(3))
    for k, L in enumerate(lens):
        s, n, est = _triple(L, 60 + k)
        x[k, :L], y[k, :L] = s, n
        e[k, 3:L] = est[:L - 3]                                              # three samples late
    x, y, e = (v.to(dev) for v in (x, y, e))
    plain = score_batch(x, y, e, lengths=lens)
    got = score_batch(x, y, e, lengths=lens, sdr=True)
    assert sorted(got) == sorted(list(plain) + ["sdr"])
    for k in plain:
        assert np.array_equal(_bits(got[k].cpu().numpy()), _bits(plain[k].cpu().numpy())), k
    assert torch.equal(got["sdr"], ops.bss_sdr_rows(x, e, lengths=lens))
    assert torch.equal(score_batch(x, y, e, lengths=lens, sdr=True, sdr_taps=64)["sdr"], ops.bss_sdr_rows(x, e, lengths=lens, flen=64))
    assert float(got["sdr"][0]) > float(got["si_sdr"][0]) + 5.0              # the delay is inside the filter
    # align: on the moved estimate; the other keys are those of align alone, lag stays
    al, als = score_batch(x, y, e, lengths=lens, align=True), score_batch(x, y, e, lengths=lens, align=True, sdr=True)
    assert als["lag"].tolist() == [3, 3] and list(als)[-1] == "lag" and all(torch.equal(al[k], als[k]) for k in al)
    back, _ = ops.xcorr_lag_rows(e, x, lengths=lens, ref_lengths=lens)
    assert torch.equal(als["sdr"], ops.bss_sdr_rows(x, ops.shift_rows(e, back, lengths=lens, wrap=False), lengths=lens))
    # hp: on the filtered rows
    sos = ops.butter_sos(10, 80 / 16000 * 2)
    f = [ops.sosfilt_rows(v, sos, lengths=lens, out_dtype=torch.float32) for v in (x, y, e)]
    hp, hps = score_batch(x, y, e, lengths=lens, hp=80), score_batch(x, y, e, lengths=lens, hp=80, sdr=True)
    assert all(torch.equal(hp[k], hps[k]) for k in hp) and torch.equal(hps["sdr"], ops.bss_sdr_rows(f[0], f[2], lengths=lens))


@pytest.mark.gpu
def test_calc_metrics_cli_sdr(tmp_path, monkeypatch):
    """calc_metrics.py --sdr [TAPS]: the column sdr stands after stoi,estoi and before lag (which stays last), a line does not depend on
    --batch, the values are score_batch's, and without the flag the header is the unchanged one"""
    from scipy.io import wavfile

    import calc_metrics
    from storm_amd.util.inference import score_batch
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "plain", "b1", "b2", "all1", "all2", "taps")}
    for d in dirs.values():
        os.makedirs(d)
    triples = {}
    for name, L in (("a.wav", 6000), ("b.wav", 5700)):
        s, n, est = _triple(L, L)
        late = torch.zeros(L)
        late[4:] = est[:L - 4]
        triples[name] = (s, n, late)
        for key, w in [("clean", s), ("noisy", n)] + [(k, late) for k in dirs if k not in ("clean", "noisy")]:
            wavfile.write(os.path.join(dirs[key], name), 16000, w.numpy().astype(np.float32))
    runs = {"plain": [], "b1": ["--sdr", "--batch", "1"], "b2": ["--sdr", "--batch", "2"], "taps": ["--sdr", "64"],
            "all1": ["--sdr", "--stoi", "--align", "--hp-filter", "--resample", "--batch", "1"],
            "all2": ["--sdr", "512", "--stoi", "--align", "--hp-filter", "80", "--resample", "--batch", "2"]}
    for key, extra in runs.items():
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs[key]] + extra)
        calc_metrics.main()
    read = lambda key, f="_results.csv": open(os.path.join(dirs[key], f), "rb").read().decode("utf-8").splitlines()    # noqa: E731
    assert read("b1") == read("b2") and read("all1") == read("all2")
    head = read("plain")[0].split(",")
    assert "sdr" not in head and read("b1")[0].split(",") == head + ["sdr"]
    assert [ln.split(",")[:-1] for ln in read("b1")[1:]] == [ln.split(",") for ln in read("plain")[1:]]
    assert read("all1")[0].split(",")[-4:] == ["stoi", "estoi", "sdr", "lag"]
    assert read("b1", "_avg_results.txt")[-1].startswith("sdr: ")
    dev_ = torch.device("cuda:0")
    for key, kw in (("b1", {}), ("taps", dict(sdr_taps=64)), ("all1", dict(align=True, hp=80.0, stoi=True))):
        for line in read(key)[1:]:
            cells = line.split(",")
            s, n, late = (w.to(dev_)[None] for w in triples[cells[0]])
            want = score_batch(s, n, late, sdr=True, **kw)
            assert cells[-2 if key == "all1" else -1] == f"{float(want['sdr'][0]):.6f}", (key, line)
    assert [ln.split(",")[-1] for ln in read("all1")[1:]] == ["4", "4"]
    assert f"{float('inf'):.6f}" == "inf"                                     # (what a file that is exactly a filtered clean file prints)
    monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs["plain"], "--sdr", "513"])
    with pytest.raises(SystemExit):
        calc_metrics.main()


def test_mir_eval_cross_check(dev):
    """where mir_eval imports: its bss_eval_sources SDR on a length whose FFT does not wrap, within 1e-3 dB.  It imports on none of the machines
    this project is built or tested on, so no parity with mir_eval is claimed anywhere."""
    mir_eval = pytest.importorskip("mir_eval")
    from storm_amd import ops
    s, e = BC.pair("ar2", 4097)
    want = mir_eval.separation.bss_eval_sources(s[None].astype(np.float64), e[None].astype(np.float64))[0][0]
    got = float(ops.bss_sdr_rows(T(s)[None].to(dev), T(e)[None].to(dev))[0])
    assert abs(got - want) <= 1e-3
