"""STOI / ESTOI on the device (storm_stoi_rows, storm_stoi_taps, storm_resample_poly_taps and their Python / command-line surfaces) against
the float64 numpy restatement of the definition in include/storm_hip.h (tests/stoi_cases.py).  pystoi is installed on none of the project's
machines: nothing here was compared with it except by the last test, which skips without it."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from tests import stoi_cases as SC
from tests.backend import dev  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
U32 = 2.0 ** -24                                                             # unit roundoff of fp32
# The kernel against the restatement on the SAME fp32 samples at 10 kHz: both sides are float64 throughout and differ in the order of their
# sums, in the FFT (radix-2 in LDS against pocketfft) and in libm's last bits.  Each measure is a mean of >= 15 correlations of unit vectors,
# every one off by a few 2^-53, so the results agree to about one unit in the last place of a number below 1 (2^-53 = 1.11e-16).  Measured
# largest |difference| over the rows of test_kernel_vs_restatement_at_10k: 1.11e-16 on the host simulation and 1.11e-16 on the MI355X; the
# bound is 8 x the larger of the two.
KERNEL_TOL = 8 * 1.11e-16
# End to end at 16 / 8 / 48 kHz against the ANCHORS (float64 resampling): dominated by the fp32 resampling on the device (a 117 / 73 / 349 tap
# fp32 FMA chain per sample and one rounding of every 10 kHz sample to fp32; that rounding alone moves a16k by 2e-9).  Measured worst
# |difference| over both measures of a16k, b16k, f8k, g48k: 1.20e-8 (a16k: STOI 1.20e-8, ESTOI 1.00e-8; b16k 2.2e-9, f8k 5.2e-9, g48k 1.1e-9 -
# the same figures on the host simulation and on the MI355X, whose FMA chains are the same bits); the bound is 8 x that.
E2E_TOL = 8 * 1.20e-8
WITH_SEGMENTS = [n for n, a in SC.ANCHORS.items() if a[4] > 0]


def _rows(pairs, d):
    """[(clean, processed), ...] of fp32 arrays -> zero-filled batches (clean [B, L], processed [B, L]) on d, lengths"""
    lens = [len(c) for c, _ in pairs]
    c, p = torch.zeros(len(pairs), max(lens)), torch.zeros(len(pairs), max(lens))
    for k, (a, b) in enumerate(pairs):
        c[k, :lens[k]], p[k, :lens[k]] = T(a.copy()), T(b.copy())
    return c.to(d), p.to(d), lens


def _unpermute(Tab, n):
    """phase-major [up][M] -> h[j], j = p + m up (the first n), and the slots past it"""
    flat = Tab.numpy().T.reshape(-1)
    return flat[:n], flat[n:]


# ---- 1. restatement and anchors --------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_anchors(dev):
    """tests/stoi_cases.py reproduces the definition's anchor values to 1e-9 (the counts exactly), stoi(x, x) = 1 within 1e-12 for both
    measures in every case that has a segment (1e-5 in the one that has none), the band edges are the literals, no frame of a case lies
    within 1 dB of the gate threshold (so no rounding can flip the mask in the tests below), and its resampling filter is the library's:
    the same length at every rate of the cases, and at 16 kHz the same fp32 taps (test_taps_equal_the_numpy_design has the other rates)"""
    from storm_amd import _lib, ops
    lo, hi = SC.band_edges()
    assert tuple(lo) == SC.BAND_EDGES[:-1] and tuple(hi) == SC.BAND_EDGES[1:]
    assert SC.EPS == 2.0 ** -52
    assert [len(SC.resample_filter(fs)) for fs in (16000, 48000)] == [581, 1741] and SC.ratio(16000) == (5, 8) and SC.ratio(48000) == (5, 24)
    assert [_lib.lib().storm_stoi_num_taps(fs) for fs in (16000, 8000, 48000)] == [len(SC.resample_filter(fs)) for fs in (16000, 8000, 48000)]
    assert np.array_equal(_unpermute(ops.stoi_taps(16000), 581)[0], (SC.resample_filter(16000) * 5).astype(np.float32))
    for name, (estoi, stoi, frames, kept, segs) in SC.ANCHORS.items():
        r = SC.restated(name)
        print(f"restatement {name}: ESTOI {r['estoi']:.12f} STOI {r['stoi']:.12f} frames {r['frames']} / {r['kept']} / {r['segments']} "
              f"gate margin {r['margin']:.2f} dB")
        assert (r["frames"], r["kept"], r["segments"]) == (frames, kept, segs), name
        assert r["margin"] > 1.0, name
        assert abs(r["estoi"] - estoi) < 1e-9 and abs(r["stoi"] - stoi) < 1e-9, (name, r)
        c, _ = SC.signals(name)
        same = SC.stoi64(c, c, SC.CASES[name][2])
        want = 1.0 if segs else SC.TOO_SHORT
        assert abs(same["stoi"] - want) < 1e-12 and abs(same["estoi"] - want) < 1e-12, (name, same)
    assert min(SC.restated(n)["margin"] for n in WITH_SEGMENTS) > 3.0


@pytest.mark.parametrize("fs", [16000, 8000, 48000, 44100])
def test_taps_equal_the_numpy_design(dev, fs):
    """storm_stoi_taps, un-permuted from phase-major [up][M], against np.kaiser * np.sinc in float64 (sum 1, times up) rounded to fp32.  Both
    designs are float64 and differ in I0 (power series here, Chebyshev fits in numpy: a few 1e-16 relative), which no fp32 rounding of
    these 581 / 365 / 1741 / 31947 taps sits on: every tap EQUALS numpy's (largest gap 0 ulp, on the host simulation and on the MI355X);
    the slots past a phase's last tap are zero."""
    from storm_amd import _lib, ops
    up, down = SC.ratio(fs)
    h = SC.resample_filter(fs) * up
    n = len(h)
    assert _lib.lib().storm_stoi_num_taps(fs) == n
    Tab = ops.stoi_taps(fs)
    assert Tab.shape == (up, -(-n // up)) and Tab.dtype == torch.float32
    got, rest = _unpermute(Tab, n)
    h32 = h.astype(np.float32)
    ulp = np.spacing(np.abs(h32)).astype(np.float64)
    gap = np.abs(got.astype(np.float64) - h32.astype(np.float64)) / ulp
    print(f"stoi taps {fs} Hz ({up}/{down}): {n} taps, {int((got != h32).sum())} differ from numpy's design, largest gap {gap.max():.0f} ulp")
    assert np.array_equal(got, h32)
    assert (rest == 0).all()
    assert abs(float(got.astype(np.float64).sum()) - up) < 1e-5 * up


# ---- 2. the kernel against the restatement at 10 kHz ---------------------------------------------------------------------------------------
def test_kernel_vs_restatement_at_10k(dev):
    """ops.stoi_rows(fs=10000) on c10k (two gaps: 29 gated frames), d10k_min (the shortest row with a segment), e10k_short (M = 29), rows of
    256 and 257 samples (no spectrogram frame) and a16k resampled by scipy in float64 and rounded to fp32 - one ragged batch and one-row
    calls, against the restatement in float64 on the same fp32 samples; the counts of frames, kept frames and segments exactly"""
    from storm_amd import ops
    g = np.random.default_rng(5)
    tiny = [(g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)) for n in (256, 257)]
    pairs = [SC.signals("c10k"), SC.signals("d10k_min"), SC.signals("e10k_short"), tiny[0], tiny[1], SC.at_10k_fp32("a16k")]
    want = [SC.stoi64(c, p, SC.FS) for c, p in pairs]
    assert [w["segments"] for w in want] == [96, 1, 0, 0, 0, 103] and [w["frames"] for w in want] == [155, 31, 30, 0, 1, 155]
    assert all(w["margin"] > 1.0 for w in want if w["segments"])
    c, p, lens = _rows(pairs, dev)
    got, counts = ops.stoi_rows(c, p, lengths=lens, fs=SC.FS, counts=True)
    got, counts = got.cpu().numpy(), counts.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (6, 2) and counts.shape == (6, 3)
    worst = 0.0
    for k, w in enumerate(want):
        assert tuple(counts[k]) == (w["frames"], w["kept"], w["segments"]), (k, counts[k], w)
        alone = ops.stoi_rows(c[k:k + 1, :lens[k]], p[k:k + 1, :lens[k]], fs=SC.FS).cpu().numpy()
        assert np.array_equal(alone[0], got[k]), (k, alone, got[k])
        diff = max(abs(got[k, 0] - w["stoi"]), abs(got[k, 1] - w["estoi"]))
        print(f"stoi_rows row {k} ({lens[k]} samples): STOI {got[k, 0]:.15f} ESTOI {got[k, 1]:.15f}, |difference| vs the restatement {diff:.2e}")
        worst = max(worst, diff)
        if not w["segments"]:
            assert got[k, 0] == got[k, 1] == SC.TOO_SHORT
    print(f"stoi_rows at 10 kHz: largest difference {worst:.2e} (bound {KERNEL_TOL:.2e})")
    assert worst < KERNEL_TOL
    same = ops.stoi_rows(c[:2], c[:2], lengths=lens[:2], fs=SC.FS).cpu().numpy()
    assert np.abs(same - 1.0).max() < 1e-12                                # a signal against itself


# ---- 3. the resampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a16k", "f8k", "g48k"])
def test_resampler_vs_scipy(dev, name):
    """storm_resample_poly_taps with the STOI filter against scipy.signal.resample_poly(x, up, down, window=h) in float64 on the case's two
    signals.  Every output is ONE fp32 FMA chain over its M_p <= M = ceil(num_taps / up) taps: the chain's rounding is at most
    gamma_M = M u / (1 - M u) times sum_k |t_k x_k| (u = 2^-24; Higham, Accuracy and Stability, sec. 3.1), the taps' own rounding to fp32 adds
    u times that sum, and scipy's float64 error is 2^-29 of either - so |y - y_ref| <= (M + 2) u (|up h| applied to |x|), per output."""
    from scipy.signal import resample_poly

    from storm_amd import ops
    fs = SC.CASES[name][2]
    up, down = SC.ratio(fs)
    h = SC.resample_filter(fs)
    M = -(-len(h) // up)
    x = np.stack(SC.signals(name))
    y = ops.stoi_resample(T(x.copy()).to(dev), fs).cpu().numpy()
    ref = resample_poly(x.astype(np.float64), up, down, axis=1, window=h)
    scale = resample_poly(np.abs(x).astype(np.float64), up, down, axis=1, window=np.abs(h))
    assert y.shape == ref.shape == (2, -(-x.shape[1] * up // down)) and y.dtype == np.float32
    err = np.abs(y - ref)
    bound = (M + 2) * U32 * scale
    print(f"stoi resample {fs} -> 10000 ({up}/{down}, {len(h)} taps, M = {M}): largest |y - scipy fp64| {err.max():.3e}, largest share of its bound "
          f"{float((err / bound).max()):.3f}, rel-L2 {float(np.linalg.norm(err) / np.linalg.norm(ref)):.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("fs", [16000, 8000, 48000])
def test_resampler_impulse_is_the_table(dev, fs):
    """x = delta[k - k0]: y[n] = T[n down - k0 up + half] bit for bit (0 where the index leaves the filter) - every other product is a zero"""
    from storm_amd import _lib, ops
    up, down = SC.ratio(fs)
    n_taps = _lib.lib().storm_stoi_num_taps(fs)
    half = (n_taps - 1) // 2
    h, _ = _unpermute(ops.stoi_taps(fs), n_taps)
    L = 2 * n_taps * down // up + 50
    ks = [0, 1, L // 2 + 3, L - 1]
    x = torch.zeros(len(ks), L)
    for r, k0 in enumerate(ks):
        x[r, k0] = 1.0
    y = ops.stoi_resample(x.to(dev), fs).cpu().numpy()
    n = np.arange(y.shape[1], dtype=np.int64)
    for r, k0 in enumerate(ks):
        j = n * down - k0 * up + half
        ok = (j >= 0) & (j < n_taps)
        want = np.where(ok, h[np.clip(j, 0, n_taps - 1)], np.float32(0))
        assert ok.any() and np.array_equal(y[r], want), (fs, k0)


def test_resample_poly_itself_is_untouched(dev):
    """the old entry point (storm_resample_poly through ops.resample_poly, its own Kaiser(5) design) on one case of tests/test_resample.py:
    160 / 441 on three workgroups' worth of samples, against scipy's defaults within that file's bound"""
    from scipy.signal import resample_poly

    from storm_amd import ops
    from tests.test_resample import F32_TOL, _signal
    from tests.util import rel_l2
    up, down = 160, 441
    x = _signal(1, 2 * ops.RESAMPLE_TILE * down // up + 5, 100)
    y = ops.resample_poly(T(x).to(dev), up, down).cpu()
    ref = resample_poly(x.astype(np.float64), up, down, axis=1)
    err = rel_l2(y, ref)
    print(f"resample {up}/{down} L={x.shape[1]} -> {y.shape[1]}: rel-L2 vs scipy fp64 {err:.3e}")
    assert y.shape == ref.shape and err < F32_TOL


# ---- 4. end to end at 16 / 8 / 48 kHz ------------------------------------------------------------------------------------------------------------
def test_end_to_end_vs_anchors(dev):
    """ops.stoi_rows at the cases' own rates (device resampling + metric) against the anchors"""
    from storm_amd import ops
    worst = 0.0
    for name in ("a16k", "b16k", "f8k", "g48k"):
        c, p = SC.signals(name)
        estoi, stoi, frames, kept, segs = SC.ANCHORS[name]
        got, counts = ops.stoi_rows(T(c.copy())[None].to(dev), T(p.copy())[None].to(dev), fs=SC.CASES[name][2], counts=True)
        got = got.cpu().numpy()[0]
        assert tuple(counts.cpu().numpy()[0]) == (frames, kept, segs), name
        diff = max(abs(got[0] - stoi), abs(got[1] - estoi))
        print(f"stoi end to end {name}: STOI {got[0]:.12f} ESTOI {got[1]:.12f}, |difference| vs the anchors {abs(got[0] - stoi):.2e} {abs(got[1] - estoi):.2e}")
        worst = max(worst, diff)
    print(f"stoi end to end: largest difference {worst:.2e} (bound {E2E_TOL:.2e})")
    assert worst < E2E_TOL


# ---- 5. a row's numbers do not depend on the batch ----------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(dev):
    """a ragged batch at fs = 16000 of a16k, b16k, a row of d10k_min's length and a 256-sample row, zero filled: every row's two numbers are
    the bits of its own one-row call on the trimmed row, of the batch with 1000 more zero columns, of the batch with its rows permuted and
    of a strided view (every second row of a [2 B, L] buffer)"""
    from storm_amd import ops
    d = SC.signals("d10k_min")
    pairs = [SC.signals("a16k"), SC.signals("b16k"), d, (d[0][:256], d[1][:256])]
    c, p, lens = _rows(pairs, dev)
    assert lens == [32000, 16001, 4224, 256]
    base = ops.stoi_rows(c, p, lengths=lens, fs=16000).cpu()
    assert base.shape == (4, 2) and base.dtype == torch.float64 and torch.isfinite(base).all()
    assert (base[:2] > 0.3).all() and (base[2:] == SC.TOO_SHORT).all()
    for k, n in enumerate(lens):
        alone = ops.stoi_rows(c[k:k + 1, :n], p[k:k + 1, :n], fs=16000).cpu()
        assert torch.equal(alone[0], base[k]), (k, alone, base[k])
    wide = [torch.cat([x, torch.zeros(4, 1000, device=dev)], 1) for x in (c, p)]
    assert torch.equal(ops.stoi_rows(*wide, lengths=lens, fs=16000).cpu(), base)
    perm = [2, 0, 3, 1]
    assert torch.equal(ops.stoi_rows(c[perm], p[perm], lengths=[lens[i] for i in perm], fs=16000).cpu(), base[perm])
    bufs = []
    for x in (c, p):
        buf = torch.full((8, x.shape[1]), 7.0, device=dev)
        buf[::2] = x
        bufs.append(buf[::2])
    assert bufs[0].stride(0) == 2 * c.shape[1]
    assert torch.equal(ops.stoi_rows(*bufs, lengths=lens, fs=16000).cpu(), base)


# ---- 6. surfaces ----------------------------------------------------------------------------------------------------------------------------------------
def test_score_batch_and_util_stoi(dev):
    from storm_amd import ops
    from storm_amd.util import other as O
    from storm_amd.util.inference import METRIC_KEYS, score_batch
    pairs = [SC.signals("b16k"), tuple(v[:3000] for v in SC.signals("b16k"))]
    c, p, lens = _rows(pairs, dev)
    noisy = p + 0.01
    assert sorted(score_batch(c, noisy, p, lengths=lens)) == sorted(METRIC_KEYS) == ["isnr", "lsd", "si_sar", "si_sdr", "si_sir"]
    got = score_batch(c, noisy, p, lengths=lens, stoi=True)
    assert sorted(got) == ["estoi", "isnr", "lsd", "si_sar", "si_sdr", "si_sir", "stoi"]
    want = ops.stoi_rows(c, p, lengths=lens, fs=16000)
    assert torch.equal(got["stoi"], want[:, 0]) and torch.equal(got["estoi"], want[:, 1]) and got["stoi"].dtype == torch.float64
    plain = score_batch(c, noisy, p, lengths=lens)
    assert all(torch.equal(plain[k], got[k]) for k in METRIC_KEYS)
    # pystoi's signature: 1-D -> float, [B, L] -> tensor; a short row warns and gives 1e-5
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        one = O.stoi(c[0], p[0], 16000)
        ext = O.stoi(c[0], p[0], 16000, extended=True)
        arr = O.stoi(c[0].cpu().numpy(), p[0], 16000, extended=True)                 # an array beside a tensor goes to the tensor's device
        f64 = O.stoi(c[0].cpu().numpy().astype(np.float64), p[0].double(), 16000)    # pystoi's callers pass float64: rounded to fp32
    assert isinstance(one, float) and one == f64 == float(want[0, 0]) and ext == arr == float(want[0, 1])
    with pytest.warns(RuntimeWarning, match="Not enough STFT frames"):
        both = O.stoi(c, p, 16000, extended=True, lengths=lens)
    assert both.shape == (2,) and torch.equal(both, want[:, 1]) and float(both[1]) == SC.TOO_SHORT
    with pytest.warns(RuntimeWarning):
        assert O.stoi(c[1, :3000], p[1, :3000], 16000) == SC.TOO_SHORT
    with pytest.raises(Exception, match="same length"):
        O.stoi(c[0], p[0, :-1], 16000)
    with pytest.raises(ValueError, match="stoi_rows"):
        ops.stoi_rows(c, p.double())
    with pytest.raises(ValueError, match="lengths"):
        ops.stoi_rows(c, p, lengths=[1, c.shape[1] + 1])


def test_evaluate_model_device_estoi(dev, golden, monkeypatch):
    """evaluate_model(..., estoi='device') on F10's pairs with injected per-file noise: elements 1, 2, 4, 5 are those of the default call,
    the third is the mean of the files' own ops.stoi_rows ESTOI, metrics=True gains stoi and estoi; the default call still returns NaN
    for ESTOI when pystoi does not import"""
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import ScoreModel
    from storm_amd.util.inference import METRIC_KEYS, evaluate_model
    from storm_amd import ops
    monkeypatch.setitem(sys.modules, "pystoi", None)                         # (import pystoi raises ImportError)
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
    plain = evaluate_model(m, 3, **kw)
    full = evaluate_model(m, 3, metrics=True, estoi="device", **kw)
    assert len(plain) == 5 and len(full) == 6 and math.isnan(plain[2])
    assert plain[1] == full[1] and (plain[0] == full[0] or (math.isnan(plain[0]) and math.isnan(full[0])))
    assert plain[3] is None and full[3] is None
    assert all(torch.equal(a, b) for la, lb in zip(plain[4], full[4]) for a, b in zip(la, lb))
    each = torch.cat([ops.stoi_rows(pairs[i][0].to(dev), full[4][1][i][None].to(dev), fs=16000).cpu() for i in range(3)])
    # (a seeded, untrained network: its estimates correlate weakly with the clean files - either sign; the 4000-sample file has no segment)
    assert (each[:2].abs() < 1).all() and (each[:2] != SC.TOO_SHORT).all() and (each[2] == SC.TOO_SHORT).all()
    assert abs(full[2] - float(each[:, 1].mean())) <= 1e-12
    assert sorted(full[5]) == sorted(METRIC_KEYS + ("stoi", "estoi"))
    assert full[5]["estoi"] == full[2] and abs(full[5]["stoi"] - float(each[:, 0].mean())) <= 1e-12
    with pytest.raises(ValueError, match="estoi"):
        evaluate_model(m, 3, estoi="host", **kw)


@pytest.mark.gpu
def test_calc_metrics_cli_stoi(tmp_path, monkeypatch):
    """calc_metrics.py --stoi --resample on three 16 kHz triples (one too short for a segment) and one 8 kHz triple: --batch 1 and --batch 3
    write the same bytes, the columns stoi,estoi come last and equal score_batch's of the trimmed triple to the printed decimals, the
    averages list them; without --stoi the header and the line count are what tests/test_metrics.py expects of the unchanged tool"""
    from scipy.io import wavfile

    import calc_metrics
    from storm_amd.data_module import SpecsDataModule
    from storm_amd.util.inference import _optional, score_batch
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "enh1", "enh3", "plain")}
    for d in dirs.values():
        os.makedirs(d)
    g = torch.Generator().manual_seed(2490)
    triples = {}
    for name, L, sr in (("a.wav", 9000, 16000), ("b.wav", 12000, 16000), ("c.wav", 3000, 16000), ("d.wav", 6000, 8000)):
        s, n = 0.1 * torch.randn(L, generator=g), 0.05 * torch.randn(L, generator=g)
        triples[name] = (s, s + n, 0.8 * s + 0.3 * n, sr)
        for key, w in (("clean", triples[name][0]), ("noisy", triples[name][1]), ("enh1", triples[name][2]), ("enh3", triples[name][2]),
                       ("plain", triples[name][2])):
            wavfile.write(os.path.join(dirs[key], name), sr, w.numpy().astype(np.float32))
    for key, extra in (("enh1", ["--batch", "1", "--stoi"]), ("enh3", ["--batch", "3", "--stoi"]), ("plain", ["--batch", "3"])):
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs[key],
                                          "--resample"] + extra)
        calc_metrics.main()
    read = lambda key, f: open(os.path.join(dirs[key], f), "rb").read()    # noqa: E731
    assert read("enh1", "_results.csv") == read("enh3", "_results.csv") and read("enh1", "_avg_results.txt") == read("enh3", "_avg_results.txt")
    lines = read("enh1", "_results.csv").decode().splitlines()
    header = lines[0].split(",")
    host = ["pesq"] if _optional("pesq", "pesq") is not None else []
    assert header == ["Filename", "Length", "iSNR", "si_sdr", "si_sir", "si_sar", "lsd"] + host + ["stoi", "estoi"] and len(lines) == 5
    dev_ = torch.device("cuda:0")
    short = 0
    for line in lines[1:]:
        cells = line.split(",")
        x, y, e, sr = triples[cells[0]]
        x, y, e = (SpecsDataModule.resample(w.to(dev_), sr, 16000) for w in (x, y, e))
        want = score_batch(x[None], y[None], e[None], stoi=True)
        assert cells[2:7] == [f"{float(want[k][0]):.6f}" for k in ("isnr", "si_sdr", "si_sir", "si_sar", "lsd")], (cells, want)
        assert cells[-2:] == [f"{float(want[k][0]):.6f}" for k in ("stoi", "estoi")], (cells, want)
        short += cells[-1] == "0.000010"
    assert short == 1                                                        # c.wav: 1875 samples at 10 kHz
    avg = read("enh1", "_avg_results.txt").decode("utf-8").splitlines()
    assert [a.split(":")[0] for a in avg] == header[2:]
    # without --stoi: the tool's files as before this option existed
    plain = read("plain", "_results.csv").decode().splitlines()
    assert plain[0].split(",")[:7] == ["Filename", "Length", "iSNR", "si_sdr", "si_sir", "si_sar", "lsd"] and len(plain) == 5
    assert "stoi" not in plain[0].split(",") and len(plain[0].split(",")) in (7, 9)
    assert [ln.split(",")[:7] for ln in plain[1:]] == [ln.split(",")[:7] for ln in lines[1:]]
    assert len(read("plain", "_avg_results.txt").decode("utf-8").splitlines()) == len(plain[0].split(",")) - 2


# ---- 7. pystoi, where it exists ---------------------------------------------------------------------------------------------------------------------------
def test_pystoi_cross_check(dev):
    """skipped on every machine of the project (pystoi is installed on none): where it imports, both measures of every case within 1e-6
    of pystoi.stoi (its ESTOI jitter moves the last digits)"""
    pystoi = pytest.importorskip("pystoi")
    from storm_amd import ops
    for name in SC.CASES:
        c, p = SC.signals(name)
        fs = SC.CASES[name][2]
        got = ops.stoi_rows(T(c.copy())[None].to(dev), T(p.copy())[None].to(dev), fs=fs).cpu().numpy()[0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = [pystoi.stoi(c.astype(np.float64), p.astype(np.float64), fs, extended=ext) for ext in (False, True)]
        print(f"pystoi {name}: STOI {got[0]:.9f} / {want[0]:.9f} ESTOI {got[1]:.9f} / {want[1]:.9f}")
        assert abs(got[0] - want[0]) < 1e-6 and abs(got[1] - want[1]) < 1e-6, name
