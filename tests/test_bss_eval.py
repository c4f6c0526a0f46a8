"""BSS-eval SDR / SIR / SAR with two sources on the device (storm_bss_eval_rows: the correlations of four pairs per piece, round 18's solve for
the SDR, a block Levinson recursion per row for the joint projection) and its Python / command-line surfaces - the correlations bit for bit
against storm_bss_sdr_rows and the np.cumsum restatement, the solve against two dense host solvers on the device's own correlations and
against the time-domain least-squares form (tests/bss_eval_cases.py), anchors that need no solver.  include/storm_hip.h is the specification."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl
import torch

from tests import bss_cases as BC
from tests import bss_eval_cases as EC
from tests.backend import dev, switch  # noqa: F401

T = torch.from_numpy
DB_TOL = 1e-4                    # the project's bound for dB numbers (tests/test_metrics.py), the issue's bound for sir and sar
SOLVERS_AGREE = 1e-8             # dB: the two host solvers among themselves, before either is a reference
COND_CAP = 1e8                   # joint condition number up to which the bound is asserted
TIME_DOMAIN_TOL = 1e-6           # dB against the lstsq form at F = 8, L = 500
SYM_TOL = 1e-8                   # dB: sar with the two sources exchanged
CLOSED_TOL = 1e-10               # dB: F = 1 against the closed 2 x 2 form
FILT_TOL = 1e-8                  # relative L2 of the recovered filters of an exact estimate


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


def _one(v, d):
    return T(np.ascontiguousarray(v))[None].to(d)


def _same(a, b):
    """bit-equal, NaNs included"""
    return a.shape == b.shape and np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


# ---- 1. correlations bit for bit; 2. the sdr column -------------------------------------------------------------------------------------
def _ragged_rows():
    """the issue's lengths, then an all-zero estimate (NaN) and an estimate that is twice the target (nothing left: +inf)"""
    rows = [EC.ragged_triple(L) for L in EC.LENGTHS]
    s1, s2, _ = EC.ragged_triple(700)
    return rows + [(s1, s2, np.zeros(700, np.float32)), (s1, s2, 2.0 * s1)]


def _ragged_batch(d):
    rows = _ragged_rows()
    tgt, lens = _batch([r[0] for r in rows], d, junk=7.0, offset=1)
    noi, _ = _batch([r[1] for r in rows], d, junk=5.0, offset=2)
    est, _ = _batch([r[2] for r in rows], d, junk=-3.0, offset=3)
    return rows, tgt, noi, est, lens


def _check_parts(d, flen, who):
    """parts of the ragged batch (junk past every length, rows off the 16-byte grid, strides wider than the batch) = the concatenation of
    storm_bss_sdr_rows' parts of the four pairs = the np.cumsum restatement; the sdr column = storm_bss_sdr_rows(target, estimate)"""
    from storm_amd import ops
    rows, tgt, noi, est, lens = _ragged_batch(d)
    out, parts = ops.bss_eval_rows(tgt, noi, est, lengths=lens, flen=flen, return_parts=True)
    assert out.dtype == parts.dtype == torch.float64 and out.shape == (len(rows), 3) and parts.shape == (len(rows), 6 * flen + 1)
    F = flen
    sdr, a = ops.bss_sdr_rows(tgt, est, lengths=lens, flen=F, return_parts=True)
    b, c, e = (ops.bss_sdr_rows(u, v, lengths=lens, flen=F, return_parts=True)[1] for u, v in ((noi, est), (tgt, noi), (noi, tgt)))
    four = torch.cat([a[:, :F], a[:, F:2 * F], b[:, :F], b[:, F:2 * F], c[:, F:2 * F], e[:, F:2 * F], a[:, 2 * F:]], dim=1)
    assert _same(parts, four), (who, flen)
    parts = parts.cpu().numpy()
    for k, L in enumerate(EC.LENGTHS):
        assert np.array_equal(_bits(parts[k]), _bits(EC.restated_parts(L, F))), (who, L, flen)
    X12, X21 = parts[:, 4 * F:5 * F], parts[:, 5 * F:6 * F]
    assert F == 1 or not np.array_equal(X12[6], X21[6])                      # (the noise row holds the target three samples late)
    assert _same(out[:, 0], sdr), (who, flen)                                # 2. the same bits, NaN and inf rows included
    n = len(EC.LENGTHS)
    assert bool(torch.isnan(out[n]).all()) and float(out[n + 1, 0]) == np.inf and bool(torch.isfinite(out[2:n, 0]).all())


@pytest.mark.parametrize("flen", EC.FLENS)
def test_correlations_and_sdr_column_bit_equal(dev, flen):
    _check_parts(dev, flen, "launcher's rule")


@pytest.mark.parametrize("flen", EC.FLENS)
@pytest.mark.parametrize("R", [2, 4, 8])
def test_lags_per_thread_change_no_bit(dev, switch, R, flen):
    """every lags-per-thread choice of the launcher (forced through the library's test switch) on the same ragged batch"""
    switch("STORM_BSS_LAGS", R)
    _check_parts(dev, flen, f"R={R}")


# ---- 3. the solve against two host solvers on the device's own correlations ---------------------------------------------------------------
SOLVE_CASES = [(p, 4097, F) for p in EC.PAIRS for F in (1, 2, 3, 64)] + [(p, 20000, 512) for p in EC.PAIRS]


def _host(parts, F):
    M, _ = EC.joint_system(parts, F)
    cond = float(np.linalg.cond(M))
    dense = EC.numbers(parts, F, np.linalg.solve)[0]
    pos = EC.numbers(parts, F, lambda A, y: sl.solve(A, y, assume_a="pos"))[0]
    return cond, dense, pos


@pytest.mark.parametrize("colours,L,flen", SOLVE_CASES, ids=[f"{c[0]}+{c[1]}-{L}-{F}" for c, L, F in SOLVE_CASES])
def test_solve_against_two_host_solvers(dev, colours, L, flen):
    """np.linalg.solve and scipy.linalg.solve(assume_a='pos') on the 2 F x 2 F matrix built here from the device's parts: first the host
    alone (condition <= 1e8, the two solvers within 1e-8 dB), then the device's sir and sar within 1e-4 dB of both"""
    from storm_amd import ops
    s1, s2, e = EC.triple(colours, L, flen)
    out, parts = (v.cpu().numpy()[0] for v in ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=flen, return_parts=True))
    cond, dense, pos = _host(parts, flen)
    apart = float(np.abs(dense - pos).max())
    gap = float(max(np.abs(out[1:] - dense[1:]).max(), np.abs(out[1:] - pos[1:]).max()))
    print(f"bss_eval {colours[0]}/{colours[1]} L={L} F={flen}: sdr {out[0]:.4f} sir {out[1]:.4f} sar {out[2]:.4f} dB, joint condition {cond:.2e}, "
          f"|solvers apart| {apart:.2e} dB, |device - host solvers| {gap:.2e} dB (sdr {abs(out[0] - dense[0]):.2e})")
    assert cond <= COND_CAP and apart <= SOLVERS_AGREE
    assert -15.0 < out[1] < 40.0 and -15.0 < out[2] < 40.0                   # (inputs: what the issue's CPU check of this recipe gave)
    assert gap <= DB_TOL and abs(out[0] - dense[0]) <= DB_TOL


def test_lowpass_pair_is_printed(dev):
    """a low-pass pair: asserted like the others while its joint condition is below the cap, printed only above it"""
    from storm_amd import ops
    s1, s2, e = EC.triple(("lowpass", "lowpass"), 4097, 64)
    out, parts = (v.cpu().numpy()[0] for v in ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=64, return_parts=True))
    cond, dense, pos = _host(parts, 64)
    gap = float(max(np.abs(out[1:] - dense[1:]).max(), np.abs(out[1:] - pos[1:]).max()))
    print(f"bss_eval lowpass/lowpass L=4097 F=64: {out}, joint condition {cond:.2e}, |solvers apart| {np.abs(dense - pos).max():.2e} dB, "
          f"|device - host solvers| {gap:.2e} dB")
    assert cond > COND_CAP or gap <= DB_TOL


# ---- 4. the definition against the time-domain form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("colours", EC.PAIRS, ids=["+".join(c) for c in EC.PAIRS])
def test_time_domain_least_squares(dev, colours):
    """mir_eval's formulation at F = 8, L = 500: lstsq onto the zero-padded delayed copies, energies of the projected signals"""
    from storm_amd import ops
    s1, s2, e = EC.triple(colours, 500, 8)
    got = ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=8).cpu().numpy()[0]
    want = EC.time_domain(s1, s2, e, 8)
    print(f"bss_eval {colours} F=8 L=500: device {got}, time domain {want}, apart {np.abs(got - want).max():.2e} dB")
    assert np.abs(got - want).max() <= TIME_DOMAIN_TOL


# ---- 5. exactness and symmetry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", [64, 512])
def test_exact_estimate(dev, flen):
    """an estimate that is exactly h1 * target + h2 * noise (EC.exact_triple: no rounding anywhere, no tail cut off): no artefacts are left
    and the joint solve returns the two filters.  The inputs are exact on purpose: one rounding of the estimate to fp32 alone would move the
    filters by about 2^-24 sqrt(2 F / L), which is the bound itself at these sizes."""
    from storm_amd import ops
    L = 4097
    s1, s2, e, h1, h2 = EC.exact_triple(L, flen)
    out, filt = ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=flen, return_filter=True)
    out, filt = out.cpu().numpy()[0], filt.cpu().numpy()[0]
    want = np.zeros((2, flen))
    want[0, :len(h1)], want[1, :len(h2)] = h1, h2
    rel = float(np.linalg.norm(filt - want) / np.linalg.norm(want))
    print(f"exact estimate F={flen}: sdr {out[0]:.3f} sir {out[1]:.3f} sar {out[2]}, filters rel. L2 {rel:.2e}")
    assert filt.shape == (2, flen) and (out[2] == np.inf or out[2] >= 120.0)
    assert rel <= FILT_TOL


def test_sar_is_symmetric_in_the_sources(dev):
    from storm_amd import ops
    for colours in EC.PAIRS:
        s1, s2, e = EC.triple(colours, 4097, 64)
        a = float(ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=64)[0, 2])
        b = float(ops.bss_eval_rows(_one(s2, dev), _one(s1, dev), _one(e, dev), flen=64)[0, 2])
        print(f"sar {colours}: {a:.12f} and, sources exchanged, {b:.12f}")
        assert abs(a - b) <= SYM_TOL


def test_one_tap_closed_form(dev):
    """F = 1: the 2 x 2 system by Cramer's rule in numpy from the device's parts"""
    from storm_amd import ops
    for colours in EC.PAIRS:
        s1, s2, e = EC.triple(colours, 4097, 1)
        out, parts = (v.cpu().numpy()[0] for v in ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=1, return_parts=True))
        G11, D1, G22, D2, X12, X21, Ee = parts
        assert _bits(X12) == _bits(X21)
        det = G11 * G22 - X12 * X12
        P12 = D1 * (G22 * D1 - X12 * D2) / det + D2 * (G11 * D2 - X12 * D1) / det
        want = EC.ratios(D1 * D1 / G11, P12, Ee)
        print(f"one tap {colours}: device {out}, closed form {want}")
        assert np.abs(out - want).max() <= CLOSED_TOL


# ---- 6. edge rules --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", [64, 512])
def test_edge_rows_and_their_neighbours(dev, flen):
    from storm_amd import ops
    L = 700
    s1, s2, e = EC.triple(("white", "white"), L, 64)
    t1, t2, te = EC.triple(("ar2", "white"), L, 64)
    z = np.zeros(L, np.float32)
    #        plain         silent noise  noise = half the target  no samples     all-zero estimate  plain
    tgts = [s1, s1, s1, s1, s1, t1]
    nois = [s2, z, 0.5 * s1, s2, s2, t2]
    ests = [e, e, e, e, z, te]
    lens = [L, L, L, 0, L, L]
    tgt, noi, est = (_batch(v, dev, junk=2.0)[0] for v in (tgts, nois, ests))
    out, filt, parts = ops.bss_eval_rows(tgt, noi, est, lengths=lens, flen=flen, return_filter=True, return_parts=True)
    nan, fin = torch.isnan(out), torch.isfinite(out)
    assert fin[0].all() and fin[5].all() and bool(torch.isfinite(filt[0]).all()) and bool(torch.isfinite(filt[5]).all())
    for k in (1, 2):                                                         # sdr is still given; sir, sar and the filters are NaN
        assert bool(fin[k, 0]) and bool(nan[k, 1:].all()) and bool(torch.isnan(filt[k]).all())
        assert float(out[k, 0]) == float(ops.bss_sdr_rows(tgt[k:k + 1, :L], est[k:k + 1, :L], flen=flen)[0])
    for k in (3, 4):                                                         # whatever makes the SDR NaN makes all three NaN
        assert bool(nan[k].all()) and bool(torch.isnan(filt[k]).all())
    assert not parts[3].any() and float(parts[1, 2 * flen]) == 0.0           # (no samples: zeros; silent noise: G22[0] == 0)
    for k in (0, 5):
        alone = ops.bss_eval_rows(_one(tgts[k], dev), _one(nois[k], dev), _one(ests[k], dev), flen=flen, return_filter=True, return_parts=True)
        assert all(_same(g[k], a[0]) for g, a in zip((out, filt, parts), alone)), k


def test_two_samples_and_512_taps(dev):
    """L = 2 with F = 512: 1024 delayed copies in 513 dimensions are dependent whatever the samples are - sir and sar are NaN by the row's
    length (the header's rule), the sdr (512 copies of one row: independent) is still round 18's number; the neighbour keeps its bits"""
    from storm_amd import ops
    s1, s2, e = EC.triple(("white", "white"), 700, 64)
    two = [np.array([0.5, -0.25], np.float32), np.array([0.125, 1.0], np.float32), np.array([0.75, 0.5], np.float32)]
    tgt, lens = _batch([two[0], s1], dev, junk=4.0)
    noi, est = _batch([two[1], s2], dev, junk=4.0)[0], _batch([two[2], e], dev, junk=4.0)[0]
    out, filt = ops.bss_eval_rows(tgt, noi, est, lengths=lens, flen=512, return_filter=True)
    assert not bool(torch.isnan(out[0, 0])) and bool(torch.isnan(out[0, 1:]).all()) and bool(torch.isnan(filt[0]).all())
    assert float(out[0, 0]) == float(ops.bss_sdr_rows(_one(two[0], dev), _one(two[2], dev), flen=512)[0])
    alone = ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=512, return_filter=True)
    assert _same(out[1], alone[0][0]) and _same(filt[1], alone[1][0]) and bool(torch.isfinite(out[1]).all())
    # F = 1 on the same two samples: two copies in two dimensions, a solvable system
    assert bool(torch.isfinite(ops.bss_eval_rows(_one(two[0], dev), _one(two[1], dev), _one(two[2], dev), flen=1)[0, :2]).all())


# ---- 7. batch independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", [64, 512])
def test_a_row_does_not_depend_on_its_batch(dev, flen):
    """a row alone; first and last in a ragged batch of three rows of different lengths and levels; as a strided view off the 16-byte grid;
    with and without the optional outputs: out, filters and correlations are the same bits"""
    from storm_amd import ops
    L = BC.PIECE + 511
    row = EC.ragged_triple(L)
    others = [EC.triple(("white", "white"), 700, 64), EC.triple(("ar2", "white"), 4097, 64)]
    alone = ops.bss_eval_rows(*(_one(v, dev) for v in row), flen=flen, return_filter=True, return_parts=True)
    assert bool(torch.isfinite(alone[0]).all())
    for pos, offset in ((0, 0), (2, 3)):
        rows = others.copy()
        rows.insert(pos, row)
        scale = [1000.0 if len(r[0]) == 700 else 1.0 for r in rows]
        tgt, lens = _batch([k * r[0] for k, r in zip(scale, rows)], dev, width=L + 5 * offset, junk=9.0, offset=offset)
        noi = _batch([r[1] for r in rows], dev, width=L + 5 * offset, junk=1.0, offset=offset)[0]
        est = _batch([r[2] for r in rows], dev, width=L + 5 * offset, junk=-9.0, offset=offset)[0]
        got = ops.bss_eval_rows(tgt, noi, est, lengths=lens, flen=flen, return_filter=True, return_parts=True)
        assert all(_same(g[pos], a[0]) for g, a in zip(got, alone)), (pos, offset)
        plain = ops.bss_eval_rows(tgt, noi, est, lengths=lens, flen=flen)
        assert isinstance(plain, torch.Tensor) and _same(plain, got[0])


# ---- 8. surfaces --------------------------------------------------------------------------------------------------------------------------
def _files(L, seed):
    g = torch.Generator().manual_seed(seed)
    s, n = 0.1 * torch.randn(L, generator=g), 0.05 * torch.randn(L, generator=g)
    est = 0.8 * s + 0.3 * n + 0.01 * torch.randn(L, generator=g)
    late = torch.zeros(L)
    late[3:] = est[:L - 3]                                                   # three samples late
    return s, s + n, late


def test_util_other_bss_eval(dev):
    from storm_amd import ops
    from storm_amd.util.other import bss_eval
    s1, s2, e = EC.triple(("ar2", "white"), 4097, 64)
    want = ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev))
    got = bss_eval(T(s1).to(dev), T(s2).to(dev), T(e).to(dev))
    assert all(isinstance(v, float) for v in got) and list(got) == want[0].tolist()
    rows = bss_eval(T(np.stack([s1, s2])).to(dev), T(np.stack([s2, s1])).to(dev), T(np.stack([e, e])).to(dev), flen=64, lengths=[4097, 1000])
    assert len(rows) == 3 and all(r.shape == (2,) and r.dtype == torch.float64 and r.device.type == dev.type for r in rows)
    assert [float(r[0]) for r in rows] == ops.bss_eval_rows(_one(s1, dev), _one(s2, dev), _one(e, dev), flen=64)[0].tolist()


def test_score_batch_bss(dev):
    """score_batch(bss=True): the three keys are the separate ops call on (clean, noisy - clean, estimate) bit for bit, on what hp= and
    align= leave; every other key keeps its bits and, without the keyword, the keys are the ones of before"""
    from storm_amd import ops
    from storm_amd.util.inference import score_batch
    lens = [2000, 1500]
    x, y, e = (torch.zeros(2, 2000) for _ in range(3))
    for k, L in enumerate(lens):
        x[k, :L], y[k, :L], e[k, :L] = _files(L, 70 + k)
    x, y, e = (v.to(dev) for v in (x, y, e))
    keys = ("bss_sdr", "bss_sir", "bss_sar")
    cols = lambda d: torch.stack([d[k] for k in keys], dim=1)                # noqa: E731
    plain = score_batch(x, y, e, lengths=lens)
    assert list(plain) == ["si_sdr", "si_sir", "si_sar", "lsd", "isnr"]
    got = score_batch(x, y, e, lengths=lens, bss=True)
    assert list(got) == list(plain) + list(keys) and all(_same(got[k], plain[k]) for k in plain)
    assert _same(cols(got), ops.bss_eval_rows(x, y - x, e, lengths=lens))
    assert _same(cols(score_batch(x, y, e, lengths=lens, bss=True, bss_taps=64)), ops.bss_eval_rows(x, y - x, e, lengths=lens, flen=64))
    both = score_batch(x, y, e, lengths=lens, sdr=True, sdr_taps=64, bss=True, bss_taps=64)
    assert list(both)[-4:] == ["sdr"] + list(keys) and _same(both["sdr"], both["bss_sdr"])
    assert float(got["bss_sir"][0]) > float(got["si_sir"][0]) + 5.0          # the delay is inside the filter
    # align: on the moved estimate, lag stays last; hp: on the filtered rows
    al, alb = score_batch(x, y, e, lengths=lens, align=True), score_batch(x, y, e, lengths=lens, align=True, bss=True, bss_taps=64)
    assert alb["lag"].tolist() == [3, 3] and list(alb)[-1] == "lag" and all(_same(al[k], alb[k]) for k in al)
    back, _ = ops.xcorr_lag_rows(e, x, lengths=lens, ref_lengths=lens)
    assert _same(cols(alb), ops.bss_eval_rows(x, y - x, ops.shift_rows(e, back, lengths=lens, wrap=False), lengths=lens, flen=64))
    sos = ops.butter_sos(10, 80 / 16000 * 2)
    f = [ops.sosfilt_rows(v, sos, lengths=lens, out_dtype=torch.float32) for v in (x, y, e)]
    hp, hpb = score_batch(x, y, e, lengths=lens, hp=80), score_batch(x, y, e, lengths=lens, hp=80, bss=True, bss_taps=64)
    assert all(_same(hp[k], hpb[k]) for k in hp) and _same(cols(hpb), ops.bss_eval_rows(f[0], f[1] - f[0], f[2], lengths=lens, flen=64))


@pytest.mark.gpu
def test_calc_metrics_cli_bss(tmp_path, monkeypatch):
    """calc_metrics.py --bss 64 on three short files (its main() under the command line's argv, as tests/test_bss_sdr.py runs it): the columns
    bss_sdr,bss_sir,bss_sar stand after sdr where present and before lag, a line does not depend on --batch, the values are score_batch's
    per file, and without the flag the header is the unchanged one"""
    from scipy.io import wavfile

    import calc_metrics
    from storm_amd.util.inference import score_batch
    from tests.backend import setup_backend
    setup_backend("hip")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "plain", "b1", "b3", "all")}
    for d in dirs.values():
        os.makedirs(d)
    triples = {}
    for name, L in (("a.wav", 6000), ("b.wav", 5700), ("c.wav", 5000)):
        triples[name] = _files(L, L)
        for key, w in [("clean", triples[name][0]), ("noisy", triples[name][1])] + [(k, triples[name][2]) for k in ("plain", "b1", "b3", "all")]:
            wavfile.write(os.path.join(dirs[key], name), 16000, w.numpy().astype(np.float32))
    runs = {"plain": [], "b1": ["--bss", "64", "--batch", "1"], "b3": ["--bss", "64", "--batch", "3"],
            "all": ["--bss", "64", "--sdr", "64", "--stoi", "--align", "--hp-filter", "--resample", "--batch", "2"]}
    for key, extra in runs.items():
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"], "--enhanced_dir", dirs[key]] + extra)
        calc_metrics.main()
    read = lambda key, f="_results.csv": open(os.path.join(dirs[key], f), "rb").read().decode("utf-8").splitlines()    # noqa: E731
    head = read("plain")[0].split(",")
    assert head[:7] == ["Filename", "Length", "iSNR", "si_sdr", "si_sir", "si_sar", "lsd"] and not any("bss" in c for c in head)
    assert read("b1") == read("b3") and read("b1")[0].split(",") == head + ["bss_sdr", "bss_sir", "bss_sar"]
    assert [ln.split(",")[:-3] for ln in read("b1")[1:]] == [ln.split(",") for ln in read("plain")[1:]]
    assert read("all")[0].split(",")[-7:] == ["stoi", "estoi", "sdr", "bss_sdr", "bss_sir", "bss_sar", "lag"]
    assert [ln.split(":")[0] for ln in read("b1", "_avg_results.txt")[-3:]] == ["bss_sdr", "bss_sir", "bss_sar"]
    dev_ = torch.device("cuda:0")
    for key, kw, at in (("b1", {}, -3), ("all", dict(align=True, hp=80.0), -4)):
        for line in read(key)[1:]:
            cells = line.split(",")
            s, n, late = (w.to(dev_)[None] for w in triples[cells[0]])
            want = score_batch(s, n, late, bss=True, bss_taps=64, **kw)
            assert cells[at:at + 3 or None] == [f"{float(want[k][0]):.6f}" for k in ("bss_sdr", "bss_sir", "bss_sar")], (key, line)
    assert [ln.split(",")[-1] for ln in read("all")[1:]] == ["3", "3", "3"] and f"{float('inf'):.6f}" == "inf"


def test_calc_metrics_refuses_taps_outside_1_to_512(monkeypatch, capsys):
    """--bss 0 and --bss 513 are argument errors (before any file is read or the device is touched)"""
    import calc_metrics
    for bad in ("0", "513"):
        monkeypatch.setattr(sys, "argv", ["calc_metrics.py", "--clean_dir", "c", "--noisy_dir", "n", "--enhanced_dir", "e", "--bss", bad])
        with pytest.raises(SystemExit) as exc:
            calc_metrics.main()
        assert exc.value.code == 2 and "--bss TAPS" in capsys.readouterr().err


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument(dev):
    from storm_amd import _lib, ops
    from storm_amd._lib import StormError
    x = torch.zeros(2, 100, device=dev)
    for flen in (0, -1, 513):
        with pytest.raises(StormError, match="flen"):
            ops.bss_eval_rows(x, x, x, flen=flen)
    with pytest.raises(ValueError, match="lengths"):
        ops.bss_eval_rows(x, x, x, lengths=[100, 101])
    with pytest.raises(ValueError, match="noise"):
        ops.bss_eval_rows(x, x.double(), x)
    with pytest.raises(ValueError, match="bss_eval_rows"):
        ops.bss_eval_rows(x, x, x[:, :99])
    lib = _lib.lib()
    q = lib.storm_bss_eval_scratch_bytes
    assert q(2, 100, 512) == 4 * 2 * 1025 * 8 + 2 * 8 and q(2, BC.PIECE + 1, 3) == 4 * 2 * 2 * 7 * 8 + 2 * 8
    assert q(3, 100, 8) == 4 * lib.storm_bss_sdr_scratch_bytes(3, 100, 8) + 3 * 8
    assert 0 == q(0, 100, 8) == q(65536, 100, 8) == q(1, 0, 8) == q(1, 2 ** 30 + 1, 8) == q(1, 100, 0) == q(1, 100, 513)
    need = q(2, 100, 512)
    out, ws = torch.full((2, 3), 7.0, dtype=torch.float64, device=dev), torch.zeros(need // 8, dtype=torch.float64, device=dev)
    p = x.data_ptr()

    def call(t=p, n=p, e=p, o=out.data_ptr(), w=ws.data_ptr(), B=2, L=100, flen=512, bytes_=need, strides=(100, 100, 100)):
        return lib.storm_bss_eval_rows(t, n, e, o, None, None, w, bytes_, B, L, *strides, None, flen, _lib.stream())
    for kw, word in ((dict(t=None), "null pointer"), (dict(n=None), "null pointer"), (dict(e=None), "null pointer"), (dict(o=None), "null pointer"),
                     (dict(w=None), "null pointer"), (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(L=0), "L=0"), (dict(L=2 ** 30 + 1), "L="),
                     (dict(bytes_=need - 8), "scratch"), (dict(flen=0), "flen=0"), (dict(flen=513), "flen=513"),
                     (dict(strides=(99, 100, 100)), "strides 99"), (dict(strides=(100, 100, 99)), "strides 100 100 99")):
        assert call(**kw) != 0 and word in lib.storm_last_error().decode(), kw
    assert bool((out == 7.0).all())                                          # no kernel ran
    assert call() == 0 and bool(torch.isnan(out).all())                      # (all-zero rows: NaN)


# ---- 10. the kernels under the simulator's skewed wave schedules ----------------------------------------------------------------------------
SKEWED = ["tests/test_bss_eval.py::test_edge_rows_and_their_neighbours[sim-512]",       # four waves per correlation workgroup, the solves, every edge row
          "tests/test_bss_eval.py::test_solve_against_two_host_solvers[sim-ar2+white-4097-64]"]


@pytest.mark.parametrize("waves", ["reverse", "first", "last"])
def test_kernels_under_skewed_wave_schedules(waves):
    """the four-pair correlation grid and the joint solve with the simulator's waves run in another order (STORM_SIM_WAVES, read when the
    simulation is loaded: a process of its own, as tests/test_sim_schedules.py runs its selection): the same cases pass"""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, STORM_SIM_WAVES=waves, STORM_TEST_WORKERS="2")
    env.pop("STORM_SIM_DMA", None)
    r = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(root, t) for t in SKEWED] + ["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(SKEWED) and "skipped" not in r.stdout, r.stdout[-1000:]
