"""Metrics of enhanced audio on the device (storm_energy_ratios_rows, storm_lsd_rows and their Python / command-line surfaces) against
the REFERENCE's util/other.py: fixture F24 (tests/golden/f24_metrics.npz, written by tools/make_golden_metrics.py from the seeded
inputs of tests/metrics_cases.py) holds what the reference computed in float64 and in float32."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from tests.backend import dev  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
# SI-SDR / SI-SIR / SI-SAR / input SNR against the reference's float64 values, in dB.  Each Gram entry is a sum of L exact products accumulated
# in fp64: relative error <= L 2^-53; the ratios are inside +- 60 dB, so the expanded residual norms lose at most a factor 10^(60 / 10) to
# cancellation; times 10 / ln 10 per unit of relative error that is 48001 * 2^-53 * 1e6 * 4.35 = 2.3e-5 dB at the longest case, and a margin
# of 4 covers the order of the sums.  (The reference's own float32 run is off by up to 1.2e-4 dB on these inputs: never the yardstick.)
ENERGY_TOL_DB = 1e-4


def _case(cases, name):
    return next(c for c in cases if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _lsd_alone(kind, name):
    """util.other.lsd of one LSD case as a one-row call (computed once per backend; the `dev` fixture has loaded the backend `kind`)"""
    from storm_amd.util import other as O
    d = torch.device("cpu" if kind == "cpu" else "cuda:0")
    sh, s, _ = MC.lsd_inputs(_case(MC.LSD_CASES, name))
    return O.lsd(T(sh)[None].to(d), T(s)[None].to(d)).cpu()


def _ragged_rows(d):
    """the rows of MC.RAGGED as a zero-filled batch: (s_hat, s, n) [3, 48001] on the device, lengths"""
    rows = [MC.lsd_inputs(_case(MC.LSD_CASES, name)) for name in MC.RAGGED]
    lens = [r[0].shape[0] for r in rows]
    out = torch.zeros(3, len(rows), max(lens))
    for k, r in enumerate(rows):
        for j in range(3):
            out[j, k, :lens[k]] = T(r[j])
    return out[0].to(d), out[1].to(d), out[2].to(d), lens


# ---- 1. energy ratios and input SNR vs the reference --------------------------------------------------------------------------------------
def test_energy_ratios_vs_reference_golden(dev, golden):
    """storm_energy_ratios_rows against energy_ratios / snr_dB of the reference in float64 (util/other.py:21-44, 96-100) on F24's cases:
    lengths 1, 37, the partition boundary 16384 +- 1 and 48001, ratios between -2 and 55 dB; every number within 1e-4 dB."""
    from storm_amd import ops
    g = golden["f24_metrics"]
    assert ops.METRICS_CHUNK == MC.CHUNK and [str(v) for v in g["energy_names"]] == [c["name"] for c in MC.ENERGY_CASES]
    worst = 0.0
    for k, case in enumerate(MC.ENERGY_CASES):
        sh, s, n = MC.energy_inputs(case)
        assert MC.sha256(sh, s, n) == str(g["energy_sha"][k]), case["name"]
        want = g["energy_ref64"][k]
        assert np.all(np.abs(want) < 60.0)
        got = ops.energy_ratios_rows(T(sh)[None].to(dev), T(s)[None].to(dev), T(n)[None].to(dev)).cpu().numpy()[0]
        diff = np.abs(got - want)
        print(f"energy {case['name']}: |dB difference| vs the reference in float64 " + " ".join(f"{v:.2e}" for v in diff))
        worst = max(worst, float(diff.max()))
        assert got.dtype == np.float64 and diff.max() < ENERGY_TOL_DB, (case["name"], got, want)
    print(f"energy: largest difference {worst:.2e} dB")


# ---- 2. a row's numbers do not depend on the batch ------------------------------------------------------------------------------------------
def test_energy_rows_do_not_depend_on_the_batch(dev):
    """a ragged batch of lengths (300, 16385, 48001): every row's four numbers are the bits of its own one-row call on the trimmed row, of the
    batch with 1000 more zero columns, of the batch with its rows permuted and of a strided view (every second row of a [2 B, L] buffer)"""
    from storm_amd import ops
    sh, s, n, lens = _ragged_rows(dev)
    base = ops.energy_ratios_rows(sh, s, n, lengths=lens).cpu()
    assert base.shape == (3, 4) and base.dtype == torch.float64 and torch.isfinite(base).all()
    for k, L in enumerate(lens):
        alone = ops.energy_ratios_rows(sh[k:k + 1, :L], s[k:k + 1, :L], n[k:k + 1, :L]).cpu()
        assert torch.equal(alone[0], base[k]), (k, alone, base[k])
    wide = [torch.cat([x, torch.zeros(3, 1000, device=dev)], 1) for x in (sh, s, n)]
    assert torch.equal(ops.energy_ratios_rows(*wide, lengths=lens).cpu(), base)
    perm = [2, 0, 1]
    got = ops.energy_ratios_rows(sh[perm], s[perm], n[perm], lengths=[lens[i] for i in perm]).cpu()
    assert torch.equal(got, base[perm])
    bufs = []
    for x in (sh, s, n):
        buf = torch.full((6, x.shape[1]), 7.0, device=dev)
        buf[::2] = x
        bufs.append(buf[::2])
    assert bufs[0].stride(0) == 2 * sh.shape[1]
    assert torch.equal(ops.energy_ratios_rows(*bufs, lengths=lens).cpu(), base)


# ---- 3. log-spectral distance -----------------------------------------------------------------------------------------------------------------
def test_lsd_vs_reference_golden(dev, golden):
    """util.other.lsd (the engine's two STFTs + storm_lsd_rows) against the reference's lsd in float64 (util/other.py:16-19) on F24's cases:
    L = 256 (the shortest legal signal), 300, 16385, 48001 and one whose last 2000 samples are zeros in both signals.  Bound: 4 x the largest
    |float32 - float64| of the reference's own two runs over these cases, read from the fixture (the 4: our STFT sums in another order than torch's)."""
    g = golden["f24_metrics"]
    assert [str(v) for v in g["lsd_names"]] == [c["name"] for c in MC.LSD_CASES]
    bound = 4.0 * float(np.max(np.abs(g["lsd_ref32"] - g["lsd_ref64"])))
    assert 0.0 < bound < 1e-5
    for k, case in enumerate(MC.LSD_CASES):
        sh, s, _ = MC.lsd_inputs(case)
        assert MC.sha256(sh, s) == str(g["lsd_sha"][k]), case["name"]
        got = _lsd_alone(dev.type, case["name"])
        diff = abs(float(got[0]) - float(g["lsd_ref64"][k]))
        print(f"lsd {case['name']}: {float(got[0]):.12f}, |difference| vs the reference in float64 {diff:.2e} (bound {bound:.2e})")
        assert got.dtype == torch.float64 and got.shape == (1,) and diff < bound, (case["name"], float(got[0]), float(g["lsd_ref64"][k]))


def test_lsd_ragged_rows_equal_their_own_calls(dev):
    """rows of (300, 16385, 48001) samples in one batch with lengths=: each row's LSD is the bits of its own one-row call, and the frames past
    1 + len // 128 are never counted (whatever they hold)"""
    from storm_amd import ops
    from storm_amd.util import other as O
    sh, s, _, lens = _ragged_rows(dev)
    got = O.lsd(sh, s, lengths=lens).cpu()
    for k, name in enumerate(MC.RAGGED):
        assert torch.equal(got[k:k + 1], _lsd_alone(dev.type, name)), (name, got[k], _lsd_alone(dev.type, name))
    frames = [1 + L // 128 for L in lens]
    A, S = ops.stft(sh, lengths=lens), ops.stft(s, lengths=lens)
    assert A.shape == (3, 256, 1 + lens[2] // 128)
    assert torch.equal(ops.lsd_rows(A, S, frames=frames).cpu(), got)
    for k in range(2):
        assert float(A[k, :, frames[k]:].abs().max()) == 0.0                 # the STFT's own padding
        A[k, :, frames[k]:] = 123.0
    assert torch.equal(ops.lsd_rows(A, S, frames=frames).cpu(), got)


@pytest.mark.parametrize("T_", [1, 3, 129])
def test_lsd_rows_vs_float64_expression(dev, T_):
    """storm_lsd_rows alone on seeded complex64 spectrograms, F = 257, ragged frame counts (129 frames: three 64-frame tiles, counts on and
    next to a tile edge), some bins exactly zero: against the same expression in float64 torch.  The inputs are exact in float64 and only the
    rounding of log and sqrt remains: 1e-12 relative."""
    from storm_amd import ops
    F, eps = 257, 1e-10
    frames = {1: [1, 1, 1], 3: [3, 1, 2], 129: [129, 64, 65]}[T_]
    g = torch.Generator().manual_seed(2470 + T_)
    A = torch.complex(torch.randn(3, F, T_, generator=g), torch.randn(3, F, T_, generator=g))
    S = torch.complex(torch.randn(3, F, T_, generator=g), torch.randn(3, F, T_, generator=g)) * 0.01
    A[:, 5] = 0
    S[:, 5:7] = 0
    got = ops.lsd_rows(A.to(dev), S.to(dev), frames=frames, eps=eps).cpu()
    full = ops.lsd_rows(A[:1].to(dev), S[:1].to(dev), eps=eps).cpu()
    assert torch.equal(full[0], got[0])                                      # frames=None: every frame
    for b in range(3):
        a, s = A[b, :, :frames[b]].to(torch.complex128).abs(), S[b, :, :frames[b]].to(torch.complex128).abs()
        want = float(torch.sqrt(torch.mean(torch.abs(2 * torch.log(eps + a) - 2 * torch.log(eps + s)))))
        rel = abs(float(got[b]) - want) / want
        print(f"lsd_rows T={T_} row {b}: {float(got[b]):.15f} relative difference {rel:.2e}")
        assert rel < 1e-12, (b, float(got[b]), want)


# ---- 4. surfaces --------------------------------------------------------------------------------------------------------------------------------
def test_util_other_batch_forms(dev, golden):
    """util.other.energy_ratios / snr_dB / lsd / mean_std under the reference's names return the values of sections 1 and 3"""
    from storm_amd.util import other as O
    g = golden["f24_metrics"]
    ks = [k for k, c in enumerate(MC.ENERGY_CASES) if c["L"] == 48001][:2]
    rows = [MC.energy_inputs(MC.ENERGY_CASES[k]) for k in ks]
    sh, s, n = (torch.stack([T(r[j]) for r in rows]).to(dev) for j in range(3))
    sdr, sir, sar = O.energy_ratios(sh, s, n)
    snr = O.snr_dB(s, n)
    got = torch.stack([sdr, sir, sar, snr], 1).cpu().numpy()
    assert got.shape == (2, 4) and np.abs(got - g["energy_ref64"][ks]).max() < ENERGY_TOL_DB
    one = O.energy_ratios(sh[0], s[0], n[0])                                # 1-D tensors: one row
    assert all(v.shape == (1,) for v in one) and float(one[0][0]) == float(sdr[0])
    k = [c["name"] for c in MC.LSD_CASES].index("L300")
    bound = 4.0 * float(np.max(np.abs(g["lsd_ref32"] - g["lsd_ref64"])))
    assert abs(float(_lsd_alone(dev.type, "L300")[0]) - float(g["lsd_ref64"][k])) < bound
    m, sd = O.mean_std(np.array([1.0, np.nan, 3.0, 5.0]))
    assert m == 3.0 and abs(sd - np.std([1.0, 3.0, 5.0])) < 1e-15
    m, sd = O.mean_std(torch.tensor([2.0, float("nan"), 4.0], dtype=torch.float64))
    assert (m, sd) == (3.0, 1.0)


def test_score_batch_keys_and_shapes(dev):
    from storm_amd import ops
    from storm_amd.util import other as O
    from storm_amd.util.inference import score_batch
    rows = [MC.lsd_inputs(_case(MC.LSD_CASES, name)) for name in ("L300", "L256")]
    lens = [300, 256]
    est, clean, noise = (torch.zeros(2, 300) for _ in range(3))
    for k, r in enumerate(rows):
        est[k, :lens[k]], clean[k, :lens[k]], noise[k, :lens[k]] = T(r[0]), T(r[1]), T(r[2])
    est, clean, noisy = est.to(dev), clean.to(dev), (clean + noise).to(dev)
    got = score_batch(clean, noisy, est, lengths=lens)
    assert sorted(got) == ["isnr", "lsd", "si_sar", "si_sdr", "si_sir"]
    assert all(v.shape == (2,) and v.dtype == torch.float64 and torch.isfinite(v).all() for v in got.values())
    r = ops.energy_ratios_rows(est, clean, noisy - clean, lengths=lens)
    for j, key in enumerate(("si_sdr", "si_sir", "si_sar", "isnr")):
        assert torch.equal(got[key], r[:, j])
    assert torch.equal(got["lsd"], O.lsd(est, clean, lengths=lens))
    assert torch.equal(got["lsd"][1:].cpu(), _lsd_alone(dev.type, "L256"))
    assert -5.0 < float(got["isnr"][0]) < 5.0 and float(got["si_sdr"][0]) > 0.0


def test_evaluate_model_metrics(dev, golden):
    """evaluate_model(..., metrics=True) on F10's pairs with injected per-file noise: six elements, the first five equal to those of the
    metrics=False call, the sixth the means of score_batch's numbers over the files"""
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import ScoreModel
    from storm_amd.util.inference import METRIC_KEYS, evaluate_model, score_batch
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
    full = evaluate_model(m, 3, metrics=True, **kw)
    assert len(plain) == 5 and len(full) == 6
    assert plain[1] == full[1] and all(a == b or (a != a and b != b) for a, b in ((plain[0], full[0]), (plain[2], full[2])))
    assert plain[3] is None and full[3] is None
    assert all(torch.equal(a, b) for la, lb in zip(plain[4], full[4]) for a, b in zip(la, lb))
    scores = full[5]
    assert sorted(scores) == sorted(METRIC_KEYS) and all(isinstance(v, float) and np.isfinite(v) for v in scores.values())
    each = [score_batch(pairs[i][0].to(dev), pairs[i][1].to(dev), full[4][1][i][None].to(dev)) for i in range(3)]
    for key in METRIC_KEYS:
        want = float(torch.cat([e[key] for e in each]).mean())
        assert abs(scores[key] - want) <= 1e-12 * max(1.0, abs(want)), (key, scores[key], want)
    assert abs(scores["si_sdr"] - full[1]) < 2e-3                            # storm_si_sdr (eps = 0, fp32 out) on the same estimates


def test_metric_errors(dev):
    from storm_amd import _lib, ops
    from storm_amd.util import other as O
    x = torch.zeros(2, 400, device=dev)
    with pytest.raises(ValueError, match="400"):
        ops.energy_ratios_rows(x, x, x[:, :399])
    with pytest.raises(ValueError):
        ops.energy_ratios_rows(x, x, x.double())
    for bad in ([400], [400, 401], [0, 400]):
        with pytest.raises(ValueError, match="lengths"):
            ops.energy_ratios_rows(x, x, x, lengths=bad)
    S = torch.zeros(2, 257, 4, dtype=torch.complex64, device=dev)
    with pytest.raises(ValueError):
        ops.lsd_rows(S, S[:, :, :3])
    with pytest.raises(ValueError):
        ops.lsd_rows(S, torch.view_as_real(S)[..., 0])
    for bad in ([4], [4, 5], [0, 4]):
        with pytest.raises(ValueError, match="frames"):
            ops.lsd_rows(S, S, frames=bad)
    with pytest.raises(ValueError, match="too short"):
        O.lsd(x[:, :255], x[:, :255])
    with pytest.raises(ValueError, match="too short"):
        O.lsd(x, x, lengths=[400, 255])
    with pytest.raises(ValueError):
        O.lsd(x, x[:, :300])
    if dev.type == "cuda":                                                   # the product has no CPU path: host tensors are refused
        c = torch.zeros(1, 400)
        with pytest.raises(_lib.StormError):
            ops.energy_ratios_rows(c, c, c)
        Sc = torch.zeros(1, 257, 4, dtype=torch.complex64)
        with pytest.raises(_lib.StormError):
            ops.lsd_rows(Sc, Sc)


# ---- 5. command line ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calc_metrics_cli(tmp_path):
    """calc_metrics.py on three 16 kHz triples of 6000 / 4321 / 9000 samples (one member of each a little longer: trimmed) and one 8 kHz triple,
    with --resample: --batch 1 and --batch 3 write the same bytes, every value is score_batch's of the trimmed triple to the printed decimals,
    the averages are mean_std of the columns, and the 8 kHz file reports its length at 16 kHz"""
    from scipy.io import wavfile

    from storm_amd.data_module import SpecsDataModule
    from storm_amd.util.inference import score_batch
    from storm_amd.util.other import mean_std
    dirs = {k: os.path.join(tmp_path, k) for k in ("clean", "noisy", "enh1", "enh3")}
    for d in dirs.values():
        os.makedirs(d)
    g = torch.Generator().manual_seed(2480)
    triples = {}
    for name, L, sr, extra in (("a.wav", 6000, 16000, (0, 17, 0)), ("b.wav", 4321, 16000, (5, 0, 0)), ("c.wav", 9000, 16000, (0, 0, 33)), ("d.wav", 4000, 8000, (0, 0, 0))):
        s, n = 0.1 * torch.randn(L + 40, generator=g), 0.05 * torch.randn(L + 40, generator=g)
        x, y, e = s[:L + extra[0]], (s + n)[:L + extra[1]], (0.8 * s + 0.3 * n)[:L + extra[2]]
        triples[name] = (x, y, e, L, sr)
        for key, w in (("clean", x), ("noisy", y), ("enh1", e), ("enh3", e)):
            wavfile.write(os.path.join(dirs[key], name), sr, w.numpy().astype(np.float32))
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=ROOT).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for key, batch in (("enh1", "1"), ("enh3", "3")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "calc_metrics.py"), "--clean_dir", dirs["clean"], "--noisy_dir", dirs["noisy"],
                            "--enhanced_dir", dirs[key], "--batch", batch, "--resample"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    csv1 = open(os.path.join(dirs["enh1"], "_results.csv"), "rb").read()
    assert csv1 == open(os.path.join(dirs["enh3"], "_results.csv"), "rb").read()
    assert open(os.path.join(dirs["enh1"], "_avg_results.txt"), "rb").read() == open(os.path.join(dirs["enh3"], "_avg_results.txt"), "rb").read()
    lines = csv1.decode().splitlines()
    header = lines[0].split(",")
    assert header[:7] == ["Filename", "Length", "iSNR", "si_sdr", "si_sir", "si_sar", "lsd"] and len(lines) == 5
    dev_ = torch.device("cuda:0")
    table = {}
    for line in lines[1:]:
        cells = line.split(",")
        x, y, e, L, sr = triples[cells[0]]
        x, y, e = (SpecsDataModule.resample(w.to(dev_), sr, 16000) for w in (x, y, e))
        n = min(len(x), len(y), len(e))
        assert n == L * 16000 // sr and cells[1] == str(n)
        want = score_batch(x[None, :n], y[None, :n], e[None, :n])
        assert cells[2:7] == [f"{float(want[k][0]):.6f}" for k in ("isnr", "si_sdr", "si_sir", "si_sar", "lsd")], (cells, want)
        table[cells[0]] = cells
    assert table["d.wav"][1] == "8000"
    avg = open(os.path.join(dirs["enh1"], "_avg_results.txt"), encoding="utf-8").read().splitlines()
    assert len(avg) == len(header) - 2
    for j, name in enumerate(header[2:]):
        m, sd = mean_std(np.array([float(table[f][2 + j]) for f in sorted(table)]))
        assert avg[j] == f"{name}: {m:.6f} ± {sd:.6f}"
