"""Resampling on the device (storm_resample_taps / storm_resample_poly, ops.resample_poly, SpecsDataModule.resample, the sr= keyword of the
model classes and enhancement.py --resample): audio at any sample rate through a 16 kHz model.

The operation is scipy.signal.resample_poly(x, up, down) with its defaults - the Kaiser(5) windowed sinc of 2 * 10 * max(up, down) + 1
taps - so scipy is the oracle: its firwin for the taps (designed in fp64 on both sides: only the final rounding to fp32 can differ), its
resample_poly in fp64 for the signals.  The kernel sums every output as one fp32 FMA chain; the same sum restated in fp32 on the host
gives rel-L2 0.2 - 1.7e-7 against the fp64 oracle, and the bound is the project's fp32 bound for single kernels (tests/test_convtasnet.py)."""
import math
import os

import numpy as np
import pytest
import torch

from tests.backend import dev, switch  # noqa: F401
from tests.util import rel_l2

F32_TOL = 2e-6
TAP_RATIOS = [(1, 3), (3, 1), (160, 441), (441, 160), (3, 2), (441, 640)]
IMPULSE_CASES = [(1, 3, 40), (3, 1, 40), (160, 441, 300), (441, 160, 300)]
# (1, 12) is not on the issue's list: the steepest of these, its tile of outputs spans more input samples than one staged window holds
SCIPY_RATIOS = [(1, 3), (3, 1), (1, 2), (2, 1), (160, 441), (441, 160), (3, 2), (1, 12)]


def _half(up, down):
    return 10 * max(up, down)


def _h32(up, down):
    """the filter as scipy designs it (signal.resample_poly: firwin(2 half + 1, 1 / R, window=('kaiser', 5.0)) * up), rounded to fp32"""
    from scipy.signal import firwin
    R = max(up, down)
    return np.float32(firwin(2 * _half(up, down) + 1, 1.0 / R, window=("kaiser", 5.0)) * up)


def _out_len(L, up, down):
    return -(-L * up // down)


@pytest.mark.parametrize("up,down", TAP_RATIOS)
def test_taps_equal_scipys_design(dev, up, down):
    """ops.resample_taps, un-permuted from phase-major [up][M] to h[p + m up], equals scipy's filter within one fp32 ulp per tap; the
    slots past a phase's last tap are zero; the table has M = ceil((2 half + 1) / up) taps per phase."""
    from storm_amd import ops
    T = ops.resample_taps(up, down)
    n = 2 * _half(up, down) + 1
    M = -(-n // up)
    assert T.shape == (up, M) and T.dtype == torch.float32
    flat = T.numpy().T.reshape(-1)                                   # index m * up + p = j
    h = _h32(up, down)
    err = np.abs(flat[:n].astype(np.float64) - h.astype(np.float64))
    print(f"taps {up}/{down}: {n} taps, {int((flat[:n] != h).sum())} differ from scipy's, worst |t - h| / |h| {float((err / np.maximum(np.abs(h), 1e-300)).max()):.3e}")
    assert (err <= 2.0 ** -23 * np.abs(h).astype(np.float64)).all()
    assert (flat[n:] == 0).all()
    assert abs(float(flat.astype(np.float64).sum()) - up) < 1e-5 * up          # unit DC gain, times up


@pytest.mark.parametrize("up,down,L", IMPULSE_CASES)
def test_impulse_response_is_the_table_bit_for_bit(dev, up, down, L):
    """x = delta[k - k0]: y[n] = h32[n down - k0 up + half] exactly (0 where the index leaves the filter) - every other product is a zero.
    Pins the phase / offset arithmetic with no tolerance."""
    from storm_amd import ops
    half = _half(up, down)
    T = ops.resample_taps(up, down).numpy()
    h = np.zeros(T.size, np.float32)
    h[:] = T.T.reshape(-1)                                          # h[j], zero past 2 half
    Lout = _out_len(L, up, down)
    ks = [0, 1, L // 2 + 3, L - 1]
    x = torch.zeros(len(ks), L)
    for r, k0 in enumerate(ks):
        x[r, k0] = 1.0
    y = ops.resample_poly(x.to(dev), up, down).cpu().numpy()
    assert y.shape == (len(ks), Lout)
    n = np.arange(Lout, dtype=np.int64)
    for r, k0 in enumerate(ks):
        j = n * down - k0 * up + half
        ok = (j >= 0) & (j <= 2 * half)
        want = np.where(ok, h[np.clip(j, 0, h.size - 1)], np.float32(0))
        assert ok.any() and np.array_equal(y[r], want), (up, down, k0)


def _scipy_lengths(up, down):
    """the smallest lengths that reach each edge of the kernel: 1 sample; 5 (the filter longer than the signal on both sides); outputs
    one below / at / one above a workgroup's tile (as near as the ratio lets L_out land); three workgroups"""
    from storm_amd import ops
    tile = ops.RESAMPLE_TILE
    Ls = {1, 5, 2 * tile * down // up + 5}
    for t in (tile - 1, tile, tile + 1):
        Ls |= {(t - 1) * down // up + 1, max(1, t * down // up)}
    return sorted(Ls)


def _signal(B, L, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((B, L)) * 0.1 + 0.05).astype(np.float32)          # Gaussian + a DC offset


@pytest.mark.parametrize("up,down", SCIPY_RATIOS)
def test_against_scipy_resample_poly(dev, up, down):
    from scipy.signal import resample_poly

    from storm_amd import ops
    tile = ops.RESAMPLE_TILE
    louts = set()
    for L in _scipy_lengths(up, down):
        x = _signal(1, L, 100 + L)
        ref = resample_poly(x.astype(np.float64), up, down, axis=1)
        y = ops.resample_poly(torch.from_numpy(x).to(dev), up, down).cpu()
        assert y.shape == ref.shape == (1, _out_len(L, up, down))
        err = rel_l2(y, ref)
        print(f"resample {up}/{down} L={L} -> {y.shape[1]}: rel-L2 vs scipy fp64 {err:.3e}")
        assert err < F32_TOL, (up, down, L)
        louts.add(y.shape[1])
    assert min(louts) == _out_len(1, up, down) and max(louts) > 2 * tile
    assert any(tile - max(up, 2) < v <= tile for v in louts) and any(tile < v <= tile + max(up, 2) for v in louts)
    if up <= down:                                                  # every output count is reachable: exactly one below, at, one above
        assert {tile - 1, tile, tile + 1} <= louts
    # three rows of a wider tensor (row stride > L, the rows do not start on 16 bytes): every row as its own call
    L = 2 * tile * down // up + 5
    wide = torch.from_numpy(_signal(3, L + 10, 7)).to(dev)
    xs = wide[:, 3:3 + L]
    assert xs.stride(0) > L
    y = ops.resample_poly(xs, up, down).cpu()
    ref = resample_poly(xs.cpu().numpy().astype(np.float64), up, down, axis=1)
    err = rel_l2(y, ref)
    print(f"resample {up}/{down} B=3 strided L={L}: rel-L2 vs scipy fp64 {err:.3e}")
    assert err < F32_TOL
    for b in range(3):
        assert torch.equal(y[b:b + 1], ops.resample_poly(xs[b:b + 1].contiguous(), up, down).cpu()), b


def test_unreduced_rates_are_reduced_by_the_wrapper(dev):
    from scipy.signal import resample_poly

    from storm_amd import ops
    x = _signal(2, 4801, 3)
    y = ops.resample_poly(torch.from_numpy(x).to(dev), 16000, 48000).cpu()
    ref = resample_poly(x.astype(np.float64), 1, 3, axis=1)
    err = rel_l2(y, ref)
    print(f"resample 48000 -> 16000 L=4801: rel-L2 vs scipy fp64 {err:.3e}")
    assert y.shape == ref.shape and err < F32_TOL
    assert torch.equal(y, ops.resample_poly(torch.from_numpy(x).to(dev), 1, 3).cpu())
    assert ops.resample_length(4801, 16000, 48000) == y.shape[1] == 1601


@pytest.mark.parametrize("up,down,L", [(160, 441, 3000), (3, 1, 400)])
def test_ragged_rows_equal_their_own_calls(dev, up, down, L):
    """lengths = [L, L - 1, 7], NaN past every row's length: row b's first ceil(len_b up / down) outputs are bit-equal to its own
    B = 1 call, everything after them is exactly 0, and no NaN is read"""
    from storm_amd import ops
    lengths = [L, L - 1, 7]
    x = torch.from_numpy(_signal(3, L, 11))
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
    y = ops.resample_poly(x.to(dev), up, down, lengths=lengths).cpu()
    assert y.shape == (3, _out_len(L, up, down)) and y.shape[1] > ops.RESAMPLE_TILE
    assert not torch.isnan(y).any()
    for b, n in enumerate(lengths):
        own = ops.resample_poly(x[b:b + 1, :n].contiguous().to(dev), up, down).cpu()
        k = _out_len(n, up, down)
        assert own.shape == (1, k) and torch.equal(y[b:b + 1, :k], own), b
        assert (y[b, k:] == 0).all(), b
    with pytest.raises(ValueError, match=str(L + 1)):
        ops.resample_poly(x.to(dev), up, down, lengths=[L + 1, 1, 1])


def test_identity_and_refusals(dev):
    from storm_amd import _lib, ops
    from storm_amd.data_module import SpecsDataModule
    assert SpecsDataModule.sample_rate == 16000
    w = torch.from_numpy(_signal(2, 50, 1)).to(dev)
    w0 = w[0]
    assert SpecsDataModule.resample(w, 16000, 16000) is w and SpecsDataModule.resample(w0, 44100, 44100) is w0
    assert ops.resample_poly(w, 5, 5) is w
    assert SpecsDataModule.resample(w[0], 16000, 48000).shape == (150,) and SpecsDataModule.resample(w, 48000, 16000).shape == (2, 17)
    with pytest.raises(_lib.StormError, match="1025"):
        ops.resample_taps(1025, 1)
    with pytest.raises(_lib.StormError, match="1031"):
        ops.resample_poly(w, 3, 1031)
    with pytest.raises(ValueError, match="up=0"):
        ops.resample_poly(w, 0, 1)
    with pytest.raises(ValueError, match="down=-2"):
        ops.resample_taps(1, -2)
    # the raw binding: the library itself refuses, and names the value
    lib = _lib.lib()
    err = lambda: lib.storm_last_error().decode()                   # noqa: E731
    assert lib.storm_resample_num_taps(1, 3) == 61 and lib.storm_resample_num_taps(160, 441) == 8821 and lib.storm_resample_num_taps(1024, 1) == 20481
    assert lib.storm_resample_num_taps(0, 1) < 0 and "up=0" in err()
    assert lib.storm_resample_num_taps(2, 4) < 0 and "2 / 4" in err()
    assert lib.storm_resample_num_taps(1, 1025) < 0 and "1025" in err()
    small = torch.empty(10)
    assert lib.storm_resample_taps(1, 3, small.data_ptr(), 10) != 0 and "capacity 10" in err()
    assert lib.storm_resample_taps(1, 3, None, 61) != 0 and "null" in err()
    taps = ops.resample_taps(1, 3, device=dev)
    y = torch.empty(2, 18, device=dev)
    args = lambda Lout, up=1, down=3, x=w, t=taps: (_lib.ptr(x), _lib.ptr(y), _lib.ptr(t), 2, 50, 50, Lout, 18, None, up, down, _lib.stream())  # noqa: E731
    assert lib.storm_resample_poly(*args(18)) != 0 and "L_out=18" in err() and "17" in err()
    assert lib.storm_resample_poly(*args(17, x=None)) != 0 and "null" in err()
    assert lib.storm_resample_poly(*args(17, t=None)) != 0 and "null" in err()
    assert lib.storm_resample_poly(*args(17, up=2, down=6)) != 0 and "2 / 6" in err()
    assert lib.storm_resample_poly(*args(17)) == 0


def test_cpu_tensor_is_refused_by_the_real_library():
    """with libstorm_hip.so bound (not the simulator) a CPU tensor is refused, as everywhere: there is no CPU fallback"""
    from storm_amd import _lib, ops
    from storm_amd.build import build
    build()
    _lib._lib, _lib._sim = None, False
    _lib.lib()
    with pytest.raises(_lib.StormError, match="CPU tensor"):
        ops.resample_poly(torch.zeros(1, 100), 1, 3)


# ---- the model classes: sr= --------------------------------------------------------------------------------------------------------
def _storm_model(dev):
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import StochasticRegenerationModel
    from tests.test_model import COMMON
    m = StochasticRegenerationModel(backbone_denoiser="ncsnpp", backbone_score="ncsnpp", condition="both", **dict(COMMON))
    m.denoiser_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=31))
    m.score_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=6), seed=32))
    m._error_loading_ema = True
    return m.eval().to(dev)


def test_score_model_at_48k_equals_resample_enhance_resample(dev):
    """8000 samples at 16 kHz = 24000 at 48 kHz: enhance_batch(y, sr=48000, seed=s) is bit-equal to the three steps done by hand;
    sr=16000 and sr=None take the same path"""
    from tests.test_model import score_model
    m = score_model(dev)
    rs = m.data_module.resample
    y = torch.from_numpy(_signal(1, 24000, 5))
    kw = dict(N=1, corrector="ald", snr=0.5, seed=77)
    got = m.enhance_batch(y, sr=48000, **kw)
    y16 = rs(y.to(dev), 48000, 16000)
    assert y16.shape == (1, 8000)
    x16 = m.enhance_batch(y16, **kw)
    want = rs(x16, 16000, 48000)[:, :24000]
    assert got.shape == (1, 24000) and torch.equal(got, want) and torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert torch.equal(m.enhance_batch(y16, sr=16000, **kw), m.enhance_batch(y16, sr=None, **kw))
    if dev.type != "cpu":                                            # (the simulator walks every lane: the one-utterance call on the GPU only)
        one = m.enhance(y, sr=48000, **kw)                           # the same numbers on the host
        assert one.shape == (24000,) and one.device.type == "cpu" and torch.equal(one, got[0].cpu())
        assert torch.equal(m.enhance(y16, sr=16000, **kw), x16[0].cpu())


def test_storm_model_ragged_at_44k1_with_row_seeds(dev):
    """two rows of 22050 and 20000 samples at 44.1 kHz (8000 and 7257 at 16 kHz: one padded frame count) with a key per row: bit-equal
    to resampling, enhancing the ragged 16 kHz batch and resampling back by hand, every row trimmed to its input count and zero past it.
    Rows whose 16 kHz lengths do not share a padded frame count are refused, and the message says at which rate."""
    m = _storm_model(dev)
    rs = m.data_module.resample
    lengths = [22050, 20000]
    y = torch.from_numpy(_signal(2, 22050, 6))
    y[1, 20000:] = 0
    kw = dict(N=1, corrector="none", row_seeds=[11, 2 ** 40 + 5])
    got = m.enhance_batch(y, sr=44100, lengths=lengths, **kw)
    l16 = [8000, 7257]
    assert l16 == [math.ceil(v * 160 / 441) for v in lengths]
    y16 = rs(y.to(dev), 44100, 16000, lengths=lengths)
    x16 = m.enhance_batch(y16, lengths=l16, **kw)
    want = rs(x16, 16000, 44100, lengths=l16)
    assert got.shape == (2, 22050) and torch.isfinite(got).all()
    for b, n in enumerate(lengths):
        assert torch.equal(got[b, :n], want[b, :n]) and float(got[b, :n].abs().max()) > 0, b
        assert (got[b, n:] == 0).all(), b
    with pytest.raises(ValueError, match="16000 Hz"):
        m.enhance_batch(torch.zeros(2, 30000), sr=44100, lengths=[30000, 20000], **kw)


def test_discriminative_model_at_8k(dev):
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import DiscriminativeModel
    from tests.test_model import COMMON
    m = DiscriminativeModel(backbone="ncsnpp", input_channels=2, discriminative=True, **dict(COMMON))
    m.dnn.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=41))
    m.eval(no_ema=True)
    m = m.to(dev)
    rs = m.data_module.resample
    y = torch.from_numpy(_signal(1, 4000, 8)).to(dev)
    got = m.enhance(y, sr=8000)
    y16 = rs(y, 8000, 16000)
    assert y16.shape == (1, 8000)
    x16 = m.enhance(y16)
    want = rs(x16.reshape(1, -1), 16000, 8000)[0, :4000]
    assert got.shape == (4000,) and torch.equal(got, want) and torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert torch.equal(m.enhance(y16, sr=16000), x16)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_enhancement_cli_resample(tmp_path, switch):
    """enhancement.py --resample on a directory of a 48 kHz, a 44.1 kHz and a 16 kHz file (one frame bucket at 16 kHz: one ragged batch):
    every output has its input's rate and sample count and equals model.enhance(w, sr=sr, row_seeds=[the file's key]).  Both sides run
    batch-invariant, where a row is bit for bit what its own call gives (storm_amd.set_batch_invariant): what is left is the wav file's
    float32.  --output-sr model writes 16 kHz; the same directory without --resample is refused with upstream's message."""
    import importlib.util
    import subprocess
    import sys

    from scipy.io import wavfile

    from oracle import ncsnpp_ref as NR
    from storm_amd.model import ScoreModel
    from tests.test_model import COMMON
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("enhancement_cli", os.path.join(root, "enhancement.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5)
    ckpt = os.path.join(tmp_path, "m.ckpt")
    torch.save({"state_dict": {"dnn." + k: v for k, v in sd.items()}, "hyper_parameters": dict(backbone="ncsnpp", **COMMON)}, ckpt)
    files = {"a48.wav": (48000, 18000), "b44.wav": (44100, 16500), "c16.wav": (16000, 6000)}
    noisy = os.path.join(tmp_path, "noisy")
    os.makedirs(noisy)
    wavs = {}
    for k, (name, (sr, n)) in enumerate(files.items()):
        wavs[name] = _signal(1, n, 40 + k)[0]
        wavfile.write(os.path.join(noisy, name), sr, wavs[name])
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=root).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = [sys.executable, os.path.join(root, "enhancement.py"), "--test_dir", noisy, "--ckpt", ckpt, "--mode", "score-only", "--N", "2",
              "--utterance-seed", "5", "--batch-invariant"]
    out = os.path.join(tmp_path, "enhanced")
    r = subprocess.run(common + ["--enhanced_dir", out, "--resample"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = ScoreModel.load_from_checkpoint(ckpt, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    m.eval(no_ema=False)
    m = m.cuda()
    switch("STORM_BATCH_INVARIANT", 1)
    for name, (sr, n) in files.items():
        got_sr, x = wavfile.read(os.path.join(out, name))
        assert got_sr == sr and x.shape == (n,) and x.dtype == np.float32 and np.isfinite(x).all(), name
        want = m.enhance(torch.from_numpy(wavs[name])[None], sr=sr, N=2, row_seeds=[cli.utterance_key(5, name)])
        err = rel_l2(torch.from_numpy(x), want)
        print(f"enhancement.py --resample {name} ({sr} Hz): rel-L2 vs model.enhance(sr=) {err:.3e}")
        assert err < 1e-6, name
    out16 = os.path.join(tmp_path, "enhanced16")
    r = subprocess.run(common + ["--enhanced_dir", out16, "--resample", "--output-sr", "model"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, (sr, n) in files.items():
        got_sr, x = wavfile.read(os.path.join(out16, name))
        assert got_sr == 16000 and x.shape == (-(-n * 16000 // sr),), name
    r = subprocess.run(common + ["--enhanced_dir", os.path.join(tmp_path, "refused")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "resample to 16kHz" in (r.stderr + r.stdout)
