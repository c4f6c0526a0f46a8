"""storm_peak_abs / storm_stft / storm_istft at the edges of their argument range, on the host simulation and on the device.

Every case is compared with float64 torch.stft / torch.istft called with the reference data module's arguments, frame by frame (forward)
and sample by sample (inverse), and the tolerance is measured in the test from that reference alone: MARGIN = 4 times what torch's own
float32 transform shows against float64 over the setting's cases (tests/frontend_cases.py says why).  The case tables - both parities of
n_fft, the table limit, a hop above n_fft / 2, a hop that does not divide n_fft, lengths from the shortest legal row to 64 frames on
either side of every multiple of the hop - are in tests/frontend_cases.py."""
import pytest
import torch

from tests import frontend_cases as FC
from tests.backend import dev  # noqa: F401

SETTING_PARAMS = [pytest.param(s, id=FC.setting_id(s)) for s in FC.SETTINGS]
FUSED_PARAMS = [pytest.param(s, id=FC.setting_id(s)) for s in FC.FUSED_SETTINGS]
RAGGED_PARAMS = [pytest.param(s, id=FC.setting_id(s)) for s in FC.RAGGED_SETTINGS]


def _kw(setting):
    return dict(n_fft=setting[0], hop=setting[1], window=setting[2])


def _dm(setting, **kw):
    from storm_amd.data_module import SpecsDataModule
    return SpecsDataModule(gpu=False, n_fft=setting[0], hop_length=setting[1], window=setting[2], **kw)


def _tag(dev):
    return "device" if dev.type == "cuda" else "simulation"


# ---------------------------------------------------------------- forward -----------------
@pytest.mark.parametrize("setting", SETTING_PARAMS)
def test_stft_per_frame_vs_torch_float64(dev, setting):
    """shape == torch.stft's (odd n_fft: one frame fewer than 1 + L // hop whenever hop divides L); every frame within MARGIN x torch
    float32's worst frame of the setting"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    cases = [FC.stft_case(setting, L) for L in FC.lengths(n_fft, hop)]
    bound = FC.MARGIN * max(c[2] for c in cases)
    worst = 0.0
    for L, (y, ref, _) in zip(FC.lengths(n_fft, hop), cases):
        Y = ops.stft(y.to(dev), None, **_kw(setting)).cpu()
        assert Y.shape == ref.shape, (L, tuple(Y.shape), tuple(ref.shape))
        assert torch.isfinite(torch.view_as_real(Y)).all()
        worst = max(worst, FC.frame_err(Y, ref))
    print(f"frontend stft {FC.setting_id(setting)} {_tag(dev)}: worst frame (max bin error / largest bin; not a rel-L2 of the tensor) "
          f"{worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("e,factor", FC.COMPRESSIONS)
@pytest.mark.parametrize("setting", FUSED_PARAMS)
def test_stft_fused_peak_and_compression_vs_float64(dev, setting, e, factor):
    """spec_fwd(stft(y / peak)) in one launch against the same expression in float64; frames past the row's own count are exactly zero"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    cases = [FC.fused_case(setting, L, e, factor) for L in FC.lengths(n_fft, hop)]
    bound = FC.MARGIN * max(c[3] for c in cases)
    worst = 0.0
    for L, (y, peak, ref, _) in zip(FC.lengths(n_fft, hop), cases):
        yd = y.to(dev)
        pk = ops.peak_abs(yd)
        assert torch.equal(pk.cpu(), peak)
        Y = ops.stft(yd, pk, spec_factor=factor, spec_abs_exponent=e, pad_to=64, **_kw(setting)).cpu()
        T = ref.shape[-1]
        assert Y.shape == (FC.BATCH, n_fft // 2 + 1, 64) and T <= 64
        assert not torch.view_as_real(Y[..., T:]).any()
        worst = max(worst, FC.frame_err(Y[..., :T], ref))
    print(f"frontend fused stft {FC.setting_id(setting)} e={e} factor={factor} {_tag(dev)}: worst frame (not a rel-L2) {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


# ---------------------------------------------------------------- inverse -----------------
@pytest.mark.parametrize("setting", SETTING_PARAMS)
def test_istft_per_sample_vs_torch_float64(dev, setting):
    """every output length (L, the default hop (T - 1), the largest covered one): the error weighted by the window envelope - the error
    of the overlap-add numerator - and the unweighted error on the samples whose envelope is at least 1e-3 of its maximum, both within
    MARGIN x torch float32's worst of the setting; length=None through SpecsDataModule.istft has torch's length"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    todo = [(L, n) for L in FC.lengths(n_fft, hop) for n in FC.istft_lengths(setting, L)[1]]
    cases = [FC.istft_case(setting, L, n) for L, n in todo]
    bound_w = FC.MARGIN * max(c[3][0] for c in cases)
    bound_k = FC.MARGIN * max(c[3][1] for c in cases)
    worst_w = worst_k = worst_out = 0.0
    for (L, n), (X, ref, env, _) in zip(todo, cases):
        x = ops.istft(X.to(dev), n, None, **_kw(setting)).cpu()
        assert x.shape == ref.shape and torch.isfinite(x).all()
        w, k, out = FC.wav_err(x, ref, env)
        worst_w, worst_k, worst_out = max(worst_w, w), max(worst_k, k), max(worst_out, out)
    print(f"frontend istft {FC.setting_id(setting)} {_tag(dev)}: envelope-weighted error (not a rel-L2) {worst_w:.3e}, bound {bound_w:.3e}; "
          f"unweighted on the kept samples {worst_k:.3e}, bound {bound_k:.3e}; share left out {worst_out:.4f}")
    assert worst_out < FC.MAX_LEFT_OUT
    assert worst_w <= bound_w and worst_k <= bound_k
    dm = _dm(setting)
    for L in FC.lengths(n_fft, hop)[:3]:
        X = FC.spectrum(n_fft // 2 + 1, FC.torch_frames(L, n_fft, hop), n_fft % 2 == 0)
        ref = FC.istft_t(X, setting, None, torch.float64)
        x = dm.istft(X.to(dev)).cpu()
        assert x.shape == ref.shape, (L, tuple(x.shape), tuple(ref.shape))
        assert torch.equal(x, ops.istft(X.to(dev), ref.shape[-1], None, **_kw(setting)).cpu())


@pytest.mark.parametrize("setting", SETTING_PARAMS)
def test_round_trip_returns_the_signal(dev, setting):
    """istft(stft(y), L) == y on the samples whose envelope is at least 1e-3 of its maximum (the windows of every setting overlap),
    within MARGIN x what torch float32's own round trip loses"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    Ls = FC.lengths(n_fft, hop)
    bound = FC.MARGIN * max(FC.round_trip_torch32(setting, L)[0] for L in Ls)
    worst = 0.0
    for L in Ls:
        y = FC.signal(L)
        back = ops.istft(ops.stft(y.to(dev), None, **_kw(setting)), L, None, **_kw(setting)).cpu()
        _, k, out = FC.wav_err(back, y.double(), FC.envelope(setting, FC.torch_frames(L, n_fft, hop), L))
        assert out < FC.MAX_LEFT_OUT
        worst = max(worst, k)
    print(f"frontend round trip {FC.setting_id(setting)} {_tag(dev)}: error on the kept samples (not a rel-L2) {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


# ---------------------------------------------------------------- ragged batches ----------
def _ragged_batch(n_fft):
    lens = FC.ragged_lengths(n_fft)
    W = max(lens)
    g = torch.Generator().manual_seed(4242 + n_fft)
    wav = torch.randn(len(lens), W, generator=g) * 0.3
    for b, n in enumerate(lens):
        wav[b, n:] = 1e6 * (b + 1)                                   # junk, not zeros, past each row's length: never read
    return lens, wav


@pytest.mark.parametrize("setting", RAGGED_PARAMS)
def test_ragged_rows_equal_their_own_calls(dev, setting):
    """rows of 63 and 64 frames under one padded count of 64 (8192 samples at n_fft = 511: 64 frames, where 1 + L // hop said 65):
    peak, fused forward and inverse of every row are bit-equal to the row's own call, the inverse is zero past the row's length"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    lens, wav = _ragged_batch(n_fft)
    W = wav.shape[1]
    dm = _dm(setting, spec_factor=0.15, spec_abs_exponent=0.5)
    assert {FC.torch_frames(n, n_fft, hop) for n in lens} == {63, 64}
    assert {dm.padded_frames(n) for n in lens} == {64}
    wd = wav.to(dev)
    Y, peak = dm.wav_to_spec(wd, lengths=lens)
    assert Y.shape == (len(lens), 1, n_fft // 2 + 1, 64)
    g = torch.Generator().manual_seed(99)
    S = torch.complex(torch.randn(Y.shape, generator=g), torch.randn(Y.shape, generator=g)).to(dev) * 0.1
    S[:, :, 0] = S[:, :, 0].real.to(torch.complex64)
    if n_fft % 2 == 0:
        S[:, :, -1] = S[:, :, -1].real.to(torch.complex64)
    x = dm.spec_to_wav(S, W, peak, lengths=lens)
    for b, n in enumerate(lens):
        row = wav[b:b + 1, :n].contiguous().to(dev)
        Yb, pb = dm.wav_to_spec(row)
        assert float(pb.cpu()) == float(wav[b, :n].abs().max())
        assert torch.equal(peak[b:b + 1].cpu(), pb.cpu())
        assert torch.equal(Y[b:b + 1].cpu(), Yb.cpu())
        T = FC.torch_frames(n, n_fft, hop)
        assert not torch.view_as_real(Y[b, 0, :, T:].cpu()).any() and torch.view_as_real(Y[b, 0, :, T - 1].cpu()).any()
        xb = dm.spec_to_wav(S[b:b + 1], n, pb)
        assert torch.equal(x[b, :n].cpu(), xb[0].cpu())
        assert not x[b, n:].cpu().any()
    # rows that do not share a padded count are refused: one sample more than the longest row here starts the next 64 frames
    over = 8192 if n_fft % 2 == 0 else 8193
    assert dm.padded_frames(over) == 128 and dm.padded_frames(over - 1) == 64
    with pytest.raises(ValueError, match="padded frame count"):
        dm.wav_to_spec(torch.zeros(2, over).to(dev), lengths=[over, over - 1])


def test_rows_read_in_place_equal_their_copy(dev):
    """a strided view of overlapping windows of one recording (what enhance_long passes), starting at a sample offset that is not a
    multiple of four: the same bits as its contiguous copy"""
    from storm_amd import ops
    W, H, B, off = 4001, 1500, 4, 3
    rec = (torch.randn(off + (B - 1) * H + W, generator=torch.Generator().manual_seed(31)) * 0.3).to(dev)
    view = torch.as_strided(rec, (B, W), (H, 1), storage_offset=off)
    assert view.data_ptr() % 16 != 0 and not view.is_contiguous()
    copy = view.contiguous()
    assert torch.equal(ops.peak_abs(view).cpu(), ops.peak_abs(copy).cpu())
    peak = ops.peak_abs(rec[None, :]).expand(B).contiguous()        # the recording's peak for every window
    for setting in FC.RAGGED_SETTINGS:
        kw = dict(spec_factor=0.15, spec_abs_exponent=0.5, pad_to=64, **_kw(setting))
        assert torch.equal(ops.stft(view, peak, **kw).cpu(), ops.stft(copy, peak, **kw).cpu())


# ---------------------------------------------------------------- degenerate values -------
@pytest.mark.parametrize("setting", RAGGED_PARAMS)
def test_all_zero_row_stays_zero_and_alone(dev, setting):
    """an all-zero row: peak PEAK_FLOOR, an all-zero spectrum, an all-zero inverse, no NaN; the bits of its batch neighbours are those
    of a batch without it"""
    from storm_amd import ops
    n_fft = setting[0]
    L = 1000
    y = FC.signal(L, seed=3)
    wav = torch.stack([y[0], torch.zeros(L), y[1]]).to(dev)
    both = y.to(dev)
    kw = dict(spec_factor=0.15, spec_abs_exponent=0.5, **_kw(setting))
    peak, peak2 = ops.peak_abs(wav), ops.peak_abs(both)
    assert float(peak[1].cpu()) == float(torch.tensor(ops.PEAK_FLOOR, dtype=torch.float32))
    assert torch.equal(peak[[0, 2]].cpu(), peak2.cpu())
    Y, Y2 = ops.stft(wav, peak, pad_to=64, **kw), ops.stft(both, peak2, pad_to=64, **kw)
    assert not torch.view_as_real(Y[1].cpu()).any()
    assert torch.equal(Y[[0, 2]].cpu(), Y2.cpu())
    x, x2 = ops.istft(Y, L, peak, **kw), ops.istft(Y2, L, peak2, **kw)
    assert not x[1].cpu().any() and torch.isfinite(x.cpu()).all()
    assert torch.equal(x[[0, 2]].cpu(), x2.cpu())
    # exact-zero bins among others: exactly zero after spec_fwd and spec_back, the others finite and non-zero
    z = FC.spectrum(n_fft // 2 + 1, 5, n_fft % 2 == 0).clone()
    z[:, ::3, 1] = 0
    for e, factor in FC.COMPRESSIONS:
        for inverse in (False, True):
            out = ops.spec_transform(z.to(dev), factor, e, inverse).cpu()
            assert torch.isfinite(torch.view_as_real(out)).all()
            assert torch.equal(out == 0, z == 0)


@pytest.mark.parametrize("setting", FUSED_PARAMS)
def test_tiny_bins_keep_their_magnitude(dev, setting):
    """bins of magnitude 1e-30: re^2 + im^2 underflows in fp32 where torch.abs does not.  The compression takes |z| by hypotf there, so
    the fused forward is within the same bound of spec_fwd(stft(y)) in float64 as at ordinary levels; spec_transform in both directions
    is within 1e-6 of the float64 value (hypotf and powf to a few ulp and two products: under 8 fp32 roundings of 6e-8 each)"""
    from storm_amd import ops
    n_fft, hop, _ = setting
    scale, e, factor = 2e-31, 0.5, 0.15
    Ls = FC.lengths(n_fft, hop)[:6]
    cases = [FC.stft_case(setting, L, scale) for L in Ls]
    refs = [FC.spec_fwd_t(c[1], e, factor) for c in cases]
    t32 = [FC.frame_err(FC.spec_fwd_t(FC.stft_t(c[0], setting, torch.float32), e, factor), r) for c, r in zip(cases, refs)]
    bound = FC.MARGIN * max(t32)
    worst = 0.0
    for (y, ref0, _), ref in zip(cases, refs):
        assert 1e-31 < float(ref0.abs().median()) < 1e-29
        Y = ops.stft(y.to(dev), None, spec_factor=factor, spec_abs_exponent=e, **_kw(setting)).cpu()
        assert (Y != 0).all()
        worst = max(worst, FC.frame_err(Y, ref))
    print(f"frontend fused stft of 1e-30 bins {FC.setting_id(setting)} {_tag(dev)}: worst frame (not a rel-L2) {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    z = (FC.spectrum(n_fft // 2 + 1, 4, n_fft % 2 == 0) * 1e-30).contiguous()
    z64 = z.to(torch.complex128)
    fwd = ops.spec_transform(z.to(dev), factor, e, False).cpu().to(torch.complex128)
    want = FC.spec_fwd_t(z64, e, factor)
    assert float(((fwd - want).abs() / want.abs()).max()) < 1e-6
    # spec_back with an exponent of 2 (|z|^(1 / 2) as well: its result is representable, which |z|^2 of 1e-30 is not)
    back = ops.spec_transform(z.to(dev), factor, 2.0, True).cpu().to(torch.complex128)
    want = (z64 / factor).abs() ** 0.5 * torch.exp(1j * (z64 / factor).angle())
    assert float(((back - want).abs() / want.abs()).max()) < 1e-6


# ---------------------------------------------------------------- host rules, refusals ----
@pytest.mark.parametrize("setting", SETTING_PARAMS)
def test_host_frame_rules_agree_with_torch(setting):
    """ops.stft_frames, SpecsDataModule.padded_frames and distributed.bucket_by_frames against torch.stft's own frame count, exact and
    rounded up to 64, for every case length and for 64 hop (the first length whose count differs between the parities under the
    round-up)"""
    from storm_amd import distributed as D
    from storm_amd import ops
    n_fft, hop, _ = setting
    dm = _dm(setting)
    Ls = FC.lengths(n_fft, hop) + (64 * hop,)
    T = [FC.stft_t(torch.zeros(1, L), setting, torch.float32).shape[-1] for L in Ls]
    for L, t in zip(Ls, T):
        assert FC.torch_frames(L, n_fft, hop) == t
        assert ops.stft_frames(L, n_fft, hop) == t, (L, t)
        for pad in (1, 64):
            assert dm.padded_frames(L, pad) == -(-t // pad) * pad, (L, t, pad)
    for multiple in (1, 64):
        buckets = D.bucket_by_frames(list(Ls), len(Ls), hop=hop, multiple=multiple, n_fft=n_fft)
        assert sorted(i for b in buckets for i in b) == list(range(len(Ls)))
        keys = [{-(-T[i] // multiple) * multiple for i in b} for b in buckets]
        assert all(len(k) == 1 for k in keys), keys
        assert len({next(iter(k)) for k in keys}) == len(keys), keys
    if n_fft == 510:                                                 # n_fft defaults to the data module's default
        assert D.bucket_by_frames(list(Ls), 3, hop=hop) == D.bucket_by_frames(list(Ls), 3, hop=hop, n_fft=510)


@pytest.mark.parametrize("setting", SETTING_PARAMS)
def test_refusals_stay_refusals(dev, setting):
    """a row of p = n_fft // 2 samples (torch.stft refuses its reflect padding), ragged or not; an inverse longer than its frames cover"""
    from storm_amd import _lib, ops
    n_fft, hop, _ = setting
    p = n_fft // 2
    with pytest.raises(RuntimeError):
        FC.stft_t(torch.zeros(1, p), setting, torch.float32)
    with pytest.raises(ValueError, match="too short for reflect padding"):
        ops.stft(torch.zeros(2, p).to(dev), None, **_kw(setting))
    with pytest.raises(ValueError, match="too short for reflect padding"):
        ops.stft(torch.zeros(2, p + 9).to(dev), None, lengths=[p + 9, p], **_kw(setting))
    with pytest.raises(ValueError, match="too short for reflect padding"):
        _dm(setting).wav_to_spec(torch.zeros(2, p + 9).to(dev), lengths=[p + 9, p])
    T = 3
    X = FC.spectrum(p + 1, T, n_fft % 2 == 0).to(dev)
    covered = n_fft + hop * (T - 1) - p
    assert ops.istft(X, covered, None, **_kw(setting)).shape == (FC.BATCH, covered)
    with pytest.raises(_lib.StormError, match="not covered"):
        ops.istft(X, covered + 1, None, **_kw(setting))


def test_transform_sizes_above_the_table_are_refused(dev):
    from storm_amd import _lib, ops
    with pytest.raises(_lib.StormError, match="n_fft=1025"):
        ops.stft(torch.zeros(1, 4000).to(dev), None, n_fft=1025, hop=256)
    with pytest.raises(_lib.StormError, match="n_fft=1026"):
        ops.istft(torch.zeros(1, 514, 4, dtype=torch.complex64).to(dev), 512, None, n_fft=1026, hop=256)
