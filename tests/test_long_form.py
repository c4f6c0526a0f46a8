"""Long recordings: storm_crossfade_rows / storm_crossfade_ramp against the numpy restatement of their definition (bit equality), their
properties, and enhance_long against its own composition from enhance_batch calls (tests/long_form_cases.py)."""
import os

import numpy as np
import pytest
import torch

from tests import long_form_cases as LC
from tests.backend import dev, setup_backend, switch  # noqa: F401
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dev, pool, win_row, rec_len, rec_windows, W, V, kind="hann", width=None):
    """(kernel output, numpy restatement) of one launch"""
    from storm_amd import ops
    ramp = ops.crossfade_ramp(V, kind, dev)
    got = ops.crossfade_rows(pool.to(dev) if pool.is_contiguous() else _strided_to(pool, dev), win_row, rec_len, rec_windows, W, V, ramp=ramp, width=width)
    want = LC.launch_ref(pool, win_row, rec_len, rec_windows, W, V, LC.ramp_ref(V, kind), got.shape[1])
    return got.cpu().numpy(), want


def _strided_to(view, dev):
    """a [N, W] view of a wider tensor on `dev`, with the same row stride"""
    big = torch.zeros(view.shape[0], view.stride(0))
    big[:, :view.shape[1]] = view
    return big.to(dev)[:, :view.shape[1]]


# ---- 1. the kernel against the restatement, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("V", [1, 16, 32])
def test_stitch_equals_its_definition(dev, V, n):
    """W = 64, the smallest and the largest overlap and one between, at the smallest and the largest length that has n windows; both ramps.
    (H = 48 and 32 are multiples of 4: 16-byte path; H = 63 is not: scalar path.)"""
    W, H = 64, 64 - V
    for L in ((n - 1) * H + V + 1, (n - 1) * H + W):
        assert LC.plan_ref(L, W, V)[0] == n
        for kind in ("hann", "linear"):
            got, want = _run(dev, *LC.launch_case([L], W, V, seed=100 * V + n), W, V, kind)
            assert got.shape == (1, L) and np.array_equal(got, want), (V, n, L, kind)
            assert np.isfinite(got).all() and np.abs(got).max() > 0


@pytest.mark.parametrize("dW", [-1, 0, 1])
def test_windows_around_one_workgroups_outputs(dev, dW):
    """W = a workgroup's outputs - 1, + 0, + 1; lengths that end in the second and in the third workgroup, and one sample before / at / after
    a workgroup's end"""
    from storm_amd import ops
    tile = ops.CROSSFADE_TILE
    W, V = tile + dW, 100
    for L in (tile + 5, 2 * tile - 1, 2 * tile, 2 * tile + 1, 2 * tile + 3, 3 * tile - 7):
        got, want = _run(dev, *LC.launch_case([L], W, V, seed=L), W, V)
        assert got.shape == (1, L) and np.array_equal(got, want), (W, L)


@pytest.mark.parametrize("recs", [[150, 260], [97, 64 + 48 * 4, 140], [40, 200]])
def test_several_recordings_in_one_launch(dev, recs):
    """two and three recordings of different window counts (the last case: one of a single window), pool rows permuted and interleaved,
    a pool row that no window names; the output is as wide as the longest recording, the shorter rows end in zeros"""
    W, V = 64, 16
    case = LC.launch_case(recs, W, V, seed=sum(recs), extra_rows=2)
    assert len(set(case[3])) == len(recs) and sorted(case[1]) != case[1]
    got, want = _run(dev, *case, W, V)
    assert got.shape == (len(recs), max(recs)) and np.array_equal(got, want)
    for r, L in enumerate(recs):
        assert (got[r, L:] == 0).all() and np.abs(got[r, :L]).max() > 0


@pytest.mark.parametrize("stride", [64 + 8, 64 + 3])
def test_pool_with_a_row_stride(dev, stride):
    """the pool as a view of a wider tensor: a stride that keeps rows on 16 bytes and one that does not"""
    W, V = 64, 16
    case = LC.launch_case([200, 130], W, V, seed=stride, stride=stride)
    assert case[0].stride(0) == stride and not case[0].is_contiguous()
    got, want = _run(dev, *case, W, V)
    assert np.array_equal(got, want)


def test_output_wider_than_the_longest_recording(dev):
    from storm_amd import ops
    W, V = 64, 32
    case = LC.launch_case([100, 161], W, V, seed=4)
    width = ops.CROSSFADE_TILE + 37                                   # (a second workgroup that writes zeros only)
    got, want = _run(dev, *case, W, V, width=width)
    assert got.shape == (2, width) and np.array_equal(got, want)
    assert (got[0, 100:] == 0).all() and (got[1, 161:] == 0).all()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_skipped_window_reads_as_zeros(dev, where):
    W, V, n = 64, 16, 4
    H, L = W - V, 3 * 48 + 50
    k = {"first": 0, "middle": 2, "last": n - 1}[where]
    case = LC.launch_case([L, 120], W, V, seed=7 + k, skip={(0, k)})
    assert case[1][k] == -1 and case[3][0] == n
    got, want = _run(dev, *case, W, V)
    assert np.array_equal(got, want)
    lo, hi = (k * H + V if k > 0 else 0), min((k + 1) * H, L)       # the samples that come from window k alone
    assert (got[0, lo:hi] == 0).all() and np.abs(got[0]).max() > 0
    ramp = LC.ramp_ref(V, "hann")
    if k > 0:                                                         # its fade-in: the predecessor fading out towards zero
        prev = case[0][case[1][k - 1]].numpy()[H:H + V]
        assert np.array_equal(got[0, k * H:k * H + V], (prev + (ramp * (0 - prev)).astype(np.float32)).astype(np.float32))


# ---- 2. properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hann", "linear"])
def test_windows_cut_from_a_signal_stitch_back_to_it(dev, kind):
    """cur == prev in every overlap: prev + ramp * 0 is prev, whatever the ramp"""
    from storm_amd import ops
    g = torch.Generator().manual_seed(11)
    for W, V, L in ((64, 16, 201), (64, 1, 190), (ops.CROSSFADE_TILE + 1, 500, 3 * ops.CROSSFADE_TILE + 9)):
        x = torch.randn(L, generator=g)
        n, padded = ops.window_plan(L, W, V)
        assert (n, padded) == LC.plan_ref(L, W, V) and padded >= L > padded - (W - V)
        buf = torch.zeros(padded)
        buf[:L] = x
        view = buf.to(dev).as_strided((n, W), (W - V, 1))
        out = ops.crossfade_rows(view.clone(), list(range(n)), [L], [n], W, V, ramp=ops.crossfade_ramp(V, kind, dev))
        assert torch.equal(out[0].cpu(), x), (W, V, L)


def test_a_recording_does_not_see_the_launchs_other_recordings(dev):
    from storm_amd import ops
    W, V = 64, 16
    pool, win_row, rec_len, rec_windows = LC.launch_case([150, 260, 97], W, V, seed=21)
    pool = pool.to(dev)
    three = ops.crossfade_rows(pool, win_row, rec_len, rec_windows, W, V)
    at = rec_windows[0]
    alone = ops.crossfade_rows(pool, win_row[at:at + rec_windows[1]], rec_len[1:2], rec_windows[1:2], W, V)
    assert alone.shape == (1, 260) and torch.equal(alone[0], three[1, :260])


@pytest.mark.parametrize("V", [1, 2, 7, 1024, 8192])
def test_ramp(dev, V):
    """the fp64 formula rounded once; strictly increasing; hann: ramp[j] + ramp[V - 1 - j] = sin^2 + cos^2 - each term is below 1 and
    rounded to fp32 with an error of at most 2^-25, the fp32 sum then lands on 1 - 2^-24, 1 or 1 + 2^-23: within one ulp of 1"""
    from storm_amd import ops
    for kind in ("hann", "linear"):
        r = ops.crossfade_ramp(V, kind, dev)
        assert r.dtype == torch.float32 and r.shape == (V,) and r.device.type == dev.type
        assert ops.crossfade_ramp(V, kind, dev) is r                  # cached per device
        r = r.cpu().numpy()
        assert np.array_equal(r, LC.ramp_ref(V, kind)), kind
        assert (np.diff(r) > 0).all() and 0 < r[0] and r[-1] < 1
        s = r + r[::-1]
        assert s.dtype == np.float32 and (np.abs(s.astype(np.float64) - 1.0) <= 2.0 ** -23).all()
        if V == 1:
            assert r.tolist() == [0.5]


def test_plan_and_keys():
    from storm_amd import ops
    W, V = 65408, 8192
    H = W - V
    assert ops.window_plan(W, W, V) == (1, W) and ops.window_plan(5, W, V) == (1, 5)
    assert ops.window_plan(W + 1, W, V) == (2, H + W)
    assert ops.window_plan(H + W, W, V) == (2, H + W) and ops.window_plan(H + W + 1, W, V) == (3, 2 * H + W)
    for L in (W + 1, 3 * H + V, 3 * H + V + 1, 960000):
        n, padded = ops.window_plan(L, W, V)
        assert (n - 1) * H + V < L <= padded == (n - 1) * H + W      # the last window holds more than V real samples
    assert ops.window_key(5, 0) == (5 + 0x9E3779B97F4A7C15) % 2 ** 63 == LC.key_ref(5, 0)
    assert ops.window_key(2 ** 63 - 1, 3) == LC.key_ref(2 ** 63 - 1, 3) and 0 <= ops.window_key(2 ** 63 - 1, 3) < 2 ** 63
    assert len({ops.window_key(9, k) for k in range(100)} | {9}) == 101


def test_refusals(dev):
    from storm_amd import ops
    W, V = 64, 16
    pool = torch.zeros(5, W).to(dev)
    ok = dict(win_row=[0, 1, 2], rec_len=[150], rec_windows=[3])
    ops.crossfade_rows(pool, W=W, V=V, **ok)
    for bad_v in (0, 33, -1):
        with pytest.raises(ValueError, match="V="):
            ops.crossfade_rows(pool, W=W, V=bad_v, **ok)
        with pytest.raises(ValueError, match="V="):
            ops.window_plan(150, W, bad_v)
    for bad in ([0, 1, 5], [0, -2, 1]):
        with pytest.raises(ValueError, match="win_row"):
            ops.crossfade_rows(pool, W=W, V=V, **{**ok, "win_row": bad})
    with pytest.raises(ValueError, match="win_row"):
        ops.crossfade_rows(pool, W=W, V=V, **{**ok, "win_row": [0, 1]})
    for bad_len in (2 * 48 + 16, 2 * 48 + 64 + 1, 0):                   # no sample of its own in the last window; past the last window
        with pytest.raises(ValueError, match="rec_len"):
            ops.crossfade_rows(pool, W=W, V=V, **{**ok, "rec_len": [bad_len]})
    with pytest.raises(ValueError, match="width"):
        ops.crossfade_rows(pool, W=W, V=V, width=149, **ok)
    with pytest.raises(ValueError, match="pool"):
        ops.crossfade_rows(torch.zeros(5, W + 1).to(dev), W=W, V=V, **ok)
    with pytest.raises(ValueError, match="ramp"):
        ops.crossfade_rows(pool, W=W, V=V, ramp=torch.zeros(V + 1).to(dev), **ok)
    with pytest.raises(ValueError, match="ramp"):
        ops.crossfade_ramp(8, "triangle", dev)
    from storm_amd import _lib
    lib, err = _lib.lib(), lambda: _lib.lib().storm_last_error().decode()
    assert lib.storm_crossfade_ramp(0, 0, 1) != 0 and "V=0" in err()
    assert lib.storm_crossfade_ramp(4, 2, 1) != 0 and "kind=2" in err()


def test_front_end_takes_a_peak_and_a_strided_view(dev):
    """wav_to_spec(peak=): the spectrogram of wav / peak for the peak handed in (here: of the whole recording, not of the window), the same
    bits from the overlapping windows as a strided view and from a copy of them; peak=None is the call without the keyword"""
    from storm_amd import ops
    from storm_amd.data_module import SpecsDataModule
    dm = SpecsDataModule(spec_factor=0.15, spec_abs_exponent=0.5)
    W, V = 2048, 256
    H = W - V
    x = 0.1 * torch.randn(H + W, generator=torch.Generator().manual_seed(3))
    x[:W] *= 0.2                                                       # window 0's own peak is far below the recording's, which lies in window 1
    x = x.to(dev)
    view = x.as_strided((2, W), (H, 1))
    rec_peak = ops.peak_abs(x[None]).expand(2).contiguous()
    Y, pk = dm.wav_to_spec(view, peak=rec_peak)
    Yc, _ = dm.wav_to_spec(view.clone(), peak=rec_peak)
    assert torch.equal(pk, rec_peak) and torch.equal(torch.view_as_real(Y), torch.view_as_real(Yc))
    own, own_pk = dm.wav_to_spec(view.clone())
    none, none_pk = dm.wav_to_spec(view.clone(), peak=None)
    assert torch.equal(own_pk, none_pk) and torch.equal(torch.view_as_real(own), torch.view_as_real(none))
    assert torch.equal(own_pk, ops.peak_abs(view)) and float(own_pk[0]) < 0.5 * float(rec_peak[0])
    assert own_pk[1] == rec_peak[1] and torch.equal(torch.view_as_real(Y[1]), torch.view_as_real(own[1]))
    assert not torch.equal(torch.view_as_real(Y[0]), torch.view_as_real(own[0]))
    with pytest.raises(ValueError, match="peak"):
        dm.wav_to_spec(view, peak=rec_peak[:1])


# ---- 3. the schedule of enhance_long around a stand-in for the sampler (both backends: no network) ----------------------------------------
def _stand_in(dev):
    """_Base.enhance_long around an enhance_batch that is elementwise in (row, peak, key): x = y / peak * gain(key).  What the pooling,
    the keys, the peaks and the stitch do shows in the result; the calls are recorded."""
    from storm_amd.data_module import SpecsDataModule
    from storm_amd.model import _Base

    class StandIn(_Base):
        def __init__(self):
            super().__init__()
            self.data_module = SpecsDataModule()
            self.calls = []

        device = property(lambda self: dev)

        @staticmethod
        def gain(key):
            return 0.25 + (key % 13) / 16.0

        def enhance_batch(self, y, lengths=None, peak=None, row_seeds=None, return_nfe=False, sr=None, **kw):
            from storm_amd import ops
            self.calls.append((tuple(y.shape), lengths, None if peak is None else peak.cpu().tolist(), list(row_seeds), kw))
            pk = ops.peak_abs(y.contiguous(), lengths) if peak is None else peak
            g = torch.tensor([self.gain(k) for k in row_seeds], dtype=torch.float32).to(y.device)
            x = y / pk[:, None] * g[:, None]
            return (x, 3) if return_nfe else x
    return StandIn()


def test_enhance_long_schedule(dev):
    """[2.4 windows, 0.5 window, 3 windows, one with a silent window]: batches of one shape in (recording, window) order with the recording's
    peak and ops.window_key per row, the short one through its own call with its own key, the stitch of all in the result; batch sizes
    2 and 5 agree; skip_silent leaves the silent window out of the calls and its samples zero"""
    W, V = 8064, 1024
    H = W - V
    g = torch.Generator().manual_seed(5)
    lens = [int(2.4 * W), W // 2, 3 * W]
    recs = [0.1 * (1 + i) * torch.randn(n, generator=g) for i, n in enumerate(lens)]
    quiet = 0.1 * torch.randn(2 * H + W, generator=g)
    quiet[H + V:2 * H] = 0                                              # not a whole window: still sampled
    quiet[H:2 * H + V] = 0                                              # window 1 whole: skipped with skip_silent
    recs.append(quiet)
    keys = [3, 2 ** 40 + 1, 2 ** 63 - 2, 17]
    m = _stand_in(dev)
    outs, nfe = m.enhance_long(recs, window=W, overlap=V, batch=5, keys=keys, return_nfe=True, N=2)
    assert [o.shape for o in outs] == [(n,) for n in lens] + [quiet.shape] and all(o.device.type == dev.type for o in outs)
    n_win = [LC.plan_ref(n, W, V)[0] for n in (lens[0], lens[2], quiet.numel())]
    assert n_win == [3, 4, 3] and nfe == 3 * (sum(n_win) + 1)
    pooled = [c for c in m.calls if c[0][1] == W]
    assert [c[0][0] for c in pooled] == [5, 5] and all(c[1] is None and c[4] == {"N": 2} for c in m.calls)
    want_keys = [LC.key_ref(keys[i], k) for i, n in ((0, 3), (2, 4), (3, 3)) for k in range(n)]
    assert [k for c in pooled for k in c[3]] == want_keys
    peaks = [float(recs[i].abs().max()) for i in (0, 2, 3)]
    assert [p for c in pooled for p in c[2]] == [peaks[0]] * 3 + [peaks[1]] * 4 + [peaks[2]] * 3
    short = [c for c in m.calls if c[0][1] != W]
    assert len(short) == 1 and short[0][0] == (1, W // 2) and short[0][2] is None and short[0][3] == [keys[1]]
    for i, x in enumerate(recs):
        if x.numel() <= W:
            want = x / x.abs().max() * m.gain(keys[i])
        else:
            want = LC.compose(m, x.to(dev), keys[i], W, V, "hann", lambda rows, pk, ks: m.enhance_batch(rows, peak=pk, row_seeds=ks))
        assert torch.equal(outs[i].cpu(), want.cpu()), i
    for kw in (dict(batch=2), dict(batch=16, ramp="hann")):
        again = m.enhance_long(recs, window=W, overlap=V, keys=keys, N=2, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, outs))
    m.calls.clear()
    skipped, nfe_s = m.enhance_long(recs, window=W, overlap=V, batch=5, keys=keys, return_nfe=True, skip_silent=True, N=2)
    assert nfe_s == nfe - 3 and sorted(c[0][0] for c in m.calls if c[0][1] == W) == [4, 5]
    assert LC.key_ref(17, 1) not in [k for c in m.calls for k in c[3]]
    assert all(torch.equal(a, b) for a, b in zip(skipped[:3], outs[:3]))
    assert (skipped[3][H:2 * H + V] == 0).all() and torch.equal(skipped[3][:H], outs[3][:H]) and torch.equal(skipped[3][2 * H + V:], outs[3][2 * H + V:])
    # seed=s: recording i has the key s + i; a linear ramp changes the overlaps only
    m.calls.clear()
    lin = m.enhance_long(recs[:1], window=W, overlap=V, seed=40, ramp="linear")
    assert m.calls[0][3] == [LC.key_ref(40, k) for k in range(3)]
    assert torch.equal(lin[0][V:H], m.enhance_long(recs[:1], window=W, overlap=V, keys=[40])[0][V:H])


def test_enhance_long_refusals(dev):
    m = _stand_in(dev)
    x = [torch.zeros(30000)]
    for bad in (0, 4033):
        with pytest.raises(ValueError, match="overlap"):
            m.enhance_long(x, window=8064, overlap=bad)
    with pytest.raises(ValueError, match="window"):
        m.enhance_long(x, window=255, overlap=100)
    with pytest.raises(ValueError, match="exclude"):
        m.enhance_long(x, window=8064, overlap=1024, keys=[1], seed=2)
    with pytest.raises(ValueError, match="keys"):
        m.enhance_long(x, window=8064, overlap=1024, keys=[1, 2])
    with pytest.raises(ValueError, match="row_seeds"):
        m.enhance_long(x, window=8064, overlap=1024, row_seeds=[1])


# ---- 4. the pipeline around the tiny networks (fp32, N = 2, W = 63 * 128 = 8064 samples = 64 frames, V = 1024) ------------------------------
W_T, V_T = 63 * 128, 1024
KW_T = dict(N=2, corrector="ald", snr=0.5)
KEYS_T = [7, 2 ** 40 + 3, 2 ** 63 - 1]
_cache = {}


@pytest.fixture
def gpu():
    return setup_backend("hip")


def _recordings():
    g = torch.Generator().manual_seed(77)
    return [0.05 * (1 + i) * torch.randn(n, generator=g) for i, n in enumerate((int(2.4 * W_T), W_T // 2, 3 * W_T))]


def _score(dev):
    from tests.test_model import score_model
    return score_model(dev)                                           # (per test: a model belongs to the backend library that was bound when it was made)


def _reference(m, invariant):
    """the test's own composition, computed once per mode: every window alone through enhance_batch with the recording's peak and the
    window's key, stitched in numpy; the short recording through enhance_batch(row_seeds=[key])"""
    from tests.test_row_seeds import _batch_invariant
    name = ("ref", invariant)
    if name not in _cache:
        with _batch_invariant(invariant):
            out = []
            for x, key in zip(_recordings(), KEYS_T):
                x = x.to(m.device)
                if x.numel() <= W_T:
                    out.append(m.enhance_batch(x[None], row_seeds=[key], **KW_T)[0].cpu())
                else:
                    out.append(LC.compose(m, x, key, W_T, V_T, "hann", lambda rows, pk, ks: m.enhance_batch(rows, peak=pk, row_seeds=ks, **KW_T)))
        _cache[name] = out
    return _cache[name]


@pytest.mark.gpu
@pytest.mark.parametrize("how", [dict(batch=16), dict(batch=2), dict(batch=5), dict(batch=16, grouped=True)], ids=["batch16", "batch2", "batch5", "grouped"])
@pytest.mark.parametrize("invariant", [True, False], ids=["invariant", "fp32"])
def test_pooled_equals_per_window(gpu, invariant, how):
    """enhance_long of [2.4 windows, 0.5 window, 3 windows] against the composition from batch-1 calls, whatever the batch size and with
    the batches in lockstep: bit for bit under set_batch_invariant, otherwise within the fp32 bound of tests/test_row_seeds.py for a row
    against its batch-1 run (ROW_TOL).  Every output has its input's sample count."""
    from tests.test_row_seeds import ROW_TOL, _batch_invariant
    m = _score(gpu)
    want = _reference(m, invariant)
    recs = _recordings()
    with _batch_invariant(invariant):
        got, nfe = m.enhance_long(recs, window=W_T, overlap=V_T, keys=KEYS_T, return_nfe=True, **how, **KW_T)
    assert nfe == 4 * (3 + 1 + 4)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == recs[i].shape == b.shape and torch.isfinite(a).all() and float(a.abs().max()) > 0
        err = rel_l2(a.cpu(), b)
        print(f"enhance_long {how} invariant={invariant} recording {i}: rel-L2 vs its per-window composition {err:.2e}")
        assert torch.equal(a.cpu(), b) if invariant else err < ROW_TOL, (i, err)


@pytest.mark.gpu
def test_skip_silent(gpu):
    """a recording whose second window is all zero: with skip_silent that window is not sampled (one window's evaluations fewer), the
    samples it alone covers are zero, and the samples that only other windows cover are what they are without skip_silent"""
    m = _score(gpu)
    H = W_T - V_T
    x = _recordings()[2].clone()
    x[H:2 * H + V_T] = 0
    full, nfe = m.enhance_long([x], window=W_T, overlap=V_T, keys=[5], return_nfe=True, **KW_T)
    skip, nfe_s = m.enhance_long([x], window=W_T, overlap=V_T, keys=[5], return_nfe=True, skip_silent=True, **KW_T)
    assert nfe == 4 * 4 and nfe_s == 4 * 3
    # zeros where the skipped window is alone; its neighbours (which the sampler fills although their input is zero there) fade to zero
    assert (skip[0][H + V_T:2 * H] == 0).all() and float(full[0][H + V_T:2 * H].abs().max()) > 0
    assert rel_l2(skip[0][:H].cpu(), full[0][:H].cpu()) < 1e-5 and rel_l2(skip[0][2 * H + V_T:].cpu(), full[0][2 * H + V_T:].cpu()) < 1e-5


@pytest.mark.gpu
def test_peak_none_is_the_call_without_the_keyword(gpu):
    from tests.test_resample import _storm_model
    y = torch.stack([x[:4500] for x in (_recordings()[0], _recordings()[2])]).to(gpu)
    for m, kw in ((_score(gpu), KW_T), (_storm_model(gpu), dict(N=2, corrector="none"))):
        a = m.enhance_batch(y, row_seeds=[1, 2], **kw)
        assert torch.equal(a, m.enhance_batch(y, row_seeds=[1, 2], peak=None, **kw))
        from storm_amd import ops
        assert torch.equal(a, m.enhance_batch(y, row_seeds=[1, 2], peak=ops.peak_abs(y), **kw))    # the rows' own peaks from outside: the same bits
        assert not torch.equal(a, m.enhance_batch(y, row_seeds=[1, 2], peak=2 * ops.peak_abs(y), **kw))


@pytest.mark.gpu
def test_sr_48000(gpu):
    """enhance_long(sr=48000) == resample to 16 kHz, enhance_long there, resample back, trimmed to the input's sample count"""
    m = _score(gpu)
    rs = m.data_module.resample
    g = torch.Generator().manual_seed(9)
    recs = [0.1 * torch.randn(n, generator=g) for n in (3 * int(2.2 * W_T) + 1, 3 * 3000)]
    got = m.enhance_long(recs, window=W_T, overlap=V_T, keys=[4, 5], sr=48000, **KW_T)
    x16 = [rs(x.to(gpu), 48000, 16000) for x in recs]
    assert x16[0].numel() > 2 * W_T > W_T > x16[1].numel()
    mid = m.enhance_long(x16, window=W_T, overlap=V_T, keys=[4, 5], **KW_T)
    for x, a, b in zip(recs, got, mid):
        assert a.shape == x.shape and torch.equal(a, rs(b.contiguous(), 16000, 48000)[:x.numel()])
    mixed = m.enhance_long([recs[0], x16[1]], window=W_T, overlap=V_T, keys=[4, 5], sr=[48000, None], **KW_T)
    assert torch.equal(mixed[0], got[0]) and torch.equal(mixed[1], mid[1])


def _discriminative(backbone, dev):
    from oracle import ncsnpp_ref as NR
    from storm_amd.model import DiscriminativeModel
    from tests import convtasnet_cases as CC
    from tests.test_model import COMMON
    if backbone == "ncsnpp":
        m = DiscriminativeModel(backbone="ncsnpp", input_channels=2, discriminative=True, **dict(COMMON))
        m.dnn.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=41))
    else:
        m = DiscriminativeModel(backbone="convtasnet", **CC.MODEL_KW, **CC.CASES["small"])
        CC.fill(m.dnn)
    m.eval(no_ema=True)
    return m.to(dev)


@pytest.mark.parametrize("backend,backbone", [pytest.param("hip", "ncsnpp", marks=pytest.mark.gpu), pytest.param("hip", "convtasnet", marks=pytest.mark.gpu),
                                              pytest.param("sim", "convtasnet")])
def test_discriminative_enhance_batch_and_long(backend, backbone):
    """DiscriminativeModel.enhance_batch: row b equals enhance(y[b:b+1]) (equal lengths and a ragged pair of one frame bucket), fp32 within
    the bound of a row against its batch-1 run; its enhance_long equals the per-window composition.  (The simulator walks every lane of
    the NCSN++: it runs the small ConvTasNet only.)"""
    from tests.test_row_seeds import ROW_TOL
    gpu = setup_backend(backend)
    m = _discriminative(backbone, gpu)
    recs = _recordings()
    y = torch.stack([recs[0][:5003], recs[2][:5003]]).to(gpu)
    x = m.enhance_batch(y)
    assert x.shape == y.shape and torch.isfinite(x).all()
    for b in range(2):
        one = m.enhance(y[b:b + 1])
        e = rel_l2(x[b].cpu(), one.cpu())
        print(f"DiscriminativeModel({backbone}).enhance_batch row {b}: rel-L2 vs enhance {e:.2e}")
        assert one.shape == (5003,) and float(one.abs().max()) > 0 and e < ROW_TOL
    y[1, 4500:] = 0
    xr = m.enhance_batch(y, lengths=[5003, 4500])
    assert (xr[1, 4500:] == 0).all() and rel_l2(xr[1, :4500].cpu(), m.enhance(y[1:2, :4500]).cpu()) < ROW_TOL
    got = m.enhance_long([recs[0], recs[1]], window=W_T, overlap=V_T, batch=2)
    want = LC.compose(m, recs[0].to(gpu), 0, W_T, V_T, "hann", lambda rows, pk, ks: m.enhance_batch(rows, peak=pk))
    assert got[0].shape == recs[0].shape and rel_l2(got[0].cpu(), want) < ROW_TOL
    assert got[1].shape == recs[1].shape and rel_l2(got[1].cpu(), m.enhance(recs[1][None].to(gpu)).cpu()) < ROW_TOL


# ---- 5. the command line --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_enhancement_cli_window(tmp_path, switch):
    """enhancement.py --window 0.504 --overlap 0.064 (8064 / 1024 samples) --utterance-seed 1 --batch-invariant on a long and a short file:
    files of the input sample counts, equal to enhance_long(keys = the files' utterance keys) up to the wav file's float32; the long file's
    bytes do not change when a third file joins the directory; without --window the files equal the per-file path's"""
    import importlib.util
    import subprocess
    import sys

    from scipy.io import wavfile

    from oracle import ncsnpp_ref as NR
    from storm_amd.model import ScoreModel
    from tests.test_model import COMMON
    spec = importlib.util.spec_from_file_location("enhancement_cli", os.path.join(ROOT, "enhancement.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5)
    ckpt = os.path.join(tmp_path, "m.ckpt")
    torch.save({"state_dict": {"dnn." + k: v for k, v in sd.items()}, "hyper_parameters": dict(backbone="ncsnpp", **COMMON)}, ckpt)
    recs = _recordings()
    files = {"long.wav": recs[0].numpy(), "short.wav": recs[1].numpy(), "third.wav": recs[2].numpy()[:20000]}
    two, three = os.path.join(tmp_path, "two"), os.path.join(tmp_path, "three")
    for d, names in ((two, ("long.wav", "short.wav")), (three, tuple(files))):
        os.makedirs(d)
        for name in names:
            wavfile.write(os.path.join(d, name), 16000, files[name])
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=ROOT).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = [sys.executable, os.path.join(ROOT, "enhancement.py"), "--ckpt", ckpt, "--mode", "score-only", "--N", "2", "--utterance-seed", "1", "--batch-invariant"]
    windowed = ["--window", "0.504", "--overlap", "0.064"]

    def run(src, extra):
        out = src + "_out" + str(len(extra))
        r = subprocess.run(common + ["--test_dir", src, "--enhanced_dir", out] + extra, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return out
    out2, out3, plain = run(two, windowed), run(three, windowed + ["--batch", "3"]), run(two, [])
    m = ScoreModel.load_from_checkpoint(ckpt, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    m.eval(no_ema=False)
    m = m.cuda()
    switch("STORM_BATCH_INVARIANT", 1)
    names = ("long.wav", "short.wav")
    want = m.enhance_long([torch.from_numpy(files[n]) for n in names], window=W_T, overlap=V_T, keys=[cli.utterance_key(1, n) for n in names], **KW_T)
    for name, w in zip(names, want):
        sr, x = wavfile.read(os.path.join(out2, name))
        assert sr == 16000 and x.shape == files[name].shape and x.dtype == np.float32 and np.isfinite(x).all(), name
        assert rel_l2(torch.from_numpy(x), w.cpu()) < 1e-6, name
        sr, p = wavfile.read(os.path.join(plain, name))
        one = m.enhance(torch.from_numpy(files[name])[None], row_seeds=[cli.utterance_key(1, name)], **KW_T)
        assert p.shape == files[name].shape and rel_l2(torch.from_numpy(p), one) < 1e-6, name
    assert open(os.path.join(out2, "long.wav"), "rb").read() == open(os.path.join(out3, "long.wav"), "rb").read()
    assert not np.array_equal(wavfile.read(os.path.join(out2, "long.wav"))[1], wavfile.read(os.path.join(plain, "long.wav"))[1])
