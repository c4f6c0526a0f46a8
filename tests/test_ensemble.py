"""Posterior ensembles - K draws per utterance combined on the device (storm_ensemble_combine_rows, ops.ensemble_combine, enhance_ensemble and
the command line) - against the float64 numpy restatement of the definition in include/storm_hip.h (tests/ensemble_cases.py).

Bounds of the kernel comparisons, derived from the definition: the restatement evaluates the header's expressions with the same IEEE
operations in the same order, so the fp64 values agree to a few fp64 units in the last place even where pow is involved; out and spread are
those values rounded to fp32 once, hence at most 1 fp32 ulp of the value's magnitude apart (a rounding boundary between the two fp64 values);
a number of rows_out is a sum of n_terms non-negative terms, each good to a few fp64 ulp, hence n_terms * 2^-53 relative; best is equal.
Every test prints the number of elements that are not bit-equal and the worst ratio to its bound."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ncsnpp_ref as NR
from tests import ensemble_cases as EC
from tests.backend import dev, setup_backend  # noqa: F401
from tests.test_model import COMMON, score_model
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
U = 2.0 ** -53


def _bits(a):
    return a.view(np.uint32) if a.dtype in (np.float32, np.complex64) else a.view(np.uint64)


def _ulp32(mag):
    return np.spacing(np.abs(mag).astype(np.float32)).astype(np.float64)


def _compare(tag, got, ref, F, Tn, K, valid=None, want_spread=True):
    """device results (out, spread, rows, best) against the restatement's: every element, within the bounds of the module's docstring"""
    out, spread, rows, best = (None if v is None else v.cpu().numpy() for v in got)
    ro, rs, rr, rb = ref
    ro32 = ro.astype(np.complex64)
    lim = _ulp32(np.abs(ro))
    eo = np.maximum(np.abs(out.real.astype(np.float64) - ro32.real), np.abs(out.imag.astype(np.float64) - ro32.imag))
    worst_o = float(np.max(np.where(eo == 0, 0.0, eo / lim)))
    ne = [int((_bits(out) != _bits(ro32)).sum())]
    worst_s = 0.0
    if want_spread:
        rs32 = rs.astype(np.float32)
        es = np.abs(spread.astype(np.float64) - rs32)
        worst_s = float(np.max(np.where(es == 0, 0.0, es / _ulp32(rs))))
        ne.append(int((_bits(spread) != _bits(rs32)).sum()))
    else:
        assert spread is None
    bound = np.array([EC.n_terms(F, Tn, K, None if valid is None else valid[b]) for b in range(rr.shape[0])])[:, None] * U * np.abs(rr)
    er = np.abs(rows - rr)
    worst_r = float(np.max(np.where(er == 0, 0.0, er / np.where(bound > 0, bound, 1e-300))))
    ne.append(int((_bits(rows) != _bits(rr)).sum()))
    print(f"ensemble {tag}: not bit-equal out {ne[0]} / {2 * ro.size}, spread {ne[1] if want_spread else '-'} / {rs.size}, rows {ne[-1]} / {rr.size}; "
          f"worst / bound: out {worst_o:.3f} spread {worst_s:.3f} rows {worst_r:.3e}")
    assert out.dtype == np.complex64 and rows.dtype == np.float64 and best.dtype == np.int32
    assert worst_o <= 1.0 and worst_s <= 1.0 and worst_r <= 1.0, (tag, worst_o, worst_s, worst_r)
    assert best.tolist() == rb.tolist(), (tag, best, rb)


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------------
def test_case_table_covers_what_it_claims():
    cs = EC.KERNEL_CASES
    assert {c[0] for c in cs} == {1, 5, 257} and {c[1] for c in cs} == {1, 2, 63, 64, 65, 130} and {c[3] for c in cs} == {1, 3}
    assert {c[2] for c in cs if c[1] % 2} == {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32}
    for K in (2, 5, 32):
        assert {c[4] for c in cs if c[2] == K} == set(EC.MODES), K
    assert {(c[4], c[5]) for c in cs} >= {(m, t) for m in EC.MODES for t in range(3)}
    assert max(c[0] * c[1] for c in cs) > 32 * EC.TILE and len(set(cs)) == len(cs)
    assert EC.TILE == __import__("storm_amd.ops", fromlist=["x"]).ENSEMBLE_TILE and EC.MAX_DRAWS == 32


@pytest.mark.parametrize("case", EC.KERNEL_CASES, ids=EC.case_id)
def test_kernel_against_restatement(dev, case):
    from storm_amd import ops
    F, Tn, K, B, mode, tf = case
    pool, rows, ref = EC.kernel_case(case)
    got = ops.ensemble_combine(T(pool.copy()).to(dev), rows, *EC.TRANSFORMS[tf], mode=mode, spread=True)
    assert got[0].shape == got[1].shape == (B, F, Tn) and got[2].shape == (B, 2 + K) and got[3].shape == (B,)
    _compare(EC.case_id(case), got, ref, F, Tn, K)


def test_without_spread_and_with_a_device_table(dev):
    """spread=False returns None and changes no other bit; draw_row as a device int32 tensor is the same call"""
    from storm_amd import ops
    case = EC.KERNEL_CASES[7]
    pool, rows, ref = EC.kernel_case(case)
    p = T(pool.copy()).to(dev)
    a = ops.ensemble_combine(p, rows, *EC.TRANSFORMS[case[5]], mode=case[4], spread=True)
    b = ops.ensemble_combine(p, torch.tensor(rows, dtype=torch.int32).to(dev), *EC.TRANSFORMS[case[5]], mode=case[4])
    assert b[1] is None and all(torch.equal(torch.view_as_real(a[i]) if i == 0 else a[i], torch.view_as_real(b[i]) if i == 0 else b[i]) for i in (0, 2, 3))
    _compare("no spread", b, ref, case[0], case[1], case[2], want_spread=False)


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------
def _z(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 10.0 ** rng.uniform(-2.0, 1.0, shape)).astype(np.complex64)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7, 8, 16, 32])
def test_identical_draws(dev, K):
    """all K draws the same pool row: best 0 and, where the running sum k x of the definition's order is exact, spread 0, every d_k 0 and the
    mean is the draw itself bit for bit.  That holds for K = 1, 2, 4 whatever x is (x + x and 3 x + x round to 2 x and 4 x; 3 x itself may
    round, and from 5 x on the roundings add up past half an ulp of K x), and for every K when x has few mantissa bits: the (1, 1) transform
    of real or imaginary z is z itself, 24 bits.  Elsewhere the spread is of rounding size: far below one fp32 ulp of |x|."""
    from storm_amd import ops
    z = _z((1, 5, 63), 3)
    axis = np.zeros_like(z)                                                   # (+0 in the other part: a sum from +0 does not keep a -0)
    axis.real[0, :, ::2], axis.imag[0, :, 1::2] = z.real[0, :, ::2], z.imag[0, :, 1::2]
    for pool, tr, exact in ((z, (0.15, 0.5), K in (1, 2, 4)), (z, (0.33, 0.667), K in (1, 2, 4)), (axis, (1.0, 1.0), True)):
        x = EC.back_transform(pool[0], *tr)
        for mode in EC.MODES:
            out, spread, rows, best = ops.ensemble_combine(T(pool).to(dev), [[0] * K], *tr, mode=mode, spread=True)
            assert int(best[0]) == 0
            if exact and (K & (K - 1) == 0 or tr == (1.0, 1.0)):
                assert bool((spread == 0).all()) and bool((rows[0, 1:] == 0).all()), (K, mode, tr)
                want = np.empty(x[0].shape, dtype=np.complex64)
                want.real, want.imag = x[0], x[1]
                got = out[0].cpu().numpy()
                if mode == "mean" or tr == (1.0, 1.0):
                    assert (_bits(got) == _bits(want)).all(), (K, mode, tr)
                else:                                                          # |x| (c / |c|): the unit vector is formed again, a few fp64 ulp
                    assert (np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) <= _ulp32(np.abs(want))).all(), (K, mode, tr)
            else:
                # K - 1 roundings of the running sum and one of the quotient: |x_k - c| <= K 2^-53 |x|, the spread sqrt(K / (K - 1)) times that
                assert float((spread[0].cpu().double() / T(x[2])).max()) <= 2 * K * U and float((rows[0, 1:] / rows[0, 0]).max()) <= (2 * K * U) ** 2
                got = out[0].cpu().numpy()                                     # ... and the combined value is x within one fp32 ulp of |x|
                assert (np.maximum(np.abs(got.real - x[0]), np.abs(got.imag - x[1])) <= _ulp32(x[2])).all(), (K, mode, tr)


@pytest.mark.parametrize("tf", range(3))
def test_opposite_and_rotated_draws(dev, tf):
    """(z, -z): out 0 in every mode, spread sqrt(2) |x| to 1 ulp;  m (1, j, -1, -j) with a real m per bin: c = 0, every d_k = sum |x|^2"""
    from storm_amd import ops
    factor, e = EC.TRANSFORMS[tf]
    z = _z((1, 5, 65), 4)
    g = EC.back_transform(z[0], factor, e)[2]
    m = np.abs(z).astype(np.float32).astype(np.complex64)
    gm = EC.back_transform(m[0], factor, e)[2]
    pool = T(np.concatenate([z, -z, m, 1j * m, -m, -1j * m])).to(dev)
    for mode in EC.MODES:
        out, spread, rows, best = ops.ensemble_combine(pool, [[0, 1]], factor, e, mode=mode, spread=True)
        assert bool((torch.view_as_real(out) == 0).all()) and float(rows[0, 0]) == 0.0 and int(best[0]) == 0
        want = (math.sqrt(2.0) * g).astype(np.float32)
        assert (np.abs(spread[0].cpu().numpy().astype(np.float64) - want) <= _ulp32(want)).all()
        out4, _, rows4, best4 = ops.ensemble_combine(pool, [[2, 3, 4, 5]], factor, e, mode=mode)
        assert bool((torch.view_as_real(out4) == 0).all()) and float(rows4[0, 0]) == 0.0 and int(best4[0]) == 0
        assert np.abs(rows4[0, 1:].cpu().numpy() / float((gm * gm).sum()) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("K", [2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
def test_arithmetic_progression(dev, K):
    """the (1, 1) transform with z_k = k + 1: mean and median are (K + 1) / 2 exactly, for odd and even K, the spread is the closed form
    sqrt(K (K + 1) / 12); on top of 1024 in steps of 1 / 1024 the same holds (E[x^2] - |c|^2 would lose the spread there)"""
    from storm_amd import ops
    order = np.random.default_rng(K).permutation(K)                           # the median does not get them sorted
    for base, step in ((0.0, 1.0), (1024.0, 1.0 / 1024.0)):
        vals = base + step * (np.arange(K) + 1.0)
        pool = np.zeros((K, 1, 3), dtype=np.complex64)
        pool[:, 0, 0], pool[:, 0, 1], pool[:, 0, 2] = vals[order], 1j * vals[order], -vals[order]
        mid = base + step * (K + 1) / 2.0
        sd = np.float32(step * math.sqrt(K * (K + 1) / 12.0))
        for mode in EC.MODES:
            out, spread, rows, best = ops.ensemble_combine(T(pool).to(dev), [list(range(K))], 1.0, 1.0, mode=mode, spread=True)
            assert torch.view_as_real(out[0, 0]).tolist() == [[mid, 0.0], [0.0, mid], [-mid, 0.0]], (K, mode, base)
            assert (np.abs(spread[0, 0].cpu().numpy().astype(np.float64) - sd) <= np.spacing(sd)).all(), (K, mode, base, spread)
            assert float(rows[0, 0]) == 3 * mid * mid
            assert int(best[0]) == int(np.argmin(np.abs(vals[order] - mid)))   # (even K: the two middle draws tie, the lower k wins)


def test_planted_medoid_and_tie(dev):
    """draws c + d_k with |d_k| planted: the closest draw is best; with two equally close ones the lowest k wins, wherever they stand"""
    from storm_amd import ops
    base = np.full((1, 4, 8), 2.0 + 0j, dtype=np.complex64)
    offs = [4.0, -4.0, 1.0, -1.0, 0.5j, -0.5j, 8.0, -8.0]                     # mean = base exactly; |d| = 0.5 twice, at k = 4 and 5
    pool = T(np.concatenate([base + o for o in offs]).astype(np.complex64)).to(dev)
    for rows, want in (([0, 1, 2, 3, 4, 5, 6, 7], 4), ([5, 4, 0, 1, 2, 3, 6, 7], 0), ([0, 1, 6, 7, 2, 3, 5, 4], 6), ([0, 1, 2, 3, 6, 7, 4, 5], 6),
                       ([2, 3, 0, 1], 0), ([0, 1, 3, 2], 2)):
        out, _, r, best = ops.ensemble_combine(pool, [rows], 1.0, 1.0)
        d = r[0, 2:].tolist()
        assert int(best[0]) == want and d[want] == min(d) and d.count(min(d)) == 2, (rows, d)
        assert bool((out == 2.0).all()) and float(r[0, 0]) == 4.0 * 32 and float(r[0, 1]) == sum(d) / len(d)


# ---- 3. layout and independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,Tn,K,mode", [(5, 65, 5, "mag_median"), (257, 63, 3, "mean")])
def test_rows_do_not_depend_on_batch_stride_or_pool_order(dev, F, Tn, K, mode):
    """an utterance of a B = 3 call is bit-equal to its own B = 1 call; the same at another (odd: rows off 16 bytes) pool stride and with
    the pool rows reversed and interleaved through draw_row"""
    from storm_amd import ops
    N = 3 * K
    pool = T(EC.pool_for(N, F, Tn, 77)).to(dev)
    table = [[b * K + k for k in range(K)] for b in range(3)]
    whole = ops.ensemble_combine(pool, table, 0.33, 0.667, mode=mode, spread=True)
    same = lambda a, b: torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)      # noqa: E731
    for b in range(3):
        alone = ops.ensemble_combine(pool, [table[b]], 0.33, 0.667, mode=mode, spread=True)
        assert all(same(alone[i][0], whole[i][b]) for i in range(4)), b
    wide = torch.zeros((N + 1, F * Tn + 3), dtype=torch.complex64, device=dev)
    view = wide[:N, :F * Tn].unflatten(1, (F, Tn))
    view.copy_(pool)
    assert view.stride() == (F * Tn + 3, Tn, 1) and view.data_ptr() == wide.data_ptr()
    again = ops.ensemble_combine(view, table, 0.33, 0.667, mode=mode, spread=True)
    assert all(same(again[i], whole[i]) for i in range(4))
    perm = [(7 * r + 2) % N for r in range(N)][::-1]                          # pool row r moves to perm[r]: reversed and interleaved
    assert sorted(perm) == list(range(N))
    moved = torch.empty_like(pool)
    moved[perm] = pool
    shuffled = ops.ensemble_combine(moved, [[perm[r] for r in row] for row in table], 0.33, 0.667, mode=mode, spread=True)
    assert all(same(shuffled[i], whole[i]) for i in range(4))
    assert not same(ops.ensemble_combine(moved, table, 0.33, 0.667, mode=mode)[0], whole[0])          # (the table is really read)


def test_frames_keep_padding_out(dev):
    """frames: NaN in every bin past frames[b] reaches nothing - rows_out is the restatement's over the valid bins, out and spread are zero
    there; an odd and an even count, a full row and a single frame"""
    from storm_amd import ops
    F, Tn, K, B = 5, 64, 3, 4
    frames = [37, 64, 1, 22]
    pool = EC.pool_for(B * K, F, Tn, 88)
    table = [[b * K + k for k in range(K)] for b in range(B)]
    for mode in ("mean", "mag_median"):
        ref = EC.combine(pool, table, 0.15, 0.5, mode, frames=frames)
        dirty = pool.copy()
        for b in range(B):
            dirty[b * K:(b + 1) * K, :, frames[b]:] = np.nan + 1j * np.nan
        got = ops.ensemble_combine(T(dirty).to(dev), table, 0.15, 0.5, mode=mode, frames=frames, spread=True)
        assert bool(torch.isfinite(got[2]).all())
        for b in range(B):
            assert bool((torch.view_as_real(got[0][b, :, frames[b]:]) == 0).all()) and bool((got[1][b, :, frames[b]:] == 0).all())
        _compare(f"frames {mode}", got, ref, F, Tn, K, valid=frames)
        full = EC.combine(pool, table, 0.15, 0.5, mode)
        assert all(full[2][b, 0] > ref[2][b, 0] for b in (0, 2, 3)) and full[2][1, 0] == ref[2][1, 0]       # (padding counted in E would be seen)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(dev):
    from storm_amd import _lib, ops
    lib = _lib.lib()
    q = lib.storm_ensemble_scratch_bytes
    assert q(2, 5, 63, 3) == 2 * 1 * 4 * 8 and q(1, 257, 130, 32) == 33 * 33 * 8
    assert 0 == q(0, 5, 63, 3) == q(2, 0, 63, 3) == q(2, 5, 0, 3) == q(2, 5, 63, 0) == q(2, 5, 63, 33) == q(65536, 5, 63, 3) == q(1, 65536, 65536, 2)
    B, K, F, Tn, N = 2, 3, 5, 63, 6
    pool = torch.zeros((N, F, Tn), dtype=torch.complex64, device=dev)
    table = torch.arange(6, dtype=torch.int32, device=dev).reshape(2, 3)
    out = torch.full((B, F, Tn, 2), 7.0, device=dev)
    spread = torch.full((B, F, Tn), 7.0, device=dev)
    rows = torch.full((B, 2 + K), 7.0, dtype=torch.float64, device=dev)
    best = torch.full((B,), 7, dtype=torch.int32, device=dev)
    need = q(B, F, Tn, K)
    ws = torch.full((need // 8 + 1,), 7.0, dtype=torch.float64, device=dev)

    def call(p=pool.data_ptr(), N=N, stride=F * Tn, t=table.data_ptr(), o=out.data_ptr(), r=rows.data_ptr(), b=best.data_ptr(), s=ws.data_ptr(),
             bytes_=need, B=B, K=K, F=F, Tn=Tn, factor=0.15, e=0.5, mode=0):
        return lib.storm_ensemble_combine_rows(p, N, stride, t, o, spread.data_ptr(), r, b, s, bytes_, B, K, F, Tn, None, factor, e, mode, _lib.stream())
    for kw, word in ((dict(p=None), "null pointer"), (dict(t=None), "null pointer"), (dict(o=None), "null pointer"), (dict(r=None), "null pointer"),
                     (dict(b=None), "null pointer"), (dict(s=None), "null pointer"), (dict(B=0), "B=0"), (dict(F=0), "F=0"), (dict(Tn=0), "T=0"),
                     (dict(N=0), "N=0"), (dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(stride=F * Tn - 1), f"pool_stride={F * Tn - 1}"),
                     (dict(p=pool.data_ptr() + 8), "16-byte aligned"), (dict(o=out.data_ptr() + 8), "16-byte aligned"), (dict(bytes_=need - 8), "scratch"),
                     (dict(s=ws.data_ptr() + 4), "8-byte aligned"), (dict(mode=3), "mode=3"), (dict(mode=-1), "mode=-1"), (dict(factor=0.0), "factor=0"),
                     (dict(e=0.0), "exponent=0"), (dict(e=-0.5), "exponent=-0.5")):
        assert call(**kw) != 0 and word in lib.storm_last_error().decode(), (kw, lib.storm_last_error().decode())
    assert all(bool((v == 7).all()) for v in (out, spread, rows, best, ws))  # no kernel ran: every canary stands
    assert call() == 0 and bool((out == 0).all()) and bool((rows == 0).all()) and best.tolist() == [0, 0]
    with pytest.raises(ValueError, match="mode"):
        ops.ensemble_combine(pool, [[0, 1]], 0.15, 0.5, mode="median")
    with pytest.raises(ValueError, match="outside the pool"):
        ops.ensemble_combine(pool, [[0, 6]], 0.15, 0.5)
    with pytest.raises(ValueError, match="draws"):
        ops.ensemble_combine(pool, [[0] * 33], 0.15, 0.5)
    with pytest.raises(ValueError, match="complex64"):
        ops.ensemble_combine(torch.view_as_real(pool), [[0, 1]], 0.15, 0.5)
    with pytest.raises(ValueError, match="frames"):
        ops.ensemble_combine(pool, [[0, 1]], 0.15, 0.5, frames=[64])


def test_draw_key():
    from storm_amd import ops
    assert ops.draw_key(11, 0) == 11 and ops.draw_key(11, 1) == 11 + 0xD1B54A32D192ED03 - 2 ** 63
    assert ops.draw_key(2 ** 63 - 1, 3) == (2 ** 63 - 1 + 3 * 0xD1B54A32D192ED03) % 2 ** 63 == EC.draw_key(2 ** 63 - 1, 3)
    assert len({ops.draw_key(5, k) for k in range(32)} | {ops.window_key(5, k) for k in range(32)}) == 64
    assert tuple(ops.ENSEMBLE_MODES) == EC.MODES
    with pytest.raises(ValueError):
        ops.draw_key(5, -1)


# ---- 5. the models, on a tiny net ----------------------------------------------------------------------------------------------------------
# nf = 8, N = 2 reverse steps, two utterances of about 4000 samples with ragged lengths in one 64-frame bucket, K = 3, batch-invariant.  On
# the MI355X the networks are the seeded tiny NCSN++ of tests/test_model.py.  The host simulation walks every lane of every kernel (seconds
# per row and network evaluation), so there the networks' forward passes are replaced by elementwise functions of their inputs; everything
# the ensemble adds - keys, pooling, replication, the combine launch, the gather, both iSTFT routes - runs its kernels on both.
KEYS, LENS, K3 = [11, 2 ** 40 + 5], [4000, 3777], 3
SAMPLER = dict(N=2, snr=0.5)


def _storm_model(dev):
    from storm_amd.model import StochasticRegenerationModel
    m = StochasticRegenerationModel(backbone_denoiser="ncsnpp", backbone_score="ncsnpp", condition="both", **dict(COMMON))
    m.denoiser_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=2, discriminative=True), seed=42))
    m.score_net.load_state_dict(NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=6), seed=43))
    m._error_loading_ema = True
    return m.eval().to(dev)


def _model(dev, kind):
    m = score_model(dev) if kind == "score" else _storm_model(dev)
    if dev.type == "cpu":
        std = lambda t: m.sde._std(t)[:, None, None, None] ** 2 + 0.1         # noqa: E731
        if kind == "score":
            m.forward = lambda x, t, y, **kw: -(x - y) * (1 + 4 * y.abs()) / std(t)
        else:
            m.forward_score = lambda x, t, score_conditioning, sde_input, **kw: -(x - sde_input) * (1 + 4 * score_conditioning[0].abs()) / std(t)
            m.forward_denoiser = lambda y, **kw: y * (0.5 + 0.25 * torch.tanh(y.abs()))
    return m


def _utterances(dev):
    g = torch.Generator().manual_seed(61)
    y = torch.zeros(2, max(LENS))
    for b, n in enumerate(LENS):
        y[b, :n] = 0.1 * (b + 1) * torch.randn(n, generator=g)
    return y.to(dev)


class _invariant:
    def __enter__(self):
        import storm_amd
        storm_amd.set_batch_invariant(True)

    def __exit__(self, *exc):
        import storm_amd
        storm_amd.set_batch_invariant(False)


def _same(a, b):
    return a.shape == b.shape and (torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b))


@pytest.mark.parametrize("kind", ["score", "storm"])
def test_model_ensemble_is_the_combine_of_the_public_per_draw_calls(dev, kind):
    """enhance_ensemble(return_stft=True) == ops.ensemble_combine over the K samples of the public per-draw calls (ScoreModel:
    enhance(return_stft=True, seed=draw_key(key, k)); StoRM: enhance_batch(return_stft=True, row_seeds=[that key])), bit for bit, spread and
    agreement included; the waveform == ops.istft of that spectrogram times the peak; StoRM's denoiser runs ONCE, with B rows;
    'medoid' is the chosen draw's own enhance_batch result; the waveform of 'mean' agrees with the mean of the K per-draw enhance_batch
    waveforms within 4 x the measured rel-L2 between one draw's fp32 spec_to_wav and the float64 back-transform + ops.istft(1, 1)"""
    from storm_amd import ops
    m = _model(dev, kind)
    dm = m.data_module
    y = _utterances(dev)
    frames = [-(-(n + dm.n_fft // 2) // dm.hop_length) for n in LENS]        # the frames that reach the utterance's samples: 34 and 32 of 64
    calls = []
    if kind == "storm":
        inner = m.forward_denoiser
        m.forward_denoiser = lambda Y, **kw: (calls.append(Y.shape[0]), inner(Y, **kw))[1]
    with _invariant():
        x, spread, agree, stft = m.enhance_ensemble(y, draws=K3, combine="mean", keys=KEYS, lengths=LENS, return_spread=True, return_stft=True, **SAMPLER)
        assert calls == ([2] if kind == "storm" else [])
        calls.clear()
        x_med, stft_med = m.enhance_ensemble(y, draws=K3, combine="medoid", keys=KEYS, lengths=LENS, return_stft=True, **SAMPLER)
        x_mm = m.enhance_ensemble(y, draws=K3, combine="mag_median", keys=KEYS, lengths=LENS, **SAMPLER)
        samples, waves, peaks = [], [], []
        for b, n in enumerate(LENS):
            for k in range(K3):
                key = ops.draw_key(KEYS[b], k)
                if kind == "score":
                    s, _, _, pk = m.enhance(y[b:b + 1, :n], return_stft=True, seed=key, **SAMPLER)
                else:
                    s, _, _, pk = m.enhance_batch(y[b:b + 1, :n], return_stft=True, row_seeds=[key], **SAMPLER)
                samples.append(s)
                waves.append(m.enhance_batch(y[b:b + 1, :n], row_seeds=[key], **SAMPLER)[0])
            peaks.append(pk)
    pool = torch.stack(samples)
    table = [[b * K3 + k for k in range(K3)] for b in range(2)]
    want = ops.ensemble_combine(pool, table, dm.spec_factor, dm.spec_abs_exponent, mode="mean", frames=frames, spread=True)
    assert x.shape == y.shape and stft.shape == spread.shape == (2,) + tuple(pool.shape[1:])
    assert _same(stft, want[0]) and _same(spread, want[1]) and _same(agree, 10.0 * torch.log10(want[2][:, 0] / want[2][:, 1]))
    assert bool(torch.isfinite(agree).all()) and float(spread.max()) > 0 and bool((spread[1, :, frames[1]:] == 0).all())
    peak = torch.tensor(peaks, dtype=torch.float32, device=dev)
    wav = ops.istft(want[0], y.shape[1], peak, n_fft=dm.n_fft, hop=dm.hop_length, spec_factor=1.0, spec_abs_exponent=1.0, window=dm.window_type, lengths=LENS)
    assert _same(x, wav) and bool((x[1, LENS[1]:] == 0).all())
    # medoid: the chosen draw's own result, bit for bit
    best = want[3].tolist()
    for b, n in enumerate(LENS):
        assert _same(x_med[b, :n], waves[b * K3 + best[b]]) and _same(stft_med[b], dm.spec_back(samples[b * K3 + best[b]][None])[0]), b
    assert not _same(x_mm, x) and bool(torch.isfinite(x_mm).all())
    # the waveform of the mean against the mean of the per-draw waveforms
    s0 = samples[0][None]
    xr, xi, _ = EC.back_transform(s0.cpu().numpy(), dm.spec_factor, dm.spec_abs_exponent)
    lin = T((xr + 1j * xi).astype(np.complex64)).to(dev)
    route = ops.istft(lin, LENS[0], peak[:1], n_fft=dm.n_fft, hop=dm.hop_length, spec_factor=1.0, spec_abs_exponent=1.0, window=dm.window_type)
    one = rel_l2(waves[0].cpu(), route[0].cpu())
    for b, n in enumerate(LENS):
        mean = torch.stack([waves[b * K3 + k].double() for k in range(K3)]).mean(0)
        err = rel_l2(x[b, :n].double().cpu(), mean.cpu())
        print(f"ensemble {kind} {dev.type}: utterance {b} mean-of-draws waveform rel-L2 {err:.3e}, one draw's two routes {one:.3e} (bound 4 x)")
        assert err <= 4 * one and one > 0, (b, err, one)


@pytest.mark.parametrize("kind", ["score", "storm"])
def test_one_draw_is_enhance_batch(dev, kind):
    """draws=1: enhance_batch(y, row_seeds=keys) bit for bit, whatever `combine`; the spread is zeros, the agreement +inf"""
    m = _model(dev, kind)
    y = _utterances(dev)
    with _invariant():
        want = m.enhance_batch(y, lengths=LENS, row_seeds=KEYS, **SAMPLER)
        x, spread, agree, stft = m.enhance_ensemble(y, draws=1, combine="mag_median", keys=KEYS, lengths=LENS, return_spread=True, return_stft=True, **SAMPLER)
        x2, nfe = m.enhance_ensemble(y, keys=KEYS, lengths=LENS, return_nfe=True, batch=1, **SAMPLER)      # (batch < B: still the one run of enhance_batch)
    assert _same(x, want) and _same(x2, want) and nfe == 2 * SAMPLER["N"] * (2 if kind == "score" else 1)
    assert bool((spread == 0).all()) and spread.shape == stft.shape and agree.tolist() == [math.inf, math.inf] and stft.dtype == torch.complex64


def test_model_argument_errors(dev):
    from storm_amd.model import DiscriminativeModel
    m = _model(dev, "score")
    y = _utterances(dev)
    for kw, word in ((dict(draws=0), "draws=0"), (dict(draws=33), "draws=33"), (dict(combine="median"), "combine"), (dict(keys=[1]), "keys has 1"),
                     (dict(keys=KEYS, seed=3), "exclude"), (dict(row_seeds=KEYS), "row_seeds"), (dict(batch=0), "batch=0")):
        with pytest.raises(ValueError, match=word):
            m.enhance_ensemble(y, **{"draws": 2, **kw})
    d = DiscriminativeModel(backbone="ncsnpp", **dict(COMMON))
    with pytest.raises(ValueError, match="draws=2"):
        d.enhance_ensemble(y, draws=2)


def test_evaluate_model_with_one_draw_changes_nothing(dev):
    from storm_amd.util.inference import evaluate_model
    m = _model(dev, "score")
    g = torch.Generator().manual_seed(5)
    pairs = [(0.1 * torch.randn(1, n, generator=g), 0.1 * torch.randn(1, n, generator=g)) for n in (4000, 3900)]
    kw = dict(audio=True, pairs=pairs, batch=2, metrics=True, seed=9, **SAMPLER)
    a, b = evaluate_model(m, 2, **kw), evaluate_model(m, 2, draws=1, combine="mean", **kw)
    assert a[1] == b[1] and a[5] == b[5] and all(torch.equal(u, v) for u, v in zip(a[4][1], b[4][1]))
    c = evaluate_model(m, 2, draws=2, combine="mag_mean", **kw)
    assert c[1] != a[1] and math.isfinite(c[1])
    with pytest.raises(ValueError, match="noise_for"):
        evaluate_model(m, 2, draws=2, noise_for=lambda ids: None, **kw)
    # keys=: one per file, handed to the micro-batch its file is in (batch=1: two micro-batches) - seed=9 is keys=[9, 10]
    kw.pop("seed")
    with _invariant():
        e, f = evaluate_model(m, 2, draws=2, combine="mag_mean", keys=[9, 10], **kw), evaluate_model(m, 2, draws=2, combine="mag_mean", seed=9, **kw)
        d = evaluate_model(m, 2, draws=2, combine="mag_mean", **{**kw, "batch": 1, "keys": [9, 10]})
    assert all(torch.equal(u, v) and torch.equal(u, w) for u, v, w in zip(d[4][1], e[4][1], f[4][1]))


def test_ode_sampler_passes_through(dev):
    """sampler_type='ode' (one step controller per row): 'medoid' returns one of the per-draw enhance_batch(sampler_type='ode') waveforms
    bit for bit, and return_nfe is the sum of the rows' own evaluation counts.  An elementwise score on both backends: the ODE takes some
    hundred evaluations"""
    from storm_amd import ops
    m = _model(torch.device("cpu"), "score") if dev.type == "cpu" else score_model(dev)
    if dev.type != "cpu":
        std = lambda t: m.sde._std(t)[:, None, None, None] ** 2 + 0.1         # noqa: E731
        m.forward = lambda x, t, y, **kw: -(x - y) * (1 + 4 * y.abs()) / std(t)
    y = _utterances(dev)[:1, :LENS[0]]
    with _invariant():
        x, nfe = m.enhance_ensemble(y, draws=2, combine="medoid", keys=KEYS[:1], return_nfe=True, sampler_type="ode")
        each, counts = [], []
        for k in range(2):
            w, _ = m.enhance_batch(y, row_seeds=[ops.draw_key(KEYS[0], k)], return_nfe=True, sampler_type="ode")
            each.append(w[0])
            counts.append(int(m.last_nfev_rows[0]))
    assert nfe == sum(counts) and min(counts) > 10
    assert sum(_same(x[0], w) for w in each) == 1


# ---- 6. the command line (GPU only, like the other command-line tests) ----------------------------------------------------------------------
@pytest.mark.gpu
def test_enhancement_cli_draws(tmp_path):
    """enhancement.py --draws 3 --utterance-seed 5 --spread-dir on three files of two lengths: wavs and spreads equal enhance_ensemble of
    the same files (keys = the files' utterance keys); without --draws, and with --draws 1, the files are what the flags of before give -
    enhance_batch with the files' keys"""
    import importlib.util

    from scipy.io import wavfile

    from storm_amd.model import ScoreModel
    setup_backend("hip")
    spec = importlib.util.spec_from_file_location("enhancement_cli", os.path.join(ROOT, "enhancement.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    sd = NR.seeded_state_dict(NR.NCSNppConfig(nf=8, input_channels=4), seed=5)
    ckpt = os.path.join(tmp_path, "m.ckpt")
    torch.save({"state_dict": {"dnn." + k: v for k, v in sd.items()}, "hyper_parameters": dict(backbone="ncsnpp", **COMMON)}, ckpt)
    g = torch.Generator().manual_seed(9)
    files = {"a0.wav": 6000, "a1.wav": 6000, "b0.wav": 5100}
    src = os.path.join(tmp_path, "noisy")
    os.makedirs(src)
    wavs = {}
    for name, n in files.items():
        wavs[name] = (0.1 * torch.randn(n, generator=g)).numpy().astype(np.float32)
        wavfile.write(os.path.join(src, name), 16000, wavs[name])
    env = {k: v for k, v in dict(os.environ, PYTHONPATH=ROOT).items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--ckpt", ckpt, "--mode", "score-only", "--N", "2", "--corrector", "ald", "--utterance-seed", "5", "--batch-invariant", "--batch", "4"]
    runs = {"k3": ["--draws", "3", "--combine", "mag_mean", "--spread-dir", os.path.join(tmp_path, "spread")], "plain": [], "k1": ["--draws", "1"]}
    for key, extra in runs.items():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "enhancement.py"), "--test_dir", src, "--enhanced_dir", os.path.join(tmp_path, key)] + common + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "enhancement.py"), "--test_dir", src, "--enhanced_dir", os.path.join(tmp_path, "w")] + common
                       + ["--draws", "3", "--window", "4.0"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--window" in (r.stderr + r.stdout) and "--draws" in (r.stderr + r.stdout)
    m = ScoreModel.load_from_checkpoint(ckpt, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    m.eval(no_ema=False)
    m.cuda()
    dm = m.data_module
    skw = dict(corrector="ald", N=2, corrector_steps=1, snr=0.5)
    names = sorted(files)
    with _invariant():
        for name in names:
            y = T(wavs[name])[None].cuda()
            key = cli.utterance_key(5, name)
            x, spread, _ = m.enhance_ensemble(y, draws=3, combine="mag_mean", keys=[key], batch=4, return_spread=True, **skw)
            got = wavfile.read(os.path.join(tmp_path, "k3", name))[1]
            assert got.dtype == np.float32 and (got == x[0].cpu().numpy()).all(), name
            sp = np.load(os.path.join(tmp_path, "spread", name[:-4] + ".npy"))
            frames = 1 + files[name] // dm.hop_length
            assert sp.shape == (dm.n_fft // 2 + 1, frames) and sp.dtype == np.float32 and (sp == spread[0, :, :frames].cpu().numpy()).all() and sp.max() > 0
            plain = m.enhance_batch(y, row_seeds=[key], **skw)
            assert (wavfile.read(os.path.join(tmp_path, "plain", name))[1] == plain[0].cpu().numpy()).all(), name
            assert open(os.path.join(tmp_path, "plain", name), "rb").read() == open(os.path.join(tmp_path, "k1", name), "rb").read()
            assert not (got == plain[0].cpu().numpy()).all()


# ---- 7. the kernels under the simulator's skewed wave schedules ------------------------------------------------------------------------------
# the two smallest cases in which more than one wave of a workgroup holds bins: the tile's sums cross waves through LDS behind a barrier
SKEWED = ["tests/test_ensemble.py::test_kernel_against_restatement[sim-1-130-8-1-mean-2]",            # 130 bins, 65 pairs: waves 0 and 1 (one lane of wave 1)
          "tests/test_ensemble.py::test_kernel_against_restatement[sim-5-63-1-1-mean-0]"]             # 315 bins, 158 pairs: waves 0, 1 and 2, a lone last bin


@pytest.mark.parametrize("waves", ["reverse", "first", "last", "seed:1"])
def test_kernels_under_skewed_wave_schedules(waves):
    """the combine and the row kernel with the simulator's waves run in another order (STORM_SIM_WAVES, read when the simulation is loaded: a
    process of its own, as tests/test_sim_schedules.py runs its selection): the two smallest multi-wave cases pass"""
    env = dict(os.environ, PYTHONPATH=ROOT, STORM_SIM_WAVES=waves, STORM_TEST_WORKERS="2")
    env.pop("STORM_SIM_DMA", None)
    r = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(ROOT, t) for t in SKEWED] + ["-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == len(SKEWED) and "skipped" not in r.stdout, r.stdout[-1000:]
