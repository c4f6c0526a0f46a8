"""storm_attention_ws / storm_attention_group (storm_amd/csrc/attention.hip) per QUERY ROW, on the host simulation and on the device:
the 16-bit body (unsplit, key split + merge, grouped launch) and the fp32 kernel at lengths around a key tile (32), a wave's queries (32)
and a query block (128), at C = 32 .. 256.

  * three regimes of the running maximum (jumps and rests; creeps on every tile; rises for even rows and rests for odd ones), every row
    within MARGIN x what a plain float32 restatement with 16-bit P and output shows against float64 (tests/attention_cases.py);
  * cases whose arithmetic is exact by construction - weights 0 / 1, 1 / 1, all equal - with torch.equal;
  * batch strides, ldv, batch rows alone and the grouped launch, bit for bit against the contiguous unsplit call;
  * the refusals of the alignment contract (never launched)."""
import ctypes

import pytest
import torch

from tests import attention_cases as AC
from tests.backend import dev, switch  # noqa: F401

DT = [pytest.param(dt, id=AC.dt_id(dt)) for dt in AC.DTYPES]
DT16 = DT[:2]


def _tag(dev):
    return "device" if dev.type == "cuda" else "simulation"


def _attn(dev, c, switch, S=1, vT=None):
    """the tensor-level call (contiguous operands) with the key split forced to S (1 = never)"""
    from storm_amd import ops
    switch("STORM_ATTN_SPLIT", S)
    bias = c.bias.to(dev) if c.bias is not None else None
    return ops.attention(c.q.to(dev), c.k.to(dev), (c.vT if vT is None else vT).to(dev), bias, c.scale).cpu()


def _splits(dt, L):
    """the forced splits that do split this length (the others run the unsplit kernel: see test_split_rule)"""
    return [S for S in AC.splits_of(dt) if S == 1 or S <= AC.ntiles(L)]


# ---------------------------------------------------------------- measured regimes --------
SETTINGS = [pytest.param(r, dt, C, S, id=f"{r}-{AC.dt_id(dt)}-{C}-S{S}")
            for r in AC.REGIMES for dt in AC.DTYPES for C in AC.CHANNELS for S in AC.splits_of(dt)]


@pytest.mark.parametrize("regime,dt,C,S", SETTINGS)
def test_rows_within_the_plain_restatement(dev, regime, dt, C, S, switch):
    """every query row of every length: worst element and rel-L2 against float64 within MARGIN x the plain restatement's own worst row
    of the setting (regime, dtype, C).  S = the forced key split; lengths it does not split are S = 1's cases."""
    Ls = [L for L in AC.lengths(C) if S in _splits(dt, L)]
    (bound_el, bound_l2), (own_el, own_l2) = AC.regime_bounds(regime, dt, C)
    worst_el = worst_l2 = 0.0
    at = None
    for L in Ls:
        c = AC.regime_case(regime, dt, C, L)
        out = _attn(dev, c, switch, S)
        assert torch.isfinite(out.float()).all(), L
        el, l2 = AC.row_errors(out, AC.regime_refs(regime, dt, C, L)[0])
        if float(el.max()) > worst_el:
            worst_el, at = float(el.max()), (L, int(el.argmax()) // L, int(el.argmax()) % L)
        worst_l2 = max(worst_l2, float(l2.max()))
    print(f"attention {regime} {AC.dt_id(dt)} C={C} S={S} {_tag(dev)}: worst row, element error / row maximum {worst_el:.3e} (bound {bound_el:.3e}, "
          f"restatement {own_el:.3e}) at (L, b, i) = {at}; row rel-L2 {worst_l2:.3e} (bound {bound_l2:.3e}, restatement {own_l2:.3e})")
    assert worst_el <= bound_el and worst_l2 <= bound_l2


@pytest.mark.parametrize("dt", DT)
def test_split_rule(dev, dt, switch):
    """storm_attention_scratch_bytes > 0 exactly when the forced S is at most the key tiles of the call (S = 8 exceeds them at L <= 224);
    never for fp32"""
    from storm_amd import _lib as L_
    for S in AC.SPLITS[1:]:
        switch("STORM_ATTN_SPLIT", S)
        for C in AC.CHANNELS:
            for L in AC.LENGTHS_FULL + (224, 225):
                need = L_.lib().storm_attention_scratch_bytes(AC.BATCH, L, C, L_.dt(dt))
                splits = dt != torch.float32 and S <= AC.ntiles(L)
                assert need == (S * AC.BATCH * L * (C + 2) * 4 if splits else 0), (S, C, L)


# ---------------------------------------------------------------- exact cases -------------
@pytest.mark.parametrize("L", AC.EXACT_LENGTHS)
@pytest.mark.parametrize("C", AC.CHANNELS)
@pytest.mark.parametrize("dt", DT)
def test_one_hot_is_exact(dev, dt, C, L, switch):
    """every query's winner lies 200 binary orders above the rest (asserted in float64 when the case is built), so the weights are exactly
    0 and 1 and the output is v[pi(i)] + bias, bit for bit: the key-to-slot order of the P^T / V^T fragments at every key position, the
    maximum moving on the last tile, the sole valid key of a ragged tile winning and losing, the merge with weights 0 and 1"""
    c, want, gap = AC.one_hot_case(dt, C, L)
    for S in _splits(dt, L):
        out = _attn(dev, c, switch, S)
        assert torch.equal(out, want), (S, gap, int((out != want).any(-1).sum()))


@pytest.mark.parametrize("place", list(AC.TIE_PAIRS))
@pytest.mark.parametrize("C", AC.CHANNELS)
@pytest.mark.parametrize("dt", DT)
def test_tie_is_exact(dev, dt, C, place, switch):
    """two identical keys chosen together: p = 1, 1 and l = 2, within one tile, across the first and the ragged last tile, across split
    ranges - (v_a + v_b) / 2 + bias exactly"""
    c, want = AC.tie_case(dt, C, place)
    for S in _splits(dt, c.L):
        out = _attn(dev, c, switch, S)
        assert torch.equal(out, want), (S, int((out != want).any(-1).sum()))


@pytest.mark.parametrize("C", AC.CHANNELS)
@pytest.mark.parametrize("dt", DT)
def test_uniform_weights_sum_exactly_the_valid_keys(dev, dt, C, switch):
    """q = 0, bias = NULL, v = a_c + 64 s_j with the s_j summing to zero over exactly the L keys: a_c, exactly in the 16-bit types; in
    fp32 within 4 x 2^-23 a_c (the sums are exact; 1 / l and the product round once each, or a reciprocal instruction's last place)"""
    for L in AC.lengths(C):
        c, a = AC.uniform_case(dt, C, L)
        for S in _splits(dt, L)[:2]:                                    # (unsplit and the first split)
            out = _attn(dev, c, switch, S).float()
            if dt == torch.float32:
                assert float(((out - a).abs() / a).max()) <= 4 * 2.0 ** -23, (L, S)
            else:
                assert torch.equal(out, a.expand_as(out)), (L, S, float((out - a).abs().max()))


# ---------------------------------------------------------------- layout ------------------
def _raw(dev, c, q, k, vT, out, ldv, strides, S, switch):
    """storm_attention_ws through the raw binding: q, k, vT, out are device tensors whose data_ptr is the first batch item"""
    from storm_amd import _lib as L_
    switch("STORM_ATTN_SPLIT", S)
    need = L_.lib().storm_attention_scratch_bytes(c.B, c.L, c.C, L_.dt(c.dt))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need > 0 else None
    bias = c.bias.to(dev) if c.bias is not None else None
    L_.check(L_.lib().storm_attention_ws(q.data_ptr(), k.data_ptr(), vT.data_ptr(), L_.ptr(bias), out.data_ptr(), c.B, c.L, c.C, ldv, *strides,
                                         c.scale, L_.dt(c.dt), L_.ptr(ws), need, L_.stream()), "storm_attention_ws")
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _wide(t, gap, fill, dev):
    """[B, n] rows of a [B, n + gap] tensor whose gaps hold `fill`"""
    B = t.shape[0]
    w = torch.full((B, t[0].numel() + gap), fill, dtype=t.dtype)
    w[:, :t[0].numel()] = t.reshape(B, -1)
    return w.to(dev)


LAYOUT = [pytest.param(dt, C, L, id=f"{AC.dt_id(dt)}-{C}-{L}") for dt, C, L in (
    (torch.bfloat16, 64, 33), (torch.float16, 128, 161), (torch.float16, 32, 129), (torch.float32, 64, 161), (torch.float32, 128, 33))]


@pytest.mark.parametrize("dt,C,L", LAYOUT)
def test_batch_strides_other_than_a_packed_batch(dev, dt, C, L, switch):
    """q, k, vT and out as batch rows of wider tensors (strides that are multiples of 8 elements and of nothing larger), NaN in the
    gaps of the inputs and a canary in the gaps of out: the contiguous call's bits, no NaN, the canary untouched - unsplit and split"""
    c = AC.regime_case("random", dt, C, L)
    n, ldv = L * C, c.vT.shape[-1]
    gaps = (8, 24, 40, 72)
    q, k, vT = (_wide(t, g, float("nan"), dev) for t, g in zip((c.q, c.k, c.vT), gaps))
    for S in _splits(dt, L)[:2]:
        want = _attn(dev, c, switch, S)
        out = torch.full((c.B, n + gaps[3]), 77.0, dtype=dt).to(dev)
        _raw(dev, c, q, k, vT, out, ldv, (n + gaps[0], n + gaps[1], C * ldv + gaps[2], n + gaps[3]), S, switch)
        out = out.cpu()
        assert torch.equal(out[:, :n].reshape(c.B, L, C), want), S
        assert bool((out[:, n:] == 77.0).all()), S


@pytest.mark.parametrize("dt,C,L", LAYOUT)
def test_ldv_wider_than_the_rounded_length(dev, dt, C, L, switch):
    """ldv = round_up(L, 8) + 8 and + 64, zeros past L: the bits of ldv = round_up(L, 8)"""
    c = AC.regime_case("random", dt, C, L)
    want = _attn(dev, c, switch)
    for extra in (8, 64):
        assert torch.equal(_attn(dev, c, switch, vT=AC.v_transposed(c.v, AC.round_up(L, 8) + extra)), want), extra


@pytest.mark.parametrize("dt,C,L", LAYOUT)
def test_batch_rows_equal_their_own_calls(dev, dt, C, L, switch):
    """a row of a batch equals its own B = 1 call bit for bit, unsplit and under a forced split"""
    c = AC.regime_case("random", dt, C, L)
    for S in _splits(dt, L)[:2]:
        both = _attn(dev, c, switch, S)
        for b in range(c.B):
            one = AC.Case(c.q[b:b + 1], c.k[b:b + 1], c.v[b:b + 1], c.bias, c.scale, dt)
            assert torch.equal(_attn(dev, one, switch, S), both[b:b + 1]), (S, b)


# ---------------------------------------------------------------- grouped launch ----------
def _group(dev, cases, switch):
    from storm_amd import ops
    switch("STORM_ATTN_SPLIT", 1)
    c0 = cases[0]
    return [o.cpu() for o in ops.attention_group([(c.q.to(dev), c.k.to(dev), c.vT.to(dev)) for c in cases], c0.bias.to(dev), c0.scale)]


@pytest.mark.parametrize("C", (32, 128, 256))
@pytest.mark.parametrize("dt", DT16)
def test_group_problems_equal_their_own_unsplit_calls(dev, dt, C, switch):
    """problems (B, L) = (1, 1), (2, 33), (1, 161), (3, 129) in ONE storm_attention_group launch: each equals its own unsplit call bit
    for bit, and that call is within the setting's bound (so the group is)"""
    cases = [c for c, _ in AC.group_cases(dt, C, "random")]
    outs = _group(dev, cases, switch)
    for c, out in zip(cases, outs):
        assert torch.equal(out, _attn(dev, c, switch)), (c.B, c.L)
        el, l2 = AC.row_errors(out, AC.ref64(c))
        (bound_el, bound_l2), _ = AC.regime_bounds("random", dt, C)
        assert float(el.max()) <= bound_el and float(l2.max()) <= bound_l2, (c.B, c.L)


@pytest.mark.parametrize("C", AC.CHANNELS)
@pytest.mark.parametrize("dt", DT16)
def test_group_one_hot_is_exact(dev, dt, C, switch):
    """the one-hot problems (one bias and one scale for the group: that of the smallest gap) through the grouped launch, bit for bit"""
    cases = AC.group_cases(dt, C, "one_hot")
    outs = _group(dev, [c for c, _ in cases], switch)
    for (c, want), out in zip(cases, outs):
        assert torch.equal(out, want), (c.B, c.L)


@pytest.mark.parametrize("C", AC.CHANNELS)
@pytest.mark.parametrize("dt", DT16)
def test_group_tie_and_uniform_are_exact(dev, dt, C, switch):
    """the uniform case at four lengths in one grouped launch (bias = NULL: a_c exactly), and each placement of the tie as a group of
    its own (its bias and scale are its own)"""
    from storm_amd import ops
    switch("STORM_ATTN_SPLIT", 1)
    cases = [AC.uniform_case(dt, C, L) for _, L in AC.GROUP_PROBLEMS]
    outs = ops.attention_group([(c.q.to(dev), c.k.to(dev), c.vT.to(dev)) for c, _ in cases], None, C ** -0.5)
    for (c, a), out in zip(cases, outs):
        assert torch.equal(out.cpu().float(), a.expand(c.B, c.L, C)), c.L
    for place in AC.TIE_PAIRS:
        c, want = AC.tie_case(dt, C, place)
        assert torch.equal(_group(dev, [c], switch)[0], want), place


# ---------------------------------------------------------------- alignment contract ------
@pytest.mark.parametrize("dt", DT)
def test_calls_outside_the_alignment_contract_are_refused(dev, dt, switch):
    """include/storm_hip.h: q, k, vT, out 16-byte aligned, batch strides multiples of 16 bytes.  Every argument outside it is refused by
    name BEFORE anything is launched (out keeps its canary); nothing misaligned ever runs"""
    from storm_amd import _lib as L_
    C, L = 32, 9
    c = AC.regime_case("random", dt, C, L)
    n, ldv, per16 = L * C, c.vT.shape[-1], 16 // c.q.element_size()
    slack = 2 * per16
    q, k, vT = (_wide(t, slack, 0.0, dev) for t in (c.q, c.k, c.vT))
    out = torch.full((c.B, n + slack), 77.0, dtype=dt).to(dev)
    good = (n + slack, n + slack, C * ldv + slack, n + slack)
    half = per16 // 2                                                    # elements of 8 bytes: aligned for everything but the contract
    for i, name in enumerate(("q", "k", "vT", "out")):
        t = [q, k, vT, out]
        t[i] = t[i].reshape(-1)[half:]
        with pytest.raises(L_.StormError, match=rf"storm_attention: {name} is outside the alignment contract"):
            _raw(dev, c, *t, ldv, good, 1, switch)
        strides = list(good)
        strides[i] += half
        with pytest.raises(L_.StormError, match=rf"storm_attention: {name}_bstride is outside the alignment contract"):
            _raw(dev, c, q, k, vT, out, ldv, tuple(strides), 1, switch)
    assert bool((out.cpu() == 77.0).all())
    _raw(dev, c, q, k, vT, out, ldv, good, 1, switch)                    # (the same call inside the contract runs)
    assert torch.equal(out.cpu()[:, :n].reshape(c.B, L, C), _attn(dev, c, switch))
    if dt == torch.float32:
        return
    # the grouped launch: every pointer of every problem
    P = 2
    bias, blob = c.bias.to(dev), torch.zeros(4096, dtype=torch.uint8, device=dev)
    arr = lambda ts: (ctypes.c_void_p * P)(*[t.data_ptr() for t in ts])  # noqa: E731
    ints = lambda v: (ctypes.c_int * P)(v, v)                            # noqa: E731
    assert L_.lib().storm_attention_group_blob_bytes(ints(1), ints(L), P) <= 4096
    for i, name in enumerate(("q", "k", "vT", "out")):
        t = [[q, q], [k, k], [vT, vT], [out, out.clone()]]
        t[i][1] = t[i][1].reshape(-1)[half:]
        with pytest.raises(L_.StormError, match=rf"storm_attention_group: {name} of problem 1 is outside the alignment contract"):
            L_.check(L_.lib().storm_attention_group(arr(t[0]), arr(t[1]), arr(t[2]), arr(t[3]), ints(1), ints(L), ints(ldv), P, L_.ptr(bias), C,
                                                    c.scale, L_.dt(dt), L_.ptr(blob), 4096, L_.stream()), "storm_attention_group")
    assert not blob.cpu().any()                                          # (nothing was copied, nothing launched)
