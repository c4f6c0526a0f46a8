"""Case tables, seeded inputs and host references for tests/test_attention_edges.py (storm_attention_ws, storm_attention_group: the
kernels of storm_amd/csrc/attention.hip), per QUERY ROW.

Two references, both on the host and neither mirroring the kernel's tiling:
  ref64      float64 softmax(scale q k^T) v + bias on the values the kernel is given (16-bit-valued for bf16 / fp16);
  plain(dt)  the same in float32; for a 16-bit dt the softmax weights are rounded to dt before the second product and the result is
             rounded to dt - what include/storm_hip.h says the kernel does ("P and the output rounded to the operand type").
Every bound of a measured regime is MARGIN[dt] times what plain(dt) shows against ref64, in the same per-row metric, over the cases of
the setting (regime, dtype, C): 2 for the 16-bit types (both errors are the rounding of P and of the output; the kernel rounds P relative
to the running maximum, which if anything is kinder), 4 for fp32 (the device's exp2 and the MFMA's summation order are not the host's).

The exact cases are those where the arithmetic is exact by construction: weights of exactly 0 and 1 (one-hot), 1 and 1 (tie), all 1
with sums that are small integers (uniform).  They are compared with torch.equal."""
import functools
import math

import torch

BATCH = 2
BK, BQ = 32, 128                        # attention.hip: keys per tile, queries per workgroup
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
MARGIN = {torch.bfloat16: 2.0, torch.float16: 2.0, torch.float32: 4.0}
CHANNELS = (32, 64, 128, 256)
# one below / at / one above a key tile (32), a wave's 32 queries, a query block (128); 161 = 5 x 32 + 1 = 128 + 33: ONE valid key in the
# ragged tile, and a second query block of a full wave plus one query; 257: 9 key tiles, which split unevenly
LENGTHS_FULL = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 257)
LENGTHS_THIN = (1, 7, 33, 129, 161, 257)
EXACT_LENGTHS = (1, 2, 7, 33, 129, 161, 257)
REGIMES = ("random", "flat", "ramp")
SPLITS = (1, 2, 4, 8)                   # STORM_ATTN_SPLIT: 1 = never; S > ceil(L / 32) runs unsplit
GROUP_PROBLEMS = ((1, 1), (2, 33), (1, 161), (3, 129))      # (B, L) of one storm_attention_group launch
MIN_GAP = 160                           # one-hot / tie: binary orders between the winner and every other key (2^-160 is 0 in fp32)


def lengths(C):
    return LENGTHS_FULL if C == 64 else LENGTHS_THIN


def ntiles(L):
    return -(-L // BK)


def splits_of(dt):
    return (1,) if dt == torch.float32 else SPLITS


def dt_id(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dt]


def round_up(x, m):
    return (x + m - 1) // m * m


def v_transposed(v, ldv=None):
    """v [B, L, C] -> the kernel's vT [B, C, ldv], zeros past L"""
    B, L, C = v.shape
    vT = torch.zeros(B, C, ldv or round_up(L, 8), dtype=v.dtype)
    vT[:, :, :L] = v.transpose(1, 2)
    return vT


class Case:
    """q, k, v [B, L, C] and vT [B, C, ldv] in the operand type, bias fp32 [C] or None, scale"""

    def __init__(self, q, k, v, bias, scale, dt):
        self.q, self.k, self.v = q.to(dt).contiguous(), k.to(dt).contiguous(), v.to(dt).contiguous()
        self.vT = v_transposed(self.v)
        self.bias, self.scale, self.dt = bias, float(scale), dt
        self.B, self.L, self.C = q.shape


# ---------------------------------------------------------------- references --------------
def ref64(c):
    w = torch.softmax(torch.einsum("bic,bjc->bij", c.q.double(), c.k.double()) * c.scale, -1)
    out = torch.einsum("bij,bjc->bic", w, c.v.double())
    return out + c.bias.double() if c.bias is not None else out


def plain(c):
    w = torch.softmax(torch.einsum("bic,bjc->bij", c.q.float(), c.k.float()) * torch.tensor(c.scale, dtype=torch.float32), -1)
    if c.dt != torch.float32:
        w = w.to(c.dt).float()
    out = torch.einsum("bij,bjc->bic", w, c.v.float())
    if c.bias is not None:
        out = out + c.bias
    return out.to(c.dt)


def row_errors(out, ref):
    """per query row [B, L]: (largest element error / the row's largest reference element, the row's rel-L2)"""
    d = out.double() - ref
    return d.abs().amax(-1) / ref.abs().amax(-1), d.norm(dim=-1) / ref.norm(dim=-1)


# ---------------------------------------------------------------- measured regimes --------
@functools.lru_cache(maxsize=None)
def regime_case(regime, dt, C, L):
    """random: q, k Gaussian, q *= 1.5 (the running maximum jumps in the first tiles, then rests).
    flat:   q *= 0.02: every tile moves the running maximum by less than a percent - an accumulator that is not rescaled for small
            moves keeps stale weight here.
    ramp:   only channel 0 of q is set, k[j, 0] = j / 64, scale 1; q[i, 0] = +1, -1, +0.5, -0.5, ...: even rows raise the maximum on
            every tile, odd rows never after the first, so a wave holds both kinds.
    v and bias are random in all three; the batch items hold different data."""
    g = torch.Generator().manual_seed(1_000_003 * REGIMES.index(regime) + 4099 * C + L)
    q, k, v = (torch.randn(BATCH, L, C, generator=g) for _ in range(3))
    bias = 0.1 * torch.randn(C, generator=g)
    scale = C ** -0.5
    if regime == "random":
        q = q * 1.5
    elif regime == "flat":
        q = q * 0.02
    else:
        q = torch.zeros(BATCH, L, C)
        steps = torch.tensor([1.0, -1.0, 0.5, -0.5])
        for b in range(BATCH):
            q[b, :, 0] = steps.roll(-2 * b)[torch.arange(L) % 4]           # (item 1 starts at +0.5: other data, the same parities)
        k[:, :, 0] = torch.arange(L, dtype=torch.float32) / 64            # (exact in bf16 up to L = 257)
        scale = 1.0
    return Case(q, k, v, bias, scale, dt)


@functools.lru_cache(maxsize=None)
def regime_refs(regime, dt, C, L):
    """(ref64, the per-row errors of plain(dt) against it)"""
    c = regime_case(regime, dt, C, L)
    r = ref64(c)
    return r, row_errors(plain(c), r)


@functools.lru_cache(maxsize=None)
def regime_bounds(regime, dt, C):
    """(bound on the worst element, bound on the rel-L2) of one query row, and plain(dt)'s own worst values: over every length"""
    own = [regime_refs(regime, dt, C, L)[1] for L in lengths(C)]
    worst = max(float(e[0].max()) for e in own), max(float(e[1].max()) for e in own)
    return (MARGIN[dt] * worst[0], MARGIN[dt] * worst[1]), worst


# ---------------------------------------------------------------- exact cases -------------
def _sign_keys(g, B, L, C, twin=None):
    """L distinct rows of {-1, +1}^C per batch item (twin = (a, b): row b is then made a copy of row a, the only equal pair); and
    gap = C - the largest <k_i, k_j> over the pairs that are meant to differ"""
    while True:
        k = torch.randint(0, 2, (B, L, C), generator=g).float() * 2 - 1
        if twin:
            k[:, twin[1]] = k[:, twin[0]]
        dots = torch.einsum("bic,bjc->bij", k, k)
        dots.diagonal(dim1=1, dim2=2).fill_(-C)
        if twin:
            dots[:, twin[0], twin[1]] = -C
            dots[:, twin[1], twin[0]] = -C
        gap = C - int(dots.max()) if L > 1 else C
        if gap > 0:
            return k, gap


def _eighths(g, shape, lim, step=8):
    return torch.randint(-lim * step, lim * step + 1, shape, generator=g).float() / step


def _winner_scale(gap):
    """q = 8 k_winner: the winner's score is 8 C, every other at most 8 (C - gap); in the kernel's log2 domain the distance is
    scale * log2(e) * 8 gap = 200 binary orders"""
    return 200.0 / (8 * gap * math.log2(math.e))


def _assert_gap(c, winners):
    """float64, with the scale as the fp32 number the kernel is given: the winner(s) of every row hold its maximum and every other key
    lies at least MIN_GAP binary orders below"""
    s = torch.einsum("bic,bjc->bij", c.q.double(), c.k.double()) * float(torch.tensor(c.scale, dtype=torch.float32)) * math.log2(math.e)
    top = s.amax(-1, keepdim=True)
    lost = torch.ones_like(s, dtype=torch.bool)
    for w in winners:
        lost &= torch.arange(c.L)[None, None, :] != w[:, :, None]
        assert bool((s.gather(2, w[:, :, None]) == top).all())
    if lost.any():
        assert float((top - s)[lost].min()) >= MIN_GAP


def _one_hot_parts(g, B, L, C):
    """keys, their gap, the permutation (pi(0) = L - 1) and v of one one-hot problem"""
    k, gap = _sign_keys(g, B, L, C)
    pi = torch.stack([torch.randperm(L, generator=g) for _ in range(B)])
    for b in range(B):
        at = int((pi[b] == L - 1).nonzero())
        pi[b, at] = pi[b, 0]
        pi[b, 0] = L - 1
    return k, gap, pi, _eighths(g, (B, L, C), 4)


def _one_hot_finish(k, pi, v, bias, gap, dt):
    B = k.shape[0]
    c = Case(8 * torch.stack([k[b, pi[b]] for b in range(B)]), k, v, bias, _winner_scale(gap), dt)
    _assert_gap(c, [pi])
    want = torch.stack([v[b, pi[b]] for b in range(B)]) + bias
    assert torch.equal(want.to(dt).float(), want)                     # (the conversion is exact: no bit of the output may differ)
    return c, want.to(dt)


@functools.lru_cache(maxsize=None)
def one_hot_case(dt, C, L):
    """(case, expected, gap): q_i = 8 k_pi(i) for a seeded permutation with pi(0) = L - 1 (the LAST key, the sole valid one of a ragged
    tile at L = 33 / 129 / 161 / 257, wins a row of the first wave; every other key wins one row and loses all others); v in eighths
    within [-4, 4], bias in eighths within [-2, 2]: v[pi(i)] + bias is exact in every operand type.  The scores reach +-500 binary
    orders and the maximum of row 0 moves on the last tile."""
    g = torch.Generator().manual_seed(131 * C + L)
    k, gap, pi, v = _one_hot_parts(g, BATCH, L, C)
    return _one_hot_finish(k, pi, v, _eighths(g, (C,), 2), gap, dt) + (gap,)


TIE_L = 161
# (a, b): in one key tile (and in both lane halves of it); in tile 0 and the sole valid key of the ragged last tile; in tiles 1 and 4,
# which every split of the six tiles (S = 2: 0-2 | 3-5; S = 4: 0 | 1-2 | 3 | 4-5) puts in different ranges
TIE_PAIRS = {"one_tile": (5, 20), "first_and_ragged": (3, 160), "two_ranges": (40, 130)}


@functools.lru_cache(maxsize=None)
def tie_case(dt, C, place):
    """keys a != b are the same row; every fourth query chooses it (p = 1, 1, l = 2), the others choose a key of their own.  v in
    quarters, so (v_a + v_b) / 2 + bias is exact.  -> (case, expected)"""
    a, b = TIE_PAIRS[place]
    L = TIE_L
    g = torch.Generator().manual_seed(9_001 * C + 17 * a + b)
    k, gap = _sign_keys(g, BATCH, L, C, twin=(a, b))
    pi = torch.stack([torch.randperm(L, generator=g) for _ in range(BATCH)])
    pi[:, ::4] = a
    pi[:, L - 1] = b                                                  # (chosen through its other copy as well)
    q = 8 * torch.stack([k[i, pi[i]] for i in range(BATCH)])
    v, bias = _eighths(g, (BATCH, L, C), 4, step=4), _eighths(g, (C,), 2)
    c = Case(q, k, v, bias, _winner_scale(gap), dt)
    tied = (pi == a) | (pi == b)
    first, second = torch.where(tied, a, pi), torch.where(tied, b, pi)
    _assert_gap(c, [first, second])
    want = torch.stack([(v[i, first[i]] + v[i, second[i]]) / 2 for i in range(BATCH)]) + bias
    assert torch.equal(want.to(dt).float(), want)
    return c, want.to(dt)


@functools.lru_cache(maxsize=None)
def uniform_case(dt, C, L):
    """q = 0 (every weight is 1 / L), k random, no bias; v[j][c] = a_c + 64 s_j with a_c in {1, 2, 3} and s_j = +-1 balanced (one 0
    where L is odd): the sum over exactly the L valid keys is L a_c, and one key dropped, doubled or masked wrongly moves the result
    by 64 / L.  -> (case, a [C])"""
    g = torch.Generator().manual_seed(5_003 * C + L)
    k = torch.randn(BATCH, L, C, generator=g)
    a = torch.randint(1, 4, (C,), generator=g).float()
    s = torch.cat([torch.ones(L // 2), -torch.ones(L // 2), torch.zeros(L % 2)])
    s = torch.stack([s[torch.randperm(L, generator=g)] for _ in range(BATCH)])
    v = a[None, None, :] + 64 * s[:, :, None]
    return Case(torch.zeros(BATCH, L, C), k, v, None, C ** -0.5, dt), a


@functools.lru_cache(maxsize=None)
def group_cases(dt, C, kind):
    """the problems of GROUP_PROBLEMS, which share one bias and one scale, as (case, expected or None): kind = "random" (the random
    regime's data) or "one_hot" (the scale of the smallest gap among the problems: the others lie further apart still)"""
    if kind == "one_hot":
        g = torch.Generator().manual_seed(271 * C)
        parts = [_one_hot_parts(g, B, L, C) for B, L in GROUP_PROBLEMS]
        bias, gap = _eighths(g, (C,), 2), min(p[1] for p in parts)
        return [_one_hot_finish(k, pi, v, bias, gap, dt) for k, _, pi, v in parts]
    out, bias = [], regime_case("random", dt, C, GROUP_PROBLEMS[0][1]).bias
    for B, L in GROUP_PROBLEMS:
        c0 = regime_case("random", dt, C, L)
        rows = [i % BATCH for i in range(B)]                          # (B = 3: item 0 again, at another place in memory)
        out.append((Case(c0.q[rows], c0.k[rows], c0.v[rows], bias, C ** -0.5, dt), None))
    return out
