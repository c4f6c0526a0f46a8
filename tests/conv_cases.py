"""Case tables, seeded inputs and host references for tests/test_conv_edges.py (storm_conv: conv_igemm.hip, conv_pipe.hip, conv_pipe128.hip,
conv_duo.hip, conv_thin.hip, conv_narrow.hip and the shared conv_epilogue.h), per OUTPUT ELEMENT.

Exact cases.  Activations are integers in [-2, 2], weights are -1 / 0 / +1 and sparse, bias / temb bias / skip are small integers, the
output scale is 1 or 0.5 and the fused GroupNorm table holds scales of 1, 2, -1, 0.5 and integer shifts (no SiLU).  Every product and
every partial sum is then a multiple of the case's quantum (1, 1/2 or 1/4) far below 2^24 quanta, so fp32 accumulates it exactly in any
order - any K split, any ring schedule, any slice order - and the result is representable in the storage type: the kernel's output is
the float64 reference bit for bit, and the per-tile GroupNorm partials sum to the reference's (sum, sum of squares) exactly.  The
conditions are asserted in float64 WHEN THE CASE IS BUILT (build_exact), before any kernel has run.

Impulse cases.  One non-zero weight (+1) per output channel at (tap, cin), Gaussian activations already rounded to the type: output
channel co is input channel cin shifted by the tap with a zero border, bit for bit.

Measured cases.  Gaussian operands, with and without a fused GroupNorm + SiLU.  Two host references, neither mirroring a kernel's tiling:
  ref64   float64 of the operation on the values the kernel is given (16-bit activations / weights, the fp32 (scale, shift) table);
          SiLU(x scale + shift) is NOT rounded;
  plain   the float32 restatement of what the kernels do: affine and SiLU in fp32, the activation rounded to the operand type, fp32
          F.conv2d, the fp32 epilogue, rounding to the storage type.
A kernel's worst pixel / worst channel / worst element (errors against ref64 over the RMS of ref64) must lie within MARGIN x plain's own
figure of the same setting: 2 for the 16-bit types, 4 for fp32, as in tests/attention_cases.py."""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

DT16 = (torch.bfloat16, torch.float16)
DT_ALL = DT16 + (torch.float32,)
MARGIN = {torch.bfloat16: 2.0, torch.float16: 2.0, torch.float32: 4.0}
# the constants the edges sit on
TILE_H, TILE_W = 8, 32                   # conv_index.h: the output tile of every kernel but the two below, and of the GroupNorm partials
PIPE128_TH = 16                          # conv_pipe128.hip: pipe128::TH (two partial tiles per workgroup tile)
NARROW_TH = 20                           # conv_narrow.hip: narrow::TH
KC64, KC32 = 64, 32                      # channels per K chunk: conv_pipe.hip KC (and conv_igemm.hip's 8 x PER16 for 16 bits) / pipe128::KC, duo::KC
LIMIT = 2.0 ** 24


def dt_id(dt):
    return {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dt]


def round_up(x, m):
    return (x + m - 1) // m * m


class Spec(NamedTuple):
    """one storm_conv call: a `taps`-tap convolution over cat[xa (Ca), xb (Cb)] (gn: a fused (scale, shift) table on it), optionally a fused
    1x1 shortcut over cat[sa (Sa), sb (Sb)], then (+ bias + tbias[b] + skip) * scale.  why: the constant the shape sits on."""
    B: int
    H: int
    W: int
    Cout: int
    Ca: int
    Cb: int = 0
    taps: int = 9
    Sa: int = 0
    Sb: int = 0
    gn: bool = False
    bias: bool = True
    tbias: bool = False
    skip: bool = False
    scale: float = 1.0
    out_f32: bool = False
    why: str = ""

    @property
    def outC(self):
        return round_up(self.Cout, 8)

    @property
    def tiles(self):
        """8 x 32-pixel tiles of the call (the unit a persistent workgroup walks)"""
        return self.B * -(-self.H // TILE_H) * -(-self.W // TILE_W)


# ---------------------------------------------------------------- shape tables ------------
IMAGE_H = (1, 2, 7, 8, 9, 15, 16, 17, 19, 20, 21)      # around TILE_H = 8, PIPE128_TH = 16, NARROW_TH = 20; 1 / 2 / 7: the 4 x 2 and 2 x 4 wave rows of write_stats
IMAGE_W = (1, 31, 32, 33, 63, 65)                      # around TILE_W = 32
CHANNELS_K = (8, 24, 32, 40, 56, 64, 72, 128, 136)     # around a chunk of 64 (32 for conv_pipe128 / conv_duo): one below / at / one octet above


def image_specs(Cout, Ca, taps=9, **kw):
    """H swept at a ragged width of two tile columns, W swept at a ragged height of two tile rows; every third case has two batch
    items, H = 17 has three (three tile rows: 18 tiles, a persistent walk across batch items)"""
    nb = lambda i, H=0: 3 if H == 17 else 2 if i % 3 == 1 else 1  # noqa: E731
    out = [Spec(nb(i, H), H, 33, Cout, Ca, taps=taps, why=f"H = {H} (tile rows of 8 / 16 / 20)", **kw) for i, H in enumerate(IMAGE_H)]
    out += [Spec(nb(i), 9, W, Cout, Ca, taps=taps, why=f"W = {W} (TILE_W = 32)", **kw) for i, W in enumerate(IMAGE_W)]
    return out


FLAT_IMAGES = ((1, 1), (1, 33), (7, 33), (8, 32), (9, 33), (16, 32), (17, 65))     # H W around the 256 flat pixels of a one-tap tile


def flat_specs(Cout, Ca, **kw):
    """one-tap convolutions of conv_igemm.hip tile the image as H W flat pixels (storm_conv_tiles): 1, 33, 231, 256, 297, 512, 1105"""
    return [Spec(1 + i % 3, H, W, Cout, Ca, taps=1, why=f"H W = {H * W} (flat tiles of 256 pixels)", **kw) for i, (H, W) in enumerate(FLAT_IMAGES)]


def k_specs(Cout, taps=9, **kw):
    return [Spec(1, 9, 33, Cout, C, taps=taps, why=f"K = {C} (chunk of 64 / 32)", **kw) for C in CHANNELS_K]


def cout_specs(couts, Ca=24, taps=9, **kw):
    return [Spec(2, 9, 33, Co, Ca, taps=taps, why=f"Cout = {Co} (octet / wave of 64 / tile of 128, 256)", **kw) for Co in couts]


def epilogue_specs(Cin_tile, Co_ragged, Ca=40, taps=9, shortcut=True):
    """Cin_tile: a Cout that fills whole workgroup tiles (with 16 x 64 pixels: every tile takes the interior fast path of store_tile);
    Co_ragged: one that does not and is no multiple of 8 either (the general path; bias / temb bias of the last octet element by element,
    pad channels beside valid ones in one 16-byte store)"""
    out = []
    for B, Co, H, W, path in ((2, Cin_tile, 16, 64, "interior fast path"), (1, Co_ragged, 17, 65, "general path"), (2, Cin_tile, 17, 65, "both paths in one call")):
        for skip in (False, True):
            out.append(Spec(B, H, W, Co, Ca, taps=taps, skip=skip, scale=0.5 if skip else 1.0, why=f"epilogue: {path}, skip = {skip}"))
    out += [Spec(2, 9, 33, Co_ragged, Ca, taps=taps, bias=False, why="epilogue: no bias"),
            Spec(2, 9, 33, Co_ragged, Ca, taps=taps, bias=False, tbias=True, why="epilogue: temb bias alone (offset into a wider table)"),
            Spec(3, 9, 33, Co_ragged, Ca, taps=taps, tbias=True, skip=True, scale=0.5, why="epilogue: bias + temb bias + skip, scale 0.5"),
            Spec(2, 9, 33, Co_ragged, Ca, taps=taps, out_f32=True, why="epilogue: fp32 output"),
            Spec(1, 16, 64, Cin_tile, Ca, taps=taps, out_f32=True, skip=True, why="epilogue: fp32 output of whole tiles (never the fast path)")]
    if shortcut:
        out.append(Spec(2, 9, 33, Co_ragged, Ca, taps=taps, Sa=24, tbias=True, scale=0.5, why="epilogue: block tail (fused shortcut, bias, temb bias)"))
    return out


def concat_specs(Cout, kc, taps=9, gn=True):
    """the K edges beyond one operand: concat splits inside a chunk and on a chunk boundary, a fused shortcut over a concat, the fused
    affine over a concat, and the deep_k shape (tests/test_ops.py): more chunks than ring slots, the last chunk of every run ragged"""
    out = [Spec(2, 9, 33, Cout, kc + 8, kc - 16, taps=taps, why="concat: the split falls inside a chunk"),
           Spec(2, 9, 33, Cout, kc, 24, taps=taps, why="concat: the split falls on a chunk boundary"),
           Spec(2, 9, 33, Cout, 40, 0, taps=taps, Sa=kc + 8, Sb=24, why="fused 1x1 shortcut over a concat"),
           Spec(1, 9, 33, Cout, 136, 88, taps=taps, Sa=136, Sb=72, scale=0.5, why="deep_k: every ring slot wraps, ragged last chunk of each run")]
    if gn:
        out += [Spec(2, 9, 33, Cout, 72, 56, taps=taps, gn=True, why="fused affine over a concat (ragged last chunks)"),
                Spec(1, 10, 36, Cout, 136, 88, taps=taps, gn=True, Sa=136, Sb=72, why="deep_k with the fused affine")]
    return out


def tiled_family(couts, tile_cout, ragged_cout, kc, gn=True):
    return (image_specs(ragged_cout, 24) + k_specs(ragged_cout) + cout_specs(couts) + epilogue_specs(tile_cout, ragged_cout)
            + concat_specs(ragged_cout, kc, gn=gn) + [Spec(2, 9, 33, ragged_cout, 72, gn=True, why="fused affine, one operand")])


class Family(NamedTuple):
    switches: tuple        # ((name, value), ...) set before the call
    name: str              # the kernel name the call must resolve to, with {T} for the operand type and {taps}
    dtypes: tuple
    specs: tuple
    backends: tuple = ("sim", "hip")


_T = {torch.bfloat16: "storm::bf16_t", torch.float16: "storm::half_t", torch.float32: "float"}


def kernel_name(fam, dt, spec, silu=False):
    """the name storm_conv_kernel_name must give for a case of the family (silu: a fused GroupNorm table WITH SiLU is attached)"""
    any9 = spec.taps == 9
    return FAMILIES[fam].name.format(T=_T[dt], taps=9 if any9 else 1, dma="true" if any9 else "false", cg=spec.Ca // 64,
                                     silu="true" if silu and spec.gn else "false")


def _narrow_specs():
    out = []
    for i, H in enumerate(IMAGE_H):
        out.append(Spec(1 + i % 3, H, 33, 1 + i % 4, 128, gn=i % 2 == 0, why=f"H = {H} (narrow::TH = 20)"))
    for i, W in enumerate(IMAGE_W):
        out.append(Spec(1 + i % 3, 21, W, 4 - i % 4, 256 if i % 2 else 128, gn=i % 2 == 1, why=f"W = {W} (narrow::TW = 32)"))
    for Co in (1, 2, 3, 4):
        for C in (128, 256):
            for gn in (False, True):
                out.append(Spec(2, 9, 33, Co, C, gn=gn, bias=Co != 2, why=f"Cout = {Co} of 4 planes, Cin = {C}"))
    return out


def _thin_specs(taps):
    out = image_specs(69, 8, taps=taps) + cout_specs((64, 69, 128, 133, 256, 261), Ca=8, taps=taps)
    for Co, H, W in ((128, 16, 64), (69, 17, 65)):
        for skip in (False, True):
            out.append(Spec(2, H, W, Co, 8, taps=taps, skip=skip, scale=0.5 if skip else 1.0, why=f"epilogue: whole / ragged tiles, skip = {skip}"))
    out.append(Spec(2, 9, 33, 69, 8, taps=taps, bias=False, why="epilogue: no bias"))
    return out


def _small_specs():
    out = image_specs(21, 24) + k_specs(8)
    for Co in (1, 2, 3, 4, 8, 12, 24, 32):
        out.append(Spec(2, 9, 33, Co, 40, why=f"Cout = {Co} (outC <= 32: the 32-cout tile)"))
    out += [Spec(2, 9, 33, 24, 40, 24, skip=True, tbias=True, scale=0.5, why="epilogue: bias + temb bias + skip over a concat"),
            Spec(2, 9, 33, 24, 72, 56, gn=True, why="fused affine over a concat"),
            Spec(2, 9, 33, 12, 40, out_f32=True, why="fp32 output"),
            Spec(2, 17, 65, 32, 40, taps=1, skip=True, why="one tap, flat pixel tiles"),
            Spec(1, 9, 33, 24, 40, Sa=72, Sb=24, why="fused shortcut over a concat")]
    return out


def _one_tap_specs(couts, ragged):
    return (flat_specs(ragged, 24) + k_specs(ragged, taps=1) + cout_specs(couts, taps=1)
            + epilogue_specs(couts[-2], ragged, taps=1, shortcut=False)
            + [Spec(2, 9, 33, ragged, 72, 24, taps=1, why="concat: the split falls inside a chunk"),
               Spec(2, 9, 33, ragged, 64, 24, taps=1, why="concat: the split falls on a chunk boundary"),
               Spec(1, 9, 33, ragged, 136, 88, taps=1, scale=0.5, why="many chunks, ragged last chunk of each operand")])


def _n9(s):
    """nine-tap chunks of 64 channels: conv_splitk_slices splits them into at most that many slices"""
    return -(-s.Ca // KC64) + (-(-s.Cb // KC64) if s.Cb else 0)


def _split_specs(S):
    """the cases S slices apply to; S = 3 (never the dispatcher's own choice) leaves the image sweep to S = 2 and 4"""
    return tuple(s for s in _SPLIT if _n9(s) >= S and not (S == 3 and s.why[:3] in ("H =", "W =")))


_SPLIT = [Spec(1 + i % 2, H, 33, 133, 200, tbias=True, why=f"H = {H}") for i, H in enumerate((1, 7, 8, 9, 17))] + \
         [Spec(2, 9, 33, 136, 136, why="three chunks, the last ragged: slices of 1 and 2 chunks (S = 2), of 1 each (S = 3)"),
          Spec(1, 9, 33, 136, 72, tbias=True, why="two chunks, the last ragged (S = 2 only)")] + \
         [Spec(1 + i % 2, 9, W, 261, 128, 72, why=f"W = {W}") for i, W in enumerate((1, 31, 32, 33, 65))] + \
         [Spec(2, 9, 33, Co, 200, why=f"Cout = {Co} (cout tiles of 128: the last one ragged)") for Co in (133, 136, 256, 261)] + \
         [Spec(2, 9, 33, 133, 136, 88, skip=True, tbias=True, scale=0.5, why="slices of unequal length over a concat; skip, temb bias"),
          Spec(2, 16, 64, 256, 256, skip=True, why="whole tiles, whole cout tiles"),
          Spec(3, 9, 65, 136, 200, skip=True, why="18 pixel tiles: a persistent walk over (tile, cout tile, slice)"),
          Spec(1, 9, 33, 261, 136, 88, Sa=136, Sb=72, scale=0.5, why="deep_k: the one-tap chunks ride with the last slice"),
          Spec(1, 10, 36, 264, 136, 88, gn=True, Sa=136, Sb=72, why="deep_k with the fused affine"),
          Spec(2, 9, 33, 136, 200, 56, gn=True, why="fused affine over a concat")]

FAMILIES = {
    # conv_igemm.hip: variant 0 = 128 couts x 8 x 32 pixels, 4 waves; 2 = 256 couts, 8 waves; 7 = 64 couts; outC <= 32 = the 32-cout tile
    "igemm0": Family((("STORM_CONV_VARIANT", 0),), "storm::conv_igemm_kernel<{T}, {taps}, 2, 2, 2, false, {dma}, 0>", DT_ALL,
                     tuple(tiled_family((37, 64, 72, 128, 133, 264), 128, 69, KC64))),
    "igemm0_1x1": Family((("STORM_CONV_VARIANT", 0),), "storm::conv_igemm_kernel<{T}, {taps}, 2, 2, 2, false, {dma}, 0>", DT_ALL,
                         tuple(_one_tap_specs((37, 64, 72, 128, 133), 69))),
    "igemm2": Family((("STORM_CONV_VARIANT", 2),), "storm::conv_igemm_kernel<{T}, {taps}, 2, 4, 2, true, false, 0>", DT_ALL,
                     tuple(tiled_family((37, 136, 256, 261), 256, 133, KC64))),
    "igemm2_1x1": Family((("STORM_CONV_VARIANT", 2),), "storm::conv_igemm_kernel<{T}, {taps}, 2, 4, 2, true, false, 0>", DT_ALL,
                         tuple(_one_tap_specs((37, 136, 256, 261), 133))),
    "igemm7": Family((("STORM_CONV_VARIANT", 7),), "storm::conv_igemm_kernel<{T}, 9, 1, 2, 2, false, true, 0>", DT_ALL,
                     tuple(tiled_family((37, 64, 72, 128, 133), 64, 69, KC64))),
    "igemm_small": Family((), "storm::conv_igemm_kernel<{T}, {taps}, 1, 1, 4, false, false, 0>", DT_ALL, tuple(_small_specs())),
    # conv_pipe.hip: 256- and 128-cout tiles, 64-channel chunks; split-K over the nine-tap chunks
    "pipe256": Family((("STORM_CONV_VARIANT", 3),), "storm::conv_pipe_kernel<{T}, 256, 8, 0>", DT16,
                      tuple(tiled_family((37, 136, 256, 261), 256, 133, KC64))),
    "pipe_half": Family((("STORM_CONV_VARIANT", 9),), "storm::conv_pipe_kernel<{T}, 128, 8, 0>", DT16,
                        tuple(tiled_family((37, 72, 128, 133, 264), 128, 69, KC64))),
    "splitk2": Family((("STORM_SPLITK", 2),), "storm::conv_pipe_splitk_kernel<{T}, 128, 8>", DT16, _split_specs(2)),
    "splitk3": Family((("STORM_SPLITK", 3),), "storm::conv_pipe_splitk_kernel<{T}, 128, 8>", DT16, _split_specs(3)),
    "splitk4": Family((("STORM_SPLITK", 4),), "storm::conv_pipe_splitk_kernel<{T}, 128, 8>", DT16, _split_specs(4)),
    # <= 128 couts, 32-channel chunks: conv_pipe128.hip (16-row tiles), conv_duo.hip (the simulation and the profiling library only)
    "pipe128": Family((("STORM_CONV_VARIANT", 4),), "storm::conv_pipe128_kernel<{T}, 0>", DT16,
                      tuple(tiled_family((37, 64, 72, 125, 128), 128, 69, KC32))),
    "duo": Family((("STORM_CONV_VARIANT", 5),), "storm::conv_duo_kernel<{T}, 0>", DT16,
                  tuple(tiled_family((37, 64, 72, 125, 128), 128, 69, KC32)), backends=("sim",)),
    # conv_thin.hip: 8 input channels, nine taps / one tap; conv_narrow.hip: 128 / 256 -> 1 .. 4 planes, 20-row tiles
    "thin9": Family((("STORM_CONV_VARIANT", 6),), "storm::conv_thin_kernel<{T}, 9>", DT16, tuple(_thin_specs(9))),
    "thin1": Family((("STORM_CONV_VARIANT", 6),), "storm::conv_thin_kernel<{T}, 1>", DT16, tuple(_thin_specs(1))),
    "narrow": Family((("STORM_CONV_VARIANT", 8),), "storm::conv_narrow_kernel<{T}, {cg}, {silu}>", DT16, tuple(_narrow_specs())),
}
NO_PARTIALS = ("narrow",)                # conv_narrow_supports: no GroupNorm partials (its output feeds no GroupNorm)
WALK = {
    # family: (rows of a workgroup tile, couts of a workgroup tile, K slices, chunk, workgroups per CU) - the launch code of each kernel
    "pipe256": (TILE_H, 256, 1, KC64, 1), "pipe_half": (TILE_H, 128, 1, KC64, 1), "pipe128": (PIPE128_TH, 128, 1, KC32, 1),
    "duo": (TILE_H, 128, 1, KC32, 2), "splitk2": (TILE_H, 128, 2, KC64, 1), "splitk3": (TILE_H, 128, 3, KC64, 1),
    "splitk4": (TILE_H, 128, 4, KC64, 1),
}


def walk_cus(fam):
    """STORM_CONV_CUS values worth a run of their own.  conv_pipe.hip (both tiles, split-K), conv_pipe128.hip and conv_duo.hip launch
    (cus + 7) / 8 * 8 workgroups per CU slot, so 3 pretend CUs are the 8 of the other run: only conv_narrow.hip (min(tiles, cus)
    workgroups) sees the 3.  conv_igemm.hip and conv_thin.hip launch one workgroup per tile, placed by the hardware (the persistent
    walk of conv_igemm.hip exists in the profiling build only): the switch changes nothing there, and they have no walk run"""
    return (8, 3) if fam == "narrow" else (8,) if fam in WALK else ()


def walks(fam, s, cus):
    """does a workgroup of this call store more than one tile with `cus` pretend CUs: virtual blocks (8 x ceil(tiles / 8) x cout tiles
    x slices) against resident workgroups, as the launch code computes them"""
    if fam == "narrow":
        return s.B * -(-s.H // NARROW_TH) * -(-s.W // TILE_W) > cus
    th, bn, S, _, per_cu = WALK[fam]
    tiles = s.B * -(-s.H // th) * -(-s.W // TILE_W)
    return 8 * -(-tiles // 8) * -(-s.outC // bn) * S > per_cu * round_up(cus, 8)


def walk_extra(fam):
    """multi-tile variants of the K edges, 3 images of 17 x 33 pixels (18 tiles of 8 rows, 12 of 16 rows: every workgroup stores several
    tiles and crosses batch items), so that the hand-over of the ring and of the patch-buffer parity to the NEXT tile runs with a
    second operand, the fused affine, one-tap shortcut chunks and the deep_k shape - with even and with odd chunk counts (the chunks
    of each run, at 64 / 32 channels, beside each case)"""
    if fam not in WALK:
        return []
    kc = WALK[fam][3]
    co = 133 if fam != "pipe128" and fam != "duo" else 69
    B, H, W = 3, 17, 33
    out = [Spec(B, H, W, co, kc + 8, kc - 16, why="walk: concat split inside a chunk (2 + 1 chunks: odd)"),
           Spec(B, H, W, co, kc, kc, skip=True, why="walk: concat split on a chunk boundary (1 + 1 chunks: even), skip"),
           Spec(B, H, W, co, 128, gn=True, why="walk: fused affine, one operand (2 / 4 chunks: even)"),
           Spec(B, H, W, co, 72, 56, gn=True, tbias=True, why="walk: fused affine over a concat (2 + 1 / 3 + 2 chunks: odd)"),
           Spec(B, H, W, co, 40, Sa=kc + 8, Sb=24, tbias=True, scale=0.5, why="walk: block tail, shortcut over a concat (1 + 2 + 1 / 2 + 2 + 1 chunks)"),
           Spec(B, H, W, co, 136, 88, gn=True, Sa=136, Sb=72, why="walk: deep_k with the fused affine (10 / 16 chunks: even)"),
           Spec(B, H, W, co, 136, 88, Sa=72, scale=0.5, why="walk: deep_k, one shortcut operand (7 / 11 chunks: odd)")]
    if fam.startswith("splitk"):
        out = [s for s in out if _n9(s) >= WALK[fam][2]]
    return out


def specs_of(fam, dt):
    """the family's table for a type (the same for every type the family has)"""
    return FAMILIES[fam].specs


def walk_specs(fam, cus=8):
    """the cases of a family's table in which a workgroup stores several tiles with `cus` pretend CUs, and the multi-tile K edges"""
    if not walk_cus(fam):
        return []
    return [s for s in tuple(FAMILIES[fam].specs) + tuple(walk_extra(fam)) if walks(fam, s, cus)]


# ---------------------------------------------------------------- exact cases -------------
class Case:
    """host tensors of one call (activations NHWC in the operand type, weights fp32 [Cout, Cin, k, k]) and its float64 reference"""
    spec = dt = xa = xb = w = sa = sb = w2 = gn_scale = gn_shift = bias = tb = skip = ref = None


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def _sparse(g, shape, density):
    return _ints(g, shape, 1) * (torch.rand(shape, generator=g) < density).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def reference64(c):
    """float64: conv(affine(cat[xa, xb])) + conv1x1(cat[sa, sb]) + bias + tbias + skip, times scale -> [B, H, W, Cout]; and the largest
    sum of |terms| of one output (the bound on every partial sum, in whatever order)"""
    s = c.spec
    x = torch.cat([t.double() for t in (c.xa, c.xb) if t is not None], -1).permute(0, 3, 1, 2)
    if c.gn_scale is not None:
        x = x * c.gn_scale.double()[:, :, None, None] + c.gn_shift.double()[:, :, None, None]
        if c.gn_silu:
            x = x * torch.sigmoid(x)
    out = F.conv2d(x, c.w.double(), padding=s.taps // 9)
    mag = F.conv2d(x.abs(), c.w.double().abs(), padding=s.taps // 9)
    if c.w2 is not None:
        sc = torch.cat([t.double() for t in (c.sa, c.sb) if t is not None], -1).permute(0, 3, 1, 2)
        out = out + F.conv2d(sc, c.w2.double())
        mag = mag + F.conv2d(sc.abs(), c.w2.double().abs())
    if c.bias is not None:
        out = out + c.bias.double()[None, :, None, None]
        mag = mag + c.bias.double().abs()[None, :, None, None]
    if c.tb is not None:
        out = out + c.tb.double()[:, 8:8 + s.Cout, None, None]
        mag = mag + c.tb.double().abs()[:, 8:8 + s.Cout, None, None]
    if c.skip is not None:
        out = out + c.skip.double()[..., :s.Cout].permute(0, 3, 1, 2)
        mag = mag + c.skip.double().abs()[..., :s.Cout].permute(0, 3, 1, 2)
    return nhwc(out * s.scale), float(mag.max())


def _quantum(t):
    for q in (1.0, 0.5, 0.25, 0.125):
        if bool((t / q == (t / q).round()).all()):
            return q
    raise AssertionError("the case is finer than eighths")


def _build_exact(spec, dt, density_scale):
    g = torch.Generator().manual_seed(hash(tuple(spec[:15])) % (2 ** 31))
    s, c = spec, Case()
    c.spec, c.dt, c.gn_silu = s, dt, False
    cin, sc = s.Ca + s.Cb, s.Sa + s.Sb
    x = _ints(g, (s.B, s.H, s.W, cin), 2)
    c.xa, c.xb = x[..., :s.Ca].to(dt).contiguous(), (x[..., s.Ca:].to(dt).contiguous() if s.Cb else None)
    # about 15 % (nine taps) / 30 % (one tap) non-zero, thinned for a long K so that an output sums about 24 terms: every (tap, cin)
    # still meets a non-zero weight in some cout, and the sums stay far inside the storage type
    base = 0.15 if s.taps == 9 else 0.30
    c.w = _sparse(g, (s.Cout, cin, 3 if s.taps == 9 else 1, 3 if s.taps == 9 else 1), min(base, 24.0 / (s.taps * cin)) * density_scale).float()
    if sc:
        xs = _ints(g, (s.B, s.H, s.W, sc), 2)
        c.sa, c.sb = xs[..., :s.Sa].to(dt).contiguous(), (xs[..., s.Sa:].to(dt).contiguous() if s.Sb else None)
        c.w2 = _sparse(g, (s.Cout, sc, 1, 1), min(0.30, 12.0 / sc) * density_scale).float()
    if s.gn:
        pick = torch.randint(0, 4, (s.B, cin), generator=g)
        c.gn_scale = torch.tensor([1.0, 2.0, -1.0, 0.5])[pick]
        c.gn_shift = _ints(g, (s.B, cin), 2).float()
    if s.bias:
        c.bias = _ints(g, (s.Cout,), 3).float()
    if s.tbias:
        # (the call reads columns 8 .. 8 + Cout: an offset into a wider table.  Rows and offset are multiples of 4 floats, as every temb
        #  table of the networks is: the kernels read a row 16 bytes at a time)
        c.tb = _ints(g, (s.B, s.outC + 16), 3).float()
    if s.skip:
        sk = torch.zeros(s.B, s.H, s.W, s.outC, dtype=torch.float64)
        sk[..., :s.Cout] = _ints(g, (s.B, s.H, s.W, s.Cout), 4)  # (pad channels zero, as in every activation the library writes)
        c.skip = sk.to(dt)
    c.ref, c.mag = reference64(c)
    return c


def _exact_ok(c):
    """the two conditions of the module docstring, in float64 -> None, or what is violated"""
    s, store = c.spec, (torch.float32 if c.spec.out_f32 else c.dt)
    q = _quantum(c.ref)
    if not c.mag / min(q, 0.5 if s.gn else 1.0, s.scale) < LIMIT:
        return "a partial sum may leave fp32's exact range"
    top = float(c.ref.abs().max())
    if top > {torch.bfloat16: 256.0, torch.float16: 2048.0, torch.float32: LIMIT}[store] or not torch.equal(c.ref.to(store).double(), c.ref):
        return "an output is not representable in the storage type"
    if not s.H * s.W * top * top / (q * q) < LIMIT:
        return "a sum of squares may leave fp32's exact range"
    return None


@functools.lru_cache(maxsize=64)
def build_exact(spec, dt):
    """the exact case of a spec: the weights are thinned (halved at most three times) until the conditions hold, then they are ASSERTED"""
    for shrink in (1.0, 0.5, 0.25, 0.125):
        c = _build_exact(spec, dt, shrink)
        if _exact_ok(c) is None:
            break
    why = _exact_ok(c)
    assert why is None, (spec, why)
    assert int((c.w != 0).sum()) > 0
    # what the partials must sum to, per (image, channel): integers of quanta, exact in float64
    c.sums = torch.stack([c.ref.sum((1, 2)), (c.ref * c.ref).sum((1, 2))], -1)
    return c


# ---------------------------------------------------------------- impulse cases -----------
def impulse_positions(spec, kc):
    """the input channels an impulse is placed at: in the first chunk, in the ragged last chunk of xa, in the second operand"""
    pos = [("first chunk", min(5, spec.Ca - 1))]
    if spec.Ca > kc:
        pos.append(("last chunk of xa", spec.Ca - 3))
    if spec.Cb:
        pos.append(("second operand", spec.Ca + spec.Cb - 2))
    return pos


def impulse_spec(fam):
    """the impulse call of a family: ragged rows, columns and couts; a concat whose operands both end in a ragged chunk"""
    if fam == "narrow":
        return Spec(2, 9, 33, 4, 128, bias=False), KC64
    if fam.startswith("thin"):
        return Spec(2, 9, 33, 69, 8, taps=9 if fam == "thin9" else 1, bias=False), KC64
    if fam.startswith("splitk"):
        return Spec(2, 9, 33, 133, 200, 72, bias=False), KC64
    taps = 1 if fam.endswith("_1x1") else 9
    if fam == "igemm_small":
        return Spec(2, 9, 33, 27, 72, 24, bias=False), KC64
    co = 133 if fam in ("igemm2", "igemm2_1x1", "pipe256") else 37
    return Spec(2, 9, 33, co, 72, 24, taps=taps, bias=False), (KC32 if fam in ("pipe128", "duo") else KC64)


@functools.lru_cache(maxsize=16)
def build_impulses(fam, dt):
    """-> [(case, [(cout, tap, cin, where)])]: every output channel listed has ONE weight of +1; Gaussian activations rounded to dt.
    The reference is a shifted copy of the input channel (zero border); all other couts are zero."""
    spec, kc = impulse_spec(fam)
    g = torch.Generator().manual_seed(4242 + spec.Ca)
    cin = spec.Ca + spec.Cb
    x = torch.randn(spec.B, spec.H, spec.W, cin, generator=g).to(dt)
    todo = [(tap, ci, where) for where, ci in impulse_positions(spec, kc) for tap in range(spec.taps)]
    # the couts used end on the LAST valid cout (inside the ragged octet)
    per_call = min(spec.Cout, len(todo))
    out = []
    for i in range(0, len(todo), per_call):
        chunk = todo[i:i + per_call]
        c = Case()
        c.spec, c.dt, c.gn_silu = spec, dt, False
        c.xa, c.xb = x[..., :spec.Ca].contiguous(), (x[..., spec.Ca:].contiguous() if spec.Cb else None)
        k = 3 if spec.taps == 9 else 1
        c.w = torch.zeros(spec.Cout, cin, k, k)
        c.ref = torch.zeros(spec.B, spec.H, spec.W, spec.Cout, dtype=torch.float64)
        placed = []
        for j, (tap, ci, where) in enumerate(chunk):
            co = spec.Cout - len(chunk) + j
            ky, kx = (tap // 3, tap % 3) if spec.taps == 9 else (0, 0)
            c.w[co, ci, ky, kx] = 1.0
            dy, dx = (ky - 1, kx - 1) if spec.taps == 9 else (0, 0)     # out[y, x] = in[y + dy, x + dx], zero outside the image
            ys, xs = slice(max(0, -dy), spec.H - max(0, dy)), slice(max(0, -dx), spec.W - max(0, dx))
            yt, xt = slice(max(0, dy), spec.H - max(0, -dy)), slice(max(0, dx), spec.W - max(0, -dx))
            c.ref[:, ys, xs, co] = x[:, yt, xt, ci].double()
            placed.append((co, tap, ci, where))
        out.append((c, placed))
    return out


# ---------------------------------------------------------------- measured cases ----------
def measured_spec(fam, gn):
    """one edge shape per family: ragged H and W (two tile rows, two tile columns), a concat, at least two chunks, a ragged cout octet"""
    if fam == "narrow":
        return Spec(2, 21, 33, 3, 128, gn=gn)
    if fam.startswith("thin"):
        return None if gn else Spec(2, 9, 33, 69, 8, taps=9 if fam == "thin9" else 1)    # (conv_thin_supports: no fused affine)
    if fam.startswith("splitk"):
        return Spec(2, 9, 33, 133, 200, 72, gn=gn)
    taps = 1 if fam.endswith("_1x1") else 9
    if fam == "igemm_small":
        return Spec(2, 9, 33, 21, 72, 24, gn=gn)
    co = 133 if fam in ("igemm2", "igemm2_1x1", "pipe256") else 37
    return Spec(2, 17 if fam == "pipe128" else 9, 33, co, 72, 24, taps=taps, gn=gn)


@functools.lru_cache(maxsize=32)
def build_measured(spec, dt):
    """Gaussian operands rounded to dt, a Gaussian fp32 bias, with spec.gn a (scale, shift) table around (1, 0) and SiLU -> the case
    with .ref (float64) and .own = the float32 restatement's figures"""
    g = torch.Generator().manual_seed(977 + spec.Ca + 13 * spec.Cout + spec.taps)
    c = Case()
    c.spec, c.dt, c.gn_silu = spec, dt, True
    cin = spec.Ca + spec.Cb
    x = torch.randn(spec.B, spec.H, spec.W, cin, generator=g).to(dt)
    c.xa, c.xb = x[..., :spec.Ca].contiguous(), (x[..., spec.Ca:].contiguous() if spec.Cb else None)
    k = 3 if spec.taps == 9 else 1
    c.w = (torch.randn(spec.Cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5).to(dt).float()
    c.bias = torch.randn(spec.Cout, generator=g)
    if spec.gn:
        c.gn_scale = 1 + 0.1 * torch.randn(spec.B, cin, generator=g)
        c.gn_shift = 0.1 * torch.randn(spec.B, cin, generator=g)
    c.ref, _ = reference64(c)
    c.own = figures(plain(c), c.ref)
    return c


def plain(c):
    """the float32 restatement of a measured case -> [B, H, W, Cout] in the storage type"""
    x = torch.cat([t.float() for t in (c.xa, c.xb) if t is not None], -1).permute(0, 3, 1, 2)
    if c.gn_scale is not None:
        x = x * c.gn_scale[:, :, None, None] + c.gn_shift[:, :, None, None]
        x = (x * torch.sigmoid(x)).to(c.dt).float()
    out = F.conv2d(x, c.w, padding=c.spec.taps // 9) + c.bias[None, :, None, None]
    return nhwc(out * torch.tensor(c.spec.scale)).to(c.dt)


def figures(out, ref):
    """(worst pixel: RMS of the error over its couts, worst channel: RMS over its pixels, worst element), each over the RMS of ref"""
    d = out.double() - ref
    rms = float(ref.pow(2).mean().sqrt())
    return (float(d.pow(2).mean(-1).sqrt().max()) / rms, float(d.pow(2).mean((1, 2)).sqrt().max()) / rms, float(d.abs().max()) / rms)
