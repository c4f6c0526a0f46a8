// The slots of a storm_op (include/storm_hip.h), by op code: which reference of p[], integer of i[] and float of f[] means what.
// The planner (ncsnpp_graph.hip) writes an op through these names, the interpreter and the grouped evaluation (program.hip) read it
// through them; the numbers are the record's layout as callers outside the library read it (tests/py_planner.py restates them
// independently and is compared with the planner bit for bit), so none may change without STORM_ABI_VERSION.
// One namespace per op code: an enum each for p, i and f, closed by the number of slots in use (N_P, N_I, N_F).
#pragma once
#include "../../include/storm_hip.h"

namespace storm {
namespace opf {

namespace op_memset {      // STORM_OP_MEMSET: hipMemsetAsync(DST, 0, BYTES)
enum { DST, N_P };
enum { BYTES, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_pack {        // STORM_OP_PACK_INPUT (storm_pack_input): up to three complex inputs IN0, IN0 + 1, IN0 + 2
enum { IN0, OUT = 3, N_P };
enum { N_IN, B, F, T, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_temb {        // STORM_OP_TEMB (storm_time_embedding)
enum { TIME, GFP_W, W1, B1, W2, B2, OUT, N_P };
enum { B, NF, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_dense {       // STORM_OP_DENSE (storm_dense)
enum { X, W, BIAS, OUT, N_P };
enum { B, N, K, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_conv {        // STORM_OP_CONV (storm_conv): up to two K segments; segment g's pointers and integers through pseg / iseg
enum { SRC_A0, SRC_B0, W0, SRC_A1, SRC_B1, W1, OUT, BIAS, TBIAS, SKIP, GN_PART, GN_SS, SPLITK_WS, N_P };
enum { NSEG, B, H, W, OUTC, COUT, TBIAS_STRIDE, OUT_F32, SEG0 = 8, SEG_STRIDE = 7, SRC0_BSTRIDE = 22, OUT_BSTRIDE = 23, N_I };
enum { CA, CB, CINP, ROWS, TAPS, W_BSTRIDE, W_TAPSTRIDE };          // per segment, relative to SEG0 + g * SEG_STRIDE
enum { SCALE, GN_SILU, SPLITK_SLABS, N_F };
constexpr int iseg(int g, int s) { return SEG0 + SEG_STRIDE * g + s; }         // integer slot s (CA ...) of segment g
constexpr int pseg(int g, int s) { return (SRC_A1 - SRC_A0) * g + s; }         // pointer slot s (SRC_A0, SRC_B0, W0) of segment g
static_assert(iseg(1, W_TAPSTRIDE) < SRC0_BSTRIDE && pseg(1, W0) == W1 && W1 < OUT, "the two segments overlap the slots behind them");
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_gnstats {     // STORM_OP_GN_STATS (storm_gn_stats)
enum { XA, XB, STATS, N_P };
enum { CA, CB, B, HW, G, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_gnapply {     // STORM_OP_GN_APPLY (storm_gn_apply)
enum { XA, XB, STATS, GAMMA, BETA, OUT_ACT, OUT_RAW, N_P };
enum { CA, CB, B, H, W, G, SILU, RESAMPLE, N_I };
enum { EPS, N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_firup {       // STORM_OP_FIR_UP (storm_fir_up2)
enum { X, ADD, OUT, N_P };
enum { B, H, W, C, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_firdown {     // STORM_OP_FIR_DOWN (storm_fir_down2)
enum { X, OUT, N_P };
enum { B, H, W, C, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_softmax {     // STORM_OP_SOFTMAX (storm_softmax_rows)
enum { SCORES, PROBS, N_P };
enum { ROWS, L, LD, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_head {        // STORM_OP_OUTPUT_HEAD (storm_output_head)
enum { PYR, TIME, W, BIAS, OUT, N_P };
enum { CIN, B, F, T, NEGATE, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_gnfin {       // STORM_OP_GN_FINALIZE (storm_gn_finalize; with SS: storm_gn_finalize_ss, which also reads GAMMA, BETA, COUNT, EPS)
enum { PART_A, PART_B, STATS, GAMMA, BETA, SS, N_P };
enum { CA, TILES_A, CB, TILES_B, B, G, COUNT, N_I };
enum { EPS, N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_attention {   // STORM_OP_ATTENTION (storm_attention_ws)
enum { Q, K, VT, BIAS, OUT, SCRATCH, N_P };
enum { B, L, C, LDV, SCRATCH_BYTES, N_I };
enum { SCALE, N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_inpyr {       // STORM_OP_INPUT_PYRAMID (storm_input_pyramid_ex): inputs IN0 .. IN0 + 2, levels LEVEL0 .. LEVEL0 + 3
enum { IN0, LEVEL0 = 3, N_P = LEVEL0 + 4 };
enum { N_IN, B, F, T, N_LEVELS, MEAN, CENTERED, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
namespace op_outpyr {      // STORM_OP_OUTPUT_PYRAMID (storm_output_pyramid): levels PH0 .. PH0 + 7, finest first
enum { PH0, TIME = 8, W, BIAS, OUT, N_P };
enum { CIN, B, F, T, NEGATE, N_LEVELS, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}
static_assert((int)op_head::NEGATE == (int)op_outpyr::NEGATE, "an evaluation's last op is patched with the call's negate whichever of the two it is");
namespace op_combine {     // STORM_OP_COMBINE_CAT (storm_combine_cat)
enum { X, W, BIAS, H, OUT, N_P };
enum { NPIX, C, CINP, N_I };
enum { N_F };
static_assert(N_P <= STORM_OP_NPTR && N_I <= STORM_OP_NINT && N_F <= STORM_OP_NFLT, "slots beyond storm_op");
}

}  // namespace opf
}  // namespace storm
