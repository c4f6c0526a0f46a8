// Program interpreter: executes a host-planned op list (one NCSN++ forward) with a single
// C-ABI call, so the ~300 kernel launches of a score evaluation cost no Python dispatch.
// The slots of an op are named by op_fields.h; the Python mirror of the record is storm_amd/_lib.py (class Op).
#include <cstring>
#include <vector>
#include "common.h"
#include "conv_params.h"
#include "op_fields.h"

using namespace storm;
using namespace storm::opf;

// the STORM_OP_NPTR references of an op against one problem's buffers (g: the problem of a grouped evaluation, < 0 = storm_program_run's own list)
static int resolve_op(const storm_op& op, void* const* bufs, int n_bufs, int k, int g, void** p) {
    bool ok = true;
    for (int j = 0; j < STORM_OP_NPTR; ++j) {
        const storm_ref& r = op.p[j];
        p[j] = nullptr;
        if (r.buf < 0) continue;
        if (r.buf >= n_bufs || bufs[r.buf] == nullptr) ok = false;
        else p[j] = static_cast<char*>(bufs[r.buf]) + r.off;
    }
    if (g < 0) STORM_CHECK(ok, "storm_program_run: op %d (code %d) references a missing buffer", k, op.code);
    else STORM_CHECK(ok, "storm_program_group: op %d of problem %d references a missing buffer", k, g);
    return STORM_OK;
}

void storm::conv_args_of(const storm_op& op, void* const* p, int dtype, storm_conv_args& a) {
    using namespace op_conv;
    const int64_t* i = op.i;
    memset(&a, 0, sizeof(a));
    a.nseg = (int)i[NSEG]; a.B = (int)i[B]; a.H = (int)i[H]; a.W = (int)i[W];
    a.outC = (int)i[OUTC]; a.Cout = (int)i[COUT]; a.tbias_stride = (int)i[TBIAS_STRIDE]; a.out_f32 = (int)i[OUT_F32];
    const long long hw = (long long)a.H * a.W;
    for (int g = 0; g < 2; ++g) {
        storm_conv_seg& sgm = a.seg[g];
        sgm.src_a = p[pseg(g, SRC_A0)]; sgm.src_b = p[pseg(g, SRC_B0)]; sgm.w = p[pseg(g, W0)];
        sgm.Ca = (int)i[iseg(g, CA)]; sgm.Cb = (int)i[iseg(g, CB)]; sgm.CinP = (int)i[iseg(g, CINP)]; sgm.w_rows = (int)i[iseg(g, ROWS)];
        sgm.ntaps = (int)i[iseg(g, TAPS)]; sgm.w_bstride = i[iseg(g, W_BSTRIDE)]; sgm.w_tapstride = i[iseg(g, W_TAPSTRIDE)];
        sgm.bstride_a = hw * sgm.Ca; sgm.bstride_b = hw * sgm.Cb;
    }
    if (i[SRC0_BSTRIDE] >= 0) a.seg[0].bstride_a = i[SRC0_BSTRIDE];
    a.out = p[OUT]; a.bias = (const float*)p[BIAS]; a.tbias = (const float*)p[TBIAS]; a.skip = p[SKIP];
    a.out_bstride = i[OUT_BSTRIDE] >= 0 ? i[OUT_BSTRIDE] : hw * a.outC;
    a.skip_bstride = hw * a.outC;
    a.scale = op.f[SCALE];
    a.dtype = dtype;
    a.gn_part = (float*)p[GN_PART];
    a.seg[0].gn_ss = (const float*)p[GN_SS];
    a.seg[0].gn_silu = op.f[GN_SILU] != 0.f;
    if (p[SPLITK_WS] != nullptr) {                          // split-K scratch: SPLITK_SLABS fp32 slabs [B][H][W][outC] (storm_conv_splitk_bytes at plan time)
        a.splitk_ws = p[SPLITK_WS];
        a.splitk_ws_bytes = (long long)op.f[SPLITK_SLABS] * a.B * hw * a.outC * 4;
    }
}
void storm::conv_shape_args_of(const storm_op& op, int dtype, storm_conv_args& a) {
    void* p[STORM_OP_NPTR];
    for (int j = 0; j < STORM_OP_NPTR; ++j) p[j] = op.p[j].buf >= 0 ? reinterpret_cast<void*>(uintptr_t(16)) : nullptr;
    conv_args_of(op, p, dtype, a);
}

static int run_ops(const storm_op* ops, int n_ops, void* const* bufs, int n_bufs, int dtype, storm_stream_t s,
                   hipEvent_t* ev) {
    STORM_CHECK(ops && bufs && n_ops >= 0, "storm_program_run: bad arguments");
    hipStream_t st = (hipStream_t)s;
    for (int k = 0; k < n_ops; ++k) {
        if (ev) STORM_HIP(hipEventRecord(ev[k], st));
        const storm_op& op = ops[k];
        void* p[STORM_OP_NPTR];
        if (int rc = resolve_op(op, bufs, n_bufs, k, -1, p)) return rc;
        const int64_t* i = op.i;
        int rc = STORM_OK;
        switch (op.code) {                                   // (each case names its op's slots by its namespace of op_fields.h)
            case STORM_OP_MEMSET: { using namespace op_memset;
                STORM_HIP(hipMemsetAsync(p[DST], 0, (size_t)i[BYTES], st));
                break; }
            case STORM_OP_PACK_INPUT: { using namespace op_pack;
                const float* in[3] = {(const float*)p[IN0], (const float*)p[IN0 + 1], (const float*)p[IN0 + 2]};
                rc = storm_pack_input(in, (int)i[N_IN], p[OUT], (int)i[B], (int)i[F], (int)i[T], dtype, s);
                break; }
            case STORM_OP_TEMB: { using namespace op_temb;
                rc = storm_time_embedding((const float*)p[TIME], (const float*)p[GFP_W], (const float*)p[W1], (const float*)p[B1], (const float*)p[W2],
                                          (const float*)p[B2], (float*)p[OUT], (int)i[B], (int)i[NF], s);
                break; }
            case STORM_OP_DENSE: { using namespace op_dense;
                rc = storm_dense((const float*)p[X], (const float*)p[W], (const float*)p[BIAS], (float*)p[OUT], (int)i[B], (int)i[N], (int)i[K], s);
                break; }
            case STORM_OP_CONV: {
                storm_conv_args a;
                conv_args_of(op, p, dtype, a);
                rc = storm_conv(&a, s);
                break; }
            case STORM_OP_GN_STATS: { using namespace op_gnstats;
                rc = storm_gn_stats(p[XA], (int)i[CA], p[XB], (int)i[CB], (int)i[B], (int)i[HW], (int)i[G], (double*)p[STATS], dtype, s);
                break; }
            case STORM_OP_GN_FINALIZE: { using namespace op_gnfin;
                if (p[SS] != nullptr)
                    rc = storm_gn_finalize_ss((const float*)p[PART_A], (int)i[CA], (int)i[TILES_A], (const float*)p[PART_B], (int)i[CB], (int)i[TILES_B],
                                              (int)i[B], (int)i[G], (long long)i[COUNT], (const float*)p[GAMMA], (const float*)p[BETA],
                                              op.f[EPS], (double*)p[STATS], (float*)p[SS], s);
                else
                    rc = storm_gn_finalize((const float*)p[PART_A], (int)i[CA], (int)i[TILES_A], (const float*)p[PART_B], (int)i[CB], (int)i[TILES_B],
                                           (int)i[B], (int)i[G], (double*)p[STATS], s);
                break; }
            case STORM_OP_GN_APPLY: { using namespace op_gnapply;
                rc = storm_gn_apply(p[XA], (int)i[CA], p[XB], (int)i[CB], (int)i[B], (int)i[H], (int)i[W], (int)i[G],
                                    (const double*)p[STATS], (const float*)p[GAMMA], (const float*)p[BETA], op.f[EPS], (int)i[SILU],
                                    (int)i[RESAMPLE], p[OUT_ACT], p[OUT_RAW], dtype, s);
                break; }
            case STORM_OP_FIR_UP: { using namespace op_firup;
                rc = storm_fir_up2(p[X], p[ADD], p[OUT], (int)i[B], (int)i[H], (int)i[W], (int)i[C], dtype, s);
                break; }
            case STORM_OP_FIR_DOWN: { using namespace op_firdown;
                rc = storm_fir_down2(p[X], p[OUT], (int)i[B], (int)i[H], (int)i[W], (int)i[C], dtype, s);
                break; }
            case STORM_OP_SOFTMAX: { using namespace op_softmax;
                rc = storm_softmax_rows((const float*)p[SCORES], p[PROBS], (long long)i[ROWS], (int)i[L], (int)i[LD], dtype, s);
                break; }
            case STORM_OP_ATTENTION: { using namespace op_attention;
                rc = storm_attention_ws(p[Q], p[K], p[VT], (const float*)p[BIAS], p[OUT], (int)i[B], (int)i[L], (int)i[C], (int)i[LDV],
                                        (long long)i[L] * i[C], (long long)i[L] * i[C], (long long)i[C] * i[LDV], (long long)i[L] * i[C],
                                        op.f[SCALE], dtype, p[SCRATCH], (long long)i[SCRATCH_BYTES], s);
                break; }
            case STORM_OP_OUTPUT_HEAD: { using namespace op_head;
                rc = storm_output_head(p[PYR], (const float*)p[TIME], (const float*)p[W], (const float*)p[BIAS], (int)i[CIN],
                                       (float*)p[OUT], (int)i[B], (int)i[F], (int)i[T], (int)i[NEGATE], dtype, s);
                break; }
            case STORM_OP_INPUT_PYRAMID: { using namespace op_inpyr;
                const float* in[3] = {(const float*)p[IN0], (const float*)p[IN0 + 1], (const float*)p[IN0 + 2]};
                rc = storm_input_pyramid_ex(i[N_IN] > 0 ? in : nullptr, (int)i[N_IN], p + LEVEL0, (int)i[N_LEVELS], (int)i[B], (int)i[F], (int)i[T], (int)i[MEAN], (int)i[CENTERED], dtype, s);
                break; }
            case STORM_OP_OUTPUT_PYRAMID: { using namespace op_outpyr;
                rc = storm_output_pyramid(p + PH0, (int)i[N_LEVELS], (const float*)p[TIME], (const float*)p[W], (const float*)p[BIAS], (int)i[CIN],
                                          (float*)p[OUT], (int)i[B], (int)i[F], (int)i[T], (int)i[NEGATE], dtype, s);
                break; }
            case STORM_OP_COMBINE_CAT: { using namespace op_combine;
                rc = storm_combine_cat(p[X], p[W], (int)i[CINP], (const float*)p[BIAS], p[H], p[OUT], (long long)i[NPIX], (int)i[C], dtype, s);
                break; }
            default:
                STORM_CHECK(false, "storm_program_run: op %d has unknown code %d", k, op.code);
        }
        if (rc != STORM_OK) return rc;
    }
    if (ev) STORM_HIP(hipEventRecord(ev[n_ops], st));
    return STORM_OK;
}


// ---- grouped evaluation (common.h) ---------------------------------------------------------------------------------------------------------
// One descriptor per grouped kind (GROUP_TABLE): match says whether op k of the P lists is this kind and computes its geometry ONCE - the sizing
// (program_group_blob_bytes) and the fill (program_group_build) consume the same GroupGeom; fill writes the host image of the kind's table and item
// list and the launch record of its GroupOp; launch runs it from the device copy (program_run_group).  No other function enumerates kinds.
namespace {
struct GroupGeom { long long table_bytes, tiles_bytes, items; GnApplyGroupPlan apply; };   // bytes of the problems' table and of the item / tile list, its entries
// the P lists and the problems' buffers of one program_group_build call (args: scratch of the convolution kinds)
struct GroupCtx { const storm_op* const* ops; void* const* const* bufs; int n_bufs, P, dtype; std::vector<storm_conv_args> args; };
struct GroupDesc {
    bool (*match)(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo);
    // 1 = filled, 0 = not groupable after all (the op runs problem by problem), < 0 = error
    int (*fill)(GroupCtx& c, int k, const GroupGeom& geo, char* table, char* tiles, GroupOp& go);
    int (*launch)(const GroupOp& go, const char* dev_table, const char* dev_tiles, int dtype, hipStream_t st);
};

long long align256(long long v) { return (v + 255) / 256 * 256; }
bool is16(int dtype) { return dtype == STORM_BF16 || dtype == STORM_F16; }

// -- fused attention of the bottleneck (STORM_OP_ATTENTION): same channels and scale in every problem
bool attn_match(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    const storm_op& o0 = ops[0][k];
    if (o0.code != STORM_OP_ATTENTION || !attn_group_supported((int)o0.i[op_attention::C], dtype)) return false;
    geo.items = 0;
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (o.code != STORM_OP_ATTENTION || o.i[op_attention::C] != o0.i[op_attention::C] || o.f[op_attention::SCALE] != o0.f[op_attention::SCALE]) return false;
        geo.items += attn_group_items((int)o.i[op_attention::B], (int)o.i[op_attention::L]);
    }
    geo.table_bytes = attn_group_table_bytes(P); geo.tiles_bytes = align256(geo.items * (long long)sizeof(AttnItem));
    return geo.items < (1LL << 31);                          // (the launch's grid.x)
}
int attn_fill(GroupCtx& c, int k, const GroupGeom&, char* table, char* tiles, GroupOp& go) {
    using namespace op_attention;
    AttnProblem* t = reinterpret_cast<AttnProblem*>(table);
    AttnItem* it = reinterpret_cast<AttnItem*>(tiles);
    long long ni = 0;
    void* p[STORM_OP_NPTR];
    for (int g = 0; g < c.P; ++g) {
        const storm_op& o = c.ops[g][k];
        if (int rc = resolve_op(o, c.bufs[g], c.n_bufs, k, g, p)) return rc;
        ni += attn_group_problem(g, p[Q], p[K], p[VT], p[OUT], (int)o.i[B], (int)o.i[L], (int)o.i[C], (int)o.i[LDV], t[g], it + ni);
    }
    go.attention.C = (int)c.ops[0][k].i[C]; go.attention.bias = static_cast<const float*>(p[BIAS]); go.attention.scale = c.ops[0][k].f[SCALE];
    return 1;
}
int attn_launch(const GroupOp& go, const char* dev_table, const char* dev_tiles, int dtype, hipStream_t st) {
    return launch_attention_group(reinterpret_cast<const AttnProblem*>(dev_table), reinterpret_cast<const AttnItem*>(dev_tiles), (int)go.ntiles, go.attention.bias,
                                  go.attention.C, go.attention.scale, dtype, st);
}

// -- the GroupNorm finalizes (45 per evaluation, ~6 us each whatever the problem's size): same channels and group count in every problem
bool fin_match(const storm_op* const* ops, int k, int P, int, GroupGeom& geo) {
    const storm_op& o0 = ops[0][k];
    geo.items = 0;
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (o.code != STORM_OP_GN_FINALIZE || o.i[op_gnfin::G] != o0.i[op_gnfin::G] || o.i[op_gnfin::CA] + o.i[op_gnfin::CB] != o0.i[op_gnfin::CA] + o0.i[op_gnfin::CB]) return false;
        geo.items += o.i[op_gnfin::B];
    }
    geo.table_bytes = align256((long long)P * sizeof(GnFinProblem)); geo.tiles_bytes = align256(geo.items * (long long)sizeof(GnFinItem));
    return geo.items < 65536;                                // (the launch's grid.y)
}
int fin_fill(GroupCtx& c, int k, const GroupGeom&, char* table, char* tiles, GroupOp& go) {
    using namespace op_gnfin;
    GnFinProblem* t = reinterpret_cast<GnFinProblem*>(table);
    GnFinItem* it = reinterpret_cast<GnFinItem*>(tiles);
    for (int g = 0; g < c.P; ++g) {
        const storm_op& o = c.ops[g][k];
        void* p[STORM_OP_NPTR];
        if (int rc = resolve_op(o, c.bufs[g], c.n_bufs, k, g, p)) return rc;
        GnFinProblem& q = t[g];
        memset(&q, 0, sizeof(q));
        q.pa = (const float*)p[PART_A]; q.pb = (const float*)p[PART_B]; q.stats = (double*)p[STATS]; q.gamma = (const float*)p[GAMMA]; q.beta = (const float*)p[BETA];
        q.ss = (float*)p[SS]; q.count = p[SS] != nullptr ? (long long)o.i[COUNT] : 0; q.Ca = (int)o.i[CA]; q.tiles_a = (int)o.i[TILES_A]; q.Cb = (int)o.i[CB];
        q.tiles_b = (int)o.i[TILES_B]; q.eps = p[SS] != nullptr ? o.f[EPS] : 0.f;
        for (int b = 0; b < (int)o.i[B]; ++b) { it->problem = g; it->b = b; ++it; }
    }
    go.finalize.groups = (int)c.ops[0][k].i[G];
    return 1;
}
int fin_launch(const GroupOp& go, const char* dev_table, const char* dev_tiles, int, hipStream_t st) {
    return launch_gn_finalize_group(reinterpret_cast<const GnFinProblem*>(dev_table), dev_tiles, (int)go.ntiles, go.finalize.groups, st);
}

// -- GroupNorm-apply + SiLU + FIR x2 of h and x (the up / down resblocks' first op: STORM_OP_GN_APPLY with resample 1 / 2): same channels, groups and
// affine parameters in every problem
bool apply_match(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    using namespace op_gnapply;
    const storm_op& o0 = ops[0][k];
    if (!is16(dtype) || o0.code != STORM_OP_GN_APPLY || (o0.i[RESAMPLE] != 1 && o0.i[RESAMPLE] != 2) || o0.i[SILU] == 0 || P > 64) return false;
    int Bs[64], Hs[64], Ws[64];
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (o.code != STORM_OP_GN_APPLY || o.i[CA] != o0.i[CA] || o.i[CB] != o0.i[CB] || o.i[G] != o0.i[G] || o.i[SILU] != o0.i[SILU] || o.i[RESAMPLE] != o0.i[RESAMPLE] || o.f[EPS] != o0.f[EPS]) return false;
        if (o.p[OUT_RAW].buf < 0) return false;              // (the resampling form always writes both tensors)
        Bs[g] = (int)o.i[B]; Hs[g] = (int)o.i[H]; Ws[g] = (int)o.i[W];
    }
    if (!gn_apply_group_plan((int)o0.i[RESAMPLE], (int)(o0.i[CA] + o0.i[CB]), P, Bs, Hs, Ws, dtype, geo.apply)) return false;
    geo.items = geo.apply.items;
    geo.table_bytes = align256((long long)P * sizeof(GnApplyProblem)); geo.tiles_bytes = align256(geo.items * (long long)sizeof(GnFinItem));
    return true;
}
int apply_fill(GroupCtx& c, int k, const GroupGeom& geo, char* table, char* tiles, GroupOp& go) {
    using namespace op_gnapply;
    GnApplyProblem* t = reinterpret_cast<GnApplyProblem*>(table);
    GnFinItem* it = reinterpret_cast<GnFinItem*>(tiles);
    const storm_op& o0 = c.ops[0][k];
    long long ni = 0;
    void* p[STORM_OP_NPTR];
    for (int g = 0; g < c.P; ++g) {
        const storm_op& o = c.ops[g][k];
        if (int rc = resolve_op(o, c.bufs[g], c.n_bufs, k, g, p)) return rc;
        GnApplyProblem& q = t[g];
        memset(&q, 0, sizeof(q));
        q.xa = p[XA]; q.xb = p[XB]; q.stats = (const double*)p[STATS]; q.out_act = p[OUT_ACT]; q.out_raw = p[OUT_RAW]; q.H = (int)o.i[H]; q.W = (int)o.i[W];
        ni += gn_apply_group_problem((int)o0.i[RESAMPLE], (int)(o0.i[CA] + o0.i[CB]), (int)o.i[B], c.dtype, geo.apply, g, q, it + ni);
    }
    STORM_CHECK(ni == geo.items, "storm_program_group: GroupNorm-apply items %lld != %lld", ni, geo.items);
    go.apply.Ca = (int)o0.i[CA]; go.apply.Cb = (int)o0.i[CB]; go.apply.groups = (int)o0.i[G]; go.apply.resample = (int)o0.i[RESAMPLE]; go.apply.plan = geo.apply;
    go.apply.gamma = static_cast<const float*>(p[GAMMA]); go.apply.beta = static_cast<const float*>(p[BETA]); go.apply.eps = o0.f[EPS];
    return 1;
}
int apply_launch(const GroupOp& go, const char* dev_table, const char* dev_tiles, int dtype, hipStream_t st) {
    return launch_gn_apply_group(go.apply.resample, reinterpret_cast<const GnApplyProblem*>(dev_table), dev_tiles, go.apply.plan, go.apply.Ca, go.apply.Cb, go.apply.groups,
                                 go.apply.gamma, go.apply.beta, go.apply.eps, dtype, st);
}

// -- the three 16-bit convolution kinds (STORM_OP_CONV)
constexpr int CA0 = op_conv::iseg(0, op_conv::CA), CB0 = op_conv::iseg(0, op_conv::CB), TAPS0 = op_conv::iseg(0, op_conv::TAPS);   // segment 0's channels and taps
bool conv_match(const storm_op& o, int dtype) {
    return is16(dtype) && switches().conv_variant < 0 &&     // a forced kernel family (tests, A/B) is honoured problem by problem
           o.code == STORM_OP_CONV && (int)o.i[op_conv::OUT_F32] == 0;
}
long long conv_tiles(const storm_op* const* ops, int k, int P, int th, int tw) {   // B x th-row x tw-pixel tiles of all problems
    long long t = 0;
    for (int g = 0; g < P; ++g) t += (long long)ops[g][k].i[op_conv::B] * cdiv(ops[g][k].i[op_conv::H], th) * cdiv(ops[g][k].i[op_conv::W], tw);
    return t;
}
// storm_conv_args of op k of every problem in c.args
int conv_group_args(GroupCtx& c, int k) {
    c.args.resize((size_t)c.P);
    for (int g = 0; g < c.P; ++g) {
        void* p[STORM_OP_NPTR];
        if (int rc = resolve_op(c.ops[g][k], c.bufs[g], c.n_bufs, k, g, p)) return rc;
        conv_args_of(c.ops[g][k], p, c.dtype, c.args[(size_t)g]);
        c.args[(size_t)g].splitk_ws = nullptr; c.args[(size_t)g].splitk_ws_bytes = 0;      // (a grouped launch never splits K)
    }
    return STORM_OK;
}

// the output pyramid's 3x3 convolutions to <= 4 planes (conv_narrow.hip): 4 per evaluation, one 8-wave workgroup per CU walking 20 x 32-pixel tiles
bool narrow_match(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (!conv_match(o, dtype) || (int)o.i[op_conv::OUTC] != 8 || (int)o.i[op_conv::NSEG] != 1 || (int)o.i[TAPS0] != 9) return false;
        if (o.i[op_conv::COUT] != ops[0][k].i[op_conv::COUT] || o.i[CA0] != ops[0][k].i[CA0] || o.i[CB0] != 0) return false;
    }
    geo.items = conv_tiles(ops, k, P, 20, 32);
    geo.table_bytes = conv_narrow_group_bytes(P); geo.tiles_bytes = align256(geo.items * (long long)sizeof(pipe::GroupTile));
    return true;
}
int narrow_fill(GroupCtx& c, int k, const GroupGeom& geo, char* table, char* tiles, GroupOp& go) {
    if (int rc = conv_group_args(c, k)) return rc;
    if (conv_narrow_group_prepare(c.args.data(), c.P, table, reinterpret_cast<pipe::GroupTile*>(tiles), geo.items) != geo.items) return 0;
    const storm_conv_seg& s0 = c.args[0].seg[0];
    go.narrow.Cin = s0.Ca; go.narrow.has_gn = s0.gn_ss != nullptr; go.narrow.silu = s0.gn_silu != 0;
    return 1;
}
int narrow_launch(const GroupOp& go, const char* dev_table, const char* dev_tiles, int dtype, hipStream_t st) {
    return launch_conv_narrow_group(dtype, go.narrow.Cin, go.narrow.has_gn, go.narrow.silu, dev_table, reinterpret_cast<const pipe::GroupTile*>(dev_tiles), go.ntiles, st);
}

// the 8-channel-input convolutions (conv_thin.hip: the stem and the three input-skip 1x1s); the image is one piece (its tile count is fill's)
bool thin_match(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (!conv_match(o, dtype) || (int)o.i[op_conv::NSEG] != 1 || (int)o.i[CA0] != 8 || (int)o.i[CB0] != 0 || (int)o.i[op_conv::OUTC] < 64) return false;
        if (o.i[op_conv::OUTC] != ops[0][k].i[op_conv::OUTC] || o.i[TAPS0] != ops[0][k].i[TAPS0]) return false;
    }
    geo.items = 0; geo.table_bytes = conv_thin_group_bytes(P); geo.tiles_bytes = 0;
    return true;
}
int thin_fill(GroupCtx& c, int k, const GroupGeom&, char* table, char*, GroupOp& go) {
    if (int rc = conv_group_args(c, k)) return rc;
    go.ntiles = conv_thin_group_prepare(c.args.data(), c.P, table);
    if (go.ntiles <= 0) return 0;
    go.thin.P = c.P; go.thin.ntaps = c.args[0].seg[0].ntaps;
    return 1;
}
int thin_launch(const GroupOp& go, const char* dev_table, const char*, int dtype, hipStream_t st) {
    return launch_conv_thin_group(dev_table, go.thin.P, go.ntiles, go.thin.ntaps, dtype, st);
}

// the same 3x3 convolution of the conv_pipe family (> 128 output channels) in every problem: 8-row x 32-pixel tiles
bool pipe_match(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    for (int g = 0; g < P; ++g) {
        const storm_op& o = ops[g][k];
        if (!conv_match(o, dtype) || (int)o.i[op_conv::OUTC] <= 128 || (int)o.i[TAPS0] != 9) return false;
        if (o.i[op_conv::OUTC] != ops[0][k].i[op_conv::OUTC] || o.i[op_conv::COUT] != ops[0][k].i[op_conv::COUT] || o.i[op_conv::NSEG] != ops[0][k].i[op_conv::NSEG]) return false;
    }
    geo.items = conv_tiles(ops, k, P, 8, 32);
    geo.table_bytes = align256((long long)P * sizeof(pipe::PipeParams)); geo.tiles_bytes = align256(geo.items * (long long)sizeof(pipe::GroupTile));
    return true;
}
int pipe_fill(GroupCtx& c, int k, const GroupGeom& geo, char* table, char* tiles, GroupOp& go) {
    if (int rc = conv_group_args(c, k)) return rc;
    if (conv_pipe_group_prepare(c.args.data(), c.P, reinterpret_cast<pipe::PipeParams*>(table), reinterpret_cast<pipe::GroupTile*>(tiles), geo.items) != geo.items)
        return 0;                                            // outside the pipelined kernel's coverage
    go.pipe.outC = c.args[0].outC;
    go.pipe.bn = geo.items * cdiv(go.pipe.outC, 256) >= 512 ? 256 : 128;   // the ladder's rule for the pipelined kernel's two tiles, on the GROUP's tile count
    return 1;
}
int pipe_launch(const GroupOp& go, const char* dev_table, const char* dev_tiles, int dtype, hipStream_t st) {
    return launch_conv_pipe_group(reinterpret_cast<const pipe::PipeParams*>(dev_table), reinterpret_cast<const pipe::GroupTile*>(dev_tiles), go.ntiles, go.pipe.outC,
                                  go.pipe.bn, dtype, st);
}

// indexed by GroupKind, which is the order of precedence: the FIRST kind that matches op k owns it (narrow before thin before pipe) - where its
// fill then declines, the op runs problem by problem, it is not offered to the next kind
const GroupDesc GROUP_TABLE[GROUP_KINDS] = {
    {attn_match, attn_fill, attn_launch},         // GROUP_ATTENTION
    {fin_match, fin_fill, fin_launch},            // GROUP_GN_FINALIZE
    {apply_match, apply_fill, apply_launch},      // GROUP_GN_APPLY
    {narrow_match, narrow_fill, narrow_launch},   // GROUP_CONV_NARROW
    {thin_match, thin_fill, thin_launch},         // GROUP_CONV_THIN
    {pipe_match, pipe_fill, pipe_launch},         // GROUP_CONV_PIPE
};
// the kind of op k of the P lists and its geometry; GROUP_KINDS = none
int group_kind_of(const storm_op* const* ops, int k, int P, int dtype, GroupGeom& geo) {
    int kind = 0;
    while (kind < GROUP_KINDS && !GROUP_TABLE[kind].match(ops, k, P, dtype, geo)) ++kind;
    return kind;
}
}  // namespace

long long storm::program_group_blob_bytes(const storm_op* const* ops, int n_ops, int P, int dtype) {
    long long n = 0;
    if (P < 2) return 0;
    for (int k = 0; k < n_ops; ++k) {
        GroupGeom geo;
        if (group_kind_of(ops, k, P, dtype, geo) < GROUP_KINDS) n += geo.table_bytes + geo.tiles_bytes;
    }
    return n;
}

int storm::program_group_build(const storm_op* const* ops, int n_ops, void* const* const* bufs, int n_bufs, int P, int dtype, char* host_blob,
                               long long blob_bytes, GroupOp* gops, int max_gops, int stable_bufs) {
    int n = 0;
    long long off = 0;
    GroupCtx c{ops, bufs, n_bufs, P, dtype, {}};
    for (int k = 0; k < n_ops; ++k) {
        bool stable = true;                                  // (tables are rebuilt only when a stable buffer moves: nothing else may be in them)
        for (int g = 0; g < P && stable; ++g)
            for (int j = 0; j < STORM_OP_NPTR; ++j) stable = stable && ops[g][k].p[j].buf < stable_bufs;
        if (!stable) continue;
        GroupGeom geo;
        const int kind = group_kind_of(ops, k, P, dtype, geo);
        if (kind == GROUP_KINDS) continue;
        STORM_CHECK(n < max_gops, "storm_program_group: more than %d grouped ops", max_gops);
        STORM_CHECK(off + geo.table_bytes + geo.tiles_bytes <= blob_bytes, "storm_program_group: table blob too small");
        GroupOp& go = gops[n];
        go = GroupOp();
        go.k = k; go.kind = (GroupKind)kind; go.table_off = off; go.tiles_off = off + geo.table_bytes; go.ntiles = geo.items;
        const int rc = GROUP_TABLE[kind].fill(c, k, geo, host_blob + go.table_off, host_blob + go.tiles_off, go);
        if (rc < 0) return rc;
        if (rc == 0) continue;
        ++n;
        off += geo.table_bytes + geo.tiles_bytes;
    }
    return n;
}

int storm::program_run_group(const storm_op* const* ops, int n_ops, void* const* const* bufs, int n_bufs, int P, int dtype, const char* dev_blob,
                             const GroupOp* gops, int n_gops, int negate, storm_stream_t s) {
    int gi = 0;
    for (int k = 0; k < n_ops; ++k) {
        if (gi < n_gops && gops[gi].k == k) {
            const GroupOp& go = gops[gi++];
            if (int rc = GROUP_TABLE[go.kind].launch(go, dev_blob + go.table_off, dev_blob + go.tiles_off, dtype, (hipStream_t)s)) return rc;
            continue;
        }
        for (int g = 0; g < P; ++g) {
            if (k == n_ops - 1 && (ops[g][k].code == STORM_OP_OUTPUT_HEAD || ops[g][k].code == STORM_OP_OUTPUT_PYRAMID)) {
                storm_op head = ops[g][k];
                head.i[op_outpyr::NEGATE] = negate ? 1 : 0;         // (= op_head::NEGATE)
                if (int rc = run_ops(&head, 1, bufs[g], n_bufs, dtype, s, nullptr)) return rc;
            } else if (int rc = run_ops(ops[g] + k, 1, bufs[g], n_bufs, dtype, s, nullptr)) return rc;
        }
    }
    return STORM_OK;
}

extern "C" int storm_program_run(const storm_op* ops, int n_ops, void* const* bufs, int n_bufs, int dtype,
                                 storm_stream_t s) {
    return run_ops(ops, n_ops, bufs, n_bufs, dtype, s, nullptr);
}

// Profiling variant: brackets every op with HIP events ON THE LAUNCH STREAM and returns the
// elapsed milliseconds per op (host array ms[n_ops]); synchronises the stream at the end.
extern "C" int storm_program_run_timed(const storm_op* ops, int n_ops, void* const* bufs, int n_bufs, int dtype,
                                       storm_stream_t s, float* ms) {
    STORM_CHECK(ms != nullptr && n_ops > 0, "storm_program_run_timed: bad arguments");
    hipEvent_t* ev = new hipEvent_t[n_ops + 1];
    int created = 0, rc = STORM_OK;
    for (; created <= n_ops; ++created)
        if (hipEventCreate(&ev[created]) != hipSuccess) { storm::set_error("hipEventCreate failed"); rc = STORM_ERR_HIP; break; }
    if (rc == STORM_OK) rc = run_ops(ops, n_ops, bufs, n_bufs, dtype, s, ev);
    if (rc == STORM_OK && hipEventSynchronize(ev[n_ops]) != hipSuccess) { storm::set_error("hipEventSynchronize failed"); rc = STORM_ERR_HIP; }
    if (rc == STORM_OK)
        for (int k = 0; k < n_ops; ++k)
            if (hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) { storm::set_error("hipEventElapsedTime failed"); rc = STORM_ERR_HIP; break; }
    for (int k = 0; k < created; ++k) (void)hipEventDestroy(ev[k]);
    delete[] ev;
    return rc;
}

// Name of the kernel op k of the program launches (conv ops; "" otherwise): the dispatch decision depends on shapes, dtype
// and which optional pointers are present, not on their values.
extern "C" const char* storm_program_kernel_name(const storm_op* ops, int k, int dtype) {
    if (ops == nullptr || k < 0 || ops[k].code != STORM_OP_CONV) return "";
    storm_conv_args a;
    conv_shape_args_of(ops[k], dtype, a);
    return storm_conv_kernel_name(&a);
}
