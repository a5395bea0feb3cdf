// The frame's plan: everything forward() (engine.hip) decides about one call -- which LayerNorms are launches and which fold into the
// linears either side of them, which linears take e4m3 operands, which neck branches run on the side stream, the two up-sample folds
// and the fused tail of the head, the folded forms of the temporal modules -- decided once, before anything is launched, from the
// model description, the engine's geometry, the batch and the engine state (plan_forward).  forward, neck_proj, neck_rest and
// run_temporal branch on a ForwardPlan only; d2s_forward_plan reports it and tests/test_cpu_forward_plan.py pins it.  Decisions that
// follow from what a GEMM launch does (the statistics slots a LayerNorm producer leaves, whether a convolution folds the up-sample in
// front of it) are obtained by asking plan_gemm about THE launch forward makes: its operand and epilogue come from the op_* functions
// below, which both callers use -- forward with the buffers, plan_forward with a placeholder address (plan_gemm reads pointers for
// presence only, gemm.h).  Host side only.
#pragma once
#include <algorithm>
#include "linear_site.h"

namespace d2s {

// ---- geometry ------------------------------------------------------------------------------------------------------------
// What the model-input shape and max_batch fix for an engine: the token grid, the four neck maps, the workspaces sized from them and the
// temporal modules' (channels, sites).  d2s_engine_finalize allocates from it, plan_forward plans on it, d2s_forward_plan reports it.
struct EngineGeom {
    int gh, gw, P, N, Npad;         // patches per column / row, patch tokens, tokens (+ cls), tokens padded to 64 (V^T rows)
    int fH[4], fW[4];               // the neck maps: 4 x, 2 x, 1 x and (stride-2 3x3) half the patch grid
    size_t splitk_elems;            // fp32 partials of a split-K launch (tiny-M, long-K DPT convs), per stream
    size_t scr_elems;               // one of the five fusion / head scratch maps
    int tmC[4], tmS[4];             // temporal modules layer_3, layer_4, path_4, path_3: channels, sites per frame
};
static inline EngineGeom engine_geom(const d2s_model_desc& d, int h, int w, int max_batch) {
    EngineGeom g = {};
    const int F = d.fusion;
    g.gh = h / d.patch; g.gw = w / d.patch; g.P = g.gh * g.gw; g.N = g.P + 1; g.Npad = (g.N + 63) / 64 * 64;
    g.fH[0] = g.gh * 4; g.fW[0] = g.gw * 4; g.fH[1] = g.gh * 2; g.fW[1] = g.gw * 2; g.fH[2] = g.gh; g.fW[2] = g.gw;
    g.fH[3] = (g.gh - 1) / 2 + 1; g.fW[3] = (g.gw - 1) / 2 + 1;
    g.splitk_elems = (size_t)max_batch * 16 * g.fH[2] * g.fW[2] * std::max(F, d.neck[3]);
    g.scr_elems = std::max({(size_t)64 * g.gh * g.gw * F, (size_t)h * w * (F / 2), (size_t)h * w * d.head_hidden}) * max_batch;
    const int tC[4] = {d.neck[2], d.neck[3], F, F}, tM[4] = {2, 3, 2, 1};       // (reference dpt_temporal.py:50-60)
    for (int m = 0; m < 4; ++m) { g.tmC[m] = tC[m]; g.tmS[m] = g.fH[tM[m]] * g.fW[tM[m]]; }
    return g;
}

// ---- operands and epilogues of the planned launches ----------------------------------------------------------------------------
static inline GemmA plainA(const void* p, long lda) { GemmA a = {}; a.ptr = p; a.mode = A_PLAIN; a.lda = lda; return a; }
static inline GemmA splitA(const void* p, long lda, bool split) { GemmA a = plainA(p, lda); a.bx3 = split ? 1 : 0; return a; }   // bf16x3 engines: pre-split rows
static inline GemmA convA(const void* p, int Hi, int Wi, int C, int Ho, int Wo, int stride, int relu) {
    GemmA a = {}; a.ptr = p; a.mode = A_CONV3; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = Ho; a.Wo = Wo; a.stride = stride; a.relu = relu; return a;
}
struct LinearOp { GemmA a; GemmEpi ep; };

// The encoder's residual updates, x += ls (A W^T + b): proj (A = the attention output, K = D) and FC2 (A = the GELU output, K = mlp).
// slots (not null): the launch is also the producer of the LayerNorm behind it -- the raw residual copy in lnbuf (out2_qscale > 0:
// as e4m3), the row statistics in lnstats, their slot count in *slots
static inline LinearOp op_residual(float* resid, int D, const void* A, int K, bool x3, const float* bias, const float* ls, void* lnbuf,
                                   float* lnstats, int* slots, float out2_qscale) {
    LinearOp o = {splitA(A, K, x3), epi_residual(resid, D, bias, ls)};
    if (slots) epi_ln_producer(o.ep, lnbuf, lnstats, slots, x3, out2_qscale);
    return o;
}
// A temporal module's proj_in (hs = A W^T + b) and to_out (residual: hs += ...), [S, C] x [C, C]; slots as above (copy, stats)
static inline LinearOp op_tm_residual(float* hs, int C, const void* A, const float* bias, bool residual, void* copy, float* stats, int* slots) {
    LinearOp o = {plainA(A, C), residual ? epi_residual(hs, C, bias, nullptr) : rowsE(hs, OUT_F32, C, bias)};
    if (slots) epi_ln_producer(o.ep, copy, stats, slots);
    return o;
}
// A 3x3 convolution of the head on the (Ho, Wo) map with the align_corners up-sample of its (Hs, Ws) source folded into the loader
static inline GemmA upsA(const void* src, int Hs, int Ws, int C, int Ho, int Wo) {
    GemmA a = convA(src, Ho, Wo, C, Ho, Wo, 1, 0);
    a.ups = 1; a.Hs = Hs; a.Ws = Ws; a.usy = linear_scale(Hs, Ho, true); a.usx = linear_scale(Ws, Wo, true);
    return a;
}
// head conv1 reading the last fusion stage's projected map (Hs, Ws) through its x 2 up-sample
static inline LinearOp op_head1_ups(const void* src, int Hs, int Ws, int F, void* out, const float* bias) {
    return {upsA(src, Hs, Ws, F, 2 * Hs, 2 * Ws), rowsE(out, OUT_T, F / 2, bias)};
}
// the fused tail: conv2 + ReLU + conv3 (1x1 -> 1 channel) + ReLU | sigmoid in one launch (MAP_HEAD); ups: conv1's (Hs, Ws) output read
// through the interpolate to (h, w), else the interpolated map itself
static inline LinearOp op_head_tail(const void* in, bool ups, int Hs, int Ws, int h, int w, int C, float* depth, const float* bias, const float* w3,
                                    float b3, float max_depth) {
    LinearOp o = {ups ? upsA(in, Hs, Ws, C, h, w) : convA(in, h, w, C, h, w, 1, 0), rowsE(depth, OUT_F32, 1, bias)};
    o.ep.map = MAP_HEAD; o.ep.scale = w3; o.ep.head_b3 = b3; o.ep.head_max_depth = max_depth;
    return o;
}

// a packed linear's shape for plan_linear / plan_gemm: what finalize will have packed, every pointer the placeholder
static inline void* plan_addr() { static float word[4]; return word; }
static inline DevLinear linear_shape(int gprec, int N, int K) {
    DevLinear L;
    L.w = plan_addr(); L.bias = (const float*)plan_addr(); L.deq = gprec == D2S_PREC_FP8_OPERANDS ? (float*)plan_addr() : nullptr;
    L.N = N; L.K = K; L.Kpad = gemm_kpad(K, gprec); L.prec = gprec;
    return L;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
// the engine state a frame's decisions depend on
struct FrameState {
    bool calib;          // the calibration pass of an e4m3 engine (bf16 operands, LayerNorm kernels, amax of every site)
    bool fp8_ready;      // e4m3 engine: the activation scales are set
    bool taps;           // D2S_TAPS at creation: hidden states are copied out
    bool prof;           // per-kernel timing on
    bool side;           // the engine has its side stream (D2S_NO_OVERLAP unset)
    bool no_lnfuse;      // D2S_NO_LNFUSE at creation
    bool tm_fold;        // temporal engine: the folded forms of its modules were built (bf16, D2S_VDA_FUSE)
    bool tap_private;    // the engine has a LayerNorm operand pair per side tap (D2S_SIDE_SYNC, bf16 engines that fold)
};
// statistics partials per row a consumer kernel takes; a producer that leaves more (or none: WN == 1 tiles) is followed by the LN kernel
constexpr int LN_SLOTS_MAX = 16;
struct ForwardPlan {
    bool use_side;                  // neck branches on the side stream (tap_side); per-kernel timing passes run un-overlapped
    bool f8, f8a, x3;               // FC1 / FC2 on e4m3 operands; QKV / proj too; bf16x3: the encoder linears' A operands travel pre-split
    bool pp_fold, lnf, tap_fold;    // the regimes of the table below
    int slots_proj, slots_fc2;      // statistics partials per row proj / FC2 leave (0: not a producer)
    bool ln1_folded;                // LN1 inside QKV, layers 1 .. (layer 0 has no producer in front of it: always the kernel)
    bool ln2_folded;                // LN2 inside FC1
    bool fc2_stats, fc2_stats_last; // FC2 is a producer; the last layer's too (only the folded reassemble projections read it)
    bool tap_folded;                // the final LayerNorm inside the four reassemble projections
    bool tap_side[4];               // tap i's neck branch runs on the side stream under the remaining encoder layers
    bool tap_private[4];            // ... and its folded projection reads the tap's own LayerNorm operands, not lnbuf / lnstats (engine.hip
                                    // tap_ln_pair; where and how the streams fork and join is not a reported field)
    bool head1_ups;                 // the last fusion stage's up-sample folded into head conv1's loader
    bool head2_fused, head2_ups;    // conv2 + conv3 in one launch (bn: its column tile); the interpolate in front folded into its loader
    int bn;
    bool rcu_fused[4];              // fusion stage idx: r2c1 + r2c2 + the 1x1 projection as one launch (conv3.hip conv3_rcu_kernel<1>)
    bool rcu1_fused[4];             // tap i (< 3): the RCU1 of its fusion layer, r1c1 + r1c2, as one launch (conv3_rcu_kernel<0>)
    bool rcu_wide[4], rcu1_wide[4]; // the same as one launch of the kernel's wide form (conv3_rcu_kernel<PROJ, 1>, 8 x 8-pixel tiles)
    bool tm_fold;                   // temporal modules: proj_in / to_out / ff2 leave the bf16 copy (and statistics) of the folded forms
    struct { int slots[3]; bool folded[3]; } tm[4];   // per temporal module: norms.0 -> kvq[0], norms.1 -> kvq[1], ff_norm -> ff1
    int ln_launches;                // LayerNorm launches of the frame
};

// Regimes by batch B and precision (M = B tokens; measured on ViT-B @ 294 x 518 unless noted):
//   lnf, B <= 3 (bf16x3: <= 8)   LN1 / LN2 fold into QKV / FC1 on the small-tile kernels, proj / FC2 produce the statistics.  Folding wins
//                                7 % at 1 frame, 3-5 % at 2-4, 2 % at 8, is even at 16 and loses 1 % at 32 (the LN kernels' launch floor is
//                                amortised there, the wider epilogues are not).  The limit is 3, not 8, because the ping-pong kernel takes
//                                QKV / FC1 from 100 tiles (4 frames) and folding would keep them on the small tiles: 1 670 -> 1 758 frames/s
//                                at batch 4, 1 815 -> 2 000 at 5, 2 052 -> 2 275 at 8 with the limit at 3.  bf16x3 has no ping-pong kernel
//                                to give way to: 8.  fp32 never folds; the MLP-only e4m3 engine folds LN2 only (PrecRules::ln_folds).
//   in between                   QKV / FC1 on the ping-pong kernel, proj / FC2 (N = D) not yet: nothing folds, 2 layers + 4 LN launches.
//   pp_fold                      bf16 only (pp_supported): once the residual updates run on the ping-pong kernel too -- gemm_pp_min_tiles()
//                                tiles of 256 x 256 over [M, D] -- that kernel folds LayerNorm itself (PP_K_*_LN): the 24 LayerNorm
//                                launches of the batched regime (0.66 ms of a 9.8 ms step at batch 32) are gone as well.  D % 256, D <= 1024
//                                (<= 4 partials per row); D2S_LNF_PP=0 / D2S_GEMM_PP=0: off.
//   tap_fold                     bf16, B == 1 or pp_fold: the shared final LayerNorm folds into the four reassemble projections (the
//                                statistics and the raw residual of a tap layer are still in lnbuf / lnstats when its projection runs).
//   rcu_fused                    bf16, fusion width 128, a map whose 4 x 8-pixel tiles x B fit the CUs: the stage's residual unit and
//                                projection (the taps' RCU1) are one launch; at 294 x 518 the three small maps at B = 1, two at B = 2-4.
//   rcu_wide                     the same engines, a map the 4 x 8 tiles do not fit and whose 8 x 8-pixel tiles x B do (c3_rcu_wide_ok): one
//                                launch of the kernel's wide form; at 294 x 518 the 84 x 148 map (stage 3, tap 0's RCU1) at B = 1, the
//                                42 x 74 map at B = 3-4, 21 x 37 at B = 9-17 (each faster than its launches: profiles/rcu_wide_ab.txt).
//   calibrating, D2S_TAPS        calibration folds nothing (it measures the LayerNorm outputs); taps keep pp_fold off.
static inline int plan_forward(const d2s_model_desc& d, const EngineGeom& g, int h, int w, int B, const FrameState& s, ForwardPlan& pl) {
    pl = ForwardPlan{};
    const PrecRules pr = prec_rules(d.precision);
    if (pr.e4m3 && !s.fp8_ready && !s.calib) {
        set_error("D2S_PREC_FP8 engine: activation scales are not set, call d2s_engine_calibrate first");
        return D2S_E_STATE;
    }
    const int D = d.hidden, F = d.fusion, M = B * g.N;
    float* const ws = (float*)plan_addr();
    pl.use_side = s.side && !s.prof;
    pl.f8 = pr.e4m3 && !s.calib;
    pl.f8a = pl.f8 && pr.e4m3_attn;
    pl.x3 = pr.w == D2S_PREC_BF16X3;
    static EnvInt lnf_pp{"D2S_LNF_PP", 1};
    const int pp_min = gemm_pp_min_tiles();
    const bool forms_lnf = pr.ln_folds(D2S_LIN_FC1) && !pr.e4m3 && !s.no_lnfuse;      // finalize built the bf16 / bf16x3 folded forms
    pl.pp_fold = lnf_pp.get() && forms_lnf && pr.w == D2S_PREC_BF16 && !s.calib && !s.taps && D % 256 == 0 && D <= 1024 && pp_min > 0 &&
                 (long)cdiv(M, 256) * (D / 256) >= pp_min;
    pl.lnf = (pr.ln_folds(D2S_LIN_FC1) && !s.no_lnfuse && !s.calib && B <= (pl.x3 ? 8 : 3)) || pl.pp_fold;
    pl.tap_fold = pl.lnf && pr.ln_folds(D2S_LIN_NECK_PROJ) && (B == 1 || pl.pp_fold);
    pl.fc2_stats = pl.lnf && pr.ln_folds(D2S_LIN_FC2);
    pl.fc2_stats_last = pl.fc2_stats && pl.tap_fold;
    // the producers' slot counts: what plan_gemm says of proj and FC2 as forward launches them
    GemmPlan gp;
    int slots = 0;
    const float qs = pl.f8 ? 1.f : 0.f;                                                   // (e4m3 raw-residual copy: only its presence matters)
    if (pl.lnf) {
        const LinearOp o = op_residual(ws, D, ws, D, pl.x3, ws, ws, ws, ws, &slots, qs);
        if (plan_linear(linear_shape(pl.f8a ? D2S_PREC_FP8_OPERANDS : pr.w, D, D), o.a, M, o.ep, ws, g.splitk_elems, gp)) { set_error(gp.error); return D2S_E_INVALID; }
        pl.slots_proj = gp.stats_slots;
    }
    if (pl.fc2_stats && (d.layers > 1 || pl.fc2_stats_last)) {
        const LinearOp o = op_residual(ws, D, ws, d.mlp, pl.x3, ws, ws, ws, ws, &slots, qs);
        if (plan_linear(linear_shape(pl.f8 ? D2S_PREC_FP8_OPERANDS : pr.w, D, d.mlp), o.a, M, o.ep, ws, g.splitk_elems, gp)) { set_error(gp.error); return D2S_E_INVALID; }
        pl.slots_fc2 = gp.stats_slots;
    }
    pl.ln2_folded = pl.lnf && pl.slots_proj <= LN_SLOTS_MAX;
    pl.ln1_folded = pl.fc2_stats && pr.ln_folds(D2S_LIN_QKV) && pl.slots_fc2 <= LN_SLOTS_MAX;
    pl.tap_folded = pl.tap_fold && pl.slots_fc2 <= LN_SLOTS_MAX;
    // taps 0..2 (+ the RCU1 of their fusion layer) only depend on their tap: side stream.  VDA: the temporal modules of branches 2 and 3
    // share the tm_* workspaces, so branch 3 queues behind branch 2 on the side stream instead of racing it
    for (int i = 0; i < 4; ++i) pl.tap_side[i] = pl.use_side && (i < 3 || d.temporal);
    for (int i = 0; i < 4; ++i) pl.tap_private[i] = pl.tap_side[i] && pl.tap_folded && s.tap_private;
    pl.ln_launches = 1 + (d.layers - 1) * !pl.ln1_folded + d.layers * !pl.ln2_folded + 4 * !pl.tap_folded;
    // ---- the fusion stages' residual units: one launch where c3_rcu_ok (conv3.hip) takes the map -- a bf16 engine with plain row
    // epilogues (no e4m3 operands, not the calibration pass), fusion width 128, every block resident at once.  Stage idx works on neck
    // map 3 - idx; the RCU1 of tap i < 3 on map i (tap 3's map has none).  The same under profiling; D2S_RCU_FUSE=0: the separate launches
    {
        static EnvInt rcu_fuse{"D2S_RCU_FUSE", 1};
        const bool plain_bf16 = rcu_fuse.get() && pr.precision == D2S_PREC_BF16 && !s.calib;
        for (int i = 0; i < 4; ++i) {
            const bool ok = c3_rcu_ok(plain_bf16, F, B, g.fH[i], g.fW[i]);
            pl.rcu_fused[3 - i] = ok;
            pl.rcu1_fused[i] = ok && i < 3;
            const bool wide = c3_rcu_wide_ok(plain_bf16, F, B, g.fH[i], g.fW[i]);     // (never with ok: the rule asks that c3_rcu_ok refuses)
            pl.rcu_wide[3 - i] = wide;
            pl.rcu1_wide[i] = wide && i < 3;
        }
    }
    // ---- temporal modules: the LayerNorm in front of kvq[0] / kvq[1] / ff1 folds where its producer (proj_in / to_out[0] / to_out[1])
    // leaves 1 .. 16 partials per row
    pl.tm_fold = d.temporal && s.tm_fold;
    for (int m = 0; m < 4 && d.temporal; ++m) {
        const int C = g.tmC[m], S = B * g.tmS[m];
        for (int j = 0; j < 3; ++j) {
            if (pl.tm_fold) {
                const LinearOp o = op_tm_residual(ws, C, ws, ws, j > 0, ws, ws, &slots);
                if (plan_linear(linear_shape(pr.w, C, C), o.a, S, o.ep, ws, g.splitk_elems, gp)) { set_error(gp.error); return D2S_E_INVALID; }
                pl.tm[m].slots[j] = gp.stats_slots;
            }
            pl.tm[m].folded[j] = pl.tm_fold && pl.tm[m].slots[j] >= 1 && pl.tm[m].slots[j] <= LN_SLOTS_MAX;
            pl.ln_launches += !pl.tm[m].folded[j];
        }
    }
    // ---- head: the two up-sample folds (where an LDS-resident-input kernel runs the convolution, conv3_upsample_ok) and the fused tail
    // (MAP_HEAD needs a WN == 1 tile over all head_hidden columns; from 224 tiles of 256 pixels)
    {
        const DevLinear h1 = linear_shape(pr.w, F / 2, 9 * F);
        const LinearOp o = op_head1_ups(ws, g.fH[0], g.fW[0], F, ws, ws);
        pl.head1_ups = conv3_upsample_ok(pr.w, 0, o.a, B * 4 * g.fH[0] * g.fW[0], h1.N, h1.K, h1.Kpad, o.ep);
    }
    {
        const int Mh = B * h * w, Nh = d.head_hidden;
        pl.bn = Nh <= 32 ? 32 : 64;
        pl.head2_fused = Nh <= 64 && (long)cdiv(Mh, 256) * cdiv(Nh, pl.bn) >= 224;
        const DevLinear h2 = linear_shape(pr.w, Nh, 9 * (F / 2));
        const LinearOp o = op_head_tail(ws, true, 2 * g.fH[0], 2 * g.fW[0], h, w, F / 2, ws, ws, ws, 0.f, d.max_depth);
        pl.head2_ups = pl.head2_fused && conv3_upsample_ok(pr.w, head_tile(pl.bn), o.a, Mh, Nh, h2.K, h2.Kpad, o.ep);
    }
    return D2S_OK;
}

}  // namespace d2s
