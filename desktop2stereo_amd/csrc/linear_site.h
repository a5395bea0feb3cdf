// The engine's linears, site by site: what an engine precision decides for them, the GemmEpi each launch site builds (engine.hip
// forward, neck_proj, neck_rest, run_temporal), the host-side preparation of their weights (LinearImage: plain, e4m3, LayerNorm
// folded), the packed linear on the device (DevLinear, upload_linear), the forms a launch site picks from (LinearForms) and THE launch
// (launch_linear).  The engine and d2s_linear_probe (gemm.hip) upload and launch through these same two functions, so the probe
// launches what the engine launches by construction; d2s_conv3_probe shares the packing.  Host side only.
#pragma once
#include "gemm.h"
#include <cmath>
#include <vector>

namespace d2s {

// ---- precision -----------------------------------------------------------------------------------------------------------
// What an engine precision (d2s_model_desc.precision, D2S_PREC_*) decides for its linears.  Which batches fold a LayerNorm, and the
// switches that keep one a kernel, are the frame's plan's (forward_plan.h plan_forward).
struct PrecRules {
    int precision;
    int act;            // activations and the kernels that write them: fp32 or bf16 (the e4m3 engines are bf16 engines whose encoder
                        // linears switch to e4m3 operands)
    int w;              // weight packing and GEMM operands: = act, or bf16x3 (split precision on fp32 activations)
    bool e4m3;          // FC1 / FC2 take e4m3 operands once calibrated (D2S_PREC_FP8, D2S_PREC_FP8_MLP) ...
    bool e4m3_attn;     // ... and QKV / proj too (D2S_PREC_FP8)

    // the linear at engine site s (D2S_LIN_*) runs on e4m3 operands
    bool e4m3_site(int s) const {
        return e4m3 && (s == D2S_LIN_FC1 || s == D2S_LIN_FC2 || (e4m3_attn && (s == D2S_LIN_QKV || s == D2S_LIN_PROJ)));
    }
    // a LayerNorm can fold into the linear at engine site s that consumes it, or out of the one that produces it:
    // not on fp32 engines; LN1 (QKV; FC2 produces) not on the MLP-only e4m3 engine either, whose LN1 writes QKV's bf16 operand; the
    // final LayerNorm (reassemble projections) on bf16 engines only, its bf16x3 and e4m3 forms stay kernels; the temporal modules'
    // wherever they run on bf16 operands
    bool ln_folds(int s) const {
        switch (s) {
            case D2S_LIN_QKV: case D2S_LIN_FC2: return precision != D2S_PREC_FP32 && precision != D2S_PREC_FP8_MLP;
            case D2S_LIN_FC1: case D2S_LIN_PROJ: return precision != D2S_PREC_FP32;
            case D2S_LIN_NECK_PROJ: return precision == D2S_PREC_BF16;
            case D2S_LIN_TM_PROJ_IN: case D2S_LIN_TM_KVQ: case D2S_LIN_TM_FF1: case D2S_LIN_TM_TO_OUT: case D2S_LIN_TM_FF2:
                return act == D2S_PREC_BF16 && w == D2S_PREC_BF16;
            default: return false;
        }
    }
};
static inline PrecRules prec_rules(int precision) {
    PrecRules r = {};
    const bool x3 = precision == D2S_PREC_BF16X3;
    r.precision = precision;
    r.e4m3 = precision == D2S_PREC_FP8 || precision == D2S_PREC_FP8_MLP;
    r.e4m3_attn = precision == D2S_PREC_FP8;
    r.act = r.e4m3 ? D2S_PREC_BF16 : (x3 ? D2S_PREC_FP32 : precision);
    r.w = x3 ? D2S_PREC_BF16X3 : r.act;
    return r;
}

// ---- epilogues -----------------------------------------------------------------------------------------------------------
static inline GemmEpi rowsE(void* out, int out_type, long ldc, const float* bias) {
    GemmEpi e = {}; e.out = out; e.out_type = out_type; e.ldc = ldc; e.bias = bias; return e;
}

// patch embedding: patch row m of frame b lands on token row b * ntok + 1 + m % P of the fp32 residual stream (row 0: the cls token,
// written by patchify), plus the position embedding of that token (pos [ntok, D])
static inline GemmEpi epi_patch_embed(float* resid, int D, const float* bias, const float* pos, int P, int ntok) {
    GemmEpi e = rowsE(resid, OUT_F32, D, bias);
    e.rows_per_img = P; e.img_rows = ntok; e.row_off = 1;
    e.res1 = pos; e.res1_mod = P; e.res1_off = 1;
    return e;
}

// QKV output type: bf16 for the attention on the e4m3 engines, the pre-split unit format on bf16x3 engines, else the operand type
static inline int qkv_out_type(bool f8, bool x3) { return f8 ? OUT_BF16 : (x3 ? OUT_BX3 : OUT_T); }
// FC1 output type: the A operand of FC2 (pre-split on bf16x3 engines)
static inline int fc1_out_type(bool x3) { return x3 ? OUT_BX3 : OUT_T; }

// QKV: q | k as rows [M, 3D] (the first 2D columns), v transposed to vt [B, heads, 64, npad] (token t of frame b = row b * ntok + t)
static inline GemmEpi epi_qkv(void* qkv, int out_type, int D, const float* bias, void* vt, int ntok, int npad, int heads) {
    GemmEpi e = rowsE(qkv, out_type, 3 * D, bias);
    e.map = MAP_QKV; e.vt = vt; e.ntok = ntok; e.npad = npad; e.qk_cols = 2 * D; e.heads = heads;
    return e;
}

// the fp32 residual stream updated in place (proj / FC2 with LayerScale ls, a temporal module's to_out / ff2 without):
// x += ls * (A W^T + b)
static inline GemmEpi epi_residual(float* resid, int D, const float* bias, const float* ls) {
    GemmEpi e = rowsE(resid, OUT_F32, D, bias);
    e.scale = ls; e.res1 = resid;
    return e;
}

// FC1: GELU(A W^T + b)
static inline GemmEpi epi_fc1(void* out, int out_type, int N, const float* bias) {
    GemmEpi e = rowsE(out, out_type, N, bias);
    e.act = ACT_GELU;
    return e;
}

// ConvTranspose2d(k = s) of the reassemble stage as a linear: [B gh gw, C] x [s s C, C]^T, pixel-shuffled into [B, s gh, s gw, C]
static inline GemmEpi epi_convT(void* out, int C, const float* bias, int gh, int gw, int ks) {
    GemmEpi e = rowsE(out, OUT_T, C, bias);
    e.map = MAP_SHUFFLE; e.gh = gh; e.gw = gw; e.ks = ks; e.cout = C;
    return e;
}

// LayerNorm folded into the linear that consumes it (DESIGN.md §3.1 "LayerNorm fusion"): A = the RAW residual, W' = W diag(gamma),
// v = rstd (acc - mean csum) before bias' = b + W beta; stats = the producer's partials, slots = the column blocks it reported
static inline void epi_ln_consumer(GemmEpi& e, const float* stats, int slots, const float* csum, float eps, int dim) {
    e.ln_stats = stats; e.ln_slots = slots; e.ln_csum = csum; e.ln_eps = eps; e.ln_dim = dim;
}
// ... and the residual update in front of it: the raw residual copy out2 (bf16; the unit format on bf16x3 engines; e4m3 of
// v * out2_qscale on the e4m3 engines) and the (sum, sum of squares) partials of every row (stats null: the copy only)
static inline void epi_ln_producer(GemmEpi& e, void* out2, float* stats, int* slots, bool bx3 = false, float out2_qscale = 0.f) {
    e.out2 = out2; e.out2_bx3 = bx3 ? 1 : 0; e.stats_out = stats; e.stats_slots = slots; e.out2_qscale = out2_qscale;
}
// the reassemble projection with the final LayerNorm folded in, several frames: it runs over ALL token rows and the store mapping
// drops the cls row of every frame -- token t of frame b lands on patch row b * P + t - 1 (gemm_epi.h epilogue4: row_off < 0)
static inline void epi_drop_cls(GemmEpi& e, int ntok, int P) { e.rows_per_img = ntok; e.img_rows = P; e.row_off = -1; }
// The rows of the folded reassemble projection (after epi_ln_consumer with the statistics of all token rows): one frame skips its cls
// row by starting one row in -- A and the statistics (ln_M = ntok rows per slot); returns that A row offset, 1, and the launch has P
// rows -- while several frames run over all B * ntok token rows and drop the cls rows on store (returns 0).  (0.13 % more rows.)
static inline int epi_tap_fold_rows(GemmEpi& e, int B, int ntok, int P) {
    if (B == 1) { e.ln_stats += 2; e.ln_M = ntok; return 1; }
    epi_drop_cls(e, ntok, P);
    return 0;
}

// ---- weights -------------------------------------------------------------------------------------------------------------
// a logical [N][K] float matrix (given by accessor) -> host [Npad][Kpad] of the weight precision: bf16 (RNE), bf16x3 units, fp32
template <typename F>
static inline std::vector<uint8_t> pack_rows_host(int wprec, int N, int K, F at) {
    const int Kp = gemm_kpad(K, wprec), Np = gemm_npad(N);
    std::vector<uint8_t> buf((size_t)Np * Kp * elem_size(wprec), 0);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            float v = at(n, k);
            if (wprec == D2S_PREC_BF16) ((bf16_t*)buf.data())[(size_t)n * Kp + k] = f2bf(v);
            else if (wprec == D2S_PREC_BF16X3) bx3_pack_elem(buf.data() + (size_t)n * Kp * 4, k, v);      // [8 hi | 8 lo] units
            else ((float*)buf.data())[(size_t)n * Kp + k] = v;
        }
    return buf;
}

// e4m3 weights: row n is divided by s_w[n] = max|row| / 448 (1 for a zero row) and rounded to e4m3 (RNE, saturating)
static inline float fp8_row_scale(float amax) { return amax > 0.f ? amax / FP8_MAX : 1.f; }
template <typename F>
static inline std::vector<uint8_t> pack_rows_fp8_host(int N, int K, F at, std::vector<float>& sw) {
    const int Kp = gemm_kpad(K, D2S_PREC_FP8_OPERANDS), Np = gemm_npad(N);
    std::vector<uint8_t> buf((size_t)Np * Kp, 0);
    sw.assign(N, 1.f);
    for (int n = 0; n < N; ++n) {
        float amax = 0.f;
        for (int k = 0; k < K; ++k) amax = fmaxf(amax, fabsf(at(n, k)));
        const float s = fp8_row_scale(amax);
        sw[n] = s;
        for (int k = 0; k < K; ++k) buf[(size_t)n * Kp + k] = f2e4m3(at(n, k) / s);
    }
    return buf;
}

// LN(x) W^T + b  =  rstd * (x W'^T - mean * colsum(W')) + (b + W beta),  W' = W diag(gamma).  One output row n of the fold: bias'
// (accumulated in double) and the colsum over what the MFMAs sum -- bf16(W'), or its hi + lo halves on bf16x3 engines.  at(n, k): W.
template <typename F>
static inline void ln_fold_row(int wprec, int K, const float* g, const float* beta, F at, int n, double b, float& bias2, float& csum) {
    double sb = b, sc = 0.0;
    for (int k = 0; k < K; ++k) {
        sb += (double)beta[k] * at(n, k);
        const float v = g[k] * at(n, k);
        const float hi = bf2f(f2bf(v));
        sc += wprec == D2S_PREC_BF16X3 ? (double)hi + (double)bf2f(f2bf(v - hi)) : (double)hi;
    }
    bias2 = (float)sb; csum = (float)sc;
}
// the same on e4m3 weights: the colsum over the de-quantised W' (sw: the row scale of W'[n])
template <typename F>
static inline void ln_fold_row_fp8(int K, const float* g, const float* beta, F at, int n, double b, float sw, float& bias2, float& csum) {
    double sb = b, sc = 0.0;
    for (int k = 0; k < K; ++k) { sb += (double)beta[k] * at(n, k); sc += e4m32f(f2e4m3(g[k] * at(n, k) / sw)); }
    bias2 = (float)sb; csum = (float)(sc * sw);
}

// One linear's weights as the GEMM takes them (host side): what upload_linear puts on the device
struct LinearImage {
    int N = 0, K = 0, Kpad = 0;
    int prec = 0;                       // the GEMM precision it was packed for
    std::vector<uint8_t> w;             // [Npad][Kpad] in the GEMM precision
    std::vector<float> bias;            // [N]: the bias, or bias' = b + W beta when a LayerNorm is folded in; empty: none
    std::vector<float> csum;            // [N], folded: the colsum over what the MFMAs add (ln_fold_row*)
    std::vector<float> sw;              // [N], e4m3: the row scales s_w
};
// W [N][K] through at(n, k) in the packed row order, with its bias [N] (or null), for the GEMM precision gprec: the weight precision
// (bf16, bf16x3, fp32) or D2S_PREC_FP8_OPERANDS (e4m3 with per-row scales).  gamma / beta (not null): the LayerNorm in front of the
// linear folded in -- W' = W diag(gamma) packed, bias' = b + W beta (b = 0 without a bias) and its colsum.
template <typename F>
static inline LinearImage prepare_linear(int gprec, int N, int K, F at, const float* bias, const float* gamma = nullptr,
                                         const float* beta = nullptr) {
    LinearImage im;
    im.N = N; im.K = K; im.Kpad = gemm_kpad(K, gprec); im.prec = gprec;
    const bool e4m3 = gprec == D2S_PREC_FP8_OPERANDS;
    auto atg = [&](int n, int k) { return gamma ? gamma[k] * at(n, k) : at(n, k); };
    im.w = e4m3 ? pack_rows_fp8_host(N, K, atg, im.sw) : pack_rows_host(gprec, N, K, atg);
    if (gamma) {
        im.bias.resize(N); im.csum.resize(N);
        for (int n = 0; n < N; ++n) {
            const double b = bias ? bias[n] : 0.0;
            if (e4m3) ln_fold_row_fp8(K, gamma, beta, at, n, b, im.sw[n], im.bias[n], im.csum[n]);
            else ln_fold_row(gprec, K, gamma, beta, at, n, b, im.bias[n], im.csum[n]);
        }
    } else if (bias) {
        im.bias.assign(bias, bias + N);
    }
    return im;
}
// an e4m3 linear's de-quantisation: deq[n] = s_act * s_w[n], s_act the scale of its A operand
static inline std::vector<float> deq_scales(float s_act, const std::vector<float>& sw) {
    std::vector<float> dq(sw.size());
    for (size_t n = 0; n < dq.size(); ++n) dq[n] = s_act * sw[n];
    return dq;
}

// ConvTranspose2d(k = s) weight [Ci, Co, s, s] as a linear's row n = (ky * s + kx) * Co + co, column k = ci
static inline size_t convT_weight_index(int n, int k, int Co, int ks) { const int tap = n / Co, co = n % Co; return ((size_t)k * Co + co) * ks * ks + tap; }
// GEGLU folded into ff1 (ACT_GEGLU): packed row n' = 8 g + w holds x row 4 g + w (w < 4) or gate row 4C + 4 g + (w - 4) of [8C, C]
static inline int geglu_row(int n, int C) { const int g = n >> 3, w = n & 7; return w < 4 ? 4 * g + w : 4 * C + 4 * g + (w - 4); }

// ---- a packed linear on the device -----------------------------------------------------------------------------------------
// A LinearImage on the device: W [Npad][Kpad] in the GEMM precision prec (the engine's weight precision, or D2S_PREC_FP8_OPERANDS)
struct DevLinear {
    void* w = nullptr;                  // null: this form was not built
    const float *bias = nullptr, *csum = nullptr;   // [N] or null: the bias (bias' of a folded form); folded: the colsum
    float* deq = nullptr;               // [N], e4m3: deq[n] = s_act * sw[n], s_act the scale of the A operand
    int N = 0, K = 0, Kpad = 0, prec = 0;
    std::vector<float> sw;              // e4m3: the row scales (host), for whoever sets deq later
};
// im on the device.  alloc(void** dev, const void* host, size_t bytes) -> D2S_OK or an error: the caller's device memory holding the
// host bytes (null: zeroes); the engine tracks it, a probe frees it on return.  folded: a LayerNorm is folded in, the image must have
// its colsum.  twin_bias: an e4m3 form packed without a bias shares its bf16 twin's.  deq: from *s_act, or zeroed until calibrated.
template <typename Alloc>
static inline int upload_linear(Alloc&& alloc, LinearImage im, DevLinear& out, bool folded = false, const float* twin_bias = nullptr,
                                const float* s_act = nullptr) {
    D2S_REQUIRE(!folded || !im.csum.empty(), "upload_linear: a colsum was asked for, but no LayerNorm is folded into this linear");
    out = DevLinear();
    out.N = im.N; out.K = im.K; out.Kpad = im.Kpad; out.prec = im.prec;
    out.bias = twin_bias;
    int rc = alloc(&out.w, im.w.data(), im.w.size());
    if (rc == D2S_OK && !im.bias.empty()) rc = alloc((void**)&out.bias, im.bias.data(), im.bias.size() * sizeof(float));
    if (rc == D2S_OK && folded) rc = alloc((void**)&out.csum, im.csum.data(), im.csum.size() * sizeof(float));
    if (rc == D2S_OK && !im.sw.empty()) {
        const std::vector<float> dq = s_act ? deq_scales(*s_act, im.sw) : std::vector<float>();
        rc = alloc((void**)&out.deq, s_act ? dq.data() : nullptr, im.sw.size() * sizeof(float));
    }
    out.sw = std::move(im.sw);
    return rc;
}

// The forms of one linear, f[e4m3][folded]; a launch site picks by what its A operand is:
//   form(0, 0)  W in the engine's weight precision; A = the LayerNorm-ed (or plain) activation            every linear
//   form(0, 1)  W' = W diag(gamma), bias', colsum; A = the RAW residual copy its producer left             QKV, FC1, reassemble proj, kvq, ff1
//   form(1, 0)  e4m3 W, row scales, deq, the bias vector of form(0, 0); A = e4m3 of the activation         QKV, proj, FC1, FC2
//   form(1, 1)  e4m3 W', bias', colsum over the de-quantised W'; A = e4m3 of the raw residual              QKV, FC1
// Finalize builds those the engine's precision can launch (PrecRules); the others stay empty (w null).
struct LinearForms {
    DevLinear f[2][2];
    DevLinear& form(bool e4m3, bool folded) { return f[e4m3][folded]; }
    const DevLinear& form(bool e4m3, bool folded) const { return f[e4m3][folded]; }
};

// The encoder's calibration sites per layer: LN1 out, attention out, LN2 out, GELU out, the residual after proj, after FC2.
// CALIB_SITE[lin][folded]: the one whose scale is s_act of an e4m3 form of encoder linear lin (0 QKV, 1 proj, 2 FC1, 3 FC2): plain
// forms read their own operand (0..3), folded ones the raw residual -- FC1 site 4 of its layer, QKV site 5 of the layer before
// (dlayer -1: none for layer 0); site -1: no such form
constexpr int NSITE = 6;
struct CalibSite { int site, dlayer; };
constexpr CalibSite CALIB_SITE[4][2] = {{{0, 0}, {5, -1}}, {{1, 0}, {-1, 0}}, {{2, 0}, {4, 0}}, {{3, 0}, {-1, 0}}};

// What a packed linear hands launch_gemm beside its operands: the K the launch runs to and the epilogue as launched.  e4m3: the record's
// deq, K as it is, NO partials -- launch_gemm dispatches on their presence.  Otherwise a ragged K (patch embedding) runs to Kpad, A zero
// padded, and a row-mapped epilogue gets the split-K workspace ws / ws_elems (GemmEpi::part).
static inline int linear_args(const DevLinear& L, GemmEpi& ep, float* ws, size_t ws_elems) {
    if (L.prec == D2S_PREC_FP8_OPERANDS) { ep.deq = L.deq; return L.K; }
    if (ep.map == MAP_ROWS) { ep.part = ws; ep.part_elems = ws_elems; }
    return L.K % (L.prec == D2S_PREC_BF16 ? 8 : 4) ? L.Kpad : L.K;      // (bf16 activations: 8 per chunk; fp32, also under bf16x3 weights: 4)
}
// THE launch of a packed linear, [M, K] x W^T through ep, in the record's GEMM precision; tile: 0, or a probe's override; stop: launch_gemm's
static inline int launch_linear(const DevLinear& L, const GemmA& a, int M, GemmEpi ep, float* ws, size_t ws_elems, int tile, hipStream_t st,
                                hipEvent_t stop = nullptr) {
    D2S_REQUIRE(L.w, "launch_linear: this form of the linear was not built for the engine's precision");
    const int Kl = linear_args(L, ep, ws, ws_elems);
    return launch_gemm(L.prec, tile, a, L.w, M, L.N, Kl, L.Kpad, ep, st, stop);
}
// ... and what launch_gemm would run for it (plan_gemm): host only.  L may be a shape record (linear_shape) -- plan_gemm reads the
// pointers of a launch for presence only (gemm.h)
static inline int plan_linear(const DevLinear& L, const GemmA& a, int M, GemmEpi ep, float* ws, size_t ws_elems, GemmPlan& p) {
    const int Kl = linear_args(L, ep, ws, ws_elems);
    return plan_gemm(L.prec, 0, a, M, L.N, Kl, L.Kpad, ep, p);
}

}  // namespace d2s
