// Depth-Anything-v2 engine: weights, workspaces, forward orchestration, frame pipeline.
// Replaces DepthModelWrapper + its engine plug-ins (reference depth.py:1539-1781) and the
// per-frame glue of predict_depth / make_sbs (reference depth.py:1897-2025, 2186-2231).
#include <map>
#include <string>
#include <vector>
#include <cmath>
#include <cstring>

#include "gemm.h"
#include "forward_plan.h"
#include "dibr_xr.h"
#include "vit_ops.h"

using namespace d2s;

namespace {

struct HostT { std::vector<float> data; std::vector<int64_t> shape; };

struct Layer {
    float *ln1g, *ln1b, *ln2g, *ln2b, *ls1, *ls2;
    LinearForms qkv, proj, fc1, fc2;        // the forms of each (linear_site.h): plain / LayerNorm folded, on e4m3 operands or not
    LinearForms& lin(int i) { LinearForms* const a[4] = {&qkv, &proj, &fc1, &fc2}; return *a[i]; }     // in CALIB_SITE's order
};

}  // namespace

struct d2s_engine {
    d2s_model_desc d;
    int device = 0;
    int prec = D2S_PREC_BF16;          // activation / kernel type: fp32 or bf16
    int wprec = D2S_PREC_BF16;         // weight packing and GEMM operand precision: = prec, or D2S_PREC_BF16X3 (on fp32 activations)
    std::map<std::string, HostT> host;
    bool finalized = false;
    int h = 0, w = 0, maxB = 0;
    EngineGeom g = {};                 // token grid, neck maps, workspace sizes (forward_plan.h engine_geom)
    uint64_t bytes = 0;
    std::vector<void*> allocs;

    // weights
    DevLinear patch;
    float *cls = nullptr, *pos = nullptr;          // pos: [N, D] interpolated (row 0 = cls position)
    std::vector<Layer> L;
    float *lnfg = nullptr, *lnfb = nullptr;
    struct { LinearForms proj; DevLinear resize, conv; } re[4];     // proj's folded form: the final LayerNorm folded in (bf16)
    struct { DevLinear proj, r1c1, r1c2, r2c1, r2c2; } fu[4];
    DevLinear head1, head2;
    float* w3 = nullptr;
    float b3 = 0.f;

    // workspaces
    float* resid = nullptr;                        // [maxB*N, D] fp32 residual stream
    void *lnbuf = nullptr, *qkv = nullptr, *vt = nullptr, *attn = nullptr, *mlp = nullptr, *patchA = nullptr;
    void* tapbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    void* rproj[4] = {nullptr, nullptr, nullptr, nullptr};
    void* rres[4] = {nullptr, nullptr, nullptr, nullptr};
    void* feat[4] = {nullptr, nullptr, nullptr, nullptr};
    void* scr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float* splitk_ws = nullptr;                    // fp32 partials for split-K launches (tiny-M, long-K DPT convs)
    // Neck branches of taps 0..2 (+ the RCU1 of their fusion layer) only depend on their tap, not on later encoder
    // layers: they run on a second stream under the remaining layers (batch 1 leaves most CUs idle per launch).
    hipStream_t side = nullptr;
    hipEvent_t ev_tap[4] = {nullptr, nullptr, nullptr, nullptr}, ev_ln[4] = {nullptr, nullptr, nullptr, nullptr}, ev_side = nullptr;
    bool overlap = true;
    bool side_sync = true;                         // D2S_SIDE_SYNC=0 at creation: shared LayerNorm operands and ev_ln, the fork a recorded event
    // LayerNorm operands owned by side tap i (sized like lnbuf / lnstats): see tap_ln_pair
    void* tap_ln[4] = {nullptr, nullptr, nullptr, nullptr};
    float* tap_stats[4] = {nullptr, nullptr, nullptr, nullptr};
    float* splitk_ws_side = nullptr;               // the side stream's own split-K partials
    void* r1[3] = {nullptr, nullptr, nullptr};     // RCU1(feat[i]) = feat[i] + conv2(relu(conv1(relu(feat[i])))), i = 0..2
    void* r1tmp = nullptr;
    // Video-Depth-Anything temporal modules (desc.temporal): layer_3, layer_4, path_4, path_3
    struct TMod {
        int C = 0, sites = 0;
        float *gn_g = nullptr, *gn_b = nullptr;
        float *ln_g[2] = {nullptr, nullptr}, *ln_b[2] = {nullptr, nullptr}, *ffn_g = nullptr, *ffn_b = nullptr;
        DevLinear proj_in, proj_out, to_out[2], ff2;
        // kvq: fused to_k | to_v | to_q, [3C][C].  Folded forms (round 5, bf16 engine): the module's three LayerNorms folded into their
        // consumers, like the ViT's; ff1's has its rows interleaved x | gate in fours, GEGLU in its epilogue
        LinearForms kvq[2], ff1;
        float* ptab[2] = {nullptr, nullptr};       // [32][3C] = pe @ kvq^T: the positional encoding's share of k | v | q
        void* cache[2] = {nullptr, nullptr};       // rings [max_batch][31][sites][2C] T per attention block: projected k' | v' rows, one ring per stream slot
        size_t ring_bytes = 0;                     // one slot's ring (the single-stream layout: 32-bit offsets hold inside a ring)
    } tm[4];
    float* tm_stats = nullptr;                     // (sum, sum of squares) partials per (row, column block) of the folded LayerNorms
    bool tm_fold = false;
    struct TSlot { int head = 0, filled = 0; };    // a stream slot's window: oldest ring slot; filled = 0 until its first frame has filled the rings
    std::vector<TSlot> tm_slot;                    // [max_batch]
    int row_ids[D2S_MAX_STREAMS] = {0};            // temporal engines: the stream slot of every batch row of the call in flight
    float* tm_hs = nullptr;                        // [max_batch * sites_max, C_max] fp32 residual of the temporal transformer
    void *tm_a = nullptr, *tm_kv = nullptr, *tm_u = nullptr, *tm_g = nullptr, *tm_out = nullptr;
    // pipeline buffers
    float *pre_x = nullptr, *depth_small = nullptr, *depth_post = nullptr;    // model output; post-processed copy (d2s_pipeline)
    void* post_ws = nullptr;
    uint64_t post_ws_bytes = 0;
    float* ema_state = nullptr;                    // [h w]; temporal engines: [max_batch][h w], one state per stream slot
    int ema_init = 0;
    std::vector<int> ema_slot_init;                // temporal engines: [max_batch]
    // debug taps (env D2S_TAPS=1): hidden states of frame 0 after embeddings and each layer
    bool taps = false;
    float* tap_hidden = nullptr;                   // [(layers+1), N, D]
    int last_batch = 0;
    // D2S_PREC_FP8 (BASELINE config 3): encoder linears on e4m3 operands once calibrated
    bool fp8 = false, fp8_ready = false, calib = false;
    bool lnf = false;                 // LayerNorm folded into the producing / consuming linears (bf16, not fp8)
    bool no_lnfuse = false;           // D2S_NO_LNFUSE=1 at creation: the LayerNorms stay kernels (e4m3 engines too)
    bool attn_prescaled = false;      // softmax scale folded into W_q / b_q (bf16 and fp8 engines)
    float* lnstats = nullptr;         // [slots][M][2] partial row sums written by the residual-update GEMMs
    float* amax = nullptr;                         // device [layers][4]: max |.| of LN1 out, attention out, LN2 out, GELU out
    std::vector<float> act_scale;                  // host   [layers][4]: amax / 448
    // per-kernel-class timing with HIP events (d2s_engine_profile): off in the throughput path
    struct ProfRec { int cls; double flops, bytes; hipEvent_t a, b; };
    bool prof_on = false;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    size_t prof_used = 0;
};

namespace {

int dev_alloc(d2s_engine* e, void** p, size_t bytes, bool zero = false) {
    if (bytes == 0) bytes = 16;
    D2S_HIP(hipMalloc(p, bytes));
    e->allocs.push_back(*p);
    e->bytes += bytes;
    if (zero) D2S_HIP(hipMemset(*p, 0, bytes));
    return D2S_OK;
}

int dev_upload(d2s_engine* e, void** p, const void* host, size_t bytes) {
    int rc = dev_alloc(e, p, bytes);
    if (rc) return rc;
    D2S_HIP(hipMemcpy(*p, host, bytes, hipMemcpyHostToDevice));
    return D2S_OK;
}

#define RC(x) do { int _rc = (x); if (_rc != D2S_OK) return _rc; } while (0)

enum { PC_GEMM = 0, PC_CONV, PC_ATTN, PC_LN, PC_ELT, PC_PRE, PC_POST, PC_WARP, PC_N };
const char* const PC_NAMES[PC_N] = {"gemm_linear", "gemm_conv3x3", "attention", "layernorm", "elementwise", "preprocess",
                                    "post_process", "stereo_warp"};

hipEvent_t prof_event(d2s_engine* e) {
    if (e->prof_used == e->prof_pool.size()) { hipEvent_t ev; (void)hipEventCreate(&ev); e->prof_pool.push_back(ev); }
    return e->prof_pool[e->prof_used++];
}
void prof_begin(d2s_engine* e, int cls, double flops, double bytes, hipStream_t st) {
    if (!e->prof_on) return;
    d2s_engine::ProfRec r; r.cls = cls; r.flops = flops; r.bytes = bytes; r.a = prof_event(e); r.b = prof_event(e);
    (void)hipEventRecord(r.a, st);
    e->prof_recs.push_back(r);
}
void prof_end(d2s_engine* e, hipStream_t st) {
    if (!e->prof_on) return;
    (void)hipEventRecord(e->prof_recs.back().b, st);
}
#define PROF(cls, fl, by, call) do { prof_begin(e, cls, fl, by, st); int _rc = (call); prof_end(e, st); if (_rc != D2S_OK) return _rc; } while (0)

const HostT* find(d2s_engine* e, const std::string& name) {
    auto it = e->host.find(name);
    if (it == e->host.end()) { set_error("missing weight tensor: " + name); return nullptr; }
    return &it->second;
}

// THE read of a host tensor: its n values, or null (-> D2S_E_MISSING) with the error set: missing (find), or not n elements (err)
const float* host_f32(d2s_engine* e, const std::string& name, size_t n, const std::string& err) {
    const HostT* t = find(e, name);
    if (t && t->data.size() != n) { set_error(err); t = nullptr; }
    return t ? t->data.data() : nullptr;
}
const float* host_vec(d2s_engine* e, const std::string& name, size_t n) { return host_f32(e, name, n, "weight " + name + ": wrong element count"); }
// a linear's weight (n values) and its bias (N values; bname empty: none, *b = null)
int host_wb(d2s_engine* e, const std::string& wname, size_t n, const std::string& bname, size_t N, const float** w, const float** b) {
    *b = nullptr;
    if (!(*w = host_f32(e, wname, n, "weight " + wname + ": wrong shape"))) return D2S_E_MISSING;
    if (!bname.empty() && !(*b = host_f32(e, bname, N, "bad bias " + bname))) { set_error("bad bias " + bname); return D2S_E_MISSING; }
    return D2S_OK;
}

int upload_f32(d2s_engine* e, const std::string& name, size_t n, float** out) {
    const float* t = host_vec(e, name, n);
    return t ? dev_upload(e, (void**)out, t, n * sizeof(float)) : D2S_E_MISSING;
}

// a prepared linear on the device (linear_site.h upload_linear), in memory the engine tracks
int upload_linear(d2s_engine* e, LinearImage im, DevLinear& out, bool folded = false, const float* twin_bias = nullptr) {
    auto alloc = [e](void** p, const void* host, size_t bytes) { return host ? dev_upload(e, p, host, bytes) : dev_alloc(e, p, bytes, true); };
    return d2s::upload_linear(alloc, std::move(im), out, folded, twin_bias);
}

// The forms of one linear that this engine launches, from W = at(n, k) and its bias: plain; fold: LayerNorm gamma / beta folded in; e8:
// both on e4m3 operands instead (the calibration pass, the one user of an e4m3 engine's bf16 forms, runs the LayerNorm kernels)
template <typename F>
int build_forms(d2s_engine* e, LinearForms& lf, int N, int K, F at, const float* bias, bool fold, const float* gamma, const float* beta, bool e8 = false) {
    RC(upload_linear(e, prepare_linear(e->wprec, N, K, at, bias), lf.form(false, false)));
    if (fold && !e8) RC(upload_linear(e, prepare_linear(e->wprec, N, K, at, bias, gamma, beta), lf.form(false, true), true));
    if (e8) RC(upload_linear(e, prepare_linear(D2S_PREC_FP8_OPERANDS, N, K, at, nullptr), lf.form(true, false), false, lf.form(false, false).bias));
    if (e8 && fold) RC(upload_linear(e, prepare_linear(D2S_PREC_FP8_OPERANDS, N, K, at, bias, gamma, beta), lf.form(true, true), true));
    return D2S_OK;
}
// W [N][K] row-major
auto rows_at(const float* w, int K) { return [w, K](int n, int k) { return w[(size_t)n * K + k]; }; }

int pack_linear(d2s_engine* e, const std::string& wname, const std::string& bname, int N, int K, DevLinear& out) {
    const float *p, *b;
    RC(host_wb(e, wname, (size_t)N * K, bname, N, &p, &b));
    return upload_linear(e, prepare_linear(e->wprec, N, K, rows_at(p, K), b), out);
}

// Conv2d 3x3 weight [Co,Ci,3,3] -> [Co][(ky*3+kx)*Ci + ci]
int pack_conv3(d2s_engine* e, const std::string& wname, const std::string& bname, int Co, int Ci, DevLinear& out) {
    const float *p, *b;
    RC(host_wb(e, wname, (size_t)Co * Ci * 9, bname, Co, &p, &b));
    return upload_linear(e, prepare_linear(e->wprec, Co, 9 * Ci, [&](int n, int k) { return p[conv3_weight_index(n, k, Ci)]; }, b), out);
}

// ConvTranspose2d k==s weight [Ci,Co,k,k] -> rows n = (ky*k+kx)*Co + co, K = Ci; bias expanded
int pack_convT(d2s_engine* e, const std::string& wname, const std::string& bname, int C, int ks, DevLinear& out) {
    const std::string err = "weight " + wname + ": wrong shape";
    const float *p = host_f32(e, wname, (size_t)C * C * ks * ks, err), *bt = host_f32(e, bname, C, err);
    if (!p || !bt) return D2S_E_MISSING;
    int N = ks * ks * C;
    std::vector<float> bias(N);
    for (int n = 0; n < N; ++n) bias[n] = bt[n % C];
    return upload_linear(e, prepare_linear(e->wprec, N, C, [&](int n, int k) { return p[convT_weight_index(n, k, C, ks)]; }, bias.data()), out);
}

// ---- bicubic (align_corners=False, A=-0.75) resample of the position table, float32 like torch ----
void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    auto c1 = [&](float x) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; };
    auto c2 = [&](float x) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; };
    c[0] = c2(t + 1.f); c[1] = c1(t); c[2] = c1(1.f - t); c[3] = c2(2.f - t);
}

void interp_pos(const float* pos, int grid, int D, int gh, int gw, std::vector<float>& out, double offset = 0.0) {
    out.assign((size_t)(1 + gh * gw) * D, 0.f);
    std::memcpy(out.data(), pos, D * sizeof(float));
    if (gh == grid && gw == grid) { std::memcpy(out.data() + D, pos + D, (size_t)grid * grid * D * sizeof(float)); return; }
    float sy = (float)grid / (float)gh, sx = (float)grid / (float)gw;
    if (offset != 0.0) {   // vendored DINOv2 (VDA): scale_factor = (g + 0.1) / grid enters as float(1 / scale_factor), dinov2.py:179-210
        sy = (float)(1.0 / (((double)gh + offset) / (double)grid)); sx = (float)(1.0 / (((double)gw + offset) / (double)grid));
    }
    for (int oy = 0; oy < gh; ++oy) {
        float fy = sy * ((float)oy + 0.5f) - 0.5f;
        float iyf = floorf(fy);
        float cy[4]; cubic_coeffs(fy - iyf, cy);
        int iy = (int)iyf;
        for (int ox = 0; ox < gw; ++ox) {
            float fx = sx * ((float)ox + 0.5f) - 0.5f;
            float ixf = floorf(fx);
            float cx[4]; cubic_coeffs(fx - ixf, cx);
            int ix = (int)ixf;
            float* o = out.data() + (size_t)(1 + oy * gw + ox) * D;
            for (int d = 0; d < D; ++d) {
                float acc = 0.f;
                for (int a = 0; a < 4; ++a) {
                    int yy = std::min(std::max(iy - 1 + a, 0), grid - 1);
                    float row = 0.f;
                    for (int b = 0; b < 4; ++b) {
                        int xx = std::min(std::max(ix - 1 + b, 0), grid - 1);
                        row += pos[(size_t)(1 + yy * grid + xx) * D + d] * cx[b];
                    }
                    acc += row * cy[a];
                }
                o[d] = acc;
            }
        }
    }
}

// the engine state plan_forward decides on
FrameState frame_state(const d2s_engine* e) {
    return FrameState{e->calib, e->fp8_ready, e->taps, e->prof_on, e->overlap && e->side != nullptr, e->no_lnfuse, e->tm_fold, e->tap_ln[0] != nullptr};
}

// The LayerNorm operands of the launches around tap i: the bf16 raw residual and the row statistics a tap layer's FC2 leaves for the
// LayerNorm folded into its two consumers.  pl.tap_private[i] (tap i's branch runs on the side stream and its projection is folded):
// the pair the tap owns.  INVARIANT of that pair, per frame:
//   one writer    the FC2 launch of tap i's layer, on the main stream;
//   two readers   the next layer's LN-folded QKV, on the main stream behind the writer, and neck_proj(i), on the side stream behind the
//                 fork event, which completes with the writer;
//   nothing else on either stream touches it: the next layer's proj, which overwrites the shared lnbuf / lnstats while neck_proj(i)
//                 may still be running, no longer writes what neck_proj(i) reads, so the main stream does not wait for it;
//   next writer   the same FC2 launch of the NEXT frame: it is queued on the main stream behind this frame's join with the side stream
//                 (forward joins every frame that forked, in front of its fusion stage), so both readers are done.  Callers keep one
//                 engine's frames on one stream or order them themselves, as for every other workspace of the engine.
// Every other tap, and every other LayerNorm of the frame, uses the shared pair.
struct LnPair { void* buf; float* stats; };
LnPair tap_ln_pair(const d2s_engine* e, const ForwardPlan& pl, int i) {
    return i >= 0 && i < 4 && pl.tap_private[i] ? LnPair{e->tap_ln[i], e->tap_stats[i]} : LnPair{e->lnbuf, e->lnstats};
}

// The slot guard: a LayerNorm producer reported another number of statistics partials than plan_forward took from plan_gemm for the
// same launch -- plan and launch have drifted apart, and the consumer behind it would read the wrong slots
int slots_check(int got, int planned, const char* site) {
    if (got == planned) return D2S_OK;
    set_error(std::string("forward: ") + site + " left " + std::to_string(got) + " LayerNorm statistics slots, the frame's plan says " + std::to_string(planned));
    return D2S_E_STATE;
}

// a packed linear (convA: an implicit-GEMM convolution): launch_linear with the split-K partials of its stream, each has its own
// stop: an event that completes with the launch (launch_gemm)
int linear(d2s_engine* e, const GemmA& a, const DevLinear& w, int M, const GemmEpi& ep, hipStream_t st, hipEvent_t stop = nullptr) {
    float* ws = (e->side && st == e->side) ? e->splitk_ws_side : e->splitk_ws;
    PROF(a.mode == A_CONV3 ? PC_CONV : PC_GEMM, 2.0 * M * w.N * w.K, 0, launch_linear(w, a, M, ep, ws, e->g.splitk_elems, 0, st, stop));
    return D2S_OK;
}

// 3x3 conv (pad 1) as implicit GEMM over NHWC
int conv3(d2s_engine* e, const void* in, int B, int Hi, int Wi, int C, int stride, int relu_in, const DevLinear& w,
          void* out, int act, const void* res1, const void* res2, hipStream_t st) {
    int Ho = (Hi + 2 - 3) / stride + 1, Wo = (Wi + 2 - 3) / stride + 1;
    GemmA a = convA(in, Hi, Wi, C, Ho, Wo, stride, relu_in);
    GemmEpi ep = rowsE(out, OUT_T, w.N, w.bias);
    ep.act = act; ep.res1 = res1; ep.res2 = res2;
    return linear(e, a, w, B * Ho * Wo, ep, st);
}

// A fusion stage's residual unit as one launch (pl.rcu_fused / pl.rcu1_fused; conv3.hip conv3_rcu_kernel):
// out = x + c2(relu(c1(relu(x)))), through proj where given -- what conv3, conv3 (+ linear) compute in two (three) launches, bit for bit
int rcu(d2s_engine* e, const void* x, int B, int H, int W, const DevLinear& c1, const DevLinear& c2, const DevLinear* proj, bool wide, void* out, hipStream_t st) {
    GemmPlan p;
    if (!plan_conv3_rcu(true, e->d.fusion, B, H, W, proj != nullptr, wide, p) || c1.Kpad != c2.Kpad || !c1.bias || !c2.bias || (proj && !proj->bias)) {
        set_error("forward: the frame's plan fuses a residual unit that conv3_rcu_kernel does not take");
        return D2S_E_STATE;
    }
    const RcuOp o = {x, out, B, H, W, c1.w, c2.w, proj ? proj->w : nullptr, c1.bias, c2.bias, proj ? proj->bias : nullptr, c1.Kpad, proj ? proj->Kpad : 0};
    const double macs = (double)c1.N * c1.K + (double)c2.N * c2.K + (proj ? (double)proj->N * proj->K : 0.0);
    PROF(PC_CONV, 2.0 * B * H * W * macs, 0, (launch_conv3_rcu(p, o, st), D2S_OK));
    return D2S_OK;
}

// One row's entries of an attention block's two row tables, from its stream slot's window and ring.  THE rule for where a frame's
// projected k' | v' rows join the window:
//   fused, filled    the attention kernel overwrites the oldest slot (head) itself, nothing is left for the store launch
//   unfused, filled  the store launch replaces the oldest slot
//   fresh            a window of one (the frame itself at position 0); the store launch fills all 31 slots from 0
void window_rows(const d2s_engine::TSlot& sl, bool fold, void* ring, AttnRow& attn, CacheRow& store) {
    const bool in_attn = fold && sl.filled;
    attn = AttnRow{ring, (int16_t)sl.head, (int16_t)(sl.filled ? 32 : 1), in_attn ? sl.head : -1};
    store = CacheRow{ring, sl.filled ? sl.head : 0, sl.filled ? (in_attn ? 0 : 1) : 31};
}

// One streaming TemporalModule on NHWC maps x [B][sites, C] -> out; row r is the next frame of stream slot e->row_ids[r] and reads, then
// updates, that slot's ring caches.  The linears, LayerNorms and GEGLU see M = B sites rows; GroupNorm, the attention and the ring
// stores are per row.  (reference motion_module.py:102-134, 164-196, 242-321; cache semantics vda2_s.py:177-218)
int run_temporal(d2s_engine* e, const ForwardPlan& pl, int m, const void* x, void* out, int B, hipStream_t st, const void* add = nullptr) {   // out = module(x) [+ add]
    d2s_engine::TMod& t = e->tm[m];
    const int C = t.C, S = B * t.sites, prec = e->prec;   // S: rows of every token matrix of this call
    const int* ids = e->row_ids;
    // bf16 engine (D2S_VDA_FUSE=0: 18 launches per module instead of 11): (i) the three LayerNorms live in the linears
    // either side of them -- the residual-update GEMM (proj_in, to_out) also leaves the raw residual as bf16 in tm_a and the row
    // statistics in tm_stats, the consumer (kvq, ff1) runs on gamma-folded weights (section 3.1b's algebra, eps 1e-5); (ii) the ring
    // store of a frame's k' | v' rows happens inside the attention kernel (the lanes that read the oldest slot's segment overwrite it
    // once both of their passes over it are done); (iii) ff2's epilogue leaves the bf16 copy proj_out reads (no cast kernel).
    const bool fold = pl.tm_fold;
    // the residual update in front of LayerNorm j (0: proj_in, 1 / 2: to_out); folded engines: the producer of the plan's slots
    auto residual = [&](int j, const void* A, const DevLinear& W, const char* site) -> int {
        int slots = -1;
        const LinearOp o = op_tm_residual(e->tm_hs, C, A, W.bias, j > 0, e->tm_a, e->tm_stats, fold ? &slots : nullptr);
        RC(linear(e, o.a, W, S, o.ep, st));
        return fold ? slots_check(slots, pl.tm[m].slots[j], site) : D2S_OK;
    };
    auto consumer = [&](GemmEpi& ep, int j, const float* csum) { epi_ln_consumer(ep, e->tm_stats, pl.tm[m].slots[j], csum, 1e-5f, C); };
    // (folded: proj_in leaves its bf16 copy in tm_a, so the GroupNorm output it reads goes to tm_out -- free until the attention writes it)
    void* gn_out = fold ? e->tm_out : e->tm_a;
    PROF(PC_ELT, 0, 0, launch_groupnorm(prec, x, t.gn_g, t.gn_b, gn_out, t.sites, C, 32, 1e-6f, st, B));
    RC(residual(0, gn_out, t.proj_in, "a temporal module's proj_in"));
    for (int a = 0; a < 2; ++a) {
        const bool folded = pl.tm[m].folded[a];
        if (!folded) PROF(PC_LN, 0, 0, launch_layernorm(prec, e->tm_hs, t.ln_g[a], t.ln_b[a], e->tm_a, S, C, 1e-5f, 0, 0, 0, st));
        // project THIS frame only (k' | v' | q'); the window's other 31 positions are already projected in the ring
        {
            const DevLinear& W = t.kvq[a].form(false, folded);
            GemmEpi ep = rowsE(e->tm_kv, OUT_T, 3 * C, W.bias);
            if (folded) consumer(ep, a, W.csum);
            RC(linear(e, plainA(e->tm_a, C), W, S, ep, st));
        }
        // the frame's projected rows join the window (window_rows): per-row ring / head / window / store slot by value
        AttnRows attn = {};
        CacheRows store = {};
        double win_rows = 0;                            // sum of the rows' window lengths (attention FLOPs)
        bool store_due = false;                         // fused: only fresh rows are left to store (their first-frame fill)
        for (int r = 0; r < B; ++r) {
            window_rows(e->tm_slot[ids[r]], fold, (char*)t.cache[a] + (size_t)ids[r] * t.ring_bytes, attn.r[r], store.r[r]);
            win_rows += attn.r[r].Tw;
            store_due |= store.r[r].nslots > 0;
        }
        PROF(PC_ATTN, 4.0 * t.sites * win_rows * C, 0, launch_temporal_attn(prec, e->tm_kv, t.ptab[a], e->tm_out, t.sites, C, 31, B, attn, st));
        RC(residual(a + 1, e->tm_out, t.to_out[a], "a temporal module's to_out"));
        if (store_due) PROF(PC_ELT, 0, 0, launch_cache_store(prec, e->tm_kv, t.sites, C, B, store, st));
    }
    {
        const bool folded = pl.tm[m].folded[2];
        if (!folded) PROF(PC_LN, 0, 0, launch_layernorm(prec, e->tm_hs, t.ffn_g, t.ffn_b, e->tm_a, S, C, 1e-5f, 0, 0, 0, st));
        // folded: x * gelu(gate) in ff1's own epilogue (interleaved rows): tm_g [S, 4C] directly, no [S, 8C] intermediate, no GEGLU launch
        const DevLinear& W = t.ff1.form(false, folded);
        GemmEpi ep = rowsE(folded ? e->tm_g : e->tm_u, OUT_T, (folded ? 4 : 8) * C, W.bias);
        if (folded) { ep.act = ACT_GEGLU; consumer(ep, 2, W.csum); }
        RC(linear(e, plainA(e->tm_a, C), W, S, ep, st));
        if (!folded) PROF(PC_ELT, 0, 0, launch_geglu(prec, e->tm_u, e->tm_g, S, 4 * C, st));
    }
    {
        GemmEpi ep = epi_residual(e->tm_hs, C, t.ff2.bias, nullptr);
        if (fold) epi_ln_producer(ep, e->tm_a, nullptr, nullptr);     // the bf16 copy proj_out multiplies (no statistics: nothing normalises it)
        RC(linear(e, plainA(e->tm_g, 4 * C), t.ff2, S, ep, st));
    }
    const void* a_out = e->tm_a;
    if (!fold) {
        if (prec == D2S_PREC_BF16) PROF(PC_ELT, 0, 0, launch_cast_f32(prec, e->tm_hs, e->tm_a, (long)S * C, st));
        else a_out = e->tm_hs;                          // fp32 activations: the residual itself is the operand (round 4 copied it)
    }
    {
        GemmEpi ep = rowsE(out, OUT_T, C, t.proj_out.bias);
        ep.res1 = x; ep.res2 = add;
        RC(linear(e, plainA(a_out, C), t.proj_out, S, ep, st));
    }
    return D2S_OK;
}

// Tap i of the neck: reassemble (HF DepthAnythingReassembleStage) + 3x3 to fusion width (neck.convs), then -- for the
// three shallower taps -- the first residual unit of their fusion layer, RCU1(m) = m + conv2(relu(conv1(relu(m)))),
// which depends on this map only (HF DepthAnythingFeatureFusionLayer adds it to the deeper stage's output later).
// reassemble projection of tap i.  pl.tap_folded: the shared final LayerNorm happens inside it -- A = the raw bf16
// residual the tap layer's FC2 left in the tap's LayerNorm operands (tap_ln_pair; patch rows: skip the cls row), statistics likewise
int neck_proj(d2s_engine* e, const ForwardPlan& pl, int i, int B, hipStream_t st) {
    const d2s_model_desc& d = e->d;
    const int D = d.hidden, Mp = B * e->g.P, c = d.neck[i];
    const DevLinear& W = e->re[i].proj.form(false, pl.tap_folded);
    GemmEpi ep = rowsE(e->rproj[i], OUT_T, c, W.bias);
    if (!pl.tap_folded) return linear(e, plainA(e->tapbuf[i], D), W, Mp, ep, st);
    const LnPair ln = tap_ln_pair(e, pl, i);
    epi_ln_consumer(ep, ln.stats, pl.slots_fc2, W.csum, d.ln_eps, D);
    const int skip = epi_tap_fold_rows(ep, B, e->g.N, e->g.P);     // one frame: start one row in; several: all token rows, cls rows dropped
    return linear(e, plainA((const bf16_t*)ln.buf + (size_t)skip * D, D), W, skip ? Mp : B * e->g.N, ep, st);
}

int neck_rest(d2s_engine* e, const ForwardPlan& pl, int i, int B, hipStream_t st) {
    const d2s_model_desc& d = e->d;
    const int F = d.fusion, gh = e->g.gh, gw = e->g.gw, Mp = B * e->g.P, c = d.neck[i];
    const void* src = e->rproj[i];
    int Hs = gh, Ws = gw;
    if (i < 2) {
        int ks = i == 0 ? 4 : 2;
        RC(linear(e, plainA(e->rproj[i], c), e->re[i].resize, Mp, epi_convT(e->rres[i], c, e->re[i].resize.bias, gh, gw, ks), st));
        src = e->rres[i]; Hs = gh * ks; Ws = gw * ks;
    } else if (i == 3) {
        RC(conv3(e, e->rproj[i], B, gh, gw, c, 2, 0, e->re[i].resize, e->rres[i], ACT_NONE, nullptr, nullptr, st));
        src = e->rres[i]; Hs = (gh - 1) / 2 + 1; Ws = (gw - 1) / 2 + 1;
    }
    if (d.temporal && i == 2) { RC(run_temporal(e, pl, 0, src, e->rres[2], B, st)); src = e->rres[2]; }     // layer_3
    if (d.temporal && i == 3) { RC(run_temporal(e, pl, 1, src, e->scr[0], B, st)); src = e->scr[0]; }       // layer_4
    RC(conv3(e, src, B, Hs, Ws, c, 1, 0, e->re[i].conv, e->feat[i], ACT_NONE, nullptr, nullptr, st));
    if (i < 3) {
        const int idx = 3 - i;                          // the fusion layer that consumes this map
        if (pl.rcu1_fused[i] || pl.rcu1_wide[i]) RC(rcu(e, e->feat[i], B, Hs, Ws, e->fu[idx].r1c1, e->fu[idx].r1c2, nullptr, pl.rcu1_wide[i], e->r1[i], st));
        else {
            RC(conv3(e, e->feat[i], B, Hs, Ws, F, 1, 1, e->fu[idx].r1c1, e->r1tmp, ACT_NONE, nullptr, nullptr, st));
            RC(conv3(e, e->r1tmp, B, Hs, Ws, F, 1, 1, e->fu[idx].r1c2, e->r1[i], ACT_NONE, e->feat[i], nullptr, st));
        }
    }
    return D2S_OK;
}

// x: the pre-processed frames [B,3,h,w], or null when d2s_pipeline has already written the patch rows (and cls rows) itself
int forward(d2s_engine* e, const float* x, float* depth, int B, hipStream_t st) {
    const d2s_model_desc& d = e->d;
    const int D = d.hidden, N = e->g.N, P = e->g.P, M = B * N, Mp = B * P, prec = e->prec;
    const int F = d.fusion;
    // every decision of this call (forward_plan.h): from here on the launches below branch on pl only
    ForwardPlan pl;
    RC(plan_forward(d, e->g, e->h, e->w, B, frame_state(e), pl));
    // ---- embeddings (HF Dinov2Embeddings)
    if (x) PROF(PC_ELT, 0, 0, launch_patchify(prec, x, e->patchA, B, e->h, e->w, d.patch, e->patch.Kpad, e->cls, e->pos, e->resid, N, D, st));
    {
        RC(linear(e, plainA(e->patchA, e->patch.Kpad), e->patch, Mp, epi_patch_embed(e->resid, D, e->patch.bias, e->pos, P, N), st));
    }
    if (e->taps) D2S_HIP(hipMemcpyAsync(e->tap_hidden, e->resid, (size_t)N * D * 4, hipMemcpyDeviceToDevice, st));
    // ---- encoder (HF Dinov2Layer x L)
    int tap_i = 0;
    // pl.f8 (D2S_PREC_FP8, calibrated): the producers of the four linears' A operands write e4m3 (x / s_act, saturated); the linears run
    // on e4m3 operands and de-quantise in their epilogue (deq[n] = s_act * s_w[n]); QKV still emits bf16 for the attention.
    // D2S_PREC_FP8_MLP: only FC1 / FC2 take e4m3 operands; LN-1 output / attention output stay bf16 and QKV / proj run the bf16
    // kernels.  pl.f8a = "the attention-side linears are e4m3 too" (the all-four scheme)
    // pl.x3 (bf16x3 engines): the A operands of the four encoder linears are written PRE-SPLIT (bf16 hi | lo units, common.h) by their
    // producers -- LayerNorm, attention, the GELU epilogue -- so that they travel by LDS-DMA like the bf16 engine's; every other
    // GEMM / conv reads fp32 activations and splits them between its staging registers and LDS
    const bool f8 = pl.f8, f8a = pl.f8a, x3 = pl.x3;
    int pending_ln = -1;
    bool fork_in_launch = false;
    int ln_tap = -1;                // the tap whose layer ran last, -1: none -- where this layer's folded LN1 finds its operands (tap_ln_pair)
    for (int l = 0; l < d.layers; ++l) {
        const Layer& ly = e->L[l];
        const float* sa = f8 ? &e->act_scale[(size_t)l * NSITE] : nullptr; // s_act of LN1 out, attention out, LN2 out, GELU out, residual x 2
        float* am = e->calib ? e->amax + (size_t)l * NSITE : nullptr;
        // lnf: the previous layer's FC2 epilogue left the raw bf16 residual in lnbuf and the row statistics in lnstats;
        // LN1 then happens inside the QKV linear (layer 0 has no such producer and runs the LN kernel)
        const bool ln1_folded = pl.ln1_folded && l > 0;
        if (!ln1_folded) PROF(PC_LN, 0, 0, launch_layernorm(prec, e->resid, ly.ln1g, ly.ln1b, e->lnbuf, M, D, d.ln_eps, 0, 0, 0, st, f8a ? 1.0f / sa[0] : 0.f, x3));
        if (am) RC(launch_amax(prec, e->lnbuf, (long)M * D, am + 0, st));
        {
            const DevLinear& W = ly.qkv.form(f8a, ln1_folded);
            GemmEpi ep = epi_qkv(e->qkv, qkv_out_type(f8, x3), D, W.bias, e->vt, N, e->g.Npad, d.heads);
            const LnPair ln = tap_ln_pair(e, pl, ln1_folded ? ln_tap : -1);      // (the LN kernel writes the shared lnbuf)
            if (ln1_folded) epi_ln_consumer(ep, ln.stats, pl.slots_fc2, W.csum, d.ln_eps, D);
            RC(linear(e, splitA(ln.buf, D, x3), W, M, ep, st));
            ln_tap = -1;
        }
        PROF(PC_ATTN, 4.0 * B * d.heads * (double)N * N * 64, 0,
             launch_attention(x3 ? D2S_PREC_BF16X3 : prec, e->qkv, e->vt, e->attn, B, N, e->g.Npad, d.heads, st, f8a ? 1.0f / sa[1] : 0.f, e->attn_prescaled));
        if (am) RC(launch_amax(prec, e->attn, (long)M * D, am + 1, st));
        {
            if (pending_ln >= 0) { D2S_HIP(hipStreamWaitEvent(st, e->ev_ln[pending_ln], 0)); pending_ln = -1; }
            const DevLinear& W = ly.proj.form(f8a, false);
            int slots = -1;
            const LinearOp o = op_residual(e->resid, D, e->attn, D, x3, W.bias, ly.ls1, e->lnbuf, e->lnstats, pl.lnf ? &slots : nullptr, f8 ? 1.0f / sa[4] : 0.f);
            RC(linear(e, o.a, W, M, o.ep, st));
            if (pl.lnf) RC(slots_check(slots, pl.slots_proj, "proj"));
        }
        const bool ln2_folded = pl.ln2_folded;                      // (more than 16 column blocks: the LN kernel runs instead)
        if (!ln2_folded) PROF(PC_LN, 0, 0, launch_layernorm(prec, e->resid, ly.ln2g, ly.ln2b, e->lnbuf, M, D, d.ln_eps, 0, 0, 0, st, f8 ? 1.0f / sa[2] : 0.f, x3));
        if (am) RC(launch_amax(D2S_PREC_FP32, e->resid, (long)M * D, am + 4, st));       // (raw residual: the LN-folded FC1's A operand)
        if (am) RC(launch_amax(prec, e->lnbuf, (long)M * D, am + 2, st));
        {
            const DevLinear& W = ly.fc1.form(f8, ln2_folded);
            GemmEpi ep = epi_fc1(e->mlp, fc1_out_type(x3), d.mlp, W.bias);
            if (ln2_folded) epi_ln_consumer(ep, e->lnstats, pl.slots_proj, W.csum, d.ln_eps, D);
            if (f8) ep.out_qscale = 1.0f / sa[3];
            RC(linear(e, splitA(e->lnbuf, D, x3), W, M, ep, st));
        }
        if (am) RC(launch_amax(prec, e->mlp, (long)M * d.mlp, am + 3, st));
        {
            const DevLinear& W = ly.fc2.form(f8, false);
            const bool stats = l + 1 < d.layers ? pl.fc2_stats : pl.fc2_stats_last;
            const bool tap_layer = tap_i < 4 && l + 1 == d.out_indices[tap_i];
            int slots = -1;
            const LnPair ln = tap_ln_pair(e, pl, tap_layer ? tap_i : -1);
            const LinearOp o = op_residual(e->resid, D, e->mlp, d.mlp, x3, W.bias, ly.ls2, ln.buf, ln.stats, stats ? &slots : nullptr, f8 ? 1.0f / sa[5] : 0.f);
            // a folded side tap forks behind this launch: its own completion is the fork event (no marker packet on the main stream)
            fork_in_launch = tap_layer && pl.tap_side[tap_i] && pl.tap_folded && e->side_sync;
            RC(linear(e, o.a, W, M, o.ep, st, fork_in_launch ? e->ev_tap[tap_i] : nullptr));
            if (tap_layer) ln_tap = tap_i;
            if (stats) RC(slots_check(slots, pl.slots_fc2, "FC2"));
        }
        if (am) RC(launch_amax(D2S_PREC_FP32, e->resid, (long)M * D, am + 5, st));       // (raw residual: the next layer's LN-folded QKV)
        if (e->taps) D2S_HIP(hipMemcpyAsync(e->tap_hidden + (size_t)(l + 1) * N * D, e->resid, (size_t)N * D * 4, hipMemcpyDeviceToDevice, st));
        if (tap_i < 4 && l + 1 == d.out_indices[tap_i]) {     // HF Dinov2Backbone: shared final LN, drop cls
            // folded: the statistics and the raw residual of the tap layer are still in its LayerNorm operands when its projection runs
            // (tap_ln_pair).  Where those are the shared lnbuf / lnstats (D2S_SIDE_SYNC=0) the main stream waits for that launch -- ev_ln --
            // before the next layer's projection GEMM overwrites them
            if (!pl.tap_folded) PROF(PC_LN, 0, 0, launch_layernorm(prec, e->resid, e->lnfg, e->lnfb, e->tapbuf[tap_i], Mp, D, d.ln_eps, P, N, 1, st));
            // this tap's neck branch runs under the remaining encoder layers (pl.tap_side)
            if (pl.tap_side[tap_i]) {
                if (!fork_in_launch) D2S_HIP(hipEventRecord(e->ev_tap[tap_i], st));
                D2S_HIP(hipStreamWaitEvent(e->side, e->ev_tap[tap_i], 0));
                RC(neck_proj(e, pl, tap_i, B, e->side));
                if (pl.tap_folded && !pl.tap_private[tap_i]) { D2S_HIP(hipEventRecord(e->ev_ln[tap_i], e->side)); pending_ln = tap_i; }
                RC(neck_rest(e, pl, tap_i, B, e->side));
            } else {
                RC(neck_proj(e, pl, tap_i, B, st));           // (its inputs are overwritten by the next layer; the rest can wait)
            }
            ++tap_i;
        }
    }
    // ---- neck branches that did not run on the side stream, then join it (every frame that forked joins here: tap_ln_pair relies on it)
    for (int i = 0; i < 4; ++i)
        if (!pl.tap_side[i]) RC(neck_rest(e, pl, i, B, st));
    if (pl.use_side) {
        D2S_HIP(hipEventRecord(e->ev_side, e->side));
        D2S_HIP(hipStreamWaitEvent(st, e->ev_side, 0));
    }
    // ---- fusion, deep -> shallow (HF DepthAnythingFeatureFusionStage).  hidden(idx) = fused(idx-1) + RCU1(m): the sum is
    // formed where fused(idx-1) is produced (up-sample / temporal-module epilogue), from the r1[] maps of the neck branches.
    void *X = e->scr[0], *Y = e->scr[1], *Z = e->scr[2];
    void* fused = nullptr;
    int Hc = 0, Wc = 0;
    for (int idx = 0; idx < 4; ++idx) {
        int mi = 3 - idx;
        void* m = e->feat[mi];
        Hc = e->g.fH[mi]; Wc = e->g.fW[mi];
        const void* hcur = idx == 0 ? m : fused;
        // RCU2 and the projection behind it (below): X = proj(h + r2c2(relu(r2c1(relu(h))))), one launch where the plan fuses the stage
        const bool one_launch = pl.rcu_fused[idx] || pl.rcu_wide[idx];
        if (one_launch) RC(rcu(e, hcur, B, Hc, Wc, e->fu[idx].r2c1, e->fu[idx].r2c2, &e->fu[idx].proj, pl.rcu_wide[idx], X, st));
        else {
            RC(conv3(e, hcur, B, Hc, Wc, F, 1, 1, e->fu[idx].r2c1, X, ACT_NONE, nullptr, nullptr, st));
            RC(conv3(e, X, B, Hc, Wc, F, 1, 1, e->fu[idx].r2c2, Z, ACT_NONE, hcur, nullptr, st));
        }
        int Ho, Wo;
        if (idx < 3) { Ho = e->g.fH[mi - 1]; Wo = e->g.fW[mi - 1]; } else { Ho = Hc * 2; Wo = Wc * 2; }
        // HF: projection(interpolate(h)).  The 1x1 projection (+bias) commutes with bilinear interpolation
        // (interpolation weights sum to 1), so it runs BEFORE the up-sample on 4x fewer pixels.
        void* pout = e->scr[3 + (idx & 1)];
        const void* next_r1 = idx < 3 ? e->r1[2 - idx] : nullptr;      // RCU1 of the next (shallower) stage's map
        if (!one_launch) RC(linear(e, plainA(Z, F), e->fu[idx].proj, B * Hc * Wc, rowsE(X, OUT_T, F, e->fu[idx].proj.bias), st));
        if (d.temporal && idx < 2) {                     // path_4 / path_3 (dpt_temporal.py:98-103)
            PROF(PC_ELT, 0, 0, launch_bilinear_nhwc(prec, X, pout, B, Hc, Wc, Ho, Wo, F, st));
            void* alt = e->scr[3 + ((idx + 1) & 1)];
            RC(run_temporal(e, pl, 2 + idx, pout, alt, B, st, next_r1));
            pout = alt;
        } else {
            // the last stage's up-sample feeds the head's conv1 only: folded into its halo loader where an LDS-resident-input
            // kernel runs it (pl.head1_ups); conv1 then reads X (the projected map) and writes Y
            if (!(idx == 3 && pl.head1_ups)) PROF(PC_ELT, 0, 0, launch_bilinear_nhwc(prec, X, pout, B, Hc, Wc, Ho, Wo, F, st, next_r1));
        }
        fused = pout; Hc = Ho; Wc = Wo;
    }
    // ---- head (HF DepthAnythingDepthEstimationHead)
    void* c1out = X;                                     // conv1 output; the (optional) up-sample between conv1 and conv2 goes c1out -> up2
    void* up2 = Y;
    if (pl.head1_ups) {
        c1out = Y; up2 = X;
        const LinearOp o = op_head1_ups(X, e->g.fH[0], e->g.fW[0], F, c1out, e->head1.bias);
        PROF(PC_CONV, 2.0 * B * Hc * Wc * e->head1.N * e->head1.K, 0, launch_gemm(e->wprec, 0, o.a, e->head1.w, B * Hc * Wc, e->head1.N, e->head1.K, e->head1.Kpad, o.ep, st));
    } else {
        RC(conv3(e, fused, B, Hc, Wc, F, 1, 0, e->head1, c1out, ACT_NONE, nullptr, nullptr, st));
    }
    {
        const int Mh = B * e->h * e->w, Nh = d.head_hidden;
        // the interpolate between conv1 and conv2 folded into conv2's halo loader where the persistent head kernel runs (conv3.hip)
        if (!pl.head2_ups) PROF(PC_ELT, 0, 0, launch_bilinear_nhwc(prec, c1out, up2, B, Hc, Wc, e->h, e->w, F / 2, st));
        if (pl.head2_fused) {
            const LinearOp o = op_head_tail(pl.head2_ups ? c1out : up2, pl.head2_ups, Hc, Wc, e->h, e->w, F / 2, depth, e->head2.bias, e->w3, e->b3, d.max_depth);
            PROF(PC_CONV, 2.0 * Mh * Nh * e->head2.K, 0, launch_gemm(e->wprec, head_tile(pl.bn), o.a, e->head2.w, Mh, Nh, e->head2.K, e->head2.Kpad, o.ep, st));
        } else {
            RC(conv3(e, up2, B, e->h, e->w, F / 2, 1, 0, e->head2, Z, ACT_RELU, nullptr, nullptr, st));
            PROF(PC_ELT, 0, 0, launch_head_final(prec, Z, e->w3, e->b3, d.max_depth, depth, (long)B * e->h * e->w, d.head_hidden, st));
        }
    }
    if (d.temporal) {                                    // one window step per frame (vda2_s.py:177-187, 214-221), for the streams of this call only
        for (int r = 0; r < B; ++r) {
            d2s_engine::TSlot& sl = e->tm_slot[e->row_ids[r]];
            if (sl.filled) sl.head = (sl.head + 1) % 31;
            sl.filled = 1;
        }
    }
    e->last_batch = B;
    return D2S_OK;
}

// what d2s_engine_create refuses of a model description, and d2s_engine_finalize of a shape for it (d2s_forward_plan: the same words)
int check_desc(const d2s_model_desc* desc) {
    D2S_REQUIRE(desc->hidden > 0 && desc->heads > 0 && desc->hidden == desc->heads * 64, "head_dim must be 64");
    D2S_REQUIRE(desc->layers > 0 && desc->patch > 0 && desc->pos_grid > 0 && desc->fusion % 8 == 0, "bad model desc");
    D2S_REQUIRE(desc->precision == D2S_PREC_FP32 || desc->precision == D2S_PREC_BF16 || desc->precision == D2S_PREC_FP8 ||
                desc->precision == D2S_PREC_BF16X3 || desc->precision == D2S_PREC_FP8_MLP, "bad precision");
    for (int i = 0; i < 4; ++i) D2S_REQUIRE(desc->neck[i] % 8 == 0 && desc->out_indices[i] >= 1 && desc->out_indices[i] <= desc->layers, "bad neck / out_indices");
    D2S_REQUIRE(desc->head_hidden % 4 == 0 && desc->mlp % 8 == 0, "bad head_hidden / mlp");
    D2S_REQUIRE(desc->max_depth >= 0.f && !(desc->temporal && desc->max_depth > 0.f),
                "max_depth must be >= 0, and 0 for a Video-Depth-Anything engine (its head ends in ReLU, dpt_temporal.py:136)");
    return D2S_OK;
}
int check_shape(const d2s_model_desc& d, int h, int w, int max_batch) {
    D2S_REQUIRE(h > 0 && w > 0 && h % d.patch == 0 && w % d.patch == 0 && max_batch >= 1, "h, w must be patch multiples");
    D2S_REQUIRE(!d.temporal || max_batch <= D2S_MAX_STREAMS, "a Video-Depth-Anything engine has at most D2S_MAX_STREAMS (32) stream slots: max_batch too large");
    for (int c : {d.neck[2], d.neck[3], d.fusion})
        D2S_REQUIRE(!d.temporal || (c % 32 == 0 && c <= 1024), "temporal module channels must be a multiple of 32 (GroupNorm) and <= 1024");
    return D2S_OK;
}

}  // namespace

// ================================================================================================
extern "C" int d2s_engine_create(const d2s_model_desc* desc, int device_id, d2s_engine** out) {
    D2S_REQUIRE(desc && out, "null pointer");
    RC(check_desc(desc));
    D2S_ON_DEVICE(device_id);
    d2s_engine* e = new d2s_engine();
    e->d = *desc; e->device = device_id;
    const PrecRules pr = prec_rules(desc->precision);
    e->fp8 = pr.e4m3;
    // LayerNorm fusion into the encoder's own bf16 / bf16x3 linears (the e4m3 engines fold into their e4m3 copies)
    e->no_lnfuse = env_int("D2S_NO_LNFUSE", 0) != 0;
    e->lnf = pr.ln_folds(D2S_LIN_FC1) && !pr.e4m3 && !e->no_lnfuse;
    e->prec = pr.act;
    e->wprec = pr.w;
    e->attn_prescaled = e->prec == D2S_PREC_BF16;
    e->taps = env_int("D2S_TAPS", 0) != 0;
    *out = e;
    return D2S_OK;
}

extern "C" int d2s_engine_set_weight(d2s_engine* e, const char* name, const float* host, const int64_t* shape, int ndim) {
    D2S_REQUIRE(e && name && host && shape && ndim >= 1 && ndim <= 4, "bad argument");
    if (e->finalized) { set_error("d2s_engine_set_weight after finalize"); return D2S_E_STATE; }
    HostT t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { D2S_REQUIRE(shape[i] > 0, "bad shape"); n *= (size_t)shape[i]; t.shape.push_back(shape[i]); }
    t.data.assign(host, host + n);
    e->host[name] = std::move(t);
    return D2S_OK;
}

extern "C" int d2s_engine_finalize(d2s_engine* e, int h, int w, int max_batch) {
    D2S_REQUIRE(e, "null engine");
    if (e->finalized) { set_error("engine already finalized"); return D2S_E_STATE; }
    const d2s_model_desc& d = e->d;
    RC(check_shape(d, h, w, max_batch));
    D2S_ON_DEVICE(e->device);
    const int D = d.hidden, F = d.fusion;
    const PrecRules pr = prec_rules(d.precision);
    e->h = h; e->w = w; e->maxB = max_batch;
    e->g = engine_geom(d, h, w, max_batch);
    const int N = e->g.N, P = e->g.P, B = max_batch;
    const size_t es = elem_size(e->prec);
    std::string pe = "backbone.embeddings.";
    // ---- weights
    RC(pack_linear(e, pe + "patch_embeddings.projection.weight", pe + "patch_embeddings.projection.bias", D, 3 * d.patch * d.patch, e->patch));
    RC(upload_f32(e, pe + "cls_token", D, &e->cls));
    {
        const float* pt = host_f32(e, pe + "position_embeddings", (size_t)(d.pos_grid * d.pos_grid + 1) * D, "position_embeddings: wrong shape");
        if (!pt) return D2S_E_MISSING;
        std::vector<float> pos;
        interp_pos(pt, d.pos_grid, D, e->g.gh, e->g.gw, pos, d.temporal ? 0.1 : 0.0);
        RC(dev_alloc(e, (void**)&e->pos, pos.size() * 4));
        D2S_HIP(hipMemcpy(e->pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice));
    }
    e->L.resize(d.layers);
    for (int l = 0; l < d.layers; ++l) {
        std::string p = "backbone.encoder.layer." + std::to_string(l) + ".";
        Layer& ly = e->L[l];
        RC(upload_f32(e, p + "norm1.weight", D, &ly.ln1g)); RC(upload_f32(e, p + "norm1.bias", D, &ly.ln1b));
        RC(upload_f32(e, p + "norm2.weight", D, &ly.ln2g)); RC(upload_f32(e, p + "norm2.bias", D, &ly.ln2b));
        RC(upload_f32(e, p + "layer_scale1.lambda1", D, &ly.ls1)); RC(upload_f32(e, p + "layer_scale2.lambda1", D, &ly.ls2));
        const float *g1 = host_vec(e, p + "norm1.weight", D), *bn1 = host_vec(e, p + "norm1.bias", D), *g2 = host_vec(e, p + "norm2.weight", D),
                    *bn2 = host_vec(e, p + "norm2.bias", D);                    // (uploaded above: all there)
        // encoder linear `site`: folded where the precision folds there (bf16 / bf16x3: unless switched off), e4m3 where it runs on it
        auto forms = [&](LinearForms& lf, int site, int N, int K, auto at, const float* bias, const float* gamma, const float* beta) {
            const bool e8 = pr.e4m3_site(site);
            return build_forms(e, lf, N, K, at, bias, gamma && pr.ln_folds(site) && (e8 || e->lnf), gamma, beta, e8);
        };
        // fused QKV: rows q | k | v
        const std::string qa = p + "attention.attention.";
        const char* const qkv_err = "qkv weight: wrong shape";
        const float* ws[3] = {host_f32(e, qa + "query.weight", (size_t)D * D, qkv_err), host_f32(e, qa + "key.weight", (size_t)D * D, qkv_err), host_f32(e, qa + "value.weight", (size_t)D * D, qkv_err)};
        const float *bq = host_vec(e, qa + "query.bias", D), *bk = host_vec(e, qa + "key.bias", D), *bv = host_vec(e, qa + "value.bias", D);
        if (!ws[0] || !ws[1] || !ws[2] || !bq || !bk || !bv) return D2S_E_MISSING;
        std::vector<float> bias(3 * D);
        for (int i = 0; i < D; ++i) { bias[i] = bq[i]; bias[D + i] = bk[i]; bias[2 * D + i] = bv[i]; }
        // bf16 / fp8 engines: the softmax scale 64^-0.5 log2(e) goes into the q rows of the fused QKV weight and bias (fp32
        // product, then the ONE rounding every weight gets): the attention kernels see log2-domain scores, the batched one
        // straight from the matrix pipe (attention.hip).  The fp32 engine (parity class) keeps the reference's order of operations.
        std::vector<float> wq_scaled;
        if (e->attn_prescaled) {
            wq_scaled.assign(ws[0], ws[0] + (size_t)D * D);
            for (float& v : wq_scaled) v *= ATTN_SCALE_LOG2E;
            for (int i = 0; i < D; ++i) bias[i] *= ATTN_SCALE_LOG2E;
            ws[0] = wq_scaled.data();
        }
        RC(forms(ly.qkv, D2S_LIN_QKV, 3 * D, D, [&](int n, int k) { return ws[n / D][(size_t)(n % D) * D + k]; }, bias.data(), g1, bn1));
        auto dense = [&](LinearForms& lf, int site, const std::string& nm, int N, int K, const float* gamma, const float* beta) {
            const float *w, *b;
            RC(host_wb(e, nm + "weight", (size_t)N * K, nm + "bias", N, &w, &b));
            return forms(lf, site, N, K, rows_at(w, K), b, gamma, beta);
        };
        RC(dense(ly.proj, D2S_LIN_PROJ, p + "attention.output.dense.", D, D, nullptr, nullptr));
        RC(dense(ly.fc1, D2S_LIN_FC1, p + "mlp.fc1.", d.mlp, D, g2, bn2));
        RC(dense(ly.fc2, D2S_LIN_FC2, p + "mlp.fc2.", D, d.mlp, nullptr, nullptr));
    }
    if (e->fp8) {
        RC(dev_alloc(e, (void**)&e->amax, (size_t)d.layers * NSITE * sizeof(float), true));
        e->act_scale.assign((size_t)d.layers * NSITE, 0.f);
    }
    RC(upload_f32(e, "backbone.layernorm.weight", D, &e->lnfg));
    RC(upload_f32(e, "backbone.layernorm.bias", D, &e->lnfb));
    for (int i = 0; i < 4; ++i) {
        std::string p = "neck.reassemble_stage.layers." + std::to_string(i) + ".";
        int c = d.neck[i];
        // (the final LayerNorm folded into the reassemble projection too)
        const float *wt, *bt, *gf = host_vec(e, "backbone.layernorm.weight", D), *bf = host_vec(e, "backbone.layernorm.bias", D);   // (uploaded above)
        RC(host_wb(e, p + "projection.weight", (size_t)c * D, p + "projection.bias", c, &wt, &bt));
        RC(build_forms(e, e->re[i].proj, c, D, rows_at(wt, D), bt, e->lnf, gf, bf));
        if (i == 0) RC(pack_convT(e, p + "resize.weight", p + "resize.bias", c, 4, e->re[i].resize));
        if (i == 1) RC(pack_convT(e, p + "resize.weight", p + "resize.bias", c, 2, e->re[i].resize));
        if (i == 3) RC(pack_conv3(e, p + "resize.weight", p + "resize.bias", c, c, e->re[i].resize));
        RC(pack_conv3(e, "neck.convs." + std::to_string(i) + ".weight", "", F, c, e->re[i].conv));
    }
    for (int i = 0; i < 4; ++i) {
        std::string p = "neck.fusion_stage.layers." + std::to_string(i) + ".";
        RC(pack_linear(e, p + "projection.weight", p + "projection.bias", F, F, e->fu[i].proj));
        RC(pack_conv3(e, p + "residual_layer1.convolution1.weight", p + "residual_layer1.convolution1.bias", F, F, e->fu[i].r1c1));
        RC(pack_conv3(e, p + "residual_layer1.convolution2.weight", p + "residual_layer1.convolution2.bias", F, F, e->fu[i].r1c2));
        RC(pack_conv3(e, p + "residual_layer2.convolution1.weight", p + "residual_layer2.convolution1.bias", F, F, e->fu[i].r2c1));
        RC(pack_conv3(e, p + "residual_layer2.convolution2.weight", p + "residual_layer2.convolution2.bias", F, F, e->fu[i].r2c2));
    }
    RC(pack_conv3(e, "head.conv1.weight", "head.conv1.bias", F / 2, F, e->head1));
    RC(pack_conv3(e, "head.conv2.weight", "head.conv2.bias", d.head_hidden, F / 2, e->head2));
    RC(upload_f32(e, "head.conv3.weight", d.head_hidden, &e->w3));
    { const HostT* b3 = find(e, "head.conv3.bias"); if (!b3) return D2S_E_MISSING; e->b3 = b3->data[0]; }
    // ---- workspaces
    const size_t M = (size_t)B * N, Mp = (size_t)B * P;
    RC(dev_alloc(e, (void**)&e->resid, M * D * 4));
    RC(dev_alloc(e, &e->lnbuf, M * D * es));
    const size_t lnstats_bytes = (size_t)(D / 16 + 1) * M * 2 * sizeof(float);
    if (e->lnf || e->fp8) RC(dev_alloc(e, (void**)&e->lnstats, lnstats_bytes));
    RC(dev_alloc(e, &e->qkv, M * 3 * D * es));
    RC(dev_alloc(e, &e->vt, (size_t)B * D * e->g.Npad * es, true));     // zero beyond N, never written there
    RC(dev_alloc(e, &e->attn, M * D * es));
    RC(dev_alloc(e, &e->mlp, M * d.mlp * es));
    RC(dev_alloc(e, &e->patchA, Mp * e->patch.Kpad * es, true));        // (zero: the padding columns are never written again)
    for (int i = 0; i < 4; ++i) {
        RC(dev_alloc(e, &e->tapbuf[i], Mp * D * es));
        RC(dev_alloc(e, &e->rproj[i], Mp * d.neck[i] * es));
        RC(dev_alloc(e, &e->rres[i], (size_t)B * e->g.fH[i] * e->g.fW[i] * d.neck[i] * es));
        RC(dev_alloc(e, &e->feat[i], (size_t)B * e->g.fH[i] * e->g.fW[i] * F * es));
    }
    for (int i = 0; i < 5; ++i) RC(dev_alloc(e, &e->scr[i], e->g.scr_elems * es));
    // (+ GEMM_PART_CTR_WORDS zeroed words BEHIND the partials: the ping-pong kernel's tail counters, which no split-K launch can reach)
    RC(dev_alloc(e, (void**)&e->splitk_ws, (e->g.splitk_elems + GEMM_PART_CTR_WORDS) * 4, true));
    // side stream of the neck branches (D2S_NO_OVERLAP=1 keeps everything on the caller's stream)
    for (int i = 0; i < 3; ++i) RC(dev_alloc(e, &e->r1[i], (size_t)B * e->g.fH[i] * e->g.fW[i] * F * es));
    RC(dev_alloc(e, &e->r1tmp, (size_t)B * e->g.fH[0] * e->g.fW[0] * F * es));
    RC(dev_alloc(e, (void**)&e->splitk_ws_side, (e->g.splitk_elems + GEMM_PART_CTR_WORDS) * 4, true));
    e->overlap = env_int("D2S_NO_OVERLAP", 0) == 0;
    e->side_sync = env_int("D2S_SIDE_SYNC", 1) != 0;
    if (e->overlap) {
        D2S_HIP(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
        for (int i = 0; i < 4; ++i) D2S_HIP(hipEventCreateWithFlags(&e->ev_tap[i], hipEventDisableTiming));
        for (int i = 0; i < 4; ++i) D2S_HIP(hipEventCreateWithFlags(&e->ev_ln[i], hipEventDisableTiming));
        D2S_HIP(hipEventCreateWithFlags(&e->ev_side, hipEventDisableTiming));
    }
    // a LayerNorm operand pair per side tap (tap_ln_pair) for the engines whose frames can fold a side tap's projection: the precision
    // folds there (bf16), any max_batch reaches batch 1, and the side stream exists
    if (e->side_sync && e->overlap && e->lnf && pr.ln_folds(D2S_LIN_NECK_PROJ))
        for (int i = 0; i < (d.temporal ? 4 : 3); ++i) {
            RC(dev_alloc(e, &e->tap_ln[i], M * D * es));
            RC(dev_alloc(e, (void**)&e->tap_stats[i], lnstats_bytes));
        }
    if (d.temporal) {
        // ---- Video-Depth-Anything temporal modules (reference dpt_temporal.py:50-60): layer_3, layer_4, path_4, path_3
        size_t sc_max = 0, max_sites = 0;
        e->tm_fold = pr.ln_folds(D2S_LIN_TM_KVQ) && env_int("D2S_VDA_FUSE", 1) != 0;
        for (int m = 0; m < 4; ++m) {
            d2s_engine::TMod& t = e->tm[m];
            t.C = e->g.tmC[m]; t.sites = e->g.tmS[m];
            max_sites = std::max(max_sites, (size_t)t.sites);
            const int C = t.C;
            sc_max = std::max(sc_max, (size_t)t.sites * C);
            std::string p = "head.motion_modules." + std::to_string(m) + ".temporal_transformer.";
            std::string b = p + "transformer_blocks.0.";
            RC(upload_f32(e, p + "norm.weight", C, &t.gn_g)); RC(upload_f32(e, p + "norm.bias", C, &t.gn_b));
            RC(pack_linear(e, p + "proj_in.weight", p + "proj_in.bias", C, C, t.proj_in));
            RC(pack_linear(e, p + "proj_out.weight", p + "proj_out.bias", C, C, t.proj_out));
            // sinusoidal APE over the 32-frame window (motion_module.py:214-222), float32 like torch
            std::vector<float> pe((size_t)32 * C);
            for (int i = 0; i < C / 2; ++i) {
                float div = expf((float)(2 * i) * (float)(-std::log(10000.0) / C));
                for (int pos = 0; pos < 32; ++pos) { pe[(size_t)pos * C + 2 * i] = sinf((float)pos * div); pe[(size_t)pos * C + 2 * i + 1] = cosf((float)pos * div); }
            }
            for (int a = 0; a < 2; ++a) {
                std::string q = b + "attention_blocks." + std::to_string(a) + ".";
                const std::string nm = b + "norms." + std::to_string(a);
                RC(upload_f32(e, nm + ".weight", C, &t.ln_g[a]));
                RC(upload_f32(e, nm + ".bias", C, &t.ln_b[a]));
                const char* const kvq_err = "to_q/to_k/to_v: wrong shape";
                const float* kvq[3] = {host_f32(e, q + "to_k.weight", (size_t)C * C, kvq_err), host_f32(e, q + "to_v.weight", (size_t)C * C, kvq_err),
                                       host_f32(e, q + "to_q.weight", (size_t)C * C, kvq_err)};      // fused rows: k | v | q (no biases)
                if (!kvq[0] || !kvq[1] || !kvq[2]) return D2S_E_MISSING;
                auto kvq_at = [&](int n, int k) { return kvq[n / C][(size_t)(n % C) * C + k]; };
                RC(build_forms(e, t.kvq[a], 3 * C, C, kvq_at, nullptr, e->tm_fold, host_vec(e, nm + ".weight", C), host_vec(e, nm + ".bias", C)));
                // W (x + pe_j) = W x + W pe_j: the positional share of every window position, float32
                std::vector<float> pt((size_t)32 * 3 * C);
                for (int j = 0; j < 32; ++j)
                    for (int n = 0; n < 3 * C; ++n) {
                        const float* wr = kvq[n / C] + (size_t)(n % C) * C;
                        double acc = 0.0;
                        for (int k = 0; k < C; ++k) acc += (double)pe[(size_t)j * C + k] * (double)wr[k];
                        pt[(size_t)j * 3 * C + n] = (float)acc;
                    }
                RC(dev_alloc(e, (void**)&t.ptab[a], pt.size() * 4));
                D2S_HIP(hipMemcpy(t.ptab[a], pt.data(), pt.size() * 4, hipMemcpyHostToDevice));
                RC(pack_linear(e, q + "to_out.0.weight", q + "to_out.0.bias", C, C, t.to_out[a]));
                t.ring_bytes = (size_t)31 * t.sites * 2 * C * es;
                RC(dev_alloc(e, &t.cache[a], (size_t)B * t.ring_bytes, true));
            }
            RC(upload_f32(e, b + "ff_norm.weight", C, &t.ffn_g)); RC(upload_f32(e, b + "ff_norm.bias", C, &t.ffn_b));
            RC(pack_linear(e, b + "ff.net.0.proj.weight", b + "ff.net.0.proj.bias", 8 * C, C, t.ff1.form(false, false)));
            RC(pack_linear(e, b + "ff.net.2.weight", b + "ff.net.2.bias", C, 4 * C, t.ff2));
            if (e->tm_fold) {
                const float *g = host_vec(e, b + "ff_norm.weight", C), *bt = host_vec(e, b + "ff_norm.bias", C),
                            *w1p = host_vec(e, b + "ff.net.0.proj.weight", (size_t)8 * C * C), *b1 = host_vec(e, b + "ff.net.0.proj.bias", 8 * C);
                if (!g || !bt || !w1p || !b1) return D2S_E_MISSING;
                // GEGLU in the epilogue (ACT_GEGLU): packed row n' = 8 g + w holds x row 4 g + w (w < 4) or gate row 4C + 4 g + (w - 4)
                auto orig = [C](int n) { return geglu_row(n, C); };
                std::vector<float> b1p((size_t)8 * C);
                for (int n = 0; n < 8 * C; ++n) b1p[n] = b1[orig(n)];
                RC(upload_linear(e, prepare_linear(e->wprec, 8 * C, C, [&](int n, int k) { return w1p[(size_t)orig(n) * C + k]; }, b1p.data(), g, bt),
                                 t.ff1.form(false, true), true));
            }
        }
        sc_max *= (size_t)B; max_sites *= (size_t)B;      // every row of a call runs through the same workspaces
        e->tm_slot.assign(B, d2s_engine::TSlot());
        e->ema_slot_init.assign(B, 0);
        if (e->tm_fold) RC(dev_alloc(e, (void**)&e->tm_stats, (size_t)17 * max_sites * 2 * sizeof(float)));
        RC(dev_alloc(e, (void**)&e->tm_hs, sc_max * 4));
        RC(dev_alloc(e, &e->tm_a, sc_max * es)); RC(dev_alloc(e, &e->tm_out, sc_max * es));
        RC(dev_alloc(e, &e->tm_kv, sc_max * 3 * es));                  // k' | v' | q' of the current frame
        RC(dev_alloc(e, &e->tm_u, sc_max * 8 * es)); RC(dev_alloc(e, &e->tm_g, sc_max * 4 * es));
    }
    e->host.clear();
    RC(dev_alloc(e, (void**)&e->pre_x, (size_t)B * 3 * h * w * 4));
    RC(dev_alloc(e, (void**)&e->depth_small, (size_t)B * h * w * 4));
    RC(dev_alloc(e, (void**)&e->depth_post, (size_t)B * h * w * 4));
    e->post_ws_bytes = d2s_post_process_workspace(B, h, w);
    RC(dev_alloc(e, &e->post_ws, e->post_ws_bytes));
    RC(dev_alloc(e, (void**)&e->ema_state, (size_t)(d.temporal ? B : 1) * h * w * 4));
    if (e->taps) RC(dev_alloc(e, (void**)&e->tap_hidden, (size_t)(d.layers + 1) * N * D * 4));
    D2S_HIP(hipDeviceSynchronize());
    e->finalized = true;
    return D2S_OK;
}

extern "C" int d2s_engine_destroy(d2s_engine* e) {
    if (!e) return D2S_OK;
    D2S_ON_DEVICE(e->device);
    if (e->side) (void)hipStreamSynchronize(e->side);
    for (int i = 0; i < 4; ++i) if (e->ev_tap[i]) (void)hipEventDestroy(e->ev_tap[i]);
    for (int i = 0; i < 4; ++i) if (e->ev_ln[i]) (void)hipEventDestroy(e->ev_ln[i]);
    if (e->ev_side) (void)hipEventDestroy(e->ev_side);
    if (e->side) (void)hipStreamDestroy(e->side);
    for (void* p : e->allocs) (void)hipFree(p);
    delete e;
    return D2S_OK;
}

extern "C" int d2s_engine_memory(const d2s_engine* e, uint64_t* bytes) {
    D2S_REQUIRE(e && bytes, "null pointer");
    *bytes = e->bytes;
    return D2S_OK;
}

namespace {
// the stream slot of every batch row of a call (e->row_ids), checked before anything is launched
int resolve_streams(d2s_engine* e, int batch, const int* stream_ids) {
    if (!e->d.temporal) {
        D2S_REQUIRE(!stream_ids, "stream_ids on an engine that is not a Video-Depth-Anything engine: its batch rows are not streams");
        return D2S_OK;
    }
    uint32_t seen = 0;
    for (int r = 0; r < batch; ++r) {
        const int id = stream_ids ? stream_ids[r] : r;
        if (id < 0 || id >= e->maxB) { set_error("stream id " + std::to_string(id) + " out of range: the engine has " + std::to_string(e->maxB) + " stream slot(s)"); return D2S_E_INVALID; }
        if (seen >> id & 1u) { set_error("stream id " + std::to_string(id) + " named twice in one call"); return D2S_E_INVALID; }
        seen |= 1u << id;
    }
    for (int r = 0; r < batch; ++r) e->row_ids[r] = stream_ids ? stream_ids[r] : r;
    return D2S_OK;
}
}  // namespace

extern "C" int d2s_model_forward_streams(d2s_engine* e, const float* x, float* depth, int batch, const int* stream_ids, void* stream) {
    D2S_REQUIRE(e && x && depth, "null pointer");
    if (!e->finalized) { set_error("d2s_model_forward before d2s_engine_finalize"); return D2S_E_STATE; }
    D2S_REQUIRE(batch >= 1 && batch <= e->maxB, "batch exceeds max_batch");
    RC(resolve_streams(e, batch, stream_ids));
    D2S_ON_DEVICE(e->device);
    return forward(e, x, depth, batch, (hipStream_t)stream);
}

extern "C" int d2s_model_forward(d2s_engine* e, const float* x, float* depth, int batch, void* stream) {
    return d2s_model_forward_streams(e, x, depth, batch, nullptr, stream);
}

extern "C" int d2s_forward_plan(const d2s_model_desc* desc, int h, int w, int batch, int flags, d2s_forward_plan_result* res) {
    D2S_REQUIRE(desc && res, "null pointer");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_forward_plan_result), "d2s_forward_plan_result.struct_size must be sizeof(d2s_forward_plan_result)");
    RC(check_desc(desc));
    RC(check_shape(*desc, h, w, batch));
    const d2s_model_desc& d = *desc;
    const PrecRules pr = prec_rules(d.precision);
    // the state of an engine created and finalised now (d2s_engine_create, d2s_engine_finalize), in the situation the flags name
    FrameState s = {};
    s.calib = (flags & D2S_PLAN_CALIBRATING) != 0; s.fp8_ready = (flags & D2S_PLAN_CALIBRATED) != 0; s.prof = (flags & D2S_PLAN_PROFILING) != 0;
    s.taps = env_int("D2S_TAPS", 0) != 0; s.side = env_int("D2S_NO_OVERLAP", 0) == 0; s.no_lnfuse = env_int("D2S_NO_LNFUSE", 0) != 0;
    s.tm_fold = d.temporal && pr.ln_folds(D2S_LIN_TM_KVQ) && env_int("D2S_VDA_FUSE", 1) != 0;
    D2S_REQUIRE(!s.calib || (pr.e4m3 && !d.temporal), "D2S_PLAN_CALIBRATING: not a D2S_PREC_FP8 engine (or a Video-Depth-Anything engine)");
    const EngineGeom g = engine_geom(d, h, w, batch);
    ForwardPlan pl;
    RC(plan_forward(d, g, h, w, batch, s, pl));
    d2s_forward_plan_result r = {};
    r.struct_size = sizeof(r);
    r.f8 = pl.f8; r.f8a = pl.f8a; r.x3 = pl.x3; r.lnf = pl.lnf; r.pp_fold = pl.pp_fold; r.tap_fold = pl.tap_fold; r.use_side = pl.use_side;
    r.ln_slots[0] = pl.slots_proj; r.ln_slots[1] = pl.slots_fc2;
    const int e4a = pl.f8a ? D2S_PLAN_E4M3 : 0, e4 = pl.f8 ? D2S_PLAN_E4M3 : 0;
    r.site[D2S_PLAN_SITE_QKV0] = e4a;
    r.site[D2S_PLAN_SITE_QKV] = e4a | (pl.ln1_folded ? D2S_PLAN_FOLDED : 0);
    r.site[D2S_PLAN_SITE_PROJ] = e4a | (pl.lnf ? D2S_PLAN_STATS : 0);
    r.site[D2S_PLAN_SITE_FC1] = e4 | (pl.ln2_folded ? D2S_PLAN_FOLDED : 0);
    r.site[D2S_PLAN_SITE_FC2] = e4 | (pl.fc2_stats ? D2S_PLAN_STATS : 0);
    r.site[D2S_PLAN_SITE_FC2_LAST] = e4 | (pl.fc2_stats_last ? D2S_PLAN_STATS : 0);
    for (int i = 0; i < 4; ++i) { r.site[D2S_PLAN_SITE_NECK0 + i] = pl.tap_folded ? D2S_PLAN_FOLDED : 0; r.tap_side[i] = pl.tap_side[i]; }
    r.head1_ups = pl.head1_ups; r.head2_fused = pl.head2_fused; r.head2_ups = pl.head2_ups; r.bn = pl.bn;
    r.tm_fold = s.tm_fold;
    r.tm_cache_store = d.temporal && !(s.tm_fold && (flags & D2S_PLAN_WINDOW_FILLED));       // (window_rows: fused and filled rows store in-kernel)
    for (int m = 0; m < 4; ++m)
        for (int j = 0; j < 3; ++j) { r.tm_slots[m][j] = pl.tm[m].slots[j]; r.tm_folded[m][j] = pl.tm[m].folded[j]; }
    r.gh = g.gh; r.gw = g.gw; r.P = g.P; r.N = g.N; r.Npad = g.Npad;
    for (int i = 0; i < 4; ++i) { r.fH[i] = g.fH[i]; r.fW[i] = g.fW[i]; r.tm_C[i] = d.temporal ? g.tmC[i] : 0; r.tm_sites[i] = d.temporal ? g.tmS[i] : 0; }
    r.ln_launches = pl.ln_launches;
    for (int i = 0; i < 4; ++i)
        r.rcu_fused |= (pl.rcu_fused[i] ? 1 << i : 0) | (pl.rcu1_fused[i] ? 256 << i : 0) | (pl.rcu_wide[i] ? 1 << (16 + i) : 0) | (pl.rcu1_wide[i] ? 1 << (24 + i) : 0);
    r.splitk_elems = g.splitk_elems; r.scr_elems = g.scr_elems;
    *res = r;
    return D2S_OK;
}

extern "C" int d2s_engine_calibrate(d2s_engine* e, const float* x, int batch, void* stream) {
    D2S_REQUIRE(e && x, "null pointer");
    if (!e->finalized) { set_error("d2s_engine_calibrate before d2s_engine_finalize"); return D2S_E_STATE; }
    D2S_REQUIRE(e->fp8, "d2s_engine_calibrate: not a D2S_PREC_FP8 engine");
    D2S_REQUIRE(batch >= 1 && batch <= e->maxB && !e->d.temporal, "bad batch (or a Video-Depth-Anything engine)");
    D2S_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    const int L = e->d.layers;
    // one bf16 forward over the calibration frames, recording max |activation| at the four quantisation sites per layer
    D2S_HIP(hipMemsetAsync(e->amax, 0, (size_t)L * NSITE * sizeof(float), st));
    const bool prof = e->prof_on;
    e->prof_on = false;
    e->calib = true;
    int rc = forward(e, x, e->depth_small, batch, st);
    e->calib = false;
    e->prof_on = prof;
    if (rc != D2S_OK) return rc;
    // headroom over the calibration frames' maxima (D2S_FP8_HEADROOM, default 1: later frames with larger activations
    // saturate at +-448 instead of wrapping; 1.25-1.5 trades a fraction of a bit of resolution for that margin)
    static const float headroom = getenv("D2S_FP8_HEADROOM") ? std::max(1.0f, (float)atof(getenv("D2S_FP8_HEADROOM"))) : 1.0f;
    std::vector<float> am((size_t)L * NSITE);
    D2S_HIP(hipMemcpyAsync(am.data(), e->amax, am.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    D2S_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < L; ++l) {
        Layer& ly = e->L[l];
        for (int s = 0; s < NSITE; ++s) {
            float a = am[(size_t)l * NSITE + s];
            if (!(a > 0.f) || !std::isfinite(a)) { set_error("d2s_engine_calibrate: degenerate activation range"); return D2S_E_INVALID; }
            e->act_scale[(size_t)l * NSITE + s] = a * headroom / FP8_MAX;
        }
        for (int i = 0; i < 4; ++i)                           // every e4m3 form: deq from the scale of the site that feeds it (CALIB_SITE)
            for (int folded = 0; folded < 2; ++folded) {
                const DevLinear& W = ly.lin(i).form(true, folded);
                const CalibSite cs = CALIB_SITE[i][folded];
                if (!W.w || l + cs.dlayer < 0) continue;
                const std::vector<float> dq = deq_scales(e->act_scale[(size_t)(l + cs.dlayer) * NSITE + cs.site], W.sw);
                D2S_HIP(hipMemcpy(W.deq, dq.data(), dq.size() * sizeof(float), hipMemcpyHostToDevice));
            }
    }
    e->fp8_ready = true;
    return D2S_OK;
}

extern "C" int d2s_engine_reset_stream(d2s_engine* e) {
    D2S_REQUIRE(e, "null engine");
    e->ema_init = 0;
    for (auto& sl : e->tm_slot) sl = d2s_engine::TSlot();     // VDA: drop every temporal window (a slot's next frame re-seeds it)
    for (auto& i : e->ema_slot_init) i = 0;
    return D2S_OK;
}

extern "C" int d2s_engine_reset_stream_at(d2s_engine* e, int stream_id) {
    D2S_REQUIRE(e, "null engine");
    const int slots = e->d.temporal ? (int)e->tm_slot.size() : 1;       // (not a temporal engine: one EMA state, slot 0)
    if (stream_id < 0 || stream_id >= slots) {
        set_error("d2s_engine_reset_stream_at: stream " + std::to_string(stream_id) + " does not exist (the engine has " + std::to_string(slots) + " slot(s))");
        return D2S_E_INVALID;
    }
    if (!e->d.temporal) { e->ema_init = 0; return D2S_OK; }
    e->tm_slot[stream_id] = d2s_engine::TSlot();
    e->ema_slot_init[stream_id] = 0;
    return D2S_OK;
}

extern "C" int d2s_pipeline(d2s_engine* e, const uint8_t* frames, int batch, int H, int W, int depth_resolution,
                            const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_sbs_params* sp, int use_ema,
                            void* out, int out_fmt, float* depth_full, void* stream) {
    return d2s_pipeline_streams(e, frames, batch, nullptr, H, W, depth_resolution, pre, pp, sp, use_ema, out, out_fmt, depth_full, stream);
}

namespace d2s {      // (dibr.hip, dibr_composite.hip) check_only: every argument check of the entry point, nothing launched
int dibr_warp_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                  void* out, int out_fmt, void* stream, bool check_only);
int dibr_composite_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                       int composite, void* out, int out_fmt, void* stream, bool check_only);
int dibr_warp_crop_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                       const double* crop, void* out, int out_fmt, void* stream, bool check_only);
}

namespace {
// d2s_pipeline_streams and d2s_view_pipeline_streams are one call up to and including the EMA step; they differ in the warp that
// reads e->depth_post.  pipeline_check: every refusal of that shared part (nothing is launched); *stride: the decimation of the
// pre-process.  pipeline_depth: frames -> e->depth_post at model resolution (+ depth_full, predict_depth's return value).
int pipeline_check(d2s_engine* e, int batch, const int* stream_ids, int H, int W, int depth_resolution, const d2s_pre_params* pre, int* stride_out) {
    if (!e->finalized) { set_error("d2s_pipeline before d2s_engine_finalize"); return D2S_E_STATE; }
    D2S_REQUIRE(batch >= 1 && batch <= e->maxB, "batch exceeds max_batch");
    RC(resolve_streams(e, batch, stream_ids));
    // model-input shape of this frame size must be the engine's (reference: fixed at first frame, depth.py:1951-1953)
    D2S_REQUIRE(H > 0 && W > 0 && depth_resolution > 0, "bad frame shape");
    int longest = H > W ? H : W;
    int stride = 1;
    if (pre && pre->square) {
        // fixed-square branch (get_patch_size() is None: CAPTURE_MODE == "Window", reference depth.py:531-538, 1937-1946)
        if (e->h != depth_resolution || e->w != depth_resolution) {
            set_error("d2s_pipeline: the fixed-square branch needs a depth_resolution x depth_resolution engine"); return D2S_E_INVALID;
        }
    } else {   // _resize_patch_aligned_t integer logic (reference depth.py:677-689); Python round() = half-to-even
        double scale = longest != depth_resolution ? (double)depth_resolution / (double)longest : 1.0;
        int sh = std::max(1, (int)nearbyint(H * scale)), sw = std::max(1, (int)nearbyint(W * scale));
        auto nm = [&](int x) { int p = e->d.patch, down = (x / p) * p, up = down + p; return (std::abs(up - x) <= std::abs(x - down)) ? up : down; };
        if (std::max(1, nm(sh)) != e->h || std::max(1, nm(sw)) != e->w) {
            set_error("d2s_pipeline: frame maps to a model-input shape different from the engine's"); return D2S_E_INVALID;
        }
        stride = longest / (depth_resolution * 2);
        if (stride < 1) stride = 1;
    }
    *stride_out = stride;
    return D2S_OK;
}

int pipeline_depth(d2s_engine* e, const uint8_t* frames, int batch, int H, int W, int stride, const d2s_pre_params* pre,
                   const d2s_post_params* pp, int use_ema, float* depth_full, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    {   // pre-process straight into the patch rows where that form exists (bilinear branch), else planes + the engine's patchify
        const bool fused = !e->taps && preprocess_patches_ok(e->prec, D2S_FMT_U8_HWC, pre, H, W, e->h, e->w, e->d.patch, e->patch.Kpad);
        if (fused) PROF(PC_PRE, 0, (double)batch * ((double)H * W * 3 + (double)e->h * e->w * 6),
                        launch_preprocess_patches(e->prec, frames, D2S_FMT_U8_HWC, batch, H, W, stride, pre, e->patchA, e->h, e->w, e->d.patch, e->patch.Kpad,
                                                  e->cls, e->pos, e->resid, e->g.N, e->d.hidden, st));
        if (!fused) PROF(PC_PRE, 0, (double)batch * ((double)H * W * 3 + (double)e->h * e->w * 12), d2s_preprocess(frames, D2S_FMT_U8_HWC, batch, H, W, e->pre_x, e->h, e->w, stride, pre, stream));
        RC(forward(e, fused ? nullptr : e->pre_x, e->depth_small, batch, st));
    }
    // post-process out of place (raw model output -> depth_post): few frames take the one-launch form (post.hip)
    PROF(PC_POST, 0, 0, d2s_post_process_to(e->depth_small, e->depth_post, batch, e->h, e->w, pp, e->post_ws, e->post_ws_bytes, stream));
    if (use_ema && e->d.temporal) {                      // one state per stream slot: a row continues (or starts) its own
        EmaRows tab = {};
        for (int r = 0; r < batch; ++r) tab.r[r] = EmaRow{e->row_ids[r], e->ema_slot_init[e->row_ids[r]]};
        RC(ema_rows(e->depth_post, e->ema_state, batch, tab, e->h * e->w, pp->ema_alpha, st));
        for (int r = 0; r < batch; ++r) e->ema_slot_init[e->row_ids[r]] = 1;
    } else if (use_ema) {
        RC(ema_batch(e->depth_post, e->ema_state, e->ema_init, batch, e->h * e->w, pp->ema_alpha, st));
        e->ema_init = 1;
    }
    if (depth_full) RC(d2s_upsample_depth(e->depth_post, batch, e->h, e->w, depth_full, H, W, stream));
    return D2S_OK;
}
}  // namespace

extern "C" int d2s_pipeline_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W, int depth_resolution,
                                    const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_sbs_params* sp, int use_ema,
                                    void* out, int out_fmt, float* depth_full, void* stream) {
    D2S_REQUIRE(e && frames && pp && sp && out, "null pointer");
    int stride = 1;
    RC(pipeline_check(e, batch, stream_ids, H, W, depth_resolution, pre, &stride));
    D2S_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    RC(pipeline_depth(e, frames, batch, H, W, stride, pre, pp, use_ema, depth_full, stream));
    {
        int oh = 0, ow = 0;
        RC(d2s_sbs_shape(H, W, sp, &oh, &ow));
        double obytes = (double)oh * ow * 3 * (out_fmt == D2S_FMT_U8_HWC ? 1 : 4);
        PROF(PC_WARP, 0, batch * ((double)H * W * 3 + (double)e->h * e->w * 4 + obytes),
             d2s_make_sbs(frames, D2S_FMT_U8_HWC, e->depth_post, e->h, e->w, batch, H, W, sp, out, out_fmt, stream));
    }
    return D2S_OK;
}

// d2s_view_pipeline_streams (crop == nullptr) and d2s_view_pipeline_crop_streams: one code path, the warp differs
static int view_pipeline_any(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W, int depth_resolution,
                             const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp, int view, const double* crop,
                             int use_ema, void* out, int out_fmt, float* depth_full, void* stream) {
    D2S_REQUIRE(frames && pp && dp && out, "null pointer");
    D2S_REQUIRE(view >= -1 && view <= D2S_COMPOSITE_DEPTH_MAP, "bad view (-1: the stereo warp, or D2S_COMPOSITE_*)");
    D2S_REQUIRE(!crop || view == -1, "bad view with a crop (the composites are not an OpenXR path: view must be -1)");
    D2S_REQUIRE(dp->struct_size == sizeof(d2s_dibr_params), "d2s_dibr_params.struct_size must be sizeof(d2s_dibr_params) = 80");
    // what depends on the frame and the uniforms alone (display mode / viewport), then the engine
    int oh = 0, ow = 0;
    RC(crop ? d2s_dibr_crop_shape(H, W, crop, dp->display_mode, &oh, &ow)
            : view < 0 ? d2s_dibr_shape(H, W, dp->display_mode, &oh, &ow) : d2s_dibr_composite_shape(H, W, dp, view, &oh, &ow));
    D2S_REQUIRE(e, "null engine");
    int stride = 1;
    RC(pipeline_check(e, batch, stream_ids, H, W, depth_resolution, pre, &stride));
    // the warp's own refusals (struct_size, viewport, formats, limits) before anything is launched
    auto warp = [&](bool check_only) {
        if (crop) return dibr_warp_crop_any(frames, e->depth_post, e->h, e->w, batch, H, W, dp, crop, out, out_fmt, stream, check_only);
        return view < 0 ? dibr_warp_any(frames, e->depth_post, e->h, e->w, batch, H, W, dp, out, out_fmt, stream, check_only)
                        : dibr_composite_any(frames, e->depth_post, e->h, e->w, batch, H, W, dp, view, out, out_fmt, stream, check_only);
    };
    RC(warp(true));
    D2S_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    RC(pipeline_depth(e, frames, batch, H, W, stride, pre, pp, use_ema, depth_full, stream));
    const int nch = dp->alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    const double obytes = (double)oh * ow * nch * (out_fmt == D2S_FMT_U8_HWC ? 1 : 4);
    const double ibytes = view == D2S_COMPOSITE_DEPTH_MAP ? 0.0 : (double)H * W * 3;
    PROF(PC_WARP, 0, batch * (ibytes + (double)e->h * e->w * 4 + obytes), warp(false));
    return D2S_OK;
}

extern "C" int d2s_view_pipeline_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W, int depth_resolution,
                                         const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp, int view, int use_ema,
                                         void* out, int out_fmt, float* depth_full, void* stream) {
    return view_pipeline_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, view, nullptr, use_ema, out, out_fmt, depth_full, stream);
}

extern "C" int d2s_view_pipeline_crop_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                              int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                              const d2s_dibr_params* dp, int view, const double* crop, int use_ema, void* out, int out_fmt,
                                              float* depth_full, void* stream) {
    D2S_REQUIRE(crop, "null pointer (crop)");
    return view_pipeline_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, view, crop, use_ema, out, out_fmt, depth_full, stream);
}

// d2s_view_pipeline_crop_streams with the OpenXR eye views (d2s_dibr_xr_eyes) as the last stage: the same checks and depth path
// (d2s_view_pipeline_xr_glow_streams: the same call with the glow; glow == nullptr is d2s_view_pipeline_xr_streams;
//  curved: d2s_view_pipeline_xr_glow_curved_streams, whose last stage is d2s_dibr_xr_eyes_glow_curved)
static int view_pipeline_xr_any(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels, void* stream,
                                int entry, const d2s_xr_frost* frost = nullptr, const d2s_xr_panorama* pano = nullptr,
                                const uint8_t* pano_rgb = nullptr, const uint8_t* pano_levels = nullptr) {
    D2S_REQUIRE(frames && pp && dp && out && screen && eyes, "null pointer");
    D2S_REQUIRE(dp->struct_size == sizeof(d2s_dibr_params), "d2s_dibr_params.struct_size must be sizeof(d2s_dibr_params) = 80");
    uint64_t offs[2], total = 0;
    RC(d2s_dibr_xr_shape(eyes, n_eyes, batch > 0 ? batch : 1, dp->alpha_mode, offs, &total));
    D2S_REQUIRE(e, "null engine");
    int stride = 1;
    RC(pipeline_check(e, batch, stream_ids, H, W, depth_resolution, pre, &stride));
    auto warp = [&](bool check_only) {
        return dibr_xr_entry_any(entry, frames, e->depth_post, e->h, e->w, batch, H, W, dp, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                                 workspace_bytes, glow, frost, levels, stream, check_only, pano, pano_rgb, pano_levels);
    };
    RC(warp(true));
    D2S_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    RC(pipeline_depth(e, frames, batch, H, W, stride, pre, pp, use_ema, depth_full, stream));
    const double obytes = (double)total / batch * (out_fmt == D2S_FMT_U8_HWC ? 1 : 4);
    PROF(PC_WARP, 0, batch * ((double)H * W * 3 + (double)e->h * e->w * 4 + obytes), warp(false));
    return D2S_OK;
}

extern "C" int d2s_view_pipeline_xr_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                            int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                            const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                            const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                            void* workspace, uint64_t workspace_bytes, void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, nullptr, nullptr, stream, D2S_XR_ENTRY_EYES);
}

extern "C" int d2s_view_pipeline_xr_glow_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                 int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                 const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                 const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                                 void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels,
                                                 void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, glow, levels, stream, D2S_XR_ENTRY_GLOW);
}

// the engine's pipeline up to the EMA step, then d2s_dibr_xr_eyes_glow_curved on the model-resolution depth
extern "C" int d2s_view_pipeline_xr_glow_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                        int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                        const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                        const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt,
                                                        float* depth_full, void* workspace, uint64_t workspace_bytes,
                                                        const d2s_xr_glow* glow, const uint8_t* levels, void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, glow, levels, stream, D2S_XR_ENTRY_GLOW_CURVED);
}

// the engine's pipeline up to the EMA step, then d2s_dibr_xr_eyes_frost on the model-resolution depth
extern "C" int d2s_view_pipeline_xr_frost_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                  int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                  const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                  const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                                  void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                                  void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, nullptr, levels, stream, XR_ENTRY_FROST, frost);
}

// the engine's pipeline up to the EMA step, then d2s_dibr_xr_eyes_frost_curved on the model-resolution depth
extern "C" int d2s_view_pipeline_xr_frost_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                         int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                         const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                         const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt,
                                                         float* depth_full, void* workspace, uint64_t workspace_bytes,
                                                         const d2s_xr_frost* frost, const uint8_t* levels, void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, nullptr, levels, stream, XR_ENTRY_FROST_CURVED, frost);
}

// the engine's pipeline up to the EMA step, then d2s_dibr_xr_eyes_panorama on the model-resolution depth
extern "C" int d2s_view_pipeline_xr_panorama_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                     int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                     const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                     const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                                     void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                                     const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                                                     const uint8_t* pano_levels, void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, glow, levels, stream, XR_ENTRY_PANORAMA, frost, pano, pano_rgb,
                                pano_levels);
}

// the same with d2s_dibr_xr_eyes_panorama_curved as the last stage: the panorama also behind the curved screen's looks
extern "C" int d2s_view_pipeline_xr_panorama_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                            int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                            const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                            const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt,
                                                            float* depth_full, void* workspace, uint64_t workspace_bytes,
                                                            const d2s_xr_frost* frost, const uint8_t* levels, const d2s_xr_glow* glow,
                                                            const d2s_xr_panorama* pano, const uint8_t* pano_rgb, const uint8_t* pano_levels,
                                                            void* stream) {
    return view_pipeline_xr_any(e, frames, batch, stream_ids, H, W, depth_resolution, pre, pp, dp, crop, screen, eyes, n_eyes, use_ema, out,
                                out_fmt, depth_full, workspace, workspace_bytes, glow, levels, stream, XR_ENTRY_PANORAMA_CURVED, frost, pano,
                                pano_rgb, pano_levels);
}

extern "C" int d2s_engine_tap(d2s_engine* e, const char* name, float* out, uint64_t out_elems, int* rows, int* cols, void* stream) {
    D2S_REQUIRE(e && name && out && rows && cols, "null pointer");
    if (!e->finalized || e->last_batch == 0) { set_error("d2s_engine_tap: no forward pass yet"); return D2S_E_STATE; }
    D2S_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    std::string n(name);
    const int D = e->d.hidden, F = e->d.fusion;
    if (n == "embeddings" || n.rfind("layer", 0) == 0) {
        if (!e->taps) { set_error("hidden-state taps need D2S_TAPS=1 at engine creation"); return D2S_E_STATE; }
        int l = n == "embeddings" ? 0 : atoi(n.c_str() + 5);
        D2S_REQUIRE(l >= 0 && l <= e->d.layers, "bad layer index");
        *rows = e->g.N; *cols = D;
        D2S_REQUIRE(out_elems >= (uint64_t)e->g.N * D, "tap buffer too small");
        D2S_HIP(hipMemcpyAsync(out, e->tap_hidden + (size_t)l * e->g.N * D, (size_t)e->g.N * D * 4, hipMemcpyDeviceToDevice, st));
        return D2S_OK;
    }
    if (n.rfind("neck_feat", 0) == 0) {
        int i = atoi(n.c_str() + 9);
        D2S_REQUIRE(i >= 0 && i < 4, "bad neck index");
        *rows = e->g.fH[i] * e->g.fW[i]; *cols = F;
        D2S_REQUIRE(out_elems >= (uint64_t)(*rows) * F, "tap buffer too small");
        return launch_to_f32(e->prec, e->feat[i], out, (long)(*rows) * F, st);
    }
    set_error("unknown tap: " + n);
    return D2S_E_INVALID;
}

extern "C" int d2s_engine_profile(d2s_engine* e, int enable) {
    D2S_REQUIRE(e, "null engine");
    e->prof_on = enable != 0;
    e->prof_recs.clear();
    e->prof_used = 0;
    return D2S_OK;
}

extern "C" int d2s_engine_profile_read(d2s_engine* e, int max_classes, double* ms, double* flops, double* bytes,
                                       int64_t* launches, int* n_classes) {
    D2S_REQUIRE(e && ms && flops && bytes && launches && n_classes && max_classes >= PC_N, "bad argument");
    D2S_ON_DEVICE(e->device);
    for (int c = 0; c < PC_N; ++c) { ms[c] = 0; flops[c] = 0; bytes[c] = 0; launches[c] = 0; }
    const bool dump = env_int("D2S_PROF_DUMP", 0) != 0;     // tuning aid: one line per recorded launch on stderr
    int idx = 0;
    for (auto& r : e->prof_recs) {
        D2S_HIP(hipEventSynchronize(r.b));
        float t = 0.f;
        D2S_HIP(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.cls] += t; flops[r.cls] += r.flops; bytes[r.cls] += r.bytes; launches[r.cls] += 1;
        if (dump)
            fprintf(stderr, "[d2s-prof] %4d %-12s %8.2f us %9.3f GF %7.1f TF/s\n", idx, PC_NAMES[r.cls], t * 1e3, r.flops * 1e-9,
                    t > 0.f ? r.flops / (t * 1e-3) * 1e-12 : 0.0);
        ++idx;
    }
    *n_classes = PC_N;
    return D2S_OK;
}

extern "C" const char* d2s_profile_class_name(int cls) { return cls >= 0 && cls < PC_N ? PC_NAMES[cls] : ""; }
