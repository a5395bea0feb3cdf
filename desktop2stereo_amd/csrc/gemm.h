// MFMA GEMM with implicit-conv A loader and fused epilogues (gemm.hip).
//   C[m, n] = epilogue( sum_k A[m, k] * W[n, k] )          W packed [Npad][Kpad], K contiguous
#pragma once
#include "common.h"
#include <hip/hip_ext.h>
#include <cstring>

namespace d2s {

enum { A_PLAIN = 0, A_CONV3 = 1 };
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2,
       ACT_GEGLU = 3 };   // out[m, c] = x[m, c] * gelu(gate[m, c]) with the weight rows interleaved x0-3 | g0-3 | x4-7 | g4-7 ...: N/2 output columns
                           // (gemm_glds_kernel only: the exchange relies on its lane <-> column map, gemm_epi.h)
enum { MAP_ROWS = 0, MAP_SHUFFLE = 1, MAP_QKV = 2, MAP_HEAD = 3 };
enum { OUT_T = 0, OUT_F32 = 1, OUT_BF16 = 2, OUT_BX3 = 3 };   // OUT_T: operand type (fp8 operands: e4m3 of v * out_qscale; bf16x3: fp32)
                                                            // OUT_BX3 (bf16x3 launches): the unit format, A operand of the next linear

constexpr int D2S_PREC_FP8_OPERANDS = D2S_PREC_FP8;   // as a GEMM precision: e4m3 operands (A and W), fp32 accumulate
// D2S_PREC_BF16X3 as a GEMM precision: A is fp32 in memory (split into bf16 hi + lo on its way into LDS), W is packed in the
// bf16x3 unit format (gemm_epi.h), outputs / residuals of type OUT_T are fp32

struct GemmA {
    const void* ptr;      // T*
    int mode;             // A_PLAIN / A_CONV3
    long lda;             // A_PLAIN: row stride (elements)
    int Hi, Wi, C;        // A_CONV3: input NHWC [B,Hi,Wi,C], 3x3, pad 1
    int Ho, Wo, stride;   //          output grid, conv stride
    int relu;             // max(x,0) on load (pre-activation)
    int buf;              // set by the launcher (plain linears with whole K tiles, < 2 GiB operands): LDS-DMA through buffer descriptors
    int bx3;              // D2S_PREC_BF16X3 launches: A is ALREADY in the split unit format (plain rows): LDS-DMA tiles; 0: fp32, split when staged
    // A_CONV3 with the align_corners bilinear up-sample in front of it folded into the halo loader (the LDS-resident-input kernels; the
    // caller asks conv3_upsample_ok first): ptr = the SOURCE map [B, Hs, Ws, C], (Hi, Wi) = the up-sampled size the conv sees
    int ups, Hs, Ws;
    float usy, usx;       // linear_scale(Hs, Hi, true), linear_scale(Ws, Wi, true)
};

constexpr int GEMM_PART_CTR_WORDS = 256;   // counter words behind GemmEpi::part's part_elems partials (gemm_pp.hip: 4 per tail tile)
struct GemmEpi {
    void* out;
    int out_type;         // OUT_T: same type as the operands; OUT_F32
    long ldc;             // MAP_ROWS: row stride of out (elements)
    const float* bias;    // [N] or null
    const float* scale;   // [N] LayerScale or null: v = scale * (acc + bias)
    int act;
    const void* res1;     // residual(s), type = out type, added after scale/act
    const void* res2;
    // row mapping (MAP_ROWS): out_row = (m / rows_per_img) * img_rows + (m % rows_per_img) + row_off
    int rows_per_img, img_rows, row_off;   // rows_per_img == 0 -> out_row = m
    int res1_mod, res1_off;                // res1 row = res1_mod ? (m % res1_mod) + res1_off : out_row; ld = ldc
    // MAP_SHUFFLE (ConvTranspose k == s): m -> (b, y, x) over [B, gh, gw]; n -> (ky, kx, co)
    int map, gh, gw, ks, cout;
    // MAP_QKV: row-major [M, 3D] for q | k; the v third goes TRANSPOSED to vt[B, heads, 64, npad]
    // (m = b*ntok + t, n - 2D = h*64 + d) so the attention kernel reads V^T rows with 16-byte chunks.
    void* vt; int ntok, npad, qk_cols, heads;
    // split-K workspace (optional): fp32 partials [ksplit][M][N]; ksplit is chosen by the launcher.  The owner allocates
    // part_elems + GEMM_PART_CTR_WORDS words: the words behind the partials are gemm_pp's tail-tile counters (zero between launches)
    float* part; size_t part_elems; int ksplit;
    // MAP_HEAD: out = float depth[M]; bias = conv2 bias, scale = conv3 weights [N], head_b3 = conv3 bias
    float head_b3;
    float head_max_depth;                  // 0: ReLU; > 0: sigmoid * max_depth (metric head)
    // fp8 operands: acc is in units of (activation scale * weight scale[n]); deq[n] = s_act * s_w[n] turns it back
    // into real values before bias.  out_qscale = 1 / s_out for an e4m3 output (OUT_T with fp8 operands).
    const float* deq;
    float out_qscale;
    // LayerNorm folded into the linears either side of it (bf16 encoder; DESIGN.md §3.1 "LayerNorm fusion").
    // Producer (OUT_F32, MAP_ROWS -- the residual update): every stored value also goes to out2 as bf16 (same offsets),
    // and each block writes the (sum v, sum v^2) of its BN columns for every row: stats_out[column block][M][2]; the
    // launcher reports the number of column blocks through stats_slots (host int; the consumer takes at most 16).
    void* out2; float* stats_out; int* stats_slots;
    float out2_qscale;                            // 0: out2 is bf16; > 0: out2 is e4m3 of v * out2_qscale (the e4m3 encoder path)
    int out2_bx3;                                 // bf16x3 engines: out2 is the pre-split unit format (A operand of the LN-folded consumer)
    // Consumer: A rows are the RAW bf16 residual and W is gamma-folded, so LN(x) W = rstd * (x W' - mean * colsum(W'));
    // the kernel applies v = rstd[m] * (acc - mean[m] * ln_csum[n]) before bias (bias already holds b + W beta).
    const float* ln_stats; int ln_slots; const float* ln_csum; float ln_eps; int ln_dim;
    int ln_M;                                     // rows per slot of ln_stats when it is not this GEMM's M (0: M)
};

// precision: D2S_PREC_FP32 (T = float) / D2S_PREC_BF16 (T = bf16) / D2S_PREC_FP8_OPERANDS (T = e4m3).  tile: 0 = auto.
// stop (optional): an event that completes when the launch -- its last kernel -- has finished.  gemm_glds_kernel and the ping-pong kernel
// hand it to the dispatch itself (D2S_LAUNCH_STOP: the kernel's own completion signal, no marker packet behind it); behind the other
// families it is recorded on st.
int launch_gemm(int precision, int tile, const GemmA& a, const void* W, int M, int N, int K, int Kpad,
                const GemmEpi& e, hipStream_t st, hipEvent_t stop = nullptr);
// a kernel launch on st whose completion is the event `stop`; stop == nullptr: the plain launch
#define D2S_LAUNCH_STOP(stop, kernel, grid, block, st, ...)                                                            \
    do {                                                                                                               \
        if (stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, nullptr, stop, 0, __VA_ARGS__);                    \
        else hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                                              \
    } while (0)

// would launch_gemm fold the up-sample a.ups describes into this convolution's halo loader? (engine: skip the bilinear launch)
bool conv3_upsample_ok(int precision, int tile, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e);

// smallest number of 256 x 256 tiles from which plain linears go to the ping-pong kernel (D2S_GEMM_PP; 0 = never)
int gemm_pp_min_tiles();

// What launch_gemm runs, decided on the host before anything is launched (plan_gemm, gemm.hip): the kernel family and the entry of
// that family's instantiation table, its grid, and everything the launch sets up around it.  The family launchers start a plan as is.
enum { GEMM_GLDS = 0, GEMM_HALO = 1, GEMM_CONV3 = 2, GEMM_PP = 3, GEMM_SK = 4 };   // gemm_glds_kernel, conv3_halo_kernel, conv3.hip, gemm_pp, gemm_sk
enum { NOTE_TAIL_NONE = 0, NOTE_TAIL_INKERNEL = 1, NOTE_TAIL_TWO_LAUNCH = 2, NOTE_TAIL_ROWSPLIT = 3 };
struct GemmPlan {
    int family, inst;            // GEMM_*, entry of the family's table
    const char* name;            // the instantiation, as the probes report it
    int tile;                    // gemm_glds_kernel: the tile code the dispatch settled on; ping-pong kernel: 256256; 0 otherwise
    unsigned grid, gridy;        // blocks (gridy: split-K ranges of gemm_glds_kernel, column groups of gemm_sk_kernel)
    int block;                   // threads per block
    unsigned grid2;              // blocks of the second launch (splitk_reduce_kernel, pp_tail_reduce_kernel); 0: none
    int xn;                      // the tile map's XCD grid (pick_xn); the persistent conv3.hip kernels: their tile count
    int buf;                     // GemmA::buf of the launch (descriptor-addressed operands)
    int ksplit, tail;            // split-K ranges (gemm_glds_kernel) or units per tail tile (ping-pong kernel); NOTE_TAIL_*
    int stats_slots;             // what *e.stats_slots receives (LayerNorm statistics partials per row); -1: left unwritten
    int ups;                     // the up-sample a.ups describes is folded into the loader
    int kps, tw, ink, lxn, skew_us;   // ping-pong kernel: K tiles per unit, whole-tile units, tail mode, log2(xn), start skew
    const char* error;           // plan_gemm failed: the message launch_gemm reports
};
// INVARIANT: plan_gemm and everything under it (plan_glds, plan_halo, plan_conv3_halo2, pp_supported / plan_gemm_pp, sk_supported /
// plan_gemm_sk) read the pointers of GemmA / GemmEpi for PRESENCE only (e.part, e.stats_out, e.stats_slots, e.out2, e.deq, e.res1, ...;
// and whether e.res1 == e.out), never their value or alignment, and the scales (out_qscale, out2_qscale) for their sign only.  The
// frame's plan (forward_plan.h plan_forward) relies on it: it asks about a launch with a placeholder address in every pointer.
int plan_gemm(int precision, int tile, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p);

// the families outside gemm.hip: eligibility / plan (host only) and the launcher of a plan
bool plan_conv3_halo2(const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p);   // stride-1 3x3 convs, input in LDS
void launch_conv3_halo2(const GemmPlan& p, const GemmA& a, const void* W, int M, int N, int Kpad, const GemmEpi& e, hipStream_t st);
// A fusion stage's residual unit on a small map as one launch (conv3.hip conv3_rcu_kernel): out = x + conv2(relu(conv1(relu(x)))),
// and with wp the stage's 1x1 projection of that; bf16, C = 128, weights as pack_conv3 / pack_linear leave them.  c3_rcu_ok: the
// geometry rule (every block resident at once); which engines ask is plan_forward's (forward_plan.h).
struct RcuOp {
    const void* x; void* out;            // [nimg, H, W, 128] bf16
    int nimg, H, W;
    const void *w1, *w2, *wp;            // conv1, conv2 [256][Kpad]; the projection [256][KpadP] or null
    const float *b1, *b2, *bp;           // [128] each (bp with wp)
    int Kpad, KpadP;
};
bool c3_rcu_ok(bool plain_bf16, int C, int nimg, int H, int W);
bool c3_rcu_wide_fits(bool plain_bf16, int C, int nimg, int H, int W);   // the wide form (8 x 8-pixel tiles): its own residency
bool c3_rcu_wide_ok(bool plain_bf16, int C, int nimg, int H, int W);     // ... and the plan's rule: c3_rcu_ok refuses, the wide form fits
bool plan_conv3_rcu(bool plain_bf16, int C, int nimg, int H, int W, bool proj, bool wide, GemmPlan& p);
void launch_conv3_rcu(const GemmPlan& p, const RcuOp& o, hipStream_t st);
// 256 x 256 ping-pong kernel (gemm_pp.hip): batched plain linears
bool pp_supported(int precision, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e);
int plan_gemm_pp(int precision, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p);
int launch_gemm_pp(const GemmPlan& p, int precision, const GemmA& a, const void* W, int M, int N, int K, int Kpad, const GemmEpi& e, hipStream_t st,
                   hipEvent_t stop = nullptr);
// streaming kernel for the thin linears of the DPT neck (gemm_sk.hip: K <= 256, W tile resident in LDS, A streamed)
bool sk_supported(int precision, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e);
void plan_gemm_sk(const GemmA& a, int M, int N, int K, GemmPlan& p);
void launch_gemm_sk(const GemmPlan& p, const GemmA& a, const void* W, int M, int N, int Kpad, const GemmEpi& e, hipStream_t st);

// Which kernel the last launch_gemm of this host thread ran: launch_gemm records its plan (host side only, a few stores), and only
// the probes (d2s_conv3_probe, d2s_linear_probe) read it -- the tests pin the dispatch with it.  tile: the implicit-GEMM tile code
// the plan settled on (0 for the other kernels); ksplit > 1: split-K partials + splitk_reduce_kernel (gemm_glds_kernel), or the
// ping-pong kernel's tail tiles cut into ksplit units, tail = how they are finished.
struct KernelNote { const char* name; int tile; int ksplit; int tail; };
KernelNote& kernel_note();

// tile of the fused head launch: MAP_HEAD needs a tile whose waves own all N columns of their rows (WN == 1)
static inline int head_tile(int bn) { return bn == 32 ? 912832 : 9256648; }

// Conv2d 3x3 weight [Co, Ci, 3, 3] in K order: element k = tap * Ci + ci (tap = ky * 3 + kx) of packed row n
static inline size_t conv3_weight_index(int n, int k, int Ci) { const int tap = k / Ci, ci = k % Ci; return ((size_t)n * Ci + ci) * 9 + tap; }

// packed-weight geometry
static inline size_t elem_size(int precision) { return precision == D2S_PREC_BF16 ? 2 : (precision == D2S_PREC_FP8_OPERANDS ? 1 : 4); }   // fp32, bf16x3: 4
// host-side packing of one bf16x3 weight row: element k of a row lives in unit k / 8
static inline void bx3_pack_elem(uint8_t* row, int k, float v) {
    const bf16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
    uint8_t* u = row + (size_t)(k >> 3) * 32 + (k & 7) * 2;
    memcpy(u, &hi, 2); memcpy(u + 16, &lo, 2);
}
static inline int gemm_bk(int precision) { return 128 / (int)elem_size(precision); }   // 128-byte K tile
static inline int gemm_kpad(int K, int precision) { int bk = 2 * gemm_bk(precision); return (K + bk - 1) / bk * bk; }   // 256-byte multiple
static inline int gemm_npad(int N) { return (N + 255) / 256 * 256; }

}  // namespace d2s
