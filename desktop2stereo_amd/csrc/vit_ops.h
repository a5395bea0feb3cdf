// Launchers of the non-GEMM model kernels (vit_ops.hip, attention.hip).
#pragma once
#include "common.h"

namespace d2s {

int launch_patchify(int prec, const float* x, void* A, int B, int h, int w, int p, int Kp,
                    const float* cls, const float* pos, float* resid, int N, int D, hipStream_t st);   // also writes the cls rows
// d2s_pipeline: pre-process + patchify in one launch (frame_ops.hip); D2S_E_UNSUPPORTED = not eligible, nothing launched
bool preprocess_patches_ok(int prec, int fmt, const d2s_pre_params* pre, int H, int W, int h, int w, int p, int Kp);
int launch_preprocess_patches(int prec, const void* frames, int fmt, int batch, int H, int W, int decim_stride, const d2s_pre_params* pre,
                              void* A, int h, int w, int p, int Kp, const float* cls, const float* pos, float* resid, int N, int D, hipStream_t st);
// The output type launch_layernorm writes for (engine precision, e4m3 scale, unit-format flag): the one place that decision is made;
// the launcher switches on it and d2s_temporal_probe names the kernel by it.
enum LnOut { LN_OUT_F32, LN_OUT_BF16, LN_OUT_BX3, LN_OUT_E4M3 };
LnOut layernorm_out_type(int prec, float fp8_qscale, bool bx3_out);
const char* layernorm_kernel_name(LnOut t);              // "layernorm_kernel<f32 | bf16 | bx3 | e4m3>"
int launch_layernorm(int prec, const float* x, const float* g, const float* b, void* out, int rows_out, int D, float eps,
                     int rows_per_img, int img_rows, int row_off, hipStream_t st, float fp8_qscale = 0.f,   // > 0: e4m3 output
                     bool bx3_out = false);                                                     // fp32 engines: the bf16x3 unit format
int launch_amax(int prec, const void* x, long n, float* slot, hipStream_t st);       // *slot = max(*slot, max |x|); fp8 calibration
int launch_bilinear_nhwc(int prec, const void* in, void* out, int B, int Hi, int Wi, int Ho, int Wo, int C, hipStream_t st,
                         const void* addend = nullptr);    // out = upsample(in) [+ addend]
int launch_head_final(int prec, const void* x, const float* w3, float b3, float max_depth, float* depth, long npix, int C, hipStream_t st);
int launch_to_f32(int prec, const void* in, float* out, long n, hipStream_t st);

// Multi-head self-attention over the fused QKV activation [B*N, 3*D] (q | k | v, head-major inside
// each), head_dim 64: out[B*N, D] = softmax(q k^T / 8) v.  (HF Dinov2SelfAttention.forward)
// vt: V transposed [B, heads, 64, Npad] (Npad = N rounded up to 64, zero beyond N), see MAP_QKV in gemm.h.
// fp8_qscale > 0 (bf16 inputs only): out is e4m3 = sat(result * fp8_qscale), the A operand of an fp8 output projection.
// prescaled: the q third of qkv already carries ATTN_SCALE_LOG2E (bf16 / fp8 engines fold it into W_q and b_q: one rounding, and
// the batched kernel gets log2-domain scores straight from the matrix pipe); false: the kernel applies it (fp32 parity class).
constexpr float ATTN_SCALE_LOG2E = 0.125f * 1.4426950408889634f;          // 64^-0.5 * log2(e)
// Plans the launch (attention.hip plan_attention: host arithmetic on (prec, e4m3 output, B heads, N) picks one row of the file's
// instance list, its grid and scales) and launches that plan; an unsupported combination is an error, nothing is launched.
int launch_attention(int prec, const void* qkv, const void* vt, void* out, int B, int N, int Npad, int heads, hipStream_t st,
                     float fp8_qscale = 0.f, bool prescaled = false);

// Video-Depth-Anything temporal-module kernels (temporal.hip)
// x, out [rows][sites, C]: one normalisation per (row, group)
// Which GroupNorm kernel a call runs: the register kernel groupnorm_reg_kernel<T, cpg, rpt> for an even channels-per-group of the model
// zoo (2, 4, 6, 8, 12, 16, 24, 32), rpt = 1 | 2 | 4 sites per thread (up to 4096 sites; 4 only while cpg <= 24: 96 values per thread),
// else -- and with D2S_GN_OLD=1 -- the general groupnorm_kernel<T>.  plan_name: e.g. "groupnorm_reg_kernel<bf16,CPG=8,RPT=2>",
// "groupnorm_kernel<f32>" (the tests pin the dispatch with it; not built on the launch path).
struct GnPlan { bool reg; int cpg, rpt; };
GnPlan plan_groupnorm(int prec, int sites, int C, int groups);
void plan_name(const GnPlan& p, int prec, char* buf, size_t n);
int launch_groupnorm(int prec, const void* x, const float* g, const float* b, void* out, int sites, int C, int groups, float eps, hipStream_t st,
                     int rows = 1);
// cur [rows][S][3C] = k' | v' | q' of this frame, batch row r = the next frame of one stream; that stream's ring [slots][S][2C] = k' | v' of
// its past frames; ptab [32][3C] = pe @ W^T.  What differs per row travels BY VALUE in the kernel arguments -- TA_MAX_ROWS entries of
// 16 bytes -- so a call needs no upload and no extra launch.
constexpr int TA_MAX_ROWS = D2S_MAX_STREAMS;
struct AttnRow { void* ring; int16_t head, Tw; int32_t store_slot; };      // the stream's ring, its oldest slot, window 1 | 32, slot to fill or -1
struct AttnRows { AttnRow r[TA_MAX_ROWS]; };
struct CacheRow { void* ring; int32_t slot0, nslots; };                    // ring[slot0 .. slot0 + nslots) = this row's k' | v' rows (nslots 0: none)
struct CacheRows { CacheRow r[TA_MAX_ROWS]; };
struct EmaRow { int32_t slot, initialised; };
struct EmaRows { EmaRow r[TA_MAX_ROWS]; };
static_assert(sizeof(AttnRow) == 16 && sizeof(CacheRow) == 16, "row tables are 16 bytes per row");
int launch_cache_store(int prec, const void* cur, int sites, int C, int rows, const CacheRows& tab, hipStream_t st);
// The attention instance of a call: ch = channels per lane (8 when the head dimension C / 8 is a multiple of 8, else 4), lpu = lanes per
// (site, head) unit (the power of two >= head_dim / ch), table = several rows (WinTable; one row: WinRow).  plan_name: e.g.
// "temporal_attn_kernel<bf16,CH=8,WinTable>" (lpu is a run-time argument of the kernel, not part of the instance).
struct TattPlan { int ch, lpu; bool table; };
TattPlan plan_temporal_attn(int prec, int C, int rows);
void plan_name(const TattPlan& p, int prec, char* buf, size_t n);
int launch_temporal_attn(int prec, const void* cur, const float* ptab, void* out, int sites, int C, int slots, int rows,
                         const AttnRows& tab, hipStream_t st);
int launch_geglu(int prec, const void* u, void* g, long rows, int C4, hipStream_t st);
int launch_cast_f32(int prec, const float* in, void* out, long n, hipStream_t st);

// engine-internal (post.hip)
int ema_batch(float* depth, float* state, int initialised, int nframes, int hw, float alpha, hipStream_t st);
// one EMA state per stream slot: row r of depth [rows][hw] updates state[tab.r[r].slot][hw] (started by it when not initialised)
int ema_rows(float* depth, float* state, int rows, const EmaRows& tab, int hw, float alpha, hipStream_t st);

}  // namespace d2s
