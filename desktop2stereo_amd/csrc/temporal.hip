// Video-Depth-Anything temporal modules (streaming, one frame per call) -- A17 in SURVEY.md section 8a.
//   TemporalTransformer3DModel.forward   reference motion_module/motion_module.py:102-134
//   TemporalTransformerBlock.forward     :164-196
//   TemporalAttention.forward            :242-321   (q = current frame, k/v = 31 cached + current, APE by window index)
//   FeedForward / GEGLU                  motion_module/attention.py:296-384
//   cache update                         vda2_s.py:177-187, 203-218
// Activations are NHWC = [sites, C] token matrices, so every Linear is the engine's MFMA GEMM; this file
// holds the small kernels around them: GroupNorm, the 32-key attention per (spatial site, head) reading the
// ring-buffer window of projected K'/V' rows, GEGLU, and the ring store (the reference shift-copies the whole
// cache of hidden states every frame and re-projects all 32 window positions; here the oldest slot of projected
// rows is overwritten in place and only the new frame is projected).
#include "vit_ops.h"
#include <algorithm>
#include <cstdio>
#include <type_traits>

namespace d2s {

template <typename T> __device__ __forceinline__ T tcvt(float v);
template <> __device__ __forceinline__ float tcvt<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t tcvt<bf16_t>(float v) { return f2bf(v); }
__device__ __forceinline__ float tf(float v) { return v; }
__device__ __forceinline__ float tf(bf16_t v) { return bf2f(v); }

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;
}

// nn.GroupNorm(32 groups, eps) on NHWC maps [rows][sites, C]: one block per (group, row), two-pass statistics (mean, then the sum of squared
// deviations) over values that STAY IN REGISTERS.  Round 4's kernel took 16 us for 2-9 k elements: three passes of scalar bf16 loads in a
// run-time loop, every load waited for before the next was issued (rocprofv3, profiles/r5_04) -- 64 us of a 1.06 ms VDA frame.  Here a
// thread owns whole sites (the group's cpg channels of a site are contiguous: one 8 / 16-byte aligned vector load per chunk), all of a
// thread's loads are issued before the first is used (compile-time unroll), and the normalised values are written from the registers.
// CPG = channels per group (2, 4, 6, 8, 12, 16, 24, 32 for the model zoo: C / 32), RPT = sites per thread.
template <typename T, int CPG, int RPT>
__global__ void __launch_bounds__(1024)
groupnorm_reg_kernel(const T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, T* __restrict__ out,
                     int sites, int C, float eps) {
    __shared__ float red[16];
    const int c0 = blockIdx.x * CPG, tid = threadIdx.x;
    x += (long)blockIdx.y * sites * C; out += (long)blockIdx.y * sites * C;      // blockIdx.y: the row (stream) of a batched call -- statistics never cross rows
    float v[RPT][CPG];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int s_ = tid + r * 1024;
        const T* p = x + (long)(s_ < sites ? s_ : 0) * C + c0;
#pragma unroll
        for (int c = 0; c < CPG; c += 2) {                            // (CPG is even; 4-byte loads are aligned for any even c0)
            if constexpr (std::is_same<T, float>::value) { const float2 t = *(const float2*)(p + c); v[r][c] = t.x; v[r][c + 1] = t.y; }
            else { const uint32_t t = *(const uint32_t*)(p + c); v[r][c] = __uint_as_float(t << 16); v[r][c + 1] = __uint_as_float(t & 0xffff0000u); }
        }
    }
    auto bsum = [&](float a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = a;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i];
        return t;
    };
    const float n = (float)sites * (float)CPG;
    float s1 = 0.f;
#pragma unroll
    for (int r = 0; r < RPT; ++r)
        if (tid + r * 1024 < sites) {
#pragma unroll
            for (int c = 0; c < CPG; ++c) s1 += v[r][c];
        }
    const float mu = bsum(s1) / n;
    float s2 = 0.f;
#pragma unroll
    for (int r = 0; r < RPT; ++r)
        if (tid + r * 1024 < sites) {
#pragma unroll
            for (int c = 0; c < CPG; ++c) { const float d = v[r][c] - mu; s2 += d * d; }
        }
    const float rstd = 1.0f / sqrtf(bsum(s2) / n + eps);
    float gg[CPG], bb[CPG];
#pragma unroll
    for (int c = 0; c < CPG; ++c) { gg[c] = g[c0 + c]; bb[c] = b[c0 + c]; }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int s_ = tid + r * 1024;
        if (s_ < sites) {
            T* q = out + (long)s_ * C + c0;
#pragma unroll
            for (int c = 0; c < CPG; ++c) q[c] = tcvt<T>((v[r][c] - mu) * rstd * gg[c] + bb[c]);
        }
    }
}

// (general shapes: the round-1 kernel, one block per group, three strided passes)
template <typename T>
__global__ void __launch_bounds__(256)
groupnorm_kernel(const T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b, T* __restrict__ out,
                 int sites, int C, int groups, float eps) {
    __shared__ float red[4];
    const int cpg = C / groups, c0 = blockIdx.x * cpg;
    x += (long)blockIdx.y * sites * C; out += (long)blockIdx.y * sites * C;
    const int n = sites * cpg;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += tf(x[(long)(i / cpg) * C + c0 + i % cpg]);
    const float mu = block_sum(s, red) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { float d = tf(x[(long)(i / cpg) * C + c0 + i % cpg]) - mu; q += d * d; }
    const float rstd = 1.0f / sqrtf(block_sum(q, red) / (float)n + eps);
    for (int i = threadIdx.x; i < n; i += 256) {
        int c = c0 + i % cpg;
        long off = (long)(i / cpg) * C + c;
        out[off] = tcvt<T>((tf(x[off]) - mu) * rstd * g[c] + b[c]);
    }
}

// The window caches hold the PROJECTED rows K' = W_k x, V' = W_v x of the past 31 frames (x = the normed hidden state,
// without the positional encoding): the reference projects (x_j + pe_j) for all 32 window positions every frame
// (motion_module.py:288-300), but the projection is linear, W (x + pe_j) = W x + W pe_j, and W pe_j is a constant
// 32 x 3C table per attention block.  So a frame projects only its own rows (one [S, C] x [C, 3C] GEMM instead of
// [32 S, C] x [C, 2C]), and the attention adds the table rows on the fly.

// ring[slot][s][0:2C] = cur[s][0:2C] for slot in [slot0, slot0 + nslots); cur rows are 3C wide (k | v | q).  blockIdx.y = batch row: row r
// copies its k' | v' rows of cur [rows][S][3C] into slots [slot0, slot0 + nslots) of ITS stream's ring -- 31 slots for a stream's first
// frame, one (or none) otherwise.  The table travels by value in the kernel arguments and is read with a block-uniform index.
template <typename T>
__global__ void __launch_bounds__(256)
cache_store_rows_kernel(const T* __restrict__ cur, int sites, int C, const CacheRows tab) {
    const CacheRow r = tab.r[blockIdx.y];
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int C2 = 2 * C;
    const long per = (long)sites * C2;
    if (idx >= per * r.nslots) return;
    const long q = idx % per;
    ((T*)r.ring)[(long)r.slot0 * per + idx] = cur[((long)blockIdx.y * sites + q / C2) * 3 * C + q % C2];
}

template <int CH> __device__ __forceinline__ void load_ch(const float* p, float v[CH]) {
#pragma unroll
    for (int i = 0; i < CH; i += 4) { float4 t = *(const float4*)(p + i); v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w; }
}
template <int CH> __device__ __forceinline__ void load_ch(const bf16_t* p, float v[CH]) {
#pragma unroll
    for (int i = 0; i < CH; i += 4) {
        uint2 t = *(const uint2*)(p + i);
        v[i] = __uint_as_float(t.x << 16); v[i + 1] = __uint_as_float(t.x & 0xffff0000u);
        v[i + 2] = __uint_as_float(t.y << 16); v[i + 3] = __uint_as_float(t.y & 0xffff0000u);
    }
}
// a row segment of CH values kept RAW (as loaded) until it is used: CH * sizeof(T) / 4 registers
template <typename T, int CH> struct RawSeg {
    static constexpr int W = CH * (int)sizeof(T) / 4;
    uint32_t w[W];
    __device__ __forceinline__ void load(const T* p) {
        if constexpr (W == 2) { const uint2 t = *(const uint2*)p; w[0] = t.x; w[1] = t.y; }
        else {
#pragma unroll
            for (int i = 0; i < W; i += 4) { const uint4 t = *(const uint4*)((const uint32_t*)p + i); w[i] = t.x; w[i + 1] = t.y; w[i + 2] = t.z; w[i + 3] = t.w; }
        }
    }
    __device__ __forceinline__ float get(int i) const {
        if constexpr (std::is_same<T, float>::value) return __uint_as_float(w[i]);
        else return (i & 1) ? __uint_as_float(w[i >> 1] & 0xffff0000u) : __uint_as_float(w[i >> 1] << 16);
    }
};

// One (site, head) UNIT = LPU x KG lanes: LPU (2..16, power of two >= head_dim / CH) lanes own one CH-channel chunk of the head each,
// KG = 4 key groups own 8 of the 32 window positions each.  Every K' / V' row segment of a head is read once, coalesced (head_dim *
// sizeof(T) contiguous bytes per key); score partials are xor-reduced over the unit's channel lanes, softmax statistics and the output
// over its key groups (lanes LPU and 2 LPU apart).
// cur [rows][S][3C] (k' | v' | q' of this frame; row r is the next frame of ONE stream), that stream's ring [slots][S][2C] (k' | v' of
// its past frames, oldest at `head`), ptab [32][3C] float = pe @ [W_k | W_v | W_q]^T.  Window position j < Tw-1 is ring slot
// (head + j) % slots, j = Tw-1 the current frame (reference motion_module.py:259-300: q from the last position, k / v from all).
// out [rows][S][C]; units = rows * S * 8.
// Round 5.  Round 4's kernel gave a lane all 32 keys: ~3 500 instructions per lane (32 x 2 row addresses with an integer modulo each,
// 32 x 3 shuffles, fully unrolled), ONE 4-wave block per CU (194 blocks for a ViT-B stream) -- 19-28 us per launch, 8 launches per
// frame, and the time did not move when its ring requests were batched 8 / 16 / 32 at a time (variant builds, gpurun_out/r5j): it was
// bound by its own instruction stream at one wave per SIMD, not by the rings' latency.  Splitting the keys over lanes gives 4 x the
// threads with ~1/7 of the instructions each: all 16 ring segments of a lane are requested up front, 3+ waves per SIMD cover them.
constexpr int TA_KG = 4, TA_KPG = 8;           // key groups per unit, keys per group (TA_KG * TA_KPG = the 32-frame window)

// Where a lane's window lives.  A Win travels BY VALUE in the kernel arguments (no upload, no dependent launch) and maps a lane's site
// over all rows, gs, to its row's entry -- ring, oldest slot, window length (1 for a stream's first frame, else 32), store slot (-1: none)
// -- and the site s inside that row.
struct WinRow {                                // a call of one row: the entry is wave-uniform, no divide, no table read
    AttnRow r;
    __device__ __forceinline__ AttnRow at(int gs, int, int& s) const { s = gs; return r; }
};
// Several rows: looked up PER LANE -- a 256-thread block usually straddles two rows, and a wave does whenever upl = 16 (C <= 64) and the
// site count is odd.  A unit never straddles rows, so every shuffle stays inside one row's lanes; a fresh row (Tw = 1) beside a warm
// one (Tw = 32) differs in masks and addresses only -- no branch encloses a shuffle.
struct WinTable {
    AttnRows t;
    __device__ __forceinline__ AttnRow at(int gs, int sites, int& s) const {
        const int row = gs / sites;                                // row < rows <= TA_MAX_ROWS for every lane (dead lanes: row 0)
        s = gs - row * sites;
        return t.r[row];
    }
};

template <typename T, int CH, typename Win>
__global__ void __launch_bounds__(256)
temporal_attn_kernel(const T* __restrict__ cur, const float* __restrict__ ptab, T* __restrict__ out,
                     int sites, int C, int slots, float scale, int lpu, int units, const Win win) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int upl = lpu * TA_KG;                                   // lanes per unit (<= 64: a unit never straddles a wave)
    const int unit = gid / upl, sub = gid % upl, kg = sub / lpu, li = sub % lpu;
    const bool live = unit < units;                                // (no early return: the shuffles below need every lane)
    const int gs = live ? unit >> 3 : 0, h = unit & 7, dh = C >> 3, C2 = 2 * C, C3 = 3 * C;   // gs: site over all rows
    int s;
    const AttnRow ar = win.at(gs, sites, s);
    T* const ring = (T*)ar.ring;
    const int Tw = ar.Tw, head = ar.head, store_slot = ar.store_slot;
    const bool act = live && li * CH < dh;                         // lanes beyond the head's channels only take part in shuffles
    const int c = h * dh + (act ? li * CH : 0);                    // this lane's first channel
    const T* cur_row = cur + (long)gs * C3;
    // this lane's 8 window positions and their rows (32-bit element offsets: a ring is < 2^31 elements, checked by the launcher);
    // positions >= Tw (first frame only: Tw = 1) re-read the last valid row and are masked out of the softmax
    const int slot_stride = sites * C2, base_s = s * C2 + c;
    const T* krow[TA_KPG];
    int jpos[TA_KPG];
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) {
        const int j = kg * TA_KPG + t, jj = min(j, Tw - 1);
        int slot = head + jj; if (slot >= slots) slot -= slots;    // (head < slots, jj < 32 <= slots + 1: one conditional subtract, no modulo)
        if (slot >= slots) slot -= slots;
        krow[t] = (act && jj < Tw - 1) ? ring + (slot * slot_stride + base_s) : cur_row + c;   // (padding / dead lanes never touch the ring: see the store below)
        jpos[t] = jj;
    }
    RawSeg<T, CH> rk[TA_KPG], rv[TA_KPG];
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) rk[t].load(krow[t]);
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) rv[t].load(krow[t] + C);
    float q[CH];
    {
        float pq[CH];
        load_ch<CH>(cur_row + C2 + c, q);
        load_ch<CH>(ptab + (long)(Tw - 1) * C3 + C2 + c, pq);
#pragma unroll
        for (int i = 0; i < CH; ++i) q[i] = act ? q[i] + pq[i] : 0.f;
    }
    float sc[TA_KPG];
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) {
        float pk[CH];
        load_ch<CH>(ptab + (long)jpos[t] * C3 + c, pk);
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) a += q[i] * (rk[t].get(i) + pk[i]);
        for (int o = lpu >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o);
        sc[t] = kg * TA_KPG + t < Tw ? a * scale : -1e30f;
    }
    float mx = -1e30f;
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) mx = fmaxf(mx, sc[t]);
    mx = fmaxf(mx, __shfl_xor(mx, lpu)); mx = fmaxf(mx, __shfl_xor(mx, 2 * lpu));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) { sc[t] = kg * TA_KPG + t < Tw ? __expf(sc[t] - mx) : 0.f; sum += sc[t]; }
    sum += __shfl_xor(sum, lpu); sum += __shfl_xor(sum, 2 * lpu);
    const float inv = 1.0f / sum;
    float acc[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) acc[i] = 0.f;
#pragma unroll
    for (int t = 0; t < TA_KPG; ++t) {
        float pv[CH];
        load_ch<CH>(ptab + (long)jpos[t] * C3 + C + c, pv);
        const float p = sc[t] * inv;                               // 0 for masked positions
#pragma unroll
        for (int i = 0; i < CH; ++i) acc[i] += p * (rv[t].get(i) + pv[i]);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) { acc[i] += __shfl_xor(acc[i], lpu); acc[i] += __shfl_xor(acc[i], 2 * lpu); }
    if (act && kg == 0) {
#pragma unroll
        for (int i = 0; i < CH; ++i) out[(long)gs * C + c + i] = tcvt<T>(acc[i]);
    }
    // round 5: the frame's k' | v' rows join the window HERE, in the row's own ring (the store kernel's launch is gone for every frame but a
    // stream's first).  The oldest slot's segment [c, c + CH) of site s is READ by the key group that owns window position 0 -- kg 0's ACTIVE
    // lane -- and by nobody else (the padding lanes of a head, li * CH >= head_dim, and the lanes of dead units read the current frame's row
    // instead of the ring: their q is 0 and they store nothing, but they used to load this segment too -- an unordered read beside the store,
    // ADVICE r5), so that lane overwrites it once its own two loads of it are behind it: program order within one thread is all the
    // ordering needed.  Rows do not change the argument: a row's lanes touch that row's ring only.
    if (act && kg == 0 && store_slot >= 0) {
        T* dst = ring + ((long)store_slot * slot_stride + base_s);
#pragma unroll
        for (int i = 0; i < CH; ++i) { dst[i] = cur_row[c + i]; dst[C + i] = cur_row[C + c + i]; }
    }
}

// GEGLU: g[r, c] = u[r, c] * gelu_exact(u[r, 4C + c]),  u [rows, 8C] -> g [rows, 4C]
template <typename T>
__global__ void __launch_bounds__(256)
geglu_kernel(const T* __restrict__ u, T* __restrict__ g, long rows, int C4) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * C4) return;
    long r = idx / C4;
    int c = (int)(idx % C4);
    float x = tf(u[r * 2 * C4 + c]), gate = tf(u[r * 2 * C4 + C4 + c]);
    g[idx] = tcvt<T>(x * (0.5f * gate * (1.0f + erff(gate * 0.70710678118654752f))));
}

template <typename T>
__global__ void __launch_bounds__(256)
cast_f32_kernel(const float* __restrict__ in, T* __restrict__ out, long n) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = tcvt<T>(in[idx]);
}

static const char* prec_tag(int prec) { return prec == D2S_PREC_BF16 ? "bf16" : "f32"; }

// groupnorm_reg_kernel's instances: C / 32 of the model zoo (fusion 64 / 128 / 256, neck 192 / 384 / 512 / 768 / 1024) x sites per thread;
// RPT 4 while CPG * 4 <= 96 registers of values
#define D2S_GN_INSTANCES(X) X(2, 1) X(2, 2) X(2, 4) X(4, 1) X(4, 2) X(4, 4) X(6, 1) X(6, 2) X(6, 4) X(8, 1) X(8, 2) X(8, 4) \
    X(12, 1) X(12, 2) X(12, 4) X(16, 1) X(16, 2) X(16, 4) X(24, 1) X(24, 2) X(24, 4) X(32, 1) X(32, 2)

GnPlan plan_groupnorm(int /*prec*/, int sites, int C, int groups) {
    static EnvInt old{"D2S_GN_OLD", 0};                   // A/B aid: round 4's kernel
    GnPlan p{false, C / groups, 0};
    const int need = (sites + 1023) / 1024;               // sites per thread of a 1024-thread block
    const int rpt = need <= 2 ? need : 4;
    if (!old.get() && need <= 4) {
#define D2S_GN(CPG_, RPT_) if (p.cpg == CPG_ && rpt == RPT_) { p.reg = true; p.rpt = rpt; }
        D2S_GN_INSTANCES(D2S_GN)
#undef D2S_GN
    }
    return p;
}
void plan_name(const GnPlan& p, int prec, char* buf, size_t n) {
    if (p.reg) snprintf(buf, n, "groupnorm_reg_kernel<%s,CPG=%d,RPT=%d>", prec_tag(prec), p.cpg, p.rpt);
    else snprintf(buf, n, "groupnorm_kernel<%s>", prec_tag(prec));
}

template <typename T>
static void launch_groupnorm_plan(const GnPlan& p, const void* x, const float* g, const float* b, void* out, int sites, int C, int groups, float eps, int rows, hipStream_t st) {
    if (!p.reg) {
        hipLaunchKernelGGL(groupnorm_kernel<T>, dim3(groups, rows), dim3(256), 0, st, (const T*)x, g, b, (T*)out, sites, C, groups, eps);
        return;
    }
#define D2S_GN(CPG_, RPT_) if (p.cpg == CPG_ && p.rpt == RPT_) hipLaunchKernelGGL((groupnorm_reg_kernel<T, CPG_, RPT_>), dim3(groups, rows), dim3(1024), 0, st, (const T*)x, g, b, (T*)out, sites, C, eps);
    D2S_GN_INSTANCES(D2S_GN)
#undef D2S_GN
}

int launch_groupnorm(int prec, const void* x, const float* g, const float* b, void* out, int sites, int C, int groups, float eps, hipStream_t st, int rows) {
    if (rows < 1 || rows > 65535) { set_error("groupnorm: bad row count"); return D2S_E_INVALID; }
    if (groups < 1 || C % groups) { set_error("groupnorm: C must be a multiple of the group count"); return D2S_E_INVALID; }
    const GnPlan p = plan_groupnorm(prec, sites, C, groups);
    if (prec == D2S_PREC_BF16) launch_groupnorm_plan<bf16_t>(p, x, g, b, out, sites, C, groups, eps, rows, st);
    else launch_groupnorm_plan<float>(p, x, g, b, out, sites, C, groups, eps, rows, st);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

// rows >= 1 batch rows; returns without a launch when no row has slots to fill
int launch_cache_store(int prec, const void* cur, int sites, int C, int rows, const CacheRows& tab, hipStream_t st) {
    if (rows < 1 || rows > TA_MAX_ROWS) { set_error("cache_store: bad row count"); return D2S_E_INVALID; }
    int most = 0;
    for (int r = 0; r < rows; ++r) most = std::max(most, tab.r[r].nslots);
    if (most == 0) return D2S_OK;
    const dim3 grid(cdiv((long)sites * 2 * C * most, 256), rows);
    if (prec == D2S_PREC_BF16) hipLaunchKernelGGL(cache_store_rows_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)cur, sites, C, tab);
    else hipLaunchKernelGGL(cache_store_rows_kernel<float>, grid, dim3(256), 0, st, (const float*)cur, sites, C, tab);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

TattPlan plan_temporal_attn(int /*prec*/, int C, int rows) {
    TattPlan p{(C / 8) % 8 == 0 ? 8 : 4, 1, rows > 1};           // head dim multiple of 8: 16-byte bf16 chunks
    while (p.lpu * p.ch < C / 8) p.lpu <<= 1;                    // lanes per (site, head) unit: power of two >= head_dim / chunk
    return p;
}
void plan_name(const TattPlan& p, int prec, char* buf, size_t n) {
    snprintf(buf, n, "temporal_attn_kernel<%s,CH=%d,%s>", prec_tag(prec), p.ch, p.table ? "WinTable" : "WinRow");
}

int launch_temporal_attn(int prec, const void* cur, const float* ptab, void* out, int sites, int C, int slots, int rows,
                         const AttnRows& tab, hipStream_t st) {
    if (C % 32 || rows < 1 || rows > TA_MAX_ROWS) { set_error("temporal_attn: C % 32 == 0 and 1 <= rows <= 32 required"); return D2S_E_INVALID; }
    for (int r = 0; r < rows; ++r) {
        const AttnRow& a = tab.r[r];
        if (!a.ring || (a.Tw != 1 && a.Tw != 32) || a.head < 0 || a.head >= slots || a.store_slot < -1 || a.store_slot >= slots) {
            set_error("temporal_attn: bad row table"); return D2S_E_INVALID;
        }
    }
    const float scale = 1.0f / sqrtf((float)(C / 8));
    const TattPlan p = plan_temporal_attn(prec, C, rows);
    const int lpu = p.lpu;
    if (lpu * TA_KG > 64) { set_error("temporal_attn: head dim too large"); return D2S_E_UNSUPPORTED; }
    // (per-stream limit: offsets inside ONE ring are 32-bit; rows are reached through 64-bit pointers)
    if ((long)slots * sites * 2 * C >= (1L << 31) || slots < 31) { set_error("temporal_attn: ring too large for 32-bit offsets (or fewer than 31 slots)"); return D2S_E_UNSUPPORTED; }
    if ((long)rows * sites * 8 * lpu * TA_KG >= (1L << 31)) { set_error("temporal_attn: too many units"); return D2S_E_UNSUPPORTED; }
    const int units = rows * sites * 8;
    const dim3 grid(cdiv((long)units * lpu * TA_KG, 256)), block(256);
    auto launch = [&](auto win) {                      // one row: the instance without the per-lane divide and table read
#define D2S_TATT(TT, CH) hipLaunchKernelGGL((temporal_attn_kernel<TT, CH, decltype(win)>), grid, block, 0, st, (const TT*)cur, ptab, (TT*)out, \
                                            sites, C, slots, scale, lpu, units, win)
        if (prec == D2S_PREC_BF16) { if (p.ch == 8) D2S_TATT(bf16_t, 8); else D2S_TATT(bf16_t, 4); }
        else { if (p.ch == 8) D2S_TATT(float, 8); else D2S_TATT(float, 4); }
#undef D2S_TATT
    };
    if (p.table) launch(WinTable{tab}); else launch(WinRow{tab.r[0]});
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

int launch_geglu(int prec, const void* u, void* g, long rows, int C4, hipStream_t st) {
    long total = rows * C4;
    if (prec == D2S_PREC_BF16) hipLaunchKernelGGL(geglu_kernel<bf16_t>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const bf16_t*)u, (bf16_t*)g, rows, C4);
    else hipLaunchKernelGGL(geglu_kernel<float>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)u, (float*)g, rows, C4);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

int launch_cast_f32(int prec, const float* in, void* out, long n, hipStream_t st) {
    if (prec == D2S_PREC_BF16) hipLaunchKernelGGL(cast_f32_kernel<bf16_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, in, (bf16_t*)out, n);
    else hipLaunchKernelGGL(cast_f32_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, in, (float*)out, n);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

}  // namespace d2s

// ---- test probe ------------------------------------------------------------------------------------
// One call of a launcher above (or of launch_layernorm) on the caller's device buffers, as they are: nothing is packed, allocated or
// copied.  Everything the kernel will index is checked against the element counts the caller states before the launcher is reached.
extern "C" int d2s_temporal_probe(d2s_temporal_probe_params* p, void* stream) {
    using namespace d2s;
    D2S_REQUIRE(p && p->struct_size == sizeof(d2s_temporal_probe_params), "d2s_temporal_probe_params.struct_size must be sizeof(d2s_temporal_probe_params)");
    p->kernel[0] = 0;
    const int prec = p->precision, rows = p->rows, sites = p->sites, C = p->C, slots = p->slots;
    D2S_REQUIRE(prec == D2S_PREC_BF16 || prec == D2S_PREC_FP32, "bad precision (bf16 or fp32)");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t LIM = 1ull << 31;                       // (a b and c d at most 2^31 each: the product stays inside 64 bits)
    auto holds = [&](uint64_t have, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {      // have >= a b c d, without overflow
        return a <= LIM && b <= LIM && a * b <= LIM && c <= LIM && d <= LIM && c * d <= LIM && a * b * (c * d) <= have;
    };
    int rc = D2S_OK;
    switch (p->op) {
    case D2S_TP_GROUPNORM: {
        D2S_REQUIRE(p->x && p->out && p->gamma && p->beta, "groupnorm: null buffer");
        D2S_REQUIRE(rows >= 1 && rows <= 65535 && sites >= 1 && C >= 1 && p->groups >= 1 && p->groups <= 65535 && C % p->groups == 0, "groupnorm: bad shape");
        D2S_REQUIRE(holds(p->x_elems, rows, sites, C, 1) && holds(p->out_elems, rows, sites, C, 1), "groupnorm: x / out smaller than rows * sites * C");
        D2S_REQUIRE(p->gamma_elems >= (uint64_t)C && p->beta_elems >= (uint64_t)C, "groupnorm: gamma / beta smaller than C");
        D2S_REQUIRE((long)sites * C < (1L << 31), "groupnorm: sites * C must stay below 2^31");
        rc = launch_groupnorm(prec, p->x, p->gamma, p->beta, p->out, sites, C, p->groups, p->eps, st, rows);
        if (rc == D2S_OK) plan_name(plan_groupnorm(prec, sites, C, p->groups), prec, p->kernel, sizeof(p->kernel));
        break;
    }
    case D2S_TP_TEMPORAL_ATTN: {
        D2S_REQUIRE(p->x && p->out && p->ptab, "temporal_attn: null buffer");
        D2S_REQUIRE(rows >= 1 && rows <= TA_MAX_ROWS && sites >= 1 && C >= 32 && C % 32 == 0 && slots >= 31 && slots <= 32767, "temporal_attn: bad shape");
        D2S_REQUIRE(holds(p->x_elems, rows, sites, 3, C) && holds(p->out_elems, rows, sites, C, 1), "temporal_attn: cur / out smaller than rows * sites * 3C / C");
        D2S_REQUIRE(p->ptab_elems >= (uint64_t)32 * 3 * C, "temporal_attn: ptab smaller than 32 * 3C");
        AttnRows tab{};
        for (int r = 0; r < rows; ++r) {
            D2S_REQUIRE(p->ring[r] && holds(p->ring_elems[r], slots, sites, 2, C), "temporal_attn: a ring is null or smaller than slots * sites * 2C");
            D2S_REQUIRE((p->Tw[r] == 1 || p->Tw[r] == 32) && p->head[r] >= 0 && p->head[r] < slots && p->store_slot[r] >= -1 && p->store_slot[r] < slots,
                        "temporal_attn: bad row table");
            for (int q = 0; q < r; ++q) D2S_REQUIRE(p->ring[q] != p->ring[r], "temporal_attn: two rows share a ring");
            tab.r[r] = AttnRow{p->ring[r], (int16_t)p->head[r], (int16_t)p->Tw[r], p->store_slot[r]};
        }
        rc = launch_temporal_attn(prec, p->x, p->ptab, p->out, sites, C, slots, rows, tab, st);
        if (rc == D2S_OK) plan_name(plan_temporal_attn(prec, C, rows), prec, p->kernel, sizeof(p->kernel));
        break;
    }
    case D2S_TP_CACHE_STORE: {
        D2S_REQUIRE(p->x, "cache_store: null buffer");
        D2S_REQUIRE(rows >= 1 && rows <= TA_MAX_ROWS && sites >= 1 && C >= 1 && slots >= 1 && slots <= 32767, "cache_store: bad shape");
        D2S_REQUIRE(holds(p->x_elems, rows, sites, 3, C), "cache_store: cur smaller than rows * sites * 3C");
        CacheRows tab{};
        bool any = false;
        for (int r = 0; r < rows; ++r) {
            D2S_REQUIRE(p->slot0[r] >= 0 && p->nslots[r] >= 0 && p->slot0[r] <= slots && p->nslots[r] <= slots - p->slot0[r], "cache_store: slots outside the ring");
            D2S_REQUIRE(p->nslots[r] == 0 || (p->ring[r] && holds(p->ring_elems[r], slots, sites, 2, C)), "cache_store: a ring is null or smaller than slots * sites * 2C");
            tab.r[r] = CacheRow{p->ring[r], p->slot0[r], p->nslots[r]};
            any = any || p->nslots[r] > 0;
        }
        rc = launch_cache_store(prec, p->x, sites, C, rows, tab, st);
        if (rc == D2S_OK && any) snprintf(p->kernel, sizeof(p->kernel), "cache_store_rows_kernel<%s>", prec_tag(prec));
        break;
    }
    case D2S_TP_GEGLU: {
        D2S_REQUIRE(p->x && p->out && rows >= 1 && C >= 1, "geglu: null buffer or bad shape");
        D2S_REQUIRE(holds(p->x_elems, rows, 2, C, 1) && holds(p->out_elems, rows, C, 1, 1), "geglu: u / g smaller than rows * 2C / rows * C");
        rc = launch_geglu(prec, p->x, p->out, rows, C, st);
        if (rc == D2S_OK) snprintf(p->kernel, sizeof(p->kernel), "geglu_kernel<%s>", prec_tag(prec));
        break;
    }
    case D2S_TP_CAST_F32: {
        D2S_REQUIRE(p->x && p->out && p->n >= 1 && p->n <= (1ll << 40), "cast_f32: null buffer or bad count");
        D2S_REQUIRE(p->x_elems >= (uint64_t)p->n && p->out_elems >= (uint64_t)p->n, "cast_f32: in / out smaller than n");
        rc = launch_cast_f32(prec, (const float*)p->x, p->out, p->n, st);
        if (rc == D2S_OK) snprintf(p->kernel, sizeof(p->kernel), "cast_f32_kernel<%s>", prec_tag(prec));
        break;
    }
    case D2S_TP_LAYERNORM: {
        D2S_REQUIRE(p->x && p->out && p->gamma && p->beta && rows >= 1 && C >= 1, "layernorm: null buffer or bad shape");
        D2S_REQUIRE(p->rows_per_img >= 0 && p->row_off >= 0 && (p->rows_per_img == 0 || p->img_rows >= p->rows_per_img + p->row_off), "layernorm: bad row map");
        const uint64_t last_in = p->rows_per_img ? (uint64_t)((rows - 1) / p->rows_per_img) * p->img_rows + (rows - 1) % p->rows_per_img + p->row_off
                                                 : (uint64_t)rows - 1;
        D2S_REQUIRE(holds(p->x_elems, last_in + 1, C, 1, 1) && holds(p->out_elems, rows, C, 1, 1), "layernorm: x / out smaller than the rows read / written");
        D2S_REQUIRE(p->gamma_elems >= (uint64_t)C && p->beta_elems >= (uint64_t)C, "layernorm: gamma / beta smaller than D");
        D2S_REQUIRE(!(p->qscale < 0.f) && p->qscale == p->qscale, "layernorm: bad qscale");
        D2S_REQUIRE(((uintptr_t)p->x & 15) == 0 && ((uintptr_t)p->gamma & 15) == 0 && ((uintptr_t)p->beta & 15) == 0 &&
                    ((uintptr_t)p->out & (p->bx3_out ? 31 : 15)) == 0, "layernorm: buffers must be 16-byte aligned (bf16x3 output: 32)");
        rc = launch_layernorm(prec, (const float*)p->x, p->gamma, p->beta, p->out, rows, C, p->eps, p->rows_per_img, p->img_rows, p->row_off, st,
                              p->qscale, p->bx3_out != 0);
        if (rc == D2S_OK) snprintf(p->kernel, sizeof(p->kernel), "%s", layernorm_kernel_name(layernorm_out_type(prec, p->qscale, p->bx3_out != 0)));
        break;
    }
    default:
        D2S_REQUIRE(false, "d2s_temporal_probe: unknown op");
    }
    const hipError_t err = hipStreamSynchronize(st);
    if (rc != D2S_OK) { p->kernel[0] = 0; return rc; }
    D2S_HIP(err);
    return D2S_OK;
}
