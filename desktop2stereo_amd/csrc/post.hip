// Depth post-process at model resolution (latency-bound, tiny):
//   A10  normalize (subsample + order statistic, no lerp) -> gamma -> foreground scale
//        reference depth.py:816-867, 784-794, 775-776, 709-736
//   A11  anti_alias: separable Gaussian, zero padding, H then V     reference depth.py:740-765
//   A12  DepthStabilizer (EMA)                                      reference depth.py:1865-1887
#include "common.h"
#include "vit_ops.h"
#include <math.h>

namespace d2s {

constexpr int SORT_N = 8192;       // >= subsample_cap (6144), power of two
constexpr int SORT_THREADS = 1024;

__device__ __forceinline__ uint32_t f2key(float f) {          // order-preserving float -> uint
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// One block per frame: v = depth.flatten()[::step] (m <= cap values, held in registers), then an exact
// radix select (4 passes x 8 bits, LDS histograms) of the two order statistics
//   bounds[b] = { s[tail-1], s[m-tail] }   (the tail-th smallest / largest; no lerp, depth.py:784-794).
//
// METRIC (is_metric(), depth.py:844-847): the values are inv = 1/max(d,1e-12) of the VALID pixels (d > 0) only, in
// row-major order, so the subsample positions depend on the data: a block-wide scan ranks the valid pixels, the
// step / m / tail follow from the valid count, and the r-th valid pixel is sample r/step iff r % step == 0.
__device__ __forceinline__ float metric_inverse(float d) { return d > 0.f ? 1.0f / fmaxf(d, 1e-12f) : d; }

// The subsample of n values under the cap, and the rank of the lower bound in it: the host plans with it (plan_post), the metric
// kernel restates it for its data-dependent n.
struct Subsample { int step, m, tail; };
__host__ __device__ inline Subsample subsample_of(int n, int cap, double lo_q) {
    Subsample s;
    s.step = n > cap ? (n + cap - 1) / cap : 1;
    s.m = (n + s.step - 1) / s.step;
    s.tail = (int)nearbyint(lo_q * (double)(s.m - 1)) + 1;
    s.tail = s.tail > s.m ? s.m : s.tail;
    s.tail = s.tail < 1 ? 1 : s.tail;
    return s;
}

typedef unsigned u4_ __attribute__((ext_vector_type(4)));

// WORDS zeros at p, shared among the block's THREADS threads: 16-byte stores (p aligned) where every thread has one, else one word each
template <int THREADS, int WORDS>
__device__ __forceinline__ void zero_lds(unsigned* p, int tid) {
    static_assert(WORDS <= THREADS || WORDS % (4 * THREADS) == 0, "the same number of stores per thread");
    if constexpr (WORDS > THREADS) {
#pragma unroll
        for (int i = 0; i < WORDS / (4 * THREADS); ++i) ((u4_*)p)[tid + i * THREADS] = (u4_){0u, 0u, 0u, 0u};
    } else if (tid < WORDS) p[tid] = 0u;
}

// [kmin, kmax] of the block's m keys (thread tid holds keys tid + i * THREADS); one barrier.  m == 0: [~0, 0].  EVERY: in every thread
// (each reads all the waves' results), else in thread 0 alone, which adds the other waves' to its own.
template <int THREADS, bool EVERY, int PER>
__device__ __forceinline__ void block_key_range(const uint32_t (&key)[PER], int m, unsigned* red_min, unsigned* red_max, unsigned& kmin, unsigned& kmax) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    kmin = 0xffffffffu; kmax = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (tid + i * THREADS < m) { kmin = min(kmin, key[i]); kmax = max(kmax, key[i]); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o)); kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o)); }
    if (lane == 0) { red_min[wid] = kmin; red_max[wid] = kmax; }
    __syncthreads();
    if (EVERY || tid == 0)
        for (int w_ = EVERY ? 0 : 1; w_ < THREADS / 64; ++w_) { kmin = min(kmin, red_min[w_]); kmax = max(kmax, red_max[w_]); }
}

// One wave scans one histogram of 64 * BINS_PER_LANE bins (16-byte aligned, BINS_PER_LANE consecutive bins per lane).  The lane whose
// bins hold rank `target` returns hit with the bin, the rank inside it and the bin's count; every other lane returns no hit.
struct Pick { bool hit; unsigned bin, rank, count; };
template <int BINS_PER_LANE>
__device__ __forceinline__ Pick pick_bin(const unsigned* hist, int lane, unsigned target) {
    constexpr int Q = BINS_PER_LANE / 4;
    const u4_* hp = (const u4_*)(hist + BINS_PER_LANE * lane);
    u4_ c[Q];
    unsigned s_ = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) { c[q] = hp[q]; s_ += (c[q][0] + c[q][1]) + (c[q][2] + c[q][3]); }
    unsigned incl = s_;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    const unsigned excl = incl - s_;
    if (target < excl || target >= incl) return Pick{false, 0u, 0u, 0u};
    unsigned rr = target - excl, b = 0, cnt_b = 0;
    bool found = false;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned cnt = c[q][k];
            if (!found) { if (rr < cnt) { found = true; b = 4 * q + k; cnt_b = cnt; } else rr -= cnt; }
        }
    return Pick{true, BINS_PER_LANE * lane + b, rr, cnt_b};
}

template <bool METRIC>
__global__ void __launch_bounds__(SORT_THREADS)
percentile_bounds_kernel(const float* __restrict__ depth, int n, int step, int m, int tail, int cap, double lo_q,
                         float* __restrict__ bounds) {
    constexpr int PER = SORT_N / SORT_THREADS;
    __shared__ __attribute__((aligned(16))) unsigned hist[2][256];
    __shared__ unsigned sel_rank[2];
    const float* d = depth + (long)blockIdx.x * n;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t key[PER];
    int nvalid = n;
    if constexpr (METRIC) {
        __shared__ uint32_t samp[SORT_N];
        __shared__ int wave_cnt[SORT_THREADS / 64];
        __shared__ int s_nv;
        const int chunk = (n + SORT_THREADS - 1) / SORT_THREADS;
        const int i0 = min(n, tid * chunk), i1 = min(n, i0 + chunk);
        int cnt = 0;
        for (int i = i0; i < i1; ++i) cnt += d[i] > 0.f;
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) wave_cnt[wid] = incl;
        __syncthreads();
        int base = incl - cnt;
        for (int w = 0; w < wid; ++w) base += wave_cnt[w];
        if (tid == SORT_THREADS - 1) s_nv = base + cnt;
        __syncthreads();
        nvalid = s_nv;
        const Subsample sub = subsample_of(nvalid, cap, lo_q);
        step = sub.step; m = sub.m; tail = sub.tail;
        int r = base;
        for (int i = i0; i < i1; ++i) {
            float v = d[i];
            if (v > 0.f) { if (r % step == 0) samp[r / step] = f2key(metric_inverse(v)); ++r; }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tid + i * SORT_THREADS; key[i] = idx < m ? samp[idx] : 0u; }
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i) { int idx = tid + i * SORT_THREADS; key[i] = idx < m ? f2key(d[(long)idx * step]) : 0u; }
    }
    // Range-adaptive radix select.  A fixed 8-bits-from-the-top radix puts all of a depth map's keys (same sign, one or two
    // exponents) into one or two bins of the first passes -- 6144 LDS atomics on the same address, serialised: 20 us for a
    // 24 KB problem.  Here a pass bins (key - lo) >> shift with [lo, lo + (256 << shift)) the range that still holds the
    // target, starting from the block's [min key, max key]: the first pass spreads over all 256 bins, later passes see only
    // the few keys of the chosen bin.  Exact: the binning is monotone in the key.
    __shared__ unsigned red_min[SORT_THREADS / 64], red_max[SORT_THREADS / 64];
    __shared__ unsigned sel_lo[2], sel_shift;
    {
        unsigned kmin, kmax;
        block_key_range<SORT_THREADS, false>(key, m, red_min, red_max, kmin, kmax);
        if (tid == 0) {
            if (m <= 0) { kmin = kmax = 0u; }
            const unsigned span = kmax - kmin;
            const int bits = span ? 32 - __clz((int)span) : 0;              // span < 2^bits
            sel_shift = bits > 8 ? bits - 8 : 0;
            sel_lo[0] = sel_lo[1] = kmin;
            bool all = tail >= m;                                   // depth.py:790-791: (min, max)
            sel_rank[0] = all ? 0 : tail - 1; sel_rank[1] = all ? m - 1 : m - tail;
        }
        __syncthreads();
    }
    while (true) {
        const unsigned shift = sel_shift;
        zero_lds<SORT_THREADS, 2 * 256>(&hist[0][0], tid);
        __syncthreads();
        const unsigned l0 = sel_lo[0], l1 = sel_lo[1];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (tid + i * SORT_THREADS < m) {
                const unsigned d0 = key[i] - l0, d1 = key[i] - l1;           // (unsigned: keys below lo wrap to huge values)
                if (key[i] >= l0 && (d0 >> shift) < 256u) atomicAdd(&hist[0][d0 >> shift], 1u);
                if (key[i] >= l1 && (d1 >> shift) < 256u) atomicAdd(&hist[1][d1 >> shift], 1u);
            }
        }
        __syncthreads();
        if (wid < 2) {                                           // wave r resolves rank r: 4 bins per lane
            const Pick pk = pick_bin<4>(hist[wid], lane, sel_rank[wid]);
            if (pk.hit) { sel_lo[wid] += pk.bin << shift; sel_rank[wid] = pk.rank; }
        }
        __syncthreads();
        if (shift == 0) break;
        if (tid == 0) sel_shift = shift > 8 ? shift - 8 : 0;
        __syncthreads();
    }
    if (tid == 0) {
        float lo = key2f(sel_lo[0]), hi = key2f(sel_lo[1]);
        if (nvalid <= 10) { lo = 0.f; hi = 0.f; }                // depth.py:852-854
        bounds[2 * blockIdx.x] = lo;
        bounds[2 * blockIdx.x + 1] = hi;
    }
}

// x^y for x in [0, 1] on the transcendental pipe: exp2(y log2 x), v_log_f32 / v_exp_f32 (1 ulp each).  On this domain the result is
// <= 1 and |y log2 x| is small wherever the result is not: max |error| 1.0e-7 over [0, 1] for y in {1.45, 1/1.05, 2/3, 2, 1/2} against 5.9e-8
// for a correctly rounded powf (float64 reference, 2 M points) -- two orders below the 5e-6 the post-process is held
// to.  ocml's powf is ~200 instructions of double-float arithmetic; every pixel takes two, and the one-launch kernel re-shapes its
// window borders (2.7 x the pixels): 8 us of a 24 us kernel at batch 1 (rocprofv3, profiles/r5_*).  x = 0 -> 0 (y = 0 -> 1), like powf.
__device__ __forceinline__ float pow01(float x, float y) {
    const float r = __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
    return x > 0.f ? r : (y == 0.f ? 1.f : 0.f);
}
__device__ __forceinline__ float shape_depth(float d, float dmin, float dmax, float gamma, float fg_exp, bool fg_on) {
    float denom = fmaxf(dmax - dmin, 1e-6f);                                      // depth.py:865
    float nrm = fminf(fmaxf((d - dmin) / denom, 0.f), 1.f);
    float g = pow01(nrm, gamma);                                                  // depth.py:775-776
    g = fminf(fmaxf(g, 0.f), 1.f);                                                // depth.py:729
    if (!fg_on) return g;
    float dist = g - 0.5f;
    float sgn = dist > 0.f ? 1.f : (dist < 0.f ? -1.f : 0.f);
    float o = 0.5f + sgn * pow01(fabsf(dist), fg_exp);                            // depth.py:733-735
    return fminf(fmaxf(o, 0.f), 1.f);
}

// One pixel of the shaped map: the raw value is requested first (the one-launch kernel has its bounds only later), then inverted if
// metric (depth.py:844-846) and shaped; zero outside the image.
struct ShapeArgs { float dmin, dmax, gamma, fg_exp; bool fg_on, metric; };
__device__ __forceinline__ float raw_pixel(const float* __restrict__ src, long i, bool inside) { return inside ? src[i] : 0.f; }
__device__ __forceinline__ float shape_pixel(float v, bool inside, const ShapeArgs& s) {
    if (!inside) return 0.f;
    if (s.metric) v = metric_inverse(v);
    return shape_depth(v, s.dmin, s.dmax, s.gamma, s.fg_exp, s.fg_on);
}

constexpr int MAX_TAPS = 63;
struct GaussTaps { int k; float w[MAX_TAPS]; };

// The two tap loops of the separable Gaussian, KT taps known at compile time (unrolled, weights in SGPRs) or KT = 0: nt = taps.k at run
// time.  Every form of the post-process takes its products from these two in this order, which is why the forms are bit-identical.
// Horizontal: row points at tap 0 of a zero-padded row (r = nt / 2; nt = 1: no blur, the centre).
template <int KT>
__device__ __forceinline__ float hblur_taps(const float* row, const GaussTaps& taps, int nt, int r) {
    if (nt < 3) return row[r];
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < nt; ++t) acc += taps.w[t] * row[t];
    return acc;
}
// Vertical: tap t is col[(row0 + t) * stride] and belongs to image row y + t - r; rows outside the image are skipped.
// (compile-time tap count: all column loads are issued before the first product -- with a run-time count every tap was a scalar
//  load of its weight plus a dependent global load, 13 round trips per pixel)
template <int KT>
__device__ __forceinline__ float vblur_taps(const float* col, long stride, int row0, int y, int h, const GaussTaps& taps, int nt, int r) {
    float v[KT ? KT : 1];
    if constexpr (KT != 0) {
#pragma unroll
        for (int t = 0; t < KT; ++t) { const int yy = y + t - r; v[t] = (yy >= 0 && yy < h) ? col[(row0 + t) * stride] : 0.f; }
    }
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < nt; ++t) {
        const int yy = y + t - r;
        if (yy >= 0 && yy < h) acc += taps.w[t] * (KT ? v[KT ? t : 0] : col[(row0 + t) * stride]);
    }
    return acc;
}

// normalise + gamma + foreground-scale fused with the horizontal Gaussian pass: one block per row,
// shaped row staged in LDS (zero padded), k taps out of LDS.
template <int KT>      // taps known at compile time (13 = the reference's default): unrolled tap loops, weights in SGPRs; 0 = run-time count
__global__ void __launch_bounds__(256)
shape_hblur_kernel(const float* __restrict__ depth, const float* __restrict__ bounds, float* __restrict__ tmp,
                   int h, int w, float gamma, float fg_exp, int fg_on, int metric, GaussTaps taps) {
    extern __shared__ float row[];                       // w + 2r
    int y = blockIdx.x % h, b = blockIdx.x / h;
    const int nt = KT ? KT : taps.k;
    int r = nt / 2;
    const ShapeArgs sa{bounds[2 * b], bounds[2 * b + 1], gamma, fg_exp, fg_on != 0, metric != 0};
    const float* src = depth + ((long)b * h + y) * w;
    for (int i = threadIdx.x; i < w + 2 * r; i += 256) {
        const int x = i - r;
        const bool inside = x >= 0 && x < w;
        row[i] = shape_pixel(raw_pixel(src, x, inside), inside, sa);
    }
    __syncthreads();
    float* dst = tmp + ((long)b * h + y) * w;
    for (int x = threadIdx.x; x < w; x += 256) dst[x] = hblur_taps<KT>(row + x, taps, nt, r);
}

template <int KT>
__global__ void __launch_bounds__(256)
vblur_kernel(const float* __restrict__ tmp, float* __restrict__ out, int B, int h, int w, GaussTaps taps) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * h * w) return;
    int x = (int)(idx % w);
    int y = (int)((idx / w) % h);
    int b = (int)(idx / ((long)w * h));
    const float* p = tmp + (long)b * h * w + x;
    const int nt = KT ? KT : taps.k;
    const int r = nt / 2;
    out[idx] = vblur_taps<KT>(p, w, y - r, y, h, taps, nt, r);
}

// Both passes in one launch (few frames: the two launches above are two launch floors for 0.6 MB): a block owns an 8 x 128 tile, shapes
// the (8 + 2r) x (128 + 2r) window it taps into LDS (zero outside the image, exactly what the two-pass form sees: the horizontal
// pass pads its row with zeros, the vertical pass skips rows outside the image), blurs horizontally into a second LDS plane and
// vertically out of it -- the same products in the same order, so the result is bit-identical to shape_hblur_kernel + vblur_kernel.
constexpr int SB_TR = 8, SB_TC = 128;
__global__ void __launch_bounds__(256)
shape_blur_kernel(const float* __restrict__ depth_in, const float* __restrict__ bounds, float* __restrict__ out,
                  int h, int w, float gamma, float fg_exp, int fg_on, int metric, GaussTaps taps) {
    extern __shared__ float sb_lds[];
    const int r = taps.k / 2, WR = SB_TC + 2 * r, HR = SB_TR + 2 * r;
    float* shp = sb_lds;                 // [HR][WR]
    float* hb = sb_lds + HR * WR;        // [HR][SB_TC]
    const int b = blockIdx.z, y0 = blockIdx.y * SB_TR, x0 = blockIdx.x * SB_TC;
    const ShapeArgs sa{bounds[2 * b], bounds[2 * b + 1], gamma, fg_exp, fg_on != 0, metric != 0};
    const float* src = depth_in + (long)b * h * w;
    for (int i = threadIdx.x; i < HR * WR; i += 256) {
        const int ry = i / WR, rx = i - ry * WR;
        const int y = y0 + ry - r, x = x0 + rx - r;
        const bool inside = y >= 0 && y < h && x >= 0 && x < w;
        shp[i] = shape_pixel(raw_pixel(src, (long)y * w + x, inside), inside, sa);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HR * SB_TC; i += 256) {
        const int ry = i / SB_TC, cx = i - ry * SB_TC;
        hb[i] = hblur_taps<0>(shp + ry * WR + cx, taps, taps.k, r);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SB_TR * SB_TC; i += 256) {
        const int ty = i / SB_TC, cx = i - ty * SB_TC;
        const int y = y0 + ty, x = x0 + cx;
        if (y >= h || x >= w) continue;
        out[((long)b * h + y) * w + x] = vblur_taps<0>(hb + cx, SB_TC, ty, y, h, taps, taps.k, r);
    }
}

// ---- round 5: the whole post-process of a few frames in ONE launch (batch <= D2S_POST_FUSE_MAXB, relative models) --------------------
// percentile_bounds_kernel (one 1024-thread block per frame, 18 us) + shape_blur_kernel (23 us) were 45 us at the END of the batch-1
// critical path (3.8 % of the frame) for 0.6 MB of data.  Where the time went: (i) the select's four 8-bit passes are ~20 block barriers of
// 16 waves with single-thread sections between them; (ii) shape_blur's window loop issued one global load per iteration behind the
// previous iteration's two powf() -- eleven dependent memory round trips per thread.  Here every block of the (8 x 128)-tile grid
//   * requests its window pixels FIRST (<= 6 per thread, all in flight at once),
//   * derives the frame's bounds itself while they are in flight -- the same exact order statistics (any exact select returns the same
//     two values): range-adaptive radix select with 2048 bins per target (<= 3 passes), two alternating histogram buffers so a pass
//     costs two barriers, nothing done by one thread alone -- redundantly in every block (the subsample is 24 KB out of L2; 185 blocks
//     on 256 CUs: no block waits for another, no second launch),
//   * shapes the window (16 waves share the powf work a 256-thread block did alone), blurs horizontally and vertically out of LDS with
//     the products in shape_hblur_kernel / vblur_kernel's order: bit-identical to the separate launches.
constexpr int PF_THREADS = 1024, PF_TR = 8, PF_TC = 128, PF_MAXR = 8, PF_BITS = 11, PF_BINS = 1 << PF_BITS;
constexpr int PF_HR = PF_TR + 2 * PF_MAXR, PF_WR = PF_TC + 2 * PF_MAXR;
template <int KT>      // taps known at compile time (13 = the reference's default Anti-aliasing 4: the tap loops unroll and the weights stay
                        // in SGPRs -- with a run-time count every tap is an s_load from the kernarg segment inside the loop); 0 = run-time count
__global__ void __launch_bounds__(PF_THREADS)
post_fused_kernel(const float* __restrict__ depth_in, float* __restrict__ out, float* __restrict__ bounds_out, int h, int w, int step, int m, int tail,
                  float gamma, float fg_exp, int fg_on, GaussTaps taps) {
    constexpr int PER = SORT_N / PF_THREADS;
    __shared__ __attribute__((aligned(16))) unsigned lds_u[2 * 2 * PF_BINS];          // two buffers x two targets; the tile planes alias them afterwards
    __shared__ unsigned red_min[PF_THREADS / 64], red_max[PF_THREADS / 64];
    __shared__ unsigned sel_lo[2], sel_rank[2], sel_n[2], sel_cnt[2], sel_res[2];
    static_assert(sizeof(float) * (PF_HR * PF_WR + PF_HR * PF_TC) <= sizeof(unsigned) * 4 * PF_BINS, "tile planes alias the histograms");
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.z, y0 = blockIdx.y * PF_TR, x0 = blockIdx.x * PF_TC;
    const int nt = KT ? KT : taps.k;
    const int r = nt / 2, WR = PF_TC + 2 * r, HR = PF_TR + 2 * r;
    const float* src = depth_in + (long)b * h * w;
    // (1) window pixels: wave `wid` owns window rows wid and wid + 16, lanes the columns lane, lane + 64, lane + 128
    float raw[2][3];
    bool inside[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ry = wid + 16 * i, rx = lane + 64 * j;
            const int y = y0 + ry - r, x = x0 + rx - r;
            inside[i][j] = ry < HR && rx < WR && y >= 0 && y < h && x >= 0 && x < w;
            raw[i][j] = raw_pixel(src, (long)y * w + x, inside[i][j]);
        }
    // (2) the frame's subsample
    uint32_t key[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) { const int idx = tid + i * PF_THREADS; key[i] = idx < m ? f2key(src[(long)idx * step]) : 0u; }
    zero_lds<PF_THREADS, 4 * PF_BINS>(lds_u, tid);                      // both histogram buffers start at zero
    unsigned kmin, kmax;
    block_key_range<PF_THREADS, true>(key, m, red_min, red_max, kmin, kmax);
    const unsigned span = kmax - kmin;
    const int bits = span ? 32 - __clz((int)span) : 0;                  // span < 2^bits
    int shift = bits > PF_BITS ? bits - PF_BITS : 0;
    const bool all = tail >= m;                                         // depth.py:790-791: (min, max)
    unsigned lo0 = kmin, lo1 = kmin, rk0 = all ? 0u : (unsigned)(tail - 1), rk1 = all ? (unsigned)(m - 1) : (unsigned)(m - tail);
    // ---- fast path (round 5): ONE value-linear histogram pass + ranking of the target bins' few candidates.  The radix passes below bin
    // key BITS: a depth map's keys share their exponent bits, so the first pass piles 6 000 keys on ~50 bins (serialised LDS atomics) and
    // three passes are needed (6.8 us of the 16 us kernel, profiles/r5_01).  Binning floor((v - vmin) * (BINS - 1) / (vmax - vmin)) is monotone
    // non-decreasing in the key order too (rounding is monotone), so the keys of lower bins are strictly smaller than those of the target's
    // bin and the order statistic is the (rank - lower count)-th smallest KEY of that bin: the same element the radix select returns.
    // Both targets share the histogram.  Taken when the value range is finite and both target bins hold <= PF_CAND keys (a map with
    // thousands of identical values -- ReLU zeros -- falls through to the radix passes).
    constexpr int PF_CAND = 512;
    bool done = false;
    {
        const float vmin = key2f(kmin), vmax = key2f(kmax), rng = vmax - vmin;
        if (kmin != kmax && rng > 0.f && rng < 3.0e38f && fabsf(vmin) < 3.0e38f) {                 // (block-uniform; NaN / Inf keys fail it)
            // bins 0 and BINS-1 hold ONLY the values equal to the minimum / maximum (a ReLU head leaves hundreds of exact zeros in the
            // subsample, a sigmoid head saturates at the top): a target that lands there is the minimum / maximum itself, no candidates
            const float bscale = (float)(PF_BINS - 2) / rng;
            auto bin_of = [&](uint32_t k) {
                const float v = key2f(k);
                if (v <= vmin) return 0u;
                if (v >= vmax) return (unsigned)(PF_BINS - 1);
                return 1u + (unsigned)min(max((int)((v - vmin) * bscale), 0), PF_BINS - 3);
            };
            unsigned* hist = lds_u;                                     // buffer 0, target-0 half: zero since the start of the kernel
            unsigned* cand = lds_u + 2 * PF_BINS;                       // buffer 1: 2 x PF_CAND candidate keys
            unsigned mybin[PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                mybin[i] = 0xffffffffu;
                if (tid + i * PF_THREADS < m) { mybin[i] = bin_of(key[i]); atomicAdd(&hist[mybin[i]], 1u); }
            }
            if (tid < 2) sel_cnt[tid] = 0u;
            __syncthreads();
            if (wid < 2) {                                              // wave t resolves target t: 32 consecutive bins per lane
                const Pick pk = pick_bin<PF_BINS / 64>(hist, lane, wid == 0 ? rk0 : rk1);
                if (pk.hit) {
                    const unsigned tb = pk.bin, rr = pk.rank, cnt_b = pk.count;
                    const bool edge = tb == 0u || tb == (unsigned)(PF_BINS - 1);
                    sel_lo[wid] = tb;                                   // (here: the target's BIN)
                    sel_rank[wid] = rr;
                    sel_n[wid] = edge ? 0u : cnt_b;                     // an edge bin's keys all equal the minimum / maximum value
                    sel_res[wid] = tb == 0u ? kmin : kmax;              // (overwritten by the ranking unless the bin is an edge bin)
                }
            }
            __syncthreads();
            const unsigned b0 = sel_lo[0], b1 = sel_lo[1], r0 = sel_rank[0], r1 = sel_rank[1], n0 = sel_n[0], n1 = sel_n[1];
            if (n0 <= (unsigned)PF_CAND && n1 <= (unsigned)PF_CAND) {   // (block-uniform)
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    if (n0 && mybin[i] == b0) cand[atomicAdd(&sel_cnt[0], 1u)] = key[i];
                    if (n1 && mybin[i] == b1) cand[PF_CAND + atomicAdd(&sel_cnt[1], 1u)] = key[i];
                }
                __syncthreads();
                // threads 0 .. n0-1 rank list 0, threads 512 .. 512+n1-1 rank list 1: the element with  #{u < v} <= r < #{u <= v}
                const int li = tid >> 9, ti = tid & 511;
                const unsigned nn = li ? n1 : n0, rr = li ? r1 : r0;
                if ((unsigned)ti < nn) {
                    const unsigned* L = cand + li * PF_CAND;
                    const unsigned v = L[ti];
                    unsigned less = 0, leq = 0;
                    for (unsigned u = 0; u < nn; ++u) { const unsigned x = L[u]; less += x < v; leq += x <= v; }
                    if (less <= rr && rr < leq) sel_res[li] = v;        // (equal keys write the same value)
                }
                __syncthreads();
                lo0 = sel_res[0]; lo1 = sel_res[1];
                done = true;
            } else {
                // fall through to the radix passes: they expect both histogram buffers at zero
                __syncthreads();
                zero_lds<PF_THREADS, 4 * PF_BINS>(lds_u, tid);
                __syncthreads();
            }
        }
    }
    if (!done)
    for (int pass = 0;; ++pass) {
        unsigned* hist = lds_u + (pass & 1) * (2 * PF_BINS);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (tid + i * PF_THREADS < m) {
                const unsigned d0 = key[i] - lo0, d1 = key[i] - lo1;          // (unsigned: keys below lo wrap to huge values)
                if (key[i] >= lo0 && (d0 >> shift) < (unsigned)PF_BINS) atomicAdd(&hist[d0 >> shift], 1u);
                if (key[i] >= lo1 && (d1 >> shift) < (unsigned)PF_BINS) atomicAdd(&hist[PF_BINS + (d1 >> shift)], 1u);
            }
        }
        // the other buffer (pass - 1's, read for the last time before the barrier behind its scan)
        if (pass >= 1) zero_lds<PF_THREADS, 2 * PF_BINS>(lds_u + ((pass + 1) & 1) * (2 * PF_BINS), tid);
        __syncthreads();
        if (wid < 2) {                                                  // wave t resolves target t: 32 consecutive bins per lane
            const Pick pk = pick_bin<PF_BINS / 64>(hist + wid * PF_BINS, lane, wid == 0 ? rk0 : rk1);
            if (pk.hit) { sel_lo[wid] = (wid == 0 ? lo0 : lo1) + (pk.bin << shift); sel_rank[wid] = pk.rank; }
        }
        __syncthreads();
        lo0 = sel_lo[0]; lo1 = sel_lo[1]; rk0 = sel_rank[0]; rk1 = sel_rank[1];
        if (shift == 0) break;
        shift = shift > PF_BITS ? shift - PF_BITS : 0;
    }
    ShapeArgs sa{key2f(lo0), key2f(lo1), gamma, fg_exp, fg_on != 0, false};
    if (h * w <= 10) { sa.dmin = 0.f; sa.dmax = 0.f; }               // depth.py:852-854
    if (bounds_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) { bounds_out[2 * b] = sa.dmin; bounds_out[2 * b + 1] = sa.dmax; }
    // (3) shape the window into LDS (zero outside the image: what the two-pass form's zero padding / skipped rows see)
    float* shp = (float*)lds_u;                  // [HR][WR]
    float* hb = shp + HR * WR;                   // [HR][PF_TC]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ry = wid + 16 * i, rx = lane + 64 * j;
            if (ry < HR && rx < WR) shp[ry * WR + rx] = shape_pixel(raw[i][j], inside[i][j], sa);
        }
    __syncthreads();
    // (4) horizontal pass: rows wid, wid + 16; columns lane, lane + 64
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ry = wid + 16 * i, cx = lane + 64 * j;
            if (ry < HR) hb[ry * PF_TC + cx] = hblur_taps<KT>(shp + ry * WR + cx, taps, nt, r);
        }
    __syncthreads();
    // (5) vertical pass: one output per thread
    {
        const int ty = wid >> 1, cx = (wid & 1) * 64 + lane;
        const int y = y0 + ty, x = x0 + cx;
        if (y < h && x < w) out[((long)b * h + y) * w + x] = vblur_taps<KT>(hb + cx, PF_TC, ty, y, h, taps, nt, r);
    }
}

// EMA over `nframes` consecutive frames (recurrence in frame order); thread per pixel.
__global__ void __launch_bounds__(256)
ema_kernel(float* __restrict__ depth, float* __restrict__ state, int initialised, int nframes, int hw, float wgt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    float prev = initialised ? state[i] : 0.f;
    for (int f = 0; f < nframes; ++f) {
        float d = depth[(long)f * hw + i];
        if (!initialised && f == 0) prev = d;
        else prev = prev + wgt * (d - prev);                 // torch lerp_, weight < 0.5
        depth[(long)f * hw + i] = prev;
    }
    state[i] = prev;
}

// EMA per stream slot (temporal engines): batch row blockIdx.y is ONE new frame of stream tab.r[row].slot; no chain across rows.
__global__ void __launch_bounds__(256)
ema_rows_kernel(float* __restrict__ depth, float* __restrict__ state, int hw, float wgt, const EmaRows tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const EmaRow r = tab.r[blockIdx.y];
    float* d = depth + (long)blockIdx.y * hw + i;
    float* s = state + (long)r.slot * hw + i;
    float prev = *d;
    if (r.initialised) { const float p0 = *s; prev = p0 + wgt * (prev - p0); }     // torch lerp_, weight < 0.5
    *d = prev;
    *s = prev;
}

}  // namespace d2s

using namespace d2s;

extern "C" uint64_t d2s_post_process_workspace(int batch, int h, int w) {
    return (uint64_t)batch * h * w * sizeof(float) + (uint64_t)batch * 2 * sizeof(float) + 256;
}

// Everything d2s_post_process_to decides, stated once on the host (d2s_post_plan reports it; the tests pin it).  Three forms compute the
// same bits; each is the one production takes for some input:
//   fused  post_fused_kernel, one launch: relative models, <= D2S_POST_FUSE_MAXB (2) frames, out of place, r <= 8;
//   tile   percentile_bounds_kernel + shape_blur_kernel: metric models or r > 8, few frames, out of place (tiles tap their neighbours'
//          inputs, so never in place), the (8 + 2r) x (128 + 2r) window and its blurred rows within 64 KiB of LDS;
//   rows   percentile_bounds_kernel + shape_hblur_kernel + vblur_kernel: more frames (the tile forms re-shape the window borders,
//          1.8 x the pow() work: +0.6 % at batch 1, -0.7 % at 4), in place, or a tile too large for LDS.
// D2S_POST_ONE=0 takes the fused form out, D2S_POST_FUSE_MAXB=0 both tile forms: the tests hold the forms to each other that way.
struct PostLaunch { const char* name; dim3 grid, block; size_t lds; };
struct PostPlan {
    Subsample sub; double lo_q;            // (metric: the kernel derives its own from the valid count)
    GaussTaps taps; int r; bool k13;       // k13: the <13> tap instantiation, else <0> = run-time count
    int fg_on; float fg_exp;
    int form, nlaunch; PostLaunch launch[3];
};
// Gaussian taps: k = int(3 s) | 1, sigma = 0.5 s, float32 like the reference (depth.py:746-758)
static int gauss_k(const d2s_post_params* p) { return ((int)(3.0f * p->aa_strength)) | 1; }
static int check_post_params(const d2s_post_params* p) {
    D2S_REQUIRE(p->subsample_cap > 0 && p->subsample_cap <= SORT_N, "subsample_cap must be <= 8192");
    D2S_REQUIRE(p->foreground_scale > -1.0f + 1e-12f, "scale must be greater than -1.0");   // depth.py:726-727
    D2S_REQUIRE(gauss_k(p) <= MAX_TAPS, "aa_strength too large");
    return D2S_OK;
}
static PostPlan plan_post(int batch, int h, int w, const d2s_post_params* p, bool in_place) {
    PostPlan pl;
    pl.lo_q = fmax(0.0, fmin(1.0, (double)p->percentile / 100.0));
    pl.sub = subsample_of(h * w, p->subsample_cap, pl.lo_q);
    const int k = gauss_k(p);
    pl.taps.k = k >= 3 ? k : 1;
    if (k >= 3) {
        float sigma = 0.5f * p->aa_strength, sum = 0.f;
        for (int i = 0; i < k; ++i) { float c = (float)(i - k / 2); pl.taps.w[i] = expf(-(c * c) / (2.f * sigma * sigma)); sum += pl.taps.w[i]; }
        for (int i = 0; i < k; ++i) pl.taps.w[i] /= sum;
    } else pl.taps.w[0] = 1.f;
    pl.fg_on = fabsf(p->foreground_scale) >= 1e-6f;
    pl.fg_exp = 1.0f / (1.0f + p->foreground_scale);
    const int r = pl.r = pl.taps.k / 2;
    const bool k13 = pl.k13 = pl.taps.k == 13;
    static EnvInt fuse_max{"D2S_POST_FUSE_MAXB", 2}, one_launch{"D2S_POST_ONE", 1};
    const size_t sb_bytes = ((size_t)(SB_TR + 2 * r) * (SB_TC + 2 * r) + (size_t)(SB_TR + 2 * r) * SB_TC) * sizeof(float);
    const bool few = !in_place && batch <= fuse_max.get() && batch <= 65535;
    const PostLaunch bounds{p->metric ? "percentile_bounds<metric>" : "percentile_bounds<relative>", dim3(batch), dim3(SORT_THREADS), 0};
    if (one_launch.get() && !p->metric && few && r <= PF_MAXR && cdiv(h, PF_TR) <= 65535) {
        pl.form = D2S_POST_FORM_FUSED; pl.nlaunch = 1;
        pl.launch[0] = {k13 ? "post_fused<13>" : "post_fused<0>", dim3(cdiv(w, PF_TC), cdiv(h, PF_TR), batch), dim3(PF_THREADS), 0};
    } else if (few && sb_bytes <= 64 * 1024 && cdiv(h, SB_TR) <= 65535) {
        pl.form = D2S_POST_FORM_TILE; pl.nlaunch = 2;
        pl.launch[0] = bounds;
        pl.launch[1] = {"shape_blur", dim3(cdiv(w, SB_TC), cdiv(h, SB_TR), batch), dim3(256), sb_bytes};
    } else {
        pl.form = D2S_POST_FORM_ROWS; pl.nlaunch = 3;
        pl.launch[0] = bounds;
        pl.launch[1] = {k13 ? "shape_hblur<13>" : "shape_hblur<0>", dim3(batch * h), dim3(256), (w + 2 * r) * sizeof(float)};
        pl.launch[2] = {k13 ? "vblur<13>" : "vblur<0>", dim3(cdiv((long)batch * h * w, 256)), dim3(256), 0};
    }
    return pl;
}

static void launch_post(const PostPlan& pl, const float* depth, float* depth_out, int batch, int h, int w, const d2s_post_params* p,
                        float* tmp, float* bounds, hipStream_t st) {
    const PostLaunch* L = pl.launch;
    const bool k13 = pl.k13;
    const int metric = p->metric != 0;
    auto go = [st](auto kernel, const PostLaunch& l, auto... args) { hipLaunchKernelGGL(kernel, l.grid, l.block, l.lds, st, args...); };
    if (pl.form == D2S_POST_FORM_FUSED)
        return go(k13 ? post_fused_kernel<13> : post_fused_kernel<0>, L[0], depth, depth_out, bounds, h, w, pl.sub.step, pl.sub.m, pl.sub.tail,
                  p->gamma, pl.fg_exp, pl.fg_on, pl.taps);
    go(metric ? percentile_bounds_kernel<true> : percentile_bounds_kernel<false>, L[0], depth, h * w, pl.sub.step, pl.sub.m, pl.sub.tail,
       p->subsample_cap, pl.lo_q, bounds);
    if (pl.form == D2S_POST_FORM_TILE) return go(shape_blur_kernel, L[1], depth, bounds, depth_out, h, w, p->gamma, pl.fg_exp, pl.fg_on, metric, pl.taps);
    go(k13 ? shape_hblur_kernel<13> : shape_hblur_kernel<0>, L[1], depth, bounds, tmp, h, w, p->gamma, pl.fg_exp, pl.fg_on, metric, pl.taps);
    go(k13 ? vblur_kernel<13> : vblur_kernel<0>, L[2], tmp, depth_out, batch, h, w, pl.taps);
}

extern "C" int d2s_post_process_to(const float* depth_in, float* depth_out, int batch, int h, int w, const d2s_post_params* p,
                                   void* workspace, uint64_t workspace_bytes, void* stream) {
    D2S_REQUIRE(depth_in && depth_out && p && workspace, "null pointer");
    D2S_REQUIRE(batch > 0 && h > 0 && w > 0, "bad shape");
    D2S_REQUIRE(workspace_bytes >= d2s_post_process_workspace(batch, h, w), "workspace too small");
    if (const int rc = check_post_params(p)) return rc;
    {   // in place (equal pointers) or disjoint: a partially overlapping pair would be corrupted silently by every form
        const char *i0 = (const char*)depth_in, *o0 = (const char*)depth_out;
        const size_t nb = (size_t)batch * h * w * sizeof(float);
        D2S_REQUIRE(depth_out == depth_in || i0 + nb <= o0 || o0 + nb <= i0, "d2s_post_process_to: depth_in and depth_out overlap without being equal");
    }
    float* tmp = (float*)workspace;
    float* bounds = (float*)((char*)workspace + (((uint64_t)batch * h * w * sizeof(float) + 255) & ~255ull));
    launch_post(plan_post(batch, h, w, p, depth_out == depth_in), depth_in, depth_out, batch, h, w, p, tmp, bounds, (hipStream_t)stream);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

extern "C" int d2s_post_plan(int batch, int h, int w, const d2s_post_params* p, int in_place, d2s_post_plan_result* res) {
    D2S_REQUIRE(p && res, "null pointer");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_post_plan_result), "d2s_post_plan_result.struct_size must be sizeof(d2s_post_plan_result)");
    D2S_REQUIRE(batch > 0 && h > 0 && w > 0, "bad shape");
    if (const int rc = check_post_params(p)) return rc;
    const PostPlan pl = plan_post(batch, h, w, p, in_place != 0);
    *res = d2s_post_plan_result{sizeof(d2s_post_plan_result), pl.form, pl.nlaunch, pl.taps.k, pl.r, pl.sub.step, pl.sub.m, pl.sub.tail, {}, {}};
    for (int i = 0; i < pl.nlaunch; ++i) {
        res->lds_bytes[i] = (uint32_t)pl.launch[i].lds;
        snprintf(res->kernel[i], sizeof(res->kernel[i]), "%s", pl.launch[i].name);
    }
    return D2S_OK;
}

extern "C" int d2s_post_process(float* depth, int batch, int h, int w, const d2s_post_params* p,
                                void* workspace, uint64_t workspace_bytes, void* stream) {
    return d2s_post_process_to(depth, depth, batch, h, w, p, workspace, workspace_bytes, stream);
}

extern "C" int d2s_ema_update(float* depth, float* state, int initialised, int h, int w, float alpha, void* stream) {
    D2S_REQUIRE(depth && state && h > 0 && w > 0, "bad argument");
    hipLaunchKernelGGL(ema_kernel, dim3(cdiv((long)h * w, 256)), dim3(256), 0, (hipStream_t)stream,
                       depth, state, initialised, 1, h * w, 1.0f - alpha);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

namespace d2s {
// engine-internal: EMA over a batch of frames in order
int ema_rows(float* depth, float* state, int rows, const EmaRows& tab, int hw, float alpha, hipStream_t st) {
    if (rows < 1 || rows > TA_MAX_ROWS) { set_error("ema_rows: bad row count"); return D2S_E_INVALID; }
    hipLaunchKernelGGL(ema_rows_kernel, dim3(cdiv(hw, 256), rows), dim3(256), 0, st, depth, state, hw, 1.0f - alpha, tab);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

int ema_batch(float* depth, float* state, int initialised, int nframes, int hw, float alpha, hipStream_t st) {
    hipLaunchKernelGGL(ema_kernel, dim3(cdiv(hw, 256)), dim3(256), 0, st, depth, state, initialised, nframes, hw, 1.0f - alpha);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}
}  // namespace d2s
