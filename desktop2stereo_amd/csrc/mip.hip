// d2s_mip_chain: the mip chain glGenerateMipmap builds for the OpenXR viewer's colour texture (xr_viewer/effects.py:597-646), which the
// glow, frost and veil passes sample with textureLod.  Restated from renders (tests/golden/make_golden_xr_glow.py): level k is
// max(1, floor(n / 2)) per axis; each texel is the bilinear sample of the ALREADY 8-BIT level k - 1 at the texel's normalised centre,
//     source coordinate = (i + 0.5) * n_prev / n_k - 0.5   (clamped to the edge),
// rounded half to even.  The weights are rationals with denominator 2 * n_k, so everything here is integer arithmetic and exact; where
// both sizes are even the sample is the 2 x 2 box.
//
// Launches: (1) while a level is too large for LDS, mip_box_kernel takes it down through up to three levels that are 2 : 1 in both
// axes -- a 64 x 64 tile per block, the only HBM-sized read -- or, where a size is odd, mip_step_kernel takes one general step;
// (2) mip_tail_kernel, one workgroup per frame, holds the first level of at most MIP_TAIL_SRC bytes in LDS and walks the rest of the
// chain down to 1 x 1 with a barrier per level.  1920 x 1080: box (960 x 540, 480 x 270, 240 x 135), step (120 x 67), tail (60 x 33 .. 1 x 1).
#include "mip.h"

namespace d2s {

// The tail's first level, in LDS.  One workgroup walks the tail, so what it starts from is kept small: from 1080p's 240 x 135 level
// (97 KB, which LDS would hold) the tail took 40 us, 24 texel-channels per thread in its first step; that step as a grid-wide launch
// and the tail from 120 x 67 is a fraction of it.
constexpr int MIP_TAIL_SRC = 32 * 1024;
constexpr int MIP_TAIL_DST = 16 * 1024;       // the level under it: at most a quarter of it (both sizes >= 2), or half of <= 24 KB (a size of 1)

// round(num / den) half to even; den > 0
// (num < 2^34, den <= 2^26, the quotient <= 255: a float quotient is within 1 of it and the remainder puts it right -- a 64-bit
// division is ~10 x the rest of a texel here)
__device__ __forceinline__ uint32_t mip_round(uint64_t num, uint32_t den) {
    int64_t q = (int64_t)((float)num / (float)den);
    int64_t r = (int64_t)num - q * den;
    if (r < 0) { --q; r += den; }
    if (r >= den) { ++q; r -= den; }
    if (r < 0) { --q; r += den; }
    if (r >= den) { ++q; r -= den; }
    const int64_t r2 = 2 * r;
    if (r2 > den || (r2 == den && (q & 1))) ++q;
    return (uint32_t)q;
}
// one axis of texel i: the two source texels and the second one's weight r over den = 2 * nk
__device__ __forceinline__ void mip_axis(int i, int np, int nk, int& i0, int& i1, uint32_t& r) {
    const uint32_t num = (uint32_t)(2 * i + 1) * (uint32_t)np - (uint32_t)nk, den = 2u * (uint32_t)nk;      // >= 0: np >= nk
    i0 = (int)(num / den);
    r = num - (uint32_t)i0 * den;
    if (i0 >= np - 1) { i0 = np - 1; r = 0; }      // CLAMP_TO_EDGE
    i1 = i0 + 1 < np ? i0 + 1 : np - 1;
}
// texel (x, y), channel c of the level under src [hp, wp, 3]
__device__ __forceinline__ uint8_t mip_texel(const uint8_t* src, int hp, int wp, int hk, int wk, int x, int y, int c) {
    int x0, x1, y0, y1;
    uint32_t rx, ry;
    mip_axis(x, wp, wk, x0, x1, rx);
    mip_axis(y, hp, hk, y0, y1, ry);
    const uint32_t dx = 2u * wk, dy = 2u * hk;
    const uint64_t top = (uint64_t)(dx - rx) * src[(y0 * wp + x0) * 3 + c] + (uint64_t)rx * src[(y0 * wp + x1) * 3 + c];
    const uint64_t bot = (uint64_t)(dx - rx) * src[(y1 * wp + x0) * 3 + c] + (uint64_t)rx * src[(y1 * wp + x1) * 3 + c];
    return (uint8_t)mip_round((uint64_t)(dy - ry) * top + (uint64_t)ry * bot, dx * dy);
}

// One general step, global to global: one thread = one byte of the new level.
__global__ void __launch_bounds__(256)
mip_step_kernel(const uint8_t* __restrict__ src_all, long src_stride, uint8_t* __restrict__ dst_all, long dst_stride, int hp, int wp, int hk, int wk) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= hk * wk * 3) return;
    const int c = idx % 3, px = idx / 3;
    dst_all[blockIdx.y * dst_stride + idx] = mip_texel(src_all + blockIdx.y * src_stride, hp, wp, hk, wk, px % wk, px / wk, c);
}

// n (1 .. 3) levels that are 2 : 1 in both axes: h and w are multiples of 2^n.  A block = a 64 x 64 tile of the source (less at the
// right and bottom edges, still a multiple of 2^n), staged in LDS as bytes; each new level is written to LDS and to its place in the
// chain.  The 2 x 2 box: (a + b + c + d) / 4 rounded half to even.
struct MipBoxDst { uint32_t off[3]; };
__global__ void __launch_bounds__(256)
mip_box_kernel(const uint8_t* __restrict__ src_all, long src_stride, uint8_t* __restrict__ dst_all, long dst_stride, int h, int w, int n, MipBoxDst d) {
    __shared__ __attribute__((aligned(16))) uint8_t lv0[64 * 64 * 3];
    __shared__ uint8_t lv1[32 * 32 * 3], lv2[16 * 16 * 3];
    const int tid = threadIdx.x, x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    const int vw = min(64, w - x0), vh = min(64, h - y0);
    const uint8_t* src = src_all + blockIdx.z * src_stride;
    uint8_t* dst = dst_all + blockIdx.z * dst_stride;
    if ((((uintptr_t)src | (uintptr_t)(w * 3) | (uintptr_t)(vw * 3)) & 3) == 0) {      // every row of the tile starts and ends on a dword
        const int dpr = vw * 3 / 4, nd = vh * dpr;                                           // <= 48 per row, <= 12 per thread: all requested at once
        uint32_t v[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int i = tid + 256 * j, row = i / dpr, col = i - row * dpr;
            v[j] = i < nd ? ((const uint32_t*)(src + ((long)(y0 + row) * w + x0) * 3))[col] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int i = tid + 256 * j, row = i / dpr, col = i - row * dpr;
            if (i < nd) ((uint32_t*)lv0)[row * 48 + col] = v[j];
        }
    } else {
        for (int i = tid; i < vh * vw * 3; i += 256) {
            const int row = i / (vw * 3), col = i - row * (vw * 3);
            lv0[row * 192 + col] = src[((long)(y0 + row) * w + x0) * 3 + col];
        }
    }
    __syncthreads();
    const uint8_t* from = lv0;
    uint8_t* to = lv1;
    for (int j = 1; j <= n; ++j) {
        const int ss = 64 >> (j - 1), ds = 64 >> j, lw = vw >> j, lh = vh >> j, gw = w >> j;
        uint8_t* g = dst + d.off[j - 1] + ((long)(y0 >> j) * gw + (x0 >> j)) * 3;
        for (int i = tid; i < lh * lw * 3; i += 256) {
            const int row = i / (lw * 3), col = i - row * (lw * 3), px = col / 3, c = col - px * 3;
            const uint8_t* p = from + ((2 * row) * ss + 2 * px) * 3 + c;
            const uint32_t s = (uint32_t)p[0] + p[3] + p[ss * 3] + p[ss * 3 + 3];
            uint32_t q = s >> 2;
            const uint32_t r = s & 3u;
            q += (r == 3u || (r == 2u && (q & 1u))) ? 1u : 0u;
            if (j < n) to[(row * ds + px) * 3 + c] = (uint8_t)q;
            g[(long)row * gw * 3 + col] = (uint8_t)q;
        }
        __syncthreads();
        from = to;
        to = lv2;
    }
}

// The rest of the chain in one workgroup per frame: level `first` (<= MIP_TAIL_SRC bytes; 0 = the frame) is copied into LDS, then
// every further level is formed from the one above it in LDS and written to the chain.
__global__ void __launch_bounds__(1024)
mip_tail_kernel(const uint8_t* __restrict__ rgb_all, long rgb_stride, uint8_t* __restrict__ lev_all, MipShape s, int first) {
    __shared__ __attribute__((aligned(16))) uint8_t big[MIP_TAIL_SRC];
    __shared__ uint8_t small[MIP_TAIL_DST];
    const int tid = threadIdx.x;
    uint8_t* lev = lev_all + (long)blockIdx.x * s.total;
    const uint8_t* src = first == 0 ? rgb_all + blockIdx.x * rgb_stride : lev + s.off[first];
    const int n0 = s.h[first] * s.w[first] * 3;
    if ((((uintptr_t)src | (uintptr_t)n0) & 3) == 0) {                                      // dwords, eight requests in flight per thread
        const uint32_t* s4 = (const uint32_t*)src;
        const int n4 = n0 / 4;
        for (int i0 = tid; i0 < n4; i0 += 8 * 1024) {
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = i0 + 1024 * j < n4 ? s4[i0 + 1024 * j] : 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) if (i0 + 1024 * j < n4) ((uint32_t*)big)[i0 + 1024 * j] = v[j];
        }
    } else {
        for (int i = tid; i < n0; i += 1024) big[i] = src[i];
    }
    __syncthreads();
    uint8_t* from = big;
    uint8_t* to = small;
    for (int k = first + 1; k <= s.q; ++k) {
        const int hp = s.h[k - 1], wp = s.w[k - 1], hk = s.h[k], wk = s.w[k];
        uint8_t* g = lev + s.off[k];
        for (int i = tid; i < hk * wk * 3; i += 1024) {
            const int c = i % 3, px = i / 3;
            const uint8_t v = mip_texel(from, hp, wp, hk, wk, px % wk, px / wk, c);
            to[i] = v;
            g[i] = v;
        }
        __syncthreads();
        uint8_t* t = from; from = to; to = t;
    }
}

static int mip_check(int H, int W) {
    D2S_REQUIRE(H >= 2 && W >= 2 && H <= 8192 && W <= 8192, "frame must be 2 .. 8192 on a side");
    return D2S_OK;
}

}  // namespace d2s

using namespace d2s;

extern "C" int d2s_mip_shape(int H, int W, int* n_levels, uint64_t* offsets, int* hs, int* ws, uint64_t* total_bytes) {
    D2S_REQUIRE(n_levels && offsets && hs && ws && total_bytes, "null pointer (n_levels, offsets, hs, ws, total_bytes)");
    int rc = mip_check(H, W);
    if (rc) return rc;
    MipShape s;
    mip_shape(H, W, s);
    *n_levels = s.q;
    for (int k = 1; k <= s.q; ++k) { offsets[k - 1] = s.off[k]; hs[k - 1] = s.h[k]; ws[k - 1] = s.w[k]; }
    *total_bytes = s.total;
    return D2S_OK;
}

extern "C" int d2s_mip_chain(const uint8_t* rgb, int batch, int H, int W, uint8_t* levels, void* stream) {
    D2S_REQUIRE(rgb && levels, "null pointer (rgb, levels)");
    D2S_REQUIRE(batch >= 1 && batch <= 65535, "bad batch (1 .. 65535)");
    int rc = mip_check(H, W);
    if (rc) return rc;
    MipShape s;
    mip_shape(H, W, s);
    hipStream_t st = (hipStream_t)stream;
    const long rgb_stride = (long)H * W * 3;
    int k = 0;                                             // the finest level formed so far
    while ((long)s.h[k] * s.w[k] * 3 > MIP_TAIL_SRC) {
        const uint8_t* src = k == 0 ? rgb : levels + s.off[k];
        const long src_stride = k == 0 ? rgb_stride : (long)s.total;
        int n = 0;
        while (n < 3 && s.h[k] % (2 << n) == 0 && s.w[k] % (2 << n) == 0) ++n;
        if (n > 0) {
            MipBoxDst d = {};
            for (int j = 0; j < n; ++j) d.off[j] = s.off[k + 1 + j];
            hipLaunchKernelGGL(mip_box_kernel, dim3(cdiv(s.w[k], 64), cdiv(s.h[k], 64), batch), dim3(256), 0, st, src, src_stride, levels,
                               (long)s.total, s.h[k], s.w[k], n, d);
            k += n;
        } else {
            hipLaunchKernelGGL(mip_step_kernel, dim3(cdiv((long)s.h[k + 1] * s.w[k + 1] * 3, 256), batch), dim3(256), 0, st, src, src_stride,
                               levels + s.off[k + 1], (long)s.total, s.h[k], s.w[k], s.h[k + 1], s.w[k + 1]);
            k += 1;
        }
        D2S_CHECK_LAUNCH();
    }
    if ((long)s.h[k + 1] * s.w[k + 1] * 3 > MIP_TAIL_DST) { set_error("internal: the mip tail's second level does not fit"); return D2S_E_INVALID; }
    hipLaunchKernelGGL(mip_tail_kernel, dim3(batch), dim3(1024), 0, st, rgb, rgb_stride, levels, s, k);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}
