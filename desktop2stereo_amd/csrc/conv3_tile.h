// Pieces the 3x3 convolution kernels of conv3.hip share: which output tile
// a block works on, where that tile's input lies, the weight fragments the register-resident kernels preload and the fused head
// tail.  Plain inlined structs and functions: every kernel keeps its own schedule, LDS layout and loaders.
//   C3Tiles::org      conv3_head<0|1>, conv3_head_ups, conv3_c128_ups, conv3_wide, conv3_rcu<0|1>  (the one-shot row-tile kernels conv3_halo2 and
//                     conv3_halo keep their inline origin: with org's prologue they measured slower, profiles/conv3_shared_ab.md)
//   C3Tiles::src_org  conv3_head<1>, conv3_head_ups (rows only, through its tile_geo), conv3_c128_ups
//   C3Walk            conv3_head<0|1>, conv3_head_ups, conv3_c128_ups, conv3_wide
//   c3_load_wfrags    conv3_head<0|1>, conv3_head_ups, conv3_c128_ups
//   c3_head_consts    conv3_head<0|1>, conv3_head_ups
//   c3_head_dot       conv3_halo2 (MAP_HEAD), conv3_head<0|1>, conv3_head_ups
// The ReLU-on-load (relu_frag) and the row-tile epilogue (conv_tile_epilogue) are in gemm_epi.h beside conv_halo_fill.
// Register use and instruction counts of every kernel before and after this sharing: profiles/conv3_shared_isa.md.
#pragma once
#include "gemm_epi.h"

namespace d2s {

// The TH x TW-pixel output tiles of a batch of Ho x Wo maps, numbered frame by frame and row-major inside a frame.
template <int TH, int TW> struct C3Tiles {
    int tiles_x, tiles_y;
    __device__ __forceinline__ explicit C3Tiles(const GemmA& a) : tiles_x((a.Wo + TW - 1) / TW), tiles_y((a.Ho + TH - 1) / TH) {}
    __device__ __forceinline__ int per_img() const { return tiles_y * tiles_x; }
    // tile t -> its frame and its first output row / column
    __device__ __forceinline__ void org(int t, int& b, int& ty0, int& tx0) const {
        b = t / (tiles_y * tiles_x);
        const int r = t - b * (tiles_y * tiles_x);
        ty0 = (r / tiles_x) * TH; tx0 = (r % tiles_x) * TW;
    }
    // a.ups: first source row / column under the halo of the tile at (ty0, tx0); the staged source window starts there
    __device__ __forceinline__ static void src_org(const GemmA& a, int ty0, int tx0, int& rs0, int& cs0) {
        rs0 = linear_tap(ty0 > 0 ? ty0 - 1 : 0, a.usy, a.Hs, true).i0;
        cs0 = linear_tap(tx0 > 0 ? tx0 - 1 : 0, a.usx, a.Ws, true).i0;
    }
};

// Tile walk of the persistent blocks: XCD x (= blockIdx % 8) owns the contiguous run [x per, (x + 1) per) and its CUs take consecutive
// tiles of it, so the overlapping windows of neighbouring tiles meet in ONE L2 (in launch order -- tile = block + k grid -- neighbours
// sat on eight XCDs: PMC with the up-sample folded in, profiles/r3_06: L2 hit 0.15, 376 MB fetched per launch for a 204 MB source).
// A grid that is no multiple of 8 walks in launch order; XCD_ONLY leaves that branch out for a kernel whose planner always launches
// a multiple of 8 blocks (conv3_wide_kernel: with the branch <16,16> spills a scalar register).  at(k): the k-th tile of this
// block, -1 past its last.
template <bool XCD_ONLY = false> struct C3Walk {
    int ntiles, xcd_, slot_, nslot_, per_;
    bool xcd_walk;
    __device__ __forceinline__ explicit C3Walk(int ntiles_)
        : ntiles(ntiles_), xcd_(blockIdx.x & 7), slot_(blockIdx.x >> 3), nslot_(gridDim.x >> 3), per_((ntiles_ + 7) >> 3), xcd_walk((gridDim.x & 7) == 0) {}
    __device__ __forceinline__ int at(int k) const {
        if constexpr (!XCD_ONLY)
            if (!xcd_walk) { const int tt = blockIdx.x + k * gridDim.x; return tt < ntiles ? tt : -1; }
        const int j = slot_ + k * nslot_, tt = xcd_ * per_ + j;
        return (j < per_ && tt < ntiles) ? tt : -1;
    }
};

// W as MFMA fragments in registers, once per block: row n0 + j * 16 + fr (zeros from row N on), K step (tap, ks) -> chunk ks * 4 + fg of
// the tap's C channels
template <int C, int KS, int NJ>
__device__ __forceinline__ void c3_load_wfrags(u32x4 (&wf)[9][KS][NJ], const bf16_t* __restrict__ W, int N, int Kpad, int n0, int fr, int fg) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + j * 16 + fr;
                wf[tap][ks][j] = n < N ? *(const u32x4*)(W + (long)n * Kpad + tap * C + (ks * 4 + fg) * 8) : (u32x4){0u, 0u, 0u, 0u};
            }
}

// MAP_HEAD constants of this lane's columns j * 16 + fg * 4 ..: conv2's bias (cb) and conv3's 1x1 weights (cw), zeros from column N on
__device__ __forceinline__ void c3_head_consts(const GemmEpi& e, int N, int fg, float (&cb)[2][4], float (&cw)[2][4]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n0 = j * 16 + fg * 4;
        if (n0 < N) { load4(e.bias + n0, cb[j]); load4(e.scale + n0, cw[j]); }
        else { cb[j][0] = cb[j][1] = cb[j][2] = cb[j][3] = 0.f; cw[j][0] = cw[j][1] = cw[j][2] = cw[j][3] = 0.f; }
    }
}

// The fused head tail of one column fragment: sum over its four channels of relu(acc + bias) * w3.  A pixel's depth is
// act(b3 + the sum of these over its column fragments and its four lane groups); how the lane groups are summed is the kernel's.
__device__ __forceinline__ float c3_head_dot(const f32x4& acc, const float (&cb)[4], const float (&cw)[4]) {
    return fmaxf(acc[0] + cb[0], 0.f) * cw[0] + fmaxf(acc[1] + cb[1], 0.f) * cw[1] + fmaxf(acc[2] + cb[2], 0.f) * cw[2] + fmaxf(acc[3] + cb[3], 0.f) * cw[3];
}

}  // namespace d2s
