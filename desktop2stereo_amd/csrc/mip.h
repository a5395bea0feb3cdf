// The colour mip chain's layout (d2s_mip_shape, d2s_mip_chain, mip.hip) -- shared with the glow pass of the OpenXR eye kernel (dibr.hip),
// which reads the chain's coarse levels.  Level k of an H x W frame is max(1, floor(size of level k - 1 / 2)) per axis, levels 1 .. q
// with q = floor(log2(max(H, W))): what glGenerateMipmap allocates (the reference: xr_viewer/effects.py:597-646).
#pragma once
#include "common.h"

namespace d2s {

constexpr int MIP_MAX_LEVELS = 14;      // q = 13 for an 8192-wide frame; [0] is the frame itself
struct MipShape {
    int q;                               // the last level, 1 x 1
    int h[MIP_MAX_LEVELS], w[MIP_MAX_LEVELS];
    uint32_t off[MIP_MAX_LEVELS];        // byte offset of level k >= 1 within one frame's chain (uint8 RGB, HWC); off[0] is unused
    uint32_t total;                      // bytes of one frame's chain (< 2^27: a third of an 8192 x 8192 x 3 frame)
};

// H, W in 2 .. 8192 (checked by the callers)
inline void mip_shape(int H, int W, MipShape& s) {
    s = MipShape{};
    s.h[0] = H; s.w[0] = W;
    uint32_t at = 0;
    int k = 0;
    while (s.h[k] > 1 || s.w[k] > 1) {
        ++k;
        s.h[k] = s.h[k - 1] / 2 > 1 ? s.h[k - 1] / 2 : 1;
        s.w[k] = s.w[k - 1] / 2 > 1 ? s.w[k - 1] / 2 : 1;
        s.off[k] = at;
        at += (uint32_t)s.h[k] * s.w[k] * 3;
    }
    s.q = k;
    s.total = at;
}

}  // namespace d2s
