// The panorama background of the OpenXR eye views (d2s_dibr_xr_eyes_panorama; reference _render_panorama_background,
// xr_viewer/effects.py:930-1021, shader _PANORAMA_FRAG, xr_viewer/glsl.py:57-94): the host's d2s_xr_panorama ->
// XrPanoDev, the equirectangular coordinate of a pixel's ray, the implicit LOD of texture() by the renderer's 2 x 2 quad rule, and
// the trilinear REPEAT / CLAMP_TO_EDGE fetch from the panorama and its d2s_mip_chain.  Built with -ffp-contract=off, as dibr.hip is.
#pragma once
#include "dibr_tex.h"
#include "mip.h"

namespace d2s {

// What the kernel takes in its arguments.  ray[eye]: row-major 3 x 3 from the pixel centre relative to the image centre (xc, yc, 1),
// y down (XrPix), to an un-normalised world direction: the caller's NDC matrix with the eye image's pixel -> NDC map folded in and
// scaled so that its largest entry is 1 (atan2 does not care).  Level k >= 1 of the chain is max(1, W >> k) x max(1, H >> k)
// (floor-halving composes, mip.h) and the levels lie one after another, so a level's offset is a sum the kernel forms itself.
struct XrPanoDev {
    float ray[2][9];
    float yaw, exposure;                          // u_yaw_offset in turns; max(u_exposure, 0)
    int flip;                                     // u_flip_y
    int H, W, q;
};
struct XrNoPano {};                               // the argument of the kernels without a panorama

// d2s_xr_panorama's refusals that need no device pointer (xr_plan), and the fold.  n_eyes, eyes: accepted by xr_screen_check before.
inline int xr_pano_check(const d2s_xr_panorama* pn, int n_eyes) {
    if (!pn) return D2S_OK;
    D2S_REQUIRE(pn->struct_size == sizeof(d2s_xr_panorama), "d2s_xr_panorama.struct_size must be sizeof(d2s_xr_panorama) = 176");
    D2S_REQUIRE(pn->flip_y == 0 || pn->flip_y == 1, "panorama flip_y must be 0 or 1");
    D2S_REQUIRE(pn->height >= 2 && pn->width >= 2 && pn->height <= 8192 && pn->width <= 8192,
                "panorama must be 2 .. 8192 on a side (d2s_mip_chain's range, the reference's texture cap)");
    D2S_REQUIRE(std::isfinite(pn->yaw_offset) && std::isfinite(pn->exposure), "the panorama's fields must be finite");
    for (int i = 0; i < n_eyes; ++i) {
        bool any = false, finite = true;
        for (int k = 0; k < 9; ++k) { finite = finite && std::isfinite(pn->ray[i][k]); any = any || pn->ray[i][k] != 0.0; }
        D2S_REQUIRE(finite, "the panorama's ray matrices must be finite");
        D2S_REQUIRE(any, "the panorama's ray matrix of an eye in use is all zero (xr.panorama_rays forms it)");
    }
    return D2S_OK;
}
struct XrEyeSize { int w, h; };
inline void xr_pano_dev(const d2s_xr_panorama* pn, const XrEyeSize* eyes, int n_eyes, XrPanoDev& P) {
    P = XrPanoDev{};
    for (int i = 0; i < n_eyes; ++i) {
        double m[9], big = 0.0;
        for (int r = 0; r < 3; ++r) {                      // ndc = (xc / (w / 2), -yc / (h / 2)): xr_facet_row's D, inverted
            m[3 * r] = pn->ray[i][3 * r] * 2.0 / eyes[i].w;
            m[3 * r + 1] = -pn->ray[i][3 * r + 1] * 2.0 / eyes[i].h;
            m[3 * r + 2] = pn->ray[i][3 * r + 2];
        }
        for (int k = 0; k < 9; ++k) big = fmax(big, fabs(m[k]));
        for (int k = 0; k < 9; ++k) P.ray[i][k] = (float)(m[k] / big);      // (big > 0: the all-zero matrix was refused)
    }
    P.yaw = (float)(pn->yaw_offset - floor(pn->yaw_offset));                // fract(u) takes whole turns out anyway
    P.exposure = (float)fmax(pn->exposure, 0.0);
    P.flip = pn->flip_y;
    MipShape ms;
    mip_shape(pn->height, pn->width, ms);
    P.H = pn->height; P.W = pn->width; P.q = ms.q;
}

#ifdef __HIPCC__
// atan(y, x) in turns, -0.5 .. 0.5.  The library's atan2f, an ulp or two: the coordinate is differenced between neighbouring
// pixels and scaled by the panorama's size, so a fast approximation of 1e-5 rad would show as whole levels of LOD.
__device__ __forceinline__ float pano_turns(float y, float x) { return atan2f(y, x) * 0.15915494309189535f; }

// (fract(u), clamp(v, 0, 1)) of the pixel centre (xc, yc): glsl.py:81-91.  The direction is not normalised: atan(x, -z) does not
// need it, and asin(clamp(y / |d|)) is atan(y, |(x, z)|), exact at the poles where asin of a rounded y / |d| loses half its bits.
struct PanoUv { float u, v; };
__device__ __forceinline__ PanoUv pano_uv(const XrPanoDev& P, const float* __restrict__ m, float xc, float yc) {
    const float dx = m[0] * xc + m[1] * yc + m[2], dy = m[3] * xc + m[4] * yc + m[5], dz = m[6] * xc + m[7] * yc + m[8];
    const float u = pano_turns(dx, -dz) + 0.5f + P.yaw;
    float v = 0.5f - 2.0f * pano_turns(dy, sqrtf(dx * dx + dz * dz));
    if (P.flip) v = 1.0f - v;
    PanoUv o;
    o.u = u - floorf(u); o.v = fminf(fmaxf(v, 0.f), 1.f);
    return o;
}
// One GL_LINEAR tap of a uint8 RGB level [h][w][3]: REPEAT in x with the level's own width, CLAMP_TO_EDGE in y.  Every index is
// brought into the level before it is used.
__device__ __forceinline__ void pano_level(const uint8_t* __restrict__ lev, int w, int h, float u, float v, float o[3]) {
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f, x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = wrapi((int)x0f, w), x1 = x0 + 1 == w ? 0 : x0 + 1;
    const int y0 = min(max((int)y0f, 0), h - 1), y1 = min(max((int)y0f + 1, 0), h - 1);
    const uint8_t* a = lev + ((long)y0 * w + x0) * 3;
    const uint8_t* b = lev + ((long)y0 * w + x1) * 3;
    const uint8_t* c = lev + ((long)y1 * w + x0) * 3;
    const uint8_t* d = lev + ((long)y1 * w + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = lerp2((float)a[k], (float)b[k], (float)c[k], (float)d[k], fx, fy);
}
// level l's size and, for l >= 1, its texels within the chain
__device__ __forceinline__ const uint8_t* pano_level_at(const XrPanoDev& P, const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ chain,
                                                        int l, int& w, int& h) {
    long off = 0;
    for (int j = 1; j < l; ++j) off += (long)max(1, P.W >> j) * max(1, P.H >> j) * 3;
    w = max(1, P.W >> l); h = max(1, P.H >> l);
    return l == 0 ? rgb : chain + off;
}

// The background policy of xr_tail: what an uncovered pixel starts from.  No panorama: the clear colour.
struct XrClearBg {
    using Dev = XrNoPano;
    static constexpr bool ON = false;
    template <class EX, class PX> __device__ __forceinline__ void operator()(const EX& ex, const PX&, float c[4]) const {
        c[0] = ex.clear[0] * 255.0f; c[1] = ex.clear[1] * 255.0f; c[2] = ex.clear[2] * 255.0f; c[3] = ex.clear[3];
    }
};
// The panorama.  texture()'s level is the renderer's: ONE per 2 x 2 quad of GL window pixels, quads aligned to even window x and y
// counted from the bottom-left, from the forward differences of the quad's lower-left pixel -- c(x0 + 1, y0) - c(x0, y0) and
// c(x0, y0 + 1) - c(x0, y0) of the coordinate that is sampled, fract() included, so a quad the u seam crosses takes the coarsest
// levels, as the reference's render shows.  The library's row y is window row h - 1 - y whatever the eye's flip_y (that lives in the
// matrices), so window y0 + 1 is the row ABOVE: with an odd height the top row is a quad of its own.  The three points are
// evaluated where they lie, outside the image or under the screen included; every thread forms its own quad's (no lane exchange: a
// 16 x 16 tile does not align with the quads of an odd height).
struct XrPanoBg {
    using Dev = XrPanoDev;
    static constexpr bool ON = true;
    const XrPanoDev& P;
    const uint8_t* __restrict__ rgb;
    const uint8_t* __restrict__ chain;
    template <class EX, class PX> __device__ __forceinline__ void operator()(const EX&, const PX& px, float c[4]) const {
        const float* __restrict__ m = P.ray[px.ei];
        const int gy = px.e.h - 1 - px.y, qx = px.x & ~1, qy = px.e.h - 1 - (gy & ~1);      // the quad's lower-left pixel, library row
        const float x00 = ((float)qx + 0.5f) - 0.5f * (float)px.e.w, y00 = ((float)qy + 0.5f) - 0.5f * (float)px.e.h;
        const PanoUv own = pano_uv(P, m, px.xc, px.yc);
        const PanoUv c00 = pano_uv(P, m, x00, y00), c10 = pano_uv(P, m, x00 + 1.0f, y00), c01 = pano_uv(P, m, x00, y00 - 1.0f);
        const float fw = (float)P.W, fh = (float)P.H;
        const float ax = (c10.u - c00.u) * fw, ay = (c10.v - c00.v) * fh, bx = (c01.u - c00.u) * fw, by = (c01.v - c00.v) * fh;
        const float rho2 = fmaxf(ax * ax + ay * ay, bx * bx + by * by);
        const float lam = fminf(fmaxf(0.5f * __builtin_amdgcn_logf(rho2), 0.f), (float)P.q), l0f = floorf(lam), f = lam - l0f;
        const int l0 = (int)l0f, l1 = min(l0 + 1, P.q);
        int w0, h0, w1, h1;
        const uint8_t* __restrict__ lev0 = pano_level_at(P, rgb, chain, l0, w0, h0);
        const uint8_t* __restrict__ lev1 = pano_level_at(P, rgb, chain, l1, w1, h1);
        float a[3], b[3];
#ifdef D2S_PANO_NO_FETCH      // a timing aid (tools/build_variant.sh, never the shipped build): the eight texel loads cut out, the arithmetic kept live
        a[0] = a[1] = a[2] = own.u * (float)(w0 + h0) + (float)(lev0 == rgb);
        b[0] = b[1] = b[2] = own.v * (float)(w1 + h1) + (float)(lev1 == rgb);
#else
        pano_level(lev0, w0, h0, own.u, own.v, a);
        pano_level(lev1, w1, h1, own.u, own.v, b);
#endif
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = fminf(fmaxf((a[k] * (1.0f - f) + b[k] * f) * P.exposure, 0.f), 255.0f);
        c[3] = 1.0f;
    }
};
#endif

}  // namespace d2s
