// Texture filtering, samplers and in-painting helpers shared by the DIBR kernels: f1 (dibr.hip, the reference's FRAGMENT_SHADER)
// and the viewer's composite modes (dibr_composite.hip: Anaglyph, Interleaved, Interleaved-V, Depth Map).  Both files are built
// with -ffp-contract=off: the float32 operation sequence is the shader's, term for term.  Line numbers below are viewer.py.
#pragma once
#include "common.h"
#include <math.h>
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace d2s {

struct DibrGeom {
    int H, W;              // source frame == depth size
    int oh, ow;            // per-eye viewport
    int mode;              // D2S_MODE_*: where the two eyes land in the output
    int out_h, out_w;      // packed output
    float c, s;            // cos / sin(u_roll)
    float psx, psy;        // pixel_size
    float half_ipd, strength, conv;
    float tol, blur, feather_w;
    int search, feather;
    int alpha_mode;        // D2S_DIBR_ALPHA_*
    float corner_r, vpx, vpy, vpw, vph;             // u_corner_radius; u_viewport in eye-image pixels (y up)
    float w1[20], w2[20];  // exp(-i*0.15), exp(-i*0.2), i < 16 (the sweeps index in groups of four: up to [16..18], never used)
    int dh, dw;            // UpDep only: the [dh, dw] map the H x W depth texture is up-sampled from, and its scales
    float dsy, dsx;        //   linear_scale(dh, H, false), linear_scale(dw, W, false) as d2s_upsample_depth forms them
    static constexpr bool crop = false;
    static constexpr bool proj = false;
};
// d2s_dibr_warp_crop: the OpenXR screen shader's u_source_crop (xr_viewer/implementation.py:111-126) as (float) of the caller's
// doubles, the way GL receives a uniform.  A geometry TYPE of its own: the kernels are templates over it, so the instantiations
// over DibrGeom -- every kernel that existed before the crop -- keep their argument block and their device code.
struct DibrGeomCrop : DibrGeom {
    float cx, cy, cw, ch;  // xy = source top-left, zw = source size, in uv of the full texture
    static constexpr bool crop = true;
};
// d2s_dibr_xr_eyes: the screen's own uv of a pixel comes from a projected facet (the kernel hands it to dibr_pixel) instead of the
// pixel index; everything after it is the cropped shader (crop NULL = (0, 0, 1, 1): x * 1 + 0 is x).  oh, ow, mode, out_h, out_w and
// the viewport are not used: the eye images have their own table (XrEyes, dibr.hip).
struct DibrGeomProj : DibrGeomCrop {
    static constexpr bool proj = true;
};
// flipped_uv = u_source_crop.xy + screen_flipped_uv * u_source_crop.zw (implementation.py:123): quad uv -> texture uv
template <class G> __device__ __forceinline__ float tex_u(const G& g, float us) { if constexpr (G::crop) return g.cx + us * g.cw; else return us; }
template <class G> __device__ __forceinline__ float tex_v(const G& g, float vs) { if constexpr (G::crop) return g.cy + vs * g.ch; else return vs; }

// GL_REPEAT index: one conditional add / subtract covers every coordinate within one period of the texture (all but
// absurd parallax settings); the integer modulo (~25 instructions on this ISA) is the fallback
__device__ __forceinline__ int wrapi(int i, int n) {
    if (i < 0) i += n; else if (i >= n) i -= n;
    if ((unsigned)i >= (unsigned)n) { i %= n; if (i < 0) i += n; }
    return i;
}

struct TexTap { int x0, x1, y0, y1; float fx, fy; };
__device__ __forceinline__ TexTap tex_tap(float u, float v, int H, int W) {
    float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    float x0f = floorf(x), y0f = floorf(y);
    TexTap t;
    t.fx = x - x0f; t.fy = y - y0f;
    t.x0 = wrapi((int)x0f, W); t.y0 = wrapi((int)y0f, H);
    t.x1 = t.x0 + 1 == W ? 0 : t.x0 + 1;
    t.y1 = t.y0 + 1 == H ? 0 : t.y0 + 1;
    return t;
}
__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float fx, float fy) {
    float top = a + (b - a) * fx, bot = c + (d - c) * fx;
    return top + (bot - top) * fy;
}
// Where a texel of the H x W depth texture comes from -- a template parameter of the samplers and kernels below.
//   FullDep: the texture itself, float [H, W] in memory (d2s_dibr_warp / d2s_dibr_composite).
//   UpDep:   a [dh, dw] map at model resolution (d2s_dibr_*_depth, d2s_view_pipeline_streams).  Texel (y, x) is the value
//            upsample_depth_kernel would have stored there (common.h upsample_texel: the same linear_tap calls, the same
//            w0 * a + w1 * b order, no contraction), so every filtered tap -- lerp2 over four texels, as FullDep's -- has the bits
//            of the two-call form without the full-resolution map ever existing.  The 0.6 MB map stays in L2.
// Row: the depth half of a texture row pair (y0, y1); pair(): texels (y0, x) and (y1, x).
struct FullDep {
    const float* dep;
    struct Row { const float* d0; const float* d1; };
    __device__ __forceinline__ static FullDep make(const float* dep_all, int b, const DibrGeom& g) { return FullDep{dep_all + (long)b * g.H * g.W}; }
    __device__ __forceinline__ Row row(int y0, int y1, int W) const { return Row{dep + y0 * W, dep + y1 * W}; }
    __device__ __forceinline__ void pair(const Row& r, int x, float& a, float& b) const { a = r.d0[x]; b = r.d1[x]; }
};
// Orders two on-demand texel evaluations: x becomes available only once `after` exists.  Left to itself the compiler requests the
// 16 (a row tap) or 32 (the two vertical-blur taps) source loads of the rare paths below at once, and their addresses and values
// take the row kernels past the 72 VGPRs of seven waves per SIMD into scratch.  No arithmetic: the bits are not affected.
__device__ __forceinline__ int ordered_after(int x, float after) { asm volatile("" : "+v"(x) : "v"(after)); return x; }
struct UpDep {
    const float* dep; int dh, dw; float sy, sx;
    // a texture row = two source rows (offsets into the map) and the weight of the second; w0 = 1 - w1 is re-formed where it is used
    // (linear_tap's own expression: the same bits) -- six block-uniform values instead of eight, the row kernels live at their SGPR limit
    struct RowTap { int o0, o1; float w1; };
    struct Row { RowTap t0, t1; };
    __device__ __forceinline__ static UpDep make(const float* dep_all, int b, const DibrGeom& g) {
        return UpDep{dep_all + (long)b * g.dh * g.dw, g.dh, g.dw, g.dsy, g.dsx};
    }
    __device__ __forceinline__ RowTap row_tap(int y) const { const Tap t = linear_tap(y, sy, dh, false); return RowTap{t.i0 * dw, t.i1 * dw, t.w1}; }
    __device__ __forceinline__ Row row(int y0, int y1, int) const { return Row{row_tap(y0), row_tap(y1)}; }
    __device__ __forceinline__ float one(const RowTap& r, const Tap& tx) const {
        Tap ty; ty.i0 = 0; ty.i1 = 0; ty.w1 = r.w1; ty.w0 = 1.0f - r.w1;
        return upsample_texel_rows(dep + r.o0, dep + r.o1, ty, tx);
    }
    __device__ __forceinline__ float one(const RowTap& r, int x) const { return one(r, linear_tap(x, sx, dw, false)); }
    __device__ __forceinline__ void pair(const Row& r, int x, float& a, float& b) const {
        const Tap tx = linear_tap(x, sx, dw, false);
        a = one(r.t0, tx);
        b = one(r.t1, tx);
    }
};
// The two texels of a row are adjacent except across the GL_REPEAT seam: one 8-byte load per row (gfx950 runs with
// unaligned access enabled: a dwordx2 at a 4-byte / a byte address is one instruction) instead of two 4-byte / six
// 1-byte loads -- the kernel is bound by the number of gather instructions, not by bytes.
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ float tex_depth(const float* __restrict__ dep, int H, int W, float u, float v) {
    TexTap t = tex_tap(u, v, H, W);
    const float* r0 = dep + t.y0 * W;                // (H * W < 2^31 / 3 is checked by the launcher: 32-bit texel indices)
    const float* r1 = dep + t.y1 * W;
    if (t.x1 == t.x0 + 1) {
        f32x2u a = *(const f32x2u*)(r0 + t.x0), b = *(const f32x2u*)(r1 + t.x0);
        return lerp2(a.x, a.y, b.x, b.y, t.fx, t.fy);
    }
    return lerp2(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.fx, t.fy);
}
__device__ __forceinline__ float tex_depth(const FullDep& d, int H, int W, float u, float v) { return tex_depth(d.dep, H, W, u, v); }
// ORD (the LDS-window kernels, which live at 72 VGPRs): one texel -- four source loads -- at a time (ordered_after); the gather
// kernels have the registers to request all sixteen at once.
template <bool ORD = false>
__device__ __forceinline__ float tex_depth(const UpDep& d, int H, int W, float u, float v) {
    const TexTap t = tex_tap(u, v, H, W);
    const float a = upsample_texel(d.dep, d.dh, d.dw, d.sy, d.sx, t.y0, t.x0);
    const float b = upsample_texel(d.dep, d.dh, d.dw, d.sy, d.sx, t.y0, ORD ? ordered_after(t.x1, a) : t.x1);
    const float c = upsample_texel(d.dep, d.dh, d.dw, d.sy, d.sx, t.y1, ORD ? ordered_after(t.x0, b) : t.x0);
    const float e = upsample_texel(d.dep, d.dh, d.dw, d.sy, d.sx, t.y1, ORD ? ordered_after(t.x1, c) : t.x1);
    return lerp2(a, b, c, e, t.fx, t.fy);
}
__device__ __forceinline__ void tex_color(const uint8_t* __restrict__ rgb, int H, int W, float u, float v, float o[3]) {
    TexTap t = tex_tap(u, v, H, W);
    const int ia = (t.y0 * W + t.x0) * 3, ic = (t.y1 * W + t.x0) * 3, end = H * W * 3;
    if (t.x1 == t.x0 + 1 && ia + 8 <= end && ic + 8 <= end) {          // (the 8-byte window must stay inside the frame)
        uint2 p, q;
        __builtin_memcpy(&p, rgb + ia, 8);
        __builtin_memcpy(&q, rgb + ic, 8);
        const float a[3] = {(float)(p.x & 255u), (float)((p.x >> 8) & 255u), (float)((p.x >> 16) & 255u)};
        const float b[3] = {(float)(p.x >> 24), (float)(p.y & 255u), (float)((p.y >> 8) & 255u)};
        const float c[3] = {(float)(q.x & 255u), (float)((q.x >> 8) & 255u), (float)((q.x >> 16) & 255u)};
        const float d[3] = {(float)(q.x >> 24), (float)(q.y & 255u), (float)((q.y >> 8) & 255u)};
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = lerp2(a[k], b[k], c[k], d[k], t.fx, t.fy);
        return;
    }
    const uint8_t* a = rgb + ia;
    const uint8_t* b = rgb + (t.y0 * W + t.x1) * 3;
    const uint8_t* c = rgb + ic;
    const uint8_t* d = rgb + (t.y1 * W + t.x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = lerp2((float)a[k], (float)b[k], (float)c[k], (float)d[k], t.fx, t.fy);
}
// roll == 0 (the desktop viewer; OpenXR sets a roll): every tap of a pixel except the two vertical-blur taps lies on the pixel's own
// texture row pair, so the y half of tex_tap -- v * H - 0.5, floor, GL_REPEAT wrap, the two row bases -- is formed ONCE per pixel
// (same expressions on the same v: the same bits as a per-tap evaluation) and a tap is its x half alone.
template <class D> struct RowCtx { typename D::Row d; int c0, c1; float fy; };
template <class D>
__device__ __forceinline__ RowCtx<D> row_ctx(const D& dep, int H, int W, float v) {
    const float y = v * (float)H - 0.5f, y0f = floorf(y);
    RowCtx<D> r;
    r.fy = y - y0f;
    const int y0 = wrapi((int)y0f, H), y1 = y0 + 1 == H ? 0 : y0 + 1;
    r.d = dep.row(y0, y1, W);
    r.c0 = y0 * W * 3; r.c1 = y1 * W * 3;
    return r;
}
struct XTap { int x0, x1; float fx; };
__device__ __forceinline__ XTap x_tap(float u, int W) {
    const float x = u * (float)W - 0.5f, x0f = floorf(x);
    XTap t;
    t.fx = x - x0f;
    t.x0 = wrapi((int)x0f, W);
    t.x1 = t.x0 + 1 == W ? 0 : t.x0 + 1;
    return t;
}
__device__ __forceinline__ float tex_depth_row(const FullDep&, const RowCtx<FullDep>& r, int W, float u) {
    const XTap t = x_tap(u, W);
    if (t.x1 == t.x0 + 1) {
        f32x2u a = *(const f32x2u*)(r.d.d0 + t.x0), b = *(const f32x2u*)(r.d.d1 + t.x0);
        return lerp2(a.x, a.y, b.x, b.y, t.fx, r.fy);
    }
    return lerp2(r.d.d0[t.x0], r.d.d0[t.x1], r.d.d1[t.x0], r.d.d1[t.x1], t.fx, r.fy);
}
template <bool ORD = false>       // (ORD: a tap that left the LDS window, as above)
__device__ __forceinline__ float tex_depth_row(const UpDep& d, const RowCtx<UpDep>& r, int W, float u) {
    const XTap t = x_tap(u, W);
    const float a = d.one(r.d.t0, t.x0);
    const float b = d.one(r.d.t0, ORD ? ordered_after(t.x1, a) : t.x1);
    const float c = d.one(r.d.t1, ORD ? ordered_after(t.x0, b) : t.x0);
    const float e = d.one(r.d.t1, ORD ? ordered_after(t.x1, c) : t.x1);
    return lerp2(a, b, c, e, t.fx, r.fy);
}
template <class D>
__device__ __forceinline__ void tex_color_row(const uint8_t* __restrict__ rgb, const RowCtx<D>& r, int H, int W, float u, float o[3]) {
    const XTap t = x_tap(u, W);
    const int ia = r.c0 + t.x0 * 3, ic = r.c1 + t.x0 * 3, end = H * W * 3;
    if (t.x1 == t.x0 + 1 && ia + 8 <= end && ic + 8 <= end) {
        uint2 p, q;
        __builtin_memcpy(&p, rgb + ia, 8);
        __builtin_memcpy(&q, rgb + ic, 8);
        const float a[3] = {(float)(p.x & 255u), (float)((p.x >> 8) & 255u), (float)((p.x >> 16) & 255u)};
        const float b[3] = {(float)(p.x >> 24), (float)(p.y & 255u), (float)((p.y >> 8) & 255u)};
        const float c[3] = {(float)(q.x & 255u), (float)((q.x >> 8) & 255u), (float)((q.x >> 16) & 255u)};
        const float d[3] = {(float)(q.x >> 24), (float)(q.y & 255u), (float)((q.y >> 8) & 255u)};
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = lerp2(a[k], b[k], c[k], d[k], t.fx, r.fy);
        return;
    }
    const uint8_t* a = rgb + ia;
    const uint8_t* b = rgb + r.c0 + t.x1 * 3;
    const uint8_t* c = rgb + ic;
    const uint8_t* d = rgb + r.c1 + t.x1 * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = lerp2((float)a[k], (float)b[k], (float)c[k], (float)d[k], t.fx, r.fy);
}
// Where a pixel's taps come from.  own_*: taps on the pixel's own texture row pair when roll == 0 (any (u, v) otherwise);
// any_*: the two vertical-blur taps of the in-painting (other rows), always the general gather.
template <class D>
struct GenSmp {                                    // general: every tap evaluates both coordinates (roll != 0)
    const uint8_t* rgb; D dep; int H, W;
    __device__ __forceinline__ float own_depth(float u, float v) const { return tex_depth(dep, H, W, u, v); }
    __device__ __forceinline__ void own_color(float u, float v, float o[3]) const { tex_color(rgb, H, W, u, v, o); }
    __device__ __forceinline__ float any_depth(float u, float v) const { return tex_depth(dep, H, W, u, v); }
    __device__ __forceinline__ void any_color(float u, float v, float o[3]) const { tex_color(rgb, H, W, u, v, o); }
    static constexpr bool up = std::is_same<D, UpDep>::value;
    static constexpr bool serial_blur = up;        // push_pull_finish: the two vertical-blur taps one after the other
};
template <class D>
struct RowSmp : GenSmp<D> {                        // roll == 0: the row pair is formed once per pixel
    RowCtx<D> rc;
    __device__ __forceinline__ float own_depth(float u, float) const { return tex_depth_row(this->dep, rc, this->W, u); }
    __device__ __forceinline__ void own_color(float u, float, float o[3]) const { tex_color_row(this->rgb, rc, this->H, this->W, u, o); }
};
// roll == 0, the block's row pair staged in LDS: a window of WW texels starting at (unwrapped) texel wx0, GL_REPEAT applied by
// the staging loop; planes d0 | d1 | R0 G0 B0 | R1 G1 B1 as floats (the same byte -> float conversions the gather path makes per
// tap).  A tap is index arithmetic + ds_read2_b32 pairs; taps that leave the window (parallax settings beyond the margin the
// launcher sized it for) take the row gather: same values either way.
// SERIAL: take the vertical-blur taps one after the other for FullDep too (the cropped row kernels with feather / corner code: their
// six loads requested together are 12 bytes of scratch at the 72 VGPRs of seven waves per SIMD).
template <class D, bool SERIAL = false>
struct WinSmp : RowSmp<D> {
    static constexpr bool serial_blur = SERIAL || RowSmp<D>::up;
    const float* dwin;          // [2][WW]: the row pair of the depth texture
    const float* cwin;          // [6][WW]: R0 G0 B0 R1 G1 B1 as floats
    int wx0, WW;
    __device__ __forceinline__ float own_depth(float u, float v) const {
        const float x = u * (float)this->W - 0.5f, x0f = floorf(x), fx = x - x0f;
        const int j = (int)x0f - wx0;
        if ((unsigned)j < (unsigned)(WW - 1)) {
            const float* p = dwin + j;
            return lerp2(p[0], p[1], p[WW], p[WW + 1], fx, this->rc.fy);
        }
        if constexpr (RowSmp<D>::up) return tex_depth_row<true>(this->dep, this->rc, this->W, u);
        else return RowSmp<D>::own_depth(u, v);
    }
    __device__ __forceinline__ void own_color(float u, float v, float o[3]) const {
        const float x = u * (float)this->W - 0.5f, x0f = floorf(x), fx = x - x0f;
        const int j = (int)x0f - wx0;
        if ((unsigned)j < (unsigned)(WW - 1)) {
            const float* p = cwin + j;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = lerp2(p[k * WW], p[k * WW + 1], p[(3 + k) * WW], p[(3 + k) * WW + 1], fx, this->rc.fy);
            return;
        }
        RowSmp<D>::own_color(u, v, o);
    }
    __device__ __forceinline__ float any_depth(float u, float v) const {
        if constexpr (RowSmp<D>::up) return tex_depth<true>(this->dep, this->H, this->W, u, v);
        else return RowSmp<D>::any_depth(u, v);
    }
};
__device__ __forceinline__ float smoothstepf(float e0, float e1, float x) {
    float t = fminf(fmaxf((x - e0) / (e1 - e0), 0.f), 1.f);
    return t * t * (3.f - 2.f * t);
}
// constant edges: 1 / (e1 - e0) is a literal (an IEEE division is ~20 instructions here and the kernel is VALU-bound:
// profiles/r1_09: 610 VALU instructions per pixel before, 7 of these per pixel)
#define SMOOTHSTEP_C(E0, E1, X) smoothstep_inv((E0), (float)(1.0 / ((double)(E1) - (double)(E0))), (X))
__device__ __forceinline__ float smoothstep_inv(float e0, float inv, float x) {
    float t = fminf(fmaxf((x - e0) * inv, 0.f), 1.f);
    return t * t * (3.f - 2.f * t);
}
__device__ __forceinline__ bool oob(float u, float v) { return u < 0.f || v < 0.f || u > 1.f || v > 1.f; }

__device__ __forceinline__ float g_w_phase1(float w1i, float sdi, float cdi) { return w1i * (1.0f + (sdi - cdi) * 10.0f); }   // :459
// phase 3 of push_pull_inpaint (:484-505): normalise + 3-tap vertical blur, or the pixel's own colour when nothing was found
template <class S>
__device__ __forceinline__ void push_pull_finish(const S& smp, const DibrGeom& g, float u, float v, float cdi, const float best[3], float bw, float out[3]) {
    if (bw > 0.01f) {                                                                 // phase 3 (:484-502)
        float va[3] = {best[0] / bw * 0.5f, best[1] / bw * 0.5f, best[2] / bw * 0.5f}, vw = 0.5f;
        if constexpr (S::serial_blur) {
            // UpDep: a depth tap is sixteen source loads, not two: the taps run one after the other in a loop that is not unrolled
            // (requested together they take the row kernels past their register budget into scratch).  The same values added in the
            // same order dy = -1, +1: the same bits.
#pragma clang loop unroll(disable)
            for (int t = 0; t < 2; ++t) {
                const float vv = v + (float)(2 * t - 1) * g.psy * g.blur;
                if (!(vv >= 0.f && vv <= 1.f)) continue;
                if (1.0f - smp.any_depth(u, vv) > cdi + g.tol * 0.5f) {
                    float vc[3];
                    smp.any_color(u, vv, vc);
                    va[0] += vc[0] * 0.25f; va[1] += vc[1] * 0.25f; va[2] += vc[2] * 0.25f;
                    vw += 0.25f;
                }
            }
            out[0] = va[0] / vw; out[1] = va[1] / vw; out[2] = va[2] / vw;
            return;
        }
        // the two vertical taps touch other texture rows: global gathers.  All six of their loads are requested before the first is
        // used (the depth test decides what is ADDED, not what is fetched): one round trip instead of up to four dependent ones at
        // the end of every in-painted pixel; the sums keep the order dy = -1, +1
        float vdi[2], vc[2][3];
        bool ok[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float vv = v + (float)(2 * t - 1) * g.psy * g.blur;
            ok[t] = vv >= 0.f && vv <= 1.f;
            const float vs = ok[t] ? vv : v;                                          // (a valid row for the unconditional loads)
            vdi[t] = 1.0f - smp.any_depth(u, vs);
            smp.any_color(u, vs, vc[t]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (ok[t] && vdi[t] > cdi + g.tol * 0.5f) {
                va[0] += vc[t][0] * 0.25f; va[1] += vc[t][1] * 0.25f; va[2] += vc[t][2] * 0.25f;
                vw += 0.25f;
            }
        out[0] = va[0] / vw; out[1] = va[1] / vw; out[2] = va[2] / vw;
        return;
    }
    smp.own_color(u, v, out);                                                         // :505
}

template <int OUT_FMT>
__device__ __forceinline__ void dibr_store(void* __restrict__ out_all, long o, int nch, const float c[4]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (OUT_FMT == D2S_FMT_U8_HWC) ((uint8_t*)out_all)[o + k] = (uint8_t)__builtin_amdgcn_cvt_pk_u8_f32(c[k], 0, 0);
        else ((float*)out_all)[o + k] = c[k];
    }
    if (nch == 4) {
        if (OUT_FMT == D2S_FMT_U8_HWC) ((uint8_t*)out_all)[o + 3] = (uint8_t)__builtin_amdgcn_cvt_pk_u8_f32(c[3] * 255.0f, 0, 0);
        else ((float*)out_all)[o + 3] = c[3];
    }
}

// ---- Host side: the launch plan of f1 (dibr.hip) and of the composites (dibr_composite.hip), DESIGN.md 3.4 ----

// H x W frame limits of every DIBR entry, the shape queries included (32-bit texel indices: tex_color's 8-byte window)
inline int dibr_check_frame(int H, int W) {
    D2S_REQUIRE(H > 1 && W > 1, "bad shape (H, W > 1)");
    D2S_REQUIRE((long)H * W * 3 + 8 < (1L << 31), "frame too large (32-bit texel indices)");
    return D2S_OK;
}
// What every launching entry refuses, whatever the program; the launchers add their own (pointers, display_mode / composite,
// viewport, crop).  No HIP call here or before it.
inline int dibr_check(const d2s_dibr_params* p, int dh, int dw, int batch, int H, int W, int out_fmt) {
    D2S_REQUIRE(p->struct_size == sizeof(d2s_dibr_params),
                "d2s_dibr_params.struct_size must be sizeof(d2s_dibr_params) = 80 (header of d2s_version() >= 110; the 72-byte struct of "
                "version 100 has no alpha_mode)");
    D2S_REQUIRE(batch > 0 && batch <= 65535, "bad batch (1 .. 65535)");
    const int rc = dibr_check_frame(H, W);
    if (rc) return rc;
    D2S_REQUIRE(dh > 0 && dw > 0 && (long)dh * dw < (1L << 31), "bad depth shape (dh, dw > 0)");
    D2S_REQUIRE(out_fmt == D2S_FMT_U8_HWC || out_fmt == D2S_FMT_F32_HWC, "bad out_fmt (U8_HWC or F32_HWC)");
    D2S_REQUIRE(p->search_radius >= 0.f && p->search_radius < 16.f, "search_radius must be in [0,16)");
    D2S_REQUIRE(p->corner_radius >= 0.f && p->corner_radius <= 0.5f, "corner_radius must be in [0, 0.5]");
    D2S_REQUIRE(p->alpha_mode >= D2S_DIBR_ALPHA_WINDOW && p->alpha_mode <= D2S_DIBR_ALPHA_RGBA, "bad alpha_mode");
    return D2S_OK;
}

// The uniforms every program shares, from checked parameters.  Left to the launcher: oh, ow, mode, out_h, out_w, vpx .. vph (and the
// crop): f1's eye shape and defaulted float viewport, the composites' integer window viewport.
inline void dibr_fill_geom(DibrGeom& g, const d2s_dibr_params* p, int H, int W, int dh, int dw) {
    g.H = H; g.W = W;
    g.dh = dh; g.dw = dw; g.dsy = linear_scale(dh, H, false); g.dsx = linear_scale(dw, W, false);      // (d2s_upsample_depth's scales)
    g.c = cosf(p->roll); g.s = sinf(p->roll);
    g.psx = 1.0f / (p->res_w > 0.f ? p->res_w : (float)W);
    g.psy = 1.0f / (p->res_h > 0.f ? p->res_h : (float)H);
    g.half_ipd = (float)(p->ipd_uv / 2.0);                                            // u_eye_offset (viewer.py:2638, 2701)
    g.strength = p->depth_strength; g.conv = p->convergence;
    g.tol = p->depth_tolerance; g.blur = p->blur_radius; g.feather_w = p->feather_width;
    g.search = (int)p->search_radius; g.feather = p->feather_enabled != 0;
    g.corner_r = p->corner_radius;
    g.alpha_mode = p->alpha_mode;
    for (int i = 0; i < 20; ++i) { g.w1[i] = i < 16 ? expf((float)(-i * 0.15)) : 0.f; g.w2[i] = i < 16 ? expf((float)(-i * 0.2)) : 0.f; }
}

// Per-eye viewport (oh, ow) and packed output of an eh x ew eye image: the Half modes halve the eye along the packing axis, and
// the packed size is twice the eye along it (d2s_dibr_shape, d2s_dibr_crop_shape, the f1 launcher).
inline int dibr_eye_shape(int eh, int ew, int display_mode, int* oh, int* ow, int* out_h, int* out_w) {
    D2S_REQUIRE(display_mode >= D2S_MODE_HALF_SBS && display_mode <= D2S_MODE_FULL_TAB, "bad display_mode");
    *oh = display_mode == D2S_MODE_HALF_TAB ? eh / 2 : eh;
    *ow = display_mode == D2S_MODE_HALF_SBS ? ew / 2 : ew;
    *out_h = display_mode == D2S_MODE_FULL_TAB || display_mode == D2S_MODE_HALF_TAB ? 2 * *oh : *oh;
    *out_w = display_mode == D2S_MODE_FULL_SBS || display_mode == D2S_MODE_HALF_SBS ? 2 * *ow : *ow;
    return D2S_OK;
}

// _movie_crop_pixel_bounds (xr_viewer/crop.py:165-173): Python's round() is half-to-even = nearbyint on doubles
inline void crop_pixel_bounds(int W, int H, const double crop[4], int b[4]) {
    auto clampi = [](long v, long lo, long hi) { return (int)std::max(lo, std::min(v, hi)); };
    b[0] = clampi((long)nearbyint(crop[0] * W), 0, std::max(0, W - 1));
    b[1] = clampi((long)nearbyint(crop[1] * H), 0, std::max(0, H - 1));
    b[2] = std::max(b[0] + 1, (int)std::min((long)nearbyint((crop[0] + crop[2]) * W), (long)W));
    b[3] = std::max(b[1] + 1, (int)std::min((long)nearbyint((crop[1] + crop[3]) * H), (long)H));
}
inline int crop_check(const double* crop) {
    D2S_REQUIRE(crop, "null pointer (crop)");
    for (int i = 0; i < 4; ++i) D2S_REQUIRE(std::isfinite(crop[i]), "crop must be finite");
    const double e = 1e-6;
    D2S_REQUIRE(crop[0] >= -e && crop[1] >= -e, "crop x, y must be >= 0");
    D2S_REQUIRE(crop[2] > 0.0 && crop[3] > 0.0, "crop w, h must be > 0");
    D2S_REQUIRE(crop[0] + crop[2] <= 1.0 + e && crop[1] + crop[3] <= 1.0 + e, "crop x + w, y + h must be <= 1");
    return D2S_OK;
}
// the per-eye viewport of a cropped warp: the crop's pixel size, halved by the Half modes as d2s_dibr_shape halves the frame
inline int crop_eye_shape(int H, int W, const double* crop, int display_mode, int* oh, int* ow, int* out_h, int* out_w) {
    D2S_REQUIRE(H > 1 && W > 1, "bad shape");
    int rc = crop_check(crop);
    if (rc) return rc;
    int b[4];
    crop_pixel_bounds(W, H, crop, b);
    rc = dibr_eye_shape(b[3] - b[1], b[2] - b[0], display_mode, oh, ow, out_h, out_w);
    if (rc) return rc;
    D2S_REQUIRE(*oh >= 2 && *ow >= 2, "crop: the eye viewport must be at least 2 x 2 pixels");
    return D2S_OK;
}

// The LDS window of the row kernels (roll == 0).  margin: how far from its own texel a pixel's same-row taps can land -- the sweeps
// (search texels of pixel_size.x), the +-2 pixel_size confidence taps, the parallax shift (|shaped| <= 1 and |depth_inv + conv| <=
// 1 + |conv| for depth in 0..1) -- in texels of the source; taps beyond it take the row gather, the same values.
// tex_per_col: source texels per output column (W / ow, of the cropped span with a crop).  A block of `cols` columns stages
// win_words(cols) texels of 8 float planes.  cols starts at col_cap and halves down to 256 while the window exceeds widen_words or
// half the block would lie past the viewport; the row kernel is taken when rows_ok (roll == 0 and the launcher's own switches)
// and the 256-column window fits rows_words, else the gather kernel.
// A block's LDS: 8 float planes of WW words (dynamic) and the row kernel's static second-pass queue, int[2 * COLS] and its counter
// (dibr_rows_kernel asserts that its arrays have this size).  A block's request may not exceed 64 KB, and the row kernel is taken on
// the 256-column window: f1's rows_words is the largest WW with planes * 4 * WW + static(256) <= 65 536, which is 1 983.
constexpr int DIBR_WIN_PLANES = 8;
constexpr unsigned DIBR_LDS_LIMIT = 64u * 1024u;
constexpr unsigned dibr_rows_static_lds(int cols) { return (unsigned)(sizeof(int[2]) * (size_t)cols + sizeof(int)); }
constexpr unsigned dibr_rows_dynamic_lds(int WW) { return (unsigned)(DIBR_WIN_PLANES * sizeof(float)) * (unsigned)WW; }
constexpr int DIBR_F1_ROWS_WORDS = (int)((DIBR_LDS_LIMIT - dibr_rows_static_lds(256)) / (DIBR_WIN_PLANES * sizeof(float)));
static_assert(dibr_rows_dynamic_lds(DIBR_F1_ROWS_WORDS) + dibr_rows_static_lds(256) <= DIBR_LDS_LIMIT &&
              dibr_rows_dynamic_lds(DIBR_F1_ROWS_WORDS + 1) + dibr_rows_static_lds(256) > DIBR_LDS_LIMIT, "f1's rows_words is the LDS bound");
struct DibrWindow { int margin, cols, WW; bool rows; };
inline DibrWindow dibr_plan_window(const DibrGeom& g, double tex_per_col, bool rows_ok, int col_cap, int widen_words, int rows_words) {
    const double tex_per_px = (double)g.W * (double)g.psx;
    const double reach = fmax(fmax(2.0, (double)g.search) * tex_per_px,
                              fabs((double)g.half_ipd) * (1.0 + fabs((double)g.conv)) * fabs((double)g.strength) * (double)g.W);
    DibrWindow w;
    w.margin = (int)ceil(reach) + 2;
    auto win_words = [&](int c) { return (int)ceil((double)(c - 1) * tex_per_col) + 2 * w.margin + 4; };
    w.rows = rows_ok && win_words(256) <= rows_words;
    w.cols = col_cap;
    while (w.cols > 256 && (win_words(w.cols) > widen_words || g.ow <= w.cols / 2)) w.cols >>= 1;
    w.WW = win_words(w.cols);
    return w;
}

}  // namespace d2s
