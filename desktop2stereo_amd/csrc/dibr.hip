// f1: the reference's GLSL DIBR fragment shader with disocclusion in-painting (viewer.py:386-631; the warp its default
// Viewer / OpenXR modes show) as a HIP kernel: 3-tap depth smoothing along the parallax direction, non-linear depth
// shaping, 5 % edge fall-off, soft disocclusion confidence, 12-tap directional push-pull + opposite sweep + 3-tap
// vertical blur, sub-pixel border alpha, optional edge feathering.  One thread = one output pixel of one eye.
//
// texture() is exact float32 GL_LINEAR filtering with texel centres at (i+0.5)/N and GL_REPEAT wrapping (moderngl's
// defaults; the reference sets neither, viewer.py:2385-2386).  u_resolution is never assigned in the reference
// (viewer.py:395, 413: pixel_size = 1/0), so the resolution is a parameter here (0 -> source size).  Colours are kept
// in 0..255; frag_color.a follows d2s_dibr_params.alpha_mode (the reference draws these quads with blending off: WINDOW = rgb as written).
// Line numbers in the comments below are viewer.py.
#include "dibr_tex.h"
#include "dibr_xr.h"
#include <algorithm>
#include <cmath>

namespace d2s {

// push_pull_inpaint (:437-506)
template <class S>
__device__ void push_pull(const S& smp, const DibrGeom& g,
                          float u, float v, float cdi, float parx, float pary, float sweep_sign, float out[3]) {
    // (roll == 0: sy == 0, every sweep tap lies on the pixel's own row pair -- the samplers' own_* taps)
    auto depth_at = [&](float su, float sv) { return smp.own_depth(su, sv); };
    auto color_at = [&](float su, float sv, float* o) { smp.own_color(su, sv, o); };
    float best[3] = {0.f, 0.f, 0.f}, bw = 0.f, col[3];
    const float sx = parx * g.psx * sweep_sign, sy = pary * g.psx * sweep_sign;      // both use pixel_size.x (:442)
    // (Requesting the sweep's depth taps four at a time before testing them -- same values, same order of the sums -- was built and
    //  measured: no faster in the row kernel, 5-9 % slower in the gather kernels, and 30 more VGPRs took the row kernel from 7 to 4
    //  waves per SIMD.  The loops stay as the shader writes them.)
    for (int i = 1; i <= g.search; ++i) {                                             // phase 1 (:445-466)
        float su = u + sx * (float)i, sv = v + sy * (float)i;
        if (oob(su, sv)) continue;
        float sdi = 1.0f - depth_at(su, sv);
        if (sdi > cdi + g.tol) {
            color_at(su, sv, col);
            float w = g_w_phase1(g.w1[i], sdi, cdi);
            best[0] += col[0] * w; best[1] += col[1] * w; best[2] += col[2] * w;
            bw += w;
            if (bw > 5.0f) break;
        }
    }
    if (bw < 2.0f) {                                                                  // phase 2 (:469-481)
        for (int i = 1; i <= g.search; ++i) {
            float su = u - sx * (float)i, sv = v - sy * (float)i;
            if (oob(su, sv)) continue;
            float sdi = 1.0f - depth_at(su, sv);
            if (sdi > cdi + g.tol) {
                color_at(su, sv, col);
                float w = g.w2[i];
                best[0] += col[0] * w; best[1] += col[1] * w; best[2] += col[2] * w;
                bw += w;
            }
        }
    }
    push_pull_finish(smp, g, u, v, cdi, best, bw, out);
}

// roll == 0: the five depth taps of a pixel that do not depend on its shift -- the centre, the smoothing pair at -+1.5 pixel_size
// and the confidence pair at -+2 pixel_size along the parallax direction -- are the SAME texture positions for the two eyes:
// sg(right) = -sg(left), and a negation is exact through (c * sg) * pixel_size * k, so u - dsx(right) is bit for bit u + dsx(left).
// They are evaluated once per output column with the left eye's offsets and handed to both eyes (dm / dp change places for the right
// eye, |a - b| == |b - a|): 5 taps instead of 10 per column of the row kernel, the same bits.
struct PixTaps { float d0, dA, dB, jA, jB; };      // depth at u, u - dsx(left), u + dsx(left), u - s2x(left), u + s2x(left)
template <class S, class G>
__device__ __forceinline__ PixTaps pix_taps(const S& smp, const G& g, int x, int y) {
    const float eye_offset = -g.half_ipd;
    const float sg = eye_offset > 0.f ? 1.f : (eye_offset < 0.f ? -1.f : 0.f);
    const float parx = g.c * sg;
    const float u = tex_u(g, ((float)x + 0.5f) / (float)g.ow), v = tex_v(g, ((float)y + 0.5f) / (float)g.oh);
    const float dsx = parx * g.psx * 1.5f, s2x = parx * g.psx * 2.0f;
    // (One window test for the five taps instead of a branch pair per tap: measured, no faster, 12 bytes of scratch.)
    PixTaps t;
    t.d0 = smp.own_depth(u, v);
    t.dA = smp.own_depth(u - dsx, v);
    t.dB = smp.own_depth(u + dsx, v);
    t.jA = smp.own_depth(u - s2x, v);
    t.jB = smp.own_depth(u + s2x, v);
    return t;
}

// one output pixel of one eye: FRAGMENT_SHADER.main (:533-631) -> colour * alpha
// DEFER: return true WITHOUT a result when the pixel needs the in-painting (the caller queues it for a second, lane-compacted pass
// that calls this function again with DEFER = false: the same expressions on the same inputs -> the same bits).
// sh: the column's five shift-independent depth taps (roll == 0 only, pix_taps) or nullptr = take them here.
// FX = false: u_feather_enabled == 0 and u_corner_radius == 0 (the desktop viewer's state) as a compile-time fact.  As run-time branches
// the two blocks depend on the column and row only, so the compiler hoists them out of the eye loop and -- free of side effects --
// speculates them: every pixel paid for four IEEE divisions, a powf and a sqrtf it did not use (~250 of ~900 instructions of pass 1).
// G = DibrGeomCrop (the OpenXR screen shader, implementation.py:111-126): every texture coordinate -- the depth taps, the edge
// fall-off, the shift, the in-painting, the border alpha -- follows the CROPPED uv (u, v); the rounded-corner SDF stays on the quad's
// own uv (us, vs) and the feathering on the pixel index and u_viewport.
// G = DibrGeomProj (d2s_dibr_xr_eyes): quv = the screen's own uv (u, 1 - v of the interpolated vertex uv) of this pixel; x, y are not used.
// RAW: frag_color as the shader writes it whatever alpha_mode says (the glow passes blend over it first).
template <bool DEFER = false, bool SHARED = false, bool FX = true, bool RAW = false, class S, class G>
__device__ __forceinline__ bool dibr_pixel(const S& smp, const G& g, int x, int y, int eye, float outc[4], const PixTaps* sh = nullptr,
                                           const float* quv = nullptr) {
    const float eye_offset = eye ? g.half_ipd : -g.half_ipd;                          // :2701, 2714
    const float sg = eye_offset > 0.f ? 1.f : (eye_offset < 0.f ? -1.f : 0.f);
    const float parx = g.c * sg, pary = g.s * sg;                                     // :540
    const float sweep_sign = eye_offset > 0.f ? -1.f : 1.f;                           // :541
    float us, vs;
    if constexpr (G::proj) { us = quv[0]; vs = quv[1]; }
    else { us = ((float)x + 0.5f) / (float)g.ow; vs = ((float)y + 0.5f) / (float)g.oh; }
    const float u = tex_u(g, us), v = tex_v(g, vs);
    auto depth_at = [&](float su, float sv) { return smp.own_depth(su, sv); };       // (roll == 0: v - 0 * k == v, every tap below shares the row pair)
    // 3-tap depth smoothing along the parallax direction (:545-549)
    const float dsx = parx * g.psx * 1.5f, dsy = pary * g.psy * 1.5f;
    float d0, dm, dp;
    if constexpr (SHARED) { d0 = sh->d0; dm = eye ? sh->dB : sh->dA; dp = eye ? sh->dA : sh->dB; }
    else { d0 = depth_at(u, v); dm = depth_at(u - dsx, v - dsy); dp = depth_at(u + dsx, v + dsy); }
    float d = d0 * 0.7f + dm * 0.15f + dp * 0.15f;
#if defined(DIBR_CUT) && DIBR_CUT == 1      // (tuning aid, timing only: stop after the three smoothing taps)
    outc[0] = outc[1] = outc[2] = d; outc[3] = 1.f; return false;
#endif
    float dinv = -d;
    float shaped = dinv * (1.0f + 0.35f * (1.0f - d));                                // :554
    float shift = shaped + g.conv;
    float fall = 1.f;                                                                 // :560-562 (exactly 1 away from the edges)
    if (u < 0.05f || u > 0.95f) fall = SMOOTHSTEP_C(0.f, 0.05f, u) * SMOOTHSTEP_C(1.f, 0.95f, u);
    float px = eye_offset * shift * g.strength * fall;                                // :563
    float su = u - px * g.c, sv = v - px * g.s;                                       // :564
    float conf;                                                                        // :419-435
#if defined(DIBR_CUT) && DIBR_CUT == 5      // (timing only: no in-painting for pixels whose source lies outside the frame)
    if (su < 0.f || su > 1.f || sv < 0.f || sv > 1.f) conf = 0.f;
#else
    if (su < 0.f || su > 1.f || sv < 0.f || sv > 1.f) conf = 1.f;
#endif
    else {
        const float s2x = parx * g.psx * 2.0f, s2y = pary * g.psy * 2.0f;
        float jump;
        if constexpr (SHARED) jump = eye ? fabsf(sh->jB - sh->jA) : fabsf(sh->jA - sh->jB);
        else jump = fabsf(depth_at(u - s2x, v - s2y) - depth_at(u + s2x, v + s2y));
        conf = SMOOTHSTEP_C(0.04f, 0.10f, jump);
    }
#if defined(DIBR_CUT) && DIBR_CUT == 2      // (timing only: stop after the confidence taps)
    outc[0] = outc[1] = outc[2] = conf + su; outc[3] = 1.f; return false;
#endif
    if (DEFER && conf > 0.001f) return true;
    float col[3];
    smp.own_color(su, sv, col);                                                       // :570
#if defined(DIBR_CUT) && DIBR_CUT == 3      // (timing only: no in-painting)
    outc[0] = col[0] + conf; outc[1] = col[1]; outc[2] = col[2]; outc[3] = 1.f; return false;
#endif
#if defined(DIBR_CUT) && DIBR_CUT == 4      // (timing only: everything but the in-painting call)
    if (conf > 1e30f) {
#else
    if (conf > 0.001f) {
#endif
        float fill[3];
        push_pull(smp, g, u, v, dinv, parx, pary, sweep_sign, fill);
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = col[k] * (1.0f - conf) + fill[k] * conf; // mix (:575)
    }
    float alpha = 1.f;                                                                // :582 (exactly 1 inside the frame)
    if (su < 0.001f || su > 0.999f || sv < 0.001f || sv > 0.999f) {
        float bx = SMOOTHSTEP_C(-0.001f, 0.001f, su) * SMOOTHSTEP_C(1.001f, 0.999f, su);
        float by = SMOOTHSTEP_C(-0.001f, 0.001f, sv) * SMOOTHSTEP_C(1.001f, 0.999f, sv);
        alpha = fminf(bx, by);
    }
    // (G = DibrGeomCrop: the two blocks below depend on the column and the row alone, so the compiler forms them ahead of the eye loop
    //  and keeps their results across the whole pixel -- 12 of the 24 bytes of scratch the FullDep row kernels with FX would have.  fx / fy are x / y made available only once the colour exists (ordered_after: no arithmetic, the same bits).)
    int fx = x, fy = y;
    if constexpr (FX && G::crop && !G::proj) { fx = ordered_after(x, col[0]); fy = ordered_after(y, col[1]); }
    if (FX && !G::proj && g.feather) {                                                 // :587-616 (never with a projected screen: refused)
        // (gl_FragCoord.xy - u_viewport.xy) / u_viewport.zw; gl_FragCoord is y-up, pixel centres at +0.5
        float fu = (((float)fx + 0.5f) - g.vpx) / g.vpw, fv = (((float)g.oh - ((float)fy + 0.5f)) - g.vpy) / g.vph, fw = g.feather_w;
        float fo = smoothstepf(0.f, fw, fu) * smoothstepf(0.f, fw, 1.0f - fu) * smoothstepf(0.f, fw, fv) * smoothstepf(0.f, fw, 1.0f - fv);
        float sh = powf(fo, 0.7f);
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] *= sh;
    }
    if (FX && g.corner_r > 0.f) {
        // rounded-box SDF over the quad's own uv (the shader's inner `uv` of the feather block shadows only that block), :617-624
        // (with a crop the quad's own uv is formed here: the same expressions dibr_pixel starts with)
        float qu = u, qv = v;
        if constexpr (G::proj) { qu = us; qv = vs; }
        else if constexpr (G::crop) { qu = ((float)fx + 0.5f) / (float)g.ow; qv = ((float)fy + 0.5f) / (float)g.oh; }
        const float dx = fabsf(qu - 0.5f) - 0.5f + g.corner_r, dy = fabsf(qv - 0.5f) - 0.5f + g.corner_r;
        const float mx = fmaxf(dx, 0.f), my = fmaxf(dy, 0.f);
        const float sdf = sqrtf(mx * mx + my * my) + fminf(fmaxf(dx, dy), 0.f) - g.corner_r;
        alpha = fminf(alpha, 1.0f - smoothstepf(0.f, 0.01f, sdf));
    }
    // frag_color = (col, alpha).  The reference's quads are drawn with blending off: its window shows col as written (WINDOW);
    // PREMULTIPLIED = col * alpha (composited over black); RGBA hands out both (d2s.h)
#pragma unroll
    for (int k = 0; k < 3; ++k) outc[k] = !RAW && g.alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED ? col[k] * alpha : col[k];
    outc[3] = alpha;
    return false;
}

// General kernel: one thread = one output pixel of one eye, every tap a global gather.  (4 pixels per thread with packed dword
// stores measured SLOWER -- 113 -> 120 us Full-SBS, 38 -> 97 us Half-SBS at 1080p: this kernel lives on the locality of neighbouring
// threads' gathers, not on its stores.)  ROLL0: the row pair of a pixel formed once (104.5 -> 89.5 us Full-SBS 1080p, same bits).
template <int OUT_FMT, bool ROLL0, class D = FullDep, class G = DibrGeom>
__global__ void __launch_bounds__(256)
dibr_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all, G g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y % g.oh, eye = blockIdx.y / g.oh, b = blockIdx.z;
    if (x >= g.ow) return;
    const uint8_t* rgb = rgb_all + (long)b * g.H * g.W * 3;
    const D dep = D::make(dep_all, b, g);
    const bool sbs = g.mode == D2S_MODE_HALF_SBS || g.mode == D2S_MODE_FULL_SBS;
    const int ox = sbs ? eye * g.ow + x : x, oy = sbs ? y : eye * g.oh + y;
    const int nch = g.alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    const long o = (((long)b * g.out_h + oy) * g.out_w + ox) * nch;
    float c[4];
    if constexpr (ROLL0) {
        RowSmp<D> smp;
        smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
        smp.rc = row_ctx(dep, g.H, g.W, tex_v(g, ((float)y + 0.5f) / (float)g.oh));     // (the v dibr_pixel forms)
        dibr_pixel(smp, g, x, y, eye, c);
    } else {
        GenSmp<D> smp;
        smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
        dibr_pixel(smp, g, x, y, eye, c);
    }
    dibr_store<OUT_FMT>(out_all, o, nch, c);
}

// roll == 0, the common case (the desktop viewer never rolls): a block = 256 output columns of ONE output row, both eyes.  Every tap
// of those 512 pixels except the in-painting's two vertical-blur taps reads the same two texture rows, within `margin` texels of the
// block's own span: the block stages that window once -- depth rows as they are, colour rows converted to float planes (the same
// conversion a tap makes) -- and the taps become LDS reads at a window index (WinSmp).  Same expressions on the same values as the
// gather kernel: bit-identical (tests/test_gpu_dibr.py).  The gather kernel spent ~600 VALU instructions per pixel, most of them
// address arithmetic of its ~14 eight-byte gathers (64-bit row bases, GL_REPEAT wraps, byte unpacking).
#ifndef DIBR_WAVES
#define DIBR_WAVES 7                  // (<= 72 VGPRs: 5 -> 7 waves per SIMD, 73.8 -> 69.0 us in round 5; 8: no faster.  FX = false: 71 VGPRs, no scratch)
#endif
// COLS (round 6): output columns per block, 256 per thread-pass.  The second pass costs one mostly-empty wave per block that has
// queued pixels whatever their number; a block twice as wide halves those waves (and stages a window 2 x as wide once).
// D = UpDep: the staging loop evaluates the two depth texels of a window entry from the model-resolution map (four source values
// each, L2-resident) instead of loading them; everything after the barrier runs on the staged values as it does for FullDep.
// G = DibrGeomCrop: the block's texture row and the window's first texel follow the cropped coordinate; the reach (margin) is in
// source texels and does not change; a window that starts left of the texture or runs past its right edge wraps as before (wrapi).
template <int OUT_FMT, bool FX, int COLS, class D = FullDep, class G = DibrGeom>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DIBR_WAVES)))
dibr_rows_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all, G g, int margin, int WW) {
    extern __shared__ float dibr_win[];                // [2][WW] the row pair of the depth texture | [6][WW] R0 G0 B0 R1 G1 B1 as floats
    __shared__ int queue[2 * COLS], qn;                // (column - xb) * 2 + eye of the pixels that need the in-painting
    static_assert(sizeof(queue) + sizeof(qn) == dibr_rows_static_lds(COLS), "the launch plan's LDS bound counts these arrays (dibr_tex.h)");
    const int tid = threadIdx.x, xb = blockIdx.x * COLS;
    const int y = blockIdx.y, b = blockIdx.z;
    const uint8_t* rgb = rgb_all + (long)b * g.H * g.W * 3;
    const D dep = D::make(dep_all, b, g);
    if (tid == 0) qn = 0;
    WinSmp<D, FX && G::crop> smp;
    smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
    smp.rc = row_ctx(dep, g.H, g.W, tex_v(g, ((float)y + 0.5f) / (float)g.oh));         // block-uniform (the v dibr_pixel forms)
    smp.dwin = dibr_win; smp.cwin = dibr_win + 2 * WW; smp.WW = WW;
    smp.wx0 = (int)floorf(tex_u(g, ((float)xb + 0.5f) / (float)g.ow) * (float)g.W - 0.5f) - margin;
    // (Four texels per thread -- 16-byte depth loads, 12-byte colour loads, vector LDS writes, a sixth of the load instructions -- was
    //  built and measured: 54.2 us against 51.6 at 1080p Full-SBS; a quarter of the threads then carry the whole round trip.)
#if defined(DIBR_CUT) && (DIBR_CUT == 8 || DIBR_CUT == 10)      // (timing only: no staging, no second pass)
    for (int j = tid; j < 0; j += 256) {
#else
    for (int j = tid; j < WW; j += 256) {
#endif
        const int xs = wrapi(smp.wx0 + j, g.W);        // (one conditional add / subtract unless the window is wider than the texture: then the modulo)
        float da, db;
        dep.pair(smp.rc.d, xs, da, db);
        dibr_win[j] = da;
        dibr_win[WW + j] = db;
        const uint8_t* p0 = rgb + smp.rc.c0 + xs * 3;
        const uint8_t* p1 = rgb + smp.rc.c1 + xs * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) { dibr_win[(2 + k) * WW + j] = (float)p0[k]; dibr_win[(5 + k) * WW + j] = (float)p1[k]; }
    }
    __syncthreads();
    const bool sbs = g.mode == D2S_MODE_HALF_SBS || g.mode == D2S_MODE_FULL_SBS;
    const int nch = g.alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    auto out_index = [&](int px, int eye) {
        const int ox = sbs ? eye * g.ow + px : px, oy = sbs ? y : eye * g.oh + y;
        return (((long)b * g.out_h + oy) * g.out_w + ox) * nch;
    };
#if defined(DIBR_CUT)
    const int x = xb + tid;
#endif
#if defined(DIBR_CUT) && DIBR_CUT == 9      // (timing only: the staging and one dword store per thread)
    if (x < g.ow) ((float*)out_all)[((long)b * g.out_h + y) * g.out_w * nch / 4 + x] = dibr_win[tid] + dibr_win[WW + tid] + dibr_win[2 * WW + tid];
    if (qn >= 0) return;
#endif
#if defined(DIBR_CUT) && (DIBR_CUT == 7 || DIBR_CUT == 10)      // (timing only: the staging and the stores / 10: the stores)
    if (x < g.ow) {
        for (int eye = 0; eye < 2; ++eye) {
            const float c[4] = {dibr_win[tid + eye], dibr_win[WW + tid], dibr_win[2 * WW + tid], 1.f};
            dibr_store<OUT_FMT>(out_all, out_index(x, eye), nch, c);
        }
    }
    if (qn >= 0) return;
#endif
    // pass 1: every pixel up to the in-painting decision.  Disocclusions are thin (0.3-0.5 % of the pixels of a 1080p scene, but a
    // vertical depth edge crosses every row: 5-8 % of the waves): run in place, a wave with three such lanes walks the whole 24-tap
    // sweep at 5 % lane occupancy.  Those pixels are queued instead ...
    for (int cx = tid; cx < COLS; cx += 256) {
        const int x = xb + cx;
        if (x >= g.ow) break;
        const PixTaps taps = pix_taps(smp, g, x, y);
#pragma unroll
        for (int eye = 0; eye < 2; ++eye) {
            float c[4];
            if (dibr_pixel<true, true, FX>(smp, g, x, y, eye, c, &taps)) queue[atomicAdd(&qn, 1)] = cx * 2 + eye;
            else dibr_store<OUT_FMT>(out_all, out_index(x, eye), nch, c);
        }
    }
    __syncthreads();
#if defined(DIBR_CUT) && (DIBR_CUT == 6 || DIBR_CUT == 8)      // (timing only: no second pass)
    if (qn >= 0) return;
#endif
    // ... and pass 2 gives each queued pixel a lane of its own: the whole pixel function again, in-painting included (same inputs,
    // same expressions: the same bits as the single-pass kernel; the order of the queue does not matter, every entry is independent).
    // Measured at 1080p Full-SBS (tools/dibr_bench.py): in place 85.6 us, queued 73.7; everything but this pass 45 us -- what is left
    // is one mostly-empty wave per block walking ~2 500 instructions.  Round 6 (profiles/r6_06): 50.5 us, 25 of them this pass; a
    // launch-wide queue finished by a second kernel (one lane or sixteen lanes per pixel) was built and lost (31-47 us for that kernel).  Tried on top of it and not kept: queues shared by 2-8 rows with
    // the rows' windows kept in LDS or pass-2 taps by gather (fewer second-pass waves, but 99 VGPRs / 25 KB of LDS per block halve
    // the resident waves: 69-101 us at one frame, 45-98 us Half-SBS), sweep taps requested four at a time (no faster, +30 VGPRs).
    for (int q = tid; q < qn; q += 256) {
        const int e = queue[q], px = xb + (e >> 1), eye = e & 1;
        float c[4];
        dibr_pixel<false, false, FX>(smp, g, px, y, eye, c);
        dibr_store<OUT_FMT>(out_all, out_index(px, eye), nch, c);
    }
}

// d2s_dibr_xr_eyes: the OpenXR screen drawn into each eye's swapchain image (xr_viewer/effects.py:1023-1137).  One thread = one pixel
// of one eye image; a wave = a 16 x 4 pixel tile (block = 16 x 16), so that along the screen's outline covered and uncovered pixels
// share few waves and the taps of a wave stay within a few texture rows whatever the minification.  Every facet of the eye's table
// (dibr_xr.h; block-uniform addresses) is tested: ~14 float operations each, at most 48.  Covered: the facet's homography gives the
// interpolated vertex uv, and the pixel function runs on (u, 1 - v) as the shader's screen_flipped_uv; uncovered: the clear colour.
// (set-up: up to 24 facets of one eye's table travel in the arguments and are copied to the workspace, one float per thread)
__global__ void __launch_bounds__(256) dibr_xr_table_kernel(XrFacetChunk c, float* __restrict__ dst, int n_floats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_floats) dst[i] = ((const float*)&c)[i];
}
// ---- the glow passes (_GLOW_FRAG, xr_viewer/glsl.py:580-666), GLOW = true only.  lds: levels G.m .. G.q of the frame's mip chain as float
// RGB, one after another (level l is max(1, W >> l) x max(1, H >> l): floor-halving composes).
// one GL_LINEAR tap of level l, CLAMP_TO_EDGE (xr_viewer/frame.py:39-40); u, v in 0..1
__device__ __forceinline__ void glow_level(const float* __restrict__ lds, const XrGlowDev& G, int H, int W, int l, float u, float v, float o[3]) {
    int off = 0;
    for (int j = G.m; j < l; ++j) off += max(1, W >> j) * max(1, H >> j);
    const int w = max(1, W >> l), h = max(1, H >> l);
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f, x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = min(max((int)x0f, 0), w - 1), x1 = min(max((int)x0f + 1, 0), w - 1);
    const int y0 = min(max((int)y0f, 0), h - 1), y1 = min(max((int)y0f + 1, 0), h - 1);
    const float* a = lds + (off + y0 * w + x0) * 3;
    const float* b = lds + (off + y0 * w + x1) * 3;
    const float* c = lds + (off + y1 * w + x0) * 3;
    const float* d = lds + (off + y1 * w + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = lerp2(a[k], b[k], c[k], d[k], fx, fy);
}
// textureLod(u_source, source_uv(s), lod): LOD clamped to the chain (lod >= 7 >= G.m), trilinear
__device__ __forceinline__ void glow_texture_lod(const float* __restrict__ lds, const XrGlowDev& G, const DibrGeomProj& g, float su, float sv,
                                                 float lod, float o[3]) {
    const float u = fminf(fmaxf(g.cx + fminf(fmaxf(su, 0.f), 1.f) * g.cw, 0.f), 1.f);      // source_uv (:597-600)
    const float v = fminf(fmaxf(g.cy + fminf(fmaxf(sv, 0.f), 1.f) * g.ch, 0.f), 1.f);
    const float lam = fminf(fmaxf(lod, (float)G.m), (float)G.q), l0f = floorf(lam), f = lam - l0f;
    const int l0 = (int)l0f, l1 = min(l0 + 1, G.q);
    float a[3], b[3];
    glow_level(lds, G, g.H, g.W, l0, u, v, a);
    glow_level(lds, G, g.H, g.W, l1, u, v, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = a[k] * (1.0f - f) + b[k] * f;
}
// the Chebyshev signed distance (:621-623) at the screen's plane coordinates (a, b)
__device__ __forceinline__ float glow_sd(const XrGlowDev& G, float a, float b, float& cx, float& cy) {
    cx = (a - 0.5f) * G.inner_w; cy = (b - 0.5f) * G.inner_h;                                // uv - 0.5
    return fmaxf(fabsf(cx) - G.half_x, fabsf(cy) - G.half_y);
}
// main() of one pass: false = discarded, else src = (colour * glow in 0..255, glow).  A non-finite (a, b) -- far from the screen
// a / nw grows without bound -- ends in a comparison that fails: no glow.
__device__ __forceinline__ bool glow_frag(const float* __restrict__ lds, const XrGlowDev& G, const DibrGeomProj& g, float a, float b,
                                          bool inner_only, float src[4]) {
    float cx, cy;
    const float sd = glow_sd(G, a, b, cx, cy);
    const float inv_range = fmaxf(G.inv_range, 0.001f), inner = fmaxf(G.inner, 0.f);
    if (inner_only) { if (inner <= 0.f || sd > 0.f || sd < -inner) return false; }
    else if (!(sd > 0.f)) return false;
    const float edge_t = fminf(fmaxf((inner_only ? sd + inner : sd) * inv_range, 0.f), 1.f);
    float glow = powf(fmaxf(1.0f - smoothstepf(0.f, 1.f, edge_t), 0.f), 0.58f);
    if (inner_only) {
        float dens = smoothstepf(0.f, fmaxf(inner, 1e-6f), sd + inner);
        dens = dens * dens * (3.0f - 2.0f * dens);
        glow *= dens;
    }
    if (!(glow > 0.001f)) return false;
    // the screen's own uv again, from the glow's (:654-656), v flipped to the frame's top-left origin
    const float rx = ((cx + 0.5f) - (0.5f - G.half_x)) / fmaxf(G.half_x * 2.0f, 1e-5f);
    const float ry = 1.0f - ((cy + 0.5f) - (0.5f - G.half_y)) / fmaxf(G.half_y * 2.0f, 1e-5f);
    // extended_screen_color (:608-617)
    float dx = rx - 0.5f + 1e-5f, dy = ry - 0.5f;
    const float len = sqrtf(dx * dx + dy * dy);
    dx /= len; dy /= len;
    const float es = fminf(0.5f / fmaxf(fabsf(dx), 1e-5f), 0.5f / fmaxf(fabsf(dy), 1e-5f));      // edge_point_for_dir (:602-606)
    const float ex = fminf(fmaxf(0.5f + dx * es, 0.f), 1.f), ey = fminf(fmaxf(0.5f + dy * es, 0.f), 1.f);
    const float blur_t = inner_only ? 0.f : smoothstepf(0.f, 1.f, edge_t);
    const float back = 0.015f * (1.0f - blur_t) + 0.060f * blur_t, lod = 7.0f * (1.0f - blur_t) + 9.0f * blur_t;
    float local[3], edge[3];
    glow_texture_lod(lds, G, g, ex - dx * back, ey - dy * back, lod, local);
    if (inner_only) { edge[0] = local[0]; edge[1] = local[1]; edge[2] = local[2]; }      // (mixed in with weight 0: one textureLod)
    else glow_texture_lod(lds, G, g, ex, ey, lod + 1.0f, edge);
    const float mt = blur_t * 0.5f;
#pragma unroll
    for (int k = 0; k < 3; ++k) src[k] = (local[k] * (1.0f - mt) + edge[k] * mt) * glow;      // (u_glow_alpha_cap = 1: min(glow, 1) = glow)
    src[3] = glow;
    return true;
}
__device__ __forceinline__ void glow_blend(float c[4], const float src[4]) {      // ONE, ONE_MINUS_SRC_ALPHA, rgb and alpha
    const float k = 1.0f - src[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = src[i] + c[i] * k;
}

// ---- the veil and frosted passes (_FROST_VEIL_FRAG, _FROST_GLOW_FRAG, xr_viewer/glsl.py:698-791) on the flat screen's four walls
// (dibr_xr.h).  Colours are 0..255 as everywhere in this file; no contraction (built with -ffp-contract=off).
// one GL_LINEAR tap of a uint8 RGB level [h][w][3] in global memory, CLAMP_TO_EDGE; u, v in 0..1 (every index is clamped to the level)
__device__ __forceinline__ void frost_level(const uint8_t* __restrict__ lev, int w, int h, float u, float v, float o[3]) {
    const float x = u * (float)w - 0.5f, y = v * (float)h - 0.5f, x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = min(max((int)x0f, 0), w - 1), x1 = min(max((int)x0f + 1, 0), w - 1);
    const int y0 = min(max((int)y0f, 0), h - 1), y1 = min(max((int)y0f + 1, 0), h - 1);
    const uint8_t* a = lev + ((long)y0 * w + x0) * 3;
    const uint8_t* b = lev + ((long)y0 * w + x1) * 3;
    const uint8_t* c = lev + ((long)y1 * w + x0) * 3;
    const uint8_t* d = lev + ((long)y1 * w + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = lerp2((float)a[k], (float)b[k], (float)c[k], (float)d[k], fx, fy);
}
// hash12 (:718-722) in the shader's operation order, every product and sum rounded on its own.  Its argument is an integer cell; the
// intermediate values stay below (2 * 104) * 104 = 2.2e4, where a float32 ulp is 2e-3: the result is a fixed function of the cell only
// when every implementation keeps this order, which the CPU float32 emulation (tests/xr_frost_ref.py) does.
__device__ __forceinline__ float frost_fract(float x) { return x - floorf(x); }
__device__ __forceinline__ float frost_hash12(float px, float py) {
    float x = frost_fract(px * 0.1031f), y = frost_fract(py * 0.1031f), z = x;
    const float d = (x * (y + 33.33f) + y * (z + 33.33f)) + z * (x + 33.33f);
    x += d; y += d; z += d;
    return frost_fract((x + y) * z);
}
// main() of either program at the mesh's interpolated (v_uv, v_local.z = t): false = discarded (a NaN alpha discards), else
// src = (colour * alpha in 0..255, alpha).  MODE 1 veil, 2 frosted.  lev0 / lev1: the two levels textureLod mixes (veil: the frame).
template <int MODE>
__device__ __forceinline__ bool frost_frag(const XrFrostDev& F, const DibrGeomProj& g, const uint8_t* __restrict__ lev0,
                                           const uint8_t* __restrict__ lev1, float su, float sv, float t, float src[4]) {
    const float u = fminf(fmaxf(g.cx + su * g.cw, 0.f), 1.f), v = fminf(fmaxf(g.cy + sv * g.ch, 0.f), 1.f);      // sample_uv
    const float depth = fminf(fmaxf(t, 0.f), 1.f);
    float beam = expf(-depth / fmaxf(F.softness, 0.001f));
    beam = fmaxf(beam, 0.f);
    const float inv_thick = 1.0f / fmaxf(F.thickness, 0.1f);
    beam = beam > 0.f ? __builtin_amdgcn_exp2f(inv_thick * __builtin_amdgcn_logf(beam)) : 0.f;      // pow (post.hip's pow01 form)
    const float edge_dist = fminf(fminf(su, 1.0f - su), fminf(sv, 1.0f - sv));
    const float e0 = fmaxf(F.inset, 0.0001f);
    const float edge = 1.0f - smoothstepf(e0, e0 * 4.0f, edge_dist);
    float c[3];
    if (MODE == 1) {
        float alpha = edge * beam * F.alpha * F.intensity;
        if (!(alpha > 0.002f)) return false;
        alpha = fminf(alpha, 1.0f);
        frost_level(lev0, F.w0, F.h0, u, v, c);                                                  // textureLod(.., 0.0)
#pragma unroll
        for (int k = 0; k < 3; ++k) src[k] = c[k] * alpha;
        src[3] = alpha;
        return true;
    }
    float c1[3];
    frost_level(lev0, F.w0, F.h0, u, v, c);                                                      // textureLod(.., max(u_lod, 0))
    frost_level(lev1, F.w1, F.h1, u, v, c1);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = c[k] * (1.0f - F.lf) + c1[k] * F.lf;
    const float n = frost_hash12(floorf((u + F.tx) * F.noise_scale), floorf((v + F.ty) * F.noise_scale));
    const float luma255 = (c[0] * 0.2126f + c[1] * 0.7152f) + c[2] * 0.0722f, luma = luma255 * (1.0f / 255.0f);
    const float bright = smoothstepf(F.threshold, 1.0f, luma);
    const float scatter = fmaxf(bright, luma * fminf(fmaxf(F.diffuse, 0.f), 2.0f) * 0.35f);
    float alpha = edge * beam * scatter * F.alpha * F.intensity * (0.82f + 0.30f * n);
    if (!(alpha > 0.002f)) return false;
    alpha = fminf(alpha, 1.0f);
    const float gain = 0.55f + F.blend * 0.35f;
#pragma unroll
    for (int k = 0; k < 3; ++k) src[k] = ((c[k] * (1.0f - 0.28f) + luma255 * 0.28f) * gain + c[k] * bright * 0.35f) * alpha;
    src[3] = alpha;
    return true;
}

// ---- what the four eye-view kernels share.  A table row is 24 floats (XrFacet's fields in order: ha 0, hb 3, hw 6, hz 9, he 12, the uv
// affine 15 .. 20), read through a const float* so that one function serves a global XrFacet and an LDS row of stride XR_LDS_ROW.
// The block prologue.  It NEVER returns a thread early: in the glow kernels a thread outside its eye image (the other eye is larger,
// or a side is no multiple of 16) must still reach every barrier.  dibr_xr_kernel, which has none, returns on !inside itself.
struct XrPix { int ei, b; XrEyeDev e; int x, y; bool inside; float xc, yc; };
// (tx, ty): the thread's 16 x 16 tile of the eye image; the block's own, except in the binned kernel, whose block walks several
__device__ __forceinline__ XrPix xr_pix_at(const XrEyes& ex, int tx, int ty) {
    XrPix p;
    p.ei = blockIdx.z % ex.n; p.b = blockIdx.z / ex.n;
    p.e = ex.e[p.ei];
    p.x = tx * 16 + (threadIdx.x & 15); p.y = ty * 16 + (threadIdx.x >> 4);
    p.inside = p.x < p.e.w && p.y < p.e.h;
    p.xc = ((float)p.x + 0.5f) - 0.5f * (float)p.e.w; p.yc = ((float)p.y + 0.5f) - 0.5f * (float)p.e.h;      // exact: multiples of 0.5 below 2^13
    return p;
}
__device__ __forceinline__ XrPix xr_pix(const XrEyes& ex) { return xr_pix_at(ex, blockIdx.x, blockIdx.y); }
struct XrPt { float na, nb, nw, z; };
__device__ __forceinline__ XrPt xr_row_at(const float* __restrict__ r, float xc, float yc) {
    XrPt p;
    p.na = r[0] * xc + r[1] * yc + r[2]; p.nb = r[3] * xc + r[4] * yc + r[5];
    p.nw = r[6] * xc + r[7] * yc + r[8]; p.z = r[9] * xc + r[10] * yc + r[11];
    return p;
}
// The cover rule, the one copy: both sides of a seam evaluate its edge function here, with these operations (no contraction in this
// file), which is what makes the strip watertight.  false: the pixel lies outside facet f's two a-edges (p.z is then not formed).
struct XrHit { int best; float bz, ba, bb, bw; };      // bz starts at 1, the cleared depth buffer: LESS fails at and beyond the far plane
__device__ __forceinline__ bool xr_cover(const float* __restrict__ r, int f, float xc, float yc, XrHit& h, XrPt& p) {
    p.na = r[0] * xc + r[1] * yc + r[2]; p.nb = r[3] * xc + r[4] * yc + r[5];
    p.nw = r[6] * xc + r[7] * yc + r[8];
    const float ne = r[12] * xc + r[13] * yc + r[14];      // the upper a-edge: the next facet's na, negated (dibr_xr.h)
    if (!(p.na >= 0.f && ne >= 0.f)) return false;
    p.z = r[9] * xc + r[10] * yc + r[11];
    // (GL clips at the near plane, NDC z = -1)  GL_LESS: a tie keeps the lower facet index
    if (p.nb >= 0.f && p.nb <= p.nw && p.nw > 0.f && p.z >= -1.0f && p.z < h.bz) { h.bz = p.z; h.best = f; h.ba = p.na; h.bb = p.nb; h.bw = p.nw; }
    return true;
}
// the covering facet's interpolated vertex uv = the pixel's point in the screen's coordinates
__device__ __forceinline__ void xr_hit_uv(const float* __restrict__ r, const XrHit& h, float& sa, float& sb) {
    const float a = h.ba / h.bw, bq = h.bb / h.bw;
    sa = r[15] + a * r[16] + bq * r[17]; sb = r[18] + a * r[19] + bq * r[20];
}
// every facet of the eye's table, from global memory (block-uniform addresses)
__device__ __forceinline__ XrHit xr_search_all(const float* __restrict__ tab, int nf, float xc, float yc) {
    XrHit h = {-1, 1.0f, 0.f, 0.f, 1.f};
    XrPt p;
    for (int f = 0; f < nf; ++f) xr_cover(tab + f * XR_ROW_FLOATS, f, xc, yc, h, p);
    return h;
}
// A block stages the chain's coarse levels in LDS once, unless none of its pixels draws a band.  Every thread of the block calls this.
__device__ __forceinline__ void xr_stage_chain(bool need, const uint8_t* __restrict__ levels, int b, const XrGlowDev& G, float* __restrict__ lds) {
    if (__syncthreads_or(need)) {
        const uint8_t* __restrict__ src = levels + (long)b * G.chain_total + G.chain_off;
        for (int i = threadIdx.x; i < G.n_tex * 3; i += 256) lds[i] = (float)src[i];
        __syncthreads();
    }
}
// The tail of a pixel inside its eye image, _render_eye's order (effects.py:1050-1145) in float: clear; the outer band blended over
// it where no facet covers the pixel (where one does the screen, drawn with blending off, overwrites the band); the screen at
// (sa, sb); the inner band's draws blended over the screen, in draw order; the frost kernel's walls blended over whatever is there
// (a kernel has a glow or walls, never both); alpha_mode; the store.  plane: the outer band's piece is
// drawn at this pixel, (ga, gb) its point in the screen's coordinates.  N = 0: no glow.
struct XrDraw { bool on; float a, b; };
// The walls of the veil and frosted looks, drawn after the screen with the depth test off (_render_flat_frost_with_uniforms,
// effects.py:804-814): operator() blends every wall that covers the pixel into c, in draw order, and says whether one drew.
struct XrNoWalls {
    static constexpr bool ON = false;
    __device__ __forceinline__ bool operator()(float*) const { return false; }
};
// rows: the eye's four wall rows (dibr_xr.h).  Per wall: the plane point's (a, t); inside the trapezoid |a| <= g(t), 0 <= t <= 1, with
// clip w > 0 and NDC z in [-1, 1]; the grid cell -- row i from t, column j between the column lines a = (j / 4 - 1) * g(t); the cell's
// triangle (the strip's order A (s_j, t_i), B (s_j, t_i+1), C (s_j+1, t_i), D (s_j+1, t_i+1) makes B - C the diagonal); s at the
// point, affine over the triangle in (a, t): ABC: s_j + (a - a_j(t)) / (2 g(t_i)); BCD: s_j+1 - (a_j+1(t) - a) / (2 g(t_i+1)).
template <int MODE>
struct XrWalls {
    static constexpr bool ON = true;
    const float* __restrict__ rows;
    float xc, yc;
    const XrFrostDev& F;
    const DibrGeomProj& g;
    const uint8_t* __restrict__ lev0;
    const uint8_t* __restrict__ lev1;
    __device__ __forceinline__ bool operator()(float c[4]) const {
        bool drew = false;
        for (int k = 0; k < XR_WALLS; ++k) {
            const float* __restrict__ r = rows + k * XR_ROW_FLOATS;
            const XrPt p = xr_row_at(r, xc, yc);
            if (!(p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f)) continue;
            const float a = p.na / p.nw, t = p.nb / p.nw, slope = r[15], gt = 1.0f + slope * t;
            if (!(t >= 0.f && t <= 1.0f && fabsf(a) <= gt)) continue;
            const int i = min((int)(t * (float)XR_FROST_GRID), XR_FROST_GRID - 1);
            const int j = min(max((int)floorf((a / gt + 1.0f) * (0.5f * (float)XR_FROST_GRID)), 0), XR_FROST_GRID - 1);
            const float t1 = (float)(i + 1) * (1.0f / XR_FROST_GRID), g0 = 1.0f + slope * ((float)i * (1.0f / XR_FROST_GRID)), g1 = 1.0f + slope * t1;
            const float pj = (float)j * (2.0f / XR_FROST_GRID) - 1.0f, pj1 = (float)(j + 1) * (2.0f / XR_FROST_GRID) - 1.0f;
            const float xb = pj * g1, xcn = pj1 * g0;
            const bool abc = (xcn - xb) * (t - t1) + (1.0f / XR_FROST_GRID) * (a - xb) <= 0.f;
            const float s = abc ? (float)j * (1.0f / XR_FROST_GRID) + (a - pj * gt) / (2.0f * g0)
                                : (float)(j + 1) * (1.0f / XR_FROST_GRID) - (pj1 * gt - a) / (2.0f * g1);
            const bool s_is_v = r[16] != 0.f;
            float src[4];
            if (frost_frag<MODE>(F, g, lev0, lev1, s_is_v ? r[17] : s, s_is_v ? s : r[17], t, src)) { glow_blend(c, src); drew = true; }
        }
        return drew;
    }
};
// BG: the background an uncovered pixel starts from (dibr_pano.h): XrClearBg, the clear colour, or XrPanoBg, the panorama.
template <int OUT_FMT, class D, int N, class WALLS = XrNoWalls, class BG = XrClearBg>
__device__ __forceinline__ void xr_tail(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
                                        const DibrGeomProj& g, const XrEyes& ex, const XrGlowDev& G, const float* __restrict__ lds,
                                        const XrPix& px, bool covered, float sa, float sb, bool plane, float ga, float gb, const XrDraw* draws,
                                        const WALLS walls = WALLS(), const BG bg = BG()) {
    const int nch = g.alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    const long o = px.e.out_off + (((long)px.b * px.e.h + px.y) * px.e.w + px.x) * nch;
    float c[4], src[4];
    if (!covered) {
        bg(ex, px, c);
        if (N > 0 && plane && glow_frag(lds, G, g, ga, gb, false, src)) {
            glow_blend(c, src);
            if (g.alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED) { c[0] *= c[3]; c[1] *= c[3]; c[2] *= c[3]; }
        }
        if (WALLS::ON && walls(c) && g.alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED) { c[0] *= c[3]; c[1] *= c[3]; c[2] *= c[3]; }
        dibr_store<OUT_FMT>(out_all, o, nch, c);
        return;
    }
    const float quv[2] = {sa, 1.0f - sb};
    GenSmp<D> smp;
    smp.rgb = rgb_all + (long)px.b * g.H * g.W * 3; smp.dep = D::make(dep_all, px.b, g); smp.H = g.H; smp.W = g.W;
    dibr_pixel<false, false, true, true>(smp, g, 0, 0, px.e.eye, c, nullptr, quv);      // the framebuffer's own (rgb, a): alpha_mode acts after the inner band
    // (written out, not a loop: unrolled late, the curved kernel's FullDep form took 74 VGPRs for 72 and lost a wave per SIMD)
    if (N > 0 && draws[0].on && glow_frag(lds, G, g, draws[0].a, draws[0].b, true, src)) glow_blend(c, src);
    if (N > 1 && draws[1].on && glow_frag(lds, G, g, draws[1].a, draws[1].b, true, src)) glow_blend(c, src);
    if (WALLS::ON) walls(c);
    if (g.alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED) { c[0] *= c[3]; c[1] *= c[3]; c[2] *= c[3]; }
    dibr_store<OUT_FMT>(out_all, o, nch, c);
}

// d2s_dibr_xr_eyes: every facet of the eye's table is tested.  No barrier in this kernel: a thread outside its image leaves at once.
// BG (here and in the two kernels below): XrClearBg, or XrPanoBg with the panorama's XrPanoDev, image and chain behind it.
template <class BG> __device__ __forceinline__ BG xr_bg(const typename BG::Dev& P, const uint8_t* __restrict__ pano_rgb, const uint8_t* __restrict__ pano_chain) {
    if constexpr (BG::ON) return BG{P, pano_rgb, pano_chain}; else return BG{};
}
template <int OUT_FMT, class D, class BG = XrClearBg>
__global__ void __launch_bounds__(256)
dibr_xr_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
               const XrFacet* __restrict__ tab_all, DibrGeomProj g, XrEyes ex, typename BG::Dev P = {},
               const uint8_t* __restrict__ pano_rgb = nullptr, const uint8_t* __restrict__ pano_chain = nullptr) {
    const XrPix px = xr_pix(ex);
    if (!px.inside) return;
    const float* __restrict__ tab = (const float*)(tab_all + px.ei * XR_MAX_FACETS);
    const XrHit h = xr_search_all(tab, px.e.nf, px.xc, px.yc);
    float sa = 0.f, sb = 0.f;
    if (h.best >= 0) xr_hit_uv(tab + h.best * XR_ROW_FLOATS, h, sa, sb);
    xr_tail<OUT_FMT, D, 0, XrNoWalls, BG>(rgb_all, dep_all, out_all, g, ex, XrGlowDev{}, nullptr, px, h.best >= 0, sa, sb, false, 0.f, 0.f, nullptr,
                                          XrNoWalls(), xr_bg<BG>(P, pano_rgb, pano_chain));
}
// d2s_dibr_xr_eyes_glow (flat screen, one facet).  The glow quad is the screen's plane: facet 0's homography without the 0..1 bound
// gives its coordinates; it is drawn where clip w > 0 and NDC z is in [-1, 1].  (The quad ends at screen + range; the glow reaches 0
// there or sooner -- edge_t = 1 -- so the quad's own bound is not tested.)  The chain is staged unless the block's whole tile is plain
// screen or undrawn.  Barriers: xr_stage_chain's, reached by every thread; the threads outside the image leave after it.
template <int OUT_FMT, class D, class BG = XrClearBg>
__global__ void __launch_bounds__(256)
dibr_xr_glow_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
                    const XrFacet* __restrict__ tab_all, DibrGeomProj g, XrEyes ex, XrGlowDev G, const uint8_t* __restrict__ levels,
                    typename BG::Dev P = {}, const uint8_t* __restrict__ pano_rgb = nullptr, const uint8_t* __restrict__ pano_chain = nullptr) {
    extern __shared__ float xr_glow_lds[];               // [n_tex][3]
    const XrPix px = xr_pix(ex);
    const float* __restrict__ tab = (const float*)(tab_all + px.ei * XR_MAX_FACETS);
    const XrHit h = xr_search_all(tab, px.e.nf, px.xc, px.yc);
    const XrPt p = xr_row_at(tab, px.xc, px.yc);
    const bool plane = p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f;
    const float ga = p.na / p.nw, gb = p.nb / p.nw;
    float cx, cy;
    xr_stage_chain(px.inside && plane && (h.best < 0 || (G.mode == 1 && glow_sd(G, ga, gb, cx, cy) >= -G.inner)), levels, px.b, G, xr_glow_lds);
    if (!px.inside) return;
    float sa = 0.f, sb = 0.f;
    if (h.best >= 0) xr_hit_uv(tab + h.best * XR_ROW_FLOATS, h, sa, sb);
    const XrDraw inner = {G.mode == 1 && plane, ga, gb};
    xr_tail<OUT_FMT, D, 1, XrNoWalls, BG>(rgb_all, dep_all, out_all, g, ex, G, xr_glow_lds, px, h.best >= 0, sa, sb, plane, ga, gb, &inner,
                                          XrNoWalls(), xr_bg<BG>(P, pano_rgb, pano_chain));
}

// d2s_dibr_xr_eyes_frost (flat screen): dibr_xr_kernel with the four walls of the veil (MODE 1) or frosted (MODE 2) look blended after
// the screen.  No barrier and no LDS: the wall rows are block-uniform global reads as the facet's are; the frosted taps read the two
// chain levels textureLod(u_lod) mixes from global memory (at the default LOD 5.4 of a 1080p frame 60 x 33 and 30 x 16 texels).
template <int OUT_FMT, class D, int MODE, class BG = XrClearBg>
__global__ void __launch_bounds__(256)
dibr_xr_frost_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
                     const XrFacet* __restrict__ tab_all, DibrGeomProj g, XrEyes ex, XrFrostDev F, const uint8_t* __restrict__ levels,
                     typename BG::Dev P = {}, const uint8_t* __restrict__ pano_rgb = nullptr, const uint8_t* __restrict__ pano_chain = nullptr) {
    const XrPix px = xr_pix(ex);
    if (!px.inside) return;
    const float* __restrict__ tab = (const float*)(tab_all + px.ei * xr_table_rows(D2S_XR_KIND_FROST));
    const XrHit h = xr_search_all(tab, px.e.nf, px.xc, px.yc);
    float sa = 0.f, sb = 0.f;
    if (h.best >= 0) xr_hit_uv(tab + h.best * XR_ROW_FLOATS, h, sa, sb);
    const uint8_t* __restrict__ frame = rgb_all + (long)px.b * g.H * g.W * 3;
    const uint8_t* __restrict__ chain = MODE == 2 ? levels + (long)px.b * F.chain_total : nullptr;      // (the veil never reads levels)
    const XrWalls<MODE> walls = {tab + px.e.nf * XR_ROW_FLOATS, px.xc, px.yc, F, g, (MODE == 2 && F.l0 > 0) ? chain + F.off0 : frame,
                                 (MODE == 2 && F.l1 > 0) ? chain + F.off1 : frame};
    xr_tail<OUT_FMT, D, 0, XrWalls<MODE>, BG>(rgb_all, dep_all, out_all, g, ex, XrGlowDev{}, nullptr, px, h.best >= 0, sa, sb, false, 0.f, 0.f,
                                              nullptr, walls, xr_bg<BG>(P, pano_rgb, pano_chain));
}

// d2s_dibr_xr_eyes_frost_curved: the curved screen with the 196 triangles of its veil (MODE 1) or frosted (MODE 2) walls blended after it
// in draw order (_render_curved_frost_with_uniforms, xr_viewer/effects.py:759-787; rows: dibr_xr.h).  A block draws
// XR_BIN_TILES x XR_BIN_TILES tiles of 16 x 16 pixels.  It bins first: thread r < 244 tests row r at the four corners of the block's
// pixel centres grown by one pixel (the per-pixel test rounds by about 1e-4 pixel) and drops the row when one of its edge functions,
// or nw, is negative at all four -- each is linear, so it is negative at every pixel of the block.  The rows kept are the four waves'
// ballots, 32 bytes of LDS: bit r of word r / 64.  One barrier, reached by every thread; a mask word is then read into scalar
// registers and every pixel walks its set bits in row order, so the row reads stay block-uniform as dibr_xr_kernel's are.  Bits < 48 go through
// xr_cover (the screen: dibr_xr_kernel's facet, a / w and b / w, since a facet that covers no pixel of the block changes no hit);
// bits >= 48 are the walls' functor in xr_tail.  bin == 0 (D2S_XR_BIN=0): every row is kept.
__device__ __forceinline__ uint64_t xr_uniform64(uint64_t v) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}
// the row can cover no pixel centre of x0 .. x1, y0 .. y1
__device__ __forceinline__ bool xr_row_out(const float* __restrict__ r, bool tri, float x0, float y0, float x1, float y1) {
    const float xs[4] = {x0, x1, x0, x1}, ys[4] = {y0, y0, y1, y1};
    float na = -INFINITY, nb = -INFINITY, nw = -INFINITY, ne = -INFINITY, nu = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float b = r[3] * xs[k] + r[4] * ys[k] + r[5], w = r[6] * xs[k] + r[7] * ys[k] + r[8];
        na = fmaxf(na, r[0] * xs[k] + r[1] * ys[k] + r[2]); nb = fmaxf(nb, b); nw = fmaxf(nw, w);
        ne = fmaxf(ne, r[12] * xs[k] + r[13] * ys[k] + r[14]); nu = fmaxf(nu, w - b);
    }
    return na < 0.f || nb < 0.f || nw < 0.f || ne < 0.f || (!tri && nu < 0.f);      // (a facet also ends at b = 1)
}
template <int MODE>
struct XrTriWalls {
    static constexpr bool ON = true;
    const float* __restrict__ tab;                       // the eye's table: row 48 is triangle 0
    const uint64_t* __restrict__ kept;                   // the block's four masks in LDS (re-read per word: one copy of the shading below)
    float xc, yc;
    const XrFrostDev& F;
    const DibrGeomProj& g;
    const uint8_t* __restrict__ lev0;
    const uint8_t* __restrict__ lev1;
    __device__ __forceinline__ bool operator()(float c[4]) const {
        bool drew = false;
#pragma unroll 1
        for (int w = 0; w < 4; ++w) {
            uint64_t m = xr_uniform64(kept[w]);
            if (w == 0) m &= ~((1ull << XR_MAX_FACETS) - 1);
            while (m) {
                const int row = w * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const float* __restrict__ r = tab + row * XR_ROW_FLOATS;
                const XrPt p = xr_row_at(r, xc, yc);
                const float ne = r[12] * xc + r[13] * yc + r[14];      // the wall's previous triangle's nb, negated (dibr_xr.h)
                if (!(p.na >= 0.f && p.nb >= 0.f && (xr_tri_first(row - XR_MAX_FACETS) ? ne >= 0.f : ne > 0.f))) continue;
                if (!(p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f)) continue;
                const float a = p.na / p.nw, b = p.nb / p.nw;
                float src[4];
                if (frost_frag<MODE>(F, g, lev0, lev1, r[15] + a * r[16] + b * r[17], r[18] + a * r[19] + b * r[20],
                                     r[21] + a * r[22] + b * r[23], src)) { glow_blend(c, src); drew = true; }
            }
        }
        return drew;
    }
};
// BG: dibr_xr_kernel's.  The background is block-invariant: it is built once, outside the tile loop, and adds no barrier.
template <int OUT_FMT, class D, int MODE, class BG = XrClearBg>
__global__ void __launch_bounds__(256)
dibr_xr_frost_curved_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
                            const XrFacet* __restrict__ tab_all, DibrGeomProj g, XrEyes ex, XrFrostDev F, const uint8_t* __restrict__ levels,
                            int bin, typename BG::Dev P = {}, const uint8_t* __restrict__ pano_rgb = nullptr,
                            const uint8_t* __restrict__ pano_chain = nullptr) {
    __shared__ uint64_t kept[4];
    const int ei = blockIdx.z % ex.n;
    const float* __restrict__ tab = (const float*)(tab_all + ei * XR_FROST_CURVED_ROWS);
    {
        const int r = threadIdx.x, side = 16 * XR_BIN_TILES;
        bool keep = r < XR_FROST_CURVED_ROWS;
        if (keep && bin) {
            const float x0 = ((float)(blockIdx.x * side) + 0.5f) - 0.5f * (float)ex.e[ei].w - 1.0f;
            const float y0 = ((float)(blockIdx.y * side) + 0.5f) - 0.5f * (float)ex.e[ei].h - 1.0f;
            keep = !xr_row_out(tab + r * XR_ROW_FLOATS, r >= XR_MAX_FACETS, x0, y0, x0 + (float)(side + 1), y0 + (float)(side + 1));
        }
        const uint64_t m = __ballot(keep);
        if ((threadIdx.x & 63) == 0) kept[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    const uint64_t facets = xr_uniform64(kept[0]) & ((1ull << XR_MAX_FACETS) - 1);
    const BG bg = xr_bg<BG>(P, pano_rgb, pano_chain);
#pragma unroll 1
    for (int t = 0; t < XR_BIN_TILES * XR_BIN_TILES; ++t) {
        const XrPix px = xr_pix_at(ex, blockIdx.x * XR_BIN_TILES + t % XR_BIN_TILES, blockIdx.y * XR_BIN_TILES + t / XR_BIN_TILES);
        if (!px.inside) continue;                          // (no barrier below)
        XrHit h = {-1, 1.0f, 0.f, 0.f, 1.f};
        XrPt p;
        for (uint64_t m = facets; m; m &= m - 1) {
            const int f = __builtin_ctzll(m);
            xr_cover(tab + f * XR_ROW_FLOATS, f, px.xc, px.yc, h, p);
        }
        float sa = 0.f, sb = 0.f;
        if (h.best >= 0) xr_hit_uv(tab + h.best * XR_ROW_FLOATS, h, sa, sb);
        const uint8_t* __restrict__ frame = rgb_all + (long)px.b * g.H * g.W * 3;
        const uint8_t* __restrict__ chain = MODE == 2 ? levels + (long)px.b * F.chain_total : nullptr;      // (the veil never reads levels)
        const XrTriWalls<MODE> walls = {tab, kept, px.xc, px.yc, F, g, (MODE == 2 && F.l0 > 0) ? chain + F.off0 : frame,
                                        (MODE == 2 && F.l1 > 0) ? chain + F.off1 : frame};
        xr_tail<OUT_FMT, D, 0, XrTriWalls<MODE>, BG>(rgb_all, dep_all, out_all, g, ex, XrGlowDev{}, nullptr, px, h.best >= 0, sa, sb, false, 0.f,
                                                     0.f, nullptr, walls, bg);
    }
}

// d2s_dibr_xr_eyes_glow_curved: the curved screen with its glow (_render_curved_glow, xr_viewer/effects.py:408-474, in _render_eye's
// order, :1050-1145).  Threads and tiles as above.  The eye's 52 piece rows (dibr_xr.h) and 49 seam rows are staged in LDS -- a
// lane's search index diverges, so they are LDS reads, rows padded to 25 floats and seams 3 floats apart (odd strides: lanes on
// neighbouring rows read different banks, lanes on one row broadcast).  A pixel finds its piece from the seams' signs: the two arc
// ends say whether its ray passes the arc (then a binary search over the 47 interior seams, 6 steps), a tangent piece, or -- a ray
// more than a half turn from one end, both end seams "beyond" -- either tangent piece.  The facet found and its two neighbours then
// go through xr_cover, so a screen pixel has the facet, a / w and b / w of dibr_xr_kernel; a pixel no facet covers takes the band on
// the piece the seams gave it.  Homographies per pixel: at most 3 facets + 2 others, whatever the strip's 48.
// Barriers: the one after the rows' staging and xr_stage_chain's, each reached by every thread; the threads outside the image leave
// after the second.  BG: dibr_xr_kernel's; the background is formed in xr_tail, after both barriers.
template <int OUT_FMT, class D, class BG = XrClearBg>
__global__ void __launch_bounds__(256)
dibr_xr_glow_curved_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all,
                           const XrFacet* __restrict__ tab_all, DibrGeomProj g, XrEyes ex, XrGlowDev G, XrCurvedDev Q,
                           const uint8_t* __restrict__ levels, typename BG::Dev P = {}, const uint8_t* __restrict__ pano_rgb = nullptr,
                           const uint8_t* __restrict__ pano_chain = nullptr) {
    extern __shared__ float xr_glow_lds[];               // [n_tex][3]
    __shared__ float rows[XR_PIECES * XR_LDS_ROW];
    __shared__ float seams[XR_SEAMS * 3];
    const XrPix px = xr_pix(ex);
    {
        const float* __restrict__ src = (const float*)(tab_all + px.ei * XR_PIECES);
        for (int i = threadIdx.x; i < XR_PIECES * XR_ROW_FLOATS; i += 256) rows[(i / XR_ROW_FLOATS) * XR_LDS_ROW + i % XR_ROW_FLOATS] = src[i];
        if (threadIdx.x < XR_SEAMS * 3) {
            const int s = threadIdx.x / 3, k = threadIdx.x % 3;
            seams[threadIdx.x] = s < XR_MAX_FACETS ? src[s * XR_ROW_FLOATS + k] : -src[(XR_MAX_FACETS - 1) * XR_ROW_FLOATS + 12 + k];
        }
        __syncthreads();
    }
    const float xc = px.xc, yc = px.yc;
    auto seam = [&](int s) { return seams[s * 3] * xc + seams[s * 3 + 1] * yc + seams[s * 3 + 2]; };
    // f: the facet the seams give (0 .. 47), -1 / 48: the tangent piece at the lower / upper end, -2: either tangent piece
    int f;
    {
        const bool lo_in = seam(0) >= 0.f, hi_in = seam(XR_MAX_FACETS) < 0.f;
        if (lo_in && hi_in) {
            int lo = 0, hi = XR_MAX_FACETS;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (seam(mid) >= 0.f) lo = mid; else hi = mid;
            }
            f = lo;
        } else f = lo_in ? XR_MAX_FACETS : (hi_in ? -1 : -2);
    }
    XrHit h = {-1, 1.0f, 0.f, 0.f, 1.f};
    bool plane = false, band_set = false;                // the band's piece is drawn at this pixel; a facet has claimed the band
    float pz = 0.f, ga = 0.f, gb = 0.f;                  // its depth and its point in the screen's coordinates
    auto band = [&](const float* __restrict__ r, const XrPt& p) {
        if (p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f && (!plane || p.z < pz)) {
            const float a = p.na / p.nw, bq = p.nb / p.nw;
            plane = true; pz = p.z;
            ga = r[15] + a * r[16] + bq * r[17]; gb = r[18] + a * r[19] + bq * r[20];
        }
    };
    for (int c = max(f - 1, 0); c <= min(f + 1, XR_MAX_FACETS - 1) && f >= -1; ++c) {
        const float* __restrict__ r = rows + c * XR_LDS_ROW;
        XrPt p;
        if (xr_cover(r, c, xc, yc, h, p) && !band_set && f >= 0 && f < XR_MAX_FACETS) { band_set = true; band(r, p); }      // (the lowest facet between its seams)
    }
    if (f < 0) { const float* r = rows + XR_T0 * XR_LDS_ROW; band(r, xr_row_at(r, xc, yc)); }
    if (f == XR_MAX_FACETS || f == -2) { const float* r = rows + XR_T1 * XR_LDS_ROW; band(r, xr_row_at(r, xc, yc)); }
    // the screen pixel: its facet's uv, which is also its point in the screen's coordinates; mode 1: the inner band's two draws
    bool fband = false, cband = false;
    float sa = 0.f, sb = 0.f, ca = 0.f, cb = 0.f;
    if (h.best >= 0) {
        xr_hit_uv(rows + h.best * XR_LDS_ROW, h, sa, sb);
        if (G.mode == 1) {
            const float al = Q.vertical ? sb : sa, ac = Q.vertical ? sa : sb;
            const bool edge_ac = ac <= Q.e_ac || ac >= 1.0f - Q.e_ac;
            fband = Q.vertical ? (edge_ac && al >= Q.e_al && al <= 1.0f - Q.e_al) : edge_ac;
            const float* __restrict__ rc = rows + (al < 0.5f ? XR_C0 : XR_C1) * XR_LDS_ROW;
            const XrPt p = xr_row_at(rc, xc, yc);
            if (p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f && p.na >= 0.f && p.na <= p.nw) {
                const float a2 = p.na / p.nw, b2 = p.nb / p.nw;
                ca = rc[15] + a2 * rc[16] + b2 * rc[17]; cb = rc[18] + a2 * rc[19] + b2 * rc[20];
                const float cac = Q.vertical ? ca : cb;
                cband = Q.vertical ? (cac >= 0.f && cac <= 1.0f) : (cac >= Q.e_ac && cac <= 1.0f - Q.e_ac);
            }
        }
    }
    xr_stage_chain(px.inside && (h.best < 0 ? plane : (fband || cband)), levels, px.b, G, xr_glow_lds);
    if (!px.inside) return;
    // the mesh's draw order (_build_curved_glow_band_verts:401-404): the u-long bands, then the v-long ones
    const XrDraw on_facet = {fband, sa, sb}, on_chord = {cband, ca, cb};
    const XrDraw draws[2] = {Q.vertical ? on_chord : on_facet, Q.vertical ? on_facet : on_chord};
    xr_tail<OUT_FMT, D, 2, XrNoWalls, BG>(rgb_all, dep_all, out_all, g, ex, G, xr_glow_lds, px, h.best >= 0, sa, sb, plane, ga, gb, draws,
                                          XrNoWalls(), xr_bg<BG>(P, pano_rgb, pano_chain));
}

// d2s_dibr_xr_panels: the world-space panels, in place over finished eye images (rows: dibr_xr.h; _OVERLAY_FRAG and _SOLID_FRAG,
// xr_viewer/glsl.py:28-40, 106-112).  Threads and tiles as dibr_xr_kernel's, over the rectangle of tiles the panels' boxes touch; a
// block whose tile no box touches leaves before it reads anything but the boxes.  No barrier, no LDS: the rows and the textures'
// records are block-uniform reads.  Per pixel: z = the screen's depth from xr_search_all (1.0 uncovered), the destination read once,
// the panels in order, one store if a panel passed.
// One GL_LINEAR tap of an RGBA8 texture whose row 0 is the picture's top: GL's row coordinate v * h - 0.5 counted from the top is
// (1 - v) * h - 0.5.  -> rgb in levels, alpha 0..1
__device__ __forceinline__ void panel_texture(const XrTexDev& t, float u, float v, float s[4]) {
    const float x = u * (float)t.w - 0.5f, y = (1.0f - v) * (float)t.h - 0.5f;
    const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;
    if (t.wrap == D2S_XR_WRAP_REPEAT) {
        x0 %= t.w; x0 += x0 < 0 ? t.w : 0; x1 %= t.w; x1 += x1 < 0 ? t.w : 0;
        y0 %= t.h; y0 += y0 < 0 ? t.h : 0; y1 %= t.h; y1 += y1 < 0 ? t.h : 0;
    } else {
        x0 = min(max(x0, 0), t.w - 1); x1 = min(max(x1, 0), t.w - 1); y0 = min(max(y0, 0), t.h - 1); y1 = min(max(y1, 0), t.h - 1);
    }
    const uint32_t* __restrict__ px = (const uint32_t*)t.rgba;
    const uint32_t a = px[(long)y0 * t.w + x0], b = px[(long)y0 * t.w + x1], c = px[(long)y1 * t.w + x0], d = px[(long)y1 * t.w + x1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float fa = (float)((a >> (8 * k)) & 255u), fb = (float)((b >> (8 * k)) & 255u);
        const float fc = (float)((c >> (8 * k)) & 255u), fd = (float)((d >> (8 * k)) & 255u);
        const float top = fa + (fb - fa) * fx, bot = fc + (fd - fc) * fx;
        s[k] = top + (bot - top) * fy;
    }
    s[3] *= 1.0f / 255.0f;
}
template <int OUT_FMT>
__global__ void __launch_bounds__(256)
dibr_xr_panels_kernel(void* __restrict__ out_all, const XrFacet* __restrict__ tab_all, XrEyes ex, XrPanelsDev P) {
    const int ei = blockIdx.z % ex.n;
    if ((int)blockIdx.x >= P.tiles[ei][0] || (int)blockIdx.y >= P.tiles[ei][1]) return;
    const int tx = P.tile0[ei][0] + (int)blockIdx.x, ty = P.tile0[ei][1] + (int)blockIdx.y;
    const float* __restrict__ tab = (const float*)(tab_all + ei * XR_PANEL_ROWS);
    const int nf = ex.e[ei].nf;
    uint32_t live = 0;                                     // the panels whose box touches this tile (block-uniform)
    for (int k = 0; k < P.n; ++k) {
        const float* __restrict__ r = tab + (nf + k) * XR_ROW_FLOATS;
        if ((float)(tx * 16) < r[14] && (float)(tx * 16 + 16) > r[12] && (float)(ty * 16) < r[15] && (float)(ty * 16 + 16) > r[13]) live |= 1u << k;
    }
    if (!live) return;
    const XrPix px = xr_pix_at(ex, tx, ty);
    if (!px.inside) return;
    float z = xr_search_all(tab, nf, px.xc, px.yc).bz;
    const long o = px.e.out_off + (((long)px.b * px.e.h + px.y) * px.e.w + px.x) * P.nch;
    float c[4] = {0.f, 0.f, 0.f, 1.f};
    if (OUT_FMT == D2S_FMT_U8_HWC) {
        const uint8_t* __restrict__ d = (const uint8_t*)out_all + o;
        c[0] = (float)d[0]; c[1] = (float)d[1]; c[2] = (float)d[2];
        if (P.nch == 4) c[3] = (float)d[3] * (1.0f / 255.0f);
    } else {
        const float* __restrict__ d = (const float*)out_all + o;
        c[0] = d[0]; c[1] = d[1]; c[2] = d[2];
        if (P.nch == 4) c[3] = d[3];
    }
    bool drew = false;
    for (uint32_t m = live; m; m &= m - 1) {
        const float* __restrict__ r = tab + (nf + __builtin_ctz(m)) * XR_ROW_FLOATS;
        const XrPt p = xr_row_at(r, px.xc, px.yc);
        if (!(p.na >= 0.f && p.nb >= 0.f && p.na <= p.nw && p.nb <= p.nw && p.nw > 0.f && p.z >= -1.0f && p.z <= 1.0f)) continue;
        const uint32_t flags = (uint32_t)r[17];
        if ((flags & D2S_XR_PANEL_DEPTH_TEST) && !(p.z < z)) continue;      // GL_LESS
        float s[4] = {r[18], r[19], r[20], r[21]};
        const int tex = (int)r[16];
        if (tex >= 0) {
            panel_texture(P.t[tex], p.na / p.nw, p.nb / p.nw, s);
            s[3] *= r[22];
        }
        if (flags & D2S_XR_PANEL_BLEND) {                    // SRC_ALPHA, ONE_MINUS_SRC_ALPHA, alpha included
            const float sa = s[3], ia = 1.0f - sa;
            c[0] = sa * s[0] + ia * c[0]; c[1] = sa * s[1] + ia * c[1]; c[2] = sa * s[2] + ia * c[2]; c[3] = sa * sa + ia * c[3];
        } else { c[0] = s[0]; c[1] = s[1]; c[2] = s[2]; c[3] = s[3]; }
        // (GL writes depth only where the depth test is enabled)
        if ((flags & (D2S_XR_PANEL_DEPTH_TEST | D2S_XR_PANEL_DEPTH_WRITE)) == (D2S_XR_PANEL_DEPTH_TEST | D2S_XR_PANEL_DEPTH_WRITE)) z = p.z;
        drew = true;
    }
    if (drew) dibr_store<OUT_FMT>(out_all, o, P.nch, c);
}

int dibr_warp_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                  void* out, int out_fmt, void* stream, bool check_only);      // (also called by d2s_view_pipeline_streams, engine.hip)
int dibr_warp_crop_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                       const double* crop, void* out, int out_fmt, void* stream, bool check_only);      // (d2s_view_pipeline_crop_streams)

}  // namespace d2s

using namespace d2s;

extern "C" int d2s_dibr_shape(int H, int W, int display_mode, int* out_h, int* out_w) {
    D2S_REQUIRE(out_h && out_w && H > 0 && W > 0, "bad argument");
    int oh = 0, ow = 0;
    return dibr_eye_shape(H, W, display_mode, &oh, &ow, out_h, out_w);
}

// Everything dibr_warp_impl decides, stated once on the host (d2s_dibr_warp_plan reports it; tests/test_cpu_dibr_plan.py pins it):
// the checks of everything that is no pointer, the uniforms, the eye shape, the three switches, the window plan, and from them the
// kernel, its grid and its LDS.  No HIP call.
struct DibrWarpPlan {
    DibrWindow win;
    bool roll0, up, fx, u8;
    dim3 grid, block;
    unsigned lds_dynamic, lds_static;      // the row kernel's request; 0 for the gather kernel
};
// the kernel's name with its template arguments (formed for d2s_dibr_warp_plan only: the launch path formats nothing)
static void dibr_plan_name(const DibrWarpPlan& pl, bool crop, char* name, size_t n) {
    const char* fmt = pl.u8 ? "u8" : "f32";
    const char* dname = pl.up ? "UpDep" : "FullDep";
    if (pl.win.rows) snprintf(name, n, "dibr_rows<%s,fx=%d,%d,%s%s>", fmt, pl.fx ? 1 : 0, pl.win.cols, dname, crop ? ",crop" : "");
    else snprintf(name, n, "dibr<%s,%s,%s%s>", fmt, pl.roll0 ? "roll0" : "general", dname, crop ? ",crop" : "");
}
template <class G>
static int dibr_warp_plan_impl(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double* crop, int out_fmt,
                               G& g, DibrWarpPlan& pl) {
    constexpr bool CR = G::crop;
    int rc = dibr_check(p, dh, dw, batch, H, W, out_fmt);
    if (rc) return rc;
    dibr_fill_geom(g, p, H, W, dh, dw);
    g.mode = p->display_mode;
    pl.up = dh != H || dw != W;
    rc = CR ? crop_eye_shape(H, W, crop, p->display_mode, &g.oh, &g.ow, &g.out_h, &g.out_w)
            : dibr_eye_shape(H, W, p->display_mode, &g.oh, &g.ow, &g.out_h, &g.out_w);
    if (rc) return rc;
    if constexpr (CR) { g.cx = (float)crop[0]; g.cy = (float)crop[1]; g.cw = (float)crop[2]; g.ch = (float)crop[3]; }
    const bool vp0 = p->viewport[2] == 0.f && p->viewport[3] == 0.f;
    D2S_REQUIRE(vp0 || (p->viewport[2] > 0.f && p->viewport[3] > 0.f), "viewport width / height must be positive (or all zero)");
    g.vpx = vp0 ? 0.f : p->viewport[0]; g.vpy = vp0 ? 0.f : p->viewport[1];
    g.vpw = vp0 ? (float)g.ow : p->viewport[2]; g.vph = vp0 ? (float)g.oh : p->viewport[3];
    D2S_REQUIRE(2 * g.oh <= 65535, "frame too large for one launch");
    static EnvInt no_roll0{"D2S_DIBR_NO_ROLL0", 0};        // (A/B aids: the general per-tap evaluation for roll == 0 too;
    static EnvInt no_rows{"D2S_DIBR_NO_ROWS", 0};          //  the gather kernel instead of the LDS-window kernel;
    static EnvInt cols_env{"D2S_DIBR_COLS", 512};          //  256 | 512 | 1024 caps the columns per block)
    pl.roll0 = g.s == 0.f && g.c == 1.f && !no_roll0.get();
    // source texels per output column: W / ow, of the cropped span with a crop (1 when the eye viewport is the crop's pixel size)
    double tex_per_col = (double)W / (double)g.ow;
    if constexpr (CR) tex_per_col *= (double)g.cw;
    // columns per block: 512 while the window stays <= 640 texels (20 KB of LDS: seven blocks per CU either way).  1080p Full-SBS
    // 50.8 -> 46.8 us (half the second-pass waves); Half-SBS (two source texels per column) keeps 256: 24.4 us against 26.8;
    // 1024 columns: 63.9 us (34 KB per block), an A/B aid of the uncropped FullDep kernels only, up to 1536 texels (48 KB).
    // Windows above DIBR_F1_ROWS_WORDS = 1983 texels -- the largest whose 8 planes fit 64 KB of LDS beside the 256-column kernel's
    // static queue -- take the gather kernel.
    const bool wide = cols_env.get() >= 1024 && !pl.up && !CR;
    pl.win = dibr_plan_window(g, tex_per_col, pl.roll0 && !no_rows.get(), wide ? 1024 : (cols_env.get() >= 512 ? 512 : 256),
                              wide ? 1536 : 640, DIBR_F1_ROWS_WORDS);
    pl.fx = g.feather || g.corner_r > 0.f;
    pl.u8 = out_fmt == D2S_FMT_U8_HWC;
    pl.block = dim3(256);
    if (pl.win.rows) {
        pl.grid = dim3(cdiv(g.ow, pl.win.cols), g.oh, batch);
        pl.lds_dynamic = dibr_rows_dynamic_lds(pl.win.WW);
        pl.lds_static = dibr_rows_static_lds(pl.win.cols);
        D2S_REQUIRE(pl.lds_dynamic + pl.lds_static <= DIBR_LDS_LIMIT, "internal: the window plan exceeds the LDS of a block");
    } else {
        pl.grid = dim3(cdiv(g.ow, 256), 2 * g.oh, batch);
        pl.lds_dynamic = pl.lds_static = 0;
    }
    return D2S_OK;
}

// d2s_dibr_warp (dh == H && dw == W: depth IS the texture, the FullDep kernels) and d2s_dibr_warp_depth (any other [dh, dw]: the
// UpDep kernels).  Every argument is checked before any HIP call.
// G = DibrGeom: crop == nullptr; G = DibrGeomCrop: d2s_dibr_warp_crop.
// The decision is dibr_warp_plan_impl's; this function looks at the pointers and launches what the plan says.
template <class G>
static int dibr_warp_impl(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                          const double* crop, void* out, int out_fmt, void* stream, bool check_only) {
    constexpr bool CR = G::crop;
    D2S_REQUIRE(rgb && depth && p && out, "null pointer");
    G g;
    DibrWarpPlan pl;
    const int rc = dibr_warp_plan_impl<G>(dh, dw, batch, H, W, p, crop, out_fmt, g, pl);
    if (rc) return rc;
    if (check_only) return D2S_OK;
    const bool up = pl.up, roll0 = pl.roll0, fx = pl.fx;
    const dim3 grid = pl.grid, block = pl.block;
    if (pl.win.rows) {
        const int margin = pl.win.margin, cols = pl.win.cols, WWc = pl.win.WW;
        const dim3 rgrid = grid;
        const size_t lds = pl.lds_dynamic;
#define DIBR_ROWS(FMT, FXV, COLS, D) hipLaunchKernelGGL((dibr_rows_kernel<FMT, FXV, COLS, D, G>), rgrid, block, lds, (hipStream_t)stream, rgb, depth, out, g, margin, WWc)
// (the 1 024-column form exists for the uncropped FullDep kernels only: `wide` is false otherwise, and it is not instantiated with a crop)
#define DIBR_ROWS_C(FMT, FXV) do { bool wide_done = false; \
                                   if constexpr (!CR) { if (cols == 1024) { DIBR_ROWS(FMT, FXV, 1024, FullDep); wide_done = true; } } \
                                   if (wide_done) break; \
                                   if (up) { if (cols == 512) DIBR_ROWS(FMT, FXV, 512, UpDep); else DIBR_ROWS(FMT, FXV, 256, UpDep); } \
                                   else if (cols == 512) DIBR_ROWS(FMT, FXV, 512, FullDep); \
                                   else DIBR_ROWS(FMT, FXV, 256, FullDep); } while (0)
        if (pl.u8) { if (fx) DIBR_ROWS_C(D2S_FMT_U8_HWC, true); else DIBR_ROWS_C(D2S_FMT_U8_HWC, false); }
        else { if (fx) DIBR_ROWS_C(D2S_FMT_F32_HWC, true); else DIBR_ROWS_C(D2S_FMT_F32_HWC, false); }
#undef DIBR_ROWS_C
#undef DIBR_ROWS
    } else {
#define DIBR_GEN(FMT, R0, D) hipLaunchKernelGGL((dibr_kernel<FMT, R0, D, G>), grid, block, 0, (hipStream_t)stream, rgb, depth, out, g)
#define DIBR_GEN_D(FMT, R0) do { if (up) DIBR_GEN(FMT, R0, UpDep); else DIBR_GEN(FMT, R0, FullDep); } while (0)
        if (pl.u8) { if (roll0) DIBR_GEN_D(D2S_FMT_U8_HWC, true); else DIBR_GEN_D(D2S_FMT_U8_HWC, false); }
        else { if (roll0) DIBR_GEN_D(D2S_FMT_F32_HWC, true); else DIBR_GEN_D(D2S_FMT_F32_HWC, false); }
#undef DIBR_GEN_D
#undef DIBR_GEN
    }
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

int d2s::dibr_warp_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                       void* out, int out_fmt, void* stream, bool check_only) {
    return dibr_warp_impl<DibrGeom>(rgb, depth, dh, dw, batch, H, W, p, nullptr, out, out_fmt, stream, check_only);
}
int d2s::dibr_warp_crop_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                            const double* crop, void* out, int out_fmt, void* stream, bool check_only) {
    D2S_REQUIRE(crop, "null pointer (crop)");
    return dibr_warp_impl<DibrGeomCrop>(rgb, depth, dh, dw, batch, H, W, p, crop, out, out_fmt, stream, check_only);
}

extern "C" int d2s_dibr_warp(const uint8_t* rgb, const float* depth, int batch, int H, int W, const d2s_dibr_params* p,
                             void* out, int out_fmt, void* stream) {
    return dibr_warp_any(rgb, depth, H, W, batch, H, W, p, out, out_fmt, stream, false);
}

extern "C" int d2s_dibr_warp_depth(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                   const d2s_dibr_params* p, void* out, int out_fmt, void* stream) {
    return dibr_warp_any(rgb, depth, dh, dw, batch, H, W, p, out, out_fmt, stream, false);
}

// The OpenXR screen's cropped warp (xr_viewer/implementation.py:111-126, crop.py:165-173).
extern "C" int d2s_dibr_crop_shape(int H, int W, const double crop[4], int display_mode, int* out_h, int* out_w) {
    D2S_REQUIRE(out_h && out_w, "null pointer (out_h, out_w)");
    int oh = 0, ow = 0;
    return crop_eye_shape(H, W, crop, display_mode, &oh, &ow, out_h, out_w);
}

extern "C" int d2s_dibr_warp_crop(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                  const d2s_dibr_params* p, const double crop[4], void* out, int out_fmt, void* stream) {
    return dibr_warp_crop_any(rgb, depth, dh, dw, batch, H, W, p, crop, out, out_fmt, stream, false);
}

// What the three entries above would launch: dibr_warp_plan_impl, the function the launcher takes its decision from.
extern "C" int d2s_dibr_warp_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double* crop, int out_fmt,
                                  d2s_dibr_warp_plan_result* res) {
    D2S_REQUIRE(p && res, "null pointer");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_dibr_warp_plan_result), "d2s_dibr_warp_plan_result.struct_size must be sizeof(d2s_dibr_warp_plan_result)");
    DibrWarpPlan pl;
    DibrGeomCrop g;      // (a DibrGeom with the crop's four floats: either instantiation fills it)
    const int rc = crop ? dibr_warp_plan_impl<DibrGeomCrop>(dh, dw, batch, H, W, p, crop, out_fmt, g, pl)
                        : dibr_warp_plan_impl<DibrGeom>(dh, dw, batch, H, W, p, nullptr, out_fmt, g, pl);
    if (rc) return rc;
    *res = d2s_dibr_warp_plan_result{sizeof(d2s_dibr_warp_plan_result), pl.win.rows ? 1 : 0, pl.win.cols, pl.win.margin, pl.win.WW,
                                     pl.roll0 ? 1 : 0, pl.up ? 1 : 0, pl.fx ? 1 : 0, g.oh, g.ow, g.out_h, g.out_w,
                                     {pl.grid.x, pl.grid.y, pl.grid.z}, pl.block.x, pl.lds_dynamic, pl.lds_static, {}};
    dibr_plan_name(pl, crop != nullptr, res->kernel, sizeof(res->kernel));
    return D2S_OK;
}

// The OpenXR eye views (xr_viewer/effects.py:1023-1137; the curved screen's glow: effects.py:408-474).  xr_plan (dibr_xr.h) checks
// every argument that is no device pointer and forms both eyes' tables; the launcher below looks at the pointers, then launches.
extern "C" int d2s_dibr_xr_shape(const d2s_xr_eye* eyes, int n_eyes, int batch, int alpha_mode, uint64_t* offsets, uint64_t* total) {
    D2S_REQUIRE(offsets && total, "null pointer (offsets, total)");
    D2S_REQUIRE(eyes && n_eyes >= 1 && n_eyes <= 2, "bad eyes (n_eyes must be 1 or 2)");
    D2S_REQUIRE(batch > 0 && batch <= 65535, "bad batch (1 .. 65535)");
    D2S_REQUIRE(alpha_mode >= D2S_DIBR_ALPHA_WINDOW && alpha_mode <= D2S_DIBR_ALPHA_RGBA, "bad alpha_mode");
    for (int i = 0; i < n_eyes; ++i) {
        D2S_REQUIRE(eyes[i].struct_size == sizeof(d2s_xr_eye), "d2s_xr_eye.struct_size must be sizeof(d2s_xr_eye) = 144");
        D2S_REQUIRE(eyes[i].width >= 2 && eyes[i].height >= 2 && eyes[i].width <= 8192 && eyes[i].height <= 8192, "eye image must be 2 .. 8192 on a side");
    }
    xr_out_layout(eyes, n_eyes, batch, alpha_mode, offsets, total);
    return D2S_OK;
}

static int xr_workspace_query(int kind, int n_eyes, uint64_t* bytes) {
    D2S_REQUIRE(bytes, "null pointer (bytes)");
    D2S_REQUIRE(n_eyes >= 1 && n_eyes <= 2, "n_eyes must be 1 or 2");
    *bytes = (uint64_t)n_eyes * xr_table_rows(kind) * sizeof(XrFacet);
    return D2S_OK;
}
extern "C" int d2s_dibr_xr_workspace(int n_eyes, uint64_t* bytes) { return xr_workspace_query(D2S_XR_KIND_PLAIN, n_eyes, bytes); }
extern "C" int d2s_dibr_xr_glow_curved_workspace(int n_eyes, uint64_t* bytes) { return xr_workspace_query(D2S_XR_KIND_GLOW_CURVED, n_eyes, bytes); }
extern "C" int d2s_dibr_xr_frost_workspace(int n_eyes, uint64_t* bytes) { return xr_workspace_query(D2S_XR_KIND_FROST, n_eyes, bytes); }
extern "C" int d2s_dibr_xr_frost_curved_workspace(int n_eyes, uint64_t* bytes) { return xr_workspace_query(D2S_XR_KIND_FROST_CURVED, n_eyes, bytes); }

static void xr_plan_result(const XrPlan& pl, d2s_xr_plan_result* res) {
    *res = d2s_xr_plan_result{sizeof(d2s_xr_plan_result), pl.kind, pl.rows_per_eye, pl.setup_launches, {pl.grid[0], pl.grid[1], pl.grid[2]},
                              pl.lds_dynamic, pl.lds_static, pl.pano ? 1u : 0u, pl.workspace_bytes, pl.total, {pl.offs[0], pl.offs[1]}};
}
extern "C" int d2s_dibr_xr_plan(int entry, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_glow* glow,
                                d2s_xr_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_plan_result), "d2s_xr_plan_result.struct_size must be sizeof(d2s_xr_plan_result)");
    D2S_REQUIRE(entry >= D2S_XR_ENTRY_EYES && entry <= D2S_XR_ENTRY_GLOW_CURVED, "bad entry (D2S_XR_ENTRY_*)");
    D2S_REQUIRE(entry != D2S_XR_ENTRY_EYES || !glow, "d2s_dibr_xr_eyes takes no glow: glow must be NULL with D2S_XR_ENTRY_EYES");
    XrPlan pl;
    const int rc = xr_plan(entry, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, glow, nullptr, pl);
    if (rc) return rc;
    xr_plan_result(pl, res);
    return D2S_OK;
}

// xr_launch's render launch with the panorama behind the screen: every kind (the two curved looks: d2s_dibr_xr_eyes_panorama_curved's
// plan only, xr_plan refuses them to d2s_dibr_xr_eyes_panorama).  bin: xr_launch's, the curved frost's.
static int xr_launch_pano(const XrPlan& pl, const uint8_t* rgb, const float* depth, void* out, int out_fmt, const XrFacet* tab, const uint8_t* levels,
                          const uint8_t* pano_rgb, const uint8_t* pano_levels, int bin, hipStream_t st) {
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(256);
#define DIBR_XR_PANO(FMT, D) do { \
        if (pl.kind == D2S_XR_KIND_PLAIN) hipLaunchKernelGGL((dibr_xr_kernel<FMT, D, XrPanoBg>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.P, pano_rgb, pano_levels); \
        else if (pl.kind == D2S_XR_KIND_FROST && pl.F.mode == 1) hipLaunchKernelGGL((dibr_xr_frost_kernel<FMT, D, 1, XrPanoBg>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, pl.P, pano_rgb, pano_levels); \
        else if (pl.kind == D2S_XR_KIND_FROST) hipLaunchKernelGGL((dibr_xr_frost_kernel<FMT, D, 2, XrPanoBg>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, pl.P, pano_rgb, pano_levels); \
        else if (pl.kind == D2S_XR_KIND_FROST_CURVED && pl.F.mode == 1) hipLaunchKernelGGL((dibr_xr_frost_curved_kernel<FMT, D, 1, XrPanoBg>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, bin, pl.P, pano_rgb, pano_levels); \
        else if (pl.kind == D2S_XR_KIND_FROST_CURVED) hipLaunchKernelGGL((dibr_xr_frost_curved_kernel<FMT, D, 2, XrPanoBg>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, bin, pl.P, pano_rgb, pano_levels); \
        else if (pl.kind == D2S_XR_KIND_GLOW) hipLaunchKernelGGL((dibr_xr_glow_kernel<FMT, D, XrPanoBg>), grid, block, pl.lds_dynamic, st, rgb, depth, out, tab, pl.g, pl.ex, pl.G, levels, pl.P, pano_rgb, pano_levels); \
        else hipLaunchKernelGGL((dibr_xr_glow_curved_kernel<FMT, D, XrPanoBg>), grid, block, pl.lds_dynamic, st, rgb, depth, out, tab, pl.g, pl.ex, pl.G, pl.Q, levels, pl.P, pano_rgb, pano_levels); } while (0)
    if (out_fmt == D2S_FMT_U8_HWC) { if (pl.up) DIBR_XR_PANO(D2S_FMT_U8_HWC, UpDep); else DIBR_XR_PANO(D2S_FMT_U8_HWC, FullDep); }
    else { if (pl.up) DIBR_XR_PANO(D2S_FMT_F32_HWC, UpDep); else DIBR_XR_PANO(D2S_FMT_F32_HWC, FullDep); }
#undef DIBR_XR_PANO
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

// The device pointers and the workspace, the rows' upload, the render launch.
static int xr_launch(const XrPlan& pl, const uint8_t* rgb, const float* depth, void* out, int out_fmt, void* workspace, uint64_t workspace_bytes,
                     const uint8_t* levels, void* stream, bool check_only, const uint8_t* pano_rgb = nullptr, const uint8_t* pano_levels = nullptr) {
    D2S_REQUIRE(workspace, "null pointer (workspace)");
    D2S_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    D2S_REQUIRE(workspace_bytes >= pl.workspace_bytes, (pl.kind == D2S_XR_KIND_GLOW_CURVED    ? "workspace_bytes below d2s_dibr_xr_glow_curved_workspace"
                                                        : pl.kind == D2S_XR_KIND_FROST_CURVED ? "workspace_bytes below d2s_dibr_xr_frost_curved_workspace"
                                                        : pl.kind == D2S_XR_KIND_FROST        ? "workspace_bytes below d2s_dibr_xr_frost_workspace"
                                                                                              : "workspace_bytes below d2s_dibr_xr_workspace"));
    if (pl.kind == D2S_XR_KIND_FROST || pl.kind == D2S_XR_KIND_FROST_CURVED) D2S_REQUIRE(pl.F.mode != 2 || levels, "null pointer (levels: the frosted look reads d2s_mip_chain's output)");
    else D2S_REQUIRE(pl.kind == D2S_XR_KIND_PLAIN || levels, "null pointer (levels: the glow reads d2s_mip_chain's output)");
    D2S_REQUIRE(rgb && depth && out, "null pointer");
    D2S_REQUIRE(!pl.pano || (pano_rgb && pano_levels), "null pointer (pano_rgb, pano_levels: the panorama and its d2s_mip_chain)");
    if (check_only) return D2S_OK;
    hipStream_t st = (hipStream_t)stream;
    const XrFacet* tab = (const XrFacet*)workspace;
    const int stride = xr_table_rows(pl.kind);
    for (int i = 0; i < pl.ex.n; ++i)
        for (int f0 = 0; f0 < pl.rows_per_eye; f0 += XR_CHUNK_FACETS) {
            const int nf = std::min(XR_CHUNK_FACETS, pl.rows_per_eye - f0), n_floats = nf * XR_ROW_FLOATS;
            XrFacetChunk chunk;
            for (int f = 0; f < nf; ++f) chunk.f[f] = pl.rows[i][f0 + f];
            hipLaunchKernelGGL(dibr_xr_table_kernel, dim3(cdiv(n_floats, 256)), dim3(256), 0, st, chunk, (float*)(tab + i * stride + f0), n_floats);
        }
    const char* bin_env = getenv("D2S_XR_BIN");      // "0": the binned kernel walks every row (read at the call)
    const int bin = !(bin_env && bin_env[0] == '0' && bin_env[1] == 0);
    if (pl.pano) return xr_launch_pano(pl, rgb, depth, out, out_fmt, tab, levels, pano_rgb, pano_levels, bin, st);
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(256);
#define DIBR_XR(FMT, D) do { \
        if (pl.kind == D2S_XR_KIND_PLAIN) hipLaunchKernelGGL((dibr_xr_kernel<FMT, D>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex); \
        else if (pl.kind == D2S_XR_KIND_FROST && pl.F.mode == 1) hipLaunchKernelGGL((dibr_xr_frost_kernel<FMT, D, 1>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels); \
        else if (pl.kind == D2S_XR_KIND_FROST) hipLaunchKernelGGL((dibr_xr_frost_kernel<FMT, D, 2>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels); \
        else if (pl.kind == D2S_XR_KIND_FROST_CURVED && pl.F.mode == 1) hipLaunchKernelGGL((dibr_xr_frost_curved_kernel<FMT, D, 1>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, bin); \
        else if (pl.kind == D2S_XR_KIND_FROST_CURVED) hipLaunchKernelGGL((dibr_xr_frost_curved_kernel<FMT, D, 2>), grid, block, 0, st, rgb, depth, out, tab, pl.g, pl.ex, pl.F, levels, bin); \
        else if (pl.kind == D2S_XR_KIND_GLOW) hipLaunchKernelGGL((dibr_xr_glow_kernel<FMT, D>), grid, block, pl.lds_dynamic, st, rgb, depth, out, tab, pl.g, pl.ex, pl.G, levels); \
        else hipLaunchKernelGGL((dibr_xr_glow_curved_kernel<FMT, D>), grid, block, pl.lds_dynamic, st, rgb, depth, out, tab, pl.g, pl.ex, pl.G, pl.Q, levels); } while (0)
    if (out_fmt == D2S_FMT_U8_HWC) { if (pl.up) DIBR_XR(D2S_FMT_U8_HWC, UpDep); else DIBR_XR(D2S_FMT_U8_HWC, FullDep); }
    else { if (pl.up) DIBR_XR(D2S_FMT_F32_HWC, UpDep); else DIBR_XR(D2S_FMT_F32_HWC, FullDep); }
#undef DIBR_XR
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}
int d2s::dibr_xr_entry_any(int entry, const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                           const double* crop, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt,
                           void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const d2s_xr_frost* frost,
                           const uint8_t* levels, void* stream, bool check_only, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                           const uint8_t* pano_levels) {
    XrPlan pl;
    const int rc = xr_plan(entry, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, glow, frost, pl, pano);
    return rc ? rc : xr_launch(pl, rgb, depth, out, out_fmt, workspace, workspace_bytes, levels, stream, check_only, pano_rgb, pano_levels);
}

extern "C" int d2s_dibr_xr_eyes(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                int out_fmt, void* workspace, uint64_t workspace_bytes, void* stream) {
    return dibr_xr_entry_any(D2S_XR_ENTRY_EYES, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, nullptr, nullptr, nullptr, stream, false);
}

extern "C" int d2s_dibr_xr_eyes_glow(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                     const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                     int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels,
                                     void* stream) {
    return dibr_xr_entry_any(D2S_XR_ENTRY_GLOW, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, glow, nullptr, levels, stream, false);
}

extern "C" int d2s_dibr_xr_eyes_glow_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                            const d2s_dibr_params* p, const double crop[4], const d2s_xr_screen* screen,
                                            const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt, void* workspace,
                                            uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels, void* stream) {
    return dibr_xr_entry_any(D2S_XR_ENTRY_GLOW_CURVED, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, glow, nullptr, levels, stream, false);
}

// The veil and frosted looks of the flat screen (xr_viewer/effects.py:789-857): xr_plan's fourth entry and its host-only query.
extern "C" int d2s_dibr_xr_eyes_frost(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                      const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                      int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                      void* stream) {
    return dibr_xr_entry_any(XR_ENTRY_FROST, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, nullptr, frost, levels, stream, false);
}

extern "C" int d2s_dibr_xr_frost_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                      const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_frost* frost,
                                      d2s_xr_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_plan_result), "d2s_xr_plan_result.struct_size must be sizeof(d2s_xr_plan_result)");
    XrPlan pl;
    const int rc = xr_plan(XR_ENTRY_FROST, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, nullptr, frost, pl);
    if (rc) return rc;
    xr_plan_result(pl, res);
    return D2S_OK;
}

// The veil and frosted looks of the curved screen (xr_viewer/effects.py:189-254, 759-787): xr_plan's fifth entry and its host-only query.
extern "C" int d2s_dibr_xr_eyes_frost_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                             const d2s_dibr_params* p, const double crop[4], const d2s_xr_screen* screen,
                                             const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt, void* workspace,
                                             uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels, void* stream) {
    return dibr_xr_entry_any(XR_ENTRY_FROST_CURVED, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, nullptr, frost, levels, stream, false);
}

extern "C" int d2s_dibr_xr_frost_curved_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                             const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt,
                                             const d2s_xr_frost* frost, d2s_xr_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_plan_result), "d2s_xr_plan_result.struct_size must be sizeof(d2s_xr_plan_result)");
    XrPlan pl;
    const int rc = xr_plan(XR_ENTRY_FROST_CURVED, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, nullptr, frost, pl);
    if (rc) return rc;
    xr_plan_result(pl, res);
    return D2S_OK;
}

// The panorama background behind the screen (xr_viewer/effects.py:930-1021): xr_plan's sixth entry and its host-only query.
extern "C" int d2s_dibr_xr_eyes_panorama(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                         const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                         int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                         const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                                         const uint8_t* pano_levels, void* stream) {
    return dibr_xr_entry_any(XR_ENTRY_PANORAMA, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, glow, frost, levels, stream, false, pano, pano_rgb, pano_levels);
}

extern "C" int d2s_dibr_xr_panorama_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                         const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_frost* frost,
                                         const d2s_xr_glow* glow, const d2s_xr_panorama* pano, d2s_xr_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_plan_result), "d2s_xr_plan_result.struct_size must be sizeof(d2s_xr_plan_result)");
    XrPlan pl;
    const int rc = xr_plan(XR_ENTRY_PANORAMA, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, glow, frost, pl, pano);
    if (rc) return rc;
    xr_plan_result(pl, res);
    return D2S_OK;
}

// The panorama behind every look, the curved screen's glow, veil and frosted included: xr_plan's seventh entry and its host-only
// query.  d2s_dibr_xr_eyes_panorama's argument lists; that entry keeps refusing the curved looks with a panorama.
extern "C" int d2s_dibr_xr_eyes_panorama_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                                const d2s_dibr_params* p, const double crop[4], const d2s_xr_screen* screen,
                                                const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt, void* workspace,
                                                uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                                const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                                                const uint8_t* pano_levels, void* stream) {
    return dibr_xr_entry_any(XR_ENTRY_PANORAMA_CURVED, rgb, depth, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out, out_fmt, workspace,
                             workspace_bytes, glow, frost, levels, stream, false, pano, pano_rgb, pano_levels);
}

extern "C" int d2s_dibr_xr_panorama_curved_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                                const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt,
                                                const d2s_xr_frost* frost, const d2s_xr_glow* glow, const d2s_xr_panorama* pano,
                                                d2s_xr_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_plan_result), "d2s_xr_plan_result.struct_size must be sizeof(d2s_xr_plan_result)");
    XrPlan pl;
    const int rc = xr_plan(XR_ENTRY_PANORAMA_CURVED, dh, dw, batch, H, W, p, crop, screen, eyes, n_eyes, out_fmt, glow, frost, pl, pano);
    if (rc) return rc;
    xr_plan_result(pl, res);
    return D2S_OK;
}

// The world-space panels over finished eye images (xr_viewer/overlay.py:81-249, 1427-1510; xr_viewer/effects.py:1157-1225):
// xr_panels_plan (dibr_xr.h) checks every argument that is no device pointer and forms both eyes' rows; the launcher looks at the
// pointers, writes the rows with the eye views' set-up launches and draws.
extern "C" int d2s_dibr_xr_panels_workspace(int n_eyes, uint64_t* bytes) {
    D2S_REQUIRE(bytes, "null pointer (bytes)");
    D2S_REQUIRE(n_eyes >= 1 && n_eyes <= 2, "n_eyes must be 1 or 2");
    *bytes = (uint64_t)n_eyes * XR_PANEL_ROWS * sizeof(XrFacet);
    return D2S_OK;
}

extern "C" int d2s_dibr_xr_panels_plan(int out_fmt, int batch, int alpha_mode, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes,
                                       const d2s_xr_panel* panels, int n_panels, const d2s_xr_texture* textures, int n_textures,
                                       d2s_xr_panels_plan_result* res) {
    D2S_REQUIRE(res, "null pointer (res)");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_xr_panels_plan_result), "d2s_xr_panels_plan_result.struct_size must be sizeof(d2s_xr_panels_plan_result) = 104");
    XrPanelsPlan pl;
    const int rc = xr_panels_plan(out_fmt, batch, alpha_mode, screen, eyes, n_eyes, panels, n_panels, textures, n_textures, pl);
    if (rc) return rc;
    *res = d2s_xr_panels_plan_result{};
    res->struct_size = sizeof(d2s_xr_panels_plan_result);
    res->rows_per_eye = pl.rows_per_eye; res->setup_launches = pl.setup_launches; res->render_launches = pl.render_launches;
    for (int i = 0; i < n_eyes; ++i) {
        res->drawn[i] = pl.drawn[i]; res->offsets[i] = pl.offs[i];
        for (int k = 0; k < 2; ++k) { res->tile0[i][k] = pl.P.tile0[i][k]; res->tiles[i][k] = pl.P.tiles[i][k]; }
    }
    for (int k = 0; k < 3; ++k) res->grid[k] = pl.grid[k];
    res->workspace_bytes = pl.workspace_bytes; res->out_elems = pl.total;
    return D2S_OK;
}

extern "C" int d2s_dibr_xr_panels(void* out, int out_fmt, int batch, int alpha_mode, const d2s_xr_screen* screen, const d2s_xr_eye* eyes,
                                  int n_eyes, const d2s_xr_panel* panels, int n_panels, const d2s_xr_texture* textures, int n_textures,
                                  void* workspace, uint64_t workspace_bytes, void* stream) {
    XrPanelsPlan pl;
    const int rc = xr_panels_plan(out_fmt, batch, alpha_mode, screen, eyes, n_eyes, panels, n_panels, textures, n_textures, pl);
    if (rc) return rc;
    D2S_REQUIRE(workspace, "null pointer (workspace)");
    D2S_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    D2S_REQUIRE(workspace_bytes >= pl.workspace_bytes, "workspace_bytes below d2s_dibr_xr_panels_workspace");
    D2S_REQUIRE(out, "null pointer (out)");
    for (int k = 0; k < n_panels; ++k) {
        if (panels[k].texture < 0) continue;
        const uint8_t* t = textures[panels[k].texture].rgba;
        D2S_REQUIRE(t && ((uintptr_t)t & 3) == 0, "a panel's texture needs a 4-byte aligned device pointer (rgba)");
    }
    if (!pl.render_launches) return D2S_OK;
    hipStream_t st = (hipStream_t)stream;
    const XrFacet* tab = (const XrFacet*)workspace;
    for (int i = 0; i < pl.ex.n; ++i)
        for (int f0 = 0; f0 < pl.rows_per_eye; f0 += XR_CHUNK_FACETS) {
            const int nf = std::min(XR_CHUNK_FACETS, pl.rows_per_eye - f0), n_floats = nf * XR_ROW_FLOATS;
            XrFacetChunk chunk;
            for (int f = 0; f < nf; ++f) chunk.f[f] = pl.rows[i][f0 + f];
            hipLaunchKernelGGL(dibr_xr_table_kernel, dim3(cdiv(n_floats, 256)), dim3(256), 0, st, chunk, (float*)(tab + i * XR_PANEL_ROWS + f0), n_floats);
        }
    const dim3 grid(pl.grid[0], pl.grid[1], pl.grid[2]), block(256);
    if (out_fmt == D2S_FMT_U8_HWC) hipLaunchKernelGGL((dibr_xr_panels_kernel<D2S_FMT_U8_HWC>), grid, block, 0, st, out, tab, pl.ex, pl.P);
    else hipLaunchKernelGGL((dibr_xr_panels_kernel<D2S_FMT_F32_HWC>), grid, block, 0, st, out, tab, pl.ex, pl.P);
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}
