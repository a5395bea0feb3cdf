// The viewer's composite display modes as HIP kernels: the reference's ANAGLYPH_FRAGMENT (viewer.py:678-832),
// INTERLEAVED_FRAGMENT (:835-1017), VERTICAL_INTERLEAVED_FRAGMENT (:1020-1197) and DEPTH_FRAGMENT (:633-675), each run over the
// program's viewport in window pixels exactly as the viewer draws it (:2604-2662: u_eye_offset = +ipd_uv / 2, blending off).
// These are NOT f1 with another packing: their depth shaping, edge margin (0.02), disocclusion test, in-painting use and sweep
// signs differ per program, and are restated below term for term (texture(), the samplers, push_pull_finish: dibr_tex.h).
// Line numbers in the comments are viewer.py.
#include "dibr_tex.h"
#include <algorithm>
#include <type_traits>

namespace d2s {

struct CompGeom {
    DibrGeom g;            // oh, ow = the viewport (= output) size; vpx .. vph = u_viewport = the viewport in window pixels
    int vx, vy;            // viewport origin (window pixels, y up): gl_FragCoord = (vx + col + 0.5, vy + oh - 1 - row + 0.5)
};

// push_pull_inpaint of the three warp programs: f1's phases with the program's own sweep step.
//   Interleaved (:871, 875):           sweep = vec2(c, s) * eye_dir;   uv +- sweep * pixel_size.x * float(i)
//   Anaglyph / Interleaved-V (:717-720, :1058-1062): search_dir = eye_dir > 0 ? -1 : 1;
//                                      uv +- vec2(float(search_dir * i) * pixel_size.x * c, float(search_dir * i) * pixel_size.x * s)
// (the Interleaved-V sweep therefore runs the opposite way to the Interleaved one for the same eye)
template <int MODE, class S>
__device__ void comp_push_pull(const S& smp, const DibrGeom& g, float u, float v, float cdi, float eye_dir, float out[3]) {
    float best[3] = {0.f, 0.f, 0.f}, bw = 0.f, col[3];
    const float kx = g.c * eye_dir * g.psx, ky = g.s * eye_dir * g.psx;
    const int sd = eye_dir > 0.f ? -1 : 1;
    auto step = [&](int i, float& du, float& dv) {
        if constexpr (MODE == D2S_COMPOSITE_INTERLEAVED) { du = kx * (float)i; dv = ky * (float)i; }
        else { const float t = (float)(sd * i) * g.psx; du = t * g.c; dv = t * g.s; }
    };
    for (int i = 1; i <= g.search; ++i) {                                             // phase 1
        float du, dv;
        step(i, du, dv);
        const float su = u + du, sv = v + dv;
        if (oob(su, sv)) continue;
        const float sdi = 1.0f - smp.own_depth(su, sv);
        if (sdi > cdi + g.tol) {
            smp.own_color(su, sv, col);
            const float w = g_w_phase1(g.w1[i], sdi, cdi);
            best[0] += col[0] * w; best[1] += col[1] * w; best[2] += col[2] * w;
            bw += w;
            if (bw > 5.0f) break;
        }
    }
    if (bw < 2.0f) {                                                                  // phase 2: the opposite sweep
        for (int i = 1; i <= g.search; ++i) {
            float du, dv;
            step(i, du, dv);
            const float su = u - du, sv = v - dv;
            if (oob(su, sv)) continue;
            const float sdi = 1.0f - smp.own_depth(su, sv);
            if (sdi > cdi + g.tol) {
                smp.own_color(su, sv, col);
                const float w = g.w2[i];
                best[0] += col[0] * w; best[1] += col[1] * w; best[2] += col[2] * w;
                bw += w;
            }
        }
    }
    push_pull_finish(smp, g, u, v, cdi, best, bw, out);                               // phase 3 / fallback
}

__device__ __forceinline__ float edge_falloff_002(float u) {                          // smoothstep(0, 0.02, u) * smoothstep(1, 0.98, u)
    return SMOOTHSTEP_C(0.f, 0.02f, u) * SMOOTHSTEP_C(1.f, 0.98f, u);
}

// the feathering and rounded corners every warp program applies over fuv = (gl_FragCoord.xy - u_viewport.xy) / u_viewport.zw
// (f1 takes the corner SDF over the quad's uv instead; with u_corner_radius = 0 the SDF leaves alpha as it is, so FX = false skips both)
__device__ __forceinline__ void comp_fx(const CompGeom& G, int x, int y, float col[3], float& alpha) {
    const DibrGeom& g = G.g;
    const float fx = (float)(G.vx + x) + 0.5f, fy = (float)(G.vy + g.oh - 1 - y) + 0.5f;
    const float fu = (fx - g.vpx) / g.vpw, fv = (fy - g.vpy) / g.vph;
    if (g.feather) {
        const float fw = g.feather_w;
        const float fo = smoothstepf(0.f, fw, fu) * smoothstepf(0.f, fw, 1.0f - fu) * smoothstepf(0.f, fw, fv) * smoothstepf(0.f, fw, 1.0f - fv);
        const float sh = powf(fo, 0.7f);
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] *= sh;
    }
    if (g.corner_r > 0.f) {
        const float dx = fabsf(fu - 0.5f) - 0.5f + g.corner_r, dy = fabsf(fv - 0.5f) - 0.5f + g.corner_r;
        const float mx = fmaxf(dx, 0.f), my = fmaxf(dy, 0.f);
        const float sdf = sqrtf(mx * mx + my * my) + fminf(fmaxf(dx, dy), 0.f) - g.corner_r;
        alpha = fminf(alpha, 1.0f - smoothstepf(0.f, 0.01f, sdf));
    }
}

__device__ __forceinline__ void comp_out(const DibrGeom& g, const float col[3], float alpha, float outc[4]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) outc[k] = g.alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED ? col[k] * alpha : col[k];
    outc[3] = alpha;
}

// Interleaved / Interleaved-V main() (:933-1016, :1095-1196) for one fragment whose eye is eye_dir (-1 left, +1 right).
// DEFER: return true without a result when the fragment needs the in-painting (queued for the lane-compacted second pass, which calls
// this again with DEFER = false: same expressions on the same inputs -> the same bits).
template <int MODE, bool DEFER, bool FX, class S>
__device__ __forceinline__ bool il_pixel(const S& smp, const CompGeom& G, int x, int y, float eye_dir, float outc[4]) {
    const DibrGeom& g = G.g;
    const float my_offset = eye_dir * g.half_ipd;                                     // :937
    const float parx = g.c * eye_dir, pary = g.s * eye_dir;                           // :944
    const float u = ((float)x + 0.5f) / (float)g.ow, v = ((float)y + 0.5f) / (float)g.oh;
    const float dsx = parx * g.psx * 1.5f, dsy = pary * g.psy * 1.5f;                 // :948
    const float d0 = smp.own_depth(u, v), dm = smp.own_depth(u - dsx, v - dsy), dp = smp.own_depth(u + dsx, v + dsy);
    const float d = d0 * 0.7f + dm * 0.15f + dp * 0.15f;
    const float dinv = -d;
    const float shaped = dinv * (1.0f + 0.35f * (1.0f - d));                          // :957
    const float shift = shaped + g.conv;
    const float px = my_offset * shift * g.strength * edge_falloff_002(u);            // :962-966
    const float su = u - px * g.c, sv = v - px * g.s;
    float conf;                                                                        // :970-980
    if (su < 0.f || su > 1.f || sv < 0.f || sv > 1.f) conf = 1.f;
    else {
        const float s2x = parx * g.psx * 2.0f, s2y = pary * g.psy * 2.0f;
        conf = SMOOTHSTEP_C(0.06f, 0.12f, fabsf(smp.own_depth(u - s2x, v - s2y) - smp.own_depth(u + s2x, v + s2y)));
    }
    if (DEFER && conf > 0.001f) return true;
    float col[3];
    if (conf > 0.001f) comp_push_pull<MODE>(smp, g, u, v, dinv, eye_dir, col);       // :982-987: the in-painting REPLACES the colour
    else smp.own_color(su, sv, col);
    float alpha = 1.f;                                                                // :992-993 (exactly 1 inside the frame)
    if (su < 0.001f || su > 0.999f || sv < 0.001f || sv > 0.999f) {
        const float bx = SMOOTHSTEP_C(-0.001f, 0.001f, su) * SMOOTHSTEP_C(1.001f, 0.999f, su);
        const float by = SMOOTHSTEP_C(-0.001f, 0.001f, sv) * SMOOTHSTEP_C(1.001f, 0.999f, sv);
        alpha = fminf(bx, by);
    }
    if (FX) comp_fx(G, x, y, col, alpha);                                             // :997-1015
    comp_out(g, col, alpha, outc);
    return false;
}

// Anaglyph main() (:780-831): both eyes of one fragment.  The three smoothing taps run along (c, s) for both eyes, and the two
// disocclusion taps are the same pair for both (is_disoccluded's grad_dir = (c, s) * eye_dir only swaps them, |a - b| == |b - a|):
// five depth taps per fragment, one jump test.  Of each eye's colour only the channels the output keeps are used (left R, right G
// and B): the others' conversions and lerps are dead code after inlining.
template <bool DEFER, bool FX, class S>
__device__ __forceinline__ bool ana_pixel(const S& smp, const CompGeom& G, int x, int y, float outc[4]) {
    const DibrGeom& g = G.g;
    const float u = ((float)x + 0.5f) / (float)g.ow, v = ((float)y + 0.5f) / (float)g.oh;
    const float dsx = g.c * g.psx * 1.5f, dsy = g.s * g.psy * 1.5f;                   // :785
    const float d0 = smp.own_depth(u, v), dm = smp.own_depth(u - dsx, v - dsy), dp = smp.own_depth(u + dsx, v + dsy);
    const float d = d0 * 0.7f + dm * 0.15f + dp * 0.15f;
    const float dinv = -d;
    const float sa = (dinv + g.conv) * g.strength * edge_falloff_002(u);              // :791-797 (no depth shaping)
    const float ox = g.half_ipd * sa * g.c, oy = g.half_ipd * sa * g.s;
    const float lu = u + ox, lv = v + oy, ru = u - ox, rv = v - oy;                   // :799-800
    bool occl = oob(lu, lv), occr = oob(ru, rv);                                      // is_disoccluded (:700-711), hard test
    if (!occl || !occr) {
        const float s2x = g.c * g.psx * 2.0f, s2y = g.s * g.psy * 2.0f;
        const bool jump = fabsf(smp.own_depth(u + s2x, v + s2y) - smp.own_depth(u - s2x, v - s2y)) > 0.08f;
        occl |= jump; occr |= jump;
    }
    if (DEFER && (occl || occr)) return true;
    float lc[3], rc[3];
    if (occl) comp_push_pull<D2S_COMPOSITE_ANAGLYPH>(smp, g, u, v, dinv, -1.f, lc);   // :802-810
    else smp.own_color(lu, lv, lc);
    if (occr) comp_push_pull<D2S_COMPOSITE_ANAGLYPH>(smp, g, u, v, dinv, 1.f, rc);
    else smp.own_color(ru, rv, rc);
    float col[3] = {lc[0], rc[1], rc[2]};                                             // :812
    const float blx = SMOOTHSTEP_C(0.f, 0.015f, lu) * SMOOTHSTEP_C(1.f, 0.985f, lu), bly = SMOOTHSTEP_C(0.f, 0.015f, lv) * SMOOTHSTEP_C(1.f, 0.985f, lv);
    const float brx = SMOOTHSTEP_C(0.f, 0.015f, ru) * SMOOTHSTEP_C(1.f, 0.985f, ru), bry = SMOOTHSTEP_C(0.f, 0.015f, rv) * SMOOTHSTEP_C(1.f, 0.985f, rv);
    float alpha = fminf(fminf(blx, bly), fminf(brx, bry));                            // :814-816
    if (FX) comp_fx(G, x, y, col, alpha);                                             // :818-831
    comp_out(g, col, alpha, outc);
    return false;
}

// gl_FragCoord parity -> eye (:933 / :1096: int(mod(gl_FragCoord.y | .x, 2.0)) == 0 -> -1)
template <int MODE, bool DEFER, bool FX, class S>
__device__ __forceinline__ bool comp_pixel(const S& smp, const CompGeom& G, int x, int y, float outc[4]) {
    if constexpr (MODE == D2S_COMPOSITE_ANAGLYPH) return ana_pixel<DEFER, FX>(smp, G, x, y, outc);
    else {
        const int par = MODE == D2S_COMPOSITE_INTERLEAVED ? G.vy + G.g.oh - 1 - y : G.vx + x;
        return il_pixel<MODE, DEFER, FX>(smp, G, x, y, (par & 1) ? 1.f : -1.f, outc);
    }
}

// roll == 0 (the desktop viewer): a block = COLS (256 | 512) output columns of ONE output row.  Interleaved: the row is one eye, so the eye is
// block-uniform; Interleaved-V: the eye alternates by column, but it enters only as a sign (eye_dir, search_dir), never as a branch,
// so neighbouring lanes of opposite eyes run the same instructions; Anaglyph: both eyes per lane.  As in f1's dibr_rows_kernel
// (dibr.hip), every tap but the in-painting's two vertical-blur taps reads the block's texture row pair within `margin` texels of its
// span: the window is staged in LDS once (WinSmp), and fragments that need the in-painting are queued for a second, lane-compacted pass.
// The queue is filled per wave -- one LDS atomic per wave that has queued fragments, slots by lane rank -- instead of one returning
// atomic per fragment on the same address.  COLS = 512 (two columns per thread) halves the mostly-empty second-pass waves, as
// for f1 (dibr.hip: 50.8 -> 46.8 us at 1080p Full-SBS).
// D = UpDep: the depth rows of the window are evaluated from the model-resolution map by the staging loop (dibr.hip).
template <int MODE, int OUT_FMT, bool FX, int COLS, class D = FullDep>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7)))
comp_rows_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all, CompGeom G, int margin, int WW) {
    extern __shared__ float comp_win[];                // [2][WW] depth row pair | [6][WW] R0 G0 B0 R1 G1 B1 as floats
    __shared__ int queue[COLS], qn;                    // column - xb of the fragments that need the in-painting
    const DibrGeom& g = G.g;
    const int tid = threadIdx.x, xb = blockIdx.x * COLS;
    const int y = blockIdx.y, b = blockIdx.z;
    const uint8_t* rgb = rgb_all + (long)b * g.H * g.W * 3;
    const D dep = D::make(dep_all, b, g);
    if (tid == 0) qn = 0;
    WinSmp<D> smp;
    smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
    smp.rc = row_ctx(dep, g.H, g.W, ((float)y + 0.5f) / (float)g.oh);         // block-uniform (the v the pixel functions form)
    smp.dwin = comp_win; smp.cwin = comp_win + 2 * WW; smp.WW = WW;
    smp.wx0 = (int)floorf((((float)xb + 0.5f) / (float)g.ow) * (float)g.W - 0.5f) - margin;
    for (int j = tid; j < WW; j += 256) {
        const int xs = wrapi(smp.wx0 + j, g.W);
        float da, db;
        dep.pair(smp.rc.d, xs, da, db);
        comp_win[j] = da;
        comp_win[WW + j] = db;
        const uint8_t* p0 = rgb + smp.rc.c0 + xs * 3;
        const uint8_t* p1 = rgb + smp.rc.c1 + xs * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) { comp_win[(2 + k) * WW + j] = (float)p0[k]; comp_win[(5 + k) * WW + j] = (float)p1[k]; }
    }
    __syncthreads();
    const int nch = g.alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    const long orow = ((long)b * g.oh + y) * g.ow;
    for (int cx = tid; cx < COLS; cx += 256) {          // (a block-uniform trip count: every lane reaches the ballot)
        const int x = xb + cx;
        bool defer = false;
        if (x < g.ow) {
            float c[4];
            defer = comp_pixel<MODE, true, FX>(smp, G, x, y, c);
            if (!defer) dibr_store<OUT_FMT>(out_all, (orow + x) * nch, nch, c);
        }
        const unsigned long long m = __ballot(defer);
        if (m) {
            const int lane = __lane_id(), first = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == first) base = atomicAdd(&qn, __popcll(m));
            base = __shfl(base, first);
            if (defer) queue[base + __popcll(m & ((1ull << lane) - 1ull))] = cx;
        }
    }
    __syncthreads();
    for (int q = tid; q < qn; q += 256) {
        const int px = xb + queue[q];
        float c[4];
        comp_pixel<MODE, false, FX>(smp, G, px, y, c);
        dibr_store<OUT_FMT>(out_all, (orow + px) * nch, nch, c);
    }
}

// Any roll (the OpenXR screen), or a window too wide for LDS: one thread = one fragment, every tap a global gather.
template <int MODE, int OUT_FMT, bool ROLL0, class D = FullDep>
__global__ void __launch_bounds__(256)
comp_kernel(const uint8_t* __restrict__ rgb_all, const float* __restrict__ dep_all, void* __restrict__ out_all, CompGeom G) {
    const DibrGeom& g = G.g;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= g.ow) return;
    const uint8_t* rgb = rgb_all + (long)b * g.H * g.W * 3;
    const D dep = D::make(dep_all, b, g);
    const int nch = g.alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    float c[4];
    if constexpr (ROLL0) {
        RowSmp<D> smp;
        smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
        smp.rc = row_ctx(dep, g.H, g.W, ((float)y + 0.5f) / (float)g.oh);
        comp_pixel<MODE, false, true>(smp, G, x, y, c);
    } else {
        GenSmp<D> smp;
        smp.rgb = rgb; smp.dep = dep; smp.H = g.H; smp.W = g.W;
        comp_pixel<MODE, false, true>(smp, G, x, y, c);
    }
    dibr_store<OUT_FMT>(out_all, (((long)b * g.oh + y) * g.ow + x) * nch, nch, c);
}

// DEPTH_FRAGMENT.spectral_r_ultrafast (:640-664) -> 0..255
__device__ __forceinline__ void spectral(float t, float o[3]) {
    float w1 = fmaxf(0.0f, 1.0f - fabsf(t - 0.125f) * 4.0f);
    float w2 = fmaxf(0.0f, 1.0f - fabsf(t - 0.375f) * 4.0f);
    float w3 = fmaxf(0.0f, 1.0f - fabsf(t - 0.625f) * 4.0f);
    float w4 = fmaxf(0.0f, 1.0f - fabsf(t - 0.875f) * 4.0f);
    const float total = w1 + w2 + w3 + w4;
    if (total > 0.0f) { w1 /= total; w2 /= total; w3 /= total; w4 /= total; }
    const float c1[3] = {0.0f, 0.298f, 0.651f}, c2[3] = {0.0f, 0.5f, 0.0f}, c3[3] = {1.0f, 0.851f, 0.0f}, c4[3] = {0.988f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (c1[k] * w1 + c2[k] * w2 + c3[k] * w3 + c4[k] * w4) * 255.0f;
}

// Depth Map: element-wise and byte-bound.  A thread = 4 consecutive output pixels of the flattened [batch, h, w] output: one bilinear
// depth tap each (8-byte row loads; the viewport may differ from the source), stored as one 12 / 16-byte (u8: 3 / 4 channels) or
// 48 / 64-byte (f32) vector store.  VEC = false: an output pointer not 16-byte aligned, byte / float stores.
// D = UpDep (up = the [dh, dw] map and its scales): the tap's four texels are evaluated from the model-resolution map.
struct UpArgs { int dh, dw; float sy, sx; };
template <int OUT_FMT, int NCH, bool VEC, class D = FullDep>
__global__ void __launch_bounds__(256)
depth_map_kernel(const float* __restrict__ dep_all, void* __restrict__ out_all, int H, int W, int oh, int ow, long npix, UpArgs up) {
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const long img = (long)oh * ow;
    long b = p0 / img;
    int r = (int)((p0 - b * img) / ow), c = (int)(p0 - b * img - (long)r * ow);
    float v[4][4] = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the last thread's pixels past npix would index frame b == batch, which does not exist: no taps for them (never stored)
        if (p0 + k < npix) {
            const float cu = ((float)c + 0.5f) / (float)ow, cv = ((float)r + 0.5f) / (float)oh;
            float t;
            if constexpr (std::is_same<D, UpDep>::value) t = tex_depth(UpDep{dep_all + b * up.dh * up.dw, up.dh, up.dw, up.sy, up.sx}, H, W, cu, cv);
            else t = tex_depth(dep_all + b * H * W, H, W, cu, cv);
            spectral(t, v[k]);
            v[k][3] = 1.0f;
        }
        if (++c == ow) { c = 0; if (++r == oh) { r = 0; ++b; } }
    }
    if (VEC && p0 + 4 <= npix) {
        if constexpr (OUT_FMT == D2S_FMT_U8_HWC) {
            unsigned d[NCH] = {};
#pragma unroll
            for (int i = 0; i < 4 * NCH; ++i) {
                const float x = i % NCH == 3 ? 255.0f : v[i / NCH][i % NCH];
                d[i / 4] = __builtin_amdgcn_cvt_pk_u8_f32(x, i % 4, d[i / 4]);
            }
            if constexpr (NCH == 4) *(uint4*)((uint8_t*)out_all + p0 * 4) = make_uint4(d[0], d[1], d[2], d[3]);
            else { uint3* o = (uint3*)((uint8_t*)out_all + p0 * 3); *o = make_uint3(d[0], d[1], d[2]); }
        } else {
            float4* o = (float4*)((float*)out_all + p0 * NCH);
#pragma unroll
            for (int q = 0; q < NCH; ++q)
                o[q] = make_float4(v[(4 * q) / NCH][(4 * q) % NCH], v[(4 * q + 1) / NCH][(4 * q + 1) % NCH],
                                   v[(4 * q + 2) / NCH][(4 * q + 2) % NCH], v[(4 * q + 3) / NCH][(4 * q + 3) % NCH]);
        }
        return;
    }
    for (int k = 0; k < 4 && p0 + k < npix; ++k) dibr_store<OUT_FMT>(out_all, (p0 + k) * NCH, NCH, v[k]);
}

// viewport = (x, y, w, h) in window pixels; all zeros = (0, 0, W, H).  Also every frame / viewport limit of d2s_dibr_composite, so
// that d2s_dibr_composite_shape accepts exactly what the launch accepts.
static int comp_viewport(int H, int W, const d2s_dibr_params* p, int* vx, int* vy, int* vw, int* vh) {
    const int rc = dibr_check_frame(H, W);
    if (rc) return rc;
    const float* q = p->viewport;
    if (q[0] == 0.f && q[1] == 0.f && q[2] == 0.f && q[3] == 0.f) { *vx = 0; *vy = 0; *vw = W; *vh = H; }
    else {
        for (int i = 0; i < 4; ++i)
            D2S_REQUIRE(q[i] == floorf(q[i]) && q[i] >= 0.f && q[i] <= 32768.f, "viewport (x, y, w, h) must be whole window pixels in [0, 32768]");
        D2S_REQUIRE(q[2] > 0.f && q[3] > 0.f, "viewport width / height must be positive (or the viewport all zero)");
        *vx = (int)q[0]; *vy = (int)q[1]; *vw = (int)q[2]; *vh = (int)q[3];
    }
    D2S_REQUIRE(*vh <= 65535, "viewport too tall for one launch (h <= 65535)");
    return D2S_OK;
}

int dibr_composite_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                       int composite, void* out, int out_fmt, void* stream, bool check_only);      // (also called by d2s_view_pipeline_streams, engine.hip)

}  // namespace d2s

using namespace d2s;

extern "C" int d2s_dibr_composite_shape(int H, int W, const d2s_dibr_params* p, int composite, int* out_h, int* out_w) {
    D2S_REQUIRE(p && out_h && out_w, "null pointer");
    D2S_REQUIRE(p->struct_size == sizeof(d2s_dibr_params), "d2s_dibr_params.struct_size must be sizeof(d2s_dibr_params) = 80");
    D2S_REQUIRE(composite >= D2S_COMPOSITE_ANAGLYPH && composite <= D2S_COMPOSITE_DEPTH_MAP, "bad composite (D2S_COMPOSITE_*)");
    int vx, vy, vw, vh;
    const int rc = comp_viewport(H, W, p, &vx, &vy, &vw, &vh);
    if (rc) return rc;
    *out_h = vh; *out_w = vw;
    return D2S_OK;
}

// Everything dibr_composite_any decides, stated once on the host (d2s_dibr_composite_plan reports it; tests/test_cpu_composite_f64.py
// and test_cpu_dibr_plan.py pin it): the checks of everything that is no pointer, the viewport, the uniforms, the window plan
// (512 columns per block while the window stays <= 640 texels, as f1 chooses; windows above 1536 texels -- 8 planes x 1536 floats =
// 48 KB beside the queue -- take the gather kernel), the Depth Map's store form, and from them the kernel, its grid
// and its LDS.  No HIP call.  out_align = the output address modulo 16 (only the Depth Map looks at it).
struct CompPlan {
    int composite;
    DibrWindow win;                        // (rows = false and all zero for the Depth Map)
    bool roll0, up, fx, u8, vec;           // vec: the Depth Map's 16-byte vector stores
    int nch, vw, vh;
    long npix;                             // the Depth Map's flattened output
    UpArgs ua;
    dim3 grid, block;
    unsigned lds_dynamic, lds_static;      // the row kernel's request; 0 otherwise
};
constexpr unsigned comp_rows_static_lds(int cols) { return (unsigned)(sizeof(int) * (size_t)cols + sizeof(int)); }      // queue[COLS], qn
// the kernel's name with its template arguments (formed for d2s_dibr_composite_plan only: the launch path formats nothing)
static void comp_plan_name(const CompPlan& pl, char* name, size_t n) {
    const char* fmt = pl.u8 ? "u8" : "f32";
    const char* dname = pl.up ? "UpDep" : "FullDep";
    const char* m = pl.composite == D2S_COMPOSITE_ANAGLYPH ? "ana" : pl.composite == D2S_COMPOSITE_INTERLEAVED ? "il" : "ilv";
    if (pl.composite == D2S_COMPOSITE_DEPTH_MAP) snprintf(name, n, "depth_map<%s,%d,%s,%s>", fmt, pl.nch, pl.vec ? "vec" : "scalar", dname);
    else if (pl.win.rows) snprintf(name, n, "comp_rows<%s,%s,fx=%d,%d,%s>", m, fmt, pl.fx ? 1 : 0, pl.win.cols, dname);
    else snprintf(name, n, "comp<%s,%s,%s,%s>", m, fmt, pl.roll0 ? "roll0" : "general", dname);
}
static int comp_plan_impl(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, int composite, int out_fmt,
                          unsigned out_align, CompGeom& G, CompPlan& pl) {
    D2S_REQUIRE(composite >= D2S_COMPOSITE_ANAGLYPH && composite <= D2S_COMPOSITE_DEPTH_MAP, "bad composite (D2S_COMPOSITE_*)");
    int rc = dibr_check(p, dh, dw, batch, H, W, out_fmt);
    if (rc) return rc;
    DibrGeom& g = G.g;
    rc = comp_viewport(H, W, p, &G.vx, &G.vy, &pl.vw, &pl.vh);
    if (rc) return rc;
    const int vw = pl.vw, vh = pl.vh;
    pl.composite = composite;
    pl.nch = p->alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    pl.up = dh != H || dw != W;
    pl.u8 = out_fmt == D2S_FMT_U8_HWC;
    pl.ua = UpArgs{dh, dw, linear_scale(dh, H, false), linear_scale(dw, W, false)};      // (d2s_upsample_depth's scales)
    pl.block = dim3(256);
    pl.win = DibrWindow{0, 0, 0, false};
    pl.roll0 = pl.fx = pl.vec = false;
    pl.npix = 0;
    pl.lds_dynamic = pl.lds_static = 0;
    if (composite == D2S_COMPOSITE_DEPTH_MAP) {
        pl.npix = (long)batch * vh * vw;
        D2S_REQUIRE((pl.npix + 1023L) / 1024L < (1L << 31), "output too large for one launch");      // (cdiv returns int)
        pl.grid = dim3((unsigned)cdiv(pl.npix, 1024L));
        pl.vec = (out_align & 15u) == 0;
        return D2S_OK;
    }
    dibr_fill_geom(g, p, H, W, dh, dw);
    g.oh = vh; g.ow = vw; g.mode = -1; g.out_h = vh; g.out_w = vw;
    g.vpx = (float)G.vx; g.vpy = (float)G.vy; g.vpw = (float)vw; g.vph = (float)vh;   // u_viewport
    pl.roll0 = g.s == 0.f && g.c == 1.f;
    pl.win = dibr_plan_window(g, (double)W / (double)vw, pl.roll0, 512, 640, 1536);
    pl.fx = g.feather || g.corner_r > 0.f;
    if (pl.win.rows) {
        pl.grid = dim3(cdiv(vw, pl.win.cols), vh, batch);
        pl.lds_dynamic = dibr_rows_dynamic_lds(pl.win.WW);
        pl.lds_static = comp_rows_static_lds(pl.win.cols);
        D2S_REQUIRE(pl.lds_dynamic + pl.lds_static <= DIBR_LDS_LIMIT, "internal: the window plan exceeds the LDS of a block");
    } else {
        pl.grid = dim3(cdiv(vw, 256), vh, batch);
    }
    return D2S_OK;
}

// d2s_dibr_composite (dh == H && dw == W: depth IS the texture) and d2s_dibr_composite_depth (any other [dh, dw]: the UpDep kernels).
// The decision is comp_plan_impl's; this function looks at the pointers and launches what the plan says.
int d2s::dibr_composite_any(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                            int composite, void* out, int out_fmt, void* stream, bool check_only) {
    D2S_REQUIRE(depth && p && out, "null pointer");
    D2S_REQUIRE(composite >= D2S_COMPOSITE_ANAGLYPH && composite <= D2S_COMPOSITE_DEPTH_MAP, "bad composite (D2S_COMPOSITE_*)");
    D2S_REQUIRE(rgb || composite == D2S_COMPOSITE_DEPTH_MAP, "rgb may be NULL for D2S_COMPOSITE_DEPTH_MAP only");
    CompGeom G;
    CompPlan pl;
    const int rc = comp_plan_impl(dh, dw, batch, H, W, p, composite, out_fmt, (unsigned)((uintptr_t)out & 15), G, pl);
    if (rc) return rc;
    if (check_only) return D2S_OK;
    const bool up = pl.up, roll0 = pl.roll0, fx = pl.fx, vec = pl.vec;
    const int nch = pl.nch, vw = pl.vw, vh = pl.vh;
    const dim3 grid = pl.grid, block = pl.block;
    if (composite == D2S_COMPOSITE_DEPTH_MAP) {
        const long npix = pl.npix;
        const UpArgs ua = pl.ua;
#define DM(FMT, N, V, D) hipLaunchKernelGGL((depth_map_kernel<FMT, N, V, D>), grid, block, 0, (hipStream_t)stream, depth, out, H, W, vh, vw, npix, ua)
#define DM_D(FMT, N, V) do { if (up) DM(FMT, N, V, UpDep); else DM(FMT, N, V, FullDep); } while (0)
#define DM_V(FMT, N) do { if (vec) DM_D(FMT, N, true); else DM_D(FMT, N, false); } while (0)
        if (pl.u8) { if (nch == 4) DM_V(D2S_FMT_U8_HWC, 4); else DM_V(D2S_FMT_U8_HWC, 3); }
        else { if (nch == 4) DM_V(D2S_FMT_F32_HWC, 4); else DM_V(D2S_FMT_F32_HWC, 3); }
#undef DM_V
#undef DM_D
#undef DM
        D2S_CHECK_LAUNCH();
        return D2S_OK;
    }
    if (pl.win.rows) {
        const int margin = pl.win.margin, cols = pl.win.cols, WW = pl.win.WW;
        const size_t lds = pl.lds_dynamic;
        const dim3 rgrid = grid;
#define CR_K(M, FMT, FXV, COLS, D) hipLaunchKernelGGL((comp_rows_kernel<M, FMT, FXV, COLS, D>), rgrid, block, lds, (hipStream_t)stream, rgb, depth, out, G, margin, WW)
#define CR(M, FMT, FXV, D) do { if (cols == 512) CR_K(M, FMT, FXV, 512, D); else CR_K(M, FMT, FXV, 256, D); } while (0)
#define CR_F(M, FMT) do { if (up) { if (fx) CR(M, FMT, true, UpDep); else CR(M, FMT, false, UpDep); } \
                          else if (fx) CR(M, FMT, true, FullDep); else CR(M, FMT, false, FullDep); } while (0)
#define CR_M(FMT) do { if (composite == D2S_COMPOSITE_ANAGLYPH) CR_F(D2S_COMPOSITE_ANAGLYPH, FMT); \
                       else if (composite == D2S_COMPOSITE_INTERLEAVED) CR_F(D2S_COMPOSITE_INTERLEAVED, FMT); \
                       else CR_F(D2S_COMPOSITE_INTERLEAVED_V, FMT); } while (0)
        if (pl.u8) CR_M(D2S_FMT_U8_HWC); else CR_M(D2S_FMT_F32_HWC);
#undef CR_M
#undef CR_F
#undef CR
#undef CR_K
    } else {
#define CG(M, FMT, R0, D) hipLaunchKernelGGL((comp_kernel<M, FMT, R0, D>), grid, block, 0, (hipStream_t)stream, rgb, depth, out, G)
#define CG_R(M, FMT) do { if (up) { if (roll0) CG(M, FMT, true, UpDep); else CG(M, FMT, false, UpDep); } \
                          else if (roll0) CG(M, FMT, true, FullDep); else CG(M, FMT, false, FullDep); } while (0)
#define CG_M(FMT) do { if (composite == D2S_COMPOSITE_ANAGLYPH) CG_R(D2S_COMPOSITE_ANAGLYPH, FMT); \
                       else if (composite == D2S_COMPOSITE_INTERLEAVED) CG_R(D2S_COMPOSITE_INTERLEAVED, FMT); \
                       else CG_R(D2S_COMPOSITE_INTERLEAVED_V, FMT); } while (0)
        if (pl.u8) CG_M(D2S_FMT_U8_HWC); else CG_M(D2S_FMT_F32_HWC);
#undef CG_M
#undef CG_R
#undef CG
    }
    D2S_CHECK_LAUNCH();
    return D2S_OK;
}

// What d2s_dibr_composite / d2s_dibr_composite_depth would launch: comp_plan_impl, the function the launcher takes its decision from.
static_assert(sizeof(d2s_dibr_composite_plan_result) == 132, "d2s_dibr_composite_plan_result is part of the ABI (tests/test_cpu_composite_abi.py)");
extern "C" int d2s_dibr_composite_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, int composite, int out_fmt,
                                       unsigned out_align, d2s_dibr_composite_plan_result* res) {
    D2S_REQUIRE(p && res, "null pointer");
    D2S_REQUIRE(res->struct_size == sizeof(d2s_dibr_composite_plan_result),
                "d2s_dibr_composite_plan_result.struct_size must be sizeof(d2s_dibr_composite_plan_result)");
    CompGeom G;
    CompPlan pl;
    const int rc = comp_plan_impl(dh, dw, batch, H, W, p, composite, out_fmt, out_align, G, pl);
    if (rc) return rc;
    *res = d2s_dibr_composite_plan_result{sizeof(d2s_dibr_composite_plan_result), pl.win.rows ? 1 : 0, pl.win.cols, pl.win.margin, pl.win.WW,
                                          pl.roll0 ? 1 : 0, pl.up ? 1 : 0, pl.fx ? 1 : 0, pl.vec ? 1 : 0, pl.vh, pl.vw,
                                          {pl.grid.x, pl.grid.y, pl.grid.z}, pl.block.x, pl.lds_dynamic, pl.lds_static, {}};
    comp_plan_name(pl, res->kernel, sizeof(res->kernel));
    return D2S_OK;
}

extern "C" int d2s_dibr_composite(const uint8_t* rgb, const float* depth, int batch, int H, int W, const d2s_dibr_params* p,
                                  int composite, void* out, int out_fmt, void* stream) {
    return dibr_composite_any(rgb, depth, H, W, batch, H, W, p, composite, out, out_fmt, stream, false);
}

extern "C" int d2s_dibr_composite_depth(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                        const d2s_dibr_params* p, int composite, void* out, int out_fmt, void* stream) {
    return dibr_composite_any(rgb, depth, dh, dw, batch, H, W, p, composite, out, out_fmt, stream, false);
}
