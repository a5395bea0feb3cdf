// d2s_dibr_xr_eyes, host side: the OpenXR screen as planar facets and, per eye, the facet table the render kernel searches
// (DESIGN.md 3.4).  Everything here is double precision; the table is rounded to float once, at the end.  References:
// _build_model_mat4 (xr_viewer/screen.py:29-70), _build_curved_screen_verts (screen.py:110-173), _screen_effect_basis
// (xr_viewer/effects.py:65-82), _CURVED_HALF_ANGLE_RAD (xr_viewer/constants.py:50-51), _render_eye (effects.py:1023-1137).
#pragma once
#include "dibr_pano.h"
#include "dibr_tex.h"
#include "mip.h"
#include <cmath>

namespace d2s {

constexpr int XR_MAX_FACETS = 48;                 // the strip's N (effects.py:1116: n_verts = (48 + 1) * 2)
constexpr double XR_HALF_ANGLE = 0.6 * 0.8;       // _CURVED_HALF_ANGLE_RAD = 0.6 * _CURVED_CURVATURE_SCALE

// One planar facet of one eye, over the pixel centre RELATIVE TO THE IMAGE CENTRE (xc, yc) = (x + 0.5 - w / 2, y + 0.5 - h / 2), y down:
//   (na, nb, nw) = (ha, hb, hw) . (xc, yc, 1);  nw = 1 / clip w > 0;  the facet's own coordinates a = na / nw, b = nb / nw in 0..1;
//   covered <=> 0 <= na <= nw and 0 <= nb <= nw;  depth (NDC z, what GL_LESS compares) = hz . (xc, yc, 1);
//   uv (GL's, v up) = (u0 + a * ua + b * ub, v0 + a * va + b * vb): the vertex uvs are affine over a facet.
//   he = the upper a-edge, hw - ha, as a row of its own: covered <=> na >= 0, he . (xc, yc, 1) >= 0, 0 <= nb <= nw.  Along the strip facet
//   f's he is the exact NEGATION of facet f + 1's float32 ha row -- one edge function per interior seam, evaluated by both sides with the
//   same operations (no contraction in this file's kernels), so -x >= 0 or x >= 0 always holds: the strip is watertight, as GL's is.
struct XrFacet { float ha[3], hb[3], hw[3], hz[3], he[3]; float u0, ua, ub, v0, va, vb, pad[3]; };
static_assert(sizeof(XrFacet) == 96, "XrFacet is 24 floats");
constexpr int XR_CHUNK_FACETS = 24;
struct XrFacetChunk { XrFacet f[XR_CHUNK_FACETS]; };    // 2 304 bytes: a set-up launch carries half an eye's table in its arguments

struct XrVert { double p[3], u, v; };
// The surface as facets: corner (a, b) = (0, 0), (1, 0), (0, 1); the fourth corner is p10 + p01 - p00 (flat: the model matrix is
// affine; curved: two generator lines of a cylinder).  all[]: every vertex GL would transform (the clip-w refusal looks at each).
struct XrSurface { int n; XrVert p00[XR_MAX_FACETS], p10[XR_MAX_FACETS], p01[XR_MAX_FACETS]; int n_all; XrVert all[2 * (XR_MAX_FACETS + 1)]; };

inline void xr_basis(const d2s_xr_screen* s, double R[3][3], double centre[3]) {
    const double cy = cos(s->yaw), sy = sin(s->yaw), cp = cos(s->pitch), sp = sin(s->pitch), cr = cos(s->roll), sr = sin(s->roll);
    const double r[3][3] = {{cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, sy * cp},
                            {cp * sr, cp * cr, -sp},
                            {-sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, cy * cp}};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = r[i][j];
    centre[0] = s->pan_x; centre[1] = s->pan_y; centre[2] = -s->distance;
}

inline void xr_surface(const d2s_xr_screen* s, XrSurface& S) {
    double R[3][3], c[3];
    xr_basis(s, R, c);
    auto world = [&](double lx, double ly, double lz, double u, double v) {
        XrVert w;
        for (int i = 0; i < 3; ++i) w.p[i] = c[i] + R[i][0] * lx + R[i][1] * ly + R[i][2] * lz + R[i][2] * s->normal_offset;
        w.u = u; w.v = v;
        return w;
    };
    const double hw = s->width / 2.0, hh = s->height / 2.0;
    if (s->curve == D2S_XR_CURVE_FLAT) {                   // T @ R @ S applied to (+-1, +-1, 0, 1), uv as quad_vao has them
        S.n = 1; S.n_all = 4;
        S.all[0] = world(-hw, -hh, 0, 0, 0); S.all[1] = world(hw, -hh, 0, 1, 0); S.all[2] = world(-hw, hh, 0, 0, 1); S.all[3] = world(hw, hh, 0, 1, 1);
        S.p00[0] = S.all[0]; S.p10[0] = S.all[1]; S.p01[0] = S.all[2];
        return;
    }
    const int N = XR_MAX_FACETS;
    const bool vert = s->curve == D2S_XR_CURVE_VERTICAL;
    const double radius = (vert ? hh : hw) / XR_HALF_ANGLE, step = 2.0 * XR_HALF_ANGLE / N;
    S.n = N; S.n_all = 2 * (N + 1);
    for (int i = 0; i <= N; ++i) {                         // column pair i of the strip; the vertex uv is the float32 the strip stores
        const double ang = i == N ? XR_HALF_ANGLE : -XR_HALF_ANGLE + i * step, t = (double)(float)((double)i / N);
        const double along = radius * sin(ang), lz = radius * (1.0 - cos(ang));
        S.all[2 * i] = vert ? world(-hw, along, lz, 0, t) : world(along, -hh, lz, t, 0);
        S.all[2 * i + 1] = vert ? world(hw, along, lz, 1, t) : world(along, hh, lz, t, 1);
    }
    for (int i = 0; i < N; ++i) {
        S.p00[i] = S.all[2 * i];
        S.p10[i] = S.all[2 * i + 2];                       // a runs ALONG the strip for both curves (xr_facets: the shared seams),
        S.p01[i] = S.all[2 * i + 1];                       // b across it; the uv affine says which of u, v each one moves
    }
}

inline void xr_clip(const double vp[16], const double p[3], double w1, double out[4]) {
    for (int r = 0; r < 4; ++r) out[r] = vp[4 * r] * p[0] + vp[4 * r + 1] * p[1] + vp[4 * r + 2] * p[2] + vp[4 * r + 3] * w1;
}
// smallest clip w over the surface's vertices
inline double xr_min_w(const XrSurface& S, const double vp[16]) {
    double m = INFINITY;
    for (int i = 0; i < S.n_all; ++i) { double c[4]; xr_clip(vp, S.all[i].p, 1.0, c); m = c[3] < m ? c[3] : m; }
    return m;
}
// One eye's table.  clip(a, b) = C0 + a * CA + b * CB; with D = diag(w / 2, -h / 2, 1): (xc, yc, 1) * clip.w = D * M * (a, b, 1),
// M = [CA.xyw | CB.xyw | C0.xyw], so (a, b, 1) / clip.w = inverse(D * M) * (xc, yc, 1).  A facet seen edge-on (no inverse) covers no
// pixel centre: its ha row becomes the constant -1.
// tri: the row is a triangle (the curved frost's), he = hw - ha - hb, the edge p10 - p01
inline void xr_facet_row(const XrVert& p00, const XrVert& p10, const XrVert& p01, const double vp[16], int w, int h, XrFacet& F, bool tri = false) {
    double dA[3], dB[3], C0[4], CA[4], CB[4];
    for (int i = 0; i < 3; ++i) { dA[i] = p10.p[i] - p00.p[i]; dB[i] = p01.p[i] - p00.p[i]; }
    xr_clip(vp, p00.p, 1.0, C0); xr_clip(vp, dA, 0.0, CA); xr_clip(vp, dB, 0.0, CB);
    const double sx = w / 2.0, sy = -h / 2.0;
    const double m[3][3] = {{sx * CA[0], sx * CB[0], sx * C0[0]}, {sy * CA[1], sy * CB[1], sy * C0[1]}, {CA[3], CB[3], C0[3]}};
    double adj[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
        adj[i][j] = m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0];
    }
    const double det = m[0][0] * adj[0][0] + m[0][1] * adj[1][0] + m[0][2] * adj[2][0];
    double scale = 0.0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) scale = fmax(scale, fabs(m[i][j]));
    F = XrFacet{};
    if (!(fabs(det) > 1e-14 * scale * scale * scale)) { F.ha[2] = -1.f; return; }
    double inv[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) inv[i][j] = adj[i][j] / det;
    for (int j = 0; j < 3; ++j) {
        F.ha[j] = (float)inv[0][j]; F.hb[j] = (float)inv[1][j]; F.hw[j] = (float)inv[2][j];
        F.hz[j] = (float)(CA[2] * inv[0][j] + CB[2] * inv[1][j] + C0[2] * inv[2][j]);
        F.he[j] = tri ? (float)(inv[2][j] - inv[0][j] - inv[1][j]) : (float)(inv[2][j] - inv[0][j]);
    }
    F.u0 = (float)p00.u; F.ua = (float)(p10.u - p00.u); F.ub = (float)(p01.u - p00.u);
    F.v0 = (float)p00.v; F.va = (float)(p10.v - p00.v); F.vb = (float)(p01.v - p00.v);
}
inline void xr_facets(const XrSurface& S, const double vp[16], int w, int h, XrFacet* out) {
    for (int f = 0; f < S.n; ++f) xr_facet_row(S.p00[f], S.p10[f], S.p01[f], vp, w, h, out[f]);
    // interior seams: facet f ends where facet f + 1 begins (a runs along the strip) -- one edge function for both
    auto live = [&](int f) { return !(out[f].ha[0] == 0.f && out[f].ha[1] == 0.f && out[f].ha[2] == -1.f); };
    for (int f = 0; f + 1 < S.n; ++f)
        if (live(f) && live(f + 1))
            for (int j = 0; j < 3; ++j) out[f].he[j] = -out[f + 1].ha[j];
}

inline bool xr_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// What d2s_dibr_xr_eyes refuses about the screen and the eyes, in the header's order (xr_plan; the workspace is the launcher's).
inline int xr_screen_check(const d2s_xr_screen* s, const d2s_xr_eye* eyes, int n_eyes, int batch) {
    D2S_REQUIRE(s && eyes, "null pointer (screen, eyes)");
    D2S_REQUIRE(s->struct_size == sizeof(d2s_xr_screen), "d2s_xr_screen.struct_size must be sizeof(d2s_xr_screen) = 96");
    D2S_REQUIRE(n_eyes >= 1 && n_eyes <= 2, "n_eyes must be 1 or 2");
    D2S_REQUIRE(s->curve >= D2S_XR_CURVE_FLAT && s->curve <= D2S_XR_CURVE_VERTICAL, "bad curve (0 flat, 1 horizontal, 2 vertical)");
    const double geo[9] = {s->width, s->height, s->distance, s->pan_x, s->pan_y, s->yaw, s->pitch, s->roll, s->normal_offset};
    D2S_REQUIRE(xr_finite(geo, 9) && std::isfinite(s->clear[0]) && std::isfinite(s->clear[1]) && std::isfinite(s->clear[2]) &&
                std::isfinite(s->clear[3]), "the screen must be finite");
    D2S_REQUIRE(s->width > 0.0 && s->height > 0.0 && s->distance > 0.0, "screen width, height and distance must be > 0");
    for (int i = 0; i < n_eyes; ++i) {
        D2S_REQUIRE(eyes[i].struct_size == sizeof(d2s_xr_eye), "d2s_xr_eye.struct_size must be sizeof(d2s_xr_eye) = 144");
        D2S_REQUIRE(xr_finite(eyes[i].vp, 16), "eye vp must be finite");
        D2S_REQUIRE(eyes[i].width >= 2 && eyes[i].height >= 2 && eyes[i].width <= 8192 && eyes[i].height <= 8192, "eye image must be 2 .. 8192 on a side");
        D2S_REQUIRE(eyes[i].eye == 0 || eyes[i].eye == 1, "eye must be 0 (left) or 1 (right)");
    }
    D2S_REQUIRE((long)n_eyes * batch <= 65535, "n_eyes * batch too large for one launch");
    return D2S_OK;
}
// The eye images one after another in out: eye i is [batch][height_i][width_i][nch] at offsets[i] (d2s_dibr_xr_shape, xr_plan)
inline void xr_out_layout(const d2s_xr_eye* eyes, int n_eyes, int batch, int alpha_mode, uint64_t* offsets, uint64_t* total) {
    const uint64_t nch = alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    uint64_t at = 0;
    for (int i = 0; i < n_eyes; ++i) {
        offsets[i] = at;
        at += (uint64_t)batch * eyes[i].height * eyes[i].width * nch;
    }
    *total = at;
}

// ---- the glow around the flat screen (d2s_dibr_xr_eyes_glow; _render_glow, xr_viewer/effects.py:476-585) ----
constexpr int XR_GLOW_LOD = 7;                    // GLOW_SOURCE_LOD (xr_viewer/glsl.py:595): the glow reads LOD 7 .. 10
// The uniforms _render_glow sets, rounded to float once, and the part of the mip chain the kernel keeps in LDS.  The glow quad lies in
// the screen's plane, so with (a, b) the screen facet's own coordinates its uv is 0.5 + ((a, b) - 0.5) * (inner_w, inner_h).
struct XrGlowDev {
    int mode;                                     // 1 glow, 2 glow2
    float half_x, half_y;                         // u_screen_half
    float inner_w, inner_h;
    float inv_range, inner;                       // u_glow_inv_range, u_glow_inner
    int m, q, n_tex;                              // levels m = min(7, q) .. q are staged: n_tex texels, 12 bytes each (<= 5461: 64 KB)
    uint32_t chain_off, chain_total;              // level m's byte offset within a frame's chain; the chain's bytes per frame
};

// What d2s_dibr_xr_eyes_glow refuses about the glow, after xr_screen_check has accepted the screen (levels, a device pointer, is the
// launcher's).  curved_ok: the asking entry draws the curved screen's glow.
inline int xr_glow_check(const d2s_xr_screen* s, const d2s_xr_glow* glow, bool curved_ok) {
    if (!glow) return D2S_OK;
    D2S_REQUIRE(glow->struct_size == sizeof(d2s_xr_glow), "d2s_xr_glow.struct_size must be sizeof(d2s_xr_glow) = 24");
    D2S_REQUIRE(glow->mode >= 0 && glow->mode <= 2, "bad glow mode (0 off, 1 glow, 2 glow2)");
    if (glow->mode == 0) return D2S_OK;
    D2S_REQUIRE(std::isfinite(glow->range_m) && glow->range_m > 0.0, "glow range_m must be finite and > 0");
    D2S_REQUIRE(std::isfinite(glow->inner_edge_fraction) && glow->inner_edge_fraction >= 0.0, "glow inner_edge_fraction must be finite and >= 0");
    if (s->curve != D2S_XR_CURVE_FLAT && !curved_ok) {
        set_error("unsupported: the glow of a curved screen (a band mesh in the reference) is not built; curve must be 0 with glow on");
        return D2S_E_UNSUPPORTED;
    }
    D2S_REQUIRE(s->normal_offset == 0.0, "normal_offset must be 0 with glow on (the reference offsets the screen only under a room model, which has no planar glow)");
    return D2S_OK;
}

// _render_glow:486-495 and _render_curved_glow:414-423 in double precision: the glow quad's extents.  inner_uv: mode 1's; glow2 has
// no inner band.
struct XrGlowExtents { double uv_range, inner_w, inner_h, inner_uv; };
inline XrGlowExtents xr_glow_extents(const d2s_xr_screen* s, const d2s_xr_glow* glow) {
    double range = fmax(glow->range_m, 1e-4);
    if (glow->mode == 2) range *= 0.5;
    const double glow_w = s->width + 2.0 * range, glow_h = s->height + 2.0 * range;
    XrGlowExtents x;
    x.uv_range = range / fmax(glow_w, glow_h); x.inner_w = s->width / glow_w; x.inner_h = s->height / glow_h;
    x.inner_uv = fmin(x.inner_w, x.inner_h) * fmax(glow->inner_edge_fraction, 0.0);
    return x;
}
// H x W: the frame the chain was built from
inline void xr_glow_dev(const XrGlowExtents& x, int mode, int H, int W, XrGlowDev& G) {
    G = XrGlowDev{};
    G.mode = mode;
    G.half_x = (float)(x.inner_w * 0.5); G.half_y = (float)(x.inner_h * 0.5);
    G.inner_w = (float)x.inner_w; G.inner_h = (float)x.inner_h;
    G.inv_range = (float)(1.0 / fmax(x.uv_range, 1e-6)); G.inner = (float)(mode == 2 ? 0.0 : x.inner_uv);
    MipShape ms;
    mip_shape(H, W, ms);
    G.q = ms.q; G.m = ms.q < XR_GLOW_LOD ? ms.q : XR_GLOW_LOD;
    G.chain_off = ms.off[G.m]; G.chain_total = ms.total;
    for (int k = G.m; k <= ms.q; ++k) G.n_tex += ms.h[k] * ms.w[k];
}

// ---- the glow around the curved screen (d2s_dibr_xr_eyes_glow_curved; _render_curved_glow, _build_curved_glow_band_verts,
// xr_viewer/effects.py:314-474) ----
// The band mesh as planar pieces.  With "along" the strip's direction (u of a horizontal curve, v of a vertical one)
// and "across" the other one:
//   0 .. 47  the strip's facets, each continued without bound across the strip (the outer bands beside the arc; the inner bands that
//            run along it lie on them);
//   48, 49   the tangent planes at the arc's two ends (_local_axes at -+0.48 rad; the outer band beyond an end, its two corners
//            included): origin = the end's generator, a = metres along the tangent / the screen's length, b across as a facet's;
//   50, 51   mode 1: the chord planes between an end and the strip coordinate e_al = inner_uv / inner_(w | h) (the inner band at that
//            end, ONE quad along the strip in the mesh), a = 0 at the lower strip coordinate, 1 at the upper.
// Every row carries the affine map from its own (a, b) to the screen's coordinates (ga, gb) -- what glow_frag takes -- in the uv
// fields; a facet's is its vertex uv.  The 49 seams (47 interior ones and the arc's two ends) are the facets' own float32 rows: seam
// s < 48 = facet s's ha, seam 48 = facet 47's he negated, so a tangent piece and the end facet beside it share ONE edge function.
constexpr int XR_PIECES = 52, XR_T0 = 48, XR_T1 = 49, XR_C0 = 50, XR_C1 = 51, XR_SEAMS = 49;
constexpr int XR_ROW_FLOATS = sizeof(XrFacet) / sizeof(float);
// vertical: the strip runs along v.  e_al, e_ac: the inner band's width in screen coordinates along / across the strip (each <= 0.5)
struct XrCurvedDev { int vertical; float e_al, e_ac; };
struct XrCurvedPieces { XrVert p00[4], p10[4], p01[4]; double axis[3], radius; };      // pieces 48 .. 51; a point of the cylinder's axis

// _build_curved_glow_band_verts:381-388: u0i - u0 = min(inner_uv, inner_w / 2) in glow uv, / inner_w in the screen's
inline void xr_curved_dev(const d2s_xr_screen* s, const XrGlowExtents& x, XrCurvedDev& Q, double* e_al_out) {
    const double eu = fmin(0.5, x.inner_uv / x.inner_w), ev = fmin(0.5, x.inner_uv / x.inner_h);
    Q.vertical = s->curve == D2S_XR_CURVE_VERTICAL;
    Q.e_al = (float)(Q.vertical ? ev : eu); Q.e_ac = (float)(Q.vertical ? eu : ev);
    *e_al_out = Q.vertical ? ev : eu;
}

inline void xr_curved_pieces(const d2s_xr_screen* s, double e_al, XrCurvedPieces& P) {
    double R[3][3], c[3];
    xr_basis(s, R, c);
    const bool vert = s->curve == D2S_XR_CURVE_VERTICAL;
    const double len = vert ? s->height : s->width, wid = vert ? s->width : s->height, radius = len / 2.0 / XR_HALF_ANGLE;
    // local (along, across, towards the viewer) -> world; uv likewise (along, across)
    auto make = [&](double al, double ac, double lz, double t_al, double t_ac, bool dir) {
        const double lx = vert ? ac : al, ly = vert ? al : ac;
        XrVert w;
        for (int i = 0; i < 3; ++i) w.p[i] = (dir ? 0.0 : c[i]) + R[i][0] * lx + R[i][1] * ly + R[i][2] * lz;
        w.u = vert ? t_ac : t_al; w.v = vert ? t_al : t_ac;
        return w;
    };
    auto arc = [&](double t, double ac) {
        const double ang = -XR_HALF_ANGLE + 2.0 * XR_HALF_ANGLE * t;
        return make(radius * sin(ang), (ac - 0.5) * wid, radius * (1.0 - cos(ang)), t, ac, false);
    };
    auto plus = [&](const XrVert& a, const XrVert& d) {
        XrVert w;
        for (int i = 0; i < 3; ++i) w.p[i] = a.p[i] + d.p[i];
        w.u = a.u + d.u; w.v = a.v + d.v;
        return w;
    };
    for (int k = 0; k < 2; ++k) {                          // the tangent planes
        const double ang = k ? XR_HALF_ANGLE : -XR_HALF_ANGLE;
        P.p00[k] = arc((double)k, 0.0);
        P.p10[k] = plus(P.p00[k], make(cos(ang) * len, 0.0, sin(ang) * len, 1.0, 0.0, true));
        P.p01[k] = arc((double)k, 1.0);
    }
    P.p00[2] = arc(0.0, 0.0); P.p10[2] = arc(e_al, 0.0); P.p01[2] = arc(0.0, 1.0);
    P.p00[3] = arc(1.0 - e_al, 0.0); P.p10[3] = arc(1.0, 0.0); P.p01[3] = arc(1.0 - e_al, 1.0);
    const XrVert ax = make(0.0, 0.0, radius, 0.0, 0.0, false);
    for (int i = 0; i < 3; ++i) P.axis[i] = ax.p[i];
    P.radius = radius;
}

// The eye's position: the null space of vp's x, y and w rows (every point of clip x = y = w = 0).  false: no finite one.
inline bool xr_eye_pos(const double vp[16], double e[3]) {
    const double* r[3] = {vp, vp + 4, vp + 12};
    double h[4];
    for (int k = 0; k < 4; ++k) {
        int c[3], n = 0;
        for (int j = 0; j < 4; ++j) if (j != k) c[n++] = j;
        const double d = r[0][c[0]] * (r[1][c[1]] * r[2][c[2]] - r[1][c[2]] * r[2][c[1]])
                       - r[0][c[1]] * (r[1][c[0]] * r[2][c[2]] - r[1][c[2]] * r[2][c[0]])
                       + r[0][c[2]] * (r[1][c[0]] * r[2][c[1]] - r[1][c[1]] * r[2][c[0]]);
        h[k] = (k & 1) ? -d : d;
    }
    const double m = fmax(fmax(fabs(h[0]), fabs(h[1])), fabs(h[2]));
    if (!(fabs(h[3]) > 1e-12 * m) || !(fabs(h[3]) > 0.0)) return false;
    for (int i = 0; i < 3; ++i) e[i] = h[i] / h[3];
    return xr_finite(e, 3);
}
// The arc and its two tangent rays bound, extruded, a convex region that opens towards the viewer.  true: the eye lies on the inner
// side of all 50 outer piece planes (the side of the cylinder's axis) by more than 1e-4 of the radius: then every ray from it meets
// the surface at most once, and the seams order the pieces monotonically across the image.
inline bool xr_eye_inside(const XrSurface& S, const XrCurvedPieces& P, const double vp[16]) {
    double e[3];
    if (!xr_eye_pos(vp, e)) return false;
    for (int k = 0; k < XR_MAX_FACETS + 2; ++k) {
        const XrVert& a = k < XR_MAX_FACETS ? S.p00[k] : P.p00[k - XR_MAX_FACETS];
        const XrVert& b = k < XR_MAX_FACETS ? S.p10[k] : P.p10[k - XR_MAX_FACETS];
        const XrVert& d = k < XR_MAX_FACETS ? S.p01[k] : P.p01[k - XR_MAX_FACETS];
        double dA[3], dB[3];
        for (int i = 0; i < 3; ++i) { dA[i] = b.p[i] - a.p[i]; dB[i] = d.p[i] - a.p[i]; }
        const double n[3] = {dA[1] * dB[2] - dA[2] * dB[1], dA[2] * dB[0] - dA[0] * dB[2], dA[0] * dB[1] - dA[1] * dB[0]};
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        double de = 0.0, da = 0.0;
        for (int i = 0; i < 3; ++i) { de += n[i] * (e[i] - a.p[i]); da += n[i] * (P.axis[i] - a.p[i]); }
        if (!((da < 0.0 ? -de : de) > 1e-4 * P.radius * nn)) return false;
    }
    return true;
}
// One eye's 52 rows: the facets exactly as xr_facets forms them, then the tangent and chord pieces (mode 2: the chord rows cover nothing).
inline void xr_curved_table(const XrSurface& S, const XrCurvedPieces& P, int mode, const double vp[16], int w, int h, XrFacet* out) {
    xr_facets(S, vp, w, h, out);
    for (int k = 0; k < 4; ++k) {
        if (k >= 2 && mode != 1) { out[XR_T0 + k] = XrFacet{}; out[XR_T0 + k].ha[2] = -1.f; continue; }
        xr_facet_row(P.p00[k], P.p10[k], P.p01[k], vp, w, h, out[XR_T0 + k]);
    }
}

// ---- the veil and frosted looks of the flat screen (d2s_dibr_xr_eyes_frost; _render_flat_frost_with_uniforms, _frost_front_layout,
// _build_flat_frost_verts, xr_viewer/effects.py:102-187, 789-857) ----
// Four planar walls in the screen's local frame (x, y in half-sizes, z in front_depth), from a screen edge (t = 0) to the matching edge
// of the front rectangle (t = 1): a mesh vertex is (px * (1 + t * (fx - 1)), py * (1 + t * (fy - 1)), t).  Wall k's row is an XrFacet
// whose own coordinates are a = the local coordinate along the edge, signed so that it grows with the mesh's s (x for top and bottom,
// -y for left and right), and b = t: origin the edge's midpoint, p10 = one half-size along the edge, p01 = the front edge's midpoint.
// ha, hb, hw, hz are as a facet's; he is not read.  The uv fields carry what the mesh walk needs instead of an affine map:
//   u0 = k, the slope of g(t) = 1 + k * t (k = fx - 1 for top and bottom, fy - 1 for left and right): column line j of the 8 x 8 grid
//        is a = (j / 4 - 1) * g(t);   ua = 0: s is v_uv.x, 1: s is v_uv.y;   ub = the other, constant component of v_uv (0 or 1).
constexpr int XR_WALLS = 4, XR_FROST_GRID = 8;          // _FLAT_FROST_N = _FLAT_FROST_M = 8 (effects.py:140-141)
constexpr int XR_ENTRY_FROST = 3;                        // xr_plan's fourth entry: d2s_dibr_xr_eyes_frost (d2s_dibr_xr_plan knows 0..2)
// The uniforms the two setters hand GL (effects.py:651-718), rounded to float once, and the two chain levels textureLod(u_lod) mixes
struct XrFrostDev {
    int mode;                                     // 1 veil, 2 frosted
    float inset, intensity, alpha, softness, thickness;
    float threshold, noise_scale, blend, diffuse, tx, ty;      // (tx, ty) = u_time * (0.011, -0.007)
    int l0, l1;                                   // floor(lambda) and the next level, lambda = clamp(max(u_lod, 0), 0, q); level 0 is the frame
    float lf;                                     // lambda - l0
    int w0, h0, w1, h1;
    uint32_t off0, off1, chain_total;             // byte offsets within a frame's chain (unused for level 0)
};
struct XrFrostLayout { double front_depth, front_half_w, front_half_h, fx, fy; };

inline bool xr_frost_on(const d2s_xr_frost* f) {      // the reference's early returns (effects.py:822-857); NaN was refused before
    return f && f->mode != 0 && f->intensity > 0.0 && !(f->mode == 1 && f->alpha <= 0.002);
}
// What d2s_dibr_xr_eyes_frost refuses about the frost, after xr_screen_check has accepted the screen.  curved_ok: the asking entry
// (d2s_dibr_xr_eyes_frost_curved) draws the curved screen's walls.
inline int xr_frost_check(const d2s_xr_screen* s, const d2s_xr_frost* f, bool curved_ok) {
    if (!f) return D2S_OK;
    D2S_REQUIRE(f->struct_size == sizeof(d2s_xr_frost), "d2s_xr_frost.struct_size must be sizeof(d2s_xr_frost) = 120");
    D2S_REQUIRE(f->mode >= 0 && f->mode <= 2, "bad frost mode (0 off, 1 veil, 2 frosted)");
    if (f->mode == 0) return D2S_OK;
    const double v[14] = {f->head[0], f->head[1], f->head[2], f->intensity, f->alpha, f->edge_inset, f->beam_softness, f->beam_thickness,
                          f->lod, f->threshold, f->noise_scale, f->blend, f->diffuse, f->time};
    D2S_REQUIRE(xr_finite(v, 14), "the frost's fields must be finite");
    D2S_REQUIRE(f->noise_scale >= 0.0 && f->lod >= 0.0, "frost noise_scale and lod must be >= 0");
    if (!xr_frost_on(f)) return D2S_OK;
    if (s->curve != D2S_XR_CURVE_FLAT && !curved_ok) {
        set_error("unsupported: the frost and veil of a curved screen (a mesh of its own in the reference, _build_curved_frost_verts) "
                  "are not built; curve must be 0 with frost on");
        return D2S_E_UNSUPPORTED;
    }
    D2S_REQUIRE(s->normal_offset == 0.0, "normal_offset must be 0 with frost on (the walls start at the screen's own plane)");
    return D2S_OK;
}
// _frost_front_layout:120-128 and _build_flat_frost_verts:146-149 in double precision
inline XrFrostLayout xr_frost_layout(const d2s_xr_screen* s, const d2s_xr_frost* f) {
    double R[3][3], c[3], hl[3];
    xr_basis(s, R, c);
    for (int j = 0; j < 3; ++j) hl[j] = R[0][j] * (f->head[0] - c[0]) + R[1][j] * (f->head[1] - c[1]) + R[2][j] * (f->head[2] - c[2]);
    XrFrostLayout L;
    L.front_depth = fmax(fmax(hl[2] + 0.55, s->distance + 0.35), 0.75);
    L.front_half_w = fmax(fmax(s->width * 0.5, fabs(hl[0]) + 0.65), 0.65);
    L.front_half_h = fmax(fmax(s->height * 0.5, fabs(hl[1]) + 0.65), 0.65);
    L.fx = L.front_half_w / fmax(s->width * 0.5, 1e-6); L.fy = L.front_half_h / fmax(s->height * 0.5, 1e-6);
    return L;
}
// One eye's four wall rows, in draw order: top, bottom, left, right (_build_flat_frost_verts:179-186)
inline void xr_frost_walls(const d2s_xr_screen* s, const XrFrostLayout& L, const double vp[16], int w, int h, XrFacet* out) {
    double R[3][3], c[3];
    xr_basis(s, R, c);
    const double sx = s->width / 2.0, sy = s->height / 2.0;      // _screen_effect_model(width, height, z_scale = front_depth)
    auto world = [&](double x, double y, double z) {
        XrVert v{};
        for (int i = 0; i < 3; ++i) v.p[i] = c[i] + R[i][0] * sx * x + R[i][1] * sy * y + R[i][2] * L.front_depth * z;
        return v;
    };
    for (int k = 0; k < XR_WALLS; ++k) {
        const bool horiz = k < 2;                              // top, bottom: s runs along x; left, right: along -y (TL -> BL)
        const double side = (k == 0 || k == 3) ? 1.0 : -1.0;  // the edge's own coordinate: y = +1 top, -1 bottom; x = -1 left, +1 right
        const double f_ac = horiz ? L.fy : L.fx, f_al = horiz ? L.fx : L.fy;
        const XrVert p00 = horiz ? world(0, side, 0) : world(side, 0, 0);
        const XrVert p10 = horiz ? world(1, side, 0) : world(side, -1, 0);
        const XrVert p01 = horiz ? world(0, side * f_ac, 1) : world(side * f_ac, 0, 1);
        xr_facet_row(p00, p10, p01, vp, w, h, out[k]);
        out[k].u0 = (float)(f_al - 1.0); out[k].ua = horiz ? 0.f : 1.f; out[k].ub = (k == 1 || k == 3) ? 1.f : 0.f;    }
}
// ---- the veil and frosted looks of the curved screen (d2s_dibr_xr_eyes_frost_curved; _build_curved_frost_verts,
// _render_curved_frost_with_uniforms, xr_viewer/effects.py:189-254, 759-787) ----
// The reference's mesh is 98 quads of two triangles, one TRIANGLES draw: two long walls of 48 quads along the arc's curved edges
// (horizontal: the top edge, then the bottom; vertical: u = 0, then u = 1), then one quad at each end of the arc.  A quad runs from
// two strip vertices (rear, t = 0) to their points on the front rectangle (t = 1): (rear0, rear1, front0), (front0, rear1, front1).  A
// long wall's quad is NOT planar (a chord of the arc against a straight front edge), so the unit is the triangle: 196 rows after the
// strip's 48, in draw order.  A triangle's row is a facet row over (p00, p10, p01) with he = hw - ha - hb, the uv fields the affine
// v_uv = (u, 1 - v), pad[] = (t0, ta, tb); covered <=> na >= 0, nb >= 0, he . (xc, yc, 1) >= 0, nw > 0, -1 <= z <= 1.
// Within a wall the triangles are a chain, each sharing an edge with the next.  They are labelled so that the edge shared with the
// predecessor is p10 - p01 (he) and the edge shared with the successor is p00 - p10 (b = 0): p00 is the vertex the triangle adds, p10
// the one that stays.  Triangle k + 1's he row is then set to the exact negation of triangle k's float32 hb row and tested > 0 where
// triangle k tests nb >= 0: one edge function for both, exactly one of the two covers a pixel centre (the strip's device).  That holds
// while the eye sees both triangles from the same side.  Where it lies BETWEEN their two planes (a long wall's quads are not planar, so
// a wall seen edge-on has a silhouette along some interior edge) both triangles lie on one side of the projected edge, as they do in
// GL's rasteriser: -hb(k) then points the other way than he(k + 1), and the triangle keeps its own edge.  Two different walls share
// only their first and last edges; there nothing of the kind is done.
constexpr int XR_TRIS = 4 * XR_MAX_FACETS + 4, XR_FROST_CURVED_ROWS = XR_MAX_FACETS + XR_TRIS;      // 196, 244
constexpr int XR_ENTRY_FROST_CURVED = 4;                // xr_plan's fifth entry
constexpr int XR_ENTRY_PANORAMA = 5;                    // the sixth: d2s_dibr_xr_eyes_panorama, which takes a glow OR a frost, and the panorama
constexpr int XR_ENTRY_PANORAMA_CURVED = 6;             // the seventh: d2s_dibr_xr_eyes_panorama_curved, PANORAMA without its one refusal
constexpr int XR_BIN_TILES = 4;                         // a block bins for XR_BIN_TILES x XR_BIN_TILES tiles of 16 x 16 pixels
constexpr uint32_t XR_BIN_LDS = 4 * sizeof(uint64_t);   // the bin list: one ballot per wave of the block
// triangle k (0 .. 195) opens its wall: its he is its own edge, tested >= 0
constexpr bool xr_tri_first(int k) { return k == 0 || k == 2 * XR_MAX_FACETS || k == 4 * XR_MAX_FACETS || k == 4 * XR_MAX_FACETS + 2; }

struct XrWallVert { double p[3], u, v, t; };
inline void xr_tri_row(const XrWallVert& p00, const XrWallVert& p10, const XrWallVert& p01, const double vp[16], int w, int h, XrFacet& F) {
    auto vert = [](const XrWallVert& q) { XrVert x; for (int i = 0; i < 3; ++i) x.p[i] = q.p[i]; x.u = q.u; x.v = 1.0 - q.v; return x; };
    xr_facet_row(vert(p00), vert(p10), vert(p01), vp, w, h, F, true);
    F.pad[0] = (float)p00.t; F.pad[1] = (float)(p10.t - p00.t); F.pad[2] = (float)(p01.t - p00.t);
}
// One eye's 196 triangle rows from the strip's own double-precision vertices (S.all) and the front rectangle
inline void xr_frost_curved_tris(const d2s_xr_screen* s, const XrSurface& S, const XrFrostLayout& L, const double vp[16], int w, int h, XrFacet* out) {
    double R[3][3], c[3];
    xr_basis(s, R, c);
    const int N = XR_MAX_FACETS;
    auto rear = [&](int col, int side) {
        const XrVert& q = S.all[2 * col + side];
        return XrWallVert{{q.p[0], q.p[1], q.p[2]}, q.u, q.v, 0.0};
    };
    auto front = [&](const XrWallVert& r) {
        const double lx = (2.0 * r.u - 1.0) * L.front_half_w, ly = (2.0 * r.v - 1.0) * L.front_half_h;
        XrWallVert f = r;
        for (int i = 0; i < 3; ++i) f.p[i] = c[i] + R[i][0] * lx + R[i][1] * ly + R[i][2] * L.front_depth;
        f.t = 1.0;
        return f;
    };
    int k = 0;
    auto quad = [&](const XrWallVert& r0, const XrWallVert& r1) {      // (rear0, rear1, front0), (front0, rear1, front1), labelled as above
        const XrWallVert f0 = front(r0), f1 = front(r1);
        xr_tri_row(r1, f0, r0, vp, w, h, out[k++]);
        xr_tri_row(f1, r1, f0, vp, w, h, out[k++]);
    };
    const bool vert = s->curve == D2S_XR_CURVE_VERTICAL;
    for (int wall = 0; wall < 2; ++wall) {
        const int side = vert ? wall : 1 - wall;
        for (int i = 0; i < N; ++i) quad(rear(i, side), rear(i + 1, side));
    }
    for (int end = 0; end < 2; ++end) quad(rear(end * N, 0), rear(end * N, 1));
    auto live = [&](int t) { return !(out[t].ha[0] == 0.f && out[t].ha[1] == 0.f && out[t].ha[2] == -1.f); };
    for (int t = 1; t < XR_TRIS; ++t) {
        if (xr_tri_first(t) || !live(t - 1) || !live(t)) continue;
        double same = 0.0;                                 // both rows are multiples of ONE line, the projected edge: of one sign?
        for (int j = 0; j < 3; ++j) same -= (double)out[t].he[j] * (double)out[t - 1].hb[j];
        if (same > 0.0)
            for (int j = 0; j < 3; ++j) out[t].he[j] = -out[t - 1].hb[j];
    }
}
// H x W: the frame (and its chain, frosted only)
inline void xr_frost_dev(const d2s_xr_frost* f, int H, int W, XrFrostDev& F) {
    F = XrFrostDev{};
    F.mode = f->mode;
    F.inset = (float)f->edge_inset; F.intensity = (float)f->intensity; F.alpha = (float)f->alpha;
    F.softness = (float)f->beam_softness; F.thickness = (float)f->beam_thickness;
    F.w0 = F.w1 = W; F.h0 = F.h1 = H;
    if (f->mode != 2) return;
    F.threshold = (float)f->threshold; F.noise_scale = (float)f->noise_scale; F.blend = (float)f->blend; F.diffuse = (float)f->diffuse;
    const float t = (float)f->time;
    F.tx = t * 0.011f; F.ty = -t * 0.007f;
    MipShape ms;
    mip_shape(H, W, ms);
    const float lam = fminf(fmaxf((float)f->lod, 0.f), (float)ms.q), l0f = floorf(lam);
    F.l0 = (int)l0f; F.l1 = F.l0 + 1 < ms.q ? F.l0 + 1 : ms.q; F.lf = lam - l0f;
    F.w0 = ms.w[F.l0]; F.h0 = ms.h[F.l0]; F.w1 = ms.w[F.l1]; F.h1 = ms.h[F.l1];
    F.off0 = ms.off[F.l0]; F.off1 = ms.off[F.l1]; F.chain_total = ms.total;
}

// ---- the eye views' plan: everything the four entries decide from the arguments that are no device pointers ----
struct XrEyeDev { int w, h, eye, nf; long out_off; };      // out_off: the eye image's first element in out; its table: eye index * rows_per_eye
struct XrEyes { XrEyeDev e[2]; int n; float clear[4]; };
// The curved glow's kernel keeps the eye's rows (padded to 25 floats) and the 49 seams in static LDS
constexpr int XR_LDS_ROW = XR_ROW_FLOATS + 1;
constexpr uint32_t XR_CURVED_LDS = (XR_PIECES * XR_LDS_ROW + XR_SEAMS * 3) * sizeof(float);
// rows an eye's table occupies in the workspace (d2s_dibr_xr_workspace, d2s_dibr_xr_glow_curved_workspace, d2s_dibr_xr_frost_workspace,
// d2s_dibr_xr_frost_curved_workspace, the kernels' stride).  FROST: the screen's rows, then the four wall rows directly after the rows
// written (row nf .. nf + 3); FROST_CURVED: the strip's 48 rows, then the 196 triangles
constexpr int xr_table_rows(int kind) {
    return kind == D2S_XR_KIND_FROST_CURVED ? XR_FROST_CURVED_ROWS : kind == D2S_XR_KIND_GLOW_CURVED ? XR_PIECES
         : kind == D2S_XR_KIND_FROST ? XR_MAX_FACETS + XR_WALLS : XR_MAX_FACETS;
}

struct XrPlan {
    int kind;                                     // D2S_XR_KIND_*: which kernel draws
    DibrGeomProj g;
    XrEyes ex;
    XrGlowDev G;                                  // kind GLOW, GLOW_CURVED
    XrFrostDev F;                                 // kind FROST, FROST_CURVED
    XrCurvedDev Q;                                // kind == GLOW_CURVED
    bool pano;                                    // the background is the panorama P (GLOW_CURVED, FROST_CURVED: XR_ENTRY_PANORAMA_CURVED only)
    XrPanoDev P;
    bool up;                                      // depth is not at the frame's resolution: the UpDep sampler
    int rows_per_eye;                             // rows written per eye: the surface's facets (1 | 48), XR_PIECES, FROST: facets + 4,
    XrFacet rows[2][XR_FROST_CURVED_ROWS];        // FROST_CURVED: 244
    int setup_launches;                           // all eyes': XR_CHUNK_FACETS rows travel in one launch's arguments
    unsigned grid[3];
    uint32_t lds_dynamic, lds_static;
    uint64_t workspace_bytes;
    uint64_t offs[2], total;                      // the out layout (xr_out_layout)
};

// entry: D2S_XR_ENTRY_*, XR_ENTRY_FROST or XR_ENTRY_FROST_CURVED, the public call that asks.  EYES takes no glow (the caller passes
// none); GLOW refuses a curved screen with glow on; FROST takes the frost and no glow and refuses a curved screen with frost on,
// FROST_CURVED draws it; PANORAMA takes a glow or a frost, flat or curved, as GLOW_CURVED and FROST_CURVED do, and with a panorama
// refuses the two curved looks; PANORAMA_CURVED is PANORAMA in every check but that refusal, which it does not make.  Every refusal of
// the seven entries that needs no device pointer, in their order; no HIP call.
inline int xr_plan(int entry, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double* crop, const d2s_xr_screen* screen,
                   const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_glow* glow, const d2s_xr_frost* frost, XrPlan& pl,
                   const d2s_xr_panorama* pano = nullptr) {
    const bool curved_pano = entry == XR_ENTRY_PANORAMA_CURVED;
    if (curved_pano) entry = XR_ENTRY_PANORAMA;
    D2S_REQUIRE(p, "null pointer");
    int rc = dibr_check(p, dh, dw, batch, H, W, out_fmt);
    if (rc) return rc;
    D2S_REQUIRE(!p->feather_enabled, "feather_enabled must be 0 (the OpenXR viewer never enables the feathering)");
    if (crop) {                                            // what d2s_dibr_warp_crop refuses about a crop, its 2 x 2 pixel floor included
        int a, b2, c2, d2;
        rc = crop_eye_shape(H, W, crop, D2S_MODE_FULL_SBS, &a, &b2, &c2, &d2);
        if (rc) return rc;
    }
    rc = xr_screen_check(screen, eyes, n_eyes, batch);
    if (rc) return rc;
    rc = xr_glow_check(screen, glow, entry == D2S_XR_ENTRY_GLOW_CURVED || entry == XR_ENTRY_PANORAMA);
    if (rc) return rc;
    const bool frost_entry = entry == XR_ENTRY_FROST || entry == XR_ENTRY_FROST_CURVED || entry == XR_ENTRY_PANORAMA;
    rc = xr_frost_check(screen, frost_entry ? frost : nullptr, entry == XR_ENTRY_FROST_CURVED || entry == XR_ENTRY_PANORAMA);
    if (rc) return rc;
    const bool glow_on = glow && glow->mode != 0, frost_on = frost_entry && xr_frost_on(frost);
    D2S_REQUIRE(!(glow_on && frost_on), "at most one of glow and frost may be on (the reference draws one look)");
    rc = xr_pano_check(entry == XR_ENTRY_PANORAMA ? pano : nullptr, n_eyes);
    if (rc) return rc;
    pl.pano = entry == XR_ENTRY_PANORAMA && pano;
    if (pl.pano && !curved_pano && screen->curve != D2S_XR_CURVE_FLAT && (glow_on || frost_on)) {
        set_error("unsupported: a panorama behind the glow, veil or frosted look of a CURVED screen is not built (the two heaviest eye "
                  "kernels get the background in a change of their own); with a panorama, curve must be 0 or glow and frost off");
        return D2S_E_UNSUPPORTED;
    }
    D2S_REQUIRE(!(frost_on && frost->mode == 2) || (H >= 2 && W >= 2 && H <= 8192 && W <= 8192),
                "frame must be 2 .. 8192 on a side with the frosted look on (d2s_mip_chain's range)");
    D2S_REQUIRE(!glow_on || (H >= 2 && W >= 2 && H <= 8192 && W <= 8192), "frame must be 2 .. 8192 on a side with glow on (d2s_mip_chain's range)");
    const bool tris = frost_on && screen->curve != D2S_XR_CURVE_FLAT;      // (only FROST_CURVED and the two panorama entries come this far with one)
    pl.kind = tris ? D2S_XR_KIND_FROST_CURVED : frost_on ? D2S_XR_KIND_FROST : !glow_on ? D2S_XR_KIND_PLAIN : screen->curve == D2S_XR_CURVE_FLAT ? D2S_XR_KIND_GLOW : D2S_XR_KIND_GLOW_CURVED;
    const bool curved = pl.kind == D2S_XR_KIND_GLOW_CURVED;
    xr_out_layout(eyes, n_eyes, batch, p->alpha_mode, pl.offs, &pl.total);
    pl.G = XrGlowDev{};
    pl.Q = XrCurvedDev{};
    pl.F = XrFrostDev{};
    pl.P = XrPanoDev{};
    if (pl.pano) {
        const XrEyeSize es[2] = {{eyes[0].width, eyes[0].height}, {eyes[n_eyes - 1].width, eyes[n_eyes - 1].height}};
        xr_pano_dev(pano, es, n_eyes, pl.P);
    }
    XrFrostLayout L{};
    if (frost_on) { xr_frost_dev(frost, H, W, pl.F); L = xr_frost_layout(screen, frost); }
    XrSurface S;
    xr_surface(screen, S);
    XrCurvedPieces P;
    if (glow_on) {
        const XrGlowExtents x = xr_glow_extents(screen, glow);
        xr_glow_dev(x, glow->mode, H, W, pl.G);
        if (curved) {
            double e_al;
            xr_curved_dev(screen, x, pl.Q, &e_al);
            xr_curved_pieces(screen, e_al, P);
        }
    }
    pl.lds_dynamic = (uint32_t)pl.G.n_tex * 3 * sizeof(float);      // <= 65 532 bytes (an 8192 x 8192 frame)
    pl.lds_static = curved ? XR_CURVED_LDS : tris ? XR_BIN_LDS : 0;
    if (pl.lds_dynamic + pl.lds_static > 65536) {                   // (only an 8192 x 8192 frame's 5 461 texels)
        set_error("unsupported: the frame's coarse mip levels and the piece table exceed 64 KB of LDS (a frame of 8192 x 8192)");
        return D2S_E_UNSUPPORTED;
    }
    for (int i = 0; i < n_eyes; ++i) {
        if (!(xr_min_w(S, eyes[i].vp) > 1e-6)) {
            set_error("unsupported: a vertex of the screen has clip w <= 1e-6 (the screen crosses the eye plane)");
            return D2S_E_UNSUPPORTED;
        }
        if (curved && !xr_eye_inside(S, P, eyes[i].vp)) {
            set_error("unsupported: an eye lies outside the convex region the curved screen and its two tangent planes bound (behind the "
                      "screen or beyond an end of the arc): the glow's pieces would overlap and need blending in draw order");
            return D2S_E_UNSUPPORTED;
        }
    }
    DibrGeomProj& g = pl.g;
    dibr_fill_geom(g, p, H, W, dh, dw);
    g.c = cosf((float)screen->roll); g.s = sinf((float)screen->roll);                 // u_roll = screen_roll (effects.py:1113, 1129)
    g.feather = 0;
    g.mode = 0; g.oh = g.ow = g.out_h = g.out_w = 0;
    g.vpx = g.vpy = 0.f; g.vpw = g.vph = 1.f;
    g.cx = crop ? (float)crop[0] : 0.f; g.cy = crop ? (float)crop[1] : 0.f; g.cw = crop ? (float)crop[2] : 1.f; g.ch = crop ? (float)crop[3] : 1.f;
    pl.up = dh != H || dw != W;
    pl.rows_per_eye = curved ? XR_PIECES : tris ? XR_FROST_CURVED_ROWS : S.n + (frost_on ? XR_WALLS : 0);
    pl.ex = XrEyes{};
    pl.ex.n = n_eyes;
    for (int k = 0; k < 4; ++k) pl.ex.clear[k] = screen->clear[k];
    int mw = 0, mh = 0;
    for (int i = 0; i < n_eyes; ++i) {
        pl.ex.e[i] = XrEyeDev{eyes[i].width, eyes[i].height, eyes[i].eye, S.n, (long)pl.offs[i]};
        mw = std::max(mw, eyes[i].width); mh = std::max(mh, eyes[i].height);
        if (curved) xr_curved_table(S, P, glow->mode, eyes[i].vp, eyes[i].width, eyes[i].height, pl.rows[i]);
        else xr_facets(S, eyes[i].vp, eyes[i].width, eyes[i].height, pl.rows[i]);
        if (tris) xr_frost_curved_tris(screen, S, L, eyes[i].vp, eyes[i].width, eyes[i].height, pl.rows[i] + S.n);
        else if (frost_on) xr_frost_walls(screen, L, eyes[i].vp, eyes[i].width, eyes[i].height, pl.rows[i] + S.n);
    }
    pl.setup_launches = n_eyes * cdiv(pl.rows_per_eye, XR_CHUNK_FACETS);               // per eye: 1 (flat, frost), 2 (curved), 3 (curved glow), 11
    const int side = tris ? 16 * XR_BIN_TILES : 16;                                    // the pixels a block draws, each way
    pl.grid[0] = cdiv(mw, side); pl.grid[1] = cdiv(mh, side); pl.grid[2] = n_eyes * batch;
    pl.workspace_bytes = (uint64_t)n_eyes * xr_table_rows(pl.kind) * sizeof(XrFacet);
    return D2S_OK;
}

// ---- the world-space panels drawn after the screen and its look (d2s_dibr_xr_panels; _render_fps_overlay and _render_keyboard,
// xr_viewer/overlay.py:81-249, 1427-1510; the OSDs and lasers of _render_eye, xr_viewer/effects.py:1157-1225) ----
// A panel is the unit quad under an affine model matrix: one facet row per eye, written after the screen's own rows (row nf + k) by
// the same set-up launches.  ha, hb, hw, hz are a facet's; the other twelve floats carry what the pass needs instead of he and a uv
// affine (a panel's uv IS (a, b)), every one a small integer or a colour, exact in float:
//   12 .. 15  the panel's pixel box on this eye image, x0, y0, x1, y1 (x1 <= x0: not on this image): the projected corners' bounds
//             grown by one pixel (the per-pixel test rounds by about 1e-4 pixel) and clamped to the image;
//   16 texture index or -1;  17 flags (D2S_XR_PANEL_*);  18 .. 21 colour, rgb in levels (0..255);  22 u_alpha;  23 unused.
constexpr int XR_MAX_PANELS = D2S_XR_MAX_PANELS, XR_MAX_TEXTURES = 32;
constexpr int XR_PANEL_ROWS = XR_MAX_FACETS + XR_MAX_PANELS;      // an eye's table in the workspace (d2s_dibr_xr_panels_workspace)
struct XrTexDev { const uint8_t* rgba; int w, h, wrap, pad; };
// tile0, tiles: per eye, the 16 x 16 tiles the boxes touch, as a rectangle of tiles (a block whose tile no box touches leaves at once)
struct XrPanelsDev { int n, nch; int tile0[2][2], tiles[2][2]; XrTexDev t[XR_MAX_TEXTURES]; };

struct XrPanelsPlan {
    XrEyes ex;
    XrPanelsDev P;
    int rows_per_eye, setup_launches, render_launches, drawn[2];
    XrFacet rows[2][XR_PANEL_ROWS];
    unsigned grid[3];
    uint64_t workspace_bytes, offs[2], total;
};

// Everything d2s_dibr_xr_panels decides from the arguments that are no device pointers, and every refusal of that kind; no HIP call.
inline int xr_panels_plan(int out_fmt, int batch, int alpha_mode, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes,
                          const d2s_xr_panel* panels, int n_panels, const d2s_xr_texture* textures, int n_textures, XrPanelsPlan& pl) {
    D2S_REQUIRE(out_fmt == D2S_FMT_U8_HWC || out_fmt == D2S_FMT_F32_HWC, "bad out_fmt (U8_HWC or F32_HWC)");
    D2S_REQUIRE(batch > 0 && batch <= 65535, "bad batch (1 .. 65535)");
    D2S_REQUIRE(alpha_mode >= D2S_DIBR_ALPHA_WINDOW && alpha_mode <= D2S_DIBR_ALPHA_RGBA, "bad alpha_mode");
    if (alpha_mode == D2S_DIBR_ALPHA_PREMULTIPLIED) {
        set_error("unsupported: D2S_DIBR_ALPHA_PREMULTIPLIED eye images (rgb already times alpha: the destination the reference blends "
                  "its panels over cannot be formed); draw the panels over D2S_DIBR_ALPHA_RGBA or D2S_DIBR_ALPHA_WINDOW images");
        return D2S_E_UNSUPPORTED;
    }
    int rc = xr_screen_check(screen, eyes, n_eyes, batch);
    if (rc) return rc;
    D2S_REQUIRE(n_panels >= 0 && n_panels <= XR_MAX_PANELS, "n_panels must be 0 .. 32 (D2S_XR_MAX_PANELS)");
    D2S_REQUIRE(n_textures >= 0 && n_textures <= XR_MAX_TEXTURES, "n_textures must be 0 .. 32");
    D2S_REQUIRE((n_panels == 0 || panels) && (n_textures == 0 || textures), "null pointer (panels, textures)");
    pl.P = XrPanelsDev{};
    for (int t = 0; t < n_textures; ++t) {
        D2S_REQUIRE(textures[t].struct_size == sizeof(d2s_xr_texture), "d2s_xr_texture.struct_size must be sizeof(d2s_xr_texture) = 24");
        D2S_REQUIRE(textures[t].width >= 1 && textures[t].height >= 1 && textures[t].width <= 8192 && textures[t].height <= 8192,
                    "a panel texture must be 1 .. 8192 on a side");
        D2S_REQUIRE(textures[t].wrap == D2S_XR_WRAP_REPEAT || textures[t].wrap == D2S_XR_WRAP_CLAMP, "bad texture wrap (D2S_XR_WRAP_*)");
        pl.P.t[t] = XrTexDev{textures[t].rgba, textures[t].width, textures[t].height, textures[t].wrap, 0};
    }
    for (int k = 0; k < n_panels; ++k) {
        const d2s_xr_panel& q = panels[k];
        D2S_REQUIRE(q.struct_size == sizeof(d2s_xr_panel), "d2s_xr_panel.struct_size must be sizeof(d2s_xr_panel) = 160");
        D2S_REQUIRE(xr_finite(q.model, 16), "a panel's model matrix must be finite");
        D2S_REQUIRE(q.model[12] == 0.0 && q.model[13] == 0.0 && q.model[14] == 0.0 && q.model[15] == 1.0,
                    "a panel's model matrix must be affine (last row 0 0 0 1)");
        D2S_REQUIRE(q.texture >= -1 && q.texture < n_textures, "a panel's texture must be -1 (solid) or an index into textures");
        D2S_REQUIRE((q.flags & ~(uint32_t)(D2S_XR_PANEL_DEPTH_TEST | D2S_XR_PANEL_DEPTH_WRITE | D2S_XR_PANEL_BLEND)) == 0, "unknown panel flags (D2S_XR_PANEL_*)");
        D2S_REQUIRE(std::isfinite(q.alpha) && std::isfinite(q.color[0]) && std::isfinite(q.color[1]) && std::isfinite(q.color[2]) &&
                    std::isfinite(q.color[3]), "a panel's alpha and color must be finite");
    }
    XrSurface S;
    xr_surface(screen, S);
    for (int i = 0; i < n_eyes; ++i)
        if (!(xr_min_w(S, eyes[i].vp) > 1e-6)) {
            set_error("unsupported: a vertex of the screen has clip w <= 1e-6 (the screen crosses the eye plane)");
            return D2S_E_UNSUPPORTED;
        }
    xr_out_layout(eyes, n_eyes, batch, alpha_mode, pl.offs, &pl.total);
    pl.P.n = n_panels; pl.P.nch = alpha_mode == D2S_DIBR_ALPHA_RGBA ? 4 : 3;
    pl.ex = XrEyes{};
    pl.ex.n = n_eyes;
    pl.rows_per_eye = S.n + n_panels;
    pl.workspace_bytes = (uint64_t)n_eyes * XR_PANEL_ROWS * sizeof(XrFacet);
    int mx = 0, my = 0, any = 0;
    for (int i = 0; i < n_eyes; ++i) {
        const int w = eyes[i].width, h = eyes[i].height;
        pl.ex.e[i] = XrEyeDev{w, h, eyes[i].eye, S.n, (long)pl.offs[i]};
        xr_facets(S, eyes[i].vp, w, h, pl.rows[i]);
        pl.drawn[i] = 0;
        int bx0 = w, by0 = h, bx1 = 0, by1 = 0;
        for (int k = 0; k < n_panels; ++k) {
            const d2s_xr_panel& q = panels[k];
            XrVert v[4];                                   // (-1, -1), (1, -1), (-1, 1), (1, 1): uv (0, 0), (1, 0), (0, 1), (1, 1)
            int behind = 0;
            double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
            for (int c = 0; c < 4; ++c) {
                const double lx = (c & 1) ? 1.0 : -1.0, ly = (c & 2) ? 1.0 : -1.0;
                for (int r = 0; r < 3; ++r) v[c].p[r] = q.model[4 * r] * lx + q.model[4 * r + 1] * ly + q.model[4 * r + 3];
                v[c].u = (c & 1) ? 1.0 : 0.0; v[c].v = (c & 2) ? 1.0 : 0.0;
                double cl[4];
                xr_clip(eyes[i].vp, v[c].p, 1.0, cl);
                if (!(cl[3] > 1e-6)) { ++behind; continue; }
                const double px = (cl[0] / cl[3] + 1.0) * 0.5 * w, py = (1.0 - cl[1] / cl[3]) * 0.5 * h;
                x0 = fmin(x0, px); x1 = fmax(x1, px); y0 = fmin(y0, py); y1 = fmax(y1, py);
            }
            if (behind != 0 && behind != 4) {
                set_error("unsupported: a vertex of a panel has clip w <= 1e-6 but not all four (the panel crosses the eye plane)");
                return D2S_E_UNSUPPORTED;
            }
            XrFacet& F = pl.rows[i][S.n + k];
            xr_facet_row(v[0], v[1], v[2], eyes[i].vp, w, h, F);
            const bool live = !(F.ha[0] == 0.f && F.ha[1] == 0.f && F.ha[2] == -1.f);      // (edge-on: covers no pixel centre)
            int ix0 = 0, iy0 = 0, ix1 = 0, iy1 = 0;
            if (behind == 0 && live && std::isfinite(x0) && std::isfinite(x1) && std::isfinite(y0) && std::isfinite(y1)) {
                ix0 = (int)fmax(0.0, floor(x0) - 1.0); iy0 = (int)fmax(0.0, floor(y0) - 1.0);
                ix1 = (int)fmin((double)w, ceil(x1) + 1.0); iy1 = (int)fmin((double)h, ceil(y1) + 1.0);
            }
            if (ix1 <= ix0 || iy1 <= iy0) ix0 = iy0 = ix1 = iy1 = 0;
            else { ++pl.drawn[i]; bx0 = std::min(bx0, ix0); by0 = std::min(by0, iy0); bx1 = std::max(bx1, ix1); by1 = std::max(by1, iy1); }
            F.he[0] = (float)ix0; F.he[1] = (float)iy0; F.he[2] = (float)ix1; F.u0 = (float)iy1;
            F.ua = (float)q.texture; F.ub = (float)q.flags;
            F.v0 = q.color[0] * 255.0f; F.va = q.color[1] * 255.0f; F.vb = q.color[2] * 255.0f; F.pad[0] = q.color[3];
            F.pad[1] = q.alpha; F.pad[2] = 0.f;
        }
        if (pl.drawn[i]) {
            pl.P.tile0[i][0] = bx0 / 16; pl.P.tile0[i][1] = by0 / 16;
            pl.P.tiles[i][0] = cdiv(bx1, 16) - bx0 / 16; pl.P.tiles[i][1] = cdiv(by1, 16) - by0 / 16;
            mx = std::max(mx, pl.P.tiles[i][0]); my = std::max(my, pl.P.tiles[i][1]);
            any = 1;
        }
    }
    pl.render_launches = any;
    pl.setup_launches = any ? n_eyes * cdiv(pl.rows_per_eye, XR_CHUNK_FACETS) : 0;
    pl.grid[0] = mx; pl.grid[1] = my; pl.grid[2] = any ? n_eyes * batch : 0;
    return D2S_OK;
}

// The seven entries as one call (dibr.hip): xr_plan, then the device pointers and the workspace, then the launches.  check_only:
// every refusal, nothing launched (the view pipelines ask before they start the model).
int dibr_xr_entry_any(int entry, const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                      const double* crop, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt,
                      void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const d2s_xr_frost* frost, const uint8_t* levels, void* stream,
                      bool check_only, const d2s_xr_panorama* pano = nullptr, const uint8_t* pano_rgb = nullptr,
                      const uint8_t* pano_levels = nullptr);

}  // namespace d2s
