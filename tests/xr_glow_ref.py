"""CPU restatement (numpy) of the colour mip chain (d2s_mip_chain) and of the glow around the flat OpenXR screen
(d2s_dibr_xr_eyes_glow).  TEST INFRASTRUCTURE ONLY.

The chain: what glGenerateMipmap gives the reference's colour texture (xr_viewer/effects.py:597-646), as renders show it
(tests/golden/make_golden_xr_glow.py): level k is max(1, floor(n / 2)) per axis, each texel the bilinear sample of the already 8-bit
level k - 1 at the texel's normalised centre -- source coordinate (i + 0.5) * n_prev / n_k - 0.5, clamped to the edge -- rounded half
to even.  The four weights are integers over the denominator 4 * w_k * h_k; in float64 the products and their sum are exact and the
one division is correctly rounded, so the float64 form IS the exact value (a tie stays a tie); the float32 form rounds the products.

The glow: EffectsMixin._render_glow (effects.py:476-585) and its shader _GLOW_FRAG (xr_viewer/glsl.py:580-666) in _render_eye's
order (effects.py:1050-1145) -- clear; the outer band blended over it (ONE, ONE_MINUS_SRC_ALPHA, on rgb and alpha, depth test off,
where the plane point has clip w > 0 and NDC z in [-1, 1]); the screen (xr_eye_ref: blending off, it overwrites); mode 1: the inner
band blended over the screen -- over a number type T, the uniforms being the float32 values GL receives.  The glow quad lies in the
screen's plane: with (a, b) the screen facet's own coordinates (its homography without the 0..1 bound) the glow's uv is
0.5 + ((a, b) - 0.5) * (inner_w, inner_h).
"""
from __future__ import annotations

import numpy as np

import xr_eye_ref as X

GLOW_SOURCE_LOD = 7


# ---- the chain ----

def level_sizes(H, W):
    """[(h, w)] of levels 0 .. q."""
    out = [(H, W)]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append((max(1, h // 2), max(1, w // 2)))
    return out


def _axis(npv, nk):
    """(i0, i1, r): the two source texels of every texel of an axis and the second one's weight over 2 * nk (integers)."""
    i = np.arange(nk, dtype=np.int64)
    num, den = (2 * i + 1) * npv - nk, 2 * nk
    i0 = num // den
    r = num - i0 * den
    last = i0 >= npv - 1
    i0, r = np.where(last, npv - 1, i0), np.where(last, 0, r)
    return i0, np.minimum(i0 + 1, npv - 1), r


def next_level(prev, T=np.float64):
    """uint8 [hp, wp, 3] -> uint8 [hk, wk, 3].  T = float64: exact (see the module text); T = float32: the same sum in float32."""
    hp, wp = prev.shape[:2]
    hk, wk = max(1, hp // 2), max(1, wp // 2)
    x0, x1, rx = _axis(wp, wk)
    y0, y1, ry = _axis(hp, hk)
    wx1, wx0 = rx.astype(T)[None, :, None], (2 * wk - rx).astype(T)[None, :, None]
    wy1, wy0 = ry.astype(T)[:, None, None], (2 * hk - ry).astype(T)[:, None, None]
    p = prev.astype(T)
    top = wx0 * p[y0][:, x0] + wx1 * p[y0][:, x1]
    bot = wx0 * p[y1][:, x0] + wx1 * p[y1][:, x1]
    v = ((wy0 * top + wy1 * bot).astype(T) / T(4 * wk * hk)).astype(T)
    return np.rint(v).astype(np.uint8)                     # rint: half to even


def chain(img, T=np.float64):
    """uint8 [H, W, 3] -> [level 0 (the frame), level 1, .. level q]."""
    out = [np.ascontiguousarray(img)]
    while out[-1].shape[:2] != (1, 1):
        out.append(next_level(out[-1], T))
    return out


def pack(levels):
    """levels 1 .. q as d2s_mip_chain lays them out: uint8 [total]."""
    return np.concatenate([l.reshape(-1) for l in levels[1:]])


# ---- the glow ----

def uniforms(screen_w, screen_h, mode, range_m, inner_edge_fraction):
    """_render_glow:486-495 in float64 -> dict(inner_w, inner_h, half (x, y), inv_range, inner)."""
    rng = max(float(range_m), 1e-4) * (0.5 if mode == 2 else 1.0)
    glow_w, glow_h = screen_w + 2 * rng, screen_h + 2 * rng
    inner_w, inner_h = screen_w / glow_w, screen_h / glow_h
    inner_uv = 0.0 if mode == 2 else min(inner_w, inner_h) * max(float(inner_edge_fraction), 0.0)
    return dict(glow_w=glow_w, glow_h=glow_h, inner_w=inner_w, inner_h=inner_h, half=(inner_w * 0.5, inner_h * 0.5),
                inv_range=1.0 / max(rng / max(glow_w, glow_h), 1e-6), inner=inner_uv)


def _smooth01(t, T):
    t = np.clip(t, T(0), T(1)).astype(T)
    return (t * t * (T(3) - T(2) * t)).astype(T)


def _level_tap(lev, u, v, T):
    """GL_LINEAR, CLAMP_TO_EDGE, of one level [h, w, 3] (already T) at flat u, v -> [n, 3]."""
    h, w = lev.shape[:2]
    x, y = u * T(w) - T(0.5), v * T(h) - T(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(T)[:, None], (y - y0f).astype(T)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    a, b, c, d = lev[ya, xa], lev[ya, xb], lev[yb, xa], lev[yb, xb]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    return (top + (bot - top) * fy).astype(T)


def texture_lod(levels, su, sv, lod, crop, T):
    """textureLod(u_source, source_uv(s), lod).rgb in 0..255: LOD clamped to [0, q], trilinear."""
    q = len(levels) - 1
    cx, cy, cw, ch = (T(np.float32(c)) for c in crop)
    u = np.clip(cx + np.clip(su, T(0), T(1)) * cw, T(0), T(1)).astype(T)
    v = np.clip(cy + np.clip(sv, T(0), T(1)) * ch, T(0), T(1)).astype(T)
    lam = np.clip(lod, T(0), T(q)).astype(T)
    l0f = np.floor(lam)
    f = (lam - l0f).astype(T)[:, None]
    l0 = l0f.astype(np.int64)
    l1 = np.minimum(l0 + 1, q)
    a, b = np.zeros((u.size, 3), T), np.zeros((u.size, 3), T)
    for l in np.unique(np.concatenate([l0, l1])):
        lev = levels[l].astype(T)
        m = l0 == l
        if m.any():
            a[m] = _level_tap(lev, u[m], v[m], T)
        m = l1 == l
        if m.any():
            b[m] = _level_tap(lev, u[m], v[m], T)
    return (a * (T(1) - f) + b * f).astype(T)


def glow_frag(levels, a, b, U, crop, inner_only, T):
    """_GLOW_FRAG.main at the plane coordinates a, b (flat arrays) -> (drawn [n] bool, src [n, 4] = (colour * glow in 0..255, glow))."""
    f32 = np.float32
    half_x, half_y = T(f32(U["half"][0])), T(f32(U["half"][1]))
    inner_w, inner_h = T(f32(U["inner_w"])), T(f32(U["inner_h"]))
    inv_range, inner = max(T(f32(U["inv_range"])), T(f32(0.001))), max(T(f32(U["inner"])), T(0))
    a, b = a.astype(T), b.astype(T)
    with np.errstate(all="ignore"):
        cx, cy = ((a - T(0.5)) * inner_w).astype(T), ((b - T(0.5)) * inner_h).astype(T)
        sd = np.maximum(np.abs(cx) - half_x, np.abs(cy) - half_y).astype(T)
        if inner_only:
            keep = ~((sd > 0) | (sd < -inner)) if inner > 0 else np.zeros(a.shape, bool)
            edge_pos = sd + inner
        else:
            keep = sd > 0
            edge_pos = sd
        edge_t = np.clip(edge_pos * inv_range, T(0), T(1)).astype(T)
        glow = np.power(np.maximum(T(1) - _smooth01(edge_t, T), T(0)), T(f32(0.58))).astype(T)
        if inner_only:
            dens = _smooth01((sd + inner) / max(inner, T(f32(1e-6))), T)
            dens = (dens * dens * (T(3) - T(2) * dens)).astype(T)
            glow = (glow * dens).astype(T)
        keep &= glow > T(f32(0.001))                       # (NaN fails: no glow)
    src = np.zeros((a.size, 4), T)
    if not keep.any():
        return keep, src
    k = keep
    rx = (((cx[k] + T(0.5)) - (T(0.5) - half_x)) / max(half_x * T(2), T(f32(1e-5)))).astype(T)
    ry = (T(1) - ((cy[k] + T(0.5)) - (T(0.5) - half_y)) / max(half_y * T(2), T(f32(1e-5)))).astype(T)
    dx, dy = (rx - T(0.5) + T(f32(1e-5))).astype(T), (ry - T(0.5)).astype(T)
    ln = np.sqrt(dx * dx + dy * dy).astype(T)
    dx, dy = (dx / ln).astype(T), (dy / ln).astype(T)
    es = np.minimum(T(0.5) / np.maximum(np.abs(dx), T(f32(1e-5))), T(0.5) / np.maximum(np.abs(dy), T(f32(1e-5)))).astype(T)
    ex, ey = np.clip(T(0.5) + dx * es, T(0), T(1)).astype(T), np.clip(T(0.5) + dy * es, T(0), T(1)).astype(T)
    blur_t = np.zeros(rx.shape, T) if inner_only else _smooth01(edge_t[k], T)
    back = (T(f32(0.015)) * (T(1) - blur_t) + T(f32(0.060)) * blur_t).astype(T)
    lod = (T(7) * (T(1) - blur_t) + T(9) * blur_t).astype(T)
    local = texture_lod(levels, ex - dx * back, ey - dy * back, lod, crop, T)
    edge = local if inner_only else texture_lod(levels, ex, ey, lod + T(1), crop, T)
    mt = (blur_t * T(0.5))[:, None]
    g = glow[k][:, None]
    src[k, :3] = (local * (T(1) - mt) + edge * mt) * g
    src[k, 3] = glow[k]
    return keep, src.astype(T)


def plane_coords(tab, w, h, T):
    """The screen facet's homography without its bounds: (drawn [h,w]: clip w > 0 and NDC z in [-1, 1]; a, b [h,w])."""
    r = X._rows(tab, T)[0]
    yc, xc = np.meshgrid((np.arange(h, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(w, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")
    na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
    z = r[9] * xc + r[10] * yc + r[11]
    with np.errstate(all="ignore"):
        return (nw > 0) & (z >= -1) & (z <= 1), (na / nw).astype(T), (nb / nw).astype(T)


NONE, OUTER, SCREEN, SCREEN_INNER = 0, 1, 2, 3


def render_eye(rgb_u8_hwc, depth, levels, facets, vp, w, h, eye, clear, screen_w, screen_h, mode, range_m, inner_edge_fraction=0.075,
               crop=(0.0, 0.0, 1.0, 1.0), T=np.float64, **shade_kw):
    """One eye image with the glow -> (framebuffer [h,w,4] T: rgb 0..255, alpha 0..1; region class [h,w]: NONE, OUTER (the outer band
    drew), SCREEN, SCREEN_INNER (the inner band drew over the screen)).  levels: chain(rgb); mode 1 glow, 2 glow2."""
    assert len(facets) == 1, "the glow is the flat screen's"
    tab = X.facet_table(facets, vp, w, h)
    out, cov = X.render_eye(rgb_u8_hwc, depth, facets, vp, w, h, eye, clear, crop=crop, T=T, **shade_kw)
    U = uniforms(screen_w, screen_h, mode, range_m, inner_edge_fraction)
    plane, a, b = plane_coords(tab, w, h, T)
    cls = np.where(cov, SCREEN, NONE)
    m = plane & ~cov
    if m.any():
        keep, src = glow_frag(levels, a[m], b[m], U, crop, False, T)
        dst = out[m]
        dst[keep] = src[keep] + dst[keep] * (T(1) - src[keep, 3:4])
        out[m] = dst
        c = cls[m]
        c[keep] = OUTER
        cls[m] = c
    m = plane & cov
    if mode == 1 and m.any():
        keep, src = glow_frag(levels, a[m], b[m], U, crop, True, T)
        dst = out[m]
        dst[keep] = src[keep] + dst[keep] * (T(1) - src[keep, 3:4])
        out[m] = dst
        c = cls[m]
        c[keep] = SCREEN_INNER
        cls[m] = c
    return out.astype(T), cls


def uniform3x3(cls):
    """Pixels whose 3 x 3 neighbourhood (clamped at the border) has one region class."""
    p = np.pad(cls, 1, mode="edge")
    h, w = cls.shape
    ok = np.ones(cls.shape, bool)
    for dy in range(3):
        for dx in range(3):
            ok &= p[dy:dy + h, dx:dx + w] == cls
    return ok


# ---- the cases of tests/golden/xr_glow.json (make_golden_xr_glow.py) ----

def case_scene(c):
    """(rgb, depth) of a manifest case."""
    from desktop2stereo_amd import synth
    H, W = c["source"]
    return synth.dibr_scene(H, W, c["seed"], "boxes")


def case_kw(c):
    return dict(crop=c["crop"], ipd_uv=c["ipd_uv"], depth_strength=0.1 * c["depth_ratio"], convergence=c["convergence"],
                roll=c["screen"]["roll"], corner_radius=c["corner_radius"])


def case_render(c, e, img, dep, levels, eye_w, eye_h, T=np.float64):
    return render_eye(img, dep, levels, X.facets_flat(np.array(c["model"])), np.array(e["vp"]), eye_w, eye_h, e["eye"], c["clear"],
                      c["screen"]["width"], c["screen"]["height"], c["mode"], c["range_m"], c["inner_edge_fraction"], T=T, **case_kw(c))


def golden_eye(z, c, eye):
    return np.concatenate([z[f"{c['name']}_{eye}_rgb"].astype(np.float64) / 16.0, z[f"{c['name']}_{eye}_a"].astype(np.float64)[..., None] / 65535.0], -1)
