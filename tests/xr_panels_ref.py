"""CPU restatement (numpy) of the world-space panels of the OpenXR eye image (d2s_dibr_xr_panels).  TEST INFRASTRUCTURE ONLY.

What EffectsMixin._render_eye draws after the screen and its look (xr_viewer/effects.py:1157-1225; _render_fps_overlay and
_render_keyboard, xr_viewer/overlay.py:81-249, 1427-1510): unit quads (+-1, +-1, 0, 1) under an affine model matrix, textured
(_WORLD_VERT + _OVERLAY_FRAG, xr_viewer/glsl.py:3-13, 28-40) or solid (_SOLID_VERT + _SOLID_FRAG, glsl.py:97-112), blended
SRC_ALPHA / ONE_MINUS_SRC_ALPHA (alpha included) or not, depth-tested LESS against a depth buffer that holds the screen's NDC z (1.0
where the screen does not cover) and written or not.

render() takes the destination image as an input and a number type T: float64 is the reference the tests compare with, float32 the
same expressions in the kernel's precision and order (a table formed in float64 and rounded once, products summed left to right, no
contraction).  tests/test_xr_panels_oracle.py holds the float64 form to renders of the reference's own shaders
(tests/golden/xr_panels.npz).
"""
from __future__ import annotations

import numpy as np

import xr_eye_ref as X

DEPTH_STEPS = 2.0        # near-tie: NDC depths closer than this many 24-bit steps of the window depth (one step = 2^-23 in NDC)


def panel_facet(model):
    """The unit quad under model [4,4] as a facet (p00, p10, p01, uv00, uv10, uv01): its own coordinates (a, b) ARE its uv."""
    m = np.asarray(model, np.float64).reshape(4, 4)
    c = lambda x, y: (m @ np.array([x, y, 0.0, 1.0]))[:3]
    return (c(-1, -1), c(1, -1), c(-1, 1), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))


def corners_clip(model, vp):
    m, vp = np.asarray(model, np.float64).reshape(4, 4), np.asarray(vp, np.float64).reshape(4, 4)
    return np.array([vp @ m @ np.array([x, y, 0.0, 1.0]) for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1))])


def pixel_box(model, vp, w, h):
    """The library's pixel box of a panel on an eye image, (x0, y0, x1, y1) half-open, or None: every vertex behind the eye or
    nothing on the image.  The projected corners' bounds grown by one pixel, clamped."""
    c = corners_clip(model, vp)
    if (c[:, 3] <= 1e-6).all():
        return None
    assert (c[:, 3] > 1e-6).all(), "the panel crosses the eye plane"
    px, py = (c[:, 0] / c[:, 3] + 1.0) * 0.5 * w, (1.0 - c[:, 1] / c[:, 3]) * 0.5 * h
    x0, y0 = int(max(0.0, np.floor(px.min()) - 1.0)), int(max(0.0, np.floor(py.min()) - 1.0))
    x1, y1 = int(min(float(w), np.ceil(px.max()) + 1.0)), int(min(float(h), np.ceil(py.max()) + 1.0))
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


def _grid(w, h, T):
    return np.meshgrid((np.arange(h, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(w, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")


def screen_depth(facets, vp, w, h, T=np.float64):
    """(z [h,w] T: the screen's NDC depth, 1 where it does not cover; covered [h,w]) -- the eye views' cover rule (xr_eye_ref.eye_uv)."""
    t = X._rows(X.facet_table(facets, vp, w, h), T)
    yc, xc = _grid(w, h, T)
    bz = np.full((h, w), 1.0, T)
    for f in range(t.shape[0]):
        r = t[f]
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        z = r[9] * xc + r[10] * yc + r[11]
        ne = r[18] * xc + r[19] * yc + r[20]
        hit = (na >= 0) & (ne >= 0) & (nb >= 0) & (nb <= nw) & (nw > 0) & (z >= -1) & (z < bz)
        bz = np.where(hit, z, bz)
    return bz, bz < 1


def texture(tex, u, v, wrap, T):
    """One GL_LINEAR tap of an RGBA8 picture [h,w,4] whose row 0 is the TOP row (GL's v = 1) -> (rgb in levels [n,3], alpha 0..1 [n])."""
    th, tw = tex.shape[:2]
    x, y = u * T(tw) - T(0.5), (T(1) - v) * T(th) - T(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf).astype(T)[:, None], (y - yf).astype(T)[:, None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    if wrap == "repeat":
        x0, x1, y0, y1 = np.mod(x0, tw), np.mod(x1, tw), np.mod(y0, th), np.mod(y1, th)
    else:
        x0, x1, y0, y1 = np.clip(x0, 0, tw - 1), np.clip(x1, 0, tw - 1), np.clip(y0, 0, th - 1), np.clip(y1, 0, th - 1)
    t = tex.astype(T)
    a, b, c, d = t[y0, x0], t[y0, x1], t[y1, x0], t[y1, x1]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    s = (top + (bot - top) * fy).astype(T)
    return s[:, :3], (s[:, 3] * T(np.float32(1.0) / np.float32(255.0))).astype(T)


def render(dst, facets, vp, w, h, panels, textures, wrap="repeat", T=np.float64):
    """dst [h,w,4] (rgb in levels 0..255, alpha 0..1; for 3 channels pass alpha 1 and ignore it) with the panels drawn over it in
    order -> (out [h,w,4] T, info).  panels: dicts with model [4,4], texture (index or None), color, alpha, depth_test, depth_write,
    blend.  info: screen [h,w] bool; passed [n,h,w] bool (the panel covers the pixel and passes its depth test); z [n,h,w] the
    panel's depth where its plane is in front of the eye; z0 the screen's depth; tie [h,w]: a panel's depth within DEPTH_STEPS steps
    of the depth it is tested against or of another covering panel's."""
    f32 = np.float32
    out = np.array(dst, T).copy()
    z, cov = screen_depth(facets, vp, w, h, T)
    z0 = z.copy()
    yc, xc = _grid(w, h, T)
    n = len(panels)
    passed, zs, covers = np.zeros((n, h, w), bool), np.full((n, h, w), np.nan), np.zeros((n, h, w), bool)
    tie = np.zeros((h, w), bool)
    eps = DEPTH_STEPS * 2.0 ** -23
    for k, q in enumerate(panels):
        c = corners_clip(q["model"], vp)
        if (c[:, 3] <= 1e-6).all():
            continue
        r = X.facet_table([panel_facet(q["model"])], vp, w, h)[0].astype(T)
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        pz = r[9] * xc + r[10] * yc + r[11]
        cover = (na >= 0) & (nb >= 0) & (na <= nw) & (nb <= nw) & (nw > 0) & (pz >= -1) & (pz <= 1)
        covers[k], zs[k] = cover, pz
        if q["depth_test"]:
            tie |= cover & (np.abs(pz.astype(np.float64) - z.astype(np.float64)) <= eps)
        for j in range(k):
            tie |= cover & covers[j] & (np.abs(pz.astype(np.float64) - zs[j]) <= eps)
        ok = cover & (pz < z) if q["depth_test"] else cover
        passed[k] = ok
        if not ok.any():
            continue
        if q["texture"] is None:
            col = q["color"]
            rgb = np.array([T(f32(col[0]) * f32(255.0)), T(f32(col[1]) * f32(255.0)), T(f32(col[2]) * f32(255.0))], T)[None, :].repeat(int(ok.sum()), 0)
            sa = np.full(int(ok.sum()), T(f32(col[3])), T)
        else:
            rgb, sa = texture(textures[q["texture"]], (na[ok] / nw[ok]).astype(T), (nb[ok] / nw[ok]).astype(T), wrap, T)
            sa = (sa * T(f32(q["alpha"]))).astype(T)
        d = out[ok]
        if q["blend"]:
            ia = (T(1) - sa).astype(T)
            d = np.concatenate([sa[:, None] * rgb + ia[:, None] * d[:, :3], (sa * sa + ia * d[:, 3])[:, None]], 1)
        else:
            d = np.concatenate([rgb, sa[:, None]], 1)
        out[ok] = d.astype(T)
        if q["depth_test"] and q["depth_write"]:
            z = np.where(ok, pz, z)
    return out, dict(screen=cov, passed=passed, z=zs, z0=z0, tie=tie, covers=covers)


def pixel_class(info):
    """[h,w] int64: the screen's coverage plus the set of panels that pass, as one number per pixel."""
    cls = info["screen"].astype(np.int64)
    for k in range(info["passed"].shape[0]):
        cls = cls + (info["passed"][k].astype(np.int64) << (k + 1))
    return cls


def uniform3x3(cls):
    p = np.pad(cls, 1, mode="edge")
    h, w = cls.shape
    ok = np.ones(cls.shape, bool)
    for dy in range(3):
        for dx in range(3):
            ok &= p[dy:dy + h, dx:dx + w] == cls
    return ok


def compared(info):
    """The pixels the tests compare: class uniform on 3 x 3, no depth near-tie (dilated by one pixel: the class rule's own reach)."""
    tie = np.pad(info["tie"], 1, mode="constant")
    h, w = info["tie"].shape
    near = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            near |= tie[dy:dy + h, dx:dx + w]
    return uniform3x3(pixel_class(info)) & ~near


# ---- the cases of tests/golden/xr_panels.json (make_golden_xr_panels.py) ----

def case_textures(c):
    """The case's pictures, uint8 [h,w,4], TOP row first, from its seeds.  Every picture differs in all four corners and along both
    axes, so that a wrong flip, transpose or tap shows: per channel a ramp between four random corner values, a texel checker of
    +-24 levels on red and +-8 levels of noise; alpha a ramp from alpha_lo (left) to 255 (right) with +-6 of noise.  (A renderer
    quantises the bilinear weights to about 1 / 256: a step of s levels between neighbouring texels costs s / 256 levels of
    agreement with it, which is why the steps are kept small.)  "opaque": alpha 255 and full-range random texels instead -- the
    picture whose opposite edges differ by whole ranges, for the wrap."""
    out = []
    for t in c["textures"]:
        rng = np.random.default_rng(t["seed"])
        h, w = t["size"]
        yy, xx = np.mgrid[0:h, 0:w]
        if t.get("opaque"):
            img = rng.integers(0, 256, (h, w, 4)).astype(np.float64)
            img[..., 3] = 255
        else:
            fy, fx = yy / max(h - 1, 1), xx / max(w - 1, 1)
            img = np.empty((h, w, 4))
            for k in range(3):
                c00, c01, c10, c11 = rng.integers(40, 216, 4).astype(np.float64)
                img[..., k] = (c00 * (1 - fx) + c01 * fx) * (1 - fy) + (c10 * (1 - fx) + c11 * fx) * fy + rng.integers(-8, 9, (h, w))
            img[..., 0] += np.where((xx + yy) % 2 == 0, 24, -24)
            img[..., 3] = t["alpha_lo"] + (255 - t["alpha_lo"]) * fx + rng.integers(-6, 7, (h, w))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def case_panels(c):
    return [dict(model=np.array(q["model"], np.float64), texture=q["texture"], color=q["color"], alpha=q["alpha"],
                 depth_test=q["depth_test"], depth_write=q["depth_write"], blend=q["blend"]) for q in c["panels"]]
