"""The panorama background of the OpenXR eye views (d2s_dibr_xr_eyes_panorama) restated in numpy: the reference's
_render_panorama_background (xr_viewer/effects.py:930-1021) and _PANORAMA_FRAG (xr_viewer/glsl.py:57-94) per pixel, the renderer's
implicit LOD by its 2 x 2 quad rule, and the eye image composed over it in _render_eye's order.

Two forms of the pixel's texture coordinate:
  * coord_shader: float64, the shader's own formula over the uniforms the reference RECORDED (float32 inv_proj and inv_view_rot) --
    what tests/test_xr_panorama_oracle.py holds to the SwiftShader renders of tests/golden/xr_panorama.npz;
  * coord_kernel: a float32 emulation of the kernel's arithmetic (csrc/dibr_pano.h) over the library's own ray matrices
    (xr.panorama_rays in float64, the pixel -> NDC map folded in, scaled, rounded to float32 once): no normalisation, and
    atan(y, |(x, z)|) for asin(y / |d|).
The LOD (background(rule="quad")): ONE per 2 x 2 quad of GL window pixels, quads aligned to even window x and y counted from the
bottom-left (row y of an image here is window row h - 1 - y), from the forward differences of the quad's lower-left pixel over x + 1
and window y + 1, of the coordinate that is sampled -- fract(u) included; the three points are evaluated analytically, outside the
image too.  rule="pixel" is the per-pixel analytic-derivative LOD of the unwrapped coordinate, which the renderer does NOT follow: the
oracle test shows that it lies further from the renders.

The rest of the eye image comes from the existing restatements (xr_eye_ref, xr_glow_ref, xr_frost_ref), which take a constant clear
colour.  Every blend of _render_eye is ONE, ONE_MINUS_SRC_ALPHA, so the framebuffer is affine in what it started from:
final = S + background * K with K the product of the (1 - alpha) of what drew over an uncovered pixel (0 under the screen, which
overwrites).  Two runs, clear (0, 0, 0, 0) and (1, 1, 1, 1), give S and K.
"""
import numpy as np

import xr_eye_ref as X
import xr_frost_ref as F
import xr_glow_ref as R


def synth_panorama(h, w, seed):
    """uint8 [h, w, 3]: a few sinusoids (whole cycles in x: the REPEAT seam is smooth) plus a vertical gradient, wide enough to clip
    at 0 and at 255 in places, with noise of +-3 levels.  A plain noise image would turn the renderer's 0.02-level log2 error into
    whole colour levels."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    out = np.empty((h, w, 3))
    for k in range(3):
        v = 118.0 + 80.0 * (y - 0.5) * rng.choice([-1.0, 1.0])
        for _ in range(3):
            cx, cy, ph = int(rng.integers(1, 6)), float(rng.uniform(0.5, 3.0)), float(rng.uniform(0, 2 * np.pi))
            v = v + 45.0 * np.sin(2 * np.pi * (cx * x + cy * y) + ph)
        out[..., k] = v + rng.uniform(-3.0, 3.0, (h, w))
    return np.rint(np.clip(out, 0, 255)).astype(np.uint8)


# ---- the coordinate ----

def coord_shader(inv_proj, inv_view_rot, yaw, flip, w, h):
    """-> coord(x, y) of pixel indices of a w x h image (row 0 the top; any integers, outside the image too) -> (fract(u),
    clamp(v, 0, 1)), float64; glsl.py:81-91 over numpy-convention 4 x 4 matrices."""
    A, V = np.asarray(inv_proj, np.float64), np.asarray(inv_view_rot, np.float64)[:3, :3]

    def coord(x, y):
        nx, ny = (2.0 * x + 1.0) / w - 1.0, 1.0 - (2.0 * y + 1.0) / h
        vh = [A[i, 0] * nx + A[i, 1] * ny + A[i, 2] + A[i, 3] for i in range(4)]
        d = np.stack(vh[:3]) / np.maximum(np.abs(vh[3]), 1e-6)
        d = d / np.sqrt((d * d).sum(0))
        d = np.stack([V[i, 0] * d[0] + V[i, 1] * d[1] + V[i, 2] * d[2] for i in range(3)])
        d = d / np.sqrt((d * d).sum(0))
        u = np.arctan2(d[0], -d[2]) / (2.0 * np.pi) + 0.5 + yaw
        v = 0.5 - np.arcsin(np.clip(d[1], -1.0, 1.0)) / np.pi
        if flip:
            v = 1.0 - v
        return u - np.floor(u), np.clip(v, 0.0, 1.0)
    coord.raw = lambda x, y: _raw_shader(A, V, yaw, flip, w, h, x, y)
    return coord


def _raw_shader(A, V, yaw, flip, w, h, x, y):
    """(u before fract, |dir.y|) at fractional pixel positions: the fixture conditions and the analytic derivative."""
    nx, ny = (2.0 * x + 1.0) / w - 1.0, 1.0 - (2.0 * y + 1.0) / h
    vh = [A[i, 0] * nx + A[i, 1] * ny + A[i, 2] + A[i, 3] for i in range(4)]
    d = np.stack(vh[:3]) / np.maximum(np.abs(vh[3]), 1e-6)
    d = np.stack([V[i, 0] * d[0] + V[i, 1] * d[1] + V[i, 2] * d[2] for i in range(3)])
    d = d / np.sqrt((d * d).sum(0))
    u = np.arctan2(d[0], -d[2]) / (2.0 * np.pi) + 0.5 + yaw
    v = 0.5 - np.arcsin(np.clip(d[1], -1.0, 1.0)) / np.pi
    return u, (1.0 - v if flip else v), np.abs(d[1])


def kernel_matrix(rays, w, h):
    """csrc/dibr_pano.h xr_pano_dev: the caller's NDC (x, y, 1) -> direction matrix with the pixel-centre -> NDC map of a w x h image
    folded in, scaled to a largest entry of 1, float32 [9]."""
    m = np.asarray(rays, np.float64).reshape(3, 3).copy()
    m[:, 0] *= 2.0 / w
    m[:, 1] *= -2.0 / h
    return (m / np.abs(m).max()).astype(np.float32).ravel()


def coord_kernel(rays, yaw, flip, w, h):
    """-> coord(x, y) as coord_shader's, in the kernel's float32 operations (pano_uv, csrc/dibr_pano.h)."""
    T = np.float32
    m = kernel_matrix(rays, w, h)
    yaw32 = T(yaw - np.floor(yaw))
    inv2pi = T(0.15915494309189535)

    def coord(x, y):
        xc = (np.asarray(x).astype(T) + T(0.5)) - T(0.5) * T(w)
        yc = (np.asarray(y).astype(T) + T(0.5)) - T(0.5) * T(h)
        dx, dy, dz = ((m[3 * r] * xc + m[3 * r + 1] * yc) + m[3 * r + 2] for r in range(3))
        u = (np.arctan2(dx, -dz).astype(T) * inv2pi + T(0.5)) + yaw32
        v = T(0.5) - T(2.0) * (np.arctan2(dy, np.sqrt(dx * dx + dz * dz).astype(T)).astype(T) * inv2pi)
        if flip:
            v = T(1.0) - v
        return (u - np.floor(u)).astype(T), np.clip(v, T(0), T(1)).astype(T)
    return coord


# ---- the fetch ----

def _tap_repeat(lev, u, v, T):
    """GL_LINEAR of one level [h, w, 3] (already T) at flat u, v -> [n, 3]: REPEAT in x with the level's own width, CLAMP_TO_EDGE in y."""
    h, w = lev.shape[:2]
    x, y = u * T(w) - T(0.5), v * T(h) - T(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(T)[:, None], (y - y0f).astype(T)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb, ya, yb = x0 % w, (x0 + 1) % w, np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    a, b, c, d = lev[ya, xa], lev[ya, xb], lev[yb, xa], lev[yb, xb]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    return (top + (bot - top) * fy).astype(T)


def background(levels, coord, w, h, exposure, T=np.float64, rule="quad"):
    """The panorama pass over a whole w x h eye image -> dict(rgb [h, w, 3] T in 0..255 (exposure applied, clamped), lam [h, w],
    seam [h, w]: the pixel's quad has fract(u) wrapping inside it, u, v).  levels: R.chain(panorama)."""
    q = len(levels) - 1
    Hp, Wp = levels[0].shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    u, v = coord(x, y)
    qx, qy = x & ~1, h - 1 - ((h - 1 - y) & ~1)
    u00, v00 = coord(qx, qy)
    u10, v10 = coord(qx + 1, qy)
    u01, v01 = coord(qx, qy - 1)
    seam = (np.abs(u10 - u00) > 0.5) | (np.abs(u01 - u00) > 0.5)
    if rule == "quad":
        ax, ay, bx, by = ((u10 - u00) * T(Wp)).astype(T), ((v10 - v00) * T(Hp)).astype(T), ((u01 - u00) * T(Wp)).astype(T), ((v01 - v00) * T(Hp)).astype(T)
    else:                                                      # d / dx and d / d(window y) of the unwrapped coordinate at the pixel itself
        assert T is np.float64 and hasattr(coord, "raw")
        s = 1e-3
        xf, yf = x.astype(np.float64), y.astype(np.float64)
        ua, va, _ = coord.raw(xf - s, yf)
        ub, vb, _ = coord.raw(xf + s, yf)
        uc, vc, _ = coord.raw(xf, yf + s)
        ud, vd, _ = coord.raw(xf, yf - s)
        wrap = lambda d: (d + 0.5) % 1.0 - 0.5
        ax, ay, bx, by = wrap(ub - ua) / (2 * s) * Wp, (vb - va) / (2 * s) * Hp, wrap(ud - uc) / (2 * s) * Wp, (vd - vc) / (2 * s) * Hp
    rho2 = np.maximum((ax * ax + ay * ay).astype(T), (bx * bx + by * by).astype(T))
    with np.errstate(divide="ignore"):
        lam = np.clip((T(0.5) * np.log2(rho2).astype(T)).astype(T), T(0), T(q)).astype(T)
    l0f = np.floor(lam)
    f = (lam - l0f).astype(T).ravel()[:, None]
    l0 = l0f.astype(np.int64).ravel()
    l1 = np.minimum(l0 + 1, q)
    uf, vf = u.astype(T).ravel(), v.astype(T).ravel()
    a, b = np.zeros((uf.size, 3), T), np.zeros((uf.size, 3), T)
    for l in np.unique(np.concatenate([l0, l1])):
        lev = levels[l].astype(T)
        m = l0 == l
        if m.any():
            a[m] = _tap_repeat(lev, uf[m], vf[m], T)
        m = l1 == l
        if m.any():
            b[m] = _tap_repeat(lev, uf[m], vf[m], T)
    rgb = ((a * (T(1) - f) + b * f).astype(T) * T(np.float32(max(exposure, 0.0)))).astype(T)
    return dict(rgb=np.clip(rgb, T(0), T(255)).reshape(h, w, 3), lam=lam, seam=seam, u=u, v=v)


# ---- the eye image ----

def _base(c, e, clear, img, dep, levels, verts, T, lib):
    """The eye image of case c over a constant clear colour, by the existing restatement of its kind -> (framebuffer, class, covered)."""
    w, h = e["size"]
    vp = np.array(e["vp"])
    cc = dict(c, clear=list(clear))
    kw = dict(crop=c["crop"], ipd_uv=c["ipd_uv"], depth_strength=0.1 * c["depth_ratio"], convergence=c["convergence"],
              roll=c["screen"]["roll"], corner_radius=c["corner_radius"])
    if c["kind"] == "frost":
        out, cls, info = F.case_render(cc, e, img, dep, levels, verts, T, mesh=not lib)
        return out, cls, info["covered"]
    if lib:       # the library's own surface: formed in double precision from the screen's numbers (csrc/dibr_xr.h xr_surface; the strip's uv float32)
        from desktop2stereo_amd import xr
        sc = xr.XrScreen(**c["screen"])
        strip = sc.curved_verts()
        strip[:, 3:] = strip[:, 3:].astype(np.float32)
        facets = X.facets_flat(sc.model_mat4()) if sc.curve == "flat" else X.facets_strip(strip, sc.curve == "vertical")
    else:         # the reference's: its recorded float32 model matrix or strip
        facets = X.facets_flat(np.array(c["screen_model"])) if c["screen"]["curve"] == "flat" else \
            X.facets_strip(np.array(c["strip"]), c["screen"]["curve"] == "vertical")
    if c["kind"] == "glow":
        g = c["glow"]
        out, cls = R.render_eye(img, dep, levels, facets, vp, w, h, e["eye"], clear, c["screen"]["width"], c["screen"]["height"], g["mode"],
                                g["range_m"], g["inner_edge_fraction"], T=T, **kw)
        return out, cls, (cls == R.SCREEN) | (cls == R.SCREEN_INNER)
    out, cov = X.render_eye(img, dep, facets, vp, w, h, e["eye"], clear, T=T, **kw)
    return out, cov.astype(np.int64), cov


def case_coord(c, e, lib):
    """coord(x, y) of a manifest case's eye: the shader's over the recorded uniforms, or (lib) the kernel's over xr.panorama_rays."""
    w, h = e["size"]
    p = c["panorama"]
    if lib:
        from desktop2stereo_amd import xr
        return coord_kernel(xr.panorama_rays(np.array(e["proj"]), np.array(e["view"])), p["yaw_offset_deg"] / 360.0, p["flip_y"], w, h)
    return coord_shader(np.array(e["u_inv_proj"]), np.array(e["u_inv_view_rot"]), e["u_yaw_offset"], p["flip_y"], w, h)


def case_render(c, e, img, dep, levels, pano_levels, verts=None, T=np.float64, lib=False, rule="quad"):
    """A manifest case's eye -> (framebuffer [h, w, 4] T: rgb 0..255, alpha 0..1; class [h, w]; info dict(covered, lam, seam, bg, K)).
    lib False: float64 over the reference's recorded matrices; lib True: the library's geometry and, with T float32, the kernel's
    arithmetic for the panorama."""
    w, h = e["size"]
    out0, cls, cov = _base(c, e, (0.0, 0.0, 0.0, 0.0), img, dep, levels, verts, T, lib)
    out1, _, _ = _base(c, e, (1.0, 1.0, 1.0, 1.0), img, dep, levels, verts, T, lib)
    K = (out1[..., 3] - out0[..., 3]).astype(T)
    bg = background(pano_levels, case_coord(c, e, lib), w, h, c["panorama"]["exposure"], T, rule)
    bg4 = np.concatenate([bg["rgb"], np.ones((h, w, 1), T)], -1)
    out = (out0 + bg4 * K[..., None]).astype(T)
    return out, cls, dict(covered=cov, lam=bg["lam"], seam=bg["seam"], bg=bg["rgb"], K=K)


uniform3x3 = R.uniform3x3


def case_scene(c):
    """(frame rgb, depth, panorama) of a manifest case."""
    from desktop2stereo_amd import synth
    H, W = c["source"]
    img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
    ph, pw = c["panorama"]["size"]
    return img, dep, synth_panorama(ph, pw, c["panorama"]["seed"])


def golden_eye(z, c, eye):
    """The stored render of a case's eye -> [h, w, 4]: rgb 0..255 to half a level, alpha 0..1; 0 at the pixels that are not stored."""
    rgb = z[f"{c['name']}_{eye}_rgb"].astype(np.float64) + z[f"{c['name']}_{eye}_rgbf"].astype(np.float64) / 2.0
    return np.concatenate([rgb, z[f"{c['name']}_{eye}_a"].astype(np.float64)[..., None] / 65535.0], -1)
