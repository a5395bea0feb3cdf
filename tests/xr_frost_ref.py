"""CPU restatement (numpy) of the veil and frosted looks around the flat OpenXR screen (d2s_dibr_xr_eyes_frost).  TEST INFRASTRUCTURE ONLY.

What EffectsMixin._render_flat_frost_with_uniforms draws (xr_viewer/effects.py:789-817) after the screen, in _render_eye's order
(effects.py:1023-1145): four TRIANGLE_STRIPs -- the walls top, bottom, left, right of _build_flat_frost_verts (effects.py:145-187) --
with the depth test off, each fragment blended ONE / ONE_MINUS_SRC_ALPHA on rgb and alpha; programs _FROST_GLOW_VERT with
_FROST_VEIL_FRAG or _FROST_GLOW_FRAG (xr_viewer/glsl.py:668-791).  Two forms:

  * mesh_hits: float64, over the RECORDED vertex arrays (tests/golden/xr_frost.json): every wall is planar, so the pixel's ray meets
    its plane once (a homography, as xr_eye_ref forms the screen's); the point is then looked up among the strip's 128 triangles in the
    plane's own two coordinates and v_uv interpolated barycentrically -- GL's perspective-correct interpolation of a planar triangle
    is affine in the plane's coordinates.  v_local.z is the point's t.  This is what the renders are held to.
  * walk_hits: the library's walk (csrc/dibr.hip XrWalls) over a number type T -- the wall rows of csrc/dibr_xr.h formed in float64 and
    rounded to T, the grid cell from t and the column lines, the triangle from the strip's diagonal, s affine over it.  T = float32 is
    the kernel's arithmetic; T = float64 against mesh_hits shows that the walk IS the mesh.  With it the SCREEN is the library's too (case_render,
    mesh=False): its corners formed in double precision from the screen's numbers, where the float64 restatement keeps the reference's
    recorded float32 model matrix.  The two differ in the eighth digit, which moves float32 table rows by an ulp and with them most
    pixels' texture coordinates: an emulation that starts from the recorded matrix has its worst pixel elsewhere than the kernel.

The shaders run over T with the float32 uniforms GL receives.  hash12 is always float32 in the shader's operation order, every product
and sum rounded on its own: its intermediate values reach 2e4, where float32 resolves 2e-3, so the noise is a function of the cell
only for a fixed order and precision -- the kernel's, and (measured by the oracle test) SwiftShader's.
"""
from __future__ import annotations

import numpy as np

import xr_eye_ref as X
import xr_glow_ref as R

GRID = 8
F32 = np.float32


# ---- geometry ----

def strip_triangles(wall):
    """One wall's TRIANGLE_STRIP [158, 5] = x y t u v -> [n, 3, 5], degenerate triangles (the joins between depth rows) dropped."""
    v = np.asarray(wall, np.float64)
    tri = np.stack([v[:-2], v[1:-1], v[2:]], 1)
    a, t = tri[:, :, _axis(v)], tri[:, :, 2]
    area = (a[:, 1] - a[:, 0]) * (t[:, 2] - t[:, 0]) - (a[:, 2] - a[:, 0]) * (t[:, 1] - t[:, 0])
    return tri[np.abs(area) > 1e-12]


def _axis(v):
    """The wall's long axis in the local frame: 0 (x: top, bottom) or 1 (y: left, right) -- the one the edge t = 0 runs along."""
    e = v[v[:, 2] == 0.0]
    return 0 if np.ptp(e[:, 0]) > np.ptp(e[:, 1]) else 1


def _pixels(w, h, T):
    return np.meshgrid((np.arange(h, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(w, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")


def _plane(p00, p10, p01, vp, w, h, T):
    """The homography of the plane through three world points -> (a, b, clip w > 0, NDC z) per pixel, the table rounded to T."""
    tab = X.facet_table([(p00, p10, p01, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))], vp, w, h)[0].astype(T)
    yc, xc = _pixels(w, h, T)
    na, nb, nw = tab[0] * xc + tab[1] * yc + tab[2], tab[3] * xc + tab[4] * yc + tab[5], tab[6] * xc + tab[7] * yc + tab[8]
    z = tab[9] * xc + tab[10] * yc + tab[11]
    with np.errstate(all="ignore"):
        return (na / nw).astype(T), (nb / nw).astype(T), nw > 0, z


def mesh_hits(verts, model, vp, w, h):
    """float64, over the recorded strips verts [4, 158, 5] and model matrix [4, 4] -> per wall dict(hit [h,w] bool: inside a triangle,
    clip w > 0, NDC z in [-1, 1]; cut [h,w]: inside a triangle with clip w > 0 but beyond the near or far plane; u, v, t [h,w])."""
    m = np.asarray(model, np.float64).reshape(4, 4)
    out = []
    for wall in np.asarray(verts, np.float64):
        ax = _axis(wall)
        e0 = wall[(wall[:, 2] == 0.0)]
        l0 = e0[np.argmin(e0[:, ax])][:3]
        l1 = e0[np.argmax(e0[:, ax])][:3]
        f = wall[wall[:, 2] == 1.0]
        l2 = f[np.argmin(f[:, ax])][:3]
        world = lambda p: (m @ np.append(p, 1.0))[:3]
        a, b, front, z = _plane(world(l0), world(l1), world(l2), vp, w, h, np.float64)
        loc = l0[None, None] + a[..., None] * (l1 - l0) + b[..., None] * (l2 - l0)      # the point in the walls' local frame
        c, t = loc[..., ax], loc[..., 2]
        inside = np.zeros((h, w), bool)
        u, v = np.zeros((h, w)), np.zeros((h, w))
        for tri in strip_triangles(wall):
            (c0, t0), (c1, t1), (c2, t2) = tri[:, [ax, 2]]
            den = (c1 - c0) * (t2 - t0) - (c2 - c0) * (t1 - t0)
            with np.errstate(all="ignore"):
                w1 = ((c - c0) * (t2 - t0) - (c2 - c0) * (t - t0)) / den
                w2 = ((c1 - c0) * (t - t0) - (c - c0) * (t1 - t0)) / den
            w0 = 1.0 - w1 - w2
            k = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & ~inside
            u[k] = (w0 * tri[0, 3] + w1 * tri[1, 3] + w2 * tri[2, 3])[k]
            v[k] = (w0 * tri[0, 4] + w1 * tri[1, 4] + w2 * tri[2, 4])[k]
            inside |= k
        vis = front & (z >= -1) & (z <= 1)
        out.append(dict(hit=inside & vis, cut=inside & front & ~vis, u=u, v=v, t=t))
    return out


def layout(screen, head):
    """(front_depth, front_half_w, front_half_h) in float64 (xr.XrFrost.layout restated: _frost_front_layout, effects.py:120-128)."""
    from desktop2stereo_amd import xr
    return xr.XrFrost(head=tuple(head)).layout(xr.XrScreen(**screen))


def wall_rows(screen, head, vp, w, h):
    """The library's four wall rows (csrc/dibr_xr.h xr_frost_walls) in float64 -> [4, 14]: ha, hb, hw, hz (12), the slope of g(t), and
    which of v_uv's components s is (0: u) with the other's constant in the last column -> [4, 15]."""
    from desktop2stereo_amd import xr
    sc = xr.XrScreen(**screen)
    fd, fhw, fhh = layout(screen, head)
    fx, fy = fhw / max(sc.width * 0.5, 1e-6), fhh / max(sc.height * 0.5, 1e-6)
    Rm, centre = sc.basis()
    M = np.eye(4)
    M[:3, 3] = centre
    M = M @ Rm @ np.diag([sc.width / 2.0, sc.height / 2.0, fd, 1.0])
    world = lambda x, y, z: (M @ np.array([x, y, z, 1.0]))[:3]
    rows = []
    for k in range(4):
        horiz, side = k < 2, (1.0 if k in (0, 3) else -1.0)
        f_ac, f_al = (fy, fx) if horiz else (fx, fy)
        p00 = world(0, side, 0) if horiz else world(side, 0, 0)
        p10 = world(1, side, 0) if horiz else world(side, -1, 0)
        p01 = world(0, side * f_ac, 1) if horiz else world(side * f_ac, 0, 1)
        tab = X.facet_table([(p00, p10, p01, (0.0, 0.0), (1.0, 0.0), (0.0, 1.0))], vp, w, h)[0]
        rows.append(list(tab[:12]) + [f_al - 1.0, 0.0 if horiz else 1.0, 1.0 if k in (1, 3) else 0.0])
    return np.array(rows, np.float64)


def walk_hits(rows, w, h, T):
    """The kernel's walk over T (rows rounded to T first) -> per wall dict(hit, cut, u, v, t)."""
    yc, xc = _pixels(w, h, T)
    out = []
    g8 = T(1.0 / GRID)
    for r64 in rows:
        r = r64.astype(T)
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        z = r[9] * xc + r[10] * yc + r[11]
        with np.errstate(all="ignore"):
            a, t = (na / nw).astype(T), (nb / nw).astype(T)
            slope = r[12]
            gt = (T(1) + slope * t).astype(T)
            inside = (t >= 0) & (t <= 1) & (np.abs(a) <= gt)
            i = np.minimum(np.nan_to_num(t * T(GRID), nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), GRID - 1)
            jf = np.floor((a / gt + T(1)).astype(T) * T(0.5 * GRID))
            j = np.clip(np.nan_to_num(jf, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), 0, GRID - 1)
            t1 = ((i + 1).astype(T) * g8).astype(T)
            g0, g1 = (T(1) + slope * (i.astype(T) * g8)).astype(T), (T(1) + slope * t1).astype(T)
            pj, pj1 = (j.astype(T) * T(2.0 / GRID) - T(1)).astype(T), ((j + 1).astype(T) * T(2.0 / GRID) - T(1)).astype(T)
            xb, xcn = (pj * g1).astype(T), (pj1 * g0).astype(T)
            abc = ((xcn - xb) * (t - t1)).astype(T) + (g8 * (a - xb)).astype(T) <= 0
            s_abc = (j.astype(T) * g8 + (a - pj * gt) / (T(2) * g0)).astype(T)
            s_bcd = ((j + 1).astype(T) * g8 - (pj1 * gt - a) / (T(2) * g1)).astype(T)
        s = np.where(abc, s_abc, s_bcd).astype(T)
        const = np.full((h, w), r[14], T)
        u, v = (const, s) if r[13] != 0 else (s, const)
        front = nw > 0
        vis = front & (z >= -1) & (z <= 1)
        out.append(dict(hit=inside & vis, cut=inside & front & ~vis, u=u, v=v, t=t, s_analytic=((a / gt + T(1)) * T(0.5)).astype(T)))
    return out


# ---- the two fragment programs ----

def hash12(px, py):
    """hash12 (glsl.py:718-722) in float32, the shader's operation order, each operation rounded on its own."""
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    fr = lambda x: (x - np.floor(x)).astype(F32)
    k, c = F32(0.1031), F32(33.33)
    x, y = fr(px * k), fr(py * k)
    z = x
    d = ((x * (y + c)).astype(F32) + (y * (z + c)).astype(F32)).astype(F32) + (z * (x + c)).astype(F32)
    x, y, z = (x + d).astype(F32), (y + d).astype(F32), (z + d).astype(F32)
    return fr(((x + y).astype(F32) * z).astype(F32))


def uniforms(f):
    """The float32 values GL receives, of a manifest case's `frost` dict."""
    return {k: F32(v) for k, v in f.items() if k not in ("mode", "head")}


def sample_uv(u, v, crop, T):
    cx, cy, cw, ch = (T(F32(c)) for c in crop)
    return np.clip(cx + u * cw, T(0), T(1)).astype(T), np.clip(cy + v * ch, T(0), T(1)).astype(T)


def noise_cell(su, sv, U, T):
    """The integer cell hash12 is given: floor((sample_uv + time * (0.011, -0.007)) * noise_scale), the products in float32 as the
    shader forms them."""
    tx, ty = T(F32(U["time"]) * F32(0.011)), T(-F32(U["time"]) * F32(0.007))
    ns = T(U["noise_scale"])
    return np.floor(((su + tx).astype(T) * ns).astype(T)), np.floor(((sv + ty).astype(T) * ns).astype(T))


def _smoothstep(e0, e1, x, T):
    with np.errstate(all="ignore"):
        t = np.clip(((x - e0) / (e1 - e0)).astype(T), T(0), T(1)).astype(T)
    return (t * t * (T(3) - T(2) * t)).astype(T)


def frag(mode, U, crop, levels, u, v, t, T):
    """main() of _FROST_VEIL_FRAG (mode 1) or _FROST_GLOW_FRAG (mode 2) at flat arrays v_uv = (u, v), v_local.z = t ->
    (drawn [n] bool, src [n, 4] = (colour * alpha in 0..255, alpha)).  levels: R.chain(frame); the veil reads levels[0] only."""
    u, v, t = u.astype(T), v.astype(T), t.astype(T)
    su, sv = sample_uv(u, v, crop, T)
    depth = np.clip(t, T(0), T(1)).astype(T)
    beam = np.exp((-depth / max(T(U["beam_softness"]), T(F32(0.001)))).astype(T)).astype(T)
    beam = np.power(np.maximum(beam, T(0)), (T(1) / max(T(U["beam_thickness"]), T(F32(0.1))))).astype(T)
    edge_dist = np.minimum(np.minimum(u, T(1) - u), np.minimum(v, T(1) - v)).astype(T)
    e0 = max(T(U["edge_inset"]), T(F32(0.0001)))
    edge = (T(1) - _smoothstep(e0, (e0 * T(4)), edge_dist, T)).astype(T)
    fa, fi = T(U["alpha"]), T(U["intensity"])
    src = np.zeros((u.size, 4), T)
    if mode == 1:
        alpha = (edge * beam * fa * fi).astype(T)
        keep = alpha > T(F32(0.002))
        alpha = np.minimum(alpha, T(1))
        col = R._level_tap(levels[0].astype(T), su, sv, T)
    else:
        lod = np.full(u.shape, max(T(U["lod"]), T(0)), T)
        col = R.texture_lod(levels, u, v, lod, crop, T)                    # (source_uv there is sample_uv here: the same clamps)
        n = hash12(*noise_cell(su, sv, U, T)).astype(T)
        luma255 = ((col[:, 0] * T(F32(0.2126)) + col[:, 1] * T(F32(0.7152))).astype(T) + col[:, 2] * T(F32(0.0722))).astype(T)
        luma = (luma255 / T(255)).astype(T)
        bright = _smoothstep(T(U["threshold"]), T(1), luma, T)
        scatter = np.maximum(bright, luma * np.clip(T(U["diffuse"]), T(0), T(2)) * T(F32(0.35))).astype(T)
        alpha = (edge * beam * scatter * fa * fi * (T(F32(0.82)) + T(F32(0.30)) * n)).astype(T)
        keep = alpha > T(F32(0.002))
        alpha = np.minimum(alpha, T(1))
        gain = T(F32(0.55)) + T(U["blend"]) * T(F32(0.35))
        col = ((col * T(1.0 - 0.28) + luma255[:, None] * T(F32(0.28))) * gain + col * (bright * T(F32(0.35)))[:, None]).astype(T)
    src[:, :3] = col * alpha[:, None]
    src[:, 3] = alpha
    return keep, src.astype(T)


# ---- one eye ----

def render_eye(rgb_u8_hwc, depth, levels, facets, hits, vp, w, h, eye, clear, frost, crop=(0.0, 0.0, 1.0, 1.0), T=np.float64, **shade_kw):
    """One eye image with the walls of `hits` (mesh_hits or walk_hits) blended in draw order over the screen and the clear colour ->
    (framebuffer [h,w,4] T: rgb 0..255, alpha 0..1; class [h,w] int64; info dict).  class: bit 0 the screen covers, bits 1..4 wall k's
    geometry covers (drawn or discarded), and for frosted the noise cells of the covering walls from bit 5 up: what must be uniform on a
    pixel's 3 x 3 neighbourhood for it to be compared.  frost: the manifest's dict; mode 0 or an undrawn look: the screen alone."""
    out, cov = X.render_eye(rgb_u8_hwc, depth, facets, vp, w, h, eye, clear, crop=crop, T=T, **shade_kw)
    cls = cov.astype(np.int64)
    cells = np.zeros((h, w), np.int64)
    U, mode = uniforms(frost), int(frost["mode"])
    on = mode != 0 and frost["intensity"] > 0 and not (mode == 1 and frost["alpha"] <= 0.002)
    drawn = np.zeros((h, w), np.int64)
    if on:
        for k, wh in enumerate(hits):
            m = wh["hit"]
            if not m.any():
                continue
            cls[m] |= 2 << k
            uu, vv, tt = wh["u"][m].astype(T), wh["v"][m].astype(T), wh["t"][m].astype(T)
            if mode == 2:
                cxs, cys = noise_cell(*sample_uv(uu, vv, crop, T), U, T)
                cell = (cxs.astype(np.int64) + 4096) * 8192 + (cys.astype(np.int64) + 4096)
                cells[m] = (cells[m] * (1 << 26) + cell) % (1 << 56)
            keep, src = frag(mode, U, crop, levels, uu, vv, tt, T)
            dst = out[m]
            dst[keep] = src[keep] + dst[keep] * (T(1) - src[keep, 3:4])
            out[m] = dst
            d = drawn[m]
            d[keep] += 1
            drawn[m] = d
    walls = sum(((cls >> (k + 1)) & 1 for k in range(4)))
    return out.astype(T), cls + 32 * cells, dict(covered=cov, n_walls=walls, drawn=drawn, geom=cls, cells=cells)


uniform3x3 = R.uniform3x3


# ---- the cases of tests/golden/xr_frost.json (make_golden_xr_frost.py) ----

def case_scene(c):
    """(rgb, depth) of a manifest case: synth.dibr_scene, darkened by the case's `dim` (a dark source for the scatter's second branch)."""
    from desktop2stereo_amd import synth
    H, W = c["source"]
    img, dep = synth.dibr_scene(H, W, c["seed"], "boxes")
    if c.get("dim", 1.0) != 1.0:
        img = np.rint(img.astype(np.float64) * c["dim"]).astype(np.uint8)
    return img, dep


def case_kw(c):
    return dict(crop=c["crop"], ipd_uv=c["ipd_uv"], depth_strength=0.1 * c["depth_ratio"], convergence=c["convergence"],
                roll=c["screen"]["roll"], corner_radius=c["corner_radius"])


def case_render(c, e, img, dep, levels, verts, T=np.float64, mesh=True):
    """A manifest case's eye e -> render_eye's result.  mesh: the recorded triangles `verts` (xr_frost.npz <case>_verts) in float64 (T
    must be float64); else the library's walk in T."""
    w, h = e["size"]
    vp = np.array(e["vp"])
    if mesh:      # the reference's own screen: its recorded float32 model matrix
        facets = X.facets_flat(np.array(c["screen_model"]))
    else:         # the library's: formed in double precision from the screen's numbers (csrc/dibr_xr.h xr_surface), as wall_rows forms the walls
        from desktop2stereo_amd import xr
        facets = X.facets_flat(xr.XrScreen(**c["screen"]).model_mat4())
    if mesh:
        assert T is np.float64
        hits = mesh_hits(np.asarray(verts).reshape(4, -1, 5), np.array(c["frost_model"]), vp, w, h)
    else:
        hits = walk_hits(wall_rows(c["screen"], c["frost"]["head"], vp, w, h), w, h, T)
    return render_eye(img, dep, levels, facets, hits, vp, w, h, e["eye"], c["clear"], c["frost"], T=T, **case_kw(c))


def case_stored(c, e, verts, cls):
    """The pixels xr_frost.npz stores: class uniform on 3 x 3 and covered by a wall's geometry (drawn or not)."""
    w, h = e["size"]
    mh = mesh_hits(np.asarray(verts).reshape(4, -1, 5), np.array(c["frost_model"]), np.array(e["vp"]), w, h)
    return uniform3x3(cls) & np.any([m["hit"] for m in mh], 0)


def golden_eye(z, c, eye):
    """The stored render of a case's eye -> [h, w, 4]: rgb 0..255 to 1 / 16 level, alpha 0..1; 0 at the pixels that are not stored."""
    rgb = z[f"{c['name']}_{eye}_rgb"].astype(np.float64) + z[f"{c['name']}_{eye}_rgbf"].astype(np.float64) / 16.0
    return np.concatenate([rgb, z[f"{c['name']}_{eye}_a"].astype(np.float64)[..., None] / 65535.0], -1)
