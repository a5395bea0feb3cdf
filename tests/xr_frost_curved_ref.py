"""CPU restatement (numpy) of the veil and frosted looks around the curved OpenXR screen (d2s_dibr_xr_eyes_frost_curved).  TEST
INFRASTRUCTURE ONLY.

What EffectsMixin._render_curved_frost_with_uniforms draws (xr_viewer/effects.py:759-787) after the curved strip, in _render_eye's
order: ONE TRIANGLES draw of the 588 vertices of _build_curved_frost_verts (effects.py:189-254; 8 floats a vertex: world xyz, v_uv,
v_local), depth test off, every fragment blended ONE / ONE_MINUS_SRC_ALPHA; program _FROST_CURVED_VERT (no model matrix) with the flat
look's _FROST_VEIL_FRAG or _FROST_GLOW_FRAG, which tests/xr_frost_ref.py restates (frag).  Two forms:

  * mesh_hits: float64, over a vertex array [588, 8] (the recorded one, or xr.XrFrost.curved_wall_verts): per triangle the homogeneous
    barycentrics b = inverse([clip x * w / 2, -clip y * h / 2, clip w] of its vertices) @ (xc, yc, 1) = lambda / clip w, as
    tests/xr_glow_curved_ref.py forms them; covered <=> every b >= 0, sum b > 0, -1 <= NDC z <= 1; v_uv and t = sum b * attribute /
    sum b.  It knows nothing of rows, labels or bins.
  * walk_hits: the library's rows (csrc/dibr_xr.h xr_frost_curved_tris) formed in float64 from xr.XrFrost.curved_wall_verts -- a
    triangle (v0, v1, v2) of a quad's first half is labelled (p00, p10, p01) = (v1, v2, v0), of its second half (v2, v1, v0): the edge
    shared with the wall's previous triangle is then p10 - p01 (he), the one shared with the next p00 - p10 (b = 0) -- rounded to T,
    triangle k + 1's he set to the negation of triangle k's hb within a wall, and the kernel's cover rule and interpolation over T.

Both return, per triangle, the flat pixel indices it covers and u, v, t there (sparse: 196 triangles, each a few hundred pixels).
"""
from __future__ import annotations

import numpy as np

import xr_eye_ref as X
import xr_frost_ref as F
import xr_glow_curved_ref as G
import xr_glow_ref as R

N = 48
TRIS = 4 * N + 4
FIRST = (0, 2 * N, 4 * N, 4 * N + 2)                     # the triangles that open a wall
WALL = np.array([0] * (2 * N) + [1] * (2 * N) + [2, 2, 3, 3])
F32 = np.float32


def _grid(w, h, T, box=None):
    x0, y0, x1, y1 = box or (0, 0, w, h)
    return np.meshgrid((np.arange(y0, y1, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(x0, x1, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")


def boxes(verts, vp, w, h, pad=3):
    """Per triangle the pixel box (x0, y0, x1, y1) that holds everything it can cover: the triangle clipped at clip w >= 1e-6 of its
    largest |w| (the walls run past the eye), projected, grown by `pad` pixels; None: wholly behind the eye."""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 8)[..., :3]
    vp = np.asarray(vp, np.float64).reshape(4, 4)
    out = []
    for tri in v:
        c = np.array([vp @ np.append(p, 1.0) for p in tri])
        eps = 1e-6 * np.abs(c[:, 3]).max()
        poly = []
        for i in range(3):
            a, b = c[i], c[(i + 1) % 3]
            if a[3] >= eps:
                poly.append(a)
            if (a[3] >= eps) != (b[3] >= eps):
                s = (eps - a[3]) / (b[3] - a[3])
                poly.append(a + s * (b - a))
        if not poly:
            out.append(None)
            continue
        poly = np.array(poly)
        px, py = (poly[:, 0] / poly[:, 3] + 1) * w / 2.0, (1 - poly[:, 1] / poly[:, 3]) * h / 2.0
        px, py = np.clip(px, -pad, w + pad), np.clip(py, -pad, h + pad)
        box = (int(max(0, np.floor(px.min()) - pad)), int(max(0, np.floor(py.min()) - pad)),
               int(min(w, np.ceil(px.max()) + pad)), int(min(h, np.ceil(py.max()) + pad)))
        out.append(box if box[0] < box[2] and box[1] < box[3] else None)
    return out


def mesh_hits(verts, vp, w, h, bx=None):
    """float64 over verts [588, 8] -> per triangle dict(idx: flat indices of the pixels it covers, u, v, t there; cut: how many pixels
    lie inside it with clip w > 0 but beyond the near or far plane)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 8)
    B, Z, _ = G.tri_rows(v[..., :5].reshape(-1, 5), vp, w, h)
    out = []
    for n in range(v.shape[0]):
        box = (0, 0, w, h) if bx is None else bx[n]
        if box is None or not B[n].any():
            out.append(dict(idx=np.zeros(0, np.int64), u=np.zeros(0), v=np.zeros(0), t=np.zeros(0), cut=0))
            continue
        yc, xc = _grid(w, h, np.float64, box)
        b = np.einsum("ij,jhw->ihw", B[n], np.stack([xc, yc, np.ones_like(xc)]))
        s = b.sum(0)
        z = np.einsum("i,ihw->hw", Z[n], b)
        inside = (b >= 0).all(0) & (s > 0)
        hit = inside & (z >= -1) & (z <= 1)
        yy, xx = np.nonzero(hit)
        at = np.einsum("ic,in->cn", v[n, :, [3, 4, 7]].T, b[:, yy, xx]) / s[yy, xx]
        out.append(dict(idx=(yy + box[1]) * w + xx + box[0], u=at[0], v=at[1], t=at[2], cut=int((inside & ~hit).sum())))
    return out


def lib_rows(screen, head, vp, w, h):
    """The library's 196 triangle rows in float64 -> [196, 24]: ha, hb, hw, hz, he = hw - ha - hb, the v_uv affine (u0, ua, ub, v0, va,
    vb), (t0, ta, tb) -- XrFacet's layout."""
    from desktop2stereo_amd import xr
    v = xr.XrFrost(head=tuple(head)).curved_wall_verts(xr.XrScreen(**screen)).reshape(-1, 3, 8)
    rows = []
    for k, (v0, v1, v2) in enumerate(v):
        p00, p10, p01 = (v1, v2, v0) if k % 2 == 0 else (v2, v1, v0)
        t = X.facet_table([(p00[:3], p10[:3], p01[:3], tuple(p00[3:5]), tuple(p10[3:5]), tuple(p01[3:5]))], vp, w, h)[0]
        dead = t[0] == 0 and t[1] == 0 and t[2] == -1
        he = np.zeros(3) if dead else t[6:9] - t[0:3] - t[3:6]
        rows.append(list(t[:12]) + list(he) + list(t[12:18]) + [p00[7], p10[7] - p00[7], p01[7] - p00[7]])
    return np.array(rows, np.float64)


def link(rows, T, shared=True):
    """The rows rounded to T; shared: within a wall triangle k + 1's he becomes the negation of triangle k's hb where the two point the
    same way (the library's form)."""
    r = rows.astype(T)
    live = ~((r[:, 0] == 0) & (r[:, 1] == 0) & (r[:, 2] == -1))
    if shared:
        for k in range(1, r.shape[0]):
            # (a fold -- the eye between the two triangles' planes -- keeps the triangle's own edge: csrc/dibr_xr.h)
            if k not in FIRST and live[k] and live[k - 1] and -(r[k, 12:15].astype(np.float64) * r[k - 1, 3:6].astype(np.float64)).sum() > 0:
                r[k, 12:15] = -r[k - 1, 3:6]
    return r


def walk_hits(rows, w, h, T, shared=True, bx=None, attrs=True):
    """The kernel's cover rule and interpolation over T -> mesh_hits' result (without cut).  shared=False: every triangle tests its own
    he >= 0 (NOT what the library does: the per-triangle form, kept to show that the watertightness test can fail)."""
    r = link(rows, T, shared)
    out = []
    for k in range(r.shape[0]):
        box = (0, 0, w, h) if bx is None else bx[k]
        if box is None:
            out.append(dict(idx=np.zeros(0, np.int64), u=np.zeros(0, T), v=np.zeros(0, T), t=np.zeros(0, T)))
            continue
        yc, xc = _grid(w, h, T, box)
        q = r[k]
        na, nb, nw = q[0] * xc + q[1] * yc + q[2], q[3] * xc + q[4] * yc + q[5], q[6] * xc + q[7] * yc + q[8]
        z, ne = q[9] * xc + q[10] * yc + q[11], q[12] * xc + q[13] * yc + q[14]
        hit = (na >= 0) & (nb >= 0) & ((ne >= 0) if (k in FIRST or not shared) else (ne > 0)) & (nw > 0) & (z >= -1) & (z <= 1)
        yy, xx = np.nonzero(hit)
        d = dict(idx=(yy + box[1]) * w + xx + box[0])
        if attrs:
            a, b = (na[yy, xx] / nw[yy, xx]).astype(T), (nb[yy, xx] / nw[yy, xx]).astype(T)
            d.update(u=(q[15] + a * q[16] + b * q[17]).astype(T), v=(q[18] + a * q[19] + b * q[20]).astype(T),
                     t=(q[21] + a * q[22] + b * q[23]).astype(T))
        out.append(d)
    return out


def wall_counts(hits, w, h):
    """[4, h, w]: how many triangles of each wall cover each pixel."""
    c = np.zeros((4, h * w), np.int32)
    for k, hk in enumerate(hits):
        np.add.at(c[WALL[k]], hk["idx"], 1)
    return c.reshape(4, h, w)


# ---- one eye ----

def render_eye(rgb, dep, levels, strip_facets, hits, vp, w, h, eye, clear, frost, crop=(0.0, 0.0, 1.0, 1.0), T=np.float64, **shade_kw):
    """One eye image: the curved strip (xr_eye_ref.render_eye), then every covering triangle of `hits` blended in draw order ->
    (framebuffer [h,w,4] T: rgb 0..255, alpha 0..1; class [h,w] int64; info).  class: the screen covers, each wall's hit count, and for
    frosted the noise cells of the covering triangles: what must be uniform on a pixel's 3 x 3 neighbourhood for it to be compared
    (the triangles of one wall share their edges' attributes, so a wall's interior edges are no class boundary)."""
    out, cov = X.render_eye(rgb, dep, strip_facets, vp, w, h, eye, clear, crop=crop, T=T, **shade_kw)
    out = out.reshape(h * w, 4)
    U, mode = F.uniforms(frost), int(frost["mode"])
    on = mode != 0 and frost["intensity"] > 0 and not (mode == 1 and frost["alpha"] <= 0.002)
    counts = wall_counts(hits, w, h)
    cells = np.zeros(h * w, np.int64)
    drawn = np.zeros(h * w, np.int64)
    if on:
        for hk in hits:
            m = hk["idx"]
            if not m.size:
                continue
            uu, vv, tt = hk["u"].astype(T), hk["v"].astype(T), hk["t"].astype(T)
            if mode == 2:
                cxs, cys = F.noise_cell(*F.sample_uv(uu, vv, crop, T), U, T)
                cell = (cxs.astype(np.int64) + 4096) * 8192 + (cys.astype(np.int64) + 4096)
                cells[m] = (cells[m] * (1 << 26) + cell) % (1 << 56)
            keep, src = F.frag(mode, U, crop, levels, uu, vv, tt, T)
            dst = out[m]
            dst[keep] = src[keep] + dst[keep] * (T(1) - src[keep, 3:4])
            out[m] = dst
            drawn[m[keep]] += 1
    geom = cov.astype(np.int64) + 2 * (counts[0] + 4 * counts[1] + 16 * counts[2] + 64 * counts[3]).astype(np.int64)
    cls = geom + 512 * cells.reshape(h, w)
    return out.reshape(h, w, 4).astype(T), cls, dict(covered=cov, geom=geom, n_walls=(counts > 0).sum(0), n_hits=counts.sum(0), counts=counts,
                                                    drawn=drawn.reshape(h, w), cells=cells.reshape(h, w))


uniform3x3 = R.uniform3x3
case_scene = F.case_scene


def load(golden_dir):
    """(npz, manifest) of tests/golden/xr_frost_curved.*, each case given its recorded strip (<case>_strip of the .npz) as c["strip"]."""
    import json
    import os
    z = np.load(os.path.join(golden_dir, "xr_frost_curved.npz"))
    with open(os.path.join(golden_dir, "xr_frost_curved.json")) as f:
        meta = json.load(f)
    for c in meta["cases"]:
        c["strip"] = z[f"{c['name']}_strip"]
    return z, meta
case_kw = F.case_kw
golden_eye = F.golden_eye


def case_render(c, e, img, dep, levels, verts=None, T=np.float64):
    """A manifest case's eye e -> render_eye's result.  verts: the triangles to rasterise in float64 (the recorded ones, or
    curved_wall_verts) behind the recorded strip; None: the library's walk in T from its own double-precision geometry, screen included."""
    from desktop2stereo_amd import xr
    w, h = e["size"]
    vp = np.array(e["vp"])
    sc = xr.XrScreen(**c["screen"])
    facets = X.facets_strip(sc.curved_verts(), sc.curve == "vertical")
    if verts is not None:
        assert T is np.float64
        facets = X.facets_strip(np.array(c["strip"]), sc.curve == "vertical")      # the reference's own screen: its recorded float32 strip
        hits = mesh_hits(verts, vp, w, h)
    else:
        hits = walk_hits(lib_rows(c["screen"], c["frost"]["head"], vp, w, h), w, h, T)
    return render_eye(img, dep, levels, facets, hits, vp, w, h, e["eye"], c["clear"], c["frost"], T=T, **case_kw(c))
