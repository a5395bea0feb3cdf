"""CPU restatement (numpy) of the glow around the CURVED OpenXR screen (d2s_dibr_xr_eyes_glow_curved).  TEST INFRASTRUCTURE ONLY.

Two independent forms:
  * render_eye: a rasteriser of the RECORDED triangles -- the band mesh as the reference's own _build_curved_glow_band_verts wrote it
    (tests/golden/xr_glow_curved.json, make_golden_xr_glow_curved.py) -- over a number type T.  Homogeneous rasterisation: with the
    triangle's clip coordinates as the columns of M = [[x0 x1 x2], [y0 y1 y2], [w0 w1 w2]], b = inverse(M) . (ndc x, ndc y, 1) are the
    perspective-correct barycentrics over clip w; the pixel is inside where every b_i >= 0 and sum b > 0 (in front of the eye), its
    NDC z is sum b_i z_i (kept in [-1, 1]) and its uv sum b_i uv_i / sum b.  No clipping is needed and a triangle that crosses the eye
    plane is handled as GL's clipper handles it.  Every covering triangle is blended in draw order (ONE, ONE_MINUS_SRC_ALPHA, depth
    test off); the strip is xr_eye_ref's (depth test LESS, blending off: it overwrites); the inner vertices follow for mode 1.  It
    knows nothing of the library's 52 pieces.
  * search_eye: the kernel's own steps over the piece table (desktop2stereo_amd/xr.py XrScreen.glow_pieces -> xr_eye_ref.facet_table,
    rounded to T with the library's shared seams): the two arc-end seams, the binary search over the interior seams, the found facet and
    its two neighbours through dibr_xr_eyes' rule, the band on the seams' piece, the inner band's facet and chord draws.
Both shade with xr_eye_ref.shade and xr_glow_ref.glow_frag.
"""
from __future__ import annotations

import numpy as np

import xr_eye_ref as X
import xr_glow_ref as R

NONE, OUTER, SCREEN, SCREEN_INNER = R.NONE, R.OUTER, R.SCREEN, R.SCREEN_INNER
N = 48
T0, T1, C0, C1, ARC = 48, 49, 50, 51, -1
N_OUTER_QUADS, N_INNER_QUADS = 24 * 4 + N * 4, N * 4


def quad_pieces(vertical):
    """The piece every quad of the mesh is claimed to lie on, in the mesh's order (_build_curved_glow_band_verts:392-404): 0 .. 47 a
    facet's plane, T0 / T1 a tangent plane, C0 / C1 a chord plane, ARC: one of the 48 chords of a vertical curve's long inner bands,
    which start at strip coordinate e_al, not at a facet seam, and lie within radius * (1 - cos(step / 2)) of the facets."""
    f = list(range(N))
    if not vertical:
        outer = [T0] * 24 + f + [T1] * 24 + [T0] * 24 + f + [T1] * 24 + [T0] * N + [T1] * N
        inner = f + f + [C0] * N + [C1] * N
    else:
        outer = [T0] * (24 + N + 24) + [T1] * (24 + N + 24) + f + f
        inner = [C0] * N + [C1] * N + [ARC] * N + [ARC] * N
    return outer + inner


def piece_table(screen, glow, vp, w, h):
    """[52, 21] float64 rows in xr_eye_ref.facet_table's layout (mode "glow2": the chord rows cover nothing), uv = (ga, gb)."""
    pcs = screen.glow_pieces(glow)
    tab = X.facet_table([(p[1], p[2], p[3], p[4], p[5], p[6]) for p in pcs], vp, w, h)
    if glow.mode != "glow":
        tab[C0:] = np.array([0, 0, -1.0] + [0.0] * 18)
    return tab


def _grid(w, h, T):
    return np.meshgrid((np.arange(h, dtype=T) + T(0.5)) - T(0.5) * T(h), (np.arange(w, dtype=T) + T(0.5)) - T(0.5) * T(w), indexing="ij")


def glow_keep(ga, gb, U, inner_only, T=np.float64):
    """Whether _GLOW_FRAG draws at the screen coordinates (ga, gb): xr_glow_ref.glow_frag's tests without its texture reads."""
    f32 = np.float32
    half_x, half_y, inner_w, inner_h = T(f32(U["half"][0])), T(f32(U["half"][1])), T(f32(U["inner_w"])), T(f32(U["inner_h"]))
    inv_range, inner = max(T(f32(U["inv_range"])), T(f32(0.001))), max(T(f32(U["inner"])), T(0))
    with np.errstate(all="ignore"):
        cx, cy = (ga.astype(T) - T(0.5)) * inner_w, (gb.astype(T) - T(0.5)) * inner_h
        sd = np.maximum(np.abs(cx) - half_x, np.abs(cy) - half_y)
        if inner_only:
            keep = ~((sd > 0) | (sd < -inner)) if inner > 0 else np.zeros(ga.shape, bool)
            pos = sd + inner
        else:
            keep, pos = sd > 0, sd
        glow = np.power(np.maximum(T(1) - R._smooth01(pos * inv_range, T), T(0)), T(f32(0.58)))
        if inner_only:
            dens = R._smooth01((sd + inner) / max(inner, T(f32(1e-6))), T)
            glow = glow * (dens * dens * (T(3) - T(2) * dens))
        return keep & (glow > T(f32(0.001)))


# ---- the rasteriser of the recorded triangles ----

def tri_rows(verts, vp, w, h):
    """verts [3 n, 5] = x y z u v (TRIANGLES) -> (B [n,3,3]: b = B @ (xc, yc, 1); Z [n,3]: NDC z = Z . b; UV [n,3,2]); a triangle seen
    edge-on covers nothing (B = 0)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 5)
    vp = np.asarray(vp, np.float64).reshape(4, 4)
    clip = np.einsum("rc,ntc->ntr", vp, np.concatenate([v[..., :3], np.ones(v.shape[:2] + (1,))], -1))      # [n, 3 vertices, 4]
    M = np.stack([clip[..., 0] * (w / 2.0), clip[..., 1] * (-h / 2.0), clip[..., 3]], 1)                    # [n, 3 rows, 3 vertices]
    det = np.linalg.det(M)
    ok = np.abs(det) > 1e-14 * np.abs(M).max((1, 2)) ** 3
    B = np.zeros_like(M)
    B[ok] = np.linalg.inv(M[ok])
    return B, clip[..., 2], v[..., 3:]


def raster(B, Z, UV, xc, yc):
    """The triangles covering each point, in draw order: yields (point index [m], triangle index [m], u [m], v [m]) per layer (the
    k-th covering triangle of every point that has one)."""
    xc, yc, n = xc.ravel(), yc.ravel(), B.shape[0]
    for at in range(0, xc.size, 4096):                      # (chunks of points: b is [n, 3, points])
        P = np.stack([xc[at:at + 4096], yc[at:at + 4096], np.ones(xc[at:at + 4096].size)])
        b = (B.reshape(n * 3, 3) @ P).reshape(n, 3, -1)
        s = b.sum(1)
        with np.errstate(all="ignore"):
            z = np.einsum("nt,ntp->np", Z, b)
            inside = (b >= 0).all(1) & (s > 0) & (z >= -1) & (z <= 1)
        while inside.any():
            pts = np.nonzero(inside.any(0))[0]
            tri = inside[:, pts].argmax(0)
            bb = b[tri, :, pts]                             # [m, 3]
            uv = np.einsum("mt,mtc->mc", bb, UV[tri]) / s[tri, pts][:, None]
            yield pts + at, tri, uv[:, 0], uv[:, 1]
            inside[tri, pts] = False


def _to_screen(u, v, U):
    """The glow's uv -> the screen's coordinates (ga, gb), which glow_frag takes."""
    return (u - 0.5) / U["inner_w"] + 0.5, (v - 0.5) / U["inner_h"] + 0.5


def classes(verts, n_outer, n_inner, strip_facets, vp, w, h, U, mode, xc=None, yc=None):
    """Region class and the quad that decided it at the points (xc, yc) (default: every pixel centre of a w x h image), float64:
    -> (cls, quad): quad = the FIRST outer quad that drew (OUTER), the facet (SCREEN), the LAST inner quad that drew (SCREEN_INNER)."""
    if xc is None:
        yc, xc = _grid(w, h, np.float64)
    shape = xc.shape
    tab = X._rows(X.facet_table(strip_facets, vp, w, h), np.float64)
    cov, facet = _strip_cover(tab, xc.ravel(), yc.ravel())
    cls, quad = np.where(cov, SCREEN, NONE), np.where(cov, facet, -1)
    B, Z, UV = tri_rows(verts, vp, w, h)
    no = n_outer // 3
    for pts, tri, u, v in raster(B[:no], Z[:no], UV[:no], xc, yc):
        keep = glow_keep(*_to_screen(u, v, U), U, False) & ~cov[pts] & (cls[pts] == NONE)
        cls[pts[keep]], quad[pts[keep]] = OUTER, tri[keep] // 2
    if mode == 1:
        for pts, tri, u, v in raster(B[no:], Z[no:], UV[no:], xc, yc):
            keep = glow_keep(*_to_screen(u, v, U), U, True) & cov[pts]
            cls[pts[keep]], quad[pts[keep]] = SCREEN_INNER, no // 2 + tri[keep] // 2
    return cls.reshape(shape), quad.reshape(shape)


def _strip_cover(t, xc, yc):
    """dibr_xr_eyes' rule at flat points, float64 rows t (shared seams) -> (covered, facet)."""
    bz, best = np.full(xc.shape, 1.0), np.full(xc.shape, -1, np.int64)
    for f in range(N):
        r = t[f]
        na, nb, nw = r[0] * xc + r[1] * yc + r[2], r[3] * xc + r[4] * yc + r[5], r[6] * xc + r[7] * yc + r[8]
        z, ne = r[9] * xc + r[10] * yc + r[11], r[18] * xc + r[19] * yc + r[20]
        hit = (na >= 0) & (ne >= 0) & (nb >= 0) & (nb <= nw) & (nw > 0) & (z >= -1) & (z < bz)
        bz, best = np.where(hit, z, bz), np.where(hit, f, best)
    return best >= 0, best


def _blend(dst, src):
    return src + dst * (1 - src[:, 3:4])


def render_eye(rgb, dep, levels, verts, n_outer, n_inner, strip_facets, vp, w, h, eye, clear, U, mode, crop=(0.0, 0.0, 1.0, 1.0), T=np.float64,
               **shade_kw):
    """One eye image from the recorded mesh -> (framebuffer [h,w,4]: rgb 0..255, alpha 0..1; region class [h,w])."""
    yc, xc = _grid(w, h, np.float64)
    screen, cov = X.render_eye(rgb, dep, strip_facets, vp, w, h, eye, clear, crop=crop, T=T, **shade_kw)
    out = np.empty((h * w, 4), np.float64)
    out[...] = [np.float32(clear[0]) * 255.0, np.float32(clear[1]) * 255.0, np.float32(clear[2]) * 255.0, np.float32(clear[3])]
    cls = np.full(h * w, NONE)
    B, Z, UV = tri_rows(verts, vp, w, h)
    no = n_outer // 3
    for pts, tri, u, v in raster(B[:no], Z[:no], UV[:no], xc, yc):
        keep, src = R.glow_frag(levels, *_to_screen(u, v, U), U, crop, False, T)
        out[pts[keep]] = _blend(out[pts[keep]], src[keep].astype(np.float64))
        cls[pts[keep]] = OUTER
    c = cov.ravel()
    out[c], cls[c] = screen.reshape(-1, 4)[c], SCREEN
    if mode == 1:
        for pts, tri, u, v in raster(B[no:], Z[no:], UV[no:], xc, yc):
            keep, src = R.glow_frag(levels, *_to_screen(u, v, U), U, crop, True, T)
            out[pts[keep]] = _blend(out[pts[keep]], src[keep].astype(np.float64))
            cls[pts[keep]] = np.where(c[pts[keep]], SCREEN_INNER, OUTER)
    return out.reshape(h, w, 4), cls.reshape(h, w)


# ---- the kernel's search ----

def search(tab, vertical, e_al, e_ac, mode, xc, yc, T=np.float32):
    """The kernel's steps at the points (xc, yc) over the 52-row table `tab` (float64, rounded to T here) ->
    dict(best: the screen's facet or -1; piece: the band's piece (best < 0) or -1; plane: it is drawn; ga, gb: the band's or the
    screen's point; fband, cband: the inner band's facet / chord draw; ca, cb: the chord's point)."""
    t = tab.astype(T)
    live = ~((t[:, 0] == 0) & (t[:, 1] == 0) & (t[:, 2] == -1))
    for f in range(N - 1):
        if live[f] and live[f + 1]:
            t[f, 18:21] = -t[f + 1, 0:3]
    seams = np.concatenate([t[:N, 0:3], -t[N - 1:N, 18:21]])
    xc, yc = xc.astype(T), yc.astype(T)
    E = lambda s: seams[s, 0] * xc + seams[s, 1] * yc + seams[s, 2]
    row = lambda r, k: r[:, k] * xc + r[:, k + 1] * yc + r[:, k + 2]
    zero = np.zeros(xc.shape, np.int64)
    lo_in, hi_in = E(zero) >= 0, E(zero + N) < 0
    lo, hi = zero.copy(), zero + N
    for _ in range(6):
        mid = (lo + hi) >> 1
        act, ge = hi - lo > 1, E(mid) >= 0
        lo, hi = np.where(act & ge, mid, lo), np.where(act & ~ge, mid, hi)
    f = np.where(lo_in & hi_in, lo, np.where(lo_in, N, np.where(hi_in, -1, -2)))
    best, bz = zero - 1, np.ones(xc.shape, T)
    ba, bb, bw = np.zeros(xc.shape, T), np.zeros(xc.shape, T), np.ones(xc.shape, T)
    plane, band_set, piece = np.zeros(xc.shape, bool), np.zeros(xc.shape, bool), zero - 1
    pz, ga, gb = np.zeros(xc.shape, T), np.zeros(xc.shape, T), np.zeros(xc.shape, T)

    def band(r, idx, na, nb, nw, z, m):
        nonlocal plane, pz, ga, gb, piece
        with np.errstate(all="ignore"):
            m = m & (nw > 0) & (z >= -1) & (z <= 1) & (~plane | (z < pz))
            a, bq = (na / nw).astype(T), (nb / nw).astype(T)
            u, v = r[:, 12] + a * r[:, 13] + bq * r[:, 14], r[:, 15] + a * r[:, 16] + bq * r[:, 17]
        plane, pz, piece = plane | m, np.where(m, z, pz), np.where(m, idx, piece)
        ga, gb = np.where(m, u, ga).astype(T), np.where(m, v, gb).astype(T)

    for dc in (-1, 0, 1):
        c = f + dc
        valid = (f >= -1) & (c >= 0) & (c <= N - 1)
        r = t[np.clip(c, 0, N - 1)]
        na, nb, nw, z, ne = row(r, 0), row(r, 3), row(r, 6), row(r, 9), row(r, 18)
        seam_ok = valid & (na >= 0) & (ne >= 0)
        hit = seam_ok & (nb >= 0) & (nb <= nw) & (nw > 0) & (z >= -1) & (z < bz)
        bz, best = np.where(hit, z, bz), np.where(hit, c, best)
        ba, bb, bw = np.where(hit, na, ba), np.where(hit, nb, bb), np.where(hit, nw, bw)
        claim = seam_ok & ~band_set & (f >= 0) & (f < N)
        band_set |= claim
        band(r, c, na, nb, nw, z, claim)
    for idx, m in ((T0, f < 0), (T1, (f == N) | (f == -2))):
        r = np.broadcast_to(t[idx], (xc.size, 21)) if xc.ndim == 1 else t[np.full(xc.shape, idx)]
        band(r, idx, row(r, 0), row(r, 3), row(r, 6), row(r, 9), m)
    scr = best >= 0
    r = t[np.maximum(best, 0)]
    with np.errstate(all="ignore"):
        a, bq = (ba / bw).astype(T), (bb / bw).astype(T)
    sa, sb = (r[:, 12] + a * r[:, 13] + bq * r[:, 14]).astype(T), (r[:, 15] + a * r[:, 16] + bq * r[:, 17]).astype(T)
    fband, cband = np.zeros(xc.shape, bool), np.zeros(xc.shape, bool)
    ca, cb, cidx = np.zeros(xc.shape, T), np.zeros(xc.shape, T), zero - 1
    if mode == 1:
        e_al, e_ac = T(np.float32(e_al)), T(np.float32(e_ac))
        al, ac = (sb, sa) if vertical else (sa, sb)
        edge_ac = (ac <= e_ac) | (ac >= T(1) - e_ac)
        fband = scr & ((edge_ac & (al >= e_al) & (al <= T(1) - e_al)) if vertical else edge_ac)
        cidx = np.where(al < T(0.5), C0, C1)
        rc = t[cidx]
        na, nb, nw, z = row(rc, 0), row(rc, 3), row(rc, 6), row(rc, 9)
        with np.errstate(all="ignore"):
            a2, b2 = (na / nw).astype(T), (nb / nw).astype(T)
            ca, cb = (rc[:, 12] + a2 * rc[:, 13] + b2 * rc[:, 14]).astype(T), (rc[:, 15] + a2 * rc[:, 16] + b2 * rc[:, 17]).astype(T)
            cac = ca if vertical else cb
            cband = scr & (nw > 0) & (z >= -1) & (z <= 1) & (na >= 0) & (na <= nw) & \
                (((cac >= 0) & (cac <= 1)) if vertical else ((cac >= e_ac) & (cac <= T(1) - e_ac)))
    return dict(best=best, piece=np.where(scr, -1, piece), plane=plane & ~scr, ga=np.where(scr, sa, ga), gb=np.where(scr, sb, gb),
                fband=fband, cband=cband, ca=ca, cb=cb, cidx=cidx, vertical=bool(vertical))


def search_classes(s, U, mode, T=np.float32):
    """Region class of search()'s result, and the piece that decided it (SCREEN_INNER: the piece of the last draw, C0 / C1 or the facet)."""
    scr = s["best"] >= 0
    cls = np.where(scr, SCREEN, NONE)
    piece = np.where(scr, s["best"], -1)
    m = s["plane"]
    k = np.zeros(m.shape, bool)
    k[m] = glow_keep(s["ga"][m], s["gb"][m], U, False, T)
    cls, piece = np.where(k, OUTER, cls), np.where(k, s["piece"], piece)
    if mode == 1:
        kf, kc = np.zeros(m.shape, bool), np.zeros(m.shape, bool)
        kf[s["fband"]] = glow_keep(s["ga"][s["fband"]], s["gb"][s["fband"]], U, True, T)
        kc[s["cband"]] = glow_keep(s["ca"][s["cband"]], s["cb"][s["cband"]], U, True, T)
        cls = np.where(kf | kc, SCREEN_INNER, cls)
        last_chord = kc & ~(kf & s["vertical"])            # the draw order: a horizontal curve's chords come last, a vertical one's first
        piece = np.where(last_chord, s["cidx"], piece)
    return cls, piece


def search_eye(rgb, dep, levels, screen, glow, vp, w, h, eye, clear, U, crop=(0.0, 0.0, 1.0, 1.0), T=np.float32, **shade_kw):
    """One eye image as the kernel forms it, over T -> (framebuffer [h,w,4], region class [h,w])."""
    vertical, mode = screen.curve == "vertical", 1 if glow.mode == "glow" else 2
    e_u, e_v = min(0.5, U["inner"] / U["inner_w"]), min(0.5, U["inner"] / U["inner_h"])
    yc, xc = _grid(w, h, T)
    xc, yc = xc.ravel(), yc.ravel()
    s = search(piece_table(screen, glow, vp, w, h), vertical, e_v if vertical else e_u, e_u if vertical else e_v, mode, xc, yc, T)
    out = np.empty((h * w, 4), T)
    out[...] = [T(np.float32(clear[0])) * T(255), T(np.float32(clear[1])) * T(255), T(np.float32(clear[2])) * T(255), T(np.float32(clear[3]))]
    cls = np.full(h * w, NONE)
    m = s["plane"]
    if m.any():
        keep, src = R.glow_frag(levels, s["ga"][m], s["gb"][m], U, crop, False, T)
        i = np.nonzero(m)[0][keep]
        out[i], cls[i] = _blend(out[i], src[keep]).astype(T), OUTER
    scr = s["best"] >= 0
    if scr.any():
        out[scr] = X.shade(rgb, dep, s["ga"][scr], (T(1) - s["gb"][scr]).astype(T), crop, (shade_kw.pop("ipd_uv", 0.064) / 2.0) * (1.0 if eye else -1.0),
                           shade_kw.pop("depth_strength", 0.1), shade_kw.pop("convergence", 0.0), shade_kw.pop("roll", 0.0),
                           shade_kw.pop("corner_radius", 0.0), T=T)
        cls[scr] = SCREEN
    if mode == 1:
        order = (("cband", "ca", "cb"), ("fband", "ga", "gb")) if vertical else (("fband", "ga", "gb"), ("cband", "ca", "cb"))
        for mk, ak, bk in order:
            m = s[mk]
            if m.any():
                keep, src = R.glow_frag(levels, s[ak][m], s[bk][m], U, crop, True, T)
                i = np.nonzero(m)[0][keep]
                out[i], cls[i] = _blend(out[i], src[keep]).astype(T), SCREEN_INNER
    return out.reshape(h, w, 4), cls.reshape(h, w)


# ---- the recorded mesh against the pieces ----

def check_mesh(verts, screen, glow, U):
    """Every recorded quad against the piece it is claimed to lie on (quad_pieces; pieces = screen.glow_pieces) -> dict of maxima:
    plane_m: a vertex's distance from its piece's plane, uv: |recorded glow uv - the piece's affine map there| (both over the quads
    with a piece); arc_m, arc_uv: the same for every vertex of the ARC quads against the facet whose strip range holds it."""
    vertical = screen.curve == "vertical"
    pcs = screen.glow_pieces(glow)
    v = np.asarray(verts, np.float64).reshape(-1, 6, 5)
    ids = quad_pieces(vertical)
    assert v.shape[0] == len(ids) == N_OUTER_QUADS + N_INNER_QUADS, v.shape
    out = dict(plane_m=0.0, uv=0.0, arc_m=0.0, arc_uv=0.0)
    def one(q, pid, km, ku):
        _, p00, p10, p01, g00, g10, g01 = pcs[pid]
        dA, dB = p10 - p00, p01 - p00
        n = np.cross(dA, dB)
        n /= np.linalg.norm(n)
        d = q[:, :3] - p00
        ab = np.linalg.lstsq(np.stack([dA, dB], 1), d.T, rcond=None)[0].T            # [vertices, 2]
        g = np.asarray(g00) + ab[:, :1] * (np.asarray(g10) - g00) + ab[:, 1:] * (np.asarray(g01) - g00)
        uv = 0.5 + (g - 0.5) * np.array([U["inner_w"], U["inner_h"]])
        out[km] = max(out[km], float(np.abs(d @ n).max()))
        out[ku] = max(out[ku], float(np.abs(uv - q[:, 3:]).max()))
    for q, pid in zip(v, ids):
        if pid != ARC:
            one(q, pid, "plane_m", "uv")
            continue
        for vert in q:                                     # each vertex lies on the arc: against the facet under it
            al = (vert[4 if vertical else 3] - 0.5) / (U["inner_h"] if vertical else U["inner_w"]) + 0.5
            one(vert[None], int(np.clip(np.floor(al * N), 0, N - 1)), "arc_m", "arc_uv")
    return out


# ---- the cases of tests/golden/xr_glow_curved.json (make_golden_xr_glow_curved.py) ----

def case_objects(c):
    """(xr.XrScreen, xr.XrGlow, uniforms U, strip facets) of a manifest case."""
    from desktop2stereo_amd import xr
    sc = xr.XrScreen(**c["screen"], clear=tuple(c["clear"]))
    glow = xr.XrGlow("glow" if c["mode"] == 1 else "glow2", c["range_m"], c["inner_edge_fraction"])
    U = uniforms(sc.width, sc.height, c["mode"], c["range_m"], c["inner_edge_fraction"])
    return sc, glow, U, X.facets_strip(np.array(c["strip"]), sc.curve == "vertical")


def uniforms(screen_w, screen_h, mode, range_m, inner_edge_fraction):
    """xr_glow_ref.uniforms as _render_curved_glow:414-423 forms them: inner_uv is NOT zeroed for glow2 (it has no inner pass)."""
    U = R.uniforms(screen_w, screen_h, mode, range_m, inner_edge_fraction)
    U["inner"] = min(U["inner_w"], U["inner_h"]) * max(float(inner_edge_fraction), 0.0)
    return U


def case_render(c, e, verts, img, dep, levels, T=np.float64):
    """verts: the case's recorded triangle list, <case>_verts of xr_glow_curved.npz."""
    sc, glow, U, facets = case_objects(c)
    return render_eye(img, dep, levels, verts, c["draw"]["outer"][0], c["draw"]["inner"][0], facets, np.array(e["vp"]),
                      e["size"][0], e["size"][1], e["eye"], c["clear"], U, c["mode"], T=T, **R.case_kw(c))


def case_search(c, e, img, dep, levels, T=np.float32):
    sc, glow, U, _ = case_objects(c)
    return search_eye(img, dep, levels, sc, glow, np.array(e["vp"]), e["size"][0], e["size"][1], e["eye"], c["clear"], U, T=T,
                      **R.case_kw(c))


def golden_eye(z, c, eye):
    return np.concatenate([z[f"{c['name']}_{eye}_rgb"].astype(np.float64), z[f"{c['name']}_{eye}_a"].astype(np.float64)[..., None] / 255.0], -1)
