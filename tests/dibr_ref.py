"""Float64 reference of the DIBR warp's fragment shader (FRAGMENT_SHADER.main, viewer.py:533-631; dibr.hip dibr_pixel) with decision
margins, its per-value judge, a float32 emulation in the kernel's forms, and the cases test_cpu_dibr_ref.py and test_gpu_dibr_f64.py
share.  numpy only.  u = 2^-24.

OPERANDS.  What dibr_fill_geom forms in float32 is an operand of the reference, not part of its error: cos / sin of the roll, psx, psy,
half_ipd = (float)(ipd / 2), strength, conv, tol, blur, the crop's four floats, the tables expf(-0.15 i) and expf(-0.2 i); so are the
pixel's own uv ((float)x + 0.5f) / (float)ow and the cropped cx + us * cw (IEEE operations), the feather's fu, fv, and a depth texel:
for a map of another size it is what upsample_depth_kernel stores (frame_ref.upsample in float32), so UpDep and FullDep share one
judge.  Everything after the operands is float64.  (cosf, sinf and expf of the host's libm may differ from numpy's by an ulp: the
bounds below count one u for each.)

BOUNDS, from the kernel's arithmetic; nothing here was measured on the kernel.  A quantity q carries a bound e_q of |float32 q - q|.
 coordinates: a tap at uv coordinate t = a +- k with k a product of n float32 factors: e_t = (n + 1) u |k| + u |t| (+ the bound of a);
   in texels X = t W - 0.5 (a product and a difference): e_X = W e_t + 2 u (|t| W + 0.5).  Rows likewise -- the row coordinate's two
   roundings exist at roll 0 too, so every tap has a rectangle [X +- e_X] x [Y +- e_Y].
 a tap: GL_LINEAR with GL_REPEAT is piecewise bilinear with knots at the integers of (X, Y); its range over the rectangle is taken at the
   rectangle's corners and at the knot lines inside it (3 x 3 points, exact: a bilinear patch has its extrema at its corners; e_X, e_Y <
   0.5 is required, a pixel with more is exempt), then widened by the lerp's own roundings, 10 u max |texel| (three differences, three
   products, three sums, and fx, fy exact).
 depth chain: d = 0.7 d0 + 0.15 dm + 0.15 dp: e_d = 0.7 e_0 + 0.15 (e_m + e_p) + 8 u sum |terms|; shaped = -d (1 + 0.35 (1 - d)):
   e = (1.35 + 0.7 |d|) e_d + 8 u |d| (1.35 + 0.35 |d|); shift = shaped + conv: + u |shift|; fall (two smoothsteps of the operand u): 20 u;
   px = eye_offset shift strength fall: e = |eo strength| (|fall| e_shift + |shift| 20 u) + 4 u |px|; su = u - px c: e = |c| e_px + 2 u |px c|
   + u |su| (one u of the 2 is cosf's), sv likewise.
 smoothstep(e0, e1, x), both the oracle's (x - e0) / (e1 - e0) and the kernel's (x - e0) * (float)(1 / (e1 - e0)): t carries
   (e_x + u |x - e0|) / |e1 - e0| + 3 u |t|, the polynomial has slope <= 1.5 and five roundings on values <= 3: e = 1.5 e_t + 8 u.
 confidence: jump = |dA - dB|: e = e_A + e_B + u |jump|; conf through the smoothstep bound.  Border alpha likewise from e_su, e_sv (the
   kernel's `su < 0.001 || ...` guard is no decision: the smoothsteps are exactly 1 where it skips them).
 sweeps: w = w1[i] (1 + 10 (sdi - cdi)): e_w = w1[i] (10 (e_sdi + e_cdi) + 4 u (1 + 10 |sdi - cdi|)) + 2 u w (expf's ulp and the product);
   w2[i]: 2 u w.  best = sum w col with w in [w - e_w, w + e_w] (>= 0) and col in the tap's range: the interval sum, widened by
   (1 +- 64 u) for up to 24 products and sums; bw likewise, e_bw = sum e_w + 32 u bw.  best / bw 0.5: [lo / (bw + e), hi / (bw - e)];
   the vertical taps add 0.25 col each, vw is exact; the final division and the sums: (1 +- 8 u).
 mix(col, fill, conf): linear in conf, so its range is taken at conf -+ e_conf (clipped to 0..1) with col, fill at their ends; four
   roundings.  feather: fo is a product of four smoothsteps of operands (e = 50 u), sh = powf(fo, 0.7) lies in
   [pow(fo - e, 0.7), pow(fo + e, 0.7)] (1 -+ 16 u).  corner: sdf from operands, e = 10 u, then the smoothstep bound over 0.01.
   Everything after the mix is products of non-negative intervals; the result is widened by (1 +- 16 u) and 2 u 255.
 u8 (v_cvt_pk_u8_f32: nearest-even, saturating; alpha scaled by 255): a byte n is accepted iff ceil(lo - 1/2) <= n <= floor(hi + 1/2)
   with lo, hi clipped to 0..255, so a tie inside the interval admits both bytes.

DECISIONS.  The shader's hard comparisons -- su, sv outside [0, 1]; per sweep tap oob and sdi > cdi + tol; bw > 5, bw < 2, bw > 0.01; the
vertical taps' 0 <= vv <= 1 and vdi > cdi + tol / 2; conf > 0.001 -- are recorded per pixel where |lhs - rhs| <= the bound of the two
sides.  A pixel with none is decided.  A pixel with one or two is evaluated under all outcome combinations of those comparisons (at
most four) and a value matching any one evaluation is accepted; if such an evaluation meets a further undecided comparison the pixel is
exempt, as is a pixel with three or more.  Exempt values must be finite and within [0, 255 (1 + 2^-20)].  Per case: exempt pixels
<= 0.1 % and <= 8; decided + branch-judged >= 99 %.  With u_resolution = the viewport and blur_radius = 2.5 the vertical tap of output
row 2 (and oh - 3) is a tie on vv >= 0 whatever the height: those rows are branch-judged; blur_radius = 2.25 or Half-TAB has no tie.
"""
import itertools

import numpy as np

import frame_ref

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
MODES = ("Half-SBS", "Full-SBS", "Half-TAB", "Full-TAB")
DEFAULTS = dict(ipd_uv=0.064, depth_ratio=1.0, convergence=0.0, roll=0.0, search_radius=12.0, depth_tolerance=0.012, blur_radius=2.5,
                resolution=(0.0, 0.0), feather=False, feather_width=0.02, corner_radius=0.0, viewport=(0.0, 0.0, 0.0, 0.0))
XR_CROPS = [(0.25, 0.1, 0.5, 0.8), (0.025, 0.0, 0.95, 1.0), (0.4, 0.1, 0.6, 0.8), (0.0, 1.0 / 6.0, 1.0, 2.0 / 3.0)]      # test_gpu_xr_crop.py's


# ------------------------------------------------------------------------------------------------ cases and inputs
def case(name, H, W, mode="Full-SBS", crop=None, dhw=None, colors="noise", dscale=1.0, batch=1, seed=0, env=None, expect=None, **kw):
    """expect = (kernel name for u8 output, rows, cols) under the default switches; env: {switch: value} -> expected kernel name, each
    asserted through ops.dibr_warp_plan before the case runs"""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(name=name, H=H, W=W, mode=mode, crop=crop, dhw=dhw or (H, W), colors=colors, dscale=dscale, batch=batch, seed=seed,
                env=env or {}, expect=expect, kw=kw)


def _cases():
    R512, R256 = "dibr_rows<u8,fx=0,512,FullDep>", "dibr_rows<u8,fx=0,256,FullDep>"
    GEN, R0 = "dibr<u8,general,FullDep>", "dibr<u8,roll0,FullDep>"
    sw = {"D2S_DIBR_NO_ROWS=1": R0, "D2S_DIBR_NO_ROLL0=1": GEN}
    c = [
        case("sbs530", 12, 530, expect=(R512, True, 512), env=dict(sw, **{"D2S_DIBR_COLS=256": R256})),      # two blocks, the second ragged
        case("sbs257", 8, 257, expect=(R512, True, 512), seed=1),                 # ow = 257 > 512 / 2: stays one ragged block of 512 ...
        case("sbs256", 8, 256, expect=(R256, True, 256), seed=2),                 # ... ow = 256 takes the halving rule down to 256
        case("wide520", 8, 520, blur_radius=2.25, expect=(R512, True, 512), env={"D2S_DIBR_COLS=1024": "dibr_rows<u8,fx=0,1024,FullDep>"}, seed=3),
        case("wide1030", 6, 1030, blur_radius=2.25, expect=(R512, True, 512), env={"D2S_DIBR_COLS=1024": "dibr_rows<u8,fx=0,1024,FullDep>"}, seed=4),
        case("hsbs", 10, 540, "Half-SBS", expect=(R256, True, 256), env=sw, seed=5),
        case("htab", 12, 530, "Half-TAB", expect=(R512, True, 512), seed=6),        # oh != H: no tie on the vertical taps
        case("ftab", 10, 300, "Full-TAB", expect=(R512, True, 512), seed=7),
        case("batch2", 8, 530, batch=2, blur_radius=2.25, expect=(R512, True, 512), seed=8),
        case("smooth", 12, 530, colors="smooth", expect=(R512, True, 512), seed=9),
        case("dscale4", 10, 530, blur_radius=2.25, dscale=4.0, depth_ratio=5.0, ipd_uv=0.2, expect=(R512, True, 512), env=sw, seed=10),      # shifts beyond the margin
        case("winedge", 10, 700, dscale=4.0, depth_ratio=5.0, ipd_uv=0.2, blur_radius=2.25, expect=(R512, True, 512), seed=26),      # taps at the window's last texel pair
        case("res", 10, 530, resolution=(400.0, 30.0), expect=(R512, True, 512), seed=11),
        case("sr0", 8, 300, search_radius=0.0, expect=(R512, True, 512), seed=12),
        case("sr5_b225", 12, 300, search_radius=5.0, blur_radius=2.25, expect=(R512, True, 512), seed=13),        # tie-free
        case("sr15_tol", 10, 300, search_radius=15.0, depth_tolerance=0.3, expect=(R512, True, 512), seed=14),
        case("parallax", 6, 2400, blur_radius=2.25, ipd_uv=0.5, depth_ratio=20.0, expect=(R0, False, 256), seed=15),      # WW above rows_words: the plan says gather; wrapi's modulo
        case("roll03", 16, 300, roll=0.3, convergence=0.03, expect=(GEN, False, 512), seed=16),
        case("roll12fx", 16, 300, roll=-1.2, feather=True, feather_width=0.1, corner_radius=0.2, viewport=(10.0, 1.0, 270.0, 12.0),
             expect=("dibr<u8,general,FullDep>", False, 512), seed=17),
        case("fx", 16, 530, feather=True, corner_radius=0.03, convergence=0.03, expect=("dibr_rows<u8,fx=1,512,FullDep>", True, 512),
             env={"D2S_DIBR_NO_ROWS=1": R0, "D2S_DIBR_NO_ROLL0=1": GEN}, seed=18),
        case("fxvp", 16, 300, feather=True, feather_width=0.1, corner_radius=0.2, viewport=(10.0, 1.0, 270.0, 12.0),
             expect=("dibr_rows<u8,fx=1,512,FullDep>", True, 512), seed=19),
        case("up5x19", 24, 530, dhw=(5, 19), expect=("dibr_rows<u8,fx=0,512,UpDep>", True, 512),
             env={"D2S_DIBR_NO_ROWS=1": "dibr<u8,roll0,UpDep>", "D2S_DIBR_NO_ROLL0=1": "dibr<u8,general,UpDep>"}, seed=20),
        case("up37x66", 24, 530, dhw=(37, 66), expect=("dibr_rows<u8,fx=0,512,UpDep>", True, 512), seed=21),
        case("upw", 12, 530, dhw=(12, 97), expect=("dibr_rows<u8,fx=0,512,UpDep>", True, 512), seed=22),          # dh = H, dw != W
        case("tiny", 2, 2, expect=(R256, True, 256), seed=23),
        case("h3", 3, 700, blur_radius=2.25, expect=(R512, True, 512), seed=24),
        case("rows270", 270, 96, expect=(R256, True, 256), seed=25),               # the wrong-row class
    ]
    for k, cr in enumerate(XR_CROPS):
        c.append(case(f"crop{k}", 96, 128, crop=cr, corner_radius=0.03 if k % 2 == 0 else 0.0, dhw=(11, 17) if k == 3 else None,
                      expect=(f"dibr_rows<u8,fx={1 if k % 2 == 0 else 0},256,{'UpDep' if k == 3 else 'FullDep'},crop>", True, 256),
                      env={"D2S_DIBR_NO_ROWS=1": f"dibr<u8,roll0,{'UpDep' if k == 3 else 'FullDep'},crop>"} if k in (0, 3) else None, seed=30 + k))
    c.append(case("cropwide", 8, 720, crop=(0.05, 0.0, 0.9, 1.0), expect=("dibr_rows<u8,fx=0,512,FullDep,crop>", True, 512), seed=35))
    return {x["name"]: x for x in c}


CASES = _cases()


def inputs(c):
    """-> rgb uint8 [B,H,W,3], depth float32 [B,dh,dw]: smooth depth with hard-edged boxes inside the image and at its edges"""
    rng = np.random.default_rng(1000 + c["seed"])
    B, H, W = c["batch"], c["H"], c["W"]
    dh, dw = c["dhw"]
    yy, xx = np.meshgrid((np.arange(dh) + 0.5) / dh, (np.arange(dw) + 0.5) / dw, indexing="ij")
    rgbs, deps = [], []
    for b in range(B):
        ph = rng.uniform(0, 6.28, 3)
        d = 0.35 + 0.2 * np.sin(5.0 * xx + ph[0]) * np.cos(3.0 * yy + ph[1]) + 0.1 * np.sin(11.0 * xx * yy + ph[2])
        d[(yy > 0.2) & (yy < 0.7) & (xx > 0.3) & (xx < 0.45)] = 0.93          # a near box inside
        d[(yy > 0.4) & (xx > 0.6) & (xx < 0.68)] = 0.05                       # a far slot down to the bottom edge
        d[(yy > 0.1) & (yy < 0.4) & (xx > 0.6) & (xx < 0.68)] = 0.83            # a near patch right above the slot (the vertical taps' depth test)
        d[(yy < 0.55) & (xx < 0.04)] = 0.85                                   # a near box on the left edge
        d[(yy > 0.3) & (xx > 0.93)] = 0.9                                     # ... and on the right edge
        deps.append((d * c["dscale"]).astype(F32))
        if c["colors"] == "noise":
            rgbs.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        else:
            gy, gx = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
            rgbs.append(np.stack([40 + 180 * gx, 230 - 150 * gy, 128 + 100 * np.sin(9 * gx + 2 * gy)], -1).astype(np.uint8))
    return np.stack(rgbs), np.stack(deps)


def depth_texels(c, depth, mut=None):
    """the H x W depth texture of one frame as float32: the map itself or what upsample_depth_kernel stores"""
    if tuple(depth.shape) == (c["H"], c["W"]):
        return depth.astype(F32)
    return frame_ref.upsample(depth[None].astype(F32), c["H"], c["W"], dt=F32, mut="align_corners" if mut == "updep_align_corners" else None)[0]


def geom(c):
    """the float32 uniforms as dibr_fill_geom and the launcher form them"""
    p = dict(DEFAULTS, **c["kw"])
    H, W, mode, crop = c["H"], c["W"], c["mode"], c["crop"]
    eh, ew = H, W
    g = dict(H=H, W=W, mode=mode, crop=crop is not None)
    if crop is not None:
        x0 = min(max(round(crop[0] * W), 0), W - 1)
        y0 = min(max(round(crop[1] * H), 0), H - 1)
        x1 = max(x0 + 1, min(round((crop[0] + crop[2]) * W), W))
        y1 = max(y0 + 1, min(round((crop[1] + crop[3]) * H), H))
        eh, ew = y1 - y0, x1 - x0
        g.update(cx=F32(crop[0]), cy=F32(crop[1]), cw=F32(crop[2]), ch=F32(crop[3]))
    oh = eh // 2 if mode == "Half-TAB" else eh
    ow = ew // 2 if mode == "Half-SBS" else ew
    roll = F32(p["roll"])
    vp = p["viewport"]
    vp0 = vp[2] == 0 and vp[3] == 0
    g.update(oh=oh, ow=ow, c=F32(np.cos(roll)), s=F32(np.sin(roll)),
             psx=F32(1) / (F32(p["resolution"][0]) if p["resolution"][0] > 0 else F32(W)),
             psy=F32(1) / (F32(p["resolution"][1]) if p["resolution"][1] > 0 else F32(H)),
             half_ipd=F32(p["ipd_uv"] / 2.0), strength=F32(0.1 * p["depth_ratio"]), conv=F32(p["convergence"]), tol=F32(p["depth_tolerance"]),
             blur=F32(p["blur_radius"]), feather_w=F32(p["feather_width"]), search=int(p["search_radius"]), feather=bool(p["feather"]),
             corner_r=F32(p["corner_radius"]), vpx=F32(0 if vp0 else vp[0]), vpy=F32(0 if vp0 else vp[1]), vpw=F32(ow if vp0 else vp[2]),
             vph=F32(oh if vp0 else vp[3]),
             w1=np.array([np.exp(F32(-i * 0.15)) for i in range(16)], F32), w2=np.array([np.exp(F32(-i * 0.2)) for i in range(16)], F32))
    return g


def pixel_uv(g, idx):
    """the operands (us, vs, u, v) of the pixels idx (flat, row-major in the eye viewport), float32"""
    y, x = np.divmod(idx, g["ow"])
    us = ((x.astype(F32) + F32(0.5)) / F32(g["ow"])).astype(F32)
    vs = ((y.astype(F32) + F32(0.5)) / F32(g["oh"])).astype(F32)
    if g["crop"]:
        return us, vs, (g["cx"] + (us * g["cw"]).astype(F32)).astype(F32), (g["cy"] + (vs * g["ch"]).astype(F32)).astype(F32), x, y
    return us, vs, us, vs, x, y


def pack(mode, left, right):
    return np.concatenate([left, right], -2 if mode.endswith("SBS") else -3)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _tex64(img, X, Y):
    """GL_LINEAR + GL_REPEAT at texel coordinates (X, Y) = (u W - 0.5, v H - 0.5), float64; img [H,W] or [H,W,3]"""
    H, W = img.shape[:2]
    x0f, y0f = np.floor(X), np.floor(Y)
    fx, fy = X - x0f, Y - y0f
    x0, y0 = np.mod(x0f.astype(np.int64), W), np.mod(y0f.astype(np.int64), H)
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    a, b, cc, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top, bot = a + (b - a) * fx, cc + (d - cc) * fx
    return top + (bot - top) * fy


def tex_range(img, tu, eu, tv, ev, amax):
    """A tap at uv (tu, tv) whose float32 coordinates are within (eu, ev): -> value, lo, hi (the exact range of the piecewise-bilinear
    blend over the rectangle in texels, widened by the lerp's roundings) and `big` where the rectangle is 0.5 texels or wider"""
    H, W = img.shape[:2]
    X, Y = tu * W - 0.5, tv * H - 0.5
    eX = W * eu + 2 * U * (np.abs(tu) * W + 0.5)
    eY = H * ev + 2 * U * (np.abs(tv) * H + 0.5)
    big = (eX >= 0.5) | (eY >= 0.5)
    eX, eY = np.minimum(eX, 0.49), np.minimum(eY, 0.49)
    xs = np.stack([X - eX, np.clip(np.ceil(X - eX), X - eX, X + eX), X + eX])          # the ends and the knot between them, if any
    ys = np.stack([Y - eY, np.clip(np.ceil(Y - eY), Y - eY, Y + eY), Y + eY])
    v = _tex64(img, xs[:, None], ys[None, :])
    val = _tex64(img, X, Y)
    r = 10 * U * amax
    return val, v.min((0, 1)) - r, v.max((0, 1)) + r, big


def _sstep(e0, e1, x, ex):
    """smoothstep and its bound (both the division and the multiply-by-inverse form)"""
    t = np.clip((x - e0) / (e1 - e0), 0.0, 1.0)
    et = (ex + U * np.abs(x - e0)) / abs(e1 - e0) + 3 * U * t
    return t * t * (3.0 - 2.0 * t), 1.5 * et + 8 * U


# comparison ids
_SU0, _SU1, _SV0, _SV1, _CONF, _BW2, _BW01 = 0, 1, 2, 3, 4, 5, 6
_V = 10            # + 3 t + {0: vv >= 0, 1: vv <= 1, 2: depth}
_P1, _P2 = 100, 300      # + 6 i + {0..3: oob, 4: depth, 5: break}


class _Run:
    """the undecided comparisons of one evaluation over n pixels; flips = (id1, id2, bit1, bit2): outcomes forced per pixel"""
    def __init__(self, n, flips=None):
        self.n, self.flips = n, flips
        self.nund = np.zeros(n, np.int64)
        self.ids = np.full((n, 2), -1, np.int64)
        self.extra = np.zeros(n, bool)

    def cmp(self, cid, w, natural, margin, err, live):
        und = live & (np.abs(margin) <= err)
        if self.flips is None:
            k = w[und]
            first = self.nund[k] == 0
            self.ids[k[first], 0] = cid
            second = self.nund[k] == 1
            self.ids[k[second], 1] = cid
            self.nund[k] += 1
            return natural
        f1, f2, b1, b2 = self.flips
        self.extra[w[und & (f1[w] != cid) & (f2[w] != cid)]] = True
        return natural ^ (((f1[w] == cid) & b1) | ((f2[w] == cid) & b2))


def _eval(g, rgb, dep, eye, idx, run):
    """FRAGMENT_SHADER.main in float64 for the pixels idx of one eye -> colour range [n,3] x 2, alpha range [n] x 2, big [n]"""
    H, W = g["H"], g["W"]
    n = idx.size
    alln = np.arange(n)
    us, vs, u32, v32, px_x, px_y = pixel_uv(g, idx)
    us, vs, u, v = us.astype(F64), vs.astype(F64), u32.astype(F64), v32.astype(F64)
    c, s, psx, psy = float(g["c"]), float(g["s"]), float(g["psx"]), float(g["psy"])
    rolled = s != 0.0
    eo = float(g["half_ipd"]) * (1.0 if eye else -1.0)
    sg = float(np.sign(eo))
    parx, pary = c * sg, s * sg
    sweep = -1.0 if eo > 0 else 1.0
    strength, conv, tol, blur = float(g["strength"]), float(g["conv"]), float(g["tol"]), float(g["blur"])
    dmax, cmax = float(np.abs(dep).max()), 255.0
    big = np.zeros(n, bool)

    def off(a, k, nf):          # the coordinate a + k, k a product of nf float32 factors (one more u: cosf / sinf)
        t = a + k
        return t, ((nf + 1) * U * np.abs(k) + U * np.abs(t)) * (k != 0)

    def dtap(tu, eu, tv, ev, w=None):
        val, lo, hi, b = tex_range(dep, tu, eu, tv, ev, dmax)
        if w is None:
            big[:] |= b
        else:
            big[w] |= b
        return val, np.maximum(hi - val, val - lo)

    # 3-tap smoothing, shaping, shift
    dsx, dsy = parx * psx * 1.5, pary * psy * 1.5
    d0, e0 = dtap(u, 0.0, v, 0.0)
    (um, eum), (vm, evm) = off(u, -dsx, 3), off(v, -dsy, 3)
    (up, eup), (vp, evp) = off(u, dsx, 3), off(v, dsy, 3)
    dm, em = dtap(um, eum, vm, evm)
    dp, ep = dtap(up, eup, vp, evp)
    d = 0.7 * d0 + 0.15 * dm + 0.15 * dp
    e_d = 0.7 * e0 + 0.15 * (em + ep) + 8 * U * (0.7 * np.abs(d0) + 0.15 * np.abs(dm) + 0.15 * np.abs(dp))
    shaped = -d * (1.0 + 0.35 * (1.0 - d))
    e_sh = (1.35 + 0.7 * np.abs(d)) * e_d + 8 * U * np.abs(d) * (1.35 + 0.35 * np.abs(d))
    shift = shaped + conv
    e_shift = e_sh + U * np.abs(shift)
    fall = _sstep(0.0, float(F32(0.05)), u, 0.0)[0] * _sstep(1.0, float(F32(0.95)), u, 0.0)[0]
    px = eo * shift * strength * fall
    e_px = abs(eo * strength) * (fall * e_shift + np.abs(shift) * 20 * U) + 4 * U * np.abs(px)
    su, sv = u - px * c, v - px * s
    e_su = abs(c) * e_px + 2 * U * np.abs(px * c) + U * np.abs(su)
    e_sv = (abs(s) * e_px + 2 * U * np.abs(px * s) + U * np.abs(sv)) * rolled
    live = np.ones(n, bool)
    oob = (run.cmp(_SU0, alln, su < 0, su, e_su, live) | run.cmp(_SU1, alln, su > 1, su - 1, e_su, live)
           | run.cmp(_SV0, alln, sv < 0, sv, e_sv, live) | run.cmp(_SV1, alln, sv > 1, sv - 1, e_sv, live))
    s2x, s2y = parx * psx * 2.0, pary * psy * 2.0
    (ua, eua), (va_, eva) = off(u, -s2x, 3), off(v, -s2y, 3)
    (ub, eub), (vb, evb) = off(u, s2x, 3), off(v, s2y, 3)
    dA, eA = dtap(ua, eua, va_, eva)
    dB, eB = dtap(ub, eub, vb, evb)
    jump = np.abs(dA - dB)
    conf, e_conf = _sstep(float(F32(0.04)), float(F32(0.10)), jump, eA + eB + U * jump)
    conf, e_conf = np.where(oob, 1.0, conf), np.where(oob, 0.0, e_conf)
    _, clo, chi, b = tex_range(rgb, su, e_su, sv, e_sv, cmax)
    big |= b
    m = run.cmp(_CONF, alln, conf > 0.001, conf - 0.001, e_conf, ~oob)
    if m.any():
        w = np.nonzero(m)[0]
        flo, fhi = _inpaint(g, rgb, dep, u[w], v[w], -d[w], e_d[w], parx, pary, sweep, w, run, big, dtap, cmax)
        c_lo, c_hi = np.clip(conf[w] - e_conf[w], 0, 1)[:, None], np.clip(conf[w] + e_conf[w], 0, 1)[:, None]
        lo = np.minimum(clo[w] * (1 - c_lo) + flo * c_lo, clo[w] * (1 - c_hi) + flo * c_hi)
        hi = np.maximum(chi[w] * (1 - c_lo) + fhi * c_lo, chi[w] * (1 - c_hi) + fhi * c_hi)
        clo[w], chi[w] = lo * (1 - 4 * U), hi * (1 + 4 * U)
    # border alpha
    bx0, ebx0 = _sstep(-0.001, 0.001, su, e_su)
    bx1, ebx1 = _sstep(1.001, 0.999, su, e_su)
    by0, eby0 = _sstep(-0.001, 0.001, sv, e_sv)
    by1, eby1 = _sstep(1.001, 0.999, sv, e_sv)
    bx, by = bx0 * bx1, by0 * by1
    ebx, eby = ebx0 + ebx1 + 2 * U, eby0 + eby1 + 2 * U
    alo, ahi = np.minimum(bx - ebx, by - eby), np.minimum(bx + ebx, by + eby)
    if g["feather"]:
        fu = (((px_x.astype(F32) + F32(0.5)) - g["vpx"]).astype(F32) / g["vpw"]).astype(F64)
        fv = (((F32(g["oh"]) - (px_y.astype(F32) + F32(0.5))).astype(F32) - g["vpy"]).astype(F32) / g["vph"]).astype(F64)
        fw = float(g["feather_w"])
        fo = _sstep(0, fw, fu, 0.0)[0] * _sstep(0, fw, 1 - fu, U)[0] * _sstep(0, fw, fv, 0.0)[0] * _sstep(0, fw, 1 - fv, U)[0]
        e_fo = 50 * U + 4 * 1.5 * 2 * U / fw
        sh_lo = np.power(np.clip(fo - e_fo, 0, 1), 0.7) * (1 - 16 * U)
        sh_hi = np.power(np.clip(fo + e_fo, 0, 1), 0.7) * (1 + 16 * U)
        clo, chi = clo * sh_lo[:, None], chi * sh_hi[:, None]
    if g["corner_r"] > 0:
        r = float(g["corner_r"])
        dx, dy = np.abs(us - 0.5) - 0.5 + r, np.abs(vs - 0.5) - 0.5 + r
        sdf = np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2) + np.minimum(np.maximum(dx, dy), 0) - r
        a2, e2 = _sstep(0.0, float(F32(0.01)), sdf, 10 * U)
        alo, ahi = np.minimum(alo, 1 - a2 - e2 - U), np.minimum(ahi, 1 - a2 + e2 + U)
    alo, ahi = np.clip(alo, 0, 1), np.clip(ahi, 0, 1)
    return np.maximum(clo, 0) * (1 - 16 * U) - 2 * U * 255, chi * (1 + 16 * U) + 2 * U * 255, alo, ahi, big


def _inpaint(g, rgb, dep, u, v, cdi, e_cdi, parx, pary, sweep, w, run, big, dtap, cmax):
    """push_pull_inpaint for the pixels at positions w of the evaluation -> the fill's range [m,3] x 2"""
    m = u.size
    psx, psy, tol, blur = float(g["psx"]), float(g["psy"]), float(g["tol"]), float(g["blur"])
    sx, sy = parx * psx * sweep, pary * psx * sweep                 # both use pixel_size.x (:442)
    rolled = sy != 0.0
    blo, bhi = np.zeros((m, 3)), np.zeros((m, 3))
    bw, ebw = np.zeros(m), np.zeros(m)

    def coord(a, k, nf):
        t = a + k
        return t, ((nf + 1) * U * abs(k) + U * np.abs(t)) * (k != 0)

    def tap(base, i, sign, live, wtab, phase1):
        nonlocal blo, bhi, bw, ebw
        tu, eu = coord(u, sign * sx * i, 3)
        tv, ev = coord(v, sign * sy * i, 3)
        o = (run.cmp(base, w, tu < 0, tu, eu, live) | run.cmp(base + 1, w, tv < 0, tv, ev, live)
             | run.cmp(base + 2, w, tu > 1, tu - 1, eu, live) | run.cmp(base + 3, w, tv > 1, tv - 1, ev, live))
        live = live & ~o
        dv, e_t = dtap(tu, eu, tv, ev, w)
        sdi = 1.0 - dv
        e_sdi = e_t + U * np.abs(sdi)
        rhs = cdi + tol
        ok = live & run.cmp(base + 4, w, sdi > rhs, sdi - rhs, e_sdi + e_cdi + U * np.abs(rhs), live)
        wi = float(wtab[i])
        if phase1:
            wt = wi * (1.0 + (sdi - cdi) * 10.0)
            ew = wi * (10 * (e_sdi + e_cdi) + 4 * U * (1 + 10 * np.abs(sdi - cdi))) + 2 * U * np.abs(wt)
        else:
            wt, ew = np.full(m, wi), np.full(m, 2 * U * wi)
        _, lo, hi, b = tex_range(rgb, tu, eu, tv, ev, cmax)
        big[w] |= b & ok
        blo = blo + np.where(ok, np.maximum(wt - ew, 0), 0)[:, None] * np.maximum(lo, 0)
        bhi = bhi + np.where(ok, wt + ew, 0)[:, None] * hi
        bw = bw + np.where(ok, wt, 0)
        ebw = ebw + np.where(ok, ew, 0)
        return ok

    active = np.ones(m, bool)
    for i in range(1, g["search"] + 1):
        ok = tap(_P1 + 6 * i, i, 1.0, active, g["w1"], True)
        brk = run.cmp(_P1 + 6 * i + 5, w, bw > 5, bw - 5, ebw + 32 * U * bw, ok)
        active = active & ~(ok & brk)
    need2 = run.cmp(_BW2, w, bw < 2, bw - 2, ebw + 32 * U * bw, np.ones(m, bool))
    for i in range(1, g["search"] + 1):
        tap(_P2 + 6 * i, i, -1.0, need2, g["w2"], False)
    e_bw = ebw + 32 * U * bw
    has = run.cmp(_BW01, w, bw > 0.01, bw - 0.01, e_bw, np.ones(m, bool))
    blo, bhi = blo * (1 - 64 * U), bhi * (1 + 64 * U)
    safe = np.maximum(bw - e_bw, 1e-9)
    va_lo, va_hi = blo / (bw + e_bw + 1e-300)[:, None] * 0.5, bhi / safe[:, None] * 0.5
    vw = np.full(m, 0.5)
    for t, dy in enumerate((-1.0, 1.0)):
        vv = v + dy * psy * blur
        ev = U * abs(psy * blur) + U * np.abs(vv)
        inside = run.cmp(_V + 3 * t, w, vv >= 0, vv, ev, has) & run.cmp(_V + 3 * t + 1, w, vv <= 1, vv - 1, ev, has)
        live = has & inside
        dv, e_t = dtap(u, 0.0, vv, ev, w)
        vdi = 1.0 - dv
        rhs = cdi + tol * 0.5
        ok = live & run.cmp(_V + 3 * t + 2, w, vdi > rhs, vdi - rhs, e_t + U * np.abs(vdi) + e_cdi + U * np.abs(rhs), live)
        _, lo, hi, b = tex_range(rgb, u, 0.0, vv, ev, cmax)
        big[w] |= b & ok
        va_lo = va_lo + np.where(ok, 0.25, 0)[:, None] * np.maximum(lo, 0)
        va_hi = va_hi + np.where(ok, 0.25, 0)[:, None] * hi
        vw = vw + np.where(ok, 0.25, 0)
    flo, fhi = va_lo / vw[:, None] * (1 - 8 * U), va_hi / vw[:, None] * (1 + 8 * U)
    _, olo, ohi, b = tex_range(rgb, u, 0.0, v, 0.0, cmax)                           # nothing found: the pixel's own colour (:505)
    return np.where(has[:, None], flo, olo), np.where(has[:, None], fhi, ohi)


def reference_eye(g, rgb, dep, eye):
    """-> dict: lo, hi [K=4, oh, ow, 4] (rgb 0..255 and alpha, un-multiplied), valid [4, oh, ow], cls [oh, ow] (0 decided, 1 branch-judged,
    2 exempt)"""
    n = g["oh"] * g["ow"]
    rgb, dep = rgb.astype(F64), dep.astype(F64)
    run = _Run(n)
    clo, chi, alo, ahi, big = _eval(g, rgb, dep, eye, np.arange(n), run)
    lo = np.repeat(np.concatenate([clo, alo[:, None]], 1)[None], 4, 0)
    hi = np.repeat(np.concatenate([chi, ahi[:, None]], 1)[None], 4, 0)
    valid = np.zeros((4, n), bool)
    valid[0] = True
    cls = np.where(big | (run.nund > 2), 2, np.where(run.nund > 0, 1, 0))
    br = np.nonzero(cls == 1)[0]
    if br.size:
        f1, f2 = run.ids[br, 0], run.ids[br, 1]
        for k, (b1, b2) in enumerate(itertools.product((False, True), repeat=2)):
            sub = _Run(br.size, (f1, f2, b1, b2))
            a, b, c_, d_, bg = _eval(g, rgb, dep, eye, br, sub)
            lo[k, br], hi[k, br] = np.concatenate([a, c_[:, None]], 1), np.concatenate([b, d_[:, None]], 1)
            valid[k, br] = True
            cls[br[sub.extra | bg]] = 2
    sh = (g["oh"], g["ow"])
    return dict(lo=lo.reshape(4, *sh, 4), hi=hi.reshape(4, *sh, 4), valid=valid.reshape(4, *sh), cls=cls.reshape(sh))


def reference(c, rgb, depth):
    """both eyes of every frame, packed as the kernel packs -> lo, hi [B, 4, out_h, out_w, 4], valid [B, 4, out_h, out_w], cls"""
    g = geom(c)
    out = {k: [] for k in ("lo", "hi", "valid", "cls")}
    for b in range(rgb.shape[0]):
        dep = depth_texels(c, depth[b])
        l, r = reference_eye(g, rgb[b], dep, 0), reference_eye(g, rgb[b], dep, 1)
        out["lo"].append(pack(c["mode"], l["lo"], r["lo"]))
        out["hi"].append(pack(c["mode"], l["hi"], r["hi"]))
        out["valid"].append(np.concatenate([l["valid"], r["valid"]], -1 if c["mode"].endswith("SBS") else -2))
        out["cls"].append(np.concatenate([l["cls"], r["cls"]], -1 if c["mode"].endswith("SBS") else -2))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the judge
def judge(ref, got, alpha, u8):
    """got [B, out_h, out_w, 3 | 4] float32 or uint8 as dibr_store writes it for alpha in window / premultiplied / rgba.
    -> dict(ok, decided, branch, exempt, bad = indices of the first failures, worst = the largest |got - mid| / half-width over the colour values of decided pixels, float32 output)"""
    lo, hi = ref["lo"], ref["hi"]
    clo, chi, alo, ahi = lo[..., :3], hi[..., :3], lo[..., 3:], hi[..., 3:]
    if alpha == "premultiplied":
        clo, chi = clo * alo * (1 - U) - U, chi * ahi * (1 + U) + U
    L, Hh = (np.concatenate([clo, alo], -1), np.concatenate([chi, ahi], -1)) if alpha == "rgba" else (clo, chi)
    x = got.astype(F64)[:, None]
    assert x.shape[2:] == L.shape[2:], (x.shape, L.shape)
    if u8:
        scale = np.array([1, 1, 1, 255.0])[:L.shape[-1]]
        inside = (x >= np.ceil(np.clip(L * scale, 0, 255) - 0.5)) & (x <= np.floor(np.clip(Hh * scale, 0, 255) + 0.5))
    else:
        inside = (x >= L) & (x <= Hh)
    match = (inside.all(-1) & ref["valid"]).any(1)                                       # any one evaluation, the whole pixel
    cls = ref["cls"]
    sane = np.isfinite(x[:, 0]).all(-1) & (x[:, 0] >= 0).all(-1) & (x[:, 0] <= 255 * (1 + 2.0 ** -20)).all(-1)
    okpix = np.where(cls == 2, sane, match)
    half = np.maximum((Hh[:, 0] - L[:, 0]) / 2, 1e-30)
    rel = np.abs(x[:, 0] * (1.0 if not u8 else 1.0 / np.array([1, 1, 1, 255.0])[:L.shape[-1]]) - (Hh[:, 0] + L[:, 0]) / 2) / half
    worst = float(rel[..., :3][cls == 0].max()) if (cls == 0).any() and not u8 else float("nan")          # colour values of decided pixels
    p50, p99 = (np.percentile(rel[..., :3][cls == 0], [50, 99]).tolist() if (cls == 0).any() and not u8 else (float("nan"),) * 2)
    n = cls.size
    return dict(p50=p50, p99=p99, ok=bool(okpix.all()), n=n, decided=int((cls == 0).sum()), branch=int((cls == 1).sum()), exempt=int((cls == 2).sum()),
                bad=np.argwhere(~okpix)[:8].tolist(), nbad=int((~okpix).sum()), worst=worst)


def condition(j):
    """the per-case condition on the reference's own classes"""
    return j["exempt"] <= 8 and j["exempt"] <= 0.001 * j["n"] and j["decided"] + j["branch"] >= 0.99 * j["n"]


# ------------------------------------------------------------------------------------------------ the float32 emulation (kernel forms)
MUTANTS = ("tap_off_one", "repeat_clamp", "sweep_other_eye", "sy_psy", "w1_prev", "no_break", "no_phase2", "vblur_psx", "vblur_tol",
           "no_smooth", "no_falloff", "eyes_swapped", "half_offset", "no_premult", "sdf_on_crop_uv", "feather_no_flip",
           "updep_align_corners", "u8_trunc", "corner_pixel", "wrong_row", "win_neighbour")


def _tex32(img, u, v, *, clamp=False, xoff=0, win=None):
    """tex_tap + lerp2 of dibr_tex.h in float32; win = (wx0 per pixel, WW): the deliberate window error (the tap at j = WW - 2 reads
    one texel to the left)"""
    H, W = img.shape[:2]
    x = (u * F32(W)).astype(F32) - F32(0.5)
    y = (v * F32(H)).astype(F32) - F32(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(F32), (y - y0f).astype(F32)
    xi, yi = x0f.astype(np.int64) + xoff, y0f.astype(np.int64)
    if win is not None:
        xi = xi - ((xi - win[0]) == win[1] - 2)
    if clamp:
        x0, x1, y0, y1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1), np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    else:
        x0, y0 = np.mod(xi, W), np.mod(yi, H)
        x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top = (a + ((b - a) * fx).astype(F32)).astype(F32)
    bot = (c + ((d - c) * fx).astype(F32)).astype(F32)
    return (top + ((bot - top) * fy).astype(F32)).astype(F32)


def _ss_inv(e0, e1, x):
    """SMOOTHSTEP_C: multiply by the float32 inverse of the constant edge distance"""
    inv = F32(1.0 / (float(F32(e1)) - float(F32(e0))))
    t = np.clip(((x - F32(e0)).astype(F32) * inv).astype(F32), F32(0), F32(1))
    return (t * t * (F32(3) - F32(2) * t).astype(F32)).astype(F32)


def _ss_div(e0, e1, x):
    t = np.clip(((x - F32(e0)).astype(F32) / (F32(e1) - F32(e0))).astype(F32), F32(0), F32(1))
    return (t * t * (F32(3) - F32(2) * t).astype(F32)).astype(F32)


def emulate_eye(g, rgb_u8, dep, eye, mut=None, plan=None):
    """dibr_pixel in float32 -> [oh, ow, 4]: frag_color's rgb (0..255) and alpha, un-multiplied"""
    oh, ow, W = g["oh"], g["ow"], g["W"]
    n = oh * ow
    rgb = rgb_u8.astype(F32)
    us, vs, u, v, px_x, px_y = pixel_uv(g, np.arange(n))
    clamp = mut == "repeat_clamp"
    win = None
    if mut == "win_neighbour":
        xb = (px_x // plan["cols"]) * plan["cols"]
        ub = ((xb.astype(F32) + F32(0.5)) / F32(ow)).astype(F32)
        if g["crop"]:
            ub = (g["cx"] + (ub * g["cw"]).astype(F32)).astype(F32)
        win = (np.floor((ub * F32(W)).astype(F32) - F32(0.5)).astype(np.int64) - plan["margin"], plan["WW"])
    c, s, psx, psy = g["c"], g["s"], g["psx"], g["psy"]
    eo = g["half_ipd"] if eye else -g["half_ipd"]
    sg = F32(np.sign(eo))
    parx, pary = F32(c * sg), F32(s * sg)
    sweep = F32(-1.0 if eo > 0 else 1.0)
    own = lambda img, a, b, w_=None, **k: _tex32(img, a, b, clamp=clamp, win=w_, **k)

    def T(img, a, b, **k):          # a tap on the pixel's own row pair: through the window when the row kernel runs
        return own(img, a, b, None if win is None else win, **k)
    d0 = T(dep, u, v)
    if s == 0:                       # PixTaps: the left eye's offsets, dm and dp exchanged for the right eye
        lx = F32(F32(c * F32(-1)) * psx)
        dsl, s2l = F32(lx * F32(1.5)), F32(lx * F32(2.0))
        tA, tB = T(dep, (u - dsl).astype(F32), v), T(dep, (u + dsl).astype(F32), v)
        jA, jB = T(dep, (u - s2l).astype(F32), v), T(dep, (u + s2l).astype(F32), v)
        dm, dp = (tB, tA) if eye else (tA, tB)
        jump = np.abs(jB - jA) if eye else np.abs(jA - jB)
    else:
        dsx, dsy = F32(F32(parx * psx) * F32(1.5)), F32(F32(pary * psy) * F32(1.5))
        s2x, s2y = F32(F32(parx * psx) * F32(2.0)), F32(F32(pary * psy) * F32(2.0))
        dm, dp = T(dep, (u - dsx).astype(F32), (v - dsy).astype(F32)), T(dep, (u + dsx).astype(F32), (v + dsy).astype(F32))
        jump = np.abs(T(dep, (u - s2x).astype(F32), (v - s2y).astype(F32)) - T(dep, (u + s2x).astype(F32), (v + s2y).astype(F32)))
    d = (((d0 * F32(0.7)).astype(F32) + (dm * F32(0.15)).astype(F32)).astype(F32) + (dp * F32(0.15)).astype(F32)).astype(F32)
    if mut == "no_smooth":
        d = d0
    dinv = -d
    shaped = (dinv * (F32(1) + (F32(0.35) * (F32(1) - d).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    shift = (shaped + g["conv"]).astype(F32)
    fall = np.where((u < F32(0.05)) | (u > F32(0.95)), (_ss_inv(0.0, 0.05, u) * _ss_inv(1.0, 0.95, u)).astype(F32), F32(1))
    if mut == "no_falloff":
        fall = np.ones_like(u)
    px = (((eo * shift).astype(F32) * g["strength"]).astype(F32) * fall).astype(F32)
    su, sv = (u - (px * c).astype(F32)).astype(F32), (v - (px * s).astype(F32)).astype(F32)
    oob = (su < 0) | (su > 1) | (sv < 0) | (sv > 1)
    conf = np.where(oob, F32(1), _ss_inv(0.04, 0.10, jump)).astype(F32)
    col = T(rgb, su, sv, xoff=1 if mut == "tap_off_one" else 0)
    m = conf > F32(0.001)
    if m.any():
        w_ = None if win is None else (win[0][m], win[1])
        fill = _emu_inpaint(g, rgb, dep, u[m], v[m], dinv[m], parx, pary, sweep, mut, clamp, w_)
        cm = conf[m][:, None]
        col[m] = ((col[m] * (F32(1) - cm).astype(F32)).astype(F32) + (fill * cm).astype(F32)).astype(F32)
    bx = (_ss_inv(-0.001, 0.001, su) * _ss_inv(1.001, 0.999, su)).astype(F32)
    by = (_ss_inv(-0.001, 0.001, sv) * _ss_inv(1.001, 0.999, sv)).astype(F32)
    alpha = np.where((su < F32(0.001)) | (su > F32(0.999)) | (sv < F32(0.001)) | (sv > F32(0.999)), np.minimum(bx, by), F32(1)).astype(F32)
    if g["feather"]:
        fu = (((px_x.astype(F32) + F32(0.5)) - g["vpx"]).astype(F32) / g["vpw"]).astype(F32)
        yy = (px_y.astype(F32) + F32(0.5)) if mut == "feather_no_flip" else (F32(oh) - (px_y.astype(F32) + F32(0.5))).astype(F32)
        fv = ((yy - g["vpy"]).astype(F32) / g["vph"]).astype(F32)
        fw = g["feather_w"]
        fo = (((_ss_div(0, fw, fu) * _ss_div(0, fw, (F32(1) - fu).astype(F32))).astype(F32) * _ss_div(0, fw, fv)).astype(F32)
              * _ss_div(0, fw, (F32(1) - fv).astype(F32))).astype(F32)
        col = (col * np.power(fo, F32(0.7)).astype(F32)[:, None]).astype(F32)
    if g["corner_r"] > 0:
        r = g["corner_r"]
        qu, qv = (u, v) if mut == "sdf_on_crop_uv" else (us, vs)
        dx = ((np.abs(qu - F32(0.5)) - F32(0.5)).astype(F32) + r).astype(F32)
        dy = ((np.abs(qv - F32(0.5)) - F32(0.5)).astype(F32) + r).astype(F32)
        mx, my = np.maximum(dx, F32(0)), np.maximum(dy, F32(0))
        sdf = ((np.sqrt(((mx * mx).astype(F32) + (my * my).astype(F32)).astype(F32)).astype(F32) + np.minimum(np.maximum(dx, dy), F32(0))).astype(F32) - r).astype(F32)
        alpha = np.minimum(alpha, (F32(1) - _ss_div(0.0, 0.01, sdf)).astype(F32))
    return np.concatenate([col, alpha[:, None]], 1).astype(F32).reshape(oh, ow, 4)


def _emu_inpaint(g, rgb, dep, u, v, cdi, parx, pary, sweep, mut, clamp, win):
    n = u.size
    psx, psy, tol, blur = g["psx"], g["psy"], g["tol"], g["blur"]
    if mut == "sweep_other_eye":
        sweep = -sweep
    sx = F32(F32(parx * psx) * sweep)
    sy = F32(F32(pary * (psy if mut == "sy_psy" else psx)) * sweep)
    T = lambda img, a, b: _tex32(img, a, b, clamp=clamp, win=win)
    best, bw = np.zeros((n, 3), F32), np.zeros(n, F32)
    active = np.ones(n, bool)
    for i in range(1, g["search"] + 1):
        tu, tv = (u + F32(sx * F32(i))).astype(F32), (v + F32(sy * F32(i))).astype(F32)
        ok = active & ~((tu < 0) | (tv < 0) | (tu > 1) | (tv > 1))
        sdi = (F32(1) - T(dep, tu, tv)).astype(F32)
        ok &= sdi > (cdi + tol).astype(F32)
        wi = g["w1"][i - 1 if mut == "w1_prev" else i]
        w = (wi * (F32(1) + ((sdi - cdi).astype(F32) * F32(10)).astype(F32)).astype(F32)).astype(F32)
        col = T(rgb, tu, tv)
        best = np.where(ok[:, None], (best + (col * w[:, None]).astype(F32)).astype(F32), best)
        bw = np.where(ok, (bw + w).astype(F32), bw)
        if mut != "no_break":
            active &= ~(ok & (bw > F32(5)))
    need2 = (bw < F32(2)) & (mut != "no_phase2")
    for i in range(1, g["search"] + 1):
        tu, tv = (u - F32(sx * F32(i))).astype(F32), (v - F32(sy * F32(i))).astype(F32)
        ok = need2 & ~((tu < 0) | (tv < 0) | (tu > 1) | (tv > 1))
        sdi = (F32(1) - T(dep, tu, tv)).astype(F32)
        ok &= sdi > (cdi + tol).astype(F32)
        w = g["w2"][i]
        col = T(rgb, tu, tv)
        best = np.where(ok[:, None], (best + (col * w).astype(F32)).astype(F32), best)
        bw = np.where(ok, (bw + w).astype(F32), bw)
    has = bw > F32(0.01)
    va = ((best / np.where(has, bw, F32(1))[:, None]).astype(F32) * F32(0.5)).astype(F32)
    vw = np.full(n, 0.5, F32)
    for dy in (-1.0, 1.0):
        vv = (v + F32(F32(F32(dy) * (psx if mut == "vblur_psx" else psy)) * blur)).astype(F32)
        ok = has & (vv >= 0) & (vv <= 1)
        vs_ = np.where(ok, vv, v)
        vdi = (F32(1) - _tex32(dep, u, vs_, clamp=clamp)).astype(F32)
        ok &= vdi > (cdi + (tol if mut == "vblur_tol" else F32(tol * F32(0.5)))).astype(F32)
        col = _tex32(rgb, u, vs_, clamp=clamp)
        va = np.where(ok[:, None], (va + (col * F32(0.25)).astype(F32)).astype(F32), va)
        vw = np.where(ok, (vw + F32(0.25)).astype(F32), vw)
    out = T(rgb, u, v)
    return np.where(has[:, None], (va / vw[:, None]).astype(F32), out).astype(F32)


def store(x, alpha, u8, mut=None):
    """dibr_store of [.., 4] frag_color for an alpha mode: float32 as it is, uint8 nearest-even and saturating, alpha scaled by 255"""
    col, a = x[..., :3], x[..., 3:]
    if alpha == "premultiplied" and mut != "no_premult":
        col = (col * a).astype(F32)
    out = np.concatenate([col, a], -1) if alpha == "rgba" else col
    if not u8:
        return np.ascontiguousarray(out.astype(F32))
    if alpha == "rgba":
        out = np.concatenate([col, (a * F32(255)).astype(F32)], -1)
    out = np.clip(out, 0, 255)
    return (np.floor(out) if mut == "u8_trunc" else np.rint(out)).astype(np.uint8)


def emulate(c, rgb, depth, alpha="window", u8=False, mut=None, plan=None):
    """the float32 emulation of the whole call (kernel forms; mut: one deliberate error) -> what ops.dibr_warp returns"""
    g = geom(c)
    outs = []
    for b in range(rgb.shape[0]):
        dep = depth_texels(c, depth[b], mut)
        l, r = emulate_eye(g, rgb[b], dep, 0, mut, plan), emulate_eye(g, rgb[b], dep, 1, mut, plan)
        if mut == "eyes_swapped":
            l, r = r, l
        o = pack(c["mode"], l, r)
        if mut == "half_offset":          # the right / lower eye starts one column / row late
            if c["mode"].endswith("SBS"):
                o[:, g["ow"] + 1:] = r[:, :-1]
            else:
                o[g["oh"] + 1:] = r[:-1]
        if mut == "corner_pixel":
            o[-1, -1, :3] = o[-1, -2, :3]
        if mut == "wrong_row":
            o[o.shape[0] // 3] = o[o.shape[0] // 3 + 1]
        outs.append(o)
    return store(np.stack(outs), alpha, u8, mut)
