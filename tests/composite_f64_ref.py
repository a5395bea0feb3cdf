"""Float64 reference of the viewer's composite display modes (dibr_composite.hip: ana_pixel, il_pixel, comp_push_pull, comp_fx,
comp_out, depth_map_kernel; ANAGLYPH_FRAGMENT, INTERLEAVED_FRAGMENT, VERTICAL_INTERLEAVED_FRAGMENT and DEPTH_FRAGMENT, viewer.py:633-1197)
with decision margins, a float32 emulation in the kernels' forms, and the cases test_cpu_composite_f64.py and
test_gpu_composite_f64.py share.  numpy only.  The texture tap's range, the smoothstep bound, the record of undecided comparisons, the
in-painting's sweeps, the judge, the per-case condition, the inputs and u = 2^-24 are dibr_ref.py's (imported, not copied): what that
module's docstring derives for them holds here unchanged.  What differs from f1 is stated below, term for term from the kernels.

OPERANDS (float32, bit-reproducible, no part of the error): what dibr_fill_geom forms (cos / sin of the roll, psx, psy, half_ipd,
strength, conv, tol, blur, the two weight tables); u = (x + 0.5f) / ow, v = (y + 0.5f) / oh; the integer gl_FragCoord (vx + x,
vy + oh - 1 - y) and from it fu = (float(vx + x) + 0.5f - vpx) / vpw, fv likewise, as comp_fx forms them; a depth texel (UpDep: what
upsample_depth_kernel stores, frame_ref.upsample in float32); the literal edges of SMOOTHSTEP_C as float32.  Everything after the
operands is float64.

BOUNDS, from the kernels' arithmetic; nothing here was measured on a kernel.  Coordinates, taps, the three-tap depth chain (e_d), the
smoothstep, the sweeps, best / bw, the vertical taps, the feather, the corner, the final widening (1 +- 16 u) and 2 u 255, and the u8
rule are dibr_ref.py's.  New:
 Interleaved / Interleaved-V (il_pixel).  eye_dir = -1 where the parity of vy + oh - 1 - y (Interleaved) or vx + x (Interleaved-V) is
   even, else +1.  shaped, shift, px, su, sv as f1 with eye_offset = eye_dir half_ipd, except that the fall-off is
   smoothstep(0, 0.02f, u) smoothstep(1, 0.98f, u) (operands only: 20 u, as f1's).  conf = smoothstep(0.06f, 0.12f, jump) through the
   smoothstep bound; the colour is the in-painting's where conf > 0.001 (a decision) and the tap at (su, sv) otherwise: no mix, so no
   mix term.  Border alpha as f1.
 Anaglyph (ana_pixel).  The smoothing taps run along (c, s) for both eyes (k = c psx 1.5: three factors).  shift = -d + conv:
   e = e_d + u |shift|; sa = shift strength fall: e_sa = |strength| (fall e_shift + |shift| 20 u) + 3 u |sa|; ox = half_ipd sa c:
   e_ox = |half_ipd c| e_sa + 3 u |ox| (two products and cosf's ulp), oy likewise with s; lu = u + ox: e_lu = e_ox + u |lu|, and so
   lv, ru, rv (the v coordinates exact at roll 0).  Decisions: the four comparisons of oob per eye, and ONE jump > 0.08f shared by both
   eyes (live unless both eyes are already out of bounds), jump = |dA - dB| with e = e_A + e_B + u |jump|.  An eye that is occluded takes
   the in-painting swept with search_dir, the other the tap at its coordinate; the output keeps (L.r, R.g, R.b) and only those channels
   are bounded.  alpha = min of four products of two smoothsteps over 0.015f (each product: the two smoothstep bounds + 2 u).  The
   comparisons of both eyes count together towards a pixel's one or two undecided ones (the right eye's ids are offset by 1000).
 In-painting (comp_push_pull): dibr_ref._inpaint with the program's step -- Interleaved (c, s) eye_dir psx i (parx = c eye_dir,
   sweep = +1), Anaglyph and Interleaved-V search_dir i psx (c, s) with search_dir = -eye_dir (parx = c, sweep = search_dir).  Both forms
   are three float32 factors and cosf's ulp: _inpaint's coordinate bound (4 u |k| + u |t|) covers either.
 comp_fx: fu, fv are operands; the feather and the corner SDF are f1's bounds taken over (fu, fv).
 Depth Map.  t = one tap at the operands (cu, cv) with its range e_t.  w_k = fmaxf(0, 1 - |t - k| 4): a difference, an exact product
   by 4 and a difference: e_k = 4 (e_t + u |t - k|) + u |1 - 4 |t - k||, and the clamp is 1-Lipschitz and exact at 0: w_k in
   [max(0, w - e), max(0, w + e)].  total = the sum of four non-negative terms: the interval sum (1 +- 3 u).  total > 0 is the only hard
   comparison: decided true where the lower end is positive, decided false where the upper end is 0 (every w_k exactly 0 in float32
   too), else undecided -- it is so only where the texel lies within its bound of -0.125 or 1.125.  Normalised w_k / total: [w_lo /
   total_hi, w_hi / total_lo] (1 +- u), at most 1 (a correctly rounded quotient of a <= b is <= 1).  A channel: four products with the
   float32 key colours, three sums and the product by 255: the interval sum (1 +- 8 u); alpha is exactly 1.

DECISIONS and the PER-CASE CONDITION are dibr_ref.py's: a comparison is recorded where |lhs - rhs| is within the bound of its sides; one
or two per pixel are evaluated under every outcome combination (at most four) and a whole-pixel match with any is accepted; more than
two, or a further one met under a forced outcome, exempt the pixel (finite and within [0, 255 (1 + 2^-20)]).  Per case (condition):
exempt <= 8 and <= 0.1 % of the pixels, decided + branch-judged >= 99 %.

TWO ERRORS THE JUDGE CANNOT SEE, BY SYMMETRY.  The composites' u_viewport is the output rectangle itself, so fu == u bit for bit and
fv == 1 - v up to an ulp; the feather (a product of smoothsteps of fv and 1 - fv) and the corner SDF (|fv - 0.5|) are symmetric under
fv <-> 1 - fv.  "fv not flipped" and "the feather over (u, v)" therefore compute the same picture; test_cpu_composite_f64.py shows the
judge accepting both, and rejects the error that is one: gl_FragCoord taken without subtracting the viewport's origin.
"""
import itertools

import numpy as np

import dibr_ref as R
from dibr_ref import F32, F64, U, _Run, _inpaint, _sstep, condition, depth_texels, inputs, judge, tex_range      # noqa: F401 (re-exported)

WARP_MODES = ("Anaglyph", "Interleaved", "Interleaved-V")
TAG = {"Anaglyph": "ana", "Interleaved": "il", "Interleaved-V": "ilv"}
FAMILIES = ("rows256", "rows512", "fx", "updep_rows", "roll0", "general")
_RIGHT = 1000          # id offset of the Anaglyph's right-eye comparisons
_JUMP = R._CONF


# ------------------------------------------------------------------------------------------------ cases
def case(name, H, W, expect, vp=(0, 0, 0, 0), modes=None, dhw=None, colors="noise", dscale=1.0, batch=1, seed=0, **kw):
    """expect = (kind, cols): kind "rows" | "roll0" | "general"; the kernel's name follows from it, the mode and the parameters"""
    bad = set(kw) - set(R.DEFAULTS)
    assert not bad and "viewport" not in kw, (bad, kw)
    kw = dict(kw, viewport=tuple(float(x) for x in vp))
    return dict(name=name, H=H, W=W, vp=tuple(vp), modes=modes, dhw=dhw or (H, W), colors=colors, dscale=dscale, batch=batch, seed=100 + seed,
                expect=expect, kw=kw)


ALL3 = ("full530", "up2x", "over1564", "roll03", "fxvp", "up5x19")


def _cases():
    fx = dict(feather=True, feather_width=0.1, corner_radius=0.2)
    big = dict(dscale=4.0, depth_ratio=5.0, ipd_uv=0.2, blur_radius=2.25)
    c = [
        case("full530", 12, 530, ("rows", 512)),                                        # two 512-column blocks, the second ragged
        case("w257", 8, 257, ("rows", 512), seed=1),                                    # ow > cols / 2 stays one ragged block of 512
        case("w256", 8, 256, ("rows", 256), seed=2),                                    # the halving rule
        case("tiny", 2, 2, ("rows", 256), seed=3),                                      # wrap on every tap
        case("up2x", 10, 300, ("rows", 512), vp=(1, 3, 600, 20), seed=4),               # half a texel per column; odd origin: both parities flip
        case("down2x", 12, 1060, ("rows", 256), vp=(2, 1, 530, 6), seed=5),             # two texels per column; 512 window > 640; three blocks
        case("fits1534", 8, 1200, ("rows", 256), vp=(0, 0, 204, 8), seed=6),            # the last window that fits (WW 1534 <= 1536)
        case("over1564", 8, 1200, ("roll0", None), vp=(0, 0, 200, 8), seed=7),          # the first that does not (WW 1564)
        case("parallax", 6, 2400, ("roll0", None), ipd_uv=0.5, depth_ratio=20.0, blur_radius=2.25, seed=8),      # the margin alone exceeds the window
        case("dscale4", 10, 530, ("rows", 512), seed=9, **big),                         # taps leave the LDS window: the row-gather fallback
        case("winedge", 10, 700, ("rows", 512), seed=10, **big),                        # taps on the window's last texel pair
        case("fxvp", 16, 300, ("rows", 512), vp=(10, 1, 270, 12), seed=11, **fx),       # comp_fx over gl_FragCoord with an origin
        case("fx530", 16, 530, ("rows", 512), feather=True, corner_radius=0.03, convergence=0.03, seed=12),      # FX across a block seam
        case("roll03", 16, 300, ("general", None), roll=0.3, convergence=0.03, seed=13),      # general gather; sweeps with a y component
        case("roll12fx", 16, 300, ("general", None), vp=(10, 1, 270, 12), roll=-1.2, seed=14, **fx),
        case("up5x19", 24, 530, ("rows", 512), dhw=(5, 19), seed=15),                   # UpDep staging loop
        case("up37x66roll", 24, 300, ("general", None), dhw=(37, 66), roll=0.3, seed=16),
        case("sr0", 8, 300, ("rows", 512), search_radius=0.0, seed=17),                 # the in-painting finds nothing: own colour
        case("sr15_tol", 10, 300, ("rows", 512), search_radius=15.0, depth_tolerance=0.3, seed=18),
        case("res", 10, 530, ("rows", 512), resolution=(400.0, 30.0), seed=19),         # psx != 1 / W; tie-free
        case("batch2", 8, 530, ("rows", 512), batch=2, blur_radius=2.25, seed=20),      # frame stride
        case("smooth", 12, 530, ("rows", 512), colors="smooth", seed=21),               # the u8 rounding class
        case("rows270", 270, 96, ("rows", 256), seed=22),                               # a wrong-row error among many rows
    ]
    k = 0
    for x in c:
        if x["name"] in ALL3:
            x["modes"] = WARP_MODES
        else:
            x["modes"] = (WARP_MODES[k % 3],)
            k += 1
    return {x["name"]: x for x in c}


CASES = _cases()
DM_CASES = {x["name"]: x for x in (
    case("dm_odd", 30, 52, None, vp=(0, 0, 61, 37), seed=40),                           # 2257 pixels: the last thread has one
    case("dm_odd_b3", 30, 52, None, vp=(0, 0, 61, 37), batch=3, seed=41),               # groups of four pixels straddle frames
    case("dm_up", 30, 52, None, vp=(0, 0, 61, 37), dhw=(5, 19), seed=42),
    case("dm_black", 8, 64, None, dscale=1.3, seed=43),                                 # texels above 1.125 and at it
    case("dm_2x2", 2, 2, None, seed=44))}


def case_inputs(c):
    """dibr_ref.inputs; dm_black additionally holds texels AT 1.125 (total is exactly 0) and one float32 below it (total = 2^-21, inside
    the bound of the tap's own roundings): both undecided; and texels at 1.12 (total = 0.02: decided, pure red after the division) -- its
    viewport is the source, 64 columns, so a tap is its texel exactly"""
    rgb, dep = inputs(c)
    if c["name"] == "dm_black":
        dep[0, 2:4, 10:14] = F32(1.125)
        dep[0, 5:7, 20:24] = np.nextafter(F32(1.125), F32(0))
        dep[0, 5:7, 30:34] = F32(1.12)
        assert (dep > 1.125).sum() > 8
    return rgb, dep


def family(c):
    kind, cols = c["expect"]
    p = dict(R.DEFAULTS, **c["kw"])
    if kind != "rows":
        return kind
    if c["dhw"] != (c["H"], c["W"]):
        return "updep_rows"
    if p["feather"] or p["corner_radius"] > 0:
        return "fx"
    return f"rows{cols}"


def kernel_name(c, mode, u8):
    kind, cols = c["expect"]
    p = dict(R.DEFAULTS, **c["kw"])
    fmt, d = "u8" if u8 else "f32", "UpDep" if c["dhw"] != (c["H"], c["W"]) else "FullDep"
    if kind == "rows":
        return f"comp_rows<{TAG[mode]},{fmt},fx={1 if p['feather'] or p['corner_radius'] > 0 else 0},{cols},{d}>"
    return f"comp<{TAG[mode]},{fmt},{kind},{d}>"


def dm_kernel_name(c, u8, nch, vec):
    return f"depth_map<{'u8' if u8 else 'f32'},{nch},{'vec' if vec else 'scalar'},{'UpDep' if c['dhw'] != (c['H'], c['W']) else 'FullDep'}>"


def geom(c):
    """the float32 uniforms as dibr_fill_geom and comp_plan_impl form them: the viewport is the output and u_viewport"""
    g = R.geom(dict(c, mode="Full-SBS", crop=None, kw=dict(c["kw"], viewport=(0.0, 0.0, 0.0, 0.0))))
    vx, vy, vw, vh = c["vp"] if any(c["vp"]) else (0, 0, c["W"], c["H"])
    g.update(oh=vh, ow=vw, vx=vx, vy=vy, vpx=F32(vx), vpy=F32(vy), vpw=F32(vw), vph=F32(vh))
    return g


def _uv(g, idx):
    y, x = np.divmod(idx, g["ow"])
    return ((x.astype(F32) + F32(0.5)) / F32(g["ow"])).astype(F32), ((y.astype(F32) + F32(0.5)) / F32(g["oh"])).astype(F32), x, y


def _fuv(g, x, y, mut=None):
    """comp_fx's fu, fv in float32"""
    gx = (F32(1) * (g["vx"] + x)).astype(F32) + F32(0.5)
    gy = (F32(1) * ((g["vy"] + y) if mut == "feather_no_flip" else (g["vy"] + g["oh"] - 1 - y))).astype(F32) + F32(0.5)
    if mut == "feather_no_origin":
        return (gx / g["vpw"]).astype(F32), (gy / g["vph"]).astype(F32)
    return ((gx - g["vpx"]).astype(F32) / g["vpw"]).astype(F32), ((gy - g["vpy"]).astype(F32) / g["vph"]).astype(F32)


def eye_dir(g, mode, x, y, mut=None):
    """-1 (left) where gl_FragCoord's parity is even"""
    vx, vy = (0, 0) if mut == "parity_no_origin" else (g["vx"], g["vy"])
    if mode == "Interleaved":
        par = (y if mut == "parity_output_row" else vy + g["oh"] - 1 - y)
    else:
        par = vx + x
    e = np.where(par & 1, 1.0, -1.0)
    return -e if mut == "eyes_swapped" else e


# ------------------------------------------------------------------------------------------------ the float64 reference
class _Shift:
    """a _Run whose comparison ids are offset (the Anaglyph's right eye)"""
    def __init__(self, run, off):
        self.run, self.off = run, off

    def cmp(self, cid, *a):
        return self.run.cmp(cid + self.off, *a)


def _off(a, k, nf):
    t = a + k
    return t, ((nf + 1) * U * np.abs(k) + U * np.abs(t)) * (k != 0)


def _mk_dtap(dep, big, dmax):
    def dtap(tu, eu, tv, ev, w=None):
        val, lo, hi, b = tex_range(dep, tu, eu, tv, ev, dmax)
        if w is None:
            big[:] |= b
        else:
            big[w] |= b
        return val, np.maximum(hi - val, val - lo)
    return dtap


def _smooth_depth(u, v, kx, ky, dtap):
    """d = 0.7 d0 + 0.15 dm + 0.15 dp at u -+ (kx, ky) (per-pixel arrays or scalars) and its bound"""
    d0, e0 = dtap(u, 0.0, v, 0.0)
    (um, eum), (vm, evm) = _off(u, -kx, 3), _off(v, -ky, 3)
    (up, eup), (vp, evp) = _off(u, kx, 3), _off(v, ky, 3)
    dm, em = dtap(um, eum, vm, evm)
    dp, ep = dtap(up, eup, vp, evp)
    d = 0.7 * d0 + 0.15 * dm + 0.15 * dp
    return d, 0.7 * e0 + 0.15 * (em + ep) + 8 * U * (0.7 * np.abs(d0) + 0.15 * np.abs(dm) + 0.15 * np.abs(dp))


def _fall002(u):
    return _sstep(0.0, float(F32(0.02)), u, 0.0)[0] * _sstep(1.0, float(F32(0.98)), u, 0.0)[0]


def _band(e0, e1, t, et):
    """smoothstep(e0, e1, t) smoothstep(1 - e0, 1 - e1, t)-style product of two smoothsteps and its bound"""
    a, ea = _sstep(e0[0], e0[1], t, et)
    b, eb = _sstep(e1[0], e1[1], t, et)
    return a * b, ea + eb + 2 * U


def _fx_out(g, x, y, clo, chi, alo, ahi):
    """comp_fx over (fu, fv) and the final widening -> lo, hi [n, 4]"""
    fu32, fv32 = _fuv(g, x, y)
    fu, fv = fu32.astype(F64), fv32.astype(F64)
    if g["feather"]:
        fw = float(g["feather_w"])
        fo = _sstep(0, fw, fu, 0.0)[0] * _sstep(0, fw, 1 - fu, U)[0] * _sstep(0, fw, fv, 0.0)[0] * _sstep(0, fw, 1 - fv, U)[0]
        e_fo = 50 * U + 4 * 1.5 * 2 * U / fw
        sh_lo = np.power(np.clip(fo - e_fo, 0, 1), 0.7) * (1 - 16 * U)
        sh_hi = np.power(np.clip(fo + e_fo, 0, 1), 0.7) * (1 + 16 * U)
        clo, chi = clo * sh_lo[:, None], chi * sh_hi[:, None]
    if g["corner_r"] > 0:
        r = float(g["corner_r"])
        dx, dy = np.abs(fu - 0.5) - 0.5 + r, np.abs(fv - 0.5) - 0.5 + r
        sdf = np.sqrt(np.maximum(dx, 0) ** 2 + np.maximum(dy, 0) ** 2) + np.minimum(np.maximum(dx, dy), 0) - r
        a2, e2 = _sstep(0.0, float(F32(0.01)), sdf, 10 * U)
        alo, ahi = np.minimum(alo, 1 - a2 - e2 - U), np.minimum(ahi, 1 - a2 + e2 + U)
    alo, ahi = np.clip(alo, 0, 1), np.clip(ahi, 0, 1)
    lo = np.concatenate([np.maximum(clo, 0) * (1 - 16 * U) - 2 * U * 255, alo[:, None]], 1)
    hi = np.concatenate([chi * (1 + 16 * U) + 2 * U * 255, ahi[:, None]], 1)
    return lo, hi


def _eval_il(g, mode, rgb, dep, eye, idx, run):
    """il_pixel in float64 for the pixels idx, all of eye_dir `eye` (-1.0 | 1.0) -> lo, hi [n, 4], big [n]"""
    n = idx.size
    alln = np.arange(n)
    u32, v32, x, y = _uv(g, idx)
    u, v = u32.astype(F64), v32.astype(F64)
    c, s, psx, psy = float(g["c"]), float(g["s"]), float(g["psx"]), float(g["psy"])
    rolled = s != 0.0
    eo = eye * float(g["half_ipd"])
    parx, pary = c * eye, s * eye
    strength, conv = float(g["strength"]), float(g["conv"])
    big = np.zeros(n, bool)
    dtap = _mk_dtap(dep, big, float(np.abs(dep).max()))
    d, e_d = _smooth_depth(u, v, parx * psx * 1.5, pary * psy * 1.5, dtap)
    shaped = -d * (1.0 + 0.35 * (1.0 - d))
    e_sh = (1.35 + 0.7 * np.abs(d)) * e_d + 8 * U * np.abs(d) * (1.35 + 0.35 * np.abs(d))
    shift = shaped + conv
    e_shift = e_sh + U * np.abs(shift)
    fall = _fall002(u)
    px = eo * shift * strength * fall
    e_px = abs(eo * strength) * (fall * e_shift + np.abs(shift) * 20 * U) + 4 * U * np.abs(px)
    su, sv = u - px * c, v - px * s
    e_su = abs(c) * e_px + 2 * U * np.abs(px * c) + U * np.abs(su)
    e_sv = (abs(s) * e_px + 2 * U * np.abs(px * s) + U * np.abs(sv)) * rolled
    live = np.ones(n, bool)
    oob = (run.cmp(R._SU0, alln, su < 0, su, e_su, live) | run.cmp(R._SU1, alln, su > 1, su - 1, e_su, live)
           | run.cmp(R._SV0, alln, sv < 0, sv, e_sv, live) | run.cmp(R._SV1, alln, sv > 1, sv - 1, e_sv, live))
    s2x, s2y = parx * psx * 2.0, pary * psy * 2.0
    (ua, eua), (va_, eva) = _off(u, -s2x, 3), _off(v, -s2y, 3)
    (ub, eub), (vb, evb) = _off(u, s2x, 3), _off(v, s2y, 3)
    dA, eA = dtap(ua, eua, va_, eva)
    dB, eB = dtap(ub, eub, vb, evb)
    jump = np.abs(dA - dB)
    conf, e_conf = _sstep(float(F32(0.06)), float(F32(0.12)), jump, eA + eB + U * jump)
    conf, e_conf = np.where(oob, 1.0, conf), np.where(oob, 0.0, e_conf)
    _, clo, chi, b = tex_range(rgb, su, e_su, sv, e_sv, 255.0)
    m = run.cmp(R._CONF, alln, conf > 0.001, conf - 0.001, e_conf, ~oob)
    big |= b & ~m                                                           # (the tap at (su, sv) is read only where nothing is in-painted)
    if m.any():
        w = np.nonzero(m)[0]
        if mode == "Interleaved":
            flo, fhi = _inpaint(g, rgb, dep, u[w], v[w], -d[w], e_d[w], parx, pary, 1.0, w, run, big, dtap, 255.0)
        else:
            flo, fhi = _inpaint(g, rgb, dep, u[w], v[w], -d[w], e_d[w], c, s, -1.0 if eye > 0 else 1.0, w, run, big, dtap, 255.0)
        clo[w], chi[w] = flo, fhi                                           # the in-painting REPLACES the colour
    bx, ebx = _band((-0.001, 0.001), (1.001, 0.999), su, e_su)
    by, eby = _band((-0.001, 0.001), (1.001, 0.999), sv, e_sv)
    alo, ahi = np.minimum(bx - ebx, by - eby), np.minimum(bx + ebx, by + eby)
    lo, hi = _fx_out(g, x, y, clo, chi, alo, ahi)
    return lo, hi, big


def _eval_ana(g, rgb, dep, idx, run):
    """ana_pixel in float64 -> lo, hi [n, 4] (L.r, R.g, R.b, alpha), big [n]"""
    n = idx.size
    alln = np.arange(n)
    u32, v32, x, y = _uv(g, idx)
    u, v = u32.astype(F64), v32.astype(F64)
    c, s, psx, psy = float(g["c"]), float(g["s"]), float(g["psx"]), float(g["psy"])
    rolled = s != 0.0
    hi_, strength, conv = float(g["half_ipd"]), float(g["strength"]), float(g["conv"])
    big = np.zeros(n, bool)
    dtap = _mk_dtap(dep, big, float(np.abs(dep).max()))
    d, e_d = _smooth_depth(u, v, c * psx * 1.5, s * psy * 1.5, dtap)
    shift = -d + conv                                                       # no depth shaping
    e_shift = e_d + U * np.abs(shift)
    fall = _fall002(u)
    sa = shift * strength * fall
    e_sa = abs(strength) * (fall * e_shift + np.abs(shift) * 20 * U) + 3 * U * np.abs(sa)
    ox, oy = hi_ * sa * c, hi_ * sa * s
    e_ox, e_oy = abs(hi_ * c) * e_sa + 3 * U * np.abs(ox), (abs(hi_ * s) * e_sa + 3 * U * np.abs(oy)) * rolled
    live = np.ones(n, bool)
    eyes = []
    for sign, rr in ((1.0, run), (-1.0, _Shift(run, _RIGHT))):             # left: uv + o, right: uv - o
        eu_, ev_ = u + sign * ox, v + sign * oy
        e_u, e_v = e_ox + U * np.abs(eu_), (e_oy + U * np.abs(ev_)) * rolled
        occ = (rr.cmp(R._SU0, alln, eu_ < 0, eu_, e_u, live) | rr.cmp(R._SV0, alln, ev_ < 0, ev_, e_v, live)
               | rr.cmp(R._SU1, alln, eu_ > 1, eu_ - 1, e_u, live) | rr.cmp(R._SV1, alln, ev_ > 1, ev_ - 1, e_v, live))
        eyes.append([eu_, e_u, ev_, e_v, occ, rr])
    both = eyes[0][4] & eyes[1][4]
    s2x, s2y = c * psx * 2.0, s * psy * 2.0
    (ua, eua), (va_, eva) = _off(u, s2x, 3), _off(v, s2y, 3)
    (ub, eub), (vb, evb) = _off(u, -s2x, 3), _off(v, -s2y, 3)
    dA, eA = dtap(ua, eua, va_, eva)
    dB, eB = dtap(ub, eub, vb, evb)
    jmp = np.abs(dA - dB)
    thr = float(F32(0.08))
    jump = run.cmp(_JUMP, alln, jmp > thr, jmp - thr, eA + eB + U * jmp, ~both) & ~both
    clo, chi = np.zeros((n, 3)), np.zeros((n, 3))
    alo, ahi = np.full(n, np.inf), np.full(n, np.inf)
    for k, (eu_, e_u, ev_, e_v, occ, rr) in enumerate(eyes):
        occ = occ | jump
        _, lo, hi, b = tex_range(rgb, eu_, e_u, ev_, e_v, 255.0)
        big |= b & ~occ
        if occ.any():
            w = np.nonzero(occ)[0]
            flo, fhi = _inpaint(g, rgb, dep, u[w], v[w], -d[w], e_d[w], c, s, 1.0 if k == 0 else -1.0, w, rr, big, dtap, 255.0)
            lo[w], hi[w] = flo, fhi
        ch = [0] if k == 0 else [1, 2]
        clo[:, ch], chi[:, ch] = lo[:, ch], hi[:, ch]
        e015, e985 = float(F32(0.015)), float(F32(0.985))
        for t, et in ((eu_, e_u), (ev_, e_v)):
            bb, eb = _band((0.0, e015), (1.0, e985), t, et)
            alo, ahi = np.minimum(alo, bb - eb), np.minimum(ahi, bb + eb)
    lo, hi = _fx_out(g, x, y, clo, chi, alo, ahi)
    return lo, hi, big


KEYS = np.array([[0.0, 0.298, 0.651], [0.0, 0.5, 0.0], [1.0, 0.851, 0.0], [0.988, 0.0, 0.0]], F32).astype(F64)


def _eval_dm(g, dep, idx, run):
    """depth_map_kernel's pixel in float64 -> lo, hi [n, 4], big"""
    n = idx.size
    u32, v32, _, _ = _uv(g, idx)
    t, tlo, thi, big = tex_range(dep, u32.astype(F64), 0.0, v32.astype(F64), 0.0, float(np.abs(dep).max()))
    e_t = np.maximum(thi - t, t - tlo)
    wl, wh = [], []
    for k in (0.125, 0.375, 0.625, 0.875):
        a = np.abs(t - k)
        raw, e = 1.0 - 4.0 * a, 4 * (e_t + U * a) + U * np.abs(1.0 - 4.0 * a)
        wl.append(np.maximum(0.0, raw - e))
        wh.append(np.maximum(0.0, raw + e))
    wl, wh = np.stack(wl, 1), np.stack(wh, 1)
    tot_lo, tot_hi = wl.sum(1) * (1 - 3 * U), wh.sum(1) * (1 + 3 * U)
    und = ~(tot_lo > 0) & ~(tot_hi == 0)
    pos = run.cmp(0, np.arange(n), tot_hi > 0, np.where(und, 0.0, 1.0), np.zeros(n), np.ones(n, bool))
    safe_lo = np.where(tot_lo > 0, tot_lo, 1.0)
    nl = np.where(pos[:, None], wl / np.maximum(tot_hi, 1e-300)[:, None] * (1 - U), wl)
    nh = np.where(pos[:, None], np.where((tot_lo > 0)[:, None], np.minimum(wh / safe_lo[:, None] * (1 + U), 1.0), (wh > 0) * 1.0), wh)
    lo = (nl @ KEYS) * 255.0 * (1 - 8 * U)
    hi = (nh @ KEYS) * 255.0 * (1 + 8 * U)
    one = np.ones((n, 1))
    return np.concatenate([lo, one], 1), np.concatenate([hi, one], 1), big


def _classify(fn, idx, lo, hi, valid, cls):
    """fn(idx, run) -> lo, hi [n, 4], big for the flat pixels idx; fills lo, hi [4, N, 4], valid [4, N], cls [N] at idx"""
    run = _Run(idx.size)
    l0, h0, big = fn(idx, run)
    lo[:, idx], hi[:, idx] = l0[None], h0[None]
    valid[0, idx] = True
    k_ = np.where(big | (run.nund > 2), 2, np.where(run.nund > 0, 1, 0))
    br = np.nonzero(k_ == 1)[0]
    if br.size:
        f1, f2 = run.ids[br, 0], run.ids[br, 1]
        for k, (b1, b2) in enumerate(itertools.product((False, True), repeat=2)):
            sub = _Run(br.size, (f1, f2, b1, b2))
            l, h, bg = fn(idx[br], sub)
            lo[k, idx[br]], hi[k, idx[br]] = l, h
            valid[k, idx[br]] = True
            k_[br[sub.extra | bg]] = 2
    cls[idx] = k_


def reference(c, mode, rgb, depth):
    """every frame -> lo, hi [B, 4, oh, ow, 4], valid [B, 4, oh, ow], cls [B, oh, ow] (0 decided, 1 branch-judged, 2 exempt): dibr_ref.judge's input"""
    g = geom(c)
    N, sh = g["oh"] * g["ow"], (g["oh"], g["ow"])
    out = {k: [] for k in ("lo", "hi", "valid", "cls")}
    for b in range(depth.shape[0]):
        dep = depth_texels(c, depth[b]).astype(F64)
        lo, hi, valid, cls = np.zeros((4, N, 4)), np.zeros((4, N, 4)), np.zeros((4, N), bool), np.zeros(N, np.int64)
        allp = np.arange(N)
        if mode == "Depth Map":
            _classify(lambda i, r: _eval_dm(g, dep, i, r), allp, lo, hi, valid, cls)
        elif mode == "Anaglyph":
            col = rgb[b].astype(F64)
            _classify(lambda i, r: _eval_ana(g, col, dep, i, r), allp, lo, hi, valid, cls)
        else:
            col = rgb[b].astype(F64)
            y, x = np.divmod(allp, g["ow"])
            e = eye_dir(g, mode, x, y)
            for eye in (-1.0, 1.0):
                sel = allp[e == eye]
                if sel.size:
                    _classify(lambda i, r, eye=eye: _eval_il(g, mode, col, dep, eye, i, r), sel, lo, hi, valid, cls)
        out["lo"].append(lo.reshape(4, *sh, 4))
        out["hi"].append(hi.reshape(4, *sh, 4))
        out["valid"].append(valid.reshape(4, *sh))
        out["cls"].append(cls.reshape(sh))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the float32 emulation (kernel forms)
MUTANTS = ("tap_off_one", "repeat_clamp", "parity_no_origin", "parity_output_row", "eyes_swapped", "sweep_other_program", "ana_f1_shaping",
           "ana_channels", "ana_jump_006", "conf_edges_f1", "inpaint_mixed", "edge_margin_005", "ana_border_001", "feather_no_origin",
           "no_premult", "updep_align_corners", "u8_trunc", "corner_pixel", "wrong_row", "win_neighbour", "wx0_tpc1", "dm_no_norm",
           "dm_straddle", "dm_tail_dropped")
EQUIVALENT = ("feather_no_flip", "feather_on_uv")          # the same picture by symmetry (module docstring): the judge must ACCEPT them


class _Taps:
    """the samplers: own() = a tap on the pixel's own row pair (through the LDS window in the row kernel), any() = the vertical taps"""
    def __init__(self, g, rgb, dep, x, mut, plan):
        self.g, self.rgb, self.dep, self.mut, self.clamp = g, rgb, dep, mut, mut == "repeat_clamp"
        self.wx0 = self.delta = None
        if mut in ("win_neighbour", "wx0_tpc1"):
            assert plan["rows"], "a window error needs the row kernel"
            xb = (x // plan["cols"]) * plan["cols"]
            ub = ((xb.astype(F32) + F32(0.5)) / F32(g["ow"])).astype(F32)
            self.wx0 = np.floor((ub * F32(g["W"])).astype(F32) - F32(0.5)).astype(np.int64) - plan["margin"]
            self.WW = plan["WW"]
            self.delta = (xb - plan["margin"]) - self.wx0          # staged from a wx0 formed with one texel per column, read with the right one

    def sub(self, m):
        t = _Taps.__new__(_Taps)
        t.__dict__.update(self.__dict__)
        if self.wx0 is not None:
            t.wx0, t.delta = self.wx0[m], self.delta[m]
        return t

    def own(self, img, u, v, xoff=0):
        if self.mut == "win_neighbour":
            return R._tex32(img, u, v, clamp=self.clamp, xoff=xoff, win=(self.wx0, self.WW))
        if self.mut == "wx0_tpc1":
            j = np.floor((u * F32(self.g["W"])).astype(F32) - F32(0.5)).astype(np.int64) - self.wx0
            xoff = np.where((j >= 0) & (j < self.WW - 1), self.delta, 0)
        return R._tex32(img, u, v, clamp=self.clamp, xoff=xoff)

    def any(self, img, u, v):
        return R._tex32(img, u, v, clamp=self.clamp)


def _f(x):
    return np.asarray(x, F32)


def _emu_inpaint(g, T, u, v, cdi, eye, mode, mut):
    """comp_push_pull in float32 for flat pixels of eye_dir `eye` [n]"""
    n = u.size
    psx, psy, tol, blur, c, s = g["psx"], g["psy"], g["tol"], g["blur"], g["c"], g["s"]
    il = (mode == "Interleaved") != (mut == "sweep_other_program" and mode != "Anaglyph")
    kx, ky = (_f(c * _f(eye)) * psx).astype(F32), (_f(s * _f(eye)) * psx).astype(F32)
    sd = np.where(eye > 0, -1, 1)

    def step(i):
        if il:
            return (kx * F32(i)).astype(F32), (ky * F32(i)).astype(F32)
        t = ((sd * i).astype(F32) * psx).astype(F32)
        return (t * c).astype(F32), (t * s).astype(F32)
    best, bw = np.zeros((n, 3), F32), np.zeros(n, F32)
    active = np.ones(n, bool)
    for i in range(1, g["search"] + 1):
        du, dv = step(i)
        tu, tv = (u + du).astype(F32), (v + dv).astype(F32)
        ok = active & ~((tu < 0) | (tv < 0) | (tu > 1) | (tv > 1))
        sdi = (F32(1) - T.own(T.dep, tu, tv)).astype(F32)
        ok &= sdi > (cdi + tol).astype(F32)
        w = (g["w1"][i] * (F32(1) + ((sdi - cdi).astype(F32) * F32(10)).astype(F32)).astype(F32)).astype(F32)
        col = T.own(T.rgb, tu, tv)
        best = np.where(ok[:, None], (best + (col * w[:, None]).astype(F32)).astype(F32), best)
        bw = np.where(ok, (bw + w).astype(F32), bw)
        active &= ~(ok & (bw > F32(5)))
    need2 = bw < F32(2)
    for i in range(1, g["search"] + 1):
        du, dv = step(i)
        tu, tv = (u - du).astype(F32), (v - dv).astype(F32)
        ok = need2 & ~((tu < 0) | (tv < 0) | (tu > 1) | (tv > 1))
        sdi = (F32(1) - T.own(T.dep, tu, tv)).astype(F32)
        ok &= sdi > (cdi + tol).astype(F32)
        w = g["w2"][i]
        col = T.own(T.rgb, tu, tv)
        best = np.where(ok[:, None], (best + (col * w).astype(F32)).astype(F32), best)
        bw = np.where(ok, (bw + w).astype(F32), bw)
    has = bw > F32(0.01)
    va = ((best / np.where(has, bw, F32(1))[:, None]).astype(F32) * F32(0.5)).astype(F32)
    vw = np.full(n, 0.5, F32)
    for dy in (-1.0, 1.0):
        vv = (v + F32(F32(F32(dy) * psy) * blur)).astype(F32)
        ok = has & (vv >= 0) & (vv <= 1)
        vs_ = np.where(ok, vv, v)
        vdi = (F32(1) - T.any(T.dep, u, vs_)).astype(F32)
        ok &= vdi > (cdi + F32(tol * F32(0.5))).astype(F32)
        col = T.any(T.rgb, u, vs_)
        va = np.where(ok[:, None], (va + (col * F32(0.25)).astype(F32)).astype(F32), va)
        vw = np.where(ok, (vw + F32(0.25)).astype(F32), vw)
    return np.where(has[:, None], (va / vw[:, None]).astype(F32), T.own(T.rgb, u, v)).astype(F32)


def _emu_fx(g, x, y, u, v, col, alpha, mut):
    fu, fv = (u, v) if mut == "feather_on_uv" else _fuv(g, x, y, mut)
    if g["feather"]:
        fw = g["feather_w"]
        fo = (((R._ss_div(0, fw, fu) * R._ss_div(0, fw, (F32(1) - fu).astype(F32))).astype(F32) * R._ss_div(0, fw, fv)).astype(F32)
              * R._ss_div(0, fw, (F32(1) - fv).astype(F32))).astype(F32)
        col = (col * np.power(fo, F32(0.7)).astype(F32)[:, None]).astype(F32)
    if g["corner_r"] > 0:
        r = g["corner_r"]
        dx = ((np.abs(fu - F32(0.5)) - F32(0.5)).astype(F32) + r).astype(F32)
        dy = ((np.abs(fv - F32(0.5)) - F32(0.5)).astype(F32) + r).astype(F32)
        mx, my = np.maximum(dx, F32(0)), np.maximum(dy, F32(0))
        sdf = ((np.sqrt(((mx * mx).astype(F32) + (my * my).astype(F32)).astype(F32)).astype(F32) + np.minimum(np.maximum(dx, dy), F32(0))).astype(F32) - r).astype(F32)
        alpha = np.minimum(alpha, (F32(1) - R._ss_div(0.0, 0.01, sdf)).astype(F32))
    return col, alpha


def _smooth32(T, u, v, dsx, dsy):
    d0, dm, dp = T.own(T.dep, u, v), T.own(T.dep, (u - dsx).astype(F32), (v - dsy).astype(F32)), T.own(T.dep, (u + dsx).astype(F32), (v + dsy).astype(F32))
    return (((d0 * F32(0.7)).astype(F32) + (dm * F32(0.15)).astype(F32)).astype(F32) + (dp * F32(0.15)).astype(F32)).astype(F32)


def _fall32(u, mut):
    e = 0.05 if mut == "edge_margin_005" else 0.02
    return (R._ss_inv(0.0, e, u) * R._ss_inv(1.0, float(F32(1.0) - F32(e)) if mut == "edge_margin_005" else 0.98, u)).astype(F32)


def emulate_frame(g, mode, rgb_u8, dep, mut=None, plan=None):
    """one frame in float32 -> [oh, ow, 4]: frag_color's rgb (0..255) and alpha, un-multiplied"""
    oh, ow = g["oh"], g["ow"]
    n = oh * ow
    u, v, x, y = _uv(g, np.arange(n))
    if mode == "Depth Map":
        t = R._tex32(dep, u, v)
        w = [np.maximum(F32(0), (F32(1) - (np.abs(t - F32(k)) * F32(4)).astype(F32)).astype(F32)) for k in (0.125, 0.375, 0.625, 0.875)]
        total = (((w[0] + w[1]).astype(F32) + w[2]).astype(F32) + w[3]).astype(F32)
        if mut != "dm_no_norm":
            pos = total > 0
            w = [np.where(pos, (wk / np.where(pos, total, F32(1))).astype(F32), wk) for wk in w]
        K = KEYS.astype(F32)
        col = np.stack([((((K[0, k] * w[0]).astype(F32) + (K[1, k] * w[1]).astype(F32)).astype(F32) + (K[2, k] * w[2]).astype(F32)).astype(F32)
                         + (K[3, k] * w[3]).astype(F32)).astype(F32) * F32(255) for k in range(3)], 1).astype(F32)
        return np.concatenate([col, np.ones((n, 1), F32)], 1).reshape(oh, ow, 4)
    T = _Taps(g, rgb_u8.astype(F32), dep, x, mut, plan)
    c, s, psx, psy = g["c"], g["s"], g["psx"], g["psy"]
    xo = 1 if mut == "tap_off_one" else 0
    if mode == "Anaglyph":
        dsx, dsy = F32(F32(c * psx) * F32(1.5)), F32(F32(s * psy) * F32(1.5))
        d = _smooth32(T, u, v, dsx, dsy)
        dinv = -d
        sh = (dinv * (F32(1) + (F32(0.35) * (F32(1) - d).astype(F32)).astype(F32)).astype(F32)).astype(F32) if mut == "ana_f1_shaping" else dinv
        sa = (((sh + g["conv"]).astype(F32) * g["strength"]).astype(F32) * _fall32(u, mut)).astype(F32)
        ox, oy = ((g["half_ipd"] * sa).astype(F32) * c).astype(F32), ((g["half_ipd"] * sa).astype(F32) * s).astype(F32)
        lu, lv, ru, rv = (u + ox).astype(F32), (v + oy).astype(F32), (u - ox).astype(F32), (v - oy).astype(F32)
        if mut == "eyes_swapped":
            lu, lv, ru, rv = ru, rv, lu, lv
        oobf = lambda a, b: (a < 0) | (b < 0) | (a > 1) | (b > 1)
        occl, occr = oobf(lu, lv), oobf(ru, rv)
        s2x, s2y = F32(F32(c * psx) * F32(2.0)), F32(F32(s * psy) * F32(2.0))
        jump = np.abs(T.own(T.dep, (u + s2x).astype(F32), (v + s2y).astype(F32)) - T.own(T.dep, (u - s2x).astype(F32), (v - s2y).astype(F32))) \
            > F32(0.06 if mut == "ana_jump_006" else 0.08)
        jump &= ~(occl & occr)
        cols = []
        for eu_, ev_, occ, eye in ((lu, lv, occl | jump, -1.0), (ru, rv, occr | jump, 1.0)):
            if mut == "eyes_swapped":
                eye = -eye
            col = T.own(T.rgb, eu_, ev_, xoff=xo)
            if occ.any():
                col[occ] = _emu_inpaint(g, T.sub(occ), u[occ], v[occ], dinv[occ], np.full(int(occ.sum()), eye), mode, mut)
            cols.append(col)
        L, Rr = (cols[1], cols[0]) if mut == "ana_channels" else (cols[0], cols[1])
        col = np.stack([L[:, 0], Rr[:, 1], Rr[:, 2]], 1).astype(F32)
        e0, e1 = (0.001, 0.999) if mut == "ana_border_001" else (0.015, 0.985)
        band = lambda t: (R._ss_inv(0.0, e0, t) * R._ss_inv(1.0, e1, t)).astype(F32)
        alpha = np.minimum(np.minimum(band(lu), band(lv)), np.minimum(band(ru), band(rv))).astype(F32)
    else:
        eye = eye_dir(g, mode, x, y, mut).astype(F32)
        my_off = (eye * g["half_ipd"]).astype(F32)
        parx, pary = (c * eye).astype(F32), (s * eye).astype(F32)
        dsx, dsy = ((parx * psx).astype(F32) * F32(1.5)).astype(F32), ((pary * psy).astype(F32) * F32(1.5)).astype(F32)
        d = _smooth32(T, u, v, dsx, dsy)
        dinv = -d
        shaped = (dinv * (F32(1) + (F32(0.35) * (F32(1) - d).astype(F32)).astype(F32)).astype(F32)).astype(F32)
        shift = (shaped + g["conv"]).astype(F32)
        px = (((my_off * shift).astype(F32) * g["strength"]).astype(F32) * _fall32(u, mut)).astype(F32)
        su, sv = (u - (px * c).astype(F32)).astype(F32), (v - (px * s).astype(F32)).astype(F32)
        oob = (su < 0) | (su > 1) | (sv < 0) | (sv > 1)
        s2x, s2y = ((parx * psx).astype(F32) * F32(2.0)).astype(F32), ((pary * psy).astype(F32) * F32(2.0)).astype(F32)
        jump = np.abs(T.own(T.dep, (u - s2x).astype(F32), (v - s2y).astype(F32)) - T.own(T.dep, (u + s2x).astype(F32), (v + s2y).astype(F32)))
        ce = (0.04, 0.10) if mut == "conf_edges_f1" else (0.06, 0.12)
        conf = np.where(oob, F32(1), R._ss_inv(ce[0], ce[1], jump)).astype(F32)
        col = T.own(T.rgb, su, sv, xoff=xo)
        m = conf > F32(0.001)
        if m.any():
            fill = _emu_inpaint(g, T.sub(m), u[m], v[m], dinv[m], eye[m], mode, mut)
            if mut == "inpaint_mixed":
                cm = conf[m][:, None]
                fill = ((col[m] * (F32(1) - cm).astype(F32)).astype(F32) + (fill * cm).astype(F32)).astype(F32)
            col[m] = fill
        bx = (R._ss_inv(-0.001, 0.001, su) * R._ss_inv(1.001, 0.999, su)).astype(F32)
        by = (R._ss_inv(-0.001, 0.001, sv) * R._ss_inv(1.001, 0.999, sv)).astype(F32)
        alpha = np.where((su < F32(0.001)) | (su > F32(0.999)) | (sv < F32(0.001)) | (sv > F32(0.999)), np.minimum(bx, by), F32(1)).astype(F32)
    col, alpha = _emu_fx(g, x, y, u, v, col, alpha, mut)
    return np.concatenate([col, alpha[:, None]], 1).astype(F32).reshape(oh, ow, 4)


def emulate(c, mode, rgb, depth, alpha="window", u8=False, mut=None, plan=None):
    """the float32 emulation of the whole call (kernel forms; mut: one deliberate error) -> what ops.dibr_composite returns"""
    g = geom(c)
    B = depth.shape[0]
    deps = [depth_texels(c, depth[b], mut) for b in range(B)]
    outs = []
    for b in range(B):
        o = emulate_frame(g, mode, rgb[b], deps[b], mut, plan)
        if mut == "corner_pixel":
            o[-1, -1, :3] = o[-1, -2, :3]
        if mut == "wrong_row":
            o[o.shape[0] // 3] = o[o.shape[0] // 3 + 1]
        outs.append(o)
    out = np.stack(outs)
    if mut == "dm_straddle":          # a thread = four consecutive pixels of the flattened output; its first pixel's frame serves all four
        img = g["oh"] * g["ow"]
        flat = out.reshape(-1, 4)
        p = np.arange(flat.shape[0])
        b0, bb = (p // 4 * 4) // img, p // img
        for q in p[b0 != bb]:
            flat[q] = emulate_frame(g, mode, None, deps[b0[q]], None, None).reshape(-1, 4)[q - bb[q] * img]
    res = R.store(out, alpha, u8, mut)
    if mut == "dm_tail_dropped":
        tail = res.reshape(-1, res.shape[-1])
        tail[(tail.shape[0] // 4) * 4:] = 0
    return res
