"""Float64 references, bounds, judges, emulations and input families of the frame-side kernel tests (frame_ops.hip: test_gpu_frame_ops.py
on the device, test_cpu_frame_ref.py on the host).  numpy only.

OPERANDS.  What is discrete and bit-reproducible in the kernels is restated in float32 and is an operand of the reference, not part of
its error: linear_tap (csrc/common.h: multiply, add and subtract rounded separately -> two indices and two weights), the geometry of a
bicubic-antialias axis (aa_cubic_taps: scale, support, center, xmin, xsize -- one float32 operation each, then the double + 0.5
truncation), the float32 parameters (mean, std, ratio, convergence, max_px = float32(ipd_uv W), the constant 0.05f).  Everything else is
float64.  u = 2^-24; g(k) = k u / (1 - k u) bounds k successive float32 roundings of a sum of products.

BOUNDS (derived from each kernel's arithmetic; nothing here was measured on the code under test -- test_cpu_frame_ref.py checks that
float32 / integer emulations pass and that deliberate errors do not).

 preprocess_kernel, preprocess_patch_kernel: v = wy0 (wx0 a + wx1 c) + wy1 (wx0 d + wx1 e): every pixel goes through 4 roundings (product,
   sum, product, sum) and all terms are >= 0: |v - V| <= g(4) V.  q = v / 255, t = q - mean, o = t / std are one rounding each:
   dq = g(4) V / 255 + u |q|, dt = dq + u |t|, delta = dt / std + u |o|  (each |.| taken at reference + its own error).  bf16 rows: the
   stored value lies in RNE_bf16([ref - delta, ref + delta]).
 upsample_depth_kernel: the same 4 roundings with signed values: delta = g(4) sum |w| |v|.
 preprocess_aa_kernel: a raw Keys weight is a float32 polynomial of x = |(j - center + 0.5) invscale|: x carries <= 11 u (two sums of
   magnitude <= 2 scale + 1.5 scaled by invscale <= 1 / scale: <= 7 u, the product and invscale's own rounding: <= 4 u as x < 2 where the
   weight is not 0), |dw/dx| <= 25/18 < 1.5, and Horner's five operations on magnitudes <= 4 add <= 40 u: EW = 57 u per raw weight.  The
   normaliser T = sum of n raw weights: dT <= n EW + g(n) sum |raw|; w / T is one more rounding:
   |dw_j| <= a + b |w_j|, a = EW / |T|, b = dT / |T| + u.  A pass accumulates n products in order: g(n + 1) sum |w| |p|.  With
   AH = sum_x |wx| |p|, SH = sum over the window of |p|:
       d_acc = sum_y |wy| (a_x SH + (b_x + g(nx + 1)) AH)   +   sum_y (a_y [y in window] + (b_y + g(ny + 1)) |wy|) AH
   (negative lobes: every term is scaled by sum |w| |p|, never by the value), then / 255, - mean, / std as above.
 stereo_warp_generic (and the gather kernel's float path wg_slow_row): one term per rounding of the coordinate:
       eps_x = |K| (g(4) sum |w| |depth| + u |d|)        depth blend (4 roundings), d = blend - conv
             + 3 u |shift|                               the three products (-d ratio) max_px 0.05f
             + u (|x| + |shift|)                         x + sign shift: half an ulp at |x| + |shift|
             + u (W - 1)                                 span - (x - span) / span - extra of a reflection
     K = ratio max_px 0.05.  w1 = sx - x0 is exact, w0 = 1 - w1 one rounding, w0 p0 + w1 p1 three more: delta_b = g(4) 255 per sample,
     g(5) 255 for the mean of a Half-mode pair ((a + b) one rounding, 0.5 exact).  u8 output: v_cvt_pk_u8_f32, round-half-even.
 stereo_warp_gather (16.16 fixed point): a depth COLUMN becomes a fixed-point shift first, scol = fma(fma(wy1, d1, wy0 d0), K', ck) with
     K' = ((-ratio max_px) 0.05f) 65536 (3 roundings), ck = -conv K' (1 more): e_col <= |K'| (g(2) + g(3)) A + g(4) |ck| + u |scol|,
     A = sum |wy| |depth|; a pixel is scol[0] + sum_j wkj (scol[j+1] - scol[j]) (NC - 1 fused multiply-adds on column differences, partial
     sums are columns' convex combinations, |.| <= M = max |scol|): e_sh <= (2 NC - 1) max e_col + 3 (NC - 1) u M.  Then
       eps_x = e_sh / 65536 + 2^-16 ((int)sh truncates) + 2^-16 (s <= span_fx - 1 at the right edge)
     and a channel is (p0 (65535 - w1) + p1 w1 + 32768) >> 16 = round-half-up(E(s / 65536) - p0 2^-16): delta_b = 255 2^-16 (p0 <= 255 for every element: at most 0.004 of a level above the
     element's own p0 2^-16); the Half
     modes shift the pair's sum right by one first: + 2^-17.  Bounds are taken with NC = 4 and the row's largest A.  A wave-row may take
     the float path on the kernel's own float32 decision, so gather outputs are judged with the larger of the two eps_x / delta_b.
 u8 judge: E(s) = the two-tap blend is piecewise linear with knots at the integers; [v_lo, v_hi] = its range over [sx - eps_x, sx + eps_x]
   (clipped to [0, W - 1]), taken at the end points and every knot inside: exact, no gradient estimate.  A byte n is accepted iff
   ceil(v_lo - delta_b - 1/2) <= n <= floor(v_hi + delta_b + 1/2): a tie inside the interval admits both bytes, whichever rounding the
   kernel uses.  Half modes: both samples' intervals are averaged.  Per element, no element exempt, no fraction-of-pixels allowance.
"""

import numpy as np

F32 = np.float32
U = 2.0 ** -24
C05 = float(F32(0.05))
MODES = {"Half-SBS": 0, "Full-SBS": 1, "Half-TAB": 2, "Full-TAB": 3}


def g(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ operands
def linear_tap(n_out, in_size, *, align_corners=False):
    """csrc/common.h linear_tap for dst = 0 .. n_out - 1, scale = linear_scale(in_size, n_out): float32 step by step.
    -> i0, i1 (int64), w0, w1 (float32)"""
    dst = np.arange(n_out).astype(F32)
    if align_corners:
        scale = F32(in_size - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        src = (scale * dst).astype(F32)
    else:
        scale = F32(in_size) / F32(n_out)
        src = ((scale * (dst + F32(0.5))).astype(F32) - F32(0.5)).astype(F32)
        src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    w1 = (src - i0.astype(F32)).astype(F32)
    w0 = (F32(1) - w1).astype(F32)
    return i0, i1, w0, w1


def aa_axis(n_out, in_size, *, dt=np.float64, normalise=True):
    """aa_cubic_taps for every output index: dense [n_out, in_size] weight matrix in dt (float64: the reference's weights from the kernel's
    float32 geometry; float32: the kernel's own arithmetic), the window mask, and the bound's (a, b, n) per output index."""
    scale = F32(in_size) / F32(n_out)
    support = F32(2) * scale if scale >= 1 else F32(2)
    invscale = F32(1) / scale if scale >= 1 else F32(1)
    Wm = np.zeros((n_out, in_size), dt)
    mask = np.zeros((n_out, in_size), bool)
    a_b_n = np.zeros((n_out, 3))
    for i in range(n_out):
        center = F32(scale * (F32(i) + F32(0.5)))
        lo = int(float(F32(center - support)) + 0.5)
        hi = int(float(F32(center + support)) + 0.5)
        xmin = max(lo, 0)
        xsize = min(min(hi, in_size) - xmin, 64)
        j = np.arange(xmin, xmin + xsize)
        if dt == np.float64:
            x = np.abs((j - float(center) + 0.5) * float(invscale))
        else:
            x = np.abs((((j.astype(F32) - center).astype(F32) + F32(0.5)).astype(F32) * invscale).astype(F32))
        a = dt(-0.5)
        near = ((a + dt(2)) * x - (a + dt(3))) * x * x + dt(1)
        far = ((a * x - dt(5) * a) * x + dt(8) * a) * x - dt(4) * a
        raw = np.where(x < 1, near, np.where(x < 2, far, dt(0))).astype(dt)
        if dt == np.float64:
            T = raw.sum()
        else:
            T = F32(0)
            for v in raw:
                T = F32(T + v)
        wts = raw / T if (normalise and T != 0) else raw
        Wm[i, j] = wts
        mask[i, j] = True
        EW = 57 * U
        dT = xsize * EW + g(xsize) * float(np.abs(raw).sum())
        a_b_n[i] = (EW / abs(float(T)), dT / abs(float(T)) + U, xsize)
    return Wm, mask, a_b_n


def aa_taps_needed(in_size, n_out):
    """the launcher's tap count for an axis: (int)(2 support) + 2 (d2s_preprocess rejects > 64)"""
    scale = F32(in_size) / F32(n_out)
    support = F32(2) * scale if scale >= 1 else F32(2)
    return int(F32(2) * support) + 2


# ------------------------------------------------------------------------------------------------ pre-process / up-sample
def _norm_tail(v, dv, mean, std, dt):
    """(v / 255 - mean) / std on [B,h,w,3] in dt; with dv (float64 bound of v): -> (out, delta)"""
    mean = np.asarray(mean, F32).astype(dt)
    std = np.asarray(std, F32).astype(dt)
    q = (v / dt(255)).astype(dt)
    t = (q - mean).astype(dt)
    o = (t / std).astype(dt)
    if dv is None:
        return o, None
    dq = dv / 255 + U * (np.abs(q) + dv / 255)
    dtt = dq + U * (np.abs(t) + dq)
    delta = dtt / std + U * (np.abs(o) + dtt / std)
    return o, delta


def preprocess_bilinear(px, stride, h, w, mean, std, *, dt=np.float64, mut=None):
    """preprocess_kernel on px [B,H,W,3] (pixel values as float64) -> out [B,3,h,w] in dt and, for float64, delta."""
    B, H, W, _ = px.shape
    Hs, Ws = -(-H // stride), -(-W // stride)
    if mut == "decim_floor":
        Hs, Ws = max(H // stride, 1), max(W // stride, 1)
    ac = mut == "align_corners"
    y0, y1, wy0, wy1 = linear_tap(h, Hs, align_corners=ac)
    x0, x1, wx0, wx1 = linear_tap(w, Ws, align_corners=ac)
    p = px.astype(dt)
    wy0, wy1 = wy0.astype(dt)[None, :, None, None], wy1.astype(dt)[None, :, None, None]
    wx0, wx1 = wx0.astype(dt)[None, None, :, None], wx1.astype(dt)[None, None, :, None]
    r0, r1 = p[:, y0 * stride], p[:, y1 * stride]
    top = (wx0 * r0[:, :, x0 * stride]).astype(dt) + (wx1 * r0[:, :, x1 * stride]).astype(dt)
    bot = (wx0 * r1[:, :, x0 * stride]).astype(dt) + (wx1 * r1[:, :, x1 * stride]).astype(dt)
    v = ((wy0 * top).astype(dt) + (wy1 * bot).astype(dt)).astype(dt)
    if mut == "mean_wrong_channel":
        mean, std = np.roll(np.asarray(mean), 1), np.roll(np.asarray(std), 1)
    o, delta = _norm_tail(v, g(4) * np.abs(v) if dt == np.float64 else None, mean, std, dt)
    o = np.ascontiguousarray(o.transpose(0, 3, 1, 2))
    return (o, np.ascontiguousarray(delta.transpose(0, 3, 1, 2))) if dt == np.float64 else o


def patch_rows(planes, p, Kp, *, mut=None):
    """[B,3,h,w] -> the im2col rows A[(b, py, px)][c p^2 + i p + j] = x[b][c][py p + i][px p + j] (vit_ops.hip), [B gh gw, Kp] with NaN in
    the columns >= 3 p^2 (never written)"""
    B, _, h, w = planes.shape
    gh, gw = h // p, w // p
    x = planes.reshape(B, 3, gh, p, gw, p)
    x = x.transpose(0, 2, 4, 1, 5, 3) if mut == "patch_ij_swap" else x.transpose(0, 2, 4, 1, 3, 5)
    A = np.full((B * gh * gw, Kp), np.nan)
    A[:, :3 * p * p] = x.reshape(B * gh * gw, 3 * p * p)
    return A


def preprocess_aa(px, h, w, mean, std, *, dt=np.float64, mut=None):
    """preprocess_aa_kernel: horizontal pass, then vertical, no clamp.  -> out [B,3,h,w] (+ delta for float64)"""
    B, H, W, _ = px.shape
    nrm = mut != "cubic_unnormalised"
    Wx, Mx, abx = aa_axis(w, W, dt=dt, normalise=nrm)
    Wy, My, aby = aa_axis(h, H, dt=dt, normalise=nrm)
    p = px.astype(dt)
    hp = np.einsum("byxc,ox->byoc", p, Wx).astype(dt)
    acc = np.einsum("byoc,ty->btoc", hp, Wy).astype(dt)
    dacc = None
    if dt == np.float64:
        AH = np.einsum("byxc,ox->byoc", np.abs(p), np.abs(Wx))
        SH = np.einsum("byxc,ox->byoc", np.abs(p), Mx.astype(float))
        ax, bx, nx = abx[:, 0][None, None, :, None], abx[:, 1][None, None, :, None], abx[:, 2][None, None, :, None]
        eh = ax * SH + (bx + g(nx + 1)) * AH
        ay, by, ny = aby[:, 0][:, None], aby[:, 1][:, None], aby[:, 2][:, None]
        Ey = ay * My + (by + g(ny + 1)) * np.abs(Wy)
        dacc = np.einsum("byoc,ty->btoc", eh, np.abs(Wy)) + np.einsum("byoc,ty->btoc", AH, Ey)
        dacc = dacc * (1 + 1e-6)                                    # the products of two first-order terms (each < 1e-5)
    o, delta = _norm_tail(acc, dacc, mean, std, dt)
    o = np.ascontiguousarray(o.transpose(0, 3, 1, 2))
    return (o, np.ascontiguousarray(delta.transpose(0, 3, 1, 2))) if dt == np.float64 else o


def upsample(d, H, W, *, dt=np.float64, mut=None):
    """upsample_depth_kernel: d [B,h,w] float32 -> [B,H,W] in dt (+ delta)"""
    B, h, w = d.shape
    ac = mut == "align_corners"
    y0, y1, wy0, wy1 = linear_tap(H, h, align_corners=ac)
    x0, x1, wx0, wx1 = linear_tap(W, w, align_corners=ac)
    v = d.astype(dt)
    wy0, wy1 = wy0.astype(dt)[None, :, None], wy1.astype(dt)[None, :, None]
    wx0, wx1 = wx0.astype(dt)[None, None, :], wx1.astype(dt)[None, None, :]

    def blend(v):
        r0, r1 = v[:, y0], v[:, y1]
        top = (wx0 * r0[:, :, x0]).astype(dt) + (wx1 * r0[:, :, x1]).astype(dt)
        bot = (wx0 * r1[:, :, x0]).astype(dt) + (wx1 * r1[:, :, x1]).astype(dt)
        return ((wy0 * top).astype(dt) + (wy1 * bot).astype(dt)).astype(dt)
    return (blend(v), g(4) * blend(np.abs(v))) if dt == np.float64 else blend(v)


# ------------------------------------------------------------------------------------------------ judges
def rne_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(np.where(x == 0, 1.0, np.abs(x)))
    q = np.ldexp(1.0, e - 8)
    return np.where(x == 0, 0.0, np.sign(x) * np.rint(np.abs(x) / q) * q)


def judge_float(out, ref, delta):
    """-> (ok mask, worst err / delta)"""
    err = np.abs(out.astype(np.float64) - ref)
    ok = (err <= delta) & np.isfinite(out)
    return ok, float((err / np.maximum(delta, 1e-300)).max()) if err.size else 0.0


def judge_bf16(out, ref, delta):
    out = out.astype(np.float64)
    ok = (out >= rne_bf16(ref - delta)) & (out <= rne_bf16(ref + delta)) & np.isfinite(out)
    m, e = np.frexp(np.maximum(np.abs(out), 2.0 ** -120))
    err = np.maximum(np.abs(out - ref) - np.ldexp(1.0, e - 9), 0)
    return ok, float((err / np.maximum(delta, 1e-300)).max()) if err.size else 0.0


def judge_range(out, lo, hi, db, u8):
    """out inside [lo - db, hi + db] (float outputs) / inside the bytes that interval rounds to (u8).  -> (ok, worst excess / db) where
    excess = distance of out from [lo, hi], less 1/2 for bytes"""
    o = out.astype(np.float64)
    if u8:
        ok = (o >= np.clip(np.ceil(lo - db - 0.5), 0, 255)) & (o <= np.clip(np.floor(hi + db + 0.5), 0, 255))
    else:
        ok = (o >= lo - db) & (o <= hi + db) & np.isfinite(o)
    exc = np.maximum(np.maximum(lo - o, o - hi) - (0.5 if u8 else 0.0), 0)
    return ok, float((exc / db).max()) if exc.size else 0.0


# ------------------------------------------------------------------------------------------------ warp
class Geom:
    """make_geom (frame_ops.hip): padding and packed output size"""

    def __init__(self, H, W, mode, fill):
        self.H, self.W, self.mode = H, W, mode
        self.Hp, self.Wp, self.pt, self.pl = H, W, 0, 0
        if fill:
            r_img, r_t = W / H, 16.0 / 9.0
            if not abs(r_img - r_t) < 1e-3:
                if r_img > r_t:
                    nh = int(np.rint(W / r_t)); self.pt = (nh - H) // 2; self.Hp = nh
                else:
                    nw = int(np.rint(H * r_t)); self.pl = (nw - W) // 2; self.Wp = nw
        self.tab = mode in ("Half-TAB", "Full-TAB")
        self.full = mode in ("Full-SBS", "Full-TAB")
        self.oh = 2 * self.Hp if self.full and self.tab else self.Hp
        self.ow = 2 * self.Wp if self.full and not self.tab else self.Wp


def depth_blend(depth, H, W, *, dt=np.float64, mut=None):
    """depth_at for every pixel: (sum w depth, sum |w| |depth|, row-max of the vertical part sum |wy| |depth| over columns)"""
    B, dh, dw = depth.shape
    y0, y1, wy0, wy1 = linear_tap(H, dh)
    x0, x1, wx0, wx1 = linear_tap(W, dw)
    if mut == "depth_row_plus1":
        y0, y1 = np.minimum(y0 + 1, dh - 1), np.minimum(y1 + 1, dh - 1)
    if mut == "nc3":                                               # a lane's 4 pixels take their pair from 3 columns c0 .. c0 + 2
        c0 = np.minimum(x0[(np.arange(W) // 4) * 4], dw - 3)
        x0, x1 = np.minimum(x0, c0 + 2), np.minimum(x1, c0 + 2)
    v = depth.astype(dt)
    if mut == "depth_frame_plus1":
        v = np.roll(v, -1, axis=0)
    wy0, wy1 = wy0.astype(dt)[None, :, None], wy1.astype(dt)[None, :, None]
    wx0, wx1 = wx0.astype(dt)[None, None, :], wx1.astype(dt)[None, None, :]

    def blend(v):
        r0, r1 = v[:, y0], v[:, y1]
        top = (wx0 * r0[:, :, x0]).astype(dt) + (wx1 * r0[:, :, x1]).astype(dt)
        bot = (wx0 * r1[:, :, x0]).astype(dt) + (wx1 * r1[:, :, x1]).astype(dt)
        return ((wy0 * top).astype(dt) + (wy1 * bot).astype(dt)).astype(dt)
    if dt != np.float64:
        return blend(v)
    av = np.abs(v)
    Acol = (wy0 * av[:, y0] + wy1 * av[:, y1]).max(axis=2)         # [B,H]
    return blend(v), blend(av), Acol


def reflect_clip(t, span):
    """reflect about [0, span] any number of times, then clip"""
    if span <= 0:
        return np.zeros_like(t)
    m = np.mod(np.abs(t), 2.0 * span)
    return np.clip(np.where(m <= span, m, 2.0 * span - m), 0.0, span)


def _E(img, pt):
    """two-tap blend of img [B,H,W,3] rows at float64 coordinates pt [B,H,W] (inside [0, W - 1])"""
    W = img.shape[2]
    if W == 1:
        return np.broadcast_to(img[:, :, :1], pt.shape + (3,)).astype(np.float64)
    x0 = np.clip(np.floor(pt).astype(np.int64), 0, W - 2)
    f = (pt - x0)[..., None]
    p0 = np.take_along_axis(img, x0[..., None], axis=2)
    p1 = np.take_along_axis(img, x0[..., None] + 1, axis=2)
    return p0 * (1 - f) + p1 * f


def warp_ref(px, depth, *, ipd_uv=0.064, ratio=2.0, conv=0.0, mode="Half-SBS", fill=False, kernel="generic"):
    """The float64 warp.  px [B,H,W,3] pixel values (float64; float input is clamped here), depth [B,dh,dw] float32.
    kernel: "generic" | "gather" (bounds only: the value is the same).  -> dict(lo, hi: [B,oh,ow,3] range of the exact value over the
    coordinate's error interval, db: delta_b, mid: the exact value, shift: [B,H,W] float64 pixel shifts, eps: [B,H,W], geom)"""
    B, H, W, _ = px.shape
    img = np.clip(px.astype(np.float64), 0.0, 255.0)
    gm = Geom(H, W, mode, fill)
    half = not gm.full
    ratio, conv = float(F32(ratio)), float(F32(conv))
    max_px = float(F32(ipd_uv * W))
    K = ratio * max_px * C05
    blend, A, Acol = depth_blend(depth, H, W)
    d = blend - conv
    shift = -d * K
    span = float(W - 1)
    xs = np.arange(W, dtype=np.float64)[None, None, :]
    eps = abs(K) * (g(4) * A + U * np.abs(d)) + 3 * U * np.abs(shift) + U * (xs + np.abs(shift)) + U * span
    db = (g(5) if half else g(4)) * 255.0
    if kernel == "gather":
        Kf = abs(K) * 65536.0
        ecol = Kf * (g(2) + g(3)) * Acol + g(4) * abs(conv) * Kf
        M = Kf * (Acol + abs(conv)) * (1 + g(8))
        ecol = ecol + U * M
        esh = 7 * ecol + 9 * U * M                                  # NC = 4
        eg = (esh / 65536.0 + 2.0 ** -15)[:, :, None]
        eps = np.maximum(eps, eg)
        db = max(db, 255.0 * 2.0 ** -16 + (2.0 ** -17 if half else 0.0))
    eyes = []
    for sign in (1.0, -1.0):
        sx = reflect_clip(xs + sign * shift, span)
        a, b = np.clip(sx - eps, 0, span), np.clip(sx + eps, 0, span)
        mid = _E(img, sx)
        va, vb = _E(img, a), _E(img, b)
        lo, hi = np.minimum(va, vb), np.maximum(va, vb)
        k0, k1 = np.ceil(a), np.floor(b)
        for j in range(int((k1 - k0).max()) + 1 if W > 1 else 0):    # every integer knot inside the interval
            kn = np.minimum(k0 + j, k1)
            inside = (k0 + j <= k1)[..., None]
            vk = _E(img, np.clip(kn, 0, span))
            lo, hi = np.where(inside, np.minimum(lo, vk), lo), np.where(inside, np.maximum(hi, vk), hi)
        eyes.append((lo, hi, mid))

    def pack(idx):
        pads = ((0, 0), (gm.pt, gm.Hp - H - gm.pt), (gm.pl, gm.Wp - W - gm.pl), (0, 0))
        l, r = np.pad(eyes[0][idx], pads), np.pad(eyes[1][idx], pads)
        cat = np.concatenate([l, r], axis=1 if gm.tab else 2)
        if half:                                                    # F.interpolate(mode='area') on the concatenated frame
            if gm.tab:
                cat = (cat[:, 0:2 * gm.oh:2] + cat[:, 1:2 * gm.oh:2]) * 0.5
            else:
                cat = (cat[:, :, 0:2 * gm.ow:2] + cat[:, :, 1:2 * gm.ow:2]) * 0.5
        return np.clip(cat, 0.0, 255.0)
    return {"lo": pack(0), "hi": pack(1), "mid": pack(2), "db": db, "shift": shift, "eps": eps, "geom": gm}


def warp_emulate(px, depth, *, ipd_uv=0.064, ratio=2.0, conv=0.0, mode="Half-SBS", fill=False, kind="f32", u8=True, mut=None):
    """kind "f32": stereo_warp_generic's float32 arithmetic; "fx": the gather kernel's blend -- 16.16 coordinate (truncated shift, one
    reflection per side, s <= span_fx - 1), weights 65535 - w1 | w1, + 32768, byte 2, the Half chains (+ 65536, >> 1).  -> the packed
    output (uint8 when u8 or kind == "fx", else float32).  mut: one deliberate error."""
    B, H, W, _ = px.shape
    gm = Geom(H, W, mode, fill)
    half = not gm.full
    img = np.clip(px.astype(np.float64), 0, 255).astype(F32)
    blend = depth_blend(depth, H, W, dt=F32, mut=mut)
    d = (blend - F32(conv)).astype(F32)
    max_px = F32(ipd_uv * W)
    shift = ((((-d) * F32(ratio)).astype(F32) * max_px).astype(F32) * F32(0.05)).astype(F32)
    span = F32(W - 1)
    xs = np.arange(W, dtype=F32)[None, None, :]
    rows = img
    if mut == "row_next_window":
        rows = img[:, np.minimum(np.arange(H) + 1, H - 1)]
    outs = []
    for sign in (1.0, -1.0):
        sg = F32(-sign if mut == "eye_swap" else sign)
        if kind == "f32":
            t = np.abs((xs + (sg * shift).astype(F32)).astype(F32))
            sp = F32(W) if mut == "reflect_W" else span
            if W == 1:
                sx = np.zeros_like(t)
            else:
                extra = np.fmod(t, sp).astype(F32)
                flips = np.floor((t / sp).astype(F32)).astype(np.int64)
                r = np.where(flips & 1, (sp - extra).astype(F32), extra)
                sx = np.where(t <= sp, t, np.clip(r, F32(0), sp)).astype(F32)
                sx = np.minimum(sx, span)
            x0 = sx.astype(np.int64)
            w1 = (sx - x0.astype(F32)).astype(F32)[..., None]
            w0 = (F32(1) - w1).astype(F32)
            x1 = np.minimum(x0 + 1, W - 1)
            p0 = np.take_along_axis(rows, x0[..., None], axis=2)
            p1 = np.take_along_axis(rows, x1[..., None], axis=2)
            if mut == "pad_slot":
                p1 = np.where(((x0 + 1) % 32 == 0)[..., None], p0, p1)
            outs.append(((w0 * p0).astype(F32) + (w1 * p1).astype(F32)).astype(F32))
        else:
            shq = np.trunc((shift.astype(np.float64) * 65536.0).astype(F32)).astype(np.int64)
            sfx = int(W if mut == "reflect_W" else W - 1) << 16
            s = (np.arange(W, dtype=np.int64)[None, None, :] << 16) + (shq if sg > 0 else -shq)
            s = np.abs(s)
            s = np.minimum(s, 2 * sfx - s)
            s = np.clip(s, 0, ((W - 1) << 16) - 1)
            x0, w1 = s >> 16, (s & 0xFFFF)[..., None]
            p0 = np.take_along_axis(rows, x0[..., None], axis=2).astype(np.int64)
            p1 = np.take_along_axis(rows, np.minimum(x0 + 1, W - 1)[..., None], axis=2).astype(np.int64)
            if mut == "pad_slot":
                p1 = np.where(((x0 + 1) % 32 == 0)[..., None], p0, p1)
            outs.append(p0 * (65535 - w1) + p1 * w1)               # the 16.16 sum of one sample
    pads = ((0, 0), (gm.pt, gm.Hp - H - gm.pt), (gm.pl, gm.Wp - W - gm.pl), (0, 0))
    cat = np.concatenate([np.pad(outs[0], pads), np.pad(outs[1], pads)], axis=1 if gm.tab else 2)
    if half:
        if gm.tab:
            a, b = cat[:, 0:2 * gm.oh:2], cat[:, 1:2 * gm.oh:2]
        elif mut == "hsbs_pair_shift":                              # pairs (2 x - 1, 2 x)
            sh = np.concatenate([cat[:, :, :1], cat[:, :, :-1]], axis=2)
            a, b = sh[:, :, 0:2 * gm.ow:2], sh[:, :, 1:2 * gm.ow:2]
        else:
            a, b = cat[:, :, 0:2 * gm.ow:2], cat[:, :, 1:2 * gm.ow:2]
    if kind == "fx":
        rnd = 0 if mut == "trunc_byte" else 32768
        v = ((a + b + 65536 - (65536 - 2 * rnd)) >> 1) if half else cat + rnd
        return np.clip(v >> 16, 0, 255).astype(np.uint8)
    v = ((a + b).astype(F32) * F32(0.5)).astype(F32) if half else cat
    v = np.clip(v, F32(0), F32(255))
    if not u8:
        return v
    return (np.floor(v) if mut == "trunc_byte" else np.rint(v)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ input families
def noise_u8(rng, B, H, W):
    return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def naming_u8(B, H, W):
    """R = x mod 256, G = y mod 256, B = 37 frame + a hash of (x, y): a wrong column, row, frame or channel is an error of many levels"""
    y, x = np.mgrid[0:H, 0:W]
    img = np.zeros((B, H, W, 3), np.uint8)
    img[..., 0] = x % 256
    img[..., 1] = (y * 3) % 256 if H > 85 else (y * 29) % 256
    for b in range(B):
        img[b, ..., 2] = (37 * b + ((x * 7 + y * 13) % 64)) % 256
    return img


def float_frames(rng, B, H, W):
    """float pixel values with some outside [0, 255]"""
    return (rng.random((B, H, W, 3)) * 300.0 - 20.0).astype(F32)


def depth_smooth(B, dh, dw, amp=1.0):
    y, x = np.mgrid[0:dh, 0:dw]
    return np.stack([(0.5 + 0.5 * np.sin(0.9 * x / max(dw, 1) * 6 + b) * np.cos(0.7 * y / max(dh, 1) * 5 + 0.3 * b)) * amp
                     for b in range(B)]).astype(F32)


def depth_frames(B, dh, dw, lo=0.1, hi=0.9, ramp=0.05):
    """a distinct constant per frame plus a small ramp down the rows: the wrong frame's or row's depth moves every pixel of the row"""
    c = lo + (hi - lo) * ((np.arange(B) * 0.6180339887) % 1.0)
    r = np.linspace(0, ramp, dh) if dh > 1 else np.zeros(1)
    return np.ascontiguousarray(np.broadcast_to(c[:, None, None] + r[None, :, None], (B, dh, dw))).astype(F32)


def depth_for_shift(shift_rows, W, *, ipd_uv=0.064, ratio=2.0, conv=0.0):
    """depth [B,H,W] (DIRECT: dh = H) whose row (b, y) has the constant pixel shift shift_rows[b][y]"""
    s = np.asarray(shift_rows, np.float64)
    K = float(F32(ratio)) * float(F32(ipd_uv * W)) * C05
    d = -s / K + float(F32(conv))
    return np.ascontiguousarray(np.broadcast_to(d[:, :, None], s.shape + (W,))).astype(F32)


def as_format(px_u8_or_f, fmt):
    """[B,H,W,3] -> the boundary layout: "U8_HWC" | "U8_CHW" | "F32_CHW" """
    if fmt == "U8_HWC":
        return np.ascontiguousarray(px_u8_or_f.astype(np.uint8))
    if fmt == "U8_CHW":
        return np.ascontiguousarray(px_u8_or_f.astype(np.uint8).transpose(0, 3, 1, 2))
    return np.ascontiguousarray(px_u8_or_f.astype(F32).transpose(0, 3, 1, 2))
