"""Float64 references, bounds, emulations and input families of the small model-side kernel tests (vit_ops.hip through d2s_vit_probe:
test_gpu_vit_ops.py on the device, test_cpu_vit_ref.py on the host).  numpy, with torch for F.interpolate and the bf16 conversion.
Inputs are the STORED values (bf16 kernels: float32 arrays that hold bf16-representable numbers), so a reference starts from the very
numbers the kernel reads.  u = 2^-24.  Every function takes mut=: one deliberate error, for test_cpu_vit_ref.py.

BOUNDS (from each kernel's arithmetic; nothing here was measured on the code under test).

 bilinear_nhwc_kernel.  Reference: F.interpolate(mode="bilinear", align_corners=True) in float64, plus the addend in float64.
     delta = 2^-23 T (3 + 4 (sy + 1) + 4 (sx + 1)) + 2^-24 |ref|
   T = the largest |tap| of the four taps the kernel reads (frame_ref.linear_tap), (sy, sx) = the output pixel's source coordinates:
   three fp32 lerp roundings of 2^-23 T at most; the fp32 source coordinate (scale and scale * dst one rounding each: up to
   2^-23 (s + 1) in a weight, which moves a lerp by that times a tap difference <= 2 T, and the vertical weight sees the horizontal
   lerps' differences, again <= 2 T -- the count of test_gpu_conv3.test_ups_operand_matches_interpolate); one fp32 add.  fp32 outputs:
   |got - ref| <= delta; bf16 outputs are ONE rounding of the fp32 sum: got inside [RNE(ref - delta), RNE(ref + delta)].  In bf16 the
   kernel also equals rne_bf16(fl32(ups_operand_f32(x) + addend)) bit for bit, the model test_gpu_conv3.py uses for the folded loaders.
 head_final_kernel.  s = sum_c x_c w3_c + b3 in float64; ds = (C + 2) u (sum |x_c w3_c| + |b3|), the sequential fp32 summation bound
   (fused or not).  Relative (max_depth 0): max(s, 0), delta ds.  Metric: sigmoid(s) max_depth, delta ds max_depth / 4 + 2^-20 max_depth
   (the sigmoid's slope is at most 1/4; expf, the reciprocal and the product stay inside 2^-20 of the range): the bound
   test_gpu_conv3.py holds the fused tail to.
 patchify_kernel, amax_kernel, to_f32_kernel: exact, compared as bits."""
import numpy as np
import torch
import torch.nn.functional as F

from frame_ref import judge_bf16, judge_float, linear_tap, patch_rows, rne_bf16      # noqa: F401  (the judges are used through this module)

F32 = np.float32
U = 2.0 ** -24


def to_bf16_bits(a):
    """float32 array -> its RNE bf16 bits (uint16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bf16_bits_value(b):
    return (b.astype(np.uint32) << 16).view(F32)


def bf16q(a):
    """float32 array -> the float32 value of its RNE bf16"""
    return bf16_bits_value(to_bf16_bits(a))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and bool((a.view(np.uint8) == b.view(np.uint8)).all())


# ------------------------------------------------------------------------------------------------ up-sample
def upsample_inputs(rng, B, Hi, Wi, Ho, Wo, C, bf16):
    """-> x [B,Hi,Wi,C], addend [B,Ho,Wo,C]: stored values as float32"""
    x = (rng.standard_normal((B, Hi, Wi, C)) * 2).astype(F32)
    a = rng.standard_normal((B, Ho, Wo, C)).astype(F32)
    return (bf16q(x), bf16q(a)) if bf16 else (x, a)


def upsample_ref(x, Ho, Wo, addend=None):
    """-> (ref, delta), float64 [B,Ho,Wo,C]"""
    B, Hi, Wi, C = x.shape
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    ref = F.interpolate(t, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy().copy()
    if addend is not None:
        ref = ref + addend.astype(np.float64)
    y0, y1, _, _ = linear_tap(Ho, Hi, align_corners=True)
    x0, x1, _, _ = linear_tap(Wo, Wi, align_corners=True)
    ax = np.abs(x.astype(np.float64))
    r0, r1 = ax[:, y0], ax[:, y1]
    T = np.maximum(np.maximum(r0[:, :, x0], r0[:, :, x1]), np.maximum(r1[:, :, x0], r1[:, :, x1]))
    sy = np.arange(Ho) * ((Hi - 1) / (Ho - 1) if Ho > 1 else 0.0)
    sx = np.arange(Wo) * ((Wi - 1) / (Wo - 1) if Wo > 1 else 0.0)
    k = 3 + 4 * (sy[None, :, None, None] + 1) + 4 * (sx[None, None, :, None] + 1)
    return ref, 2.0 ** -23 * T * k + U * np.abs(ref)


def _fmaf(a, b, c):
    """fmaf on float32 arrays: the float64 product (exact) plus the addend, rounded once to float32 (as test_gpu_conv3._fmaf)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def upsample_emulate(x, Ho, Wo, addend=None, *, bf16=False, mut=None):
    """bilinear_nhwc_kernel in float32: linear_tap, bilerp1's three fused multiply-adds, one add, one rounding to the storage type.
    -> float32 [B,Ho,Wo,C] (bf16: the stored value)"""
    B, Hi, Wi, C = x.shape
    ac = mut != "align_corners_false"
    y0, y1, wy0, wy1 = linear_tap(Ho, Hi, align_corners=ac)
    x0, x1, wx0, wx1 = linear_tap(Wo, Wi, align_corners=ac)
    x = x.astype(F32)
    r0, r1 = x[:, y0], x[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    if mut == "swap_xy":
        v01, v10 = v10, v01
    wx0, wx1 = wx0[None, None, :, None], wx1[None, None, :, None]
    wy0, wy1 = wy0[None, :, None, None], wy1[None, :, None, None]
    top = _fmaf(np.broadcast_to(wx1, v01.shape), v01, (wx0 * v00).astype(F32))
    bot = _fmaf(np.broadcast_to(wx1, v11.shape), v11, (wx0 * v10).astype(F32))
    v = _fmaf(np.broadcast_to(wy1, bot.shape), bot, (wy0 * top).astype(F32))
    if bf16 and mut == "round_before_add":
        v = bf16q(v)
    if addend is not None and mut != "no_addend":
        v = (v + addend.astype(F32)).astype(F32)
    if not bf16:
        return v
    if mut == "trunc":
        return (v.view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    return bf16q(v)


def upsample_judge(got, ref, delta, bf16):
    """got: the stored values as float -> (ok, worst err / delta)"""
    return judge_bf16(got, ref, delta) if bf16 else judge_float(got, ref, delta)


# ------------------------------------------------------------------------------------------------ head tail
def head_inputs(rng, npix, C, bf16):
    """x >= 0 [npix, C] (as the engine's ReLU leaves it), w3 [C] of zero mean, b3: s of both signs; from pixel npix // 2 on, up to 32 pixels with
    |s| near 40 (alternating sign): x = a max(+-w3, 0), a = 40 / sum max(+-w3, 0) |w3|"""
    x = np.abs(rng.standard_normal((npix, C))).astype(F32)
    w3 = rng.standard_normal(C)
    w3 = (w3 - w3.mean()).astype(F32)                               # (zero mean: E s = b3 whatever the mean of x, so both signs occur)
    b3 = F32(0.37)
    for k, i in enumerate(range(npix // 2, min(npix // 2 + 32, npix))):
        sg = 1.0 if k % 2 == 0 else -1.0
        pos = np.maximum(sg * w3.astype(np.float64), 0.0)
        x[i] = (pos * (40.0 / float((pos * np.abs(w3)).sum()))).astype(F32)
    return (bf16q(x) if bf16 else x), w3, b3


def head_ref(x, w3, b3, max_depth, *, dt=np.float64, mut=None):
    """float64: -> (ref, delta, s).  float32 (the emulation): the kernel's sequential sum, products and sums rounded separately -> out"""
    n, C = x.shape
    Cs = C - 1 if mut == "short" else C
    bias = dt(0) if mut == "no_bias" else dt(b3)
    if dt == np.float64:
        prod = x.astype(np.float64) * w3.astype(np.float64)[None, :]
        s = prod.sum(axis=1) + float(b3)
        ds = (C + 2) * U * (np.abs(prod).sum(axis=1) + abs(float(b3)))
        if max_depth > 0:
            return float(max_depth) / (1.0 + np.exp(-s)), ds * float(max_depth) / 4 + 2.0 ** -20 * float(max_depth), s
        return np.maximum(s, 0.0), ds, s
    acc = np.zeros(n, F32)
    for c in range(Cs):
        acc = (acc + (x[:, c].astype(F32) * F32(w3[c])).astype(F32)).astype(F32)
    v = (acc + bias).astype(F32)
    if max_depth > 0 and mut != "relu_metric":
        e = np.exp(-v.astype(np.float64)).astype(F32)
        sg = (F32(1) / (F32(1) + e).astype(F32)).astype(F32)
        return sg if mut == "no_max_depth" else (sg * F32(max_depth)).astype(F32)
    return np.maximum(v, F32(0))


# ------------------------------------------------------------------------------------------------ patchify
def naming_planes(rng, B, h, w):
    """x[b][c][y][x] = an integer in [-63, 63] that names (b, c, y, x) plus a fraction in [0, 0.5): a permuted index is an error of many
    units, and the fraction makes the bf16 rounding count"""
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(3), np.arange(h), np.arange(w), indexing="ij")
    v = ((7 * x + 13 * y + 31 * c + 57 * b) % 127 - 63).astype(np.float64) + rng.random((B, 3, h, w)) * 0.5
    return v.astype(F32)


def patchify_expected(x, p, Kp, bf16):
    """-> A [B gh gw, Kp]: float32, or bf16 bits (uint16); the columns >= 3 p^2 are zero bits"""
    A = patch_rows(x.astype(np.float64), p, Kp)
    A = np.where(np.isnan(A), 0.0, A).astype(F32)
    return to_bf16_bits(A) if bf16 else A


def cls_rows_expected(resid0, cls, pos, D):
    """resid0 [B,N,D] before the call -> after: row 0 of every frame = cls + pos[0:D], one float32 add"""
    out = resid0.copy()
    if cls is not None:
        out[:, 0, :] = (cls.astype(F32) + pos[:D].astype(F32)).astype(F32)[None, :]
    return out


def patchify_emulate(x, p, Kp, bf16, A0, resid0=None, cls=None, pos=None, *, mut=None):
    """the kernel's own index decode, thread by thread: flat idx -> (row, k) -> (b, py, px), (c, i, j).  A0 / resid0: the buffers before
    the call (what an unwritten element keeps).  -> (A, resid)"""
    B, _, h, w = x.shape
    gh, gw = h // p, w // p
    P = gh * gw
    idx = np.arange(B * P * Kp)
    k, row = idx % Kp, idx // Kp
    b, pi = row // P, row % P
    py, px = pi // gw, pi % gw
    live = k < 3 * p * p
    kk = np.where(live, k, 0)
    if mut == "perm_cij":
        i, j, c = kk // (3 * p), (kk % (3 * p)) // 3, kk % 3
    else:
        c, i, j = kk // (p * p), (kk % (p * p)) // p, kk % p
    v = np.where(live, x[b, c, py * p + i, px * p + j], F32(0)).astype(F32)
    A = (to_bf16_bits(v) if bf16 else v).reshape(B * P, Kp)
    if mut == "pad_unwritten":
        A = np.where(live.reshape(B * P, Kp), A, A0)
    resid = None if resid0 is None else resid0.copy()
    if cls is not None:
        D = cls.shape[0]
        row0 = (cls.astype(F32) + (pos[D:2 * D] if mut == "pos_row1" else pos[:D]).astype(F32)).astype(F32)
        resid[:1 if mut == "cls_frame0_only" else B, 0, :] = row0[None, :]
    return A, resid


# ------------------------------------------------------------------------------------------------ amax
def amax_blocks(n):
    """launch_amax's grid: n / 2048 blocks of 256 threads, at least 1, at most 1024"""
    return min(max(n // 2048, 1), 1024)


def amax_positions(n):
    """where the one large element is planted: first, last, n / 2, the last element of the first full grid sweep (where n reaches it)"""
    sweep = amax_blocks(n) * 256
    return sorted({0, n - 1, n // 2} | ({sweep - 1} if sweep <= n else set()))


def amax_background(rng, n, bf16):
    """|x| <= 1"""
    x = (rng.random(n) * 2 - 1).astype(F32)
    return bf16q(x) if bf16 else x


def amax_inputs(rng, n, pos, negative, bf16):
    """the background with one element of magnitude 3 planted at pos"""
    x = amax_background(rng, n, bf16)
    x[pos] = F32(-3.0 if negative else 3.0)
    return x


def amax_expected(x, slot_before, *, mut=None):
    """max(slot_before, max |x|) as a float32 (inputs finite)"""
    n = x.shape[0]
    v = x.astype(F32)
    if mut == "skip_tail":
        sweep = amax_blocks(n) * 256
        v = v[:max(n // sweep * sweep, min(n, 1))]
    m = F32(max(float(v.max()), 0.0)) if mut == "no_abs" else F32(np.abs(v).max())
    return m if mut == "overwrite" else max(F32(slot_before), m)


# ------------------------------------------------------------------------------------------------ to_f32
def to_f32_inputs(rng, n, bf16):
    """bf16: bits that cover +-0, the largest finite value, the smallest normal, subnormals and several exponents (uint16);
    fp32: random finite bit patterns plus the same specials (float32)"""
    if bf16:
        sp = np.array([0x0000, 0x8000, 0x7f7f, 0xff7f, 0x0080, 0x8080, 0x0001, 0x007f, 0x3f80, 0xbf80, 0x4049, 0x0780, 0x7700, 0x1234, 0xc2f7],
                      np.uint16)
        r = rng.integers(0, 0x7f80, n, dtype=np.uint16) | (rng.integers(0, 2, n, dtype=np.uint16) << 15)
        r[:min(n, sp.size)] = sp[:min(n, sp.size)]
        return r.astype(np.uint16)
    sp = np.array([0x00000000, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x00800000, 0x00000001, 0x3f800000, 0x40490fdb], np.uint32)
    r = rng.integers(0, 0x7f800000, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31)
    r[:min(n, sp.size)] = sp[:min(n, sp.size)]
    return r.view(F32)


def to_f32_expected(x, bf16):
    return bf16_bits_value(x) if bf16 else x.copy()
