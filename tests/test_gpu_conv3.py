"""Every 3x3 convolution kernel behind launch_gemm (gemm.hip / conv3.hip) against a float64 convolution of the exact operands it
consumes, through d2s_conv3_probe: the engine's own dispatcher, operands cast and packed as the engine casts and packs them.

The reference (float64, on the device: F.unfold + matmul, one image at a time) is evaluated on the operands the kernel multiplies:
bf16-rounded input, weight and residual; for a folded up-sample, bf16(bilerp1(...)) computed in fp32 exactly as the loaders do
(ups_operand below).  Batched cases are checked on images {0, B/2, B-1}.  What "agrees" means, per output type:
  * bf16 output: the kernel's value is RNE(ref), or RNE of a value within delta of ref, delta = 2^-16 conv(|x|, |w|) (fp32
    accumulation of K = 9C terms in any order) + 2^-22 (|bias| + |res| + |ref|) (the fp32 adds of the epilogue); and at least 99 %
    of the outputs equal RNE(ref) bit for bit;
  * fp32 output and the fused head's depth: |got - ref| <= delta, delta carried through ReLU, the 1x1 w3 dot and the activation;
  * bf16x3 operands: within 2^-14 conv(|x|, |w|) (+ the epilogue term) of the float64 convolution of the UNROUNDED fp32 operands.
Weights ~ N(0, 1 / (9C)), inputs N(0, 1) and different in every image, bias and residual O(1): one wrong tap is ~0.02, a bf16 ulp
of an O(1) output ~0.004.  Every case runs twice (bit-identical) and names the kernel it expects: that pins the dispatch."""
import math
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f64_ref import bf16q, pow2, rne_bf16

GPU = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the up-sample operand
def linear_taps(n_out: int, n_in: int):
    """common.h linear_tap(dst, linear_scale(n_in, n_out, true), n_in, true) for dst = 0 .. n_out-1, in float32 like the kernels:
    the scale is a float32 division, src = scale * dst one float32 multiply, w1 = src - i0 one float32 subtract (no contraction)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    src = (np.float32(scale) * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    w0 = (np.float32(1.0) - w1).astype(np.float32)
    return i0, i1, w0, w1


def _fmaf(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf on float32 tensors: the float64 product (exact: 24 + 24 bits) plus the addend, rounded once to float32."""
    return (a.double() * b.double() + c.double()).float()


def ups_operand_f32(x: torch.Tensor, Hi: int, Wi: int) -> torch.Tensor:
    """bilerp1 (common.h) of the align_corners up-sample of x [B, Hs, Ws, C] (float32) to [B, Hi, Wi, C], in float32:
    top = fmaf(w1x, v01, w0x * v00), bot = fmaf(w1x, v11, w0x * v10), out = fmaf(w1y, bot, w0y * top)."""
    B, Hs, Ws, C = x.shape
    yi0, yi1, wy0, wy1 = (torch.from_numpy(t).to(x.device) for t in linear_taps(Hi, Hs))
    xi0, xi1, wx0, wx1 = (torch.from_numpy(t).to(x.device) for t in linear_taps(Wi, Ws))
    r0, r1 = x[:, yi0], x[:, yi1]
    v00, v01, v10, v11 = r0[:, :, xi0], r0[:, :, xi1], r1[:, :, xi0], r1[:, :, xi1]
    wx0, wx1 = wx0.view(1, 1, Wi, 1), wx1.view(1, 1, Wi, 1)
    wy0, wy1 = wy0.view(1, Hi, 1, 1), wy1.view(1, Hi, 1, 1)
    top = _fmaf(wx1.expand_as(v01), v01, wx0 * v00)
    bot = _fmaf(wx1.expand_as(v11), v11, wx0 * v10)
    return _fmaf(wy1.expand_as(bot), bot, wy0 * top)


def ups_operand(x: torch.Tensor, Hi: int, Wi: int) -> torch.Tensor:
    """The operand a folded up-sample feeds the MFMAs: bf16 (round to nearest even) of ups_operand_f32, as float32."""
    return ups_operand_f32(x, Hi, Wi).to(torch.bfloat16).float()


def test_ups_operand_matches_interpolate():
    """The fp32 bilerp1 emulation against torch's align_corners bilinear interpolation in float64 of the same bf16 source map:
    the two differ by fp32 rounding only -- three roundings of the lerps (2^-23 of the largest tap each) plus the float32 source
    coordinate (one rounding of scale and of scale * dst: up to 2^-23 (src + 1) in w1, times the largest tap difference)."""
    g = torch.Generator().manual_seed(5)
    for (Hs, Ws, Hi, Wi) in [(84, 148, 168, 296), (168, 296, 294, 518), (2, 10, 3, 19), (7, 13, 11, 21), (3, 512, 5, 1023), (11, 19, 21, 37)]:
        x = bf16q(torch.randn(2, Hs, Ws, 8, generator=g) * 2)
        got = ups_operand_f32(x, Hi, Wi).double()
        want = F.interpolate(x.double().permute(0, 3, 1, 2), size=(Hi, Wi), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        vmax = float(x.abs().max())
        bound = (3 * 2.0 ** -23 + 2.0 ** -23 * (max(Hs, Ws) + 1) * 2 * 2) * vmax
        err = float((got - want).abs().max())
        assert err <= bound, (Hs, Ws, Hi, Wi, err, bound)
        assert torch.equal(got[:, 0, 0], x[:, 0, 0].double())        # align_corners: output (0, 0) is source (0, 0) exactly


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    id: str
    C: int
    N: int
    B: int
    H: int                         # the map the convolution sees (Hi, Wi)
    W: int
    src: Optional[tuple] = None    # (Hs, Ws): an up-sample of the source map folded into the loader
    stride: int = 1
    relu_in: bool = False
    act: str = "none"
    bias: bool = True
    res: bool = False
    head: Optional[float] = None   # the fused head tail: max_depth (0: relative, ReLU; > 0: metric, sigmoid * max_depth)
    prec: str = "bf16"
    out_f32: bool = False
    splitk: int = 0                # split-K workspace elements (the engine's splitk_elems), 0: none
    env: Dict[str, str] = field(default_factory=dict)
    expect: str = ""               # kernel name, or "UNSUPPORTED" (conv3_upsample_ok refuses the fold)


def engine_cases(model: str, B: int, prec: str, frame=(1080, 1920, 518)):
    """Every 3x3 convolution of one forward pass of the engine (engine.hip neck_rest, forward, conv3()), as probe cases: the maps, the
    split-K workspace and the fused head tail are the frame's plan's (ops.forward_plan: the library's own plan_forward, host code)."""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS, engine_shape
    cfg = MODELS[model]
    h, w, _ = engine_shape(*frame)
    pl = ops.forward_plan(cfg, h, w, B, prec)
    gh, gw, fH, fW, ws, fused = pl["gh"], pl["gw"], pl["fH"], pl["fW"], pl["splitk_elems"], pl["head2_fused"]
    Fu, neck, Nh = cfg.fusion, cfg.neck, cfg.head_hidden
    tag = f"{model}-{frame[2]}-B{B}-{prec}"
    cs = [Case(f"{tag}-resize", neck[3], neck[3], B, gh, gw, stride=2, prec=prec, splitk=ws)]
    for i in range(4):
        cs.append(Case(f"{tag}-neck{i}", neck[i], Fu, B, fH[i], fW[i], bias=False, prec=prec, splitk=ws))
    for i in range(4):
        cs.append(Case(f"{tag}-rcu{i}-conv1", Fu, Fu, B, fH[i], fW[i], relu_in=True, prec=prec, splitk=ws))
        cs.append(Case(f"{tag}-rcu{i}-conv2", Fu, Fu, B, fH[i], fW[i], relu_in=True, res=True, prec=prec, splitk=ws))
    H1, W1 = 2 * fH[0], 2 * fW[0]
    if prec == "bf16":                                    # head conv1: the fusion stage's x2 up-sample folded where a kernel can
        cs.append(Case(f"{tag}-head1-ups", Fu, Fu // 2, B, H1, W1, src=(fH[0], fW[0]), prec=prec))
    cs.append(Case(f"{tag}-head1", Fu, Fu // 2, B, H1, W1, prec=prec, splitk=ws))     # the same conv on the up-sampled map
    for md in (0.0, 20.0):
        if not fused:
            break
        if prec == "bf16":
            cs.append(Case(f"{tag}-head2-ups-md{md:g}", Fu // 2, Nh, B, h, w, src=(H1, W1), head=md, bias=True, prec=prec))
        cs.append(Case(f"{tag}-head2-md{md:g}", Fu // 2, Nh, B, h, w, head=md, bias=True, prec=prec))
    cs.append(Case(f"{tag}-head2-relu", Fu // 2, Nh, B, h, w, act="relu", prec=prec, splitk=ws))
    return cs


def ragged_cases(ncu: int):
    """Small shapes that reach each kernel of the dispatcher at, just below and just above its thresholds (conv3.hip
    plan_conv3_halo2, gemm.hip plan_gemm): ragged maps, maps smaller than one tile, odd batches, persistent grids whose
    tile count is not a multiple of the grid, up-sample scales at and just above the limits.  The persistent head kernels'
    tile minimums are lowered so that they run at these sizes."""
    hp = {"D2S_HEADP_MIN": "8"}            # conv3_head*_kernel from 8 tiles of 16 x 16
    h1 = {"D2S_HEAD1P_MIN": "8"}           # conv3_c128_ups_kernel from 8 tiles of 8 x 16
    half, t384 = ncu // 2, 3 * ncu // 2    # the mid-size window (ncu/2, ncu] and the 384-tile floor (1.5 rounds of the CUs)
    W_t = lambda t: 16 * t - 3             # a 5-row map of t tiles of 8 x 16, the last one ragged
    cs = [
        # -- the fused head tail (MAP_HEAD, C = 64, N = 32): persistent kernels
        Case("head_ups-s0.5-B3", 64, 32, 3, 37, 45, src=(19, 23), head=0.0, env=hp, expect="conv3_head_ups_kernel"),
        Case("head_ups-s0.6-B5", 64, 32, 5, 11, 21, src=(7, 13), head=20.0, env=hp, expect="conv3_head_ups_kernel"),
        Case("head_ups-s0.61", 64, 32, 1, 101, 101, src=(62, 62), head=0.0, env=hp, expect="UNSUPPORTED"),
        Case("head_ups-Hs2-B9", 64, 32, 9, 3, 19, src=(2, 10), head=0.0, env=hp, expect="conv3_head_ups_kernel"),
        Case("head_ups-Ws512", 64, 32, 1, 5, 1023, src=(3, 512), head=0.0, env=hp, expect="conv3_head_ups_kernel"),
        Case("head1-Ws513", 64, 32, 1, 5, 1025, src=(3, 513), head=0.0, env=hp, expect="conv3_head_kernel<1>"),
        Case("head_ups-300tiles-B3", 64, 32, 3, 160, 153, src=(81, 77), head=20.0, env=hp, expect="conv3_head_ups_kernel"),
        Case("head_ups-v1", 64, 32, 2, 37, 45, src=(19, 23), head=0.0, env={**hp, "D2S_HEADUPS_V1": "1"}, expect="conv3_head_kernel<1>"),
        Case("head0-B2", 64, 32, 2, 40, 70, head=0.0, env=hp, expect="conv3_head_kernel<0>"),
        Case("head0-1xN", 64, 32, 1, 1, 300, head=20.0, env=hp, expect="conv3_head_kernel<0>"),
        Case("head0-2x2-B11", 64, 32, 11, 2, 2, head=0.0, env=hp, expect="conv3_head_kernel<0>"),
        Case("head0-5x300-B2", 64, 32, 2, 5, 300, head=0.0, env=hp, expect="conv3_head_kernel<0>"),
        Case("head0-300tiles-B3", 64, 32, 3, 160, 153, head=0.0, env=hp, expect="conv3_head_kernel<0>"),
        Case("head-below-min", 64, 32, 1, 40, 70, head=0.0, env={"D2S_HEADP_MIN": "16"}, expect="gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832"),
        # -- head conv1 at batch (C = 128 -> 64, folded up-sample with scale <= 0.5)
        Case("c128_ups-s0.5-B3", 128, 64, 3, 23, 39, src=(12, 20), env=h1, bias=True, expect="conv3_c128_ups_kernel"),
        Case("c128_ups-256tiles-B4", 128, 64, 4, 63, 127, src=(32, 64), env=h1, expect="conv3_c128_ups_kernel"),
        Case("c128_ups-s0.514-mid", 128, 64, 2, 71, 120, src=(37, 50), env=h1, expect="conv3_halo2_kernel<16,17,64,4,2,10,6>"),
        # -- conv3_wide: C = N = 128 from 384 tiles of 256 pixels; <8,32> when ceil(H/8) ceil(W/32) <= ceil(H/16) ceil(W/16)
        Case("wide16x16-at", 128, 128, t384 // 3, 16, 48, relu_in=True, res=True, act="relu", expect="conv3_wide_kernel<16,16>"),
        Case("wide-below", 128, 128, t384 // 3 - 1, 16, 48, relu_in=True, res=True, expect="conv3_halo2_kernel<16,17,128,2,4,2>"),
        Case("wide8x32", 128, 128, t384 // 55 + 1, 84, 148, relu_in=True, expect="conv3_wide_kernel<8,32>"),
        Case("wide8x32-ragged", 128, 128, 7, 83, 149, res=True, expect="conv3_wide_kernel<8,32>"),
        # -- the mid-size window: ncu/2 < tiles x N/64 <= ncu (C = 128)
        Case("mid-below", 128, 64, 1, 5, W_t(half), expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("mid-low", 128, 64, 1, 5, W_t(half + 1), relu_in=True, expect="conv3_halo2_kernel<16,17,64,4,2,10,6>"),
        Case("mid-high", 128, 64, 1, 5, W_t(ncu), res=True, expect="conv3_halo2_kernel<16,17,64,4,2,10,6>"),
        Case("mid-above", 128, 64, 1, 5, W_t(ncu + 1), expect="conv3_halo_kernel<bf16,64,4,2,4>"),     # (>= 200 tiles: first generation)
        # -- the one-shot halo2 blocks, C in {64, 128} x BN in {32, 64, 128}, from 384 tile-blocks
        Case("halo2-c64-n32", 64, 32, 1, 5, W_t(t384), act="relu", expect="conv3_halo2_kernel<8,10,32,4,1,3>"),
        Case("halo2-c64-n32-below", 64, 32, 1, 5, W_t(t384 - 1), act="relu", expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("halo2-c64-n64", 64, 64, 7, 37, 45 + 16 * 10, relu_in=True, res=True, expect="conv3_halo2_kernel<8,10,64,4,2,3>"),
        Case("halo2-c64-n128", 64, 128, 12, 50, 70, expect="conv3_halo2_kernel<8,10,128,2,4,3>"),
        Case("halo2-c128-n32-head", 128, 32, 7, 61, 97, head=20.0, expect="conv3_halo2_kernel<16,17,32,4,1,3>"),
        Case("halo2-c128-n64", 128, 64, 8, 47, 141, expect="conv3_halo2_kernel<16,17,64,4,2,3>"),
        Case("halo2-c128-n128", 128, 128, 7, 61, 97, act="relu", expect="conv3_halo2_kernel<16,17,128,2,4,2>"),
        Case("halo2-c64-n32-head-ups", 64, 32, 6, 77, 101, src=(60, 80), head=0.0, env={"D2S_HEADP_MIN": "100000"}, expect="conv3_halo2_kernel<8,10,32,4,1,3>"),
        # -- the first-generation halo kernel: 200 <= tiles < 384 (N <= 64), N = 96, and fp32 operands
        Case("halo1-c64-n64-at", 64, 64, 1, 5, W_t(200), relu_in=True, expect="conv3_halo_kernel<bf16,64,4,2,4>"),
        Case("halo1-c64-n64-below", 64, 64, 1, 5, W_t(199), expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("halo1-ups", 64, 64, 1, 8, W_t(200), src=(5, 1600), expect="conv3_halo_kernel<bf16,64,4,2,4>"),
        Case("halo1-n96", 64, 96, 4, 37, 149, res=True, expect="conv3_halo_kernel<bf16,128,2,4,2>"),
        Case("halo1-f32", 64, 64, 6, 41, 83, relu_in=True, res=True, prec="fp32", expect="conv3_halo_kernel<f32,64,4,2,4>"),
        # -- implicit GEMM: stride 2, wide channels, maps smaller than a tile, split-K
        Case("implicit-stride2", 96, 96, 3, 21, 37, stride=2, expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("implicit-1x1", 64, 64, 2, 1, 1, expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("implicit-c256-splitk", 256, 128, 1, 11, 19, splitk=16 * 11 * 19 * 256, expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=6"),
        Case("implicit-c1024-out_f32", 1024, 256, 1, 7, 12, out_f32=True, expect="gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264"),
        Case("bx3-ragged", 64, 64, 3, 13, 29, relu_in=True, res=True, prec="bf16x3", expect="gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264"),
        Case("bx3-head", 64, 32, 1, 37, 45, head=20.0, prec="bf16x3", expect="gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832"),
        Case("f32-head", 64, 32, 1, 37, 45, head=0.0, prec="fp32", expect="gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832"),
    ]
    return cs


# ------------------------------------------------------------------------------------------------ running one case
def _conv64(x: torch.Tensor, w: torch.Tensor, stride: int) -> torch.Tensor:
    """float64 3x3 convolution (pad 1) of x [H, W, C] with w [N, C, 3, 3]: F.unfold + matmul in row bands -> [Ho, Wo, N]."""
    H, W, C = x.shape
    N = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = F.pad(x.permute(2, 0, 1).unsqueeze(0), (1, 1, 1, 1))           # [1, C, H + 2, W + 2]
    wm = w.reshape(N, C * 9)
    out = torch.empty((Ho, Wo, N), dtype=torch.float64, device=x.device)
    band = max(1, (1 << 22) // max(1, Wo * C * 9))
    for y0 in range(0, Ho, band):
        y1 = min(Ho, y0 + band)
        rows = xp[:, :, y0 * stride:(y1 - 1) * stride + 3]
        cols = F.unfold(rows, 3, stride=stride)                          # [1, C * 9, (y1 - y0) * Wo], k = c * 9 + ky * 3 + kx
        out[y0:y1] = (wm @ cols[0]).t().reshape(y1 - y0, Wo, N)
    return out


def _images(B: int):
    return sorted({0, B // 2, B - 1})


class Stats:
    def __init__(self):
        self.n = 0
        self.exact = 0
        self.max_ulp = 0.0       # bf16 outputs with |ref| >= 1/4: |got - RNE(ref)| in bf16 ulps of ref
        self.max_rel = 0.0       # fp32 outputs / depth: max |got - ref| / delta

    def add(self, other: "Stats"):
        self.n += other.n; self.exact += other.exact
        self.max_ulp = max(self.max_ulp, other.max_ulp); self.max_rel = max(self.max_rel, other.max_rel)


def run_case(cs: Case, dev, seed: int):
    """Run one case through the probe twice, check it against float64; returns (kernel name, Stats)."""
    from desktop2stereo_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(seed)
    Hs, Ws = cs.src if cs.src else (cs.H, cs.W)
    Ho, Wo = (cs.H - 1) // cs.stride + 1, (cs.W - 1) // cs.stride + 1
    x = torch.randn((cs.B, Hs, Ws, cs.C), generator=g, device=dev)
    w = torch.randn((cs.N, cs.C, 3, 3), generator=g, device=dev) / math.sqrt(9 * cs.C)
    bias = torch.randn((cs.N,), generator=g, device=dev) * 0.5 if cs.bias else None
    res = torch.randn((cs.B, Ho, Wo, cs.N), generator=g, device=dev) if cs.res else None
    head = None
    if cs.head is not None:
        head = (torch.randn((cs.N,), generator=g, device=dev) / math.sqrt(cs.N), 0.1, cs.head)
    kw = dict(up=(cs.H, cs.W) if cs.src else None, stride=cs.stride, relu_in=cs.relu_in, act=cs.act, res=res,
              out_f32=cs.out_f32, head=head, splitk_elems=cs.splitk)
    old = {k: os.environ.get(k) for k in cs.env}
    try:
        os.environ.update(cs.env)
        ops.reload_env()
        if cs.expect == "UNSUPPORTED":
            with pytest.raises(_lib.D2SError, match="status 5"):
                ops.conv3_probe(x, w, bias, cs.prec, **kw)
            return "UNSUPPORTED", Stats()
        out, name = ops.conv3_probe(x, w, bias, cs.prec, **kw)
        out2, name2 = ops.conv3_probe(x, w, bias, cs.prec, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.reload_env()
    assert name == name2 and torch.equal(out, out2), (cs.id, "not bit-identical on a second run")
    st = Stats()
    bx3 = cs.prec == "bf16x3"
    for b in _images(cs.B):
        # the operands the kernel multiplies
        if cs.prec == "bf16":
            xb = ups_operand(bf16q(x[b:b + 1]), cs.H, cs.W)[0] if cs.src else bf16q(x[b])
            wq, rq = bf16q(w), (bf16q(res[b]) if res is not None and not cs.out_f32 else (res[b] if res is not None else None))
        else:                                  # fp32 / bf16x3: fp32 operands (bf16x3: the reference is the unrounded product)
            xb, wq, rq = x[b], w, (res[b] if res is not None else None)
        xb = xb.double()
        if cs.relu_in:
            xb = xb.clamp_min(0)
        ref = _conv64(xb, wq.double(), cs.stride)
        acc_abs = _conv64(xb.abs(), wq.double().abs(), cs.stride)
        delta = (2.0 ** -14 if bx3 else 2.0 ** -16) * acc_abs
        if bias is not None:
            ref = ref + bias.double()
            delta = delta + 2.0 ** -22 * bias.double().abs()
        if head is not None:
            w3 = head[0].double()
            hid = ref.clamp_min(0)
            s = hid @ w3 + head[1]
            ds = delta @ w3.abs() + 2.0 ** -22 * ((hid.abs() @ w3.abs()) + abs(head[1]))
            if cs.head > 0:
                want = torch.sigmoid(s) * cs.head
                dd = ds * cs.head / 4 + 2.0 ** -20 * cs.head
            else:
                want, dd = s.clamp_min(0), ds
            got = out[b].double()
            err = (got - want).abs()
            assert bool((err <= dd).all()), (cs.id, b, float(err.max()), float((err / dd).max()), name)
            st.n += err.numel(); st.exact += int((got == want.float().double()).sum())
            st.max_rel = max(st.max_rel, float((err / dd).max()))
            continue
        if cs.act == "relu":
            ref = ref.clamp_min(0)
        if rq is not None:
            ref = ref + rq.double()
            delta = delta + 2.0 ** -22 * rq.double().abs()
        delta = delta + 2.0 ** -22 * ref.abs()
        got = out[b].double()
        if out.dtype == torch.bfloat16:
            r = rne_bf16(ref)
            lo, hi = rne_bf16(ref - delta), rne_bf16(ref + delta)
            ok = (got >= lo) & (got <= hi)
            assert bool(ok.all()), (cs.id, b, "bf16 output outside RNE([ref - delta, ref + delta])", int((~ok).sum()),
                                    float((got - r).abs().max()), name)
            ulp = pow2(torch.frexp(r.abs().clamp_min(2.0 ** -100))[1] - 8)
            st.n += r.numel(); st.exact += int((got == r).sum())
            far = r.abs() >= 0.25                # (near 0 an ulp of ref is tiny and delta, an absolute bound, governs)
            if bool(far.any()):
                st.max_ulp = max(st.max_ulp, float(((got - r).abs() / ulp)[far].max()))
        else:
            err = (got - ref).abs()
            assert bool((err <= delta).all()), (cs.id, b, float(err.max()), float((err / delta).max()), name)
            st.n += err.numel(); st.exact += int((got == ref.float().double()).sum())      # correctly rounded fp32
            st.max_rel = max(st.max_rel, float((err / delta).max()))
    if out.dtype == torch.bfloat16:
        assert st.exact >= 0.99 * st.n, (cs.id, "fewer than 99 % of the outputs are RNE(ref)", st.exact / st.n, name)
    return name, st


# ------------------------------------------------------------------------------------------------ the tests
ENGINE_GROUPS = {
    "bf16-B1": [("tiny", 1, "bf16", (1080, 1920, 518)), ("vits", 1, "bf16", (1080, 1920, 518)), ("vitb", 1, "bf16", (1080, 1920, 518)),
                ("vitl", 1, "bf16", (1080, 1920, 518)), ("vitb", 1, "bf16", (720, 1280, 336))],
    "bf16-batched": [("tiny", 8, "bf16", (1080, 1920, 518)), ("vits", 8, "bf16", (1080, 1920, 518)), ("vitb", 8, "bf16", (1080, 1920, 518)),
                     ("vitl", 7, "bf16", (1080, 1920, 518))],
    "fp32": [("tiny", 1, "fp32", (1080, 1920, 518)), ("vits", 2, "fp32", (1080, 1920, 518)), ("vitb", 1, "fp32", (1080, 1920, 518)),
             ("vitl", 1, "fp32", (1080, 1920, 518))],
    "bf16x3": [("tiny", 1, "bf16x3", (1080, 1920, 518)), ("vits", 1, "bf16x3", (1080, 1920, 518)), ("vitb", 3, "bf16x3", (1080, 1920, 518)),
               ("vitl", 1, "bf16x3", (1080, 1920, 518))],
}

# the kernel every engine-derived case is expected to reach (default switches); UNSUPPORTED: conv3_upsample_ok refuses the fold,
# and the engine runs the stand-alone up-sample and the convolution case without "-ups"
EXPECTED_ENGINE = {
    "tiny-518-B1-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-neck0": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-head1-ups": "UNSUPPORTED",
    "tiny-518-B1-bf16-head1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-bf16-head2-ups-md0": "UNSUPPORTED",
    "tiny-518-B1-bf16-head2-md0": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-bf16-head2-ups-md20": "UNSUPPORTED",
    "tiny-518-B1-bf16-head2-md20": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-bf16-head2-relu": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vits-518-B1-bf16-neck0": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=4",
    "vits-518-B1-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vits-518-B1-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B1-bf16-head1-ups": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vits-518-B1-bf16-head1": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vits-518-B1-bf16-head2-ups-md0": "UNSUPPORTED",
    "vits-518-B1-bf16-head2-md0": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16-head2-ups-md20": "UNSUPPORTED",
    "vits-518-B1-bf16-head2-md20": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16-head2-relu": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B1-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B1-bf16-neck0": "gemm_glds_kernel<bf16,64,64,4,2,2,8,0> tile=64648",
    "vitb-518-B1-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vitb-518-B1-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B1-bf16-rcu0-conv1": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-518-B1-bf16-rcu0-conv2": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-518-B1-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-bf16-head1-ups": "conv3_halo2_kernel<16,17,64,4,2,3>",
    "vitb-518-B1-bf16-head1": "conv3_halo2_kernel<16,17,64,4,2,3>",
    "vitb-518-B1-bf16-head2-ups-md0": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-518-B1-bf16-head2-md0": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-518-B1-bf16-head2-ups-md20": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-518-B1-bf16-head2-md20": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-518-B1-bf16-head2-relu": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitl-518-B1-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-bf16-neck0": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitl-518-B1-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitl-518-B1-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitl-518-B1-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitl-518-B1-bf16-head1-ups": "UNSUPPORTED",
    "vitl-518-B1-bf16-head1": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-bf16-head2-ups-md0": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B1-bf16-head2-md0": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B1-bf16-head2-ups-md20": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B1-bf16-head2-md20": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B1-bf16-head2-relu": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitb-336-B1-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-336-B1-bf16-neck0": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=4",
    "vitb-336-B1-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vitb-336-B1-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-336-B1-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-336-B1-bf16-head1-ups": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-336-B1-bf16-head1": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-336-B1-bf16-head2-ups-md0": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-336-B1-bf16-head2-md0": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-336-B1-bf16-head2-ups-md20": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-336-B1-bf16-head2-md20": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitb-336-B1-bf16-head2-relu": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "tiny-518-B8-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-neck0": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B8-bf16-head1-ups": "UNSUPPORTED",
    "tiny-518-B8-bf16-head1": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-head2-ups-md0": "UNSUPPORTED",
    "tiny-518-B8-bf16-head2-md0": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-head2-ups-md20": "UNSUPPORTED",
    "tiny-518-B8-bf16-head2-md20": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B8-bf16-head2-relu": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B8-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-neck0": "gemm_glds_kernel<bf16,256,64,8,1,2,8,1> tile=9256648",
    "vits-518-B8-bf16-neck1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vits-518-B8-bf16-rcu0-conv1": "conv3_halo2_kernel<8,10,64,4,2,3>",
    "vits-518-B8-bf16-rcu0-conv2": "conv3_halo2_kernel<8,10,64,4,2,3>",
    "vits-518-B8-bf16-rcu1-conv1": "conv3_halo_kernel<bf16,64,4,2,4>",
    "vits-518-B8-bf16-rcu1-conv2": "conv3_halo_kernel<bf16,64,4,2,4>",
    "vits-518-B8-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B8-bf16-head1-ups": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vits-518-B8-bf16-head1": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vits-518-B8-bf16-head2-ups-md0": "UNSUPPORTED",
    "vits-518-B8-bf16-head2-md0": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B8-bf16-head2-ups-md20": "UNSUPPORTED",
    "vits-518-B8-bf16-head2-md20": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B8-bf16-head2-relu": "gemm_glds_kernel<bf16,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B8-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B8-bf16-neck0": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitb-518-B8-bf16-neck1": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitb-518-B8-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B8-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B8-bf16-rcu0-conv1": "conv3_wide_kernel<8,32>",
    "vitb-518-B8-bf16-rcu0-conv2": "conv3_wide_kernel<8,32>",
    "vitb-518-B8-bf16-rcu1-conv1": "conv3_halo_kernel<bf16,128,2,4,2>",
    "vitb-518-B8-bf16-rcu1-conv2": "conv3_halo_kernel<bf16,128,2,4,2>",
    "vitb-518-B8-bf16-rcu2-conv1": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-518-B8-bf16-rcu2-conv2": "conv3_halo2_kernel<16,17,64,4,2,10,6>",
    "vitb-518-B8-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B8-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B8-bf16-head1-ups": "conv3_c128_ups_kernel",
    "vitb-518-B8-bf16-head1": "conv3_halo2_kernel<16,17,64,4,2,3>",
    "vitb-518-B8-bf16-head2-ups-md0": "conv3_head_ups_kernel",
    "vitb-518-B8-bf16-head2-md0": "conv3_head_kernel<0>",
    "vitb-518-B8-bf16-head2-ups-md20": "conv3_head_ups_kernel",
    "vitb-518-B8-bf16-head2-md20": "conv3_head_kernel<0>",
    "vitb-518-B8-bf16-head2-relu": "conv3_halo2_kernel<8,10,32,4,1,3>",
    "vitl-518-B7-bf16-resize": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-neck0": "gemm_glds_kernel<bf16,128,128,2,4,2,8,0> tile=1281288",
    "vitl-518-B7-bf16-neck1": "gemm_glds_kernel<bf16,128,128,2,4,2,8,0> tile=1281288",
    "vitl-518-B7-bf16-neck2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-neck3": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-rcu0-conv1": "gemm_glds_kernel<bf16,128,128,2,4,2,8,0> tile=1281288",
    "vitl-518-B7-bf16-rcu0-conv2": "gemm_glds_kernel<bf16,128,128,2,4,2,8,0> tile=1281288",
    "vitl-518-B7-bf16-rcu1-conv1": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B7-bf16-rcu1-conv2": "gemm_glds_kernel<bf16,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B7-bf16-rcu2-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-rcu2-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-rcu3-conv1": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-rcu3-conv2": "gemm_glds_kernel<bf16,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B7-bf16-head1-ups": "UNSUPPORTED",
    "vitl-518-B7-bf16-head1": "gemm_glds_kernel<bf16,128,128,2,4,2,8,0> tile=1281288",
    "vitl-518-B7-bf16-head2-ups-md0": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B7-bf16-head2-md0": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B7-bf16-head2-ups-md20": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B7-bf16-head2-md20": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "vitl-518-B7-bf16-head2-relu": "conv3_halo2_kernel<16,17,32,4,1,3>",
    "tiny-518-B1-fp32-resize": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "tiny-518-B1-fp32-neck0": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-neck1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-neck2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-neck3": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "tiny-518-B1-fp32-rcu0-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu0-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu1-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu1-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu2-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu2-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu3-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-rcu3-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-head1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "tiny-518-B1-fp32-head2-md0": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-fp32-head2-md20": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-fp32-head2-relu": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B2-fp32-resize": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vits-518-B2-fp32-neck0": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-neck1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-neck2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=9",
    "vits-518-B2-fp32-neck3": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vits-518-B2-fp32-rcu0-conv1": "conv3_halo_kernel<f32,64,4,2,4>",
    "vits-518-B2-fp32-rcu0-conv2": "conv3_halo_kernel<f32,64,4,2,4>",
    "vits-518-B2-fp32-rcu1-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-rcu1-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-rcu2-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-rcu2-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-rcu3-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-rcu3-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vits-518-B2-fp32-head1": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B2-fp32-head2-md0": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B2-fp32-head2-md20": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B2-fp32-head2-relu": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B1-fp32-resize": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B1-fp32-neck0": "gemm_glds_kernel<f32,64,64,4,2,2,8,0> tile=64648",
    "vitb-518-B1-fp32-neck1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-fp32-neck2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B1-fp32-neck3": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitb-518-B1-fp32-rcu0-conv1": "gemm_glds_kernel<f32,64,64,4,2,2,8,0> tile=64648",
    "vitb-518-B1-fp32-rcu0-conv2": "gemm_glds_kernel<f32,64,64,4,2,2,8,0> tile=64648",
    "vitb-518-B1-fp32-rcu1-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-fp32-rcu1-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-fp32-rcu2-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitb-518-B1-fp32-rcu2-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitb-518-B1-fp32-rcu3-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitb-518-B1-fp32-rcu3-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=6",
    "vitb-518-B1-fp32-head1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitb-518-B1-fp32-head2-md0": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B1-fp32-head2-md20": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B1-fp32-head2-relu": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-fp32-resize": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-fp32-neck0": "gemm_glds_kernel<f32,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-fp32-neck1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-fp32-neck2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-fp32-neck3": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=16",
    "vitl-518-B1-fp32-rcu0-conv1": "gemm_glds_kernel<f32,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-fp32-rcu0-conv2": "gemm_glds_kernel<f32,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-fp32-rcu1-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-fp32-rcu1-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264",
    "vitl-518-B1-fp32-rcu2-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=12",
    "vitl-518-B1-fp32-rcu2-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=12",
    "vitl-518-B1-fp32-rcu3-conv1": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=12",
    "vitl-518-B1-fp32-rcu3-conv2": "gemm_glds_kernel<f32,32,64,2,2,4,8,0> tile=3264 splitk=12",
    "vitl-518-B1-fp32-head1": "gemm_glds_kernel<f32,64,128,2,4,2,8,0> tile=641288",
    "vitl-518-B1-fp32-head2-md0": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-fp32-head2-md20": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-fp32-head2-relu": "gemm_glds_kernel<f32,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-bf16x3-resize": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=6",
    "tiny-518-B1-bf16x3-neck0": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-neck1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-neck2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-neck3": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=6",
    "tiny-518-B1-bf16x3-rcu0-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu0-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu1-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu1-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu2-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu2-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu3-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-rcu3-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-head1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "tiny-518-B1-bf16x3-head2-md0": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-bf16x3-head2-md20": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "tiny-518-B1-bf16x3-head2-relu": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16x3-resize": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vits-518-B1-bf16x3-neck0": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-neck1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=4",
    "vits-518-B1-bf16x3-neck2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=9",
    "vits-518-B1-bf16x3-neck3": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vits-518-B1-bf16x3-rcu0-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu0-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu1-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu1-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu2-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu2-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu3-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-rcu3-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-head1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vits-518-B1-bf16x3-head2-md0": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16x3-head2-md20": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vits-518-B1-bf16x3-head2-relu": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B3-bf16x3-resize": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-neck0": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitb-518-B3-bf16x3-neck1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-neck2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-neck3": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vitb-518-B3-bf16x3-rcu0-conv1": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitb-518-B3-bf16x3-rcu0-conv2": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitb-518-B3-bf16x3-rcu1-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-rcu1-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-rcu2-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-rcu2-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitb-518-B3-bf16x3-rcu3-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=6",
    "vitb-518-B3-bf16x3-rcu3-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=6",
    "vitb-518-B3-bf16x3-head1": "gemm_glds_kernel<bx3,256,64,8,1,2,8,1> tile=9256648",
    "vitb-518-B3-bf16x3-head2-md0": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B3-bf16x3-head2-md20": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitb-518-B3-bf16x3-head2-relu": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-bf16x3-resize": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vitl-518-B1-bf16x3-neck0": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitl-518-B1-bf16x3-neck1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitl-518-B1-bf16x3-neck2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vitl-518-B1-bf16x3-neck3": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=16",
    "vitl-518-B1-bf16x3-rcu0-conv1": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitl-518-B1-bf16x3-rcu0-conv2": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitl-518-B1-bf16x3-rcu1-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitl-518-B1-bf16x3-rcu1-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264",
    "vitl-518-B1-bf16x3-rcu2-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=12",
    "vitl-518-B1-bf16x3-rcu2-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=12",
    "vitl-518-B1-bf16x3-rcu3-conv1": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=12",
    "vitl-518-B1-bf16x3-rcu3-conv2": "gemm_glds_kernel<bx3,32,64,2,2,2,8,1> tile=93264 splitk=12",
    "vitl-518-B1-bf16x3-head1": "gemm_glds_kernel<bx3,64,128,2,4,2,8,1> tile=964128",
    "vitl-518-B1-bf16x3-head2-md0": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-bf16x3-head2-md20": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
    "vitl-518-B1-bf16x3-head2-relu": "gemm_glds_kernel<bx3,128,32,4,1,2,8,1> tile=912832",
}

# every kernel of the dispatcher's table; the ragged cases reach each one
TABLE = ["conv3_head_ups_kernel", "conv3_head_kernel<1>", "conv3_head_kernel<0>", "conv3_c128_ups_kernel", "conv3_wide_kernel<8,32>",
         "conv3_wide_kernel<16,16>", "conv3_halo2_kernel<16,17,64,4,2,10,6>", "conv3_halo2_kernel<8,10,32,4,1,3>",
         "conv3_halo2_kernel<8,10,64,4,2,3>", "conv3_halo2_kernel<8,10,128,2,4,3>", "conv3_halo2_kernel<16,17,32,4,1,3>",
         "conv3_halo2_kernel<16,17,64,4,2,3>", "conv3_halo2_kernel<16,17,128,2,4,2>", "conv3_halo_kernel<bf16,", "conv3_halo_kernel<f32,",
         "gemm_glds_kernel<bf16,", "gemm_glds_kernel<f32,", "gemm_glds_kernel<bx3,", " splitk="]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _run_all(cases, dev, expected):
    per_kernel: Dict[str, Stats] = {}
    for i, cs in enumerate(cases):
        want = cs.expect = expected[cs.id]
        name, st = run_case(cs, dev, seed=1000 + i)
        print(f"[conv3] {cs.id:40s} {name:60s} n={st.n:9d} exact={st.exact / max(1, st.n):.4f} "
              f"max_ulp={st.max_ulp:.0f} max_err/delta={st.max_rel:.3f}")
        assert name == want, (cs.id, "dispatch moved", name, want)
        key = name.split(" splitk=")[0]
        per_kernel.setdefault(key, Stats()).add(st)
    for k, st in sorted(per_kernel.items()):
        print(f"[conv3 summary] {k:62s} outputs={st.n:10d} bit-exact={st.exact / max(1, st.n):.4f} "
              f"max_ulp={st.max_ulp:.0f} max_err/delta={st.max_rel:.3f}")
    return per_kernel


@GPU
@pytest.mark.parametrize("group", list(ENGINE_GROUPS))
def test_engine_convolutions_against_float64(dev, group):
    """Each 3x3 convolution launch of the tiny / ViT-S / ViT-B / ViT-L engines (maps from config.engine_shape and engine.hip's
    fH / fW), at batch 1 and batched, bf16 / fp32 / bf16x3 operands, against float64; each names its kernel."""
    cases = [c for (m, B, prec, frame) in ENGINE_GROUPS[group] for c in engine_cases(m, B, prec, frame)]
    _run_all(cases, dev, EXPECTED_ENGINE)


@GPU
def test_ragged_convolutions_against_float64(dev):
    """The ragged / threshold matrix (ragged_cases) against float64; together the cases reach every kernel of the table."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    cases = ragged_cases(ncu)
    seen = _run_all(cases, dev, {c.id: c.expect for c in cases})
    names = " | ".join(seen) + " | " + " | ".join(c.expect for c in cases)
    missing = [k for k in TABLE if k not in names]
    assert not missing, missing
