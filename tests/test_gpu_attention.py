"""Every attention kernel behind launch_attention (attention.hip) against a float64 softmax(q k^T / 8) v of the exact operands it
multiplies, through d2s_attention_probe_ex: the engine's own dispatcher, operands packed as the engine's QKV linear leaves them, the
output raw in the kernel's own type (bf16, fp32, bf16x3 unit words, e4m3 bytes) between two guard rows.

The dispatcher (pairs = B heads, q128 = ceil(N / 128) pairs, k64 = ceil(N / 64) pairs), and every name it can emit (TABLE):
  bf16, q128 >= 168, D2S_ATTN32 != 0      attention32_kernel<out=bf16 | fp8>
  otherwise q128 >= 512                    attention_kernel<bf16 | bx3, NW=8, ...>                   (128 query rows per block)
  otherwise k64 < 256 and N >= 256         the key-split forms: bf16 KS=2 (N < 512) / KS=4 (N >= 512); e4m3 output KS=4; bx3 KS=2
  otherwise                                attention_kernel<bf16 | bx3, NW=4, ...>
  fp32                                     attention_kernel<f32,NW=4,NS=3,out=f32> always

The reference (float64, on the device, images {0, B/2, B-1} of a batch): w = softmax over keys, ref = w v, A = w |v|, of
  * bf16:           q~ = bf16(q c) with c = 64^-0.5 log2 e (the engine folds c into W_q: one rounding), bf16(k), bf16(v);
  * fp32, bf16x3:   the unrounded fp32 operands.
Agreement is per element, |got - ref| against delta = (rP + rS T_i + rF) A, where (u = 2^-24, the fp32 unit roundoff)
  * rP  = 2^-8 (bf16 operands): P rounded to bf16 in the numerator, 2^-9 A, plus the denominator, 2^-9 |ref| <= 2^-9 A (the 32 x 32
          kernel sums the rounded P -- then both are one perturbed softmax --, the 16-row kernel the unrounded P);
          2^-16 (bf16x3): P, V and the output each split into two bf16, 2^-18 each, and the dropped lo x lo products, 2^-18;
          0 (fp32);
  * rS T_i: the score error carried through exp2.  T_i = max_j sum_d |q~_id k_jd| (log2 units).  A score is 64 fp32 products summed
          in any order, minus the running maximum (the C operand of the first MFMA, or one subtraction), times the fp32 scale constant
          (fp32 / bf16x3 only), into one FMA: at most 72 u T_i.  bf16x3 adds the operand splits and the dropped lo x lo products,
          3 x 2^-18 T_i = 192 u T_i.  An error e in every score moves numerator and denominator by a factor 2^e each, to first order
          2 ln 2 e < 1.5 e of A:  rS = 1.5 x 72 u (bf16, fp32), 1.5 x 264 u (bf16x3);
  * rF  = (2 N + 2 ceil(N / 64) + 16) u + 2^-22: numerator and denominator are sums of N fp32 terms in any order (N u each), rescaled
          once per key tile (one rounding each), v_exp_f32 is good to one ulp in each (2 x 2^-23), and the merge of the key groups,
          1 / l, the output scale and the product add a dozen roundings.
  bf16 output: got in [RNE_bf16(ref - delta), RNE_bf16(ref + delta)];  e4m3 output: the same with RNE_e4m3((ref -+ delta) oscale) (which
  saturates at +-448: an element beyond 448 by more than delta oscale must be exactly +-448), and no byte 0x7f / 0xff;  fp32 and
  bf16x3 output: |got - ref| <= delta, and on the diffuse and the peaked family also the gate of test_attention_probe,
  max |got - ref| <= 2e-5 (fp32) / 2e-4 (bf16x3) x max(1, max |ref| / 4), so the bound is nowhere looser than that test's.
Nothing is NaN or inf, both guard rows keep their 0x7f bytes, a second run is bit-identical, and the kernel name is the expected one.

Input families (seeded, different in every (batch, head)):
  F1 diffuse: randn q / k / v, V asymmetric (channel 0 + 0.5 (j mod 5), channel 63 - 1): accumulation and normalisation.
  F2 peaked permutation: k rows of norm 8, pi(i) = (a i + 7) mod N with a >= N / 3 coprime with N, q_i = 1.5 k_pi(i) + 0.25 randn,
     v[j, j mod 64] += 4.  Asserted on the reference before the kernel is judged: query i gives key pi(i) a weight >= 0.9 (pi is a
     bijection, so every key is the arg-max of exactly one query).  A dropped, duplicated, permuted or wrongly masked key moves an
     output by |v| ~ 4, a thousand delta.
  F3 far below zero: F2 with channel 63 of every key 32 and of every query -32: every score moves by -128 (-184.7 log2 units), the
     softmax is unchanged.  The first key tile's maximum lies far below the initial running maximum, and an unmasked phantom key
     of the ragged last tile (score 0) would take all the weight.
  F4 late rises: F1 with, in one 32-row query group, (b) a key in the second-to-last tile 3..6 log2 units above query 11's running
     maximum while no other row of the group rises by more than 8 there (the 32 x 32 kernel keeps P up to 256 and does not rescale),
     (c) a key in the last tile 10..20 above query 20's (unless that tile has one key), (a) the last key ~100 above query 3's;
     and two queries of the next group whose score grows by ~0.5 per key, so the maximum rises in every tile.  (b), (c), (a) and
     the slope are asserted on the reference.  (N <= 128: the last key ~100 above query 0's maximum only.)

Measured worst err / delta per kernel: DESIGN.md (float64 references, attention)."""
import math
import os
from dataclasses import dataclass, field
from typing import Dict

import pytest
import torch

from f64_ref import bx3_value, e4m3_value, pow2, rne_bf16, rne_e4m3

GPU = pytest.mark.gpu

C32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32)) * 0.125      # vit_ops.h ATTN_SCALE_LOG2E, the float the kernels hold
C64 = 0.125 * 1.4426950408889634
U = 2.0 ** -24

K32 = "attention32_kernel<out=bf16>"
K32F = "attention32_kernel<out=fp8>"
B4 = "attention_kernel<bf16,NW=4,NS=3,out=bf16>"
B8 = "attention_kernel<bf16,NW=8,NS=3,out=bf16>"
BK2 = "attention_kernel<bf16,NW=4,NS=3,out=bf16,KS=2>"
BK4 = "attention_kernel<bf16,NW=4,NS=2,out=bf16,KS=4>"
E4 = "attention_kernel<bf16,NW=4,NS=3,out=fp8>"
E8 = "attention_kernel<bf16,NW=8,NS=3,out=fp8>"
EK4 = "attention_kernel<bf16,NW=4,NS=2,out=fp8,KS=4>"
X4 = "attention_kernel<bx3,NW=4,NS=2,out=bx3>"
X8 = "attention_kernel<bx3,NW=8,NS=2,out=bx3>"
XK2 = "attention_kernel<bx3,NW=4,NS=2,out=bx3,KS=2>"
F32 = "attention_kernel<f32,NW=4,NS=3,out=f32>"
# every kernel name launch_attention can emit (the dispatcher's table above)
TABLE = [K32, K32F, B4, B8, BK2, BK4, E4, E8, EK4, X4, X8, XK2, F32]

NO32 = {"D2S_ATTN32": "0"}


@dataclass
class Case:
    id: str
    B: int
    heads: int
    N: int
    prec: str = "bf16"             # operands: bf16 | fp32 | bf16x3
    e4m3: bool = False             # bf16 operands, e4m3 output (oscale: ~1 % of the outputs saturate)
    fam: str = "2"                 # input families to run, of "1234"
    env: Dict[str, str] = field(default_factory=dict)
    expect: str = ""


N_EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 192, 193]


def cases():
    cs = []

    def add(tag, B, H, N, expect, **kw):
        cs.append(Case(f"{tag}-B{B}h{H}N{N}", B, H, N, expect=expect, **kw))
    # -- engine shapes, bf16 and e4m3 output (F1 on all; F3 / F4 on (1,12,778), (2,12,778) and one shape of every kernel name)
    for (B, H, N, kb, ke, fam) in [(1, 2, 19, B4, E4, "1234"), (1, 6, 337, BK2, EK4, "1234"), (1, 6, 778, BK4, EK4, "12"),
                                   (1, 12, 778, BK4, EK4, "1234"), (1, 16, 778, BK4, EK4, "12"), (1, 16, 1370, K32, K32F, "12"),
                                   (2, 6, 778, BK4, EK4, "12"), (3, 6, 778, BK4, EK4, "12"), (2, 12, 778, K32, K32F, "1234"),
                                   (4, 6, 778, K32, K32F, "12")]:
        add("engine", B, H, N, kb, fam=fam)
        add("engine-e4m3", B, H, N, ke, e4m3=True, fam=fam)
    for (B, H, N, kb, ke) in [(1, 16, 1370, B4, E4), (8, 12, 778, B8, E8), (4, 12, 778, B4, E4)]:
        add("engine-no32", B, H, N, kb, env=NO32, fam="1234" if kb == B8 else "12")
        add("engine-no32-e4m3", B, H, N, ke, e4m3=True, env=NO32, fam="1234" if ke == E8 else "12")
    # -- e4m3 output, 256 <= N < 512: the KS=4 kernel on 4 .. 8 key tiles
    for N in (256, 257):
        add("e4m3-ks4", 1, 6, N, EK4, e4m3=True)
    # -- thresholds at small N, one case either side
    add("thr-attn32-at", 7, 12, 130, K32)                                   # 168 blocks of 128 rows
    add("thr-attn32-below", 1, 83, 130, B4)                                 # 166
    add("thr-nw8-at", 16, 16, 130, B8, env=NO32)                            # 512
    add("thr-nw8-below", 15, 17, 130, B4, env=NO32)                         # 510
    add("thr-nw8-at", 16, 16, 130, X8, prec="bf16x3", fam="1234")
    add("thr-nw8-below", 15, 17, 130, X4, prec="bf16x3", fam="1234")
    for (N, kb) in [(255, B4), (256, BK2), (511, BK2), (512, BK4)]:
        add("thr-ks-N", 1, 2, N, kb)
    add("thr-ks-blocks-below", 7, 9, 256, BK2)                              # 63 pairs x 4 key tiles = 252 blocks of 64 rows
    add("thr-ks-blocks-at", 8, 8, 256, B4)                                  # 256
    add("thr-ks-blocks-below", 1, 31, 512, BK4)                             # 248
    add("thr-ks-blocks-at", 2, 16, 512, B4)                                 # 256
    # -- grid mapping (attn_block): plain order below 16 pairs, XCD ranges from 16, pairs not a multiple of 8
    for (B, H) in [(3, 5), (2, 8), (1, 17), (1, 23)]:
        add("grid", B, H, 130, B4, env=NO32)
        add("grid", B, H, 1430, K32)                                        # 12 q tiles: 180 .. 276 blocks
    # -- the edges of N at 168 pairs: the 16-row kernel, the 32 x 32 kernel, bf16x3, fp32
    for N in N_EDGES:
        add("edge", 14, 12, N, K32, fam="234")
        add("edge-no32", 14, 12, N, B4, env=NO32)
        add("edge", 14, 12, N, X4, prec="bf16x3")
        add("edge", 14, 12, N, F32, prec="fp32")
    # -- uneven key groups: 5, 9, 13 key tiles over 2 / 4 groups, the ragged tile in the last group; 13 x 64: no ragged tile
    add("groups", 1, 2, 300, BK2, fam="24")
    for N in (550, 800, 832):
        add("groups", 1, 2, N, BK4, fam="24")
    for N in (300, 550, 832):
        add("groups-e4m3", 1, 2, N, EK4, e4m3=True)
        add("groups", 1, 2, N, XK2, prec="bf16x3", fam="234" if N == 300 else "2")
    # -- fp32
    for (B, H, N, fam) in [(1, 12, 778, "1234"), (64, 2, 296, "12"), (90, 6, 37, "12")]:
        add("fp32", B, H, N, F32, prec="fp32", fam=fam)
    assert len({c.id + c.prec for c in cs}) == len(cs)
    return cs


CASES = cases()


def test_every_kernel_name_is_expected_by_a_case():
    """Every name launch_attention can emit is the expect of some case; F3 and F4 run on at least one shape of every name."""
    assert {c.expect for c in CASES} == set(TABLE)
    assert {c.expect for c in CASES if "3" in c.fam and "4" in c.fam} == set(TABLE)


# ------------------------------------------------------------------------------------------------ inputs
def _randn(shape, g, dev):
    return torch.randn(shape, generator=g, device=dev)


def _asym_v(B, H, N, g, dev):
    v = _randn((B, H, N, 64), g, dev)
    v[..., 0] += (torch.arange(N, device=dev) % 5 * 0.5)[None, None, :]
    v[..., 63] -= 1.0
    return v


def perm(N: int) -> torch.Tensor:
    a = max(1, -(-N // 3))
    while math.gcd(a, N) != 1:
        a += 1
    return (a * torch.arange(N) + 7) % N


def family(fam: str, B: int, H: int, N: int, g, dev, c: float):
    """-> q, k, v float32 [B, H, N, 64], info (what the family asserts on the reference).  c: the scale of the scores in log2 units."""
    if fam == "1":
        return _randn((B, H, N, 64), g, dev), _randn((B, H, N, 64), g, dev), _asym_v(B, H, N, g, dev), {}
    if fam in "23":
        k = _randn((B, H, N, 64), g, dev)
        if fam == "3":
            k[..., 63] = 0.0
        k = k * (8.0 / k.norm(dim=-1, keepdim=True))
        pi = perm(N).to(dev)
        q = 1.5 * k[:, :, pi] + 0.25 * _randn((B, H, N, 64), g, dev)
        v = _asym_v(B, H, N, g, dev)
        j = torch.arange(N, device=dev)
        v[:, :, j, j % 64] += 4.0
        if fam == "3":
            k[..., 63] = 32.0
            q[..., 63] = -32.0
        return q, k, v, {"pi": pi}
    # F4
    q, k, v = _randn((B, H, N, 64), g, dev), _randn((B, H, N, 64), g, dev), _asym_v(B, H, N, g, dev)
    nt = -(-N // 64)
    info = {}

    def plant(i, j, first_key, rise):
        """move key j, along q_i, so that query i scores it `rise` log2 units above its maximum over keys [0, first_key)"""
        s = c * torch.einsum("bhd,bhnd->bhn", q[:, :, i].double(), k.double())
        top = s[..., :first_key].max(dim=-1).values if first_key > 0 else s.max(dim=-1).values
        qi = q[:, :, i].double()
        qi[..., 62] = 0.0                          # (channel 62 carries the ramp)
        k[:, :, j] += (((top + rise - s[..., j]) / c)[..., None] * qi / (qi * qi).sum(-1, keepdim=True)).float()
    if nt >= 3:
        ramp = [r for r in (37, 38) if r < N]
        k[..., 62] = (0.5 / (c * 512.0)) * torch.arange(N, device=dev, dtype=torch.float32)[None, None, :]
        for r in ramp:
            q[:, :, r] = 0.0
            q[:, :, r, 62] = 512.0
        jb = 64 * (nt - 2) + 17
        jc = 64 * (nt - 1)
        plant(11, 5, 64 * (nt - 2), 0.5)           # query 11's maximum before (b) sits in the first tile: a lazy maximum is that one
        plant(11, jb, 64 * (nt - 2), 4.0)
        info = {"ramp": ramp, "b": (11, jb), "a": (3, N - 1)}
        if jc != N - 1:                            # (a last tile of one key holds (a) only)
            plant(20, jc, 64 * (nt - 1), 15.0)
            info["c"] = (20, jc)
        plant(3, N - 1, 64 * (nt - 1), 100.0)
    elif N >= 2:
        plant(0, N - 1, 0, 100.0)
    return q, k, v, info


# ------------------------------------------------------------------------------------------------ reference
def _images(B: int):
    return sorted({0, B // 2, B - 1})


def reference(q, k, v, prec: str):
    """float64 reference of images [n, H, N, 64] (already selected): ref, A [n, N, H * 64], T [n, N, H] and the scores / weights."""
    if prec == "bf16":
        qs = (q * C32).to(torch.bfloat16).double()             # attn_probe_pack_kernel: one fp32 multiply, one rounding
        kd, vd = k.to(torch.bfloat16).double(), v.to(torch.bfloat16).double()
    else:
        qs, kd, vd = q.double() * C64, k.double(), v.double()
    s2 = qs @ kd.transpose(-1, -2)                              # scores in log2 units [n, H, N, N]
    w = torch.softmax(s2 * math.log(2.0), dim=-1)
    T = (qs.abs() @ kd.abs().transpose(-1, -2)).max(dim=-1).values          # [n, H, N]
    n, H, N, _ = q.shape
    to_rows = lambda t: t.permute(0, 2, 1, 3).reshape(n, N, H * 64)
    return to_rows(w @ vd), to_rows(w @ vd.abs()), T.permute(0, 2, 1), s2, w


def delta_of(A, T, N: int, prec: str):
    rP = {"bf16": 2.0 ** -8, "fp32": 0.0, "bf16x3": 2.0 ** -16}[prec]
    rS = 1.5 * (264 if prec == "bf16x3" else 72) * U
    rF = (2 * N + 2 * (-(-N // 64)) + 16) * U + 2.0 ** -22
    n, Nn, H = T.shape
    Trow = T[..., None].expand(n, Nn, H, 64).reshape(n, Nn, H * 64)
    return (rP + rF + rS * Trow) * A


def check_family_conditions(fam, info, s2, w, N):
    if fam in "23":
        tw = w.gather(-1, info["pi"].view(1, 1, N, 1).expand(*w.shape[:3], 1))
        assert float(tw.min()) >= 0.9, ("F2: a target key's softmax weight is below 0.9", float(tw.min()))
    if fam == "4" and "b" in info:
        nt = -(-N // 64)
        t2 = slice(64 * (nt - 2), 64 * (nt - 1))
        ramp = info["ramp"]
        grp = [i for i in range(32) if i < N]
        rise = s2[:, :, grp, t2].max(-1).values - s2[:, :, grp, :64 * (nt - 2)].max(-1).values
        assert float(rise.max()) <= 8.0 and 3.0 <= float(rise[:, :, 11].min()) and float(rise[:, :, 11].max()) <= 6.0, \
            ("F4 (b)", float(rise.max()), float(rise[:, :, 11].min()), float(rise[:, :, 11].max()))
        first = s2[:, :, 11, info["b"][1]] - s2[:, :, 11, :64].max(-1).values         # the lazy maximum is at least the first tile's
        assert float(first.max()) <= 8.0, ("F4 (b) against the first tile", float(first.max()))
        if "c" in info:
            i, j = info["c"]
            rc = s2[:, :, i, j] - s2[:, :, i, :64 * (j // 64)].max(-1).values
            assert 10.0 <= float(rc.min()) and float(rc.max()) <= 20.0, ("F4 (c)", float(rc.min()), float(rc.max()))
        i, j = info["a"]
        ra = s2[:, :, i, j] - s2[:, :, i, :64 * (nt - 1)].max(-1).values
        assert float(ra.min()) >= 50.0, ("F4 (a)", float(ra.min()))
        for r in ramp:
            d = s2[:, :, r, :]
            steps = (d[..., 64:] - d[..., :-64]) / 64.0                                # mean slope over 64 keys
            assert 0.4 <= float(steps.min()) and float(steps.max()) <= 0.6, ("F4 ramp", float(steps.min()), float(steps.max()))


# ------------------------------------------------------------------------------------------------ running one case
WORST: Dict[str, float] = {}


def run_family(cs: Case, fam: str, dev, seed: int):
    from desktop2stereo_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    B, H, N = cs.B, cs.heads, cs.N
    D = H * 64
    q, k, v, info = family(fam, B, H, N, g, dev, C32 if cs.prec == "bf16" else C64)
    imgs = _images(B)
    ref, A, T, s2, w = reference(q[imgs], k[imgs], v[imgs], cs.prec)
    check_family_conditions(fam, info, s2, w, N)
    del s2, w
    delta = delta_of(A, T, N, cs.prec)
    oscale = 0.0
    if cs.e4m3:                                    # ~1 % of this run's outputs saturate
        srt = ref.abs().flatten().sort().values
        oscale = float(torch.tensor(448.0 / float(srt[int(0.99 * (srt.numel() - 1))]), dtype=torch.float32))
    old = {key: os.environ.get(key) for key in cs.env}
    try:
        os.environ.update(cs.env)
        ops.reload_env()
        r1 = ops.attention_probe_ex(q, k, v, cs.prec, out_e4m3=cs.e4m3, oscale=oscale)
        r2 = ops.attention_probe_ex(q, k, v, cs.prec, out_e4m3=cs.e4m3, oscale=oscale)
    finally:
        for key, val in old.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        ops.reload_env()
    name = r1["kernel"]
    tag = (cs.id, cs.prec, "F" + fam, name)
    raw = r1["guard"].view(torch.uint8)
    assert bool((raw[0] == 0x7f).all()) and bool((raw[-1] == 0x7f).all()), (tag, "a guard row was written")
    assert r2["kernel"] == name and torch.equal(raw, r2["guard"].view(torch.uint8)), (tag, "not bit-identical on a second run")
    out = r1["out"].view(B, N, -1)[imgs]
    if cs.e4m3:
        assert not bool(((out & 0x7f) == 0x7f).any()), (tag, "NaN byte (0x7f / 0xff) in the e4m3 output", int(((out & 0x7f) == 0x7f).sum()))
        got = e4m3_value(out)
        lo, hi = rne_e4m3((ref - delta) * oscale), rne_e4m3((ref + delta) * oscale)
        ok = (got >= lo) & (got <= hi)
        sat = (ref.abs() - delta) * oscale > 448.0
        assert bool((got.abs()[sat] == 448.0).all()), (tag, "an element beyond the range is not saturated")
        ge = torch.frexp(got.abs().clamp_min(2.0 ** -9))[1]
        half = torch.where(got.abs() < 2.0 ** -6, torch.full_like(got, 2.0 ** -10), pow2(ge - 5)) / oscale
        err = ((got / oscale - ref).abs() - half).clamp_min(0)
        err = torch.where(ref.abs() * oscale >= 448.0, torch.zeros_like(err), err)
    else:
        if cs.prec == "bf16x3":
            got = bx3_value(out)
        else:
            got = out.double()
        assert bool(torch.isfinite(got).all()), (tag, "NaN or inf in the output", int((~torch.isfinite(got)).sum()),
                                                 "rows", (~torch.isfinite(got)).any(-1).nonzero()[:8].tolist())
        if cs.prec == "bf16":
            lo, hi = rne_bf16(ref - delta), rne_bf16(ref + delta)
            ok = (got >= lo) & (got <= hi)
            half = pow2(torch.frexp(got.abs().clamp_min(2.0 ** -120))[1] - 9)
            err = ((got - ref).abs() - half).clamp_min(0)
        else:
            err = (got - ref).abs()
            ok = err <= delta
    ratio = float((err / delta.clamp_min(1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"[attention] {cs.id:34s} {cs.prec:6s} F{fam} {name:50s} max_err/delta={ratio:.3f} oscale={oscale:.4g}")
    assert name == cs.expect, (tag, "dispatch moved", cs.expect)
    bad = ~ok
    assert not bool(bad.any()), (tag, "outside the bound", int(bad.sum()), "of", bad.numel(), "worst err/delta", ratio,
                                 "first (image, row, column)", bad.nonzero()[:4].tolist())
    if cs.prec != "bf16" and fam in "12":           # the gate of test_attention_probe: the bound is nowhere looser than it
        gate = (2e-5 if cs.prec == "fp32" else 2e-4) * max(1.0, float(ref.abs().max()) / 4)
        assert float(err.max()) <= gate, (tag, "outside the global gate", float(err.max()), gate)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@GPU
@pytest.mark.parametrize("cs", CASES, ids=[f"{c.id}-{c.prec}" for c in CASES])
def test_attention_against_float64(dev, cs):
    """One launch of launch_attention per input family of the case, against float64, per element; names the kernel it expects."""
    for fam in cs.fam:
        run_family(cs, fam, dev, seed=7000 + 10 * CASES.index(cs) + int(fam))
    print("[attention worst] " + " | ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
