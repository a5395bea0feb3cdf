"""The small model-side kernels of vit_ops.hip against float64, through d2s_vit_probe: patchify_kernel (im2col rows + the cls row),
bilinear_nhwc_kernel (align_corners up-sample, optional + addend), head_final_kernel (1x1 C -> 1, ReLU | sigmoid * max_depth),
amax_kernel and to_f32_kernel, in both storage types.  Operands are already in the kernel's storage type, every output lies between
guard regions of 0x7f bytes, every case runs twice and must repeat bit for bit, every returned kernel name is asserted.  Per element,
nothing sampled.  References, bounds and input families live in vit_ref.py; test_cpu_vit_ref.py shows on the host that float32
emulations pass these judges on these very case tables and that sixteen deliberate errors do not.

Up-sample and head tail are held to the bounds of vit_ref.py; in bf16 the up-sample must also equal
rne_bf16(fl32(test_gpu_conv3.ups_operand_f32(x) + addend)) bit for bit.  Patchify, amax and to_f32 are exact.

Measured worst err / delta per kernel: DESIGN.md (float64 references, small model-side kernels)."""
from typing import Dict

import numpy as np
import pytest
import torch

import vit_ref as R
from test_gpu_temporal import guarded, guards_intact, twice

GPU = pytest.mark.gpu

T_OF = {"bf16": "bf16", "fp32": "f32"}
DT_OF = {"bf16": torch.bfloat16, "fp32": torch.float32}
CHUNK = {"bf16": 8, "fp32": 4}                   # elements of a 16-byte channel chunk
PRECS = ("bf16", "fp32")
KERNELS = ("patchify_kernel", "bilinear_nhwc_kernel", "head_final_kernel", "to_f32_kernel", "amax_kernel")
TABLE = [f"{k}<{t}>" for k in KERNELS for t in ("bf16", "f32")]

WORST: Dict[str, float] = {}
SEEN = set()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def note(name, ratio):
    SEEN.add(name)
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def stored(a, prec, dev):
    """float32 numpy array of stored values -> the device tensor of the precision's type (bf16-representable values convert exactly)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(DT_OF[prec]).contiguous()


def as_f32(t):
    return t.float().cpu().numpy()


def raw(t):
    """device tensor -> numpy array of its bits (uint16 for bf16, else the dtype's own)"""
    return t.cpu().view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ up-sample
UPS_SHAPES = [                                   # (id, Hi, Wi, Ho, Wo, a wider C or None): every shape also runs with C = the chunk
    ("fusion-x2", 6, 10, 12, 20, 64),
    ("non-integer-scale", 7, 13, 11, 21, 32),
    ("head-interpolate", 24, 40, 42, 70, 32),
    ("scale-1", 5, 7, 5, 7, None),
    ("one-row-source", 1, 3, 4, 9, None),
    ("scale-0", 3, 3, 1, 1, None),
    ("coordinate-error", 3, 512, 5, 1023, None),
    ("ragged-x-blocks", 37, 37, 74, 74, 128),
    ("last-grid-y", 2, 1, 65535, 1, None),
]
UPS_B = 2
UPS_CASES = [(s, prec) for s in UPS_SHAPES for prec in PRECS]


def ups_variants(shape, prec):
    """-> [(C, with addend)] of one (shape, precision)"""
    Cs = [CHUNK[prec]] + ([shape[5]] if shape[5] else [])
    return [(C, add) for C in Cs for add in (False, True)]


def ups_check(shape, prec, C, add, x, addend, got_f32, got_bits):
    """every assertion on one up-sample result that needs no device (test_cpu_vit_ref.py runs it on the emulation) -> err / delta"""
    from test_gpu_conv3 import ups_operand_f32
    sid, Hi, Wi, Ho, Wo, _ = shape
    bf = prec == "bf16"
    tag = (sid, prec, C, add)
    ref, delta = R.upsample_ref(x, Ho, Wo, addend if add else None)
    ok, ratio = R.upsample_judge(got_f32, ref, delta, bf)
    assert ok.all(), (tag, "outside the bound", int((~ok).sum()), "of", ok.size, "worst", ratio, np.argwhere(~ok)[:4].tolist())
    if bf:
        v = ups_operand_f32(torch.from_numpy(x), Ho, Wo)
        if add:
            v = v + torch.from_numpy(addend)
        assert R.same_bits(got_bits, R.to_bf16_bits(v.numpy())), (tag, "differs from rne_bf16(fl32(ups_operand_f32(x) + addend))")
    if not add:
        src = R.to_bf16_bits(x) if bf else x
        assert R.same_bits(got_bits[:, 0, 0], src[:, 0, 0]), (tag, "output (0, 0) is not source (0, 0)")
        if Ho > 1 and Wo > 1:
            assert R.same_bits(got_bits[:, Ho - 1, Wo - 1], src[:, Hi - 1, Wi - 1]), (tag, "the last corner is not the source's")
        elif Ho > 1:
            assert R.same_bits(got_bits[:, Ho - 1, 0], src[:, Hi - 1, 0]), (tag, "the last row's corner is not the source's")
        if (Hi, Wi) == (Ho, Wo):
            assert R.same_bits(got_bits, src), (tag, "scale 1 is not exact")
    return ratio


@GPU
@pytest.mark.parametrize("cs", UPS_CASES, ids=[f"{s[0]}-{p}" for s, p in UPS_CASES])
def test_upsample_against_float64(dev, cs):
    from desktop2stereo_amd import ops
    shape, prec = cs
    sid, Hi, Wi, Ho, Wo, _ = shape
    rng = np.random.default_rng(21000 + UPS_CASES.index(cs))
    for C, add in ups_variants(shape, prec):
        x, addend = R.upsample_inputs(rng, UPS_B, Hi, Wi, Ho, Wo, C, prec == "bf16")
        xd, ad = stored(x, prec, dev), stored(addend, prec, dev)
        buf, out = guarded((UPS_B, Ho, Wo, C), DT_OF[prec], dev)
        name = twice(lambda: ops.vit_probe("bilinear", prec, xd, out, B=UPS_B, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, channels=C, addend=ad if add else None),
                     [buf])
        assert name == f"bilinear_nhwc_kernel<{T_OF[prec]}>", (sid, prec, C, add, name)
        assert guards_intact(buf), (sid, prec, C, add, "a guard was written")
        ratio = ups_check(shape, prec, C, add, x, addend, as_f32(out), raw(out))
        note(name, ratio)
        print(f"[vit] upsample {sid:20s} {prec} C={C} addend={int(add)} max_err/delta={ratio:.3f}")


@GPU
@pytest.mark.parametrize("prec", PRECS)
def test_upsample_refusals(dev, prec):
    """Channels that are no chunk multiple: D2S_E_INVALID (1); 65536 output rows: D2S_E_UNSUPPORTED (5).  The buffers are large enough
    for the stated shape; the launcher refuses on the host and nothing is written."""
    from desktop2stereo_amd import _lib, ops
    ce = CHUNK[prec]
    x = torch.zeros((1, 2, 1, 2 * ce), dtype=DT_OF[prec], device=dev)
    buf, out = guarded((65536 * ce,), DT_OF[prec], dev)
    with pytest.raises(_lib.D2SError, match=r"status 1\)"):
        ops.vit_probe("bilinear", prec, x, out, B=1, Hi=2, Wi=1, Ho=4, Wo=2, channels=ce + ce // 2)
    with pytest.raises(_lib.D2SError, match=r"status 5\)"):
        ops.vit_probe("bilinear", prec, x, out, B=1, Hi=2, Wi=1, Ho=65536, Wo=1, channels=ce)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.uint8) == 0x7f).all())


# ------------------------------------------------------------------------------------------------ head tail
HEAD_C = (32, 64, 128)
HEAD_NPIX = (1, 255, 256, 257, 1000)
HEAD_DEPTH = (0.0, 20.0, 80.0)
HEAD_CASES = [(C, prec) for C in HEAD_C for prec in PRECS]


def head_check(tag, x, w3, b3, md, got):
    """-> err / delta; asserts the input family on the reference first: both signs of s, and (from 255 pixels on) saturated pixels"""
    ref, delta, s = R.head_ref(x, w3, b3, md)
    if s.size >= 255:
        assert (s > 30).sum() >= 8 and (s < -30).sum() >= 8 and ((s > 0) & (s < 30)).any() and ((s < 0) & (s > -30)).any(), (tag, "input family")
    assert np.isfinite(got).all() and (got >= 0).all(), (tag, "NaN, inf or a negative depth")
    ok, ratio = R.judge_float(got, ref, delta)
    assert ok.all(), (tag, "outside the bound", int((~ok).sum()), "of", ok.size, "worst", ratio, np.argwhere(~ok)[:4].tolist())
    return ratio


@GPU
@pytest.mark.parametrize("cs", HEAD_CASES, ids=[f"C{c}-{p}" for c, p in HEAD_CASES])
def test_head_final_against_float64(dev, cs):
    from desktop2stereo_amd import ops
    C, prec = cs
    rng = np.random.default_rng(22000 + HEAD_CASES.index(cs))
    for npix in HEAD_NPIX:
        x, w3, b3 = R.head_inputs(rng, npix, C, prec == "bf16")
        xd, wd = stored(x, prec, dev), torch.from_numpy(w3).to(dev)
        for md in HEAD_DEPTH:
            buf, out = guarded((npix,), torch.float32, dev)
            name = twice(lambda: ops.vit_probe("head_final", prec, xd, out, n=npix, channels=C, w3=wd, b3=float(b3), max_depth=md), [buf])
            assert name == f"head_final_kernel<{T_OF[prec]}>" and guards_intact(buf), (cs, npix, md, name)
            ratio = head_check((cs, npix, md), x, w3, b3, md, as_f32(out))
            note(name, ratio)
            print(f"[vit] head_final C={C} {prec} npix={npix} max_depth={md} max_err/delta={ratio:.3f}")


# ------------------------------------------------------------------------------------------------ patchify
PATCH_CASES = [                                  # (id, B, gh, gw, p, Kp, D)
    ("ordinary", 2, 2, 3, 14, 640, 384),
    ("grid-by-cls-rows-B1", 1, 1, 1, 14, 640, 1024),
    ("grid-by-cls-rows-B2", 2, 1, 1, 14, 640, 1024),
    ("wide-padding", 1, 3, 2, 4, 64, 8),
    ("no-padding", 1, 1, 5, 16, 768, 32),
]
PATCH_POS_ROWS = 3                               # pos holds more than row 0: reading row 1 shows


def patch_inputs(cs):
    """-> x [B,3,h,w], cls [D], pos [PATCH_POS_ROWS D], N"""
    cid, B, gh, gw, p, Kp, D = cs
    rng = np.random.default_rng(23000 + PATCH_CASES.index(cs))
    x = R.naming_planes(rng, B, gh * p, gw * p)
    cls = rng.standard_normal(D).astype(np.float32)
    pos = rng.standard_normal(PATCH_POS_ROWS * D).astype(np.float32)
    return x, cls, pos, gh * gw + 1


def patch_check(cs, prec, with_cls, x, cls, pos, resid0, A, resid):
    cid, B, gh, gw, p, Kp, D = cs
    tag = (cid, prec, with_cls)
    ut = np.uint16 if prec == "bf16" else np.uint32
    want = R.patchify_expected(x, p, Kp, prec == "bf16")
    assert R.same_bits(A, want), (tag, "patch rows differ", np.argwhere(A.view(ut) != want.view(ut))[:4].tolist())
    wantr = R.cls_rows_expected(resid0, cls if with_cls else None, pos, D)
    assert R.same_bits(resid, wantr), (tag, "residual rows differ", np.argwhere(resid.view(np.uint32) != wantr.view(np.uint32))[:4].tolist())
    assert R.same_bits(resid[:, 1:], resid0[:, 1:]), (tag, "a row other than the cls row was written")


@GPU
@pytest.mark.parametrize("cs", PATCH_CASES, ids=[c[0] for c in PATCH_CASES])
def test_patchify_bit_for_bit(dev, cs):
    from desktop2stereo_amd import ops
    cid, B, gh, gw, p, Kp, D = cs
    x, cls, pos, N = patch_inputs(cs)
    assert (B * gh * gw * Kp < B * D) == cid.startswith("grid-by-cls-rows")
    xd, cd, pd = (torch.from_numpy(t).to(dev) for t in (x, cls, pos))
    for prec in PRECS:
        for with_cls in (True, False):
            abuf, A = guarded((B * gh * gw, Kp), DT_OF[prec], dev)
            rbuf, resid = guarded((B, N, D), torch.float32, dev)
            resid0 = raw(resid).copy()

            def run():
                return ops.vit_probe("patchify", prec, xd, A, B=B, h=gh * p, w=gw * p, p=p, Kp=Kp, N=N, D=D, cls=cd if with_cls else None,
                                     pos=pd if with_cls else None, resid=resid)
            name = twice(run, [abuf, rbuf])
            assert name == f"patchify_kernel<{T_OF[prec]}>", (cid, prec, name)
            assert guards_intact(abuf) and guards_intact(rbuf), (cid, prec, with_cls, "a guard was written")
            patch_check(cs, prec, with_cls, x, cls, pos, resid0, raw(A), raw(resid))
            note(name, 0.0)


# ------------------------------------------------------------------------------------------------ amax
AMAX_N = (1, 63, 64, 65, 255, 257, 2047, 2048, 2049, 4101, 2048 * 1024 + 6151)
AMAX_SLOTS = (0.0, 2.0, 5.0)


def amax_cases(n):
    """-> [(planted position, negative, slot before)]: every position with every slot value, the sign alternating"""
    out = []
    for pos in R.amax_positions(n):
        for slot in AMAX_SLOTS:
            out.append((pos, len(out) % 2 == 1, slot))
    return out


@GPU
@pytest.mark.parametrize("n", AMAX_N)
def test_amax_bit_for_bit(dev, n):
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(24000 + n % 1000)
    if n == AMAX_N[-1]:
        assert R.amax_blocks(n) == 1024 and n // 2048 > 1024 and n % (1024 * 256)           # the cap, and a ragged grid-stride tail
    for prec in PRECS:
        base = R.amax_background(rng, n, prec == "bf16")
        assert float(np.abs(base).max()) <= 1.0
        xd = stored(base, prec, dev)
        for pos, neg, slot in amax_cases(n):
            xd[pos] = -3.0 if neg else 3.0
            x = base.copy()
            x[pos] = -3.0 if neg else 3.0
            buf, out = guarded((3,), torch.float32, dev)
            before = torch.tensor([11.0, slot, 13.0], device=dev)

            def run():
                out.copy_(before)
                return ops.vit_probe("amax", prec, xd, out[1:], n=n)
            name = twice(run, [buf])
            xd[pos] = float(base[pos])
            assert name == f"amax_kernel<{T_OF[prec]}>" and guards_intact(buf), (n, prec, pos, neg, slot, name)
            want = np.array([11.0, R.amax_expected(x, slot), 13.0], np.float32)
            assert float(want[1]) == max(slot, 3.0)
            assert R.same_bits(raw(out), want), (n, prec, pos, neg, slot, raw(out).tolist(), want.tolist())
            note(name, 0.0)


# ------------------------------------------------------------------------------------------------ to_f32
TOF_N = (1, 255, 256, 257, 4099)


@GPU
@pytest.mark.parametrize("prec", PRECS)
def test_to_f32_bit_for_bit(dev, prec):
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(25000)
    for n in TOF_N:
        x = R.to_f32_inputs(rng, n, prec == "bf16")
        xd = torch.from_numpy(x.view(np.int16) if prec == "bf16" else x).to(dev)
        xd = xd.view(torch.bfloat16) if prec == "bf16" else xd
        buf, out = guarded((n,), torch.float32, dev)
        name = twice(lambda: ops.vit_probe("to_f32", prec, xd, out, n=n), [buf])
        assert name == f"to_f32_kernel<{T_OF[prec]}>" and guards_intact(buf), (prec, n, name)
        assert R.same_bits(raw(out), R.to_f32_expected(x, prec == "bf16")), (prec, n)
        note(name, 0.0)


# ------------------------------------------------------------------------------------------------ the probe's own checks
REFUSED_GOOD = {"in": 16, "out": 36, "planes": 48, "A": 64, "cls": 8, "pos": 8, "resid": 40, "hx": 32, "depth": 4, "w3": 8}      # elements


def refused_cases(mk, good):
    """Malformed calls the probe refuses on the host, as (label, keyword arguments of ops.vit_probe / the raw struct).  mk(n, offset in
    bytes) makes a float buffer of n elements; good: a dict of well-formed buffers.  Shared with test_cpu_vit_ref.py, which passes host
    memory."""
    g = good
    up = dict(op="bilinear", precision="fp32", x=g["in"], out=g["out"], B=1, Hi=2, Wi=2, Ho=3, Wo=3, channels=4)
    pa = dict(op="patchify", precision="fp32", x=g["planes"], out=g["A"], B=1, h=4, w=4, p=2, Kp=16, N=5, D=8, cls=g["cls"], pos=g["pos"], resid=g["resid"])
    hd = dict(op="head_final", precision="fp32", x=g["hx"], out=g["depth"], n=4, channels=8, w3=g["w3"])
    return [
        ("bilinear: in too small", {**up, "Hi": 3}),
        ("bilinear: out too small", {**up, "Ho": 4}),
        ("bilinear: addend too small", {**up, "addend": mk(3 * 3 * 4 - 1, 0)}),
        ("bilinear: in misaligned", {**up, "x": mk(2 * 2 * 4, 4)}),
        ("bilinear: out misaligned", {**up, "out": mk(3 * 3 * 4, 8)}),
        ("bilinear: addend misaligned", {**up, "addend": mk(3 * 3 * 4, 4)}),
        ("bilinear: null out", {**up, "out": None}),
        ("bilinear: zero width", {**up, "Wo": 0}),
        ("patchify: planes too small", {**pa, "B": 2}),
        ("patchify: A too small", {**pa, "Kp": 17}),
        ("patchify: Kp below 3 p^2", {**pa, "Kp": 11}),
        ("patchify: h no multiple of p", {**pa, "h": 3}),
        ("patchify: resid too small", {**pa, "N": 6}),
        ("patchify: pos too small", {**pa, "pos": mk(7, 0)}),
        ("patchify: cls without resid", {**pa, "resid": None}),
        ("patchify: null A", {**pa, "out": None}),
        ("head_final: x too small", {**hd, "n": 5, "out": mk(5, 0)}),
        ("head_final: depth too small", {**hd, "out": mk(3, 0)}),
        ("head_final: w3 too small", {**hd, "w3": mk(7, 0)}),
        ("head_final: null w3", {**hd, "w3": None}),
        ("head_final: negative max_depth", {**hd, "max_depth": -1.0}),
        ("to_f32: out too small", dict(op="to_f32", precision="fp32", x=g["hx"], out=g["depth"], n=5)),
        ("to_f32: in too small", dict(op="to_f32", precision="fp32", x=g["depth"], out=g["hx"], n=5)),
        ("amax: x too small", dict(op="amax", precision="fp32", x=g["depth"], out=g["hx"], n=5)),
        ("amax: no count", dict(op="amax", precision="fp32", x=g["depth"], out=g["hx"], n=0)),
        ("amax: null slot", dict(op="amax", precision="fp32", x=g["depth"], out=None, n=4)),
    ]


@GPU
def test_probe_refuses_malformed_cases(dev):
    """Every case of refused_cases is an error return on the host; no buffer changes."""
    from desktop2stereo_amd import _lib, ops
    made = []

    def mk(n, off=0):
        whole = torch.empty(n + 8, dtype=torch.float32, device=dev)
        whole.view(torch.uint8).fill_(0x7f)
        made.append(whole)
        return whole[off // 4:off // 4 + n]
    good = {k: mk(n) for k, n in REFUSED_GOOD.items()}
    for label, kw in refused_cases(mk, good):
        kw = dict(kw)
        with pytest.raises(_lib.D2SError):                           # (ops.vit_probe passes a missing tensor as a null pointer)
            ops.vit_probe(kw.pop("op"), kw.pop("precision"), kw.pop("x"), kw.pop("out"), **kw)
            pytest.fail(f"malformed case was accepted: {label}")
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x7f).all()) for t in made)


# ------------------------------------------------------------------------------------------------ coverage of the table
@GPU
def test_every_kernel_name_was_produced(dev):
    """The ten names (five kernels, two types) are exactly what the cases above produced."""
    assert SEEN == set(TABLE), (sorted(set(TABLE) - SEEN), sorted(SEEN - set(TABLE)))


@GPU
def test_worst_ratios_are_reported(dev):
    """Prints the worst err / delta per kernel over the whole file (the table in DESIGN.md)."""
    print("[vit worst] " + " | ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
