"""The frame-side kernels (frame_ops.hip) against float64: pre-process (bilinear in three formats, the patch-row form through
d2s_preprocess_patches_probe, bicubic-antialias), depth up-sample, and both stereo-warp kernels through d2s_make_sbs with the kernel named
by d2s_warp_plan.  Every output lies between guard regions of 0x7f bytes that must stay intact, every case runs twice and must be
bit-identical, every warp and patch case asserts the kernel it expects.  Judges are per element with no exemptions; references, bounds
(derived in frame_ref.py's docstring from each kernel's arithmetic) and input families live in frame_ref.py, and test_cpu_frame_ref.py
shows on the host that float32 / integer emulations pass these judges and that fourteen deliberate errors do not.

Warp dispatch restated here (expect_warp): the gather kernel for u8 HWC in and out, no padding, W % 4 == 0, 8 <= W < 16384, 4-byte aligned
buffers, H W 3 % 4 == 0, even H under Half-TAB, and depth either at the frame's size (DIRECT, NC = 4) or with 3 dw < W (NC = 3) or
3 dw < 2 W (NC = 4), dw >= NC, dh <= H; the generic kernel otherwise.  In-kernel paths of the gather kernel per wave-row: LDS taps
while every column's |shift| < 63 px, taps from global memory while < W - 1, else the float path (also the buffer's last row in the
last tile); a case built for one path asserts the class on the REFERENCE's float64 shifts with >= 2 px of margin.

Measured worst err / delta per kernel: DESIGN.md (float64 references, frame-side kernels)."""
import os

import numpy as np
import pytest
import torch

import frame_ref as R

GPU = pytest.mark.gpu
GUARD = 256
WORST = {}
FMT = {"U8_HWC": 0, "F32_CHW": 1, "F32_HWC": 2, "U8_CHW": 3}
MODE_NAME = {"Half-SBS": "HALF_SBS", "Full-SBS": "FULL_SBS", "Half-TAB": "HALF_TAB", "Full-TAB": "FULL_TAB"}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN2, STD2 = (0.3, 0.55, 0.41), (0.31, 0.2, 0.27)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def guarded(shape, dtype, dev, src=None):
    """-> (whole buffer, the view of `shape` inside it); all bytes 0x7f, or the view filled from the numpy array src"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(0x7f)
    view = buf[GUARD:GUARD + n].view(tuple(shape))
    if src is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(src)).view(tuple(shape)))
    return buf, view


def guards_intact(buf) -> bool:
    raw = buf.view(torch.uint8)
    gb = GUARD * buf.element_size()
    return bool((raw[:gb] == 0x7f).all()) and bool((raw[-gb:] == 0x7f).all())


def twice(run, bufs):
    """run() on 0x7f-filled buffers, twice: the second run's result and bytes must equal the first's.  -> the first result"""
    name = run()
    torch.cuda.synchronize()
    first = [b.clone() for b in bufs]
    for b in bufs:
        b.view(torch.uint8).fill_(0x7f)
    assert run() == name
    torch.cuda.synchronize()
    for a, b in zip(first, bufs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, "not bit-identical on a second run")
        assert guards_intact(b), (name, "guard bytes overwritten")
    return name


class env:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from desktop2stereo_amd import ops
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
        ops.reload_env()

    def __exit__(self, *exc):
        from desktop2stereo_amd import ops
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.reload_env()


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"[frame_ops] {name}: err/delta {ratio:.3f}")


def where_bad(ok):
    idx = np.argwhere(~ok)
    return f"{len(idx)} of {ok.size} elements outside the bound, first at {idx[0].tolist() if len(idx) else None}"


# ================================================================================================ pre-process, bilinear
PRE_CASES = [  # (B, H, W, h, w, stride, square, mean / std)
    (1, 1, 1, 14, 14, 1, 0, 0), (3, 5, 7, 14, 14, 1, 0, 0), (1, 30, 41, 14, 28, 1, 0, 1), (3, 28, 42, 28, 42, 1, 0, 0),
    (1, 31, 45, 14, 28, 2, 0, 0), (3, 31, 45, 14, 28, 3, 0, 1), (1, 30, 44, 14, 28, 2, 0, 0), (1, 31, 46, 14, 28, 3, 0, 0),
    (1, 9, 11, 15, 17, 1, 0, 0), (1, 9, 11, 16, 16, 1, 0, 0), (1, 9, 11, 1, 257, 1, 0, 0), (3, 31, 45, 14, 14, 3, 1, 1),
]


@GPU
@pytest.mark.parametrize("fmt", ["U8_HWC", "U8_CHW", "F32_CHW"])
def test_preprocess_bilinear(dev, fmt):
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(11)
    for (B, H, W, h, w, stride, square, ms) in PRE_CASES:
        px = R.noise_u8(rng, B, H, W) if fmt != "F32_CHW" else (rng.random((B, H, W, 3)) * 255).astype(np.float32)
        mean, std = (MEAN2, STD2) if ms else (MEAN, STD)
        _, frames = guarded(R.as_format(px, fmt).shape, torch.uint8 if fmt != "F32_CHW" else torch.float32, dev, R.as_format(px, fmt))
        buf, out = guarded((B, 3, h, w), torch.float32, dev)
        pre = ops.pre_params(mean, std, "bilinear", bool(square))
        twice(lambda: ops.preprocess_to(frames, out, stride, pre) is None, [buf])
        ref, delta = R.preprocess_bilinear(px.astype(np.float64), 1 if square else stride, h, w, mean, std)   # square = 1 ignores the stride
        ok, ratio = R.judge_float(out.cpu().numpy(), ref, delta)
        assert ok.all(), (fmt, (B, H, W, h, w, stride, square), where_bad(ok), ratio)
        note(f"preprocess_kernel<{fmt}>", ratio)


# ================================================================================================ pre-process, patch rows
PATCH_CASES = [  # (B, H, W, p, gh, gw, Kp, stride, D, cls)
    (1, 20, 23, 14, 1, 1, 640, 1, 32, 1), (3, 33, 50, 14, 1, 3, 640, 1, 32, 1), (1, 61, 97, 14, 2, 3, 640, 2, 32, 1),
    (3, 30, 41, 14, 2, 3, 640, 1, 48, 0), (3, 5, 7, 2, 1, 1, 16, 1, 8, 1), (1, 9, 14, 2, 2, 3, 16, 2, 64, 1), (3, 7, 9, 2, 1, 3, 12, 1, 4, 1),
]


@GPU
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_preprocess_patch_rows(dev, prec):
    from desktop2stereo_amd import ops, _lib
    rng = np.random.default_rng(12)
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    want = f"preprocess_patch_kernel<U8_HWC,{'bf16' if prec == 'bf16' else 'float'}>"
    for (B, H, W, p, gh, gw, Kp, stride, D, use_cls) in PATCH_CASES:
        h, w, N = gh * p, gw * p, gh * gw + 1
        px = R.noise_u8(rng, B, H, W)
        _, frames = guarded(px.shape, torch.uint8, dev, px)
        bufA, A = guarded((B * gh * gw, Kp), dt, dev)
        bufR, resid = guarded((B, N, D), torch.float32, dev)
        cls = torch.from_numpy(rng.standard_normal(D).astype(np.float32)).to(dev)
        pos = torch.from_numpy(rng.standard_normal(D + 5).astype(np.float32)).to(dev)
        pre = ops.pre_params(MEAN2, STD2)
        name = twice(lambda: ops.preprocess_patches_probe(prec, frames, A, resid, h=h, w=w, p=p, Kp=Kp, N=N, D=D, cls=cls if use_cls else None,
                                                          pos=pos, decim_stride=stride, pre=pre), [bufA, bufR])
        assert name == want
        ref, delta = R.preprocess_bilinear(px.astype(np.float64), stride, h, w, MEAN2, STD2)
        refA, dA = R.patch_rows(ref, p, Kp), R.patch_rows(delta, p, Kp)
        got = A.float().cpu().numpy()
        live = ~np.isnan(refA)
        ok, ratio = (R.judge_bf16 if prec == "bf16" else R.judge_float)(got[live], refA[live], dA[live])
        assert ok.all(), (prec, (B, H, W, p, gh, gw), where_bad(ok), ratio)
        note(want, ratio)
        raw = A.view(torch.uint8).view(B * gh * gw, Kp * A.element_size())[:, 3 * p * p * A.element_size():]
        assert bool((raw == 0x7f).all()), "columns >= 3 p^2 of A were written"
        rr = resid.view(torch.int32).cpu().numpy()
        assert (rr[:, 1:] == 0x7f7f7f7f).all(), "a patch row of resid was written"
        if use_cls:
            assert torch.equal(resid[:, 0], (cls + pos[:D]).expand(B, D)), "cls rows != cls + pos[0]"       # one float32 addition: exact
        else:
            assert (rr[:, 0] == 0x7f7f7f7f).all(), "cls = null wrote the cls rows"
    # the three unsupported inputs: D2S_E_UNSUPPORTED (5), nothing written
    px = R.noise_u8(rng, 1, 28, 28)
    _, frames = guarded(px.shape, torch.uint8, dev, px)
    _, chw = guarded((1, 3, 28, 28), torch.uint8, dev, px.transpose(0, 3, 1, 2))
    bufA, A = guarded((4, 640), dt, dev)
    bufR, resid = guarded((1, 5, 8), torch.float32, dev)
    pos = torch.zeros(8, device=dev)
    for kw, fr in ((dict(h=14, w=14, p=14, Kp=640), chw),                                # a format other than U8_HWC
                   (dict(h=28, w=28, p=14, Kp=640), frames),                             # same-size input
                   (dict(h=14, w=14, p=14, Kp=512), frames)):                            # 3 p^2 > Kp
        with pytest.raises(_lib.D2SError, match="status 5"):
            ops.preprocess_patches_probe(prec, fr, A, resid, N=5, D=8, cls=pos, pos=pos, **kw)
        torch.cuda.synchronize()
        assert bool((bufA.view(torch.uint8) == 0x7f).all()) and bool((bufR.view(torch.uint8) == 0x7f).all())
    with pytest.raises(_lib.D2SError):                                                   # a buffer smaller than the shape says: refused before the launch
        ops.preprocess_patches_probe(prec, frames, A.view(-1)[:600], resid, h=14, w=14, p=14, Kp=640, N=5, D=8, cls=pos, pos=pos)


# ================================================================================================ pre-process, bicubic + antialias
AA_CASES = [(1, 60, 104, 14, 28), (2, 10, 12, 28, 42), (1, 14, 50, 14, 28), (2, 33, 50, 9, 45), (1, 154, 30, 14, 14), (1, 210, 28, 14, 14)]


@GPU
@pytest.mark.parametrize("fmt", ["U8_HWC", "U8_CHW", "F32_CHW"])
def test_preprocess_bicubic_aa(dev, fmt):
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(13)
    for (B, H, W, h, w) in AA_CASES:
        px = R.noise_u8(rng, B, H, W) if fmt != "F32_CHW" else (rng.random((B, H, W, 3)) * 255).astype(np.float32)
        _, frames = guarded(R.as_format(px, fmt).shape, torch.uint8 if fmt != "F32_CHW" else torch.float32, dev, R.as_format(px, fmt))
        buf, out = guarded((B, 3, h, w), torch.float32, dev)
        pre = ops.pre_params(MEAN2, STD2, "bicubic_aa")
        twice(lambda: ops.preprocess_to(frames, out, 3, pre) is None, [buf])              # (the stride is ignored on this branch)
        ref, delta = R.preprocess_aa(px.astype(np.float64), h, w, MEAN2, STD2)
        ok, ratio = R.judge_float(out.cpu().numpy(), ref, delta)
        assert ok.all(), (fmt, (B, H, W, h, w), where_bad(ok), ratio)
        note(f"preprocess_aa_kernel<{fmt}>", ratio)


# ================================================================================================ depth up-sample
UP_CASES = [(1, 1, 1, 3, 5, 0), (3, 2, 3, 9, 16, 0), (1, 21, 37, 90, 160, 0), (3, 20, 20, 7, 9, 0), (1, 4, 5, 15, 17, 0), (1, 4, 5, 16, 16, 0),
            (1, 4, 5, 1, 257, 1), (3, 21, 37, 45, 80, 1)]


@GPU
def test_upsample_depth(dev):
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(14)
    for (B, h, w, H, W, big) in UP_CASES:
        d = (rng.random((B, h, w)) + (1e4 if big else 0.0)).astype(np.float32)
        _, src = guarded(d.shape, torch.float32, dev, d)
        buf, out = guarded((B, H, W), torch.float32, dev)
        twice(lambda: ops.upsample_depth_to(src, out) is None, [buf])
        ref, delta = R.upsample(d, H, W)
        ok, ratio = R.judge_float(out.cpu().numpy(), ref, delta)
        assert ok.all(), ((B, h, w, H, W, big), where_bad(ok), ratio)
        note("upsample_depth_kernel", ratio)


# ================================================================================================ warp
def expect_warp(in_fmt, out_fmt, mode, fill, B, H, W, dh, dw, aligned=True):
    gm = R.Geom(H, W, mode, fill)
    fast = (in_fmt == "U8_HWC" and out_fmt == "U8_HWC" and gm.Hp == H and gm.Wp == W and W % 4 == 0 and dw <= W and dh <= H and aligned
            and H * W * 3 % 4 == 0 and not (mode == "Half-TAB" and H % 2))
    direct = dw == W and dh == H
    nc = 4 if direct else (3 if 3 * dw < W else (4 if 3 * dw < 2 * W else 0))
    if fast and nc and dw >= nc and 8 <= W < 16384:
        return f"stereo_warp_gather<{MODE_NAME[mode]},NC={nc},DIRECT={int(direct)}>"
    return f"stereo_warp_generic<{in_fmt},{out_fmt}>"


def run_warp(dev, px, in_fmt, depth, out_fmt, mode, *, fill=False, ipd_uv=0.064, ratio=2.0, conv=0.0, wpc=None, expect=None, misalign=0,
             expect_rpw=None):
    """one d2s_make_sbs call judged against the float64 reference.  -> (reference dict, plan)"""
    from desktop2stereo_amd import ops
    B, H, W, _ = px.shape
    dh, dw = depth.shape[1:]
    arr = R.as_format(px, in_fmt)
    if misalign:                                                    # frames at an odd address: the generic kernel
        fb = torch.empty(arr.size + 8, dtype=torch.uint8, device=dev)
        frames = fb[misalign:misalign + arr.size].view(arr.shape)
        frames.copy_(torch.from_numpy(arr))
    else:
        _, frames = guarded(arr.shape, torch.uint8 if arr.dtype == np.uint8 else torch.float32, dev, arr)
    _, dep = guarded(depth.shape, torch.float32, dev, depth)
    sp = ops.sbs_params(ipd_uv, ratio, conv, mode, fill)
    with env(D2S_WARP_WPC=None if wpc is None else str(wpc)):
        plan = ops.warp_plan(FMT[in_fmt], dh, dw, B, H, W, sp, FMT[out_fmt], rgb_align=(frames.data_ptr() % 256) or 256)
        want = expect or expect_warp(in_fmt, out_fmt, mode, fill, B, H, W, dh, dw, aligned=not misalign)
        assert plan["kernel"] == want, (plan, want)
        if plan["gather"]:
            assert 1 <= plan["rpw"] <= H and (mode != "Half-TAB" or plan["rpw"] % 2 == 0), plan
            assert expect_rpw is None or plan["rpw"] == expect_rpw, (plan, expect_rpw)
        oh, ow = plan["out_h"], plan["out_w"]
        shape = (B, 3, oh, ow) if out_fmt == "F32_CHW" else (B, oh, ow, 3)
        buf, out = guarded(shape, torch.uint8 if out_fmt == "U8_HWC" else torch.float32, dev)
        twice(lambda: ops.make_sbs(frames, dep, sp, FMT[out_fmt], out=out) is None, [buf])
    got = out.cpu().numpy()
    if out_fmt == "F32_CHW":
        got = got.transpose(0, 2, 3, 1)
    ref = R.warp_ref(px.astype(np.float64), depth, ipd_uv=ipd_uv, ratio=ratio, conv=conv, mode=mode, fill=fill,
                     kernel="gather" if plan["gather"] else "generic")
    assert (ref["geom"].oh, ref["geom"].ow) == (oh, ow)
    ok, r = R.judge_range(got, ref["lo"], ref["hi"], ref["db"], out_fmt == "U8_HWC")
    assert ok.all(), (want, mode, px.shape, depth.shape, dict(fill=fill, ipd_uv=ipd_uv, ratio=ratio, conv=conv, wpc=wpc), where_bad(ok), r)
    note(want, r)
    return ref, plan


def frames_for(rng, family, B, H, W):
    return {"noise": lambda: R.noise_u8(rng, B, H, W), "naming": lambda: R.naming_u8(B, H, W), "float": lambda: R.float_frames(rng, B, H, W)}[family]()


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_generic_every_instantiation(dev, mode):
    """all 9 (in, out) instantiations x fill_16_9, padding on top (wide frame) and on the left (tall frame), odd sizes"""
    rng = np.random.default_rng(21)
    names = set()
    for in_fmt in ("U8_HWC", "U8_CHW", "F32_CHW"):
        for out_fmt in ("U8_HWC", "F32_HWC", "F32_CHW"):
            for fill in (False, True):
                for (B, H, W, dh, dw) in ((2, 9, 35, 3, 11), (1, 37, 23, 37, 23)):
                    px = frames_for(rng, "float" if in_fmt == "F32_CHW" else "noise", B, H, W)
                    ref, plan = run_warp(dev, px, in_fmt, R.depth_smooth(B, dh, dw), out_fmt, mode, fill=fill, ratio=8.0, conv=0.4)
                    assert not plan["gather"]
                    names.add(plan["kernel"])
                    if fill:
                        assert (ref["geom"].pt > 0) if W > H else (ref["geom"].pl > 0)
    assert names == {f"stereo_warp_generic<{i},{o}>" for i in ("U8_HWC", "U8_CHW", "F32_CHW") for o in ("U8_HWC", "F32_HWC", "F32_CHW")}


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_generic_shapes_and_shifts(dev, mode):
    rng = np.random.default_rng(22)
    cases = [  # (B, H, W, dh, dw, ratio, ipd, conv, family)
        (2, 7, 1, 3, 1, 2.0, 0.064, 0.0, "noise"),                 # W = 1: span 0
        (1, 96, 160, 96, 160, 4.0, 0.064, 0.5, "naming"),          # depth at frame size; W % 4 == 0 but padded below
        (2, 31, 54, 10, 18, 4.0, 0.064, -0.3, "naming"),           # W % 4 != 0, depth at a third, convergence < 0
        (1, 13, 22, 30, 50, 4.0, 0.064, 0.3, "noise"),             # depth larger than the frame (dh > H)
        (1, 11, 42, 5, 9, 0.5, 0.02, 0.5, "noise"),                # |shift| < 1 px
        (2, 11, 42, 5, 9, 30.0, 1.0, 0.0, "naming"),               # beyond one reflection
        (1, 11, 22, 5, 9, 60.0, 1.0, 0.1, "noise"),                # beyond 2 (W - 1): reflect_clip_slow, odd and even flip counts
    ]
    for (B, H, W, dh, dw, ratio, ipd, conv, fam) in cases:
        px = frames_for(rng, fam, B, H, W)
        dep = R.depth_smooth(B, dh, dw) if fam == "noise" else (R.depth_frames(B, dh, dw) + R.depth_smooth(B, dh, dw, 0.2)).astype(np.float32)
        ref, plan = run_warp(dev, px, "U8_HWC", dep, "U8_HWC", mode, fill=(H, W) == (96, 160), ratio=ratio, ipd_uv=ipd, conv=conv,
                             expect="stereo_warp_generic<U8_HWC,U8_HWC>")
        s = np.abs(ref["shift"])
        if ratio == 0.5:
            assert s.max() < 1.0
        if ratio == 30.0:
            assert s.max() > W - 1
        if ratio == 60.0:
            flips = np.floor((np.arange(W)[None, None, :] + s) / (W - 1)).astype(int)
            assert s.max() > 2 * (W - 1) and (flips[flips >= 2] % 2 == 0).any() and (flips[flips >= 2] % 2 == 1).any()
    # a 4-aligned frame whose buffer is not: the generic kernel
    px = R.naming_u8(2, 6, 36)
    run_warp(dev, px, "U8_HWC", R.depth_frames(2, 6, 36), "U8_HWC", mode, ratio=8.0, misalign=1)
    with env(D2S_WARP_GATHER="0"):
        run_warp(dev, px, "U8_HWC", R.depth_frames(2, 6, 36), "U8_HWC", mode, ratio=8.0, expect="stereo_warp_generic<U8_HWC,U8_HWC>")


def gather_depth_dims(layout, H, W):
    if layout == "DIRECT":
        return H, W
    if layout == "NC3":
        return max(1, H // 2), (W - 1) // 3
    return max(1, H // 2), W // 2                                   # NC4: W <= 3 dw < 2 W


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_gather_shapes(dev, mode):
    """W in {8, 12, 36, 252, 256, 260, 580} x {NC = 3, NC = 4, DIRECT}, H in {1, 2, 3, 6, 10}, batch 1, 2, 5 (Half-TAB with odd H and
    NC = 3 at W = 8 plan the generic kernel: expect_warp)"""
    rng = np.random.default_rng(23)
    Hs, Bs, i = (1, 2, 3, 6, 10), (1, 2, 5), 0
    names = set()
    for W in (8, 12, 36, 252, 256, 260, 580):
        for layout in ("NC3", "NC4", "DIRECT"):
            for rep in range(2):
                H, B = Hs[i % 5], Bs[i % 3]
                i += 1
                dh, dw = gather_depth_dims(layout, H, W)
                if dw < 1:
                    continue
                px = frames_for(rng, "naming" if i % 2 else "noise", B, H, W)
                dep = (R.depth_frames(B, dh, dw) + R.depth_smooth(B, dh, dw, 0.3)).astype(np.float32)
                _, plan = run_warp(dev, px, "U8_HWC", dep, "U8_HWC", mode, ratio=6.0 if i % 4 else 1.0, conv=0.45)
                names.add(plan["kernel"])
    m = MODE_NAME[mode]
    assert {f"stereo_warp_gather<{m},NC=3,DIRECT=0>", f"stereo_warp_gather<{m},NC=4,DIRECT=0>", f"stereo_warp_gather<{m},NC=4,DIRECT=1>"} <= names
    if mode == "Half-TAB":
        assert "stereo_warp_generic<U8_HWC,U8_HWC>" in names


@GPU
@pytest.mark.parametrize("mode", ["Full-SBS", "Half-TAB"])
def test_warp_gather_column_rule_thresholds(dev, mode):
    """dw = 40 under W in {116, 120, 124} (3 dw vs W) and {56, 60, 64} (3 dw vs 2 W); dw = nc and nc - 1; the last column's clamp"""
    rng = np.random.default_rng(24)
    m = MODE_NAME[mode]
    for W, want in ((116, f"stereo_warp_gather<{m},NC=4,DIRECT=0>"), (120, f"stereo_warp_gather<{m},NC=4,DIRECT=0>"),
                    (124, f"stereo_warp_gather<{m},NC=3,DIRECT=0>"), (56, "stereo_warp_generic<U8_HWC,U8_HWC>"),
                    (60, "stereo_warp_generic<U8_HWC,U8_HWC>"), (64, f"stereo_warp_gather<{m},NC=4,DIRECT=0>")):
        px = R.naming_u8(2, 6, W)
        dep = (rng.random((2, 3, 40))).astype(np.float32)          # rough depth: a wrong column is a different shift
        _, plan = run_warp(dev, px, "U8_HWC", dep, "U8_HWC", mode, ratio=8.0, conv=0.5, expect=want)
        if plan["gather"]:                                          # the last column's clamp: lanes whose first tap lies beyond dw - NC
            assert (R.linear_tap(W, 40)[0][::4] > 40 - plan["nc"]).any(), (W, plan)
    for W, dw, want in ((12, 3, f"stereo_warp_gather<{m},NC=3,DIRECT=0>"), (12, 2, "stereo_warp_generic<U8_HWC,U8_HWC>"),
                        (8, 4, f"stereo_warp_gather<{m},NC=4,DIRECT=0>"), (8, 3, "stereo_warp_generic<U8_HWC,U8_HWC>")):
        px = R.naming_u8(2, 4, W)
        run_warp(dev, px, "U8_HWC", rng.random((2, 2, dw)).astype(np.float32), "U8_HWC", mode, ratio=8.0, conv=0.5, expect=want)


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_gather_bands(dev, mode):
    """rows per wave 1, 2, 3 / odd (Half-TAB rounds up), bands ending mid-frame, crossing a frame boundary, a short last band, a band of
    more than 64 rows (the tap table refills), and the bands that would be longer than a frame (capped at H by plan_warp)"""
    htab = mode == "Half-TAB"
    seen = set()
    for (B, H, W, layout, wpc) in [(5, 6, 36, "NC3", 64), (5, 6, 36, "DIRECT", None), (5, 62, 260, "NC4", 1), (2, 100, 260, "NC3", 1),
                                   (3, 10, 580, "DIRECT", 1)]:
        dh, dw = gather_depth_dims(layout, H, W)
        px = R.naming_u8(B, H, W)
        dep = (R.depth_frames(B, dh, dw) + R.depth_smooth(B, dh, dw, 0.2)).astype(np.float32)
        want_rpw = -(-(B * H * -(-W // 256)) // (256 * (wpc or 12)))
        want_rpw = min(want_rpw + (want_rpw & 1 if htab else 0), H)
        _, plan = run_warp(dev, px, "U8_HWC", dep, "U8_HWC", mode, ratio=6.0, conv=0.4, wpc=wpc, expect_rpw=want_rpw)
        seen.add(plan["rpw"])
    assert seen == ({2, 4} if htab else {1, 2, 3})                 # (5, 62, 260): 3 rows per wave (4 for Half-TAB) -- bands cross frames, the last is short
    # a band of more than 64 rows: B = 2, H = 8300, W = 8, one wave per CU -> rpw = 65 (66 for Half-TAB); crosses the frame boundary
    B, H, W = 2, 8300, 8
    dep = (R.depth_frames(B, H, W, ramp=0.5) + R.depth_smooth(B, H, W, 0.2)).astype(np.float32)
    _, plan = run_warp(dev, R.naming_u8(B, H, W), "U8_HWC", dep, "U8_HWC", mode, ratio=20.0, ipd_uv=0.5, conv=0.4, wpc=1)
    assert plan["rpw"] > 64 and (B * H) % plan["rpw"] != 0
    # bands that would span several frames: per-frame constant depth, so the wrong frame's depth moves every pixel of the row
    for (B, H, W, wpc) in ((7000, 1, 8, None), (600, 2, 8, 1)):
        if htab and H % 2:
            continue
        px = R.naming_u8(B, H, W)
        dep = R.depth_frames(B, H, W, lo=0.0, hi=1.0, ramp=0.0)
        uncapped = -(-(B * H) // (256 * (wpc or 12)))
        assert uncapped > H + 1
        run_warp(dev, px, "U8_HWC", dep, "U8_HWC", mode, ratio=40.0, ipd_uv=0.5, conv=0.5, wpc=wpc, expect_rpw=H)


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_gather_in_kernel_paths(dev, mode):
    """whole wave-rows in one in-kernel path, the class asserted on the reference's float64 shifts (>= 2 px from the 63 px halo limit
    and from W - 1).  Bands here are one row long (a row pair under Half-TAB); path changes inside a band:
    test_warp_gather_path_changes_inside_a_band"""
    m = MODE_NAME[mode]
    B, H, W = 2, 6, 580
    px = R.naming_u8(B, H, W)
    kw = dict(ipd_uv=0.064, ratio=2.0, conv=0.0)

    def shifts(rows):
        return R.depth_for_shift(np.asarray(rows, np.float64), W, **kw)

    def run(rows, wpc=None, direct=True, frames=px):
        dep = shifts(rows)
        if not direct:                                              # model-resolution depth, constant per frame
            dep = np.ascontiguousarray(dep[:, :3, :W // 4])
        ref, plan = run_warp(dev, frames, "U8_HWC", dep, "U8_HWC", mode, wpc=wpc, **kw)
        assert plan["gather"] and plan["kernel"].startswith(f"stereo_warp_gather<{m}")
        return np.abs(ref["shift"])

    s = run([[5, -40, 17, 40, -1, 33]] * B)                          # all rows LDS (left-edge, interior and right tile)
    assert s.max() <= 40 + 1e-3
    s = run([[70, -300, 150, W - 10, -70, 200]] * B)                 # all rows take global taps, one reflection on either side
    assert s.min() >= 70 - 1e-3 and s.max() <= W - 10 + 1e-3
    s = run([[W + 2, -2 * W, W + 37.5, 3 * W, -W - 3, 5 * W + 0.25]] * B)   # all rows on the float path
    assert s.min() >= W + 1
    s = run([[10] * H, [-200] * H], direct=False)                    # NC = 3 depth: one frame LDS, one global
    if mode == "Half-TAB":                                          # pairs (slow, fast) and (fast, slow): both rows take the float path
        run([[W + 20, 5, 5, W + 20, 100, W + 3], [7, 2 * W, W + 1, -3, -W - 40, 60]], wpc=1)
    # the buffer's last row in the last tile with a large shift comes out of the float path (value check)
    run([[3] * H, [3] * (H - 1) + [200]])
    run([[3] * H, [3] * (H - 1) + [-100]], frames=R.noise_u8(np.random.default_rng(5), B, H, W))


@GPU
@pytest.mark.parametrize("mode", list(R.MODES))
def test_warp_gather_path_changes_inside_a_band(dev, mode):
    """DIRECT depth (dh = H: exact per-row control), rows cycling through the LDS, global-tap and float paths with bands of 3 and more
    rows (D2S_WARP_WPC=1, rows x tiles > 256 rpw), so that every path runs as a band's first, middle and last step behind every other:
    the hand-counted vmcnt waits must hold across the changes.  Asserted on the reference's float64 shifts: every row is in one class
    with >= 2 px of margin, every band holds a change, and all nine (class of row r, class of row r + 1) pairs occur inside bands."""
    m = MODE_NAME[mode]
    kw = dict(ipd_uv=0.064, ratio=2.0, conv=0.0)
    for (B, H, W, want_rpw) in ((2, 386, 84, 4), (2, 86, 580, 4 if mode == "Half-TAB" else 3)):   # 772 rows x 1 tile; 172 rows x 3 tiles
        L, G_, F = 0, 1, 2
        val = {L: (12.0, -20.5, 30.25, -8.0), G_: (70.0, -(W - 10.0), 75.5, -66.0), F: (W + 20.0, -(W + 9.0), 2.0 * W, -(3.0 * W + 0.5))}
        # periods 7 and 11 are coprime with the band lengths: every band starts at another phase
        pat = [[L, G_, F, L, F, G_, G_], [L, L, F, F, G_, L, G_, F, G_, G_, F]]
        cls = np.array([[pat[b][y % len(pat[b])] for y in range(H)] for b in range(B)])
        rows = np.array([[val[cls[b, y]][(y // 3) % 4] for y in range(H)] for b in range(B)])
        dep = R.depth_for_shift(rows, W, **kw)
        ref, plan = run_warp(dev, R.naming_u8(B, H, W), "U8_HWC", dep, "U8_HWC", mode, wpc=1, expect_rpw=want_rpw,
                             expect=f"stereo_warp_gather<{m},NC=4,DIRECT=1>", **kw)
        s = np.abs(ref["shift"])
        lds, glb, flt = s.max(axis=2) <= 61, (s.min(axis=2) >= 65) & (s.max(axis=2) <= W - 3), s.min(axis=2) >= W + 1
        got = np.where(lds, L, np.where(glb, G_, F)).reshape(-1)
        assert (lds | glb | flt).all() and (got == cls.reshape(-1)).all()
        rpw, pairs = plan["rpw"], set()
        for r0 in range(0, B * H, rpw):
            band = got[r0:r0 + rpw]
            assert len(band) < 2 or len(set(band.tolist())) > 1 or r0 + rpw > B * H - rpw, (r0, band)
            pairs |= set(zip(band[:-1].tolist(), band[1:].tolist()))
        assert pairs == {(a, b) for a in (L, G_, F) for b in (L, G_, F)}, pairs
