"""CPU: the float64 references, bounds and judges of the small model-side kernel tests (vit_ref.py) hold what they should and nothing more.
  * float32 numpy emulations of bilinear_nhwc_kernel, head_final_kernel, patchify_kernel, amax_kernel and to_f32_kernel pass EVERY check
    of test_gpu_vit_ops.py on its own case tables (its check functions are called here on the emulation's output), and the worst
    err / delta of the two bounded kernels lies in (0.02, 1]: the bounds are of the size of float32 noise, not orders above it;
  * each of sixteen deliberate errors is rejected on a named case;
  * d2s_vit_probe refuses malformed calls on the host: the pointers here are host memory and are never dereferenced."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import test_gpu_vit_ops as G
import vit_ref as R
from desktop2stereo_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from desktop2stereo_amd import build
        build.build()
    return _lib.load()


def stored_bits(v, bf):
    return R.to_bf16_bits(v) if bf else v


# ------------------------------------------------------------------------------------------------ emulations pass every check
def test_upsample_emulation_passes_on_the_gpu_cases():
    from test_gpu_conv3 import ups_operand_f32
    worst = {p: 0.0 for p in G.PRECS}
    for cs in G.UPS_CASES:
        shape, prec = cs
        sid, Hi, Wi, Ho, Wo, _ = shape
        bf = prec == "bf16"
        rng = np.random.default_rng(21000 + G.UPS_CASES.index(cs))
        for Cn, add in G.ups_variants(shape, prec):
            assert Cn % G.CHUNK[prec] == 0 and Ho <= 65535
            x, addend = R.upsample_inputs(rng, G.UPS_B, Hi, Wi, Ho, Wo, Cn, bf)
            em = R.upsample_emulate(x, Ho, Wo, addend if add else None, bf16=bf)
            if not add:                                            # the emulation here IS test_gpu_conv3's operand model
                assert R.same_bits(R.upsample_emulate(x, Ho, Wo), ups_operand_f32(torch.from_numpy(x), Ho, Wo).numpy()), (sid, prec)
            worst[prec] = max(worst[prec], G.ups_check(shape, prec, Cn, add, x, addend, em, stored_bits(em, bf)))
    print("[vit cpu] up-sample emulation worst err / delta:", worst)
    assert all(0.02 < v <= 0.45 for v in worst.values()), worst
    # what the table is meant to reach
    s = {c[0]: c for c in G.UPS_SHAPES}
    for prec in G.PRECS:
        chunks = s["ragged-x-blocks"][4] * s["ragged-x-blocks"][5] // G.CHUNK[prec]
        assert chunks > 256 and chunks % 256                       # several x-blocks, the last one ragged
    assert s["last-grid-y"][3] == 65535 and s["scale-1"][1:3] == s["scale-1"][3:5] and s["one-row-source"][1] == 1
    assert torch.equal(torch.from_numpy(R.bf16q(np.float32([1.00390625, 1.01171875, -3.0e38]))),
                       torch.tensor([1.00390625, 1.01171875, -3.0e38]).to(torch.bfloat16).float())
    v = np.float32([1.00390625, 1.01171875, 0.3, -7.7e-5])         # the two bf16 roundings agree (ties to even)
    assert np.array_equal(R.bf16q(v).astype(np.float64), R.rne_bf16(v.astype(np.float64)))


def test_head_emulation_passes_on_the_gpu_cases():
    worst = 0.0
    for cs in G.HEAD_CASES:
        Cn, prec = cs
        rng = np.random.default_rng(22000 + G.HEAD_CASES.index(cs))
        for npix in G.HEAD_NPIX:
            x, w3, b3 = R.head_inputs(rng, npix, Cn, prec == "bf16")
            assert (x >= 0).all()
            for md in G.HEAD_DEPTH:
                worst = max(worst, G.head_check((cs, npix, md), x, w3, b3, md, R.head_ref(x, w3, b3, md, dt=np.float32)))
    print("[vit cpu] head tail emulation worst err / delta:", worst)
    assert 0.02 < worst <= 1.0


def _patch_buffers(cs, bf):
    cid, B, gh, gw, p, Kp, D = cs
    x, cls, pos, N = G.patch_inputs(cs)
    A0 = np.full((B * gh * gw, Kp), 0x7f7f, np.uint16) if bf else np.full((B * gh * gw, Kp), 0x7f7f7f7f, np.uint32).view(np.float32)
    resid0 = np.full((B, N, D), 0x7f7f7f7f, np.uint32).view(np.float32)
    return x, cls, pos, N, A0, resid0


def test_patchify_emulation_passes_on_the_gpu_cases():
    for cs in G.PATCH_CASES:
        cid, B, gh, gw, p, Kp, D = cs
        assert Kp >= 3 * p * p and (Kp == 3 * p * p) == (cid == "no-padding")
        for prec in G.PRECS:
            bf = prec == "bf16"
            x, cls, pos, N, A0, resid0 = _patch_buffers(cs, bf)
            assert pos.size > D
            for with_cls in (True, False):
                A, resid = R.patchify_emulate(x, p, Kp, bf, A0, resid0, cls if with_cls else None, pos)
                G.patch_check(cs, prec, with_cls, x, cls, pos, resid0, A, resid)


def test_amax_and_to_f32_emulations_pass_on_the_gpu_cases():
    for n in G.AMAX_N[:-1] + (2048 * 8 + 77,):
        rng = np.random.default_rng(24000 + n % 1000)
        cases = G.amax_cases(n)
        assert {c[2] for c in cases} == set(G.AMAX_SLOTS) and (n < 2 or {c[1] for c in cases} == {False, True})
        assert {0, n - 1, n // 2} <= {c[0] for c in cases}
        for bf in (True, False):
            for pos, neg, slot in cases:
                x = R.amax_inputs(rng, n, pos, neg, bf)
                # the kernel's own decomposition: per thread over the capped grid-stride loop, then the maximum of all threads
                stride = R.amax_blocks(n) * 256
                m = max(float(np.abs(x[t::stride]).max()) for t in range(min(stride, n)))
                assert np.float32(max(slot, m)) == R.amax_expected(x, slot) == np.float32(max(slot, 3.0))
    n = G.AMAX_N[-1]
    assert R.amax_blocks(n) == 1024 and n - 1 >= 1024 * 256 and len(R.amax_positions(n)) == 4
    assert R.amax_positions(2048) == [0, 255, 1024, 2047] and R.amax_positions(255) == [0, 127, 254]
    for n in G.TOF_N:
        b = R.to_f32_inputs(np.random.default_rng(25000), n, True)
        want = torch.from_numpy(b.view(np.int16)).view(torch.bfloat16).float().numpy()
        assert R.same_bits(R.to_f32_expected(b, True), want)
        f = R.to_f32_inputs(np.random.default_rng(25000), n, False)
        assert np.isfinite(f).all() and R.same_bits(R.to_f32_expected(f, False), f)
    b = R.to_f32_inputs(np.random.default_rng(25000), 255, True)
    assert {0x0000, 0x8000, 0x7f7f, 0xff7f} <= set(b.tolist()) and len({v >> 7 & 0xff for v in b.tolist()}) > 20 and ((b & 0x7f80) != 0x7f80).all()


# ------------------------------------------------------------------------------------------------ the device tests, on the emulations
def _emulated_vit_probe(op, precision, x, out, *, B=0, h=0, w=0, p=0, Kp=0, N=0, D=0, Hi=0, Wi=0, Ho=0, Wo=0, channels=0, n=0, b3=0.0,
                        max_depth=0.0, addend=None, w3=None, cls=None, pos=None, resid=None):
    """ops.vit_probe with the launch replaced by the emulations of vit_ref.py, on host tensors, written in place"""
    bf = precision == "bf16"
    f = lambda t: None if t is None else t.float().numpy()
    if op == "bilinear":
        em = R.upsample_emulate(f(x).reshape(B, Hi, Wi, channels), Ho, Wo, f(addend), bf16=bf)
        out.copy_(torch.from_numpy(em).to(out.dtype))
    elif op == "head_final":
        out.copy_(torch.from_numpy(R.head_ref(f(x).reshape(n, channels), f(w3), np.float32(b3), max_depth, dt=np.float32)))
    elif op == "patchify":
        A, r = R.patchify_emulate(f(x), p, Kp, bf, G.raw(out), None if resid is None else resid.numpy(), f(cls), f(pos))
        out.copy_(torch.from_numpy(A.view(np.int16)).view(torch.bfloat16) if bf else torch.from_numpy(A))
        if cls is not None:
            resid.copy_(torch.from_numpy(r))
    elif op == "amax":
        out[0] = float(R.amax_expected(f(x)[:n], float(out[0])))
    elif op == "to_f32":
        out.copy_(x[:n].float())
    return f"{dict(bilinear='bilinear_nhwc', head_final='head_final', patchify='patchify', amax='amax', to_f32='to_f32')[op]}_kernel<{G.T_OF[precision]}>"


def test_device_tests_pass_on_the_emulations(monkeypatch):
    """Every device test of test_gpu_vit_ops.py but the refusals, run here with the launch replaced by the emulations: the case builders,
    the guards, the second run and the name table are checked too."""
    from desktop2stereo_amd import ops
    monkeypatch.setattr(ops, "vit_probe", _emulated_vit_probe)
    monkeypatch.setattr(G, "SEEN", set())
    monkeypatch.setattr(G, "WORST", {})
    cpu = torch.device("cpu")
    for cs in G.UPS_CASES:
        G.test_upsample_against_float64(cpu, cs)
    for cs in G.HEAD_CASES:
        G.test_head_final_against_float64(cpu, cs)
    for cs in G.PATCH_CASES:
        G.test_patchify_bit_for_bit(cpu, cs)
    for n in G.AMAX_N:
        G.test_amax_bit_for_bit(cpu, n)
    for prec in G.PRECS:
        G.test_to_f32_bit_for_bit(cpu, prec)
    G.test_every_kernel_name_was_produced(cpu)
    G.test_worst_ratios_are_reported(cpu)
    assert 0.02 < G.WORST["bilinear_nhwc_kernel<f32>"] <= 0.45 and 0.02 < G.WORST["head_final_kernel<f32>"] <= 1.0


# ------------------------------------------------------------------------------------------------ deliberate errors are rejected
def _ups_rejects(mut, sid, prec, add=True, wide=True):
    shape = next(s for s in G.UPS_SHAPES if s[0] == sid)
    _, Hi, Wi, Ho, Wo, Cw = shape
    bf = prec == "bf16"
    Cn = Cw if (wide and Cw) else G.CHUNK[prec]
    x, addend = R.upsample_inputs(np.random.default_rng(7), G.UPS_B, Hi, Wi, Ho, Wo, Cn, bf)
    good = R.upsample_emulate(x, Ho, Wo, addend if add else None, bf16=bf)
    G.ups_check(shape, prec, Cn, add, x, addend, good, stored_bits(good, bf))
    bad = R.upsample_emulate(x, Ho, Wo, addend if add else None, bf16=bf, mut=mut)
    try:
        G.ups_check(shape, prec, Cn, add, x, addend, bad, stored_bits(bad, bf))
    except AssertionError:
        return True
    return False


def _ups_rejected_by_the_bound(mut, sid, prec):
    """the float64 bound alone (not the bit-for-bit model) rejects the error"""
    shape = next(s for s in G.UPS_SHAPES if s[0] == sid)
    _, Hi, Wi, Ho, Wo, Cw = shape
    bf = prec == "bf16"
    x, addend = R.upsample_inputs(np.random.default_rng(7), G.UPS_B, Hi, Wi, Ho, Wo, Cw or G.CHUNK[prec], bf)
    ref, delta = R.upsample_ref(x, Ho, Wo, addend)
    return not R.upsample_judge(R.upsample_emulate(x, Ho, Wo, addend, bf16=bf, mut=mut), ref, delta, bf)[0].all()


def test_deliberate_upsample_errors_are_rejected():
    for prec in G.PRECS:
        assert _ups_rejected_by_the_bound("align_corners_false", "fusion-x2", prec)
        assert _ups_rejected_by_the_bound("swap_xy", "non-integer-scale", prec)
        assert _ups_rejected_by_the_bound("no_addend", "head-interpolate", prec)
        assert _ups_rejects("align_corners_false", "one-row-source", prec, add=False)
    assert _ups_rejected_by_the_bound("trunc", "ragged-x-blocks", "bf16")
    assert _ups_rejected_by_the_bound("round_before_add", "fusion-x2", "bf16")
    assert _ups_rejects("round_before_add", "non-integer-scale", "bf16")


def test_deliberate_head_errors_are_rejected():
    for prec in G.PRECS:
        x, w3, b3 = R.head_inputs(np.random.default_rng(8), 257, 64, prec == "bf16")

        def rejected(mut, md):
            ref, delta, _ = R.head_ref(x, w3, b3, md)
            assert R.judge_float(R.head_ref(x, w3, b3, md, dt=np.float32), ref, delta)[0].all()
            return not R.judge_float(R.head_ref(x, w3, b3, md, dt=np.float32, mut=mut), ref, delta)[0].all()
        assert rejected("relu_metric", 20.0) and rejected("no_max_depth", 20.0) and rejected("no_max_depth", 80.0)
        for md in G.HEAD_DEPTH:
            assert rejected("no_bias", md) and rejected("short", md)


def test_deliberate_patchify_errors_are_rejected():
    by = {c[0]: c for c in G.PATCH_CASES}

    def rejected(mut, cid, prec, with_cls=True):
        cs = by[cid]
        _, B, gh, gw, p, Kp, D = cs
        bf = prec == "bf16"
        x, cls, pos, N, A0, resid0 = _patch_buffers(cs, bf)
        A, resid = R.patchify_emulate(x, p, Kp, bf, A0, resid0, cls if with_cls else None, pos, mut=mut)
        try:
            G.patch_check(cs, prec, with_cls, x, cls, pos, resid0, A, resid)
        except AssertionError:
            return True
        return False
    for prec in G.PRECS:
        assert rejected("perm_cij", "ordinary", prec) and rejected("perm_cij", "wide-padding", prec, with_cls=False)
        assert rejected("pad_unwritten", "wide-padding", prec) and rejected("pad_unwritten", "ordinary", prec)
        assert not rejected("pad_unwritten", "no-padding", prec)   # (nothing to pad there: the case is about Kp = 3 p^2 itself)
        assert rejected("pos_row1", "ordinary", prec) and rejected("pos_row1", "grid-by-cls-rows-B1", prec)
        assert rejected("cls_frame0_only", "grid-by-cls-rows-B2", prec) and rejected("cls_frame0_only", "ordinary", prec)
        assert not rejected(None, "ordinary", prec)


def test_deliberate_amax_errors_are_rejected():
    rng = np.random.default_rng(9)
    for bf in (True, False):
        x = R.amax_inputs(rng, 2049, 2048, True, bf)               # the planted element is negative and the last one, behind 8 full sweeps
        assert R.amax_expected(x, 0.0) == np.float32(3.0)
        assert R.amax_expected(x, 0.0, mut="no_abs") != np.float32(3.0)
        assert R.amax_expected(x, 0.0, mut="skip_tail") != np.float32(3.0)
        assert R.amax_expected(x, 5.0) == np.float32(5.0) and R.amax_expected(x, 5.0, mut="overwrite") != np.float32(5.0)
        x = R.amax_inputs(rng, G.AMAX_N[-1], G.AMAX_N[-1] - 1, False, bf)
        assert R.amax_expected(x, 2.0, mut="skip_tail") != np.float32(3.0) and R.amax_expected(x, 2.0) == np.float32(3.0)


# ------------------------------------------------------------------------------------------------ the probe refuses on the host
def _params(kw):
    """keyword arguments of ops.vit_probe, with numpy arrays as buffers -> d2s_vit_probe_params"""
    q = _lib.VitProbeParams()
    q.struct_size = C.sizeof(_lib.VitProbeParams)
    q.op = _lib.VIT_OPS[kw["op"]]
    q.precision = {"bf16": _lib.PREC_BF16, "fp32": _lib.PREC_FP32}[kw["precision"]]
    for k in ("B", "h", "w", "p", "Kp", "N", "D", "Hi", "Wi", "Ho", "Wo", "n"):
        setattr(q, k, int(kw.get(k, 0)))
    q.C, q.b3, q.max_depth = int(kw.get("channels", 0)), float(kw.get("b3", 0.0)), float(kw.get("max_depth", 0.0))
    for k in ("x", "out", "addend", "w3", "cls", "pos", "resid"):
        t = kw.get(k)
        if t is not None:
            setattr(q, k, t.ctypes.data)
            setattr(q, k + "_elems", t.size)
    return q


def test_probe_refuses_malformed_cases_on_the_host(lib):
    keep = []

    def mk(n, off=0):
        whole = np.zeros(n + 16, np.float32)
        base = (-whole.ctypes.data % 16) // 4                       # a 16-byte aligned start, then the stated offset
        keep.append(whole)
        return whole[base + off // 4:base + off // 4 + n]
    good = {k: mk(n) for k, n in G.REFUSED_GOOD.items()}
    cases = G.refused_cases(mk, good)
    assert len(cases) >= 25
    for label, kw in cases:
        q = _params(kw)
        assert lib.d2s_vit_probe(C.byref(q), None) == 1 and lib.d2s_last_error() and q.kernel == b"", label      # D2S_E_INVALID
    up = dict(op="bilinear", precision="fp32", x=good["in"], out=good["out"], B=1, Hi=2, Wi=2, Ho=3, Wo=3, channels=4)
    q = _params(up)
    q.struct_size -= 8
    assert lib.d2s_vit_probe(C.byref(q), None) == 1 and b"struct_size" in lib.d2s_last_error()
    q = _params(up)
    q.op = 5
    assert lib.d2s_vit_probe(C.byref(q), None) == 1 and b"unknown op" in lib.d2s_last_error()
    q = _params(up)
    q.precision = _lib.PREC_FP8
    assert lib.d2s_vit_probe(C.byref(q), None) == 1 and b"precision" in lib.d2s_last_error()
    assert lib.d2s_vit_probe(None, None) == 1
    # the launcher's own refusals, behind the probe's checks and still before any launch: the stated shape fits the buffers
    big = mk(65536 * 4)
    q = _params({**up, "channels": 6, "x": mk(2 * 2 * 6), "out": mk(3 * 3 * 6)})
    assert lib.d2s_vit_probe(C.byref(q), None) == 1 and b"chunk" in lib.d2s_last_error()
    q = _params({**up, "Hi": 2, "Wi": 1, "Ho": 65536, "Wo": 1, "out": big})
    assert lib.d2s_vit_probe(C.byref(q), None) == 5 and q.kernel == b""                                         # D2S_E_UNSUPPORTED
    assert all(not w.any() for w in keep)
