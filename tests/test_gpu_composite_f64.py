"""GPU: the composite display modes (dibr_composite.hip: comp_rows_kernel at 256 and 512 columns, with and without the feather / corner
code, FullDep and UpDep; comp_kernel at roll 0 and with a roll; depth_map_kernel with vector and scalar stores) per value against the
float64 reference of tests/composite_f64_ref.py -- no fraction-of-pixels allowance: every colour and alpha value must lie in the interval
the reference derives for it (under one of at most four outcome combinations where a hard comparison of the shader is undecided in
float32), a handful of exempt pixels per case aside, which must still be finite and in range.  Every case first asserts through
ops.dibr_composite_plan the kernel, rows, cols and LDS it was built for, then goes through ops.dibr_composite with float32 and u8
output and the three alpha modes, writes between 0x7f guard regions that must stay intact, runs twice and must be bit-identical.
The Depth Map runs each variant at an aligned output address (vector stores) and at one offset by one element (scalar stores): the
plan names the difference, the results have equal bits.  test_cpu_composite_f64.py shows on the host that the reference meets its own
condition on every case here, that float32 emulations pass and that twenty-four deliberate errors do not.

Measured worst |got - mid| / half-width per kernel: DESIGN.md (float64 references, composite modes)."""

import numpy as np
import pytest
import torch

import composite_f64_ref as Q
import dibr_ref as R

pytestmark = pytest.mark.gpu
GUARD = 256
WORST = {}
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def guarded(shape, dtype, dev, shift=0):
    """a view of `shape` between two 0x7f guard regions, `shift` elements past an aligned address"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(0x7f)
    return buf, buf[GUARD + shift:GUARD + shift + n].view(tuple(shape))


def guards_intact(buf, n, shift=0):
    raw, es = buf.view(torch.uint8), buf.element_size()
    return bool((raw[:(GUARD + shift) * es] == 0x7f).all()) and bool((raw[(GUARD + shift + n) * es:] == 0x7f).all())


def run_twice(ops, f, d, dp, mode, u8, size, shape, dev, shift=0):
    """ops.dibr_composite into a guarded buffer, twice: bit-identical, guards intact -> the result and its address modulo 16"""
    buf, view = guarded(shape, torch.uint8 if u8 else torch.float32, dev, shift)
    ops.dibr_composite(f, d, dp, mode, out_u8=u8, size=size, out=view)
    torch.cuda.synchronize()
    first = buf.clone()
    buf.view(torch.uint8).fill_(0x7f)
    ops.dibr_composite(f, d, dp, mode, out_u8=u8, size=size, out=view)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.uint8), buf.view(torch.uint8)), "not bit-identical on a second run"
    assert guards_intact(buf, view.numel(), shift), "guard bytes overwritten"
    return view.cpu().numpy(), view.data_ptr() % 16


def ref_of(c, mode):
    if (c["name"], mode) not in _REF:
        if c["name"] not in _REF:
            _REF[c["name"]] = Q.case_inputs(c)
        rgb, dep = _REF[c["name"]]
        _REF[c["name"], mode] = (rgb, dep, Q.reference(c, mode, rgb, dep))
    return _REF[c["name"], mode]


def record(kn, j, what):
    if np.isfinite(j["worst"]):
        w = WORST.setdefault(kn, [0.0, 0.0, 0.0])
        WORST[kn] = [max(w[0], j["p50"]), max(w[1], j["p99"]), max(w[2], j["worst"])]
    print(f"[composite f64, {what}, {kn}] decided {j['decided']}, branch-judged {j['branch']}, exempt {j['exempt']} of {j['n']}; "
          f"|got - mid| / half-width median {j['p50']:.3f}, 99 % {j['p99']:.3f}, worst {j['worst']:.3f}; rejected {j['nbad']}")


@pytest.mark.parametrize("name,mode", [(n, m) for n, c in Q.CASES.items() for m in c["modes"]])
def test_composite_vs_float64(dev, name, mode):
    from desktop2stereo_amd import ops
    c = Q.CASES[name]
    rgb, dep, ref = ref_of(c, mode)
    f, d = torch.from_numpy(rgb).to(dev), torch.from_numpy(dep).to(dev)
    B, (dh, dw) = c["batch"], c["dhw"]
    kind, cols = c["expect"]
    for u8 in (False, True):
        pl = ops.dibr_composite_plan(dh, dw, B, c["H"], c["W"], ops.dibr_params(**c["kw"]), mode, out_u8=u8)
        kn = Q.kernel_name(c, mode, u8)
        assert pl["kernel"] == kn, (name, mode, pl)
        assert pl["rows"] == (kind == "rows") and (not pl["rows"] or pl["cols"] == cols), (name, mode, pl)
        assert pl["lds_bytes"] <= 65536 and (pl["lds_bytes"] > 0) == pl["rows"], pl
        for alpha in ("window", "premultiplied", "rgba"):
            nch = 4 if alpha == "rgba" else 3
            got, _ = run_twice(ops, f, d, ops.dibr_params(alpha=alpha, **c["kw"]), mode, u8, (c["H"], c["W"]), (B, pl["out_h"], pl["out_w"], nch), dev)
            j = R.judge(ref, got, alpha, u8)
            record(kn, j, f"{name}, {alpha}")
            assert j["ok"], (name, mode, alpha, u8, j["nbad"], j["bad"])
            assert R.condition(j), (name, mode, j)


@pytest.mark.parametrize("name", list(Q.DM_CASES))
def test_depth_map_vs_float64(dev, name):
    from desktop2stereo_amd import ops
    c = Q.DM_CASES[name]
    rgb, dep, ref = ref_of(c, "Depth Map")
    d = torch.from_numpy(dep).to(dev)
    B, (dh, dw) = c["batch"], c["dhw"]
    for u8 in (False, True):
        for alpha, nch in (("window", 3), ("rgba", 4)):
            dp = ops.dibr_params(alpha=alpha, **c["kw"])
            outs = []
            for shift, vec in ((0, True), (1, False)):            # one element = 1 or 4 bytes past a 16-byte boundary: scalar stores
                pl0 = ops.dibr_composite_plan(dh, dw, B, c["H"], c["W"], dp, "Depth Map", out_u8=u8)
                got, align = run_twice(ops, None, d, dp, "Depth Map", u8, (c["H"], c["W"]), (B, pl0["out_h"], pl0["out_w"], nch), dev, shift)
                pl = ops.dibr_composite_plan(dh, dw, B, c["H"], c["W"], dp, "Depth Map", out_u8=u8, out_align=align)
                kn = Q.dm_kernel_name(c, u8, nch, vec)
                assert (align == 0) == vec and pl["kernel"] == kn and pl["vec"] == vec and pl["lds_bytes"] == 0, (name, shift, align, pl)
                j = R.judge(ref, got, alpha, u8)
                record(kn, j, f"{name}, {alpha}")
                assert j["ok"], (name, alpha, u8, vec, j["nbad"], j["bad"])
                assert R.condition(j), (name, j)
                outs.append(got)
            assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8)), (name, alpha, u8, "vector and scalar stores differ")


def test_report_worst_per_kernel():
    """(prints what the cases above measured; DESIGN.md quotes it)"""
    for k in sorted(WORST):
        print(f"[composite f64 worst] {k}: median {WORST[k][0]:.3f}, 99 % {WORST[k][1]:.3f}, worst {WORST[k][2]:.3f} (largest over its cases)")
