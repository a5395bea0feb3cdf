"""GPU: the DIBR warp (dibr.hip: the gather kernels, the LDS-window row kernels at 256, 512 and 1 024 columns, UpDep, the cropped
kernels) per value against the float64 reference of tests/dibr_ref.py -- no fraction-of-pixels allowance: every colour and alpha value
must lie in the interval the reference derives for it (under one of at most four outcome combinations where a hard comparison of the
shader is undecided in float32; see dibr_ref.py's docstring), a handful of exempt pixels per case aside, which must still be finite and
in range.  Every case goes through ops.dibr_warp with float32 and u8 output and the three alpha modes, writes between 0x7f guard
regions that must stay intact, runs twice and must be bit-identical, and first asserts through ops.dibr_warp_plan the kernel, cols and
rows it was built for -- under the default switches and under each D2S_DIBR_* switch the case names.  Colours are uint8 noise (smooth
in one case), depth is smooth with hard-edged boxes inside the image and on its edges.  test_cpu_dibr_ref.py shows on the host that the
reference meets its own condition on every case here, that float32 emulations pass and that twenty-one deliberate errors do not.

Measured worst |got - mid| / half-width per kernel and the per-case class counts: DESIGN.md (float64 references, DIBR warp)."""

import numpy as np
import pytest
import torch

import dibr_ref as R

pytestmark = pytest.mark.gpu
GUARD = 256
KEYS = ("D2S_DIBR_NO_ROLL0", "D2S_DIBR_NO_ROWS", "D2S_DIBR_COLS")
WORST = {}
_REF = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture()
def switches(monkeypatch):
    from desktop2stereo_amd import ops

    def set_env(spec=None):
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        if spec:
            k, v = spec.split("=")
            monkeypatch.setenv(k, v)
        ops.reload_env()
    set_env()
    yield set_env
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    ops.reload_env()


def guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(0x7f)
    return buf, buf[GUARD:GUARD + n].view(tuple(shape))


def guards_intact(buf):
    raw, gb = buf.view(torch.uint8), GUARD * buf.element_size()
    return bool((raw[:gb] == 0x7f).all()) and bool((raw[-gb:] == 0x7f).all())


def run_twice(ops, f, d, dp, u8, crop, shape, dev):
    """ops.dibr_warp into a guarded buffer, twice: bit-identical, guards intact -> the result"""
    buf, view = guarded(shape, torch.uint8 if u8 else torch.float32, dev)
    ops.dibr_warp(f, d, dp, out_u8=u8, crop=crop, out=view)
    torch.cuda.synchronize()
    first = buf.clone()
    buf.view(torch.uint8).fill_(0x7f)
    ops.dibr_warp(f, d, dp, out_u8=u8, crop=crop, out=view)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.uint8), buf.view(torch.uint8)), "not bit-identical on a second run"
    assert guards_intact(buf), "guard bytes overwritten"
    return view.cpu().numpy()


@pytest.mark.parametrize("name", list(R.CASES))
def test_dibr_warp_vs_float64(dev, switches, name):
    from desktop2stereo_amd import ops
    c = R.CASES[name]
    if name not in _REF:
        rgb, dep = R.inputs(c)
        _REF[name] = (rgb, dep, R.reference(c, rgb, dep))
    rgb, dep, ref = _REF[name]
    f, d = torch.from_numpy(rgb).to(dev), torch.from_numpy(dep).to(dev)
    B, (dh, dw) = c["batch"], c["dhw"]

    def params(alpha):
        return ops.dibr_params(display_mode=c["mode"], alpha=alpha, **c["kw"])

    def plan(u8=True):
        return ops.dibr_warp_plan(dh, dw, B, c["H"], c["W"], params("window"), out_u8=u8, crop=c["crop"])
    kernel, rows, cols = c["expect"]
    for spec, want, variants in [(None, kernel, [(a, u) for a in ("window", "premultiplied", "rgba") for u in (False, True)])] + \
                                [(s, k, [("rgba", False), ("premultiplied", True)]) for s, k in c["env"].items()]:
        switches(spec)
        pl = plan()
        assert pl["kernel"] == want, (name, spec, pl)
        if spec is None:
            assert (pl["rows"], pl["cols"]) == (rows, cols), (name, pl)
        assert plan(False)["kernel"] == want.replace("<u8", "<f32"), (name, spec)
        assert pl["lds_bytes"] <= 65536
        for alpha, u8 in variants:
            nch = 4 if alpha == "rgba" else 3
            got = run_twice(ops, f, d, params(alpha), u8, c["crop"], (B, pl["out_h"], pl["out_w"], nch), dev)
            j = R.judge(ref, got, alpha, u8)
            kn = want if u8 else want.replace("<u8", "<f32")
            if not u8:
                w = WORST.setdefault(kn, [0.0, 0.0, 0.0])
                WORST[kn] = [max(w[0], j["p50"]), max(w[1], j["p99"]), max(w[2], j["worst"])]
            print(f"[dibr f64, {name}, {spec or 'default'}, {kn}, {alpha}] decided {j['decided']}, branch-judged {j['branch']}, exempt {j['exempt']} "
                  f"of {j['n']}; |got - mid| / half-width median {j['p50']:.3f}, 99 % {j['p99']:.3f}, worst {j['worst']:.3f}; rejected {j['nbad']}")
            assert j["ok"], (name, spec, alpha, u8, j["nbad"], j["bad"])
            assert R.condition(j), (name, j)


def test_report_worst_per_kernel():
    """(prints what the cases above measured; DESIGN.md quotes it)"""
    for k in sorted(WORST):
        print(f"[dibr f64 worst] {k}: median {WORST[k][0]:.3f}, 99 % {WORST[k][1]:.3f}, worst {WORST[k][2]:.3f} (largest over its cases)")
