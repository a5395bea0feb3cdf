"""The temporal-module kernels (temporal.hip) and layernorm_kernel (vit_ops.hip) against float64, through d2s_temporal_probe: the
launchers run_temporal and the encoder call, on operands that are already in the kernel's storage type (so the float64 reference
starts from the very numbers the kernel reads), every output between guard regions of 0x7f bytes.  Per element, nothing sampled.
For every case: the kernel name is the expected one, the guards are intact, nothing is NaN or inf, a second run is bit-identical.
References, bounds and input families live in temporal_ref.py; test_cpu_temporal_ref.py shows on the host that a faithful float32
emulation passes these judges and that ten deliberate errors do not.

Dispatch (every name is in TABLE; a case names the one it expects):
  plan_groupnorm      groupnorm_reg_kernel<T,CPG,RPT> for CPG = C / 32 in {2, 4, 6, 8, 12, 16, 24, 32}, RPT = 1 (sites <= 1024), 2 (<= 2048),
                      4 (<= 4096, CPG <= 24 only); else, and with D2S_GN_OLD=1, groupnorm_kernel<T>
  plan_temporal_attn  temporal_attn_kernel<T,CH,Win>: CH = 8 when the head dimension C / 8 is a multiple of 8, else 4; WinRow for one
                      row, WinTable for several
  layernorm_kernel<f32 | bf16 | bx3 | e4m3>, geglu_kernel<T>, cast_f32_kernel<T>, cache_store_rows_kernel<T>     (T = bf16 | f32)

Bounds (u = 2^-24; bf16 / e4m3 outputs: got inside [RNE(ref - delta), RNE(ref + delta)] of the format, fp32: |got - ref| <= delta,
bf16x3 units: delta + 2^-17 |ref|, the format's own resolution).

GroupNorm / LayerNorm.  Reference: float64 mean and biased variance of one (row, group) / one row, eps the float32 passed in.
  The kernels are two-pass in fp32.  A block sum passes an element through d additions: the thread's own run, 6 xor-shuffle levels, the
  per-wave partials -- d = RPT CPG + 6 + 16 (register kernel), ceil(n / 256) + 6 + 4 (general kernel), 4 x 3 + 6 (layernorm: four
  float4 per lane, (x + y) + (z + w) added to the running sum).  So
    |mean^ - mean| <= e_mu = (d + 1) u mean|x|                                  (the sum, then the division),
    the sum of squared deviations, all terms positive, is off by a factor 1 +- (d + 3) u (deviation, square, sum) and by the
    second-order n (mean^ - mean)^2; / n and + eps are two more roundings, sqrtf and the division are held to 1 ulp = 2 u each:
    rstd^ = rstd (1 +- r),  r = ((d + 5) / 2 + 4) u + e_mu^2 / (2 (var + eps)),
    y = (x - mean^) rstd^ gamma + beta: three roundings on the product, one on the sum:
    delta = |gamma| rstd (e_mu + |x - mean| (r + 3 u)) + u |ref|.
  For a constant group this is |gamma| rstd e_mu with rstd = eps^-1/2 = 1000: the error of the mean, amplified.
  e4m3 output multiplies by qscale first: + u |ref|.
Temporal attention.  Reference per (row, site, head): q = cur_q + ptab[Tw-1][2C:], key / value j < Tw-1 from ring slot
  (head + j) mod 31 plus ptab[j][0:C] / ptab[j][C:2C], position Tw-1 from cur, out = softmax(q k / sqrt dh) v; x_j = s_j - max s.
  With w the weights, A = w |v|, T = max_j sum_d |q_d k_jd| / sqrt dh:   delta = (rS T + rF + 2 u X) A + 2 u Ax,
    rS = 2 (CH + log2 lpu + 7) u: a score is CH products summed in the lane and log2 lpu shuffle levels, on q and k that carry one
         rounding each (the table row added), times the fp32 1 / sqrtf(dh) (2 u against the exact one) in one more rounding, minus
         the maximum (|x_j| <= 2 T: 2 u T); an error e in every score moves numerator and denominator by e^e each: 2 e A;
    __expf(x) = v_exp_f32(x log2 e): the constant and the product put 2 u |x_j| on the result, the instruction 1 ulp = 2 u.  On the
         numerator that is 2 u Ax + 2 u A with Ax = w |x| |v|, on the denominator (2 X + 2) u with X = w |x| (both from the reference);
    rF = 28 u: besides those 2 + 2, v = ring + table (1), p = e / sum (1) and the sum of 8 terms per lane and 2 shuffle levels (10)
         on the numerator; the same sum (10) and the reciprocal (2) on the denominator.
  The rings afterwards are compared bit for bit: slot store_slot of a row's ring = cur's k | v rows, everything else -- other slots,
  other rows' rings, the guard slots around every ring -- unchanged.
GEGLU.  Reference x 0.5 gate (1 + erf(gate / sqrt 2)).  delta = 0.5 |x gate| (8 u |erf| + 2 u) + 4 u |ref|: erff is held to 4 ulp,
  its argument carries 2 u (constant and product: at most u on erf), 1 + erf rounds once -- an ABSOLUTE error of 1 + erf, which is
  all that is left of it where it cancels (gate << 0); the three products and the storage of 1 + erf are relative.
Cast and cache store are bit for bit.

Measured worst err / delta per kernel: DESIGN.md (float64 references, temporal modules)."""
import itertools
import os
from typing import Dict

import pytest
import torch

import temporal_ref as R

GPU = pytest.mark.gpu

T_OF = {"bf16": "bf16", "fp32": "f32"}
DT_OF = {"bf16": torch.bfloat16, "fp32": torch.float32}
REG_CPG = [2, 4, 6, 8, 12, 16, 24, 32]
GN_TABLE = [f"groupnorm_reg_kernel<{t},CPG={c},RPT={r}>" for t in ("bf16", "f32") for c in REG_CPG for r in (1, 2, 4) if not (c == 32 and r == 4)] \
    + ["groupnorm_kernel<bf16>", "groupnorm_kernel<f32>"]
TA_TABLE = [f"temporal_attn_kernel<{t},CH={ch},{w}>" for t in ("bf16", "f32") for ch in (4, 8) for w in ("WinRow", "WinTable")]
LN_TABLE = [f"layernorm_kernel<{t}>" for t in ("f32", "bf16", "bx3", "e4m3")]
EW_TABLE = [f"{k}<{t}>" for k in ("geglu_kernel", "cast_f32_kernel", "cache_store_rows_kernel") for t in ("bf16", "f32")]
TABLE = GN_TABLE + TA_TABLE + LN_TABLE + EW_TABLE

WORST: Dict[str, float] = {}
GUARD = 64                                      # guard elements on either side of an output (a multiple of 32 bytes in every type)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def guarded(shape, dtype, dev):
    """-> (whole buffer, the view of `shape` inside it), all bytes 0x7f"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(0x7f)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf) -> bool:
    raw = buf.view(torch.uint8)
    g = GUARD * buf.element_size()
    return bool((raw[:g] == 0x7f).all()) and bool((raw[-g:] == 0x7f).all())


def bits(t):
    return t.contiguous().view(torch.uint8)


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def twice(run, bufs):
    """run() twice on freshly 0x7f-filled buffers -> the first run's name; asserts the second run's name and bytes are the same"""
    name = run()
    first = [b.clone() for b in bufs]
    for b in bufs:
        b.view(torch.uint8).fill_(0x7f)
    assert run() == name
    for a, b in zip(first, bufs):
        assert torch.equal(bits(a), bits(b)), (name, "not bit-identical on a second run")
    return name


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from desktop2stereo_amd import ops
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
        ops.reload_env()

    def __exit__(self, *a):
        from desktop2stereo_amd import ops
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ops.reload_env()


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_expect(prec, sites, C, old=False):
    cpg = C // 32
    rpt = 1 if sites <= 1024 else (2 if sites <= 2048 else 4)
    if old or C % 32 or cpg not in REG_CPG or sites > 4096 or (rpt == 4 and cpg == 32):
        return f"groupnorm_kernel<{T_OF[prec]}>"
    return f"groupnorm_reg_kernel<{T_OF[prec]},CPG={cpg},RPT={rpt}>"


def gn_cases():
    cs = []          # (id, sites, C, old, expected fp32 name where it is a fall-back the issue names, else None)
    for sites in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096):
        for C in (256, 64):
            cs.append((f"sites{sites}-C{C}", sites, C, False, None))
    for cpg in REG_CPG:
        for sites in (37, 1025):
            cs.append((f"cpg{cpg}-sites{sites}", sites, 32 * cpg, False, None))
    for cpg in (24, 32):
        for sites in (2048, 2049):
            cs.append((f"rpt4rule-cpg{cpg}-sites{sites}", sites, 32 * cpg, False, "groupnorm_kernel<f32>" if (cpg, sites) == (32, 2049) else None))
    for cpg in (4, 6, 12, 16):                                  # (RPT 4 of the remaining CPG: every name of the table)
        cs.append((f"rpt4-cpg{cpg}-sites2049", 2049, 32 * cpg, False, None))
    cs.append(("fallback-cpg3", 37, 96, False, "groupnorm_kernel<f32>"))
    cs.append(("fallback-sites4097-C256", 4097, 256, False, "groupnorm_kernel<f32>"))
    cs.append(("fallback-sites4097-C64", 4097, 64, False, "groupnorm_kernel<f32>"))
    cs.append(("fallback-gn-old", 65, 256, True, "groupnorm_kernel<f32>"))
    return cs


GN_CASES = gn_cases()


@GPU
@pytest.mark.parametrize("cs", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_against_float64(dev, cs):
    from desktop2stereo_amd import ops
    cid, sites, C, old, fallback = cs
    rows = 1 + GN_CASES.index(cs) % 3
    cpg = C // 32
    g = torch.Generator(device=dev).manual_seed(9000 + GN_CASES.index(cs))
    eps = 1e-6
    for prec, fam in itertools.product(("bf16", "fp32"), ("G1", "G2", "G3", "G4")):
        expect = gn_expect(prec, sites, C, old)
        if fallback:
            assert expect == fallback.replace("f32", T_OF[prec])
        x = R.norm_family(fam, (rows, 32, sites, cpg), prec == "bf16", g, dev).permute(0, 2, 1, 3).reshape(rows, sites, C)
        x = x.to(DT_OF[prec]).contiguous()
        gamma = 1.0 + 0.5 * torch.randn(C, generator=g, device=dev)
        beta = torch.randn(C, generator=g, device=dev)
        ref, mu, var = R.groupnorm_compute(x, gamma, beta, eps, 32, torch.float64)
        reg = expect.startswith("groupnorm_reg")
        rpt = int(expect.split("RPT=")[1][0]) if reg else 0
        delta = R.groupnorm_delta(x, gamma, eps, 32, R.norm_depth_groupnorm(reg, cpg, rpt, sites), ref, mu, var)
        buf, out = guarded((rows, sites, C), DT_OF[prec], dev)
        with env(**({"D2S_GN_OLD": "1"} if old else {})):
            name = twice(lambda: ops.temporal_probe("groupnorm", prec, x, out, rows=rows, sites=sites, channels=C, groups=32, eps=eps,
                                                    gamma=gamma, beta=beta), [buf])
        tag = (cid, prec, fam, name)
        assert name == expect, (tag, "dispatch moved", expect)
        assert guards_intact(buf), (tag, "a guard was written")
        ok, ratio, got = R.judge(out, ref, delta, T_OF[prec])
        note(name, ratio)
        print(f"[temporal] {cid:28s} {prec} {fam} rows={rows} {name:44s} max_err/delta={ratio:.3f}")
        assert bool(torch.isfinite(got).all()), (tag, "NaN or inf")
        assert bool(ok.all()), (tag, "outside the bound", int((~ok).sum()), "of", ok.numel(), "worst", ratio, (~ok).nonzero()[:4].tolist())


# ------------------------------------------------------------------------------------------------ temporal attention
TA_C = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
TA_SITES = (1, 3, 8, 9, 37)
TA_HEADS = (0, 1, 15, 29, 30)
TA_ROWCFG = [("warm1", [32]), ("fresh1", [1]), ("rows2", [32, 1]), ("rows3", [1, 32, 32]), ("rows5", [32, 1, 32, 32, 1])]
TA_CASES = [(C, prec) for C in TA_C for prec in ("bf16", "fp32")]


def ta_expect(prec, C, rows):
    return f"temporal_attn_kernel<{T_OF[prec]},CH={8 if (C // 8) % 8 == 0 else 4},{'WinTable' if rows > 1 else 'WinRow'}>"


def ring_buffers(rings, dev):
    """every ring inside a buffer of 33 slots, slot 0 and slot 32 guards of 0x7f bytes -> (buffers, the [31, S, 2C] views)"""
    bufs, views = [], []
    for rg in rings:
        b = torch.empty((R.SLOTS + 2,) + tuple(rg.shape[1:]), dtype=rg.dtype, device=dev)
        b.view(torch.uint8).fill_(0x7f)
        b[1:R.SLOTS + 1] = rg
        bufs.append(b)
        views.append(b[1:R.SLOTS + 1])
    return bufs, views


def run_attn(dev, prec, C, S, Tw, fam, k):
    from desktop2stereo_amd import ops
    rows = len(Tw)
    head = [TA_HEADS[(k + 2 * r) % 5] for r in range(rows)]
    store = [head[r] if fam == "T4" or (r + k) % 2 == 0 else -1 for r in range(rows)]
    g = torch.Generator(device=dev).manual_seed(11000 + 131 * k + C)
    cur, rings, ptab, pi = R.tattn_family(fam, C, S, head, Tw, k, prec == "bf16", g, dev)
    ref, rings_ref, b = R.tattn_compute(cur, rings, ptab, head, Tw, store, torch.float64, bounds=True)
    tag = (prec, C, S, Tw, head, store, fam)
    if pi is not None and 32 in Tw:                  # asserted on the reference, before the kernel is judged
        wmin = R.tattn_target_weight(b, pi, Tw)
        assert wmin >= 0.99, (tag, "a target position's softmax weight is below 0.99", wmin)
    for r in range(rows):                            # T5: a fresh row is its own value row plus the table's row 0
        if Tw[r] == 1:
            fresh = cur[r, :, C:2 * C].double() + ptab[0, C:2 * C].double()
            assert float((ref[r] - fresh).abs().max()) <= 1e-12 * (1.0 + float(fresh.abs().max()))
    delta = R.tattn_delta(C, b)
    rbufs, rviews = ring_buffers(rings, dev)
    before = [rb.clone() for rb in rbufs]
    obuf, out = guarded((rows, S, C), DT_OF[prec], dev)

    def run():
        for rb, b0 in zip(rbufs, before):
            rb.copy_(b0)
        return ops.temporal_probe("temporal_attn", prec, cur, out, rows=rows, sites=S, channels=C, slots=R.SLOTS, ptab=ptab, rings=rviews,
                                  head=head, Tw=Tw, store_slot=store)
    name = twice(run, [obuf])
    after1 = [rb.clone() for rb in rbufs]
    assert name == ta_expect(prec, C, rows), (tag, "dispatch moved", name)
    assert guards_intact(obuf), (tag, "an output guard was written")
    for r in range(rows):
        want = before[r].clone()
        if store[r] >= 0:
            want[1 + store[r]] = cur[r, :, :2 * C]
        assert torch.equal(bits(after1[r]), bits(want)), (tag, "ring state of row", r, "differs from the expected one",
                                                          (bits(after1[r]) != bits(want)).view(R.SLOTS + 2, -1).any(-1).nonzero().flatten().tolist())
    run()
    for r in range(rows):
        assert torch.equal(bits(rbufs[r]), bits(after1[r])), (tag, "rings not bit-identical on a second run")
    ok, ratio, got = R.judge(out, ref, delta, T_OF[prec])
    note(name, ratio)
    assert bool(torch.isfinite(got).all()), (tag, name, "NaN or inf", (~torch.isfinite(got)).nonzero()[:4].tolist())
    assert bool(ok.all()), (tag, name, "outside the bound", int((~ok).sum()), "of", ok.numel(), "worst", ratio, (~ok).nonzero()[:4].tolist())
    return name, ratio


@GPU
@pytest.mark.parametrize("cs", TA_CASES, ids=[f"C{c}-{p}" for c, p in TA_CASES])
def test_temporal_attn_against_float64(dev, cs):
    C, prec = cs
    k = 0
    worst = {}
    seen = {"T2": set(), "T3": set()}
    for S in TA_SITES:
        for cfg, Tw in TA_ROWCFG:
            for fam in (("T1",) if cfg == "fresh1" else ("T1", "T2", "T3", "T4")):
                name, ratio = run_attn(dev, prec, C, S, Tw, fam, k)
                worst[name] = max(worst.get(name, 0.0), ratio)
            k += 1
    print(f"[temporal] attention C={C} {prec} " + " | ".join(f"{n} max_err/delta={v:.3f}" for n, v in sorted(worst.items())))


def test_peaked_targets_cover_the_window():
    """Over the case list of one (C, precision) the target position of T2 and of T3 takes every value 0..31."""
    dev = torch.device("cpu")
    s2, s3 = set(), set()
    for k in range(len(TA_SITES) * len(TA_ROWCFG)):
        g = torch.Generator(device=dev).manual_seed(k)
        s2 |= set(R.tattn_family("T2", 32, 3, [0, 1], [32, 32], k, False, g, dev)[3].flatten().tolist())
        s3 |= set(R.tattn_family("T3", 32, 3, [0, 1], [32, 32], k, False, g, dev)[3].flatten().tolist())
    assert s2 == set(range(32)) and s3 == set(range(32))


# ------------------------------------------------------------------------------------------------ cache store
CS_ROWS = [[(0, 31), (0, 1), (0, 0)], [(30, 1), (0, 31)], [(30, 1), (0, 31), (30, 0)], [(0, 0), (30, 0)]]       # (slot0, nslots) per row
CS_CASES = [(C, S, prec) for C in (32, 96) for S in (1, 9) for prec in ("bf16", "fp32")]


@GPU
@pytest.mark.parametrize("cs", CS_CASES, ids=[f"C{c}-S{s}-{p}" for c, s, p in CS_CASES])
def test_cache_store_bit_for_bit(dev, cs):
    from desktop2stereo_amd import _lib, ops
    C, S, prec = cs
    g = torch.Generator(device=dev).manual_seed(13000 + C + S)
    for tab in CS_ROWS:
        rows = len(tab)
        cur = torch.randn((rows, S, 3 * C), generator=g, device=dev)
        cur[..., 2 * C:] = 777.0 + torch.arange(C, device=dev)              # the q third: must never reach a ring
        cur = cur.to(DT_OF[prec]).contiguous()
        rings = [torch.randn((R.SLOTS, S, 2 * C), generator=g, device=dev).to(DT_OF[prec]) for _ in range(rows)]
        rbufs, rviews = ring_buffers(rings, dev)
        before = [rb.clone() for rb in rbufs]
        kw = dict(rows=rows, sites=S, channels=C, slots=R.SLOTS, rings=rviews, slot0=[t[0] for t in tab], nslots=[t[1] for t in tab])
        name = ops.temporal_probe("cache_store", prec, cur, **kw)
        first = [rb.clone() for rb in rbufs]
        for r, (s0, ns) in enumerate(tab):
            want = before[r].clone()
            want[1 + s0:1 + s0 + ns] = cur[r, :, :2 * C]
            assert torch.equal(bits(first[r]), bits(want)), (cs, tab, "ring of row", r)
        assert name == (f"cache_store_rows_kernel<{T_OF[prec]}>" if any(ns for _, ns in tab) else ""), (cs, tab, name)
        assert ops.temporal_probe("cache_store", prec, cur, **kw) == name
        for r in range(rows):
            assert torch.equal(bits(rbufs[r]), bits(first[r]))
        # slots beyond the ring: refused, nothing written
        with pytest.raises(_lib.D2SError):
            ops.temporal_probe("cache_store", prec, cur, **{**kw, "slot0": [30] * rows, "nslots": [2] * rows})
        for r in range(rows):
            assert torch.equal(bits(rbufs[r]), bits(first[r]))


# ------------------------------------------------------------------------------------------------ GEGLU, cast
EW_SHAPES = [(7, 37), (3, 384), (33, 128), (1, 1)]             # rows x 4C: no multiple of 256


@GPU
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_geglu_against_float64(dev, prec):
    from desktop2stereo_amd import ops
    g = torch.Generator(device=dev).manual_seed(14000)
    for rows, C4 in EW_SHAPES:
        assert (rows * C4) % 256
        u = R.geglu_family(rows, C4, prec == "bf16", g, dev)
        ref = R.geglu_compute(u, torch.float64)
        assert bool(torch.isfinite(ref).all())
        buf, out = guarded((rows, C4), DT_OF[prec], dev)
        name = twice(lambda: ops.temporal_probe("geglu", prec, u, out, rows=rows, channels=C4), [buf])
        assert name == f"geglu_kernel<{T_OF[prec]}>" and guards_intact(buf)
        ok, ratio, got = R.judge(out, ref, R.geglu_delta(u, ref), T_OF[prec])
        note(name, ratio)
        print(f"[temporal] geglu {rows}x{C4} {prec} max_err/delta={ratio:.3f}")
        assert bool(torch.isfinite(got).all()), (prec, rows, C4, "NaN or inf")
        assert bool(ok.all()), (prec, rows, C4, "outside the bound", int((~ok).sum()), ratio, (~ok).nonzero()[:4].tolist())


def cast_inputs(dev, g):
    r = torch.randn(1000, generator=g, device=dev)
    hi = torch.randint(0, 0x7f7f, (400,), generator=g, device=dev, dtype=torch.int32)
    ties = ((hi << 16) | 0x8000).view(torch.float32)                               # exactly between two bf16, even and odd
    near = torch.cat([((hi << 16) | 0x7fff), ((hi << 16) | 0x8001)]).view(torch.float32)
    sub = torch.randint(1, 0x7fffff, (200,), generator=g, device=dev, dtype=torch.int32).view(torch.float32)      # fp32 subnormals
    special = torch.tensor([0x00000000, -0x80000000, 0x7f800000, -0x00800000, 0x7f7fffff, -0x00800001, 0x7f7f7fff, 0x7f7f8000, 0x00008000,
                            0x00010000, 0x00018000], dtype=torch.int64, device=dev).to(torch.int32).view(torch.float32)
    x = torch.cat([r, ties, -ties, near, sub, -sub, special])
    return x[:x.numel() - (x.numel() % 256 == 0)].contiguous()


@GPU
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_cast_bit_for_bit(dev, prec):
    from desktop2stereo_amd import ops
    x = cast_inputs(dev, torch.Generator(device=dev).manual_seed(15000))
    n = x.numel()
    assert n % 256 and bool(torch.isinf(x.to(torch.bfloat16)[torch.isfinite(x)]).any())        # a finite fp32 that rounds to inf is in
    buf, out = guarded((n,), DT_OF[prec], dev)
    name = twice(lambda: ops.temporal_probe("cast_f32", prec, x, out, n=n), [buf])
    assert name == f"cast_f32_kernel<{T_OF[prec]}>" and guards_intact(buf)
    note(name, 0.0)
    want = x.to(DT_OF[prec])
    bad = (bits(out).view(n, -1) != bits(want).view(n, -1)).any(-1)
    assert not bool(bad.any()), (prec, int(bad.sum()), [hex(v & 0xffffffff) for v in x.view(torch.int32)[bad][:6].tolist()])


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_D = (4, 8, 64, 252, 256, 260, 384, 768, 1020, 1024)
LN_ROWS = (1, 3, 4, 5, 9)
LN_OUT = [("f32", "fp32", torch.float32), ("bf16", "bf16", torch.bfloat16), ("bx3", "fp32", torch.int32), ("e4m3", "bf16", torch.uint8),
          ("e4m3", "fp32", torch.uint8)]
SENTINEL = 3.0e30                                # in the rows the cls-dropping map skips: reaching an output it wrecks it


@GPU
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_against_float64(dev, D):
    from desktop2stereo_amd import ops
    g = torch.Generator(device=dev).manual_seed(16000 + D)
    k = 0
    for rows_out, drop, (fmt, prec, dt), fam in itertools.product(LN_ROWS, (False, True), LN_OUT, ("G1", "G2", "G3", "G4")):
        if fmt == "bx3" and D % 8:
            continue
        k += 1
        for eps in ((1e-5, 1e-6) if fam == "G3" else ((1e-5,) if k % 2 else (1e-6,))):
            xin = R.norm_family(fam, (rows_out, 1, D), False, g, dev).view(rows_out, D)
            if drop:                             # two images of P + 1 rows, the first of each dropped
                P = max(1, (rows_out + 1) // 2)
                x = torch.full((2 * (P + 1), D), SENTINEL, device=dev)
                x[1:P + 1] = xin[:P]
                x[P + 2:P + 2 + rows_out - P] = xin[P:]
                row_map = (P, P + 1, 1)
            else:
                x, row_map = xin.contiguous(), (0, 0, 0)
            gamma = 1.0 + 0.5 * torch.randn(D, generator=g, device=dev)
            beta = torch.randn(D, generator=g, device=dev)
            ref, mu, var = R.layernorm_compute(xin, gamma, beta, eps, torch.float64)
            delta = R.layernorm_delta(xin, gamma, eps, ref, mu, var)
            qs = 0.0
            if fmt == "e4m3":                    # about 1 % of the elements saturate
                srt = ref.abs().flatten().sort().values
                qs = R.f32(448.0 / float(srt[int(0.99 * (srt.numel() - 1))]))
                delta = delta + R.U * ref.abs()
            buf, out = guarded((rows_out, D), dt, dev)
            name = twice(lambda: ops.temporal_probe("layernorm", prec, x, out, rows=rows_out, channels=D, eps=eps, gamma=gamma, beta=beta,
                                                    qscale=qs, bx3_out=fmt == "bx3", row_map=row_map), [buf])
            tag = (D, rows_out, drop, fmt, prec, fam, eps)
            assert name == f"layernorm_kernel<{fmt}>", (tag, name)
            assert guards_intact(buf), (tag, "a guard was written")
            ok, ratio, got = R.judge(out, ref, delta, fmt, qs if qs else 1.0)
            note(name, ratio)
            if fmt == "e4m3":
                assert not bool(((out & 0x7f) == 0x7f).any()), (tag, "NaN byte in the e4m3 output")
                sat = (ref.abs() - delta) * qs > 448.0
                assert bool((got.abs()[sat] == 448.0).all()), (tag, "an element beyond the range is not saturated")
            assert bool(torch.isfinite(got).all()), (tag, "NaN or inf")
            assert bool(ok.all()), (tag, "outside the bound", int((~ok).sum()), "of", ok.numel(), "worst", ratio, (~ok).nonzero()[:4].tolist())
    print(f"[temporal] layernorm D={D} " + " | ".join(f"{n} {v:.3f}" for n, v in sorted(WORST.items()) if n.startswith("layernorm")))


@GPU
@pytest.mark.parametrize("D,fmt", [(1028, "f32"), (6, "f32"), (12, "bx3"), (1028, "bf16"), (6, "e4m3")])
def test_layernorm_refusals(dev, D, fmt):
    """An unsupported width is an error return and nothing is launched: the output keeps its fill."""
    from desktop2stereo_amd import _lib, ops
    prec, dt = {"f32": ("fp32", torch.float32), "bf16": ("bf16", torch.bfloat16), "bx3": ("fp32", torch.int32), "e4m3": ("bf16", torch.uint8)}[fmt]
    x = torch.randn((4, D), device=dev)
    buf, out = guarded((4, D), dt, dev)
    with pytest.raises(_lib.D2SError):
        ops.temporal_probe("layernorm", prec, x, out, rows=4, channels=D, eps=1e-6, gamma=torch.ones(D, device=dev), beta=torch.zeros(D, device=dev),
                           qscale=1.0 if fmt == "e4m3" else 0.0, bx3_out=fmt == "bx3")
    assert bool((buf.view(torch.uint8) == 0x7f).all())


# ------------------------------------------------------------------------------------------------ the probe's own checks
@GPU
def test_probe_refuses_malformed_cases(dev):
    """Sizes that do not fit the stated element counts, bad tables and shared rings are error returns; nothing is written."""
    from desktop2stereo_amd import _lib, ops
    S, C = 3, 32
    x = torch.randn((2, S, C), device=dev)
    ones = torch.ones(C, device=dev)
    buf, out = guarded((2, S, C), torch.float32, dev)
    cur = torch.randn((2, S, 3 * C), device=dev)
    ptab = torch.randn((32, 3 * C), device=dev)
    rings = [torch.randn((R.SLOTS, S, 2 * C), device=dev) for _ in range(2)]
    keep = [r.clone() for r in rings]
    att = dict(rows=2, sites=S, channels=C, slots=R.SLOTS, ptab=ptab, rings=rings, head=[0, 1], Tw=[32, 32], store_slot=[0, 1])
    bad = [
        lambda: ops.temporal_probe("groupnorm", "fp32", x, out[:1], rows=2, sites=S, channels=C, gamma=ones, beta=ones),          # out too small
        lambda: ops.temporal_probe("groupnorm", "fp32", x, out, rows=2, sites=S, channels=C, gamma=ones[:C - 1], beta=ones),      # gamma too small
        lambda: ops.temporal_probe("groupnorm", "fp32", x, out, rows=2, sites=S + 1, channels=C, gamma=ones, beta=ones),          # x too small
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "rings": [rings[0], rings[1][:30]]}),      # a short ring
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "rings": [rings[0], rings[0]]}),           # a shared ring
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "Tw": [32, 7]}),
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "head": [0, 31]}),
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "store_slot": [0, 31]}),
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "ptab": ptab[:31]}),
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur[:1], out, **att),
        lambda: ops.temporal_probe("temporal_attn", "fp32", cur, out, **{**att, "slots": 30}),
        lambda: ops.temporal_probe("geglu", "fp32", x.view(2, S * C), out, rows=2, channels=S * C),                               # u holds rows x C, not 2 C
        lambda: ops.temporal_probe("cast_f32", "fp32", x, out, n=x.numel() + 1),
        lambda: ops.temporal_probe("layernorm", "fp32", x.view(6, C), out, rows=6, channels=C, gamma=ones, beta=ones, row_map=(3, 4, 1)),   # reads row 7
    ]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.D2SError):
            f()
            pytest.fail(f"malformed case {i} was accepted")
    torch.cuda.synchronize()
    assert bool((buf.view(torch.uint8) == 0x7f).all())
    assert all(torch.equal(a, b) for a, b in zip(rings, keep))


# ------------------------------------------------------------------------------------------------ coverage of the table
def test_every_kernel_name_is_expected_by_a_case():
    """Every name the two planners (and the four fixed launchers) can emit is the expectation of some case above."""
    exp = set()
    for (_, sites, C, old, _) in GN_CASES:
        exp |= {gn_expect(p, sites, C, old) for p in ("bf16", "fp32")}
    for (C, prec) in TA_CASES:
        exp |= {ta_expect(prec, C, len(Tw)) for _, Tw in TA_ROWCFG}
    exp |= {f"layernorm_kernel<{fmt}>" for fmt, _, _ in LN_OUT}
    exp |= {f"{k}<{T_OF[p]}>" for k in ("geglu_kernel", "cast_f32_kernel", "cache_store_rows_kernel") for p in ("bf16", "fp32")}
    assert exp == set(TABLE), (sorted(set(TABLE) - exp), sorted(exp - set(TABLE)))
    assert {c for c, _ in TA_CASES} == set(TA_C) and all(R.tattn_plan(c)[1] in (1, 2, 4, 8, 16) for c in TA_C)
    assert {R.tattn_plan(c) for c in TA_C} == {(4, 1), (8, 1), (4, 4), (8, 2), (8, 4), (8, 8), (8, 16)}      # both CH, 1 .. 16 lanes per unit


@GPU
def test_worst_ratios_are_reported(dev):
    """Prints the worst err / delta per kernel over the whole file (the table in DESIGN.md)."""
    print("[temporal worst] " + " | ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v < 1.0 for v in WORST.values())
