"""References, bounds, judges and input families of the temporal-module and LayerNorm kernel tests (test_gpu_temporal.py on the
device, test_cpu_temporal_ref.py on the host).  Every `*_compute` function states one kernel's arithmetic in plain torch and takes the
dtype it computes in: float64 is the reference, float32 the faithful emulation the CPU test feeds to the judges; `mut` names one
deliberate error (the mutants the CPU test must see rejected).  Operands arrive exact in the kernel's storage type and are widened, so
reference and kernel start from the same numbers.  The bounds are derived in test_gpu_temporal.py's docstring; u = 2^-24."""
import math

import torch

from f64_ref import bx3_value, e4m3_value, pow2, rne_bf16, rne_e4m3

U = 2.0 ** -24
SLOTS = 31
HEADS = 8


def f32(v: float) -> float:
    """the float32 a kernel argument holds"""
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ judges
def judge(got_raw: torch.Tensor, ref: torch.Tensor, delta: torch.Tensor, fmt: str, qscale: float = 1.0):
    """got_raw: the kernel's output as stored (float32, bfloat16, int32 bf16x3 unit words, uint8 e4m3 bytes), ref / delta float64 of the
    same shape.  -> (ok mask, worst err / delta, got as float64).  f32: |got - ref| <= delta; bx3: the same with the unit format's own
    2^-17 |ref| (hi = bf16(v), lo = bf16(v - hi): |v - hi - lo| <= 2^-9 2^-9 |v|, twice that for the rounding of v itself to ~17
    bits); bf16 / e4m3: got inside [RNE(ref - delta), RNE(ref + delta)] of the format (e4m3: of (ref -+ delta) qscale, saturating)."""
    if fmt == "f32":
        got = got_raw.double()
        err = (got - ref).abs()
        ok = err <= delta
    elif fmt == "bx3":
        got = bx3_value(got_raw)
        delta = delta + 2.0 ** -17 * (ref.abs() + delta)
        err = (got - ref).abs()
        ok = err <= delta
    elif fmt == "bf16":
        got = got_raw.double()
        lo, hi = rne_bf16(ref - delta), rne_bf16(ref + delta)
        ok = (got >= lo) & (got <= hi)
        half = pow2(torch.frexp(got.abs().clamp_min(2.0 ** -120))[1] - 9)
        err = ((got - ref).abs() - half).clamp_min(0)
    elif fmt == "e4m3":
        got = e4m3_value(got_raw)
        lo, hi = rne_e4m3((ref - delta) * qscale), rne_e4m3((ref + delta) * qscale)
        ok = (got >= lo) & (got <= hi)
        ge = torch.frexp(got.abs().clamp_min(2.0 ** -9))[1]
        half = torch.where(got.abs() < 2.0 ** -6, torch.full_like(got, 2.0 ** -10), pow2(ge - 5)) / qscale
        err = ((got / qscale - ref).abs() - half).clamp_min(0)
        err = torch.where(ref.abs() * qscale >= 448.0, torch.zeros_like(err), err)
    else:
        raise ValueError(fmt)
    ok = ok & torch.isfinite(got)
    ratio = float((err / delta.clamp_min(1e-300)).max()) if err.numel() else 0.0
    return ok, ratio, got


def store(v: torch.Tensor, fmt: str, qscale: float = 1.0) -> torch.Tensor:
    """an emulation's float32 result -> the kernel's storage (what judge() takes as got_raw)"""
    if fmt == "f32":
        return v.float()
    if fmt == "bf16":
        return v.float().to(torch.bfloat16)
    if fmt == "e4m3":
        r = rne_e4m3((v.float() * f32(qscale)).double())              # (exact re-encoding of the rounded value)
        a = r.abs()
        e = torch.frexp(a.clamp_min(2.0 ** -9))[1]                     # a = m 2^e, 0.5 <= m < 1
        normal = a >= 2.0 ** -6
        ebits = torch.where(normal, e + 6, torch.zeros_like(e)).to(torch.int64)
        mant = torch.where(normal, torch.round(a / pow2(e - 4)).to(torch.int64) - 8, torch.round(a * 512.0).to(torch.int64))
        b = (ebits << 3) | mant
        return (b | torch.where(r < 0, 0x80, 0)).to(torch.uint8)
    if fmt == "bx3":
        v = v.float()
        hi = v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        rows, D = v.shape
        units = torch.stack([hi.view(rows, D // 8, 8), lo.view(rows, D // 8, 8)], dim=2)       # [rows, units, hi | lo, 8]
        return units.contiguous().view(torch.int16).view(rows, D // 8, 16).view(torch.int32).reshape(rows, D)
    raise ValueError(fmt)


# ------------------------------------------------------------------------------------------------ normalisation
def norm_depth_groupnorm(reg: bool, cpg: int, rpt: int, sites: int) -> int:
    """additions an element passes through on its way into a block sum: the thread's own run, 6 xor-shuffle levels, the wave partials"""
    if reg:
        return rpt * cpg + 6 + 16
    return -(-(sites * cpg) // 256) + 6 + 4


NORM_DEPTH_LAYERNORM = 4 * 3 + 6              # 4 float4 per lane, (x + y) + (z + w) then the running sum; 6 shuffle levels


def norm_compute(x: torch.Tensor, gamma, beta, eps: float, dtype, mut: str = ""):
    """x [..., n, c]: one normalisation per leading index over the n * c elements of [n, c]; gamma / beta broadcast over [n, c].
    Two-pass mean and BIASED variance.  -> (y, mean, var, mean |x|) in dtype.  mut: "unbiased" | "onepass" | "eps" (10 x eps)."""
    xd = x.to(dtype)
    n = xd.shape[-1] * xd.shape[-2]
    mu = xd.sum(dim=(-1, -2), keepdim=True) / n
    if mut == "onepass":
        var = (xd * xd).sum(dim=(-1, -2), keepdim=True) / n - mu * mu
    else:
        var = ((xd - mu) ** 2).sum(dim=(-1, -2), keepdim=True) / (n - 1 if mut == "unbiased" else n)
    e = torch.tensor(f32(eps) * (10.0 if mut == "eps" else 1.0), dtype=dtype, device=x.device)
    rstd = 1.0 / torch.sqrt(var + e)
    y = (xd - mu) * rstd * gamma.to(dtype) + beta.to(dtype)
    return y, mu, var, xd.abs().sum(dim=(-1, -2), keepdim=True) / n


def norm_delta(x, gamma, eps: float, depth: int, ref, mu, var):
    """The bound of a two-pass float32 normalisation whose block sums have `depth` additions per element (docstring of
    test_gpu_temporal.py, "GroupNorm / LayerNorm")."""
    xd = x.double()
    n = xd.shape[-1] * xd.shape[-2]
    mabs = xd.abs().sum(dim=(-1, -2), keepdim=True) / n
    e_mu = (depth + 1) * U * mabs
    ve = var + f32(eps)
    rstd = 1.0 / torch.sqrt(ve)
    r_rstd = (0.5 * (depth + 5) + 4) * U + 0.5 * e_mu * e_mu / ve
    return gamma.double().abs() * rstd * (e_mu + (xd - mu).abs() * (r_rstd + 3 * U)) + U * ref.abs()


def gn_view(x: torch.Tensor, groups: int):
    """[rows, sites, C] -> [rows, groups, sites, cpg]"""
    rows, sites, C = x.shape
    return x.view(rows, sites, groups, C // groups).permute(0, 2, 1, 3)


def groupnorm_compute(x, gamma, beta, eps, groups, dtype, mut: str = ""):
    """x [rows, sites, C] (storage type) -> y [rows, sites, C], mean, var [rows, groups, 1, 1] in dtype.  mut "rows": the statistics of
    rows 0 and 1 taken together."""
    rows, sites, C = x.shape
    cpg = C // groups
    g, b = gamma.view(1, groups, 1, cpg), beta.view(1, groups, 1, cpg)
    xv = gn_view(x, groups)
    if mut == "rows":
        two = xv[:2].permute(1, 0, 2, 3).reshape(1, groups, 2 * sites, cpg)
        y2, mu, var, _ = norm_compute(two, g, b, eps, dtype)
        y = torch.cat([y2.view(groups, 2, sites, cpg).permute(1, 0, 2, 3), norm_compute(xv[2:], g, b, eps, dtype)[0]])
    else:
        y, mu, var, _ = norm_compute(xv, g, b, eps, dtype, mut)
    return y.permute(0, 2, 1, 3).reshape(rows, sites, C), mu, var


def groupnorm_delta(x, gamma, eps, groups, depth, ref, mu, var):
    rows, sites, C = x.shape
    d = norm_delta(gn_view(x, groups), gamma.view(1, groups, 1, C // groups), eps, depth, gn_view(ref, groups), mu, var)
    return d.permute(0, 2, 1, 3).reshape(rows, sites, C)


def layernorm_compute(x, gamma, beta, eps, dtype, mut: str = ""):
    """x [rows, D] float32 -> y, mean, var [rows, 1, 1]"""
    y, mu, var, _ = norm_compute(x[:, None, :], gamma, beta, eps, dtype, mut)
    return y[:, 0, :], mu, var


def layernorm_delta(x, gamma, eps, ref, mu, var):
    return norm_delta(x[:, None, :], gamma, eps, NORM_DEPTH_LAYERNORM, ref[:, None, :], mu, var)[:, 0, :]


def norm_family(fam: str, shape, bf16: bool, g: torch.Generator, dev):
    """-> x float32 [lead..., n, c] exact in the storage type (bf16: rounded to it), one normalisation per leading index.
    G1: every leading index its own mean in [-40, 40] and scale in [0.1, 8];  G2: mean 64, standard deviation 0.5;
    G3: standard deviation 0.01 around 0;  G4: constant."""
    lead = tuple(shape[:-2]) + (1, 1)
    r = torch.randn(shape, generator=g, device=dev)
    if fam == "G1":
        x = (torch.rand(lead, generator=g, device=dev) * 80 - 40) + (0.1 + 7.9 * torch.rand(lead, generator=g, device=dev)) * r
    elif fam == "G2":
        x = 64.0 + 0.5 * r
    elif fam == "G3":
        x = 0.01 * r
    elif fam == "G4":
        x = (torch.rand(lead, generator=g, device=dev) * 80 - 40).expand(shape).contiguous()
    else:
        raise ValueError(fam)
    return x.to(torch.bfloat16).float() if bf16 else x


# ------------------------------------------------------------------------------------------------ temporal attention
def tattn_plan(C: int):
    """(CH, lpu) as plan_temporal_attn picks them"""
    dh = C // HEADS
    ch = 8 if dh % 8 == 0 else 4
    lpu = 1
    while lpu * ch < dh:
        lpu *= 2
    return ch, lpu


def tattn_compute(cur, rings, ptab, head, Tw, store_slot, dtype, mut: str = "", bounds: bool = False):
    """cur [rows, S, 3C] (k' | v' | q'), rings: one [31, S, 2C] per row, ptab float32 [32, 3C].  -> out [rows, S, C] in dtype, the
    rings afterwards (new tensors), and with bounds = True the per-element quantities the bound is built from.
    mut: "slot" (ring slot (head + j + 1) mod 31), "ptab" (table row j + 1), "store_first" (the store lands before the reads),
    "mask_last" (position Tw-1 masked out)."""
    rows, S, C3 = cur.shape
    C = C3 // 3
    dh = C // HEADS
    pt = ptab.to(dtype)
    outs, extra, rings_after = [], [], []
    for r in range(rows):
        ring_new = rings[r].clone()
        if store_slot[r] >= 0:
            ring_new[store_slot[r]] = cur[r, :, :2 * C]
        src = ring_new if mut == "store_first" else rings[r]
        T = Tw[r]
        shift = 1 if mut == "slot" else 0
        idx = [(head[r] + j + shift) % SLOTS for j in range(T - 1)]
        prow = [min(j + 1, 31) if mut == "ptab" else j for j in range(T)]
        c = cur[r].to(dtype)
        kv = torch.cat([src[idx].to(dtype), c[None, :, :2 * C]]) if T > 1 else c[None, :, :2 * C]       # [T, S, 2C]
        k = (kv[..., :C] + pt[prow, None, 0:C]).view(T, S, HEADS, dh)
        v = (kv[..., C:] + pt[prow, None, C:2 * C]).view(T, S, HEADS, dh)
        q = (c[:, 2 * C:] + pt[T - 1, 2 * C:]).view(S, HEADS, dh)
        scale = 1.0 / math.sqrt(dh) if dtype == torch.float64 else f32(1.0 / math.sqrt(dh))
        s = torch.einsum("shd,jshd->shj", q, k) * scale
        if mut == "mask_last" and T > 1:
            s[..., T - 1] = -1e30
        x = s - s.max(dim=-1, keepdim=True).values
        e = torch.exp(x)
        w = e / e.sum(dim=-1, keepdim=True)
        outs.append(torch.einsum("shj,jshd->shd", w, v).reshape(S, C))
        rings_after.append(ring_new)
        if bounds:
            Tm = (torch.einsum("shd,jshd->shj", q.abs(), k.abs()) * scale).max(dim=-1).values          # [S, 8]
            A = torch.einsum("shj,jshd->shd", w, v.abs())
            Ax = torch.einsum("shj,jshd->shd", w * x.abs(), v.abs())
            X = (w * x.abs()).sum(dim=-1)
            extra.append((Tm, A, Ax, X, w))
    out = torch.stack(outs)
    if not bounds:
        return out, rings_after
    Tm, A, Ax, X = (torch.stack([e_[i] for e_ in extra]) for i in range(4))
    return out, rings_after, {"T": Tm, "A": A.reshape(rows, S, C), "Ax": Ax.reshape(rows, S, C), "X": X, "w": [e_[4] for e_ in extra]}


def tattn_delta(C: int, b: dict):
    """delta = (rS T + rF) A + the __expf argument term (docstring of test_gpu_temporal.py, "Temporal attention")."""
    ch, lpu = tattn_plan(C)
    dh = C // HEADS
    rS = 2 * (ch + int(math.log2(lpu)) + 7) * U
    rF = 28 * U
    rows, S, _ = b["A"].shape
    per_head = lambda t: t[..., None].expand(rows, S, HEADS, dh).reshape(rows, S, C)
    return (rS * per_head(b["T"]) + rF + 2 * U * per_head(b["X"])) * b["A"] + 2 * U * b["Ax"]


def tattn_family(fam: str, C: int, S: int, head, Tw, case_idx: int, bf16: bool, g: torch.Generator, dev):
    """-> cur [rows, S, 3C], rings (one [31, S, 2C] per row; a fresh row's -- Tw = 1 -- is all NaN), ptab float32 [32, 3C], and the
    target position pi [rows, S, 8] (or None) whose softmax weight the family asserts.  Values are exact in the storage type.
    T1 diffuse;  T2 peaked by ring content;  T3 peaked by the table's k rows;  T4: T2 with pi = 0 everywhere."""
    rows = len(head)
    dh = C // HEADS
    rn = lambda *s: torch.randn(s, generator=g, device=dev)
    gq = 3.0 * dh ** 0.25
    pi = None
    if fam == "T1":
        cur, ring, ptab = rn(rows, S, 3 * C), rn(rows, SLOTS, S, 2 * C), rn(32, 3 * C)
    else:
        # window position j of row r: ring slot (head_r + j) % 31 for j < 31, the current frame for j = 31
        kwin = 0.25 * rn(rows, 32, S, HEADS, dh)
        vwin = rn(rows, 32, S, HEADS, dh)
        j = torch.arange(32, device=dev)
        vwin[:, j, :, :, j % dh] += 4.0
        qn = 0.25 * rn(rows, S, HEADS, dh)
        ptab = torch.zeros(32, 3, HEADS, dh, device=dev)
        ptab[:, 1] = rn(32, HEADS, dh)
        if fam in ("T2", "T4"):
            ci = torch.randint(0, dh, (rows, S, HEADS), generator=g, device=dev)
            e = torch.nn.functional.one_hot(ci, dh).float()                               # [rows, S, 8, dh]
            ri, si, hi = torch.meshgrid(torch.arange(rows, device=dev), torch.arange(S, device=dev), torch.arange(HEADS, device=dev), indexing="ij")
            pi = (si * HEADS + hi + 5 * case_idx + 11 * ri) % 32 if fam == "T2" else torch.zeros_like(si)
            sign = torch.where(j.view(1, 32, 1, 1) == pi[:, None], 1.0, -1.0)             # [rows, 32, S, 8]
            kwin += gq * sign[..., None] * e[:, None]
            qn += gq * e
        else:                                                                             # T3
            ci = torch.randint(0, dh, (HEADS,), generator=g, device=dev)
            e = torch.nn.functional.one_hot(ci, dh).float()                               # [8, dh]
            pih = (4 * torch.arange(HEADS, device=dev) + case_idx) % 32
            sign = torch.where(j.view(32, 1) == pih.view(1, HEADS), 1.0, -1.0)            # [32, 8]
            ptab[:, 0] = gq * sign[..., None] * e[None]
            ptab[:, 2] = 0.25 * rn(32, HEADS, dh)
            qn += gq * e
            pi = pih.view(1, 1, HEADS).expand(rows, S, HEADS)
        ptab = ptab.reshape(32, 3 * C)
        cur = torch.cat([kwin[:, 31].reshape(rows, S, C), vwin[:, 31].reshape(rows, S, C), qn.reshape(rows, S, C)], dim=-1)
        ring = torch.empty(rows, SLOTS, S, 2 * C, device=dev)
        for r in range(rows):
            slot = (head[r] + torch.arange(31, device=dev)) % SLOTS
            ring[r, slot] = torch.cat([kwin[r, :31].reshape(31, S, C), vwin[r, :31].reshape(31, S, C)], dim=-1)
    if bf16:
        cur, ring = cur.to(torch.bfloat16), ring.to(torch.bfloat16)
    rings = []
    for r in range(rows):
        rings.append(torch.full_like(ring[r], float("nan")) if Tw[r] == 1 else ring[r].contiguous())
    return cur.contiguous(), rings, ptab.contiguous(), pi


def tattn_target_weight(b: dict, pi, Tw):
    """the smallest softmax weight of a target position over the warm rows (fresh rows have one position)"""
    lo = 1.0
    for r, w in enumerate(b["w"]):
        if Tw[r] == 32:
            lo = min(lo, float(w.gather(-1, pi[r][..., None]).min()))
    return lo


# ------------------------------------------------------------------------------------------------ GEGLU
def geglu_compute(u: torch.Tensor, dtype, mut: str = ""):
    """u [rows, 2 C4] (x | gate) -> x * 0.5 gate (1 + erf(gate / sqrt 2)) [rows, C4].  mut: "swap" (halves swapped), "tanh" (tanh-GELU)."""
    C4 = u.shape[1] // 2
    x, gate = u[:, :C4].to(dtype), u[:, C4:].to(dtype)
    if mut == "swap":
        x, gate = gate, x
    if mut == "tanh":
        act = 0.5 * gate * (1.0 + torch.tanh(0.7978845608028654 * (gate + 0.044715 * gate ** 3)))
    else:
        act = 0.5 * gate * (1.0 + torch.erf(gate * 0.7071067811865476))
    return x * act


def geglu_delta(u: torch.Tensor, ref: torch.Tensor):
    C4 = u.shape[1] // 2
    x, gate = u[:, :C4].double(), u[:, C4:].double()
    erf = torch.erf(gate * 0.7071067811865476)
    return 0.5 * (x * gate).abs() * (8 * U * erf.abs() + 2 * U) + 4 * U * ref.abs()


BF16_MAX = 3.3895313892515355e38


def geglu_family(rows: int, C4: int, bf16: bool, g: torch.Generator, dev):
    """x ~ 0.5 + 0.25 randn (never near a gate's range), gates uniform over [-8, 8] with +-0, +-8 and +- the largest finite bf16
    planted (x = +-0.25 there, so the product stays finite)."""
    x = 0.5 + 0.25 * torch.randn((rows, C4), generator=g, device=dev)
    gate = torch.rand((rows, C4), generator=g, device=dev) * 16 - 8
    special = torch.tensor([0.0, -0.0, 8.0, -8.0, BF16_MAX, -BF16_MAX], device=dev)
    n = min(special.numel(), gate.numel())
    pos = torch.randperm(gate.numel(), generator=g, device=dev)[:n]
    gate.view(-1)[pos] = special[:n]
    x.view(-1)[pos] = torch.where(torch.arange(n, device=dev) % 2 == 0, 0.25, -0.25)
    u = torch.cat([x, gate], dim=1)
    return (u.to(torch.bfloat16) if bf16 else u).contiguous()
