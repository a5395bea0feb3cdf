"""GPU: the three forms of the depth post-process (desktop2stereo_amd/csrc/post.hip) against each other and against the oracle.

    fused  post_fused_kernel, one launch                                    the default for <= 2 frames of a relative model
    tile   percentile_bounds_kernel + shape_blur_kernel                     D2S_POST_ONE=0; metric models; blur radius > 8
    rows   percentile_bounds_kernel + shape_hblur_kernel + vblur_kernel     D2S_POST_FUSE_MAXB=0; > 2 frames; in place; a tile too large

Every case runs through the default dispatch, the two switches and the in-place entry point; d2s_post_plan must name the kernels the
case expects for each, all outputs must be bit-identical to each other and to a second run, and the result must lie within 5e-6 of
oracle/d2s_oracle.py::post_process_depth (the bound the in-place entry is held to in test_gpu_parity.py)."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SWITCHES = ({}, {"D2S_POST_ONE": "0"}, {"D2S_POST_FUSE_MAXB": "0"})      # default dispatch, no fused form, no tile form either
FEW = ("fused", "tile", "rows")                                          # what <= 2 frames of a relative model take under SWITCHES
PF_BINS, PF_CAND = 2048, 512                                             # post_fused_kernel's value-linear fast path (post.hip)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def params(**kw):
    from desktop2stereo_amd.config import PipelineParams
    return dataclasses.replace(PipelineParams(), **kw)


def expect_kernels(form, k, metric):
    kt = 13 if k == 13 else 0
    pb = "percentile_bounds<metric>" if metric else "percentile_bounds<relative>"
    return {"fused": [f"post_fused<{kt}>"], "tile": [pb, "shape_blur"], "rows": [pb, f"shape_hblur<{kt}>", f"vblur<{kt}>"]}[form]


def run_case(dev, monkeypatch, name, maps, p, forms, k):
    """maps [B,h,w] through the three SWITCHES (expected forms `forms`) and in place: plan, bit-identity, repeatability, oracle.
    Returns the output."""
    from desktop2stereo_amd import ops
    from oracle import d2s_oracle as O
    B, h, w = maps.shape
    d = _t(maps, dev)
    outs = []
    try:
        for env, form in zip(SWITCHES, forms):
            for key in ("D2S_POST_ONE", "D2S_POST_FUSE_MAXB"):
                monkeypatch.delenv(key, raising=False)
            for key, v in env.items():
                monkeypatch.setenv(key, v)
            ops.reload_env()
            plan = ops.post_plan(B, h, w, p)
            assert (plan["form"], plan["kernels"], plan["k"]) == (form, expect_kernels(form, k, p.metric), k), (name, env, plan)
            outs.append(ops.post_process_depth_to(d, p).cpu().numpy())
            assert np.array_equal(outs[-1], ops.post_process_depth_to(d, p).cpu().numpy()), (name, env, "second run")
    finally:
        for key in ("D2S_POST_ONE", "D2S_POST_FUSE_MAXB"):
            monkeypatch.delenv(key, raising=False)
        ops.reload_env()
    plan = ops.post_plan(B, h, w, p, in_place=True)
    assert (plan["form"], plan["kernels"]) == ("rows", expect_kernels("rows", k, p.metric)), (name, "in place", plan)
    outs.append(ops.post_process_depth(d, p).cpu().numpy())
    assert np.array_equal(outs[-1], ops.post_process_depth(d, p).cpu().numpy()), (name, "in place", "second run")
    assert np.array_equal(d.cpu().numpy(), maps), (name, "input changed")
    for label, o in zip(("D2S_POST_ONE=0", "D2S_POST_FUSE_MAXB=0", "in place"), outs[1:]):
        assert np.array_equal(outs[0], o), (name, label, float(np.abs(outs[0] - o).max()))
    for b in range(B):
        want = O.post_process_depth(maps[b], p.foreground_scale, p.aa_strength, p.gamma, metric=p.metric)
        err = float(np.abs(outs[0][b] - want).max())
        assert err <= 5e-6, (name, b, err)
    return outs[0]


def test_post_process_one_launch_equals_separate_kernels(dev, monkeypatch):
    """post_fused_kernel (D2S_POST_ONE=1: bounds + shape + both blur passes in one launch, d2s_post_process_to with <= 2
    frames) against the separate kernels (D2S_POST_ONE=0) and against the in-place entry point: bit-identical, for the default
    parameters, a non-default blur radius (the generic tap-count instantiation), a saturated map (ties at both extremes: the
    value-linear select's edge bins) and a constant map."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import PipelineParams
    rng = np.random.default_rng(11)
    maps = {"smooth": np.stack([synth.smooth_depth(294, 518, 3), synth.smooth_depth(294, 518, 4)]),
            "noise": rng.uniform(0.0, 20.0, (2, 294, 518)).astype(np.float32),
            "saturated": np.clip(rng.normal(0.5, 1.0, (2, 294, 518)), 0.0, 1.0).astype(np.float32),
            "constant": np.full((1, 196, 336), 0.25, np.float32),
            "odd": rng.uniform(0.0, 1.0, (1, 101, 203)).astype(np.float32)}
    try:
        for pname, p in (("default", PipelineParams()), ("aa2", dataclasses.replace(PipelineParams(), aa_strength=2.0)),
                         ("no_fg", dataclasses.replace(PipelineParams(), foreground_scale=0.0))):
            for mname, m in maps.items():
                d = _t(m, dev)
                outs = {}
                for one in ("1", "0"):
                    monkeypatch.setenv("D2S_POST_ONE", one)
                    ops.reload_env()
                    outs[one] = ops.post_process_depth_to(d, p).cpu().numpy()
                inplace = ops.post_process_depth(d, p).cpu().numpy()
                assert np.array_equal(outs["1"], outs["0"]), (pname, mname, float(np.abs(outs["1"] - outs["0"]).max()))
                assert np.array_equal(outs["1"], inplace), (pname, mname, "in place")
    finally:
        monkeypatch.delenv("D2S_POST_ONE", raising=False)
        ops.reload_env()
    # the same maps through every form, with the plan, a second run and the oracle
    for pname, p, k in (("default", params(), 13), ("aa2", params(aa_strength=2.0), 7), ("no_fg", params(foreground_scale=0.0), 13)):
        for mname, m in maps.items():
            run_case(dev, monkeypatch, f"{mname}/{pname}", m, p, FEW, k)


# ------------------------------------------------------------------------------------------------ maps that leave the fast path
def quantised(h, w, seed):
    """Values {1..6}/8, a single 0.0 and a single 1.0 at flat indices 0 and 4 (inside every subsample of step 1, 2 or 4)."""
    m = (np.random.default_rng(seed).integers(1, 7, (h, w)) / 8.0).astype(np.float32)
    m.reshape(-1)[0], m.reshape(-1)[4] = 0.0, 1.0
    return m


def fast_path_candidates(m, percentile=2.0, cap=6144):
    """post_fused_kernel's value-linear histogram (bin_of, post.hip) restated: how many keys share a bin with each of the two order
    statistics.  More than PF_CAND in either sends the kernel to its radix passes; (0, 0) for a target in an edge bin."""
    f32 = np.float32
    flat = m.reshape(-1)
    n = flat.size
    step = -(-n // cap) if n > cap else 1
    v = np.sort(flat[::step])
    tail = min(v.size, max(1, int(np.rint(percentile / 100.0 * (v.size - 1))) + 1))
    vmin, vmax = v[0], v[-1]
    bscale = f32(PF_BINS - 2) / f32(vmax - vmin)
    bins = 1 + np.clip(((v - vmin) * bscale).astype(f32).astype(np.int64), 0, PF_BINS - 3)
    bins = np.where(v <= vmin, 0, np.where(v >= vmax, PF_BINS - 1, bins))
    counts = []
    for rank in (tail - 1, v.size - tail):
        b = bins[rank]
        counts.append(0 if b in (0, PF_BINS - 1) else int((bins == b).sum()))
    return tuple(counts)


@pytest.mark.parametrize("h,w,step", [(64, 96, 1), (101, 203, 4)])
def test_quantised_map_takes_the_radix_passes(dev, monkeypatch, h, w, step):
    """A map of six distinct values between two outliers: both order statistics sit in bins of ~1000 equal keys, more than the fast
    path's PF_CAND candidates, so post_fused_kernel falls through to its multi-pass radix select -- span [0.0, 1.0] in key space is
    30 bits: passes of shift 19, 8 and 0."""
    from desktop2stereo_amd import ops
    m = quantised(h, w, 7 + h)
    plan = ops.post_plan(1, h, w, params())
    assert plan["step"] == step and plan["m"] == -(-h * w // step)
    c0, c1 = fast_path_candidates(m)
    print(f"quantised {h}x{w}: the target bins hold {c0} / {c1} keys")
    assert c0 > PF_CAND and c1 > PF_CAND, (c0, c1)
    sub = np.sort(m.reshape(-1)[::step])
    assert sub[0] == 0.0 and sub[-1] == 1.0 and (sub[1], sub[-2]) == (0.125, 0.75)          # both outliers are in the subsample
    # the maps the one-launch test above uses stay on the fast path: that is why this case exists
    assert max(fast_path_candidates(np.random.default_rng(11).uniform(0.0, 20.0, (294, 518)).astype(np.float32))) <= PF_CAND
    run_case(dev, monkeypatch, f"quantised {h}x{w}", m[None], params(), FEW, 13)


# ------------------------------------------------------------------------------------------------ shapes, radii, metric, batches
def odd_map():
    return np.random.default_rng(5).uniform(0.0, 1.0, (1, 101, 203)).astype(np.float32)


def metric_map():
    """101 x 203, about 30 % non-positive pixels (exact zeros and negatives), the rest in (0, 20]."""
    rng = np.random.default_rng(9)
    m = rng.uniform(0.05, 20.0, (1, 101, 203)).astype(np.float32)
    u = rng.random((1, 101, 203))
    m[u < 0.15] = 0.0
    m[(u >= 0.15) & (u < 0.30)] *= -1.0
    return m


def few_valid_map():
    m = -np.random.default_rng(10).uniform(0.0, 1.0, (1, 9, 130)).astype(np.float32)
    m.reshape(-1)[[3, 130, 131, 500, 640, 777, 900, 1000, 1100, 1169]] = [0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]
    return m


CASES = {
    # one row and two columns past a full 8 x 128 tile, n below the cap
    "9x130": (lambda: np.random.default_rng(3).uniform(0.0, 5.0, (1, 9, 130)).astype(np.float32), {}, FEW, 13),
    # n <= 10: the bounds are (0, 0)
    "3x3": (lambda: np.random.default_rng(4).uniform(0.5, 2.0, (2, 3, 3)).astype(np.float32), {}, FEW, 13),
    # r = 9 > 8: the tile form is the default
    "aa6": (odd_map, dict(aa_strength=6.0), ("tile", "tile", "rows"), 19),
    "aa6 batch 3": (lambda: np.concatenate([odd_map(), odd_map()[:, ::-1], odd_map()[:, :, ::-1]]), dict(aa_strength=6.0), ("rows",) * 3, 19),
    # k = 49: a tile of 68 096 bytes does not fit the LDS, rows even at batch 1
    "aa16": (odd_map, dict(aa_strength=16.0), ("rows",) * 3, 49),
    # k = 1: no blur
    "aa0.2": (odd_map, dict(aa_strength=0.2), FEW, 1),
    "metric": (metric_map, dict(metric=True), ("tile", "tile", "rows"), 13),
    "metric aa2": (metric_map, dict(metric=True, aa_strength=2.0), ("tile", "tile", "rows"), 7),
    # <= 10 valid pixels: the bounds are (0, 0)
    "metric few valid": (few_valid_map, dict(metric=True), ("tile", "tile", "rows"), 13),
}


@pytest.mark.parametrize("name", list(CASES))
def test_post_process_forms(dev, monkeypatch, name):
    build, kw, forms, k = CASES[name]
    maps = build()
    if name == "metric":
        frac = float((maps <= 0).mean())
        assert 0.25 < frac < 0.35 and (maps == 0).any() and (maps < 0).any(), frac
    if name == "metric few valid":
        assert int((maps > 0).sum()) == 10
    out = run_case(dev, monkeypatch, name, maps, params(**kw), forms, k)
    assert np.isfinite(out).all()


def test_batch_of_mixed_maps_equals_single_frames(dev, monkeypatch):
    """Three different maps in one call (rows form) against the same frames one at a time (fused form): bit-identical per frame --
    no frame's bounds or blur leak into another's."""
    from desktop2stereo_amd import ops
    rng = np.random.default_rng(12)
    maps = np.stack([odd_map()[0], quantised(101, 203, 108), np.clip(rng.normal(0.5, 1.0, (101, 203)), 0.0, 1.0).astype(np.float32)])
    p = params()
    out = run_case(dev, monkeypatch, "mixed batch 3", maps, p, ("rows",) * 3, 13)
    for b in range(3):
        assert ops.post_plan(1, 101, 203, p)["form"] == "fused"
        one = ops.post_process_depth_to(_t(maps[b:b + 1], dev), p).cpu().numpy()
        assert np.array_equal(one[0], out[b]), (b, float(np.abs(one[0] - out[b]).max()))
