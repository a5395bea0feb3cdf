"""GPU: the wide form of the fused residual unit (conv3.hip conv3_rcu_kernel<PROJ, 1>: 8 x 8 output pixels per block, seven conv1
fragments on the 10 x 10 ring-extended tile, four conv2 / projection fragments, a five-stage wave-private weight ring) has the bits
of the separate launches it replaces, and so those of the 4 x 8 form.

The construction is tests/test_gpu_rcu_fused.py's and tests/test_gpu_rcu_ring.py's: ops.rcu_probe(wide=True) against two
ops.conv3_probe calls and one ops.linear_probe call chained through bf16 tensors, int16 views compared, the projection on and off, two
runs equal.  Inputs with both signs; conv1's bias is +4 in every eighth channel, so a ring position outside the image computed as
relu(bias) instead of conv2's zero padding shows.  Shapes: one pixel, exactly one 8 x 8 tile, four ragged tiles, ragged in both
directions, nine tiles with one fully interior, several images (an image boundary inside the grid), and one map with eight different
inputs launched back to back (ring and LDS state across launches of free-running waves).

Engine: the tiny model with fusion width 128 at 294 x 350 -- its largest map, 84 x 100, is 273 tiles of 4 x 8 (refused on 256 CUs)
and 143 of 8 x 8 -- D2S_RCU_FUSE unset against 0, with and without the side stream, three frames queued back to back: byte-equal depth.

The bank arithmetic of the wide maps is proved at compile time (static_asserts over rcuw_slots in conv3.hip)."""
import dataclasses

import pytest
import torch

GPU = pytest.mark.gpu
C128 = 128
SHAPES = [(1, 1, 1), (1, 8, 8), (1, 9, 9), (1, 7, 17), (1, 24, 24), (3, 5, 9)]
BUSY = (1, 20, 28)


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weights():
    """One residual unit + projection, seeded on the host: w ~ N(0, 1 / fan-in) so that the intermediate keeps both signs; conv1's bias
    is +4 in every eighth channel, small with both signs elsewhere."""
    g = torch.Generator().manual_seed(8642)
    w1 = torch.randn(C128, C128, 3, 3, generator=g) / (9 * C128) ** 0.5
    w2 = torch.randn(C128, C128, 3, 3, generator=g) / (9 * C128) ** 0.5
    wp = torch.randn(C128, C128, generator=g) / C128 ** 0.5
    b1 = 0.1 * torch.randn(C128, generator=g)
    b1[::8] = 4.0
    b2 = 0.1 * torch.randn(C128, generator=g)
    bp = 0.1 * torch.randn(C128, generator=g)
    return w1, b1, w2, b2, wp, bp


def _separate(ops, x, w1, b1, w2, b2, wp, bp):
    """the launches the fused one replaces, chained through bf16 tensors as the engine chains them through its bf16 maps"""
    xb = x.to(torch.bfloat16).float()
    t, k1 = ops.conv3_probe(xb, w1, b1, "bf16", relu_in=True)
    z, k2 = ops.conv3_probe(t.float(), w2, b2, "bf16", relu_in=True, res=xb)
    assert "conv3_rcu" not in k1 and "conv3_rcu" not in k2, (k1, k2)
    if wp is None:
        return z.contiguous()
    B, H, W, C = z.shape
    r = ops.linear_probe("tm_kvq", "bf16", z.float().reshape(B * H * W, C), wp, bp)
    assert "conv3_rcu" not in r["kernel"], r["kernel"]
    return r["out"].reshape(B, H, W, C).contiguous()


def _input(dev, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn(B, H, W, C128, generator=g)).to(dev)        # both signs: the ReLU on load and the raw residual differ


def _same_bits(got, want, what):
    a, b = got.view(torch.int16), want.view(torch.int16)
    bad = (a != b).nonzero()
    assert bad.numel() == 0, (*what, "first differing (b, y, x, c):", bad[:4].tolist(), "of", bad.shape[0])


def _name(proj):
    return f"conv3_rcu_kernel<{int(proj)},1>"


@GPU
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_wide_form_has_the_bits_of_the_separate_launches(dev, weights, B, H, W, proj):
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, wp, bp = (t.to(dev) for t in weights)
    if not proj:
        wp = bp = None
    x = _input(dev, B, H, W, 1000 * B + 100 * H + W)
    want = _separate(ops, x, w1, b1, w2, b2, wp, bp)
    got, name = ops.rcu_probe(x, w1, b1, w2, b2, wp, bp, wide=True)
    got2, name2 = ops.rcu_probe(x, w1, b1, w2, b2, wp, bp, wide=True)
    assert name == name2 == _name(proj), (name, name2)
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), "two runs differ"
    wf = want.float()
    assert wf.abs().max() > 1.0 and (wf < 0).any() and (wf > 0).any()
    _same_bits(got, want, (B, H, W, proj))


@GPU
@pytest.mark.parametrize("proj", [False, True])
def test_wide_form_back_to_back(dev, weights, proj):
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, wp, bp = (t.to(dev) for t in weights)
    if not proj:
        wp = bp = None
    B, H, W = BUSY
    xs = [_input(dev, B, H, W, 9000 + 17 * s) for s in range(8)]
    torch.cuda.synchronize()
    outs = [ops.rcu_probe(x, w1, b1, w2, b2, wp, bp, wide=True) for x in xs]      # queued back to back on one stream
    again, _ = ops.rcu_probe(xs[0], w1, b1, w2, b2, wp, bp, wide=True)
    torch.cuda.synchronize()
    assert all(name == _name(proj) for _, name in outs), [n for _, n in outs]
    assert torch.equal(outs[0][0].view(torch.int16), again.view(torch.int16)), "two runs of one input differ"
    assert len({o.view(torch.int16).cpu().numpy().tobytes() for o, _ in outs}) == len(xs), "different inputs, different results"
    for s, (x, (got, _)) in enumerate(zip(xs, outs)):
        _same_bits(got, _separate(ops, x, w1, b1, w2, b2, wp, bp), (B, H, W, proj, "input", s))


@GPU
def test_wide_ring_outside_the_image_is_zero_padding(dev, weights):
    """x = 0: conv1 = bias everywhere inside; conv2 of the constant map relu(b1) differs between border and interior pixels only through
    the zero padding, so a result that is constant over the tile would mean the ring was filled with relu(bias)"""
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, _, _ = (t.to(dev) for t in weights)
    x = torch.zeros(1, 8, 8, C128, device=dev)
    got, name = ops.rcu_probe(x, w1, b1, w2, b2, wide=True)
    assert name == _name(False), name
    g = got.float()
    assert (g[0, 3, 3] - g[0, 0, 0]).abs().max() > 0.5, "border and interior agree: conv2 did not see zero padding"
    _same_bits(got, _separate(ops, x, w1, b1, w2, b2, None, None), (1, 8, 8, False))


@GPU
def test_wide_probe_refuses_what_the_kernel_does_not_take(dev, weights):
    from desktop2stereo_amd import _lib, ops
    w1, b1, w2, b2, _, _ = (t.to(dev) for t in weights)
    w64 = torch.zeros(64, 64, 3, 3, device=dev)
    with pytest.raises(_lib.D2SError, match="c3_rcu_wide_fits refuses"):
        ops.rcu_probe(torch.zeros(1, 8, 8, 64, device=dev), w64, b1[:64], w64, b2[:64], wide=True)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    with pytest.raises(_lib.D2SError, match="c3_rcu_wide_fits refuses"):
        ops.rcu_probe(torch.zeros(1, 8, 8 * cus + 1, C128, device=dev), w1, b1, w2, b2, wide=True)      # one tile over the CU count
    got, name = ops.rcu_probe(torch.zeros(1, 8, 8 * cus, C128, device=dev), w1, b1, w2, b2, wide=True)    # exactly the CU count
    assert name == _name(False) and got.shape == (1, 8, 8 * cus, C128)


# ---- engine --------------------------------------------------------------------------------------------------------------------------
def _engine(monkeypatch, env, *args, **kw):
    """An engine under the switches of `env`; D2S_RCU_FUSE is read by every forward pass (plan_forward), so it stays set for the
    caller's runs and the caller clears it; the creation-time switches are read here"""
    from desktop2stereo_amd import ops
    for k in ("D2S_NO_OVERLAP", "D2S_RCU_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops.reload_env()
    return ops.Engine(*args, **kw)


def _clear(monkeypatch):
    from desktop2stereo_amd import ops
    for k in ("D2S_NO_OVERLAP", "D2S_RCU_FUSE"):
        monkeypatch.delenv(k, raising=False)
    ops.reload_env()


@GPU
def test_engine_depth_is_byte_equal_with_and_without_the_wide_form(dev, monkeypatch):
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.weights import make_weights
    cfg = dataclasses.replace(MODELS["tiny"], fusion=C128)
    wts = make_weights(cfg, 0)
    h, w = 294, 350
    xs = [ops.preprocess(torch.from_numpy(synth.structured_frame(h, w, 500 + c)).to(dev), w).contiguous() for c in range(3)]
    assert tuple(xs[0].shape) == (1, 3, h, w)
    try:
        got = {}
        for overlap in ({}, {"D2S_NO_OVERLAP": "1"}):
            for fuse in ({}, {"D2S_RCU_FUSE": "0"}):
                env = {**overlap, **fuse}
                eng = _engine(monkeypatch, env, cfg, wts, h, w, 1, "bf16")
                plan = ops.forward_plan(cfg, h, w, 1, "bf16")
                assert (plan["fH"][0], plan["fW"][0]) == (84, 100)
                if fuse:
                    assert not any(plan["rcu_wide"]) and not any(plan["rcu1_wide"]) and not any(plan["rcu_fused"]), plan
                else:                                        # (256 CUs: the 4 x 8 rule refuses the 84 x 100 map, the wide rule admits it)
                    assert plan["rcu_wide"] == [False, False, False, True] and plan["rcu1_wide"] == [True, False, False], plan
                    assert plan["rcu_fused"] == [True, True, True, False] and plan["rcu1_fused"] == [False, True, True], plan
                outs = [eng(x) for x in xs]                  # queued back to back
                torch.cuda.synchronize()
                got[tuple(sorted(env))] = [o.cpu().numpy().tobytes() for o in outs]
                eng.close()
    finally:
        _clear(monkeypatch)
    ref = got[()]
    assert len(set(ref)) == len(xs), "different frames, different depth"
    for k, v in got.items():
        assert v == ref, (k, "differs from the fused, overlapped engine")
