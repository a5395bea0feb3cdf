"""GPU: a fusion stage's residual unit as ONE launch (conv3.hip conv3_rcu_kernel<PROJ>, plan_forward's rcu_fused / rcu1_fused) has the
bits of the separate launches it replaces -- two 3x3 convolutions (ReLU on load, the second one adding the un-ReLU'd input) and, with
PROJ, the stage's 1x1 projection.

Probe: ops.rcu_probe against two ops.conv3_probe calls and one ops.linear_probe call chained through bf16 tensors -- the same packing,
the same epilogues; those launches are held to float64 by tests/test_gpu_conv3.py and tests/test_gpu_linear.py.  Shapes: C = 128 and
the smallest maps at which the 4 x 8-pixel tiling can go wrong (one partial tile, exactly one tile, one pixel over in both directions),
the batch-1 frame's own two small maps, and a batch of two (an image boundary inside the grid: no halo may leak across it).  Inputs
with both signs, a conv1 bias that is large and positive in some channels -- a ring position outside the image computed as relu(bias)
instead of conv2's zero padding shows -- and a non-zero residual (x itself).

Engine: a tiny bf16 engine with fusion width 128 over consecutive different frames at batch 1 and 2, D2S_RCU_FUSE unset against
D2S_RCU_FUSE=0, with and without the side stream, and one temporal engine: byte-equal depth."""
import dataclasses

import pytest
import torch

GPU = pytest.mark.gpu
C128 = 128
SHAPES = [(1, 3, 5), (1, 4, 8), (1, 5, 9), (1, 11, 19), (1, 21, 37), (2, 11, 19)]


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weights():
    """One residual unit + projection, seeded on the host: w ~ N(0, 1 / fan-in) so that the intermediate keeps both signs; conv1's bias
    is +4 in every eighth channel (far above the convolution's unit-variance output there), small with both signs elsewhere."""
    g = torch.Generator().manual_seed(1234)
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
    xb = x.to(torch.bfloat16).float()                                    # what the engine's map holds (the probes round x the same way)
    t, k1 = ops.conv3_probe(xb, w1, b1, "bf16", relu_in=True)
    z, k2 = ops.conv3_probe(t.float(), w2, b2, "bf16", relu_in=True, res=xb)
    if wp is None:
        return z, (k1, k2)
    B, H, W, C = z.shape
    r = ops.linear_probe("tm_kvq", "bf16", z.float().reshape(B * H * W, C), wp, bp)
    return r["out"].reshape(B, H, W, C), (k1, k2, r["kernel"])


@GPU
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_unit_has_the_bits_of_the_separate_launches(dev, weights, B, H, W, proj):
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, wp, bp = (t.to(dev) for t in weights)
    g = torch.Generator().manual_seed(100 * H + W + B)
    x = (2.0 * torch.randn(B, H, W, C128, generator=g)).to(dev)          # both signs: the ReLU on load and the raw residual differ
    if not proj:
        wp = bp = None
    want, kernels = _separate(ops, x, w1, b1, w2, b2, wp, bp)
    assert not any("conv3_rcu" in k for k in kernels), kernels
    assert not any("splitk" in k for k in kernels), kernels              # (none of the separate launches at these shapes splits K)
    got, name = ops.rcu_probe(x, w1, b1, w2, b2, wp, bp)
    got2, name2 = ops.rcu_probe(x, w1, b1, w2, b2, wp, bp)
    assert name == name2 == f"conv3_rcu_kernel<{int(proj)}>", (name, name2)
    a, b = got.view(torch.int16).cpu(), want.contiguous().view(torch.int16).cpu()
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), "two runs differ"
    assert want.float().abs().max() > 1.0 and (want.float() < 0).any() and (want.float() > 0).any()
    bad = (a != b).nonzero()
    assert bad.numel() == 0, (B, H, W, proj, "first differing (b, y, x, c):", bad[:4].tolist(), "of", bad.shape[0])


@GPU
def test_ring_outside_the_image_is_zero_padding(dev, weights):
    """the case the large conv1 bias is for, spelled out: with conv1's ring evaluated outside the image the border pixels change, so the
    border of the fused result must equal the separate launches' border in particular (covered above) AND differ from a unit whose
    conv2 saw relu(bias) out there -- i.e. the inputs do exercise the difference"""
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, _, _ = (t.to(dev) for t in weights)
    x = torch.zeros(1, 4, 8, C128, device=dev)
    got, _ = ops.rcu_probe(x, w1, b1, w2, b2)
    # x = 0: conv1 = bias everywhere inside; conv2 of the constant map relu(b1) differs between border and interior pixels only through
    # the zero padding, so a result that is constant over the tile would mean the ring was filled with relu(bias)
    g = got.float()
    assert (g[0, 1, 3] - g[0, 0, 0]).abs().max() > 0.5, "border and interior agree: conv2 did not see zero padding"
    want, _ = _separate(ops, x, w1, b1, w2, b2, None, None)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))


@GPU
def test_probe_refuses_what_the_plan_keeps_separate(dev, weights):
    from desktop2stereo_amd import _lib, ops
    w1, b1, w2, b2, _, _ = (t.to(dev) for t in weights)
    with pytest.raises(_lib.D2SError, match="c3_rcu_ok refuses"):
        ops.rcu_probe(torch.zeros(1, 84, 148, C128, device=dev), w1, b1, w2, b2)       # 21 x 19 = 399 tiles
    w64 = torch.zeros(64, 64, 3, 3, device=dev)
    with pytest.raises(_lib.D2SError, match="c3_rcu_ok refuses"):
        ops.rcu_probe(torch.zeros(1, 4, 8, 64, device=dev), w64, b1[:64], w64, b2[:64])


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


def _frames(dev, B, calls=3):
    from desktop2stereo_amd import ops, synth
    xs = []
    for c in range(calls):
        fr = [ops.preprocess(torch.from_numpy(synth.structured_frame(90, 160, 300 + c * B + b)).to(dev), 84) for b in range(B)]
        xs.append(torch.cat(fr, 0).contiguous())
    return xs


def _run(eng, xs):
    outs = [eng(x) for x in xs]                      # queued back to back
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in outs]


@GPU
@pytest.mark.parametrize("B", [1, 2])
def test_engine_depth_is_byte_equal_with_and_without_the_fusion(dev, monkeypatch, B):
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.weights import make_weights
    cfg = dataclasses.replace(MODELS["tiny"], fusion=C128)
    wts = make_weights(cfg, 0)
    xs = _frames(dev, B)
    h, w = xs[0].shape[2:]
    try:
        got = {}
        for overlap in ({}, {"D2S_NO_OVERLAP": "1"}):
            for fuse in ({}, {"D2S_RCU_FUSE": "0"}):
                env = {**overlap, **fuse}
                eng = _engine(monkeypatch, env, cfg, wts, h, w, B, "bf16")
                plan = ops.forward_plan(cfg, h, w, B, "bf16")
                if fuse:
                    assert not any(plan["rcu_fused"]) and not any(plan["rcu1_fused"]), plan
                else:
                    assert all(plan["rcu_fused"][:3]) and plan["rcu1_fused"][1:] == [True, True], plan     # (the maps of an 84-pixel frame are tiny)
                got[tuple(sorted(env))] = _run(eng, xs)
                eng.close()
    finally:
        _clear(monkeypatch)
    ref = got[()]
    assert len(set(ref)) == len(xs), "different frames, different depth"
    for k, v in got.items():
        assert v == ref, (B, k, "differs from the fused, overlapped engine")


@GPU
def test_temporal_engine_depth_is_byte_equal_with_and_without_the_fusion(dev, monkeypatch):
    """a Video-Depth-Anything engine shares RCU2 + projection of stages 0-1 (the temporal modules sit behind the projection)"""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = dataclasses.replace(MODELS["tiny"], fusion=C128)
    wts = make_vda_weights(cfg, 0)
    xs = [ops.preprocess(torch.from_numpy(synth.structured_frame(90, 160, 40 + i)).to(dev), 84)[:, :, :42, :84].contiguous() for i in range(3)]
    try:
        got = []
        for env in ({}, {"D2S_RCU_FUSE": "0"}):
            eng = _engine(monkeypatch, env, cfg, wts, 42, 84, 1, "bf16", temporal=True)
            assert any(ops.forward_plan(cfg, 42, 84, 1, "bf16", temporal=True)["rcu_fused"]) == (not env)
            got.append(_run(eng, xs))
            eng.close()
    finally:
        _clear(monkeypatch)
    assert len(set(got[0])) == 3 and got[0] == got[1]
