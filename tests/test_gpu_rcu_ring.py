"""GPU: conv3_rcu_kernel<PROJ> with its wave-private weight ring and its conflict-free pixel maps (conv3.hip: rcu_c1_row / rcu_c1_col,
rcu_half / rcu_idx) still has the bits of the separate launches.

The construction is tests/test_gpu_rcu_fused.py's: ops.rcu_probe against two ops.conv3_probe calls and one ops.linear_probe call
chained through bf16 tensors, inputs with both signs, a conv1 bias that is large and positive in every eighth channel (a ring position
outside the image computed as relu(bias) instead of conv2's zero padding shows), the projection on and off.  What this file adds is
aimed at what the new loops can break:

  * the lane -> position maps at tile edges: which lane owns which pixel changed in conv1 (the h1 store, the in-image test), in conv2
    (the residual load, the output store) and in the projection, so the shapes put an image edge at every place of the 4 x 8 tile --
    a single pixel, one column / one row over, partial tiles in both directions at once, exact multiples with four tiles, and image
    boundaries inside the grid of a batch;
  * free-running waves: the K loops have no block barrier any more, a wave's own counters order its ring stages.  A missing wait
    would show as a wrong value (a stale or half-landed weight tile), most likely with many blocks on the chip and launches back to
    back, so two maps with 110 and 240 blocks run eight differently seeded inputs back to back on one stream, each compared bit for
    bit with the separate launches, and one input twice with equal bits.

The bank arithmetic of the maps is proved at compile time (static_asserts over rcu_b128_cycles in conv3.hip)."""
import pytest
import torch

GPU = pytest.mark.gpu
C128 = 128
EDGE_SHAPES = [(1, 1, 1), (1, 4, 9), (1, 5, 8), (1, 7, 17), (1, 8, 16), (3, 5, 9)]
BUSY_SHAPES = [(1, 42, 74), (8, 21, 37)]                       # 110 and 240 blocks of one 4 x 8 tile each


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weights():
    """One residual unit + projection, seeded on the host: w ~ N(0, 1 / fan-in) so that the intermediate keeps both signs; conv1's bias
    is +4 in every eighth channel, small with both signs elsewhere."""
    g = torch.Generator().manual_seed(4321)
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


@GPU
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("B,H,W", EDGE_SHAPES)
def test_lane_maps_at_tile_edges(dev, weights, B, H, W, proj):
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, wp, bp = (t.to(dev) for t in weights)
    if not proj:
        wp = bp = None
    x = _input(dev, B, H, W, 1000 * B + 100 * H + W)
    want = _separate(ops, x, w1, b1, w2, b2, wp, bp)
    got, name = ops.rcu_probe(x, w1, b1, w2, b2, wp, bp)
    assert name == f"conv3_rcu_kernel<{int(proj)}>", name
    wf = want.float()
    assert wf.abs().max() > 1.0 and (wf < 0).any() and (wf > 0).any()
    _same_bits(got, want, (B, H, W, proj))


@GPU
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("B,H,W", BUSY_SHAPES)
def test_free_running_waves_back_to_back(dev, weights, B, H, W, proj):
    from desktop2stereo_amd import ops
    w1, b1, w2, b2, wp, bp = (t.to(dev) for t in weights)
    if not proj:
        wp = bp = None
    xs = [_input(dev, B, H, W, 7000 + 13 * s + H) for s in range(8)]
    torch.cuda.synchronize()
    outs = [ops.rcu_probe(x, w1, b1, w2, b2, wp, bp) for x in xs]         # queued back to back on one stream
    again, _ = ops.rcu_probe(xs[0], w1, b1, w2, b2, wp, bp)
    torch.cuda.synchronize()
    assert all(name == f"conv3_rcu_kernel<{int(proj)}>" for _, name in outs), [n for _, n in outs]
    assert torch.equal(outs[0][0].view(torch.int16), again.view(torch.int16)), "two runs of one input differ"
    assert len({o.view(torch.int16).cpu().numpy().tobytes() for o, _ in outs}) == len(xs), "different inputs, different results"
    for s, (x, (got, _)) in enumerate(zip(xs, outs)):
        _same_bits(got, _separate(ops, x, w1, b1, w2, b2, wp, bp), (B, H, W, proj, "input", s))
