"""GPU: the frame's plan (d2s_forward_plan, tests/test_cpu_forward_plan.py) against what a forward pass launches -- the LayerNorm launch
count of the profiler, on the tiny model at 84 x 126, for the four regimes a small model reaches: bf16 at 1 frame (everything folded but
layer 0's LN1), at 2 (the four tap LayerNorms are launches), at 4 (nothing folds) and fp32 (never folds)."""
import pytest
import torch

GPU = pytest.mark.gpu


@GPU
def test_layernorm_launches_are_the_plans():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.weights import make_weights
    cfg, h, w = MODELS["tiny"], 84, 126
    wts = make_weights(cfg, 0)
    g = torch.Generator().manual_seed(7)
    want = {("bf16", 1): 1, ("bf16", 2): 5, ("bf16", 4): 12, ("fp32", 1): 12}       # 4 layers: 1 + 3 | 4 | 4 taps
    for (prec, B), ln in want.items():
        plan = ops.forward_plan(cfg, h, w, B, prec, profiling=True)
        x = torch.randn((B, 3, h, w), generator=g).cuda()
        eng = ops.Engine(cfg, wts, h, w, B, prec)
        eng.profile(True)
        eng(x)
        got = eng.profile_read()["layernorm"]["launches"]
        eng.profile(False)
        eng.close()
        assert got == plan["ln_launches"] == ln, (prec, B, got, plan)
