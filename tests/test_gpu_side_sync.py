"""GPU: the side stream's schedule (engine.hip forward: tap-private LayerNorm operands, the fork on the FC2 launch's own completion)
computes the bits of the schedules it replaces -- D2S_NO_OVERLAP=1 (one stream) and D2S_SIDE_SYNC=0 (shared lnbuf / lnstats and the
ev_ln waits, recorded fork events) -- over CONSECUTIVE DIFFERENT frames queued without a
host synchronisation in between: a tap-private buffer overwritten too early by frame k + 1 shows as frame k's depth changing.  The
smallest shapes at which the hazard exists: the tiny model (4 layers, every layer a tap layer) at the 84-pixel depth resolution of
the tiny_r84 fixture, and the smallest temporal engine of tests/test_gpu_vda.py.  A race depends on timing: a pass does not prove its
absence, the invariant at tap_ln_pair (engine.hip) is what is reviewed."""
import pytest
import torch

GPU = pytest.mark.gpu
SCHEDULES = ({}, {"D2S_NO_OVERLAP": "1"}, {"D2S_SIDE_SYNC": "0"})       # the new one, one stream, the replaced one


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def _engine(monkeypatch, env, *args, **kw):
    """An engine created under the switches of `env` (read once at creation), the environment put back afterwards."""
    from desktop2stereo_amd import ops
    for k in ("D2S_NO_OVERLAP", "D2S_SIDE_SYNC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops.reload_env()
    eng = ops.Engine(*args, **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    ops.reload_env()
    return eng


def _tiny_inputs(dev, B, calls=6):
    """`calls` batches of B different seeded frames (90 x 160, as tiny_r84's) at depth resolution 84"""
    from desktop2stereo_amd import ops, synth
    xs = []
    for c in range(calls):
        fr = [ops.preprocess(torch.from_numpy(synth.structured_frame(90, 160, 100 + c * B + b)).to(dev), 84) for b in range(B)]
        xs.append(torch.cat(fr, 0).contiguous())
    return xs


def _run(eng, xs):
    outs = [eng(x) for x in xs]                      # queued back to back: frame k + 1's encoder runs under frame k's side branches
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in outs]


@GPU
@pytest.mark.parametrize("prec,B,side_taps_private", [("bf16", 1, True), ("bf16", 2, False), ("fp32", 1, False), ("bf16", 4, False)])
def test_consecutive_frames_have_the_bits_of_the_other_schedules(dev, monkeypatch, prec, B, side_taps_private):
    """bf16 at 1 frame folds the taps (private operands); at 2 the taps are launches and at 4 nothing folds, fp32 never folds: lnbuf stays
    shared there, the pointer selection follows the plan and not the batch"""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.weights import make_weights
    cfg = MODELS["tiny"]
    wts = make_weights(cfg, 0)
    xs = _tiny_inputs(dev, B)
    h, w = xs[0].shape[2:]
    plan = ops.forward_plan(cfg, h, w, B, prec)
    assert plan["use_side"] and plan["tap_side"][:3] == [True] * 3
    assert plan["sites"]["neck0"]["folded"] == side_taps_private, plan["sites"]
    got = []
    for env in SCHEDULES:
        eng = _engine(monkeypatch, env, cfg, wts, h, w, B, prec)
        got.append(_run(eng, xs))
        eng.close()
    assert len(set(got[0])) == len(xs), "different frames, different depth"
    for k in range(len(xs)):
        assert got[0][k] == got[1][k], (prec, B, "call", k, "differs from D2S_NO_OVERLAP=1")
        assert got[0][k] == got[2][k], (prec, B, "call", k, "differs from D2S_SIDE_SYNC=0")


@GPU
def test_temporal_engine_stream_has_the_bits_of_the_other_schedules(dev, monkeypatch):
    """ViT-S Video-Depth-Anything at 196 x 336, a 3-frame stream: branch 3 runs on the side stream there, so tap 3 -- the last layer's --
    has private operands too"""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["vits"]
    wts = make_vda_weights(cfg, 0)
    xs = [ops.preprocess(torch.from_numpy(synth.structured_frame(1080, 1920, 40 + i)).to(dev), 336) for i in range(3)]
    assert tuple(xs[0].shape[2:]) == (196, 336)
    got = []
    for env in SCHEDULES:
        eng = _engine(monkeypatch, env, cfg, wts, 196, 336, 1, "bf16", temporal=True)
        got.append(_run(eng, xs))
        eng.close()
    assert len(set(got[0])) == 3
    for k in range(3):
        assert got[0][k] == got[1][k], ("frame", k, "differs from D2S_NO_OVERLAP=1")
        assert got[0][k] == got[2][k], ("frame", k, "differs from D2S_SIDE_SYNC=0")


@GPU
def test_engine_memory_grows_by_the_side_taps_pairs(dev, monkeypatch):
    """d2s_engine_memory: a bf16 engine has one (lnbuf, lnstats)-sized pair per side tap more than under D2S_SIDE_SYNC=0 -- 3 taps, 4 on
    a temporal engine -- and an fp32 engine, which never folds, nothing"""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.weights import make_weights
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["tiny"]

    def grown(wts, h, w, B, prec, **kw):
        mem = []
        for env in ({}, {"D2S_SIDE_SYNC": "0"}):
            eng = _engine(monkeypatch, env, cfg, wts, h, w, B, prec, **kw)
            mem.append(eng.memory_bytes())
            eng.close()
        return mem[0] - mem[1]

    for (h, w, B) in ((84, 154, 1), (84, 126, 3)):
        M = B * ((h // cfg.patch) * (w // cfg.patch) + 1)
        pair = M * cfg.hidden * 2 + (cfg.hidden // 16 + 1) * M * 2 * 4          # lnbuf (bf16) + lnstats
        assert grown(make_weights(cfg, 0), h, w, B, "bf16") == 3 * pair, (h, w, B)
        assert grown(make_weights(cfg, 0), h, w, B, "fp32") == 0, (h, w, B)
    M = (42 // cfg.patch) * (84 // cfg.patch) + 1
    pair = M * cfg.hidden * 2 + (cfg.hidden // 16 + 1) * M * 2 * 4
    assert grown(make_vda_weights(cfg, 0), 42, 84, 1, "bf16", temporal=True) == 4 * pair
