"""GPU: several Video-Depth-Anything streams on one engine (max_batch = N stream slots; include/d2s.h d2s_model_forward_streams).
Every stream, taken alone, must still be the reference's stream: the goldens are those of tests/test_gpu_vda.py, the numpy oracle is
oracle/vda_oracle.py, and every tolerance is the one that file uses for the same kind of comparison."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no ROCm device is visible")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model_input(frame, res):
    from oracle import d2s_oracle as O
    return O.normalise(O.resize_patch_aligned(np.ascontiguousarray(frame.transpose(2, 0, 1)), res))


def _tiny_inputs(h, w, res, seed0, n):
    from desktop2stereo_amd import synth
    return [_model_input(synth.structured_frame(h, w, seed0 + i), res) for i in range(n)]


def _staggered(eng, xs, n_streams, lag, check, dev):
    """All streams play the one sequence xs, shifted: stream k joins at call lag * k (reset, then named), receives frame
    call - lag * k and is dropped from the calls after its last frame.  check(k, fi, depth_row) per frame of every stream."""
    nfr = len(xs)
    for call in range(nfr + lag * (n_streams - 1)):
        rows = [k for k in range(n_streams) if 0 <= call - lag * k < nfr]
        for k in rows:
            if call == lag * k:
                eng.reset_stream(k)
        x = torch.stack([xs[call - lag * k] for k in rows])
        d = eng(x, streams=rows).cpu().numpy()
        for r, k in enumerate(rows):
            check(k, call - lag * k, d[r])


@pytest.mark.parametrize("prec,tol", [("fp32", 3e-4), ("bf16", 0.036)])
def test_each_stream_is_the_reference_stream_at_real_dimensions(dev, golden_dir, prec, tol):
    """ViT-S at 196 x 336 on the 40 frames of tests/golden/vda_vits_long (the REFERENCE's streaming model, every 7th depth row; the
    window wraps), four streams staggered by three calls: the four windows wrap at different calls, and fresh and warm rows share
    launches.  Gates of test_vda_window_wrap_at_real_dimensions."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["vits"]
    z = np.load(os.path.join(golden_dir, "vda_vits_long.npz"))
    meta = json.load(open(os.path.join(golden_dir, "vda_vits_long.json")))
    rs = meta["row_stride"]
    assert len(meta["frames"]) == 40
    xs = [ops.preprocess(_t(synth.structured_frame(fr["h"], fr["w"], fr["seed"]), dev), meta["depth_resolution"])[0] for fr in meta["frames"]]
    eng = ops.Engine(cfg, make_vda_weights(cfg, 0), 196, 336, 4, prec, temporal=True)
    worst = [0.0] * 4

    def check(k, fi, d):
        err = float(np.abs(d[::rs] - z[f"f{fi}_depth"]).max() / max(1.0, float(meta["frames"][fi]["range"][1])))
        worst[k] = max(worst[k], err)
        assert err <= tol, (prec, "stream", k, "frame", fi, err)

    _staggered(eng, xs, 4, 3, check, dev)
    print(f"[vda streams ViT-S 196x336, {prec}] worst frame error per stream {['%.2e' % v for v in worst]} of the range (49 calls)")
    eng.close()


@pytest.mark.parametrize("prec,tol", [("fp32", 3e-4), ("bf16", 0.036)])
def test_each_stream_is_the_reference_stream_tiny(dev, golden_dir, prec, tol):
    """The same on the tiny model with tests/golden/vda_tiny_long (gates of test_vda_window_wrap_vs_reference)."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["tiny"]
    z = np.load(os.path.join(golden_dir, "vda_tiny_long.npz"))
    meta = json.load(open(os.path.join(golden_dir, "vda_tiny_long.json")))
    assert len(meta["frames"]) >= 34
    xs = [_t(_model_input(synth.structured_frame(fr["h"], fr["w"], fr["seed"]), meta["depth_resolution"]), dev) for fr in meta["frames"]]
    eng = ops.Engine(cfg, make_vda_weights(cfg, 0), 42, 84, 4, prec, temporal=True)
    worst = [0.0] * 4

    def check(k, fi, d):
        ref = z[f"f{fi}_depth"]
        err = float(np.abs(d - ref).max() / max(1.0, float(ref.max())))
        worst[k] = max(worst[k], err)
        assert err <= tol, (prec, "stream", k, "frame", fi, err)

    _staggered(eng, xs, 4, 3, check, dev)
    print(f"[vda streams tiny 42x84, {prec}] worst frame error per stream {['%.2e' % v for v in worst]} of the range")
    eng.close()


@pytest.mark.parametrize("H,W,res,h,w", [(90, 160, 84, 42, 84), (90, 150, 70, 42, 70)])
def test_different_content_per_stream_vs_oracle(dev, H, W, res, h, w):
    """Three streams fed three different sequences, 40 calls, against three numpy oracles (gate of
    test_vda_longer_than_window_vs_oracle).  42 x 70 is an ODD patch grid: 3 x 5 patches, 15 / 15 / 4 / 60 sites, so the boundary between
    two rows falls inside a wave of the attention kernel in the modules with C <= 64."""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    from oracle.vda_oracle import VideoDepthOracle
    cfg = MODELS["tiny"]
    wts = make_vda_weights(cfg, 0)
    seqs = [_tiny_inputs(H, W, res, s0, 40) for s0 in (200, 400, 600)]
    assert seqs[0][0].shape[-2:] == (h, w)
    eng = ops.Engine(cfg, wts, h, w, 3, "fp32", temporal=True)
    orcs = [VideoDepthOracle(cfg, wts) for _ in range(3)]
    worst = 0.0
    for fi in range(40):
        d = eng(_t(np.stack([seqs[k][fi] for k in range(3)]), dev)).cpu().numpy()
        for k in range(3):
            ref = orcs[k].forward(seqs[k][fi])
            err = float(np.abs(d[k] - ref).max() / max(1.0, float(ref.max())))
            worst = max(worst, err)
            assert err <= 3e-4, ("stream", k, "frame", fi, err)
    print(f"[vda streams vs oracle, {h}x{w}] worst frame error {worst:.2e} of the range, 3 streams x 40 frames")
    eng.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_streams_are_independent_bit_for_bit(dev, prec):
    """An output row of every kernel on this path depends on its own input row only, and dispatch depends on shapes only: stream 1's 36
    outputs are the SAME ARRAYS whatever streams 0 and 2 are fed and whenever stream 0 is reset (at call 10, and at call 33 after the
    wrap).  Run A twice first, so a failure points at coupling and not at run-to-run noise.  (42 x 70: rows straddle waves.)"""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS["tiny"]
    n = 36
    a = [_tiny_inputs(90, 150, 70, s0, n) for s0 in (1200, 1400, 1600)]
    b = [_tiny_inputs(90, 150, 70, 1800, n), a[1], _tiny_inputs(90, 150, 70, 2000, n)]
    eng = ops.Engine(cfg, make_vda_weights(cfg, 0), 42, 70, 3, prec, temporal=True)

    def run(seqs, resets=()):
        eng.reset_stream()
        outs = []
        for fi in range(n):
            if fi in resets:
                eng.reset_stream(0)
            outs.append(eng(_t(np.stack([s[fi] for s in seqs]), dev)).cpu().numpy()[1].copy())
        return outs

    a1, a2 = run(a), run(a)
    for fi in range(n):
        assert np.array_equal(a1[fi], a2[fi]), (prec, "run A is not reproducible", fi, float(np.abs(a1[fi] - a2[fi]).max()))
    b1 = run(b, resets=(10, 33))
    for fi in range(n):
        assert np.array_equal(a1[fi], b1[fi]), (prec, "stream 1 depends on its neighbours", fi, float(np.abs(a1[fi] - b1[fi]).max()))
    eng.close()


@pytest.mark.parametrize("name,h,w,res,src", [("tiny", 42, 84, 84, (90, 160)), ("vits", 196, 336, 336, (360, 640))])
def test_subset_calls_against_single_stream_engines(dev, name, h, w, res, src):
    """40 calls that name [0, 1, 2, 3] and [0, 1, 3] alternately (stream 2 gets 20 frames); each stream against a single-stream engine
    fed the same frames.  Same arithmetic, different launch shapes: the floors of test_vda_fused_modules_agree_with_the_separate_launches
    (fp32 2e-5 of the range; bf16 3e-2 max and 5e-3 mean)."""
    from desktop2stereo_amd import ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    cfg = MODELS[name]
    wts = make_vda_weights(cfg, 0)
    seqs = [[_t(x, dev) for x in _tiny_inputs(src[0], src[1], res, 3000 + 100 * k, 40)] for k in range(4)]
    assert tuple(seqs[0][0].shape[-2:]) == (h, w)
    for prec, tol_max, tol_mean in (("fp32", 2e-5, 2e-5), ("bf16", 3e-2, 5e-3)):
        eng = ops.Engine(cfg, wts, h, w, 4, prec, temporal=True)
        got = [[] for _ in range(4)]
        for call in range(40):
            rows = [0, 1, 2, 3] if call % 2 == 0 else [0, 1, 3]
            d = eng(torch.stack([seqs[k][len(got[k])] for k in rows]), streams=rows).cpu().numpy()
            for r, k in enumerate(rows):
                got[k].append(d[r].copy())
        eng.close()
        assert [len(g) for g in got] == [40, 40, 20, 40]
        worst = [0.0, 0.0]
        for k in range(4):
            one = ops.Engine(cfg, wts, h, w, 1, prec, temporal=True)
            for fi in range(len(got[k])):
                ref = one(seqs[k][fi][None]).cpu().numpy()[0]
                dd = np.abs(got[k][fi] - ref) / max(1.0, float(ref.max()))
                worst = [max(worst[0], float(dd.max())), max(worst[1], float(dd.mean()))]
                assert dd.max() <= tol_max and dd.mean() <= tol_mean, (name, prec, "stream", k, "frame", fi, float(dd.max()), float(dd.mean()))
            one.close()
        print(f"[vda streams subset calls, {name} {prec}] vs single-stream engines: max {worst[0]:.2e} mean {worst[1]:.2e} of the range")


def test_streams_through_pipeline_at_1080p(dev, golden_dir):
    """d2s_pipeline_streams in the shape of test_vda_stream_through_pipeline_at_1080p: two streams, fp32, 40 calls; stream 1 is reset
    alone at call 20.  Pass 1, EMA off: engine A runs the bare forward, engine B the pipeline on the same frames -- B's full-resolution
    depth against oracle post-process + up-sample of A's raw maps (<= 2e-5), its Full-SBS frame against the oracle warp (<= 1 LSB) on
    calls 0, 1, 31, 32, 39.  Pass 2 after a full reset, use_ema=True, the same reset of stream 1 at call 20: each stream's depth is the
    numpy chain prev <- lerp(prev, d, 1 - alpha) over ITS pass-1 depths (the up-sample is linear: it commutes with the EMA), restarting
    for stream 1 at call 20 and not for stream 0 (<= 2e-5)."""
    from desktop2stereo_amd import ops, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams
    from desktop2stereo_amd.vda_weights import make_vda_weights
    from oracle import d2s_oracle as O
    cfg = MODELS["vits"]
    meta = json.load(open(os.path.join(golden_dir, "vda_vits_long.json")))
    res = meta["depth_resolution"]
    p = PipelineParams(depth_resolution=res)
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, "Full-SBS", p.fill_16_9)
    wts = make_vda_weights(cfg, 0)
    eng_a = ops.Engine(cfg, wts, 196, 336, 2, "fp32", temporal=True)
    eng_b = ops.Engine(cfg, wts, 196, 336, 2, "fp32", temporal=True)
    H, W = 1080, 1920
    ncall = 40

    def frames_of(call):        # stream 0: the golden sequence's frames; stream 1: other content
        fr = meta["frames"][call]
        return np.stack([synth.structured_frame(H, W, fr["seed"]), synth.structured_frame(H, W, fr["seed"] + 1000)])

    plain = [[], []]            # pass 1: full-resolution depth per stream, EMA off
    worst_d, worst_lsb = 0.0, 0
    for call in range(ncall):
        if call == 20:
            eng_a.reset_stream(1)
            eng_b.reset_stream(1)
        fr = frames_of(call)
        ft = _t(fr, dev)
        raw = eng_a(ops.preprocess(ft, res)).cpu().numpy()
        out, dfull = eng_b.pipeline(ft, p, sp, use_ema=False, want_depth=True, streams=[0, 1])
        dfull = dfull.cpu().numpy()
        for k in range(2):
            want = O.upsample_depth(O.post_process_depth(raw[k], p.foreground_scale, p.aa_strength), H, W)
            dd = float(np.abs(dfull[k] - want).max())
            worst_d = max(worst_d, dd)
            assert dd <= 2e-5, ("pipeline depth vs forward + oracle post-process", "stream", k, "call", call, dd)
            plain[k].append(dfull[k].copy())
            if call in (0, 1, 31, 32, 39):
                want_sbs = O.to_u8(O.make_sbs_core(fr[k].transpose(2, 0, 1).astype(np.float32), dfull[k], p.ipd, p.depth_strength,
                                                   "Full-SBS", p.fill_16_9, p.convergence).transpose(1, 2, 0))
                diff = np.abs(out[k].cpu().numpy().astype(np.int32) - want_sbs.astype(np.int32))
                worst_lsb = max(worst_lsb, int(diff.max()))
                assert diff.max() <= 1, ("pipeline warp vs the oracle", "stream", k, "call", call, int(diff.max()))
    eng_a.close()
    # pass 2: one EMA state per stream slot
    eng_b.reset_stream()
    wgt = np.float32(1.0) - np.float32(p.ema_alpha)
    prev = [None, None]
    worst_e = 0.0
    for call in range(ncall):
        if call == 20:
            eng_b.reset_stream(1)
            prev[1] = None
        _, dfull = eng_b.pipeline(_t(frames_of(call), dev), p, sp, use_ema=True, want_depth=True, streams=[0, 1])
        dfull = dfull.cpu().numpy()
        for k in range(2):
            d = plain[k][call]
            prev[k] = d if prev[k] is None else prev[k] + wgt * (d - prev[k])
            dd = float(np.abs(dfull[k] - prev[k]).max())
            worst_e = max(worst_e, dd)
            assert dd <= 2e-5, ("per-stream EMA vs the numpy chain", "stream", k, "call", call, dd)
    print(f"[vda streams through d2s_pipeline_streams, 1080p, 2 x 40 frames] depth max {worst_d:.2e}; Full-SBS max {worst_lsb} LSB; "
          f"per-stream EMA vs the numpy chain max {worst_e:.2e}")
    eng_b.close()


def test_stream_errors_and_memory(dev):
    """Bad stream tables raise and launch nothing -- the engine still works afterwards -- and N stream slots share one set of weights."""
    from desktop2stereo_amd import _lib, ops
    from desktop2stereo_amd.config import MODELS
    from desktop2stereo_amd.vda_weights import make_vda_weights
    from desktop2stereo_amd.weights import make_weights
    cfg = MODELS["tiny"]
    wts = make_vda_weights(cfg, 0)
    xs = [_t(x, dev) for x in _tiny_inputs(90, 160, 84, 50, 6)]
    eng = ops.Engine(cfg, wts, 42, 84, 4, "fp32", temporal=True)
    one = ops.Engine(cfg, wts, 42, 84, 1, "fp32", temporal=True)
    assert eng.memory_bytes() < 4 * one.memory_bytes()
    x2 = torch.stack(xs[:2])
    first = eng(x2, streams=[2, 0]).cpu().numpy()
    for bad in ([1, 1], [0, 4], [-1, 2]):
        with pytest.raises(_lib.D2SError):
            eng(x2, streams=bad)
    with pytest.raises(_lib.D2SError):
        eng.reset_stream(7)
    with pytest.raises(_lib.D2SError):
        eng(torch.stack(xs[:5]))                                  # batch > max_batch
    with pytest.raises(ValueError):
        eng(x2, streams=[0])                                      # one id for two frames
    # none of the refused calls advanced a stream: streams 2 and 0 continue as a pair of single-stream engines would
    second = eng(torch.stack(xs[2:4]), streams=[2, 0]).cpu().numpy()
    for r in range(2):
        one.reset_stream()
        ref0 = one(xs[r][None]).cpu().numpy()[0]
        ref1 = one(xs[2 + r][None]).cpu().numpy()[0]
        rng = max(1.0, float(ref1.max()))
        assert np.abs(first[r] - ref0).max() / rng <= 2e-5 and np.abs(second[r] - ref1).max() / rng <= 2e-5
    eng.close()
    one.close()
    dcfg = MODELS["tiny"]
    da = ops.Engine(dcfg, make_weights(dcfg, 0), 42, 84, 2, "fp32")
    with pytest.raises(_lib.D2SError):
        da(x2, streams=[0, 1])                                    # batch rows of a Depth-Anything-v2 engine are not streams
    assert da(x2).shape == (2, 42, 84)
    da.close()
