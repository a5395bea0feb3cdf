"""GPU: the OpenXR viewer's letterbox / pillarbox detector (csrc/crop_detect.hip, ops.crop_detect; reference xr_viewer/crop.py:298-435).

PINNED by tests/golden/crop_detect.npz: the six numbers the reference's own tensor path gives on seeded letterboxed frames
(make_golden_crop_detect.py; every sampled line's std is outside [4, 8] there and the centre vote is not within 10 % of its
thresholds, so the reference is unambiguous on every case).  The four run lengths must be EXACT.  center_mean within 4e-3 and
center_bright within 2e-5: the fp32 accumulation bound over <= 255 samples and <= 110 centre rows, 255 * (255 + 110) * 2^-24 with the
factor for scale, on a 0..255 and a 0..1 quantity (the reference sums in another order).  Then crop_from_stats equals the recorded
crop.  All three frame formats, batch 1 and a batch of three different frames."""
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


@pytest.fixture(scope="module")
def cases(golden_dir):
    from desktop2stereo_amd import synth
    with open(os.path.join(golden_dir, "crop_detect.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(golden_dir, "crop_detect.npz"))
    return [dict(c, img=synth.letterbox_frame(c["h"], c["w"], c["seed"], **c["frame"]), stats=z[c["name"] + "_stats"]) for c in meta["cases"]]


def _as(img, fmt, dev):
    """img uint8 [..,H,W,3] -> the device tensor of one of the three formats"""
    t = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    if fmt == "u8_hwc":
        return t
    t = t.movedim(-1, -3).contiguous()
    return t if fmt == "u8_chw" else t.float()


def _check(c, got, what):
    from desktop2stereo_amd import crop as K
    want = c["stats"]
    print(f"[crop_detect {what}] got {got.tolist()} want {want.tolist()}")
    assert [float(got[i]) for i in (0, 1, 4, 5)] == [float(want[i]) for i in (0, 1, 4, 5)], (what, got.tolist(), want.tolist())
    assert abs(float(got[2]) - want[2]) <= 4e-3, (what, "center_mean", float(got[2]), float(want[2]))
    assert abs(float(got[3]) - want[3]) <= 2e-5, (what, "center_bright", float(got[3]), float(want[3]))
    assert tuple(K.crop_from_stats(got.tolist(), c["w"], c["h"])) == tuple(c["crop"]), (what, got.tolist(), c["crop"])


@pytest.mark.parametrize("fmt", ["u8_hwc", "u8_chw", "f32_chw"])
def test_every_fixture_case_batch_1(dev, cases, fmt):
    from desktop2stereo_amd import ops
    assert len(cases) >= 15
    for c in cases:
        got = ops.crop_detect(_as(c["img"], fmt, dev))
        assert got.shape == (6,) and got.dtype == torch.float32
        _check(c, got.cpu().numpy(), (c["name"], fmt))


@pytest.mark.parametrize("fmt", ["u8_hwc", "u8_chw", "f32_chw"])
def test_batches_of_three_different_frames(dev, cases, fmt):
    """Every shape's cases three at a time (wrapping round), frame b's numbers in row b; the same workspace a second time gives the
    same bits."""
    from desktop2stereo_amd import ops
    shapes = sorted({(c["h"], c["w"]) for c in cases})
    assert len(shapes) == 5
    for hw in shapes:
        group = [c for c in cases if (c["h"], c["w"]) == hw]
        assert len(group) >= 3
        for k in range(0, len(group), 2):
            trio = [group[(k + i) % len(group)] for i in range(3)]
            f = _as(np.stack([c["img"] for c in trio]), fmt, dev)
            got = ops.crop_detect(f)
            assert got.shape == (3, 6)
            again = ops.crop_detect(f)
            for b, c in enumerate(trio):
                _check(c, got[b].cpu().numpy(), (c["name"], fmt, "batch row", b))
            assert np.array_equal(got.cpu().numpy().view(np.uint32), again.cpu().numpy().view(np.uint32)), (hw, fmt, "second call")


def test_movie_crop_update_and_poll_deliver_the_crop_without_blocking(dev, cases):
    """MovieCrop.update launches on the current stream and returns with the result still in flight (a long-running kernel is queued
    ahead of it on that stream: the event cannot have fired); poll() never waits; once the stream has drained, poll() applies it."""
    from desktop2stereo_amd import crop as K
    c = next(c for c in cases if c["name"] == "hd_239")
    f = _as(c["img"], "u8_chw", dev)
    now = [10.0]
    mc = K.MovieCrop(interval=1.0, clock=lambda: now[0])
    busy = torch.empty((8192, 8192), device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(4):
        busy = busy @ busy.clamp(-1e-3, 1e-3)              # ~ tens of milliseconds of queued work in front of the detector
    assert mc.update(f) and mc.pending
    in_flight = mc.poll()                                   # no wait: True while the stream is still busy
    assert mc.crop_uv == K.FULL or not in_flight
    torch.cuda.synchronize(dev)
    assert in_flight, "update() or poll() waited for the GPU"
    assert mc.poll() is False and not mc.pending
    assert tuple(mc.crop_uv) == tuple(c["crop"]) and mc.target_active
    now[0] += 0.5
    assert not mc.update(f)                                 # inside the interval
    now[0] += 1.0
    full = next(c for c in cases if c["name"] == "hd_full")
    for _ in range(3):                                      # three full-frame detections in a row: back to the full frame
        assert tuple(mc.crop_uv) == tuple(c["crop"])
        assert mc.update(_as(full["img"], "u8_hwc", dev))
        torch.cuda.synchronize(dev)
        assert mc.poll() is False
        now[0] += 2.0
    assert mc.crop_uv == K.FULL and not mc.target_active


def test_detector_refuses_small_frames_and_a_wrong_out(dev):
    from desktop2stereo_amd import _lib, ops
    with pytest.raises(_lib.D2SError):
        ops.crop_detect(torch.zeros((48, 160, 3), dtype=torch.uint8, device=dev))          # the reference samples nothing below 64
    with pytest.raises(ValueError):
        ops.crop_detect(torch.zeros((2, 96, 160, 3), dtype=torch.uint8, device=dev), out=torch.empty(6, device=dev))
