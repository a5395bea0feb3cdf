#!/usr/bin/env python
"""The movie-crop detector (d2s_crop_detect, csrc/crop_detect.hip) alone: event-bracketed us per call at 1080p and 4K, batch 1 / 8 / 32,
set against the op sequence the reference's tensor path issues for ONE frame (xr_viewer/crop.py:386-413: two gathers, luma, mean,
std, cumprod + flip + sum run lengths, the centre vote, stack -- restated here with torch ops) on the same GPU in the same run.
    python tools/crop_bench.py [--sizes 1080x1920 2160x3840] [--batch 1 8 32] [--iters 200] [--json FILE]
The expectation to confirm or refute: a launch-floor-class time, independent of the frame size (the sample grid is ~92 k samples
whatever the frame).  The detector is two launches per call whatever the batch; the torch sequence's launch count is taken from
torch.profiler where that works."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from desktop2stereo_amd import crop as K, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", nargs="+", default=["1080x1920", "2160x3840"])
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = torch.device("cuda")


def torch_sequence(rgb, plan):
    """One CHW uint8 frame -> the six numbers, op for op as the reference's tensor path orders them."""
    sample = rgb.index_select(1, plan["y_idx"])[:, :, plan["x0"]:plan["x1"]:plan["step_x"]].float()
    luma = sample[0] * 0.2126 + sample[1] * 0.7152 + sample[2] * 0.0722
    row_mean, row_std = luma.mean(dim=1), luma.std(dim=1)
    uniform = (row_std < 6.0).to(torch.int32)
    top = torch.cumprod(uniform, dim=0).sum().float()
    bottom = torch.cumprod(torch.flip(uniform, dims=(0,)), dim=0).sum().float()
    bright = (luma > 20.0).float().mean(dim=1)
    cm = (row_mean * plan["mask"]).sum() / plan["count"]
    cb = (bright * plan["mask"]).sum() / plan["count"]
    cs = rgb[:, plan["y0_col"]:plan["y1_col"]:plan["step_y"], :].index_select(2, plan["x_idx"]).float()
    cl = cs[0] * 0.2126 + cs[1] * 0.7152 + cs[2] * 0.0722
    ucol = (cl.std(dim=0) < 6.0).to(torch.int32)
    left = torch.cumprod(ucol, dim=0).sum().float()
    right = torch.cumprod(torch.flip(ucol, dims=(0,)), dim=0).sum().float()
    return torch.stack((top, bottom, cm, cb, left, right))


def timed(fn, iters):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type.name == "CUDA" and "memcpy" not in e.name.lower())
    except Exception:
        return None


results = []
for size in a.sizes:
    H, W = (int(v) for v in size.split("x"))
    bar = int(round((H - W / 2.39) / 2))
    img = synth.letterbox_frame(H, W, 13, top=bar, bottom=bar)
    p = K.sample_plan(W, H)
    mask = torch.tensor(p["center_mask"], dtype=torch.float32, device=dev)
    plan = dict(p, y_idx=torch.tensor(p["y_rows"], device=dev), x_idx=torch.tensor(p["x_cols"], device=dev), mask=mask,
                count=mask.sum().clamp_min(1.0))
    chw = torch.from_numpy(img).to(dev).permute(2, 0, 1).contiguous()
    ref = torch_sequence(chw, plan).cpu().numpy()
    t_ref = timed(lambda: torch_sequence(chw, plan), a.iters)
    n_ref = launches(lambda: torch_sequence(chw, plan))
    for B in a.batch:
        for name, f in (("u8_chw", chw[None].expand(B, -1, -1, -1).contiguous()),
                        ("u8_hwc", torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous())):
            out = torch.empty((B, 6), dtype=torch.float32, device=dev)
            got = ops.crop_detect(f, out=out).cpu().numpy()
            assert np.array_equal(got[0, [0, 1, 4, 5]], ref[[0, 1, 4, 5]]) and abs(got[0, 2] - ref[2]) < 4e-3, (got[0], ref)
            us = timed(lambda: ops.crop_detect(f, out=out), a.iters)
            r = dict(size=size, batch=B, fmt=name, us_per_call=us, us_per_frame=us / B, launches_per_call=2,
                     torch_sequence_us_per_frame=t_ref, torch_sequence_launches=n_ref, crop=list(K.crop_from_stats(got[0].tolist(), W, H)))
            results.append(r)
            print(f"{size} B={B:2d} {name}: detector {us:7.1f} us / call ({us / B:6.2f} us / frame, 2 launches)   torch op sequence "
                  f"{t_ref:7.1f} us / frame ({n_ref} launches)   crop {r['crop']}", flush=True)
if a.json:
    with open(a.json, "w") as fh:
        json.dump(results, fh, indent=1)
