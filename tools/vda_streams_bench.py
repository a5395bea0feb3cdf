#!/usr/bin/env python
"""N Video-Depth-Anything streams on one MI355X: (A) N single-stream engines called round robin on one HIP stream -- the only way
before stream slots -- against (B) ONE engine with N stream slots advancing all N streams per call; for N in {2, 4} also (A') the N
engines on N HIP streams (information only).  bf16, 1080p noise frames resident in HBM, Full-SBS uint8 out through the pipeline entry
point, EMA off.  A and B alternate (A B A B A B) in this process; every timed window is >= --window seconds after every shape has been
warmed, with a device synchronise on both sides.  Prints ONE JSON line; exit status 1 when a gate fails:
  gate 1: B at N = 1 lies within A's own spread at N = 1 (the stream form costs a single stream nothing);
  gate 2: B's aggregate frames/s at N = 8 exceeds A's by more than the larger of the two spreads, for every model.
    python tools/vda_streams_bench.py [--models vits:336,vitb:518] [--streams 1,2,4,8,16] [--window 2.0]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from desktop2stereo_amd import ops, synth
from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
from desktop2stereo_amd.vda_weights import make_vda_weights

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="vits:336,vitb:518")
ap.add_argument("--streams", default="1,2,4,8,16")
ap.add_argument("--window", type=float, default=2.0)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("vda_streams_bench: no ROCm device (and there is no fallback)")
H, W, mode = 1080, 1920, "Full-SBS"
NS = [int(n) for n in a.streams.split(",")]
dev = torch.device("cuda", 0)
frames = torch.from_numpy(np.stack([synth.noise_frame(H, W, i) for i in range(max(NS))])).to(dev)


def window(step, n_frames):
    """frames/s over >= a.window seconds of step() calls, synchronised on both sides"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    calls = 0
    while True:
        for _ in range(8):
            step()
        calls += 8
        if time.perf_counter() - t0 >= a.window:
            break
    torch.cuda.synchronize()
    return calls * n_frames / (time.perf_counter() - t0)


def summary(vals):
    return {"values": [round(v, 1) for v in vals], "median": round(statistics.median(vals), 1), "spread": round(max(vals) - min(vals), 1)}


def launches(engine, step):
    engine.profile(True)
    step()
    torch.cuda.synchronize()
    n = sum(int(v["launches"]) for v in engine.profile_read().values())
    engine.profile(False)
    return n


result = {"tool": "vda_streams_bench", "frames": f"{H}x{W} noise", "mode": mode, "precision": "bf16", "window_s": a.window, "cells": {}, "gates": {}}
ok = True
for spec in a.models.split(","):
    name, res = spec.split(":")
    res = int(res)
    cfg = MODELS[name]
    h, w, _ = engine_shape(H, W, res)
    wts = make_vda_weights(cfg, 0)
    p = PipelineParams(depth_resolution=res, display_mode=mode)
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, mode, p.fill_16_9)
    oh, ow = ops.sbs_shape(H, W, sp)
    cells = {}
    for N in NS:
        singles = [ops.Engine(cfg, wts, h, w, 1, "bf16", temporal=True) for _ in range(N)]
        multi = ops.Engine(cfg, wts, h, w, N, "bf16", temporal=True)
        outs = [torch.empty((1, oh, ow, 3), dtype=torch.uint8, device=dev) for _ in range(N)]
        out_b = torch.empty((N, oh, ow, 3), dtype=torch.uint8, device=dev)
        fr = [frames[k:k + 1] for k in range(N)]
        fr_b = frames[:N]
        ids = list(range(N))

        def step_a():
            for k in range(N):
                singles[k].pipeline(fr[k], p, sp, use_ema=False, out=outs[k])

        def step_b():
            multi.pipeline(fr_b, p, sp, use_ema=False, out=out_b, streams=ids)

        hip_streams = [torch.cuda.Stream() for _ in range(N)] if N in (2, 4) else None

        def step_a2():
            for k in range(N):
                with torch.cuda.stream(hip_streams[k]):
                    singles[k].pipeline(fr[k], p, sp, use_ema=False, out=outs[k])

        for _ in range(40):                     # past the first-frame fill and the window wrap, every shape warm
            step_a(); step_b()
        torch.cuda.synchronize()
        va, vb = [], []
        for _ in range(a.repeats):
            va.append(window(step_a, N))
            vb.append(window(step_b, N))
        cell = {"A": summary(va), "B": summary(vb),
                "memory_bytes": {"A": sum(e.memory_bytes() for e in singles), "B": multi.memory_bytes()},
                "launches_per_call": {"A": N * launches(singles[0], lambda: singles[0].pipeline(fr[0], p, sp, use_ema=False, out=outs[0])),
                                      "B": launches(multi, step_b)}}
        if hip_streams:
            for _ in range(5):
                step_a2()
            cell["A_n_hip_streams"] = summary([window(step_a2, N) for _ in range(a.repeats)])
        cells[str(N)] = cell
        print(f"[{name}@{res} N={N}] A {cell['A']['median']} (+-{cell['A']['spread']}) B {cell['B']['median']} (+-{cell['B']['spread']}) frames/s aggregate; "
              f"launches per call A {cell['launches_per_call']['A']} B {cell['launches_per_call']['B']}", file=sys.stderr, flush=True)
        for e in singles + [multi]:
            e.close()
        del singles, multi, outs, out_b
        torch.cuda.empty_cache()
    result["cells"][f"{name}@{res}"] = cells
    if "1" in cells:
        c = cells["1"]
        g1 = abs(c["B"]["median"] - c["A"]["median"]) <= c["A"]["spread"]
        result["gates"][f"{name}@{res} gate1 (B within A's spread at N=1)"] = bool(g1)
        ok &= bool(g1)
    if "8" in cells:
        c = cells["8"]
        g2 = c["B"]["median"] - c["A"]["median"] > max(c["A"]["spread"], c["B"]["spread"])
        result["gates"][f"{name}@{res} gate2 (B beats A at N=8 by more than the spreads)"] = bool(g2)
        ok &= bool(g2)
print(json.dumps(result))
sys.exit(0 if ok else 1)
