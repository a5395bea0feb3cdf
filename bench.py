#!/usr/bin/env python
"""Throughput bench of the hot path: stereo frames/s, 1080p, Depth-Anything-v2 ViT-B, Full-SBS.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1 with WORLD_SIZE unset: bench.py re-launches itself as N ranks (one per GPU) under torch.distributed.run on
127.0.0.1; launched BY torch.distributed.run (the driver's way) it reads RANK / LOCAL_RANK / WORLD_SIZE from the env.

One step = one pass of predict_depth + make_sbs (d2s_pipeline) over one batch of synthetic uint8 frames already
resident in HBM.  Workload = BASELINE.json configs[1]: DA-v2 ViT-B bf16, 1920x1080, batch 1, Full-SBS, Depth
Resolution 518 (model input 294x518), seeded synthetic weights.  Frames shard across ranks with no data-path
collective (weak scaling: per-GPU work fixed).

A plain run builds the engine, runs W untimed and K timed steps, writes --dump-outputs if given, and rank 0 prints ONE
JSON line: the contract fields (metric, value, unit, ms_per_step, ..., rccl_ranks = the number of ranks an actual
all-reduce counted).  --full then runs every other measurement, each in runs of its own, and adds
  roofline      -- the dominant kernel class, timed live with HIP events on the launch stream
                   (d2s_engine_profile) in a second pass over the same workload;
  kernels       -- the same numbers for every kernel class;
  roofline_warp -- the stereo-warp kernel against the HBM roofline;
  ingest_rank0  -- the other deployment SURVEY.md section 8(e) asks to report: rank 0 holds all frames, scatters uint8
                   frames / gathers packed stereo frames point-to-point over RCCL (shard.scatter_frames / gather_outputs)
                   (--ingest rank0 makes this leg the headline, with or without --full);
  batched       -- (N=1 only) the same pipeline at --also-batch frames per step (throughput regime:
                   M = batch*778 tokens fills the chip), with its own roofline;
  parity_class  -- (N=1 only) the same step on the fp32 engine, the one that meets north_star's 1e-3 depth tolerance;
  cpu_baseline  -- the numpy oracle (a port of the reference's CPU path) on a bounded sample,
                   rank 0 at N=1 only: all host threads, and one thread (the reference ships torch.set_num_threads(1),
                   depth.py:19);
  and the parity figures against the committed reference fixtures, the MJPEG sink, the f1 DIBR warp and BASELINE
  configs 1, 3 and 4 (see rank_body).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
# Kernel arguments in device memory (the HIP runtime reads this when it is loaded, i.e. before `import torch`).  It is the default of the
# ROCm 7.2 image; pinned here because the batch-1 frame is a chain of ~85 dependent launches and the other setting costs 7 % of it
# (same-box A/B, tools/ab_env.sh: 817-821 against 878-882 frames/s).
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

# dense MFMA peaks, MI355X_MICROARCH.md.  "fp8": from round 5 the batched e4m3 linears (gemm_pp) run the scaled K=64 instruction
# v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales), which issues at twice the bf16 rate -> priced against the 5 PF dense fp8 peak.
# (The small-batch tiles of gemm_glds still use the non-scaled v_mfma_f32_16x16x32_fp8_fp8 = the bf16 rate; pricing them against
# 5 PF too is the conservative side.)
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "fp8": 5000.0, "bf16x3": 2500.0 / 3}      # bf16x3: three bf16 MFMAs per product
PEAK_HBM_GBS = 8000.0                          # HBM3E spec
SURVEY_GF_PER_FRAME = {("vitb", 518): 176.9, ("vits", 518): 45.8, ("vitl", 518): 635.9,
                       ("vitb", 336): 76.5, ("vits", 336): 19.8, ("vitl", 336): 275.2}


def cpu_baseline(cfg, weights, p, H, W, mode, budget_s=10.0, max_frames=3):
    """The oracle (numpy port of the reference CPU path) timed on this host's cores: all threads, then one thread."""
    from desktop2stereo_amd import synth
    from oracle import d2s_oracle as O
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    except Exception:
        threadpool_limits = None
        threads = os.cpu_count() or 1
    orc = O.PipelineOracle(cfg, weights, p.depth_resolution, p.foreground_scale, p.aa_strength)

    def run(limit, budget, frames):
        import contextlib
        ctx = threadpool_limits(limits=limit) if (threadpool_limits and limit) else contextlib.nullcontext()
        n, t_total = 0, 0.0
        with ctx:
            while n < frames and t_total < budget:
                frame = synth.noise_frame(H, W, 100 + n)
                t0 = time.perf_counter()
                d = orc.predict_depth(frame)
                orc.make_sbs(frame, d, ipd_uv=p.ipd, depth_ratio=p.depth_strength, convergence=p.convergence,
                             display_mode=mode, fill_16_9=p.fill_16_9)
                t_total += time.perf_counter() - t0
                n += 1
        return n, t_total

    n, t = run(None, budget_s, max_frames)
    ref_note = ""
    try:                                                 # the reference itself, timed in the build container (tests/golden/time_reference.py)
        with open(os.path.join(REPO, "profiles", "r4_reference_cpu_timing.json")) as f:
            rt = json.load(f)
        r1, ra = rt["rows"]["one_thread_as_shipped"], rt["rows"]["all_cores"]
        ref_note = (f" The REFERENCE ITSELF (imported, ViT-B, same workload, bf16 CPU autocast as shipped, median of {r1['frames']} frames after "
                    f"{rt['warmups']} warm-ups) measured in the build container on {rt['cpu_model']}: {r1['frames_per_s']:.3f} frames/s on 1 thread "
                    f"(as shipped, depth.py:19), {ra['frames_per_s']:.3f} frames/s on {ra['threads']} threads (profiles/r4_reference_cpu_timing.json).")
    except (OSError, KeyError, ValueError):
        rt = None
    out = {}
    if rt is not None:
        # FIRST: the reference's own CPU path (what "the reference's CPU path timed beside it" means), measured where it can run --
        # the build container; it cannot travel to this box
        out["reference_itself"] = {"frames_per_s_1_thread_as_shipped": r1["frames_per_s"], "frames_per_s_all_cores": ra["frames_per_s"],
                                   "cores": ra["threads"], "cpu_model": rt["cpu_model"], "where": "build container (profiles/r4_reference_cpu_timing.json)",
                                   "rows": rt["rows"]}
    out.update({"value": n / t, "unit": "stereo frames/s", "cores": int(threads), "kind": "port",
                "sample": f"{n} frame(s) {W}x{H} {cfg.name} fp32 numpy oracle, {mode}, {t:.1f} s of CPU work",
                "host_cpus": os.cpu_count(),
                "note": "value / kind 'port' = the numpy restatement under oracle/ timed on THIS box's host cores (a checker, not a tuned CPU "
                        "implementation: slower than the reference itself per thread); read reference_itself first." + ref_note})
    if threadpool_limits is not None:
        n1, t1 = run(1, budget_s, 1)
        out["one_thread"] = {"value": n1 / t1, "unit": "stereo frames/s", "cores": 1,
                             "sample": f"{n1} frame(s), {t1:.1f} s of CPU work; the reference ships torch.set_num_threads(1) (depth.py:19)"}
    return out


def parity_vs_reference(ops, synth, cfg, weights, p, engines, dev):
    """The second half of BASELINE.json's metric ("...; depth L1 vs ref"), outside every timed region: the committed
    reference-generated fixtures only (no oracle, no /root/reference).
      depth: tests/golden/<model>_r518.npz -- the reference's fp32 CPU path on the seeded structured 1080p frame; post-processed
             depth at model resolution: L1 (mean |diff|) and max |diff| (the depth range is 1) per engine precision;
      warp:  tests/golden/warp.npz -- the reference's make_sbs on a 1080p frame with a GIVEN depth (isolates the warp), every
             135th row stored: max |diff| in uint8 levels after round-half-even, Full-SBS (BASELINE configs[1]'s packing)."""
    import numpy as np
    import torch
    from desktop2stereo_amd.config import engine_shape
    gdir = os.path.join(REPO, "tests", "golden")
    out = {}
    try:
        z = np.load(os.path.join(gdir, f"{cfg.name}_r518.npz"))
        with open(os.path.join(gdir, f"{cfg.name}_r518.json")) as f:
            fr = json.load(f)["frames"][0]
    except OSError:
        return None
    if p.depth_resolution != 518 or p.resample != "bilinear":
        return None
    img = synth.structured_frame(fr["h"], fr["w"], fr["seed"]) if fr["kind"] == "S2" else synth.noise_frame(fr["h"], fr["w"], fr["seed"])
    h, w, _ = engine_shape(fr["h"], fr["w"], 518)
    x = ops.preprocess(torch.from_numpy(img).to(dev), 518)
    ref = z["f0_post_depth"]
    for name, mk in engines.items():
        e = mk(h, w)
        post = ops.post_process_depth(e(x), p).cpu().numpy()[0]
        e.close()
        d = np.abs(post - ref)
        out[name] = {"depth_l1_vs_ref": float(d.mean()), "depth_max_vs_ref": float(d.max())}
    out["depth_fixture"] = f"tests/golden/{cfg.name}_r518.npz: the reference's fp32 CPU path (autocast off), frame {fr['kind']} seed {fr['seed']} {fr['w']}x{fr['h']}, seeded synthetic weights"
    try:
        zw = np.load(os.path.join(gdir, "warp.npz"))
        with open(os.path.join(gdir, "warp.json")) as f:
            cases = [c for c in json.load(f)["cases"] if c["shape"] == "hd" and c["mode"] == "Full-SBS"]
        worst, n = 0, 0
        for c in cases:
            gen = synth.structured_frame if c["kind"] == "S2" else synth.noise_frame
            rgb = torch.from_numpy(gen(c["h"], c["w"], c["seed"])).to(dev)
            dep = torch.from_numpy(synth.smooth_depth(c["h"], c["w"], c["seed"])).to(dev)
            sp = ops.sbs_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], c["mode"], c["fill_16_9"])
            got = ops.make_sbs(rgb, dep, sp).cpu().numpy()[:: c["row_stride"]].astype(np.int32)
            want = np.clip(np.rint(zw[c["key"]].astype(np.float32) / 256.0), 0, 255).astype(np.int32)
            worst = max(worst, int(np.abs(got - want).max()))
            n += 1
        out["warp_max_lsb"] = worst
        # REPORTED, not gated: the reference AS SHIPPED warps in bf16 on its CPU path (rgb cast to the bf16 depth's dtype, depth.py:2209-2215);
        # tests/golden/warp_bf16.npz is that output for the same frames with the bf16-rounded depth (structured frame, Full-SBS cases)
        try:
            zb = np.load(os.path.join(gdir, "warp_bf16.npz"))
            with open(os.path.join(gdir, "warp_bf16.json")) as f:
                mb = json.load(f)
            dep_b = torch.from_numpy(synth.smooth_depth(1080, 1920, 7)).to(torch.bfloat16).float().to(dev)
            mx, over, tot = 0, 0, 0
            for c in mb["cases"]:
                if c["mode"] != "Full-SBS" or c["kind"] != "S2":
                    continue
                rgb = torch.from_numpy(synth.structured_frame(c["h"], c["w"], c["seed"])).to(dev)
                sp = ops.sbs_params(c["ipd_uv"], c["depth_ratio"], c["convergence"], c["mode"], c["fill_16_9"])
                got = ops.make_sbs(rgb, dep_b, sp).cpu().numpy()[:: c["row_stride"]].astype(np.int32)
                want = np.clip(np.rint(zb[c["key"]].astype(np.float32) / 256.0), 0, 255).astype(np.int32)
                d = np.abs(got - want)
                mx, over, tot = max(mx, int(d.max())), over + int((d > 1).sum()), tot + d.size
            out["warp_vs_reference_as_shipped_bf16"] = {"max_lsb": mx, "frac_over_1_lsb": over / max(tot, 1), "note": (
                "reported, not gated: the reference's own bf16 warp rounds depth and every output value to 8 significant bits; the HIP warp "
                "is fp32 from the same bf16-rounded depth (tests/golden/warp_bf16.npz, structured 1080p frame, Full-SBS cases)")}
        except OSError:
            pass
        out["warp_fixture"] = f"tests/golden/warp.npz: {n} Full-SBS cases of the reference's make_sbs at 1920x1080 (given depth, every 135th row)"
    except OSError:
        pass
    return out


_PMC_CACHE = {}


def pmc_traffic_file():
    """profiles/pmc_traffic.json + whether it describes THIS tree: the file records the sha256 of the kernel sources its rocprofv3 --pmc
    passes ran on (tools/pmc_traffic.sh); a different digest here means the figures are of other code and are refused."""
    if "doc" not in _PMC_CACHE:
        doc, src = None, {"file": "profiles/pmc_traffic.json", "commit": None, "date": None, "status": "missing"}
        try:
            with open(os.path.join(REPO, "profiles", "pmc_traffic.json")) as f:
                doc = json.load(f)
            from desktop2stereo_amd.build import kernel_sources_digest
            here = kernel_sources_digest()
            src.update(commit=doc.get("commit"), date=doc.get("date_utc"), kernel_sources_sha256=doc.get("kernel_sources_sha256"))
            if doc.get("kernel_sources_sha256") == here:
                src["status"] = "ok: separate rocprofv3 --pmc passes (FETCH_SIZE / WRITE_SIZE, calibrated) of this tree's kernel sources; not collected by this run"
            else:
                src["status"] = "stale: the kernel sources changed since the PMC passes -- figure withheld (re-run tools/profile_round.sh)"
                doc = None
        except (OSError, ValueError):
            pass
        _PMC_CACHE["doc"], _PMC_CACHE["src"] = doc, src
    return _PMC_CACHE["doc"], _PMC_CACHE["src"]


def pmc_traffic(kernel_class, B, default_workload):
    """HBM-side bytes per launch from the committed PMC profile: FETCH_SIZE / WRITE_SIZE are collected in separate
    rocprofv3 --pmc passes of tools/pmc_run.sh and reduced by tools/pmc_traffic.py (FETCH_SIZE doubled per the guide's gfx950
    correction, WRITE_SIZE scaled by the calibration copy) -- they cannot be read inside this process; only for the
    workload the profile was taken on (ViT-B bf16, Depth Resolution 518) and only while the file's kernel-source digest is this
    tree's (pmc_traffic_file), else None."""
    if not default_workload:
        return None
    doc, _ = pmc_traffic_file()
    try:
        return doc["traffic_bytes_per_launch"][kernel_class].get(str(B)) if doc else None
    except KeyError:
        return None


def profile_pass(eng, step, steps, B, precision, sync, default_workload=False):
    """Second pass with HIP events around every kernel launch -> per-class table + roofline objects."""
    eng.profile(True)
    for i in range(steps):
        step(i)
    sync()
    prof = eng.profile_read()
    eng.profile(False)
    nf = steps * B
    kernels = {}
    for name, r in prof.items():
        if not r["launches"]:
            continue
        k = {"launches_per_step": r["launches"] / steps, "ms_per_step": r["ms"] / steps, "avg_launch_us": 1e3 * r["ms"] / r["launches"]}
        if r["flops"]:
            k["gflop_per_frame"] = r["flops"] / nf / 1e9
            k["tflops"] = r["flops"] / (r["ms"] * 1e-3) / 1e12
            k["frac_of_mfma_peak"] = k["tflops"] / PEAK_TFLOPS[precision]
        if r["bytes"]:
            k["mb_per_frame"] = r["bytes"] / nf / 1e6
            k["gbs"] = r["bytes"] / (r["ms"] * 1e-3) / 1e9
            k["frac_of_hbm_peak"] = k["gbs"] / PEAK_HBM_GBS
        kernels[name] = k
    out = {"kernels": kernels, "gpu_busy_ms_per_step": sum(k["ms_per_step"] for k in kernels.values()),
           "launches_per_step": sum(k["launches_per_step"] for k in kernels.values())}
    dom = max(kernels, key=lambda n: kernels[n]["ms_per_step"])
    kd = kernels[dom]
    if "tflops" in kd:
        out["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": kd["tflops"], "peak": PEAK_TFLOPS[precision], "unit": "TFLOP/s",
                           "frac": kd["frac_of_mfma_peak"], "traffic": pmc_traffic(dom, B, default_workload), "traffic_source": pmc_traffic_file()[1],
                           "flop_per_launch": 1e9 * kd["gflop_per_frame"] * B / kd["launches_per_step"], "avg_launch_us": kd["avg_launch_us"]}
    else:
        out["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": kd.get("gbs"), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                           "frac": kd.get("frac_of_hbm_peak"), "traffic": pmc_traffic(dom, B, default_workload), "traffic_source": pmc_traffic_file()[1],
                           "avg_launch_us": kd["avg_launch_us"]}
    if "stereo_warp" in kernels:
        kw = kernels["stereo_warp"]
        out["roofline_warp"] = {"kernel": "stereo_warp", "bound": "hbm", "achieved": kw["gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                "frac": kw["frac_of_hbm_peak"], "traffic": pmc_traffic("stereo_warp", B, default_workload), "traffic_source": pmc_traffic_file()[1],
                                "bytes_per_launch": 1e6 * kw["mb_per_frame"] * B, "avg_launch_us": kw["avg_launch_us"]}
    out["model_gflop_per_frame_counted"] = sum(k.get("gflop_per_frame", 0.0) for k in kernels.values())
    return out


def tile_fit_batch(tokens, hidden, mlp, upper, ncu=256):
    """Largest-efficiency batch in (upper/2, upper]: flop-weighted fraction of busy CU-rounds of the four encoder linears
    (QKV, proj, FC1, FC2) when each runs as ceil(tokens*B/256) x N/256 tiles, one tile per CU per round."""
    best, best_eff = upper, -1.0
    for B in range(upper, upper // 2, -1):
        tm = -(-tokens * B // 256)
        num = den = 0.0
        for N, K in ((3 * hidden, hidden), (hidden, hidden), (mlp, hidden), (hidden, mlp)):
            tiles = tm * -(-N // 256)
            rounds = -(-tiles // ncu)
            num += (tokens * B / (tm * 256.0)) * tiles * K          # useful tile-K work
            den += rounds * ncu * K                                  # CU-rounds paid for
        eff = num / den
        if eff > best_eff + 1e-9:
            best, best_eff = B, eff
    return best


def _r(x, sig=5):
    """floats to `sig` significant digits (the compact line is bounded in bytes)."""
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(res: dict, full_path: str) -> dict:
    """The one stdout line: contract keys, roofline (dominant class) + warp roofline, cpu_baseline, parity figures and one number per
    sub-run; everything else (per-class kernel tables, workload prose, traffic provenance) is in the full report at `full_path`."""
    RF = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us")
    out = _pick(res, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                      "dtype", "data", "rccl_ranks"))
    cfg = res.get("config", {})
    out["config"] = {"workload": str(cfg.get("workload", ""))[:160], **_pick(cfg, ("frames_per_step_per_gpu", "timed_region", "parallelism"))}
    for k in ("roofline", "roofline_warp"):
        if k in res:
            out[k] = _pick(res[k], RF)
            ts = res[k].get("traffic_source")
            if k == "roofline" and isinstance(ts, dict):
                out[k]["traffic_source"] = _pick(ts, ("file", "commit", "date"))
    cb = res.get("cpu_baseline")
    if isinstance(cb, dict):
        out["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "sample"))
        ri = cb.get("reference_itself")
        if isinstance(ri, dict):
            out["cpu_baseline"]["reference_itself"] = _pick(ri, ("frames_per_s_1_thread_as_shipped", "frames_per_s_all_cores", "cores", "cpu_model", "where"))
    out.update(_pick(res, ("depth_l1_vs_ref", "depth_max_vs_ref", "warp_max_lsb", "launches_per_step", "gpu_busy_ms_per_step", "hip_force_dev_kernarg")))
    pc = res.get("parity_class")
    if isinstance(pc, dict):
        out["parity_class"] = _pick(pc, ("value", "dtype", "ms_per_step", "depth_l1_vs_ref", "depth_max_vs_ref"))
    for k in ("batched", "batched_tile_fit"):
        b = res.get(k)
        if isinstance(b, dict):
            o = _pick(b, ("value", "frames_per_step", "ms_per_step"))
            o["roofline"] = _pick(b.get("roofline", {}), ("kernel", "achieved", "frac", "avg_launch_us"))
            o["roofline_warp"] = _pick(b.get("roofline_warp", {}), ("achieved", "frac", "avg_launch_us"))
            if k == "batched":
                o["kernels"] = {n: _pick(v, ("ms_per_step", "tflops", "frac_of_peak")) for n, v in b.get("kernels", {}).items()
                                if isinstance(v, dict) and ("tflops" in v or "frac_of_peak" in v)}
            out[k] = o
    ks = res.get("kernels")
    if isinstance(ks, dict):
        out["kernels"] = {n: _pick(v, ("launches_per_step", "ms_per_step")) for n, v in ks.items() if isinstance(v, dict)}
    c3 = res.get("config3_vitl_4k_full_tab")
    if isinstance(c3, dict):
        o = {}
        for prec in ("bf16", "fp8", "fp8_mlp"):
            r = c3.get(prec)
            if isinstance(r, dict):
                o[prec] = {"value": r.get("value"), "batch8": r.get("batch8", {}).get("value"), **_pick(r, ("depth_l1_vs_ref", "depth_max_vs_ref"))}
                if "roofline" in r:
                    o[prec]["roofline_frac_batch8"] = r["roofline"].get("frac")
        o.update(_pick(c3, ("fp8_over_bf16", "fp8_over_bf16_batch8")))
        out["config3_vitl_4k_full_tab"] = o
    c4 = res.get("config4_vda")
    if isinstance(c4, dict):
        out["config4_vda"] = {n: _pick(v, ("value", "launches_per_step")) for n, v in c4.items() if isinstance(v, dict)}
    sj = res.get("sink_jpeg")
    if isinstance(sj, dict):
        out["sink_jpeg"] = _pick(sj, ("value", "encode_us_per_frame", "identical_to_libjpeg_turbo"))
    fd = res.get("f1_dibr")
    if isinstance(fd, dict):
        out["f1_dibr_us_per_frame"] = {n: v.get("us_per_frame") for n, v in fd.items() if isinstance(v, dict)}
    hb = res.get("host_boundary")
    if isinstance(hb, dict):
        out["host_boundary"] = {n: v.get("value") for n, v in hb.items() if isinstance(v, dict)} or _pick(hb, ("error",))
    ir = res.get("ingest_rank0")
    if isinstance(ir, dict):
        out["ingest_rank0"] = _pick(ir, ("value", "frames_per_step"))
    out["full_report"] = os.path.relpath(full_path, REPO) if os.path.isabs(full_path) else full_path
    return _r(out)


DUMP_BYTES = 64_000_000


def dump_outputs(out_dir: str, arrays: dict, step: int) -> dict:
    """--dump-outputs: write each array as out_dir/<name>.npy in float32, so that two builds run with the same arguments can be
    compared output for output.  Past DUMP_BYTES in all, each array keeps the same share of its rows (leading axes flattened, the
    last two kept whole), drawn with seed 0 and left in their original order.  -> what was written, for the full report."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.size for a in arrays.values()) * 4
    written = {}
    for name, a in arrays.items():
        entry = {"shape": list(a.shape), "step": step}
        if total > DUMP_BYTES:
            rows = a.reshape((-1,) + a.shape[-2:])
            keep = max(1, len(rows) * DUMP_BYTES // total)
            a = rows[np.sort(np.random.default_rng(0).choice(len(rows), keep, replace=False))]
            entry["sampled_rows"] = {"kept": keep, "of": len(rows), "seed": 0}
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32))
        written[name] = entry
    return {"dir": out_dir, "dtype": "float32", "arrays": written}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1, help="frames per step per GPU (configs[1]: 1)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every other measurement too (profile pass and rooflines, batched sizes, parity "
                         "figures, sink, DIBR, host boundary, CPU baseline, configs 1 / 3 / 4), shaped by --also-batch, --no-tile-fit, "
                         "--profile-steps, --mixed, --sink-quality and the --no-* options.  Without it the run times the headline and "
                         "nothing else")
    ap.add_argument("--also-batch", type=int, default=32, help="extra batched measurement at N=1 (0 = off)")
    ap.add_argument("--no-tile-fit", dest="tile_fit", action="store_false",
                    help="skip the extra batched measurement at the tile-fitting batch size (see tile_fit_batch)")
    ap.add_argument("--model", default="vitb")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp8", "bf16x3"],
                    help="fp8 = BASELINE config 3 (e4m3 encoder linears; try --model vitl --height 2160 --width 3840 --mode Full-TAB)")
    ap.add_argument("--res", type=int, default=518)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--mode", default="Full-SBS")
    ap.add_argument("--resample", default="bilinear", choices=["bilinear", "bicubic_aa"],
                    help="pre-process branch of _resize_patch_aligned_t: the reference's CPU path (default) or its IS_CUDA branch")
    ap.add_argument("--profile-steps", type=int, default=10)
    ap.add_argument("--vda", action="store_true",
                    help="streaming Video-Depth-Anything (BASELINE config 4): one stream per GPU (shard.stream_owner), batch 1, 32-frame window")
    ap.add_argument("--mixed", type=int, default=0,
                    help="extra measurement (N=1): BASELINE config 5, this many frames per step drawn with seed 0 from "
                         "{1280x720, 1920x1080, 2560x1440} -- one batched model pass, per-size pre-process and warp")
    ap.add_argument("--ingest", default="both", choices=["own", "rank0", "both"],
                    help="own: every rank generates its frames (headline value, no data-path collective); rank0: rank 0 holds all "
                         "frames, RCCL point-to-point scatter / gather each step; both: headline = own, rank0 reported beside it "
                         "under --full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity-class", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the depth / warp parity leg against the committed reference fixtures (counter passes)")
    ap.add_argument("--sink-quality", type=int, default=90, help="also time the step with the MJPEG sink behind it (0 = off)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--full-out", default="", help="where the full report goes (default gpurun_out/bench_full.json); stdout carries one compact line")
    ap.add_argument("--no-config3", action="store_true", help="skip the BASELINE configs[2] sub-run (ViT-L, 3840x2160, Full-TAB: bf16 and fp8 engines)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what rank 0's last timed step returned (the packed stereo frames) to DIR/sbs_frames.npy "
                         "as float32; the inputs and weights are seeded, so two builds run with the same arguments compare output for output")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.ingest == "rank0":
        ap.error("--dump-outputs writes the headline step's frames: use --ingest own or both")
    return args


def respawn_as_ranks(n: int):
    """`python bench.py --gpus N` from a plain shell: become N ranks under torch.distributed.run (one process per GPU)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    os.execvpe(cmd[0], cmd, env)


def rank_body(args, engine_factory=None, device=None):
    """What every rank runs.  engine_factory / device are injected only by the gloo rehearsal test (tests/test_shard_gloo.py:
    a stand-in engine on CPU tensors exercises the rank logic -- sharding, scatter / gather, barriers, the max-over-ranks
    clock, rank counting -- without a GPU); bench.py itself never passes them: the product path is the HIP engine or nothing."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from desktop2stereo_amd import shard, synth
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}, "
                         f"or run `python bench.py --gpus {args.gpus}` without WORLD_SIZE set and let it spawn the ranks")
    # D2S_DIST_BACKEND=gloo: rehearsal of the multi-rank path on a box with fewer GPUs than ranks (ranks share devices)
    backend = os.environ.get("D2S_DIST_BACKEND", "nccl")
    fake = engine_factory is not None
    if not fake:
        from desktop2stereo_amd import _lib, ops
        from desktop2stereo_amd.weights import make_weights
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a ROCm device (the HIP path has no fallback)")
        _lib.load()
        ndev = torch.cuda.device_count()
        if backend == "nccl" and ndev < world:
            raise SystemExit(f"--gpus {world} but only {ndev} device(s) visible: one rank per GPU over RCCL needs {world}")
        if backend != "nccl":
            local_rank %= ndev
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        sync = torch.cuda.synchronize
    else:
        dev = device or torch.device("cpu")
        sync = lambda: None
    coll_dev = dev if backend == "nccl" else torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    rccl_ranks = 1
    if world > 1:                                        # count the ranks with a real collective (RCCL when backend == nccl)
        one = torch.ones(1, dtype=torch.int32, device=coll_dev)
        dist.all_reduce(one)
        rccl_ranks = int(one.item())
        if rccl_ranks != world:
            raise SystemExit(f"all-reduce counted {rccl_ranks} ranks, expected {world}")

    cfg = MODELS[args.model]
    H, W, B = args.height, args.width, args.batch
    B2 = args.also_batch if (world == 1 and args.also_batch > B) else 0
    p = PipelineParams(depth_resolution=args.res, display_mode=args.mode, resample=args.resample)
    h, w, _ = engine_shape(H, W, args.res)
    NM = args.mixed if (world == 1 and not args.vda) else 0
    if args.vda and B != 1:
        raise SystemExit("--vda is one stream per GPU: --batch must be 1")
    if args.vda:
        B2 = 0
    if fake:
        weights = None
        eng = engine_factory(max(B, B2, NM))
        sbs_params_, sbs_shape_ = eng.sbs_params, eng.sbs_shape
    else:
        if args.vda:
            from desktop2stereo_amd.vda_weights import make_vda_weights
            weights = make_vda_weights(cfg, 0)
        else:
            weights = make_weights(cfg, 0)
        # sized for the --full sub-runs whether or not they run: the headline steps run on the same engine either way
        eng = ops.Engine(cfg, weights, h, w, max_batch=max(B, B2, NM), precision=args.precision, device=local_rank, temporal=args.vda)
        sbs_params_, sbs_shape_ = ops.sbs_params, ops.sbs_shape
    default_wl = (args.model, args.precision, args.res, H, W, args.vda, args.resample) == ("vitb", "bf16", 518, 1080, 1920, False, "bilinear")
    if args.precision == "fp8" and not fake:     # static activation scales from two structured frames (outside the timed region)
        eng.calibrate(torch.cat([ops.preprocess(torch.from_numpy(synth.structured_frame(H, W, s)).to(dev), args.res, resample=args.resample)
                                 for s in (0, 1)][:max(B, B2)]))
    sp = sbs_params_(p.ipd, p.depth_strength, p.convergence, args.mode, p.fill_16_9)
    oh, ow = sbs_shape_(H, W, sp)
    # config 4: stateful streams never split -- stream s lives on rank shard.stream_owner(s, world); with `world` streams that
    # is one stream per rank, and this rank serves the stream(s) it owns
    my_streams = [s for s in range(world) if shard.stream_owner(s, world) == rank] if args.vda else []
    if args.vda and my_streams != [rank]:
        raise SystemExit(f"stream_owner put streams {my_streams} on rank {rank}")

    def frames_for(seed0, nb):
        return torch.from_numpy(np.stack([synth.noise_frame(H, W, seed0 + i) for i in range(nb)]))

    def make_step(nb, engine=None):
        engine = engine or eng
        # a small pool of distinct batches, resident in HBM before the timed region
        pool = [frames_for(1000 * rank + 100 * j, nb).to(dev) for j in range(4 if nb <= 4 else 2)]
        out = torch.empty((nb, oh, ow, 3), dtype=torch.uint8, device=dev)

        def step(i):
            return engine.pipeline(pool[i % len(pool)], p, sp, use_ema=False, out=out)
        step.out = out                                   # every call writes here: after a timed run it holds the last step's frames
        return step

    def barrier():
        if world > 1:
            dist.barrier()
        sync()

    def timed(step, warmup, steps):
        """W untimed steps, then exactly K steps bracketed by barrier + synchronize on both sides; MAX over ranks."""
        for i in range(warmup):
            step(i)
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            barrier()
        return dt

    def workload(nb, prec=None):
        return (f"DepthAnything-v2-{cfg.name} {prec or args.precision}, {W}x{H} uint8 RGB noise frames, batch {nb} per GPU, "
                f"Depth Resolution {args.res} (model input {h}x{w}), {args.mode} uint8 output {ow}x{oh}, "
                f"predict_depth + make_sbs fused (d2s_pipeline), EMA off, seeded synthetic weights; "
                f"timed region: HBM-resident uint8 frames in -> HBM-resident uint8 packed frame out (no H2D / D2H; the reference's make_sbs "
                f"ends with a host float32 array, depth.py:2231)"
                + (", IS_CUDA-branch pre-process (bicubic + antialias)" if args.resample == "bicubic_aa" else ""))

    result = {"metric": "stereo frames/sec @1080p DepthAnything-v2-ViT-B", "unit": "stereo frames/s", "n_gpus": world,
              "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
              "dtype": args.precision, "data": "synthetic", "rccl_ranks": rccl_ranks,
              "hip_force_dev_kernarg": os.environ.get("HIP_FORCE_DEV_KERNARG", "unset"),
              "config": {"workload": workload(B), "frames_per_step_per_gpu": B,
                         "timed_region": "HBM-resident uint8 in -> HBM uint8 out (no H2D/D2H)", "precision_class": (
                             "bf16 operands, fp32 accumulate / residual: graded against the reference's own bf16-autocast deviation, not the 1e-3 "
                             "gate (that is parity_class = bf16x3)" if args.precision == "bf16" else args.precision),
                         "parallelism": f"frame-sharded dp{world}, no data-path collective (each rank generates its own frames)"}}
    step = None
    if args.ingest in ("own", "both"):
        step = make_step(B)
        dt = timed(step, args.warmup, args.steps)
        result["value"] = args.steps * B * world / dt
        result["ms_per_step"] = 1e3 * dt / args.steps
        if args.dump_outputs and rank == 0:
            # before any later sub-run reuses the buffer
            result["dump_outputs"] = dump_outputs(args.dump_outputs, {"sbs_frames": step.out.cpu().numpy()}, args.steps - 1)

    if args.full and rank == 0 and world == 1 and not fake and B == 1 and not args.vda and not args.no_profile and step is not None:
        # Two frames in flight (reported beside `value`, never in it): the reference's own main loop overlaps consecutive frames -- capture,
        # depth and warp run in separate threads with queues between them (main.py) -- while `value` above issues frame i + 1 only after
        # frame i on ONE stream, so the serial tail of a frame (~0.2 ms of small dependent launches on a mostly idle chip) overlaps with
        # nothing.  Here two engines (same weights, own activation buffers) alternate on two HIP streams: per-frame work unchanged
        # (batch 1 per call, same kernels), throughput = what the chip gives when frame i + 1's encoder runs under frame i's tail.
        eng_b = ops.Engine(cfg, weights, h, w, max_batch=1, precision=args.precision, device=local_rank)
        streams2 = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        steps_ab = [make_step(1, eng), make_step(1, eng_b)]

        def two_in_flight(i):
            with torch.cuda.stream(streams2[i & 1]):
                steps_ab[i & 1](i >> 1)

        dt_ab = timed(two_in_flight, args.warmup, args.steps)
        lat = []
        for i in range(20):                              # frame latency with the other stream busy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(streams2[i & 1]):
                e0.record(); steps_ab[i & 1](i >> 1); e1.record()
            lat.append((e0, e1))
        sync()
        result["two_frames_in_flight"] = {"value": args.steps / dt_ab, "unit": "stereo frames/s", "ms_per_frame_throughput": 1e3 * dt_ab / args.steps,
                                          "frame_latency_ms": float(np.median([a.elapsed_time(b) for a, b in lat[4:]])),
                                          "note": "two engines on two HIP streams, batch 1 per call, frames issued alternately; `value` (one stream, one frame at a time) is the headline"}
        eng_b.close()

    if (args.ingest == "rank0" or args.ingest == "both" and args.full) and not args.vda:
        # SURVEY.md section 8(e), the other deployment: frames arrive on rank 0 (the capture host's GPU); every step rank 0
        # scatters uint8 frames point-to-point (RCCL send/recv over xGMI; xGMI has no switch, a root-centric scatter is
        # bounded by the root's egress), every rank runs the pipeline on its block, packed stereo frames are gathered back.
        n_total = B * world
        pool0 = [frames_for(5000 + 100 * j, n_total).to(dev) for j in range(2)] if rank == 0 else [None, None]
        out_r = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)

        steps_i = args.steps if args.ingest == "rank0" else max(5, args.steps // 4)
        if world > 1:
            # software-pipelined (shard.PipelinedIngest): scatter(k + 1) and gather(k - 1) travel under compute(k) on their own
            # streams, grouped point-to-point batches, double buffers; the drain is inside the timed region
            pipe = shard.PipelinedIngest(n_total, (H, W, 3), (oh, ow, 3), dev, lambda f, o: eng.pipeline(f, p, sp, use_ema=False, out=o))

            def ingest_step(i):
                return pipe.submit(pool0[i & 1])

            def ingest_run(warm, n):
                for i in range(warm):
                    ingest_step(i)
                pipe.flush()
                barrier()
                t0 = time.perf_counter()
                for i in range(n):
                    ingest_step(i)
                pipe.flush()
                sync()
                dt_ = time.perf_counter() - t0
                t = torch.tensor([dt_], dtype=torch.float64, device=coll_dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                barrier()
                return float(t.item())
            dti = ingest_run(max(2, args.warmup // 4), steps_i)
        else:
            def ingest_step(i):
                eng.pipeline(pool0[i & 1], p, sp, use_ema=False, out=out_r)
                return out_r
            dti = timed(ingest_step, max(2, args.warmup // 4), steps_i)
        ing = {"value": steps_i * n_total / dti, "unit": "stereo frames/s", "steps": steps_i, "ms_per_step": 1e3 * dti / steps_i,
               "frames_per_step": n_total,
               "exchange": (f"per step: one grouped batch of {world - 1} x isend of {B * H * W * 3 / 1e6:.1f} MB uint8 frames from rank 0 and one of "
                            f"{world - 1} x irecv of {B * oh * ow * 3 / 1e6:.1f} MB packed frames to rank 0 ({backend}), overlapped with the "
                            f"neighbouring steps' compute (shard.PipelinedIngest)") if world > 1 else "single rank: no exchange"}
        if args.ingest == "rank0":
            result["value"], result["ms_per_step"] = ing["value"], ing["ms_per_step"]
            result["config"]["parallelism"] = f"frame-sharded dp{world}, rank-0 ingest: point-to-point scatter / gather per step ({backend})"
        result["ingest_rank0"] = ing

    if args.model != "vitb" or (H, W) != (1080, 1920):
        result["metric"] = f"stereo frames/sec @{W}x{H} DepthAnything-v2-{cfg.name}"
    if args.vda:
        result["metric"] = f"stereo frames/sec @{W}x{H} VideoDepthAnything-{cfg.name} (streaming, window 32)"
        result["config"]["workload"] = result["config"]["workload"].replace("DepthAnything-v2", "VideoDepthAnything(stream, window 32)")
        result["config"]["parallelism"] = f"{world} independent stream(s), stream s on rank s % {world} (shard.stream_owner); replicas only"
        args.no_cpu_baseline = True                      # the CPU leg times the DA-v2 oracle only
        args.no_parity_class = True

    def finish():
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return result if rank == 0 else None

    if not args.full:
        eng.close()
        return finish()
    if step is None:
        step = make_step(B)

    if rank == 0 and not args.no_profile:
        result.update(profile_pass(eng, step, args.profile_steps, B, args.precision, sync, default_wl))
        result["model_gflop_per_frame"] = {"counted": result.pop("model_gflop_per_frame_counted"),
                                           "survey": SURVEY_GF_PER_FRAME.get((args.model, args.res))}
        result["model_stage_tflops_at_measured_fps"] = result["value"] / world * result["model_gflop_per_frame"]["counted"] / 1e3

    if B2:
        step2 = make_step(B2)
        steps2 = max(10, args.steps // B2)
        dt2 = timed(step2, max(3, args.warmup // 4), steps2)
        batched = {"value": steps2 * B2 / dt2, "unit": "stereo frames/s", "frames_per_step": B2, "steps": steps2,
                   "ms_per_step": 1e3 * dt2 / steps2, "workload": workload(B2)}
        if not args.no_profile:
            pr = profile_pass(eng, step2, 3, B2, args.precision, sync, default_wl)
            pr.pop("model_gflop_per_frame_counted", None)
            batched.update(pr)
        result["batched"] = batched

    if B2 and not fake and args.tile_fit:
        # The batched encoder linears run as 256 x 256 output tiles, one persistent block per CU (gemm_pp.hip): a batch whose
        # tile counts are just over a multiple of the CU count pays a whole extra round for a few tiles (batch 32: FC2 / proj
        # are 294 tiles on 256 CUs).  A deployment is free to pick its batch; this is the same measurement at the batch
        # <= --also-batch whose tile counts fill whole rounds best.  Reported beside "batched", never instead of it.
        B3 = tile_fit_batch((h // cfg.patch) * (w // cfg.patch) + 1, cfg.hidden, cfg.hidden * cfg.mlp_ratio, B2)
        if B3 != B2:
            step3 = make_step(B3)
            steps3 = max(10, args.steps // B3)
            dt3 = timed(step3, max(3, args.warmup // 4), steps3)
            fit = {"value": steps3 * B3 / dt3, "unit": "stereo frames/s", "frames_per_step": B3, "steps": steps3,
                   "ms_per_step": 1e3 * dt3 / steps3, "workload": workload(B3),
                   "note": "batch chosen so that the encoder GEMMs' 256x256 tile counts fill whole rounds of the 256 CUs"}
            if not args.no_profile:
                pr = profile_pass(eng, step3, 3, B3, args.precision, sync, False)
                pr.pop("model_gflop_per_frame_counted", None)
                fit.update(pr)
            result["batched_tile_fit"] = fit

    if NM:
        # config 5: every 16:9 size maps to the same model input (reference depth.py:676-706), so the model runs as ONE
        # batch of NM frames; only pre-process (A2-A4) and the warp (A13+A14) are per frame size
        sizes = [(720, 1280), (1080, 1920), (1440, 2560)]
        pick = np.random.default_rng(0).integers(0, 3, NM)
        groups = {s: [i for i in range(NM) if sizes[pick[i]] == s] for s in sizes}
        assert len({engine_shape(hh, ww, args.res)[:2] for hh, ww in sizes}) == 1
        frames = {s: torch.from_numpy(np.stack([synth.noise_frame(s[0], s[1], 7000 + i) for i in idx])).to(dev) for s, idx in groups.items() if idx}
        outs = {s: torch.empty((len(groups[s]),) + ops.sbs_shape(s[0], s[1], sp) + (3,), dtype=torch.uint8, device=dev) for s in frames}
        xm = torch.empty((NM, 3, h, w), dtype=torch.float32, device=dev)

        def step_mixed(i):
            for s, f in frames.items():
                xm[groups[s]] = ops.preprocess(f, args.res, resample=args.resample)
            depth = ops.post_process_depth(eng(xm), p)
            for s, f in frames.items():
                outs[s].copy_(ops.make_sbs(f, depth[groups[s]], sp))
        stepsm = max(5, args.steps // NM)
        dtm = timed(step_mixed, 2, stepsm)
        result["mixed"] = {"value": stepsm * NM / dtm, "unit": "stereo frames/s", "frames_per_step": NM, "steps": stepsm,
                           "ms_per_step": 1e3 * dtm / stepsm,
                           "workload": f"{NM} frames/step, sizes seed 0: " + ", ".join(f"{len(groups[s])}x{s[1]}x{s[0]}" for s in sizes)
                                       + f"; one {cfg.name} {args.precision} batch at {h}x{w}; {args.mode}"}

    if rank == 0 and world == 1 and not fake and args.precision not in ("fp32", "bf16x3") and not args.no_parity_class:
        # the engines that meet north_star's 1e-3 depth tolerance against the reference's fp32 CPU path (tests/test_gpu_configs.py,
        # test_full_size_predict_depth): "bf16x3" = fp32 activations, every GEMM / conv operand split into bf16 hi + lo and
        # multiplied as three bf16 MFMAs (the fast one); "fp32" = v_mfma_f32_16x16x4_f32.  Reported beside the headline, never as it.
        pc = {}
        for pname in ("bf16x3", "fp32"):
            engp = ops.Engine(cfg, weights, h, w, max_batch=B, precision=pname, device=local_rank)
            stepp = make_step(B, engp)
            stp = max(10, args.steps // 10)
            dtp = timed(stepp, 3, stp)
            pc[pname] = {"value": stp * B / dtp, "unit": "stereo frames/s", "dtype": pname, "steps": stp,
                         "ms_per_step": 1e3 * dtp / stp, "workload": workload(B, pname)}
            engp.close()
        gf = result.get("model_gflop_per_frame", {}).get("counted", 0.0)
        pc["fp32"]["frac_of_f32_mfma_peak"] = pc["fp32"]["value"] * gf / 1e3 / PEAK_TFLOPS["fp32"] if gf else None
        pc["bf16x3"]["frac_of_bf16_mfma_peak_counting_3_mfma_per_product"] = pc["bf16x3"]["value"] * 3 * gf / 1e3 / PEAK_TFLOPS["bf16"] if gf else None
        result["parity_class"] = dict(pc["bf16x3"], fp32_engine=pc["fp32"],
                                      gate="post-processed depth <= 1e-3 of the reference's fp32 CPU path, end-to-end RGB <= 1 LSB but isolated "
                                           "edge pixels (tests/test_gpu_configs.py::test_config2...); the headline bf16 engine: max 0.012-0.016 / "
                                           "mean 0.0022 (the reference's own bf16 CPU autocast: 0.036 / 0.0029)")

    if rank == 0 and world == 1 and not fake and not args.vda and not args.no_parity:
        # "depth L1 vs ref" -- the parity half of the metric, from the committed reference fixtures, outside the timed regions
        mk = {args.precision: (lambda hh, ww: ops.Engine(cfg, weights, hh, ww, max_batch=1, precision=args.precision, device=local_rank))}
        if args.precision not in ("fp32", "bf16x3") and not args.no_parity_class:
            mk["bf16x3"] = lambda hh, ww: ops.Engine(cfg, weights, hh, ww, max_batch=1, precision="bf16x3", device=local_rank)
        if args.precision != "fp8":                       # (an fp8 engine needs calibration inputs: its error is reported by tests/test_gpu_fp8.py)
            par = parity_vs_reference(ops, synth, cfg, weights, p, mk, dev)
            if par:
                result["parity"] = par
                head = par.get(args.precision, {})
                result["depth_l1_vs_ref"] = head.get("depth_l1_vs_ref")
                result["depth_max_vs_ref"] = head.get("depth_max_vs_ref")
                result["warp_max_lsb"] = par.get("warp_max_lsb")
                if "parity_class" in result and "bf16x3" in par:
                    result["parity_class"].update(par["bf16x3"])

    if rank == 0 and world == 1 and not fake and args.sink_quality > 0:
        # the Streamer modes' sink (cv2.imencode -> here the HIP JPEG encoder) behind the same step,
        # frame never leaving HBM.  Reported beside the headline number, not in it (the metric ends at make_sbs).
        q = args.sink_quality
        # like the reference's encoder thread (streamer.py:230-257) the encode runs beside the next frame's model pass:
        # own HIP stream, two output buffers, the producer waits for the encode that last read the buffer it reuses
        steps2 = [step, make_step(B)]
        side = torch.cuda.Stream(device=dev)
        done = [None, None]

        def sink_step(i):
            k = i & 1
            if done[k] is not None:
                torch.cuda.current_stream().wait_event(done[k])
            frames = steps2[k](i)
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(side):
                side.wait_event(ready)
                ops.jpeg_encode(frames, q)
                done[k] = torch.cuda.Event()
                done[k].record()

        dts = timed(sink_step, max(3, args.warmup // 4), args.steps)
        serial_step = lambda i: ops.jpeg_encode(step(i), q)
        dts_serial = timed(serial_step, max(3, args.warmup // 4), args.steps)
        frames_out = step(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            jb, jsz = ops.jpeg_encode(frames_out, q)
        e1.record()
        torch.cuda.synchronize()
        enc_us = e0.elapsed_time(e1) * 1e3 / 20 / B
        jbytes = float(jsz.float().mean())
        result["sink_jpeg"] = {"value": args.steps * B / dts, "unit": "stereo frames/s incl. JPEG encode (encode on its own stream)",
                               "value_same_stream": args.steps * B / dts_serial, "quality": q,
                               "encode_us_per_frame": enc_us, "jpeg_mb_per_frame": jbytes / 1e6,
                               "roofline": {"bound": "hbm", "achieved": (oh * ow * 3 + jbytes) / enc_us / 1e3, "peak": PEAK_HBM_GBS,
                                            "unit": "GB/s", "frac": (oh * ow * 3 + jbytes) / enc_us / 1e3 / PEAK_HBM_GBS},
                               "note": "noise frames: the largest entropy-coded stream a frame can produce"}
        try:                                             # libjpeg-turbo on one host core, same frame (Pillow, if present)
            import io
            from PIL import Image
            host = frames_out[0].cpu().numpy()
            t0 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(host).save(buf, "JPEG", quality=q, subsampling="4:2:0", optimize=False)
            result["sink_jpeg"]["cpu_libjpeg_turbo_ms_per_frame"] = 1e3 * (time.perf_counter() - t0)
            result["sink_jpeg"]["identical_to_libjpeg_turbo"] = buf.getvalue() == jb[0, :int(jsz[0])].cpu().numpy().tobytes()
        except ImportError:
            pass

    default_run = (args.model, args.res, args.precision, args.mode, H, W, B) == ("vitb", 518, "bf16", "Full-SBS", 1080, 1920, 1) and not args.vda
    if rank == 0 and world == 1 and not fake and default_run and not args.no_profile:
        # the viewer's DIBR shader with disocclusion in-painting as a HIP kernel (d2s_dibr_warp), the caller's alternative
        # to make_sbs.  1080p scene with hard depth edges (the in-painting's work), viewer defaults, both eyes, Full-SBS uint8.
        # Algorithmic bytes: 6.22 MB rgb + 8.29 MB float32 depth in, 12.44 MB out.
        img_d, dep_d = synth.dibr_scene(H, W, 11, "boxes")
        fr_d, de_d = torch.from_numpy(img_d).to(dev)[None], torch.from_numpy(dep_d).to(dev)[None]
        dp_d = ops.dibr_params(display_mode="Full-SBS")
        rows_d = {}
        for Bd in (1, 8):
            f_b, d_b = fr_d.expand(Bd, -1, -1, -1).contiguous(), de_d.expand(Bd, -1, -1).contiguous()
            for _ in range(3):
                ops.dibr_warp(f_b, d_b, dp_d)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(20):
                ops.dibr_warp(f_b, d_b, dp_d)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 20
            nbytes = Bd * (H * W * 3 + H * W * 4 + 2 * H * W * 3)
            rows_d[f"batch{Bd}"] = {"us_per_launch": us, "us_per_frame": us / Bd,
                                    "roofline": {"bound": "hbm", "achieved": nbytes / us / 1e3, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                 "frac": nbytes / us / 1e3 / PEAK_HBM_GBS}}
        result["f1_dibr"] = dict(rows_d, workload="d2s_dibr_warp: 1920x1080 uint8 frame + float32 depth (three near boxes: hard edges) -> both eyes, Full-SBS "
                                                  "3840x1080 uint8, viewer defaults (search radius 12, blending off); parity: tests/golden/dibr.npz (the reference's "
                                                  "own shader rendered off-screen)")
    if rank == 0 and world == 1 and not fake and default_run and args.resample == "bilinear" and not args.no_profile:
        # the reference's IS_CUDA pre-process branch (one bicubic + antialias resample of the full frame, depth.py:698-699) is
        # what its own GPU path runs; the headline uses the CPU branch (north_star: parity with the reference CPU path)
        import dataclasses
        p_aa = dataclasses.replace(p, resample="bicubic_aa")
        pool_aa = [frames_for(5000 + j, B).to(dev) for j in range(4)]
        out_aa = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
        st_aa = max(20, args.steps // 4)
        dt_aa = timed(lambda i: eng.pipeline(pool_aa[i % 4], p_aa, sp, use_ema=False, out=out_aa), 3, st_aa)
        result["resample_bicubic_aa"] = {"value": st_aa * B / dt_aa, "unit": "stereo frames/s", "ms_per_step": 1e3 * dt_aa / st_aa,
                                         "note": "same step with d2s_pre_params.resample = D2S_RESAMPLE_BICUBIC_AA"}

    if rank == 0 and world == 1 and not fake and default_run and not args.no_profile:
        # The boundary as the reference's callers see it: predict_depth takes a HOST uint8 frame and make_sbs returns a
        # HOST float32 HWC array (depth.py:1916-1924, 2231).  Reported beside `value`, never as `value`: (a) pinned uint8 frame in over
        # PCIe -> d2s_pipeline -> pinned uint8 packed frame out, copies and kernels in order on one stream; (b) the same with the float32
        # HWC result the reference's make_sbs hands back (4 x the bytes); (c) the drop-in Python surface itself, numpy in -> numpy out
        # (desktop2stereo_amd.depth.predict_depth + make_sbs: pageable buffers, two calls, host synchronisation per call as the API implies).
        try:
            hb = {}
            pin_in = [frames_for(6000 + j, B).pin_memory() for j in range(4)]
            dev_in = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
            out_u8 = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
            pin_u8 = torch.empty((B, oh, ow, 3), dtype=torch.uint8).pin_memory()
            pin_f32 = torch.empty((B, oh, ow, 3), dtype=torch.float32).pin_memory()
            out_f32 = torch.empty((B, oh, ow, 3), dtype=torch.float32, device=dev)

            def step_u8(i):
                dev_in.copy_(pin_in[i % 4], non_blocking=True)
                eng.pipeline(dev_in, p, sp, use_ema=False, out=out_u8)
                pin_u8.copy_(out_u8, non_blocking=True)

            def step_f32(i):
                step_u8(i)
                out_f32.copy_(out_u8)                               # uint8 -> float32 on the device (what chw_tensor_to_numpy's float frame holds)
                pin_f32.copy_(out_f32, non_blocking=True)
            nst = max(20, args.steps // 4)
            dt_u8 = timed(step_u8, 3, nst)
            dt_f32 = timed(step_f32, 3, nst)
            hb["pinned_u8_in_u8_out"] = {"value": nst * B / dt_u8, "ms_per_step": 1e3 * dt_u8 / nst, "bytes_over_pcie_per_frame": H * W * 3 + oh * ow * 3}
            hb["pinned_u8_in_f32_out"] = {"value": nst * B / dt_f32, "ms_per_step": 1e3 * dt_f32 / nst, "bytes_over_pcie_per_frame": H * W * 3 + oh * ow * 12}
            from desktop2stereo_amd import depth as dropin
            dropin.configure(args.model, weights, params=p, precision=args.precision, device=local_rank)
            np_frames = [frames_for(6100 + j, 1)[0].numpy() for j in range(4)]

            def step_api(i):
                d_ = dropin.predict_depth(np_frames[i % 4], use_temporal_smooth=False)
                dropin.make_sbs(np_frames[i % 4], d_, ipd_uv=p.ipd, depth_ratio=p.depth_strength, convergence=p.convergence, display_mode=args.mode)
            dt_api = timed(step_api, 3, nst)
            hb["dropin_numpy_in_numpy_f32_out"] = {"value": nst / dt_api, "ms_per_step": 1e3 * dt_api / nst}
            hb["unit"] = "stereo frames/s"
            hb["note"] = ("PCIe-inclusive rates of the same step, batch %d: copies and kernels serialised on one stream (no overlap of frame k's copies "
                          "with frame k+1's kernels); `value` above is the HBM-resident region" % B)
            result["host_boundary"] = hb
        except Exception as ex:                                      # (a measurement aid must not take the headline down with it)
            result["host_boundary"] = {"error": repr(ex)[:200]}

    if rank == 0 and world == 1 and not fake and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(cfg, weights, p, H, W, args.mode)
        # (no GPU / CPU ratio: a speed-up over a CPU path says nothing about kernel quality -- the roofline fractions do)
        if default_run:
            # BASELINE configs[0] (the reference's own CPU-runnable case): ViT-S, Half-SBS, 1080p, fill_16_9, Depth Resolution 518
            # and 336 -- the CPU port beside the HIP path on the same workload
            import dataclasses
            from desktop2stereo_amd.config import MODELS as _M
            from desktop2stereo_amd.weights import make_weights as _mw
            cfg1, w1 = _M["vits"], _mw(_M["vits"], 0)
            rows = {}
            for res1 in (518, 336):
                p1 = dataclasses.replace(p, depth_resolution=res1, display_mode="Half-SBS", fill_16_9=True)
                h1, w1_, _ = engine_shape(H, W, res1)
                sp1 = ops.sbs_params(p1.ipd, p1.depth_strength, p1.convergence, "Half-SBS", True)
                oh1, ow1 = ops.sbs_shape(H, W, sp1)
                e1 = ops.Engine(cfg1, w1, h1, w1_, max_batch=1, precision="bf16", device=local_rank)
                pool1 = [frames_for(7000 + j, 1).to(dev) for j in range(4)]
                out1 = torch.empty((1, oh1, ow1, 3), dtype=torch.uint8, device=dev)
                dt1 = timed(lambda i: e1.pipeline(pool1[i % 4], p1, sp1, use_ema=False, out=out1), 5, 50)
                e1.close()
                cb = cpu_baseline(cfg1, w1, p1, H, W, "Half-SBS", budget_s=5.0, max_frames=2)
                rows[f"res{res1}"] = {"gpu_frames_per_s": 50 / dt1, "cpu_port": {k: cb[k] for k in ("value", "cores", "sample")},
                                      "cpu_port_one_thread": cb.get("one_thread", {}).get("value")}
            result["config1_vits_half_sbs"] = dict(rows, workload="DepthAnything-v2-vits, 1920x1080, Half-SBS, fill_16_9, batch 1 (BASELINE configs[0]); "
                                                                  "GPU: bf16 HIP engine; CPU: numpy oracle (kind 'port') on this host")

    eng.close()
    if rank == 0 and world == 1 and not fake and default_run and not args.no_config3:
        # BASELINE configs[2]: DepthAnything-v2 ViT-L, 3840x2160, batch 1, TAB output -- bf16 engine and the e4m3 engine (the four encoder
        # linears on OCP e4m3 operands, static per-tensor activation scales calibrated on ONE structured frame: the engine is built for batch 1), Full-TAB 4320x3840.
        # Depth error of each against the committed reference fixture (vitl_r518_4k: the reference's fp32 CPU path on that frame).
        import numpy as np
        from desktop2stereo_amd.config import MODELS as _M3
        from desktop2stereo_amd.weights import make_weights as _mw3
        cfg3, H3, W3 = _M3["vitl"], 2160, 3840
        w3 = _mw3(cfg3, 0)
        h3, w3_, _ = engine_shape(H3, W3, 518)
        p3 = PipelineParams(depth_resolution=518, display_mode="Full-TAB")
        sp3 = ops.sbs_params(p3.ipd, p3.depth_strength, p3.convergence, "Full-TAB", p3.fill_16_9)
        oh3, ow3 = ops.sbs_shape(H3, W3, sp3)
        B3 = 8                                               # config 3 at batch 1 is latency-bound: the throughput row is batch 8 (both reported)
        pool3 = [torch.from_numpy(synth.noise_frame(H3, W3, 9000 + j)[None]).to(dev) for j in range(2)]
        pool3b = torch.cat([pool3[j & 1] for j in range(B3)])
        out3 = torch.empty((1, oh3, ow3, 3), dtype=torch.uint8, device=dev)
        out3b = torch.empty((B3, oh3, ow3, 3), dtype=torch.uint8, device=dev)
        ref3 = None
        try:
            z3 = np.load(os.path.join(REPO, "tests", "golden", "vitl_r518_4k.npz"))
            with open(os.path.join(REPO, "tests", "golden", "vitl_r518_4k.json")) as f:
                fr3 = json.load(f)["frames"][0]
            ref3 = (z3["f0_post_depth"], synth.structured_frame(fr3["h"], fr3["w"], fr3["seed"]))
        except OSError:
            pass
        emu3 = None
        try:
            with open(os.path.join(REPO, "tests", "golden", "fp8_frontier_vitl_4k.json")) as f:
                emu3 = json.load(f)["rows"]
        except OSError:
            pass
        rows3 = {}
        for prec3 in ("bf16", "fp8", "fp8_mlp"):
            e3 = ops.Engine(cfg3, w3, h3, w3_, max_batch=B3, precision=prec3, device=local_rank)
            if prec3 != "bf16":
                e3.calibrate(ops.preprocess(torch.from_numpy(synth.structured_frame(H3, W3, 0)).to(dev), 518))
            dt3 = timed(lambda i: e3.pipeline(pool3[i & 1], p3, sp3, use_ema=False, out=out3), 5, 40)
            dt3b = timed(lambda i: e3.pipeline(pool3b, p3, sp3, use_ema=False, out=out3b), 3, 10)
            row = {"value": 40 / dt3, "unit": "stereo frames/s", "ms_per_step": 1e3 * dt3 / 40,
                   "batch8": {"value": 10 * B3 / dt3b, "unit": "stereo frames/s", "ms_per_step": 1e3 * dt3b / 10, "frames_per_step": B3}}
            if ref3 is not None:
                post = ops.post_process_depth(e3(ops.preprocess(torch.from_numpy(ref3[1]).to(dev), 518)), p3).cpu().numpy()[0]
                dd = np.abs(post - ref3[0])
                row.update(depth_l1_vs_ref=float(dd.mean()), depth_max_vs_ref=float(dd.max()))
            if prec3 != "bf16":
                # the encoder linears of this engine against the dense fp8 peak (5 PF): the 256 x 256 tiles run the scaled K = 64 MFMA
                pr = profile_pass(e3, lambda i: e3.pipeline(pool3b, p3, sp3, use_ema=False, out=out3b), 4, B3, "fp8", sync)
                row["roofline"] = dict(pr["roofline"], note="batch 8; e4m3 operands on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (256 x 256 tiles) / v_mfma_f32_16x16x32_fp8_fp8 (smaller tiles); priced against the 5 PF dense fp8 peak")
                if emu3 is not None:
                    row["reference_emulation"] = emu3["all four e4m3" if prec3 == "fp8" else "MLP only (FC1 + FC2)"]
            rows3[prec3] = row
            e3.close()
        result["config3_vitl_4k_full_tab"] = dict(
            rows3, fp8_over_bf16=rows3["fp8"]["value"] / rows3["bf16"]["value"],
            fp8_over_bf16_batch8=rows3["fp8"]["batch8"]["value"] / rows3["bf16"]["batch8"]["value"],
            fp8_mlp_over_bf16_batch8=rows3["fp8_mlp"]["batch8"]["value"] / rows3["bf16"]["batch8"]["value"],
            workload="DepthAnything-v2-vitl, 3840x2160 uint8 noise frames, batch 1 (and batch 8), Depth Resolution 518 (CPU-branch ::3 decimation, model "
                     "input 294x518), Full-TAB uint8 output 3840x4320 (BASELINE configs[2]); depth error vs tests/golden/vitl_r518_4k (structured frame); "
                     "fp8 = e4m3 operands on all four encoder linears, fp8_mlp = on FC1 / FC2 only (QKV / proj bf16); scaled K = 64 e4m3 MFMA in the 256 x 256 tiles (2 x the bf16 issue "
                     "rate), static per-tensor activation scales; reference_emulation = the reference's own model under the same operand quantisation "
                     "(tests/golden/fp8_frontier_vitl_4k.json)")
    if rank == 0 and world == 1 and not fake and default_run and not args.no_config3:
        # BASELINE configs[3]: one Video-Depth-Anything stream (window 32, ring of projected K' / V' rows) per GPU through d2s_pipeline,
        # 1080p frames, Full-SBS; the two sizes the reference's settings select (Depth Resolution 336 / 518).  One stream never shards:
        # 8 GPUs = 8 independent streams (shard.stream_owner) -- `python bench.py --vda --gpus N` times that; this sub-object is the
        # per-stream rate on this GPU so that the driver's default run sees it.
        from desktop2stereo_amd.config import MODELS as _M4
        from desktop2stereo_amd.vda_weights import make_vda_weights as _mv4
        rows4 = {}
        for name4, res4 in (("vits", 336), ("vitb", 518)):
            cfg4 = _M4[name4]
            h4, w4, _ = engine_shape(H, W, res4)
            p4 = PipelineParams(depth_resolution=res4, display_mode="Full-SBS")
            sp4 = ops.sbs_params(p4.ipd, p4.depth_strength, p4.convergence, "Full-SBS", p4.fill_16_9)
            oh4, ow4 = ops.sbs_shape(H, W, sp4)
            e4 = ops.Engine(cfg4, _mv4(cfg4, 0), h4, w4, 1, "bf16", device=local_rank, temporal=True)
            pool4 = [torch.from_numpy(synth.noise_frame(H, W, 7000 + j)[None]).to(dev) for j in range(4)]
            out4 = torch.empty((1, oh4, ow4, 3), dtype=torch.uint8, device=dev)
            dt4 = timed(lambda i: e4.pipeline(pool4[i & 3], p4, sp4, use_ema=False, out=out4), 40, 150)      # (40 warm-up frames fill the 32-frame window)
            pr4 = profile_pass(e4, lambda i: e4.pipeline(pool4[i & 3], p4, sp4, use_ema=False, out=out4), 4, 1, "bf16", sync)
            rows4[f"{name4}_r{res4}"] = {"value": 150 / dt4, "unit": "stereo frames/s per stream", "ms_per_step": 1e3 * dt4 / 150,
                                         "launches_per_step": pr4["launches_per_step"], "model_input": [h4, w4]}
            e4.close()
        result["config4_vda"] = dict(rows4, workload="VideoDepthAnything streaming forward (32-frame window) + post-process + Full-SBS warp through d2s_pipeline, "
                                                      "1920x1080 uint8 noise frames, one stream on this GPU, bf16 engine, EMA off")
    return finish()


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_as_ranks(args.gpus)                      # does not return
    result = rank_body(args)
    if result is not None:
        # The driver parses the LAST stdout line and keeps an ~8 KB tail: the full report (20+ KB) goes to a file, stdout gets ONE compact
        # line (< 4 KB) with the contract's keys + roofline + cpu_baseline (BENCH_r05.parsed was null).
        full_path = args.full_out or os.path.join(REPO, "gpurun_out", "bench_full.json")
        try:
            os.makedirs(os.path.dirname(full_path), exist_ok=True)
            with open(full_path, "w") as f:
                json.dump(result, f)
                f.write("\n")
        except OSError as e:
            full_path = f"not written: {e}"
        line = json.dumps(compact_line(result, full_path), separators=(",", ":"))
        assert len(line) < 6000, len(line)
        print(line, flush=True)


if __name__ == "__main__":
    main()
