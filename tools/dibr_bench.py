#!/usr/bin/env python
"""d2s_dibr_warp alone: 1080p scene with hard depth edges -> both eyes; us per launch and HBM fraction.
    python tools/dibr_bench.py [--mode Full-SBS] [--batch 1 8]
    python tools/dibr_bench.py --composite Anaglyph|Interleaved|Interleaved-V|"Depth Map" [--viewport X Y W H]   (d2s_dibr_composite)
    python tools/dibr_bench.py --pipeline [--model vitb] [--precision bf16] [--mode Full-SBS | --composite Anaglyph] [--batch 1 16] [--json FILE]
        frames -> views end to end: Engine.view_pipeline (the warp reads the model-resolution depth) against the two-call path it
        replaces (Engine.pipeline(want_depth=True) for the full-resolution depth map, then dibr_warp / dibr_composite on it), alternated
        in one process with inputs resident, device events; the parent is also timed against itself (the run-to-run spread), and
        the warp stage alone is timed both ways (upsample_depth + warp on the full map against the warp on the small map).
    python tools/dibr_bench.py --crop [X Y W H] [--corner-radius 0.03]
        d2s_dibr_warp_crop (the OpenXR screen's source crop; default: the 2.39:1 letterbox of a 16:9 frame) against the UNCROPPED
        d2s_dibr_warp_depth on a frame of the crop's pixel size, alternated in one process, us per launch and ns per output pixel.
        Both sides run THIS library (the uncropped kernels' device code does not change with the crop).  A library of
        the parent commit cannot be put under this mode with D2S_LIB -- it has no d2s_dibr_warp_crop, and D2S_LIB replaces the
        library of the whole process; to time the parent, run its own checkout's `tools/dibr_bench.py --height <eye rows>` (and the
        plain `tools/dibr_bench.py` for the uncropped 1080p warp) alternated with this one on the same box.
    python tools/dibr_bench.py --xr-eye [--curve h|v] [--eye-size 2064 2208]
        d2s_dibr_xr_eyes: the OpenXR screen drawn into two swapchain-size eye images from one 1080p frame (flat, or curved
        horizontally / vertically: 48 facets), against d2s_dibr_warp_crop's gather kernel (D2S_DIBR_NO_ROWS=1, identity crop, both eyes
        at the frame's size) -- the same pixel function on a regular grid.  The screen's distance is set so that the flat screen is
        one source texel per pixel wide; us per launch and ns per COVERED pixel, alternated in one process.
    python tools/dibr_bench.py --xr-eye --curve h|v --glow glow|glow2 [--glow-range 15.0]
        d2s_dibr_xr_eyes_glow_curved (the curved screen with its glow: a per-pixel search over the band mesh's planar pieces)
        alternated in one process with (a) the curved screen without glow, (b) the flat screen with glow and (c) the flat screen
        without glow: us per launch, the shares of the images the screen and the glow cover, and the ceiling (a) + (b) - (c).
    python tools/dibr_bench.py --xr-eye --glow glow|glow2 [--glow-range 15.0]
        d2s_dibr_xr_eyes_glow (the flat screen with the reference's glow in the same launch, every pixel of both eye images drawn) and
        d2s_mip_chain (the 1080p frame's colour mip chain, which the glow samples), alternated in one process with the flat eye call
        without glow through the old entry (d2s_dibr_xr_eyes) and through the new one (glow off): us per launch, ns per image pixel.
    python tools/dibr_bench.py --xr-eye --curve h|v --frost veil|frosted [--ab-lib other/libd2s_hip.so]
        d2s_dibr_xr_eyes_frost_curved against its ceiling (a) the plain curved call + (b) the flat call with the same look - (c) the
        flat plain call, alternated in one process, with the D2S_XR_BIN=0 time (every pixel walks all 244 rows) and the curved glow
        for scale.  --ab-lib: the other build's plain, curved-glow and flat-frost calls in the same rounds, each with its own margin.
    python tools/dibr_bench.py --xr-eye --frost veil|frosted [--ab-lib other/libd2s_hip.so]
        d2s_dibr_xr_eyes_frost (the flat screen with the reference's veil or frosted walls in the same launch), alternated in one
        process with the plain eye call through d2s_dibr_xr_eyes and through the new entry (frost off), the flat glow (for scale) and
        d2s_mip_chain.  --ab-lib: another build of the library (the parent commit's), loaded beside this one; its d2s_dibr_xr_eyes
        and this build's take the same arguments through the same bare C call in the same rounds, twice each, so that the other
        build's spread against itself is the margin of the comparison.
    python tools/dibr_bench.py --xr-eye --panorama 4096 2048 [--glow glow|glow2 | --frost veil|frosted | --curve h|v] [--ab-lib other/libd2s_hip.so]
        d2s_dibr_xr_eyes_panorama (the reference's equirectangular panorama behind the screen, in the same launch) against the same
        look without a panorama, alternated in one process: us per launch and ns per BACKGROUND pixel (the pixels no facet covers),
        the existing entry of that look against the new one with pano == NULL, and the panorama's d2s_mip_chain once.  With a flat
        screen a look may be on; a curved screen takes the panorama without one.  --ab-lib: the other build's existing entry of the
        look and this build's new entry with pano == NULL through the same bare C call in the same rounds, twice each: the other
        build's spread against itself is the margin.  D2S_HIPCC_DEFS=-DD2S_PANO_NO_FETCH (tools/build_variant.sh) builds the variant
        whose background skips the eight texel fetches: what is left is the coordinate and LOD arithmetic.
    python tools/dibr_bench.py --xr-eye --panorama 4096 2048 --curve h|v (--glow glow|glow2 | --frost veil|frosted) [--ab-lib other/libd2s_hip.so]
        d2s_dibr_xr_eyes_panorama_curved (the panorama behind the curved screen's glow or walls) in the same scheme: the look's own
        curved entry, the new entry with pano == NULL, the new entry with the panorama, the first two again; us per launch and ns
        per background pixel.  --ab-lib: the other build's curved entry of the look, this build's curved entry and this build's new
        entry with pano == NULL through the same bare C call in the same rounds, twice each.
    python tools/dibr_bench.py --xr-eye --panels [--curve h|v]
        d2s_dibr_xr_panels: the status panel below the screen and the keyboard group (border, keyboard, one highlight) at the
        reference's default sizes, blended over the plain eye call's images.  In alternating rounds: the eye call alone, the eye call
        followed by the panels pass, the pass alone, the pass with no panel (its host path: 0 launches), the eye call again; us per
        call, and ns per pixel the pass changed beside the eye call's ns per covered screen pixel."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from desktop2stereo_amd import ops, synth
ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="Full-SBS")
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
ap.add_argument("--height", type=int, default=1080); ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--kind", default="boxes")
ap.add_argument("--composite", default=None, help="a composite mode instead of the f1 warp")
ap.add_argument("--viewport", type=int, nargs=4, default=None, help="composite viewport x y w h in window pixels (default: the frame)")
ap.add_argument("--pipeline", action="store_true", help="time Engine.view_pipeline against pipeline(want_depth) + the warp")
ap.add_argument("--model", default="vitb"); ap.add_argument("--precision", default="bf16")
ap.add_argument("--depth-resolution", type=int, default=518)
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--json", default=None, help="--pipeline: also write the figures to this file")
ap.add_argument("--crop", type=float, nargs="*", default=None, help="time d2s_dibr_warp_crop: x y w h in uv (no values: a 2.39:1 letterbox)")
ap.add_argument("--corner-radius", type=float, default=0.0, help="--crop: u_corner_radius (0.03 is the OpenXR screen's)")
ap.add_argument("--xr-eye", action="store_true", help="time d2s_dibr_xr_eyes against the cropped warp's gather kernel")
ap.add_argument("--curve", default=None, choices=["h", "v"], help="--xr-eye: the curved screen (horizontal / vertical)")
ap.add_argument("--eye-size", type=int, nargs=2, default=[2064, 2208], help="--xr-eye: swapchain image width height")
ap.add_argument("--glow", default=None, choices=["glow", "glow2"], help="--xr-eye: time the glow eye call and mip_chain")
ap.add_argument("--glow-range", type=float, default=None, help="--glow: range_m (default: xr.glow_range_m of the screen)")
ap.add_argument("--frost", default=None, choices=["veil", "frosted"], help="--xr-eye: time the veil / frosted eye call (flat screen)")
ap.add_argument("--panorama", type=int, nargs=2, default=None, metavar=("W", "H"), help="--xr-eye: time the panorama background of this size")
ap.add_argument("--panels", action="store_true", help="--xr-eye: time the plain eye call against the eye call + d2s_dibr_xr_panels (status panel + keyboard group)")
ap.add_argument("--ab-lib", default=None, help="--frost: another build of libd2s_hip.so whose d2s_dibr_xr_eyes is timed in the same rounds")
a = ap.parse_args()
dev = torch.device("cuda")


def pipeline_bench():
    import json
    import numpy as np
    from desktop2stereo_amd.config import MODELS, PipelineParams, engine_shape
    from desktop2stereo_amd.weights import make_weights
    H, W = a.height, a.width
    cfg = MODELS[a.model]
    p = PipelineParams(depth_resolution=a.depth_resolution)
    h, w, _ = engine_shape(H, W, p.depth_resolution, cfg.patch)
    dp = ops.dibr_params(p.ipd, p.depth_strength, p.convergence, a.mode, viewport=tuple(a.viewport) if a.viewport else (0.0, 0.0, 0.0, 0.0))
    sp = ops.sbs_params(p.ipd, p.depth_strength, p.convergence, "Half-SBS", False)
    eng = ops.Engine(cfg, make_weights(cfg, 0), h, w, max(a.batch), a.precision)
    results = []
    for B in a.batch:
        f = torch.from_numpy(np.stack([synth.dibr_scene(H, W, 11 + i, a.kind)[0] for i in range(min(B, 4))])).to(dev)
        f = f.repeat((B + f.shape[0] - 1) // f.shape[0], 1, 1, 1)[:B].contiguous()
        warp_full = (lambda d: ops.dibr_composite(f, d, dp, a.composite)) if a.composite else (lambda d: ops.dibr_warp(f, d, dp))

        def parent():
            _, depth = eng.pipeline(f, p, sp, want_depth=True)
            return warp_full(depth)

        def fused():
            return eng.view_pipeline(f, p, dp, view=a.composite)

        _, depth_full = eng.pipeline(f, p, sp, want_depth=True)
        d_small = torch.rand((B, h, w), device=dev)
        d_small[:, h // 4: h // 2, w // 4: w // 2] = 0.05                       # hard edges: the in-painting runs

        def warp_parent():
            return warp_full(ops.upsample_depth(d_small, H, W))

        def warp_fused():
            return warp_full(d_small)

        assert torch.equal(parent(), fused()) and torch.equal(warp_parent(), warp_fused()), "fused != two-call"

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(a.iters): fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.iters

        for fn in (parent, fused, warp_parent, warp_fused):
            for _ in range(3): fn()
        t = {k: [] for k in ("parent", "fused", "parent_again", "warp_parent", "warp_fused", "warp_parent_again")}
        for _ in range(a.rounds):                                                # alternated: drift hits every path alike
            t["parent"].append(timed(parent)); t["fused"].append(timed(fused)); t["parent_again"].append(timed(parent))
            t["warp_parent"].append(timed(warp_parent)); t["warp_fused"].append(timed(warp_fused)); t["warp_parent_again"].append(timed(warp_parent))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        out_bytes = fused().numel() // B
        src = 0 if a.composite == "Depth Map" else H * W * 3
        alg_fused = src + h * w * 4 + out_bytes                                  # per frame, the warp stage: frame + small depth + output
        alg_parent = alg_fused + 2 * H * W * 4                                   # + the full-resolution map written once and read once
        r = dict(view=a.composite or a.mode, model=a.model, precision=a.precision, H=H, W=W, h=h, w=w, batch=B, rounds=a.rounds, iters=a.iters,
                 us=med, us_all=t, spread_pipeline_us=abs(med["parent"] - med["parent_again"]), spread_warp_us=abs(med["warp_parent"] - med["warp_parent_again"]),
                 warp_bytes_per_frame=dict(parent=alg_parent, fused=alg_fused))
        results.append(r)
        print(f"{r['view']} {H}x{W} {a.model} {a.precision} B={B}: pipeline parent {med['parent']:9.1f} us  fused {med['fused']:9.1f} us  "
              f"(parent again {med['parent_again']:9.1f}: spread {r['spread_pipeline_us']:.1f})   fused - parent = {med['fused'] - med['parent']:+.1f} us", flush=True)
        print(f"    warp stage alone: upsample + warp {med['warp_parent']:8.1f} us  fused warp {med['warp_fused']:8.1f} us  "
              f"(again {med['warp_parent_again']:8.1f}: spread {r['spread_warp_us']:.1f})   algorithmic bytes / frame: parent {alg_parent / 1e6:.1f} MB, fused {alg_fused / 1e6:.1f} MB",
              flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)
    eng.close()


if a.pipeline:
    pipeline_bench()
    sys.exit(0)
if a.xr_eye:
    import math
    import numpy as np
    from desktop2stereo_amd import xr
    os.environ["D2S_DIBR_NO_ROWS"] = "1"                                           # the comparison is the gather kernel
    ops.reload_env()
    ew, eh = a.eye_size
    fovs = ((-0.85, 0.75, 0.80, -0.85), (-0.75, 0.85, 0.80, -0.85))
    px_per_tan = ew / (math.tan(0.85) + math.tan(0.75))
    width = 2.4
    screen = xr.XrScreen(width=width, height=width * a.height / a.width, distance=width * px_per_tan / a.width,
                         curve={None: "flat", "h": "horizontal", "v": "vertical"}[a.curve], clear=(0.0, 0.0, 0.0, 0.5))
    eyes = [xr.xr_eye(xr.fov_to_proj_mat4(*fovs[i]) @ xr.pose_to_view_mat4((0, 0, 0, 1), ((-0.032, 0.032)[i], 0, 0)), ew, eh, i) for i in range(2)]
    img, dep = synth.dibr_scene(a.height, a.width, 11, a.kind)
    dp = ops.dibr_params(corner_radius=0.03, alpha="rgba")
    for B in a.batch if a.panels else ():
        # the status panel below the screen and the keyboard group (border, keyboard, one highlight) at the reference's default sizes
        # (xr_viewer/implementation.py:621-632, 723; xr_viewer/constants.py:119), over the plain eye call's images
        rng = np.random.default_rng(7)
        texs = [torch.from_numpy(rng.integers(0, 256, (h_, w_, 4), dtype=np.uint8)).to(dev) for w_, h_ in ((768, 238), (1280, 384))]
        kb = xr.XrPanel.keyboard_world(0.0, -0.2, 0.7, 0.0, math.radians(-35.0))
        panels = [xr.XrPanel.below_screen(screen, (768, 238), texture=0)] + \
            xr.XrPanel.keyboard_group(kb, 1.6, 0.33, 1.0, [((-0.3, -0.05, -0.2, 0.0), (0.5, 0.85, 1.0, 0.70))], texture=1)
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        plan = ops.dibr_xr_panels_plan(B, screen, eyes, panels, texs)
        probe = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)
        before = [t.clone() for t in probe]
        ops.dibr_xr_panels(probe, screen, eyes, panels, texs)
        drawn = B * sum(int((x != y).any(-1).sum()) for x, y in zip(probe, before))      # pixels the pass changed
        screen_px = B * sum(int((e[..., 3] != 0.5).sum()) for e in before)             # clear alpha 0.5 marks the uncovered pixels
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        views = ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)

        def both():
            ops.dibr_xr_panels(ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out), screen, eyes, panels, texs)
        runs = {"eyes": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out), "eyes_then_panels": both,
                "panels_alone": lambda: ops.dibr_xr_panels(views, screen, eyes, panels, texs),
                "panels_none_on_screen": lambda: ops.dibr_xr_panels(views, screen, eyes, [], []),      # the host path alone: 0 launches
                "eyes_again": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)}
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        extra = med["eyes_then_panels"] - med["eyes"]
        print(f"xr-eye panels {screen.curve} {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, uint8, {len(panels)} panels, medians of {a.rounds} rounds x {a.iters} calls; "
              f"plan: {plan['rows_per_eye']} rows per eye, {plan['setup_launches']} set-up + {plan['render_launches']} render launches, tiles {plan['tiles']} "
              f"of {[(-(-ew // 16), -(-eh // 16))] * 2}, grid {plan['grid']}; the pass changed {drawn // B} pixels per frame ({drawn / (B * 2 * ew * eh):.4f} of the images)", flush=True)
        for k in runs:
            print(f"    {k:24s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f})", flush=True)
        print(f"    eyes + panels - eyes = {extra:+.1f} us = {1e3 * extra / max(drawn, 1):.4f} ns per panel-covered pixel; panels alone "
              f"{1e3 * med['panels_alone'] / max(drawn, 1):.4f} ns per panel-covered pixel; the eye call {1e3 * med['eyes'] / screen_px:.4f} ns per covered "
              f"screen pixel; eyes against itself {med['eyes_again'] - med['eyes']:+.1f} us", flush=True)
    if a.panels:
        sys.exit(0)
    for B in a.batch if a.panorama else ():
        import ctypes as C
        from desktop2stereo_amd import _lib
        curved_look = bool(a.curve and (a.glow or a.frost))      # d2s_dibr_xr_eyes_panorama_curved's own ground: the old entry refuses it
        if a.glow and a.frost:
            sys.exit("--panorama: at most one of --glow and --frost")
        pw, ph = a.panorama
        yy, xx = np.meshgrid((np.arange(ph) + 0.5) / ph, (np.arange(pw) + 0.5) / pw, indexing="ij")
        rng = np.random.default_rng(3)
        pano = np.stack([118 + 80 * (yy - 0.5) + 45 * np.sin(2 * np.pi * ((k + 1) * xx + 1.5 * yy)) + 45 * np.sin(2 * np.pi * (3 * xx - (k + 1) * yy))
                         + rng.uniform(-3, 3, (ph, pw)) for k in range(3)], -1)
        pr = torch.from_numpy(np.rint(np.clip(pano, 0, 255)).astype(np.uint8)).to(dev)
        pl = ops.mip_chain(pr).view(-1)
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        frost = None if not a.frost else xr.XrFrost.veil() if a.frost == "veil" else xr.XrFrost.frosted(time=1.0)
        glow = xr.XrGlow(a.glow, xr.glow_range_m(screen) if a.glow_range is None else a.glow_range) if a.glow else None
        levels = ops.mip_chain(f) if glow is not None or frost is not None else None
        pv = [(xr.fov_to_proj_mat4(*fovs[i]), xr.pose_to_view_mat4((0, 0, 0, 1), ((-0.032, 0.032)[i], 0, 0))) for i in range(2)]
        ps = xr.XrPanorama().c_struct(pv, (ph, pw))
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        n_px = 2 * ew * eh
        probe = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)        # clear alpha 0.5 marks the pixels no facet covers
        n_bg = sum(int((e[..., 3] == 0.5).sum()) for e in probe)
        look = "glow" if glow is not None else "frost" if frost is not None else "plain"
        if curved_look and look == "glow":
            old = lambda: ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, out=out)
        elif curved_look:
            old = lambda: ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, out=out)
        elif look == "glow":
            old = lambda: ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, out=out)
        elif look == "frost":
            old = lambda: ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, out=out)
        else:
            old = lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)
        entry = ops.dibr_xr_eyes_panorama_curved if curved_look else ops.dibr_xr_eyes_panorama
        new = lambda p, r, l: (lambda: entry(f, d, dp, screen, eyes, p, r, l, glow=glow, frost=frost, levels=levels, out=out))
        a0, b0 = [t.clone() for t in old()], [t.clone() for t in new(None, None, None)()]
        assert all(torch.equal(x, y) for x, y in zip(a0, b0)), "pano == NULL differs from the existing entry"
        runs = {f"{look}_old_entry": old, f"{look}_new_entry_no_panorama": new(None, None, None), f"{look}_panorama": new(ps, pr, pl),
                f"{look}_old_entry_again": old, f"{look}_new_entry_no_panorama_again": new(None, None, None), f"{look}_panorama_again": new(ps, pr, pl)}
        if a.ab_lib:      # the other build's existing entry of the look and this build's new entry with pano == NULL: the bare C calls
            other = C.CDLL(os.path.abspath(a.ab_lib))
            name = {"plain": "d2s_dibr_xr_eyes", "glow": "d2s_dibr_xr_eyes_glow", "frost": "d2s_dibr_xr_eyes_frost"}[look] + ("_curved" if curved_look else "")
            new_name = "d2s_dibr_xr_eyes_panorama_curved" if curved_look else "d2s_dibr_xr_eyes_panorama"
            getattr(other, name).restype, getattr(other, name).argtypes = _lib.SYMBOLS[name]
            other.d2s_version.restype = C.c_int
            sc, ea = screen.c_struct(), xr.eye_array(eyes)
            ws = torch.empty(2 * 244 * 96, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            gs, fs = (glow.c_struct() if glow is not None else None), (frost.c_struct() if frost is not None else None)
            lv = levels.data_ptr() if levels is not None else None
            head = lambda: (f.data_ptr(), d.data_ptr(), d.shape[1], d.shape[2], B, a.height, a.width, C.byref(dp), None, C.byref(sc), ea, 2,
                            out.data_ptr(), _lib.FMT_U8_HWC, ws.data_ptr(), ws.numel())
            tail = {"plain": (), "glow": (C.byref(gs) if gs else None, lv), "frost": (C.byref(fs) if fs else None, lv)}[look]

            def other_old():
                rc = getattr(other, name)(*head(), *tail, st)
                assert rc == 0, rc

            def this_old():
                rc = getattr(_lib.load(), name)(*head(), *tail, st)
                assert rc == 0, rc

            def this_new():
                rc = getattr(_lib.load(), new_name)(*head(), C.byref(fs) if fs else None, lv, C.byref(gs) if gs else None, None, None, None, st)
                assert rc == 0, rc
            other_old()
            torch.cuda.synchronize()
            same = bool(torch.equal(a0[0], out[:a0[0].numel()].view(a0[0].shape)))
            print(f"--ab-lib {a.ab_lib}: d2s_version {other.d2s_version()} (this build {_lib.load().d2s_version()}); its eye 0 is "
                  f"{'bit-identical to' if same else 'DIFFERENT from'} this build's", flush=True)
            runs = dict({"other_lib_old_entry": other_old, "this_lib_old_entry": this_old, "this_lib_new_entry_no_panorama": this_new}, **runs,
                        other_lib_old_entry_again=other_old, this_lib_old_entry_again=this_old, this_lib_new_entry_no_panorama_again=this_new)
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.mip_chain(pr, out=pl.view(1, -1)); torch.cuda.synchronize(); e0.record()
        ops.mip_chain(pr, out=pl.view(1, -1))
        e1.record(); torch.cuda.synchronize()
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {screen.curve} {look} + panorama {pw}x{ph} {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, medians of {a.rounds} rounds x {a.iters} "
              f"launches; {n_bg / n_px:.3f} of the images is background:", flush=True)
        for k in runs:
            print(f"    {k:40s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f}; {1e3 * med[k] / (B * n_px):.4f} ns / image pixel)", flush=True)
        cost = med[f"{look}_panorama"] - med[f"{look}_new_entry_no_panorama"]
        spread = max(abs(med[f"{look}_panorama_again"] - med[f"{look}_panorama"]), abs(med[f"{look}_new_entry_no_panorama_again"] - med[f"{look}_new_entry_no_panorama"]))
        print(f"    the panorama costs {cost:+.1f} us = {1e3 * cost / (B * n_bg):.4f} ns per background pixel (the rounds' spread: {spread:.1f} us = "
              f"{1e3 * spread / (B * n_bg):.4f} ns); new entry without it - old entry = "
              f"{med[f'{look}_new_entry_no_panorama'] - med[f'{look}_old_entry']:+.1f} us; old entry against itself {med[f'{look}_old_entry_again'] - med[f'{look}_old_entry']:+.1f} us; "
              f"the panorama's mip_chain, once: {e0.elapsed_time(e1) * 1e3:.1f} us", flush=True)
        if a.ab_lib:
            margin = abs(med["other_lib_old_entry_again"] - med["other_lib_old_entry"])
            print(f"    other build against itself: {med['other_lib_old_entry_again'] - med['other_lib_old_entry']:+.1f} us (the margin: {margin:.1f} us)", flush=True)
            for k, what in (("this_lib_old_entry", "this build's existing entry"), ("this_lib_new_entry_no_panorama", "this build's new entry, pano == NULL")):
                worst = max(med[k], med[k + "_again"]) - max(med["other_lib_old_entry"], med["other_lib_old_entry_again"])
                print(f"    {what}: its slower run - the other's slower run = {worst:+.1f} us: {'within' if worst <= margin else 'BEYOND'} the margin", flush=True)
    if a.panorama:
        sys.exit(0)
    for B in a.batch if a.frost and not a.curve else ():
        import ctypes as C
        from desktop2stereo_amd import _lib
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        frost = xr.XrFrost.veil() if a.frost == "veil" else xr.XrFrost.frosted(time=1.0)
        glow = xr.XrGlow("glow", xr.glow_range_m(screen))
        levels = ops.mip_chain(f)
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        probe_s = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)      # clear alpha 0.5 marks the pixels nothing drew
        probe_f = ops.dibr_xr_eyes_frost(f[:1], d[:1], dp, screen, eyes, frost, levels[:1], out_u8=False)
        n_px = 2 * ew * eh
        share_screen = sum(int((e[..., 3] != 0.5).sum()) for e in probe_s) / n_px
        share_wall = sum(int((p != q).any(-1).sum()) for p, q in zip(probe_s, probe_f)) / n_px
        runs = {"eyes_old_entry": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                "eyes_new_entry_frost_off": lambda: ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, None, None, out=out),
                f"eyes_{a.frost}": lambda: ops.dibr_xr_eyes_frost(f, d, dp, screen, eyes, frost, levels, out=out),
                "eyes_glow": lambda: ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, out=out),
                "eyes_old_entry_again": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                "mip_chain": lambda: ops.mip_chain(f, out=levels)}
        if a.ab_lib:      # the other build's plain eye call, on the same tensors and stream, through ctypes alone (it may lack newer symbols)
            other = C.CDLL(os.path.abspath(a.ab_lib))
            other.d2s_dibr_xr_eyes.restype, other.d2s_dibr_xr_eyes.argtypes = _lib.SYMBOLS["d2s_dibr_xr_eyes"]
            other.d2s_version.restype = C.c_int
            sc, ea = screen.c_struct(), xr.eye_array(eyes)
            ws = torch.empty(2 * 52 * 96, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def raw_eyes(lib):      # both builds through the SAME host path: the C call alone, no tensor checks in between
                def call():
                    rc = lib.d2s_dibr_xr_eyes(f.data_ptr(), d.data_ptr(), d.shape[1], d.shape[2], B, a.height, a.width, C.byref(dp), None, C.byref(sc),
                                              ea, 2, out.data_ptr(), _lib.FMT_U8_HWC, ws.data_ptr(), ws.numel(), st)
                    assert rc == 0, rc
                return call
            other_eyes, this_eyes = raw_eyes(other), raw_eyes(_lib.load())
            mine = ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)[0].clone()
            other_eyes()
            torch.cuda.synchronize()
            same = bool(torch.equal(mine, out[:mine.numel()].view(mine.shape)))
            print(f"--ab-lib {a.ab_lib}: d2s_version {other.d2s_version()} (this build {_lib.load().d2s_version()}); its eye 0 is "
                  f"{'bit-identical to' if same else 'DIFFERENT from'} this build's", flush=True)
            runs = dict({"other_lib_eyes": other_eyes, "this_lib_eyes": this_eyes}, **runs, other_lib_eyes_again=other_eyes, this_lib_eyes_again=this_eyes)
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {a.frost} {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, medians of {a.rounds} rounds x {a.iters} launches; the screen covers "
              f"{share_screen:.3f} of the images, the walls change {share_wall:.3f}:", flush=True)
        for k in runs:
            per = f"{1e3 * med[k] / (B * n_px):.4f} ns / image pixel" if k != "mip_chain" else f"{B * a.height * a.width * 3 / med[k] / 1e3:.1f} GB/s of the frame"
            print(f"    {k:26s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f}; {per})", flush=True)
        print(f"    new entry, frost off - old entry = {med['eyes_new_entry_frost_off'] - med['eyes_old_entry']:+.1f} us; old entry against itself: "
              f"{med['eyes_old_entry_again'] - med['eyes_old_entry']:+.1f} us", flush=True)
        if a.ab_lib:
            margin = abs(med["other_lib_eyes_again"] - med["other_lib_eyes"])
            worst = max(med["this_lib_eyes"], med["this_lib_eyes_again"]) - max(med["other_lib_eyes"], med["other_lib_eyes_again"])
            print(f"    other build against itself: {med['other_lib_eyes_again'] - med['other_lib_eyes']:+.1f} us (the margin: {margin:.1f} us); this build's "
                  f"slower run - the other's slower run = {worst:+.1f} us: {'within' if worst <= margin else 'BEYOND'} the margin", flush=True)
    for B in a.batch if a.frost and a.curve else ():
        import ctypes as C
        import dataclasses
        from desktop2stereo_amd import _lib
        flat = dataclasses.replace(screen, curve="flat")
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        frost = xr.XrFrost.veil() if a.frost == "veil" else xr.XrFrost.frosted(time=1.0)
        glow = xr.XrGlow("glow", xr.glow_range_m(screen))
        levels = ops.mip_chain(f)
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        probe_s = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)      # clear alpha 0.5 marks the pixels nothing drew
        probe_f = ops.dibr_xr_eyes_frost_curved(f[:1], d[:1], dp, screen, eyes, frost, levels[:1], out_u8=False)
        n_px = 2 * ew * eh
        share_screen = sum(int((e[..., 3] != 0.5).sum()) for e in probe_s) / n_px
        share_wall = sum(int((p != q).any(-1).sum()) for p, q in zip(probe_s, probe_f)) / n_px

        def all_rows():      # D2S_XR_BIN=0 is read at the call
            os.environ["D2S_XR_BIN"] = "0"
            ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, out=out)
            del os.environ["D2S_XR_BIN"]
        runs = {"a_curved_plain": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                f"b_flat_{a.frost}": lambda: ops.dibr_xr_eyes_frost(f, d, dp, flat, eyes, frost, levels, out=out),
                "c_flat_plain": lambda: ops.dibr_xr_eyes(f, d, dp, flat, eyes, out=out),
                f"curved_{a.frost}": lambda: ops.dibr_xr_eyes_frost_curved(f, d, dp, screen, eyes, frost, levels, out=out),
                f"curved_{a.frost}_all_rows": all_rows,
                "curved_glow": lambda: ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, out=out),
                "a_curved_plain_again": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)}
        pairs = []
        if a.ab_lib:      # the other build's plain, glow and flat-frost calls on the same tensors and stream, through ctypes alone
            other = C.CDLL(os.path.abspath(a.ab_lib))
            other.d2s_version.restype = C.c_int
            sc, fl, ea = screen.c_struct(), flat.c_struct(), xr.eye_array(eyes)
            gs, fs = glow.c_struct(), frost.c_struct()
            ws = torch.empty(2 * 52 * 96, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream

            def raw(lib, name, scr, extra):      # both builds through the SAME host path: the C call alone
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = _lib.SYMBOLS[name]

                def call():
                    rc = fn(f.data_ptr(), d.data_ptr(), d.shape[1], d.shape[2], B, a.height, a.width, C.byref(dp), None, C.byref(scr), ea, 2,
                            out.data_ptr(), _lib.FMT_U8_HWC, ws.data_ptr(), ws.numel(), *extra, st)
                    assert rc == 0, rc
                return call
            print(f"--ab-lib {a.ab_lib}: d2s_version {other.d2s_version()} (this build {_lib.load().d2s_version()})", flush=True)
            for label, name, scr, extra in (("plain_curved", "d2s_dibr_xr_eyes", sc, ()),
                                            ("glow_curved", "d2s_dibr_xr_eyes_glow_curved", sc, (C.byref(gs), levels.data_ptr())),
                                            (f"flat_{a.frost}", "d2s_dibr_xr_eyes_frost", fl, (C.byref(fs), levels.data_ptr()))):
                o, m = raw(other, name, scr, extra), raw(_lib.load(), name, scr, extra)
                m(); torch.cuda.synchronize(); mine = out.clone()
                o(); torch.cuda.synchronize()
                print(f"    {label}: the other build's output is {'bit-identical to' if torch.equal(mine, out) else 'DIFFERENT from'} this build's", flush=True)
                runs.update({f"other_{label}": o, f"this_{label}": m, f"other_{label}_again": o, f"this_{label}_again": m})
                pairs.append(label)
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {screen.curve} {a.frost} {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, medians of {a.rounds} rounds x {a.iters} launches; the "
              f"screen covers {share_screen:.3f} of the images, the walls change {share_wall:.3f}:", flush=True)
        for k in runs:
            print(f"    {k:30s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f}; {1e3 * med[k] / (B * n_px):.4f} ns / image pixel)", flush=True)
        ceiling = med["a_curved_plain"] + med[f"b_flat_{a.frost}"] - med["c_flat_plain"]
        print(f"    ceiling (a) + (b) - (c) = {ceiling:.1f} us; curved {a.frost} - ceiling = {med[f'curved_{a.frost}'] - ceiling:+.1f} us "
              f"({100.0 * (med[f'curved_{a.frost}'] / ceiling - 1.0):+.1f} %); all 244 rows per pixel (D2S_XR_BIN=0): {med[f'curved_{a.frost}_all_rows']:.1f} us; "
              f"(a) against itself {med['a_curved_plain_again'] - med['a_curved_plain']:+.1f} us", flush=True)
        for label in pairs:
            margin = abs(med[f"other_{label}_again"] - med[f"other_{label}"])
            worst = max(med[f"this_{label}"], med[f"this_{label}_again"]) - max(med[f"other_{label}"], med[f"other_{label}_again"])
            print(f"    {label}: other build against itself {med[f'other_{label}_again'] - med[f'other_{label}']:+.1f} us (the margin: {margin:.1f} us); this "
                  f"build's slower run - the other's slower run = {worst:+.1f} us: {'within' if worst <= margin else 'BEYOND'} the margin", flush=True)
    for B in a.batch if a.glow and a.curve and not a.frost else ():
        import dataclasses
        flat = dataclasses.replace(screen, curve="flat")
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        glow = xr.XrGlow(a.glow, a.glow_range if a.glow_range else xr.glow_range_m(screen))
        levels = ops.mip_chain(f)
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        probe_s = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)      # clear alpha 0.5 marks the pixels nothing drew
        probe_g = ops.dibr_xr_eyes_glow_curved(f[:1], d[:1], dp, screen, eyes, glow, levels[:1], out_u8=False)
        n_px = 2 * ew * eh
        share_screen = sum(int((e[..., 3] != 0.5).sum()) for e in probe_s) / n_px
        share_drawn = sum(int((e[..., 3] != 0.5).sum()) for e in probe_g) / n_px
        runs = {"a_curved_no_glow": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                "b_flat_glow": lambda: ops.dibr_xr_eyes_glow(f, d, dp, flat, eyes, glow, levels, out=out),
                "c_flat_no_glow": lambda: ops.dibr_xr_eyes(f, d, dp, flat, eyes, out=out),
                f"curved_{a.glow}": lambda: ops.dibr_xr_eyes_glow_curved(f, d, dp, screen, eyes, glow, levels, out=out),
                "a_curved_no_glow_again": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out)}
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {screen.curve} {a.glow} (range {glow.range_m:.2f} m) {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, medians of {a.rounds} rounds x "
              f"{a.iters} launches; the screen covers {share_screen:.3f} of the images, screen + glow {share_drawn:.3f}:", flush=True)
        for k in runs:
            print(f"    {k:26s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f}; {1e3 * med[k] / (B * n_px):.4f} ns / image pixel)", flush=True)
        ceiling = med["a_curved_no_glow"] + med["b_flat_glow"] - med["c_flat_no_glow"]
        spread = max((max(v) - min(v)) / med[k] for k, v in t.items())
        print(f"    ceiling (a) + (b) - (c) = {ceiling:.1f} us; curved {a.glow} - ceiling = {med[f'curved_{a.glow}'] - ceiling:+.1f} us "
              f"({100.0 * (med[f'curved_{a.glow}'] / ceiling - 1.0):+.1f} %); (a) against itself {med['a_curved_no_glow_again'] - med['a_curved_no_glow']:+.1f} us; "
              f"largest (max - min) / median of a row {100.0 * spread:.1f} %", flush=True)
    for B in a.batch if a.glow and not a.curve and not a.frost else ():
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        glow = xr.XrGlow(a.glow, a.glow_range if a.glow_range else xr.glow_range_m(screen))
        levels = ops.mip_chain(f)
        out = torch.empty(ops.dibr_xr_shape(eyes, B, dp.alpha_mode)[1], dtype=torch.uint8, device=dev)
        runs = {"eyes_old_entry": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                "eyes_new_entry_glow_off": lambda: ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, None, None, out=out),
                f"eyes_{a.glow}": lambda: ops.dibr_xr_eyes_glow(f, d, dp, screen, eyes, glow, levels, out=out),
                "eyes_old_entry_again": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes, out=out),
                "mip_chain": lambda: ops.mip_chain(f, out=levels)}
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {a.glow} (range {glow.range_m:.2f} m) {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}, medians of {a.rounds} rounds x {a.iters} launches:", flush=True)
        for k in runs:
            per = f"{1e3 * med[k] / (B * 2 * ew * eh):.4f} ns / image pixel" if k != "mip_chain" else f"{B * a.height * a.width * 3 / med[k] / 1e3:.1f} GB/s of the frame"
            print(f"    {k:26s} {med[k]:8.1f} us  (min {min(t[k]):.1f} max {max(t[k]):.1f}; {per})", flush=True)
        print(f"    new entry, glow off - old entry = {med['eyes_new_entry_glow_off'] - med['eyes_old_entry']:+.1f} us; old entry against itself: "
              f"{med['eyes_old_entry_again'] - med['eyes_old_entry']:+.1f} us", flush=True)
    for B in () if a.glow or a.frost else a.batch:
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        probe = ops.dibr_xr_eyes(f[:1], d[:1], dp, screen, eyes, out_u8=False)      # clear alpha 0.5 marks the uncovered pixels
        covered = B * sum(int((e[..., 3] != 0.5).sum()) for e in probe)
        runs = {"xr_eyes": lambda: ops.dibr_xr_eyes(f, d, dp, screen, eyes), "cropped_warp_gather": lambda: ops.dibr_warp(f, d, dp, crop=(0.0, 0.0, 1.0, 1.0))}
        px = {"xr_eyes": covered, "cropped_warp_gather": B * 2 * a.height * a.width}
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"xr-eye {screen.curve} {a.height}x{a.width} -> 2 x {ew}x{eh} B={B}: covered {covered / (B * 2 * ew * eh):.3f} of the images "
              f"({covered // B} pixels, the cropped warp {2 * a.height * a.width})  " +
              "  ".join(f"{k} {med[k]:8.1f} us ({1e3 * med[k] / px[k]:.4f} ns / covered pixel; min {min(t[k]):.1f} max {max(t[k]):.1f})" for k in runs) +
              f"   xr / cropped per covered pixel = {med['xr_eyes'] / px['xr_eyes'] / (med['cropped_warp_gather'] / px['cropped_warp_gather']):.3f}", flush=True)
    sys.exit(0)
if a.crop is not None:
    from desktop2stereo_amd import crop as K
    if len(a.crop) not in (0, 4):
        sys.exit("--crop takes no values or x y w h")
    bar = round((a.height - a.width / 2.39) / 2) + max(2, min(8, round(a.height * 0.004)))
    crop = tuple(a.crop) if a.crop else (0.0, bar / a.height, 1.0, (a.height - 2 * bar) / a.height)
    x0, y0, x1, y1 = K.pixel_bounds(a.width, a.height, crop)
    img, dep = synth.dibr_scene(a.height, a.width, 11, a.kind)
    dp = ops.dibr_params(display_mode=a.mode, corner_radius=a.corner_radius, alpha="rgba" if a.corner_radius > 0 else "window")
    for B in a.batch:
        f = torch.from_numpy(img).to(dev)[None].expand(B, -1, -1, -1).contiguous()
        d = torch.from_numpy(dep).to(dev)[None].expand(B, -1, -1).contiguous()
        fc, dc = f[:, y0:y1, x0:x1].contiguous(), d[:, y0:y1, x0:x1].contiguous()
        runs = {"cropped": lambda: ops.dibr_warp(f, d, dp, crop=crop), "uncropped_at_crop_size": lambda: ops.dibr_warp(fc, dc, dp)}
        px = {k: fn().numel() // fn().shape[-1] for k, fn in runs.items()}
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                for _ in range(3): fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        print(f"{a.mode} {a.height}x{a.width} crop {tuple(round(c, 4) for c in crop)} -> eye {y1 - y0}x{x1 - x0} B={B}: " +
              "  ".join(f"{k} {med[k]:8.1f} us ({1e3 * med[k] / px[k]:.4f} ns / output pixel)" for k in runs) +
              f"   cropped / uncropped per pixel = {med['cropped'] / px['cropped'] / (med['uncropped_at_crop_size'] / px['uncropped_at_crop_size']):.3f}",
              flush=True)
    sys.exit(0)
img, dep = synth.dibr_scene(a.height, a.width, 11, a.kind)
f1, d1 = torch.from_numpy(img).to(dev)[None], torch.from_numpy(dep).to(dev)[None]
dp = ops.dibr_params(display_mode=a.mode, viewport=tuple(a.viewport) if a.viewport else (0.0, 0.0, 0.0, 0.0))
if a.composite:
    run = lambda f, d: ops.dibr_composite(None if a.composite == "Depth Map" else f, d, dp, a.composite)
    a.mode = a.composite
else:
    run = lambda f, d: ops.dibr_warp(f, d, dp)
for B in a.batch:
    f, d = f1.expand(B, -1, -1, -1).contiguous(), d1.expand(B, -1, -1).contiguous()
    for _ in range(3): out = run(f, d)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(20): run(f, d)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 20
    nbytes = B * (a.height * a.width * (4 if a.composite == "Depth Map" else 7)) + out.numel()
    print(f"{a.mode} {a.kind} B={B}: {us:8.1f} us / launch  {us / B:7.1f} us / frame  {nbytes / us / 1e3:7.1f} GB/s = {nbytes / us / 1e3 / 8000:.3f} of 8 TB/s", flush=True)
