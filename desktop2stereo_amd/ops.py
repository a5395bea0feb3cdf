"""Stage-level host wrappers over the C-ABI (include/d2s.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every computation
is a call into libd2s_hip.so with ``tensor.data_ptr()`` (the same convention as the reference's
MIGraphXEngine.__call__, reference depth.py:1029-1045).  Nothing in this module computes with
torch ops, and nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import (FMT_F32_CHW, FMT_F32_HWC, FMT_U8_CHW, FMT_U8_HWC, MODE, PREC_BF16, PREC_FP32,
                   ModelDesc, PostParams, PreParams, SbsParams, check)
from .config import IMAGENET_MEAN, IMAGENET_STD, ModelConfig, PipelineParams, engine_shape


class _on:
    """Scope of one native call on `device`: the HIP current device is per host thread and the reference issues
    predict_depth and make_sbs from different threads, so the device of the tensors is made
    current around the call and the stream handed to the library is THAT device's current stream (not the calling
    thread's default device's).  `with _on(t.device) as st: lib.d2s_...(..., st)`."""

    def __init__(self, device: torch.device):
        self.device = device
        self.guard = torch.cuda.device(device)

    def __enter__(self) -> C.c_void_p:
        self.guard.__enter__()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def _same_device(a: torch.Tensor, b: torch.Tensor, what: str):
    if a.device != b.device:
        raise _lib.D2SError(f"{what}: tensors on different devices ({a.device} vs {b.device})")


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _need_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _lib.D2SError(f"{what} must be a ROCm device tensor (no CPU path in this package)")


def post_params(p: PipelineParams) -> PostParams:
    return PostParams(p.percentile, p.subsample_cap, p.gamma, p.foreground_scale, p.aa_strength, p.ema_alpha,
                      int(bool(p.metric)))


def pre_params(mean=IMAGENET_MEAN, std=IMAGENET_STD, resample: str = "bilinear", square: bool = False) -> PreParams:
    if resample not in _lib.RESAMPLE:
        raise ValueError(f"resample must be one of {list(_lib.RESAMPLE)}")
    return PreParams((C.c_float * 3)(*mean), (C.c_float * 3)(*std), _lib.RESAMPLE[resample], int(bool(square)))


def sbs_params(ipd_uv=0.064, depth_ratio=2.0, convergence=0.0, display_mode="Half-SBS", fill_16_9=False) -> SbsParams:
    if display_mode not in MODE:
        raise ValueError(f"display_mode must be one of {list(MODE)}")
    return SbsParams(float(ipd_uv), float(depth_ratio), float(convergence), MODE[display_mode], int(bool(fill_16_9)))


def sbs_shape(H: int, W: int, sp: SbsParams) -> Tuple[int, int]:
    oh, ow = C.c_int(), C.c_int()
    check(_lib.load().d2s_sbs_shape(H, W, C.byref(sp), C.byref(oh), C.byref(ow)), "d2s_sbs_shape")
    return oh.value, ow.value


def _frame_fmt(t: torch.Tensor) -> Tuple[int, int, int, int]:
    """(fmt, batch, H, W) of a frame tensor: u8 HWC / u8 CHW / f32 CHW, optional leading batch."""
    if t.dtype == torch.uint8 and t.shape[-1] == 3 and t.dim() in (3, 4):
        b = t.shape[0] if t.dim() == 4 else 1
        return FMT_U8_HWC, b, t.shape[-3], t.shape[-2]
    if t.shape[-3] == 3 and t.dim() in (3, 4):
        b = t.shape[0] if t.dim() == 4 else 1
        if t.dtype == torch.uint8:
            return FMT_U8_CHW, b, t.shape[-2], t.shape[-1]
        if t.dtype == torch.float32:
            return FMT_F32_CHW, b, t.shape[-2], t.shape[-1]
    raise ValueError(f"unsupported frame tensor {tuple(t.shape)} {t.dtype}: want uint8 [..,H,W,3], uint8/float32 [..,3,H,W]")


def process(img_bgr: torch.Tensor, target_height: int) -> torch.Tensor:
    """A1 (reference depth.py:540-566): uint8 HWC BGR(A) device tensor -> float32 CHW RGB 0..255, anti-aliased
    bilinear down-scale to even dims when target_height < H0."""
    _need_cuda(img_bgr, "img")
    if img_bgr.dtype != torch.uint8 or img_bgr.dim() != 3 or img_bgr.shape[-1] not in (3, 4):
        raise ValueError(f"process(): want uint8 [H,W,3|4] (BGR / BGRA), got {tuple(img_bgr.shape)} {img_bgr.dtype}")
    img_bgr = img_bgr.contiguous()
    H0, W0, ch = img_bgr.shape
    lib = _lib.load()
    oh, ow = C.c_int(), C.c_int()
    check(lib.d2s_process_shape(H0, W0, int(target_height), C.byref(oh), C.byref(ow)), "d2s_process_shape")
    out = torch.empty((3, oh.value, ow.value), dtype=torch.float32, device=img_bgr.device)
    with _on(img_bgr.device) as st:
        check(lib.d2s_process(_ptr(img_bgr), ch, H0, W0, int(target_height), _ptr(out), st), "d2s_process")
    return out


def process_rgb(img: torch.Tensor, target_height: int) -> torch.Tensor:
    """A1, tensor branch of the reference's non-CUDA process() (depth.py:576-601): RGB capture tensor [3|4,H,W] or [H,W,>=3]
    (uint8 or float32) -> first three channels as CHW; target_height < H0: float32 bilinear (no antialias) down-scale to even
    dims; else the frame itself (dtype unchanged, like the reference)."""
    _need_cuda(img, "img")
    if img.dim() != 3:
        raise ValueError(f"Unsupported tensor image shape: {tuple(img.shape)}")
    if img.shape[0] in (3, 4):
        chw, ch, H0, W0 = True, img.shape[0], img.shape[1], img.shape[2]
    elif img.shape[-1] >= 3:
        chw, ch, H0, W0 = False, img.shape[2], img.shape[0], img.shape[1]
    else:
        raise ValueError(f"Unsupported tensor image shape: {tuple(img.shape)}")
    if target_height >= H0:                                       # depth.py:586-587: returned as is (no resize, no cast)
        return img[:3] if chw else img[..., :3].permute(2, 0, 1).contiguous()
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    if not chw and (img.dtype != torch.uint8 or ch > 4):
        img, chw, ch = img[..., :3].permute(2, 0, 1), True, 3      # float HWC / wide HWC: plane view first
    img = img.contiguous()
    fmt = (FMT_U8_CHW if img.dtype == torch.uint8 else FMT_F32_CHW) if chw else FMT_U8_HWC
    lib = _lib.load()
    oh, ow = C.c_int(), C.c_int()
    check(lib.d2s_process_shape(H0, W0, int(target_height), C.byref(oh), C.byref(ow)), "d2s_process_shape")
    out = torch.empty((3, oh.value, ow.value), dtype=torch.float32, device=img.device)
    with _on(img.device) as st:
        check(lib.d2s_process_rgb(_ptr(img), fmt, ch, H0, W0, int(target_height), _ptr(out), st), "d2s_process_rgb")
    return out


def process_area(img_bgr: torch.Tensor, target_height: int) -> torch.Tensor:
    """A1, numpy branch of the reference's non-CUDA process() (depth.py:603-629): uint8 HWC BGR(A) device tensor -> uint8 HWC RGB,
    cv2.resize(INTER_AREA) to (int(W0*height/H0), height) when height < H0."""
    _need_cuda(img_bgr, "img")
    if img_bgr.dtype != torch.uint8 or img_bgr.dim() != 3 or img_bgr.shape[-1] not in (3, 4):
        raise ValueError(f"process(): want uint8 [H,W,3|4] (BGR / BGRA), got {tuple(img_bgr.shape)} {img_bgr.dtype}")
    img_bgr = img_bgr.contiguous()
    H0, W0, ch = img_bgr.shape
    lib = _lib.load()
    oh, ow = C.c_int(), C.c_int()
    check(lib.d2s_process_area_shape(H0, W0, int(target_height), C.byref(oh), C.byref(ow)), "d2s_process_area_shape")
    out = torch.empty((oh.value, ow.value, 3), dtype=torch.uint8, device=img_bgr.device)
    with _on(img_bgr.device) as st:
        check(lib.d2s_process_area(_ptr(img_bgr), ch, H0, W0, int(target_height), _ptr(out), st), "d2s_process_area")
    return out


def overlay_text(frame: torch.Tensor, text: str) -> torch.Tensor:
    """A15 (reference depth.py:2061-2103): paint `text` in the reference's 5x3 font, green, IN PLACE on one frame."""
    _need_cuda(frame, "frame")
    if not frame.is_contiguous():
        raise ValueError("overlay_text paints in place: the frame must be contiguous")
    if frame.dtype == torch.float32 and frame.dim() == 3 and frame.shape[-1] == 3 and frame.shape[0] != 3:
        fmt, H, W = FMT_F32_HWC, frame.shape[0], frame.shape[1]
    else:
        fmt, B, H, W = _frame_fmt(frame)
        if B != 1:
            raise ValueError("overlay_text takes one frame")
    with _on(frame.device) as st:
        check(_lib.load().d2s_overlay_text(_ptr(frame), fmt, H, W, text.encode(), st), "d2s_overlay_text")
    return frame


def preprocess(frames: torch.Tensor, target: int, patch: int = 14, mean=IMAGENET_MEAN, std=IMAGENET_STD,
               resample: str = "bilinear", square: bool = False) -> torch.Tensor:
    """A2-A4 (reference depth.py:676-706, 1916-1948) -> float32 [B,3,h,w].  resample: "bilinear" = the CPU branch of
    _resize_patch_aligned_t (decimation + bilinear), "bicubic_aa" = its IS_CUDA branch (depth.py:698-699).
    square=True: the fixed-square branch (get_patch_size() is None, CAPTURE_MODE "Window"; depth.py:1937-1946): plain bilinear
    of the full frame to target x target."""
    _need_cuda(frames, "frames")
    frames = frames.contiguous()
    fmt, B, H, W = _frame_fmt(frames)
    h, w, stride = engine_shape(H, W, target, patch, square)
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=frames.device)
    pre = pre_params(mean, std, resample, square)
    with _on(frames.device) as st:
        check(_lib.load().d2s_preprocess(_ptr(frames), fmt, B, H, W, _ptr(out), h, w, stride, C.byref(pre), st), "d2s_preprocess")
    return out


def _post_process(depth: torch.Tensor, p: PipelineParams, in_place: bool) -> torch.Tensor:
    _need_cuda(depth, "depth")
    d = depth.to(torch.float32).contiguous()
    out = d.clone() if in_place else torch.empty_like(d)
    B = d.shape[0] if d.dim() == 3 else 1
    h, w = d.shape[-2:]
    lib = _lib.load()
    nbytes = lib.d2s_post_process_workspace(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d.device)
    pp = post_params(p)
    with _on(d.device) as st:
        if in_place:
            check(lib.d2s_post_process(_ptr(out), B, h, w, C.byref(pp), _ptr(ws), nbytes, st), "d2s_post_process")
        else:
            check(lib.d2s_post_process_to(_ptr(d), _ptr(out), B, h, w, C.byref(pp), _ptr(ws), nbytes, st), "d2s_post_process_to")
    return out


def post_process_depth(depth: torch.Tensor, p: PipelineParams) -> torch.Tensor:
    """A10-A11 (reference depth.py:806-814) on float32 [B,h,w] or [h,w]; returns a new tensor (the library works in place on a copy)."""
    return _post_process(depth, p, True)


def post_process_depth_to(depth: torch.Tensor, p: PipelineParams) -> torch.Tensor:
    """The same out of place (with few frames the one-launch form runs); the input is left untouched."""
    return _post_process(depth, p, False)


def post_plan(batch: int, h: int, w: int, p: PipelineParams, in_place: bool = False) -> dict:
    """What d2s_post_process_to would launch for these arguments (include/d2s.h d2s_post_plan; host code, no GPU): the form, the kernel
    names and their dynamic LDS bytes, the taps and the subsample."""
    r = _lib.PostPlanResult()
    r.struct_size = C.sizeof(_lib.PostPlanResult)
    pp = post_params(p)
    check(_lib.load().d2s_post_plan(int(batch), int(h), int(w), C.byref(pp), int(bool(in_place)), C.byref(r)), "d2s_post_plan")
    return {"form": _lib.POST_FORM[r.form], "kernels": [r.kernel[i].value.decode() for i in range(r.launches)],
            "lds_bytes": list(r.lds_bytes[:r.launches]), "k": r.k, "r": r.r, "step": r.step, "m": r.m, "tail": r.tail}


def ema_update(depth: torch.Tensor, state: torch.Tensor, initialised: bool, alpha: float) -> torch.Tensor:
    """A12 (reference depth.py:1865-1887); depth [h,w] is overwritten with the returned value."""
    h, w = depth.shape
    _same_device(depth, state, "ema_update")
    with _on(depth.device) as st:
        check(_lib.load().d2s_ema_update(_ptr(depth), _ptr(state), int(initialised), h, w, alpha, st), "d2s_ema_update")
    return depth


def upsample_depth(depth: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """A13 (reference depth.py:1999-2004): [B,h,w] or [h,w] -> same rank at H x W."""
    _need_cuda(depth, "depth")
    d = depth.to(torch.float32).contiguous()
    B = d.shape[0] if d.dim() == 3 else 1
    h, w = d.shape[-2:]
    out = torch.empty((B, H, W) if d.dim() == 3 else (H, W), dtype=torch.float32, device=d.device)
    with _on(d.device) as st:
        check(_lib.load().d2s_upsample_depth(_ptr(d), B, h, w, _ptr(out), H, W, st), "d2s_upsample_depth")
    return out


def _sbs_out_spec(B: int, oh: int, ow: int, out_fmt: int):
    """(shape, dtype) of a make_sbs / Engine.pipeline result in out_fmt."""
    return (B, 3, oh, ow) if out_fmt == FMT_F32_CHW else (B, oh, ow, 3), torch.uint8 if out_fmt == FMT_U8_HWC else torch.float32


def make_sbs(frames: torch.Tensor, depth: torch.Tensor, sp: SbsParams, out_fmt: int = FMT_U8_HWC, out: torch.Tensor = None) -> torch.Tensor:
    """A14 (+A13 fused when depth is at model resolution) (reference depth.py:2122-2184).  `out`: a caller-allocated result (the
    C-ABI's own convention), shape [B, oh, ow, 3] / [B, 3, oh, ow] of the format's dtype."""
    _need_cuda(frames, "frames")
    _need_cuda(depth, "depth")
    _same_device(frames, depth, "make_sbs")
    frames = frames.contiguous()
    d = depth.to(torch.float32).contiguous()
    fmt, B, H, W = _frame_fmt(frames)
    dB = d.shape[0] if d.dim() == 3 else 1
    if dB != B:
        raise ValueError("frames / depth batch mismatch")
    dh, dw = d.shape[-2:]
    oh, ow = sbs_shape(H, W, sp)
    batched = frames.dim() == 4
    want = _sbs_out_spec(B, oh, ow, out_fmt)
    if out is not None:
        if tuple(out.shape) != want[0] or out.dtype != want[1] or not out.is_contiguous() or out.device != frames.device:
            raise ValueError(f"make_sbs: out must be a contiguous {want[1]} tensor of shape {want[0]} on {frames.device}")
    elif out_fmt not in (FMT_U8_HWC, FMT_F32_HWC, FMT_F32_CHW):
        raise ValueError("bad out_fmt")
    else:
        out = torch.empty(want[0], dtype=want[1], device=frames.device)
    with _on(frames.device) as st:
        check(_lib.load().d2s_make_sbs(_ptr(frames), fmt, _ptr(d), dh, dw, B, H, W, C.byref(sp), _ptr(out), out_fmt, st),
              "d2s_make_sbs")
    return out if batched else out[0]


def dibr_params(ipd_uv=0.064, depth_ratio=1.0, convergence=0.0, display_mode="Full-SBS", roll=0.0, feather=False,
                viewer_depth_strength=0.1, search_radius=12.0, depth_tolerance=0.012, blur_radius=2.5,
                feather_width=0.02, resolution=(0.0, 0.0), corner_radius=0.0, viewport=(0.0, 0.0, 0.0, 0.0),
                alpha="window") -> _lib.DibrParams:
    """Uniform block of the reference's DIBR shader with the viewer's defaults (viewer.py:1333-1343, 402-411).
    corner_radius: u_corner_radius (0 desktop viewer, 0.03 OpenXR screen); viewport: u_viewport (x, y, w, h) in pixels of
    the eye image, y up -- zeros = the eye image itself.  alpha: "window" = frag_color.rgb as the reference's window shows it
    (its stereo quads are drawn with blending off), "premultiplied" = rgb * a, "rgba" = four channels (include/d2s.h)."""
    if display_mode not in MODE:
        raise ValueError(f"display_mode must be one of {list(MODE)}")
    if alpha not in _lib.DIBR_ALPHA:
        raise ValueError(f"alpha must be one of {list(_lib.DIBR_ALPHA)}")
    return _lib.DibrParams(float(ipd_uv), float(viewer_depth_strength * depth_ratio), float(convergence), float(roll),
                           float(search_radius), float(depth_tolerance), float(blur_radius), float(resolution[0]),
                           float(resolution[1]), MODE[display_mode], int(bool(feather)), float(feather_width),
                           float(corner_radius), (C.c_float * 4)(*[float(v) for v in viewport]), _lib.DIBR_ALPHA[alpha],
                           C.sizeof(_lib.DibrParams))


def _crop4(crop) -> "C.Array":
    if len(crop) != 4:
        raise ValueError("crop must be (x, y, w, h) in uv of the source, top-left origin")
    return (C.c_double * 4)(*[float(v) for v in crop])


def dibr_crop_shape(H: int, W: int, crop, display_mode: int) -> Tuple[int, int]:
    oh, ow = C.c_int(), C.c_int()
    check(_lib.load().d2s_dibr_crop_shape(H, W, _crop4(crop), display_mode, C.byref(oh), C.byref(ow)), "d2s_dibr_crop_shape")
    return oh.value, ow.value


_CROP_WS: Dict[Tuple, torch.Tensor] = {}


def crop_detect_workspace(B: int, H: int, W: int, device) -> torch.Tensor:
    """A workspace for crop_detect(workspace=) on [B,.,H,W] frames: the detector's partial sums live there between its two launches, so
    calls that may overlap (different streams) must not share one."""
    nbytes = C.c_uint64()
    check(_lib.load().d2s_crop_detect_workspace(B, H, W, C.byref(nbytes)), "d2s_crop_detect_workspace")
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def crop_detect(frames: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The OpenXR viewer's letterbox / pillarbox detector (reference xr_viewer/crop.py:368-435, tensor path): device frames, uint8
    [B,H,W,3] / uint8 [B,3,H,W] / float32 [B,3,H,W] (or one frame without the batch axis) -> device float32 [B,6] (or [6]) =
    (top_i, bottom_count, center_mean, center_bright, left_i, right_count) per frame, two launches on the current stream, no
    synchronisation.  crop.crop_from_stats turns a row into the crop rectangle.  out: a caller-kept [B,6] float32 device tensor.
    workspace: a caller-kept crop_detect_workspace (MovieCrop owns one per capture); None: one kept here per (device, current
    stream, batch, size) -- calls on one stream are ordered, calls on different streams never share partial sums."""
    _need_cuda(frames, "frames")
    fmt, B, H, W = _frame_fmt(frames)
    batched = frames.dim() == 4
    f = frames.contiguous()
    lib = _lib.load()
    nbytes = C.c_uint64()
    check(lib.d2s_crop_detect_workspace(B, H, W, C.byref(nbytes)), "d2s_crop_detect_workspace")
    if workspace is not None:
        ws = workspace
        if not ws.is_cuda or ws.device != f.device or not ws.is_contiguous() or ws.numel() * ws.element_size() < nbytes.value:
            raise ValueError(f"crop_detect: workspace must be a contiguous tensor of >= {nbytes.value} bytes on {f.device}")
    else:
        key = (f.device, torch.cuda.current_stream(f.device).cuda_stream, B, H, W)
        ws = _CROP_WS.get(key)
        if ws is None:
            if len(_CROP_WS) >= 16:      # (capture sizes come and go; a workspace is ~0.1 MB per frame)
                _CROP_WS.clear()
            ws = _CROP_WS[key] = torch.empty(nbytes.value, dtype=torch.uint8, device=f.device)
    if out is None:
        out = torch.empty((B, 6), dtype=torch.float32, device=f.device)
    elif not out.is_cuda or out.device != f.device or out.dtype != torch.float32 or out.numel() != B * 6 or not out.is_contiguous():
        raise ValueError(f"crop_detect: out must be a contiguous float32 [{B},6] tensor on {f.device}")
    with _on(f.device) as st:
        check(lib.d2s_crop_detect(_ptr(f), fmt, B, H, W, _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), st), "d2s_crop_detect")
    return out if batched else out.view(-1)


def _dibr_out_spec(B: int, oh: int, ow: int, dp: "_lib.DibrParams", out_u8: bool):
    """(shape, dtype, D2S_FMT_*) of a dibr_warp / dibr_composite / Engine.view_pipeline result: three channels, four with alpha "rgba"."""
    nch = 4 if dp.alpha_mode == _lib.DIBR_ALPHA["rgba"] else 3
    return (B, oh, ow, nch), torch.uint8 if out_u8 else torch.float32, FMT_U8_HWC if out_u8 else FMT_F32_HWC


def dibr_warp(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", out_u8: bool = True, crop=None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f1 (reference viewer.py:386-631): uint8 HWC frames [B,H,W,3] or [H,W,3] + depth [B,dh,dw] or [dh,dw] -> both eyes
    with disocclusion in-painting, packed per dp.display_mode.  Depth of the frame's size is the shader's depth texture itself;
    any other size (the model's) is up-sampled inside the kernel, bit-identical to upsample_depth(depth, H, W) first.
    crop = (x, y, w, h) in uv, top-left origin: the OpenXR screen shader's u_source_crop (xr_viewer/implementation.py:111-126) --
    each eye is the crop's pixel size (crop.pixel_bounds), the texture taps follow the cropped coordinate.
    out: a caller-kept contiguous tensor of the result's batched shape [B, out_h, out_w, 3 | 4] and dtype (written in place)."""
    _need_cuda(frames, "frames")
    _need_cuda(depth, "depth")
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
        raise ValueError("dibr_warp: frames must be uint8 [B,H,W,3] or [H,W,3]")
    batched = frames.dim() == 4
    f = frames.contiguous() if batched else frames.contiguous().unsqueeze(0)
    d = depth.to(torch.float32).contiguous()
    d = d if d.dim() == 3 else d.unsqueeze(0)
    B, H, W, _ = f.shape
    if d.dim() != 3 or d.shape[0] != B:
        raise ValueError(f"dibr_warp: depth must be [{B},dh,dw] for frames {tuple(f.shape)}, got {tuple(d.shape)}")
    dh, dw = d.shape[1:]
    lib = _lib.load()
    oh, ow = C.c_int(), C.c_int()
    if crop is not None:
        c4 = _crop4(crop)
        check(lib.d2s_dibr_crop_shape(H, W, c4, dp.display_mode, C.byref(oh), C.byref(ow)), "d2s_dibr_crop_shape")
    else:
        check(lib.d2s_dibr_shape(H, W, dp.display_mode, C.byref(oh), C.byref(ow)), "d2s_dibr_shape")
    shape, dtype, fmt = _dibr_out_spec(B, oh.value, ow.value, dp, out_u8)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=f.device)
    elif tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != f.device:
        raise ValueError(f"dibr_warp: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {f.device}")
    _same_device(f, d, "dibr_warp")
    with _on(f.device) as st:
        if crop is not None:
            check(lib.d2s_dibr_warp_crop(_ptr(f), _ptr(d), dh, dw, B, H, W, C.byref(dp), c4, _ptr(out), fmt, st), "d2s_dibr_warp_crop")
        else:
            check(lib.d2s_dibr_warp_depth(_ptr(f), _ptr(d), dh, dw, B, H, W, C.byref(dp), _ptr(out), fmt, st), "d2s_dibr_warp_depth")
    return out if batched else out[0]


def dibr_warp_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", out_u8: bool = True, crop=None) -> dict:
    """What dibr_warp would launch for these arguments (include/d2s.h d2s_dibr_warp_plan; host code, no GPU): the kernel's name, whether
    it is the LDS-window row kernel, the window plan (cols, margin, WW), grid, block and the LDS request."""
    r = _lib.DibrWarpPlanResult()
    r.struct_size = C.sizeof(_lib.DibrWarpPlanResult)
    check(_lib.load().d2s_dibr_warp_plan(int(dh), int(dw), int(batch), int(H), int(W), C.byref(dp), None if crop is None else _crop4(crop),
                                         FMT_U8_HWC if out_u8 else FMT_F32_HWC, C.byref(r)), "d2s_dibr_warp_plan")
    return {"kernel": r.kernel.decode(), "rows": bool(r.rows), "cols": r.cols, "margin": r.margin, "WW": r.ww, "roll0": bool(r.roll0),
            "up": bool(r.up), "fx": bool(r.fx), "oh": r.oh, "ow": r.ow, "out_h": r.out_h, "out_w": r.out_w, "grid": tuple(r.grid),
            "block": r.block, "lds_dynamic": r.lds_dynamic_bytes, "lds_static": r.lds_static_bytes,
            "lds_bytes": r.lds_dynamic_bytes + r.lds_static_bytes}


_XR_WS: Dict[Tuple, torch.Tensor] = {}


class _XrEntry(NamedTuple):
    """One eye-view entry.  direct / pipeline: the function here and the Engine method, as messages name them -- the C entries are
    d2s_<direct> and d2s_<pipeline>_streams.  tail: what the C argument list has between workspace_bytes and the stream -- "" nothing,
    "glow" (glow, levels), "frost" (frost, levels), "panorama" (frost, levels, glow, panorama, pano_rgb, pano_levels)."""
    direct: str
    pipeline: str
    plan: str
    workspace: str
    tail: str


# (the two panorama entries draw whichever kind the looks ask for: the largest table's workspace serves them all)
_XR_ENTRIES = {
    "eyes": _XrEntry("dibr_xr_eyes", "view_pipeline_xr", "d2s_dibr_xr_plan", "d2s_dibr_xr_workspace", ""),
    "glow": _XrEntry("dibr_xr_eyes_glow", "view_pipeline_xr_glow", "d2s_dibr_xr_plan", "d2s_dibr_xr_workspace", "glow"),
    "glow_curved": _XrEntry("dibr_xr_eyes_glow_curved", "view_pipeline_xr_glow_curved", "d2s_dibr_xr_plan",
                            "d2s_dibr_xr_glow_curved_workspace", "glow"),
    "frost": _XrEntry("dibr_xr_eyes_frost", "view_pipeline_xr_frost", "d2s_dibr_xr_frost_plan", "d2s_dibr_xr_frost_workspace", "frost"),
    "frost_curved": _XrEntry("dibr_xr_eyes_frost_curved", "view_pipeline_xr_frost_curved", "d2s_dibr_xr_frost_curved_plan",
                             "d2s_dibr_xr_frost_curved_workspace", "frost"),
    "panorama": _XrEntry("dibr_xr_eyes_panorama", "view_pipeline_xr_panorama", "d2s_dibr_xr_panorama_plan",
                         "d2s_dibr_xr_frost_curved_workspace", "panorama"),
    "panorama_curved": _XrEntry("dibr_xr_eyes_panorama_curved", "view_pipeline_xr_panorama_curved", "d2s_dibr_xr_panorama_curved_plan",
                                "d2s_dibr_xr_frost_curved_workspace", "panorama"),
    # the pass over finished eye images: no frames, no view pipeline of its own (depth.xr_eye_views* chain it); tail: panels, textures
    "panels": _XrEntry("dibr_xr_panels", "", "d2s_dibr_xr_panels_plan", "d2s_dibr_xr_panels_workspace", "panels")}


def _xr_args(screen, eyes):
    """(d2s_xr_screen, d2s_xr_eye array) of an xr.XrScreen (or the struct itself) and 1 or 2 eye images (xr.xr_eye)."""
    from . import xr as _xr
    sc = screen if isinstance(screen, _lib.XrScreen) else screen.c_struct()
    ea = eyes if isinstance(eyes, C.Array) and getattr(eyes, "_type_", None) is _lib.XrEye else _xr.eye_array(eyes)
    return sc, ea


def dibr_xr_shape(eyes, batch: int, alpha_mode: int = 0) -> Tuple[list, int]:
    """(offsets, total) in elements of the eye images of dibr_xr_eyes laid one after another: eye i is [batch, height_i, width_i, nch] at
    offsets[i] (d2s_dibr_xr_shape)."""
    from . import xr as _xr
    ea = eyes if isinstance(eyes, C.Array) else _xr.eye_array(eyes)
    offs, total = (C.c_uint64 * len(ea))(), C.c_uint64()
    check(_lib.load().d2s_dibr_xr_shape(ea, len(ea), int(batch), int(alpha_mode), offs, C.byref(total)), "d2s_dibr_xr_shape")
    return list(offs), total.value


def _xr_workspace(n_eyes: int, device, query: str = "d2s_dibr_xr_workspace") -> torch.Tensor:
    """The facet table's home for calls on the current stream of `device`: one per (device, stream), since calls on one stream are
    ordered and calls on different streams must not share it.  query: the size query of the call it serves."""
    nbytes = C.c_uint64()
    check(getattr(_lib.load(), query)(n_eyes, C.byref(nbytes)), query)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _XR_WS.get(key)
    if ws is None or ws.numel() < nbytes.value:
        if len(_XR_WS) >= 16:      # (streams come and go; a table is a few KB, but the cache is bounded as _CROP_WS is)
            _XR_WS.clear()
        ws = _XR_WS[key] = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    return ws


def _xr_views(out: torch.Tensor, ea, B: int, nch: int, offs) -> list:
    return [out[o:o + B * e.height * e.width * nch].view(B, e.height, e.width, nch) for e, o in zip(ea, offs)]


def dibr_xr_eyes(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, crop=None, out_u8: bool = True,
                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """The OpenXR viewer's eye views (reference xr_viewer/effects.py:1023-1137): the screen `screen` (xr.XrScreen) drawn into each
    eye image of `eyes` (1 or 2 xr.xr_eye) with that eye's own view-projection matrix -- the XR shader at the projected uv, the
    clear colour elsewhere.  frames uint8 [B,H,W,3] or [H,W,3]; depth [B,dh,dw] or [dh,dw] at any resolution; crop = u_source_crop or
    None; dp as dibr_warp(crop=) reads it except display_mode, viewport and roll (screen.roll is u_roll); feathering is refused.
    Returns one tensor per eye, [B,h,w,3|4] uint8 / float32 0..255 (views of one flat buffer: `out`, a caller-kept 1-D tensor of
    dibr_xr_shape's total, or a new one).  workspace: a caller-kept uint8 device tensor of d2s_dibr_xr_workspace bytes."""
    return _dibr_xr_call("eyes", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace)


def mip_shape(H: int, W: int) -> Tuple[list, int]:
    """([(offset, h, w)] of levels 1 .. q, total bytes) of one frame's colour mip chain (d2s_mip_shape): level k is uint8 [h, w, 3] at
    byte `offset` of the frame's row of mip_chain's result."""
    n, total = C.c_int(), C.c_uint64()
    offs, hs, ws = (C.c_uint64 * 14)(), (C.c_int * 14)(), (C.c_int * 14)()
    check(_lib.load().d2s_mip_shape(int(H), int(W), C.byref(n), offs, hs, ws, C.byref(total)), "d2s_mip_shape")
    return [(offs[i], hs[i], ws[i]) for i in range(n.value)], total.value


def mip_chain(frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mip chain glGenerateMipmap builds for the OpenXR viewer's colour texture (reference xr_viewer/effects.py:597-646), which
    its glow samples: frames uint8 [B,H,W,3] or [H,W,3] -> uint8 [B, total] (mip_shape), levels 1 .. q one after another.  out: a
    caller-kept tensor of that shape."""
    _need_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
        raise ValueError("mip_chain: frames must be uint8 [B,H,W,3] or [H,W,3]")
    f = frames.contiguous() if frames.dim() == 4 else frames.contiguous().unsqueeze(0)
    B, H, W, _ = f.shape
    _, total = mip_shape(H, W)
    if out is None:
        out = torch.empty((B, total), dtype=torch.uint8, device=f.device)
    elif not out.is_cuda or out.device != f.device or out.dtype != torch.uint8 or tuple(out.shape) != (B, total) or not out.is_contiguous():
        raise ValueError(f"mip_chain: out must be a contiguous uint8 tensor of {(B, total)} on {f.device}")
    with _on(f.device) as st:
        check(_lib.load().d2s_mip_chain(_ptr(f), B, H, W, _ptr(out), st), "d2s_mip_chain")
    return out


def _xr_struct(look):
    """d2s_xr_glow / d2s_xr_frost of an xr.XrGlow / xr.XrFrost (or the struct itself; None = off)."""
    return look if look is None or isinstance(look, (_lib.XrGlow, _lib.XrFrost)) else look.c_struct()


def _xr_tail(tail: str, who: str, B: int, H: int, W: int, device, glow=None, frost=None, levels=None, panorama=None, pano_rgb=None,
             pano_levels=None):
    """(the C arguments an entry of that tail (_XrEntry) has between workspace_bytes and the stream, what the caller keeps alive over
    the call).  glow = xr.XrGlow, frost = xr.XrFrost (or their structs; None = off); levels = mip_chain's result for these frames,
    which serves whichever look is given and is not looked at without one; panorama = a _lib.XrPanorama (xr.XrPanorama.c_struct; None =
    no panorama) with pano_rgb uint8 [h, w, 3] and pano_levels = mip_chain(pano_rgb).  The tensor checks of all of them, in that order."""
    fs, gs = _xr_struct(frost), _xr_struct(glow)
    lv = pr = pl = None
    if (fs is not None or gs is not None) and levels is not None:      # (the library refuses a missing chain with a look on)
        _need_cuda(levels, "levels")
        _, total = mip_shape(H, W)
        if levels.dtype != torch.uint8 or levels.device != device or tuple(levels.shape) != (B, total) or not levels.is_contiguous():
            raise ValueError(f"{who}: levels must be mip_chain's result for these frames, a contiguous uint8 tensor of {(B, total)} on {device}")
        lv = levels
    if panorama is not None and not isinstance(panorama, _lib.XrPanorama):
        raise ValueError(f"{who}: panorama must be xr.XrPanorama.c_struct(...)'s result (it carries the eyes' ray matrices) or None")
    if panorama is not None and pano_rgb is not None and pano_levels is not None:      # (the library refuses a missing image or chain)
        _need_cuda(pano_rgb, "pano_rgb")
        _need_cuda(pano_levels, "pano_levels")
        h, w = panorama.height, panorama.width
        if pano_rgb.dtype != torch.uint8 or tuple(pano_rgb.shape) != (h, w, 3) or pano_rgb.device != device or not pano_rgb.is_contiguous():
            raise ValueError(f"{who}: pano_rgb must be a contiguous uint8 tensor of {(h, w, 3)} on {device}")
        total = mip_shape(h, w)[1] if 2 <= h <= 8192 and 2 <= w <= 8192 else -1      # (the library refuses the size itself)
        if pano_levels.dtype != torch.uint8 or pano_levels.device != device or not pano_levels.is_contiguous() or \
                (total >= 0 and pano_levels.numel() != total):
            raise ValueError(f"{who}: pano_levels must be mip_chain(pano_rgb), a contiguous uint8 tensor of {total} bytes on {device}")
        pr, pl = pano_rgb, pano_levels

    def ref(s):
        return C.byref(s) if s is not None else None

    def ptr(t):
        return _ptr(t) if t is not None else None
    args = {"": (), "glow": (ref(gs), ptr(lv)), "frost": (ref(fs), ptr(lv)),
            "panorama": (ref(fs), ptr(lv), ref(gs), ref(panorama), ptr(pr), ptr(pl))}[tail]
    return args, (fs, gs, lv, panorama, pr, pl)


def _xr_plan_query(entry: str, dh: int, dw: int, batch: int, H: int, W: int, dp, screen, eyes, crop, out_u8: bool, looks, lead=()) -> dict:
    """The entry's plan door (host code, no GPU) and its answer as a dictionary.  looks: the structs the door takes after out_fmt
    (None = NULL); lead: what it takes in front."""
    sc, ea = _xr_args(screen, eyes)
    row = _XR_ENTRIES[entry]
    r = _lib.XrPlanResult()
    r.struct_size = C.sizeof(_lib.XrPlanResult)
    check(getattr(_lib.load(), row.plan)(*lead, int(dh), int(dw), int(batch), int(H), int(W), C.byref(dp),
                                         _crop4(crop) if crop is not None else None, C.byref(sc), ea, len(ea),
                                         FMT_U8_HWC if out_u8 else FMT_F32_HWC, *(C.byref(s) if s is not None else None for s in looks),
                                         C.byref(r)), row.plan)
    plan = {"kind": _lib.XR_KIND[r.kind], "rows_per_eye": r.rows_per_eye, "setup_launches": r.setup_launches, "grid": tuple(r.grid),
            "lds_dynamic_bytes": r.lds_dynamic_bytes, "lds_static_bytes": r.lds_static_bytes, "workspace_bytes": r.workspace_bytes,
            "out_elems": r.out_elems, "offsets": list(r.offsets[:len(ea)])}
    if row.tail == "panorama":
        plan["panorama"] = bool(r.reserved)
    return plan


def dibr_xr_eyes_glow(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, glow, levels, crop=None,
                      out_u8: bool = True, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes with the reference's glow around the flat screen in the same launch (d2s_dibr_xr_eyes_glow; reference
    _render_glow, xr_viewer/effects.py:476-585): glow = xr.XrGlow (None or mode "off": exactly dibr_xr_eyes), levels = mip_chain(frames)
    -- or an older chain: the reference refreshes its mipmaps every few frames only.  Everything else as dibr_xr_eyes."""
    return _dibr_xr_call("glow", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, glow=glow, levels=levels)


def dibr_xr_eyes_glow_curved(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, glow, levels, crop=None,
                             out_u8: bool = True, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes_glow that also draws the glow around a CURVED screen (d2s_dibr_xr_eyes_glow_curved; reference _render_curved_glow,
    xr_viewer/effects.py:408-474): screen.curve "horizontal" | "vertical" with glow mode "glow" | "glow2".  A flat screen or no glow is
    exactly dibr_xr_eyes_glow.  An eye outside the convex region the screen bounds (xr.XrScreen.eye_inside) is refused.  workspace: a
    caller-kept uint8 device tensor of d2s_dibr_xr_glow_curved_workspace bytes."""
    return _dibr_xr_call("glow_curved", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, glow=glow, levels=levels)


def dibr_xr_eyes_frost(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, frost, levels=None, crop=None,
                       out_u8: bool = True, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes with the reference's "veil" or "frosted" look around the flat screen in the same launch (d2s_dibr_xr_eyes_frost;
    reference _render_frost_veil / _render_frost_glow, xr_viewer/effects.py:789-857): frost = xr.XrFrost (None, mode "off", intensity
    <= 0 or a veil of alpha <= 0.002: exactly dibr_xr_eyes).  levels = mip_chain(frames) for "frosted"; the veil reads the frame alone.
    A curved screen with frost on is refused here: dibr_xr_eyes_frost_curved draws it.  workspace: a caller-kept uint8 device tensor of
    d2s_dibr_xr_frost_workspace bytes."""
    return _dibr_xr_call("frost", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, frost=frost, levels=levels)


def dibr_xr_eyes_frost_curved(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, frost, levels=None, crop=None,
                              out_u8: bool = True, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes_frost that also draws the veil or frosted look around a CURVED screen (d2s_dibr_xr_eyes_frost_curved; reference
    _render_curved_frost_with_uniforms, xr_viewer/effects.py:759-787): the 196 triangles of xr.XrFrost.curved_wall_verts blended after
    the curved strip in draw order; the eyes may be anywhere.  A flat screen is exactly dibr_xr_eyes_frost, a look that does not draw
    exactly dibr_xr_eyes.  workspace: a caller-kept uint8 device tensor of d2s_dibr_xr_frost_curved_workspace bytes."""
    return _dibr_xr_call("frost_curved", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, frost=frost, levels=levels)


def dibr_xr_frost_curved_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", screen, eyes, frost, crop=None,
                              out_u8: bool = True) -> dict:
    """dibr_xr_frost_plan for dibr_xr_eyes_frost_curved (d2s_dibr_xr_frost_curved_plan; host code, no GPU): kind "plain", "frost" or
    "frost_curved" (244 rows per eye, blocks of 64 x 64 pixels), and the same fields."""
    return _xr_plan_query("frost_curved", dh, dw, batch, H, W, dp, screen, eyes, crop, out_u8, (_xr_struct(frost),))


def dibr_xr_frost_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", screen, eyes, frost, crop=None,
                       out_u8: bool = True) -> dict:
    """dibr_xr_plan for dibr_xr_eyes_frost (d2s_dibr_xr_frost_plan; host code, no GPU): kind "plain" or "frost", and the same fields."""
    return _xr_plan_query("frost", dh, dw, batch, H, W, dp, screen, eyes, crop, out_u8, (_xr_struct(frost),))


def dibr_xr_eyes_panorama(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, panorama, pano_rgb, pano_levels,
                          glow=None, frost=None, levels=None, crop=None, out_u8: bool = True, out: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes with the reference's panorama background behind the screen (d2s_dibr_xr_eyes_panorama; reference
    _render_panorama_background, xr_viewer/effects.py:930-1021): every pixel no facet covers starts from the equirectangular panorama
    instead of screen.clear, sampled as the reference's texture() samples it (mipmapped, one LOD per 2 x 2 quad); the glow's outer
    band and the walls blend over it.  panorama = xr.XrPanorama(...).c_struct([(proj, view), ...], pano_rgb.shape[:2]); pano_rgb
    uint8 [h, w, 3], one image for the whole batch, row 0 up; pano_levels = mip_chain(pano_rgb).  glow = xr.XrGlow or frost =
    xr.XrFrost (at most one on) with levels = mip_chain(frames) as their own calls take it.  A curved screen with a look on and a
    panorama is refused here: dibr_xr_eyes_panorama_curved draws it.  panorama None: exactly the call of that look.  workspace: a caller-kept uint8 device tensor of
    d2s_dibr_xr_frost_curved_workspace bytes (the largest table serves every kind)."""
    return _dibr_xr_call("panorama", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, glow=glow, frost=frost, levels=levels,
                         panorama=panorama, pano_rgb=pano_rgb, pano_levels=pano_levels)


def dibr_xr_eyes_panorama_curved(frames: torch.Tensor, depth: torch.Tensor, dp: "_lib.DibrParams", screen, eyes, panorama, pano_rgb,
                                 pano_levels, glow=None, frost=None, levels=None, crop=None, out_u8: bool = True,
                                 out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """dibr_xr_eyes_panorama, which also draws the panorama behind the CURVED screen's glow, glow2, veil and frosted looks
    (d2s_dibr_xr_eyes_panorama_curved): the same arguments.  A flat screen, or a curved one without a look: exactly
    dibr_xr_eyes_panorama's launch; panorama None: exactly dibr_xr_eyes_glow_curved's / dibr_xr_eyes_frost_curved's.  An eye outside
    the convex region of the curved glow (xr.XrScreen.eye_inside) stays refused."""
    return _dibr_xr_call("panorama_curved", frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, glow=glow, frost=frost,
                         levels=levels, panorama=panorama, pano_rgb=pano_rgb, pano_levels=pano_levels)


def dibr_xr_panorama_curved_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", screen, eyes, panorama, glow=None,
                                 frost=None, crop=None, out_u8: bool = True) -> dict:
    """dibr_xr_panorama_plan for dibr_xr_eyes_panorama_curved (d2s_dibr_xr_panorama_curved_plan; host code, no GPU): kind "glow_curved"
    or "frost_curved" where those draw, with "panorama" true when the background is drawn behind them."""
    return _xr_plan_query("panorama_curved", dh, dw, batch, H, W, dp, screen, eyes, crop, out_u8,
                          (_xr_struct(frost), _xr_struct(glow), panorama))


def dibr_xr_panorama_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", screen, eyes, panorama, glow=None, frost=None,
                          crop=None, out_u8: bool = True) -> dict:
    """dibr_xr_plan for dibr_xr_eyes_panorama (d2s_dibr_xr_panorama_plan; host code, no GPU): the kind the looks ask for, the same
    fields, and "panorama": whether the background is drawn."""
    return _xr_plan_query("panorama", dh, dw, batch, H, W, dp, screen, eyes, crop, out_u8, (_xr_struct(frost), _xr_struct(glow), panorama))


def _dibr_xr_call(entry, frames, depth, dp, screen, eyes, crop, out_u8, out, workspace, **looks) -> list:
    """The tensor checks and the call of the eye-view entry `entry` (_XR_ENTRIES).  looks: what its tail takes of glow, frost, levels,
    panorama, pano_rgb, pano_levels (_xr_tail)."""
    row = _XR_ENTRIES[entry]
    who, symbol = row.direct, "d2s_" + row.direct
    _need_cuda(frames, "frames")
    _need_cuda(depth, "depth")
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
        raise ValueError(f"{who}: frames must be uint8 [B,H,W,3] or [H,W,3]")
    f = frames.contiguous() if frames.dim() == 4 else frames.contiguous().unsqueeze(0)
    d = depth.to(torch.float32).contiguous()
    d = d if d.dim() == 3 else d.unsqueeze(0)
    B, H, W, _ = f.shape
    if d.dim() != 3 or d.shape[0] != B:
        raise ValueError(f"{who}: depth must be [{B},dh,dw] for frames {tuple(f.shape)}, got {tuple(d.shape)}")
    _same_device(f, d, who)
    sc, ea = _xr_args(screen, eyes)
    if looks.get("levels") is not None and looks["levels"].dim() == 1:
        looks["levels"] = looks["levels"].unsqueeze(0)
    tail, _keep = _xr_tail(row.tail, who, B, H, W, f.device, **looks)      # (_keep: alive until the call has returned)
    offs, total = dibr_xr_shape(ea, B, dp.alpha_mode)
    nch = 4 if dp.alpha_mode == _lib.DIBR_ALPHA["rgba"] else 3
    dtype, fmt = (torch.uint8, FMT_U8_HWC) if out_u8 else (torch.float32, FMT_F32_HWC)
    if out is None:
        out = torch.empty(total, dtype=dtype, device=f.device)
    elif not out.is_cuda or out.device != f.device or out.dtype != dtype or out.numel() != total or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of {total} elements on {f.device}")
    ws = workspace if workspace is not None else _xr_workspace(len(ea), f.device, row.workspace)
    _need_cuda(ws, "workspace")
    _same_device(f, ws, f"{who} workspace")
    c4 = _crop4(crop) if crop is not None else None
    with _on(f.device) as st:
        check(getattr(_lib.load(), symbol)(_ptr(f), _ptr(d), d.shape[1], d.shape[2], B, H, W, C.byref(dp), c4, C.byref(sc), ea, len(ea),
                                           _ptr(out), fmt, _ptr(ws), ws.numel() * ws.element_size(), *tail, st), symbol)
    return _xr_views(out.view(-1), ea, B, nch, offs)


def dibr_xr_plan(entry: str, dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", screen, eyes, crop=None, glow=None,
                 out_u8: bool = True) -> dict:
    """What the eye-view call `entry` ("eyes" | "glow" | "glow_curved") decides for these arguments before it looks at a device pointer
    (include/d2s.h d2s_dibr_xr_plan; host code, no GPU): the kind of kernel, the table rows per eye and the launches that write them, the
    render launch's grid and LDS bytes, the workspace bytes and the out layout.  Raises D2SError with the entry's own refusal."""
    return _xr_plan_query(entry, dh, dw, batch, H, W, dp, screen, eyes, crop, out_u8, (_xr_struct(glow),), lead=(_lib.XR_ENTRY[entry],))


def _xr_panel_args(who: str, panels, textures, device, wrap: str):
    """(d2s_xr_panel array or None, d2s_xr_texture array or None, what the caller keeps alive) of xr.XrPanel objects (or their
    structs) and [h, w, 4] uint8 tensors, TOP ROW FIRST -- the library takes them that way and accounts for GL's bottom-first rows
    itself (include/d2s.h), so no copy is made here.  device None: the plan door, which looks at no tensor's device."""
    ps = [q if isinstance(q, _lib.XrPanel) else q.c_struct() for q in (panels or ())]
    ts, keep = [], []
    for t in (textures or ()):
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 4:
            raise ValueError(f"{who}: a panel texture must be a uint8 [h, w, 4] tensor, top row first")
        if device is not None:
            _need_cuda(t, "panel texture")
            if t.device != device:
                raise ValueError(f"{who}: a panel texture is on {t.device}, the eye images on {device}")
            t = t.contiguous()
        keep.append(t)
        ts.append(_lib.XrTexture(t.data_ptr() if device is not None else None, int(t.shape[1]), int(t.shape[0]), _lib.XR_WRAP[wrap],
                                 C.sizeof(_lib.XrTexture)))
    pa = (_lib.XrPanel * len(ps))(*ps) if ps else None
    ta = (_lib.XrTexture * len(ts))(*ts) if ts else None
    return pa, len(ps), ta, len(ts), keep


def dibr_xr_panels(images, screen, eyes, panels, textures=(), alpha_mode: Optional[int] = None, wrap: str = "repeat",
                   workspace: Optional[torch.Tensor] = None) -> list:
    """The world-space panels the reference draws after the screen and its look -- the FPS / status panel, the OSDs, the calibration
    and help panels, the keyboard with its border and key highlights, the laser quads (d2s_dibr_xr_panels; reference
    xr_viewer/overlay.py:81-249, 1427-1510, xr_viewer/effects.py:1157-1225) -- blended IN PLACE into `images`: what any
    ops.dibr_xr_eyes* or Engine.view_pipeline_xr* returned for this screen and these eyes (views of one flat buffer, in the eyes'
    order).  panels: xr.XrPanel, drawn in order, each depth-tested against the screen (whose depth the pass forms itself) and the
    earlier panels that wrote depth.  textures: uint8 [h, w, 4] tensors, top row first; wrap: the GL wrap of the bilinear taps at a
    panel's edge ("repeat": the reference's; "clamp").  alpha_mode: the images' (None: 4 channels = rgba, 3 = window); premultiplied
    images are refused.  Returns `images`.  The rainbow beams, hit circles and controller meshes are not drawn."""
    who = "dibr_xr_panels"
    row = _XR_ENTRIES["panels"]
    sc, ea = _xr_args(screen, eyes)
    imgs = list(images)
    if len(imgs) != len(ea) or not imgs:
        raise ValueError(f"{who}: images must be one tensor per eye")
    first = imgs[0]
    _need_cuda(first, "images")
    B, nch = first.shape[0], first.shape[-1]
    if first.dtype not in (torch.uint8, torch.float32) or nch not in (3, 4):
        raise ValueError(f"{who}: images must be uint8 or float32 [B,h,w,3|4]")
    if alpha_mode is None:
        alpha_mode = _lib.DIBR_ALPHA["rgba"] if nch == 4 else _lib.DIBR_ALPHA["window"]
    offs, total = dibr_xr_shape(ea, B, alpha_mode)
    base = first.data_ptr()
    for t, e, o in zip(imgs, ea, offs):
        if t.dtype != first.dtype or t.device != first.device or tuple(t.shape) != (B, e.height, e.width, nch) or not t.is_contiguous() or \
                t.data_ptr() != base + o * first.element_size():
            raise ValueError(f"{who}: images must be the tensors an eye-view call returned for these eyes (views of one flat buffer, "
                             f"eye i [B,{e.height},{e.width},{nch}] at dibr_xr_shape's offset)")
    pa, n_p, ta, n_t, _keep = _xr_panel_args(who, panels, textures, first.device, wrap)
    ws = workspace if workspace is not None else _xr_workspace(len(ea), first.device, row.workspace)
    _need_cuda(ws, "workspace")
    _same_device(first, ws, f"{who} workspace")
    fmt = FMT_U8_HWC if first.dtype == torch.uint8 else FMT_F32_HWC
    with _on(first.device) as st:
        check(_lib.load().d2s_dibr_xr_panels(C.c_void_p(base), fmt, B, int(alpha_mode), C.byref(sc), ea, len(ea), pa, n_p, ta, n_t,
                                             _ptr(ws), ws.numel() * ws.element_size(), st), "d2s_" + row.direct)
    return imgs


def dibr_xr_panels_plan(batch: int, screen, eyes, panels, textures=(), alpha_mode: int = 2, out_u8: bool = True, wrap: str = "repeat") -> dict:
    """What dibr_xr_panels decides for these arguments before it looks at a device pointer (d2s_dibr_xr_panels_plan; host code, no
    GPU): the table rows per eye (the screen's facets, then one per panel), the set-up launches that write them, the render launches
    (0 with no panel on any image: the call does nothing), per eye the panels drawn and the rectangle of 16 x 16 tiles their pixel
    boxes touch, the render grid, the workspace bytes and the images' layout.  textures: tensors (any device) or (h, w) pairs.
    Raises D2SError with the call's own refusal."""
    row = _XR_ENTRIES["panels"]
    sc, ea = _xr_args(screen, eyes)
    tex = [t if isinstance(t, torch.Tensor) else torch.empty((int(t[0]), int(t[1]), 4), dtype=torch.uint8, device="meta") for t in textures]
    pa, n_p, ta, n_t, _keep = _xr_panel_args("dibr_xr_panels_plan", panels, tex, None, wrap)
    r = _lib.XrPanelsPlanResult()
    r.struct_size = C.sizeof(_lib.XrPanelsPlanResult)
    check(getattr(_lib.load(), row.plan)(FMT_U8_HWC if out_u8 else FMT_F32_HWC, int(batch), int(alpha_mode), C.byref(sc), ea, len(ea), pa, n_p,
                                         ta, n_t, C.byref(r)), row.plan)
    n = len(ea)
    return {"rows_per_eye": r.rows_per_eye, "setup_launches": r.setup_launches, "render_launches": r.render_launches,
            "drawn": list(r.drawn[:n]), "tile0": [tuple(r.tile0[i]) for i in range(n)], "tiles": [tuple(r.tiles[i]) for i in range(n)],
            "grid": tuple(r.grid), "workspace_bytes": r.workspace_bytes, "out_elems": r.out_elems, "offsets": list(r.offsets[:n])}


def dibr_composite_plan(dh: int, dw: int, batch: int, H: int, W: int, dp: "_lib.DibrParams", mode: str, out_u8: bool = True,
                        out_align: int = 0) -> dict:
    """What dibr_composite would launch for these arguments (include/d2s.h d2s_dibr_composite_plan; host code, no GPU): the kernel's
    name, whether it is the LDS-window row kernel, the window plan (cols, margin, WW), the viewport's size, grid, block and the LDS
    request.  out_align = the output address modulo 16 ("Depth Map": vector or scalar stores)."""
    if mode not in _lib.COMPOSITE:
        raise ValueError(f"mode must be one of {list(_lib.COMPOSITE)}")
    r = _lib.DibrCompositePlanResult()
    r.struct_size = C.sizeof(_lib.DibrCompositePlanResult)
    check(_lib.load().d2s_dibr_composite_plan(int(dh), int(dw), int(batch), int(H), int(W), C.byref(dp), _lib.COMPOSITE[mode],
                                              FMT_U8_HWC if out_u8 else FMT_F32_HWC, int(out_align) & 15, C.byref(r)), "d2s_dibr_composite_plan")
    return {"kernel": r.kernel.decode(), "rows": bool(r.rows), "cols": r.cols, "margin": r.margin, "WW": r.ww, "roll0": bool(r.roll0),
            "up": bool(r.up), "fx": bool(r.fx), "vec": bool(r.vec), "out_h": r.out_h, "out_w": r.out_w, "grid": tuple(r.grid),
            "block": r.block, "lds_dynamic": r.lds_dynamic_bytes, "lds_static": r.lds_static_bytes,
            "lds_bytes": r.lds_dynamic_bytes + r.lds_static_bytes}


def dibr_composite(frames: Optional[torch.Tensor], depth: torch.Tensor, dp: "_lib.DibrParams", mode: str,
                   out_u8: bool = True, size: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The viewer's composite display modes (reference viewer.py:633-1197): "Anaglyph" | "Interleaved" | "Interleaved-V" |
    "Depth Map".  uint8 HWC frames [B,H,W,3] or [H,W,3] (None for "Depth Map") + depth [B,dh,dw] or [dh,dw] -> the program's viewport,
    dp.viewport = (x, y, w, h) in window pixels, y up (zeros: the frame itself); dp.display_mode is not used (include/d2s.h).
    Depth of another size than the frame's (the model's) is up-sampled inside the kernel, bit-identical to upsample_depth first.
    size = (H, W): the frame size when there are no frames ("Depth Map" from a model-resolution map); default: the depth's own.
    out: a caller-kept contiguous tensor of the result's batched shape [B, h, w, 3 | 4] and dtype (written in place)."""
    if mode not in _lib.COMPOSITE:
        raise ValueError(f"mode must be one of {list(_lib.COMPOSITE)}")
    _need_cuda(depth, "depth")
    d = depth.to(torch.float32).contiguous()
    batched = d.dim() == 3
    d = d if batched else d.unsqueeze(0)
    if d.dim() != 3:
        raise ValueError("dibr_composite: depth must be [B,H,W] or [H,W]")
    B, dh, dw = d.shape
    H, W = (int(size[0]), int(size[1])) if size is not None else (dh, dw)
    f = None
    if frames is not None:
        _need_cuda(frames, "frames")
        if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() != (4 if batched else 3):
            raise ValueError("dibr_composite: frames must be uint8 [B,H,W,3] or [H,W,3], batched like depth")
        f = frames.contiguous() if batched else frames.contiguous().unsqueeze(0)
        if f.shape[0] != B or (size is not None and tuple(f.shape[1:3]) != (H, W)):
            raise ValueError(f"dibr_composite: frames {tuple(f.shape)} do not match depth {tuple(d.shape)} / size {size}")
        H, W = f.shape[1:3]
        _same_device(f, d, "dibr_composite")
    elif mode != "Depth Map":
        raise ValueError(f"dibr_composite: {mode} needs the frames")
    lib = _lib.load()
    oh, ow = C.c_int(), C.c_int()
    check(lib.d2s_dibr_composite_shape(H, W, C.byref(dp), _lib.COMPOSITE[mode], C.byref(oh), C.byref(ow)), "d2s_dibr_composite_shape")
    shape, dtype, fmt = _dibr_out_spec(B, oh.value, ow.value, dp, out_u8)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=d.device)
    elif tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != d.device:
        raise ValueError(f"dibr_composite: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {d.device}")
    with _on(d.device) as st:
        check(lib.d2s_dibr_composite_depth(_ptr(f) if f is not None else None, _ptr(d), dh, dw, B, H, W, C.byref(dp), _lib.COMPOSITE[mode],
                                           _ptr(out), fmt, st), "d2s_dibr_composite_depth")
    return out if batched else out[0]


_JPEG_WS: Dict[Tuple[int, int], torch.Tensor] = {}


def jpeg_bound(H: int, W: int) -> Tuple[int, int]:
    """(output bytes that can never overflow, workspace bytes per frame) for an H x W frame."""
    ob, wb = C.c_int64(), C.c_int64()
    check(_lib.load().d2s_jpeg_bound(H, W, C.byref(ob), C.byref(wb)), "d2s_jpeg_bound")
    return ob.value, wb.value


def jpeg_encode(frames: torch.Tensor, quality: int = 90, out_stride: Optional[int] = None,
                workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """f3, the MJPEG sink (reference streamer.py:249-256, 285-291 — cv2.imencode('.jpg', ...)): RGB frames
    [B,H,W,3] or [H,W,3], uint8 or float32 0..255 (rounded half-even + saturated like cv2's convertTo), on the
    device -> (bytes [B, out_stride] uint8, sizes [B] int32), both on the device, no host sync.  The first
    sizes[b] bytes of row b are the JPEG libjpeg-turbo would write for that frame at that quality (4:2:0).
    workspace: uint8 device scratch of >= B * jpeg_bound(H, W)[1] + 256 bytes owned by the caller (one per stream that
    encodes concurrently); default: a module-level buffer, good for one stream at a time."""
    _need_cuda(frames, "frames")
    if frames.shape[-1] != 3 or frames.dim() not in (3, 4) or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError("jpeg_encode: frames must be uint8/float32 [B,H,W,3] or [H,W,3]")
    f = (frames if frames.dim() == 4 else frames.unsqueeze(0)).contiguous()
    B, H, W, _ = f.shape
    safe, ws_frame = jpeg_bound(H, W)
    # default stride: the unstuffed worst case + 1/16 for 0xFF stuffing; sizes[b] = -1 reports an overflow
    stride = int(out_stride) if out_stride else (safe // 2 + safe // 32 + 1024)
    if workspace is not None:
        if workspace.dtype != torch.uint8 or not workspace.is_cuda or workspace.numel() < ws_frame * B + 256:
            raise ValueError(f"jpeg_encode: workspace must be a uint8 device tensor of >= {ws_frame * B + 256} bytes")
        ws = workspace
    else:
        key = (f.device.index or 0, torch.cuda.current_stream(f.device).cuda_stream)
        ws = _JPEG_WS.get(key)                      # one growing scratch per (device, stream): never freed under a running encode
        if ws is None or ws.numel() < ws_frame * B + 256:
            ws = _JPEG_WS[key] = torch.empty(ws_frame * B + 256, dtype=torch.uint8, device=f.device)
    pad = (-ws.data_ptr()) % 256
    out = torch.empty((B, stride), dtype=torch.uint8, device=f.device)
    sizes = torch.empty((B,), dtype=torch.int32, device=f.device)
    _same_device(f, ws, "jpeg_encode workspace")
    with _on(f.device) as st:
        check(_lib.load().d2s_jpeg_encode(_ptr(f), FMT_U8_HWC if f.dtype == torch.uint8 else FMT_F32_HWC, B, H, W, int(quality),
                                          _ptr(out), stride, _ptr(sizes), C.c_void_p(ws.data_ptr() + pad), ws_frame * B, st),
              "d2s_jpeg_encode")
    return out, sizes


def model_desc(cfg: ModelConfig, precision: str = "bf16", temporal: bool = False, max_depth: float = 0.0) -> ModelDesc:
    """d2s_model_desc of a model configuration at an engine precision."""
    if precision not in ("bf16", "fp32", "fp8", "bf16x3", "fp8_mlp"):
        raise ValueError("precision must be 'bf16', 'fp32', 'fp8', 'fp8_mlp' or 'bf16x3'")
    prec = {"bf16": PREC_BF16, "fp32": PREC_FP32, "fp8": _lib.PREC_FP8, "bf16x3": _lib.PREC_BF16X3, "fp8_mlp": _lib.PREC_FP8_MLP}[precision]
    return ModelDesc(cfg.hidden, cfg.heads, cfg.layers, (C.c_int32 * 4)(*cfg.out_indices), (C.c_int32 * 4)(*cfg.neck),
                     cfg.fusion, cfg.head_hidden, cfg.mlp, cfg.patch, cfg.pos_grid, cfg.ln_eps, prec, int(bool(temporal)), float(max_depth))


def forward_plan(cfg: ModelConfig, h: int, w: int, batch: int = 1, precision: str = "bf16", *, temporal: bool = False, max_depth: float = 0.0,
                 calibrating: bool = False, calibrated: bool = True, profiling: bool = False, window_filled: bool = False) -> dict:
    """What a forward pass of `batch` frames decides before it launches anything (include/d2s.h d2s_forward_plan; host code, no GPU): the
    regime flags, per linear site {"folded", "stats", "e4m3"}, the taps' streams, the head's folds, the temporal modules' folded forms,
    the engine geometry and the number of LayerNorm launches -- for an engine created now (the D2S_* switches of the environment) and
    finalised at (h, w) with max_batch = batch.  calibrated: an e4m3 engine after Engine.calibrate (False: refused as the forward pass
    refuses it)."""
    desc = model_desc(cfg, precision, temporal, max_depth)
    F = _lib.PLAN_FLAGS
    flags = (F["calibrating"] * bool(calibrating) | F["profiling"] * bool(profiling) | F["window_filled"] * bool(window_filled) |
             F["calibrated"] * bool(calibrated))
    r = _lib.ForwardPlanResult()
    r.struct_size = C.sizeof(_lib.ForwardPlanResult)
    check(_lib.load().d2s_forward_plan(C.byref(desc), int(h), int(w), int(batch), int(flags), C.byref(r)), "d2s_forward_plan")
    out = {k: bool(getattr(r, k)) for k in ("f8", "f8a", "x3", "lnf", "pp_fold", "tap_fold", "use_side", "head1_ups", "head2_fused",
                                            "head2_ups", "tm_fold", "tm_cache_store")}
    out.update({k: int(getattr(r, k)) for k in ("bn", "gh", "gw", "P", "N", "Npad", "ln_launches", "splitk_elems", "scr_elems")})
    out.update({k: list(getattr(r, k)) for k in ("ln_slots", "fH", "fW", "tm_C", "tm_sites")})
    out["sites"] = {n: {"folded": bool(v & 1), "stats": bool(v & 2), "e4m3": bool(v & 4)} for n, v in zip(_lib.PLAN_SITES, r.site)}
    out["tap_side"] = [bool(v) for v in r.tap_side]
    out["tm_slots"] = [list(m) for m in r.tm_slots]
    out["tm_folded"] = [[bool(v) for v in m] for m in r.tm_folded]
    out["rcu_fused"] = [bool(r.rcu_fused >> i & 1) for i in range(4)]            # fusion stages, deep -> shallow
    out["rcu1_fused"] = [bool(r.rcu_fused >> (8 + i) & 1) for i in range(3)]     # the RCU1 of taps 0..2
    out["rcu_wide"] = [bool(r.rcu_fused >> (16 + i) & 1) for i in range(4)]      # ... as one launch of the wide (8 x 8-pixel tile) form
    out["rcu1_wide"] = [bool(r.rcu_fused >> (24 + i) & 1) for i in range(3)]
    return out


class Engine:
    """The native depth engine: what DepthModelWrapper holds in ``self.model`` for an accelerated
    backend (reference depth.py:1539-1781).  ``__call__(tensor[B,3,h,w]) -> tensor[B,h,w]``."""

    def __init__(self, cfg: ModelConfig, weights: Dict[str, np.ndarray], h: int, w: int, max_batch: int = 1,
                 precision: str = "bf16", device: int = 0, temporal: bool = False, max_depth: float = 0.0):
        """temporal=True: streaming Video-Depth-Anything (weights from vda_weights); max_batch = the number of independent stream
        slots (at most 32), each with its own 32-frame window -- see __call__ / pipeline(streams=...).
        max_depth > 0: metric head, sigmoid * max_depth (HF depth_estimation_type "metric")."""
        if not torch.cuda.is_available():
            raise _lib.D2SError("no ROCm device: the HIP engine cannot run (and there is no fallback)")
        self.lib = _lib.load()
        self.cfg, self.h, self.w, self.max_batch = cfg, h, w, max_batch
        self.precision = precision
        self.device = torch.device("cuda", device)
        desc = model_desc(cfg, precision, temporal, max_depth)
        self._h = C.c_void_p()
        with _on(self.device):
            check(self.lib.d2s_engine_create(C.byref(desc), device, C.byref(self._h)), "d2s_engine_create")
            for name, arr in weights.items():
                a = np.ascontiguousarray(arr, dtype=np.float32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                check(self.lib.d2s_engine_set_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                      f"d2s_engine_set_weight({name})")
            check(self.lib.d2s_engine_finalize(self._h, h, w, max_batch), "d2s_engine_finalize")

    def _mine(self, t: torch.Tensor, what: str):
        _need_cuda(t, what)
        if t.device != self.device:
            raise _lib.D2SError(f"{what} is on {t.device}, the engine lives on {self.device}")

    def memory_bytes(self) -> int:
        b = C.c_uint64()
        check(self.lib.d2s_engine_memory(self._h, C.byref(b)))
        return b.value

    @staticmethod
    def _stream_ids(streams, B: int):
        """streams=None -> NULL (rows 0..B-1 are streams 0..B-1); else a C int array of B stream slots (the library checks them)."""
        if streams is None:
            return None
        ids = [int(s) for s in streams]
        if len(ids) != B:
            raise ValueError(f"streams names {len(ids)} slots for a batch of {B} frames")
        return (C.c_int * B)(*ids)

    def __call__(self, x: torch.Tensor, streams=None) -> torch.Tensor:
        """temporal engines: batch row r is the next frame of stream slot streams[r] (distinct slots; None: rows are slots 0..B-1).
        Only the named streams advance."""
        self._mine(x, "pixel_values")
        x = x.to(torch.float32).contiguous()
        if x.dim() == 3:
            x = x.unsqueeze(0)
        B = x.shape[0]
        if tuple(x.shape[1:]) != (3, self.h, self.w):
            raise ValueError(f"engine was built for [B,3,{self.h},{self.w}], got {tuple(x.shape)}")
        out = torch.empty((B, self.h, self.w), dtype=torch.float32, device=x.device)
        with _on(self.device) as st:
            check(self.lib.d2s_model_forward_streams(self._h, _ptr(x), _ptr(out), B, self._stream_ids(streams, B), st), "d2s_model_forward")
        return out

    def calibrate(self, x: torch.Tensor):
        """fp8 engines: set the static activation scales from one bf16 pass over calibration inputs x [B,3,h,w]
        (normalised model inputs, e.g. ops.preprocess of representative frames).  Required before the first forward."""
        self._mine(x, "calibration inputs")
        x = x.to(torch.float32).contiguous()
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if tuple(x.shape[1:]) != (3, self.h, self.w):
            raise ValueError(f"engine was built for [B,3,{self.h},{self.w}], got {tuple(x.shape)}")
        with _on(self.device) as st:
            check(self.lib.d2s_engine_calibrate(self._h, _ptr(x), x.shape[0], st), "d2s_engine_calibrate")

    def tap(self, name: str) -> torch.Tensor:
        rows, cols = C.c_int(), C.c_int()
        n = max(self.cfg.hidden * (self.h // 14 * (self.w // 14) + 1), 16 * (self.h // 14) * (self.w // 14) * self.cfg.fusion)
        buf = torch.empty(n, dtype=torch.float32, device=self.device)
        with _on(self.device) as st:
            check(self.lib.d2s_engine_tap(self._h, name.encode(), _ptr(buf), n, C.byref(rows), C.byref(cols), st), "d2s_engine_tap")
        return buf[: rows.value * cols.value].view(rows.value, cols.value)

    def profile(self, enable: bool):
        """Start (and clear) / stop HIP-event timing around every kernel launch."""
        check(self.lib.d2s_engine_profile(self._h, int(enable)), "d2s_engine_profile")

    def profile_read(self) -> Dict[str, dict]:
        n = 16
        ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        nc = C.c_int()
        check(self.lib.d2s_engine_profile_read(self._h, n, ms, fl, by, cnt, C.byref(nc)), "d2s_engine_profile_read")
        return {self.lib.d2s_profile_class_name(i).decode(): {"ms": ms[i], "flops": fl[i], "bytes": by[i], "launches": cnt[i]}
                for i in range(nc.value)}

    def reset_stream(self, stream: Optional[int] = None):
        """Forget the stream state (temporal window, EMA): of every slot, or of the one slot `stream`."""
        if stream is None:
            check(self.lib.d2s_engine_reset_stream(self._h))
        else:
            check(self.lib.d2s_engine_reset_stream_at(self._h, int(stream)), "d2s_engine_reset_stream_at")

    def _run_pipeline(self, fn, name: str, frames: torch.Tensor, p: PipelineParams, spec, mid: tuple, want_depth: bool,
                      out: Optional[torch.Tensor], streams, who: Optional[str] = None):
        """The body the pipeline methods share: frames [B,H,W,3] uint8 -> fn(engine, frames, B, streams, H, W, depth_resolution, pre, post,
        *mid, out, out_fmt, depth_full, stream).  spec(B, H, W) -> (shape, dtype, D2S_FMT_*) of the result; a caller's `out` is checked
        against it when `who` names the method (pipeline itself takes any tensor of the engine's device)."""
        self._mine(frames, "frames")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [B,H,W,3]")
        frames = frames.contiguous()
        B, H, W, _ = frames.shape
        shape, dtype, fmt = spec(B, H, W)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=frames.device)
        else:
            self._mine(out, "out")
            if who and (out.numel() != torch.Size(shape).numel() or out.dtype != dtype or not out.is_contiguous()):
                raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of {shape}")
        depth = torch.empty((B, H, W), dtype=torch.float32, device=frames.device) if want_depth else None
        pp = post_params(p)
        pre = pre_params(p.mean, p.std, p.resample, p.square_input)
        with _on(self.device) as st:
            check(fn(self._h, _ptr(frames), B, self._stream_ids(streams, B), H, W, p.depth_resolution, C.byref(pre), C.byref(pp), *mid,
                     _ptr(out), fmt, _ptr(depth) if want_depth else None, st), name)
        return (out, depth) if want_depth else out

    def pipeline(self, frames: torch.Tensor, p: PipelineParams, sp: SbsParams, use_ema: bool = False,
                 out_fmt: int = FMT_U8_HWC, want_depth: bool = False, out: Optional[torch.Tensor] = None, streams=None):
        """predict_depth + make_sbs for uint8 HWC frames [B,H,W,3] in one stream-ordered call.
        temporal engines: `streams` as in __call__; use_ema keeps one EMA state per stream slot."""
        def spec(B, H, W):
            return _sbs_out_spec(B, *sbs_shape(H, W, sp), out_fmt) + (out_fmt,)
        return self._run_pipeline(self.lib.d2s_pipeline_streams, "d2s_pipeline", frames, p, spec, (C.byref(sp), int(use_ema)),
                                  want_depth, out, streams)

    def view_pipeline(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", view: Optional[str] = None,
                      use_ema: bool = False, out_u8: bool = True, want_depth: bool = False, out: Optional[torch.Tensor] = None,
                      streams=None):
        """predict_depth + the Viewer's shader warp for uint8 HWC frames [B,H,W,3] in one stream-ordered call: `pipeline` with
        dibr_warp (view=None: both eyes with disocclusion in-painting, packed per dp.display_mode) or dibr_composite (view =
        "Anaglyph" | "Interleaved" | "Interleaved-V" | "Depth Map", over dp.viewport) in place of make_sbs.  The warp reads the
        engine's model-resolution depth; bit-identical to pipeline(want_depth=True) followed by dibr_warp / dibr_composite on that
        map.  out: a caller-allocated result (e.g. a present-ring slot), [B,oh,ow,3|4] uint8 / float32.  streams, use_ema: as pipeline."""
        def spec(B, H, W):
            if view is not None and view not in _lib.COMPOSITE:
                raise ValueError(f"view must be None or one of {list(_lib.COMPOSITE)}")
            oh, ow = C.c_int(), C.c_int()
            if view is None:
                check(self.lib.d2s_dibr_shape(H, W, dp.display_mode, C.byref(oh), C.byref(ow)), "d2s_dibr_shape")
            else:
                check(self.lib.d2s_dibr_composite_shape(H, W, C.byref(dp), _lib.COMPOSITE[view], C.byref(oh), C.byref(ow)), "d2s_dibr_composite_shape")
            return _dibr_out_spec(B, oh.value, ow.value, dp, out_u8)
        mid = (C.byref(dp), -1 if view is None else _lib.COMPOSITE.get(view), int(use_ema))
        return self._run_pipeline(self.lib.d2s_view_pipeline_streams, "d2s_view_pipeline_streams", frames, p, spec, mid, want_depth, out,
                                  streams, who="view_pipeline")

    def view_pipeline_crop(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", crop, use_ema: bool = False,
                           out_u8: bool = True, want_depth: bool = False, out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline(view=None) with the OpenXR screen's source crop (d2s_view_pipeline_crop_streams): crop = (x, y, w, h) in uv,
        top-left origin, one rectangle for the batch; each eye is the crop's pixel size.  Bit-identical to pipeline(want_depth=True)'s
        engine depth followed by dibr_warp(crop=).  (A method of its own: view_pipeline's parameter list is pinned by the ABI tests.)"""
        def spec(B, H, W):
            return _dibr_out_spec(B, *dibr_crop_shape(H, W, crop, dp.display_mode), dp, out_u8)
        mid = (C.byref(dp), -1, _crop4(crop), int(use_ema))
        return self._run_pipeline(self.lib.d2s_view_pipeline_crop_streams, "d2s_view_pipeline_crop_streams", frames, p, spec, mid,
                                  want_depth, out, streams, who="view_pipeline_crop")

    def view_pipeline_xr(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, crop=None,
                         use_ema: bool = False, out_u8: bool = True, want_depth: bool = False, out: Optional[torch.Tensor] = None,
                         streams=None):
        """view_pipeline with the OpenXR eye views as its last stage (d2s_view_pipeline_xr_streams): screen, eyes, crop as
        ops.dibr_xr_eyes.  Returns one tensor per eye (with want_depth: (list, depth)); bit-identical to pipeline(want_depth=True)'s
        engine depth followed by dibr_xr_eyes.  out: a caller-kept 1-D tensor of dibr_xr_shape's total.  (A method of its own, as
        view_pipeline_crop is: view_pipeline's parameter list is pinned by the ABI tests.)"""
        return self._view_pipeline_xr("eyes", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams)

    def _view_pipeline_xr(self, entry, frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, **looks):
        """The view pipeline of the eye-view entry `entry` (_XR_ENTRIES); looks as _dibr_xr_call takes them."""
        sc, ea = _xr_args(screen, eyes)
        nch = 4 if dp.alpha_mode == _lib.DIBR_ALPHA["rgba"] else 3
        row = _XR_ENTRIES[entry]
        name, who = "d2s_" + row.pipeline + "_streams", row.pipeline
        lay = {}

        def spec(B, H, W):
            lay["offs"], lay["total"] = dibr_xr_shape(ea, B, dp.alpha_mode)
            lay["B"] = B
            lay["tail"], lay["keep"] = _xr_tail(row.tail, who, B, H, W, self.device, **looks)
            return (lay["total"],), torch.uint8 if out_u8 else torch.float32, FMT_U8_HWC if out_u8 else FMT_F32_HWC
        ws = _xr_workspace(len(ea), self.device, row.workspace)
        nbytes = ws.numel()

        def fn(*a):      # (_run_pipeline ends every call with out, out_fmt, depth_full, stream: the workspace goes in front of the stream)
            return getattr(self.lib, name)(*a[:-1], _ptr(ws), nbytes, *lay["tail"], a[-1])
        mid = (C.byref(dp), _crop4(crop) if crop is not None else None, C.byref(sc), ea, len(ea), int(use_ema))
        r = self._run_pipeline(fn, name, frames, p, spec, mid, want_depth, out, streams, who=who)
        flat = (r[0] if want_depth else r).view(-1)
        views = _xr_views(flat, ea, lay["B"], nch, lay["offs"])
        return (views, r[1]) if want_depth else views

    def view_pipeline_xr_panorama(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, panorama, pano_rgb,
                                  pano_levels, glow=None, frost=None, levels=None, crop=None, use_ema: bool = False, out_u8: bool = True,
                                  want_depth: bool = False, out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline_xr with the panorama background behind the screen (d2s_view_pipeline_xr_panorama_streams): panorama,
        pano_rgb, pano_levels, glow, frost and levels as dibr_xr_eyes_panorama takes them.  Bit-identical to
        pipeline(want_depth=True)'s engine depth followed by dibr_xr_eyes_panorama."""
        return self._view_pipeline_xr("panorama", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, glow=glow,
                                      frost=frost, levels=levels, panorama=panorama, pano_rgb=pano_rgb, pano_levels=pano_levels)

    def view_pipeline_xr_panorama_curved(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, panorama,
                                         pano_rgb, pano_levels, glow=None, frost=None, levels=None, crop=None, use_ema: bool = False,
                                         out_u8: bool = True, want_depth: bool = False, out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline_xr_panorama with the panorama also behind the curved screen's looks
        (d2s_view_pipeline_xr_panorama_curved_streams).  Bit-identical to pipeline(want_depth=True)'s engine depth followed by
        dibr_xr_eyes_panorama_curved."""
        return self._view_pipeline_xr("panorama_curved", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams,
                                      glow=glow, frost=frost, levels=levels, panorama=panorama, pano_rgb=pano_rgb, pano_levels=pano_levels)

    def view_pipeline_xr_glow(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, glow, levels, crop=None,
                              use_ema: bool = False, out_u8: bool = True, want_depth: bool = False, out: Optional[torch.Tensor] = None,
                              streams=None):
        """view_pipeline_xr with the glow around the flat screen (d2s_view_pipeline_xr_glow_streams): glow = xr.XrGlow, levels =
        mip_chain(frames) (the caller's: it decides how often the chain is refreshed).  Bit-identical to pipeline(want_depth=True)'s
        engine depth followed by dibr_xr_eyes_glow."""
        if glow is None:
            raise ValueError("view_pipeline_xr_glow: glow must be an xr.XrGlow (mode \"off\" for none)")
        return self._view_pipeline_xr("glow", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, glow=glow, levels=levels)

    def view_pipeline_xr_glow_curved(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, glow, levels,
                                     crop=None, use_ema: bool = False, out_u8: bool = True, want_depth: bool = False,
                                     out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline_xr_glow whose last stage also draws the glow around a curved screen
        (d2s_view_pipeline_xr_glow_curved_streams).  Bit-identical to pipeline(want_depth=True)'s engine depth followed by
        dibr_xr_eyes_glow_curved."""
        if glow is None:
            raise ValueError("view_pipeline_xr_glow_curved: glow must be an xr.XrGlow (mode \"off\" for none)")
        return self._view_pipeline_xr("glow_curved", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, glow=glow,
                                      levels=levels)

    def view_pipeline_xr_frost(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, frost, levels=None,
                               crop=None, use_ema: bool = False, out_u8: bool = True, want_depth: bool = False,
                               out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline_xr with the veil or frosted look around the flat screen (d2s_view_pipeline_xr_frost_streams): frost =
        xr.XrFrost, levels = mip_chain(frames) for "frosted" (the caller's, as view_pipeline_xr_glow's).  Bit-identical to
        pipeline(want_depth=True)'s engine depth followed by dibr_xr_eyes_frost."""
        if frost is None:
            raise ValueError("view_pipeline_xr_frost: frost must be an xr.XrFrost (mode \"off\" for none)")
        return self._view_pipeline_xr("frost", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, frost=frost, levels=levels)

    def view_pipeline_xr_frost_curved(self, frames: torch.Tensor, p: PipelineParams, dp: "_lib.DibrParams", screen, eyes, frost, levels=None,
                                      crop=None, use_ema: bool = False, out_u8: bool = True, want_depth: bool = False,
                                      out: Optional[torch.Tensor] = None, streams=None):
        """view_pipeline_xr_frost that also draws the look around a curved screen (d2s_view_pipeline_xr_frost_curved_streams).
        Bit-identical to pipeline(want_depth=True)'s engine depth followed by dibr_xr_eyes_frost_curved."""
        if frost is None:
            raise ValueError("view_pipeline_xr_frost_curved: frost must be an xr.XrFrost (mode \"off\" for none)")
        return self._view_pipeline_xr("frost_curved", frames, p, dp, screen, eyes, crop, use_ema, out_u8, want_depth, out, streams, frost=frost,
                                      levels=levels)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.d2s_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reload_env() -> int:
    """Make libd2s_hip.so re-read the switches it reads while launching (D2S_NO_HALO2, D2S_NO_WIDE, ...) from the environment.
    Switches read when an engine is created or finalised (D2S_NO_LNFUSE, D2S_TAPS, D2S_NO_OVERLAP, D2S_VDA_FUSE) are not re-read
    for an engine that exists."""
    return int(_lib.load().d2s_debug_reload_env())


def gemm_probe(A: torch.Tensor, Wt: torch.Tensor, bias: Optional[torch.Tensor], precision: str, tile: int = 0, iters: int = 1):
    """C = A @ Wt^T (+bias) through the engine's MFMA kernel (test / micro-benchmark)."""
    M, K = A.shape
    N = Wt.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    check(_lib.load().d2s_gemm_probe(_ptr(A.contiguous()), _ptr(Wt.contiguous()), _ptr(bias) if bias is not None else None,
                                     _ptr(out), M, N, K, {"bf16": PREC_BF16, "fp32": PREC_FP32, "fp8": _lib.PREC_FP8, "bf16x3": _lib.PREC_BF16X3}[precision], tile, iters,
                                     C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)),
          "d2s_gemm_probe")
    return out


def conv3_probe(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, precision: str = "bf16", *,
                up: Optional[tuple] = None, stride: int = 1, relu_in: bool = False, act: str = "none",
                res: Optional[torch.Tensor] = None, out_f32: bool = False, head: Optional[tuple] = None, tile: int = 0,
                splitk_elems: int = 0):
    """One 3x3 convolution (pad 1) of the DPT neck / head through the engine's own dispatcher (test probe, include/d2s.h).
    x: float32 [B, Hs, Ws, C], w: float32 [N, C, 3, 3] (PyTorch layout), bias [N].  up = (Hi, Wi): an align_corners bilinear
    up-sample of x to that size in front of the convolution, folded into its loader; stride 1 | 2; relu_in: ReLU on load;
    act "none" | "relu" after the bias; res [B, Ho, Wo, N] added last; head = (w3 [N], b3, max_depth): the fused DPT head tail
    (out = float depth [B, Ho, Wo]); splitk_elems > 0: a split-K workspace of that many partials, as the engine's.
    Returns (out, kernel name): out [B, Ho, Wo, N] in the operand type (bfloat16 for "bf16") or float32 (out_f32 / head)."""
    _need_cuda(x, "x")
    B, Hs, Ws, Cin = x.shape
    N = w.shape[0]
    if tuple(w.shape) != (N, Cin, 3, 3):
        raise ValueError("conv3_probe: w must be [N, C, 3, 3]")
    Hi, Wi = up if up is not None else (Hs, Ws)
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    prec = {"bf16": PREC_BF16, "fp32": PREC_FP32, "bf16x3": _lib.PREC_BF16X3}[precision]
    keep = [x.float().contiguous(), w.float().contiguous()]
    p = _lib.Conv3ProbeParams()
    p.struct_size = C.sizeof(_lib.Conv3ProbeParams)
    p.precision, p.tile, p.batch, p.C, p.N = prec, int(tile), B, Cin, N
    p.Hs, p.Ws, p.Hi, p.Wi, p.stride = Hs, Ws, Hi, Wi, int(stride)
    p.relu_in, p.act, p.out_f32 = int(bool(relu_in)), {"none": 0, "relu": 1}[act], int(bool(out_f32))
    p.splitk_elems = int(splitk_elems)
    p.x, p.w = _ptr(keep[0]), _ptr(keep[1])
    if bias is not None:
        keep.append(bias.float().contiguous()); p.bias = _ptr(keep[-1])
    if res is not None:
        keep.append(res.float().contiguous()); p.res = _ptr(keep[-1])
    if head is not None:
        w3, b3, max_depth = head
        keep.append(w3.float().contiguous()); p.w3 = _ptr(keep[-1])
        p.map_head, p.b3, p.max_depth = 1, float(b3), float(max_depth)
        out = torch.empty((B, Ho, Wo), dtype=torch.float32, device=x.device)
    else:
        dt = torch.bfloat16 if precision == "bf16" and not out_f32 else torch.float32
        out = torch.empty((B, Ho, Wo, N), dtype=dt, device=x.device)
    p.out = _ptr(out)
    with _on(x.device) as st:
        check(_lib.load().d2s_conv3_probe(C.byref(p), st), "d2s_conv3_probe")
    return out, p.kernel.decode()


def rcu_probe(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
              wp: Optional[torch.Tensor] = None, bp: Optional[torch.Tensor] = None, *, wide: bool = False):
    """A fusion stage's residual unit as the one launch the engine makes of it on a small map (test probe, include/d2s.h d2s_rcu_probe):
    x + conv2(relu(conv1(relu(x)))), through the 1x1 projection (wp [C, C], bp) where given.  x: float32 [B, H, W, C], w1 / w2: float32
    [C, C, 3, 3], biases [C].  wide: the kernel's 8 x 8-pixel tile form (refused where those tiles x B exceed the CUs) instead of the 4 x 8
    one.  Returns (out bfloat16 [B, H, W, C], kernel name); D2SError where the engine would keep the separate launches."""
    _need_cuda(x, "x")
    B, H, W, Cc = x.shape
    if tuple(w1.shape) != (Cc, Cc, 3, 3) or tuple(w2.shape) != (Cc, Cc, 3, 3) or (wp is not None and tuple(wp.shape) != (Cc, Cc)):
        raise ValueError("rcu_probe: w1, w2 must be [C, C, 3, 3], wp [C, C]")
    if (wp is None) != (bp is None):
        raise ValueError("rcu_probe: wp and bp go together")
    keep = [t.float().contiguous() for t in (x, w1, b1, w2, b2)] + ([wp.float().contiguous(), bp.float().contiguous()] if wp is not None else [])
    p = _lib.RcuProbeParams()
    p.struct_size = C.sizeof(_lib.RcuProbeParams)
    p.batch, p.H, p.W, p.C = B, H, W, Cc
    p.reserved = 1 if wide else 0
    p.x, p.w1, p.b1, p.w2, p.b2 = (_ptr(t) for t in keep[:5])
    if wp is not None:
        p.wp, p.bp = _ptr(keep[5]), _ptr(keep[6])
    out = torch.empty((B, H, W, Cc), dtype=torch.bfloat16, device=x.device)
    p.out = _ptr(out)
    with _on(x.device) as st:
        check(_lib.load().d2s_rcu_probe(C.byref(p), st), "d2s_rcu_probe")
    return out, p.kernel.decode()


def linear_probe(site: str, precision: str, a: Optional[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
                 scale: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                 res2: Optional[torch.Tensor] = None, ln: Optional[tuple] = None, producer: Optional[tuple] = None, fold: bool = False,
                 ntok: int = 0, heads: int = 0, npad: int = 0, grid: Optional[tuple] = None, scales: tuple = (0.0, 0.0, 0.0, 0.0),
                 ln_eps: float = 1e-6, tile: int = 0, splitk_elems: int = 0) -> dict:
    """One linear of the engine (include/d2s.h d2s_linear_probe, sites D2S_LIN_*) through its own dispatcher, epilogue and packing (test
    probe).  Float32 device operands: a [rows, K], w [N, K] (neck_resize: ConvTranspose2d [K, K, ks, ks]), bias, LayerScale scale,
    x: the fp32 residual stream the site updates (cloned; the result comes back), res / res2 (patch: pos), grid = (gh, gw, ks);
    fold: LayerNorm folding -- consumers take ln = (gamma, beta) and producer = (pa, pw, pbias, pscale), x = the residual before it;
    scales = (s_act, s_out, s_res, s_pact) of the e4m3 engines.  precision: "fp32" | "bf16" | "bf16x3" | "fp8" | "fp8_mlp" (the engine's).
    Returns a dict: out / vt / out2 as raw storage (bfloat16, float32, uint8 e4m3 bytes, int32 bf16x3 unit words), with one guard row
    before and after out (out_guard: the whole buffer, filled with 0x7f bytes before the launch), x, stats [D / 16 + 1, M, 2], slots,
    kernel, kernel2."""
    _need_cuda(w, "w")
    dev = w.device
    prec = {"fp32": PREC_FP32, "bf16": PREC_BF16, "bf16x3": _lib.PREC_BF16X3, "fp8": _lib.PREC_FP8, "fp8_mlp": _lib.PREC_FP8_MLP}[precision]
    sid = _lib.LINEAR_SITES[site]
    N = w.shape[0] if site != "neck_resize" else w.shape[1] * w.shape[2] * w.shape[3]
    K = w.shape[1] if site != "neck_resize" else w.shape[0]
    consumer = fold and site in ("qkv", "fc1", "neck_proj", "tm_kvq", "tm_ff1")
    M = producer[0].shape[0] if consumer else (x.shape[0] if site in ("proj", "fc2", "tm_proj_in", "tm_to_out", "tm_ff2") else a.shape[0])
    if site == "neck_proj":
        M = (producer[0].shape[0] if consumer else a.shape[0] // (ntok - 1) * ntok)
    x3, f8, f8a = precision == "bf16x3", precision in ("fp8", "fp8_mlp"), precision == "fp8"
    e8 = f8 and (site in ("fc1", "fc2") or (f8a and site in ("qkv", "proj")))
    act16 = precision in ("bf16", "fp8", "fp8_mlp")
    t_out = torch.bfloat16 if act16 else torch.float32        # OUT_T

    def alloc(rows, cols, dtype):
        buf = torch.empty((rows + 2, cols), dtype=dtype, device=dev)
        buf.view(torch.uint8).fill_(0x7f)
        return buf
    keep = []

    def fp(t):
        if t is None:
            return None
        keep.append(t.float().contiguous())
        return _ptr(keep[-1])
    p = _lib.LinearProbeParams()
    p.struct_size = C.sizeof(_lib.LinearProbeParams)
    p.site, p.precision, p.ln_fold, p.M, p.N, p.K = sid, prec, int(bool(fold)), M, N, K
    p.ntok, p.heads, p.npad = int(ntok), int(heads), int(npad)
    if grid is not None:
        p.gh, p.gw, p.ks = grid
    p.ln_eps, p.tile, p.splitk_elems = float(ln_eps), int(tile), int(splitk_elems)
    p.s_act, p.s_out, p.s_res, p.s_pact = (float(v) for v in scales)
    p.a, p.w, p.bias, p.scale, p.res, p.res2 = fp(a), fp(w), fp(bias), fp(scale), fp(res), fp(res2)
    if ln is not None:
        p.ln_g, p.ln_b = fp(ln[0]), fp(ln[1])
    if producer is not None:
        p.pK = producer[0].shape[1]
        p.pa, p.pw, p.pbias, p.pscale = fp(producer[0]), fp(producer[1]), fp(producer[2]), fp(producer[3])
    r = {"out": None, "out_guard": None, "vt": None, "out2": None, "x": None, "stats": None}
    if x is not None:
        r["x"] = x.float().clone().contiguous()
        p.x = _ptr(r["x"])
    # the output in the site's type (linear_site.h qkv_out_type / fc1_out_type, OUT_T)
    if site == "qkv":
        odt = torch.bfloat16 if f8 else (torch.int32 if x3 else t_out)
        rows, cols = M, N
    elif site == "fc1":
        odt = torch.int32 if x3 else (torch.uint8 if e8 else t_out)
        rows, cols = M, N
    elif site == "neck_proj":
        odt, rows, cols = t_out, M // ntok * (ntok - 1), N
    elif site == "neck_resize":
        odt, rows, cols = t_out, M * grid[2] * grid[2], K
    elif site == "tm_ff1":
        odt, rows, cols = t_out, M, N // 2 if fold else N
    elif site in ("tm_kvq", "tm_proj_out"):
        odt, rows, cols = t_out, M, N
    else:
        odt = None
    if odt is not None:
        g = alloc(rows, cols, odt)
        r["out_guard"], r["out"] = g, g[1:rows + 1]
        p.out = _ptr(r["out"])
    if site == "qkv":
        B = M // ntok
        r["vt"] = torch.empty((B, heads, 64, npad), dtype=odt, device=dev)
        r["vt"].view(torch.uint8).fill_(0x7f)
        p.vt = _ptr(r["vt"])
    if fold:
        D = K if consumer else N
        r["out2"] = torch.empty((M, D), dtype=torch.int32 if x3 else (torch.uint8 if (e8 if consumer else f8) else torch.bfloat16), device=dev)
        r["out2"].view(torch.uint8).fill_(0x7f)
        p.out2 = _ptr(r["out2"])
        if site != "tm_ff2":
            r["stats"] = torch.full((D // 16 + 1, M, 2), float("nan"), dtype=torch.float32, device=dev)
            p.stats = _ptr(r["stats"])
    with _on(dev) as st:
        check(_lib.load().d2s_linear_probe(C.byref(p), st), "d2s_linear_probe")
    r["slots"], r["kernel"], r["kernel2"] = p.stats_slots, p.kernel.decode(), p.kernel2.decode()
    return r


def attention_probe(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, precision: str = "bf16", iters: int = 1):
    """softmax(q k^T / 8) v for float32 [B, heads, N, 64] device tensors through the engine's attention kernel
    (test / micro-benchmark).  Returns (out [B, N, heads * 64] float32, ms per launch or 0)."""
    B, H, N, d = q.shape
    if d != 64 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("attention_probe: q, k, v must be [B, heads, N, 64]")
    out = torch.empty((B, N, H * 64), dtype=torch.float32, device=q.device)
    ms = C.c_float(0.0)
    with _on(q.device) as st:
        check(_lib.load().d2s_attention_probe(_ptr(q.float().contiguous()), _ptr(k.float().contiguous()), _ptr(v.float().contiguous()),
                                              _ptr(out), B, H, N, {"bf16": PREC_BF16, "fp32": PREC_FP32, "bf16x3": _lib.PREC_BF16X3}[precision], iters,
                                              C.byref(ms), st), "d2s_attention_probe")
    return out, ms.value


def attention_probe_ex(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, precision: str = "bf16", *, out_e4m3: bool = False,
                       oscale: float = 0.0) -> dict:
    """One attention launch of the engine through its own dispatcher (test probe, include/d2s.h d2s_attention_probe_ex): float32
    [B, heads, N, 64] device tensors, packed as the engine's QKV linear leaves them.  out_e4m3 (bf16 only): the fp8 engines' e4m3
    output sat(result * oscale).  Returns a dict: out [B * N, heads * 64] as raw storage (bfloat16, float32, int32 bf16x3 unit
    words, uint8 e4m3 bytes), a view of guard [B * N + 2, heads * 64] -- one guard row before and one after, the whole buffer filled
    with 0x7f bytes before the launch -- and kernel, the name of the kernel that ran."""
    _need_cuda(q, "q")
    B, H, N, d = q.shape
    if d != 64 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("attention_probe_ex: q, k, v must be [B, heads, N, 64]")
    if out_e4m3 and precision != "bf16":
        raise ValueError("attention_probe_ex: out_e4m3 needs bf16 operands")
    dt = torch.uint8 if out_e4m3 else {"bf16": torch.bfloat16, "fp32": torch.float32, "bf16x3": torch.int32}[precision]
    guard = torch.empty((B * N + 2, H * 64), dtype=dt, device=q.device)
    keep = [t.float().contiguous() for t in (q, k, v)]
    p = _lib.AttentionProbeParams()
    p.struct_size = C.sizeof(_lib.AttentionProbeParams)
    p.precision = {"bf16": PREC_BF16, "fp32": PREC_FP32, "bf16x3": _lib.PREC_BF16X3}[precision]
    p.B, p.heads, p.N, p.out_e4m3, p.oscale = B, H, N, int(bool(out_e4m3)), float(oscale)
    p.q, p.k, p.v, p.out = _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(guard)
    with _on(q.device) as st:
        check(_lib.load().d2s_attention_probe_ex(C.byref(p), st), "d2s_attention_probe_ex")
    return {"out": guard[1:B * N + 1], "guard": guard, "kernel": p.kernel.decode()}


def temporal_probe(op: str, precision: str, x: torch.Tensor, out: Optional[torch.Tensor] = None, *, rows: int = 0, sites: int = 0,
                   channels: int = 0, groups: int = 32, slots: int = 31, eps: float = 1e-6, gamma: Optional[torch.Tensor] = None,
                   beta: Optional[torch.Tensor] = None, ptab: Optional[torch.Tensor] = None, rings=(), head=(), Tw=(), store_slot=(),
                   slot0=(), nslots=(), n: int = 0, qscale: float = 0.0, bx3_out: bool = False, row_map=(0, 0, 0)) -> str:
    """One launch of a temporal-module or LayerNorm launcher of the engine (test probe, include/d2s.h d2s_temporal_probe).  op:
    "groupnorm" | "temporal_attn" | "cache_store" | "geglu" | "cast_f32" | "layernorm"; precision "bf16" | "fp32" (the engine class).
    The tensors are device buffers ALREADY in the kernel's storage type (torch.bfloat16 = raw bf16 bits) and are used in place -- views
    into larger guarded buffers are fine; the element counts the library checks against are what each tensor holds from its first
    element (numel of a contiguous tensor).  channels: C of the header (GEGLU: the output width, LayerNorm: D).  rings: one tensor per row; row_map = (rows_per_img, img_rows, row_off) of LayerNorm.
    Returns the name of the kernel that ran ("" when cache_store had nothing to store); raises D2SError where the library refuses."""
    _need_cuda(x, "x")
    p = _lib.TemporalProbeParams()
    p.struct_size = C.sizeof(_lib.TemporalProbeParams)
    p.op = _lib.TEMPORAL_OPS[op]
    p.precision = {"bf16": PREC_BF16, "fp32": PREC_FP32}[precision]
    p.rows, p.sites, p.C, p.groups, p.slots = int(rows), int(sites), int(channels), int(groups), int(slots)
    p.eps, p.qscale, p.bx3_out, p.n = float(eps), float(qscale), int(bool(bx3_out)), int(n)
    p.rows_per_img, p.img_rows, p.row_off = (int(v) for v in row_map)

    def buf(t):
        if t is None:
            return None, 0
        if not t.is_contiguous():
            raise ValueError("temporal_probe: tensors must be contiguous")
        return _ptr(t), t.numel()
    (p.x, p.x_elems), (p.out, p.out_elems) = buf(x), buf(out)
    (p.gamma, p.gamma_elems), (p.beta, p.beta_elems), (p.ptab, p.ptab_elems) = buf(gamma), buf(beta), buf(ptab)
    for r, t in enumerate(rings):
        _need_cuda(t, "ring")
        if not t.is_contiguous():
            raise ValueError("temporal_probe: tensors must be contiguous")
        p.ring[r], p.ring_elems[r] = t.data_ptr(), t.numel()
    for name, vals in (("head", head), ("Tw", Tw), ("store_slot", store_slot), ("slot0", slot0), ("nslots", nslots)):
        arr = getattr(p, name)
        for r, v in enumerate(vals):
            arr[r] = int(v)
    with _on(x.device) as st:
        check(_lib.load().d2s_temporal_probe(C.byref(p), st), "d2s_temporal_probe")
    return p.kernel.decode()


def preprocess_to(frames: torch.Tensor, out: torch.Tensor, decim_stride: int = 1, pre: Optional[PreParams] = None) -> torch.Tensor:
    """d2s_preprocess with the C-ABI's own arguments: `out` float32 [B,3,h,w] caller-allocated (a view into a larger buffer is fine), explicit
    decimation stride and d2s_pre_params (None: ImageNet mean / std, bilinear)."""
    _need_cuda(frames, "frames")
    _same_device(frames, out, "preprocess_to")
    fmt, B, H, W = _frame_fmt(frames)
    if not (frames.is_contiguous() and out.is_contiguous()) or out.dtype != torch.float32 or out.dim() != 4 or out.shape[:2] != (B, 3):
        raise ValueError("preprocess_to: frames / out must be contiguous, out float32 [B,3,h,w]")
    with _on(frames.device) as st:
        check(_lib.load().d2s_preprocess(_ptr(frames), fmt, B, H, W, _ptr(out), out.shape[2], out.shape[3], int(decim_stride),
                                         C.byref(pre) if pre is not None else None, st), "d2s_preprocess")
    return out


def upsample_depth_to(depth: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """d2s_upsample_depth into a caller-allocated float32 [B,H,W] (a view into a larger buffer is fine)."""
    _need_cuda(depth, "depth")
    _same_device(depth, out, "upsample_depth_to")
    if not (depth.is_contiguous() and out.is_contiguous()) or depth.dtype != torch.float32 or out.dtype != torch.float32 or depth.dim() != 3 \
            or out.dim() != 3 or out.shape[0] != depth.shape[0]:
        raise ValueError("upsample_depth_to: depth / out must be contiguous float32 [B,h,w] / [B,H,W]")
    with _on(depth.device) as st:
        check(_lib.load().d2s_upsample_depth(_ptr(depth), depth.shape[0], depth.shape[1], depth.shape[2], _ptr(out), out.shape[1], out.shape[2], st),
              "d2s_upsample_depth")
    return out


def warp_plan(rgb_fmt: int, dh: int, dw: int, batch: int, H: int, W: int, sp: SbsParams, out_fmt: int = FMT_U8_HWC, rgb_align: int = 256,
              out_align: int = 256) -> dict:
    """What d2s_make_sbs would launch for these arguments (include/d2s.h d2s_warp_plan; host code, no GPU): kernel name, rpw, ntx, wpc,
    waves, grid."""
    r = _lib.WarpPlanResult()
    r.struct_size = C.sizeof(_lib.WarpPlanResult)
    check(_lib.load().d2s_warp_plan(int(rgb_fmt), int(dh), int(dw), int(batch), int(H), int(W), C.byref(sp), int(out_fmt), int(rgb_align),
                                    int(out_align), C.byref(r)), "d2s_warp_plan")
    return {"kernel": r.kernel.decode(), "gather": bool(r.gather), "direct": bool(r.direct), "nc": r.nc, "ntx": r.ntx, "wpc": r.wpc, "rpw": r.rpw,
            "waves": r.waves, "grid": r.grid, "out_h": r.out_h, "out_w": r.out_w}


def preprocess_patches_probe(precision: str, frames: torch.Tensor, A: torch.Tensor, resid: torch.Tensor, *, h: int, w: int, p: int, Kp: int,
                             N: int, D: int, cls: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, decim_stride: int = 1,
                             pre: Optional[PreParams] = None, fmt: Optional[int] = None) -> str:
    """One launch of d2s_pipeline's fused pre-process + patchify (test probe, include/d2s.h d2s_preprocess_patches_probe) on caller-owned
    device buffers, used in place: frames [B,H,W,3] uint8 (fmt overrides the format the library is told), A the patch rows (torch.bfloat16
    / float32), resid float32 [B,N,D].  Returns the kernel's name; raises D2SError where the library refuses (status in the message)."""
    _need_cuda(frames, "frames")
    q = _lib.PrepatchProbeParams()
    q.struct_size = C.sizeof(_lib.PrepatchProbeParams)
    q.precision = {"bf16": PREC_BF16, "fp32": PREC_FP32}[precision]
    f, B, H, W = _frame_fmt(frames)
    q.fmt = f if fmt is None else int(fmt)
    q.batch, q.H, q.W, q.decim_stride = B, H, W, int(decim_stride)
    q.h, q.w, q.p, q.Kp, q.N, q.D = int(h), int(w), int(p), int(Kp), int(N), int(D)
    q.pre = C.pointer(pre) if pre is not None else None
    for name, t in (("frames", frames), ("A", A), ("cls", cls), ("pos", pos), ("resid", resid)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError("preprocess_patches_probe: tensors must be contiguous")
        setattr(q, name, t.data_ptr())
        setattr(q, name + "_elems", t.numel())
    with _on(frames.device) as st:
        check(_lib.load().d2s_preprocess_patches_probe(C.byref(q), st), "d2s_preprocess_patches_probe")
    return q.kernel.decode()


def vit_probe(op: str, precision: str, x: torch.Tensor, out: torch.Tensor, *, B: int = 0, h: int = 0, w: int = 0, p: int = 0, Kp: int = 0,
              N: int = 0, D: int = 0, Hi: int = 0, Wi: int = 0, Ho: int = 0, Wo: int = 0, channels: int = 0, n: int = 0, b3: float = 0.0,
              max_depth: float = 0.0, addend: Optional[torch.Tensor] = None, w3: Optional[torch.Tensor] = None,
              cls: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None) -> str:
    """One launch of a small model-side launcher of vit_ops.hip (test probe, include/d2s.h d2s_vit_probe).  op: "patchify" | "bilinear" |
    "head_final" | "to_f32" | "amax"; precision "bf16" | "fp32".  The tensors are device buffers ALREADY in the kernel's storage type and
    are used in place -- views into larger guarded buffers are fine; the element counts the library checks against are what each tensor
    holds from its first element.  out: A (patchify), the up-sampled map, the depth, the float32 copy, or the slot (amax: the tensor whose
    first element is the slot).  Returns the name of the kernel that ran; raises D2SError where the library refuses."""
    _need_cuda(x, "x")
    q = _lib.VitProbeParams()
    q.struct_size = C.sizeof(_lib.VitProbeParams)
    q.op = _lib.VIT_OPS[op]
    q.precision = {"bf16": PREC_BF16, "fp32": PREC_FP32}[precision]
    q.B, q.h, q.w, q.p, q.Kp, q.N, q.D = int(B), int(h), int(w), int(p), int(Kp), int(N), int(D)
    q.Hi, q.Wi, q.Ho, q.Wo, q.C, q.n = int(Hi), int(Wi), int(Ho), int(Wo), int(channels), int(n)
    q.b3, q.max_depth = float(b3), float(max_depth)
    for name, t in (("x", x), ("out", out), ("addend", addend), ("w3", w3), ("cls", cls), ("pos", pos), ("resid", resid)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError("vit_probe: tensors must be contiguous")
        setattr(q, name, t.data_ptr())
        setattr(q, name + "_elems", t.numel())
    with _on(x.device) as st:
        check(_lib.load().d2s_vit_probe(C.byref(q), st), "d2s_vit_probe")
    return q.kernel.decode()
