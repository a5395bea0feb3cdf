"""ctypes binding of libd2s_hip.so (include/d2s.h).

The library is the product path: if it is missing or a symbol is absent this module raises --
there is no CPU or PyTorch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("D2S_LIB") or os.path.join(HERE, "libd2s_hip.so")     # D2S_LIB: another build of the same library (A/B runs)

OK = 0
MODE = {"Half-SBS": 0, "Full-SBS": 1, "Half-TAB": 2, "Full-TAB": 3}
FMT_U8_HWC, FMT_F32_CHW, FMT_F32_HWC, FMT_U8_CHW = 0, 1, 2, 3
PREC_FP32, PREC_BF16, PREC_FP8, PREC_BF16X3, PREC_FP8_MLP = 0, 1, 2, 3, 4


class ModelDesc(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("heads", C.c_int32), ("layers", C.c_int32),
                ("out_indices", C.c_int32 * 4), ("neck", C.c_int32 * 4), ("fusion", C.c_int32),
                ("head_hidden", C.c_int32), ("mlp", C.c_int32), ("patch", C.c_int32),
                ("pos_grid", C.c_int32), ("ln_eps", C.c_float), ("precision", C.c_int32), ("temporal", C.c_int32),
                ("max_depth", C.c_float)]


class PostParams(C.Structure):
    _fields_ = [("percentile", C.c_float), ("subsample_cap", C.c_int32), ("gamma", C.c_float),
                ("foreground_scale", C.c_float), ("aa_strength", C.c_float), ("ema_alpha", C.c_float),
                ("metric", C.c_int32)]


RESAMPLE = {"bilinear": 0, "bicubic_aa": 1}      # D2S_RESAMPLE_*: _resize_patch_aligned_t's CPU branch / IS_CUDA branch


class PreParams(C.Structure):
    _fields_ = [("mean", C.c_float * 3), ("std", C.c_float * 3), ("resample", C.c_int32), ("square", C.c_int32)]


class SbsParams(C.Structure):
    _fields_ = [("ipd_uv", C.c_double), ("depth_ratio", C.c_float), ("convergence", C.c_float),
                ("display_mode", C.c_int32), ("fill_16_9", C.c_int32)]


class DibrParams(C.Structure):
    _fields_ = [("ipd_uv", C.c_double), ("depth_strength", C.c_float), ("convergence", C.c_float), ("roll", C.c_float),
                ("search_radius", C.c_float), ("depth_tolerance", C.c_float), ("blur_radius", C.c_float),
                ("res_w", C.c_float), ("res_h", C.c_float), ("display_mode", C.c_int32),
                ("feather_enabled", C.c_int32), ("feather_width", C.c_float), ("corner_radius", C.c_float),
                ("viewport", C.c_float * 4), ("alpha_mode", C.c_int32), ("struct_size", C.c_uint32)]


class XrScreen(C.Structure):
    """d2s_xr_screen: the OpenXR viewer's screen in world space (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("curve", C.c_int32), ("width", C.c_double), ("height", C.c_double),
                ("distance", C.c_double), ("pan_x", C.c_double), ("pan_y", C.c_double), ("yaw", C.c_double), ("pitch", C.c_double),
                ("roll", C.c_double), ("normal_offset", C.c_double), ("clear", C.c_float * 4)]


class XrEye(C.Structure):
    """d2s_xr_eye: one swapchain image -- vp = proj @ view row-major, its size, and which eye's offset the shader takes."""
    _fields_ = [("vp", C.c_double * 16), ("width", C.c_int32), ("height", C.c_int32), ("eye", C.c_int32), ("struct_size", C.c_uint32)]


class XrGlow(C.Structure):
    """d2s_xr_glow: the glow around the flat screen (mode 0 off, 1 glow, 2 glow2)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("range_m", C.c_double), ("inner_edge_fraction", C.c_double)]


class XrFrost(C.Structure):
    """d2s_xr_frost: the veil / frosted look around the flat screen (mode 0 off, 1 veil, 2 frosted)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("head", C.c_double * 3), ("intensity", C.c_double), ("alpha", C.c_double),
                ("edge_inset", C.c_double), ("beam_softness", C.c_double), ("beam_thickness", C.c_double), ("lod", C.c_double),
                ("threshold", C.c_double), ("noise_scale", C.c_double), ("blend", C.c_double), ("diffuse", C.c_double), ("time", C.c_double)]


class XrPanorama(C.Structure):
    """d2s_xr_panorama: the panorama background behind the screen (ray: per eye image, NDC (x, y, 1) -> world direction, row-major)."""
    _fields_ = [("struct_size", C.c_uint32), ("flip_y", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("yaw_offset", C.c_double), ("exposure", C.c_double), ("ray", (C.c_double * 9) * 2)]


class XrPanel(C.Structure):
    """d2s_xr_panel: one world-space panel -- the unit quad under `model` (row-major), textured (index) or solid (-1, color)."""
    _fields_ = [("model", C.c_double * 16), ("texture", C.c_int32), ("flags", C.c_uint32), ("color", C.c_float * 4), ("alpha", C.c_float),
                ("struct_size", C.c_uint32)]


class XrTexture(C.Structure):
    """d2s_xr_texture: a panel's RGBA8 picture on the device, row 0 = its top row."""
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("wrap", C.c_int32), ("struct_size", C.c_uint32)]


class XrPanelsPlanResult(C.Structure):
    """d2s_xr_panels_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("rows_per_eye", C.c_int32), ("setup_launches", C.c_int32), ("render_launches", C.c_int32),
                ("drawn", C.c_int32 * 2), ("tile0", (C.c_int32 * 2) * 2), ("tiles", (C.c_int32 * 2) * 2), ("grid", C.c_uint32 * 3),
                ("reserved", C.c_uint32), ("workspace_bytes", C.c_uint64), ("out_elems", C.c_uint64), ("offsets", C.c_uint64 * 2)]


XR_PANEL_DEPTH_TEST, XR_PANEL_DEPTH_WRITE, XR_PANEL_BLEND = 1, 2, 4      # D2S_XR_PANEL_*
XR_WRAP = {"repeat": 0, "clamp": 1}      # D2S_XR_WRAP_*
XR_MAX_PANELS = 32
XR_GLOW = {"off": 0, "glow": 1, "glow2": 2}
XR_FROST = {"off": 0, "veil": 1, "frosted": 2}
XR_CURVE = {"flat": 0, "horizontal": 1, "vertical": 2}      # D2S_XR_CURVE_*
DIBR_ALPHA = {"window": 0, "premultiplied": 1, "rgba": 2}      # D2S_DIBR_ALPHA_*
COMPOSITE = {"Anaglyph": 0, "Interleaved": 1, "Interleaved-V": 2, "Depth Map": 3}      # D2S_COMPOSITE_*


class Conv3ProbeParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("precision", C.c_int32), ("tile", C.c_int32),
                ("batch", C.c_int32), ("C", C.c_int32), ("N", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("Hi", C.c_int32), ("Wi", C.c_int32), ("stride", C.c_int32), ("relu_in", C.c_int32), ("act", C.c_int32),
                ("out_f32", C.c_int32), ("map_head", C.c_int32), ("b3", C.c_float), ("max_depth", C.c_float),
                ("reserved", C.c_int32), ("splitk_elems", C.c_int64),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("w3", C.c_void_p),
                ("out", C.c_void_p), ("kernel", C.c_char * 128)]


class RcuProbeParams(C.Structure):
    """d2s_rcu_probe_params (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("batch", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("reserved", C.c_int32), ("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p),
                ("b2", C.c_void_p), ("wp", C.c_void_p), ("bp", C.c_void_p), ("out", C.c_void_p), ("kernel", C.c_char * 128)]


class AttentionProbeParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("precision", C.c_int32), ("B", C.c_int32), ("heads", C.c_int32), ("N", C.c_int32),
                ("out_e4m3", C.c_int32), ("oscale", C.c_float), ("reserved", C.c_int32),
                ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p), ("kernel", C.c_char * 128)]


class LinearProbeParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("site", C.c_int32), ("precision", C.c_int32), ("ln_fold", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ntok", C.c_int32), ("heads", C.c_int32), ("npad", C.c_int32),
                ("gh", C.c_int32), ("gw", C.c_int32), ("ks", C.c_int32), ("pK", C.c_int32), ("ln_eps", C.c_float),
                ("s_act", C.c_float), ("s_out", C.c_float), ("s_res", C.c_float), ("s_pact", C.c_float), ("tile", C.c_int32),
                ("splitk_elems", C.c_int64),
                ("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p), ("res", C.c_void_p), ("res2", C.c_void_p),
                ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("pa", C.c_void_p), ("pw", C.c_void_p), ("pbias", C.c_void_p),
                ("pscale", C.c_void_p), ("x", C.c_void_p), ("out", C.c_void_p), ("out2", C.c_void_p), ("vt", C.c_void_p),
                ("stats", C.c_void_p), ("stats_slots", C.c_int32), ("reserved", C.c_int32),
                ("kernel", C.c_char * 128), ("kernel2", C.c_char * 128)]


class TemporalProbeParams(C.Structure):
    """d2s_temporal_probe_params (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("precision", C.c_int32), ("rows", C.c_int32), ("sites", C.c_int32),
                ("C", C.c_int32), ("groups", C.c_int32), ("slots", C.c_int32), ("eps", C.c_float), ("qscale", C.c_float),
                ("bx3_out", C.c_int32), ("rows_per_img", C.c_int32), ("img_rows", C.c_int32), ("row_off", C.c_int32), ("n", C.c_int64),
                ("x", C.c_void_p), ("out", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("ptab", C.c_void_p),
                ("x_elems", C.c_uint64), ("out_elems", C.c_uint64), ("gamma_elems", C.c_uint64), ("beta_elems", C.c_uint64),
                ("ptab_elems", C.c_uint64), ("ring", C.c_void_p * 32), ("ring_elems", C.c_uint64 * 32),
                ("head", C.c_int32 * 32), ("Tw", C.c_int32 * 32), ("store_slot", C.c_int32 * 32),
                ("slot0", C.c_int32 * 32), ("nslots", C.c_int32 * 32), ("kernel", C.c_char * 128)]


class WarpPlanResult(C.Structure):
    """d2s_warp_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("gather", C.c_int32), ("direct", C.c_int32), ("nc", C.c_int32), ("ntx", C.c_int32),
                ("wpc", C.c_int32), ("rpw", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("grid", C.c_uint32),
                ("waves", C.c_int64), ("kernel", C.c_char * 64)]


class DibrWarpPlanResult(C.Structure):
    """d2s_dibr_warp_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_int32), ("cols", C.c_int32), ("margin", C.c_int32), ("ww", C.c_int32),
                ("roll0", C.c_int32), ("up", C.c_int32), ("fx", C.c_int32), ("oh", C.c_int32), ("ow", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("grid", C.c_uint32 * 3), ("block", C.c_uint32), ("lds_dynamic_bytes", C.c_uint32),
                ("lds_static_bytes", C.c_uint32), ("kernel", C.c_char * 64)]


class DibrCompositePlanResult(C.Structure):
    """d2s_dibr_composite_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_int32), ("cols", C.c_int32), ("margin", C.c_int32), ("ww", C.c_int32),
                ("roll0", C.c_int32), ("up", C.c_int32), ("fx", C.c_int32), ("vec", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("grid", C.c_uint32 * 3), ("block", C.c_uint32), ("lds_dynamic_bytes", C.c_uint32), ("lds_static_bytes", C.c_uint32),
                ("kernel", C.c_char * 64)]


class PostPlanResult(C.Structure):
    """d2s_post_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("form", C.c_int32), ("launches", C.c_int32), ("k", C.c_int32), ("r", C.c_int32),
                ("step", C.c_int32), ("m", C.c_int32), ("tail", C.c_int32), ("lds_bytes", C.c_uint32 * 3), ("kernel", (C.c_char * 32) * 3)]


POST_FORM = {0: "fused", 1: "tile", 2: "rows"}      # D2S_POST_FORM_*


class XrPlanResult(C.Structure):
    """d2s_xr_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("rows_per_eye", C.c_int32), ("setup_launches", C.c_int32),
                ("grid", C.c_uint32 * 3), ("lds_dynamic_bytes", C.c_uint32), ("lds_static_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("workspace_bytes", C.c_uint64), ("out_elems", C.c_uint64), ("offsets", C.c_uint64 * 2)]


XR_ENTRY = {"eyes": 0, "glow": 1, "glow_curved": 2}      # D2S_XR_ENTRY_*
XR_KIND = {0: "plain", 1: "glow", 2: "glow_curved", 3: "frost", 4: "frost_curved"}      # D2S_XR_KIND_*


class ForwardPlanResult(C.Structure):
    """d2s_forward_plan_result (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("f8", C.c_int32), ("f8a", C.c_int32), ("x3", C.c_int32), ("lnf", C.c_int32),
                ("pp_fold", C.c_int32), ("tap_fold", C.c_int32), ("use_side", C.c_int32), ("ln_slots", C.c_int32 * 2),
                ("site", C.c_int32 * 11), ("tap_side", C.c_int32 * 4), ("head1_ups", C.c_int32), ("head2_fused", C.c_int32),
                ("head2_ups", C.c_int32), ("bn", C.c_int32), ("tm_fold", C.c_int32), ("tm_cache_store", C.c_int32),
                ("tm_slots", (C.c_int32 * 3) * 4), ("tm_folded", (C.c_int32 * 3) * 4), ("gh", C.c_int32), ("gw", C.c_int32),
                ("P", C.c_int32), ("N", C.c_int32), ("Npad", C.c_int32), ("fH", C.c_int32 * 4), ("fW", C.c_int32 * 4),
                ("tm_C", C.c_int32 * 4), ("tm_sites", C.c_int32 * 4), ("ln_launches", C.c_int32), ("rcu_fused", C.c_int32),
                ("splitk_elems", C.c_uint64), ("scr_elems", C.c_uint64)]


PLAN_FLAGS = {"calibrating": 1, "profiling": 2, "window_filled": 4, "calibrated": 8}      # D2S_PLAN_*
PLAN_SITES = ("patch", "qkv0", "qkv", "proj", "fc1", "fc2", "fc2_last", "neck0", "neck1", "neck2", "neck3")      # D2S_PLAN_SITE_*


class PrepatchProbeParams(C.Structure):
    """d2s_prepatch_probe_params (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("precision", C.c_int32), ("fmt", C.c_int32), ("batch", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("decim_stride", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("p", C.c_int32), ("Kp", C.c_int32),
                ("N", C.c_int32), ("D", C.c_int32), ("reserved", C.c_int32), ("pre", C.POINTER(PreParams)), ("frames", C.c_void_p),
                ("A", C.c_void_p), ("cls", C.c_void_p), ("pos", C.c_void_p), ("resid", C.c_void_p),
                ("frames_elems", C.c_uint64), ("A_elems", C.c_uint64), ("cls_elems", C.c_uint64), ("pos_elems", C.c_uint64),
                ("resid_elems", C.c_uint64), ("kernel", C.c_char * 64)]


class VitProbeParams(C.Structure):
    """d2s_vit_probe_params (include/d2s.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("precision", C.c_int32), ("B", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("p", C.c_int32), ("Kp", C.c_int32), ("N", C.c_int32), ("D", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("C", C.c_int32), ("b3", C.c_float), ("max_depth", C.c_float), ("reserved", C.c_int32),
                ("n", C.c_int64), ("x", C.c_void_p), ("out", C.c_void_p), ("addend", C.c_void_p), ("w3", C.c_void_p), ("cls", C.c_void_p),
                ("pos", C.c_void_p), ("resid", C.c_void_p), ("x_elems", C.c_uint64), ("out_elems", C.c_uint64), ("addend_elems", C.c_uint64),
                ("w3_elems", C.c_uint64), ("cls_elems", C.c_uint64), ("pos_elems", C.c_uint64), ("resid_elems", C.c_uint64),
                ("kernel", C.c_char * 64)]


VIT_OPS = {"patchify": 0, "bilinear": 1, "head_final": 2, "to_f32": 3, "amax": 4}      # D2S_VP_*

TEMPORAL_OPS = {"groupnorm": 0, "temporal_attn": 1, "cache_store": 2, "geglu": 3, "cast_f32": 4, "layernorm": 5}      # D2S_TP_*

LINEAR_SITES = {"patch": 0, "qkv": 1, "proj": 2, "fc1": 3, "fc2": 4, "neck_proj": 5, "neck_resize": 6, "tm_proj_in": 7,    # D2S_LIN_*
                "tm_kvq": 8, "tm_ff1": 9, "tm_to_out": 10, "tm_ff2": 11, "tm_proj_out": 12}


# every symbol include/d2s.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "d2s_last_error": (C.c_char_p, []),
    "d2s_version": (C.c_int, []),
    "d2s_debug_reload_env": (C.c_int, []),
    "d2s_debug_lds_poison": (C.c_int, []),
    "d2s_debug_pp_tail_timeouts": (C.c_int, [C.c_int, C.POINTER(C.c_uint)]),
    "d2s_engine_create": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_P)]),
    "d2s_engine_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "d2s_engine_finalize": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "d2s_engine_destroy": (C.c_int, [_P]),
    "d2s_engine_memory": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "d2s_preprocess": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(PreParams), _P]),
    "d2s_process_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_process": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "d2s_process_rgb": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "d2s_process_area_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_process_area": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "d2s_overlay_text": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_char_p, _P]),
    "d2s_model_forward": (C.c_int, [_P, _P, _P, C.c_int, _P]),
    "d2s_model_forward_streams": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int), _P]),
    "d2s_engine_reset_stream_at": (C.c_int, [_P, C.c_int]),
    "d2s_engine_calibrate": (C.c_int, [_P, _P, C.c_int, _P]),
    "d2s_forward_plan": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ForwardPlanResult)]),
    "d2s_post_process": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(PostParams), _P, C.c_uint64, _P]),
    "d2s_post_process_workspace": (C.c_uint64, [C.c_int, C.c_int, C.c_int]),
    "d2s_post_process_to": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(PostParams), _P, C.c_uint64, _P]),
    "d2s_post_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(PostParams), C.c_int, C.POINTER(PostPlanResult)]),
    "d2s_ema_update": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "d2s_upsample_depth": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P]),
    "d2s_make_sbs": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.POINTER(SbsParams), _P, C.c_int, _P]),
    "d2s_sbs_shape": (C.c_int, [C.c_int, C.c_int, C.POINTER(SbsParams), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_dibr_shape": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_dibr_warp": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), _P, C.c_int, _P]),
    "d2s_dibr_composite_shape": (C.c_int, [C.c_int, C.c_int, C.POINTER(DibrParams), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_dibr_composite": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.c_int, _P, C.c_int, _P]),
    "d2s_dibr_warp_depth": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), _P, C.c_int, _P]),
    "d2s_dibr_composite_depth": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.c_int, _P, C.c_int, _P]),
    # the OpenXR movie crop (xr_viewer/crop.py:165-173, 298-435; xr_viewer/implementation.py:111-126)
    "d2s_dibr_crop_shape": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "d2s_dibr_warp_crop": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                     _P, C.c_int, _P]),
    # the OpenXR eye views (xr_viewer/effects.py:1023-1137, xr_viewer/screen.py:29-173)
    "d2s_dibr_composite_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.c_int, C.c_int, C.c_uint,
                                          C.POINTER(DibrCompositePlanResult)]),
    "d2s_dibr_warp_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double), C.c_int,
                                     C.POINTER(DibrWarpPlanResult)]),
    "d2s_dibr_xr_shape": (C.c_int, [C.POINTER(XrEye), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_eyes": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                   C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, _P]),
    # the colour mip chain and the glow around the flat screen (xr_viewer/effects.py:476-646, xr_viewer/glsl.py:580-666)
    "d2s_mip_shape": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_uint64)]),
    "d2s_mip_chain": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "d2s_dibr_xr_eyes_glow": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                        C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, C.POINTER(XrGlow), _P, _P]),
    "d2s_view_pipeline_xr_glow_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                    C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double), C.POINTER(XrScreen),
                                                    C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.POINTER(XrGlow), _P, _P]),
    "d2s_dibr_xr_glow_curved_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_eyes_glow_curved": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                               C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, C.POINTER(XrGlow), _P, _P]),
    "d2s_dibr_xr_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                   C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, C.POINTER(XrGlow), C.POINTER(XrPlanResult)]),
    # the veil and frosted looks of the flat screen (xr_viewer/effects.py:102-187, 789-857, xr_viewer/glsl.py:668-791)
    "d2s_dibr_xr_frost_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_eyes_frost": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                         C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, C.POINTER(XrFrost), _P, _P]),
    "d2s_dibr_xr_frost_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                         C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, C.POINTER(XrFrost), C.POINTER(XrPlanResult)]),
    "d2s_view_pipeline_xr_frost_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                     C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double), C.POINTER(XrScreen),
                                                     C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, C.POINTER(XrFrost), _P, _P]),
    # the veil and frosted looks of the curved screen (xr_viewer/effects.py:189-254, 759-787): the flat entries' argument lists
    "d2s_dibr_xr_frost_curved_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_eyes_frost_curved": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, C.POINTER(XrFrost), _P, _P]),
    "d2s_dibr_xr_frost_curved_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, C.POINTER(XrFrost), C.POINTER(XrPlanResult)]),
    "d2s_view_pipeline_xr_frost_curved_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                            C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                            C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P,
                                                            C.c_uint64, C.POINTER(XrFrost), _P, _P]),
    # the panorama background behind the screen (xr_viewer/effects.py:930-1021, xr_viewer/glsl.py:57-94): the frost entries' argument
    # lists, then the glow, the panorama, its image and its chain
    "d2s_dibr_xr_eyes_panorama": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                            C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P, C.c_uint64, C.POINTER(XrFrost), _P,
                                            C.POINTER(XrGlow), C.POINTER(XrPanorama), _P, _P, _P]),
    "d2s_dibr_xr_panorama_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                            C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, C.POINTER(XrFrost), C.POINTER(XrGlow),
                                            C.POINTER(XrPanorama), C.POINTER(XrPlanResult)]),
    "d2s_view_pipeline_xr_panorama_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                        C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                        C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P,
                                                        C.c_uint64, C.POINTER(XrFrost), _P, C.POINTER(XrGlow), C.POINTER(XrPanorama), _P, _P, _P]),
    # the panorama also behind the curved screen's glow, veil and frosted looks: the panorama entries' argument lists
    "d2s_dibr_xr_eyes_panorama_curved": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams),
                                                   C.POINTER(C.c_double), C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, _P, C.c_int, _P,
                                                   C.c_uint64, C.POINTER(XrFrost), _P, C.POINTER(XrGlow), C.POINTER(XrPanorama), _P, _P, _P]),
    "d2s_dibr_xr_panorama_curved_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                   C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, C.POINTER(XrFrost),
                                                   C.POINTER(XrGlow), C.POINTER(XrPanorama), C.POINTER(XrPlanResult)]),
    "d2s_view_pipeline_xr_panorama_curved_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                                               C.POINTER(PreParams), C.POINTER(PostParams), C.POINTER(DibrParams),
                                                               C.POINTER(C.c_double), C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int,
                                                               _P, C.c_int, _P, _P, C.c_uint64, C.POINTER(XrFrost), _P, C.POINTER(XrGlow),
                                                               C.POINTER(XrPanorama), _P, _P, _P]),
    # the world-space panels drawn in place over finished eye images (xr_viewer/overlay.py:81-249, 1427-1510)
    "d2s_dibr_xr_panels_workspace": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_dibr_xr_panels": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.POINTER(XrPanel), C.c_int,
                                     C.POINTER(XrTexture), C.c_int, _P, C.c_uint64, _P]),
    "d2s_dibr_xr_panels_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.POINTER(XrPanel), C.c_int,
                                          C.POINTER(XrTexture), C.c_int, C.POINTER(XrPanelsPlanResult)]),
    "d2s_view_pipeline_xr_glow_curved_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                           C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double),
                                                           C.POINTER(XrScreen), C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P,
                                                           C.c_uint64, C.POINTER(XrGlow), _P, _P]),
    "d2s_crop_detect_workspace":(C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "d2s_crop_detect": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_uint64, _P]),
    "d2s_jpeg_bound": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "d2s_jpeg_encode": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    "d2s_present_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "d2s_present_bind": (C.c_int, [_P, C.c_int, _P, C.c_uint64]),
    "d2s_present_bind_gl_buffer": (C.c_int, [_P, C.c_int, C.c_uint]),
    "d2s_present_acquire": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "d2s_present_publish": (C.c_int, [_P, C.c_int, _P]),
    "d2s_present_cancel": (C.c_int, [_P, C.c_int, _P]),
    "d2s_present_consume": (C.c_int, [_P, _P, C.POINTER(C.c_int), C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "d2s_present_release": (C.c_int, [_P, C.c_int, _P]),
    "d2s_present_destroy": (C.c_int, [_P]),
    "d2s_pipeline": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PreParams), C.POINTER(PostParams),
                               C.POINTER(SbsParams), C.c_int, _P, C.c_int, _P, _P]),
    "d2s_pipeline_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                       C.POINTER(PostParams), C.POINTER(SbsParams), C.c_int, _P, C.c_int, _P, _P]),
    "d2s_view_pipeline_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                            C.POINTER(PostParams), C.POINTER(DibrParams), C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "d2s_view_pipeline_crop_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                                 C.POINTER(PostParams), C.POINTER(DibrParams), C.c_int, C.POINTER(C.c_double), C.c_int, _P,
                                                 C.c_int, _P, _P]),
    "d2s_view_pipeline_xr_streams": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(PreParams),
                                               C.POINTER(PostParams), C.POINTER(DibrParams), C.POINTER(C.c_double), C.POINTER(XrScreen),
                                               C.POINTER(XrEye), C.c_int, C.c_int, _P, C.c_int, _P, _P, C.c_uint64, _P]),
    "d2s_engine_reset_stream": (C.c_int, [_P]),
    "d2s_engine_tap": (C.c_int, [_P, C.c_char_p, _P, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "d2s_engine_profile": (C.c_int, [_P, C.c_int]),
    "d2s_engine_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "d2s_profile_class_name": (C.c_char_p, [C.c_int]),
    "d2s_gemm_probe": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "d2s_attention_probe": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "d2s_attention_probe_ex": (C.c_int, [C.POINTER(AttentionProbeParams), _P]),
    "d2s_conv3_probe": (C.c_int, [C.POINTER(Conv3ProbeParams), _P]),
    "d2s_rcu_probe": (C.c_int, [C.POINTER(RcuProbeParams), _P]),
    "d2s_linear_probe": (C.c_int, [C.POINTER(LinearProbeParams), _P]),
    "d2s_temporal_probe": (C.c_int, [C.POINTER(TemporalProbeParams), _P]),
    "d2s_warp_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SbsParams), C.c_int, C.c_int, C.c_int,
                                C.POINTER(WarpPlanResult)]),
    "d2s_preprocess_patches_probe": (C.c_int, [C.POINTER(PrepatchProbeParams), _P]),
    "d2s_vit_probe": (C.c_int, [C.POINTER(VitProbeParams), _P]),
}

_lib = None


class D2SError(RuntimeError):
    pass


def load(path: str = LIB_PATH):
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise D2SError(f"{path} not found: build it with `python -m desktop2stereo_amd.build` "
                       "(there is no fallback path)")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status != OK:
        msg = load().d2s_last_error()
        raise D2SError(f"{what or 'libd2s_hip'} failed (status {status}): {msg.decode() if msg else ''}")
