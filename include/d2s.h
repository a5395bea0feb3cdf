/*
 * d2s.h -- C-ABI of libd2s_hip.so: the MI355X (gfx950) implementation of the
 * desktop2stereo per-frame hot path  depth inference -> depth post-process -> stereo warp.
 *
 * The reference has no FFI for this path; its boundary is the Python call surface of depth.py
 * plus an internal "engine object" protocol (DepthModelWrapper.__call__, reference
 * depth.py:1763-1781; MIGraphXEngine.__call__, depth.py:1029-1045: raw device pointers,
 * caller-allocated output, launched on torch's current hipStream, no host sync).  This header is
 * what a replacement engine exports under that protocol.  Conventions, mirroring the
 * reference's own ctypes->libamdhip64 usage (viewer.py:283-299: int status, != 0 -> RuntimeError):
 *
 *   - every function returns int: D2S_OK (0) or a D2S_E_* code; d2s_last_error() gives text;
 *   - all image / tensor pointers are DEVICE pointers owned by the caller (PyTorch-ROCm tensors'
 *     data_ptr()); the library allocates only weights, workspaces and per-stream state;
 *   - every call is asynchronous on the hipStream_t passed as `void* stream` (0 = null stream);
 *     there is no host synchronisation inside the library after engine finalisation;
 *   - no torch types, only plain pointers and sizes.
 *
 * Each entry point cites the reference interface it replaces (file:line in /root/reference).
 */
#ifndef D2S_H
#define D2S_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D2S_OK              0
#define D2S_E_INVALID       1   /* bad argument / shape / mode */
#define D2S_E_STATE         2   /* call order (e.g. forward before finalize) */
#define D2S_E_HIP           3   /* a HIP runtime call failed */
#define D2S_E_MISSING       4   /* a weight tensor is missing or mis-shaped */
#define D2S_E_UNSUPPORTED   5

/* display modes of make_sbs_core (reference depth.py:2178-2183) */
#define D2S_MODE_HALF_SBS   0
#define D2S_MODE_FULL_SBS   1
#define D2S_MODE_HALF_TAB   2
#define D2S_MODE_FULL_TAB   3

/* pixel formats at the boundary */
#define D2S_FMT_U8_HWC      0   /* uint8  [H,W,3]   (numpy frame, reference depth.py:1921-1922) */
#define D2S_FMT_F32_CHW     1   /* float  [3,H,W]   (make_sbs_core tensor in/out, depth.py:2135-2138) */
#define D2S_FMT_F32_HWC     2   /* float  [H,W,3]   (make_sbs return, depth.py:767-773, 2231) */
#define D2S_FMT_U8_CHW      3   /* uint8  [3,H,W]   (rgb_tensor of predict_depth(return_tuple), depth.py:1922) */

/* arithmetic of the model stage */
#define D2S_PREC_FP32       0   /* f32 MFMA (v_mfma_f32_16x16x4_f32), fp32 activations: parity class */
#define D2S_PREC_BF16       1   /* bf16 MFMA, fp32 accumulate / residual / softmax / LayerNorm */
#define D2S_PREC_FP8        2   /* BASELINE config 3: the encoder's four linears per layer (75 % of the FLOPs) run on e4m3
                                   operands (OCP e4m3fn; weights per-output-channel scales, activations static per-tensor
                                   scales set by d2s_engine_calibrate), fp32 accumulate; everything else as D2S_PREC_BF16 */
#define D2S_PREC_BF16X3     3   /* split precision (parity class on the bf16 pipe): fp32 activations everywhere as D2S_PREC_FP32, but
                                   every GEMM / convolution operand is split x = hi + lo into two bf16 values (the activation on its way
                                   into LDS, the weights once at engine build) and the product is three bf16 MFMAs
                                   hi*hi + hi*lo + lo*hi with fp32 accumulation: ~16 mantissa bits per operand at 3/16 of the
                                   fp32-MFMA cost.  Attention, LayerNorm, softmax, residual stream: exactly the fp32 engine's. */
#define D2S_PREC_FP8_MLP    4   /* round 5: as D2S_PREC_FP8 with e4m3 operands on FC1 / FC2 ONLY (60 % of the encoder FLOPs); QKV and the
                                   attention-out projection stay on bf16 operands.  The error / throughput frontier of the e4m3 schemes
                                   (profiles/r5_fp8_frontier.md): all four linears 0.0202 mean |depth error| on BASELINE configs[2]'s
                                   frame, MLP only 0.0120 */

typedef struct d2s_engine d2s_engine;     /* opaque: weights + workspaces + per-stream state */

/* Depth-Anything-v2 architecture (HF DepthAnythingConfig). */
typedef struct d2s_model_desc {
    int32_t hidden;            /* D */
    int32_t heads;
    int32_t layers;
    int32_t out_indices[4];    /* 1-based layer taps */
    int32_t neck[4];           /* neck_hidden_sizes */
    int32_t fusion;            /* fusion_hidden_size */
    int32_t head_hidden;       /* 32 */
    int32_t mlp;               /* 4*D */
    int32_t patch;             /* 14 */
    int32_t pos_grid;          /* 37 */
    float   ln_eps;            /* 1e-6 */
    int32_t precision;         /* D2S_PREC_* */
    int32_t temporal;          /* 1: Video-Depth-Anything streaming head (4 temporal modules, 32-frame window; reference
                                  models/video_depth_anything/vda2_s.py, dpt_temporal.py); max_batch = the number of
                                  independent stream slots, at most D2S_MAX_STREAMS (see d2s_model_forward_streams) */
    float   max_depth;         /* 0: relative head (conv3 -> ReLU).  > 0: metric head, sigmoid(conv3) * max_depth
                                  (HF depth_estimation_type="metric": 20 indoor / 80 outdoor; reference model ids
                                  utils.py:761-769) */
} d2s_model_desc;

/* Post-process constants (reference utils.py:858-859, depth.py:775, 816, 1889). */
typedef struct d2s_post_params {
    float   percentile;        /* 2.0 */
    int32_t subsample_cap;     /* 6144 */
    float   gamma;             /* 1.45 */
    float   foreground_scale;  /* FOREGROUND_SCALE = yaml/10 */
    float   aa_strength;       /* AA_STRENGTH = yaml*2 */
    float   ema_alpha;         /* 0.9 */
    int32_t metric;            /* is_metric() (reference depth.py:666-669): normalize() first inverts 1/d on d > 0
                                  and takes the order statistics over the valid values only (depth.py:844-847) */
} d2s_post_params;

/* Pre-processing constants of predict_depth (reference depth.py:676-706, 1794-1799, 1931-1948). */
#define D2S_RESAMPLE_BILINEAR    0   /* _resize_patch_aligned_t's CPU / DirectML branch (depth.py:700-706): [::stride] decimation,
                                        then bilinear align_corners=False -- what the reference's CPU path computes (parity default) */
#define D2S_RESAMPLE_BICUBIC_AA  1   /* its IS_CUDA branch (depth.py:698-699; IS_CUDA is true on a ROCm device): one bicubic +
                                        antialias F.interpolate from the full frame (ATen _upsample_bicubic2d_aa), no decimation */
typedef struct d2s_pre_params {
    float   mean[3];           /* (0.485, 0.456, 0.406); 0.5 for the dpt / zoedepth / depthpro ids (depth.py:1794-1799) */
    float   std[3];            /* (0.229, 0.224, 0.225) */
    int32_t resample;          /* D2S_RESAMPLE_* */
    int32_t square;            /* 0: aspect-preserving patch-aligned input (get_patch_size() = 14, depth.py:531-538).
                                  1: the fixed-square branch predict_depth takes when get_patch_size() is None -- CAPTURE_MODE ==
                                  "Window" (depth.py:532-533, 1937-1946): F.interpolate(bilinear, align_corners=False, no antialias)
                                  of the full frame to depth_resolution x depth_resolution on EVERY device (no decimation, `resample`
                                  is not consulted); the engine is depth_resolution x depth_resolution */
} d2s_pre_params;

/* Stereo parameters of make_sbs_core (reference depth.py:2122-2129). */
typedef struct d2s_sbs_params {
    double  ipd_uv;            /* 0.064; double because the reference forms ipd_uv*W in Python floats */
    float   depth_ratio;       /* 2.0 (function default) / DEPTH_STRENGTH */
    float   convergence;       /* 0.0 */
    int32_t display_mode;      /* D2S_MODE_* */
    int32_t fill_16_9;         /* 0/1 */
} d2s_sbs_params;

/* Uniforms of the reference's GLSL DIBR fragment shader (viewer.py:393-411) for d2s_dibr_warp. */
typedef struct d2s_dibr_params {
    double  ipd_uv;            /* viewer.ipd_uv (0.064): u_eye_offset = -/+ ipd_uv/2 for the left/right eye (viewer.py:2701, 2714) */
    float   depth_strength;    /* u_depth_strength = viewer.depth_strength (0.1) * depth_ratio (viewer.py:1334, 2686) */
    float   convergence;       /* u_convergence (viewer.py:1470) */
    float   roll;              /* u_roll, radians (xr_viewer/effects.py:1113); 0 in the desktop viewer */
    float   search_radius;     /* u_search_radius = 12 */
    float   depth_tolerance;   /* u_depth_tolerance = 0.012 */
    float   blur_radius;       /* u_blur_radius = 2.5 */
    float   res_w, res_h;      /* u_resolution; the reference never assigns it (pixel_size = 1/0 = +inf, viewer.py:395, 413): every
                                  tap at uv +- k * pixel_size then has a non-finite coordinate, which OpenGL leaves undefined
                                  (tests/golden/dibr.npz `as_shipped_*`: what SwiftShader renders for that state -- 6-17 % of the
                                  pixels more than one level from the intended image; recorded, not a target).
                                  0 here -> the source frame size, i.e. pixel_size = one texel: the shader's evident intent */
    int32_t display_mode;      /* D2S_MODE_*: how the two eye viewports are packed */
    int32_t feather_enabled;   /* u_feather_enabled */
    float   feather_width;     /* u_feather_width = 0.02 (viewer.py:1343) */
    float   corner_radius;     /* u_corner_radius (viewer.py:411, 617-624): rounded-box SDF over the quad's uv, alpha =
                                  1 - smoothstep(0, 0.01, sdf); 0 in the desktop viewer, 0.03 in the OpenXR screen
                                  (xr_viewer/implementation.py:293) */
    float   viewport[4];       /* u_viewport = (x, y, w, h) of the eye's viewport in pixels of the eye image, y up like
                                  gl_FragCoord (viewer.py:589: the feathering is relative to it); all 0: the eye image
                                  itself, (0, 0, out_w, out_h) */
    int32_t alpha_mode;        /* what becomes of frag_color.a (screen-edge clip :582, rounded corners :617-624), D2S_DIBR_ALPHA_*:
                                  the reference draws its stereo quads with GL_BLEND OFF (viewer.py:1304-1307 enable it around the
                                  overlay quad only), so its window shows frag_color.rgb as written = WINDOW (0, default);
                                  PREMULTIPLIED (1) = rgb * a, what an alpha-compositing consumer (the OpenXR layer) shows over
                                  black; RGBA (2) = frag_color itself, FOUR channels per pixel (rgb 0..255, a 0..255 / 0..1 for
                                  the u8 / f32 output formats) */
    uint32_t struct_size;      /* MUST be sizeof(d2s_dibr_params) = 80 (d2s_version() >= 110).  The struct grew from 72 to 80 bytes when
                                  alpha_mode was added; this field occupies what was tail padding, so the size is unchanged, and
                                  d2s_dibr_warp refuses anything else -- a caller built against the 72-byte header is rejected
                                  instead of having alpha_mode read from beyond its struct */
} d2s_dibr_params;
enum { D2S_DIBR_ALPHA_WINDOW = 0, D2S_DIBR_ALPHA_PREMULTIPLIED = 1, D2S_DIBR_ALPHA_RGBA = 2 };

/* The OpenXR viewer's screen in world space (d2s_version() >= 115), for d2s_dibr_xr_eyes: the surface EffectsMixin._render_eye draws
 * (xr_viewer/effects.py:1023-1137).  curve 0: the flat quad model * (+-1, +-1, 0, 1) of _build_model_mat4 (xr_viewer/screen.py:29-70);
 * curve 1 / 2: the 48-segment strip of _build_curved_screen_verts (screen.py:110-173) curved horizontally / vertically, half angle
 * _CURVED_HALF_ANGLE_RAD = 0.48 (xr_viewer/constants.py), radius = (width | height) / 2 / 0.48, basis and centre as _screen_effect_basis.
 * The library forms the surface in double precision (the reference rounds its matrices and vertices to float32). */
typedef struct d2s_xr_screen {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_screen) = 96 */
    int32_t  curve;            /* D2S_XR_CURVE_*: 0 flat, 1 horizontal, 2 vertical */
    double   width, height;    /* screen_width, screen_height in metres (> 0) */
    double   distance;         /* screen_distance (> 0): the centre sits at (pan_x, pan_y, -distance) */
    double   pan_x, pan_y;
    double   yaw, pitch, roll; /* radians.  roll is ALSO the shader's u_roll (effects.py:1113, 1129): d2s_dibr_params.roll is not read */
    double   normal_offset;    /* shifts the surface along its forward axis (the reference's depth bias against a room model) */
    float    clear[4];         /* the background the image is cleared to: rgb in 0..1 (_BG_COLORS) and a (the reference clears to 1) */
} d2s_xr_screen;
enum { D2S_XR_CURVE_FLAT = 0, D2S_XR_CURVE_HORIZONTAL = 1, D2S_XR_CURVE_VERTICAL = 2 };
/* One swapchain image.  vp = proj @ view (_fov_to_proj_mat4 @ _pose_to_view_mat4, xr_viewer/render.py:981-1041), row-major as numpy
 * holds it: clip = vp * (world, 1).  The reference's flip_y (effects.py:1032-1034) negates row 1 of proj before the product: the
 * CALLER applies it to vp; row 0 of the image is the top row of the GL framebuffer either way. */
typedef struct d2s_xr_eye {
    double   vp[16];
    int32_t  width, height;    /* 2 .. 8192 each */
    int32_t  eye;              /* 0: u_eye_offset = -ipd_uv / 2 (left), 1: +ipd_uv / 2 (right) */
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_eye) = 144 */
} d2s_xr_eye;

const char* d2s_last_error(void);
int d2s_version(void);
/* Kernel-selection switches (D2S_NO_HALO2, D2S_NO_WIDE, ... -- tuning aids) are read from the environment once and
 * cached; this makes the library read them again (tests run both sides of a switch in one process).  Returns the new generation. */
int d2s_debug_reload_env(void);
/* gemm_pp's in-kernel K-split tail reduce never dead-locks: a unit that has waited 50 us for its partners leaves, and the last arrival
 * sums its share (same bits).  That degradation is COUNTED, not silent: *count = units that timed out on the current device since the
 * last clear (synchronise the stream first); tests/test_gpu_soak.py requires 0.   */
int d2s_debug_pp_tail_timeouts(int clear, unsigned* count);
/* 1 if the library was built with -DD2S_LDS_POISON (LDS rings pre-filled with NaN patterns: a debug build for the parity suite). */
int d2s_debug_lds_poison(void);

/* ---------------------------------------------------------------------------------------------
 * Engine life cycle -- replaces DepthModelWrapper construction + lazy engine build
 * (reference depth.py:1539-1631, 1784-1789, 1842-1862).
 * ------------------------------------------------------------------------------------------- */
int d2s_engine_create(const d2s_model_desc* desc, int device_id, d2s_engine** out);
/* Upload one tensor by its HF state-dict name (reference weight contract: SURVEY.md section 8c).  `host`
 * is host float32, C-contiguous, `shape`/`ndim` as in the checkpoint.  Packing (bf16 cast,
 * [N][K] padding, conv tap order) happens here, once. */
int d2s_engine_set_weight(d2s_engine* e, const char* name, const float* host,
                          const int64_t* shape, int ndim);
/* Fix the model-input shape (cf. _ensure_engine_built, depth.py:1842-1862): h, w multiples of
 * patch; allocates workspaces for up to max_batch frames and pre-interpolates the position
 * embedding (HF Dinov2Embeddings.interpolate_pos_encoding, bicubic).  Synchronous. */
/* A temporal (Video-Depth-Anything) engine owns max_batch STREAM SLOTS, each with its own 32-frame window; more than this many is
 * refused (the per-call row table travels in the kernel arguments: 32 rows of 16 bytes). */
#define D2S_MAX_STREAMS 32
int d2s_engine_finalize(d2s_engine* e, int h, int w, int max_batch);
int d2s_engine_destroy(d2s_engine* e);
/* bytes of device memory the engine holds (weights + workspaces) */
int d2s_engine_memory(const d2s_engine* e, uint64_t* bytes);

/* ---------------------------------------------------------------------------------------------
 * Stages.  Each mirrors one reference function; all device pointers, stream-ordered.
 * ------------------------------------------------------------------------------------------- */

/* A1: process(img, height)  (reference depth.py:540-566, the torch branch a ROCm/CUDA device takes):
 * bgr: uint8 HWC [H0,W0,channels], channels 3 (BGR) or 4 (BGRA) -> out: float RGB CHW [3,h,w], 0..255.
 * target_height >= H0: swizzle only ((h,w) = (H0,W0)); else F.interpolate(bilinear, align_corners=False,
 * antialias=True) to (h,w) = ((target//2)*2, (int(W0*target/H0)//2)*2) -- d2s_process_shape gives (h,w). */
int d2s_process_shape(int H0, int W0, int target_height, int* out_h, int* out_w);
int d2s_process(const uint8_t* bgr, int channels, int H0, int W0, int target_height, float* out, void* stream);

/* A1, the branches of the reference's NON-CUDA process() (depth.py:570-629; what a host without a CUDA/ROCm torch device runs):
 *  - tensor input (depth.py:576-601): the capture tensor is already RGB -- first three channels, no flip; target_height < H0:
 *    F.interpolate(bilinear, align_corners=False, antialias=False) to the even sizes of d2s_process_shape; else the frame as is.
 *    rgb: D2S_FMT_U8_HWC [H0,W0,channels] or D2S_FMT_U8_CHW / D2S_FMT_F32_CHW [channels,H0,W0]; out: float RGB CHW [3,h,w];
 *  - numpy input (depth.py:603-629): cv2.cvtColor(BGR(A) -> RGB), then cv2.resize(INTER_AREA) to
 *    (int(W0*target/H0), target) -- no even rounding; d2s_process_area_shape -- uint8 HWC in, uint8 RGB HWC out.  INTER_AREA is
 *    OpenCV's published box filter (resize.cpp: exact 2x2 / integer-factor averages, fractional cell weights otherwise). */
int d2s_process_rgb(const void* rgb, int fmt, int channels, int H0, int W0, int target_height, float* out, void* stream);
int d2s_process_area_shape(int H0, int W0, int target_height, int* out_h, int* out_w);
int d2s_process_area(const uint8_t* bgr, int channels, int H0, int W0, int target_height, uint8_t* out, void* stream);

/* A15: overlay_fps  (reference depth.py:2061-2103, glyphs depth.py:641-658): paints `text` (the reference's
 * "FPS: %.1f"; characters outside its 16-glyph table render as blanks) in green (0,255,0) with the 5x3 font scaled
 * by max(1,min(8,H//60)) at margin 2*scale, IN PLACE on one frame in any D2S_FMT_* layout. */
int d2s_overlay_text(void* rgb, int fmt, int H, int W, const char* text, void* stream);

/* A2-A4: ingest + _resize_patch_aligned_t + /255 + (x-mean)/std  (reference depth.py:676-706, 1916-1948).
 * pre->resample picks the branch of _resize_patch_aligned_t: D2S_RESAMPLE_BILINEAR = the CPU branch (strided decimation
 * by decim_stride = longest // (2*target), then bilinear align_corners=False), D2S_RESAMPLE_BICUBIC_AA = the IS_CUDA
 * branch (bicubic + antialias from the full frame; decim_stride is ignored).  pre->square: the fixed-square branch (depth.py:1937-1946):
 * plain bilinear of the full frame to (h, w), decim_stride and resample ignored.  pre == NULL: ImageNet mean / std, CPU branch.
 * frames: `batch` frames, format D2S_FMT_U8_HWC or D2S_FMT_U8_CHW or D2S_FMT_F32_CHW (0..255),
 * each H x W, contiguous.  out: float [batch,3,h,w] with (h,w) the engine shape. */
int d2s_preprocess(const void* frames, int fmt, int batch, int H, int W,
                   float* out, int h, int w, int decim_stride,
                   const d2s_pre_params* pre, void* stream);

/* A5-A9: model(pixel_values=x).predicted_depth  (reference depth.py:1763-1781 -> HF
 * DepthAnythingForDepthEstimation).  x: float [batch,3,h,w]; depth: float [batch,h,w]. */
int d2s_model_forward(d2s_engine* e, const float* x, float* depth, int batch, void* stream);

/* Several Video-Depth-Anything streams on one engine (d2s_version() >= 112).  A temporal engine finalised with max_batch = N owns
 * N stream slots 0 .. N-1: per slot one 32-frame window (the rings of projected k' | v' rows of the 8 attention blocks) and, inside
 * d2s_pipeline_streams, one EMA state.  max_batch = 1 is the single-stream engine.
 *   - One call carries batch <= N frames and a HOST array stream_ids[batch] of DISTINCT slot indices: batch row r is the next frame of
 *     stream stream_ids[r].  Only the named streams advance; the others are untouched, so streams may run at different frame
 *     rates, join and leave.  stream_ids == NULL means rows 0 .. batch-1 are streams 0 .. batch-1: d2s_model_forward / d2s_pipeline
 *     on a temporal engine are exactly that form.
 *   - A slot starts fresh: its first frame sees a window of one, then all 31 ring slots hold that frame's rows (the reference's
 *     update_cache, vda2_s.py:177-218).  d2s_engine_reset_stream_at makes ONE slot fresh again (window and EMA state);
 *     d2s_engine_reset_stream all of them.  Resetting, feeding or skipping stream i never changes what stream j computes.
 *   - Duplicate or out-of-range ids, batch > N, a reset of a slot that does not exist: an error status, d2s_last_error() says which,
 *     and nothing is launched.  On a non-temporal engine a non-NULL stream_ids is refused (its batch rows are not streams).
 *   - All rows share the engine's model-input shape.  One engine, one caller at a time (as for every entry point). */
int d2s_model_forward_streams(d2s_engine* e, const float* x, float* depth, int batch, const int* stream_ids, void* stream);
int d2s_engine_reset_stream_at(d2s_engine* e, int stream_id);

/* D2S_PREC_FP8 engines only: post-training calibration of the static per-tensor activation scales.  Runs one bf16
 * forward over x (float [batch,3,h,w], the engine's input layout) recording max |activation| at the four e4m3
 * quantisation sites of every encoder layer (LayerNorm-1 output, attention output, LayerNorm-2 output, GELU output),
 * sets scale = amax / 448 and switches the engine's encoder linears to e4m3 operands.  Synchronous.  Forward calls
 * before a successful calibration fail with D2S_E_STATE.  (No reference counterpart: the reference has FP16 only.) */
int d2s_engine_calibrate(d2s_engine* e, const float* x, int batch, void* stream);

/* What d2s_model_forward decides for one call, before anything is launched (d2s_version() >= 121; pure host code: launches nothing,
 * needs no GPU): an engine of `desc` created NOW (it reads D2S_NO_LNFUSE, D2S_TAPS, D2S_NO_OVERLAP, D2S_VDA_FUSE as d2s_engine_create /
 * d2s_engine_finalize do, and D2S_LNF_PP / D2S_GEMM_PP as every call does), finalised at (h, w) with max_batch = batch, running `batch`
 * frames.  flags: D2S_PLAN_*.  Refuses what d2s_engine_create and d2s_engine_finalize refuse of desc, h, w, batch and what the forward
 * pass refuses of an e4m3 engine that is not calibrated, in the same words.  The decisions that follow from a GEMM launch (statistics
 * slots, up-sample folds) depend on the CU count of the device: on a machine without a GPU the report is the 256-CU plan (MI355X).
 *   regimes      f8 / f8a: FC1 + FC2 / all four encoder linears on e4m3 operands; x3: bf16x3; lnf: LN1 / LN2 fold into QKV / FC1 and
 *                proj / FC2 produce their statistics; pp_fold: lnf on the ping-pong kernel (batched bf16); tap_fold: the final LayerNorm
 *                folds into the reassemble projections; use_side: neck branches on the side stream
 *   ln_slots     statistics partials per row left by proj [0] and FC2 [1] (0: not a producer)
 *   site         D2S_PLAN_SITE_* -> D2S_PLAN_FOLDED (a LayerNorm is folded into it) | D2S_PLAN_STATS (it produces the raw-residual
 *                copy and statistics of the LayerNorm behind it) | D2S_PLAN_E4M3 (e4m3 operands)
 *   tap_side     tap i's neck branch runs on the side stream (else on the caller's, after the encoder)
 *   head         head1_ups / head2_ups: the up-sample in front of conv1 / conv2 is folded into its loader; head2_fused: conv2 + conv3 in
 *                one launch, bn its column tile
 *   tm_*         temporal engines, per module (layer_3, layer_4, path_4, path_3): tm_slots / tm_folded [m][j]: the partials in front of
 *                and the folded form taken for kvq[0], kvq[1], ff1; tm_fold: the modules' producers run; tm_cache_store: a ring-store
 *                launch follows each attention for rows whose window is fresh (no D2S_PLAN_WINDOW_FILLED) or on unfolded engines
 *   geometry     what d2s_engine_finalize sizes the engine with: patch grid, tokens, the four neck maps, split-K / scratch elements,
 *                the temporal modules' channels and sites
 *   rcu_fused    the fusion stages (deep -> shallow) whose RCU2 + 1x1 projection, and the taps whose RCU1, are one launch (bf16,
 *                fusion width 128, maps whose 4 x 8-pixel tiles x batch fit the CUs; D2S_RCU_FUSE=0: none); and those that are one
 *                launch of the kernel's wide form (8 x 8-pixel tiles: a map the 4 x 8 tiles do not fit and the 8 x 8 tiles do)
 *   ln_launches  LayerNorm launches of the call (d2s_engine_profile_read's "layernorm" class) */
#define D2S_PLAN_CALIBRATING    1   /* the forward pass inside d2s_engine_calibrate */
#define D2S_PLAN_PROFILING      2   /* d2s_engine_profile is on */
#define D2S_PLAN_WINDOW_FILLED  4   /* temporal engine: every stream of the call has seen a frame */
#define D2S_PLAN_CALIBRATED     8   /* e4m3 engine: d2s_engine_calibrate has run */
enum { D2S_PLAN_SITE_PATCH = 0, D2S_PLAN_SITE_QKV0, D2S_PLAN_SITE_QKV, D2S_PLAN_SITE_PROJ, D2S_PLAN_SITE_FC1, D2S_PLAN_SITE_FC2,
       D2S_PLAN_SITE_FC2_LAST, D2S_PLAN_SITE_NECK0, D2S_PLAN_SITE_NECK1, D2S_PLAN_SITE_NECK2, D2S_PLAN_SITE_NECK3, D2S_PLAN_SITES };
enum { D2S_PLAN_FOLDED = 1, D2S_PLAN_STATS = 2, D2S_PLAN_E4M3 = 4 };
typedef struct d2s_forward_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_forward_plan_result) */
    int32_t f8, f8a, x3, lnf, pp_fold, tap_fold, use_side;
    int32_t ln_slots[2];
    int32_t site[D2S_PLAN_SITES];
    int32_t tap_side[4];
    int32_t head1_ups, head2_fused, head2_ups, bn;
    int32_t tm_fold, tm_cache_store, tm_slots[4][3], tm_folded[4][3];
    int32_t gh, gw, P, N, Npad, fH[4], fW[4], tm_C[4], tm_sites[4];
    int32_t ln_launches;
    int32_t rcu_fused;         /* d2s_version() >= 125 (the word was padding, zero before): bit idx = fusion stage idx runs its residual
                                  unit and projection as one launch; bit 8 + i = the RCU1 of tap i does.  d2s_version() >= 131: bit
                                  16 + idx / bit 24 + i = the same as one launch of the wide form (never set together with the former) */
    uint64_t splitk_elems, scr_elems;
} d2s_forward_plan_result;
int d2s_forward_plan(const d2s_model_desc* desc, int h, int w, int batch, int flags, d2s_forward_plan_result* res);

/* A10-A11: post_process_depth = normalize -> gamma -> foreground_scale -> anti_alias
 * (reference depth.py:806-814), in place on float [batch,h,w].  Stateless. */
int d2s_post_process(float* depth, int batch, int h, int w, const d2s_post_params* p,
                     void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t d2s_post_process_workspace(int batch, int h, int w);
/* The same, out of place (depth_out may equal depth_in; a PARTIAL overlap is rejected with D2S_E_INVALID): with distinct buffers and few frames the normalise / gamma / foreground
 * step and both blur passes run as one launch. */
int d2s_post_process_to(const float* depth_in, float* depth_out, int batch, int h, int w, const d2s_post_params* p,
                        void* workspace, uint64_t workspace_bytes, void* stream);
/* What d2s_post_process_to would launch for these arguments (d2s_version() >= 120; pure host code: launches nothing, needs no GPU);
 * in_place: depth_out == depth_in, i.e. d2s_post_process.  Three forms compute the same bits: FUSED = one launch ("post_fused<13>" /
 * "post_fused<0>": 13 taps at compile time, the default aa_strength 4, or a run-time count), TILE = "percentile_bounds<relative>" /
 * "percentile_bounds<metric>" + "shape_blur", ROWS = percentile_bounds + "shape_hblur<13|0>" + "vblur<13|0>".  k = taps (1: no
 * blur), r = k / 2; lds_bytes = each launch's dynamic LDS.  step, m, tail: the subsample of h * w pixels (every step-th, m of them)
 * and the rank of the lower bound in it -- for metric parameters the kernel derives its own from the number of valid pixels, which
 * depends on the data: the values here are the host's, for h * w valid pixels.  Refuses what d2s_post_process_to refuses of p. */
enum { D2S_POST_FORM_FUSED = 0, D2S_POST_FORM_TILE = 1, D2S_POST_FORM_ROWS = 2 };
typedef struct d2s_post_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_post_plan_result) */
    int32_t form, launches;    /* D2S_POST_FORM_*; 1 .. 3 */
    int32_t k, r;
    int32_t step, m, tail;
    uint32_t lds_bytes[3];
    char kernel[3][32];
} d2s_post_plan_result;
int d2s_post_plan(int batch, int h, int w, const d2s_post_params* p, int in_place, d2s_post_plan_result* res);

/* A12: DepthStabilizer.__call__ (reference depth.py:1865-1887).  state: float [h,w] owned by the
 * caller; *initialised == 0 -> state = depth (first frame), else state = lerp(state, depth, 1-alpha);
 * depth is overwritten with the returned value.  Frames are processed in order. */
int d2s_ema_update(float* depth, float* state, int initialised, int h, int w, float alpha,
                   void* stream);

/* A13: F.interpolate(depth, (H,W), bilinear, align_corners=False)  (reference depth.py:1999-2004).
 * in: float [batch,h,w] -> out: float [batch,H,W]. */
int d2s_upsample_depth(const float* in, int batch, int h, int w, float* out, int H, int W,
                       void* stream);

/* A14 (+A13 fused): make_sbs_core  (reference depth.py:2122-2184).
 * rgb: `batch` frames H x W in `rgb_fmt`; depth: float [batch,dh,dw] -- either full resolution
 * (dh==H, dw==W: exactly make_sbs_core) or model resolution (the bilinear align_corners=False
 * up-sample of predict_depth, depth.py:1999-2004, is fused into the warp).
 * out: `out_fmt` in {U8_HWC (round-half-even, saturate), F32_HWC, F32_CHW}; shape from d2s_sbs_shape. */
int d2s_make_sbs(const void* rgb, int rgb_fmt, const float* depth, int dh, int dw,
                 int batch, int H, int W, const d2s_sbs_params* p,
                 void* out, int out_fmt, void* stream);
/* output frame size of make_sbs_core for an H x W input (pad_to_aspect_tensor, depth.py:2106-2119) */
int d2s_sbs_shape(int H, int W, const d2s_sbs_params* p, int* out_h, int* out_w);
/* What d2s_make_sbs would launch for these arguments (d2s_version() >= 118; pure host code: launches nothing, needs no GPU).  The shape,
 * format and parameter arguments are d2s_make_sbs's; rgb_align / out_align stand for the two pointers: their alignment in bytes (any
 * positive integer with the pointer's residue modulo 4, e.g. 256 for an allocation, 1 for an odd address).  kernel is
 * "stereo_warp_generic<IN,OUT>" (IN, OUT in U8_HWC / U8_CHW / F32_CHW / F32_HWC) or "stereo_warp_gather<MODE,NC=3|4,DIRECT=0|1>" (MODE in
 * HALF_SBS / FULL_SBS / HALF_TAB / FULL_TAB); for the gather kernel rpw = source rows per wave (even for Half-TAB, never more than H),
 * ntx = 256-pixel column tiles, wpc = resident waves per CU the grid was cut for; grid = blocks of 256 threads. */
typedef struct d2s_warp_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_warp_plan_result) */
    int32_t gather, direct, nc;
    int32_t ntx, wpc, rpw;
    int32_t out_h, out_w;
    uint32_t grid;
    int64_t waves;
    char kernel[64];
} d2s_warp_plan_result;
int d2s_warp_plan(int rgb_fmt, int dh, int dw, int batch, int H, int W, const d2s_sbs_params* p, int out_fmt,
                  int rgb_align, int out_align, d2s_warp_plan_result* res);

/* f1: the GLSL DIBR warp with disocclusion in-painting the reference's Viewer / OpenXR modes render
 * (FRAGMENT_SHADER, viewer.py:386-631): rgb uint8 HWC [batch,H,W,3], depth float [batch,H,W] (full resolution, as
 * uploaded to tex_depth, viewer.py:2386, 2456) -> both eyes, each rendered into an H x W viewport (Half modes:
 * W/2 columns resp. H/2 rows per eye) and packed left|right (SBS) or left over right (TAB); three channels per pixel
 * (four with p->alpha_mode == D2S_DIBR_ALPHA_RGBA).  out_fmt: D2S_FMT_U8_HWC (round-half-even) or D2S_FMT_F32_HWC (0..255);
 * shape from d2s_dibr_shape.  Pinned by tests/golden/dibr.npz: the reference's shader run off-screen (make_golden_dibr.py). */
int d2s_dibr_shape(int H, int W, int display_mode, int* out_h, int* out_w);
int d2s_dibr_warp(const uint8_t* rgb, const float* depth, int batch, int H, int W, const d2s_dibr_params* p,
                  void* out, int out_fmt, void* stream);
/* d2s_dibr_warp with depth at ANY resolution, float [batch,dh,dw] -- typically the model's (d2s_version() >= 113).  The shader's
 * H x W depth texture is the bilinear up-sample d2s_upsample_depth(depth, dh, dw -> H, W) would store, evaluated inside the warp
 * kernel instead of being written to memory and read back: the output is BIT-IDENTICAL to d2s_upsample_depth + d2s_dibr_warp
 * (tests/test_gpu_view_pipeline.py).  dh == H && dw == W is exactly d2s_dibr_warp.  Shape from d2s_dibr_shape. */
int d2s_dibr_warp_depth(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                        const d2s_dibr_params* p, void* out, int out_fmt, void* stream);

/* The OpenXR viewer's automatic movie crop (d2s_version() >= 114), application half: the OpenXR screen shader is FRAGMENT_SHADER with
 * one line changed (xr_viewer/implementation.py:111-126): flipped_uv = u_source_crop.xy + screen_flipped_uv * u_source_crop.zw.
 * crop = (x, y, w, h) in uv of the source, top-left origin, as u_source_crop; the kernel sees (float) of each, as GL does.  The depth
 * taps, the 5 % edge fall-off (relative to the FULL source), the parallax shift, the in-painting and the border alpha follow the
 * cropped texture coordinate; the rounded-corner SDF and the feathering stay on the quad's uv / p->viewport.  Each eye is rendered
 * into the crop's pixel size (x1 - x0) x (y1 - y0) of _movie_crop_pixel_bounds (xr_viewer/crop.py:165-173; round() there is
 * half-to-even: nearbyint on doubles here), halved by the Half modes as d2s_dibr_shape halves the frame, so the texel : pixel ratio
 * stays 1; packed as d2s_dibr_warp packs.  Refused (nothing launched): a non-finite value; x, y < 0, w, h <= 0, x + w or y + h > 1
 * (1e-6 of slack); an eye viewport under 2 x 2 pixels; everything d2s_dibr_warp_depth refuses.  crop = (0, 0, 1, 1) is bit-identical
 * to d2s_dibr_warp_depth.  Pinned by tests/golden/xr_crop.npz: the reference's XR shader run off-screen (make_golden_xr_crop.py). */
int d2s_dibr_crop_shape(int H, int W, const double crop[4], int display_mode, int* out_h, int* out_w);
int d2s_dibr_warp_crop(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                       const d2s_dibr_params* p, const double crop[4], void* out, int out_fmt, void* stream);
/* What d2s_dibr_warp / d2s_dibr_warp_depth (crop == NULL) or d2s_dibr_warp_crop would launch for these arguments (d2s_version() >= 132;
 * pure host code: launches nothing, needs no GPU).  It runs the launcher's own code up to the launch -- the checks, the uniforms, the
 * eye shape, the D2S_DIBR_NO_ROLL0 / D2S_DIBR_NO_ROWS / D2S_DIBR_COLS switches and the window plan -- and refuses what the launcher
 * refuses of these arguments.  kernel: "dibr_rows<u8|f32,fx=0|1,256|512|1024,FullDep|UpDep[,crop]>" (the LDS-window row kernel, roll == 0)
 * or "dibr<u8|f32,roll0|general,FullDep|UpDep[,crop]>" (the gather kernel).  rows = 1: the row kernel; cols, margin, ww are the
 * window plan's (columns per block, reach in source texels, words per plane) -- with rows = 0 the window the row kernel would have
 * needed.  grid / block are the launch's; lds_*_bytes the row kernel's request (0 for the gather kernel), never above 65 536. */
typedef struct d2s_dibr_warp_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_dibr_warp_plan_result) */
    int32_t rows, cols, margin, ww;
    int32_t roll0, up, fx;     /* the row pair formed once per pixel or block; depth up-sampled in the kernel; feather / corner code */
    int32_t oh, ow, out_h, out_w;
    uint32_t grid[3], block;
    uint32_t lds_dynamic_bytes, lds_static_bytes;
    char kernel[64];
} d2s_dibr_warp_plan_result;
int d2s_dibr_warp_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double* crop /* NULL = uncropped */,
                       int out_fmt, d2s_dibr_warp_plan_result* res);

/* The OpenXR viewer's eye views (d2s_version() >= 115): the screen of d2s_xr_screen drawn into each eye's swapchain image with that
 * eye's own view-projection matrix, as EffectsMixin._render_eye does (xr_viewer/effects.py:1023-1137: depth test LESS against a
 * cleared buffer, blending off, the image cleared to the background first) -- the XR fragment shader of d2s_dibr_warp_crop run at the
 * uv the rasteriser interpolates.  The surface is one planar facet (flat) or the strip's 48 planar facets (curved); inside a facet
 * GL's perspective-correct interpolation is a homography from the pixel centre to uv, formed on the host in double precision.  A
 * pixel is covered when its centre lies inside a projected facet; where several cover it the smallest depth wins, ties to the lower
 * facet index; as in GL a fragment with NDC depth outside [-1, 1) is not drawn (near / far plane, the buffer cleared to 1), and the
 * facets of a strip share one edge function per seam, so no pixel inside the surface is left uncovered.  The outline itself (which
 * centres ON an edge count) is the rasteriser's fill rule and is not reproduced.
 *   p:     read as by d2s_dibr_warp_crop (pixel_size = 1 / source size unless res_w / res_h say otherwise; alpha_mode as everywhere)
 *          EXCEPT display_mode and viewport (not consulted), roll (screen->roll is u_roll) and feather_enabled, which must be 0: the
 *          XR viewer never enables the feathering.  The rounded-corner SDF runs on the surface's own uv, every texture coordinate
 *          on the cropped uv.  crop: u_source_crop, NULL = (0, 0, 1, 1).
 *   depth: float [batch, dh, dw] at any resolution, as d2s_dibr_warp_depth.
 *   Textures are plain GL_LINEAR + GL_REPEAT WITHOUT mipmaps, the colour texture's state whenever the reference's frost and glow modes
 *   are off (effects.py:590-614); mipmapped filtering is out of scope.
 *   out:   the eye images one after another, eye i at element offsets[i] of d2s_dibr_xr_shape: [batch][height_i][width_i][nch],
 *          nch = 3 (4 with D2S_DIBR_ALPHA_RGBA), uint8 (D2S_FMT_U8_HWC) or float 0..255 (D2S_FMT_F32_HWC).  offsets[0] = 0,
 *          offsets[i] = offsets[i-1] + batch * height_(i-1) * width_(i-1) * nch; *total = the element count of out.  An uncovered
 *          pixel is clear.rgb * 255 (alpha: clear.a).
 *   workspace: device, 16-byte aligned, >= d2s_dibr_xr_workspace bytes: the facet table (small set-up launches, one per eye for the flat
 *          screen and two for a curved one, write it in front of the render launch, which draws both eyes and the whole batch).
 * Refused with D2S_E_UNSUPPORTED, nothing launched: a vertex of the surface with clip w <= 1e-6 (the screen crosses the eye plane).
 * Refused with D2S_E_INVALID: a non-finite value; curve outside 0..2; width, height or distance <= 0; an eye image under 2 x 2 or
 * over 8192 on a side; eye outside 0..1; n_eyes outside 1..2; a bad struct_size; feather_enabled; a short or misaligned workspace;
 * everything d2s_dibr_warp_crop refuses.  Stream-ordered, no host synchronisation, no allocation; every argument is checked before
 * any HIP call.  Pinned by tests/golden/xr_eye.npz: the reference's shaders drawn off-screen (make_golden_xr_eye.py). */
int d2s_dibr_xr_shape(const d2s_xr_eye* eyes, int n_eyes, int batch, int alpha_mode, uint64_t* offsets /* [n_eyes] */, uint64_t* total);
int d2s_dibr_xr_workspace(int n_eyes, uint64_t* bytes);
int d2s_dibr_xr_eyes(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                     const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt,
                     void* workspace, uint64_t workspace_bytes, void* stream);

/* The colour mip chain of the OpenXR viewer's frame texture (d2s_version() >= 119): what glGenerateMipmap builds for the reference's
 * glow, frost and veil passes (xr_viewer/effects.py:597-646), restated from renders (tests/golden/xr_glow.npz).  Levels 1 .. q of an
 * H x W frame, q = floor(log2(max(H, W))): level k is max(1, floor(size of level k - 1 / 2)) per axis, and each of its texels is the
 * bilinear sample of the ALREADY 8-BIT level k - 1 at the texel's normalised centre -- source coordinate (i + 0.5) * n_(k-1) / n_k - 0.5,
 * clamped to the edge -- rounded half to even (where both sizes are even: the 2 x 2 box).  All-integer arithmetic: exact.
 *   d2s_mip_shape: *n_levels = q (<= 13); offsets[k-1], hs[k-1], ws[k-1] = level k's byte offset within one frame's chain and its size;
 *                  *total_bytes = one frame's chain.  Host only.
 *   d2s_mip_chain: rgb uint8 [batch, H, W, 3] -> levels uint8 [batch, total_bytes], each level RGB HWC, one after another.  The
 *                  reference regenerates its mipmaps every _glow_mipmap_interval frames only; the caller decides when to call this.
 * H, W in 2 .. 8192, batch in 1 .. 65535, else D2S_E_INVALID.  Stream-ordered, no host synchronisation, no allocation; every argument
 * is checked before any HIP call. */
int d2s_mip_shape(int H, int W, int* n_levels, uint64_t* offsets /* [<= 14] */, int* hs, int* ws, uint64_t* total_bytes);
int d2s_mip_chain(const uint8_t* rgb, int batch, int H, int W, uint8_t* levels, void* stream);

/* The OpenXR viewer's "Default with Glow" looks around the FLAT screen (d2s_version() >= 119): d2s_dibr_xr_eyes with the two blended
 * passes of EffectsMixin._render_glow (xr_viewer/effects.py:476-585, shader _GLOW_FRAG xr_viewer/glsl.py:580-666) in the same launch,
 * in _render_eye's order (effects.py:1050-1145): clear; the outer band, premultiplied-blended over the clear colour (rgb and alpha:
 * src + dst * (1 - src.a); depth test off; drawn where the plane point has clip w > 0 and NDC z in [-1, 1]); the screen, exactly as
 * d2s_dibr_xr_eyes draws it (blending off: its rgba overwrites, rounded corners included); mode 1 only: the inner band blended over the
 * screen.  All of it in float, quantised once at the store; alpha_mode then acts on that (rgb, a) as it does without glow.
 *   The glow quad is the screen's plane, screen + range_m on every side, so the screen facet's homography evaluated without its
 *   0..1 bound gives the glow's uv; glow_w, glow_h, inner_w, inner_h, uv_glow_range and inner_uv are formed on the host in double
 *   precision as _render_glow:486-495 forms them.  u_glow_alpha_cap = 1, u_glow_use_source = 1 (u_glow_color is not read);
 *   _glow_intensity only gates the draw: mode 0 is the caller's "off".
 *   mode:  0 off, 1 glow, 2 glow2 (range_m halved, as the reference halves it; no inner band).
 *   range_m: what _glow_range_m returns (xr.glow_range_m).  inner_edge_fraction: _glow_inner_edge_fraction (0.075).
 *   levels: d2s_mip_chain's output for the same frames.  textureLod: LOD clamped to [0, q], trilinear between floor(lod) and the next
 *   level, bilinear within a level, CLAMP_TO_EDGE (xr_viewer/frame.py:39-40).  The glow reads LOD 7 .. 10 only.
 *   NOT reproduced: with glow on the reference also gives the colour texture LINEAR_MIPMAP_LINEAR (frame.py:34, effects.py:601-608),
 *   so ITS screen pass is trilinear where the screen is minified.  That filter needs implicit derivatives and is driver-dependent; the
 *   screen pass here stays GL_LINEAR, as d2s_dibr_xr_eyes has it.  The flat screen's veil and frosted looks: d2s_dibr_xr_eyes_frost
 *   below; the border stays with the caller.
 * Refused, nothing launched, out untouched: D2S_E_UNSUPPORTED: screen->curve != 0 with mode != 0 (the curved glow is a band mesh of
 * ~500 quads, _build_curved_glow_band_verts: d2s_dibr_xr_eyes_glow_curved below draws it).  D2S_E_INVALID: normal_offset != 0 with mode != 0 (the reference offsets the screen only
 * under a room model, which switches the planar glow off); range_m <= 0 or non-finite; inner_edge_fraction < 0 or non-finite; mode
 * outside 0..2; a bad struct_size; levels NULL with mode != 0; everything d2s_dibr_xr_eyes refuses.  glow == NULL or mode 0 is
 * bit-identical to d2s_dibr_xr_eyes (the same kernel). */
typedef struct d2s_xr_glow {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_glow) = 24 */
    int32_t  mode;             /* 0 off, 1 glow, 2 glow2 */
    double   range_m;
    double   inner_edge_fraction;
} d2s_xr_glow;
int d2s_dibr_xr_eyes_glow(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                          const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt,
                          void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels, void* stream);

/* The glow around the CURVED screen (d2s_version() >= 122): d2s_dibr_xr_eyes_glow's argument list; screen->curve 1 or 2 with mode 1 or 2
 * draws what EffectsMixin._render_curved_glow draws (xr_viewer/effects.py:408-474; mesh _build_curved_glow_band_verts, effects.py:314-406;
 * program _CURVED_VERT + _GLOW_FRAG, xr_viewer/glsl.py:580-666) in _render_eye's order (effects.py:1050-1145): clear; the mesh's outer
 * vertices blended over it; the curved strip exactly as d2s_dibr_xr_eyes draws it (a screen pixel has that call's facet and uv); mode 1:
 * the mesh's inner vertices blended over the screen.  Blending, quantisation and alpha_mode as d2s_dibr_xr_eyes_glow; glow_w .. inner_uv
 * as _render_curved_glow:414-423 forms them.
 *   The mesh is restated as planar pieces, formed on the host in double precision and rounded to float32 once: the strip's 48 facets,
 *   each continued without bound across the strip; the two tangent planes at the arc's ends (_local_axes at -+0.48 rad); mode 1: the two
 *   chord planes of the inner band at the arc's ends (one quad along the strip each).  The inner bands that run ALONG the strip are drawn
 *   on the facets (a horizontal curve's lie on them; a vertical curve's are 48 chords of the arc that do not start at a facet seam and
 *   lie within radius * (1 - cos(0.01)) = 5e-5 radius of the facets).  A pixel finds its one piece by a search over the 49 seam lines.
 *   workspace: device, 16-byte aligned, >= d2s_dibr_xr_glow_curved_workspace(n_eyes) bytes (52 rows of 96 bytes per eye), written by
 *   set-up launches whose arguments carry the rows: no host copy, no allocation, stream-ordered.
 * A flat screen, glow == NULL or mode 0: d2s_dibr_xr_eyes_glow, bit-identical (the same kernel; the larger workspace is still required
 * of a curved screen only).  Refused, nothing launched, out untouched: everything d2s_dibr_xr_eyes_glow refuses apart from the
 * curvature; D2S_E_INVALID: normal_offset != 0; D2S_E_UNSUPPORTED: an eye (the null space of vp's x, y and w rows) that does not lie
 * on the inner side of all 50 outer piece planes by 1e-4 of the arc's radius -- a viewer behind the screen or beyond an end of the arc.
 * There translucent pieces overlap and would have to be blended in draw order: an ordered multi-hit kernel, not built.  Also
 * D2S_E_UNSUPPORTED: a frame of 8192 x 8192 (its coarse levels and the piece table exceed 64 KB of LDS).  The curved screen's frost and
 * veil (_build_curved_frost_verts): d2s_dibr_xr_eyes_frost_curved below.  The border and the trilinear screen pass stay with the caller. */
int d2s_dibr_xr_glow_curved_workspace(int n_eyes, uint64_t* bytes);
int d2s_dibr_xr_eyes_glow_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                 const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                 int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels,
                                 void* stream);

/* What the three eye-view calls above decide for these arguments, before they look at a device pointer (d2s_version() >= 123; pure host
 * code: launches nothing, needs no GPU).  entry: the call that asks -- D2S_XR_ENTRY_EYES takes no glow (glow must be NULL here),
 * D2S_XR_ENTRY_GLOW refuses a curved screen with glow on, D2S_XR_ENTRY_GLOW_CURVED draws it.  Refuses exactly what that call refuses
 * before it looks at rgb, depth, out, workspace or levels, with the same code and the same d2s_last_error text; those pointers are
 * the call's last checks (workspace NULL, misaligned, short; levels NULL with glow on; rgb, depth, out NULL).
 *   kind: the kernel that draws -- PLAIN (no glow, or mode 0), GLOW (flat screen), GLOW_CURVED.
 *   rows_per_eye: table rows written per eye -- 1 (flat), 48 (curved), 52 (GLOW_CURVED); setup_launches: the launches that write them,
 *   all eyes' (24 rows travel in one launch's arguments: per eye 1, 2 or 3).
 *   grid: the render launch, 16 x 16 pixel blocks of 256 threads: (ceil(max width / 16), ceil(max height / 16), n_eyes * batch).
 *   lds_dynamic_bytes: the chain's levels min(7, q) .. q as float RGB, 12 bytes a texel (0 for PLAIN); lds_static_bytes: the kernel's own.
 *   workspace_bytes: d2s_dibr_xr_workspace's answer, GLOW_CURVED: d2s_dibr_xr_glow_curved_workspace's.
 *   out_elems, offsets: d2s_dibr_xr_shape's total and offsets.
 * D2S_E_INVALID also: res NULL, a bad res->struct_size, entry outside 0..2, a glow with D2S_XR_ENTRY_EYES. */
enum { D2S_XR_ENTRY_EYES = 0, D2S_XR_ENTRY_GLOW = 1, D2S_XR_ENTRY_GLOW_CURVED = 2 };
enum { D2S_XR_KIND_PLAIN = 0, D2S_XR_KIND_GLOW = 1, D2S_XR_KIND_GLOW_CURVED = 2 };
typedef struct d2s_xr_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_plan_result) */
    int32_t  kind;             /* D2S_XR_KIND_* */
    int32_t  rows_per_eye;
    int32_t  setup_launches;
    uint32_t grid[3];
    uint32_t lds_dynamic_bytes;
    uint32_t lds_static_bytes;
    uint32_t reserved;
    uint64_t workspace_bytes;
    uint64_t out_elems;
    uint64_t offsets[2];
} d2s_xr_plan_result;
int d2s_dibr_xr_plan(int entry, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                     const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_glow* glow,
                     d2s_xr_plan_result* res);

/* The OpenXR viewer's "veil" and "frosted" looks around the FLAT screen (d2s_version() >= 124): d2s_dibr_xr_eyes followed, in the same
 * launch, by the four "beam" walls of EffectsMixin._render_flat_frost_with_uniforms (xr_viewer/effects.py:789-817; mesh
 * _build_flat_frost_verts, effects.py:145-187; layout _frost_front_layout, effects.py:102-132; programs _FROST_GLOW_VERT with
 * _FROST_VEIL_FRAG or _FROST_GLOW_FRAG, xr_viewer/glsl.py:668-791) in _render_eye's order (effects.py:1023-1145): clear; the screen
 * (depth test LESS, blending off); then the walls top, bottom, left, right with the depth test OFF, each blended
 * src + dst * (1 - src.a) on rgb and alpha -- over the clear colour, over the screen and over each other, wherever a wall's plane point
 * lies inside the wall, has clip w > 0 and NDC z in [-1, 1] (the walls run past the eye: the near plane cuts them).  All of it in
 * float, quantised once at the store; alpha_mode then acts on that (rgb, a) as it does in d2s_dibr_xr_eyes_glow.
 *   A wall runs from a screen edge (t = 0) to the matching edge of the front rectangle (t = 1): front_depth, front_half_w and
 *   front_half_h are formed on the host in double precision from the screen and head[] as _frost_front_layout forms them (without its
 *   rounded cache keys), the model matrix as _screen_effect_model(width, height, z_scale = front_depth).  v_local.z is t; v_uv follows
 *   the MESH: an 8 x 8 grid of cells per wall, two triangles a cell, the screen-border uv interpolated over each triangle.
 *   textureLod as d2s_dibr_xr_eyes_glow has it: LOD clamped to [0, q], trilinear between floor(lod) and the next level, bilinear
 *   within a level, CLAMP_TO_EDGE; level 0 is the frame itself.  The veil reads level 0 only and never looks at levels (NULL is fine);
 *   frosted needs levels = d2s_mip_chain's output for the same frames.
 * frost == NULL, mode 0, intensity <= 0, or veil with alpha <= 0.002 (the reference's early returns, effects.py:822-857): a plain draw
 * of the screen, bit-identical to d2s_dibr_xr_eyes (the same kernel, d2s_dibr_xr_workspace's bytes suffice).  Otherwise workspace >=
 * d2s_dibr_xr_frost_workspace bytes (the screen's rows and four wall rows per eye).
 * Refused, nothing launched, out untouched: D2S_E_UNSUPPORTED: a curved screen with frost on (the curved frost is a mesh of its own,
 * _build_curved_frost_verts, 588 vertices: not built).  D2S_E_INVALID: normal_offset != 0 with frost on; a bad struct_size; mode
 * outside 0..2; a non-finite field; noise_scale or lod negative; frosted with levels NULL; everything d2s_dibr_xr_eyes refuses.  The
 * border and the curved frost stay with the caller. */
typedef struct d2s_xr_frost {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_frost) = 120 */
    int32_t  mode;             /* 0 off, 1 veil, 2 frosted (_active_glow_mode, effects.py:43-59) */
    double   head[3];          /* _head_pos_w, world space (effects.py:105-125); the reference's default: the origin */
    double   intensity;        /* u_intensity, ALREADY multiplied: _frost_veil_intensity (1.5) or _frost_glow_intensity (1.0) times
                                  max(_glow_intensity_multiplier, 0) (effects.py:839-840, 823-824) */
    double   alpha;            /* u_frost_alpha: _frost_veil_alpha 1.0 (effects.py:701) | _frost_glow_alpha 0.42 (effects.py:662) */
    double   edge_inset;       /* u_edge_inset: 0.02 (effects.py:699) | _frost_glow_inset 0.045 (effects.py:658) */
    double   beam_softness;    /* u_beam_softness: 0.34 (effects.py:702 | 652) */
    double   beam_thickness;   /* u_beam_thickness: 3.0 (effects.py:703) | _frost_glow_thickness 1.6 (effects.py:666) */
    /* frosted only (the veil's program has none of them) */
    double   lod;              /* u_lod: _frost_glow_lod 5.4 (effects.py:659) */
    double   threshold;        /* u_threshold: _frost_glow_threshold 0.46 (effects.py:660) */
    double   noise_scale;      /* u_noise_scale: _frost_glow_noise_scale 54 (effects.py:663) */
    double   blend;            /* u_frost_blend: _frost_glow_blend 1.35 (effects.py:665) */
    double   diffuse;          /* u_diffuse_scatter: _frost_glow_diffuse 0.85 (effects.py:667) */
    double   time;             /* u_time: _frame_now, seconds (effects.py:669); the noise cells drift with it */
} d2s_xr_frost;
enum { D2S_XR_KIND_FROST = 3 };          /* d2s_xr_plan_result.kind of d2s_dibr_xr_frost_plan */
int d2s_dibr_xr_frost_workspace(int n_eyes, uint64_t* bytes);
int d2s_dibr_xr_eyes_frost(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                           const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out, int out_fmt,
                           void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels, void* stream);
/* d2s_dibr_xr_plan for d2s_dibr_xr_eyes_frost: the same host plan through a second door (d2s_dibr_xr_plan itself knows entries 0..2
 * only).  kind: PLAIN or FROST; FROST: rows_per_eye 5 (the screen's row, then the four walls in draw order), one set-up launch per
 * eye, no LDS, workspace_bytes = d2s_dibr_xr_frost_workspace's. */
int d2s_dibr_xr_frost_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                           const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_frost* frost,
                           d2s_xr_plan_result* res);

/* The veil and frosted looks around the CURVED screen (d2s_version() >= 126): d2s_dibr_xr_eyes_frost's argument list; screen->curve 1 or
 * 2 with a look that draws runs what EffectsMixin._render_curved_frost_with_uniforms draws (xr_viewer/effects.py:759-787; mesh
 * _build_curved_frost_verts, effects.py:189-254; program _FROST_CURVED_VERT, xr_viewer/glsl.py:683-696, with the flat look's fragment
 * programs) in _render_eye's order: clear; the curved strip exactly as d2s_dibr_xr_eyes draws it; then ONE draw of 588 vertices, 196
 * triangles, with the depth test off, every covering triangle blended src + dst * (1 - src.a) in draw order -- two long walls of 48
 * quads along the arc's curved edges (horizontal: top, then bottom; vertical: u = 0, then u = 1), then one quad at each end of the arc,
 * each from two strip vertices (t = 0) to their points on the front rectangle of _frost_front_layout (t = 1).  A long wall's quad is
 * not planar, so the unit is the triangle: v_uv = (u, 1 - v) and t are affine over it, interpolated perspective-correctly; a triangle
 * is drawn where its plane point has clip w > 0 and NDC z in [-1, 1].  Consecutive triangles of a wall share one float32 edge function,
 * so no pixel along an interior edge is drawn twice or not at all; between two different walls nothing of the kind is done.  An eye
 * may be anywhere, outside the tube the walls form included: what overlaps is blended in draw order.
 *   The triangles' rows follow the strip's 48 in the table: 244 rows of 96 bytes per eye, d2s_dibr_xr_frost_curved_workspace bytes,
 *   written by 11 set-up launches per eye.  A block of the render launch draws 64 x 64 pixels: it first keeps, as four 64-bit masks in
 *   LDS, the rows that can cover a pixel of that square grown by one pixel, and its pixels walk those alone.  The environment variable
 *   D2S_XR_BIN=0, read at the call, makes every pixel walk all 244 rows: the same output bit for bit, for checks and timing.
 * A flat screen: d2s_dibr_xr_eyes_frost, bit-identical.  A look that does not draw (frost NULL, mode 0, intensity <= 0, a veil with
 * alpha <= 0.002): d2s_dibr_xr_eyes on the curved screen, bit-identical.  Refused, nothing launched, out untouched: everything
 * d2s_dibr_xr_eyes_frost refuses apart from the curvature; D2S_E_INVALID: normal_offset != 0 with frost on; D2S_E_UNSUPPORTED: a
 * vertex of the SCREEN with clip w <= 1e-6 (the walls' vertices may lie behind the eye); then the pointers, workspace (below
 * d2s_dibr_xr_frost_curved_workspace) and levels for frosted.  The border and the trilinear screen pass stay with the caller.
 * d2s_dibr_xr_frost_curved_plan: d2s_dibr_xr_frost_plan for this entry -- kind PLAIN, FROST or FROST_CURVED; FROST_CURVED: rows_per_eye
 * 244, setup_launches 11 per eye, grid (ceil(max width / 64), ceil(max height / 64), n_eyes * batch), lds_static_bytes 32. */
enum { D2S_XR_KIND_FROST_CURVED = 4 };
int d2s_dibr_xr_frost_curved_workspace(int n_eyes, uint64_t* bytes);
int d2s_dibr_xr_eyes_frost_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                                  const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                                  int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                  void* stream);
int d2s_dibr_xr_frost_curved_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                  const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_frost* frost,
                                  d2s_xr_plan_result* res);

/* The panorama background behind the screen (d2s_version() >= 127): what EffectsMixin._render_panorama_background draws into an eye
 * image before everything else (xr_viewer/effects.py:930-1021, shader _PANORAMA_FRAG, xr_viewer/glsl.py:57-94).  Every pixel no screen
 * facet covers starts from the panorama instead of screen->clear; the outer glow band and the walls then blend over it, alpha_mode
 * acts, one store -- d2s_dibr_xr_eyes' own tail.  Covered pixels do not change at all.  Per uncovered pixel, in float:
 *   dir = ray[eye] . (ndc.x, ndc.y, 1), the pixel's world direction (the reference's inv_view_rot . normalize((inv_proj . (ndc, 1, 1)).xyz
 *   / max(|w|, 1e-6)); for the viewer's frustum projections w does not depend on the pixel, so this is one 3 x 3 matrix per eye);
 *   u = atan(dir.x, -dir.z) / 2 pi + 0.5 + yaw_offset;  v = 0.5 - asin(dir.y / |dir|) / pi;  flip_y: v = 1 - v;
 *   the coordinate sampled AND differenced is (fract(u), clamp(v, 0, 1));
 *   texture(): LINEAR_MIPMAP_LINEAR / LINEAR, REPEAT in s with the level's own width, CLAMP_TO_EDGE in t, level 0 = pano_rgb, levels
 *   1 .. q = pano_levels.  The implicit LOD is ONE per 2 x 2 quad of GL window pixels, quads aligned to even window x and y counted from
 *   the bottom-left (row y of out is window row height - 1 - y), from the forward differences of the quad's lower-left pixel:
 *   rho = max(|(du * width, dv * height)| over x + 1, the same over window y + 1), lambda = clamp(log2 rho, 0, q); the three points are
 *   evaluated analytically also outside the image and under the screen.  Where fract(u) wraps inside a quad the difference is about 1
 *   and the quad takes the coarsest levels: a seam two pixels wide, which the reference's render shows too.
 *   background = (rgb * max(exposure, 0), 1) clamped to 0..255; the 8-bit framebuffer's quantisation before the blends is not
 *   reproduced, as everywhere in these calls.
 * Arguments: d2s_dibr_xr_eyes_frost's, then glow (d2s_dibr_xr_eyes_glow's; `levels` serves whichever look is on -- at most one of glow
 * and frost may be), pano, pano_rgb = device uint8 [height, width, 3], ONE image for the whole batch, row 0 = v 0 = up, and
 * pano_levels = d2s_mip_chain(pano_rgb, 1, height, width).  Kinds drawn with a panorama: PLAIN on a flat or curved screen, GLOW and
 * FROST (veil and frosted) on a flat one.  D2S_E_UNSUPPORTED, nothing launched: a CURVED screen with glow or frost on and a panorama --
 * those two kernels are the heaviest of the family and get the background in a change of their own.  pano == NULL: the call launches
 * the kernel d2s_dibr_xr_eyes / _glow / _glow_curved / _frost / _frost_curved launches for these arguments, bit-identical, and asks
 * that call's workspace.  D2S_E_INVALID: a bad struct_size; flip_y outside 0..1; height or width outside 2 .. 8192; a non-finite
 * field; a ray matrix of an eye in use that is all zero; pano_rgb or pano_levels NULL with pano set; glow and frost both on; everything
 * the underlying call refuses.  A negative exposure is 0, as the reference clamps it.  A refused call leaves out untouched.
 * d2s_dibr_xr_panorama_plan: d2s_dibr_xr_frost_plan for this entry (host code, no GPU): the same refusals bar the device pointers;
 * kind PLAIN, GLOW, GLOW_CURVED, FROST or FROST_CURVED; reserved = 1 when the panorama is drawn.
 * Pinned by tests/golden/xr_panorama.npz: the reference's shader drawn off-screen (make_golden_xr_panorama.py). */
typedef struct d2s_xr_panorama {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_panorama) = 176 */
    int32_t  flip_y;           /* u_flip_y: the panorama settings' flip_y, 0 or 1 (NOT the eye's) */
    int32_t  height, width;    /* the panorama, 2 .. 8192 each */
    double   yaw_offset;       /* u_yaw_offset in turns: yaw_offset_deg / 360 */
    double   exposure;         /* u_exposure; negative is 0 */
    double   ray[2][9];        /* per entry of eyes[]: row-major 3 x 3, NDC (x, y, 1) -> un-normalised world direction */
} d2s_xr_panorama;
int d2s_dibr_xr_eyes_panorama(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p,
                              const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, void* out,
                              int out_fmt, void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                              const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb, const uint8_t* pano_levels,
                              void* stream);
int d2s_dibr_xr_panorama_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                              const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt, const d2s_xr_frost* frost,
                              const d2s_xr_glow* glow, const d2s_xr_panorama* pano, d2s_xr_plan_result* res);

/* The panorama behind EVERY look, the curved screen's glow, glow2, veil and frosted included (d2s_version() >= 129): the door to what
 * d2s_dibr_xr_eyes_panorama refuses.  d2s_dibr_xr_eyes_panorama's arguments, its per-pixel rule (the same sampler, the same 2 x 2 quad
 * LOD evaluated analytically per thread) and its workspace (d2s_dibr_xr_frost_curved_workspace, the largest table, serves every kind).
 * Drawn with a panorama: kinds PLAIN, GLOW, FROST as there, and GLOW_CURVED (_render_curved_glow's band mesh, effects.py:314-474) and
 * FROST_CURVED (the 196 wall triangles, effects.py:189-254, 759-787): an uncovered pixel starts from the panorama, the outer band or the
 * walls blend over it in draw order, alpha_mode acts, one store.  Covered pixels are d2s_dibr_xr_eyes_glow_curved's /
 * d2s_dibr_xr_eyes_frost_curved's, bit for bit.  Bit-identity: a flat screen (any look) or a curved one without a look launches exactly
 * what d2s_dibr_xr_eyes_panorama launches; pano == NULL launches exactly what d2s_dibr_xr_eyes / _glow / _glow_curved / _frost /
 * _frost_curved launch for these arguments.  Refused, with the words of the entry that owns the check, nothing launched, out untouched:
 * everything d2s_dibr_xr_eyes_panorama refuses except the curved looks with a panorama -- D2S_E_UNSUPPORTED: an eye outside the convex
 * region the curved screen and its tangent planes bound with the glow on (the draw-order case), a screen vertex with clip w <= 1e-6, an
 * 8192 x 8192 frame's LDS; D2S_E_INVALID: normal_offset != 0 with a look on, a bad struct_size anywhere, glow and frost both on, the
 * panorama's own fields, a missing pointer or workspace.  d2s_dibr_xr_eyes_panorama itself is unchanged and keeps refusing.
 * d2s_dibr_xr_panorama_curved_plan: d2s_dibr_xr_panorama_plan for this entry (host code, no GPU): kind GLOW_CURVED or FROST_CURVED
 * where those draw; reserved = 1 when the panorama is drawn.
 * Pinned by tests/golden/xr_panorama_curved.npz: the reference's own shaders drawn off-screen in _render_eye's order, clear, panorama
 * quad, then the curved glow's or the curved frost's draws (make_golden_xr_panorama_curved.py). */
int d2s_dibr_xr_eyes_panorama_curved(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                                     const d2s_dibr_params* p, const double crop[4], const d2s_xr_screen* screen, const d2s_xr_eye* eyes,
                                     int n_eyes, void* out, int out_fmt, void* workspace, uint64_t workspace_bytes,
                                     const d2s_xr_frost* frost, const uint8_t* levels, const d2s_xr_glow* glow, const d2s_xr_panorama* pano,
                                     const uint8_t* pano_rgb, const uint8_t* pano_levels, void* stream);
int d2s_dibr_xr_panorama_curved_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, const double crop[4],
                                     const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int out_fmt,
                                     const d2s_xr_frost* frost, const d2s_xr_glow* glow, const d2s_xr_panorama* pano,
                                     d2s_xr_plan_result* res);

/* The world-space panels of the eye image (d2s_version() >= 133): what EffectsMixin._render_eye (xr_viewer/effects.py:1023-1225) draws
 * after the screen and its look as the unit quad (+-1, +-1, 0, 1) under an affine model matrix -- the FPS / status panel
 * (_render_fps_overlay, xr_viewer/overlay.py:81-249), the eight OSDs (effects.py:1157-1187), the calibration and help panels, the
 * keyboard with its border and key highlights (_render_keyboard, overlay.py:1427-1510) and the thin laser quads.  Textured panels are
 * _WORLD_VERT + _OVERLAY_FRAG (xr_viewer/glsl.py:3-13, 28-40: the RGBA texture at uv, alpha times u_alpha), solid ones _SOLID_VERT +
 * _SOLID_FRAG (glsl.py:97-112: one colour).  The rainbow beams, the hit circles and the controller meshes are not drawn.
 * One stream-ordered pass IN PLACE over the eye images any of the seven eye-view entries wrote into `out` (the layout of
 * d2s_dibr_xr_shape for these eyes, batch and alpha_mode), with the same screen and eyes.  Per pixel: z starts at the screen's own
 * depth there (the entries' cover rule over the screen's facets, normal_offset included; 1.0 where the screen does not cover: the
 * reference's depth buffer when its first panel is drawn, rounded corners included, since the XR fragment shader never discards);
 * then the panels in array order: covered where the panel's own coordinates a, b are in 0..1 with clip w > 0 and NDC z in [-1, 1];
 * GL_LESS against z with D2S_XR_PANEL_DEPTH_TEST; the colour is color[] or the bilinear RGBA sample at uv = (a, b) (GL_LINEAR, no mip
 * levels) with alpha times `alpha`; with D2S_XR_PANEL_BLEND it is blended SRC_ALPHA, ONE_MINUS_SRC_ALPHA, which GL applies to alpha
 * too (a = s * s + (1 - s) * d), else it overwrites; with D2S_XR_PANEL_DEPTH_WRITE and D2S_XR_PANEL_DEPTH_TEST z becomes the panel's depth (GL writes depth only under
 * an enabled depth test).  The destination is
 * read once and stored once; a pixel no panel passes is not written.  Only the 16 x 16 tiles some panel's pixel box touches run.
 * A panel with every vertex behind the eye (clip w <= 1e-6) is skipped; with no panel on any image nothing is launched.
 * textures[i].rgba: device, uint8 [height][width][4], row 0 = the TOP row of the picture (the reference uploads np.flipud of it,
 * overlay.py:191: GL's v = 1 is this row 0; this is the one place the flip is stated).  wrap: the GL wrap mode of the bilinear taps at
 * a panel's edge -- D2S_XR_WRAP_REPEAT is moderngl's default, which the reference never changes.
 * Refused, nothing launched, out untouched -- D2S_E_INVALID: a null pointer, a bad struct_size, n_panels outside 0 .. 32, n_textures
 * outside 0 .. 32, a texture index outside -1 .. n_textures - 1, a texture outside 1 .. 8192 on a side, a model matrix that is not
 * finite or not affine (last row 0 0 0 1), alpha or color not finite, unknown flags, a bad alpha_mode or out_fmt, a workspace that is
 * missing, misaligned or below d2s_dibr_xr_panels_workspace, and what the entries refuse about the screen and the eyes;
 * D2S_E_UNSUPPORTED: D2S_DIBR_ALPHA_PREMULTIPLIED (the destination's own alpha is gone: the reference's result cannot be formed), a
 * panel that crosses the eye plane (a vertex with clip w <= 1e-6, but not all four), a screen vertex with clip w <= 1e-6.
 * d2s_dibr_xr_panels_plan: what the call decides, host code, no GPU, the same refusals in the same words.
 * Pinned by tests/golden/xr_panels.npz: the reference's own shaders and its own _render_fps_overlay / _render_keyboard state drawn
 * off-screen into an RGBA8 + DEPTH24 target (tests/golden/make_golden_xr_panels.py). */
enum { D2S_XR_PANEL_DEPTH_TEST = 1, D2S_XR_PANEL_DEPTH_WRITE = 2, D2S_XR_PANEL_BLEND = 4 };
enum { D2S_XR_WRAP_REPEAT = 0, D2S_XR_WRAP_CLAMP = 1 };
enum { D2S_XR_MAX_PANELS = 32 };
typedef struct d2s_xr_panel {
    double   model[16];        /* row-major as numpy writes it: the quad's corners are model @ (+-1, +-1, 0, 1) */
    int32_t  texture;          /* index into textures[], or -1: the solid colour */
    uint32_t flags;            /* D2S_XR_PANEL_* */
    float    color[4];         /* u_color of a solid panel (r, g, b in 0..1, a) */
    float    alpha;            /* u_alpha of a textured panel */
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_panel) = 160 */
} d2s_xr_panel;
typedef struct d2s_xr_texture {
    const uint8_t* rgba;       /* device, [height][width][4], row 0 = the top row */
    int32_t  width, height;
    int32_t  wrap;             /* D2S_XR_WRAP_* */
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_texture) = 24 */
} d2s_xr_texture;
typedef struct d2s_xr_panels_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_xr_panels_plan_result) = 104 */
    int32_t  rows_per_eye;     /* table rows written per eye: the screen's facets (1 | 48), then one per panel */
    int32_t  setup_launches;   /* all eyes'; 0 when nothing is drawn */
    int32_t  render_launches;  /* 1, or 0: no panel on any image */
    int32_t  drawn[2];         /* per eye: panels with a pixel box on the image */
    int32_t  tile0[2][2];      /* per eye: the first tile (x, y) of the tiles the boxes touch */
    int32_t  tiles[2][2];      /* per eye: how many tiles across and down (0, 0: none) */
    uint32_t grid[3];          /* the render launch: the larger of the eyes' tile counts, n_eyes * batch */
    uint32_t reserved;
    uint64_t workspace_bytes;
    uint64_t out_elems;        /* d2s_dibr_xr_shape's total */
    uint64_t offsets[2];
} d2s_xr_panels_plan_result;
int d2s_dibr_xr_panels_workspace(int n_eyes, uint64_t* bytes);
int d2s_dibr_xr_panels(void* out, int out_fmt, int batch, int alpha_mode, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes,
                       const d2s_xr_panel* panels, int n_panels, const d2s_xr_texture* textures, int n_textures, void* workspace,
                       uint64_t workspace_bytes, void* stream);
int d2s_dibr_xr_panels_plan(int out_fmt, int batch, int alpha_mode, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes,
                            const d2s_xr_panel* panels, int n_panels, const d2s_xr_texture* textures, int n_textures,
                            d2s_xr_panels_plan_result* res);

/* Detection half (d2s_version() >= 114): the six numbers of the reference's tensor path (xr_viewer/crop.py:368-435,
 * _detect_movie_letterbox_crop; sample plan :298-353) for `batch` frames in TWO launches, stream-ordered, no host synchronisation,
 * no allocation.  frames: D2S_FMT_U8_HWC, D2S_FMT_U8_CHW or D2S_FMT_F32_CHW (0..255; the reference's capture tensor is CHW), device.
 * stats: device float [batch][6] = (top_i, bottom_count, center_mean, center_bright, left_i, right_count), exactly stats_t of
 * crop.py:413: the leading / trailing run lengths of sampled rows resp. columns whose unbiased luma std is < 6, and the mean luma /
 * mean `luma > 20` fraction of the sampled rows of the middle 30 %.  Host integer logic turns them into a crop rectangle
 * (desktop2stereo_amd/crop.py crop_from_stats = _movie_crop_from_stats, crop.py:235-296).  workspace: device, 4-byte aligned, at
 * least d2s_crop_detect_workspace bytes.  H < 64 or W < 64 is refused (the reference returns the identity crop before sampling,
 * crop.py:369).  Every argument is checked before any HIP call. */
int d2s_crop_detect_workspace(int batch, int H, int W, uint64_t* bytes);
int d2s_crop_detect(const void* frames, int fmt, int batch, int H, int W, float* stats /* device [batch][6] */,
                    void* workspace, uint64_t workspace_bytes, void* stream);

/* The viewer's other four `Display Mode`s (gui.py:1666, viewer.py:1340), each one program the reference runs over its letter-boxed
 * viewport (viewer.py:2604-2662: u_eye_offset = +ipd_uv/2, u_depth_strength = 0.1 * depth_ratio, blending off):
 *   ANAGLYPH       ANAGLYPH_FRAGMENT (viewer.py:678-832): both eyes per pixel, no depth shaping, hard disocclusion test
 *                  (|d(-2px) - d(+2px)| > 0.08), out = (left.r, right.g, right.b), alpha = both eyes' 0.015-wide border bands;
 *   INTERLEAVED    INTERLEAVED_FRAGMENT (viewer.py:835-1017): even window rows (gl_FragCoord.y) the left eye, odd rows the right;
 *                  in-painting REPLACES the colour where smoothstep(0.06, 0.12, jump) > 0.001;
 *   INTERLEAVED_V  VERTICAL_INTERLEAVED_FRAGMENT (viewer.py:1020-1197): the same by window column, push-pull swept the other way;
 *   DEPTH_MAP      DEPTH_FRAGMENT (viewer.py:633-675): spectral_r_ultrafast(depth) (rgb 0..255 like the other modes), alpha 1.
 * d2s_dibr_params is read as for d2s_dibr_warp except:
 *   - viewport = (x, y, w, h) of the program's viewport in WINDOW pixels, y up -- it is also u_viewport.  The output is h x w; its
 *     row r (0 = top) and column c are the fragment at gl_FragCoord = (x + c + 0.5, y + (h - 1 - r) + 0.5), so x and y decide which
 *     eye an interleaved row / column shows.  x, y >= 0 and w, h > 0 must be whole numbers (glViewport takes integers); all zeros =
 *     (0, 0, W, H).  w x h may differ from the source (a 1080p frame on a 2160-row interleaved panel: the taps filter bilinearly);
 *   - display_mode is ignored.
 * rgb may be NULL for DEPTH_MAP.  Output: three channels per pixel (four with alpha_mode == D2S_DIBR_ALPHA_RGBA) as
 * D2S_FMT_U8_HWC (round-half-even) or D2S_FMT_F32_HWC (0..255), batch-major.  Every argument is checked before any HIP call.
 * Pinned by tests/golden/composite.npz: the reference's four programs run off-screen (tests/golden/make_golden_composite.py). */
enum { D2S_COMPOSITE_ANAGLYPH = 0, D2S_COMPOSITE_INTERLEAVED = 1, D2S_COMPOSITE_INTERLEAVED_V = 2, D2S_COMPOSITE_DEPTH_MAP = 3 };
int d2s_dibr_composite_shape(int H, int W, const d2s_dibr_params* p, int composite, int* out_h, int* out_w);
int d2s_dibr_composite(const uint8_t* rgb, const float* depth, int batch, int H, int W, const d2s_dibr_params* p,
                       int composite, void* out, int out_fmt, void* stream);
/* d2s_dibr_composite with depth float [batch,dh,dw] at any resolution, as d2s_dibr_warp_depth (d2s_version() >= 113): bit-identical
 * to d2s_upsample_depth + d2s_dibr_composite; dh == H && dw == W is exactly d2s_dibr_composite.  Shape from d2s_dibr_composite_shape. */
int d2s_dibr_composite_depth(const uint8_t* rgb, const float* depth, int dh, int dw, int batch, int H, int W,
                             const d2s_dibr_params* p, int composite, void* out, int out_fmt, void* stream);
/* What d2s_dibr_composite / d2s_dibr_composite_depth would launch for these arguments (d2s_version() >= 134; pure host code: launches
 * nothing, needs no GPU).  It runs the launcher's own code up to the launch -- the checks, the viewport, the uniforms, the window
 * plan (512 columns per block while the window stays <= 640 words, the row kernel while the 256-column window stays <= 1536) and the
 * Depth Map's store form -- and refuses what the launcher refuses of these arguments.  out_align = the output address modulo 16: the
 * Depth Map stores 16-byte vectors when it is 0, bytes / floats otherwise; the other programs ignore it.  kernel:
 *   "comp_rows<ana|il|ilv,u8|f32,fx=0|1,256|512,FullDep|UpDep>"   the LDS-window row kernel (roll == 0),
 *   "comp<ana|il|ilv,u8|f32,roll0|general,FullDep|UpDep>"         the gather kernel,
 *   "depth_map<u8|f32,3|4,vec|scalar,FullDep|UpDep>"              the Depth Map.
 * rows, cols, margin, ww: the window plan, as in the warp plan's result above -- all zero for the Depth Map; out_h x out_w: the viewport;
 * grid / block: the launch's; lds_*_bytes: the row kernel's request (0 otherwise), never above 65 536. */
typedef struct d2s_dibr_composite_plan_result {
    uint32_t struct_size;      /* MUST be sizeof(d2s_dibr_composite_plan_result) */
    int32_t rows, cols, margin, ww;
    int32_t roll0, up, fx, vec;
    int32_t out_h, out_w;
    uint32_t grid[3], block;
    uint32_t lds_dynamic_bytes, lds_static_bytes;
    char kernel[64];
} d2s_dibr_composite_plan_result;
int d2s_dibr_composite_plan(int dh, int dw, int batch, int H, int W, const d2s_dibr_params* p, int composite, int out_fmt,
                            unsigned out_align, d2s_dibr_composite_plan_result* res);

/* f3: the MJPEG sink of the Streamer modes.  Replaces `cv2.imencode('.jpg', bgr, [IMWRITE_JPEG_QUALITY, q])` on the
 * frame make_sbs returns (reference streamer.py:249-256, 285-291; quality = settings.yaml "Stream Quality",
 * utils.py:821): convertTo(CV_8U) (round-half-even, saturate) + baseline JPEG as libjpeg(-turbo) writes it with
 * jpeg_set_defaults + jpeg_set_quality(q, TRUE) -- YCbCr 4:2:0, slow-integer FDCT, Annex-K tables, no restart
 * markers, JFIF 1.01 -- BYTE-IDENTICAL to libjpeg-turbo's output for the same RGB frame.
 * frames: `batch` RGB frames, D2S_FMT_U8_HWC or D2S_FMT_F32_HWC (0..255), device.  out: device bytes, frame b at
 * out + b*out_stride; sizes[b] (device int32) = JPEG length, or -1 if it would not fit out_stride (nothing usable
 * is written then).  d2s_jpeg_bound gives a stride that can never overflow and the workspace bytes PER FRAME
 * (workspace: device, 256-byte aligned, >= batch * that).  Stream-ordered, no host synchronisation. */
int d2s_jpeg_bound(int H, int W, int64_t* out_bytes, int64_t* workspace_bytes);
int d2s_jpeg_encode(const void* frames, int fmt, int batch, int H, int W, int quality, uint8_t* out,
                    int64_t out_stride, int32_t* sizes, void* workspace, int64_t workspace_bytes, void* stream);

/* f4: device-resident hand-off of a produced frame to the display path -- replaces the viewer's per-frame
 * `stream.synchronize()` + hipGraphicsMapResources + hipMemcpy(D2D into the PBO) + unmap (reference viewer.py:1584-1712,
 * 2399-2428; CUDART_GL viewer.py:232-345).  The consumer lends a ring of its own device buffers (d2s_present_bind: any
 * device pointer, e.g. a mapped GL PBO; d2s_present_bind_gl_buffer: a GL buffer id, registered WRITE_DISCARD like
 * viewer.py:293 -- needs a current GL context); the producer acquires a slot, passes its pointer as `out` of d2s_pipeline /
 * d2s_make_sbs / d2s_upsample_depth, and publishes it; the consumer picks the latest published slot.  All waits are
 * HIP events between the two streams (consumer_stream = (void*)-1: host wait, for a GL consumer): no copy, no host
 * synchronisation on the producer side.  Producer and consumer may be different host threads.  Triple buffering: the
 * producer never takes the slot the consumer holds (between consume and release) and, while another slot is free, not the
 * latest published one either -- use >= 3 slots when both sides run concurrently (with 2, a consume may find nothing
 * published while the producer rewrites the only free slot). */
typedef struct d2s_present d2s_present;
int d2s_present_create(int device_id, int slots, d2s_present** out);
int d2s_present_bind(d2s_present* p, int slot, void* dev_ptr, uint64_t bytes);
int d2s_present_bind_gl_buffer(d2s_present* p, int slot, unsigned gl_buffer);
int d2s_present_acquire(d2s_present* p, void* producer_stream, int* slot, void** dev_ptr, uint64_t* bytes);
int d2s_present_publish(d2s_present* p, int slot, void* producer_stream);
/* producer: hand an acquired slot back unpublished (the frame was not produced); it becomes acquirable again, the consumer never sees it */
int d2s_present_cancel(d2s_present* p, int slot, void* producer_stream);
int d2s_present_consume(d2s_present* p, void* consumer_stream, int* slot, void** dev_ptr, uint64_t* seq);
int d2s_present_release(d2s_present* p, int slot, void* consumer_stream);
int d2s_present_destroy(d2s_present* p);

/* ---------------------------------------------------------------------------------------------
 * Fused frame pipeline: predict_depth + make_sbs for a batch of frames
 * (capture -> depth -> warp of reference main.py:232-262, 1336-1341 in one stream-ordered
 * call).  frames u8 HWC [batch,H,W,3]; out per d2s_sbs_shape in out_fmt; depth_full (optional,
 * may be NULL) receives predict_depth's return value, float [batch,H,W].
 * use_ema: run DepthStabilizer across the batch in frame order using the engine's stream state
 * (d2s_engine_reset_stream clears it). */
int d2s_pipeline(d2s_engine* e, const uint8_t* frames, int batch, int H, int W,
                 int depth_resolution, const d2s_pre_params* pre /* NULL: ImageNet constants, CPU-branch resize */,
                 const d2s_post_params* pp, const d2s_sbs_params* sp,
                 int use_ema, void* out, int out_fmt, float* depth_full, void* stream);
/* d2s_pipeline with a stream table (see d2s_model_forward_streams).  use_ema on a temporal engine: one DepthStabilizer state per
 * stream slot, each row updating its own; on a Depth-Anything-v2 engine (stream_ids must be NULL) the in-order chain over the batch. */
int d2s_pipeline_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                         int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_sbs_params* sp,
                         int use_ema, void* out, int out_fmt, float* depth_full, void* stream);
/* The Viewer pipeline (d2s_version() >= 113): d2s_pipeline_streams with the warp the reference's Viewer / OpenXR modes show.  The
 * same call up to and including the EMA step (one code path); then the DIBR shader warp reads the engine's model-resolution depth
 * directly (d2s_dibr_warp_depth / d2s_dibr_composite_depth: no full-resolution depth map is written unless depth_full asks for it).
 *   view = -1: the stereo warp with disocclusion in-painting, both eyes packed per dp->display_mode (shape: d2s_dibr_shape);
 *   view = D2S_COMPOSITE_*: that composite program over dp->viewport (shape: d2s_dibr_composite_shape).
 * out: D2S_FMT_U8_HWC or D2S_FMT_F32_HWC, three channels (four with dp->alpha_mode == D2S_DIBR_ALPHA_RGBA); it may be a
 * d2s_present slot pointer.  depth_full (may be NULL) receives the same map d2s_pipeline gives.  Refuses what d2s_pipeline_streams
 * and the DIBR entries refuse (frame / engine shape, stream ids, struct_size, view, viewport, formats); nothing is launched on a
 * refusal.  Bit-identical to d2s_pipeline(depth_full) followed by d2s_dibr_warp / d2s_dibr_composite on that map. */
int d2s_view_pipeline_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                              int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp,
                              int view, int use_ema, void* out, int out_fmt, float* depth_full, void* stream);
/* d2s_view_pipeline_streams with the OpenXR screen's source crop (d2s_version() >= 114; xr_viewer/implementation.py:111-126): the
 * same pipeline_check + depth code path, then d2s_dibr_warp_crop on the engine's model-resolution depth (shape: d2s_dibr_crop_shape).
 * view must be -1: the composites are not an OpenXR path and are refused with a crop.  Bit-identical to d2s_pipeline(depth_full)
 * followed by d2s_dibr_warp_crop on the engine's map. */
int d2s_view_pipeline_crop_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                   int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp,
                                   int view, const double* crop, int use_ema, void* out, int out_fmt, float* depth_full, void* stream);

/* d2s_view_pipeline_crop_streams with the OpenXR eye views as its last stage (d2s_version() >= 115): the same pipeline_check + depth
 * code path, then d2s_dibr_xr_eyes on the engine's model-resolution depth, read directly (crop may be NULL = identity; out, workspace:
 * as d2s_dibr_xr_eyes).  Bit-identical to d2s_pipeline(depth_full) followed by d2s_dibr_xr_eyes on the engine's map. */
int d2s_view_pipeline_xr_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                 int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp,
                                 const double* crop, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int use_ema,
                                 void* out, int out_fmt, float* depth_full, void* workspace, uint64_t workspace_bytes, void* stream);
/* d2s_view_pipeline_xr_streams with the glow (d2s_version() >= 119): glow, levels as d2s_dibr_xr_eyes_glow.  levels is the CALLER's
 * chain of these frames (d2s_mip_chain on the same stream beforehand, or an older one: the reference refreshes its own every few
 * frames).  Bit-identical to d2s_pipeline(depth_full) followed by d2s_dibr_xr_eyes_glow on the engine's map. */
int d2s_view_pipeline_xr_glow_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                      int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp,
                                      const double* crop, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int use_ema,
                                      void* out, int out_fmt, float* depth_full, void* workspace, uint64_t workspace_bytes,
                                      const d2s_xr_glow* glow, const uint8_t* levels, void* stream);
/* d2s_view_pipeline_xr_glow_streams with d2s_dibr_xr_eyes_glow_curved as its last stage (d2s_version() >= 122; _render_eye,
 * xr_viewer/effects.py:1023-1145 with _render_curved_glow, :408-474): workspace as d2s_dibr_xr_glow_curved_workspace.  Bit-identical to
 * d2s_pipeline(depth_full) followed by d2s_dibr_xr_eyes_glow_curved on the engine's map. */
int d2s_view_pipeline_xr_glow_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                             int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                             const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                             const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                             void* workspace, uint64_t workspace_bytes, const d2s_xr_glow* glow, const uint8_t* levels,
                                             void* stream);
/* d2s_view_pipeline_xr_glow_streams with d2s_dibr_xr_eyes_frost as its last stage (d2s_version() >= 124): frost, levels and workspace as
 * that call takes them; every refusal of its plan is made before the model starts.  Bit-identical to d2s_pipeline(depth_full) followed
 * by d2s_dibr_xr_eyes_frost on the engine's map. */
int d2s_view_pipeline_xr_frost_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                       int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp, const d2s_dibr_params* dp,
                                       const double* crop, const d2s_xr_screen* screen, const d2s_xr_eye* eyes, int n_eyes, int use_ema,
                                       void* out, int out_fmt, float* depth_full, void* workspace, uint64_t workspace_bytes,
                                       const d2s_xr_frost* frost, const uint8_t* levels, void* stream);
/* d2s_view_pipeline_xr_frost_streams with d2s_dibr_xr_eyes_frost_curved as its last stage (d2s_version() >= 126): workspace as
 * d2s_dibr_xr_frost_curved_workspace.  Bit-identical to d2s_pipeline(depth_full) followed by d2s_dibr_xr_eyes_frost_curved on the
 * engine's map. */
int d2s_view_pipeline_xr_frost_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                              int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                              const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                              const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                              void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                              void* stream);
/* d2s_view_pipeline_xr_frost_streams with d2s_dibr_xr_eyes_panorama as its last stage (d2s_version() >= 127): glow, pano, pano_rgb and
 * pano_levels as that call takes them, the workspace as it asks.  Every refusal is made before the model starts.  Bit-identical to
 * d2s_pipeline(depth_full) followed by d2s_dibr_xr_eyes_panorama on the engine's map. */
int d2s_view_pipeline_xr_panorama_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                          int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                          const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                          const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                          void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                          const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                                          const uint8_t* pano_levels, void* stream);
/* The same with d2s_dibr_xr_eyes_panorama_curved as the last stage (d2s_version() >= 129).  Bit-identical to d2s_pipeline(depth_full)
 * followed by d2s_dibr_xr_eyes_panorama_curved on the engine's map. */
int d2s_view_pipeline_xr_panorama_curved_streams(d2s_engine* e, const uint8_t* frames, int batch, const int* stream_ids, int H, int W,
                                                 int depth_resolution, const d2s_pre_params* pre, const d2s_post_params* pp,
                                                 const d2s_dibr_params* dp, const double* crop, const d2s_xr_screen* screen,
                                                 const d2s_xr_eye* eyes, int n_eyes, int use_ema, void* out, int out_fmt, float* depth_full,
                                                 void* workspace, uint64_t workspace_bytes, const d2s_xr_frost* frost, const uint8_t* levels,
                                                 const d2s_xr_glow* glow, const d2s_xr_panorama* pano, const uint8_t* pano_rgb,
                                                 const uint8_t* pano_levels, void* stream);
int d2s_engine_reset_stream(d2s_engine* e);      /* every slot: temporal windows and EMA state */

/* Per-kernel-class timing with HIP events on the launch stream (used by bench.py for the
 * roofline figures; not part of the throughput path).  enable=1 clears the records and starts
 * recording around every kernel launch of d2s_model_forward / d2s_pipeline; read() synchronises on
 * the recorded events and returns per class: total milliseconds, algorithmic FLOPs, algorithmic
 * bytes and launch count.  Arrays must hold >= 8 entries; class names via d2s_profile_class_name. */
int d2s_engine_profile(d2s_engine* e, int enable);
int d2s_engine_profile_read(d2s_engine* e, int max_classes, double* ms, double* flops, double* bytes,
                            int64_t* launches, int* n_classes);
const char* d2s_profile_class_name(int cls);

/* Debug / parity taps: copy an internal activation (after the last d2s_model_forward) to a
 * caller device buffer as float32.  name: "embeddings", "layer<N>" (engines created with D2S_TAPS=1), "neck_feat<i>".
 * rows/cols describe [rows, cols] of frame 0 (tokens x D, or pixels x C, NHWC). */
int d2s_engine_tap(d2s_engine* e, const char* name, float* out, uint64_t out_elems,
                   int* rows, int* cols, void* stream);

/* Stand-alone GEMM probe used by tests and the micro-benchmark:
 * C[M,N] = A[M,K] * W[N,K]^T (+bias), A/W given as float32 device arrays, computed with the
 * engine's MFMA kernel in the requested precision. */
int d2s_gemm_probe(const float* A, const float* Wt, const float* bias, float* C,
                   int M, int N, int K, int precision, int tile, int iters, void* stream);

/* Stand-alone attention probe (tests, micro-benchmark): out[B, N, heads*64] = softmax(q k^T / 8) v for float32 device
 * arrays q, k, v [B, heads, N, 64], through the engine's attention kernel for that shape (HF Dinov2SelfAttention.forward;
 * reference call site depth.py:1778).  iters > 1: *ms_per_iter (host) = mean launch time over iters - 1 repeats. */
int d2s_attention_probe(const float* q, const float* k, const float* v, float* out, int B, int heads, int N,
                        int precision, int iters, float* ms_per_iter, void* stream);

/* d2s_attention_probe for the tests (d2s_version() >= 116): every launch the engine can make of its attention kernels -- the e4m3
 * output of the fp8 engines included -- with the operands packed as d2s_attention_probe packs them (V^T zero beyond N; bf16: the q
 * columns pre-scaled by 64^-0.5 log2 e as the engine folds it into W_q, fp32 / bf16x3: unscaled).  The output comes back raw, in
 * the kernel's own type, between two guard rows; reports the kernel it ran. */
typedef struct d2s_attention_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_attention_probe_params) = 192 */
    int32_t precision;         /* D2S_PREC_BF16 / D2S_PREC_FP32 / D2S_PREC_BF16X3 (operands and, but for out_e4m3, the output) */
    int32_t B, heads, N;       /* frames, heads (64 channels each), tokens */
    int32_t out_e4m3;          /* 1 (bf16 only): out = e4m3 sat(result * oscale), what the fp8 engines hand their output projection */
    float   oscale;            /* out_e4m3: the kernel's fp8_qscale, as the engine passes 1 / s_act */
    int32_t reserved;          /* 0 */
    const float* q;            /* device, [B, heads, N, 64] */
    const float* k;
    const float* v;
    void* out;                 /* device, [1 + B*N + 1, heads*64] elements of the output type (bf16 2 bytes, fp32 4, bf16x3 unit words 4,
                                  e4m3 1): the probe fills ALL of it with 0x7f bytes, then the kernel writes rows 1 .. B*N */
    char kernel[128];          /* out: the kernel that ran, e.g. "attention32_kernel<out=fp8>" */
} d2s_attention_probe_params;
int d2s_attention_probe_ex(d2s_attention_probe_params* p, void* stream);

/* Stand-alone 3x3 convolution probe (tests): one convolution of the DPT neck / head through the engine's own dispatcher
 * (launch_gemm), with the operands cast and packed as the engine casts and packs them.  Reports the kernel it ran. */
typedef struct d2s_conv3_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_conv3_probe_params) = 256 */
    int32_t precision;         /* D2S_PREC_BF16 / D2S_PREC_FP32 / D2S_PREC_BF16X3 (operands; bf16: bf16 activations, else fp32) */
    int32_t tile;              /* 0: what the engine passes (automatic; map_head: the fused head's tile); else a tile code */
    int32_t batch, C, N;       /* images, input channels (multiple of 8 for bf16, of 4 otherwise), output channels (multiple of 4) */
    int32_t Hs, Ws;            /* the input map x [batch, Hs, Ws, C] */
    int32_t Hi, Wi;            /* the map the convolution sees; (Hs, Ws) != (Hi, Wi): an align_corners bilinear up-sample of x in front
                                  of it, folded into the loader (bf16 only; D2S_E_UNSUPPORTED where the engine would not fold it) */
    int32_t stride;            /* 1 | 2, pad 1: output Ho = (Hi - 1) / stride + 1, Wo likewise */
    int32_t relu_in;           /* max(x, 0) on load */
    int32_t act;               /* 0: none, 1: ReLU after the bias, before the residual */
    int32_t out_f32;           /* 0: the operand type (bf16 for D2S_PREC_BF16, fp32 otherwise); 1: fp32 */
    int32_t map_head;          /* 1: the DPT head's fused tail: out = float depth [batch, Ho, Wo] = act(b3 + sum_n w3[n] relu(conv + bias)),
                                  act = ReLU (max_depth 0) or sigmoid * max_depth */
    float   b3, max_depth;
    int32_t reserved;          /* 0 */
    int64_t splitk_elems;      /* > 0: a split-K workspace of this many fp32 partials, as the engine's (0: none) */
    const float* x;            /* device, [batch, Hs, Ws, C] */
    const float* w;            /* device, PyTorch layout [N, C, 3, 3] */
    const float* bias;         /* device, [N] or null */
    const float* res;          /* device, [batch, Ho, Wo, N] or null: added last */
    const float* w3;           /* device, [N] (map_head) */
    void* out;                 /* device, [batch, Ho, Wo, N] of the output type (bf16 = 2 bytes), or float [batch, Ho, Wo] (map_head) */
    char kernel[128];          /* out: the kernel that ran, e.g. "conv3_wide_kernel<8,32>" or "gemm_glds_kernel<bf16,...> tile=3264 splitk=4" */
} d2s_conv3_probe_params;
int d2s_conv3_probe(d2s_conv3_probe_params* p, void* stream);

/* Stand-alone probe of a fusion stage's fused residual unit (tests; d2s_version() >= 125): out = x + conv2(relu(conv1(relu(x)))), and
 * with wp its 1x1 projection wp (.) + bp, as ONE launch (conv3_rcu_kernel), bf16, weights packed through the functions the engine packs
 * them with.  It plans (the engine's rule: C = 128, 4 x 8-pixel tiles x batch <= CU count; D2S_E_UNSUPPORTED otherwise), launches that
 * plan and reports the kernel.  reserved = 1 (d2s_version() >= 131): the kernel's wide form, 8 x 8-pixel tiles x batch <= CU count.  The reference is the same chain through d2s_conv3_probe (relu_in, res) and d2s_linear_probe. */
typedef struct d2s_rcu_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_rcu_probe_params) = 216 */
    int32_t batch, H, W, C;    /* the map x [batch, H, W, C] */
    int32_t reserved;          /* 0: the 4 x 8-pixel tile form; 1: the wide form */
    const float* x;            /* device, [batch, H, W, C] */
    const float* w1;           /* device, PyTorch layout [C, C, 3, 3] */
    const float* b1;           /* device, [C] */
    const float* w2;
    const float* b2;
    const float* wp;           /* device, [C, C], or null: no projection */
    const float* bp;           /* device, [C] (with wp) */
    void* out;                 /* device, [batch, H, W, C] bf16 */
    char kernel[128];          /* out: "conv3_rcu_kernel<0>" | "conv3_rcu_kernel<1>"; wide: "conv3_rcu_kernel<0,1>" | "conv3_rcu_kernel<1,1>" */
} d2s_rcu_probe_params;
int d2s_rcu_probe(d2s_rcu_probe_params* p, void* stream);

/* Stand-alone linear probe (tests): one linear of the encoder, the DPT neck or a temporal module through the engine's own dispatcher
 * (launch_gemm), its epilogue built by the engine's per-site helpers and its operands cast and packed as the engine casts and packs
 * them (bf16 / bf16x3 units / e4m3 with s_w[n] = max|row n| / 448; LayerNorm folding W' = W diag(gamma), bias' = b + W beta,
 * csum[n] = sum_k of the rounded W'[n, k]).  A LayerNorm-folded consumer takes its statistics from a real producer launch, run first
 * as the engine chains them.  Reports the kernel(s) it ran.  Matrices are row-major float32 device tensors unless noted. */
enum {
    D2S_LIN_PATCH = 0,         /* patch embedding: a [M = B*P, K] patch rows -> x [B*ntok, N] rows 1..P of every frame (+ res = pos [ntok, N]) */
    D2S_LIN_QKV = 1,           /* a [M, K = D] -> out q | k [M, 3D] (columns < 2D), vt [B, heads, 64, npad] (M = B*ntok) */
    D2S_LIN_PROJ = 2,          /* x [M, N] += scale * (a W^T + bias)            (in place; ln_fold: the producer -> out2, stats) */
    D2S_LIN_FC1 = 3,           /* out [M, N] = GELU(a W^T + bias) */
    D2S_LIN_FC2 = 4,           /* as D2S_LIN_PROJ */
    D2S_LIN_NECK_PROJ = 5,     /* out [B*P, N] = a W^T + bias, a [B*P, K] (M = B*ntok); ln_fold: the final LayerNorm folded in (bf16) */
    D2S_LIN_NECK_RESIZE = 6,   /* ConvTranspose2d(k = s = ks): a [M = B*gh*gw, K] -> out [B, ks*gh, ks*gw, K]; w [K, K, ks, ks], bias [K],
                                  N = ks*ks*K */
    D2S_LIN_TM_PROJ_IN = 7,    /* x [M, N] = a W^T + bias (ln_fold: the producer) */
    D2S_LIN_TM_KVQ = 8,        /* out [M, N] = a W^T (+ bias) */
    D2S_LIN_TM_FF1 = 9,        /* out [M, N] = a W^T + bias; ln_fold: GEGLU in the epilogue, out [M, N/2] = x * gelu(gate) (w rows: x | gate) */
    D2S_LIN_TM_TO_OUT = 10,    /* x [M, N] += a W^T + bias (ln_fold: the producer) */
    D2S_LIN_TM_FF2 = 11,       /* as D2S_LIN_TM_TO_OUT; ln_fold: out2 only, no statistics */
    D2S_LIN_TM_PROJ_OUT = 12   /* out [M, N] = a W^T + bias + res [M, N] + res2 [M, N] */
};
typedef struct d2s_linear_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_linear_probe_params) = 488 */
    int32_t site;              /* D2S_LIN_* */
    int32_t precision;         /* the ENGINE's: D2S_PREC_FP32 / BF16 / BF16X3 / FP8 (e4m3 on all four encoder linears) / FP8_MLP */
    int32_t ln_fold;           /* consumers (QKV, FC1, NECK_PROJ, TM_KVQ, TM_FF1): LayerNorm (ln_g, ln_b, ln_eps) folded in, statistics
                                  from a producer launch x += pscale * (pa pW^T + pbias) run first; producers (PROJ, FC2, TM_PROJ_IN,
                                  TM_TO_OUT, TM_FF2): write out2 and stats */
    int32_t M, N, K;           /* rows (see the sites), weight rows (packed order), reduction length */
    int32_t ntok, heads, npad; /* tokens per frame (PATCH, QKV, NECK_PROJ); QKV: heads (64 channels each), V^T row length */
    int32_t gh, gw, ks;        /* NECK_RESIZE: patch grid and ConvTranspose kernel = stride */
    int32_t pK;                /* ln_fold consumers: K of the producer (pa [M, pK], pw [K, pK], pbias / pscale [K]) */
    float   ln_eps;
    float   s_act, s_out, s_res, s_pact;   /* e4m3 scales: this linear's A, an e4m3 output (FC1), the raw residual copy out2, the producer's A */
    int32_t tile;              /* 0: what the engine passes (automatic); else a tile code */
    int64_t splitk_elems;      /* > 0: a split-K workspace of this many fp32 partials, as the engine's (row-mapped launches, bf16 / fp32 /
                                  bf16x3 operands: what the engine's linear() hands over) */
    const float* a;            /* [M, K] (ln_fold consumers: unused -- A is the producer's out2) */
    const float* w;            /* [N, K] PyTorch layout (NECK_RESIZE: ConvTranspose2d [K, K, ks, ks]) */
    const float* bias;         /* [N] or null (NECK_RESIZE: [K]) */
    const float* scale;        /* [N] LayerScale or null (PROJ, FC2) */
    const float* res;          /* PATCH: pos [ntok, N]; TM_PROJ_OUT: [M, N] */
    const float* res2;         /* TM_PROJ_OUT: [M, N] or null */
    const float* ln_g;         /* [K] (ln_fold consumers) */
    const float* ln_b;         /* [K] */
    const float* pa;           /* [M, pK] */
    const float* pw;           /* [K, pK] */
    const float* pbias;        /* [K] or null */
    const float* pscale;       /* [K] or null */
    float* x;                  /* the fp32 residual stream [M, N] (PATCH: [B*ntok, N]; ln_fold consumers: [M, K], the producer's), in / out */
    void* out;                 /* the output in the engine's type for the site (bf16, fp32, bf16x3 units, e4m3) */
    void* out2;                /* ln_fold: the raw residual copy [M, D] (D = K for consumers, N for producers): bf16 / units / e4m3 */
    void* vt;                  /* QKV: [B, heads, 64, npad] of the output type */
    float* stats;              /* ln_fold (not TM_FF2): [D / 16 + 1][M][2] (sum, sum of squares) partials */
    int32_t stats_slots;       /* out: the column blocks the producer reported */
    int32_t reserved;          /* 0 */
    char kernel[128];          /* out: the kernel this linear ran, e.g. "gemm_pp_kernel<bf16,PP_K_F32_LN> ks=3 tail=row-split" */
    char kernel2[128];         /* out: the producer's (ln_fold consumers), else "" */
} d2s_linear_probe_params;
int d2s_linear_probe(d2s_linear_probe_params* p, void* stream);

/* Stand-alone probe of the temporal-module and LayerNorm launchers (tests; d2s_version() >= 117): one call of the launcher the engine's
 * run_temporal / encoder calls, on device operands ALREADY in the kernel's storage type (bf16 = raw bf16 bits, outputs raw: bf16x3 unit
 * words, e4m3 bytes).  The probe packs nothing and allocates nothing.  Before anything is launched every size and count is checked
 * against the element counts the caller states for each buffer; a malformed case is an error return.  Reports the kernel it launched. */
enum {
    D2S_TP_GROUPNORM = 0,      /* launch_groupnorm: x, out [rows][sites, C], gamma / beta [C], groups, eps */
    D2S_TP_TEMPORAL_ATTN = 1,  /* launch_temporal_attn: x = cur [rows][sites][3C] (k' | v' | q'), ptab float [32][3C], out [rows][sites][C],
                                  row r: ring[r] [slots][sites][2C], head[r], Tw[r] (1 | 32), store_slot[r] (-1: none) */
    D2S_TP_CACHE_STORE = 2,    /* launch_cache_store: x = cur; row r: ring[r], slot0[r], nslots[r] (slot0 + nslots <= slots); kernel = ""
                                  when no row has a slot to fill (nothing is launched) */
    D2S_TP_GEGLU = 3,          /* launch_geglu: x = u [rows, 2 C], out [rows, C] = u[:, :C] * gelu(u[:, C:])   (C = the engine's 4 C) */
    D2S_TP_CAST_F32 = 4,       /* launch_cast_f32: x float [n] -> out [n] of the precision's type */
    D2S_TP_LAYERNORM = 5       /* launch_layernorm: x float, gamma / beta [C], out [rows, C] (C = D); rows_per_img > 0: output row r reads
                                  input row (r / rows_per_img) img_rows + r % rows_per_img + row_off; qscale > 0: e4m3 output;
                                  bx3_out: bf16x3 units (out 32-byte aligned) */
};
typedef struct d2s_temporal_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_temporal_probe_params) */
    int32_t op;                /* D2S_TP_* */
    int32_t precision;         /* D2S_PREC_BF16 / D2S_PREC_FP32: the engine class, i.e. the storage type of x and out (see the ops) */
    int32_t rows, sites, C;    /* batch rows (LAYERNORM, GEGLU: matrix rows), sites per row, channels */
    int32_t groups, slots;     /* GROUPNORM: groups; TEMPORAL_ATTN / CACHE_STORE: slots of a ring (the engine: 31) */
    float   eps;               /* GROUPNORM, LAYERNORM */
    float   qscale;            /* LAYERNORM: > 0 = e4m3 output sat(LN(x) * qscale) */
    int32_t bx3_out;           /* LAYERNORM: 1 = bf16x3 unit output */
    int32_t rows_per_img, img_rows, row_off;   /* LAYERNORM row map (0, 0, 0: plain) */
    int64_t n;                 /* CAST_F32: elements */
    const void* x;             /* the input (device) */
    void* out;                 /* the output (device); CACHE_STORE: unused */
    const float* gamma;        /* GROUPNORM, LAYERNORM */
    const float* beta;
    const float* ptab;         /* TEMPORAL_ATTN */
    uint64_t x_elems, out_elems, gamma_elems, beta_elems, ptab_elems;   /* elements each buffer holds, from the pointer given */
    void* ring[D2S_MAX_STREAMS];            /* per row (device), in / out */
    uint64_t ring_elems[D2S_MAX_STREAMS];
    int32_t head[D2S_MAX_STREAMS], Tw[D2S_MAX_STREAMS], store_slot[D2S_MAX_STREAMS];   /* TEMPORAL_ATTN */
    int32_t slot0[D2S_MAX_STREAMS], nslots[D2S_MAX_STREAMS];                           /* CACHE_STORE */
    char kernel[128];          /* out: the kernel that ran, e.g. "groupnorm_reg_kernel<bf16,CPG=8,RPT=2>", "temporal_attn_kernel<f32,CH=4,WinRow>" */
} d2s_temporal_probe_params;
int d2s_temporal_probe(d2s_temporal_probe_params* p, void* stream);

/* Stand-alone probe of d2s_pipeline's fused pre-process + patchify launch (tests; d2s_version() >= 118): launch_preprocess_patches on
 * caller-owned device buffers.  frames u8 HWC [batch,H,W,3]; A [batch * (h/p) * (w/p)][Kp] of the precision's type (bf16 bits / float):
 * columns c p^2 + i p + j < 3 p^2 are written, the rest left alone; resid float [batch][N][D]: row 0 of every frame = cls + pos[0] when
 * cls != NULL (pos may then not be NULL), nothing otherwise.  Every size is checked against the element counts stated here before the
 * launch; the probe packs and allocates nothing.  D2S_E_UNSUPPORTED, nothing launched, where the pipeline would not take this path (a
 * format other than U8_HWC, a frame already at (h, w), 3 p^2 > Kp, bicubic resampling, another precision). */
typedef struct d2s_prepatch_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_prepatch_probe_params) */
    int32_t precision;         /* D2S_PREC_BF16 / D2S_PREC_FP32 */
    int32_t fmt, batch, H, W, decim_stride;
    int32_t h, w, p, Kp, N, D;
    int32_t reserved;
    const d2s_pre_params* pre; /* NULL: ImageNet mean / std, bilinear */
    const void* frames;
    void* A;
    const float* cls;          /* [D] or NULL */
    const float* pos;          /* [>= D]: row 0 of the position embedding */
    float* resid;
    uint64_t frames_elems, A_elems, cls_elems, pos_elems, resid_elems;   /* elements each buffer holds (frames: bytes) */
    char kernel[64];           /* out: "preprocess_patch_kernel<U8_HWC,bf16>" / "...,float>" */
} d2s_prepatch_probe_params;
int d2s_preprocess_patches_probe(d2s_prepatch_probe_params* p, void* stream);

/* Stand-alone probe of the small model-side launchers of vit_ops.hip (tests; d2s_version() >= 128): one call of one launcher on the
 * caller's device buffers as they are (bf16 = raw bf16 bits).  The probe packs, allocates and copies nothing.  Every element the kernel
 * will index is checked against the element counts stated here, and the up-sample's in / out / addend against 16-byte alignment, before
 * the launcher is reached; a malformed case is an error return and nothing is launched.  Reports the kernel that ran. */
enum {
    D2S_VP_PATCHIFY = 0,       /* launch_patchify: x float [B,3,h,w] -> out = A [B (h/p) (w/p)][Kp] of the precision's type (columns >= 3 p^2
                                  zero); cls != NULL: resid [B][N][D] row 0 of every frame = cls + pos[0:D], nothing else of resid */
    D2S_VP_BILINEAR = 1,       /* launch_bilinear_nhwc: x [B,Hi,Wi,C] -> out [B,Ho,Wo,C] (align_corners) + addend [B,Ho,Wo,C] or NULL */
    D2S_VP_HEAD_FINAL = 2,     /* launch_head_final: x [n][C], w3 float [C], b3 -> out float [n]: ReLU (max_depth 0) or sigmoid * max_depth */
    D2S_VP_TO_F32 = 3,         /* launch_to_f32: x [n] of the precision's type -> out float [n] */
    D2S_VP_AMAX = 4            /* launch_amax: out[0] = max(out[0], max |x[0:n]|), x of the precision's type, out float (4-byte aligned) */
};
typedef struct d2s_vit_probe_params {
    uint32_t struct_size;      /* MUST be sizeof(d2s_vit_probe_params) */
    int32_t op;                /* D2S_VP_* */
    int32_t precision;         /* D2S_PREC_BF16 / D2S_PREC_FP32: the storage type (see the ops) */
    int32_t B;                 /* PATCHIFY, BILINEAR: frames */
    int32_t h, w, p, Kp, N, D; /* PATCHIFY */
    int32_t Hi, Wi, Ho, Wo, C; /* BILINEAR; HEAD_FINAL: C */
    float   b3, max_depth;     /* HEAD_FINAL */
    int32_t reserved;          /* 0 */
    int64_t n;                 /* HEAD_FINAL: pixels; TO_F32, AMAX: elements */
    const void* x;             /* the input (device) */
    void* out;                 /* the output (device): A / out / depth / out / the slot */
    const void* addend;        /* BILINEAR, or NULL */
    const float* w3;           /* HEAD_FINAL */
    const float* cls;          /* PATCHIFY: [D] or NULL */
    const float* pos;          /* PATCHIFY: [>= D], row 0 of the position embedding */
    float* resid;              /* PATCHIFY */
    uint64_t x_elems, out_elems, addend_elems, w3_elems, cls_elems, pos_elems, resid_elems;   /* elements each buffer holds */
    char kernel[64];           /* out: the kernel that ran, e.g. "patchify_kernel<bf16>", "bilinear_nhwc_kernel<f32>" */
} d2s_vit_probe_params;
int d2s_vit_probe(d2s_vit_probe_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D2S_H */
