"""The OpenXR viewer's automatic movie crop, host half (reference xr_viewer/crop.py, CropMixin).

The detector kernel (csrc/crop_detect.hip, ops.crop_detect) reduces a capture to six numbers; everything after that is integer
logic on the host, restated here line for line:

    sample_plan(w, h)              _movie_crop_sample_plan           crop.py:298-353 (the integers; the kernel restates them in C)
    crop_from_stats(stats, w, h)   _movie_crop_from_stats            crop.py:235-296
    pixel_bounds(w, h, crop)       _movie_crop_pixel_bounds          crop.py:165-173 (round() is half-to-even; d2s_dibr_crop_shape
                                                                     uses nearbyint on doubles)
    MovieCrop                      _maybe_update_movie_crop, _detect_movie_letterbox_crop(async_gpu), _poll_movie_crop_gpu_result,
                                   _apply_movie_crop_detection, _set_manual_crop_uv, _current_movie_crop_uv
                                                                     crop.py:486-514, 415-433, 218-233, 202-216, 107-115, 142-163

Not built: the cursor-reveal timer (crop.py:516-534) and the environment-profile switches (:10-49) -- both are UI.
Nothing in the logic needs torch; MovieCrop.update imports it (and ops) when it launches the detector.
"""
from __future__ import annotations

import time
from typing import Callable, List, Optional, Sequence, Tuple

FULL = (0.0, 0.0, 1.0, 1.0)
Crop = Tuple[float, float, float, float]


def _lines(n: int, stride: int) -> List[int]:
    """np.arange(0, n, stride) with n - 1 appended when it is not the last entry (crop.py:309-311, 319-321)."""
    v = list(range(0, int(n), stride))
    if not v or v[-1] != int(n) - 1:
        v.append(int(n) - 1)
    return v


def sample_plan(w: int, h: int) -> dict:
    """The sparse grid the detector samples (crop.py:306-322): sampled rows `y_rows` x columns x0:x1:step_x of the middle 80 % for
    the top / bottom scan, and its twin (x_cols, y0_col:y1_col:step_y) for the left / right scan.  center_mask: the rows of the
    middle 30 % that vote on brightness."""
    w, h = int(w), int(h)
    x0 = int(w * 0.10)
    x1 = max(x0 + 1, int(w * 0.90))
    row_stride = max(1, (h + 359) // 360)
    y_rows = _lines(h, row_stride)
    step_x = max(1, (x1 - x0) // 128)
    c_lo, c_hi = int(h * 0.35), int(h * 0.65)
    center_mask = [c_lo <= y < c_hi for y in y_rows]
    y0_col = int(h * 0.10)
    y1_col = max(y0_col + 1, int(h * 0.90))
    col_stride = max(1, (w + 359) // 360)
    x_cols = _lines(w, col_stride)
    step_y = max(1, (y1_col - y0_col) // 128)
    return {"x0": x0, "x1": x1, "step_x": step_x, "row_stride": row_stride, "y_rows": y_rows, "center_mask": center_mask,
            "center_has_rows": any(center_mask), "y0_col": y0_col, "y1_col": y1_col, "step_y": step_y, "col_stride": col_stride,
            "x_cols": x_cols, "samples_per_row": len(range(x0, x1, step_x)), "samples_per_col": len(range(y0_col, y1_col, step_y))}


def _axis_crop(lead_i: int, trail_count: int, lines: Sequence[int], size: int):
    """One axis of _movie_crop_from_stats (:255-273 rows, :275-292 columns): (first kept pixel, kept pixels) or None."""
    n = len(lines)
    anchor_i = n - trail_count - 1
    if anchor_i < lead_i:
        return None
    lead = int(lines[min(lead_i, n - 1)])
    trail = int(size) - min(int(size), int(lines[anchor_i]) + 1)
    min_bar = max(8, int(size * 0.035))
    if lead < min_bar or trail < min_bar:
        return None
    bigger, smaller = max(lead, trail), min(lead, trail)
    if bigger - smaller > max(18, int(bigger * 0.25)):              # the asymmetry test
        return None
    edge_trim = max(2, min(8, int(round(size * 0.004))))
    lo = max(0, min(lead + edge_trim, size - 2))
    hi = max(lo + 1, size - trail - edge_trim)
    kept = hi - lo
    if size - kept < max(16, int(size * 0.07)):                     # the `removed` floor
        return None
    return lo, kept


def crop_from_stats(stats: Sequence[float], w: int, h: int) -> Crop:
    """stats = (top_i, bottom_count, center_mean, center_bright, left_i, right_count) -> (x, y, w, h) in uv, top-left origin
    (crop.py:235-296).  The centre vote (mean luma >= 14 or bright fraction >= 0.035) gates the top / bottom crop only."""
    w, h = int(w), int(h)
    plan = sample_plan(w, h)
    y_rows, x_cols = plan["y_rows"], plan["x_cols"]
    top_i, bottom_count = int(round(float(stats[0]))), int(round(float(stats[1])))
    center_mean, center_bright = float(stats[2]), float(stats[3])
    left_i = int(round(float(stats[4]))) if len(stats) > 4 else 0
    right_count = int(round(float(stats[5]))) if len(stats) > 5 else 0
    has_tb = top_i > 0 and bottom_count > 0 and top_i + bottom_count < len(y_rows)
    has_lr = left_i > 0 and right_count > 0 and left_i + right_count < len(x_cols)
    if not has_tb and not has_lr:
        return FULL
    u0, v0, uw, vh = 0.0, 0.0, 1.0, 1.0
    if has_tb:
        r = _axis_crop(top_i, bottom_count, y_rows, h)
        if r is not None and (center_mean >= 14.0 or center_bright >= 0.035):
            v0, vh = r[0] / float(h), r[1] / float(h)
    if has_lr:
        r = _axis_crop(left_i, right_count, x_cols, w)
        if r is not None:
            u0, uw = r[0] / float(w), r[1] / float(w)
    if u0 == 0.0 and uw == 1.0 and v0 == 0.0 and vh == 1.0:
        return FULL
    return (u0, v0, uw, vh)


def pixel_bounds(w: int, h: int, crop: Sequence[float]) -> Tuple[int, int, int, int]:
    """(x0, y0, x1, y1) in pixels of a uv crop (crop.py:165-173).  round() is half-to-even."""
    w, h = int(w), int(h)
    x, y, cw, ch = (float(crop[0]), float(crop[1]), float(crop[2]), float(crop[3]))
    x0 = max(0, min(int(round(x * w)), max(0, w - 1)))
    y0 = max(0, min(int(round(y * h)), max(0, h - 1)))
    x1 = max(x0 + 1, min(int(round((x + cw) * w)), w))
    y1 = max(y0 + 1, min(int(round((y + ch) * h)), h))
    return x0, y0, x1, y1


def is_active(crop: Sequence[float]) -> bool:
    """_movie_crop_is_active (crop.py:51-59)."""
    return (abs(float(crop[0])) > 1e-5 or abs(float(crop[1])) > 1e-5 or abs(float(crop[2]) - 1.0) > 1e-5
            or abs(float(crop[3]) - 1.0) > 1e-5)


class MovieCrop:
    """One capture stream's crop state.  mode "auto": update(frames) launches the detector when the detection interval has passed
    and no result is pending, poll() takes a finished result through the hysteresis; neither ever waits for the GPU.  mode "manual":
    the centred crop of set_manual(w, h).  mode "off": the full frame.  crop_uv is the crop in force."""

    def __init__(self, mode: str = "auto", interval: float = 1.0, clock: Callable[[], float] = time.perf_counter):
        if mode not in ("auto", "manual", "off"):
            raise ValueError('mode must be "auto", "manual" or "off"')
        self.mode = mode
        self.interval = float(interval)
        self.clock = clock
        self.manual_uv: Crop = FULL
        self._next_detect_t = 0.0
        self._pending = None
        self._bufs = {}                 # (device, batch, w, h) -> (workspace, stats, pinned host, event): this capture's own, allocated once
        self.reset()

    def reset(self):
        """_reset_movie_crop (crop.py:96-102)."""
        self.target_uv: Crop = FULL
        self.target_active = False
        self.full_hits = 0
        self._pending = None

    def set_manual(self, w: float, h: float) -> Crop:
        """_set_manual_crop_uv (crop.py:107-115): a centred crop of the given uv size."""
        w = max(0.0, min(1.0, float(w)))
        h = max(0.0, min(1.0, float(h)))
        self.manual_uv = ((1.0 - w) / 2.0, (1.0 - h) / 2.0, w, h)
        return self.manual_uv

    @property
    def crop_uv(self) -> Crop:
        """_current_movie_crop_uv (crop.py:142-163) without the reveal timer."""
        if self.mode == "manual":
            return self.manual_uv
        if self.mode == "off":
            return FULL
        return self.target_uv

    def apply_detection(self, detected: Sequence[float], h: int):
        """_apply_movie_crop_detection (crop.py:202-216): a new target only when it moves by >= 2 / h; back to the full frame after
        three consecutive full-frame detections."""
        if is_active(detected):
            self.full_hits = 0
            old = self.target_uv
            if max(abs(float(old[i]) - float(detected[i])) for i in range(4)) >= (2.0 / max(h, 1)):
                self.target_uv = tuple(float(v) for v in detected)
            self.target_active = True
        else:
            self.full_hits += 1
            if self.full_hits >= 3 and self.target_active:
                self.reset()

    @property
    def pending(self) -> bool:
        return self._pending is not None

    def poll(self) -> bool:
        """_poll_movie_crop_gpu_result (crop.py:218-233): True while a detection is still in flight; a finished one is applied."""
        p = self._pending
        if p is None:
            return False
        if not p["event"].query():
            return True
        self._pending = None
        try:
            detected = crop_from_stats(p["host"][p["row"]].tolist(), p["w"], p["h"])
        except Exception:
            detected = FULL
        self.apply_detection(detected, p["h"])
        return False

    def update(self, frames, row: int = 0) -> bool:
        """_maybe_update_movie_crop (crop.py:486-514) for a device frame tensor (uint8 HWC / uint8 CHW / float32 CHW, optional batch;
        `row` picks the frame of a batch that belongs to this stream): polls, and when the interval has passed launches the
        detector on the current stream and copies its six floats to pinned memory behind an event (crop.py:415-433).  Returns
        True when a detection was launched.  Never synchronises."""
        if self.mode != "auto":
            self._pending = None
            return False
        if self.poll():
            return False
        now = self.clock()
        if now < self._next_detect_t:
            return False
        self._next_detect_t = now + max(0.2, self.interval)
        import torch
        from . import ops
        fmt, b, h, w = ops._frame_fmt(frames)
        if w < 64 or h < 64:                                        # crop.py:369
            self.apply_detection(FULL, h)
            return False
        key = (frames.device, b, w, h)
        if key not in self._bufs:
            self._bufs = {key: (ops.crop_detect_workspace(b, h, w, frames.device),
                                torch.empty((b, 6), dtype=torch.float32, device=frames.device),
                                torch.empty((b, 6), dtype=torch.float32).pin_memory(), torch.cuda.Event(blocking=False))}
        ws, stats, host, event = self._bufs[key]
        ops.crop_detect(frames, out=stats, workspace=ws)
        host.copy_(stats, non_blocking=True)
        event.record(torch.cuda.current_stream(frames.device))
        self._pending = {"host": host, "event": event, "w": w, "h": h, "row": int(row)}
        return True
