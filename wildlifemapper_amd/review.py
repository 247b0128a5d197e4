"""What a reviewer of a survey looks at: chips and overlays, cut and drawn on the GPU.
  * crop_chips, chip_windows (detect_frames' chips=): one fixed-size crop per detection, cut from the source-resolution
    frame around its box (chip rule: include/wm_hip.h) and resampled with PIL's bilinear arithmetic, every chip of one call
    in one launch (wm_crop_chips_u8).
  * draw_boxes, outline_rects, DEFAULT_PALETTE (detect_frames' overlay=, mosaic's markers): every box outlined in its class
    colour (outline rule: include/wm_hip.h), in place, all boxes of one call in one launch (wm_draw_boxes_u8); overlay_size
    is the size of the picture detect_frames(overlay=L) draws on.
Both launches take frames, boxes and a per-box frame index; _box_launch validates them for both."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

import torch

from . import _native as N
from . import preprocess
from ._survey import _frame_descs, _pinned_upload, _whole_number

CHIP_MAX_SIDE = 1024          # include/wm_hip.h WM_CHIP_MAX_SIDE
DRAW_MAX_WIDTH, DRAW_MAX_PALETTE = 16, 256          # include/wm_hip.h WM_DRAW_MAX_WIDTH, WM_DRAW_MAX_PALETTE
OVERLAY_MIN, OVERLAY_MAX = 64, 8192                 # detect_frames(overlay=L): the long side of the picture

# The project's own colours for labels 0..8, (R, G, B) for an RGB frame: the model's 0-based labels and the reference's
# keys 1..8 are both covered.  Rows are written as they are, whatever the channel order of the frame they are drawn on.
DEFAULT_PALETTE = np.array([(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
                            (70, 240, 240), (240, 50, 230), (255, 255, 255)], dtype=np.uint8)
DEFAULT_PALETTE.setflags(write=False)


def _check_chip(chip, what: str) -> int:
    """Validate a chip size before any device work: an integer multiple of 4 in 16..256."""
    return _whole_number(chip, what, "chip size", 16, 256, 4, "must be a multiple of 4 in 16..256", "is not an integer")


def _check_draw_width(width, what: str) -> int:
    return _whole_number(width, what, "width", 1, DRAW_MAX_WIDTH, must=f"must be in 1..{DRAW_MAX_WIDTH}", not_whole="is not an integer")


def _check_overlay(overlay, what: str) -> int:
    """Validate an overlay size before any device work: an integer in 64..8192."""
    return _whole_number(overlay, what, "overlay size", OVERLAY_MIN, OVERLAY_MAX, must=f"must be in {OVERLAY_MIN}..{OVERLAY_MAX}",
                         not_whole="is not an integer")


def _check_chip_rule(context, min_side, max_side, what: str):
    try:
        context, min_side, max_side = float(context), int(min_side), int(max_side)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: context {context!r}, min_side {min_side!r}, max_side {max_side!r}") from None
    if not (1.0 <= context <= 8.0):
        raise ValueError(f"{what}: context {context!r} must be in [1, 8]")
    if not (1 <= min_side <= max_side <= CHIP_MAX_SIDE):
        raise ValueError(f"{what}: need 1 <= min_side <= max_side <= {CHIP_MAX_SIDE}, got {min_side}, {max_side}")
    return context, min_side, max_side


def _check_palette(palette, what: str) -> np.ndarray:
    """None -> DEFAULT_PALETTE; else a (P,3) uint8 table, P in 1..256, as a contiguous host array."""
    if palette is None:
        return DEFAULT_PALETTE
    if isinstance(palette, torch.Tensor):
        palette = palette.detach().cpu().numpy()
    pal = np.asarray(palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not (1 <= pal.shape[0] <= DRAW_MAX_PALETTE):
        raise ValueError(f"{what}: palette must be a (P,3) uint8 table with P in 1..{DRAW_MAX_PALETTE}, got {pal.dtype} {pal.shape}")
    return np.ascontiguousarray(pal)


_NO_LABELS = object()          # crop_chips' launch has no labels; None is a value draw_boxes can be handed


def _box_launch(who: str, frames, boxes, box_frame, in_place: bool, labels=_NO_LABELS):
    """The frames, boxes and per-box frame index of crop_chips and draw_boxes, validated in that order: (the list of
    (H,W,3) uint8 frames on one ROCm device, that device, the (n,) int32 box_frame on it or None, the (n,) int32 labels
    on it when given).  in_place is the one rule the two differ in: a frame that is not contiguous is refused by a launch that
    writes to it and copied by one that only reads it.  labels (draw_boxes) are looked at after the boxes."""
    frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
    if not frames:
        raise RuntimeError(f"{who}: no frames")
    for i, fr in enumerate(frames):
        if not isinstance(fr, torch.Tensor) or not fr.is_cuda or fr.dtype != torch.uint8 or fr.dim() != 3 or fr.shape[-1] != 3:
            raise RuntimeError(f"{who}: frame {i}: expected an (H,W,3) uint8 ROCm tensor")
        if in_place and not fr.is_contiguous():
            raise RuntimeError(f"{who}: frame {i} is not contiguous (it is drawn on in place)")
    dev = frames[0].device
    if not in_place:
        frames = [fr.contiguous() for fr in frames]
    N.require_cuda(boxes, f"{who}: boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.device != dev or any(fr.device != dev for fr in frames):
        raise RuntimeError(f"{who}: boxes {tuple(boxes.shape)} on {boxes.device}, frames on {dev}: expected (n,4) on one device")
    n = boxes.shape[0]
    if labels is not _NO_LABELS:
        labels = torch.as_tensor(labels)
        if tuple(labels.shape) != (n,) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise RuntimeError(f"{who}: labels {tuple(labels.shape)} {labels.dtype} for {n} boxes: expected (n,) integers")
        labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    if box_frame is not None:
        box_frame = torch.as_tensor(box_frame).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(box_frame.shape) != (n,):
            raise RuntimeError(f"{who}: box_frame {tuple(box_frame.shape)} for {n} boxes")
    return frames, dev, box_frame, labels


def _host_boxes(boxes) -> np.ndarray:
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))


def chip_windows(boxes, context: float = 1.5, min_side: int = 32, max_side: int = CHIP_MAX_SIDE) -> np.ndarray:
    """The chip rule on the host (wm_chip_window; no device call): boxes (n,4) xyxy in frame pixels -> (n,3) int32
    windows (y0, x0, side).  A box with a non-finite coordinate gives (0, 0, 0)."""
    context, min_side, max_side = _check_chip_rule(context, min_side, max_side, "chip_windows")
    b = _host_boxes(boxes)
    out = np.zeros((b.shape[0], 3), dtype=np.int32)
    fn = N.lib().wm_chip_window
    FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for i in range(b.shape[0]):
        N.check(fn(b[i].ctypes.data_as(FP), context, min_side, max_side, out[i].ctypes.data_as(IP)))
    return out


def crop_chips(frames, boxes: torch.Tensor, box_frame=None, chip: int = 128, context: float = 1.5, min_side: int = 32,
               max_side: int = CHIP_MAX_SIDE) -> Tuple[torch.Tensor, torch.Tensor]:
    """One chip x chip review crop per box, all in one launch (wm_crop_chips_u8).  frames: one (H,W,3) uint8 ROCm frame
    or a list of them; boxes (n,4) fp32 xyxy in the pixels of their frame, on the frames' device; box_frame (n,) the
    frame index of each box (None: all in frame 0; an index outside the list gives a zero chip).  Returns (chips
    (n,chip,chip,3) uint8, windows (n,3) int32 = (y0, x0, side)) on the device.  Each chip is the window of the chip
    rule -- a square of side clamp(ceil(max(w, h) * context), min_side, max_side) centred on the box, zeros where it
    reaches past the frame -- resized as PIL.Image.resize((chip, chip), BILINEAR) does, bit for bit.  Runs on the current
    stream; windows and filter coefficients are derived on the device."""
    chip = _check_chip(chip, "crop_chips")
    context, min_side, max_side = _check_chip_rule(context, min_side, max_side, "crop_chips")
    frames, dev, box_frame, _ = _box_launch("crop_chips", frames, boxes, box_frame, in_place=False)
    n = boxes.shape[0]
    chips = torch.empty((n, chip, chip, 3), device=dev, dtype=torch.uint8)
    windows = torch.empty((n, 3), device=dev, dtype=torch.int32)
    if n:
        with torch.cuda.device(dev):
            desc = _frame_descs(frames, dev)
            N.check(N.lib().wm_crop_chips_u8(N.ptr(desc), len(frames), N.ptr(boxes), N.ptr(box_frame), n, chip, context, min_side,
                                             max_side, N.ptr(chips), N.ptr(windows), N.stream_ptr(dev)))
    return chips, windows


def outline_rects(boxes) -> Tuple[np.ndarray, np.ndarray]:
    """The outline rule's first step on the host (wm_box_outline_rect; no device call): boxes (n,4) xyxy -> ((n,4) int32
    rectangles (l, t, r, b), r and b inclusive, zeros for a skipped box; (n,) bool, True where the box is drawn).  A box
    is skipped here for a non-finite coordinate or r < l or b < t."""
    b = _host_boxes(boxes)
    out = np.zeros((b.shape[0], 4), dtype=np.int32)
    drawn = np.zeros(b.shape[0], dtype=bool)
    fn = N.lib().wm_box_outline_rect
    FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for i in range(b.shape[0]):
        st = fn(b[i].ctypes.data_as(FP), out[i].ctypes.data_as(IP))
        if st < 0:
            N.check(st)
        drawn[i] = st == 0
    return out, drawn


def draw_boxes(frames, boxes: torch.Tensor, labels: torch.Tensor, box_frame=None, width: int = 2, palette=None):
    """Outline every box on its frame, IN PLACE, all in one launch (wm_draw_boxes_u8), and return `frames`.  frames: one
    contiguous (H,W,3) uint8 ROCm frame or a list of them; boxes (n,4) fp32 xyxy in the pixels of their frame, on the
    frames' device; labels (n,) integers (int64 as detect_frames returns them, or int32); box_frame (n,) the frame index of
    each box (None: all in frame 0).  palette: a (P,3) uint8 table, row `label` written as it is (None: DEFAULT_PALETTE).
    The outline rule (include/wm_hip.h): corners truncated toward zero, right and bottom inclusive, a border of `width`
    pixels growing inward, clipped to the frame -- PIL.ImageDraw.rectangle's pixels wherever both sides exceed `width`.
    A box with a non-finite coordinate, an inverted box, a frame index outside the list or a label outside the palette
    draws nothing.  The result is that of drawing the boxes in index order, later over earlier.  Runs on the current
    stream."""
    width = _check_draw_width(width, "draw_boxes")
    pal = _check_palette(palette, "draw_boxes")
    given = frames
    frames, dev, box_frame, labels = _box_launch("draw_boxes", frames, boxes, box_frame, in_place=True, labels=labels)
    n = boxes.shape[0]
    if n:
        with torch.cuda.device(dev):
            desc = _frame_descs(frames, dev)
            pal_d = _pinned_upload(pal.copy(), dev)
            N.check(N.lib().wm_draw_boxes_u8(N.ptr(desc), len(frames), N.ptr(boxes), N.ptr(labels), N.ptr(box_frame), n, N.ptr(pal_d),
                                             pal.shape[0], width, N.stream_ptr(dev)))
    return given


def overlay_size(height: int, width: int, overlay: int) -> Tuple[int, int]:
    """(oh, ow) of detect_frames(overlay=L)'s picture of a height x width frame: preprocess.scaled_size(height, width,
    L / max(height, width)) when the long side exceeds L, else (height, width)."""
    m = max(height, width)
    return preprocess.scaled_size(height, width, overlay / m) if m > overlay else (height, width)
