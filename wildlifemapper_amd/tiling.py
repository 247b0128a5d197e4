"""Large-frame front end: 6000 x 4000 aerial frames (coco_annotations/*.json image sizes) -> overlapping
1024 x 1024 tiles -> the accelerated path -> cross-tile merge of the detections.

The reference has no such step (it down-scales whole frames to 768 px, dataloader_coco.py:288), so there is no behaviour to
match: the checker is oracle/tiling_oracle.py, a numpy restatement of exactly what is done here.
  * tile_origins: the fewest tiles per axis whose neighbours overlap by at least `overlap`, evenly spread, the first and
    last flush with the frame edges (no padding unless the frame is smaller than a tile): 7 x 5 tiles for 6000 x 4000;
  * frame_to_tiles: wm_tile_frames_u8 (cut + ToTensor + Normalize on the GPU) on one frame;
  * merge_tile_records / merge_frames: wm_merge_frames_nms -- detections that survived their own tile's score cut + NMS
    move to frame coordinates and compete in one more class-agnostic NMS (IoU 0.4), per frame;
  * fuse_thr= (merge_frames, detect_frame, detect_frames): opt-in wm_merge_frames_fuse instead -- a keeper absorbs the
    other tiles' views whose intersection over the smaller box exceeds fuse_thr, and reports the union box, so an
    animal cut by a tile seam is counted once with its whole box;
  * detect_frames: a survey -- many frames of any size, device or host -- with the tiles of consecutive frames packed
    into full batches (wm_tile_frames_u8) and one merge per batch for the frames it completes; detect_frame is a survey
    of one frame.
  * scale= / resize= (detect_frame, detect_frames): opt-in resampling to the scale the checkpoint was trained at -- the
    reference shrinks whole frames to a long side of 768 (dataloader_coco.py:288) -- with PIL's bilinear arithmetic on the
    GPU (wm_resample_u8), then the same tile cut and merge in the resampled frame.  Each tile's target size is its content
    extent (min(1024, ow - x0), min(1024, oh - y0)), the reference's content-normalised boxes (augmentation.py:246-258);
    returned boxes are mapped back to source pixels.
  * chips= (detect_frame, detect_frames), crop_chips, chip_windows: opt-in review chips -- one fixed-size crop per
    detection, cut from the source-resolution frame around its box (chip rule: include/wm_hip.h) and resampled with PIL's
    bilinear arithmetic, every chip of the frames a merge completed in one launch (wm_crop_chips_u8).
  * overlay= (detect_frame, detect_frames), draw_boxes, outline_rects, DEFAULT_PALETTE: opt-in survey overlays -- the source
    frame at a size that fits a screen (PIL-exact, wm_resample_u8) with every detection outlined in its class colour
    (outline rule: include/wm_hip.h), the outlines of the frames a merge completed in one launch (wm_draw_boxes_u8).
  * census, nadir_affine: the count a survey is flown for -- the detections of all frames (detect_frames' dicts) go to
    ground coordinates through each frame's georeference and are grouped into individuals, at most one detection of any
    frame per individual (census rule: include/wm_hip.h), by one wm_census launch over the whole survey.
  * coverage, ground_to_pixel, footprint_bounds: the denominator of a density -- a ground grid over the survey, every
    cell with the number of frames that saw its centre (the union of the footprints, its gaps), the census' individuals
    per cell and class, and per individual the number of frames that could have seen it (coverage rule:
    include/wm_hip.h), by wm_coverage_raster and wm_coverage_points.
  * mosaic, mosaic_plan, resampled_georef: the map -- the frames laid onto the coverage's ground grid; every cell takes its
    pixel from the one frame that saw it most vertically (seam rule and sampling: include/wm_hip.h), chosen for all cells
    by one wm_mosaic_plan launch and fetched by wm_mosaic_fill_u8, a chunk of resident frames per launch, so only the
    frames that won a cell are ever loaded; the census' individuals can be outlined on it.
Frame coordinates are fp32: a box coordinate keeps a fractional resolution below 0.01 px up to 65536 px (ulp 2**-8).
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Iterator, List, NamedTuple, Tuple

import numpy as np

import torch

from . import _native as N
from . import preprocess


def _axis_origins(size: int, tile: int, overlap: int) -> List[int]:
    """Fewest tiles whose neighbours overlap by at least `overlap`, spread evenly, first and last flush with the edges."""
    if size <= tile:
        return [0]
    stride = tile - overlap
    if stride <= 0:
        raise ValueError("overlap must be smaller than the tile")
    n = -(-(size - tile) // stride) + 1
    return [(i * (size - tile) + (n - 1) // 2) // (n - 1) for i in range(n)]


def tile_origins(height: int, width: int, tile: int = 1024, overlap: int = 128) -> List[Tuple[int, int]]:
    """(y0, x0) of every tile, row-major."""
    return [(y, x) for y in _axis_origins(height, tile, overlap) for x in _axis_origins(width, tile, overlap)]


def _frame_descs(frames: List[torch.Tensor], device: torch.device) -> torch.Tensor:
    """wm_frame_desc of each contiguous (H,W,3) uint8 device frame -- data pointer, then (height, width) as two int32 in
    one int64 -- uploaded to `device` through pinned memory without blocking the host."""
    desc = np.zeros((len(frames), 2), dtype=np.int64)
    for j, fr in enumerate(frames):
        desc[j, 0] = fr.data_ptr()
        desc[j, 1] = np.array(fr.shape[:2], dtype=np.int32).view(np.int64)[0]
    return torch.from_numpy(desc).pin_memory().to(device, non_blocking=True)


def frame_to_tiles(frame: torch.Tensor, origins: torch.Tensor) -> torch.Tensor:
    """frame (H,W,3) uint8 on a ROCm device, origins (n,2) int32 (y0, x0) on the host or the frame's device ->
    (n,3,1024,1024) fp32."""
    if not frame.is_cuda or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3:
        raise RuntimeError(f"frame_to_tiles: expected an (H,W,3) uint8 ROCm tensor, got {tuple(frame.shape)} {frame.dtype} on {frame.device}")
    frame = frame.contiguous()
    dev = frame.device
    tiles = torch.nn.functional.pad(origins.to(device=dev, dtype=torch.int32), (1, 0))      # (frame 0, y0, x0)
    n = tiles.shape[0]
    out = torch.empty((n, 3, 1024, 1024), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        N.check(N.lib().wm_tile_frames_u8(N.ptr(_frame_descs([frame], dev)), 1, N.ptr(tiles), N.ptr(out), n, N.stream_ptr(dev)))
    return out


def _check_fuse_thr(fuse_thr, what: str):
    """Validate fuse_thr= before any device work: None (the NMS merge) or a number in [0, 1)."""
    if fuse_thr is None:
        return None
    try:
        t = float(fuse_thr)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: fuse_thr {fuse_thr!r} is not a number") from None
    t = float(np.float32(t)) if math.isfinite(t) else t      # the kernel compares in fp32
    if not (math.isfinite(t) and 0.0 <= t < 1.0):
        raise ValueError(f"{what}: fuse_thr {fuse_thr!r} must be in [0, 1) in fp32")
    return t


def merge_frames(records: torch.Tensor, origins: torch.Tensor, frame_tile_offsets, iou_thr: float = 0.4,
                 fuse_thr=None) -> Dict[str, torch.Tensor]:
    """Segmented cross-tile merge (wm_merge_frames_nms).  records (n,51,8) raw per-tile records of several frames,
    origins (n,2) each tile's (y0, x0) in its own frame, frame_tile_offsets (n_frames + 1) host ints: frame f is tiles
    [offsets[f], offsets[f+1]).  Returns 'merged' (n,51,8), the records in frame coordinates with FLAG_MERGED / nms_rank
    of each frame's cross-tile NMS, and the compacted detection list: frame f's survivors in merged order are 'det' /
    'det_tile' [offsets[f] * 51 + k], k < 'det_count'[f].
    fuse_thr (a float in [0, 1)): wm_merge_frames_fuse instead of the NMS (iou_thr unused) -- FLAG_MERGED / nms_rank
    mark the keepers, 'det' carries each keeper's union box, and the result gains 'det_members' (indexed as 'det': 1 + the
    boxes the keeper absorbed) and 'slot_det' (n*51: the frame's list index of the detection a candidate slot belongs
    to, -1 for other slots)."""
    fuse_thr = _check_fuse_thr(fuse_thr, "merge_frames")
    N.require_cuda(records, "records")
    offs = np.ascontiguousarray(np.asarray(frame_tile_offsets, dtype=np.int32))
    n = records.shape[0]
    if offs.ndim != 1 or offs.shape[0] < 2 or int(offs[-1]) != n or tuple(records.shape[1:]) != (N.NUM_QUERIES, 8):
        raise RuntimeError(f"merge_frames: records {tuple(records.shape)} do not match frame_tile_offsets ending at {offs[-1] if offs.size else None}")
    origins = origins.to(device=records.device, dtype=torch.int32).contiguous()
    nf = offs.shape[0] - 1
    nbytes = N.lib().wm_merge_frames_scratch_bytes(n)
    if nbytes < 0:
        N.check(-1)
    dev = records.device
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    merged = torch.empty_like(records)
    det = torch.empty((n * N.NUM_QUERIES, 8), device=dev, dtype=torch.float32)
    det_tile = torch.empty(n * N.NUM_QUERIES, device=dev, dtype=torch.int32)
    det_count = torch.empty(nf, device=dev, dtype=torch.int32)
    import ctypes as C
    if fuse_thr is not None:
        det_members = torch.empty(n * N.NUM_QUERIES, device=dev, dtype=torch.int32)
        slot_det = torch.empty(n * N.NUM_QUERIES, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            N.check(N.lib().wm_merge_frames_fuse(N.ptr(records), N.ptr(origins), offs.ctypes.data_as(C.POINTER(C.c_int32)), nf,
                                                 fuse_thr, N.ptr(scratch), nbytes, N.ptr(merged), N.ptr(det), N.ptr(det_tile),
                                                 N.ptr(det_count), N.ptr(det_members), N.ptr(slot_det), N.stream_ptr(dev)))
        return {"merged": merged, "det": det, "det_tile": det_tile, "det_count": det_count, "det_members": det_members,
                "slot_det": slot_det}
    with torch.cuda.device(dev):
        N.check(N.lib().wm_merge_frames_nms(N.ptr(records), N.ptr(origins), offs.ctypes.data_as(C.POINTER(C.c_int32)), nf, float(iou_thr),
                                            N.ptr(scratch), nbytes, N.ptr(merged), N.ptr(det), N.ptr(det_tile), N.ptr(det_count),
                                            N.stream_ptr(dev)))
    return {"merged": merged, "det": det, "det_tile": det_tile, "det_count": det_count}


def merge_tile_records(records: torch.Tensor, origins: torch.Tensor, iou_thr: float = 0.4) -> torch.Tensor:
    """records (n,51,8) raw per-tile records of one frame (boxes in tile pixels) -> (n,51,8) merged records in frame
    coordinates with FLAG_MERGED / nms_rank of the cross-tile NMS: merge_frames of a one-frame survey."""
    return merge_frames(records, origins, [0, records.shape[0]], iou_thr)["merged"]


def _check_scale(scale, what: str) -> float:
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: scale {scale!r} is not a number") from None
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"{what}: scale {scale!r} must be positive and finite")
    return s


def _check_resample_args(scale, resize, what: str) -> bool:
    """Validate detect_frame(s)' scale= / resize= before any device work.  True if frames are resampled."""
    if scale is not None and resize is not None:
        raise ValueError(f"{what}: scale= and resize= are mutually exclusive")
    if resize is not None:
        try:
            size, max_size = resize
        except (TypeError, ValueError):
            raise ValueError(f"{what}: resize must be (size, max_size), got {resize!r}") from None
        if int(size) <= 0 or (max_size is not None and int(max_size) < 0):
            raise ValueError(f"{what}: resize {resize!r}")
    if scale is not None and not callable(scale):
        _check_scale(scale, what)
    return scale is not None or resize is not None


def resampled_size(index: int, height: int, width: int, scale=None, resize=None) -> Tuple[int, int]:
    """(oh, ow) frame `index` of size height x width is resampled to: resize=(size, max_size) -> preprocess.resized_size
    (the val transform's geometry; (768, 768) is the reference's); scale -> preprocess.scaled_size, scale a float or a
    callable (index, height, width) -> float (per-frame ground sampling distance)."""
    if resize is not None:
        return preprocess.resized_size(height, width, int(resize[0]), int(resize[1] or 0))
    s = scale(index, height, width) if callable(scale) else scale
    return preprocess.scaled_size(height, width, _check_scale(s, f"frame {index}"))


# ---- review chips ----------------------------------------------------------------------------------------------------

CHIP_MAX_SIDE = 1024          # include/wm_hip.h WM_CHIP_MAX_SIDE


def _check_chip(chip, what: str) -> int:
    """Validate a chip size before any device work: an integer multiple of 4 in 16..256."""
    if isinstance(chip, bool) or not isinstance(chip, (int, np.integer)):
        raise ValueError(f"{what}: chip size {chip!r} is not an integer")
    if chip < 16 or chip > 256 or chip % 4:
        raise ValueError(f"{what}: chip size {chip!r} must be a multiple of 4 in 16..256")
    return int(chip)


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


def chip_windows(boxes, context: float = 1.5, min_side: int = 32, max_side: int = CHIP_MAX_SIDE) -> np.ndarray:
    """The chip rule on the host (wm_chip_window; no device call): boxes (n,4) xyxy in frame pixels -> (n,3) int32
    windows (y0, x0, side).  A box with a non-finite coordinate gives (0, 0, 0)."""
    import ctypes as C
    context, min_side, max_side = _check_chip_rule(context, min_side, max_side, "chip_windows")
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.detach().cpu().numpy()
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
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
    frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
    if not frames:
        raise RuntimeError("crop_chips: no frames")
    for i, fr in enumerate(frames):
        if not isinstance(fr, torch.Tensor) or not fr.is_cuda or fr.dtype != torch.uint8 or fr.dim() != 3 or fr.shape[-1] != 3:
            raise RuntimeError(f"crop_chips: frame {i}: expected an (H,W,3) uint8 ROCm tensor")
    dev = frames[0].device
    frames = [fr.contiguous() for fr in frames]
    N.require_cuda(boxes, "crop_chips: boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.device != dev or any(fr.device != dev for fr in frames):
        raise RuntimeError(f"crop_chips: boxes {tuple(boxes.shape)} on {boxes.device}, frames on {dev}: expected (n,4) on one device")
    n = boxes.shape[0]
    if box_frame is not None:
        box_frame = torch.as_tensor(box_frame).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(box_frame.shape) != (n,):
            raise RuntimeError(f"crop_chips: box_frame {tuple(box_frame.shape)} for {n} boxes")
    chips = torch.empty((n, chip, chip, 3), device=dev, dtype=torch.uint8)
    windows = torch.empty((n, 3), device=dev, dtype=torch.int32)
    if n:
        with torch.cuda.device(dev):
            desc = _frame_descs(frames, dev)
            N.check(N.lib().wm_crop_chips_u8(N.ptr(desc), len(frames), N.ptr(boxes), N.ptr(box_frame), n, chip, context, min_side,
                                             max_side, N.ptr(chips), N.ptr(windows), N.stream_ptr(dev)))
    return chips, windows


# ---- overlays --------------------------------------------------------------------------------------------------------

DRAW_MAX_WIDTH, DRAW_MAX_PALETTE = 16, 256          # include/wm_hip.h WM_DRAW_MAX_WIDTH, WM_DRAW_MAX_PALETTE
OVERLAY_MIN, OVERLAY_MAX = 64, 8192                 # detect_frames(overlay=L): the long side of the picture

# The project's own colours for labels 0..8, (R, G, B) for an RGB frame: the model's 0-based labels and the reference's
# keys 1..8 are both covered.  Rows are written as they are, whatever the channel order of the frame they are drawn on.
DEFAULT_PALETTE = np.array([(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
                            (70, 240, 240), (240, 50, 230), (255, 255, 255)], dtype=np.uint8)
DEFAULT_PALETTE.setflags(write=False)


def _check_draw_width(width, what: str) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)):
        raise ValueError(f"{what}: width {width!r} is not an integer")
    if not (1 <= width <= DRAW_MAX_WIDTH):
        raise ValueError(f"{what}: width {width!r} must be in 1..{DRAW_MAX_WIDTH}")
    return int(width)


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


def _check_overlay(overlay, what: str) -> int:
    """Validate an overlay size before any device work: an integer in 64..8192."""
    if isinstance(overlay, bool) or not isinstance(overlay, (int, np.integer)):
        raise ValueError(f"{what}: overlay size {overlay!r} is not an integer")
    if not (OVERLAY_MIN <= overlay <= OVERLAY_MAX):
        raise ValueError(f"{what}: overlay size {overlay!r} must be in {OVERLAY_MIN}..{OVERLAY_MAX}")
    return int(overlay)


def outline_rects(boxes) -> Tuple[np.ndarray, np.ndarray]:
    """The outline rule's first step on the host (wm_box_outline_rect; no device call): boxes (n,4) xyxy -> ((n,4) int32
    rectangles (l, t, r, b), r and b inclusive, zeros for a skipped box; (n,) bool, True where the box is drawn).  A box
    is skipped here for a non-finite coordinate or r < l or b < t."""
    import ctypes as C
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.detach().cpu().numpy()
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
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
    frames = [frames] if isinstance(frames, torch.Tensor) else list(frames)
    if not frames:
        raise RuntimeError("draw_boxes: no frames")
    for i, fr in enumerate(frames):
        if not isinstance(fr, torch.Tensor) or not fr.is_cuda or fr.dtype != torch.uint8 or fr.dim() != 3 or fr.shape[-1] != 3:
            raise RuntimeError(f"draw_boxes: frame {i}: expected an (H,W,3) uint8 ROCm tensor")
        if not fr.is_contiguous():
            raise RuntimeError(f"draw_boxes: frame {i} is not contiguous (it is drawn on in place)")
    dev = frames[0].device
    N.require_cuda(boxes, "draw_boxes: boxes")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.device != dev or any(fr.device != dev for fr in frames):
        raise RuntimeError(f"draw_boxes: boxes {tuple(boxes.shape)} on {boxes.device}, frames on {dev}: expected (n,4) on one device")
    n = boxes.shape[0]
    labels = torch.as_tensor(labels)
    if tuple(labels.shape) != (n,) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise RuntimeError(f"draw_boxes: labels {tuple(labels.shape)} {labels.dtype} for {n} boxes: expected (n,) integers")
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    if box_frame is not None:
        box_frame = torch.as_tensor(box_frame).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(box_frame.shape) != (n,):
            raise RuntimeError(f"draw_boxes: box_frame {tuple(box_frame.shape)} for {n} boxes")
    if n:
        with torch.cuda.device(dev):
            desc = _frame_descs(frames, dev)
            pal_d = torch.from_numpy(pal.copy()).pin_memory().to(dev, non_blocking=True)
            N.check(N.lib().wm_draw_boxes_u8(N.ptr(desc), len(frames), N.ptr(boxes), N.ptr(labels), N.ptr(box_frame), n, N.ptr(pal_d),
                                             pal.shape[0], width, N.stream_ptr(dev)))
    return given


def overlay_size(height: int, width: int, overlay: int) -> Tuple[int, int]:
    """(oh, ow) of detect_frames(overlay=L)'s picture of a height x width frame: preprocess.scaled_size(height, width,
    L / max(height, width)) when the long side exceeds L, else (height, width)."""
    m = max(height, width)
    return preprocess.scaled_size(height, width, overlay / m) if m > overlay else (height, width)


def detect_frame(model, frame: torch.Tensor, overlap: int = 128, batch: int = 16, iou_thr: float = 0.4, scale=None,
                 resize=None, fuse_thr=None, chips=None, chip_context: float = 1.5, chip_min_side: int = 32, overlay=None,
                 overlay_width: int = 2, overlay_palette=None) -> Dict[str, torch.Tensor]:
    """One frame -> merged detections {'boxes' (k,4) frame xyxy, 'scores', 'labels', 'tile', 'origins', 'records'} in
    merged-NMS order: detect_frames on a survey of this one frame (a callable scale is called with index 0)."""
    return next(detect_frames(model, [frame], overlap, batch, iou_thr, scale=scale, resize=resize, fuse_thr=fuse_thr, chips=chips,
                              chip_context=chip_context, chip_min_side=chip_min_side, overlay=overlay, overlay_width=overlay_width,
                              overlay_palette=overlay_palette))


# ---- survey: many frames of any size ---------------------------------------------------------------------------------

class SurveyBatch(NamedTuple):
    segments: List[Tuple[int, int, int]]     # (frame index, first tile, end tile) in batch order
    completes: List[int]                     # frames whose last tile is in this batch


def plan_batches(tile_counts: Iterable[int], batch: int) -> Iterator[SurveyBatch]:
    """Pack the tiles of consecutive frames into batches of `batch`: every tile of every frame once, in frame order, every
    batch full except the last.  Lazy: a frame's tile count is read only when a batch needs its tiles."""
    if batch <= 0:
        raise ValueError(f"plan_batches: batch {batch}")
    segs: List[Tuple[int, int, int]] = []
    done: List[int] = []
    fill = 0
    for f, n in enumerate(tile_counts):
        if n <= 0:
            raise ValueError(f"plan_batches: frame {f} has {n} tiles")
        t = 0
        while t < n:
            take = min(batch - fill, n - t)
            segs.append((f, t, t + take))
            t += take
            fill += take
            if t == n:
                done.append(f)
            if fill == batch:
                yield SurveyBatch(segs, done)
                segs, done, fill = [], [], 0
    if segs:
        yield SurveyBatch(segs, done)


class _Frame:
    __slots__ = ("data", "height", "width", "origins", "origins_dev", "ready", "records", "scale_xy", "source")

    def __init__(self, data, height, width, origins, ready, scale_xy=None, source=None):
        self.data, self.height, self.width, self.origins, self.ready = data, height, width, origins, ready
        self.source = source                  # chips= / overlay= only: the source-resolution device frame, kept until finish()
        self.records: List[torch.Tensor] = []
        self.origins_dev = None
        self.scale_xy = scale_xy              # resampled mode: (sx, sy) = float32(W / ow), float32(H / oh); else None


def _as_frame_array(frame, i: int, device: torch.device, who: str = "detect_frames"):
    """Validate one survey frame as frame_to_tiles does: (H,W,3) uint8.  Returns (device tensor or None, host tensor or None)."""
    if isinstance(frame, np.ndarray):
        frame = torch.from_numpy(frame)
    if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3 \
            or frame.shape[0] <= 0 or frame.shape[1] <= 0:
        what = f"{tuple(frame.shape)} {frame.dtype} on {frame.device}" if isinstance(frame, torch.Tensor) else type(frame).__name__
        raise RuntimeError(f"{who}: frame {i}: expected an (H,W,3) uint8 tensor or array, got {what}")
    if frame.is_cuda:
        if frame.device != device:
            raise RuntimeError(f"{who}: frame {i} is on {frame.device}, the survey runs on {device}")
        return frame.contiguous(), None
    if frame.device.type != "cpu":
        raise RuntimeError(f"{who}: frame {i} is on {frame.device}")
    return None, frame.contiguous()


@torch.no_grad()
def detect_frames(model, frames: Iterable, overlap: int = 128, batch: int = 16, iou_thr: float = 0.4, scale=None,
                  resize=None, fuse_thr=None, chips=None, chip_context: float = 1.5, chip_min_side: int = 32, overlay=None,
                  overlay_width: int = 2, overlay_palette=None) -> Iterator[Dict[str, torch.Tensor]]:
    """Survey of frames of any sizes ((H,W,3) uint8 ROCm tensors, CPU tensors or numpy arrays) -> one dict per frame, in
    input order, with detect_frame's keys and values.  Tiles of consecutive frames fill batches of `batch` (plan_batches);
    after each batch one wm_merge_frames_nms covers the frames it completed.  Host frames go through one pinned staging
    buffer (grown to the largest frame) and a copy stream: the next frame's upload overlaps the current batches, ordered
    by events.  A frame's result is yielded once the batch after its merge is queued, so the host never waits on the
    batch it just launched.

    scale= (a float, or a callable (frame index, H, W) -> float) or resize=(size, max_size), mutually exclusive: each frame
    is first resampled to resampled_size(...) on the GPU (wm_resample_u8; device frames on the current stream, host frames
    on the copy stream after their upload) and tiled in the resampled frame, each tile's target size its content extent.
    'boxes' are then in source-frame pixels (merged boxes * (sx, sy) in fp32, sx = float32(W / ow), sy = float32(H / oh));
    'records' and 'origins' stay in resampled-frame pixels, and the dict gains 'resampled_size' = (oh, ow).

    fuse_thr= (a float in [0, 1)): the frames are merged by wm_merge_frames_fuse (merge_frames(fuse_thr=...)) instead of
    the NMS: 'boxes' are the keepers' union boxes (mapped back to source pixels as above when resampling), and the dict
    gains 'members' (k,) int64 -- 1 + the views each detection absorbed -- and 'slot_det' (n,51) int64, aligned with
    'records': the index of the detection each candidate slot belongs to, -1 for other slots.

    chips= (a multiple of 4 in 16..256; chip_context, chip_min_side: crop_chips' context and min_side): every detection
    also comes with a review chip, and the dict gains 'chips' (k,S,S,3) uint8, 'chip_windows' (k,3) int32 (y0, x0, side)
    and 'chip_boxes' (k,4) fp32, the detection's box in chip pixels = (boxes - (x0, y0, x0, y0)) * float32(S / side) in
    fp32; all three aligned with 'boxes' (the union boxes when fusing).  Chips are cut from the SOURCE frame at 'boxes',
    when resampling too, by one wm_crop_chips_u8 launch for the frames a merge completed, queued on the main stream once
    their detection counts have reached the host (no detections: an empty tensor and no launch).  A frame is therefore
    kept until its result is yielded instead of being released at its last tile cut, and in resampled mode its source is
    kept beside its resample instead of being released once the resample is queued: one extra source-resolution frame
    (H * W * 3 bytes, 72 MB at 6000 x 4000) of device memory per frame in flight.  chips=None: none of this.

    overlay= (an integer L in 64..8192; overlay_width, overlay_palette: draw_boxes' width and palette): every frame also
    comes with the picture a reviewer opens first, and the dict gains 'overlay' (oh,ow,3) uint8 -- the SOURCE frame at
    (oh, ow) = overlay_size(H, W, L) with every detection outlined in its label's colour -- and 'overlay_boxes' (k,4) fp32
    = boxes * (float32(ow / W), float32(oh / H), float32(ow / W), float32(oh / H)) in fp32, aligned with 'boxes' (the
    union boxes when fusing, source-pixel boxes when resampling).  A frame whose long side exceeds L is resampled as
    PIL.Image.resize((ow, oh), BILINEAR) does (wm_resample_u8), any other is copied; detections are drawn in the order
    they are listed, the most confident first, later over earlier.  One resample (or copy) per frame and one
    wm_draw_boxes_u8 launch for the frames a merge completed, queued where the chips' launch is queued.  The source frame
    is kept exactly as chips= keeps it, at the same memory cost (once, when both are set).  overlay=None: no key, no
    launch, no retained frame."""
    from .engine import split_records
    import ctypes as C
    if batch <= 0:
        raise ValueError(f"detect_frames: batch {batch}")
    resampling = _check_resample_args(scale, resize, "detect_frames")
    fuse_thr = _check_fuse_thr(fuse_thr, "detect_frames")
    if chips is not None:
        chips = _check_chip(chips, "detect_frames")
        chip_context, chip_min_side, _ = _check_chip_rule(chip_context, chip_min_side, CHIP_MAX_SIDE, "detect_frames")
    if overlay is not None:
        overlay = _check_overlay(overlay, "detect_frames")
        overlay_width = _check_draw_width(overlay_width, "detect_frames")
        overlay_palette = _check_palette(overlay_palette, "detect_frames")
    keep_source = chips is not None or overlay is not None
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    staged: Dict[int, _Frame] = {}
    pinned = [None, None]                     # staging buffer, event of the last copy out of it
    copy = [None]                             # copy stream, made for the first host frame
    it = iter(frames)

    def upload(h, H: int, W: int, resample_to=None):
        """Host frame -> device frame through the pinned staging buffer on the copy stream; resample_to=(oh, ow): the
        upload is resampled there too, after the copy.  Returns the device frame, the event its use waits for and the
        uploaded source frame."""
        nbytes = H * W * 3
        if pinned[1] is not None:
            pinned[1].synchronize()           # the previous upload has left the staging buffer
        if pinned[0] is None or pinned[0].numel() < nbytes:
            pinned[0] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        buf = pinned[0][:nbytes]
        buf.copy_(h.view(-1))
        if copy[0] is None:
            copy[0] = torch.cuda.Stream(device)
        with torch.cuda.stream(copy[0]):
            d = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
            d.view(-1).copy_(buf, non_blocking=True)
            src = d
            ready = uploaded = torch.cuda.Event()
            uploaded.record(copy[0])
            if resample_to is not None:       # the uploaded source goes once its resample is queued (chips= / overlay= keep it)
                d = preprocess.resample_u8(d, resample_to)
                ready = torch.cuda.Event()
                ready.record(copy[0])
        d.record_stream(torch.cuda.current_stream(device))
        if keep_source:
            src.record_stream(torch.cuda.current_stream(device))
        pinned[1] = uploaded
        return d, ready, src

    def stage(i: int) -> bool:
        try:
            fr = next(it)
        except StopIteration:
            return False
        d, h = _as_frame_array(fr, i, device)
        src = d if d is not None else h
        H, W = int(src.shape[0]), int(src.shape[1])
        if resampling:
            oh, ow = resampled_size(i, H, W, scale, resize)          # a bad per-frame scale raises before any device work
        if device is None:
            raise RuntimeError("detect_frames: no ROCm device (there is no CPU fallback in wildlifemapper_amd)")
        if resampling:                        # the resampled frame is what gets tiled; a caller's device frame is only read
            size = None if (oh, ow) == (H, W) else (oh, ow)
            if d is None:
                d, ready, src = upload(h, H, W, size)
            else:
                src = d
                d, ready = (d if size is None else preprocess.resample_u8(d, size)), None
            sxy = (float(np.float32(W / ow)), float(np.float32(H / oh)))
            staged[i] = _Frame(d, oh, ow, tile_origins(oh, ow, 1024, overlap), ready, sxy, src if keep_source else None)
            return True
        org = tile_origins(H, W, 1024, overlap)
        ready = None
        if d is None:
            d, ready, _ = upload(h, H, W)
        staged[i] = _Frame(d, H, W, org, ready, None, d if keep_source else None)
        return True

    def tile_counts():
        i = 0
        have = stage(0)
        while have:
            have_next = stage(i + 1)          # upload of frame i+1 overlaps the batches of frame i
            yield len(staged[i].origins)
            i += 1
            have = have_next

    def finish(pending):
        out, frames_done, offs = pending
        out["ready"].synchronize()
        counts = out["count_host"].tolist()
        done = []
        for j, f in enumerate(frames_done):
            fr = staged.pop(f)
            s0, n = offs[j] * N.NUM_QUERIES, offs[j + 1] - offs[j]
            k = counts[j]
            det = split_records(out["det"][s0:s0 + k].view(k, 1, 8))
            res = {"boxes": det["boxes"].reshape(k, 4), "scores": det["scores"].reshape(k), "labels": det["labels"].reshape(k),
                   "tile": out["det_tile"][s0:s0 + k].to(torch.int64), "origins": fr.origins_dev,
                   "records": out["merged"][offs[j]:offs[j] + n]}
            if fuse_thr is not None:
                res["members"] = out["det_members"][s0:s0 + k].to(torch.int64)
                res["slot_det"] = out["slot_det"][s0:s0 + n * N.NUM_QUERIES].view(n, N.NUM_QUERIES).to(torch.int64)
            if fr.scale_xy is not None:       # resampled-frame pixels -> source-frame pixels, one fp32 multiply per coordinate
                b = res["boxes"]
                src = torch.empty_like(b)
                src[:, 0::2] = b[:, 0::2] * fr.scale_xy[0]
                src[:, 1::2] = b[:, 1::2] * fr.scale_xy[1]
                res["boxes"] = src
                res["resampled_size"] = (fr.height, fr.width)
            if keep_source:
                done.append((fr, res))
            else:
                yield res
        if done:
            if chips is not None:
                add_chips(done)
            if overlay is not None:
                add_overlays(done)
            for fr, res in done:
                fr.source = None
                yield res

    def add_chips(done):
        """One crop launch for every detection of the frames of one merge, cut from the source frames at 'boxes'."""
        S = chips
        ks = [res["boxes"].shape[0] for _, res in done]
        if sum(ks):
            boxes = torch.cat([res["boxes"] for _, res in done]).contiguous()
            idx = torch.from_numpy(np.repeat(np.arange(len(done), dtype=np.int32), ks)).pin_memory().to(device, non_blocking=True)
            all_chips, all_win = crop_chips([fr.source for fr, _ in done], boxes, idx, S, chip_context, chip_min_side)
        else:
            all_chips = torch.empty((0, S, S, 3), device=device, dtype=torch.uint8)
            all_win = torch.empty((0, 3), device=device, dtype=torch.int32)
        pos = 0
        for (fr, res), k in zip(done, ks):
            win = all_win[pos:pos + k]
            res["chips"], res["chip_windows"] = all_chips[pos:pos + k], win
            side = win[:, 2].to(torch.float64)
            zoom = torch.where(side > 0, S / side.clamp(min=1), torch.zeros_like(side)).to(torch.float32)    # float32(S / side)
            org = win[:, [1, 0, 1, 0]].to(torch.float32)
            res["chip_boxes"] = (res["boxes"] - org) * zoom[:, None]
            pos += k

    def add_overlays(done):
        """One resample (or copy) of each source frame of one merge, then one draw launch for all their detections."""
        pics, ks = [], []
        for fr, res in done:
            H, W = int(fr.source.shape[0]), int(fr.source.shape[1])
            oh, ow = overlay_size(H, W, overlay)
            pics.append(fr.source.clone() if (oh, ow) == (H, W) else preprocess.resample_u8(fr.source, (oh, ow)))
            b = res["boxes"]
            ob = torch.empty_like(b)
            ob[:, 0::2] = b[:, 0::2] * float(np.float32(ow / W))
            ob[:, 1::2] = b[:, 1::2] * float(np.float32(oh / H))
            res["overlay"], res["overlay_boxes"] = pics[-1], ob
            ks.append(b.shape[0])
        if sum(ks):
            idx = torch.from_numpy(np.repeat(np.arange(len(done), dtype=np.int32), ks)).pin_memory().to(device, non_blocking=True)
            draw_boxes(pics, torch.cat([res["overlay_boxes"] for _, res in done]).contiguous(),
                       torch.cat([res["labels"] for _, res in done]), idx, overlay_width, overlay_palette)

    pending = None
    main = None
    for b in plan_batches(tile_counts(), batch):
        if main is None:
            main = torch.cuda.current_stream(device)
        used = list(dict.fromkeys(f for f, _, _ in b.segments))
        local = {f: j for j, f in enumerate(used)}
        for f in used:
            if staged[f].ready is not None:
                main.wait_event(staged[f].ready)
                staged[f].ready = None
        desc_d = _frame_descs([staged[f].data for f in used], device)
        tiles = np.array([(local[f], *staged[f].origins[t]) for f, t0, t1 in b.segments for t in range(t0, t1)], dtype=np.int32)
        tiles_d = torch.from_numpy(tiles).pin_memory().to(device, non_blocking=True)
        n = tiles.shape[0]
        x = torch.empty((n, 3, 1024, 1024), device=device, dtype=torch.float32)
        N.check(N.lib().wm_tile_frames_u8(N.ptr(desc_d), len(used), N.ptr(tiles_d), N.ptr(x), n, N.stream_ptr(device)))
        if resampling:                        # each tile's content extent (w, h): boxes normalised to the content
            ext = np.array([(min(1024, staged[f].width - o[1]), min(1024, staged[f].height - o[0]))
                            for f, t0, t1 in b.segments for o in staged[f].origins[t0:t1]], dtype=np.float32)
            rec = model.detect(x, torch.from_numpy(ext).pin_memory().to(device, non_blocking=True))["records"]
        else:
            rec = model.detect(x)["records"]
        pos = 0
        for f, t0, t1 in b.segments:
            staged[f].records.append(rec[pos:pos + t1 - t0])
            pos += t1 - t0
        for f in b.completes:
            staged[f].data = None             # last tile cut: the frame is no longer needed
        if pending is not None:
            yield from finish(pending)
            pending = None
        if b.completes:
            offs = [0]
            for f in b.completes:
                offs.append(offs[-1] + len(staged[f].origins))
            recs = torch.cat([r for f in b.completes for r in staged[f].records])
            org_all = torch.from_numpy(np.array([o for f in b.completes for o in staged[f].origins], dtype=np.int32)).pin_memory()
            org_d = org_all.to(device, non_blocking=True)
            for j, f in enumerate(b.completes):
                staged[f].records = []
                staged[f].origins_dev = org_d[offs[j]:offs[j + 1]]
            out = merge_frames(recs, org_d, offs, iou_thr, fuse_thr)
            out["count_host"] = torch.empty(len(b.completes), dtype=torch.int32, pin_memory=True)
            out["count_host"].copy_(out["det_count"], non_blocking=True)
            out["ready"] = torch.cuda.Event()
            out["ready"].record(main)
            pending = (out, list(b.completes), offs)
    if pending is not None:
        yield from finish(pending)


# ---- census ----------------------------------------------------------------------------------------------------------

CENSUS_MAX_DETS = N.CENSUS_MAX_DETS           # include/wm_hip.h WM_CENSUS_MAX_DETS
CENSUS_CLASSES = 7                            # 'class_counts': the model's labels 0..6 (box_decoder.py:50, 6 + 1 classes)


def _check_radius(radius, what: str) -> float:
    """Validate radius= before any device work: a finite number >= 0 whose square is finite in double."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: radius {radius!r} is not a number") from None
    if not (math.isfinite(r) and r >= 0.0 and math.isfinite(r * r)):
        raise ValueError(f"{what}: radius {radius!r} must be finite and >= 0, with a finite square")
    return r


def _check_georef(georef, what: str) -> np.ndarray:
    """(F,2,3) float64, C-contiguous: rows (a0, a1, a2) and (a3, a4, a5) of every frame.  Values are not checked: a
    georeference that is not finite makes its frame's detections invalid (the census rule)."""
    if isinstance(georef, torch.Tensor):
        georef = georef.detach().cpu().numpy()
    try:
        g = np.ascontiguousarray(np.asarray(georef, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: georef is not an array of numbers") from None
    if g.size == 0 and g.ndim <= 1:
        g = g.reshape(0, 2, 3)
    if g.ndim != 3 or g.shape[1:] != (2, 3):
        raise ValueError(f"{what}: georef of shape {g.shape}: expected (F, 2, 3)")
    return g


def nadir_affine(height, width, centre, gsd, yaw_deg=0.0) -> np.ndarray:
    """Georeference of a nadir frame, (2,3) float64 for census(): [[a0, a1, a2], [a3, a4, a5]], X = a0*x + a1*y + a2 east
    and Y = a3*x + a4*y + a5 north, in metres, of the pixel position (x, y).  centre = (E, N) is the ground position of pixel
    (width / 2, height / 2), gsd the metres per pixel, yaw_deg the heading of the image's up direction, clockwise from
    north: at 0 right is east and down is south, at 90 up is east.  Host only, in double."""
    H, W, gsd, yaw = float(height), float(width), float(gsd), float(yaw_deg)
    E, Nn = (float(v) for v in centre)
    if not (H > 0 and W > 0 and math.isfinite(H) and math.isfinite(W)):
        raise ValueError(f"nadir_affine: height {height!r}, width {width!r}")
    if not (math.isfinite(gsd) and gsd > 0 and math.isfinite(yaw) and math.isfinite(E) and math.isfinite(Nn)):
        raise ValueError(f"nadir_affine: gsd {gsd!r} must be finite and > 0, centre and yaw_deg finite")
    psi = math.radians(yaw)
    c, sn = math.cos(psi), math.sin(psi)
    a0, a1 = gsd * c, -gsd * sn
    a3, a4 = -gsd * sn, -gsd * c
    return np.array([[a0, a1, E - (a0 * W / 2 + a1 * H / 2)],
                     [a3, a4, Nn - (a3 * W / 2 + a4 * H / 2)]], dtype=np.float64)


def census(results, georef, radius, same_class: bool = False) -> Dict[str, object]:
    """Count each animal once across overlapping frames (wm_census; rule: include/wm_hip.h).  results: an iterable (a
    generator is fine) of the dicts detect_frames yields -- 'boxes' (k,4) fp32, 'scores' (k,), 'labels' (k,) are used as
    they come (union boxes when fusing, source-pixel boxes when resampling); georef (F,2,3) float64, an array or a
    sequence of nadir_affine's results: result i pairs with georef[i].  radius: metres; a detection joins the nearest
    individual within it that has no member of the detection's own frame (same_class: and whose keeper has its label),
    else it founds one.  Everything is concatenated on the device; one wm_census launch on the current stream and one
    small copy of the count (which waits for it).  Returns, with k individuals out of n detections:
      'count' k (int), 'individual' (n,) int64 (-1: invalid detection), 'det_points' (n,2) float64 ground points (NaN:
      invalid), 'det_frame' (n,) int64, 'det_offsets' host list of F + 1 (result i is detections [o[i], o[i+1]));
      per individual, from its keeper (its highest-priority member): 'keeper' (k,) int64 index into the n detections,
      'points' (k,2) float64, 'scores', 'labels', 'frame' (k,); 'members' (k,) int64; 'class_counts' (7,) int64, the
      bincount of the keepers' labels 0..6."""
    what = "census"
    radius = _check_radius(radius, what)
    g = _check_georef(georef, what)
    results = list(results)
    if len(results) != g.shape[0]:
        raise ValueError(f"{what}: {len(results)} results for {g.shape[0]} georeferences")
    dev = None
    for i, res in enumerate(results):
        try:
            b, sc, lb = res["boxes"], res["scores"], res["labels"]
        except (TypeError, KeyError):
            raise ValueError(f"{what}: result {i} has no 'boxes', 'scores' and 'labels'") from None
        if not all(isinstance(t, torch.Tensor) for t in (b, sc, lb)) or b.dim() != 2 or b.shape[1] != 4 or \
                tuple(sc.shape) != (b.shape[0],) or tuple(lb.shape) != (b.shape[0],):
            raise ValueError(f"{what}: result {i}: expected boxes (k,4), scores (k,) and labels (k,) tensors")
        dev = b.device if dev is None else dev
        if b.device != dev or sc.device != dev or lb.device != dev:
            raise ValueError(f"{what}: result {i} is on {b.device}, earlier ones on {dev}")
    ks = [int(res["boxes"].shape[0]) for res in results]
    offs = [0]
    for k in ks:
        offs.append(offs[-1] + k)
    n = offs[-1]
    if n > CENSUS_MAX_DETS:
        raise ValueError(f"{what}: {n} detections exceed {CENSUS_MAX_DETS}")
    dev = torch.device("cpu") if dev is None else dev
    i64 = dict(device=dev, dtype=torch.int64)
    if n == 0:
        return {"count": 0, "individual": torch.empty(0, **i64), "keeper": torch.empty(0, **i64),
                "points": torch.empty((0, 2), device=dev, dtype=torch.float64),
                "det_points": torch.empty((0, 2), device=dev, dtype=torch.float64),
                "scores": torch.empty(0, device=dev, dtype=torch.float32), "labels": torch.empty(0, **i64),
                "frame": torch.empty(0, **i64), "members": torch.empty(0, **i64), "det_frame": torch.empty(0, **i64),
                "det_offsets": offs, "class_counts": torch.zeros(CENSUS_CLASSES, **i64)}
    boxes = torch.cat([res["boxes"] for res in results]).contiguous()
    N.require_cuda(boxes, f"{what}: boxes")
    scores = torch.cat([res["scores"] for res in results]).contiguous()
    N.require_cuda(scores, f"{what}: scores")
    labels_in = torch.cat([res["labels"] for res in results])
    labels = labels_in.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        frame = torch.from_numpy(np.repeat(np.arange(len(ks), dtype=np.int32), ks)).pin_memory().to(dev, non_blocking=True)
        g_d = torch.from_numpy(g.reshape(-1, 6)).pin_memory().to(dev, non_blocking=True)
        nbytes = N.lib().wm_census_scratch_bytes(n)
        if nbytes < 0:
            N.check(-1)
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        points = torch.empty((n, 2), device=dev, dtype=torch.float64)
        individual = torch.empty(n, device=dev, dtype=torch.int32)
        keeper = torch.empty(n, device=dev, dtype=torch.int32)
        members = torch.empty(n, device=dev, dtype=torch.int32)
        count = torch.empty(2, device=dev, dtype=torch.int32)
        N.check(N.lib().wm_census(N.ptr(boxes), N.ptr(scores), N.ptr(labels), N.ptr(frame), n, N.ptr(g_d), g.shape[0], radius,
                                  N.CENSUS_SAME_CLASS if same_class else 0, N.ptr(scratch), nbytes, N.ptr(points),
                                  N.ptr(individual), N.ptr(keeper), N.ptr(members), N.ptr(count), N.stream_ptr(dev)))
        k, status = count.cpu().tolist()
    if status & N.CENSUS_UNSOLVED:
        raise RuntimeError(f"{what}: wm_census left detections undecided (status {status})")
    keeper = keeper[:k].to(torch.int64)
    klab = labels_in[keeper]
    ok = (klab >= 0) & (klab < CENSUS_CLASSES)
    det_frame = frame.to(torch.int64)
    return {"count": k, "individual": individual.to(torch.int64), "keeper": keeper, "points": points[keeper],
            "det_points": points, "scores": scores[keeper], "labels": klab, "frame": det_frame[keeper],
            "members": members[:k].to(torch.int64), "det_frame": det_frame, "det_offsets": offs,
            "class_counts": torch.bincount(klab[ok].to(torch.int64), minlength=CENSUS_CLASSES)}


# ---- coverage --------------------------------------------------------------------------------------------------------

COVERAGE_MAX_SIDE = N.COVERAGE_MAX_SIDE       # include/wm_hip.h WM_COVERAGE_MAX_SIDE
COVERAGE_MAX_CELLS = N.COVERAGE_MAX_CELLS     # WM_COVERAGE_MAX_CELLS
COVERAGE_MAX_FRAMES = N.COVERAGE_MAX_FRAMES   # WM_COVERAGE_MAX_FRAMES


def _check_cell(cell, what: str) -> float:
    """Validate cell= before any device work: a finite number > 0."""
    if isinstance(cell, (str, bytes)):
        raise ValueError(f"{what}: cell {cell!r} is not a number")
    try:
        c = float(cell)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: cell {cell!r} is not a number") from None
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"{what}: cell {cell!r} must be finite and > 0")
    return c


def _check_sizes(sizes, n_frames: int, what: str) -> np.ndarray:
    """(F,2) int32, C-contiguous: (height, width) of every frame, one per georeference."""
    if isinstance(sizes, torch.Tensor):
        sizes = sizes.detach().cpu().numpy()
    try:
        a = np.asarray(sizes)
        if a.size == 0 and a.ndim <= 1:
            a = a.reshape(0, 2)
        if a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and np.all(a == np.floor(a))):
            raise TypeError
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise TypeError
        s = np.ascontiguousarray(a.astype(np.int32))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: sizes is not an array of whole numbers that fit int32") from None
    if s.ndim != 2 or s.shape[1] != 2:
        raise ValueError(f"{what}: sizes of shape {s.shape}: expected (F, 2), (height, width) per frame")
    if s.shape[0] != n_frames:
        raise ValueError(f"{what}: {s.shape[0]} sizes for {n_frames} georeferences")
    return s


def _check_grid(x0, y0, gx, gy, cell: float, what: str, name: str = "bounds"):
    """Validate a grid against the limits of include/wm_hip.h; the message says what to do about a grid that is too large."""
    try:
        fx, fy = float(x0), float(y0)
        ix, iy = int(gx), int(gy)
        if ix != gx or iy != gy:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} {(x0, y0, gx, gy)!r}: expected (x0, y0, gx, gy), two numbers and two whole numbers") from None
    if not (math.isfinite(fx) and math.isfinite(fy)):
        raise ValueError(f"{what}: {name}: origin ({x0!r}, {y0!r}) is not finite")
    if ix < 1 or iy < 1:
        raise ValueError(f"{what}: {name}: a grid of {ix} x {iy} cells; gx and gy must be at least 1")
    if ix > COVERAGE_MAX_SIDE or iy > COVERAGE_MAX_SIDE or ix * iy > COVERAGE_MAX_CELLS:
        raise ValueError(f"{what}: {name}: a grid of {ix} x {iy} cells at cell {cell!r} exceeds {COVERAGE_MAX_SIDE} cells a side "
                         f"or {COVERAGE_MAX_CELLS} cells in all: choose a larger cell")
    return fx, fy, ix, iy


def ground_to_pixel(georef) -> np.ndarray:
    """The inverse of census()'s georeferences: (F,2,3) float64 [[a0, a1, a2], [a3, a4, a5]] (pixel -> ground) gives (F,2,3)
    float64 [[b0, b1, b2], [b3, b4, b5]] (ground -> pixel), x = b0*X + b1*Y + b2, y = b3*X + b4*Y + b5; a single (2,3)
    gives a (2,3).  Host only, in double, in this order: det = a0*a4 - a1*a3; b0 = a4/det, b1 = -a1/det, b3 = -a3/det,
    b4 = a0/det; b2 = -(b0*a2 + b1*a5), b5 = -(b3*a2 + b4*a5).  A frame that is singular (det == 0) or not finite, in
    its input or its inverse, gives a row of NaN: such a frame sees nothing (coverage rule: include/wm_hip.h)."""
    g = np.asarray(georef, dtype=np.float64) if not isinstance(georef, torch.Tensor) else georef.detach().cpu().numpy().astype(np.float64)
    single = g.ndim == 2
    g = _check_georef(g[None] if single else g, "ground_to_pixel")
    a0, a1, a2, a3, a4, a5 = (g[:, r, c] for r in range(2) for c in range(3))
    out = np.empty_like(g)
    with np.errstate(all="ignore"):
        det = a0 * a4 - a1 * a3
        b0, b1, b3, b4 = a4 / det, -a1 / det, -a3 / det, a0 / det
        b2 = -(b0 * a2 + b1 * a5)
        b5 = -(b3 * a2 + b4 * a5)
        out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = b0, b1, b2
        out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = b3, b4, b5
        bad = ~(np.isfinite(g).all(axis=(1, 2)) & np.isfinite(out).all(axis=(1, 2)) & (det != 0.0))
    out[bad] = np.nan
    return out[0] if single else out


def footprint_bounds(georef, sizes, cell):
    """A grid that holds every frame's footprint: (x0, y0, gx, gy) for coverage(bounds=).  georef (F,2,3) float64 as for
    census(), sizes (F,2) (height, width), cell metres.  The extent of the corners (0, 0), (W, 0), (0, H), (W, H) of every
    frame whose georeference is finite and whose size is at least 1 x 1; x0 and y0 are snapped down to multiples of cell,
    so the grids of two flights of one area line up; gx and gy are at least 1 (no usable frame: (0.0, 0.0, 1, 1)).  Host
    only.  Raises ValueError when the grid would exceed the limits of include/wm_hip.h: choose a larger cell."""
    what = "footprint_bounds"
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    ok = np.isfinite(g).all(axis=(1, 2)) & (s >= 1).all(axis=1)
    if not ok.any():
        return 0.0, 0.0, 1, 1
    g, s = g[ok], s[ok].astype(np.float64)
    cx = np.stack([np.zeros(len(g)), s[:, 1], np.zeros(len(g)), s[:, 1]], axis=1)
    cy = np.stack([np.zeros(len(g)), np.zeros(len(g)), s[:, 0], s[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        X = g[:, 0, 0:1] * cx + g[:, 0, 1:2] * cy + g[:, 0, 2:3]
        Y = g[:, 1, 0:1] * cx + g[:, 1, 1:2] * cy + g[:, 1, 2:3]
        x0, y0 = math.floor(X.min() / cell) * cell, math.floor(Y.min() / cell) * cell
        nx, ny = math.ceil((X.max() - x0) / cell), math.ceil((Y.max() - y0) / cell)
    if not all(math.isfinite(v) for v in (x0, y0, nx, ny)):
        raise ValueError(f"{what}: the footprints' extent is not finite at cell {cell!r}")
    _, _, gx, gy = _check_grid(x0, y0, max(int(nx), 1), max(int(ny), 1), cell, what, "the footprints' grid")
    return float(x0), float(y0), gx, gy


def _survey_grid(georef, sizes, cell, bounds, what: str):
    """The frames and the grid of coverage() and mosaic(), validated before any device work: (g (F,2,3) float64, s (F,2) int32,
    cell, x0, y0, gx, gy); bounds None means footprint_bounds(georef, sizes, cell)."""
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    if g.shape[0] > COVERAGE_MAX_FRAMES:
        raise ValueError(f"{what}: {g.shape[0]} frames exceed {COVERAGE_MAX_FRAMES}")
    if bounds is None:
        x0, y0, gx, gy = footprint_bounds(g, s, cell)
    else:
        try:
            bx0, by0, bgx, bgy = bounds
        except (TypeError, ValueError):
            raise ValueError(f"{what}: bounds {bounds!r}: expected (x0, y0, gx, gy)") from None
        x0, y0, gx, gy = _check_grid(bx0, by0, bgx, bgy, cell, what)
    return g, s, cell, x0, y0, gx, gy


def _survey_device(what: str, pts=None) -> torch.device:
    """The device of coverage(), mosaic() and register(): that of the census' points when they are given, else the current one."""
    if pts is not None:
        if not pts.is_cuda:
            raise RuntimeError(f"{what}: census['points'] is on {pts.device}; the HIP path needs a ROCm device tensor "
                               "(there is no CPU fallback in wildlifemapper_amd)")
        return pts.device
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what}: no GPU is present; the HIP path needs a ROCm device tensor "
                           "(there is no CPU fallback in wildlifemapper_amd)")
    return torch.device("cuda", torch.cuda.current_device())


def _pinned_upload(a: np.ndarray, dev: torch.device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def _frame_tables(g: np.ndarray, s: np.ndarray, dev: torch.device):
    """The kernels' g2p (F,6) float64 and sizes (F,2) int32 on dev, through pinned memory; (None, None) when there is no frame."""
    if not g.shape[0]:
        return None, None
    return _pinned_upload(ground_to_pixel(g).reshape(-1, 6), dev), _pinned_upload(s, dev)


def _frame_sequence(frames, sizes, what: str, indexed_for: str):
    """The frames of mosaic() and register(): a sequence that is only indexed.  Returns (len(frames), sizes); sizes None is
    inferred only from a list or tuple of tensors or arrays, whose shapes cost nothing."""
    if not (hasattr(frames, "__getitem__") and hasattr(frames, "__len__")):
        raise ValueError(f"{what}: frames must be a sequence that can be indexed (frames[i], len), got {type(frames).__name__}")
    if sizes is None:
        if not isinstance(frames, (list, tuple)) or not all(isinstance(fr, (torch.Tensor, np.ndarray)) for fr in frames):
            raise ValueError(f"{what}: sizes is required when frames is not a list of tensors or arrays (a lazy sequence is only "
                             f"indexed for {indexed_for})")
        if any(fr.ndim != 3 for fr in frames):
            raise ValueError(f"{what}: frames: expected (H,W,3) uint8 tensors or arrays")
        sizes = np.array([tuple(fr.shape[:2]) for fr in frames], dtype=np.int64).reshape(-1, 2)
    return len(frames), sizes


def _resident_chunk(frames, ids, s: np.ndarray, dev: torch.device, what: str):
    """Makes the frames `ids` (ascending) resident for one fill or render launch: frames[i] is indexed once each, in that
    order, host frames go up through pinned memory, and a shape that disagrees with s raises ValueError naming the frame.
    Returns (descriptors, the (F,) slot table, the frames), all on dev; the caller drops them after its launch."""
    resident = []
    for i in ids:
        on_dev, on_host = _as_frame_array(frames[i], i, dev, what)
        fr = on_dev if on_dev is not None else on_host.pin_memory().to(dev, non_blocking=True)
        if tuple(fr.shape[:2]) != tuple(int(v) for v in s[i]):
            raise ValueError(f"{what}: frame {i} is {tuple(fr.shape[:2])}, sizes says {tuple(int(v) for v in s[i])}")
        resident.append(fr)
    slot = np.full(s.shape[0], -1, dtype=np.int32)
    slot[ids] = np.arange(len(ids), dtype=np.int32)
    return _frame_descs(resident, dev), _pinned_upload(slot, dev), resident


def coverage(georef, sizes, cell, census=None, bounds=None) -> Dict[str, object]:
    """The ground a survey saw (wm_coverage_raster, wm_coverage_points; rule: include/wm_hip.h).  georef (F,2,3) float64 as
    for census() (pixel -> ground; inverted on the host by ground_to_pixel), sizes (F,2) (height, width) of the frames in
    the pixels the georeferences speak of, cell the side of a ground cell in metres, bounds (x0, y0, gx, gy) or None for
    footprint_bounds(georef, sizes, cell), census the dict census() returned, or None.  Everything is validated before
    any device work; the frames go up through pinned memory to the current device -- torch.cuda.current_device(), or with
    census= the device of its tensors -- and the launches run on its current stream; one small copy of the statistics
    waits for them.  No CPU fallback.  Returns
      'coverage' (gy,gx) int32 on the device: frames that saw each cell's centre.  Row 0 is the SOUTHERNMOST row: a
          north-up picture is coverage.flip(0).  The kernel writes uint16 (F <= 65535); it is widened once to int32
          (a copy of twice the raster's bytes), the narrowest dtype torch indexes, compares and sums on the device;
      'origin' (x0, y0), 'cell', 'shape' (gy, gx); 'multiplicity' (16,) int64 on the device: cells seen by 0, 1, ...,
          14 and by 15 or more frames; 'gap_cells' int = multiplicity[0], the cells no frame saw;
      'area_m2' float = (gx * gy - gap_cells) * cell * cell, the observed ground;
    and with census=, from the individuals' keeper 'points' (k,2) and 'labels' (k,):
      'seen_by' (k,) int64: frames whose footprint holds the individual's point (0: not finite, or seen by none);
      'cell_index' (k,2) int64: its cell (j, i), (-1, -1) when it is not binned (outside the grid, not finite, or a
          label outside 0..6);
      'counts' (7,gy,gx) int32: binned individuals per class and cell; 'class_counts' (7,) int64: their sums;
      'density_per_km2' (7,) float64 = class_counts / (area_m2 / 1e6), divided on the host in double; NaN when the area is 0;
      'detection_rate' float = sum of 'members' / sum of 'seen_by' over the individuals with seen_by >= 1, NaN when
          there is none: of the chances the frames had to detect an individual, the share they took.  A member's own
          ground point differs slightly from its keeper's (the georeferencing error the census radius absorbs), so at a
          frame's edge a member can lie in a frame whose footprint misses the keeper's point: a ratio slightly above 1
          is possible and is not clamped."""
    what = "coverage"
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    F = g.shape[0]
    pts = labels = members = None
    if census is not None:
        try:
            pts, labels, members = census["points"], census["labels"], census["members"]
        except (TypeError, KeyError):
            raise ValueError(f"{what}: census has no 'points', 'labels' and 'members': pass the dict census() returned") from None
        if not all(isinstance(t, torch.Tensor) for t in (pts, labels, members)) or pts.dim() != 2 or pts.shape[1] != 2 or \
                pts.dtype != torch.float64 or tuple(labels.shape) != (pts.shape[0],) or tuple(members.shape) != (pts.shape[0],):
            raise ValueError(f"{what}: census: expected 'points' (k,2) float64, 'labels' (k,) and 'members' (k,) tensors")
        if pts.shape[0] > CENSUS_MAX_DETS:
            raise ValueError(f"{what}: {pts.shape[0]} individuals exceed {CENSUS_MAX_DETS}")
        if labels.device != pts.device or members.device != pts.device:
            raise ValueError(f"{what}: census tensors are on different devices")
    dev = _survey_device(what, pts)
    lib = N.lib()
    with torch.cuda.device(dev):
        g_d, s_d = _frame_tables(g, s, dev)                   # no frames: nothing to upload, an all-zero raster
        cov16 = torch.empty((gy, gx), device=dev, dtype=torch.int16)
        stats = torch.empty(N.COVERAGE_STATS, device=dev, dtype=torch.int64)
        N.check(lib.wm_coverage_raster(N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy, N.ptr(cov16), N.ptr(stats), N.stream_ptr(dev)))
        out = {"coverage": cov16.to(torch.int32) & 0xFFFF, "origin": (x0, y0), "cell": cell, "shape": (gy, gx), "multiplicity": stats}
        gap = int(stats[0].item())
        area = float((gx * gy - gap) * cell * cell)
        out["gap_cells"], out["area_m2"] = gap, area
        if census is None:
            return out
        k = int(pts.shape[0])
        pts = pts.contiguous()
        lab32 = labels.to(torch.int32).contiguous()
        alloc = torch.empty if k else torch.zeros             # k == 0: the entry returns before writing anything
        seen = alloc(k, device=dev, dtype=torch.int32)
        cidx = alloc((k, 2), device=dev, dtype=torch.int32)
        counts = alloc((N.COVERAGE_CLASSES, gy, gx), device=dev, dtype=torch.int32)
        pstats = alloc(2, device=dev, dtype=torch.int64)
        N.check(lib.wm_coverage_points(N.ptr(g_d), N.ptr(s_d), F, N.ptr(pts), N.ptr(lab32), k, x0, y0, cell, gx, gy, N.ptr(seen),
                                       N.ptr(cidx), N.ptr(counts), N.ptr(pstats), N.stream_ptr(dev)))
        seen = seen.to(torch.int64)
        class_counts = counts.sum(dim=(1, 2), dtype=torch.int64)
        could = seen >= 1
        n_seen, n_members = int(seen[could].sum().item()), int(members[could].sum().item())
        # seven divisions, on the host: IEEE double there, where a device division by a scalar may be a multiplication
        density = class_counts.cpu().numpy().astype(np.float64) / (area / 1e6) if area > 0 else np.full(N.COVERAGE_CLASSES, np.nan)
    out.update({"seen_by": seen, "cell_index": cidx.to(torch.int64), "counts": counts, "class_counts": class_counts,
                "density_per_km2": torch.from_numpy(density).to(dev),
                "detection_rate": n_members / n_seen if n_seen > 0 else float("nan")})
    return out


# ---- mosaic ----------------------------------------------------------------------------------------------------------

MOSAIC_SAMPLES = {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}


def _check_whole(value, what: str, name: str, lo: int = 1) -> int:
    """A whole number >= lo (an int, or a float without a fraction), before any device work."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value) \
            or value != int(value) or int(value) < lo:
        raise ValueError(f"{what}: {name} {value!r} must be a whole number >= {lo}")
    return int(value)


def _mosaic_plan(g, s, cell, x0, y0, gx, gy, dev):
    """wm_mosaic_plan on validated arguments.  Returns the plan's dict and the device copies of g2p and sizes."""
    F = g.shape[0]
    with torch.cuda.device(dev):
        g_d, s_d = _frame_tables(g, s, dev)                   # no frames: nothing to upload, an all -1 raster
        won = torch.empty(F, device=dev, dtype=torch.int32) if F else None
        source = torch.empty((gy, gx), device=dev, dtype=torch.int32)
        stats = torch.empty(2, device=dev, dtype=torch.int64)
        N.check(N.lib().wm_mosaic_plan(N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy, N.ptr(source), N.ptr(won), N.ptr(stats),
                                       N.stream_ptr(dev)))
        gap = int(stats[1].item())
    won = won.to(torch.int64) if F else torch.zeros(0, device=dev, dtype=torch.int64)
    return {"source": source, "won": won, "origin": (x0, y0), "cell": cell, "shape": (gy, gx), "gap_cells": gap}, g_d, s_d


def mosaic_plan(georef, sizes, cell, bounds=None) -> Dict[str, object]:
    """Which frame shows each ground cell (wm_mosaic_plan; rule: include/wm_hip.h "Survey mosaic").  Geometry only, no
    pixels: georef (F,2,3) float64 as for census() (pixel -> ground), sizes (F,2) (height, width), cell metres, bounds
    (x0, y0, gx, gy) or None for footprint_bounds(georef, sizes, cell) -- the arguments and the validation of coverage(),
    run before any device work.  Among the frames that see a cell's centre the source is the one whose centre pixel is
    nearest to it (the most vertical view), ties to the lowest index.  One launch on the current device's current stream
    and one small copy of the statistics, which waits for it.  No CPU fallback.  Returns
      'source' (gy,gx) int32 on the device: the frame of each cell, -1 where no frame saw it; row 0 is the SOUTHERNMOST;
      'won' (F,) int64 on the device: the cells each frame is the source of;
      'origin' (x0, y0), 'cell', 'shape' (gy, gx); 'gap_cells' int, the cells without a source."""
    what = "mosaic_plan"
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    return _mosaic_plan(g, s, cell, x0, y0, gx, gy, _survey_device(what))[0]


def resampled_georef(georef, size, new_size) -> np.ndarray:
    """The georeference of a frame after resampling: georef (2,3) or (F,2,3) float64 (pixel -> ground) of frames of `size`
    (height, width) gives that of the same frames resampled to `new_size` (H', W') -- a pixel of the new frame spans W / W'
    old pixels across and H / H' down, and pixel (0, 0)'s corner stays where it was: a0' = a0 * (W / W'), a3' = a3 *
    (W / W'), a1' = a1 * (H / H'), a4' = a4 * (H / H'), a2 and a5 unchanged.  size and new_size are one (height, width)
    pair for all frames or (F,2), one pair per frame.  Host only, in double.  With preprocess.resample_u8 this is the
    route to a map coarser than the frames: mosaic() point-samples, so shrink the frames to about the cell size first."""
    what = "resampled_georef"
    g = georef.detach().cpu().numpy() if isinstance(georef, torch.Tensor) else georef
    try:
        g = np.asarray(g, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: georef is not an array of numbers") from None
    single = g.ndim == 2
    g = _check_georef(g[None] if single else g, what)
    F = g.shape[0]

    def pairs(v, name):
        try:
            a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
            if a.dtype.kind not in "iuf" or a.shape not in ((2,), (F, 2)) or not np.all(np.isfinite(a)) or not np.all(a == np.floor(a)) \
                    or not np.all(a >= 1):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} {v!r}: expected (height, width) or ({F}, 2), whole numbers >= 1") from None
        return np.broadcast_to(a.astype(np.float64), (F, 2))

    old, new = pairs(size, "size"), pairs(new_size, "new_size")
    sy, sx = old[:, 0] / new[:, 0], old[:, 1] / new[:, 1]
    out = g.copy()
    out[:, 0, 0], out[:, 1, 0] = g[:, 0, 0] * sx, g[:, 1, 0] * sx
    out[:, 0, 1], out[:, 1, 1] = g[:, 0, 1] * sy, g[:, 1, 1] * sy
    return out[0] if single else out


def mosaic(frames, georef, cell, sizes=None, bounds=None, sample: str = "bilinear", fill=(0, 0, 0), north_up: bool = True,
           chunk: int = 8, census=None, marker=None, width: int = 2, palette=None) -> Dict[str, object]:
    """The map of a survey: its frames laid onto the ground grid (wm_mosaic_plan, wm_mosaic_fill_u8; rule: include/wm_hip.h
    "Survey mosaic").  frames: a sequence that is only indexed (frames[i], len) -- a list of (H,W,3) uint8 ROCm tensors,
    CPU tensors or numpy arrays as detect_frames accepts them, or a lazy sequence that loads frame i from disk when it is
    asked for; georef (F,2,3) float64 as for census(), cell metres, bounds as for coverage().  sizes (F,2) (height, width)
    may be None only when every item of `frames` is already a tensor or an array (a list or tuple, whose shapes cost
    nothing); a lazy sequence needs it.  Everything is validated before any device work.
    The plan runs first (mosaic_plan).  Only frames that are the source of at least one cell are ever indexed, each
    exactly once, in ascending order, `chunk` at a time: host frames go up through pinned memory, one fill launch per
    chunk, and the chunk's frames are released after it -- a lazy sequence pays for the winners only, and bounds= over a
    corner of a survey touches a handful of frames.  A frame whose shape disagrees with sizes raises ValueError naming
    it, before its chunk is launched.
    sample: 'bilinear' (pixel centres at integer + 0.5, edge replicate) or 'nearest'.  A cell finer than the ground
    sampling distance magnifies; a coarser one point-samples and aliases: for a coarse map shrink the frames first
    (preprocess.resample_u8, PIL-exact) and rescale their georeferences (resampled_georef).  fill: the (r, g, b) of the
    cells no frame saw.  north_up: the picture's row 0 is the NORTHERNMOST (what a viewer expects); False keeps row 0
    south, as 'source' and coverage() always have it.
    census= (the dict census() returned) with marker= (the side of a square in cells, a whole number >= 1): every
    individual whose keeper point is finite and inside the grid is outlined in its class colour by one draw_boxes launch
    on the finished mosaic (width, palette as for draw_boxes); the square is centred on ((X - x0) / cell, (Y - y0) / cell),
    the y mirrored (gy - y) when north_up.
    Runs on the current device's current stream (with census=, on its tensors' device).  No CPU fallback.  Returns the
    plan's dict ('source', 'won', 'origin', 'cell', 'shape', 'gap_cells') plus 'mosaic' (gy,gx,3) uint8 on the device and
    'north_up'; with markers also 'marker_boxes' (k',4) fp32 xyxy in picture pixels and 'marker_index' (k',) int64, the
    individuals they belong to."""
    what = "mosaic"
    if not isinstance(sample, str) or sample not in MOSAIC_SAMPLES:
        raise ValueError(f"{what}: sample {sample!r} must be 'bilinear' or 'nearest'")
    try:
        fill_a = np.asarray(fill)
        if fill_a.shape != (3,) or fill_a.dtype.kind not in "iuf" or not np.all((fill_a >= 0) & (fill_a <= 255) & (fill_a == np.floor(fill_a))):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: fill {fill!r} must be three whole numbers in 0..255") from None
    fill_a = fill_a.astype(np.uint8)
    chunk = _check_whole(chunk, what, "chunk")
    if (census is None) != (marker is None):
        raise ValueError(f"{what}: marker {marker!r} and census go together: pass both (census= the dict census() returned) or neither")
    pts = labels = None
    if census is not None:
        marker = _check_whole(marker, what, "marker")
        width = _check_draw_width(width, what)
        palette = _check_palette(palette, what)
        try:
            pts, labels = census["points"], census["labels"]
        except (TypeError, KeyError):
            raise ValueError(f"{what}: census has no 'points' and 'labels': pass the dict census() returned") from None
        if not all(isinstance(t, torch.Tensor) for t in (pts, labels)) or pts.dim() != 2 or pts.shape[1] != 2 or \
                pts.dtype != torch.float64 or tuple(labels.shape) != (pts.shape[0],) or labels.device != pts.device:
            raise ValueError(f"{what}: census: expected 'points' (k,2) float64 and 'labels' (k,) tensors on one device")
    n_given, sizes = _frame_sequence(frames, sizes, what, "the frames that won a cell")
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    F = g.shape[0]
    if n_given != F:
        raise ValueError(f"{what}: {n_given} frames for {F} georeferences")
    dev = _survey_device(what, pts)
    out, g_d, s_d = _mosaic_plan(g, s, cell, x0, y0, gx, gy, dev)
    lib = N.lib()
    mode, flags = MOSAIC_SAMPLES[sample], N.MOSAIC_NORTH_UP if north_up else 0
    with torch.cuda.device(dev):
        picture = torch.from_numpy(fill_a).to(dev).expand(gy, gx, 3).contiguous()
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        winners = torch.nonzero(out["won"] > 0).flatten().cpu().tolist()
        for c0 in range(0, len(winners), chunk):
            ids = winners[c0:c0 + chunk]
            desc, slot_d, resident = _resident_chunk(frames, ids, s, dev, what)
            N.check(lib.wm_mosaic_fill_u8(N.ptr(desc), len(ids), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy,
                                          N.ptr(out["source"]), mode, flags, N.ptr(picture), N.ptr(status), N.stream_ptr(dev)))
            del resident, desc, slot_d                        # the stream orders their reuse after the launch
        bad = int(status.item()) if winners else 0
        if bad:
            raise RuntimeError(f"{what}: wm_mosaic_fill_u8 skipped cells (status {bad}): a resident frame did not match its slot or size")
        out.update({"mosaic": picture, "north_up": bool(north_up)})
        if pts is not None:
            p = pts.detach().cpu().numpy()
            with np.errstate(all="ignore"):
                cx, cy = (p[:, 0] - x0) / cell, (p[:, 1] - y0) / cell
                inside = np.isfinite(p).all(axis=1) & (np.floor(cx) >= 0) & (np.floor(cx) < gx) & (np.floor(cy) >= 0) & (np.floor(cy) < gy)
            idx = np.nonzero(inside)[0]
            cx, cy = cx[idx], cy[idx]
            if north_up:
                cy = gy - cy
            half = marker / 2.0
            boxes = np.stack([cx - half, cy - half, cx + half, cy + half], axis=1).astype(np.float32).reshape(-1, 4)
            boxes_d = torch.from_numpy(boxes).to(dev)
            idx_d = torch.from_numpy(idx.astype(np.int64)).to(dev)
            draw_boxes(picture, boxes_d, labels[idx_d], width=width, palette=palette)
            out.update({"marker_boxes": boxes_d, "marker_index": idx_d})
    return out


# ---- registration ----------------------------------------------------------------------------------------------------

REGISTER_MAX_SIDE = N.REGISTER_MAX_SIDE       # include/wm_hip.h WM_REGISTER_MAX_SIDE
REGISTER_MAX_SEARCH = N.REGISTER_MAX_SEARCH   # WM_REGISTER_MAX_SEARCH
REGISTER_MAX_PAIRS = N.REGISTER_MAX_PAIRS     # WM_REGISTER_MAX_PAIRS, per launch: register() chunks by pair_chunk
# wm_register_pair, 32 bytes: the patch of a pair is gx x gy cells with south-west corner (x0, y0)
REGISTER_PAIR = np.dtype([("frame_a", "<i4"), ("frame_b", "<i4"), ("gx", "<i4"), ("gy", "<i4"), ("x0", "<f8"), ("y0", "<f8")])
_REGISTER_FRAMES_RESIDENT = 8                 # frames on the device per render call of register()


def _check_register_shape(search, side, min_cells, what: str):
    search = _check_whole(search, what, "search", 0)
    side = _check_whole(side, what, "side")
    min_cells = _check_whole(min_cells, what, "min_cells")
    if search > REGISTER_MAX_SEARCH:
        raise ValueError(f"{what}: search {search} exceeds {REGISTER_MAX_SEARCH}")
    if side > REGISTER_MAX_SIDE:
        raise ValueError(f"{what}: side {side} exceeds {REGISTER_MAX_SIDE}")
    if min_cells >= 2 ** 31:
        raise ValueError(f"{what}: min_cells {min_cells} does not fit int32")
    return search, side, min_cells


def _check_pair_table(pairs, n_frames: int, side: int, what: str) -> np.ndarray:
    """A (P,) array of REGISTER_PAIR as register_pairs returns it, every entry inside the limits of include/wm_hip.h."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype != REGISTER_PAIR or pairs.ndim != 1:
        raise ValueError(f"{what}: pairs must be a (P,) array of tiling.REGISTER_PAIR, as register_pairs returns it")
    t = np.ascontiguousarray(pairs)
    if t.size:
        a, b = t["frame_a"], t["frame_b"]
        if a.min() < 0 or b.min() < 0 or a.max() >= n_frames or b.max() >= n_frames or np.any(a == b):
            raise ValueError(f"{what}: pairs: frame_a and frame_b must be two different frames in 0..{n_frames - 1}")
        if t["gx"].min() < 1 or t["gy"].min() < 1 or t["gx"].max() > side or t["gy"].max() > side:
            raise ValueError(f"{what}: pairs: gx and gy must lie in 1..side ({side})")
        if not (np.isfinite(t["x0"]).all() and np.isfinite(t["y0"]).all()):
            raise ValueError(f"{what}: pairs: x0 and y0 must be finite")
    return t


def register_pairs(georef, sizes, cell, search: int = 16, side: int = 512, min_cells: int = 4096) -> np.ndarray:
    """The overlapping pairs of a survey and their ground patches, for register().  Host only, in double.  georef (F,2,3)
    float64 as for census(), sizes (F,2) (height, width), cell metres.  A pair (i < j) is proposed when the axis-aligned
    ground bounding boxes of the two footprints (the extent of the corners (0, 0), (W, 0), (0, H), (W, H)) intersect with
    a positive area.  Its patch is that intersection snapped outward to multiples of cell -- i0 = floor(lo / cell), i1 =
    ceil(hi / cell), gx = i1 - i0, x0 = i0 * cell, the same north -- so the patches of all pairs lie on one lattice; a
    patch wider than `side` cells is centre-cropped (i0 += (gx - side) // 2, gx = side); a patch of fewer than min_cells
    cells is dropped.  A frame whose georeference is not finite or whose size is below 1 x 1 is in no pair.  search is
    only validated here (the patch does not depend on it).  Returns a (P,) array of REGISTER_PAIR (frame_a, frame_b, gx,
    gy, x0, y0), ordered by (frame_a, frame_b)."""
    what = "register_pairs"
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    search, side, min_cells = _check_register_shape(search, side, min_cells, what)
    F = g.shape[0]
    ok = np.isfinite(g).all(axis=(1, 2)) & (s >= 1).all(axis=1)
    w, h = s[:, 1].astype(np.float64), s[:, 0].astype(np.float64)
    zero = np.zeros(F)
    cx, cy = np.stack([zero, w, zero, w], axis=1), np.stack([zero, zero, h, h], axis=1)
    with np.errstate(all="ignore"):
        X = g[:, 0, 0:1] * cx + g[:, 0, 1:2] * cy + g[:, 0, 2:3]
        Y = g[:, 1, 0:1] * cx + g[:, 1, 1:2] * cy + g[:, 1, 2:3]
        xl, xh, yl, yh = X.min(axis=1), X.max(axis=1), Y.min(axis=1), Y.max(axis=1)
    out = []
    for i in range(F):
        if not ok[i]:
            continue
        js = np.arange(i + 1, F)
        lo_x, hi_x = np.maximum(xl[i], xl[js]), np.minimum(xh[i], xh[js])
        lo_y, hi_y = np.maximum(yl[i], yl[js]), np.minimum(yh[i], yh[js])
        for k in np.nonzero(ok[js] & (lo_x < hi_x) & (lo_y < hi_y))[0]:
            i0, i1 = math.floor(lo_x[k] / cell), math.ceil(hi_x[k] / cell)
            j0, j1 = math.floor(lo_y[k] / cell), math.ceil(hi_y[k] / cell)
            gx, gy = i1 - i0, j1 - j0
            if gx > side:
                i0, gx = i0 + (gx - side) // 2, side
            if gy > side:
                j0, gy = j0 + (gy - side) // 2, side
            if gx < 1 or gy < 1 or gx * gy < min_cells:
                continue
            out.append((i, int(js[k]), gx, gy, i0 * cell, j0 * cell))
    return np.array(out, dtype=REGISTER_PAIR).reshape(-1)


def adjust(n_frames, pairs, measured, weights, fixed=None) -> Dict[str, np.ndarray]:
    """One translation per frame from pairwise measurements: weighted least squares of t_b - t_a = m_p.  Host only, numpy
    double.  pairs: a REGISTER_PAIR table or a (P,2) array of (frame_a, frame_b); measured (P,2) metres (east, north);
    weights (P,) >= 0 -- register() passes the cells n of an accepted pair and 0 for a rejected one; a pair of weight 0 is
    not part of the system or of the graph.  The system is stacked with rows sqrt(w_p) * (t_b - t_a) = sqrt(w_p) * m_p and
    solved by numpy.linalg.lstsq, whose minimum-norm solution fixes what the measurements leave free: in a connected
    component of the graph without a fixed frame the mean shift of its frames is zero.  fixed: frames that stay at 0 (their
    columns are left out), which pins every component that holds one.  A frame with no pair of positive weight keeps 0.
    Returns 'shift' (n_frames,2) metres, to be added to (a2, a5); 'residual' (P,2) = (t_b - t_a) - m_p for every pair,
    whatever its weight; 'component' (n_frames,) int64, the lowest frame index of the frame's component, -1 for a frame
    with no pair of positive weight."""
    what = "adjust"
    F = _check_whole(n_frames, what, "n_frames", 0)
    if isinstance(pairs, np.ndarray) and pairs.dtype == REGISTER_PAIR:
        pairs = np.stack([pairs["frame_a"], pairs["frame_b"]], axis=1) if pairs.size else np.zeros((0, 2), dtype=np.int64)
    try:
        ab = np.asarray(pairs)
        if ab.size == 0:
            ab = ab.reshape(0, 2)
        if ab.dtype.kind not in "iu" or ab.ndim != 2 or ab.shape[1] != 2:
            raise TypeError
        ab = ab.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: pairs must be a REGISTER_PAIR table or a (P,2) array of whole numbers") from None
    P = ab.shape[0]
    if P and (ab.min() < 0 or ab.max() >= F or np.any(ab[:, 0] == ab[:, 1])):
        raise ValueError(f"{what}: pairs: frame_a and frame_b must be two different frames in 0..{F - 1}")
    try:
        m = np.asarray(measured, dtype=np.float64).reshape(-1, 2) if np.size(measured) else np.zeros((0, 2))
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: measured must be (P,2) numbers and weights (P,) numbers") from None
    if m.shape != (P, 2) or w.shape != (P,):
        raise ValueError(f"{what}: {P} pairs, measured of shape {m.shape} and weights of shape {w.shape}: expected ({P}, 2) and ({P},)")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f"{what}: weights must be finite and >= 0")
    used = w > 0
    if not np.isfinite(m[used]).all():
        raise ValueError(f"{what}: measured must be finite where the weight is positive")
    fixed_a = np.zeros(F, dtype=bool)
    if fixed is not None:
        try:
            fx = np.asarray(list(fixed))
            if fx.size and (fx.dtype.kind not in "iu" or fx.ndim != 1 or fx.min() < 0 or fx.max() >= F):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{what}: fixed {fixed!r} must be frame indices in 0..{F - 1}") from None
        fixed_a[fx.astype(np.int64)] = True
    # components of the graph of used pairs: union-find, labelled by their lowest frame
    root = np.arange(F)

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    for a, b in ab[used]:
        ra, rb = find(a), find(b)
        if ra != rb:
            root[max(ra, rb)] = min(ra, rb)
    in_graph = np.zeros(F, dtype=bool)
    in_graph[ab[used].reshape(-1)] = True
    component = np.array([find(f) if in_graph[f] else -1 for f in range(F)], dtype=np.int64).reshape(F)
    shift = np.zeros((F, 2), dtype=np.float64)
    cols = np.nonzero(in_graph & ~fixed_a)[0]
    if cols.size and used.any():
        col_of = np.full(F, -1, dtype=np.int64)
        col_of[cols] = np.arange(cols.size)
        rows = np.nonzero(used)[0]
        sw = np.sqrt(w[rows])
        A = np.zeros((rows.size, cols.size), dtype=np.float64)
        ca, cb = col_of[ab[rows, 0]], col_of[ab[rows, 1]]
        r = np.arange(rows.size)
        A[r[ca >= 0], ca[ca >= 0]] = -sw[ca >= 0]
        A[r[cb >= 0], cb[cb >= 0]] = sw[cb >= 0]
        t = np.linalg.lstsq(A, m[rows] * sw[:, None], rcond=None)[0]
        shift[cols] = t
    with np.errstate(all="ignore"):
        residual = (shift[ab[:, 1]] - shift[ab[:, 0]]) - m
    return {"shift": shift, "residual": residual, "component": component}


REGISTER_METRICS = ("sad", "zncc")


def _decode_sad(best, peak, min_corr):
    """best (P,8) -> has, has2, mean, runner_up, corr, confident: best's third of four is sad (-1: none), the fourth n."""
    sad, n1, sad2, n2 = (best[:, k].astype(np.int64) for k in (2, 3, 6, 7))
    has, has2 = sad >= 0, sad2 >= 0
    mean = np.where(has, sad / np.maximum(n1, 1), np.nan)
    runner = np.where(has2, sad2 / np.maximum(n2, 1), np.nan)
    return has, has2, mean, runner, np.full(best.shape[0], np.nan), has


def _decode_zncc(best, peak, min_corr):
    """best (P,8), peak (P,2) -> the same six: best's third of four is ok (1 / 0), peak holds q (NaN: none)."""
    has, has2 = best[:, 2] == 1, best[:, 6] == 1
    r = np.sign(peak) * np.sqrt(np.abs(peak))
    corr = np.where(has, r[:, 0], np.nan)
    mean = np.where(has, 1.0 - r[:, 0], np.nan)
    runner = np.where(has2, 1.0 - r[:, 1], np.nan)
    return has, has2, mean, runner, corr, has & (corr > min_corr)


# per metric: the entry point, its table's dtype and last dimension, whether it fills a peak buffer, best[2] of "none", the decoder
_REGISTER_METRIC = {"sad": ("wm_register_search", torch.int32, 2, False, -1, _decode_sad),
                    "zncc": ("wm_register_search_zncc", torch.int64, 6, True, 0, _decode_zncc)}


def register(frames, georef, cell, sizes=None, search: int = 16, side: int = 512, min_cells: int = 4096, min_ratio: float = 1.25,
             pairs=None, fixed=None, pair_chunk: int = 256, metric: str = "sad", min_corr: float = 0.0) -> Dict[str, object]:
    """Correct the georeferences of a survey by matching the pixels of its overlapping frames (wm_register_render_u8,
    wm_register_search or wm_register_search_zncc; rule: include/wm_hip.h "Survey registration" and "Survey registration,
    correlation search").  frames as mosaic() takes them: a sequence that is
    only indexed -- tensors, arrays, or a lazy sequence that loads frame i when asked; georef (F,2,3) float64 as for
    census(); cell metres; sizes (F,2) may be None only for a list of tensors or arrays.  pairs: the table to use, None for
    register_pairs(georef, sizes, cell, search, side, min_cells).  Everything is validated before any device work.
    The pairs are rendered and searched pair_chunk at a time, so the planes stay bounded (pair_chunk * (side^2 + (side +
    2 * search)^2) bytes); within a chunk its frames go up a few at a time and are released after their render call, so a
    frame is read only while a pair of the current chunk needs it (a frame shared by two chunks is read once per chunk).
    A pair is ACCEPTED iff a best offset exists (some offset has n >= min_cells), |dy| < search and |dx| < search (a peak
    on the window's edge is not a peak), and the runner-up outside the peak's 3 x 3 has a mean absolute difference of at
    least min_ratio times the peak's (sad2 / n2 >= min_ratio * (sad / n), in double); a runner-up that does not exist also
    accepts.  The accepted pairs, each measuring t_b - t_a = -(dx, dy) * cell with weight n, go to adjust(fixed=fixed).
    metric: "sad" (the default) is the rule above, masked sums of absolute differences; it assumes the same exposure in
    both frames of a pair (no gain or offset is fitted).  Where exposure changes between frames -- auto-exposure, cloud
    shadow -- use metric="zncc": the offsets are scored by the zero-mean normalised correlation, which a gain and an offset
    between the two frames do not change.  With r = sign(q) * sqrt(|q|) of the device's signed squared correlation q, a
    pair is then accepted iff a best offset exists (n >= min_cells and neither plane flat), |dy| < search and |dx| <
    search, r > min_corr (finite, in [-1, 1)), and the runner-up does not exist or 1 - r2 >= min_ratio * (1 - r): 1 - r
    takes the part of the mean absolute difference, so min_ratio keeps its meaning.  Both defaults are policy, not
    measurements on real imagery.  A cell coarser than the ground
    sampling distance point-samples, so shrink the frames first (preprocess.resample_u8, resampled_georef); only a
    translation is corrected, not yaw or scale; the resolution is one cell -- a second register() at a finer cell on the
    corrected georef refines it.  Runs on the current device's current stream.  No CPU fallback.  Returns host arrays:
      'georef' (F,2,3) float64 corrected (shift added to a2, a5), 'shift' (F,2) metres, 'pairs' the table,
      'offset' (P,2) int64 cells (dx, dy), 'cells' (P,) int64 n at the best offset (0: none), 'mean' (P,) float64 sad / n
      (NaN: none), 'runner_up' (P,) float64 sad2 / n2 (NaN: none), 'accepted' (P,) bool, 'residual' (P,2) metres after
      the adjustment, 'component' (F,) int64 as adjust() gives it, 'corr' (P,) float64 NaN.  Under metric="zncc" 'mean'
      is 1 - r and 'runner_up' 1 - r2 (NaN: none), and 'corr' is r (NaN: none)."""
    what = "register"
    if not isinstance(metric, str) or metric not in REGISTER_METRICS:
        raise ValueError(f"{what}: metric {metric!r} must be one of {REGISTER_METRICS}")
    try:
        if isinstance(min_corr, bool):
            raise TypeError
        min_corr = float(min_corr)
        if not (math.isfinite(min_corr) and -1.0 <= min_corr < 1.0):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: min_corr {min_corr!r} must be a finite number in [-1, 1)") from None
    entry, table_dtype, table_last, has_peak, none, decode = _REGISTER_METRIC[metric]
    search, side, min_cells = _check_register_shape(search, side, min_cells, what)
    pair_chunk = _check_whole(pair_chunk, what, "pair_chunk")
    if pair_chunk > REGISTER_MAX_PAIRS:
        raise ValueError(f"{what}: pair_chunk {pair_chunk} exceeds {REGISTER_MAX_PAIRS}")
    try:
        min_ratio = float(min_ratio)
        if isinstance(min_ratio, bool) or not (math.isfinite(min_ratio) and min_ratio >= 0.0):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: min_ratio {min_ratio!r} must be a finite number >= 0") from None
    n_given, sizes = _frame_sequence(frames, sizes, what, "the frames of the current chunk of pairs")
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    F = g.shape[0]
    if F > COVERAGE_MAX_FRAMES:
        raise ValueError(f"{what}: {F} frames exceed {COVERAGE_MAX_FRAMES}")
    if n_given != F:
        raise ValueError(f"{what}: {n_given} frames for {F} georeferences")
    table = register_pairs(g, s, cell, search, side, min_cells) if pairs is None else _check_pair_table(pairs, F, side, what)
    adjust(F, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2)), np.zeros(0), fixed)         # fixed= validated before device work
    P = table.shape[0]
    best = np.zeros((P, 8), dtype=np.int32)
    peak = np.full((P, 2), np.nan, dtype=np.float64)                 # (q, q2) of the correlation search
    best[:, 2] = best[:, 6] = none
    if P:
        dev = _survey_device(what)
        lib = N.lib()
        E = side + 2 * search
        with torch.cuda.device(dev):
            g_d, s_d = _frame_tables(g, s, dev)
            status = torch.zeros(1, device=dev, dtype=torch.int32)
            for c0 in range(0, P, pair_chunk):
                chunk = table[c0:c0 + pair_chunk]
                n = chunk.shape[0]
                pairs_d = _pinned_upload(chunk.view(np.uint8).reshape(n, REGISTER_PAIR.itemsize), dev)
                plane_a = torch.empty((n, side, side), device=dev, dtype=torch.uint8)
                plane_b = torch.empty((n, E, E), device=dev, dtype=torch.uint8)
                needed = sorted(set(chunk["frame_a"].tolist()) | set(chunk["frame_b"].tolist()))
                for f0 in range(0, len(needed), _REGISTER_FRAMES_RESIDENT):
                    ids = needed[f0:f0 + _REGISTER_FRAMES_RESIDENT]
                    desc, slot_d, resident = _resident_chunk(frames, ids, s, dev, what)
                    N.check(lib.wm_register_render_u8(N.ptr(desc), len(ids), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, N.ptr(pairs_d), n,
                                                      cell, search, side, N.ptr(plane_a), N.ptr(plane_b), N.ptr(status), N.stream_ptr(dev)))
                    del resident, desc, slot_d                    # the stream orders their reuse after the launch
                best_d = torch.empty((n, 8), device=dev, dtype=torch.int32)
                score = torch.empty((n, 2 * search + 1, 2 * search + 1, table_last), device=dev, dtype=table_dtype)
                peak_d = torch.empty((n, 2), device=dev, dtype=torch.float64) if has_peak else None
                N.check(getattr(lib, entry)(N.ptr(plane_a), N.ptr(plane_b), N.ptr(pairs_d), n, search, side, min_cells, N.ptr(score),
                                            N.ptr(best_d), *([N.ptr(peak_d)] if has_peak else []), N.stream_ptr(dev)))
                if has_peak:
                    peak[c0:c0 + n] = peak_d.cpu().numpy()
                best[c0:c0 + n] = best_d.cpu().numpy()
                del plane_a, plane_b, score, best_d, peak_d, pairs_d
            bad = int(status.item())
        if bad:
            raise RuntimeError(f"{what}: wm_register_render_u8 skipped planes (status {bad}): a resident frame did not match its slot or size")
    dy, dx, n1 = (best[:, k].astype(np.int64) for k in (0, 1, 3))
    with np.errstate(all="ignore"):
        has, has2, mean, runner, corr, confident = decode(best, peak, min_corr)
        accepted = confident & (np.abs(dy) < search) & (np.abs(dx) < search) & (~has2 | (runner >= min_ratio * mean))
    offset = np.stack([dx, dy], axis=1).reshape(P, 2)
    adj = adjust(F, table, -offset.astype(np.float64) * cell, np.where(accepted, n1, 0).astype(np.float64), fixed)
    out_g = g.copy()
    out_g[:, 0, 2] += adj["shift"][:, 0]
    out_g[:, 1, 2] += adj["shift"][:, 1]
    return {"georef": out_g, "shift": adj["shift"], "pairs": table, "offset": offset, "cells": np.where(has, n1, 0), "mean": mean,
            "runner_up": runner, "accepted": accepted, "residual": adj["residual"], "component": adj["component"], "corr": corr}
