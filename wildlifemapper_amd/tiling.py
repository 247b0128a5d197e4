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
  * chips= / overlay= (detect_frame, detect_frames): opt-in review chips and overlays of every detection, cut and drawn by
    review.py's crop_chips and draw_boxes for the frames a merge completed.
Frame coordinates are fp32: a box coordinate keeps a fractional resolution below 0.01 px up to 65536 px (ulp 2**-8).

The rest of the survey API lives beside this module and stays importable from it: chips and overlays in review.py, the
census, coverage and mosaic in ground.py, registration in registration.py, the lens model (lens_plan, undistorted) in lens.py,
roll and pitch (rectify_plan, rectified) in attitude.py, terrain relief (ortho_plan, orthorectified) in terrain.py; what they all
share is in _survey.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Iterator, List, NamedTuple, Tuple

import numpy as np

import torch

from . import _native as N
from . import preprocess
from ._survey import _as_frame_array, _finite_number, _frame_descs, _frame_index, _pinned_upload
from .ground import (CENSUS_CLASSES, CENSUS_MAX_DETS, COVERAGE_MAX_CELLS, COVERAGE_MAX_FRAMES, COVERAGE_MAX_SIDE, MOSAIC_SAMPLES,  # noqa: F401
                     census, coverage, footprint_bounds, ground_to_pixel, mosaic, mosaic_blend_plan, mosaic_plan, nadir_affine,
                     resampled_georef)
from .attitude import MAX_TILT_DEG, attitude_points, attitude_rotation, rectified, rectify_plan  # noqa: F401
from .lens import CAMERA_ENTRIES, LENS_KEEP, LENS_MAX_SIDE, distort_points, lens_plan, lens_points, undistort_points, undistorted  # noqa: F401
from .registration import (REGISTER_MAX_LEVEL, REGISTER_MAX_PAIRS, REGISTER_MAX_SEARCH, REGISTER_MAX_SIDE, REGISTER_METRICS,  # noqa: F401
                           REGISTER_PAIR, REGISTER_REFINE_SUMS, adjust, adjust_exposure, adjust_similarity, exposure_table, reduce_planes,
                           refine, refine_solve, refine_step, register, register_pairs)
from .terrain import (TERRAIN_MAX_SIDE, camera_pose, ortho_plan, orthorectified, terrain_grid, terrain_height, terrain_points,  # noqa: F401
                      to_device)
from .review import (CHIP_MAX_SIDE, DEFAULT_PALETTE, DRAW_MAX_PALETTE, DRAW_MAX_WIDTH, OVERLAY_MAX, OVERLAY_MIN, _check_chip,  # noqa: F401
                     _check_chip_rule, _check_draw_width, _check_overlay, _check_palette, chip_windows, crop_chips, draw_boxes,
                     outline_rects, overlay_size)


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
    fp32 = lambda t: float(np.float32(t))                     # the kernel compares in fp32
    return fp32(_finite_number(fuse_thr, what, "fuse_thr", lambda t: 0.0 <= fp32(t) < 1.0, "must be in [0, 1) in fp32"))


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
    out = {"merged": merged, "det": det, "det_tile": det_tile, "det_count": det_count}
    if fuse_thr is not None:                  # the fuse entry takes the NMS entry's arguments, its threshold and two more outputs
        out["det_members"] = torch.empty(n * N.NUM_QUERIES, device=dev, dtype=torch.int32)
        out["slot_det"] = torch.empty(n * N.NUM_QUERIES, device=dev, dtype=torch.int32)
        entry, thr = N.lib().wm_merge_frames_fuse, fuse_thr
    else:
        entry, thr = N.lib().wm_merge_frames_nms, float(iou_thr)
    with torch.cuda.device(dev):
        N.check(entry(N.ptr(records), N.ptr(origins), offs.ctypes.data_as(C.POINTER(C.c_int32)), nf, thr, N.ptr(scratch), nbytes,
                      *(N.ptr(t) for t in out.values()), N.stream_ptr(dev)))
    return out


def merge_tile_records(records: torch.Tensor, origins: torch.Tensor, iou_thr: float = 0.4) -> torch.Tensor:
    """records (n,51,8) raw per-tile records of one frame (boxes in tile pixels) -> (n,51,8) merged records in frame
    coordinates with FLAG_MERGED / nms_rank of the cross-tile NMS: merge_frames of a one-frame survey."""
    return merge_frames(records, origins, [0, records.shape[0]], iou_thr)["merged"]


def _check_scale(scale, what: str) -> float:
    return _finite_number(scale, what, "scale", lambda s: s > 0.0, "must be positive and finite")


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


def _scale_boxes(b: torch.Tensor, sx: float, sy: float) -> torch.Tensor:
    """(k,4) fp32 xyxy boxes with x scaled by sx and y by sy: one fp32 multiply per coordinate."""
    out = torch.empty_like(b)
    out[:, 0::2] = b[:, 0::2] * sx
    out[:, 1::2] = b[:, 1::2] * sy
    return out


class _Frame:
    __slots__ = ("data", "height", "width", "origins", "origins_dev", "ready", "records", "scale_xy", "source")

    def __init__(self, data, height, width, origins, ready, scale_xy=None, source=None):
        self.data, self.height, self.width, self.origins, self.ready = data, height, width, origins, ready
        self.source = source                  # chips= / overlay= only: the source-resolution device frame, kept until finish()
        self.records: List[torch.Tensor] = []
        self.origins_dev = None
        self.scale_xy = scale_xy              # resampled mode: (sx, sy) = float32(W / ow), float32(H / oh); else None


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
        # resampling: the resampled frame is what gets tiled, and a caller's device frame is only read
        oh, ow = resampled_size(i, H, W, scale, resize) if resampling else (H, W)      # a bad per-frame scale raises before any device work
        if device is None:
            raise RuntimeError("detect_frames: no ROCm device (there is no CPU fallback in wildlifemapper_amd)")
        org = tile_origins(oh, ow, 1024, overlap)
        size = None if (oh, ow) == (H, W) else (oh, ow)
        ready = None
        if d is None:
            d, ready, src = upload(h, H, W, size)
        elif size is not None:
            d = preprocess.resample_u8(d, size)
        sxy = (float(np.float32(W / ow)), float(np.float32(H / oh))) if resampling else None
        staged[i] = _Frame(d, oh, ow, org, ready, sxy, src if keep_source else None)
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
                res["boxes"] = _scale_boxes(res["boxes"], *fr.scale_xy)
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
            idx = _frame_index(ks, device)
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
            res["overlay"] = pics[-1]
            res["overlay_boxes"] = _scale_boxes(res["boxes"], float(np.float32(ow / W)), float(np.float32(oh / H)))
            ks.append(res["boxes"].shape[0])
        if sum(ks):
            idx = _frame_index(ks, device)
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
        tiles_d = _pinned_upload(tiles, device)
        n = tiles.shape[0]
        x = torch.empty((n, 3, 1024, 1024), device=device, dtype=torch.float32)
        N.check(N.lib().wm_tile_frames_u8(N.ptr(desc_d), len(used), N.ptr(tiles_d), N.ptr(x), n, N.stream_ptr(device)))
        if resampling:                        # each tile's content extent (w, h): boxes normalised to the content
            ext = np.array([(min(1024, staged[f].width - o[1]), min(1024, staged[f].height - o[0]))
                            for f, t0, t1 in b.segments for o in staged[f].origins[t0:t1]], dtype=np.float32)
            rec = model.detect(x, _pinned_upload(ext, device))["records"]
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
            org_d = _pinned_upload(np.array([o for f in b.completes for o in staged[f].origins], dtype=np.int32), device)
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
