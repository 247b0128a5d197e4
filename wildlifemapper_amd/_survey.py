"""What the survey modules (tiling, review, ground, registration) share on the host: the frame descriptors the kernels read,
the validation of one survey frame, the pinned upload of a small host table, and the two scalar validators behind every
_check_* helper.  Nothing here launches a kernel."""
from __future__ import annotations

import math
from typing import List

import numpy as np

import torch


def _pinned_upload(a, dev: torch.device) -> torch.Tensor:
    """A host array or CPU tensor -> `dev` through pinned memory, without blocking the host."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().to(dev, non_blocking=True)


def _frame_descs(frames: List[torch.Tensor], device: torch.device) -> torch.Tensor:
    """wm_frame_desc of each contiguous (H,W,3) uint8 device frame -- data pointer, then (height, width) as two int32 in
    one int64 -- uploaded to `device` through pinned memory without blocking the host."""
    desc = np.zeros((len(frames), 2), dtype=np.int64)
    for j, fr in enumerate(frames):
        desc[j, 0] = fr.data_ptr()
        desc[j, 1] = np.array(fr.shape[:2], dtype=np.int32).view(np.int64)[0]
    return _pinned_upload(desc, device)


def _frame_index(counts, dev: torch.device) -> torch.Tensor:
    """The frame index of every detection, (sum(counts),) int32 on dev: counts[f] times f, in frame order."""
    return _pinned_upload(np.repeat(np.arange(len(counts), dtype=np.int32), counts), dev)


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


def _finite_number(value, what: str, name: str, ok, must: str, not_a_number: str = "is not a number", refuse=(),
                   echo_float: bool = False) -> float:
    """float(value) when that is finite and ok() of it holds, before any device work.  Else ValueError "{what}: {name}
    {value!r} ..." ending in not_a_number when value is no number (or of a type in `refuse`), in `must` when it is the wrong
    one; echo_float: the wrong number is shown as the float it became."""
    try:
        if isinstance(value, refuse):
            raise TypeError
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} {value!r} {not_a_number}") from None
    if not (math.isfinite(v) and ok(v)):
        raise ValueError(f"{what}: {name} {v if echo_float else value!r} {must}")
    return v


def _whole_number(value, what: str, name: str, lo: int, hi=None, multiple: int = 1, must: str = "", not_whole=None,
                  floats: bool = False) -> int:
    """int(value) when it is a whole number (no bool; floats: a float without a fraction counts) in lo..hi (hi None: no
    upper end) that `multiple` divides, before any device work.  Else ValueError "{what}: {name} {value!r} ..." ending in
    not_whole (None: must) for what is no whole number and in `must` for one outside the range."""
    kinds = (int, float, np.integer, np.floating) if floats else (int, np.integer)
    if isinstance(value, bool) or not isinstance(value, kinds) or (floats and not (math.isfinite(value) and value == int(value))):
        raise ValueError(f"{what}: {name} {value!r} {must if not_whole is None else not_whole}")
    if value < lo or (hi is not None and value > hi) or value % multiple:
        raise ValueError(f"{what}: {name} {value!r} {must}")
    return int(value)


def _check_fill(fill, what: str) -> np.ndarray:
    """fill= of mosaic() and undistort_u8(): three whole numbers in 0..255, as (3,) uint8, before any device work."""
    try:
        fill_a = np.asarray(fill)
        if fill_a.shape != (3,) or fill_a.dtype.kind not in "iuf" or not np.all((fill_a >= 0) & (fill_a <= 255) & (fill_a == np.floor(fill_a))):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: fill {fill!r} must be three whole numbers in 0..255") from None
    return fill_a.astype(np.uint8)


def _check_whole(value, what: str, name: str, lo: int = 1) -> int:
    """A whole number >= lo (an int, or a float without a fraction), before any device work."""
    return _whole_number(value, what, name, lo, must=f"must be a whole number >= {lo}", floats=True)
