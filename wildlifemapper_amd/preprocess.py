"""Input pipeline on the GPU: uint8 HWC frames -> the model's (B,3,1024,1024) fp32 input."""
from __future__ import annotations

import torch

from . import _native as N


def resized_size(height: int, width: int, size: int = 768, max_size: int = 768):
    """(oh, ow) of the val transform's resize (augmentation.py:80-99), from the library (wm_resized_size; host-only call)."""
    import ctypes as C
    oh, ow = C.c_int(), C.c_int()
    N.check(N.lib().wm_resized_size(height, width, size, max_size, C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def tiles_from_u8(images: torch.Tensor, resize=None) -> torch.Tensor:
    """images: (B,h,w,3) uint8 on a ROCm device.  Returns ToTensor + ImageNet-normalised tiles, top-left aligned on a zero
    1024x1024 canvas (utils/misc.py:46-67).  resize=None: h, w <= 1024, no resampling (wm_preprocess_u8).
    resize=(size, max_size), e.g. (768, 768) as the val pipeline (dataloader_coco.py:288): frames of any size are first
    resampled with PIL's bilinear arithmetic (wm_preprocess_u8_resized); the content occupies resized_size(h, w, ...)."""
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise RuntimeError(f"tiles_from_u8: expected a (B,h,w,3) uint8 ROCm tensor, got {tuple(images.shape)} {images.dtype} on {images.device}")
    images = images.contiguous()
    B, h, w, _ = images.shape
    out = torch.empty((B, 3, 1024, 1024), device=images.device, dtype=torch.float32)
    with torch.cuda.device(images.device):
        if resize is None:
            N.check(N.lib().wm_preprocess_u8(N.ptr(images), N.ptr(out), B, h, w, N.stream_ptr(images.device)))
        else:
            size, max_size = resize
            N.check(N.lib().wm_preprocess_u8_resized(N.ptr(images), N.ptr(out), B, h, w, int(size), int(max_size or 0), N.stream_ptr(images.device)))
    return out


def _check_undistort_args(sample, fill, what: str):
    """(wm_undistort_u8's mode, the three fill bytes) of sample= and fill=, before any device work."""
    from ._survey import _check_fill
    from .ground import MOSAIC_SAMPLES
    if not isinstance(sample, str) or sample not in MOSAIC_SAMPLES:
        raise ValueError(f"{what}: sample {sample!r} must be 'bilinear' or 'nearest'")
    return MOSAIC_SAMPLES[sample], _check_fill(fill, what)


def _check_plan_frame(frame, pl, what: str) -> None:
    """The frame of undistort_u8, rectify_u8 and ortho_u8: an (H,W,3) uint8 ROCm tensor of the plan's size."""
    if not isinstance(frame, torch.Tensor) or not frame.is_cuda or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3:
        got = f"{tuple(frame.shape)} {frame.dtype} on {frame.device}" if isinstance(frame, torch.Tensor) else type(frame).__name__
        raise RuntimeError(f"{what}: expected an (H,W,3) uint8 ROCm tensor, got {got}")
    if tuple(frame.shape[:2]) != tuple(pl["size"]):
        raise ValueError(f"{what}: frame is {tuple(frame.shape[:2])}, the plan was made for {tuple(pl['size'])}")


def undistort_u8(frame: torch.Tensor, plan, sample: str = "bilinear", fill=(0, 0, 0), count: bool = False):
    """frame (H,W,3) uint8 on a ROCm device -> its pinhole picture (oh,ow,3) uint8 on the same device, by the dict
    lens.lens_plan() returned (wm_undistort_u8; rule: include/wm_hip.h "Survey lens").  sample: 'bilinear' (pixel centres at
    integer + 0.5, edge replicate) or 'nearest', the mosaic's sampling; fill: the (r, g, b) of the pixels that look outside
    the frame.  Every output byte is written.  count=True: returns (picture, filled), filled a device int64 tensor of one
    element, the number of filled pixels, without a host synchronisation.  A frame whose shape is not plan['size'] is
    refused.  Runs on the current stream; everything is validated before any device work."""
    from .lens import _check_plan
    what = "undistort_u8"
    return _resample_by_plan(frame, _check_plan(plan, what), None, sample, fill, count, what)


def rectify_u8(frame: torch.Tensor, plan, sample: str = "bilinear", fill=(0, 0, 0), count: bool = False):
    """frame (H,W,3) uint8 on a ROCm device -> the picture (oh,ow,3) uint8 a level camera at the same place would have taken,
    by the dict attitude.rectify_plan() returned: the plan's rotation and lens model in one gather (wm_rectify_u8; rule:
    include/wm_hip.h "Survey attitude").  sample, fill, count, the frame's shape, the stream and the validation are
    undistort_u8's; the filled pixels include those that look away from the camera's front (Z <= 0)."""
    from .attitude import _check_rectify_plan
    what = "rectify_u8"
    pl = _check_rectify_plan(plan, what)
    return _resample_by_plan(frame, pl, pl["rotation"], sample, fill, count, what)


def _resample_by_plan(frame, pl, rotation, sample, fill, count: bool, what: str):
    """undistort_u8 (rotation None) and rectify_u8 on a validated plan."""
    import ctypes as C
    mode, fill_a = _check_undistort_args(sample, fill, what)
    _check_plan_frame(frame, pl, what)
    (h, w), (oh, ow) = pl["size"], pl["out_size"]
    frame = frame.contiguous()
    cam = (C.c_double * 9)(*[float(v) for v in pl["camera"]])
    fill_c = (C.c_uint8 * 3)(*[int(v) for v in fill_a])
    with torch.cuda.device(frame.device):
        out = torch.empty((oh, ow, 3), device=frame.device, dtype=torch.uint8)
        filled = torch.empty(1, device=frame.device, dtype=torch.int64) if count else None
        tail = (N.ptr(out), oh, ow, float(pl["f_out"]), mode, fill_c, N.ptr(filled), N.stream_ptr(frame.device))
        if rotation is None:
            N.check(N.lib().wm_undistort_u8(N.ptr(frame), h, w, cam, *tail))
        else:
            rot = (C.c_double * 9)(*[float(v) for v in rotation.reshape(9)])
            N.check(N.lib().wm_rectify_u8(N.ptr(frame), h, w, cam, rot, *tail))
    return (out, filled) if count else out


def ortho_u8(frame: torch.Tensor, plan, dem, sample: str = "bilinear", fill=(0, 0, 0), count: bool = False):
    """frame (H,W,3) uint8 on a ROCm device -> its orthophoto (oh,ow,3) uint8 on the same device, by the dict
    terrain.ortho_plan() returned and the DEM it was made over, a terrain.terrain_grid(): pose, terrain height and lens model
    in one gather (wm_ortho_u8; rule: include/wm_hip.h "Survey terrain").  The DEM's posts are uploaded once and kept in the
    dict (terrain.to_device).  sample, fill, the frame's shape, the stream and the validation are undistort_u8's.  count=True:
    returns (picture, counts), counts a device int64 tensor of two elements, the filled pixels and those of them that had no
    height or a non-finite one (a DEM that is too small), without a host synchronisation."""
    import ctypes as C
    from .terrain import _check_ortho_plan, to_device
    what = "ortho_u8"
    pl, d = _check_ortho_plan(plan, dem, what)
    mode, fill_a = _check_undistort_args(sample, fill, what)
    _check_plan_frame(frame, pl, what)
    (h, w), (oh, ow) = pl["size"], pl["out_size"]
    (dh, dw), (e0, n0) = d["heights"].shape, d["origin"]
    frame = frame.contiguous()
    posts = to_device(dem, frame.device)
    cam = (C.c_double * 9)(*[float(v) for v in pl["camera"]])
    pose = (C.c_double * 12)(*[float(v) for v in pl["pose"]])
    dem_geo = (C.c_double * 3)(e0, n0, d["cell"])
    out_geo = (C.c_double * 6)(*[float(v) for v in pl["georef"].reshape(6)])
    fill_c = (C.c_uint8 * 3)(*[int(v) for v in fill_a])
    with torch.cuda.device(frame.device):
        out = torch.empty((oh, ow, 3), device=frame.device, dtype=torch.uint8)
        counts = torch.empty(2, device=frame.device, dtype=torch.int64) if count else None
        N.check(N.lib().wm_ortho_u8(N.ptr(frame), h, w, cam, pose, N.ptr(posts), dh, dw, dem_geo, N.ptr(out), oh, ow, out_geo, mode, fill_c,
                                    N.ptr(counts), N.stream_ptr(frame.device)))
    return (out, counts) if count else out


def scaled_size(height: int, width: int, scale: float):
    """(oh, ow) = (max(1, floor(height * scale + 0.5)), the same for width), in double (wm_scaled_size; host-only call)."""
    import ctypes as C
    oh, ow = C.c_int(), C.c_int()
    N.check(N.lib().wm_scaled_size(int(height), int(width), float(scale), C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def resample_u8(frame: torch.Tensor, size) -> torch.Tensor:
    """frame (H,W,3) uint8 on a ROCm device -> (oh,ow,3) uint8 on the same device, size = (oh, ow), any size to any size
    with PIL's bilinear arithmetic (wm_resample_u8: bit-exact with PIL.Image.resize).  Runs on the current stream."""
    if not frame.is_cuda or frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3:
        raise RuntimeError(f"resample_u8: expected an (H,W,3) uint8 ROCm tensor, got {tuple(frame.shape)} {frame.dtype} on {frame.device}")
    oh, ow = int(size[0]), int(size[1])
    frame = frame.contiguous()
    out = torch.empty((oh, ow, 3), device=frame.device, dtype=torch.uint8)
    with torch.cuda.device(frame.device):
        N.check(N.lib().wm_resample_u8(N.ptr(frame), frame.shape[0], frame.shape[1], N.ptr(out), oh, ow, N.stream_ptr(frame.device)))
    return out
