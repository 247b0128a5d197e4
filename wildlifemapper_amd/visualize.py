"""Prediction plots (reference: wildlifemapper/visualize_prediction.py:118-169), made on the GPU.

The reference runs the model on each validation tile, cuts the scores, applies the NMS, stretches the normalised tile to
0..255, draws every kept box in its class colour and writes prediction_plots/<image_id>.jpg.  Here
  * plot_points prepares the tile with wm_plot_image_u8 -- transpose, the cvtColor channel swap, `-= min`, `/= max`,
    `np.int32(* 255)`, bit for bit what numpy makes of those lines -- and draws the boxes with wm_draw_boxes_u8;
  * save_plot writes the picture on the host with PIL (the reference calls cv2.imwrite, which takes B, G, R);
  * visualize_predictions follows the reference's loop, with the score cut and the NMS of the existing post-process
    kernel (PostProcess.forward_with_nms).

What stays unpinned: cv2 is not installed, so neither cv2.cvtColor nor cv2.rectangle is matched against OpenCV.  The
channel swap is restated as "channels 0 and 2 change places"; the outline is the rule of include/wm_hip.h -- Pillow's
inward border of `width` pixels -- where OpenCV's thickness-2 line straddles the box edge.  The JPEG bytes are the host
encoder's and are not compared.  Text labels on the boxes are not drawn.
"""
from __future__ import annotations

import os
from typing import Sequence

import numpy as np
import torch

from . import _native as N
from . import review, tiling

PLOT_SCRATCH_BYTES = 1024          # include/wm_hip.h WM_PLOT_SCRATCH_BYTES, per image


def plot_image(image: torch.Tensor) -> torch.Tensor:
    """(3,H,W) or (B,3,H,W) fp32 on a ROCm device -> (H,W,3) or (B,H,W,3) uint8 (wm_plot_image_u8): per image
    out[y][x][c] = int(((v - mn) / mx) * 255) in fp32, v = image[2 - c][y][x], mn the image's minimum and mx its range.
    A constant image gives zeros.  Runs on the current stream."""
    N.require_cuda(image, "plot_image: image")
    if image.dim() not in (3, 4) or image.shape[-3] != 3 or image.shape[-1] <= 0 or image.shape[-2] <= 0:
        raise RuntimeError(f"plot_image: expected a (3,H,W) or (B,3,H,W) tensor, got {tuple(image.shape)}")
    single = image.dim() == 3
    B = 1 if single else image.shape[0]
    H, W = int(image.shape[-2]), int(image.shape[-1])
    out = torch.empty((B, H, W, 3), device=image.device, dtype=torch.uint8)
    if B:
        scratch = torch.empty(B * PLOT_SCRATCH_BYTES, device=image.device, dtype=torch.uint8)
        with torch.cuda.device(image.device):
            N.check(N.lib().wm_plot_image_u8(N.ptr(image), B, H, W, N.ptr(out), N.ptr(scratch), scratch.numel(), N.stream_ptr(image.device)))
    return out[0] if single else out


def _per_image(seq, B: int, single: bool, what: str):
    if single:
        return [seq]
    seq = list(seq)
    if len(seq) != B:
        raise RuntimeError(f"plot_points: {len(seq)} {what} entries for a batch of {B} images")
    return seq


def plot_points(image: torch.Tensor, labels, boxes, width: int = 2, palette=None) -> torch.Tensor:
    """The reference's plot_points without the file: image (3,H,W) fp32 on a ROCm device with labels (k,) and boxes (k,4)
    xyxy in its pixels, or a batch (B,3,H,W) with one labels / boxes entry per image -> the uint8 picture(s) (...,H,W,3)
    on the device, channels in the order the reference hands to cv2.imwrite (save_plot writes them).  Boxes are drawn in
    the order given, later over earlier, `width` pixels inward (tiling.draw_boxes).  palette: (P,3) uint8, row `label`
    written as it is -- the reference's table is given in that order; None: tiling.DEFAULT_PALETTE with each row reversed,
    so a label has the colour in the saved file that it has on a survey overlay."""
    width = review._check_draw_width(width, "plot_points")
    pal = review._check_palette(palette, "plot_points") if palette is not None else np.ascontiguousarray(tiling.DEFAULT_PALETTE[:, ::-1])
    pic = plot_image(image)
    single = image.dim() == 3
    B = 1 if single else image.shape[0]
    dev = image.device
    bs = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4).to(dev) for b in _per_image(boxes, B, single, "boxes")]
    ls = [torch.as_tensor(l).reshape(-1).to(dev) for l in _per_image(labels, B, single, "labels")]
    for j, (b, l) in enumerate(zip(bs, ls)):
        if b.shape[0] != l.shape[0]:
            raise RuntimeError(f"plot_points: image {j}: {b.shape[0]} boxes, {l.shape[0]} labels")
    if B and sum(b.shape[0] for b in bs):
        frames = [pic] if single else list(pic.unbind(0))
        idx = torch.from_numpy(np.repeat(np.arange(B, dtype=np.int32), [b.shape[0] for b in bs])).to(dev)
        tiling.draw_boxes(frames, torch.cat(bs).contiguous(), torch.cat(ls).to(torch.int64), idx, width, pal)
    return pic


def save_plot(path: str, array) -> None:
    """Write a picture of plot_points -- (H,W,3) uint8, channels as cv2.imwrite takes them -- with PIL on the host: the
    channels are reversed first.  The format follows the file name, as with cv2.imwrite."""
    from PIL import Image
    if isinstance(array, torch.Tensor):
        array = array.detach().cpu().numpy()
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"save_plot: expected an (H,W,3) uint8 array, got {a.dtype} {a.shape}")
    Image.fromarray(np.ascontiguousarray(a[..., ::-1])).save(path)


@torch.no_grad()
def visualize_predictions(model, postprocessors, data_loader, out_dir: str, threshold: float = 0.5, iou_thr: float = 0.4,
                          max_steps: int = 241, sizes: str = "orig", width: int = 2, palette=None, device=None) -> Sequence[str]:
    """The reference's plotting loop (visualize_prediction.py:137-169): for each batch of `data_loader` run the model,
    post-process against the target sizes, keep scores > threshold, apply the class-agnostic NMS (iou_thr) -- both in the
    existing post-process kernel, PostProcess.forward_with_nms -- and write out_dir/<image_id>.jpg for the batch's FIRST
    image, as the reference does; it stops after max_steps batches (the reference: 241).  Returns the paths written.
    sizes="orig" (the reference): boxes are scaled to each target's 'orig_size' and drawn, as they are, onto the padded
    model canvas -- they fit the picture only where orig_size is the canvas size.  sizes="canvas": boxes are scaled to
    the canvas (H, W) of the batch instead, so they lie on the pixels shown."""
    if sizes not in ("orig", "canvas"):
        raise ValueError(f"visualize_predictions: sizes {sizes!r} must be 'orig' or 'canvas'")
    width = review._check_draw_width(width, "visualize_predictions")
    if palette is not None:
        palette = review._check_palette(palette, "visualize_predictions")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    os.makedirs(out_dir, exist_ok=True)
    model.eval()
    written = []
    for step, data in enumerate(data_loader):
        if step >= max_steps:
            break
        image, targets = data[0], data[1]
        targets = [{k: (v.to(device) if hasattr(v, "to") else v) for k, v in t.items()} for t in targets]
        b, c, h, w = image.tensors.shape
        boxes_np = np.repeat(np.array([[0, 0, h, w]]), b, axis=0)
        image = image.to(device)
        outputs = model(image, boxes_np)
        if sizes == "orig":
            target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)
        else:
            target_sizes = torch.tensor([[h, w]] * b, device=device)
        res = postprocessors["bbox"].forward_with_nms(outputs, target_sizes, threshold, iou_thr)[0]
        pic = plot_points(image.tensors[0].float().contiguous(), res["labels"], res["boxes"].contiguous(), width, palette)
        image_id = int(torch.as_tensor(targets[0]["image_id"]).reshape(-1)[0].item())
        path = os.path.join(out_dir, f"{image_id}.jpg")
        save_plot(path, pic)
        written.append(path)
    return written
