"""Hungarian matcher (reference: segment_anything/modeling/matcher.py:11-85), on the GPU.

The reference builds the cost matrix on the device, copies it to the host and calls scipy's linear_sum_assignment once per
image (:77-80).  Here cost and assignment are HIP kernels (wm_criterion, csrc/criterion_kernels.h): the same algorithm
(shortest augmenting paths with duals, in double on the fp32 costs), one workgroup per image, nothing on the host.
`forward` keeps the reference's return value, which is a list of index tensors and therefore reads the matches back;
SetCriterion (build_sam.py) uses `match` instead, which stays on the device.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
from torch import nn

from ... import _native as N
from ...engine import criterion_native


def pack_targets(targets, device) -> Tuple[torch.Tensor, torch.Tensor, List[int]]:
    """The images' targets packed for wm_criterion: (total,4) fp32 boxes, (total,) int32 labels, counts per image.  No
    synchronisation: the counts come from the tensors' shapes."""
    sizes = [int(t["boxes"].shape[0]) for t in targets]
    for t in targets:
        for k in ("boxes", "labels"):
            if t[k].device != device:
                raise RuntimeError(f"target {k}: tensor is on {t[k].device}, the predictions on {device}; move the targets to the "
                                   "predictions' device first, as evaluate does (there is no CPU fallback in wildlifemapper_amd)")
    if sum(sizes) == 0:
        return (torch.empty((0, 4), device=device, dtype=torch.float32), torch.empty((0,), device=device, dtype=torch.int32), sizes)
    boxes = torch.cat([t["boxes"].reshape(-1, 4) for t in targets]).to(dtype=torch.float32).contiguous()
    labels = torch.cat([t["labels"].reshape(-1) for t in targets]).to(dtype=torch.int32).contiguous()
    return boxes, labels, sizes


def raise_on_status(status: torch.Tensor) -> None:
    """Reads the per-image status words back; a set bit raises (scipy raises on a non-finite cost matrix, matcher.py:80)."""
    st = status.cpu().tolist()
    bad = [(i, s) for i, s in enumerate(st) if s]
    if bad:
        what = "; ".join(f"image {i}: " + ("non-finite cost matrix or label outside 0..6" if s & N.CRITERION_NONFINITE else "assignment not solved")
                         for i, s in bad)
        raise RuntimeError("HungarianMatcher: " + what)


class HungarianMatcher(nn.Module):
    """Assignment between the targets and the predictions of the network (matcher.py:11-31)."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"

    @torch.no_grad()
    def match(self, outputs, targets, eos_coef: float = 1.0, debug: bool = False) -> Dict[str, torch.Tensor]:
        """Device-side result of one batch: {'match' (B,51) int32, 'sums' (8,) float64, 'status' (B,) int32, 'sizes'}
        (+ 'cost', 'dual_u', 'dual_v' with debug), see wm_criterion in include/wm_hip.h.  Asynchronous."""
        logits = outputs["pred_logits"]
        N.require_cuda(logits, "pred_logits")
        boxes, labels, sizes = pack_targets(targets, logits.device)
        r = criterion_native(logits, outputs["pred_boxes"], boxes, labels, sizes,
                             float(self.cost_class), float(self.cost_bbox), float(self.cost_giou), float(eos_coef), debug)
        r["sizes"] = sizes
        return r

    @torch.no_grad()
    def forward(self, outputs, targets):
        """List over the batch of (index_i, index_j) int64 tensors: the selected predictions in ascending order and their
        targets, len = min(51, targets of the image) (matcher.py:47-53, :81)."""
        r = self.match(outputs, targets)
        raise_on_status(r["status"])
        m = r["match"].cpu()
        out = []
        for b in range(m.shape[0]):
            idx = torch.nonzero(m[b] >= 0).flatten()
            out.append((idx.to(torch.int64), m[b][idx].to(torch.int64)))
        return out


def build_matcher(args):
    return HungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox, cost_giou=args.set_cost_giou)
