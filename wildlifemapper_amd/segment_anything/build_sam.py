"""Drop-in model factory (reference: segment_anything/build_sam.py:19-60, 212-334).

`build_sam(checkpoint=None, args=None)` and `sam_model_registry[...]` return the same
TUPLE `(sam, criterion, postprocessors)` as the reference (:334).  `sam` holds the HIP-backed
encoder / decoder / prompt encoder; `postprocessors['bbox']` is the HIP PostProcess.
`criterion` is the reference's pair when `args` carries its fields (set_cost_class, set_cost_bbox, set_cost_giou,
bbox_loss_coef, giou_loss_coef, eos_coef; :325-331): SetCriterion over a HungarianMatcher, both on the GPU (wm_criterion),
FORWARD only -- the validation losses `evaluate` logs (inference.py:52-64).  Gradients and the training loop stay out of
scope.  With `args=None`, or without those fields, `criterion` is a stub whose loss dict is empty (the reference would
crash there).
"""
from __future__ import annotations

from functools import partial
from typing import Dict, List, Optional

import torch
from torch import nn

from ..engine import postprocess_nms, split_records
from .. import _native as N
from .modeling import ImageEncoderViT, MaskDecoder, PromptEncoder, Sam, TwoWayTransformer
from .modeling.matcher import HungarianMatcher, build_matcher, raise_on_status
from .utils.misc import all_reduce_sum, get_world_size


def build_sam_vit_h(checkpoint=None, args=None):
    return _build_sam(encoder_embed_dim=1280, encoder_depth=32, encoder_num_heads=16,
                      encoder_global_attn_indexes=[7, 15, 23, 31], checkpoint=checkpoint, args=args)


build_sam = build_sam_vit_h


def build_sam_vit_l(checkpoint=None, args=None):
    return _build_sam(encoder_embed_dim=1024, encoder_depth=24, encoder_num_heads=16,
                      encoder_global_attn_indexes=[5, 11, 17, 23], checkpoint=checkpoint, args=args)


def build_sam_vit_b(checkpoint=None, args=None):
    return _build_sam(encoder_embed_dim=768, encoder_depth=12, encoder_num_heads=12,
                      encoder_global_attn_indexes=[2, 5, 8, 11], checkpoint=checkpoint, args=args)


sam_model_registry = {
    "default": build_sam_vit_h,
    "vit_h": build_sam_vit_h,
    "vit_l": build_sam_vit_l,
    "vit_b": build_sam_vit_b,
}


class InferenceCriterion(nn.Module):
    """Stand-in for SetCriterion (build_sam.py:62-210): inference computes no loss."""

    def __init__(self) -> None:
        super().__init__()
        self.weight_dict: Dict[str, float] = {}

    def forward(self, outputs, targets):
        return {}


CRITERION_ARGS = ("set_cost_class", "set_cost_bbox", "set_cost_giou", "bbox_loss_coef", "giou_loss_coef", "eos_coef")


class SetCriterion(nn.Module):
    """The DETR losses of the reference (build_sam.py:62-210), forward only, on the GPU: the Hungarian match and every
    sum are HIP kernels (wm_criterion); nothing is read back, so the returned 0-d tensors are still in flight.

    `forward` returns loss_ce, class_error, loss_bbox, loss_giou and cardinality_error as the reference does for
    losses = ['labels', 'boxes', 'cardinality'] (:93-147).  With no matched pair at all class_error is 100 (the
    reference's `accuracy` returns 0 for an empty target).  An image whose cost matrix is not finite cannot be matched
    (scipy raises there): every loss of that call is NaN, `last_status` holds the per-image status words and
    `check_status()` raises; `evaluate` checks once after its loop."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__()
        if num_classes != N.NUM_LOGITS - 1:
            raise NotImplementedError(f"SetCriterion: num_classes {num_classes}; the kernels are built for {N.NUM_LOGITS - 1} (+ no-object)")
        unknown = set(losses) - {"labels", "boxes", "cardinality"}
        assert not unknown, f"do you really want to compute {sorted(unknown)} loss?"
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.losses = losses
        empty_weight = torch.ones(self.num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)
        self.last_status: Optional[torch.Tensor] = None

    def check_status(self) -> None:
        """Synchronises on the last call's status words and raises RuntimeError if one is set."""
        if self.last_status is not None:
            raise_on_status(self.last_status)

    @torch.no_grad()
    def forward(self, outputs, targets):
        if "aux_outputs" in outputs:
            raise NotImplementedError("SetCriterion: auxiliary decoder outputs (training) are not built")
        r = self.matcher.match(outputs, targets, eos_coef=self.eos_coef)
        self.last_status = r["status"]
        sums = r["sums"]
        device = sums.device
        # the average number of target boxes across all nodes (:183-187), without leaving the device
        num_boxes = torch.as_tensor([float(sum(r["sizes"]))], dtype=torch.float64, device=device)
        num_boxes = torch.clamp(all_reduce_sum(num_boxes) / get_world_size(), min=1)[0]
        losses = {}
        if "labels" in self.losses:
            losses["loss_ce"] = (sums[0] / sums[1]).float()
            # no matched pair: 100; a NaN count (a status is set) is not == 0 and stays NaN like the other losses
            losses["class_error"] = torch.where(sums[4] == 0, torch.full_like(sums[4], 100.0), 100.0 - 100.0 * sums[5] / sums[4]).float()
        if "boxes" in self.losses:
            losses["loss_bbox"] = (sums[2] / num_boxes).float()
            losses["loss_giou"] = (sums[3] / num_boxes).float()
        if "cardinality" in self.losses:
            losses["cardinality_error"] = (sums[6] / len(r["sizes"])).float()
        return losses


class PostProcess(nn.Module):
    """Model output -> per-image {'scores','labels','boxes'} (build_sam.py:212-258), on the GPU.

    `forward` keeps the reference contract.  `forward_with_nms` additionally applies the
    score cut + class-agnostic NMS of visualize_prediction.py:150-157 in the same kernel and
    returns, per image, the kept indices in the order torchvision.ops.nms would.
    """

    def __init__(self, confidence_threshold: float = 0.05) -> None:
        super().__init__()
        self.confidence_threshold = confidence_threshold

    def _records(self, outputs, target_sizes, score_thr, iou_thr):
        out_logits, out_bbox = outputs["pred_logits"], outputs["pred_boxes"]
        assert len(out_logits) == len(target_sizes)
        assert target_sizes.shape[1] == 2
        rec = postprocess_nms(out_logits.contiguous().float(), out_bbox.contiguous().float(), target_sizes,
                              self.confidence_threshold, score_thr, iou_thr)
        return split_records(rec)

    @torch.no_grad()
    def forward(self, outputs, target_sizes) -> List[Dict[str, torch.Tensor]]:
        r = self._records(outputs, target_sizes, 0.5, 0.4)
        results = []
        for b in range(r["scores"].shape[0]):
            keep = (r["flags"][b] & N.FLAG_CONF) != 0
            results.append({"scores": r["scores"][b][keep], "labels": r["labels"][b][keep], "boxes": r["boxes"][b][keep]})
        return results

    @torch.no_grad()
    def forward_with_nms(self, outputs, target_sizes, score_threshold: float = 0.5, iou_threshold: float = 0.4):
        r = self._records(outputs, target_sizes, score_threshold, iou_threshold)
        results = []
        for b in range(r["scores"].shape[0]):
            flags, rank = r["flags"][b], r["nms_rank"][b]
            cand = (flags & N.FLAG_SCORE) != 0                       # results[0]['scores'] > threshold
            kept = (flags & N.FLAG_NMS) != 0
            # index of each slot inside the score-filtered list, then order kept slots by NMS rank
            pos_in_cand = torch.cumsum(cand.to(torch.int64), 0) - 1
            slots = torch.nonzero(kept).flatten()
            slots = slots[torch.argsort(rank[slots])]
            results.append({"scores": r["scores"][b][slots], "labels": r["labels"][b][slots], "boxes": r["boxes"][b][slots],
                            "nms_index": pos_in_cand[slots], "slots": slots})
        return results


def _build_sam(encoder_embed_dim, encoder_depth, encoder_num_heads, encoder_global_attn_indexes, checkpoint=None, args=None):
    prompt_embed_dim = 256
    image_size = 1024
    vit_patch_size = 16
    image_embedding_size = image_size // vit_patch_size
    sam = Sam(
        image_encoder=ImageEncoderViT(
            depth=encoder_depth, embed_dim=encoder_embed_dim, img_size=image_size, mlp_ratio=4,
            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_heads=encoder_num_heads, patch_size=vit_patch_size,
            qkv_bias=True, use_rel_pos=True, global_attn_indexes=encoder_global_attn_indexes, window_size=14,
            out_chans=prompt_embed_dim),
        prompt_encoder=PromptEncoder(embed_dim=prompt_embed_dim,
                                     image_embedding_size=(image_embedding_size, image_embedding_size),
                                     input_image_size=(image_size, image_size), mask_in_chans=16),
        mask_decoder=MaskDecoder(num_multimask_outputs=50,
                                 transformer=TwoWayTransformer(depth=2, embedding_dim=prompt_embed_dim, mlp_dim=2048, num_heads=8),
                                 transformer_dim=prompt_embed_dim, iou_head_depth=3, iou_head_hidden_dim=256),
        pixel_mean=[123.675, 116.28, 103.53], pixel_std=[58.395, 57.12, 57.375])
    sam.eval()
    precision = getattr(args, "wm_precision", None) if args is not None else None
    if precision:
        sam.image_encoder._hub.set_precision(precision)
    if checkpoint is not None:
        # build_sam.py:311-322: SAM checkpoint, mask_decoder.* keys without 'transformer' dropped, strict=False
        state_dict = torch.load(checkpoint, map_location="cpu", weights_only=True)
        if isinstance(state_dict, dict) and "model" in state_dict and isinstance(state_dict["model"], dict):
            state_dict = state_dict["model"]
        for k in [k for k in state_dict if "mask_decoder" in k and "transformer" not in k]:
            del state_dict[k]
        sam.load_state_dict(state_dict, strict=False)
    if args is not None and all(hasattr(args, k) for k in CRITERION_ARGS):
        # build_sam.py:324-332.  `empty_weight` is kept for the reference's surface only: the kernels take eos_coef as a scalar
        weight_dict = {"loss_ce": 3, "loss_bbox": args.bbox_loss_coef, "loss_giou": args.giou_loss_coef}
        criterion = SetCriterion(6 + 1, matcher=build_matcher(args), weight_dict=weight_dict, eos_coef=args.eos_coef,
                                 losses=["labels", "boxes", "cardinality"])
    else:
        criterion = InferenceCriterion()
    postprocessors = {"bbox": PostProcess(confidence_threshold=0.05)}
    return sam, criterion, postprocessors
