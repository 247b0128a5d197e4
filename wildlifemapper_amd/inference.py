"""Drop-in `evaluate` harness (reference: wildlifemapper/inference.py:30-89).

Same signature, loop shape and return contract: for each (NestedTensor, targets) batch run the model, PostProcess the
outputs against `orig_size`, hand the per-image results to a CocoEvaluator built on `base_ds`, then
synchronize -> accumulate -> summarize and return `(stats, coco_evaluator)` with
`stats['coco_eval_bbox'] = coco_evaluator.coco_eval['bbox'].stats.tolist()` (inference.py:72-89).

Differences, all outside the accelerated path:
  * the loss (`criterion`) may be None or return an empty dict (a model built without the criterion's `args`).  With the
    SetCriterion that `_build_sam(args=...)` returns, `stats` carries the reference's keys (inference.py:52-64, :84):
    `loss`, each `weight_dict` key scaled, every key `_unscaled`, `class_error`, each the mean over batches and ranks as
    MetricLogger.global_avg gives it; the sums stay on the device and are read back once after the loop, where a batch
    whose targets could not be matched (non-finite cost matrix) raises RuntimeError.  The entries of any other
    criterion are averaged into `stats` under their own names;
  * COCO mAP is computed by the build's own evaluator (coco_eval.py): pycocotools, which the reference imports
    (inference.py:15-18), is absent from this image, so that parity is unpinned;
  * `base_ds` may be a pycocotools-like object with `.dataset`, a COCO-format dict (coco_annotations/*.json) or a path;
    with `base_ds=None` no evaluator is built and `(stats, None)` is returned, as the reference's `if coco_evaluator is
    not None` branches allow;
  * detections are merged across ranks as fixed-size records by one padded all-gather (dist.gather_detections), not by
    pickling (utils/misc.py:180-220); `stats['images']` / `stats['detections']` count the MERGED set (each image once,
    although DistributedSampler repeats images to pad the last shard).
"""
from __future__ import annotations

from collections import defaultdict
from typing import Dict

import numpy as np
import torch

from .coco_eval import CocoEvaluator
from .segment_anything.utils import misc as utils


@torch.no_grad()
def evaluate(model, criterion, postprocessors, data_loader, base_ds, device, args):
    model.eval()
    if criterion is not None:
        criterion.eval()
    iou_types = tuple(k for k in ("bbox", "segm") if k in postprocessors.keys())
    coco_evaluator = CocoEvaluator(base_ds, iou_types) if base_ds is not None else None
    loss_sums: Dict[str, float] = defaultdict(float)
    n_batches = 0
    ref_keys, ref_sums, ref_bad = None, None, None   # the reference's loss stats: key order, device sums, batches with a status set
    seen: Dict[int, int] = {}                     # image id -> detections (this rank), used when no evaluator merges
    for data in data_loader:
        image, targets = data[0], data[1]
        targets = [{k: (v.to(device) if hasattr(v, "to") else v) for k, v in t.items()} for t in targets]
        # whole image as the prompt, as inference.py:47-49 builds it (MedSAM.forward ignores it, network.py:69-78)
        b, c, h, w = image.tensors.shape
        boxes_np = np.repeat(np.array([[0, 0, h, w]]), getattr(args, "batch_size", b), axis=0)
        image = image.to(device)
        outputs = model(image, boxes_np)
        if criterion is not None:
            loss_dict = criterion(outputs, targets) or {}
            weight_dict = getattr(criterion, "weight_dict", None)
            if loss_dict and weight_dict and all(torch.is_tensor(v) for v in loss_dict.values()):
                # inference.py:52-64, accumulated on the device
                red = {k: v.double() for k, v in utils.reduce_dict(loss_dict).items()}       # scaled and summed in double
                scaled = {k: v * weight_dict[k] for k, v in red.items() if k in weight_dict}
                entries = {"loss": sum(scaled.values()), **scaled, **{f"{k}_unscaled": v for k, v in red.items()}}
                if "class_error" in red:
                    entries["class_error"] = red["class_error"]
                vec = torch.stack([entries[k].double().reshape(()) for k in entries])
                if ref_keys is None:
                    ref_keys, ref_sums = list(entries), torch.zeros_like(vec)
                    ref_bad = torch.zeros((), dtype=torch.int64, device=vec.device)
                ref_sums += vec
                status = getattr(criterion, "last_status", None)
                if status is not None:
                    ref_bad += (status != 0).any().to(torch.int64)
            else:
                for k, v in loss_dict.items():
                    loss_sums[k] += float(v)
        n_batches += 1
        orig_target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)
        results = postprocessors["bbox"](outputs, orig_target_sizes)
        res = {int(target["image_id"].item()): output for target, output in zip(targets, results)}
        for k, o in res.items():
            seen[k] = len(o["scores"])
        if coco_evaluator is not None:
            coco_evaluator.update(res)

    # gather the stats from all processes (inference.py:70-76)
    if coco_evaluator is not None:
        coco_evaluator.synchronize_between_processes()
        coco_evaluator.accumulate()
        coco_evaluator.summarize()
    stats = {k: v / max(n_batches, 1) for k, v in loss_sums.items()}
    if ref_keys is not None:
        # MetricLogger.synchronize_between_processes + global_avg (utils/misc.py): total / count over all ranks; one read-back
        tot = utils.all_reduce_sum(torch.cat([ref_sums, ref_bad.double().reshape(1), ref_sums.new_tensor([float(n_batches)])])).cpu()
        if tot[-2] > 0:
            raise RuntimeError(f"evaluate: the targets of {int(tot[-2])} batch(es) could not be matched to the predictions "
                               "(non-finite cost matrix or a label outside 0..6); criterion.check_status() names the images of the last one")
        stats.update({k: float(tot[i] / tot[-1]) for i, k in enumerate(ref_keys)})
    # images / detections of the whole job, each image once: DistributedSampler pads the last shard with repeats, so a sum
    # over ranks would count those twice; the evaluator's merged set (or, without an evaluator, the same merge) does not
    if coco_evaluator is not None:
        ev = coco_evaluator.coco_eval["bbox"]
        stats["images"] = float(len(coco_evaluator.img_ids))
        stats["detections"] = float(sum(len(v) for v in ev.dts.values()))
    else:
        from . import dist as wdist
        merged = wdist.gather_detections({k: {"boxes": np.zeros((0, 4), np.float32), "scores": np.zeros((0,), np.float32),
                                              "labels": np.zeros((0,), np.int64)} for k in seen})
        stats["images"] = float(len(merged))
        if utils.get_world_size() > 1:
            t = torch.tensor([float(sum(seen.values()))], dtype=torch.float64)
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.distributed.get_backend() == "nccl" else torch.device("cpu")
            t = t.to(dev)
            torch.distributed.all_reduce(t)
            stats["detections"] = float(t.item())       # no evaluator: upper bound (sampler repeats counted per rank)
        else:
            stats["detections"] = float(sum(seen.values()))
    if coco_evaluator is not None and "bbox" in postprocessors.keys():
        stats["coco_eval_bbox"] = coco_evaluator.coco_eval["bbox"].stats.tolist()
    return stats, coco_evaluator
