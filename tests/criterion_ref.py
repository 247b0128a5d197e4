"""Restatement of the reference's validation losses for the tests: HungarianMatcher (segment_anything/modeling/matcher.py:
33-81), the forward losses of SetCriterion (build_sam.py:93-147), utils/box_ops.py:9-61 and utils/misc.py accuracy, in
torch on the CPU at a chosen dtype, with the assignment solved here (no scipy: nothing in the repository imports it, and
the GPU machine may not have it).  tests/golden/criterion_ref.npz, recorded from the reference's own code and scipy
(tools/gen_criterion_golden.py), pins it: tests/test_criterion_cpu.py.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

NUM_QUERIES, NO_OBJECT = 51, 7


def box_cxcywh_to_xyxy(x):
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([x_c - 0.5 * w, y_c - 0.5 * h, x_c + 0.5 * w, y_c + 0.5 * h], dim=-1)


def box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def generalized_box_iou(b1, b2):
    """[N, M] pairwise GIoU of xyxy boxes (box_ops.py:24-61)."""
    area1, area2 = box_area(b1), box_area(b2)
    wh = (torch.min(b1[:, None, 2:], b2[:, 2:]) - torch.max(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area1[:, None] + area2 - inter
    iou = inter / union
    wh = (torch.max(b1[:, None, 2:], b2[:, 2:]) - torch.min(b1[:, None, :2], b2[:, :2])).clamp(min=0)
    area = wh[:, :, 0] * wh[:, :, 1]
    return iou - (area - union) / area


def cost_matrices(logits, boxes, tgt_boxes: Sequence[torch.Tensor], tgt_labels: Sequence[torch.Tensor], weights, dtype=torch.float32):
    """Per image the (51, T) cost matrix of matcher.py:57-76; weights = (cost_class, cost_bbox, cost_giou)."""
    w_class, w_bbox, w_giou = weights
    out = []
    for b in range(logits.shape[0]):
        prob = logits[b].to(dtype).softmax(-1)
        pb, tb = boxes[b].to(dtype), tgt_boxes[b].to(dtype).reshape(-1, 4)
        cost_class = -prob[:, tgt_labels[b].long()]
        cost_bbox = (pb[:, None, :] - tb[None, :, :]).abs().sum(-1)
        cost_giou = -generalized_box_iou(box_cxcywh_to_xyxy(pb), box_cxcywh_to_xyxy(tb))
        out.append(w_bbox * cost_bbox + w_class * cost_class + w_giou * cost_giou)
    return out


def solve(cost) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Rectangular linear sum assignment by shortest augmenting paths with duals (the algorithm of scipy's
    linear_sum_assignment, in float64, ties to the lowest column).  Returns (row_ind ascending, col_ind, u, v) with
    u[i] + v[j] <= cost[i, j], equality on the assignment."""
    c = np.asarray(cost, dtype=np.float64)
    if c.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(c.shape[0]), np.zeros(c.shape[1])
    if not np.isfinite(c).all():
        raise ValueError("matrix contains invalid numeric entries")
    transposed = c.shape[1] < c.shape[0]
    if transposed:
        c = c.T
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        sp = np.full(nc, np.inf)
        path = np.full(nc, -1)
        sr, sc = np.zeros(nr, bool), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            sr[i] = True
            r = min_val + c[i] - u[i] - v
            upd = ~sc & (r < sp)
            sp[upd] = r[upd]
            path[upd] = i
            j = int(np.argmin(np.where(sc, np.inf, sp)))          # first minimum = lowest index
            min_val = sp[j]
            assert np.isfinite(min_val)
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
            sc[j] = True
        u[cur] += min_val
        for i in np.nonzero(sr)[0]:
            if i != cur:
                u[i] += min_val - sp[col4row[i]]
        v[sc] -= min_val - sp[sc]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows, cols = np.arange(nr), col4row.copy()
    if transposed:
        order = np.argsort(cols)
        rows, cols, u, v = cols[order], rows[order], v, u
    return rows.astype(np.int64), cols.astype(np.int64), u, v


def match(costs) -> List[Tuple[np.ndarray, np.ndarray]]:
    return [solve(c.double().numpy())[:2] for c in costs]


def losses(logits, boxes, tgt_boxes, tgt_labels, indices, eos_coef: float, dtype=torch.float64, world_size: int = 1) -> Dict[str, float]:
    """loss_ce, class_error, loss_bbox, loss_giou, cardinality_error of build_sam.py:93-147, 183-187 for one batch on one
    rank.  class_error is 100 when nothing is matched (the reference's `accuracy` returns 0 there)."""
    B = logits.shape[0]
    lg = logits.to(dtype)
    target = torch.full((B, NUM_QUERIES), NO_OBJECT, dtype=torch.int64)
    for b, (i, j) in enumerate(indices):
        target[b, torch.as_tensor(i, dtype=torch.int64)] = tgt_labels[b].long()[torch.as_tensor(j, dtype=torch.int64)]
    weight = torch.ones(NO_OBJECT + 1, dtype=dtype)
    weight[-1] = eos_coef
    nll = -lg.log_softmax(-1).gather(-1, target[..., None])[..., 0]
    w = weight[target]
    out = {"loss_ce": float((w * nll).sum() / w.sum())}
    src = torch.cat([boxes[b].to(dtype)[torch.as_tensor(i, dtype=torch.int64)] for b, (i, _) in enumerate(indices)])
    tgt = torch.cat([tgt_boxes[b].to(dtype).reshape(-1, 4)[torch.as_tensor(j, dtype=torch.int64)] for b, (_, j) in enumerate(indices)])
    cls = torch.cat([tgt_labels[b].long()[torch.as_tensor(j, dtype=torch.int64)] for b, (_, j) in enumerate(indices)])
    pred = torch.cat([logits[b][torch.as_tensor(i, dtype=torch.int64)][:, :NO_OBJECT].argmax(-1) for b, (i, _) in enumerate(indices)])
    n = len(cls)
    out["class_error"] = 100.0 - 100.0 * float((pred == cls).sum()) / n if n else 100.0
    num_boxes = max(float(sum(len(t) for t in tgt_labels)) / world_size, 1.0)
    out["loss_bbox"] = float((src - tgt).abs().sum() / num_boxes)
    giou = torch.diag(generalized_box_iou(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tgt))) if n else torch.zeros(0, dtype=dtype)
    out["loss_giou"] = float((1 - giou).sum() / num_boxes)
    card = (logits.argmax(-1) != NO_OBJECT).sum(1).to(dtype)
    out["cardinality_error"] = float((card - torch.tensor([float(len(t)) for t in tgt_labels], dtype=dtype)).abs().mean())
    return out


def load_fixture(path):
    """tests/golden/criterion_ref.npz as a dict: inputs as torch tensors, per-image lists split by `sizes`."""
    z = np.load(path)
    sizes = z["sizes"].tolist()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    fx = {"sizes": sizes, "logits": torch.from_numpy(z["logits"]), "boxes": torch.from_numpy(z["boxes"]),
          "tgt_boxes": [torch.from_numpy(z["tgt_boxes"][offs[b]:offs[b + 1]]) for b in range(len(sizes))],
          "tgt_labels": [torch.from_numpy(z["tgt_labels"][offs[b]:offs[b + 1]]) for b in range(len(sizes))],
          "pinned": int(z["pinned"]), "sets": []}
    for s in range(int(z["n_sets"])):
        cost = z[f"cost_{s}"]
        fx["sets"].append({
            "weights": tuple(float(x) for x in z[f"weights_{s}"]), "eos_coef": float(z[f"eos_coef_{s}"]),
            "cost": [cost[NUM_QUERIES * offs[b]:NUM_QUERIES * offs[b + 1]].reshape(NUM_QUERIES, sizes[b]) for b in range(len(sizes))],
            "indices": [(z[f"index_i_{s}"][z[f"index_off_{s}"][b]:z[f"index_off_{s}"][b + 1]],
                         z[f"index_j_{s}"][z[f"index_off_{s}"][b]:z[f"index_off_{s}"][b + 1]]) for b in range(len(sizes))],
            "losses": {k: float(z[f"{k}_{s}"]) for k in ("loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error")}})
    return fx
