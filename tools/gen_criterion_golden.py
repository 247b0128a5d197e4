"""Golden vectors of the validation losses (tests/test_criterion_cpu.py, tests/test_gpu_criterion.py): seeded model outputs
and targets, and what the reference's own HungarianMatcher (with scipy's linear_sum_assignment) and SetCriterion make of
them.

  python tools/gen_criterion_golden.py --reference /path/to/reference/wildlifemapper [--out tests/golden]

The reference's definitions are taken from its source files by name and executed as they stand: HungarianMatcher
(segment_anything/modeling/matcher.py), SetCriterion (segment_anything/build_sam.py), box_cxcywh_to_xyxy, box_iou,
generalized_box_iou (segment_anything/utils/box_ops.py) and accuracy (segment_anything/utils/misc.py).  Supplied here:
torchvision's one-line box_area (torchvision is absent, so that one line is unpinned) and the two single-process dist
helpers.  Nothing is stored but arrays.

One call of B = 8 with 0, 1, 3, 50, 51, 52, 80 and 300 targets per image: the empty case, both sides of the transposition
at 51, the square case and more than one column per lane; two sets of matcher weights.  Every assignment must be unique
with margin: re-solved 50 times with uniform noise of +-1e-4 on the cost matrix it has to give the same index lists,
otherwise the next seed is tried.  The file also records the fp32 cost matrices the reference computed.
"""
import argparse
import ast
import os
import types

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment
from torch import nn

SIZES = [0, 1, 3, 50, 51, 52, 80, 300]
SETS = [((1.0, 5.0, 2.0), 0.1), ((2.0, 1.0, 5.0), 0.25)]        # (cost_class, cost_bbox, cost_giou), eos_coef
NUM_QUERIES, NUM_CLASSES = 51, 7


SOLVED = []          # the cost matrices of the last matcher call, as scipy received them


def solve_and_record(c):
    SOLVED.append(torch.as_tensor(c).clone())
    return linear_sum_assignment(c)


def node_src(path, kind, name):
    with open(path) as f:
        src = f.read()
    for n in ast.parse(src).body:
        if isinstance(n, kind) and n.name == name:
            return ast.get_source_segment(src, n)
    raise KeyError(name)


def reference_classes(ref):
    sa = os.path.join(ref, "segment_anything")
    box = {"torch": torch, "box_area": lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])}      # torchvision.ops.boxes.box_area
    for name in ("box_cxcywh_to_xyxy", "box_iou", "generalized_box_iou"):
        exec(compile(node_src(os.path.join(sa, "utils", "box_ops.py"), ast.FunctionDef, name), "box_ops.py", "exec"), box)
    misc = {"torch": torch}
    exec(compile(node_src(os.path.join(sa, "utils", "misc.py"), ast.FunctionDef, "accuracy"), "misc.py", "exec"), misc)
    m = {"torch": torch, "nn": nn, "linear_sum_assignment": solve_and_record, "box_cxcywh_to_xyxy": box["box_cxcywh_to_xyxy"],
         "generalized_box_iou": box["generalized_box_iou"]}
    exec(compile(node_src(os.path.join(sa, "modeling", "matcher.py"), ast.ClassDef, "HungarianMatcher"), "matcher.py", "exec"), m)
    c = {"torch": torch, "nn": nn, "F": F, "accuracy": misc["accuracy"], "is_dist_avail_and_initialized": lambda: False,
         "get_world_size": lambda: 1,
         "box_ops": types.SimpleNamespace(generalized_box_iou=box["generalized_box_iou"], box_cxcywh_to_xyxy=box["box_cxcywh_to_xyxy"])}
    exec(compile(node_src(os.path.join(sa, "build_sam.py"), ast.ClassDef, "SetCriterion"), "build_sam.py", "exec"), c)
    return m["HungarianMatcher"], c["SetCriterion"]


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(len(SIZES), NUM_QUERIES, NUM_CLASSES + 1, generator=g) * 2

    def boxes(n):
        b = torch.sigmoid(torch.randn(n, 4, generator=g))
        b[:, 2:] = 0.01 + 0.2 * torch.rand(n, 2, generator=g)
        return b

    pred = boxes(len(SIZES) * NUM_QUERIES).view(len(SIZES), NUM_QUERIES, 4)
    targets = [{"boxes": boxes(n), "labels": torch.randint(1, 7, (n,), generator=g)} for n in SIZES]
    return logits, pred, targets


def cost_matrices(matcher, outputs, targets):
    """The fp32 matrices HungarianMatcher.forward hands to scipy, and the index lists it returns."""
    del SOLVED[:]
    indices = matcher(outputs, targets)
    return list(SOLVED), indices


def unique_with_margin(costs, indices, rng):
    for c, (i, j) in zip(costs, indices):
        c = c.double().numpy()
        if c.shape[1] == 0:
            continue
        for _ in range(50):
            ri, rj = linear_sum_assignment(c + rng.uniform(-1e-4, 1e-4, c.shape))
            if not (np.array_equal(ri, i.numpy()) and np.array_equal(rj, j.numpy())):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's wildlifemapper/ folder")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    Matcher, Criterion = reference_classes(a.reference)
    rng = np.random.default_rng(0)
    for seed in range(100):
        logits, pred, targets = make_inputs(seed)
        outputs = {"pred_logits": logits, "pred_boxes": pred}
        fx = {"sizes": np.array(SIZES, np.int32), "logits": logits.numpy(), "boxes": pred.numpy(),
              "tgt_boxes": torch.cat([t["boxes"] for t in targets]).numpy(),
              "tgt_labels": torch.cat([t["labels"] for t in targets]).numpy().astype(np.int32),
              "n_sets": np.int32(len(SETS)), "seed": np.int32(seed), "pinned": np.int32(1)}
        ok = True
        for s, (w, eos) in enumerate(SETS):
            matcher = Matcher(cost_class=w[0], cost_bbox=w[1], cost_giou=w[2])
            costs, indices = cost_matrices(matcher, outputs, targets)
            assert len(costs) == len(SIZES) and all(c.dtype == torch.float32 and c.shape == (NUM_QUERIES, n) for c, n in zip(costs, SIZES))
            if not unique_with_margin(costs, indices, rng):
                ok = False
                break
            crit = Criterion(NUM_CLASSES, matcher=matcher, weight_dict={"loss_ce": 3, "loss_bbox": 5, "loss_giou": 2}, eos_coef=eos,
                             losses=["labels", "boxes", "cardinality"])
            loss = crit(outputs, targets)
            fx[f"weights_{s}"] = np.array(w, np.float64)
            fx[f"eos_coef_{s}"] = np.float64(eos)
            fx[f"cost_{s}"] = np.concatenate([c.numpy().reshape(-1) for c in costs])
            fx[f"index_i_{s}"] = np.concatenate([i.numpy() for i, _ in indices])
            fx[f"index_j_{s}"] = np.concatenate([j.numpy() for _, j in indices])
            fx[f"index_off_{s}"] = np.concatenate([[0], np.cumsum([len(i) for i, _ in indices])]).astype(np.int64)
            for k in ("loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error"):
                fx[f"{k}_{s}"] = np.float64(float(loss[k]))
        if ok:
            break
        print("seed", seed, "has an assignment without margin, trying the next")
    else:
        raise SystemExit("no seed gave unique assignments")
    path = os.path.join(a.out, "criterion_ref.npz")
    np.savez_compressed(path, **fx)
    import scipy
    print("wrote", path, os.path.getsize(path) // 1024, "KiB (seed", seed, ", scipy", scipy.__version__, ", torch", torch.__version__ + ")")


if __name__ == "__main__":
    main()
