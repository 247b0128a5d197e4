#!/usr/bin/env python3
"""Dev tool: what the validation losses add to an `evaluate` step.  HIP events around N calls of SetCriterion.forward
(pack the targets, wm_criterion, the 0-d loss tensors; nothing read back) at B images with T targets each, beside the same
work done the reference's way on this host (device-to-host copy of logits and boxes, then tests/criterion_ref.py on the
CPU: cost matrices, assignment, losses), and the step they are added to: model forward + PostProcess at the same B -- the
step as it was before the criterion existed, measured in the same run.

  python tools/criterion_time.py [--model vit_h] [--batch 16] [--targets 51 300] [--out profiles/criterion]
"""
import argparse
import functools
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import criterion_ref as CR
import survey_bench_util
from wildlifemapper_amd import synth
from wildlifemapper_amd.segment_anything import sam_model_registry
from wildlifemapper_amd.segment_anything.build_sam import SetCriterion
from wildlifemapper_amd.engine import criterion_native
from wildlifemapper_amd.segment_anything.modeling.matcher import HungarianMatcher, pack_targets
from wildlifemapper_amd.segment_anything.network import MedSAM
from wildlifemapper_amd.segment_anything.utils.misc import NestedTensor

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="vit_h")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--targets", type=int, nargs="+", default=[51, 300])
ap.add_argument("--out", default=os.path.join(R, "profiles", "criterion"))
a = ap.parse_args()
dev = torch.device("cuda:0")
B = a.batch
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)

timed = functools.partial(survey_bench_util.timed, warmup=5, together=True)       # the mean of n calls timed together

sam, _, post = sam_model_registry[a.model](None, None)
m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(a.model).items()}, strict=True)
x = NestedTensor(torch.from_numpy(synth.make_batch(0, B)).to(dev), None)
sizes = torch.tensor([[1024, 1024]] * B, device=dev)
with torch.no_grad():
    out = m(x, None)

    def step():
        post["bbox"](m(x, None), sizes)

    step_ms = timed(step, 10)
say(f"evaluate step without the criterion ({a.model}, B = {B}: model forward + PostProcess): {step_ms:.2f} ms")

crit = SetCriterion(7, HungarianMatcher(1.0, 5.0, 2.0), {"loss_ce": 3, "loss_bbox": 5.0, "loss_giou": 2.0}, 0.1, ["labels", "boxes", "cardinality"])
g = torch.Generator().manual_seed(0)
for T in a.targets:
    tb = torch.sigmoid(torch.randn(B, T, 4, generator=g))
    tb[..., 2:] = 0.01 + 0.2 * torch.rand(B, T, 2, generator=g)
    tl = torch.randint(1, 7, (B, T), generator=g)
    targets = [{"boxes": tb[b].to(dev), "labels": tl[b].to(dev)} for b in range(B)]
    gpu_ms = timed(lambda: crit(out, targets), 50)
    crit.check_status()
    r = crit.matcher.match(out, targets, eos_coef=0.1)
    kernels_ms = timed(lambda: crit.matcher.match(out, targets, eos_coef=0.1), 50)
    # the device's share alone: the packed targets handed straight to wm_criterion (back-to-back calls, host cost ~ one ctypes call)
    pb, pl, ps = pack_targets(targets, dev)
    native_ms = timed(lambda: criterion_native(out["pred_logits"], out["pred_boxes"], pb, pl, ps, 1.0, 5.0, 2.0, 0.1), 50)
    # and the quantity the condition is about: the step with the criterion in it, as evaluate runs it
    with torch.no_grad():
        def step_with():
            o = m(x, None)
            crit(o, targets)
            post["bbox"](o, sizes)
        with_ms = timed(step_with, 10)
        again_ms = timed(step, 10)
    t0 = time.perf_counter()
    n_host = 3
    for _ in range(n_host):
        lg, bx = out["pred_logits"].cpu(), out["pred_boxes"].cpu()
        idx = CR.match(CR.cost_matrices(lg, bx, list(tb), list(tl), (1.0, 5.0, 2.0), torch.float32))
        CR.losses(lg, bx, list(tb), list(tl), idx, 0.1, torch.float32)
    host_ms = (time.perf_counter() - t0) / n_host * 1e3
    same = all(np.array_equal(np.nonzero(mr >= 0)[0], i) and np.array_equal(mr[mr >= 0], j) for mr, (i, j) in zip(r["match"].cpu().numpy(), idx))
    say(f"B = {B}, T = {T} per image: SetCriterion.forward {gpu_ms * 1e3:.0f} us per call ({kernels_ms * 1e3:.0f} us of it the match call: target packing + "
        f"kernels) = {100 * gpu_ms / step_ms:.2f} % of the step; the reference's way on this host (copy to host + numpy / torch-CPU restatement) "
        f"{host_ms:.1f} ms; same assignment: {same}")
    say(f"    wm_criterion alone (targets already packed, back-to-back): {native_ms * 1e3:.0f} us per call; step with the criterion {with_ms:.2f} ms, "
        f"without (measured again right after) {again_ms:.2f} ms: + {100 * (with_ms - again_ms) / again_ms:.2f} %")
os.makedirs(a.out, exist_ok=True)
with open(os.path.join(a.out, f"criterion_time_{a.model}_b{B}.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
