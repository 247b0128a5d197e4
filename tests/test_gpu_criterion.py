"""Validation losses on the GPU (-m gpu): wm_criterion (cost matrices, Hungarian match, loss sums) and the Python surface on
top of it (HungarianMatcher, SetCriterion, evaluate) against tests/golden/criterion_ref.npz -- recorded from the
reference's own matcher + scipy and SetCriterion -- and against the float64 restatement in tests/criterion_ref.py.

Each test prints the figures it asserts on (run with -s); the bounds are the ones stated in its docstring.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import criterion_ref as R
import gpu_util as G
from wildlifemapper_amd import _native as N
from wildlifemapper_amd.segment_anything.build_sam import SetCriterion
from wildlifemapper_amd.segment_anything.modeling.matcher import HungarianMatcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_KEYS = ("loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error")
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(os.path.join(ROOT, "tests", "golden", "criterion_ref.npz"))


def _outputs(fx):
    return {"pred_logits": fx["logits"].to(G.dev()), "pred_boxes": fx["boxes"].to(G.dev())}


def _targets(fx):
    return [{"boxes": b.to(G.dev()), "labels": l.to(G.dev()).long()} for b, l in zip(fx["tgt_boxes"], fx["tgt_labels"])]


@pytest.fixture(scope="module")
def runs(fx):
    """Per weight set: one debug call of the kernels on the fixture's inputs, read back once, and the float64 restatement."""
    out = []
    for st in fx["sets"]:
        w = st["weights"]
        r = HungarianMatcher(*w).match(_outputs(fx), _targets(fx), eos_coef=st["eos_coef"], debug=True)
        got = {k: v.cpu().numpy() for k, v in r.items() if torch.is_tensor(v)}
        c64 = [c.numpy() for c in R.cost_matrices(fx["logits"], fx["boxes"], fx["tgt_boxes"], fx["tgt_labels"], w, torch.float64)]
        out.append({"gpu": got, "c64": c64})
    return out


def _split(flat, sizes, per=1):
    offs = np.concatenate([[0], np.cumsum(sizes)]) * per
    return [flat[offs[b]:offs[b + 1]] for b in range(len(sizes))]


def _lists(match_row):
    i = np.nonzero(match_row >= 0)[0]
    return i.astype(np.int64), match_row[i].astype(np.int64)


@pytest.mark.parametrize("s", [0, 1])
def test_cost_matrices_against_fixture(fx, runs, s):
    """err = max |C_gpu - C_f64| per image, C_f64 the restatement in float64 on the same fp32 inputs; bound: 4 x the
    reference's own max |C_ref32 - C_f64| on that image (another operation order and the hardware exp)."""
    assert not runs[s]["gpu"]["status"].any()
    costs = _split(runs[s]["gpu"]["cost"], fx["sizes"], 51)
    for b, n in enumerate(fx["sizes"]):
        if n == 0:
            assert costs[b].size == 0
            continue
        c64 = runs[s]["c64"][b]
        err = float(np.abs(costs[b].reshape(51, n).astype(np.float64) - c64).max())
        ref_err = float(np.abs(fx["sets"][s]["cost"][b].astype(np.float64) - c64).max())
        print(f"[criterion cost] set {s} image {b} T={n}: gpu err {err:.3e}, reference fp32 err {ref_err:.3e}, max|C| {np.abs(c64).max():.2f}")
        assert err <= 4 * ref_err, (b, err, ref_err)


@pytest.mark.parametrize("s", [0, 1])
def test_assignment_equals_scipy(fx, runs, s):
    m = runs[s]["gpu"]["match"]
    assert m.shape == (8, 51) and m.dtype == np.int32
    for b in range(8):
        i, j = _lists(m[b])
        ri, rj = fx["sets"][s]["indices"][b]
        assert np.array_equal(i, ri) and np.array_equal(j, rj), b
    # the matcher's Python return value: the reference's list of (index_i, index_j) int64 tensors
    got = HungarianMatcher(*fx["sets"][s]["weights"])(_outputs(fx), _targets(fx))
    assert len(got) == 8
    for b, (i, j) in enumerate(got):
        ri, rj = fx["sets"][s]["indices"][b]
        assert i.dtype == j.dtype == torch.int64 and i.tolist() == ri.tolist() and j.tolist() == rj.tolist(), b


@pytest.mark.parametrize("s", [0, 1])
def test_assignment_optimal_by_duals(fx, runs, s):
    """Independent of ties and of scipy: dual feasibility u_i + v_j <= C_ij + tol everywhere, |u_i + v_j - C_ij| <= tol on
    matched pairs (with a one-to-one matching of full size that is optimality), tol = 8 * 2^-24 * max |C|."""
    g = runs[s]["gpu"]
    costs, vs = _split(g["cost"], fx["sizes"], 51), _split(g["dual_v"], fx["sizes"])
    for b, n in enumerate(fx["sizes"]):
        i, j = _lists(g["match"][b])
        assert len(i) == min(51, n) and len(set(j.tolist())) == len(j) and (n == 0 or (j.min() >= 0 and j.max() < n))
        if n == 0:
            continue
        c = costs[b].reshape(51, n).astype(np.float64)
        tol = 8 * EPS * np.abs(c).max()
        slack = c - g["dual_u"][b][:, None] - vs[b][None, :]
        print(f"[criterion duals] set {s} image {b} T={n}: min slack {slack.min():.3e}, max |slack| on matched {np.abs(slack[i, j]).max():.3e}, tol {tol:.3e}")
        assert slack.min() >= -tol, b
        assert np.abs(slack[i, j]).max() <= tol, b


def test_ties_all_predictions_and_targets_identical():
    """Every entry of the cost matrix is the same number: any one-to-one matching of full size is optimal."""
    sizes = [5, 51, 60]
    lg = torch.tensor([0.3, -1.0, 2.0, 0.5, 0.0, -0.5, 1.0, 0.2]).repeat(len(sizes), 51, 1)
    bx = torch.tensor([0.4, 0.5, 0.1, 0.2]).repeat(len(sizes), 51, 1)
    tb = [torch.tensor([0.45, 0.55, 0.12, 0.16]).repeat(n, 1) for n in sizes]
    tl = [torch.full((n,), 2, dtype=torch.int64) for n in sizes]
    r = HungarianMatcher(1, 5, 2).match({"pred_logits": lg.to(G.dev()), "pred_boxes": bx.to(G.dev())},
                                        [{"boxes": b.to(G.dev()), "labels": l.to(G.dev())} for b, l in zip(tb, tl)], debug=True)
    assert not r["status"].cpu().any()
    costs = _split(r["cost"].cpu().numpy(), sizes, 51)
    for b, n in enumerate(sizes):
        c = costs[b].reshape(51, n)
        assert (c == c[0, 0]).all()
        i, j = _lists(r["match"][b].cpu().numpy())
        assert len(i) == min(51, n) and len(set(j.tolist())) == len(j) and j.min() >= 0 and j.max() < n
        assert float(c[i, j].astype(np.float64).sum()) == min(51, n) * float(c[0, 0])      # the optimal total


def _loss_bounds(fx, s):
    """Relative bound per loss: (N + 16) * 2^-24, N = the number of summed terms."""
    matched = sum(len(i) for i, _ in fx["sets"][s]["indices"])
    return {"loss_ce": (8 * 51 + 16) * EPS, "loss_bbox": (4 * matched + 16) * EPS, "loss_giou": (matched + 16) * EPS}


@pytest.mark.parametrize("s", [0, 1])
def test_losses_against_float64_restatement(fx, s):
    st = fx["sets"][s]
    crit = SetCriterion(7, HungarianMatcher(*st["weights"]), {"loss_ce": 3, "loss_bbox": 5, "loss_giou": 2}, st["eos_coef"],
                        ["labels", "boxes", "cardinality"])
    got = crit(_outputs(fx), _targets(fx))
    assert set(got) == set(LOSS_KEYS) and all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in got.values())
    crit.check_status()
    ref = R.losses(fx["logits"], fx["boxes"], fx["tgt_boxes"], fx["tgt_labels"], st["indices"], st["eos_coef"], torch.float64)
    for k, bound in _loss_bounds(fx, s).items():
        rel = abs(float(got[k]) - ref[k]) / abs(ref[k])
        print(f"[criterion losses] set {s} {k}: gpu {float(got[k]):.9g}, float64 {ref[k]:.9g}, rel err {rel:.3e}, bound {bound:.3e}")
        assert rel <= bound, k
    assert float(got["class_error"]) == float(np.float32(ref["class_error"]))
    assert float(got["cardinality_error"]) == float(np.float32(ref["cardinality_error"]))
    # and the reference's own fp32 numbers, within its summation error
    for k in LOSS_KEYS:
        assert float(got[k]) == pytest.approx(st["losses"][k], rel=2e-6, abs=1e-6), k


def test_no_targets_at_all():
    """Nothing to match: class_error is 100 (the reference's accuracy returns 0 for an empty target), num_boxes clamps to 1."""
    g = torch.Generator().manual_seed(5)
    lg, bx = torch.randn(2, 51, 8, generator=g), torch.sigmoid(torch.randn(2, 51, 4, generator=g))
    tb, tl = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.int64)] * 2
    crit = SetCriterion(7, HungarianMatcher(1, 5, 2), {"loss_ce": 3}, 0.1, ["labels", "boxes", "cardinality"])
    got = {k: float(v) for k, v in crit({"pred_logits": lg.to(G.dev()), "pred_boxes": bx.to(G.dev())},
                                        [{"boxes": b.to(G.dev()), "labels": l.to(G.dev())} for b, l in zip(tb, tl)]).items()}
    crit.check_status()
    ref = R.losses(lg, bx, tb, tl, [(np.zeros(0, np.int64),) * 2] * 2, 0.1, torch.float64)
    assert got["class_error"] == 100.0 and got["loss_bbox"] == 0.0 and got["loss_giou"] == 0.0
    assert got["cardinality_error"] == float(np.float32(ref["cardinality_error"]))
    assert abs(got["loss_ce"] - ref["loss_ce"]) <= (2 * 51 + 16) * EPS * abs(ref["loss_ce"])


def test_repeat_is_bit_identical(fx):
    st = fx["sets"][0]
    a = HungarianMatcher(*st["weights"]).match(_outputs(fx), _targets(fx), eos_coef=st["eos_coef"], debug=True)
    b = HungarianMatcher(*st["weights"]).match(_outputs(fx), _targets(fx), eos_coef=st["eos_coef"], debug=True)
    for k in ("match", "sums", "status", "cost", "dual_u", "dual_v"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_non_finite_cost_flags_one_image(fx, runs):
    """One target box with a NaN coordinate: that image's status bit is set and its matches are -1, the other images are
    as without it, every sum is NaN and Python raises."""
    st = fx["sets"][0]
    bad = 5
    targets = _targets(fx)
    boxes = targets[bad]["boxes"].clone()
    boxes[7, 2] = float("nan")
    targets[bad] = {"boxes": boxes, "labels": targets[bad]["labels"]}
    matcher = HungarianMatcher(*st["weights"])
    r = matcher.match(_outputs(fx), targets, eos_coef=st["eos_coef"])
    status, m = r["status"].cpu().numpy(), r["match"].cpu().numpy()
    assert status.tolist() == [N.CRITERION_NONFINITE if b == bad else 0 for b in range(8)]
    assert (m[bad] == -1).all()
    clean = runs[0]["gpu"]["match"]
    assert all(np.array_equal(m[b], clean[b]) for b in range(8) if b != bad)
    assert torch.isnan(r["sums"]).all()
    with pytest.raises(RuntimeError, match="image 5: non-finite"):
        matcher(_outputs(fx), targets)
    crit = SetCriterion(7, matcher, {"loss_ce": 3, "loss_bbox": 5, "loss_giou": 2}, st["eos_coef"], ["labels", "boxes", "cardinality"])
    losses = crit(_outputs(fx), targets)
    assert all(torch.isnan(v) for v in losses.values())
    with pytest.raises(RuntimeError, match="image 5: non-finite"):
        crit.check_status()


def test_more_images_than_one_launch_takes(fx):
    """B = 65: the launcher cuts the batch into launches of 64 images; image 64 goes through the second one (image base 64, its
    own offsets).  Same results as each image alone."""
    g = torch.Generator().manual_seed(3)
    B = 65
    sizes = [(b * 7) % 5 for b in range(B)]
    sizes[64] = 3
    lg, bx = torch.randn(B, 51, 8, generator=g), torch.sigmoid(torch.randn(B, 51, 4, generator=g))
    bx[..., 2:] = 0.01 + 0.2 * torch.rand(B, 51, 2, generator=g)
    tb = [torch.cat([torch.sigmoid(torch.randn(n, 2, generator=g)), 0.01 + 0.2 * torch.rand(n, 2, generator=g)], 1) for n in sizes]
    tl = [torch.randint(1, 7, (n,), generator=g) for n in sizes]
    matcher = HungarianMatcher(1, 5, 2)
    r = matcher.match({"pred_logits": lg.to(G.dev()), "pred_boxes": bx.to(G.dev())},
                      [{"boxes": b.to(G.dev()), "labels": l.to(G.dev())} for b, l in zip(tb, tl)], eos_coef=0.1)
    assert not r["status"].cpu().any()
    m = r["match"].cpu().numpy()
    want = R.match(R.cost_matrices(lg, bx, tb, tl, (1.0, 5.0, 2.0), torch.float32))
    for b in range(B):
        i, j = _lists(m[b])
        assert np.array_equal(i, want[b][0]) and np.array_equal(j, want[b][1]), b
    ref = R.losses(lg, bx, tb, tl, want, 0.1, torch.float64)
    sums = r["sums"].cpu().numpy()
    assert sums[4] == sum(sizes) and sums[6] == round(ref["cardinality_error"] * B) and abs(sums[6] / B - ref["cardinality_error"]) < 1e-12
    assert abs(sums[0] / sums[1] - ref["loss_ce"]) <= (B * 51 + 16) * EPS * ref["loss_ce"]
    assert abs(sums[2] / sum(sizes) - ref["loss_bbox"]) <= (4 * sum(sizes) + 16) * EPS * ref["loss_bbox"]


def test_label_7_and_cpu_targets_are_refused():
    """A target's class is 0..6 (7 is no-object): a label of 7 sets the image's status bit like a non-finite cost.  Targets on
    another device than the predictions raise, they are not copied behind the caller's back."""
    lg, bx = torch.zeros(2, 51, 8, device=G.dev()), torch.full((2, 51, 4), 0.5, device=G.dev())
    tb = [torch.full((2, 4), 0.4, device=G.dev())] * 2
    matcher = HungarianMatcher(1, 5, 2)
    r = matcher.match({"pred_logits": lg, "pred_boxes": bx},
                      [{"boxes": tb[0], "labels": torch.tensor([1, 7], device=G.dev())}, {"boxes": tb[1], "labels": torch.tensor([1, 6], device=G.dev())}])
    assert r["status"].cpu().tolist() == [N.CRITERION_NONFINITE, 0] and (r["match"][0] == -1).all() and (r["match"][1] >= 0).sum() == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        matcher.match({"pred_logits": lg, "pred_boxes": bx}, [{"boxes": t.cpu(), "labels": torch.tensor([1, 2])} for t in tb])


def test_target_limit_is_an_error():
    lg, bx = torch.zeros(1, 51, 8, device=G.dev()), torch.full((1, 51, 4), 0.5, device=G.dev())
    n = N.CRITERION_MAX_TARGETS + 1
    with pytest.raises(RuntimeError, match="limit is 2048"):
        HungarianMatcher(1, 5, 2).match({"pred_logits": lg, "pred_boxes": bx},
                                        [{"boxes": torch.full((n, 4), 0.5, device=G.dev()), "labels": torch.ones(n, dtype=torch.int64, device=G.dev())}])


def test_evaluate_returns_the_reference_loss_stats():
    """evaluate on ViT-B, two synthetic tiles in two batches, targets attached, the criterion of _build_sam(args=...): the
    reference's keys, values equal to the restatement applied to the model's own read-back logits and boxes, `loss` the
    weighted sum, and COCO stats equal to a run with the stub."""
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.inference import evaluate
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.build_sam import InferenceCriterion
    from wildlifemapper_amd.segment_anything.utils.misc import nested_tensor_from_tensor_list
    from gpu_util import _model                              # the suite's one resident ViT-B (synthetic weights)
    args = SimpleNamespace(set_cost_class=1.0, set_cost_bbox=5.0, set_cost_giou=2.0, bbox_loss_coef=5.0, giou_loss_coef=2.0, eos_coef=0.1,
                           batch_size=1)
    _, crit, _ = sam_model_registry["vit_b"](None, args)
    assert isinstance(crit, SetCriterion)
    m, post = _model("vit_b", "fp16")
    seen = []

    class Recording(torch.nn.Module):
        def forward(self, image, boxes):
            out = m(image, boxes)
            seen.append({k: v.cpu() for k, v in out.items()})
            return out

    x = torch.from_numpy(synth.make_batch(0, 2))
    g = torch.Generator().manual_seed(11)
    sizes = [4, 60]
    loader, anns, tgt_cpu = [], [], []
    for i, n in enumerate(sizes):
        b = torch.sigmoid(torch.randn(n, 4, generator=g))
        b[:, 2:] = 0.01 + 0.2 * torch.rand(n, 2, generator=g)
        l = torch.randint(1, 7, (n,), generator=g)
        tgt_cpu.append((b, l))
        loader.append((nested_tensor_from_tensor_list([x[i]]), [{"image_id": torch.tensor([100 + i]), "orig_size": torch.tensor([1024, 1024]),
                                                                  "boxes": b, "labels": l}]))
        for bb, ll in zip(b.numpy() * 1024, l.numpy()):
            anns.append({"id": len(anns) + 1, "image_id": 100 + i, "category_id": int(ll), "iscrowd": 0, "area": float(bb[2] * bb[3]),
                         "bbox": [float(bb[0] - bb[2] / 2), float(bb[1] - bb[3] / 2), float(bb[2]), float(bb[3])]})
    base_ds = {"images": [{"id": 100}, {"id": 101}], "categories": [{"id": c} for c in range(7)], "annotations": anns}
    stats, _ = evaluate(Recording(), crit, {"bbox": post}, loader, base_ds, G.dev(), args)
    stub, _ = evaluate(m, InferenceCriterion(), {"bbox": post}, loader, base_ds, G.dev(), args)
    keys = {"loss", "loss_ce", "loss_bbox", "loss_giou", "class_error"} | {k + "_unscaled" for k in LOSS_KEYS}
    assert keys <= set(stats) and not (keys & set(stub))
    assert {k: v for k, v in stats.items() if k not in keys} == stub                           # COCO stats, images, detections
    assert len(seen) == 2
    want = {k: 0.0 for k in LOSS_KEYS}
    for out, (b, l) in zip(seen, tgt_cpu):
        idx = R.match(R.cost_matrices(out["pred_logits"], out["pred_boxes"], [b], [l], (1.0, 5.0, 2.0), torch.float32))
        one = R.losses(out["pred_logits"], out["pred_boxes"], [b], [l], idx, 0.1, torch.float64)
        for k in LOSS_KEYS:
            want[k] += one[k] / 2                                                               # MetricLogger.global_avg over the batches
    # bound: the loss test's (N + 16) * 2^-24 with N = 4 * 51, the most terms any sum of a one-image batch has, + the fp32 result
    rel = (4 * 51 + 16 + 1) * EPS
    for k in LOSS_KEYS:
        print(f"[criterion evaluate] {k}_unscaled: {stats[k + '_unscaled']:.9g}, restatement {want[k]:.9g}")
        assert stats[k + "_unscaled"] == pytest.approx(want[k], rel=rel, abs=1e-12), k
    assert stats["class_error"] == stats["class_error_unscaled"]
    assert stats["loss_ce"] == pytest.approx(3 * stats["loss_ce_unscaled"], rel=1e-12)
    assert stats["loss"] == pytest.approx(3 * stats["loss_ce_unscaled"] + 5.0 * stats["loss_bbox_unscaled"] + 2.0 * stats["loss_giou_unscaled"], rel=1e-12)
