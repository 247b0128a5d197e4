"""Validation losses, the parts that need no GPU: the tests' restatement (tests/criterion_ref.py) against the fixture
recorded from the reference's own matcher + scipy and SetCriterion (tools/gen_criterion_golden.py), the factory's choice
between SetCriterion and the stub, the no-CPU-fallback rule, the C-ABI's argument checks and reduce_dict over 2 gloo ranks."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import criterion_ref as R
from survey_util import _free_port
from wildlifemapper_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "criterion_ref.npz")
ARGS = dict(set_cost_class=1.0, set_cost_bbox=5.0, set_cost_giou=2.0, bbox_loss_coef=5.0, giou_loss_coef=2.0, eos_coef=0.1)


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(FIXTURE)


def test_fixture_shape(fx):
    assert fx["pinned"] == 1 and fx["sizes"] == [0, 1, 3, 50, 51, 52, 80, 300] and len(fx["sets"]) == 2
    assert fx["sets"][0]["weights"] == (1.0, 5.0, 2.0) and fx["sets"][0]["eos_coef"] == 0.1
    for s in fx["sets"]:
        for (i, j), n in zip(s["indices"], fx["sizes"]):
            assert len(i) == len(j) == min(51, n) and np.all(np.diff(i) > 0) and len(set(j.tolist())) == len(j)


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_equals_reference(fx, s):
    """Index lists identical to scipy's; fp32 costs and the five losses to fp32 round-off."""
    st = fx["sets"][s]
    c32 = R.cost_matrices(fx["logits"], fx["boxes"], fx["tgt_boxes"], fx["tgt_labels"], st["weights"], torch.float32)
    c64 = R.cost_matrices(fx["logits"], fx["boxes"], fx["tgt_boxes"], fx["tgt_labels"], st["weights"], torch.float64)
    for b, (c, ref) in enumerate(zip(c32, st["cost"])):
        assert tuple(c.shape) == ref.shape
        if ref.size:
            # both are fp32 evaluations of the same formula.  Sum and L1 / class terms: a few ulp(|C| <= 16) = 2^-20.  GIoU: its
            # widths (>= 0.01 here) are differences of coordinates near 1, so each carries up to 2^-24 / 0.01 ~ 2^-17.4 relative
            # error, and an area two of them: 2^-17 on a value of at most 1, times cost_giou
            tol = 4 * 2.0 ** -20 + st["weights"][2] * 2.0 ** -17
            assert np.abs(ref - c64[b].numpy()).max() <= tol, b
            assert np.abs(c.numpy() - ref).max() <= 2 * tol, b
    for costs in (st["cost"], [c.numpy() for c in c32]):
        for b, c in enumerate(costs):
            i, j, u, v = R.solve(c)
            assert np.array_equal(i, st["indices"][b][0]) and np.array_equal(j, st["indices"][b][1]), b
            if c.size:
                slack = c.astype(np.float64) - u[:, None] - v[None, :]
                assert slack.min() >= -1e-12 and np.abs(slack[i, j]).max() <= 1e-12
    got = R.losses(fx["logits"], fx["boxes"], fx["tgt_boxes"], fx["tgt_labels"], st["indices"], st["eos_coef"], torch.float64)
    for k, ref in st["losses"].items():
        assert got[k] == pytest.approx(ref, rel=2e-6, abs=1e-6), k           # the reference's sums are fp32
    assert got["class_error"] == pytest.approx(st["losses"]["class_error"], abs=1e-4)
    assert got["cardinality_error"] == st["losses"]["cardinality_error"]


def test_solver_ties_and_empty():
    i, j, u, v = R.solve(np.zeros((51, 0)))
    assert len(i) == len(j) == 0
    c = np.full((51, 7), 0.25)
    i, j, _, _ = R.solve(c)
    assert len(i) == 7 and sorted(j.tolist()) == list(range(7)) and np.all(np.diff(i) > 0)
    with pytest.raises(ValueError):
        R.solve(np.array([[1.0, np.nan], [0.0, 1.0]]))


def test_build_sam_returns_set_criterion_with_args_and_stub_without():
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.build_sam import InferenceCriterion, SetCriterion
    from wildlifemapper_amd.segment_anything.modeling.matcher import HungarianMatcher, build_matcher
    _, crit, post = sam_model_registry["vit_b"](None, SimpleNamespace(**ARGS))
    assert isinstance(crit, SetCriterion) and isinstance(crit.matcher, HungarianMatcher) and set(post) == {"bbox"}
    assert crit.weight_dict == {"loss_ce": 3, "loss_bbox": 5.0, "loss_giou": 2.0}                # build_sam.py:326-327
    assert crit.losses == ["labels", "boxes", "cardinality"] and crit.num_classes == 7 and crit.eos_coef == 0.1
    assert (crit.matcher.cost_class, crit.matcher.cost_bbox, crit.matcher.cost_giou) == (1.0, 5.0, 2.0)
    assert torch.equal(crit.empty_weight, torch.tensor([1, 1, 1, 1, 1, 1, 1, 0.1]))
    for args in (None, SimpleNamespace(wm_precision=None), SimpleNamespace(**{k: v for k, v in ARGS.items() if k != "eos_coef"})):
        _, stub, _ = sam_model_registry["vit_b"](None, args)
        assert isinstance(stub, InferenceCriterion) and stub(None, None) == {} and stub.weight_dict == {}
    with pytest.raises(AssertionError, match="all costs cant be 0"):
        HungarianMatcher(0, 0, 0)
    m = build_matcher(SimpleNamespace(**ARGS))
    assert (m.cost_class, m.cost_bbox, m.cost_giou) == (1.0, 5.0, 2.0)


def test_cpu_tensor_raises():
    from wildlifemapper_amd.segment_anything import sam_model_registry
    _, crit, _ = sam_model_registry["vit_b"](None, SimpleNamespace(**ARGS))
    outputs = {"pred_logits": torch.zeros(1, 51, 8), "pred_boxes": torch.full((1, 51, 4), 0.5)}
    targets = [{"boxes": torch.full((2, 4), 0.5), "labels": torch.ones(2, dtype=torch.int64)}]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(outputs, targets)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit.matcher(outputs, targets)


def test_criterion_argument_errors_without_gpu():
    lib = N.lib()
    assert lib.wm_criterion_scratch_bytes(0, 10) < 0 and b"batch 0" in lib.wm_last_error()
    assert lib.wm_criterion_scratch_bytes(2, -1) < 0
    assert lib.wm_criterion_scratch_bytes(2, 1 << 30) < 0
    assert lib.wm_criterion_scratch_bytes(2, 0) == 2 * N.CRITERION_SUMS * 8
    assert lib.wm_criterion_scratch_bytes(8, 537) == (51 * 537 * 4 + 15) // 16 * 16 + 8 * N.CRITERION_SUMS * 8
    p = C.c_void_p(4096)                                     # never dereferenced: every call below fails its checks first

    def call(offs, batch, scratch_bytes=1 << 20, logits=p, eos=0.1, scratch=p):
        arr = (C.c_int32 * len(offs))(*offs)
        return lib.wm_criterion(None, logits, p, p, p, arr, batch, 1.0, 5.0, 2.0, eos, scratch, scratch_bytes, p, p, p, None, None, None, None)

    assert call([0, 1], 1, logits=None) != 0 and b"null buffer" in lib.wm_last_error()
    assert call([0, 1], 0) != 0 and b"batch 0" in lib.wm_last_error()
    assert call([1, 2], 1) != 0 and b"tgt_offsets[0]" in lib.wm_last_error()
    assert call([0, 3, 2], 2) != 0 and b"decreasing" in lib.wm_last_error()
    assert call([0, N.CRITERION_MAX_TARGETS + 1], 1, scratch_bytes=1 << 30) != 0 and b"limit is 2048" in lib.wm_last_error()
    assert call([0, 4], 1, eos=float("nan")) != 0 and b"finite" in lib.wm_last_error()
    assert call([0, 4], 1, scratch_bytes=64) != 0 and b"scratch of 64 bytes" in lib.wm_last_error()
    assert call([0, 4], 1, scratch=C.c_void_p(4100)) != 0 and b"16-byte aligned" in lib.wm_last_error()


# ---------------------------------------------------------------------------
# reduce_dict over 2 gloo ranks (utils/misc.py:154-178)
# ---------------------------------------------------------------------------


def _reduce_worker(rank, world, port, q):
    from wildlifemapper_amd.segment_anything.utils import misc as utils
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = {"loss_giou": torch.tensor(1.0 + rank), "class_error": torch.tensor(100.0 * rank), "loss_ce": torch.tensor(0.5)}
    mean = utils.reduce_dict(dict(reversed(list(d.items()))) if rank else d)        # key order differs between ranks
    total = utils.reduce_dict(d, average=False)
    q.put((rank, {k: float(v) for k, v in mean.items()}, {k: float(v) for k, v in total.items()}, float(d["loss_giou"])))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_dict_gloo_world_2():
    from wildlifemapper_amd.segment_anything.utils import misc as utils
    d = {"a": torch.tensor(2.0)}
    assert utils.reduce_dict(d) is d                                                # world 1: the input itself, as the reference
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, mean, total, own in got:
        assert mean == {"class_error": 50.0, "loss_ce": 0.5, "loss_giou": 1.5}
        assert total == {"class_error": 100.0, "loss_ce": 1.0, "loss_giou": 3.0}
        assert own == 1.0 + rank                                                    # the input is not modified
