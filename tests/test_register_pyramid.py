"""Survey registration, pyramid: wm_register_reduce_u8 / tiling.reduce_planes against the restated rule (pyramid_cases.py:
reduce_oracle), and tiling.refine(levels=L) / tiling.register(levels=L) against the same loop with the oracles' planes and
sums.  Everything on the device is integer, so every device comparison is equality."""
import os
import re

import numpy as np
import pytest
import torch

from ground_cases import _p, entry_is_whole, header, last_error, macro
from pyramid_cases import REDUCE_SHAPES, coarse_tables, device_reduce, masked_planes, oracle_loop, point_sampled_loop, reduce_oracle
from register_cases import CELL, FAR, SIDE, SIZES, _corner_error, _oracle, _pairs, _planes, _render, _several_pairs, analytic_scene
from survey_util import DEV, ROOT, _Lazy, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

MAX_EXT = N.REGISTER_MAX_SIDE + 2 * N.REGISTER_MAX_SEARCH


# ---- CPU: the rule -----------------------------------------------------------------------------------------------------

def _one(block, level):
    return int(reduce_oracle(np.array(block, dtype=np.uint8), level)[0, 0])


def test_oracle_hand_cases():
    assert _one([[1, 1], [1, 1]], 1) == 1 and _one([[255, 255], [255, 255]], 1) == 255 and _one([[1, 2], [3, 4]], 1) == 3
    for k in range(4):
        cells = [1, 2, 3, 4]
        cells[k] = 0
        assert _one([cells[:2], cells[2:]], 1) == 0                                 # any one zero
    # the recursion rounds at every level: the 2 x 2 blocks [1,1,2,2] x 3 and [1,1,1,2] give 2, 2, 2, 1 -> (7 + 2) >> 2 = 2,
    # where the block's mean 23 / 16 rounds to 1
    block = np.array([[1, 1, 1, 1], [2, 2, 2, 2], [1, 1, 1, 1], [2, 2, 1, 2]])
    assert reduce_oracle(block, 1).tolist() == [[2, 2], [2, 1]] and _one(block, 2) == 2 and (int(block.sum()) + 8) >> 4 == 1
    plane = np.full((64, 64), 200, dtype=np.uint8)
    assert _one(plane, 6) == 200
    for j, i in ((0, 0), (63, 63), (17, 40), (32, 31)):
        holed = plane.copy()
        holed[j, i] = 0
        assert _one(holed, 6) == 0 and (reduce_oracle(holed, 5) == 0).sum() == 1     # seen iff all 4^level cells under it are
    assert reduce_oracle(np.zeros((3, 8, 8), dtype=np.uint8), 2).shape == (3, 2, 2) and reduce_oracle(plane, 0) is not plane
    np.testing.assert_array_equal(reduce_oracle(plane, 0), plane)


@pytest.mark.parametrize("ext,level", REDUCE_SHAPES)
@pytest.mark.parametrize("n_planes", (1, 3))
def test_oracle_cases_hold_both_kinds_of_cell(ext, level, n_planes):
    """What the device tests rely on: the expected output of every case holds seen and unseen cells, so a kernel that writes
    zeros or ignores the mask cannot pass.  One plane of one output cell cannot hold both: there the device test also runs the
    plane without its mask, and the two expected cells are 0 and not 0."""
    want = reduce_oracle(masked_planes(ext, level, n_planes), level)
    if want.size == 1:
        assert want.item() == 0 and reduce_oracle(masked_planes(ext, level, n_planes, masked=False), level).item() != 0
    else:
        assert (want == 0).any() and (want != 0).any()


# ---- CPU: the far-off scene, on the oracles ------------------------------------------------------------------------------

def test_far_scene_is_what_the_issue_describes():
    frames, true, pert = analytic_scene("far")
    lo, hi = min(int(f.min()) for f in frames), max(int(f.max()) for f in frames)
    first = _corner_error(pert, true)
    print("grey levels", lo, hi, "initial worst corner error", first)
    assert 2 <= lo and hi <= 254 and 9.0 < first < 10.3 and (pert[0] == true[0]).all()          # measured: 9.63 m
    table = tiling.register_pairs(pert, SIZES, CELL, 1, SIDE, 4096)
    assert len(table) == 6 and (table["gx"] == SIDE).all() and (table["gy"] == SIDE).all()


def test_pyramid_loop_on_the_oracle_converges_from_far_off():
    """levels = 3, iters = 3: measured here 2.40, 0.57, 0.21 | 0.075, 0.087, 0.079 | 0.027, 0.045, 0.028 | 0.0137, 0.0105, 0.0106 m."""
    frames, true, pert = analytic_scene("far")
    loop = oracle_loop("far", 3, 3, False)
    print("pyramid, worst corner error per iteration:", loop["errors"], "levels", loop["levels"])
    assert loop["levels"] == [3] * 3 + [2] * 3 + [1] * 3 + [0] * 3
    assert loop["errors"][-1] <= 0.25 * CELL                                       # the bound the refinement already meets
    assert all(s["accepted"].all() for s in loop["steps"])                          # every pair at every level
    assert (loop["georef"][0] == true[0]).all()                                     # the fixed frame has not moved, to the bit


def test_plain_loop_on_the_oracle_walks_away():
    """levels = 0, nine iterations from the same start: measured here 9.78, 9.93, ... 11.05 m.  The point-sampled coarse cells
    are records: 8 m ends at 5.45 m, 4 m at 4.16 m."""
    loop = oracle_loop("far", 0, 9, False)
    print("plain loop:", loop["errors"])
    assert loop["levels"] == [0] * 9 and loop["errors"][-1] > CELL
    print("point-sampled cell 8 m, side 16:", point_sampled_loop(8.0, 5), "cell 4 m, side 32:", point_sampled_loop(4.0, 5))


def _small_loop():
    """The scene's six pairs and a seventh of 7 x 128 cells, which has no cell at level 3: levels = 3, one iteration each."""
    frames, true, pert = analytic_scene("far")
    table = tiling.register_pairs(pert, SIZES, CELL, 1, SIDE, 4096)
    small = np.concatenate([table, _pairs([(0, 1, 7, 128, float(table["x0"][0]), float(table["y0"][0]))])])
    return small, oracle_loop("far", 3, 1, False, table=small)


def test_a_pair_too_small_for_a_level_takes_no_part():
    small, loop = _small_loop()
    dev_t, host_t = coarse_tables(small, 3)
    assert dev_t["gx"][-1] == 0 and dev_t["gy"][-1] == 0 and host_t["gx"][-1] == 1 and (dev_t["gx"][:-1] == 16).all()
    first = loop["steps"][0]
    assert not first["accepted"][-1] and first["cells"][-1] == 0 and first["accepted"][:-1].all()
    assert loop["steps"][-1]["cells"][-1] > 0                                       # and it counts again at level 0


# ---- CPU: argument errors, header, binding ---------------------------------------------------------------------------------

def test_python_argument_errors_before_device_work():
    g = np.stack([tiling.nadir_affine(80, 100, (50.0, 40.0), 1.0, 0.0), tiling.nadir_affine(80, 100, (60.0, 50.0), 1.0, 0.0)])
    sizes = [(80, 100), (80, 100)]
    lazy = _Lazy([np.zeros((80, 100, 3), dtype=np.uint8)] * 2)
    for bad in (-1, 7, 1.0, 2.5, True, "2", None):
        with pytest.raises(ValueError, match="levels"):
            tiling.refine(lazy, g, 1.0, sizes=sizes, side=64, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            tiling.register(lazy, g, 1.0, sizes=sizes, side=64, refine=1, levels=bad)
    for side, levels in ((66, 2), (100, 3), (96, 6), (1, 1)):
        with pytest.raises(ValueError, match="levels"):
            tiling.refine(lazy, g, 1.0, sizes=sizes, side=side, levels=levels)
        with pytest.raises(ValueError, match="levels"):
            tiling.register(lazy, g, 1.0, sizes=sizes, side=side, refine=2, levels=levels)
    with pytest.raises(ValueError, match="levels 2 without refine"):
        tiling.register(lazy, g, 1.0, sizes=sizes, side=64, levels=2, refine=0)
    with pytest.raises(ValueError, match="levels 2 without refine"):
        tiling.register(lazy, g, 1.0, sizes=sizes, side=64, levels=2)
    with pytest.raises(ValueError, match="pair_chunk"):                                # the old checks still come first or after, all before work
        tiling.refine(lazy, g, 1.0, sizes=sizes, side=64, levels=2, pair_chunk=0)
    host = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):                      # no CPU fallback
        tiling.reduce_planes(host, 1)
    for bad in (torch.zeros((2, 8, 6), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.int8),
                torch.zeros((2, 8, 8), dtype=torch.float32), np.zeros((2, 8, 8), dtype=np.uint8), None):
        with pytest.raises(ValueError, match="planes"):
            tiling.reduce_planes(bad, 1)
    for ext, level in ((6, 2), (8, 4), (36, 3), (MAX_EXT + 64, 6)):
        with pytest.raises(ValueError, match="ext"):
            tiling.reduce_planes(torch.zeros((1, ext, ext), dtype=torch.uint8), level)
    for bad in (0, 7, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="level"):
            tiling.reduce_planes(host, bad)
    with pytest.raises(ValueError, match="contiguous"):
        tiling.reduce_planes(torch.zeros((2, 8, 16), dtype=torch.uint8)[:, :, ::2], 1)
    assert lazy.asked == []                                                          # nothing was loaded on the way to an error
    # no pair at all needs no device, with levels too
    far = np.stack([g[0], tiling.nadir_affine(80, 100, (5000.0, 40.0), 1.0, 0.0)])
    out = tiling.refine(lazy, far, 1.0, sizes=sizes, side=64, levels=3)
    assert out["pairs"].shape == (0,) and np.array_equal(out["georef"], far) and out["history"] == [] and lazy.asked == []


def _abi_reduce(n_planes=3, ext=64, level=2, src=0x10000, out=0x80000):
    """wm_register_reduce_u8 with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_register_reduce_u8(_p(src), n_planes, ext, level, _p(out), None)


def test_reduce_abi_argument_errors_without_gpu():
    err = last_error
    for bad in (-1, N.REGISTER_MAX_PAIRS + 1):
        assert _abi_reduce(n_planes=bad) < 0 and "n_planes" in err() and "wm_register_reduce_u8" in err()
    for bad in (0, -1, N.REGISTER_MAX_LEVEL + 1):
        assert _abi_reduce(level=bad) < 0 and "level" in err()
    for bad in (0, -64, MAX_EXT + 1, MAX_EXT + 64):
        assert _abi_reduce(ext=bad, level=1) < 0 and "ext" in err()
    for ext, level in ((66, 2), (72, 4), (1, 1), (639, 1), (608, 6)):
        assert _abi_reduce(ext=ext, level=level) < 0 and "ext" in err() and "multiple" in err()
    assert _abi_reduce(src=0) < 0 and "in_dev" in err() and "null" in err()
    assert _abi_reduce(out=0) < 0 and "out_dev" in err() and "null" in err()
    for off in (1, 2, 3):
        assert _abi_reduce(src=0x10000 + off) < 0 and "in_dev" in err() and "aligned" in err()
        assert _abi_reduce(out=0x80000 + off) < 0 and "out_dev" in err() and "aligned" in err()
    # 3 planes of 64 x 64 in, 3 of 16 x 16 out: every way the two ranges can meet
    n_in, n_out = 3 * 64 * 64, 3 * 16 * 16
    for out in (0x10000, 0x10000 + n_in - 4, 0x10000 - n_out + 4, 0x10000 + 1024):
        assert _abi_reduce(out=out) < 0 and "overlap" in err() and "in_dev" in err() and "out_dev" in err()
    # n_planes == 0 returns 0 before looking at any pointer or size
    assert _abi_reduce(n_planes=0, src=0, out=0, ext=0, level=0) == 0


def test_reduce_symbol_constant_and_abi_13():
    hdr = header()
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey registration, pyramid" in hdr and len(re.findall("13, additive", hdr)) == 5
    assert re.search(r"13, also additive: wm_register_reduce_u8, WM_REGISTER_MAX_LEVEL", hdr)
    assert entry_is_whole("wm_register_reduce_u8")
    assert macro("WM_REGISTER_MAX_LEVEL") == N.REGISTER_MAX_LEVEL == tiling.REGISTER_MAX_LEVEL == 6
    assert callable(tiling.reduce_planes)
    kern = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "register_pyramid_kernels.h")).read()
    assert "asm" not in kern and "atomic" not in kern.replace("no atomic", "") and "__shared__" not in kern


# ---- GPU: the kernel against the rule --------------------------------------------------------------------------------------

def _check_reduce(planes, level):
    want = reduce_oracle(planes, level)
    got, before, behind, came_back = device_reduce(planes, level)
    np.testing.assert_array_equal(got, want)
    assert (before == 0x5A).all() and (behind == 0x5A).all()                          # nothing outside the output was written
    np.testing.assert_array_equal(came_back, planes)                                  # and the input is as it was
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("ext,level", REDUCE_SHAPES)
@pytest.mark.parametrize("n_planes", (1, 3))
def test_gpu_reduce_equals_the_rule(ext, level, n_planes):
    want = _check_reduce(masked_planes(ext, level, n_planes), level)
    if want.size == 1:                                                                # one cell: the same plane seen whole, too
        assert want.item() == 0 and _check_reduce(masked_planes(ext, level, n_planes, masked=False), level).item() != 0
    else:
        assert (want == 0).any() and (want != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("ext,level", REDUCE_SHAPES)
def test_gpu_reduce_of_the_extreme_planes(ext, level):
    want = _check_reduce(np.stack([np.full((ext, ext), 255, dtype=np.uint8), np.full((ext, ext), 1, dtype=np.uint8)]), level)
    assert (want[0] == 255).all() and (want[1] == 1).all()


@pytest.mark.gpu
def test_gpu_reduce_planes_wrapper_and_an_empty_stack():
    planes = masked_planes(72, 3, 3)
    got = tiling.reduce_planes(_up(planes), 3)
    assert got.shape == (3, 9, 9) and got.dtype == torch.uint8 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), reduce_oracle(planes, 3))
    assert tiling.reduce_planes(torch.zeros((0, 8, 8), device=DEV, dtype=torch.uint8), 2).shape == (0, 2, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("search,level", ((2, 1), (4, 2)))
def test_gpu_reduce_of_the_real_render_and_the_ring(search, level):
    case = dict(_several_pairs(), search=search)                                     # side 72, five pairs, one frame yawed 45 degrees
    a, b = _planes(case)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    _render(case, a, b, status, list(range(len(case["images"]))))
    assert status.item() == 0
    want = _oracle(case)
    ra, rb = tiling.reduce_planes(a, level).cpu().numpy(), tiling.reduce_planes(b, level).cpu().numpy()
    np.testing.assert_array_equal(ra, reduce_oracle(np.stack(want["a"]), level))
    np.testing.assert_array_equal(rb, reduce_oracle(np.stack(want["b"]), level))
    assert (ra != 0).any() and (ra == 0).any() and rb.shape[1] == ra.shape[1] + 2
    # both planes of a pair from one frame: the reduced B's inner grid sits on the reduced A's cells
    x0, y0 = 1000.0, 2000.0
    same = dict(case, pairs=_pairs([(0, 0, 72, 72, x0, y0), (2, 2, 72, 72, x0 - 4.0, y0 - 4.0), (3, 3, 32, 28, x0 + 9.5, y0 + 8.0)]))
    a, b = _planes(same)
    _render(same, a, b, status, list(range(len(same["images"]))))
    assert status.item() == 0
    ra, rb = tiling.reduce_planes(a, level).cpu().numpy(), tiling.reduce_planes(b, level).cpu().numpy()
    for p, (gx, gy) in enumerate(((72, 72), (72, 72), (32, 28))):                       # A ends at gx x gy, B's ring lies beyond it
        cx, cy = gx >> level, gy >> level
        np.testing.assert_array_equal(rb[p, 1:1 + cy, 1:1 + cx], ra[p, :cy, :cx])
        assert (ra[p, cy:] == 0).all() and (ra[p, :, cx:] == 0).all()
    assert (rb[2, 1:8, 1 + (32 >> level)] != 0).all() and (ra[0] != 0).all() and (ra[1] == 0).any() and (ra[1] != 0).any()            # the yawed frame's edge crosses its patch


# ---- GPU: the whole loop ---------------------------------------------------------------------------------------------------

def _equals_loop(out, want, levels):
    last = want["steps"][-1]
    np.testing.assert_array_equal(out["pairs"], want["table"])
    for key, ref in (("georef", want["georef"]), ("param", last["param"]), ("cells", last["cells"]), ("accepted", last["accepted"]),
                     ("rms", last["rms"])):
        np.testing.assert_array_equal(out[key], ref, err_msg=key)                    # the same integers into the same host code
    assert [h["level"] for h in out["history"]] == want["levels"] if levels else all("level" not in h for h in out["history"])
    assert [h["max_corner"] for h in out["history"]] == [s["max_corner"] for s in want["steps"]]


@pytest.mark.gpu
def test_gpu_refine_with_levels_equals_the_oracle_loop_and_converges():
    frames, true, pert = analytic_scene("far")
    want = oracle_loop("far", 3, 3, False)
    out = tiling.refine(frames, pert, CELL, side=SIDE, iters=3, levels=3, fixed=[0])
    _equals_loop(out, want, 3)
    first, err = _corner_error(pert, true), _corner_error(out["georef"], true)
    print("device: worst corner error", first, "->", err, "history", out["history"])
    assert err <= 0.25 * CELL and len(out["history"]) == 12 and (out["georef"][0] == true[0]).all()
    for f in range(1, 4):                                                            # as in test_register_refine: 0.5 m over 256 m
        assert abs(out["yaw"][f] + np.radians(FAR[f][2])) < 2e-3 and abs((1 + out["scale"][f]) * (1 + FAR[f][3]) - 1) < 2e-3
    # today's loop from the same start, nine iterations: it ends more than a cell off
    plain = tiling.refine(frames, pert, CELL, side=SIDE, iters=9, levels=0, fixed=[0])
    _equals_loop(plain, oracle_loop("far", 0, 9, False), 0)
    assert _corner_error(plain["georef"], true) > CELL


@pytest.mark.gpu
def test_gpu_refine_with_levels_lazy_frames_and_chunks():
    frames, true, pert = analytic_scene("far")
    whole = tiling.refine(frames, pert, CELL, side=SIDE, iters=3, levels=3, fixed=[0])
    lazy = _Lazy(frames)
    again = tiling.refine(lazy, pert, CELL, sizes=SIZES, side=SIDE, iters=3, levels=3, fixed=[0], pair_chunk=4)
    for key in ("georef", "yaw", "scale", "shift", "pairs", "param", "cells", "rms", "accepted"):
        assert np.asarray(again[key]).tobytes() == np.asarray(whole[key]).tobytes(), key
    assert again["history"] == whole["history"]
    assert lazy.asked == [0, 1, 2, 3, 1, 2, 3] * 12                                   # chunks (0,1)(0,2)(0,3)(1,2) | (1,3)(2,3), twelve times


@pytest.mark.gpu
def test_gpu_refine_with_levels_and_exposure_equals_its_oracle_loop():
    frames, true, pert = analytic_scene("far")
    out = tiling.refine(frames, pert, CELL, side=SIDE, iters=2, levels=2, exposure=True, fixed=[0])
    _equals_loop(out, oracle_loop("far", 2, 2, True), 2)
    print("exposure=True, levels=2: worst corner error", _corner_error(out["georef"], true))


@pytest.mark.gpu
def test_gpu_refine_with_a_pair_too_small_for_a_level():
    frames, true, pert = analytic_scene("far")
    want = _small_loop()[1]
    out = tiling.refine(frames, pert, CELL, side=SIDE, iters=1, levels=3, fixed=[0], pairs=want["table"])
    _equals_loop(out, want, 3)


@pytest.mark.gpu
def test_gpu_register_passes_levels_to_the_refinement():
    frames, true, pert = analytic_scene("near")                                       # test_register_refine's small perturbation
    assert 1.4 < _corner_error(pert, true) < 1.8                                      # 1.68 m there
    kw = dict(search=8, side=SIDE, fixed=[0])
    both = tiling.register(frames, pert, CELL, refine=2, levels=2, **kw)
    searched = tiling.register(frames, pert, CELL, refine=0, **kw)
    alone = tiling.refine(frames, searched["georef"], CELL, side=SIDE, iters=2, levels=2, fixed=[0], pairs=searched["pairs"])
    np.testing.assert_array_equal(both["georef"], searched["georef"])                 # 'georef' stays the search's
    np.testing.assert_array_equal(both["refine"]["georef"], alone["georef"])          # and 'refine' is refine(levels=2) from there
    assert [h["level"] for h in both["refine"]["history"]] == [2, 2, 1, 1, 0, 0]
    assert _corner_error(both["refine"]["georef"], true) <= 0.25 * CELL
