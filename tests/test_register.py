"""Survey registration (include/wm_hip.h "Survey registration", tiling.register): every overlapping pair of frames rendered
onto a common ground patch as two luma planes, and the integer shift at which they agree.  The rule has no reference
behaviour; register_oracle (tests/register_cases.py) restates it sequentially -- render, search and pick, one pair and one offset at a time,
numpy float64 for the cell centres and int64 for everything after them, the header's operation order -- and the device
result must equal it exactly: every device comparison is assert_array_equal and there is no tolerance on the GPU side.
The only bound in this file is adjust()'s 1e-9 m on consistent measurements (double rounding of such a system sits near
1e-15; the bound is slack, not measured)."""
import os
import re

import numpy as np
import pytest
import torch

from ground_cases import FRAME_SWEEP, RESIDENT_SWEEP, _p, entry_is_whole, header, last_error, macro
from register_cases import (ANIMALS, DISPLACED, HAND_A, HAND_B, INF, NAN, POISON_A, POISON_B, SHAPES, _axis_frame, _case, _content, _cover, _detections,
                            _north_up, _oracle, _pairs, _planes, _render, _search, _several_pairs, _shape_case, _survey,
                            beats, luma, per_k_planes, pick_oracle, render_plane, search_oracle)
from survey_util import DEV, ROOT, _Lazy, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling


# ---- CPU: the oracle's hand cases ------------------------------------------------------------------------------------

def test_oracle_luma_hand_cases():
    assert luma(np.array([255, 255, 255], dtype=np.uint8)) == 255          # (256 * 255 + 128) >> 8
    assert luma(np.array([0, 0, 0], dtype=np.uint8)) == 1                  # a black pixel is seen: clamped to 1
    assert luma(np.array([1, 0, 0], dtype=np.uint8)) == 1                  # (77 + 128) >> 8 = 0 -> 1
    assert luma(np.array([10, 20, 30], dtype=np.uint8)) == 18              # 770 + 3000 + 870 + 128 = 4768 >> 8
    assert luma(np.array([40, 50, 60], dtype=np.uint8)) == 48              # 3080 + 7500 + 1740 + 128 = 12448 >> 8


def _one_by_one():
    """A 1 x 1 patch at search 0: two frames of one pixel each over the cell [0, 1) x [0, 1)."""
    fa = _axis_frame(np.array([[[10, 20, 30]]], dtype=np.uint8), 0.0, 1.0, 1.0)
    fb = _axis_frame(np.array([[[40, 50, 60]]], dtype=np.uint8), 0.0, 1.0, 1.0)
    return _case([fa, fb], [(0, 1, 1, 1, 0.0, 0.0)], 1.0, 0, 1, 1)


def test_oracle_one_by_one_patch_at_search_0():
    want = _oracle(_one_by_one())
    assert want["a"][0].tolist() == [[18]] and want["b"][0].tolist() == [[48]]
    assert want["score"][0].tolist() == [[[30, 1]]]
    assert want["best"][0].tolist() == [0, 0, 30, 1, 0, 0, -1, 0]


# B[j + 1 + dy][i + 1 + dx] against A[j][i], only where both are not 0.  (0, 0): all four agree.  (0, 1): 2|1 and 4|3;
# (0, -1): 1|2 and 3|4; (1, 0): 3|1 and 4|2; (-1, 0): 1|3 and 2|4; the corners meet in one cell: (1, 1) 4|1, (-1, -1) 1|4,
# (1, -1) 3|2, (-1, 1) 2|3.
HAND_SCORE = [[(3, 1), (4, 2), (1, 1)],
              [(2, 2), (0, 4), (2, 2)],
              [(1, 1), (4, 2), (3, 1)]]


def test_oracle_3x3_score_table_at_search_1():
    score = search_oracle(HAND_A, HAND_B, 2, 2, 1)
    assert score.tolist() == [[list(c) for c in row] for row in HAND_SCORE]
    assert pick_oracle(score, 1, 1).tolist() == [0, 0, 0, 4, 0, 0, -1, 0]            # nothing lies outside the peak's 3 x 3
    assert pick_oracle(score, 1, 3).tolist() == [0, 0, 0, 4, 0, 0, -1, 0]
    assert pick_oracle(score, 1, 5).tolist() == [0, 0, -1, 0, 0, 0, -1, 0]          # no offset has 5 cells


def test_oracle_constant_planes_tie_to_the_centre():
    A, B = np.full((4, 4), 9, dtype=np.uint8), np.full((8, 8), 9, dtype=np.uint8)
    score = search_oracle(A, B, 4, 4, 2)
    assert (score[..., 0] == 0).all() and (score[..., 1] == 16).all()
    # every offset ties at sad 0: (0, 0) has the smallest dy^2 + dx^2; outside its 3 x 3 the smallest key is d2 = 4, dy = -2, dx = 0
    assert pick_oracle(score, 2, 1).tolist() == [0, 0, 0, 16, -2, 0, 0, 16]


def test_oracle_equal_cross_products_with_different_n():
    score = np.zeros((3, 3, 2), dtype=np.int64)
    score[2, 1] = (1, 2)                                                              # (dy, dx) = (1, 0): mean 1/2
    score[0, 1] = (2, 4)                                                              # (-1, 0): mean 2/4, the same
    assert not beats((1, 2, 1, 0), (2, 4, -1, 0)) and beats((2, 4, -1, 0), (1, 2, 1, 0))   # 1 * 4 == 2 * 2: dy -1 < 1
    # (1, 0) lies two rows from the peak (-1, 0), outside its 3 x 3: it is the runner-up
    assert pick_oracle(score, 1, 1).tolist() == [-1, 0, 2, 4, 1, 0, 1, 2]
    score[1, 2] = (3, 6)                                                              # (0, 1): the same mean again, key (1, 0, 1) > (1, -1, 0)
    assert pick_oracle(score, 1, 1).tolist() == [-1, 0, 2, 4, 1, 0, 1, 2]
    score[1, 1] = (5, 10)                                                             # (0, 0): the same mean, d2 = 0 wins
    assert pick_oracle(score, 1, 1).tolist() == [0, 0, 5, 10, 0, 0, -1, 0]
    score[1, 1] = (5, 9)                                                              # a worse mean loses whatever its key
    assert pick_oracle(score, 1, 1).tolist() == [-1, 0, 2, 4, 1, 0, 1, 2]


def test_oracle_black_pixel_is_seen_and_outside_is_not():
    black = _axis_frame(np.zeros((2, 2, 3), dtype=np.uint8), 1.0, 3.0, 1.0)          # covers [1, 3) x [1, 3)
    plane = render_plane(tiling.ground_to_pixel(black[1]).reshape(6), (2, 2), black[0], 0.0, 0.0, 1.0, 4, 4, 0, 5)
    want = np.zeros((5, 5), dtype=np.uint8)
    want[1:3, 1:3] = 1
    assert plane.tolist() == want.tolist()
    # the B plane is the same grid grown by `search`: cell (j + s, i + s) of B is cell (j, i) of A
    grown = render_plane(tiling.ground_to_pixel(black[1]).reshape(6), (2, 2), black[0], 0.0, 0.0, 1.0, 4, 4, 2, 9)
    assert grown[2:7, 2:7].tolist() == want.tolist() and grown.sum() == 4


# ---- CPU: register_pairs and adjust ----------------------------------------------------------------------------------


def test_register_pairs_snapping_crop_and_drop():
    # footprints [0.3, 100.3] x [0.2, 80.2] and [60.7, 160.7] x [10.6, 90.6]: intersection [60.7, 100.3] x [10.6, 80.2]
    g = np.stack([_north_up(0.3, 0.2, 100, 80), _north_up(60.7, 10.6, 100, 80)])
    sizes = [(80, 100), (80, 100)]
    t = tiling.register_pairs(g, sizes, 0.5, search=4, side=512, min_cells=1)
    assert t.dtype == tiling.REGISTER_PAIR and t.dtype.itemsize == 32 and t.shape == (1,)
    # floor(60.7 / 0.5) = 121, ceil(100.3 / 0.5) = 201: 80 cells from 60.5; floor(10.6 / 0.5) = 21, ceil(80.2 / 0.5) = 161: 140 from 10.5
    assert t[0].tolist() == (0, 1, 80, 140, 60.5, 10.5)
    # centre crop to side 64: i0 += (80 - 64) // 2 = 8 -> 129, j0 += (140 - 64) // 2 = 38 -> 59
    t = tiling.register_pairs(g, sizes, 0.5, side=64, min_cells=1)
    assert t[0].tolist() == (0, 1, 64, 64, 64.5, 29.5)
    # an odd surplus crops one cell more on the far side: (80 - 63) // 2 = 8
    t = tiling.register_pairs(g, sizes, 0.5, side=63, min_cells=1)
    assert t[0].tolist() == (0, 1, 63, 63, 64.5, 29.5)
    # dropped below min_cells: 80 * 140 = 11200
    assert tiling.register_pairs(g, sizes, 0.5, min_cells=11200).shape == (1,)
    assert tiling.register_pairs(g, sizes, 0.5, min_cells=11201).shape == (0,)


def test_register_pairs_disjoint_nan_and_order():
    g = np.stack([_north_up(0, 0, 100, 80), _north_up(500, 0, 100, 80), _north_up(50, 40, 100, 80), _north_up(100, 0, 100, 80),
                  _north_up(20, 20, 100, 80)])
    sizes = [(80, 100)] * 5
    t = tiling.register_pairs(g, sizes, 1.0, min_cells=1)
    # frame 1 is far away; frame 3 only touches frame 0 along x = 100 (no area)
    assert [(int(p["frame_a"]), int(p["frame_b"])) for p in t] == [(0, 2), (0, 4), (2, 3), (2, 4), (3, 4)]
    assert t[0].tolist() == (0, 2, 50, 40, 50.0, 40.0)
    g[4, 0, 2] = NAN
    t = tiling.register_pairs(g, sizes, 1.0, min_cells=1)
    assert [(int(p["frame_a"]), int(p["frame_b"])) for p in t] == [(0, 2), (2, 3)]
    g[:] = NAN
    assert tiling.register_pairs(g, sizes, 1.0, min_cells=1).shape == (0,)
    assert tiling.register_pairs(np.zeros((0, 2, 3)), np.zeros((0, 2), dtype=np.int32), 1.0).shape == (0,)
    # a frame below 1 x 1 is in no pair
    g = np.stack([_north_up(0, 0, 100, 80), _north_up(10, 10, 100, 80)])
    assert tiling.register_pairs(g, [(80, 100), (0, 100)], 1.0, min_cells=1).shape == (0,)
    # a yawed frame's box is its corners' extent
    # a yawed frame's box is its corners' extent: 100 wide and 80 high at yaw 90 covers [-40, 40] x [-50, 50]; the second
    # frame, [-30.5, 19.5] x [-48.5, -18.5], lies inside that (and would not inside [-50, 50] x [-40, 40])
    g = np.stack([tiling.nadir_affine(80, 100, (0.0, 0.0), 1.0, 90.0), _north_up(-30.5, -48.5, 50, 30)])
    t = tiling.register_pairs(g, [(80, 100), (30, 50)], 1.0, min_cells=1)
    assert t[0].tolist() == (0, 1, 51, 31, -31.0, -49.0)


def test_adjust_consistent_measurements_are_returned():
    true = np.array([[3.0, -2.0], [-4.0, 1.0], [2.0, 3.0], [-1.5, -2.25], [0.5, 0.25]])
    assert np.abs(true.mean(axis=0)).max() == 0.0
    ab = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 3)])
    m = true[ab[:, 1]] - true[ab[:, 0]]
    w = np.array([4096.0, 10000.0, 512.0, 7.0, 30000.0, 1.0])
    out = tiling.adjust(5, ab, m, w)
    assert np.abs(out["shift"] - true).max() < 1e-9
    assert np.abs(out["residual"]).max() < 1e-9
    assert out["component"].tolist() == [0, 0, 0, 0, 0]
    table = _pairs([(a, b, 8, 8, 0.0, 0.0) for a, b in ab])                       # the pair table is accepted as it is
    assert np.array_equal(tiling.adjust(5, table, m, w)["shift"], out["shift"])


def test_adjust_components_fixed_and_isolated():
    # frames 0-1-2 and 4-5 are two components; 3 has no pair; the pair (2, 4) has weight 0 and joins nothing
    ab = np.array([(0, 1), (1, 2), (4, 5), (2, 4)])
    m = np.array([[2.0, 0.0], [2.0, 2.0], [0.0, -6.0], [100.0, 100.0]])
    w = np.array([10.0, 10.0, 5.0, 0.0])
    out = tiling.adjust(6, ab, m, w)
    want = np.array([[-2.0, -2.0 / 3], [0.0, -2.0 / 3], [2.0, 4.0 / 3], [0.0, 0.0], [0.0, 3.0], [0.0, -3.0]])
    assert np.abs(out["shift"] - want).max() < 1e-9                              # each component's mean shift is 0
    assert out["component"].tolist() == [0, 0, 0, -1, 4, 4]
    assert np.abs(out["residual"][:3]).max() < 1e-9
    assert np.abs(out["residual"][3] - ((want[4] - want[2]) - m[3])).max() < 1e-9    # reported for the unused pair too
    # fixed frames stay at 0 and pin their component; the other component keeps its zero mean
    out = tiling.adjust(6, ab, m, w, fixed=[1, 3])
    want = np.array([[-2.0, 0.0], [0.0, 0.0], [2.0, 2.0], [0.0, 0.0], [0.0, 3.0], [0.0, -3.0]])
    assert np.abs(out["shift"] - want).max() < 1e-9
    assert (out["shift"][[1, 3]] == 0.0).all()
    # nothing to solve
    out = tiling.adjust(3, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2)), np.zeros(0))
    assert (out["shift"] == 0).all() and out["component"].tolist() == [-1, -1, -1] and out["residual"].shape == (0, 2)


def test_adjust_inconsistent_measurements_give_the_weighted_mean():
    # the same pair measured twice: t1 - t0 = 1 with weight 3 and = 5 with weight 1 -> (3 * 1 + 1 * 5) / 4 = 2
    out = tiling.adjust(2, [(0, 1), (0, 1)], [[1.0, 10.0], [5.0, 50.0]], [3.0, 1.0])
    assert np.abs(out["shift"] - np.array([[-1.0, -10.0], [1.0, 10.0]])).max() < 1e-9
    assert np.abs(out["residual"] - np.array([[1.0, 10.0], [-3.0, -30.0]])).max() < 1e-9
    assert np.abs(out["residual"]).min() > 0.5
    # a triangle that does not close: the misclosure is spread, the residuals are not 0
    out = tiling.adjust(3, [(0, 1), (1, 2), (0, 2)], [[1.0, 0.0], [1.0, 0.0], [5.0, 0.0]], [1.0, 1.0, 1.0])
    assert np.abs(out["residual"][:, 0] - np.array([1.0, 1.0, -1.0])).max() < 1e-9
    assert np.abs(out["shift"].sum(axis=0)).max() < 1e-9


def test_register_python_argument_errors_before_device_work():
    g = np.stack([_north_up(0, 0, 100, 80), _north_up(10, 10, 100, 80)])
    sizes = [(80, 100), (80, 100)]
    imgs = [np.zeros((80, 100, 3), dtype=np.uint8)] * 2
    lazy = _Lazy(imgs)
    for name, bads in (("search", (-1, 65, 2.5, "4", None, True, NAN)), ("side", (0, 513, 1.5, "64", None, True)),
                       ("min_cells", (0, -3, 2.5, None, "1", 2 ** 31))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                tiling.register(lazy, g, 1.0, sizes=sizes, **{name: bad})
            with pytest.raises(ValueError, match=name):
                tiling.register_pairs(g, sizes, 1.0, **{name: bad})
    for bad in (0, -1, 2.5, "8", None, True, 65536):
        with pytest.raises(ValueError, match="pair_chunk"):
            tiling.register(lazy, g, 1.0, sizes=sizes, pair_chunk=bad)
    for bad in (-0.5, NAN, INF, "big", None):
        with pytest.raises(ValueError, match="min_ratio"):
            tiling.register(lazy, g, 1.0, sizes=sizes, min_ratio=bad)
    for bad in (0, -1.0, NAN, INF, "wide", None):
        with pytest.raises(ValueError, match="cell"):
            tiling.register(lazy, g, bad, sizes=sizes)
        with pytest.raises(ValueError, match="cell"):
            tiling.register_pairs(g, sizes, bad)
    with pytest.raises(ValueError, match="georef"):
        tiling.register_pairs(np.zeros((2, 3, 2)), sizes, 1.0)
    with pytest.raises(ValueError, match="sizes"):
        tiling.register_pairs(g, [(4.5, 8), (4, 8)], 1.0)
    with pytest.raises(ValueError, match="sizes is required"):
        tiling.register(lazy, g, 1.0)
    with pytest.raises(ValueError, match="indexed"):
        tiling.register(iter(imgs), g, 1.0, sizes=sizes)
    with pytest.raises(ValueError, match="sizes for 2 georeferences"):
        tiling.register(lazy, g, 1.0, sizes=[(80, 100)])
    with pytest.raises(ValueError, match="1 frames for 2 georeferences"):
        tiling.register(_Lazy(imgs[:1]), g, 1.0, sizes=sizes)
    good = _pairs([(0, 1, 8, 8, 0.0, 0.0)])
    for bad in ([(0, 1, 8, 8, 0.0, 0.0)], np.zeros((1, 6)), good.reshape(1, 1), _pairs([(0, 2, 8, 8, 0.0, 0.0)]), _pairs([(-1, 1, 8, 8, 0.0, 0.0)]),
                _pairs([(1, 1, 8, 8, 0.0, 0.0)]), _pairs([(0, 1, 0, 8, 0.0, 0.0)]), _pairs([(0, 1, 8, 65, 0.0, 0.0)]), _pairs([(0, 1, 8, 8, NAN, 0.0)])):
        with pytest.raises(ValueError, match="pairs"):
            tiling.register(lazy, g, 1.0, sizes=sizes, side=64, pairs=bad)
    for bad in ([2], [-1], [0.5], "0", 7):
        with pytest.raises(ValueError, match="fixed"):
            tiling.register(lazy, g, 1.0, sizes=sizes, fixed=bad)
        with pytest.raises(ValueError, match="fixed"):
            tiling.adjust(2, [(0, 1)], [[0.0, 0.0]], [1.0], fixed=bad)
    with pytest.raises(ValueError, match="n_frames"):
        tiling.adjust(-1, [(0, 1)], [[0.0, 0.0]], [1.0])
    for bad in ([(0, 2)], [(0, 0)], [(0.5, 1)], [(0, 1, 2)]):
        with pytest.raises(ValueError, match="pairs"):
            tiling.adjust(2, bad, [[0.0, 0.0]], [1.0])
    with pytest.raises(ValueError, match="measured"):
        tiling.adjust(2, [(0, 1)], [[0.0, 0.0], [1.0, 1.0]], [1.0])
    with pytest.raises(ValueError, match="measured"):
        tiling.adjust(2, [(0, 1)], [[NAN, 0.0]], [1.0])
    for bad in ([-1.0], [NAN], [INF]):
        with pytest.raises(ValueError, match="weights"):
            tiling.adjust(2, [(0, 1)], [[0.0, 0.0]], bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device tensor"):              # no CPU fallback
            tiling.register(lazy, g, 1.0, sizes=sizes, min_cells=1)
    assert lazy.asked == []                                                     # nothing was loaded on the way to an error
    # no pair at all needs no device: every frame keeps its georeference
    far = np.stack([_north_up(0, 0, 100, 80), _north_up(1000, 0, 100, 80)])
    out = tiling.register(lazy, far, 1.0, sizes=sizes)
    assert out["pairs"].shape == (0,) and (out["shift"] == 0).all() and np.array_equal(out["georef"], far) and lazy.asked == []
    assert out["component"].tolist() == [-1, -1] and out["accepted"].shape == (0,) and out["offset"].shape == (0, 2)


def _abi_render(n_frames=2, n_resident=2, n_pairs=3, cell=1.0, search=4, side=64, frames=0x1000, slot=0x7000, g2p=0x2000, size=0x3000,
                pairs=0x4000, a=0x5001, b=0x6001, status=0x9000):
    """wm_register_render_u8 with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_register_render_u8(_p(frames), n_resident, _p(slot), _p(g2p), _p(size), n_frames, _p(pairs), n_pairs, cell, search, side,
                                         _p(a), _p(b), _p(status), None)


def _abi_search(n_pairs=3, search=4, side=64, min_cells=1, a=0x5001, b=0x6001, pairs=0x4000, score=0x8000, best=0xa000):
    return N.lib().wm_register_search(_p(a), _p(b), _p(pairs), n_pairs, search, side, min_cells, _p(score), _p(best), None)


def test_register_abi_argument_errors_without_gpu():
    err = last_error
    for call in (_abi_render, _abi_search):
        assert call(n_pairs=-1) < 0 and "n_pairs" in err()
        assert call(n_pairs=N.REGISTER_MAX_PAIRS + 1) < 0 and "n_pairs" in err()
        assert call(search=-1) < 0 and "search" in err()
        assert call(search=N.REGISTER_MAX_SEARCH + 1) < 0 and "search" in err()
        assert call(side=0) < 0 and "side" in err()
        assert call(side=N.REGISTER_MAX_SIDE + 1) < 0 and "side" in err()
        assert call(pairs=0) < 0 and "pairs_dev" in err()
        assert call(pairs=0x4004) < 0 and "pairs_dev" in err() and "aligned" in err()
        assert call(a=0) < 0 and "a_dev" in err()
        assert call(b=0) < 0 and "b_dev" in err()
        # n_pairs == 0 returns 0 before looking at any pointer or any other argument
        assert call(n_pairs=0, pairs=0, a=0, b=0, search=-5, side=0) == 0
    for kwargs, word in FRAME_SWEEP + RESIDENT_SWEEP:                         # the frame tables and the resident list of the ground entries
        assert _abi_render(**kwargs) < 0 and word in err(), ("_abi_render", kwargs, word, err())
    for bad in (0.0, -1.0, NAN, INF):
        assert _abi_render(cell=bad) < 0 and "cell" in err()
    assert _abi_render(frames=0) < 0 and "frames_dev" in err()
    assert _abi_render(slot=0) < 0 and "slot_dev" in err()
    assert _abi_render(status=0) < 0 and "status_dev" in err()
    assert _abi_render(frames=0x1004) < 0 and "aligned" in err()
    assert _abi_render(slot=0x7002) < 0 and "aligned" in err()
    assert _abi_render(status=0x9002) < 0 and "aligned" in err()
    for bad in (0, -1, -2 ** 31):
        assert _abi_search(min_cells=bad) < 0 and "min_cells" in err()
    assert _abi_search(score=0) < 0 and "score_dev" in err()
    assert _abi_search(best=0) < 0 and "best_dev" in err()
    assert _abi_search(score=0x8002) < 0 and "aligned" in err()
    assert _abi_search(best=0xa002) < 0 and "aligned" in err()


def test_register_symbols_and_abi_13():
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey registration" in header() and len(re.findall("13, additive", header())) >= 3
    for name in ("wm_register_render_u8", "wm_register_search"):
        assert entry_is_whole(name), name
    for name, val in (("WM_REGISTER_MAX_SIDE", N.REGISTER_MAX_SIDE), ("WM_REGISTER_MAX_SEARCH", N.REGISTER_MAX_SEARCH),
                       ("WM_REGISTER_MAX_PAIRS", N.REGISTER_MAX_PAIRS), ("WM_REGISTER_BAD_SLOT", N.REGISTER_BAD_SLOT),
                       ("WM_REGISTER_BAD_SIZE", N.REGISTER_BAD_SIZE), ("WM_REGISTER_BAD_PAIR", N.REGISTER_BAD_PAIR)):
        assert macro(name) == val, name
    assert (N.REGISTER_MAX_SIDE, N.REGISTER_MAX_SEARCH, N.REGISTER_MAX_PAIRS) == (512, 64, 65535)
    assert tiling.REGISTER_PAIR.itemsize == 32 and [tiling.REGISTER_PAIR.fields[k][1] for k in tiling.REGISTER_PAIR.names] == [0, 4, 8, 12, 16, 24]
    kern = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "register_kernels.h")).read()
    assert "__builtin_amdgcn_sad_u8(" in kern and "asm" not in kern


# ---- GPU -------------------------------------------------------------------------------------------------------------


def _run_and_check(case, want=None):
    """Render with every frame resident, search, and compare planes, score and best with the oracle."""
    want = _oracle(case) if want is None else want
    a, b = _planes(case)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    _render(case, a, b, status, list(range(len(case["images"]))))
    assert status.item() == 0
    score, best = _search(case, a, b)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for p in range(len(case["pairs"])):
        np.testing.assert_array_equal(a[p], want["a"][p], err_msg=f"A of pair {p}")
        np.testing.assert_array_equal(b[p], want["b"][p], err_msg=f"B of pair {p}")
        np.testing.assert_array_equal(score[p], want["score"][p], err_msg=f"score of pair {p}")
        np.testing.assert_array_equal(best[p], want["best"][p], err_msg=f"best of pair {p}")
    return want, score, best


@pytest.mark.gpu
def test_gpu_one_by_one_hand_case():
    _, score, best = _run_and_check(_one_by_one())
    assert score.tolist() == [[[[30, 1]]]] and best.tolist() == [[0, 0, 30, 1, 0, 0, -1, 0]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_smallest_shapes(name):
    gx, gy, search, side = SHAPES[name]
    want, score, best = _run_and_check(_shape_case(gx, gy, search, side, seed=sorted(SHAPES).index(name)))
    assert (score[0, :, :, 1] == gx * gy).all()                                       # both frames see everything
    assert (want["a"][0][gy:] == 0).all() and (want["a"][0][:, gx:] == 0).all()       # the zero padding up to side
    assert best[0, 2] >= 0


@pytest.mark.gpu
def test_gpu_several_pairs_in_one_launch():
    want, score, best = _run_and_check(_several_pairs())
    assert best[4].tolist() == [0, 0, -1, 0, 0, 0, -1, 0]                              # 1 cell < min_cells 40
    assert (best[:4, 2] >= 0).all() and (best[:4, 6] >= 0).all()
    diagonal = want["a"][3]                                                           # pair 3's A is the frame yawed 45 degrees
    assert 0 < (diagonal[:72, :72] != 0).sum() < 72 * 72


@pytest.mark.gpu
def test_gpu_diagonal_mask_edge_and_a_frame_that_sees_nothing():
    x0, y0, cell = 300.0, 400.0, 1.0
    small = _content(40, 40, 21), tiling.nadir_affine(40, 40, (x0 + 30.0, y0 + 30.0), 1.0, 45.0)     # a diamond inside the patch
    full = _cover(60, 60, 5, x0, y0, cell, 22)
    away = _content(30, 30, 23), tiling.nadir_affine(30, 30, (x0 + 5000.0, y0), 1.0, 0.0)
    nan = _content(30, 30, 24), np.full((2, 3), NAN)
    case = _case([small, full, away, nan], [(0, 1, 60, 60, x0, y0), (1, 0, 60, 60, x0, y0), (1, 2, 60, 60, x0, y0), (1, 3, 60, 60, x0, y0)],
                 cell, 5, 64, 100)
    want, score, best = _run_and_check(case)
    seen = want["a"][0] != 0
    assert 0 < seen.sum() < 60 * 60 and not seen[0, 0] and seen[30, 30]               # the mask's edge is diagonal
    assert len(set(score[0, :, :, 1].reshape(-1).tolist())) == 1                      # A's mask alone decides n
    assert len(set(score[1, :, :, 1].reshape(-1).tolist())) > 1                       # B's mask moves with the offset
    for p in (2, 3):                                                                  # B never sees the patch
        assert (want["b"][p] == 0).all() and (score[p] == 0).all()
        assert best[p].tolist() == [0, 0, -1, 0, 0, 0, -1, 0]


def _plane_case(A, B, gx, gy, search, min_cells=1):
    """Hand-built planes, for the search alone: a list of (A (side,side), B (E,E)) per pair."""
    side = A[0].shape[0]
    pairs = _pairs([(0, 1, gx, gy, 0.0, 0.0)] * len(A))
    return {"pairs": pairs, "search": search, "side": side, "min_cells": min_cells}, _up(np.stack(A)), _up(np.stack(B))


@pytest.mark.gpu
def test_gpu_hand_score_table_and_ties():
    case, a, b = _plane_case([HAND_A], [HAND_B], 2, 2, 1)
    score, best = _search(case, a, b)
    assert score[0].tolist() == [[list(c) for c in row] for row in HAND_SCORE]
    assert best[0].tolist() == [0, 0, 0, 4, 0, 0, -1, 0]
    # constant planes: every offset ties at sad 0, the pick is (0, 0), the runner-up (-2, 0)
    case, a, b = _plane_case([np.full((4, 4), 9, dtype=np.uint8)], [np.full((8, 8), 9, dtype=np.uint8)], 4, 4, 2)
    score, best = _search(case, a, b)
    assert (score[0, :, :, 0] == 0).all() and (score[0, :, :, 1] == 16).all()
    assert best[0].tolist() == [0, 0, 0, 16, -2, 0, 0, 16]
    # equal cross products with different n.  A's only seen cells are rows 1, 2 x columns 0, 1 = (10, 200); they meet B's
    # columns 1, 2 at dx = 0 and rows (j + 1 + dy): (-1, 0) rows 1, 2: 0 + 2 over 4 cells; (0, 0) rows 2, 3: 2 + 1 over 4;
    # (1, 0) rows 3, 4: 1 over 2 (row 4 is not seen).  2 * 2 == 1 * 4, and dy = -1 < 1 decides; dx = +-1 pairs 10 with 200.
    A = np.zeros((4, 4), dtype=np.uint8)
    A[1:3, 0], A[1:3, 1] = 10, 200
    B = np.zeros((6, 6), dtype=np.uint8)
    B[1, 1:3], B[2, 1:3], B[3, 1:3] = (10, 200), (12, 200), (10, 201)
    want = search_oracle(A, B, 4, 4, 1)
    assert want[0, 1].tolist() == [2, 4] and want[1, 1].tolist() == [3, 4] and want[2, 1].tolist() == [1, 2]
    case, a, b = _plane_case([A], [B], 4, 4, 1, min_cells=2)
    score, best = _search(case, a, b)
    np.testing.assert_array_equal(score[0], want)
    assert best[0].tolist() == [-1, 0, 2, 4, 1, 0, 1, 2] == pick_oracle(want, 1, 2).tolist()       # (1, 0): the runner-up


@pytest.mark.gpu
def test_gpu_min_cells_boundary_on_a_hand_built_mask():
    rng = np.random.default_rng(5)
    A = np.zeros((70, 70), dtype=np.uint8)
    cells = rng.permutation(66 * 67)[:1234]
    A[cells // 66, cells % 66] = rng.integers(1, 256, size=1234)                    # gx = 66, gy = 67: exactly 1234 seen cells
    A[:, 66:] = 200                                                                 # beyond gx: must not count
    A[67:, :] = 200
    B = rng.integers(1, 256, size=(70, 70), dtype=np.uint8)                         # search 0: E = side; B sees everything
    case, a, b = _plane_case([A], [B], 66, 67, 0)
    want = search_oracle(A, B, 66, 67, 0)
    assert want[0, 0, 1] == 1234
    score, best = _search(case, a, b, min_cells=1234)
    np.testing.assert_array_equal(score[0], want)
    assert best[0].tolist() == [0, 0, int(want[0, 0, 0]), 1234, 0, 0, -1, 0]          # n == min_cells is eligible
    score, best = _search(case, a, b, min_cells=1235)
    np.testing.assert_array_equal(score[0], want)
    assert best[0].tolist() == [0, 0, -1, 0, 0, 0, -1, 0]                            # n == min_cells - 1 is not


@pytest.mark.gpu
def test_gpu_extremes_white_against_black_and_sprinkled_zeros():
    white = _axis_frame(np.full((8, 8, 3), 255, dtype=np.uint8), -100.0, 700.0, 100.0)      # covers [-100, 700)^2
    black = _axis_frame(np.zeros((8, 8, 3), dtype=np.uint8), -100.0, 700.0, 100.0)
    case = _case([white, black], [(0, 1, 512, 512, 0.0, 0.0)], 1.0, 0, 512, 1)
    a, b = _planes(case)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    _render(case, a, b, status, [0, 1])
    assert status.item() == 0 and (a == 255).all().item() and (b == 1).all().item()
    score, best = _search(case, a, b)
    assert score.tolist() == [[[[66584576, 512 * 512]]]] and 254 * 512 * 512 == 66584576
    assert best.tolist() == [[0, 0, 66584576, 262144, 0, 0, -1, 0]]
    # random content with not-seen cells sprinkled into both planes, two pairs of one launch
    rng = np.random.default_rng(9)
    A = [np.where(rng.random((72, 72)) < 0.2, 0, rng.integers(1, 256, size=(72, 72))).astype(np.uint8) for _ in range(2)]
    B = [np.where(rng.random((82, 82)) < 0.3, 0, rng.integers(1, 256, size=(82, 82))).astype(np.uint8) for _ in range(2)]
    case, a, b = _plane_case(A, B, 70, 45, 5, min_cells=300)
    score, best = _search(case, a, b)
    for p in range(2):
        want = search_oracle(A[p], B[p], 70, 45, 5)
        np.testing.assert_array_equal(score[p], want)
        np.testing.assert_array_equal(best[p], pick_oracle(want, 5, 300))


_PER_K_WANT = []


def _per_k_want():
    """(score, best) of the oracle on per_k_planes() at size (70, 45), min_cells 300; computed once for the three K."""
    if not _PER_K_WANT:
        A, B = per_k_planes()
        score = search_oracle(A, B, 70, 45, 5)
        _PER_K_WANT.append((score, pick_oracle(score, 5, 300)))
    return _PER_K_WANT[0]


def test_oracle_per_k_case_has_a_best_and_a_runner_up():
    score, best = _per_k_want()                                                      # about 56 % of 3150 cells at the central offsets
    assert best[2] >= 0 and best[6] >= 0 and best[3] >= 300 and best[7] >= 300


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 2, 4))
def test_gpu_every_offsets_per_thread_instance(k, monkeypatch):
    """WM_REGISTER_K forces the instance (the launcher reads it per call); the result does not depend on it.  At search 5
    the 121 offsets leave most threads of a K = 4 block without one: they walk the last offset and drop it."""
    monkeypatch.setenv("WM_REGISTER_K", str(k))
    A, B = per_k_planes()
    want_score, want_best = _per_k_want()
    assert want_best[2] >= 0 and want_best[6] >= 0                                    # the case cannot pass by having nothing eligible
    case, a, b = _plane_case([A], [B], 70, 45, 5, min_cells=300)
    score, best = _search(case, a, b)
    np.testing.assert_array_equal(score[0], want_score)
    np.testing.assert_array_equal(best[0], want_best)


@pytest.mark.gpu
def test_gpu_render_is_order_free():
    case = _several_pairs()
    want = _oracle(case)
    for order in ([[0, 1], [2, 3]], [[3, 2], [1, 0]], [[2], [0], [3], [1]]):
        a, b = _planes(case)
        status = torch.zeros(1, device=DEV, dtype=torch.int32)
        done = set()
        for resident in order:
            _render(case, a, b, status, resident)
            done |= set(resident)
            now_a, now_b = a.cpu().numpy(), b.cpu().numpy()
            for p, pr in enumerate(case["pairs"]):                                    # after EVERY call
                np.testing.assert_array_equal(now_a[p], want["a"][p] if int(pr["frame_a"]) in done else POISON_A)
                np.testing.assert_array_equal(now_b[p], want["b"][p] if int(pr["frame_b"]) in done else POISON_B)
        assert status.item() == 0


@pytest.mark.gpu
def test_gpu_bad_residency_is_reported_and_skipped():
    case = _several_pairs()
    want = _oracle(case)
    F = len(case["images"])
    good = np.arange(F, dtype=np.int32)

    def run(c, slot, images=None):
        a, b = _planes(c)
        status = torch.zeros(1, device=DEV, dtype=torch.int32)
        _render(c, a, b, status, list(range(F)), slot=slot, images=images)
        return a, b, status.item()

    def check(c, w, a, b, skipped_frames=(), skipped_pairs=()):
        score, best = _search(c, a, b)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        for p, pr in enumerate(c["pairs"]):
            a_ok = p not in skipped_pairs and int(pr["frame_a"]) not in skipped_frames
            b_ok = p not in skipped_pairs and int(pr["frame_b"]) not in skipped_frames
            np.testing.assert_array_equal(a[p], w["a"][p] if a_ok else POISON_A, err_msg=f"A {p}")
            np.testing.assert_array_equal(b[p], w["b"][p] if b_ok else POISON_B, err_msg=f"B {p}")
            if a_ok and b_ok:                                                         # the other pairs of the launch are still exact
                np.testing.assert_array_equal(score[p], w["score"][p], err_msg=f"score {p}")
                np.testing.assert_array_equal(best[p], w["best"][p], err_msg=f"best {p}")
        return score, best

    slot = good.copy()
    slot[2] = F                                                                       # frame 2's slot points past the resident list
    a, b, status = run(case, slot)
    assert status == N.REGISTER_BAD_SLOT
    check(case, want, a, b, skipped_frames={2})
    slot = good.copy()
    slot[1] = 3                                                                       # frame 1's slot holds frame 3's descriptor
    a, b, status = run(case, slot)
    assert status == N.REGISTER_BAD_SIZE
    check(case, want, a, b, skipped_frames={1})
    images = list(case["images"])
    images[0] = images[0][:-1].copy()                                                 # a resident frame one row short of size_dev
    a, b, status = run(case, good, images)
    assert status == N.REGISTER_BAD_SIZE
    check(case, want, a, b, skipped_frames={0})
    # bad pairs: a frame index outside the survey, gx = 0, gy past side; the others still exact
    bad = dict(case, pairs=case["pairs"].copy())
    bad["pairs"]["frame_b"][0] = F
    bad["pairs"]["gx"][2] = 0
    bad["pairs"]["gy"][3] = case["side"] + 1
    a, b, status = run(bad, good)
    assert status == N.REGISTER_BAD_PAIR
    score, best = check(bad, want, a, b, skipped_pairs={0, 2, 3})
    for p in (2, 3):                                                                  # the search skips them too: score 0, no best
        assert (score[p] == 0).all() and best[p].tolist() == [0, 0, -1, 0, 0, 0, -1, 0]
    bad["pairs"]["frame_a"][1] = -1
    slot = good.copy()
    slot[0], slot[3] = F + 5, -1                                                      # with a bad slot; a negative slot is not resident
    a, b, status = run(bad, slot)
    assert status == N.REGISTER_BAD_PAIR | N.REGISTER_BAD_SLOT
    check(bad, want, a, b, skipped_frames={0, 3}, skipped_pairs={0, 1, 2, 3})


# ---- end to end ------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_gpu_register_end_to_end_corrects_the_census():
    frames, true, displaced = _survey()
    out = tiling.register(frames, displaced, 1.0, search=8, side=256, min_cells=4096)
    ab = [(int(p["frame_a"]), int(p["frame_b"])) for p in out["pairs"]]
    assert ab == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    want = np.array([DISPLACED[b] - DISPLACED[a] for a, b in ab], dtype=np.int64)
    np.testing.assert_array_equal(out["offset"], want)
    assert out["accepted"].all() and (out["mean"] == 0.0).all() and (out["runner_up"] > 0).all()
    assert np.abs(out["shift"] + DISPLACED).max() < 1e-9
    assert np.abs(out["georef"] - true).max() < 1e-9 and np.abs(out["residual"]).max() < 1e-9
    assert out["component"].tolist() == [0, 0, 0, 0] and (out["cells"] >= 4096).all()
    # the device's best equals the oracle's on this input, planes and all
    case = {"images": frames, "g2p": tiling.ground_to_pixel(displaced).reshape(-1, 6), "size": np.array([(160, 200)] * 4, dtype=np.int32),
            "pairs": out["pairs"][:2], "cell": 1.0, "search": 8, "side": 256, "min_cells": 4096}
    _run_and_check(case)
    # the census: the true count with the corrected georeferences, a larger one with the displaced ones
    dets = _detections(true)
    assert sum(len(d["boxes"]) for d in dets) >= 2 * len(ANIMALS)
    assert tiling.census(dets, out["georef"], 1.5)["count"] == len(ANIMALS) == 12
    assert tiling.census(dets, displaced, 1.5)["count"] > len(ANIMALS)
    # a lazy sequence, two pairs at a time: the same result, every frame asked for only while a chunk needs it
    lazy = _Lazy(frames)
    again = tiling.register(lazy, displaced, 1.0, sizes=[(160, 200)] * 4, search=8, side=256, min_cells=4096, pair_chunk=2)
    for key in out:
        np.testing.assert_array_equal(again[key], out[key], err_msg=key)
    assert lazy.asked == [0, 1, 2, 0, 1, 2, 3, 1, 2, 3]                              # chunks (0,1)(0,2) | (0,3)(1,2) | (1,3)(2,3)
    # fixed= pins the gauge: frame 0 stays, the others move relative to it
    pinned = tiling.register(frames, displaced, 1.0, search=8, side=256, pairs=out["pairs"], fixed=[0])
    assert np.abs(pinned["shift"] - (DISPLACED[0] - DISPLACED)).max() < 1e-9
