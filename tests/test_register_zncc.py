"""Survey registration, correlation search (include/wm_hip.h "Survey registration, correlation search",
tiling.register(metric="zncc")): the offset search of test_register.py with a score that a gain and an offset between the two
frames of a pair do not change.  The rule has no reference behaviour; zncc_search_oracle and zncc_pick_oracle (tests/register_cases.py) restate
it sequentially -- one offset at a time, Python integers for the six moments and their cross terms, three np.float64
operations for the score, in the header's order -- and the device result must equal it exactly: moments and best by
assert_array_equal, peak by its bytes (NaN included).  There is no tolerance in this file.  Planes, pairs and the SAD
oracles are the ones test_register.py uses."""
import os
import re

import numpy as np
import pytest
import torch

import register_cases as T
from ground_cases import _p, entry_is_whole, header, last_error, macro
from survey_util import ROOT, _Lazy
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

F64 = np.float64
NAN = float("nan")
INF = float("inf")
DEV = T.DEV


def corr(q):
    """r = sign(q) * sqrt(|q|), as tiling.register forms it on the host."""
    return np.sign(q) * np.sqrt(np.abs(q))


# ---- CPU: the oracle's hand cases ------------------------------------------------------------------------------------

# T.HAND_A = [[1, 2], [3, 4]] inside T.HAND_B's zero border, search 1.  (0, 0): all four cells, a = b = 1, 2, 3, 4:
# n 4, Sa = Sb = 10, Saa = Sbb = Sab = 30.  (0, 1): a (1, 3) on b (2, 4): Sa 4, Sb 6, Saa 10, Sbb 20, Sab 14; (0, -1) is its
# mirror.  (1, 0): a (1, 2) on b (3, 4): 3, 7, 5, 25, 11; (-1, 0) its mirror.  The corners meet in one cell: (1, 1) 1|4,
# (-1, -1) 4|1, (1, -1) 2|3, (-1, 1) 3|2.
HAND_MOMENTS = [[(1, 4, 1, 16, 1, 4), (2, 7, 3, 25, 5, 11), (1, 3, 2, 9, 4, 6)],
                [(2, 6, 4, 20, 10, 14), (4, 10, 10, 30, 30, 30), (2, 4, 6, 10, 20, 14)],
                [(1, 2, 3, 4, 9, 6), (2, 3, 7, 5, 25, 11), (1, 1, 4, 1, 16, 4)]]


def test_oracle_2x2_moments_at_search_1():
    mo = T.zncc_search_oracle(T.HAND_A, T.HAND_B, 2, 2, 1)
    assert mo.tolist() == [[list(c) for c in row] for row in HAND_MOMENTS]
    # (0, 0): c = 4 * 30 - 100 = 20 = va = vb: q = 400 / 400.  (0, +-1): c = 2 * 14 - 24 = 4, va = 20 - 16 = 4, vb = 40 - 36 = 4: q = 1
    # too, as (+-1, 0): c = 22 - 21 = 1 = va = vb.  One cell has va = 0.  All five tie at q == 1: (0, 0) has the smallest key.
    assert T.zncc_q(mo[1, 1]) == 1.0 and T.zncc_q(mo[1, 2]) == 1.0 and T.zncc_q(mo[0, 1]) == 1.0 and T.zncc_q(mo[0, 0]) is None
    best, peak = T.zncc_pick_oracle(mo, 1, 1)
    assert best.tolist() == [0, 0, 1, 4, 0, 0, 0, 0] and peak[0] == 1.0 and np.isnan(peak[1])   # nothing outside the peak's 3 x 3
    best, peak = T.zncc_pick_oracle(mo, 1, 3)
    assert best.tolist() == [0, 0, 1, 4, 0, 0, 0, 0] and peak[0] == 1.0
    best, peak = T.zncc_pick_oracle(mo, 1, 5)                                           # no offset has 5 cells
    assert best.tolist() == [0] * 8 and np.isnan(peak).all()


def test_oracle_constant_plane_has_no_eligible_offset():
    rng = np.random.default_rng(1)
    A, B = np.full((4, 4), 9, dtype=np.uint8), rng.integers(1, 256, size=(8, 8), dtype=np.uint8)
    mo = T.zncc_search_oracle(A, B, 4, 4, 2)
    assert (mo[..., 0] == 16).all() and (mo[..., 1] == 144).all() and (mo[..., 3] == 1296).all()      # va = 16 * 1296 - 144^2 = 0
    best, peak = T.zncc_pick_oracle(mo, 2, 1)
    assert best.tolist() == [0] * 8 and np.isnan(peak).all()
    best, peak = T.zncc_pick_oracle(T.zncc_search_oracle(B[:4, :4], np.full((8, 8), 200, dtype=np.uint8), 4, 4, 2), 2, 1)   # vb = 0
    assert best.tolist() == [0] * 8 and np.isnan(peak).all()


def test_oracle_gain_and_offset_score_exactly_one():
    rng = np.random.default_rng(2)
    A = rng.integers(1, 120, size=(6, 6), dtype=np.uint8)
    B = rng.integers(1, 256, size=(10, 10), dtype=np.uint8)
    B[2 + 1:2 + 1 + 6, 2 - 2:2 - 2 + 6] = 2 * A + 7                                   # B = 2 A + 7 at (dy, dx) = (1, -2)
    mo = T.zncc_search_oracle(A, B, 6, 6, 2)
    # c = 2 va and vb = 4 va there: q = (2 va)^2 / (va * 4 va), and both products are exact in double (va < 2^26)
    assert T.zncc_q(mo[3, 0]) == 1.0
    best, peak = T.zncc_pick_oracle(mo, 2, 1)
    assert best[:4].tolist() == [1, -2, 1, 36] and peak[0] == 1.0 and best[6] == 1 and peak[1] < 1.0


def test_oracle_anticorrelation_is_negative_and_loses():
    rng = np.random.default_rng(3)
    A = rng.integers(1, 200, size=(5, 5), dtype=np.uint8)
    B = rng.integers(1, 256, size=(9, 9), dtype=np.uint8)
    B[2:7, 2:7] = 255 - A                                                            # (0, 0): the negative of A
    mo = T.zncc_search_oracle(A, B, 5, 5, 2)
    assert T.zncc_q(mo[2, 2]) == -1.0
    table = np.zeros((5, 5, 6), dtype=np.int64)
    table[2, 2] = mo[2, 2]                                                            # q = -1 at (0, 0), the smallest key
    table[4, 4] = (4, 10, 14, 30, 54, 39)                                             # (2, 2): c = 16, va = 20, vb = 20: q = 0.64
    assert T.zncc_q(table[4, 4]) == F64(256.0) / F64(400.0)
    best, peak = T.zncc_pick_oracle(table, 2, 1)
    assert best.tolist() == [2, 2, 1, 4, 0, 0, 1, 25] and peak.tolist() == [0.64, -1.0]   # any positive score beats it
    assert not T.zncc_beats((F64(-1.0), 25, 0, 0), (F64(0.64), 4, 2, 2))


def test_oracle_equal_scores_fall_to_the_key():
    table = np.zeros((5, 5, 6), dtype=np.int64)
    m = (4, 10, 14, 30, 54, 39)                                                       # q = 0.64
    twice = (8, 20, 28, 60, 108, 78)                                                  # the same cells twice: c, va, vb * 4, q the same
    assert T.zncc_q(m) == T.zncc_q(twice)
    table[4, 2], table[0, 2] = m, twice                                               # (2, 0) and (-2, 0): dy = -2 < 2
    best, peak = T.zncc_pick_oracle(table, 2, 1)
    assert best.tolist() == [-2, 0, 1, 8, 2, 0, 1, 4] and peak[0] == peak[1]
    table[2, 3] = m                                                                   # (0, 1): d2 = 1 wins; (2, 0) then (-2, 0) are outside its 3 x 3
    best, peak = T.zncc_pick_oracle(table, 2, 1)
    assert best.tolist() == [0, 1, 1, 4, -2, 0, 1, 8]
    table[2, 3] = (4, 10, 14, 30, 54, 38)                                             # a lower score loses whatever its key
    best, peak = T.zncc_pick_oracle(table, 2, 1)
    assert best.tolist() == [-2, 0, 1, 8, 2, 0, 1, 4]


# ---- the exposure case: a scene with an illumination ramp, plane B under another gain and offset -------------------------

EXPO_TRUE = (2, -3)                                                                    # (dy, dx)
EXPO_S, EXPO_G = 4, 24


def _smooth(h, w, seed, amp):
    """A smooth field: uniform values on an 8-cell lattice, bilinearly interpolated, in [0, amp)."""
    rng = np.random.default_rng(seed)
    knots = rng.random((h // 8 + 2, w // 8 + 2)) * amp
    y, x = np.arange(h) / 8.0, np.arange(w) / 8.0
    j, i = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    fy, fx = (y - j)[:, None], (x - i)[None, :]
    return ((1 - fy) * (1 - fx) * knots[j][:, i] + (1 - fy) * fx * knots[j][:, i + 1] + fy * (1 - fx) * knots[j + 1][:, i] +
            fy * fx * knots[j + 1][:, i + 1])


def _exposure_planes():
    """A (G, G) and B (G + 2S, G + 2S) uint8: a smooth scene under a ramp of 3 grey levels per cell, A cut at the patch, B the
    scene seen (dy, dx) = EXPO_TRUE displaced and rendered as 0.5 * scene + 20."""
    S, G = EXPO_S, EXPO_G
    E = G + 2 * S
    big = _smooth(E + 2 * S, E + 2 * S, 7, 40.0) + 3.0 * np.arange(E + 2 * S)[None, :] + 20.0
    assert big.max() < 255
    dy, dx = EXPO_TRUE
    A = np.floor(big[2 * S:2 * S + G, 2 * S:2 * S + G]).astype(np.uint8)
    # B[j + S + dy][i + S + dx] shows A[j][i]'s ground: B[r][c] = big[r - dy + S][c - dx + S]
    B = np.floor(0.5 * np.floor(big[S - dy:S - dy + E, S - dx:S - dx + E]) + 20.0).astype(np.uint8)
    return A, B


def test_exposure_change_breaks_sad_and_not_zncc():
    A, B = _exposure_planes()
    S, G = EXPO_S, EXPO_G
    assert A.min() >= 1 and B.min() >= 1
    sad = T.pick_oracle(T.search_oracle(A, B, G, G, S), S, 1)
    assert tuple(sad[:2].tolist()) != EXPO_TRUE                                        # SAD's minimum has moved off the true shift
    best, peak = T.zncc_pick_oracle(T.zncc_search_oracle(A, B, G, G, S), S, 1)
    assert tuple(best[:2].tolist()) == EXPO_TRUE and best[2] == 1 and peak[0] > 0.99 and peak[1] < peak[0]
    # without the gain and the offset SAD finds it too: the fixture isolates the exposure
    same = np.floor(2.0 * (B.astype(F64) - 20.0)).astype(np.uint8)
    assert tuple(T.pick_oracle(T.search_oracle(A, same, G, G, S), S, 1)[:2].tolist()) == EXPO_TRUE


# ---- CPU: arguments ----------------------------------------------------------------------------------------------------

def _abi_zncc(n_pairs=3, search=4, side=64, min_cells=1, a=0x5001, b=0x6001, pairs=0x4000, moments=0x8000, best=0xa000, peak=0xb000):
    """wm_register_search_zncc with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_register_search_zncc(_p(a), _p(b), _p(pairs), n_pairs, search, side, min_cells, _p(moments), _p(best), _p(peak), None)


def test_zncc_abi_argument_errors_without_gpu():
    err = last_error
    assert _abi_zncc(n_pairs=-1) < 0 and "n_pairs" in err()
    assert _abi_zncc(n_pairs=N.REGISTER_MAX_PAIRS + 1) < 0 and "n_pairs" in err()
    assert _abi_zncc(search=-1) < 0 and "search" in err()
    assert _abi_zncc(search=N.REGISTER_MAX_SEARCH + 1) < 0 and "search" in err()
    assert _abi_zncc(side=0) < 0 and "side" in err()
    assert _abi_zncc(side=N.REGISTER_MAX_SIDE + 1) < 0 and "side" in err()
    assert _abi_zncc(pairs=0) < 0 and "pairs_dev" in err()
    assert _abi_zncc(pairs=0x4004) < 0 and "pairs_dev" in err() and "aligned" in err()
    assert _abi_zncc(a=0) < 0 and "a_dev" in err()
    assert _abi_zncc(b=0) < 0 and "b_dev" in err()
    for bad in (0, -1, -2 ** 31):
        assert _abi_zncc(min_cells=bad) < 0 and "min_cells" in err()
    assert _abi_zncc(moments=0) < 0 and "moments_dev" in err()
    assert _abi_zncc(best=0) < 0 and "best_dev" in err()
    assert _abi_zncc(peak=0) < 0 and "peak_dev" in err()
    for bad in (0x8001, 0x8002, 0x8004):
        assert _abi_zncc(moments=bad) < 0 and "moments_dev" in err() and "aligned" in err()
    for bad in (0xb001, 0xb002, 0xb004):
        assert _abi_zncc(peak=bad) < 0 and "peak_dev" in err() and "aligned" in err()
    assert _abi_zncc(best=0xa002) < 0 and "best_dev" in err() and "aligned" in err()
    # n_pairs == 0 returns 0 before looking at any pointer or any other argument
    assert _abi_zncc(n_pairs=0, pairs=0, a=0, b=0, moments=0, best=0, peak=0, search=-5, side=0, min_cells=0) == 0


def test_zncc_symbol_and_abi_13():
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey registration, correlation search" in header() and len(re.findall("13, additive", header())) >= 4
    assert entry_is_whole("wm_register_search_zncc")
    assert len(N.SYMBOLS["wm_register_search_zncc"][1]) == 11
    kern = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "register_kernels.h")).read()
    assert "__builtin_amdgcn_udot4(" in kern and "asm" not in kern


def test_register_metric_and_min_corr_errors_before_device_work():
    g = np.stack([T._north_up(0, 0, 100, 80), T._north_up(10, 10, 100, 80)])
    sizes = [(80, 100), (80, 100)]
    lazy = _Lazy([np.zeros((80, 100, 3), dtype=np.uint8)] * 2)
    for bad in ("ncc", "SAD", "", None, 1, b"zncc", ("zncc",)):
        with pytest.raises(ValueError, match="metric"):
            tiling.register(lazy, g, 1.0, sizes=sizes, metric=bad)
    for bad in (1.0, 1.5, -1.5, NAN, INF, -INF, "high", None, True):
        for metric in tiling.REGISTER_METRICS:
            with pytest.raises(ValueError, match="min_corr"):
                tiling.register(lazy, g, 1.0, sizes=sizes, metric=metric, min_corr=bad)
    with pytest.raises(ValueError, match="search"):                                   # the other arguments are still checked under zncc
        tiling.register(lazy, g, 1.0, sizes=sizes, metric="zncc", search=-1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device tensor"):                  # no CPU fallback
            tiling.register(lazy, g, 1.0, sizes=sizes, min_cells=1, metric="zncc", min_corr=-1.0)
    assert lazy.asked == []
    far = np.stack([T._north_up(0, 0, 100, 80), T._north_up(1000, 0, 100, 80)])           # no pair: no device, every key present
    for metric in tiling.REGISTER_METRICS:
        out = tiling.register(lazy, far, 1.0, sizes=sizes, metric=metric)
        assert out["corr"].shape == out["mean"].shape == out["accepted"].shape == (0,) and np.array_equal(out["georef"], far)
    assert lazy.asked == []


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _zncc(A, B, sizes, S, min_cells):
    """wm_register_search_zncc on hand-built planes: A a list of (side, side), B of (E, E) uint8, sizes a list of (gx, gy).
    Every output is pre-filled with a poison value.  Returns moments (P, 2S+1, 2S+1, 6) int64, best (P, 8) int64, peak (P, 2)."""
    side = A[0].shape[0]
    assert all(x.shape == (side, side) for x in A) and all(x.shape == (side + 2 * S, side + 2 * S) for x in B)
    table = T._pairs([(0, 1, gx, gy, 0.0, 0.0) for gx, gy in sizes])
    return T.device_search("zncc", T._up(np.stack(A)), T._up(np.stack(B)), table, S, side, min_cells)


def _check(A, B, sizes, S, min_cells, want=None):
    """Run the device search and require moments, best and peak of every pair to equal the oracle's.  Returns the oracle's
    (moments, best, peak) per pair; `want` passes moments that were computed before."""
    moments, best, peak = _zncc(A, B, sizes, S, min_cells)
    out = []
    for p, (gx, gy) in enumerate(sizes):
        mo = T.zncc_search_oracle(A[p], B[p], gx, gy, S) if want is None else want[p]
        wb, wp = T.zncc_pick_oracle(mo, S, min_cells)
        np.testing.assert_array_equal(moments[p], mo, err_msg=f"moments of pair {p}")
        np.testing.assert_array_equal(best[p], wb, err_msg=f"best of pair {p}")
        assert T.same_bytes(peak[p], wp), (p, peak[p], wp)
        out.append((mo, wb, wp))
    return out


def _shape_planes(name):
    """The planes of test_register's shape case `name`, by its render oracle: random content, both frames see everything."""
    gx, gy, S, side = T.SHAPES[name]
    case = T._shape_case(gx, gy, S, side, seed=sorted(T.SHAPES).index(name))
    pr = case["pairs"][0]
    A = T.render_plane(case["g2p"][0], case["size"][0], case["images"][0], pr["x0"], pr["y0"], case["cell"], gx, gy, 0, side)
    B = T.render_plane(case["g2p"][1], case["size"][1], case["images"][1], pr["x0"], pr["y0"], case["cell"], gx, gy, S, side + 2 * S)
    return A, B, gx, gy, S


# the SAD suite's shapes: tile edges in both axes, a 1-wide column, search 0, the 32-row to 16-row tile switch at search
# 62 / 63; by the launcher's rule K = 1 up to search 5, K = 2 at search 33, K = 4 at search 62, 63 and 64
ZNCC_SHAPES = ("1x1_s0", "1x1_s1_side4", "3x5_s1", "4x4_s5", "63x65_s5", "64x64_s1", "65x63_s5", "1x65_s5", "64x1_s0", "257x65_s5",
               "96x80_s64", "33x37_s62", "33x37_s63", "512x512_s4", "40x40_s33")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZNCC_SHAPES)
def test_gpu_zncc_smallest_shapes(name):
    A, B, gx, gy, S = _shape_planes(name)
    (mo, best, peak), = _check([A], [B], [(gx, gy)], S, 1)
    assert (mo[..., 0] == gx * gy).all()                                              # both frames see everything
    assert best[2] == (1 if gx * gy > 1 else 0)                                       # one cell has no variance


@pytest.mark.gpu
def test_gpu_zncc_hand_moments_and_ties():
    (mo, best, peak), = _check([T.HAND_A], [T.HAND_B], [(2, 2)], 1, 1)
    assert mo.tolist() == [[list(c) for c in row] for row in HAND_MOMENTS]
    assert best.tolist() == [0, 0, 1, 4, 0, 0, 0, 0] and peak[0] == 1.0 and np.isnan(peak[1])
    # B = 2 A + 7 at (1, -2): q == 1.0 exactly, on the device too
    rng = np.random.default_rng(2)
    A = rng.integers(1, 120, size=(6, 6), dtype=np.uint8)
    B = rng.integers(1, 256, size=(10, 10), dtype=np.uint8)
    B[3:9, 0:6] = 2 * A + 7
    (mo, best, peak), = _check([A], [B], [(6, 6)], 2, 1)
    assert best[:4].tolist() == [1, -2, 1, 36] and peak[0] == 1.0
    # the negative of A at (0, 0) scores -1 and is the last choice; a constant A has no eligible offset
    A = rng.integers(1, 200, size=(5, 5), dtype=np.uint8)
    B = np.zeros((9, 9), dtype=np.uint8)
    B[2:7, 2:7] = 255 - A
    flat = np.full((5, 5), 9, dtype=np.uint8)
    (mo, best, peak), (_, best_flat, peak_flat) = _check([A, flat], [B, B], [(5, 5), (5, 5)], 2, 25)
    assert best.tolist() == [0, 0, 1, 25, 0, 0, 0, 0] and peak[0] == -1.0             # only (0, 0) has 25 cells
    assert best_flat.tolist() == [0] * 8 and np.isnan(peak_flat).all()


@pytest.mark.gpu
def test_gpu_zncc_all_255_passes_2_to_the_32_and_has_no_variance():
    A, B = np.full((512, 512), 255, dtype=np.uint8), np.full((520, 520), 255, dtype=np.uint8)
    cell = (512 * 512, 255 * 512 * 512, 255 * 512 * 512, 255 * 255 * 512 * 512, 255 * 255 * 512 * 512, 255 * 255 * 512 * 512)
    assert cell[5] == 17045913600 > 2 ** 32
    want = np.broadcast_to(np.array(cell, dtype=np.int64), (9, 9, 6))                 # every offset sees every cell
    (mo, best, peak), = _check([A], [B], [(512, 512)], 4, 1, want=[want])
    assert best.tolist() == [0] * 8 and np.isnan(peak).all()                          # va = vb = 0 everywhere


@pytest.mark.gpu
def test_gpu_zncc_several_pairs_sprinkled_zeros_diagonal_mask_and_a_blind_frame():
    rng = np.random.default_rng(9)
    S, side = 5, 72
    E = side + 2 * S
    A = [np.where(rng.random((side, side)) < 0.2, 0, rng.integers(1, 256, size=(side, side))).astype(np.uint8) for _ in range(5)]
    B = [np.where(rng.random((E, E)) < 0.3, 0, rng.integers(1, 256, size=(E, E))).astype(np.uint8) for _ in range(5)]
    jj, ii = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    A[1][jj + ii < 60] = 0                                                            # a diagonal mask edge across the tiles
    JJ, II = np.meshgrid(np.arange(E), np.arange(E), indexing="ij")
    B[2][JJ > II + 7] = 0
    B[3][:] = 0                                                                       # a frame that sees nothing
    A[4][:, 1:] = 77                                                                  # beyond gx = 1: must not count
    sizes = [(70, 45), (72, 72), (5, 66), (33, 30), (1, 1)]                           # pairs of different sizes in one launch
    out = _check(A, B, sizes, S, 40)
    assert len(set(out[0][0][..., 0].reshape(-1).tolist())) > 1                       # B's mask moves n with the offset
    assert out[0][1][2] == 1 and out[0][1][6] == 1 and out[1][1][2] == 1 and out[2][1][2] == 1
    assert (out[3][0] == 0).all() and out[3][1].tolist() == [0] * 8 and np.isnan(out[3][2]).all()
    assert out[4][0][..., 0].max() <= 1 and out[4][1].tolist() == [0] * 8              # 1 cell < min_cells 40


@pytest.mark.gpu
def test_gpu_zncc_min_cells_boundary_on_a_hand_built_mask():
    rng = np.random.default_rng(5)
    A = np.zeros((70, 70), dtype=np.uint8)
    cells = rng.permutation(66 * 67)[:1234]
    A[cells // 66, cells % 66] = rng.integers(1, 256, size=1234)                      # gx = 66, gy = 67: exactly 1234 seen cells
    A[:, 66:] = 200                                                                   # beyond gx: must not count
    A[67:, :] = 200
    B = rng.integers(1, 256, size=(70, 70), dtype=np.uint8)                           # search 0: E = side; B sees everything
    want = T.zncc_search_oracle(A, B, 66, 67, 0)
    assert want[0, 0, 0] == 1234
    (_, best, peak), = _check([A], [B], [(66, 67)], 0, 1234, want=[want])
    assert best.tolist() == [0, 0, 1, 1234, 0, 0, 0, 0] and np.isfinite(peak[0])       # n == min_cells is eligible
    (_, best, peak), = _check([A], [B], [(66, 67)], 0, 1235, want=[want])
    assert best.tolist() == [0] * 8 and np.isnan(peak).all()                          # n == min_cells - 1 is not


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 2, 4))
def test_gpu_zncc_every_offsets_per_thread_instance(k, monkeypatch):
    """WM_REGISTER_K forces the instance (the launcher reads it per call); the result does not depend on it.  At search 5
    the 121 offsets leave most threads of a K = 4 block without one: they walk the last offset and drop it."""
    monkeypatch.setenv("WM_REGISTER_K", str(k))
    A, B = T.per_k_planes()
    _check([A], [B], [(70, 45)], 5, 300)


def _exposure_case():
    """The exposure planes as two frames: the scene is a ground raster of 40 x 40 cells of 1 m (row 0 south), frame A sees it
    through its true georeference, frame B -- rendered as 0.5 * scene + 20 -- through one displaced by (dx, dy) = (-3, 2)."""
    S, G = EXPO_S, EXPO_G
    E = G + 2 * S
    big = _smooth(E + 2 * S, E + 2 * S, 7, 40.0) + 3.0 * np.arange(E + 2 * S)[None, :] + 20.0
    grey = lambda v: np.repeat(np.flipud(v).astype(np.uint8)[:, :, None], 3, axis=2)  # luma of (v, v, v) is v; image row 0 is north
    dy, dx = EXPO_TRUE
    n = E + 2 * S
    fa = T._axis_frame(grey(np.floor(big)), 0.0, float(n), 1.0)
    fb = T._axis_frame(grey(np.floor(0.5 * np.floor(big) + 20.0)), float(dx), float(n + dy), 1.0)
    return T._case([fa, fb], [(0, 1, G, G, 2.0 * S, 2.0 * S)], 1.0, S, G, 1)


def test_exposure_case_renders_the_exposure_planes():
    case = _exposure_case()
    want = T._oracle(case)
    A, B = _exposure_planes()
    np.testing.assert_array_equal(want["a"][0], A)
    np.testing.assert_array_equal(want["b"][0], B)
    assert tuple(want["best"][0][:2].tolist()) != EXPO_TRUE


@pytest.mark.gpu
def test_gpu_exposure_pair_through_render_and_search():
    case = _exposure_case()
    want = T._oracle(case)
    a, b = T._planes(case)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    T._render(case, a, b, status, [0, 1])
    assert status.item() == 0
    A, B = a.cpu().numpy(), b.cpu().numpy()
    np.testing.assert_array_equal(A[0], want["a"][0])
    np.testing.assert_array_equal(B[0], want["b"][0])
    (_, best, peak), = _check([A[0]], [B[0]], [(EXPO_G, EXPO_G)], EXPO_S, 1)
    assert tuple(best[:2].tolist()) == EXPO_TRUE and best[2] == 1 and corr(peak[0]) > 0.99
    _, sad = T._search(case, a, b)                                                    # the SAD search on the same device planes
    np.testing.assert_array_equal(sad[0], want["best"][0])
    assert tuple(sad[0, :2].tolist()) != EXPO_TRUE


# ---- end to end --------------------------------------------------------------------------------------------------------

EXPOSURE = ((1.0, 0.0), (0.5, 20.0), (0.75, 40.0), (0.6, 5.0))                        # (gain, offset) of the four frames


def _exposure_survey():
    """test_register's four-frame survey on a grey scene with an illumination ramp (a smooth texture of 60 grey levels on a ramp
    of 0.3 per metre eastwards), every frame's pixels under a gain and an offset of its own: floor(g * scene + o)."""
    scene = np.floor(_smooth(T.SCENE_H, T.SCENE_W, 3, 60.0) + 0.3 * np.arange(T.SCENE_W)[None, :] + 10.0)
    assert 1 <= scene.min() and scene.max() < 255
    true = np.stack([tiling.nadir_affine(160, 200, c, 1.0, yaw) for c, yaw in
                     (((200.0, 200.0), 0.0), ((280.0, 220.0), 0.0), ((240.0, 170.0), 180.0), ((250.0, 210.0), 90.0))])
    yy, xx = np.meshgrid(np.arange(160) + 0.5, np.arange(200) + 0.5, indexing="ij")
    frames = []
    for g, (gain, off) in zip(true, EXPOSURE):
        X = g[0, 0] * xx + g[0, 1] * yy + g[0, 2]
        Y = g[1, 0] * xx + g[1, 1] * yy + g[1, 2]
        v = np.floor(gain * scene[T.SCENE_H - 1 - np.floor(Y).astype(np.int64), np.floor(X).astype(np.int64)] + off)
        frames.append(np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2))
    displaced = true.copy()
    displaced[:, 0, 2] += T.DISPLACED[:, 0]
    displaced[:, 1, 2] += T.DISPLACED[:, 1]
    return frames, true, displaced


E2E = dict(search=8, side=256, min_cells=4096)


def _e2e_oracles():
    """Per pair of the exposure survey: the SAD oracle's best (8,) and the correlation oracle's (best, peak)."""
    frames, true, displaced = _exposure_survey()
    sizes = np.array([(160, 200)] * 4, dtype=np.int32)
    S, side, mc = E2E["search"], E2E["side"], E2E["min_cells"]
    pairs = tiling.register_pairs(displaced, sizes, 1.0, S, side, mc)
    g2p = tiling.ground_to_pixel(displaced).reshape(-1, 6)
    out = []
    for pr in pairs:
        fa, fb, gx, gy = (int(pr[k]) for k in ("frame_a", "frame_b", "gx", "gy"))
        A = T.render_plane(g2p[fa], sizes[fa], frames[fa], pr["x0"], pr["y0"], 1.0, gx, gy, 0, side)
        B = T.render_plane(g2p[fb], sizes[fb], frames[fb], pr["x0"], pr["y0"], 1.0, gx, gy, S, side + 2 * S)
        out.append((T.pick_oracle(T.search_oracle(A, B, gx, gy, S), S, mc), T.zncc_pick_oracle(T.zncc_search_oracle(A, B, gx, gy, S), S, mc)))
    return pairs, out


def test_exposure_survey_by_the_oracles():
    """What the two rules do on the exposure survey, decided on the host: the correlation finds every pair's whole-cell
    displacement with a confident peak; SAD finds none of them, and its runner-up is within 10 % of its peak on every pair,
    so register() rejects all six at the default min_ratio: wrong shifts that are then rejected."""
    pairs, out = _e2e_oracles()
    assert len(pairs) == 6
    for pr, (sad, (best, peak)) in zip(pairs, out):
        a, b = int(pr["frame_a"]), int(pr["frame_b"])
        dx, dy = (T.DISPLACED[b] - T.DISPLACED[a]).astype(np.int64)
        assert best[:3].tolist() == [dy, dx, 1] and best[6] == 1
        r = corr(peak)
        assert r[0] > 0.999 and (1.0 - r[1]) >= 1.25 * (1.0 - r[0])
        assert sad[:2].tolist() != [dy, dx] and sad[2] > 0 and sad[6] > 0
        assert sad[6] / sad[7] < 1.25 * (sad[2] / sad[3])


@pytest.mark.gpu
def test_gpu_register_zncc_end_to_end_corrects_the_census_where_sad_does_not():
    frames, true, displaced = _exposure_survey()
    pairs, oracles = _e2e_oracles()
    out = tiling.register(frames, displaced, 1.0, metric="zncc", **E2E)
    ab = [(int(p["frame_a"]), int(p["frame_b"])) for p in out["pairs"]]
    assert ab == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    want = np.array([T.DISPLACED[b] - T.DISPLACED[a] for a, b in ab], dtype=np.int64)
    np.testing.assert_array_equal(out["offset"], want)
    assert out["accepted"].all() and (out["corr"] > 0.999).all() and (out["cells"] >= 4096).all()
    for p, (_, (best, peak)) in enumerate(oracles):                                   # the device's pick is the oracle's
        assert out["offset"][p].tolist() == [best[1], best[0]] and out["cells"][p] == best[3]
        r = corr(peak)
        assert out["corr"][p] == r[0] and out["mean"][p] == 1.0 - r[0] and out["runner_up"][p] == 1.0 - r[1]
    assert np.abs(out["shift"] + T.DISPLACED).max() < 1e-9
    assert np.abs(out["georef"] - true).max() < 1e-9 and np.abs(out["residual"]).max() < 1e-9
    assert out["component"].tolist() == [0, 0, 0, 0]
    dets = T._detections(true)
    assert tiling.census(dets, out["georef"], 1.5)["count"] == len(T.ANIMALS) == 12
    # SAD on the same frames: the oracle's wrong shifts, every pair rejected, the georeferences left displaced
    sad = tiling.register(frames, displaced, 1.0, **E2E)
    assert np.isnan(sad["corr"]).all() and sorted(sad) == sorted(out)
    for p, (best, _) in enumerate(oracles):
        assert sad["offset"][p].tolist() == [best[1], best[0]] and sad["offset"][p].tolist() != want[p].tolist()
    assert not sad["accepted"].any() and np.array_equal(sad["georef"], displaced)
    assert tiling.census(dets, sad["georef"], 1.5)["count"] > len(T.ANIMALS)
    # chunks of two pairs: the same result under zncc
    again = tiling.register(frames, displaced, 1.0, metric="zncc", pair_chunk=2, **E2E)
    for key in out:
        np.testing.assert_array_equal(again[key], out[key], err_msg=key)
    # min_corr is a gate of its own: above every pair's r nothing is accepted
    none = tiling.register(frames, displaced, 1.0, metric="zncc", min_corr=0.99999, **E2E)
    assert not none["accepted"].any() and np.array_equal(none["offset"], out["offset"])
