"""Survey coverage (include/wm_hip.h "Survey coverage", tiling.coverage): the ground a survey saw, its gaps, and the
census' individuals per cell.  The rule has no reference behaviour; coverage_oracle (tests/ground_oracle.py) restates it
sequentially -- one cell and one point at a time, numpy float64, the header's operation order -- and the device result must
equal it exactly: everything is an integer, so every comparison is assert_array_equal and there is no tolerance anywhere."""
import functools
import math

import numpy as np
import pytest
import torch

from ground_cases import (FRAME_A, FRAME_B, FRAME_SWEEP, GRID_SWEEP, INF, NAN, ORIGIN_CELL_SWEEP, _case, _geometries, _p, entry_is_whole, header,
                          last_error, macro)
from ground_oracle import coverage_oracle, coverage_oracle_by_frame
from survey_util import _axis, _kernel_constants, _some_frames, _yawed, _yawed_90
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling


def _oracle(case):
    return coverage_oracle(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"], case["points"], case["labels"])


# name -> (case, expected coverage rows from j = 0 (south) upwards, expected stats[0:3])
def _hand_cases():
    cases = {}
    one = [[1, 1, 1, 1, 0], [1, 1, 1, 1, 0], [0, 0, 0, 0, 0]]
    cases["one_frame"] = (_case([FRAME_A], 0, 0, 1, 5, 3), one, [7, 8, 0])
    # centres at multiples of 0.5: X = 0 has u == 0 (inside), X = 4 has u == 8 (outside); Y = 0 has v == 4 (outside), Y = 2 has v == 0
    row = [1] * 8 + [0]
    cases["half_open_edges"] = (_case([FRAME_A], -0.25, -0.25, 0.5, 9, 6), [[0] * 9, row, row, row, row, [0] * 9], [22, 32, 0])
    two = [1, 1, 2, 2, 1, 1, 0]
    cases["two_frames_half_overlap"] = (_case([FRAME_A, FRAME_B], 0, 0, 1, 7, 3), [two, two, [0] * 7], [9, 8, 4])
    cases["nan_coefficient"] = (_case([FRAME_A, ([2, NAN, 0, 0, -2, 4], 4, 8)], 0, 0, 1, 5, 3), one, [7, 8, 0])
    cases["inf_coefficient"] = (_case([([2, 0, 0, 0, -2, INF], 4, 8), FRAME_A], 0, 0, 1, 5, 3), one, [7, 8, 0])
    cases["height_zero"] = (_case([([2, 0, 0, 0, -2, 4], 0, 8), FRAME_A, ([2, 0, 0, 0, -2, 4], 4, -3)], 0, 0, 1, 5, 3), one, [7, 8, 0])
    side = [0, 1, 1, 0]
    cases["yawed_90"] = (_case([_yawed_90()], 8, 17, 1, 4, 6), [[0] * 4, side, side, side, side, [0] * 4], [16, 8, 0])
    return cases


HAND = _hand_cases()

# on a cell border (the higher cell), at X == x0 (cell 0), just outside the grid on either side, not finite, bad labels
HAND_POINTS = _case([FRAME_A], 0, 0, 1, 5, 3,
                    points=[(2.0, 0.5), (0.0, 1.0), (5.0, 0.5), (-1e-9, 0.5), (NAN, 1.0), (INF, 1.0), (1.5, 1.5), (1.5, 0.5), (4.5, 2.5), (1.0, -INF)],
                    labels=[0, 3, 1, 1, 2, 2, 7, -1, 6, 0])
HAND_POINTS_WANT = {"seen_by": [1, 1, 0, 0, 0, 0, 1, 1, 0, 0],
                    "cell": [(0, 2), (1, 0), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (2, 4), (-1, -1)],
                    "pstats": [3, 7], "counts_at": [(0, 0, 2), (3, 1, 0), (6, 2, 4)]}


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_hand_cases(name):
    case, rows, stats = HAND[name]
    got = _oracle(case)
    assert got["coverage"].tolist() == rows
    assert got["stats"].tolist() == stats + [0] * 13
    assert got["stats"].sum() == case["gx"] * case["gy"]
    by_frame = coverage_oracle_by_frame(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"])
    np.testing.assert_array_equal(by_frame["coverage"], got["coverage"])
    np.testing.assert_array_equal(by_frame["stats"], got["stats"])


def test_oracle_one_frame_area_is_the_footprints():
    for name, area in (("one_frame", 8.0), ("half_open_edges", 8.0), ("yawed_90", 8.0), ("two_frames_half_overlap", 12.0)):
        case, _, _ = HAND[name]
        got = _oracle(case)
        assert (case["gx"] * case["gy"] - got["stats"][0]) * case["cell"] * case["cell"] == area


def test_oracle_hand_points():
    got = _oracle(HAND_POINTS)
    assert got["seen_by"].tolist() == HAND_POINTS_WANT["seen_by"]
    assert [tuple(c) for c in got["cell"].tolist()] == HAND_POINTS_WANT["cell"]
    assert got["pstats"].tolist() == HAND_POINTS_WANT["pstats"]
    want = np.zeros((7, 3, 5), dtype=np.int64)
    for at in HAND_POINTS_WANT["counts_at"]:
        want[at] = 1
    np.testing.assert_array_equal(got["counts"], want)


def test_oracle_stats_saturate_at_15():
    got = _oracle(_case([FRAME_A] * 14 + [FRAME_B] * 3, 0, 0, 1, 7, 3))
    assert got["coverage"][0].tolist() == [14, 14, 17, 17, 3, 3, 0]
    assert got["stats"][[0, 3, 14, 15]].tolist() == [9, 4, 4, 4] and got["stats"].sum() == 21


def test_ground_to_pixel_inverts_nadir_affine():
    H, W, E, Nn, gsd = 4000, 6000, 500000.0 + 123.4, 6000000.0 + 567.8, 0.025
    px = np.array([[0.0, 0.0], [W, 0.0], [0.0, H], [W, H], [1234.5, 3210.25], [W / 2, H / 2]])
    for yaw in (0.0, 37.0, 90.0, 180.0):
        a = tiling.nadir_affine(H, W, (E, Nn), gsd, yaw)
        b = tiling.ground_to_pixel(a)
        assert b.shape == (2, 3) and b.dtype == np.float64
        ground = px @ a[:, :2].T + a[:, 2]
        back = ground @ b[:, :2].T + b[:, 2]
        assert np.abs(back - px).max() < 1e-6, (yaw, np.abs(back - px).max())
        # the stated operation order, bit for bit
        det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
        b0, b1, b3, b4 = a[1, 1] / det, -a[0, 1] / det, -a[1, 0] / det, a[0, 0] / det
        want = np.array([[b0, b1, -(b0 * a[0, 2] + b1 * a[1, 2])], [b3, b4, -(b3 * a[0, 2] + b4 * a[1, 2])]])
        np.testing.assert_array_equal(b.view(np.int64), want.view(np.int64))
    stack = tiling.ground_to_pixel(np.stack([tiling.nadir_affine(H, W, (E, Nn), gsd, y) for y in (0.0, 37.0)]))
    assert stack.shape == (2, 2, 3)
    np.testing.assert_array_equal(stack[1], tiling.ground_to_pixel(tiling.nadir_affine(H, W, (E, Nn), gsd, 37.0)))


def test_ground_to_pixel_singular_or_not_finite_is_nan():
    good = [[0.5, 0.0, 0.0], [0.0, -0.5, 2.0]]
    g = np.array([[[1.0, 2.0, 5.0], [2.0, 4.0, 7.0]], good, [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[0.5, NAN, 0.0], [0.0, -0.5, 2.0]],
                  [[0.5, 0.0, INF], [0.0, -0.5, 2.0]]])
    b = tiling.ground_to_pixel(g)
    assert np.isnan(b[[0, 2, 3, 4]]).all()
    np.testing.assert_array_equal(b[1], [[2.0, 0.0, 0.0], [0.0, -2.0, 4.0]])      # frame A
    with pytest.raises(ValueError, match="georef"):
        tiling.ground_to_pixel(np.zeros((2, 3, 2)))


def test_footprint_bounds():
    sizes = [(4, 8)]
    assert tiling.footprint_bounds([[[0.5, 0, 0.3], [0, -0.5, 2.3]]], sizes, 0.5) == (0.0, 0.0, 9, 5)        # X 0.3..4.3, Y 0.3..2.3
    x0, y0, gx, gy = tiling.footprint_bounds([[[0.5, 0, -0.3], [0, -0.5, 1.9]]], sizes, 0.5)                # X -0.3..3.7, Y -0.1..1.9
    assert (x0, y0, gx, gy) == (-0.5, -0.5, 9, 5)
    x0, y0, gx, gy = tiling.footprint_bounds([[[0.5, 0, 500000.3], [0, -0.5, 6000002.3]]], sizes, 0.3)
    assert x0 == math.floor(500000.3 / 0.3) * 0.3 and y0 == math.floor(6000000.3 / 0.3) * 0.3
    assert x0 <= 500000.3 < x0 + 0.3 and x0 + gx * 0.3 >= 500004.3 and y0 + gy * 0.3 >= 6000002.3
    # two flights of one area: the grids line up (origins a whole number of cells apart)
    xa = tiling.footprint_bounds([tiling.nadir_affine(4000, 6000, (500100.0, 6000100.0), 0.025, 12.0)], [(4000, 6000)], 0.5)
    xb = tiling.footprint_bounds([tiling.nadir_affine(4000, 6000, (500131.7, 6000077.2), 0.025, 47.0)], [(4000, 6000)], 0.5)
    assert ((xa[0] - xb[0]) / 0.5).is_integer() and ((xa[1] - xb[1]) / 0.5).is_integer()
    assert tiling.footprint_bounds([[[0.5, 0, 0.3], [0, -0.5, 2.3]]], sizes, 100.0) == (0.0, 0.0, 1, 1)      # gx, gy >= 1
    assert tiling.footprint_bounds([], [], 1.0) == (0.0, 0.0, 1, 1)
    assert tiling.footprint_bounds([[[0.5, NAN, 0.3], [0, -0.5, 2.3]]], sizes, 1.0) == (0.0, 0.0, 1, 1)       # no finite frame
    # a frame that is not finite or has no pixels does not widen the extent
    both = tiling.footprint_bounds([[[0.5, 0, 0.3], [0, -0.5, 2.3]], [[0.5, 0, INF], [0, -0.5, 2.3]], [[0.5, 0, 99.0], [0, -0.5, 99.0]]],
                                   [(4, 8), (4, 8), (0, 8)], 0.5)
    assert both == (0.0, 0.0, 9, 5)
    with pytest.raises(ValueError, match="larger cell"):
        tiling.footprint_bounds([[[0.5, 0, 0.3], [0, -0.5, 2.3]]], sizes, 1e-4)                              # 43 000 cells a side
    with pytest.raises(ValueError, match="cell"):
        tiling.footprint_bounds([[[0.5, 0, 0.3], [0, -0.5, 2.3]]], sizes, 0.0)


def test_coverage_python_argument_errors_before_device_work():
    g = [[[0.5, 0, 0.0], [0, -0.5, 2.0]]] * 2
    sizes = [(4, 8), (4, 8)]
    for bad in (0, 0.0, -1.0, NAN, INF, "wide", None):
        with pytest.raises(ValueError, match="cell"):
            tiling.coverage(g, sizes, bad)
    with pytest.raises(ValueError, match="georef"):
        tiling.coverage(np.zeros((2, 3, 2)), sizes, 1.0)
    for bad in ([(4, 8, 1), (4, 8, 1)], [4, 8], [(4.5, 8), (4, 8)], "sizes"):
        with pytest.raises(ValueError, match="sizes"):
            tiling.coverage(g, bad, 1.0)
    with pytest.raises(ValueError, match="sizes for 2 georeferences"):
        tiling.coverage(g, [(4, 8)], 1.0)
    for bad in ((0.0, 0.0, N.COVERAGE_MAX_SIDE + 1, 1), (0.0, 0.0, 1, N.COVERAGE_MAX_SIDE + 1), (0.0, 0.0, 16384, 8192)):
        with pytest.raises(ValueError, match="larger cell"):
            tiling.coverage(g, sizes, 1.0, bounds=bad)
    for bad in ((0.0, 0.0, 0, 1), (0.0, 0.0, 5, -1), (NAN, 0.0, 5, 5), (0.0, INF, 5, 5), (0.0, 0.0, 5.5, 5), (0.0, 0.0, 5), "grid"):
        with pytest.raises(ValueError, match="bounds"):
            tiling.coverage(g, sizes, 1.0, bounds=bad)
    k = 3
    cen = {"points": torch.zeros((k, 2), dtype=torch.float64), "labels": torch.zeros(k, dtype=torch.int64),
           "members": torch.ones(k, dtype=torch.int64)}
    for drop in ("points", "labels", "members"):
        with pytest.raises(ValueError, match="'points'"):
            tiling.coverage(g, sizes, 1.0, census={key: v for key, v in cen.items() if key != drop})
    with pytest.raises(ValueError, match="census"):
        tiling.coverage(g, sizes, 1.0, census=dict(cen, points=torch.zeros((k, 2))))                           # float32 points
    with pytest.raises(ValueError, match="census"):
        tiling.coverage(g, sizes, 1.0, census=dict(cen, labels=torch.zeros(k + 1, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="ROCm device tensor"):          # no CPU fallback
        tiling.coverage(g, sizes, 1.0, census=cen)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device tensor"):
            tiling.coverage(g, sizes, 1.0)


def _abi_raster(n_frames=2, x0=0.0, y0=0.0, cell=1.0, gx=5, gy=3, g2p=0x2000, size=0x3000, cov=0x4000, stats=0x5000):
    """wm_coverage_raster with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_coverage_raster(_p(g2p), _p(size), n_frames, x0, y0, cell, gx, gy, _p(cov), _p(stats), None)


def _abi_points(n_points=4, n_frames=2, x0=0.0, y0=0.0, cell=1.0, gx=5, gy=3, g2p=0x2000, size=0x3000, pts=0x4000, labels=0x5000,
                seen=0x6000, cidx=0x7000, counts=0x8000, pstats=0x9000):
    return N.lib().wm_coverage_points(_p(g2p), _p(size), n_frames, _p(pts), _p(labels), n_points, x0, y0, cell, gx, gy, _p(seen), _p(cidx),
                                      _p(counts), _p(pstats), None)


def test_coverage_abi_argument_errors_without_gpu():
    err = last_error
    for call in (_abi_raster, _abi_points):
        for kwargs, word in GRID_SWEEP + FRAME_SWEEP + ORIGIN_CELL_SWEEP:
            assert call(**kwargs) < 0 and word in err(), (call.__name__, kwargs, word, err())
    assert _abi_raster(cov=0) < 0 and "coverage_dev" in err()
    assert _abi_raster(stats=0) < 0 and "stats_dev" in err()
    assert _abi_raster(cov=0x4001) < 0 and "aligned" in err()
    assert _abi_raster(stats=0x5004) < 0 and "aligned" in err()
    for name in ("pts", "labels", "seen", "cidx", "pstats"):
        assert _abi_points(**{name: 0}) < 0 and "null" in err()
    assert _abi_points(pts=0x4004) < 0 and "aligned" in err()
    assert _abi_points(counts=0x8002) < 0 and "aligned" in err()
    assert _abi_points(n_points=-1) < 0 and "n_points" in err()
    assert _abi_points(n_points=N.CENSUS_MAX_DETS + 1) < 0 and "n_points" in err()
    # n_points == 0 returns 0 before looking at any pointer or argument
    assert N.lib().wm_coverage_points(None, None, -5, None, None, 0, NAN, NAN, -1.0, 0, 0, None, None, None, None, None) == 0


def test_coverage_symbols_and_abi_13():
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey coverage" in header() and "13, additive" in header()
    for name in ("wm_coverage_raster", "wm_coverage_points"):
        assert entry_is_whole(name), name
    for name, val in (("WM_COVERAGE_MAX_SIDE", N.COVERAGE_MAX_SIDE), ("WM_COVERAGE_MAX_CELLS", N.COVERAGE_MAX_CELLS),
                      ("WM_COVERAGE_MAX_FRAMES", N.COVERAGE_MAX_FRAMES), ("WM_COVERAGE_CLASSES", N.COVERAGE_CLASSES),
                      ("WM_COVERAGE_STATS", N.COVERAGE_STATS)):
        assert macro(name) == val, name
    assert (N.COVERAGE_MAX_SIDE, N.COVERAGE_MAX_CELLS, N.COVERAGE_MAX_FRAMES) == (16384, 2 ** 26, 65535)
    assert tiling.COVERAGE_MAX_CELLS == 2 ** 26 and tiling.CENSUS_CLASSES == N.COVERAGE_CLASSES
    k = _kernel_constants()
    assert k["chunk"] >= 64 and k["block_x"] == 64 and k["block_y"] >= 4


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _device_abi(case, with_counts=True):
    """wm_coverage_raster and, with points, wm_coverage_points through the C-ABI, every output pre-filled with a poison value."""
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    g = up(case["g2p"]) if F else None
    s = up(case["size"]) if F else None
    lib = N.lib()
    cov = torch.full((gy, gx), 0x7777, device=dev, dtype=torch.int16)
    stats = torch.full((16,), -7, device=dev, dtype=torch.int64)
    N.check(lib.wm_coverage_raster(N.ptr(g), N.ptr(s), F, case["x0"], case["y0"], case["cell"], gx, gy, N.ptr(cov), N.ptr(stats),
                                   N.stream_ptr(dev)))
    out = {"coverage": cov.cpu().numpy().view(np.uint16).astype(np.int64), "stats": stats.cpu().numpy()}
    if case["points"] is None:
        return out
    P = case["points"].shape[0]
    pts, labels = up(case["points"]), up(case["labels"])
    seen = torch.full((P,), -7, device=dev, dtype=torch.int32)
    cidx = torch.full((P, 2), -7, device=dev, dtype=torch.int32)
    counts = torch.full((7, gy, gx), -7, device=dev, dtype=torch.int32) if with_counts else None
    pstats = torch.full((2,), -7, device=dev, dtype=torch.int64)
    N.check(lib.wm_coverage_points(N.ptr(g), N.ptr(s), F, N.ptr(pts), N.ptr(labels), P, case["x0"], case["y0"], case["cell"], gx, gy,
                                   N.ptr(seen), N.ptr(cidx), N.ptr(counts), N.ptr(pstats), N.stream_ptr(dev)))
    out.update({"seen_by": seen.cpu().numpy().astype(np.int64), "cell": cidx.cpu().numpy().astype(np.int64), "pstats": pstats.cpu().numpy()})
    if with_counts:
        out["counts"] = counts.cpu().numpy().astype(np.int64)
    return out


def _assert_same(got, want, keys=None):
    for key in keys or got:
        assert got[key].shape == want[key].shape, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def _run_and_check(case, want=None):
    want = _oracle(case) if want is None else want
    got = _device_abi(case)
    assert set(got) == set(want)
    _assert_same(got, want)
    assert got["stats"].sum() == case["gx"] * case["gy"]
    _assert_same(_device_abi(case), got)                                           # determinism
    return got, want


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    """name -> (case, oracle result), computed once."""
    k = _kernel_constants()
    if name in _geometries():
        frames, grid = _geometries()[name]
        case = _case(frames, *grid)
    elif name.startswith("grid_"):                                                # grid_<gx>x<gy>: none a multiple of the block
        gx, gy = (int(v) for v in name[5:].split("x"))
        case = _case(_some_frames(gx, gy, 0.7, gx) + [_axis(-1.0, gx * 0.7 / 2, -1.0, gy, 4.0)], 0.0, 0.0, 0.7, gx, gy)
    elif name == "one_frame":
        case = _case(_some_frames(70, 19, 0.7, 1, n=1), 0.0, 0.0, 0.7, 70, 19)
    elif name == "past_one_chunk":
        # the first COV_CHUNK frames see nothing of the grid (far away, not finite, without pixels); the three after them do
        far = [_yawed((5000.0 + 40 * f, -3000.0), 0.1, 7.0 * f, 300, 400) for f in range(k["chunk"])]
        far[3] = ([2, NAN, 0, 0, -2, 4], 4, 8)
        far[100] = _axis(0.0, 49.0, 0.0, 13.0, 4.0)[:1] + (0, 196)
        near = [_yawed((20.0, 6.0), 0.05, 30.0, 300, 400), _axis(10.0, 30.0, 2.0, 9.0, 4.0), _yawed((40.0, 10.0), 0.04, 115.0, 300, 400)]
        case = _case(far + near, 0.0, 0.0, 0.7, 70, 19)
    elif name == "cover_all":
        case = _case([_axis(-10.0, 300.0, -10.0, 100.0, 2.0), _yawed((128.0, 32.0), 0.5, 45.0, 1200, 1200)], 0.0, 0.0, 1.0, 257, 65)
    elif name == "random_survey":
        rng = np.random.default_rng(11)
        x0, y0, cell, gx, gy = 500000.1, 6000000.7, 0.3, 300, 200
        frames = [_yawed((x0 + rng.uniform(-5, 95), y0 + rng.uniform(-5, 65)), 0.05, rng.uniform(0, 360), 400, 600) for _ in range(60)]
        P = 3000
        pts = np.stack([x0 + rng.uniform(-6, 96, P), y0 + rng.uniform(-6, 66, P)], axis=1)
        pts[::97, 0] = NAN
        pts[5::131, 1] = INF
        pts[7::211] = -INF
        pts[11::50] = (x0 + 0.3 * rng.integers(0, 300, len(pts[11::50])))[:, None] * [1, 0] + [0, y0 + 10.0]      # X on a cell border
        labels = rng.integers(-1, 8, P)
        case = _case(frames, x0, y0, cell, gx, gy, points=pts, labels=labels)
    else:
        raise KeyError(name)
    return case, _oracle(case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_cases(name):
    case, rows, stats = HAND[name]
    got, _ = _run_and_check(case)
    assert got["coverage"].tolist() == rows and got["stats"].tolist() == stats + [0] * 13


@pytest.mark.gpu
def test_gpu_hand_points():
    got, _ = _run_and_check(HAND_POINTS)
    assert got["seen_by"].tolist() == HAND_POINTS_WANT["seen_by"]
    assert [tuple(c) for c in got["cell"].tolist()] == HAND_POINTS_WANT["cell"]
    assert got["pstats"].tolist() == HAND_POINTS_WANT["pstats"]
    assert sorted(zip(*(v.tolist() for v in np.nonzero(got["counts"])))) == HAND_POINTS_WANT["counts_at"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_1x1", "grid_70x19", "grid_257x65", "no_frames", "one_frame", "past_one_chunk"])
def test_gpu_smallest_shapes(name):
    case, want = _gpu_case(name)
    got, _ = _run_and_check(case, want)
    if name == "no_frames":
        assert not got["coverage"].any() and got["stats"][0] == 70 * 19
    if name == "past_one_chunk":
        assert case["g2p"].shape[0] == _kernel_constants()["chunk"] + 3
        first = dict(case, g2p=case["g2p"][:-3], size=case["size"][:-3])
        assert not _oracle(first)["coverage"].any()                              # only the frames past the first chunk cover anything
        assert (want["coverage"] == 2).any() and want["stats"][0] > 0
    if name.startswith("grid_") and name != "grid_1x1":
        assert want["stats"][0] > 0 and (want["coverage"] >= 2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cull_tiny_frame", "cull_thin_between_rows", "cull_thin_on_one_row", "cull_yaw_45", "cover_all", "block_edges"])
def test_gpu_aimed_at_the_cull(name):
    case, want = _gpu_case(name)
    got, _ = _run_and_check(case, want)
    cov = got["coverage"]
    k = _kernel_constants()
    bx, by = k["block_x"], k["block_y"]
    if name == "cull_tiny_frame":
        assert cov.sum() == 1 and cov[40, 100] == 1
    elif name == "cull_thin_between_rows":
        assert cov.sum() == 0
    elif name == "cull_thin_on_one_row":
        assert cov.sum() == 257 and (cov[40] == 1).all()
    elif name == "cull_yaw_45":
        # the strips cross blocks in which they cover no centre: more blocks touched by their bounding boxes than hold a covered cell
        assert 0 < cov.sum() < 1200
        blocks = {(j // by, i // bx) for j, i in zip(*np.nonzero(cov))}
        assert 2 <= len(blocks) < ((257 + bx - 1) // bx) * ((65 + by - 1) // by)
    elif name == "cover_all":
        assert (cov == 2).all() and got["stats"][2] == 257 * 65
    elif name == "block_edges":
        want_cov = np.zeros((65, 257), dtype=np.int64)
        want_cov[by:2 * by, bx:2 * bx] += 1
        want_cov[0:by, 0:bx] += 1
        want_cov[by:2 * by, 2 * bx:4 * bx] += 1
        want_cov[by - 1:by + 1, bx - 1:bx + 1] += 1
        np.testing.assert_array_equal(cov, want_cov)


@pytest.mark.gpu
def test_gpu_random_survey():
    case, want = _gpu_case("random_survey")
    got, _ = _run_and_check(case, want)
    assert want["stats"][0] > 0 and (want["coverage"] >= 4).any()                  # gaps and overlaps
    assert 0 < want["pstats"][0] < 3000 and (want["seen_by"] >= 2).any() and (want["seen_by"] == 0).any()
    assert want["counts"].sum() == want["pstats"][0] and want["pstats"].sum() == 3000
    by_frame = coverage_oracle_by_frame(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"])
    np.testing.assert_array_equal(by_frame["coverage"], want["coverage"])


@pytest.mark.gpu
def test_gpu_counts_null():
    case, want = _gpu_case("random_survey")
    got = _device_abi(case, with_counts=False)
    assert "counts" not in got
    _assert_same(got, want, keys=("coverage", "stats", "seen_by", "cell", "pstats"))


def _python_case():
    """Pixel -> ground georeferences for tiling.coverage, their exact inverses as the oracle's g2p, and a census-like dict."""
    rng = np.random.default_rng(23)
    E0, N0 = 500000.0, 6000000.0
    specs = [((E0 + 10.0 + 9.0 * f, N0 + 12.0 + 2.0 * (f % 3)), 0.05, 10.0 * f, 400, 600) for f in range(6)]
    georef = np.stack([tiling.nadir_affine(H, W, c, gsd, yaw) for c, gsd, yaw, H, W in specs])
    sizes = np.array([(H, W) for *_, H, W in specs], dtype=np.int32)
    k = 400
    pts = np.stack([E0 + rng.uniform(-10, 90, k), N0 + rng.uniform(-10, 40, k)], axis=1)
    pts[3] = NAN
    labels = rng.integers(0, 8, k)
    members = rng.integers(1, 4, k)
    return georef, sizes, pts, labels, members


KEYS = {"coverage", "origin", "cell", "shape", "multiplicity", "area_m2", "gap_cells"}
CENSUS_KEYS = {"seen_by", "cell_index", "counts", "class_counts", "density_per_km2", "detection_rate"}


@pytest.mark.gpu
def test_gpu_python_coverage():
    dev = torch.device("cuda:0")
    georef, sizes, pts, labels, members = _python_case()
    cell = 0.3
    x0, y0, gx, gy = tiling.footprint_bounds(georef, sizes, cell)
    g2p = tiling.ground_to_pixel(georef)
    want = coverage_oracle(g2p, sizes, x0, y0, cell, gx, gy, pts, labels)
    out = tiling.coverage(georef, sizes, cell)
    assert set(out) == KEYS
    assert out["coverage"].dtype == torch.int32 and out["coverage"].device.type == "cuda" and tuple(out["coverage"].shape) == (gy, gx)
    np.testing.assert_array_equal(out["coverage"].cpu().numpy(), want["coverage"])
    np.testing.assert_array_equal(out["coverage"].flip(0).cpu().numpy(), want["coverage"][::-1])              # the north-up picture
    assert out["multiplicity"].dtype == torch.int64
    np.testing.assert_array_equal(out["multiplicity"].cpu().numpy(), want["stats"])
    assert out["origin"] == (x0, y0) and out["cell"] == cell and out["shape"] == (gy, gx)
    assert out["gap_cells"] == int(want["stats"][0]) and isinstance(out["gap_cells"], int) and out["gap_cells"] > 0
    area = float((gx * gy - int(want["stats"][0])) * cell * cell)
    assert out["area_m2"] == area and isinstance(out["area_m2"], float)
    # the union, not the sum: six frames of 600 m^2 overlap
    assert 600.0 < area < 6 * 600.0 * 0.9

    cen = {"points": torch.from_numpy(pts).to(dev), "labels": torch.from_numpy(labels).to(dev), "members": torch.from_numpy(members).to(dev),
           "count": len(pts)}
    bounds = (x0 - 3 * cell, y0, gx + 1, gy - 7)                                     # a caller's own grid, lined up with the first
    want = coverage_oracle(g2p, sizes, *bounds[:2], cell, *bounds[2:], pts, labels)
    out = tiling.coverage(torch.from_numpy(georef), torch.from_numpy(sizes), cell, census=cen, bounds=bounds)
    assert set(out) == KEYS | CENSUS_KEYS
    np.testing.assert_array_equal(out["coverage"].cpu().numpy(), want["coverage"])
    for key, wkey, dtype in (("seen_by", "seen_by", torch.int64), ("cell_index", "cell", torch.int64), ("counts", "counts", torch.int32)):
        assert out[key].dtype == dtype and out[key].device.type == "cuda"
        np.testing.assert_array_equal(out[key].cpu().numpy(), want[wkey], err_msg=key)
    cc = want["counts"].sum(axis=(1, 2))
    assert out["class_counts"].dtype == torch.int64 and out["class_counts"].cpu().tolist() == cc.tolist()
    assert cc.sum() == want["pstats"][0] and 0 < cc.sum() < len(pts)
    area = float((bounds[2] * bounds[3] - int(want["stats"][0])) * cell * cell)
    assert out["area_m2"] == area
    assert out["density_per_km2"].dtype == torch.float64
    np.testing.assert_array_equal(out["density_per_km2"].cpu().numpy(), cc.astype(np.float64) / (area / 1e6))
    could = want["seen_by"] >= 1
    assert could.any() and not could.all()
    assert out["detection_rate"] == int(members[could].sum()) / int(want["seen_by"][could].sum()) and isinstance(out["detection_rate"], float)


@pytest.mark.gpu
def test_gpu_python_nan_cases_and_empty_census():
    dev = torch.device("cuda:0")
    georef, sizes, pts, labels, members = _python_case()
    cen = lambda m: {"points": torch.from_numpy(pts[m]).to(dev), "labels": torch.from_numpy(labels[m]).to(dev),
                     "members": torch.from_numpy(members[m]).to(dev)}
    some = np.arange(len(pts)) < 20
    # a grid far from every footprint: nothing observed, so no density; nobody could be seen, so no detection rate
    out = tiling.coverage(georef, sizes, 1.0, census=cen(some), bounds=(400000.0, 6000000.0, 9, 5))
    assert out["area_m2"] == 0.0 and out["gap_cells"] == 45 and not out["coverage"].any()
    assert torch.isnan(out["density_per_km2"]).all() and tuple(out["density_per_km2"].shape) == (7,)
    assert out["class_counts"].tolist() == [0] * 7 and out["cell_index"].tolist() == [[-1, -1]] * 20
    assert (out["seen_by"] >= 1).any()                                                # seen_by does not depend on the grid
    # no frames at all: the detection rate has an empty set
    out = tiling.coverage(np.zeros((0, 2, 3)), np.zeros((0, 2), dtype=np.int32), 1.0, census=cen(some))
    assert out["shape"] == (1, 1) and out["area_m2"] == 0.0 and math.isnan(out["detection_rate"])
    assert out["seen_by"].tolist() == [0] * 20
    # a census without individuals
    none = np.zeros(len(pts), dtype=bool)
    out = tiling.coverage(georef, sizes, 0.5, census=cen(none))
    assert set(out) == KEYS | CENSUS_KEYS and out["area_m2"] > 0
    assert tuple(out["seen_by"].shape) == (0,) and tuple(out["cell_index"].shape) == (0, 2) and not out["counts"].any()
    assert out["class_counts"].tolist() == [0] * 7 and out["density_per_km2"].tolist() == [0.0] * 7 and math.isnan(out["detection_rate"])


@pytest.mark.gpu
def test_gpu_end_to_end_three_overlapping_frames():
    """Three 1500 x 1300 windows of one synthetic strip, 300 px apart, through detect_frames -> census -> coverage on the
    grid footprint_bounds gives.  A keeper lies in its own frame's footprint only up to the rounding of the inverse, and a
    label can be outside 0..6, so the identity is binned + unbinned == count."""
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    m._hub.set_precision("fp16")
    rng = np.random.default_rng(16)
    H, W, step, gsd = 1500, 1300, 300, 0.02
    strip = torch.from_numpy(rng.integers(0, 256, (H, W + 2 * step, 3), dtype=np.uint8)).to(dev)
    frames = [strip[:, f * step:f * step + W].contiguous() for f in range(3)]
    whole = tiling.nadir_affine(H, W + 2 * step, (5.0e5, 6.0e6), gsd, 3.5)
    centres = [whole[:, :2] @ np.array([f * step + W / 2, H / 2]) + whole[:, 2] for f in range(3)]
    georef = np.stack([tiling.nadir_affine(H, W, tuple(c), gsd, 3.5) for c in centres])
    sizes = [(H, W)] * 3
    results = list(tiling.detect_frames(m, frames, overlap=128, batch=4))
    m._hub.close()
    cen = tiling.census(iter(results), georef, radius=0.5)
    assert cen["count"] > 0
    cell = 0.5
    out = tiling.coverage(georef, sizes, cell, census=cen)
    assert set(out) == KEYS | CENSUS_KEYS
    x0, y0, gx, gy = tiling.footprint_bounds(georef, sizes, cell)
    assert out["origin"] == (x0, y0) and out["shape"] == (gy, gx)
    want = coverage_oracle(tiling.ground_to_pixel(georef), sizes, x0, y0, cell, gx, gy, cen["points"].cpu().numpy(), cen["labels"].cpu().numpy())
    np.testing.assert_array_equal(out["coverage"].cpu().numpy(), want["coverage"])
    np.testing.assert_array_equal(out["seen_by"].cpu().numpy(), want["seen_by"])
    np.testing.assert_array_equal(out["cell_index"].cpu().numpy(), want["cell"])
    np.testing.assert_array_equal(out["counts"].cpu().numpy(), want["counts"])
    binned = int(out["class_counts"].sum())
    unbinned = int((out["cell_index"][:, 0] < 0).sum())
    assert binned + unbinned == cen["count"] and binned == int(want["pstats"][0]) and unbinned == int(want["pstats"][1])
    assert int(out["coverage"].max()) == 3 and int(out["seen_by"].max()) <= 3            # the middle of the strip is in all three
    # the union of the footprints, not their sum: 3 frames of 780 m^2, 300 px of new ground each
    assert 780.0 * 0.98 < out["area_m2"] < (W + 2 * step) * H * gsd * gsd * 1.05
    if (out["seen_by"] >= 1).any():
        assert out["detection_rate"] > 0
