"""Survey registration, refinement (include/wm_hip.h "Survey registration, refinement", tiling.refine): the integer normal
equations of one Gauss-Newton step per pair -- 28 sums -- and the host's solve, adjustment and loop.  The rule has no
reference behaviour; refine_sums_oracle restates it: the terms of every cell are formed one expression at a time in int64
(each is below 2^37) and summed in Python integers, so nothing in it can overflow.  The device's sums must equal it exactly:
every device comparison of sums is assert_array_equal.  The bounds of the host part are stated where they are used."""
import os
import re

import numpy as np
import pytest
import torch

from ground_cases import _p, entry_is_whole, header, last_error, macro
from pyramid_cases import oracle_loop
from register_cases import (CELL, DISPLACED, F64, FRAME_H, FRAME_W, INF, NAN, NEAR, SIDE, SIZES, SUMS, _case, _content, _corner_error, _cover,
                            _oracle_sums, _pairs, _planes, _render, _several_pairs, _survey, analytic_scene, per_k_planes, refine_sums_oracle)
from survey_util import DEV, ROOT, _Lazy, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling


def _oracle_table(A, B, table, search):
    return np.array([refine_sums_oracle(A[p], B[p], int(pr["gx"]), int(pr["gy"]), search)
                     if 1 <= pr["gx"] <= A[p].shape[0] and 1 <= pr["gy"] <= A[p].shape[0] else [0] * SUMS for p, pr in enumerate(table)],
                    dtype=np.int64).reshape(len(table), SUMS)


# ---- CPU: the oracle's hand cases ------------------------------------------------------------------------------------

def test_oracle_one_by_one_patch_inside_a_ring():
    A = np.array([[10]], dtype=np.uint8)
    B = np.array([[0, 5, 0], [2, 7, 9], [0, 11, 0]], dtype=np.uint8)              # ss = 5, w = 2, b = 7, e = 9, nn = 11
    # r = 3, gxv = 7, gyv = 6, x = y = 0: c = (7, 6, 0, 0, 7, 1)
    want = [49, 42, 0, 0, 49, 7,  36, 0, 0, 42, 6,  0, 0, 0, 0,  0, 0, 0,  49, 7,  1,   21, 18, 0, 0, 21, 3,   9]
    assert refine_sums_oracle(A, B, 1, 1, 1) == want
    # the same patch inside a wider ring (search 2, side 2): only the centre offset is used
    B2 = np.full((6, 6), 200, dtype=np.uint8)
    B2[1:4, 1:4] = B
    B2[1, 1] = B2[1, 3] = B2[3, 1] = B2[3, 3] = 0
    A2 = np.array([[10, 99], [99, 99]], dtype=np.uint8)
    assert refine_sums_oracle(A2, B2, 1, 1, 2) == want
    B[0, 1] = 0                                                                      # ss not seen: nothing counts
    assert refine_sums_oracle(A, B, 1, 1, 1) == [0] * SUMS


def test_oracle_3x3_zero_neighbour_and_zero_in_a():
    A = np.full((3, 3), 50, dtype=np.uint8)
    B = (np.arange(25, dtype=np.uint8).reshape(5, 5) * 3 + 20)                       # B[J][I] = 20 + 15 J + 3 I: gxv = 6, gyv = 30
    full = refine_sums_oracle(A, B, 3, 3, 1)
    assert full[20] == 9 and full[0] == 9 * 36 and full[6] == 9 * 900 and full[1] == 9 * 180
    # x, y in (-2, 0, 2): c2 = 30 x - 6 y and c3 = 6 x + 30 y sum to 0 over the patch, and so do their products with c0, c1
    assert full[2] == full[3] == full[7] == full[8] == 0
    assert full[11] == sum((30 * x - 6 * y) ** 2 for x in (-2, 0, 2) for y in (-2, 0, 2))
    assert full[12] == sum((30 * x - 6 * y) * (6 * x + 30 * y) for x in (-2, 0, 2) for y in (-2, 0, 2))
    Bz = B.copy()
    Bz[2, 1] = 0                           # (J, I) = (2, 1) is cell (1, 0)'s b, (1, 1)'s w, (0, 0)'s nn and (2, 0)'s ss: 5 cells remain
    got = refine_sums_oracle(A, Bz, 3, 3, 1)
    kept = [(j, i) for j in range(3) for i in range(3) if (j, i) not in ((1, 0), (1, 1), (0, 0), (2, 0))]
    assert got[20] == len(kept) == 5 and got[0] == 5 * 36
    assert got[27] == sum((50 - int(B[j + 1, i + 1])) ** 2 for j, i in kept)
    assert got[19] == sum(int(B[j + 1, i + 1]) for j, i in kept)                     # sum c4 * c5 = sum b
    Az = A.copy()
    Az[2, 2] = 0                                                                     # a zero in A drops that cell alone
    got = refine_sums_oracle(Az, B, 3, 3, 1)
    assert got[20] == 8 and got[27] == full[27] - (50 - int(B[3, 3])) ** 2
    # cells of A beyond gx, gy never count
    assert refine_sums_oracle(A, B, 2, 3, 1)[20] == 6


def test_constant_planes_are_rejected_without_raising():
    A, B = np.full((80, 80), 9, dtype=np.uint8), np.full((82, 82), 9, dtype=np.uint8)
    sums = np.array([refine_sums_oracle(A, B, 80, 80, 1)], dtype=np.int64)
    assert sums[0, 20] == 6400 and sums[0, 0] == sums[0, 6] == 0 and (sums[0, 21:] == 0).all()
    table = _pairs([(0, 1, 80, 80, 0.0, 0.0)])
    for exposure in (False, True):
        out = tiling.refine_solve(sums, table, exposure=exposure, min_cells=100)
        assert out["accepted"].tolist() == [False] and out["cells"].tolist() == [6400] and np.isnan(out["param"]).all()
    # a singular system whose diagonal is positive: the gradient has one direction only (a ramp east)
    B = np.tile((np.arange(82) * 2 + 10).astype(np.uint8), (82, 1))
    sums = np.array([refine_sums_oracle(B[1:81, 1:81].copy(), B, 80, 80, 1)], dtype=np.int64)
    assert sums[0, 0] > 0 and sums[0, 6] == 0
    assert tiling.refine_solve(sums, table, min_cells=100)["accepted"].tolist() == [False]
    # no cells at all
    out = tiling.refine_solve(np.zeros((1, SUMS), dtype=np.int64), table)
    assert out["accepted"].tolist() == [False] and np.isnan(out["rms"]).all()
    assert tiling.refine_solve(np.zeros((0, SUMS), dtype=np.int64), table[:0])["param"].shape == (0, 6)


# ---- CPU: refine_solve on synthetic sums -----------------------------------------------------------------------------

def _smooth(X, Y):
    """A smooth plane in about [70, 190]: a few sinusoids with wavelengths of 15 to 60 cells."""
    return (130.0 + 22.0 * np.sin(0.21 * X + 0.09 * Y + 0.3) + 18.0 * np.sin(-0.11 * X + 0.26 * Y + 1.1) +
            12.0 * np.sin(0.35 * X - 0.31 * Y + 2.0) + 8.0 * np.cos(0.1 * X + 0.4 * Y))


def _synthetic_pair(tx, ty, theta, sigma, gamma, o, n=96):
    """A = (1 + gamma) * B(X + d(X)) + o on an n x n patch, both planes rounded to uint8."""
    c = np.arange(n) + 0.5 - n / 2
    X, Y = np.meshgrid(c, c)
    XB, YB = np.meshgrid(np.arange(n + 2) - 0.5 - n / 2, np.arange(n + 2) - 0.5 - n / 2)
    dX, dY = tx - theta * Y + sigma * X, ty + theta * X + sigma * Y
    A = np.rint((1.0 + gamma) * _smooth(X + dX, Y + dY) + o)
    B = np.rint(_smooth(XB, YB))
    assert A.min() >= 1 and A.max() <= 255 and B.min() >= 1 and B.max() <= 255
    return A.astype(np.uint8), B.astype(np.uint8)


def test_refine_solve_recovers_a_known_shift_yaw_and_scale():
    truth = (0.30, -0.20, 0.004, -0.003)
    A, B = _synthetic_pair(*truth, 0.0, 0.0)
    sums = np.array([refine_sums_oracle(A, B, 96, 96, 1)], dtype=np.int64)
    table = _pairs([(0, 1, 96, 96, 0.0, 0.0)])
    out = tiling.refine_solve(sums, table)
    assert out["accepted"].tolist() == [True] and out["cells"].tolist() == [96 * 96]
    err = np.abs(out["param"][0, :4] - np.array(truth))
    print("refine_solve errors (tx, ty, theta, sigma):", err.tolist())
    # what is left is the second order of one linearisation (the central difference of a sinusoid of wave number k is short
    # by k^2 / 6, at most 3.5 % here, and the Taylor remainder 0.5 k |d| is of the same size) and uint8 rounding: bounds
    # of a tenth of each parameter.  Measured here: 0.0028 and 0.0024 cells, 8.1e-6 rad and 6.5e-7.
    assert err[0] < 0.03 and err[1] < 0.02 and err[2] < 4e-4 and err[3] < 3e-4
    assert (out["param"][0, 4:] == 0).all()
    # exposure=True on equal exposures finds no gain and no offset to speak of, and the same geometry
    both = tiling.refine_solve(sums, table, exposure=True)
    print("with exposure terms:", both["param"][0].tolist())
    assert both["accepted"].all() and abs(both["param"][0, 4]) < 0.01 and abs(both["param"][0, 5]) < 1.0
    assert np.abs(both["param"][0, :4] - np.array(truth)).max() < 0.03
    # max_step is the displacement at the patch corners: here |d| is at most about 0.74 cells
    assert tiling.refine_solve(sums, table, max_step=0.5)["accepted"].tolist() == [False]
    assert tiling.refine_solve(sums, table, min_cells=96 * 96 + 1)["accepted"].tolist() == [False]
    assert abs(out["rms"][0] - np.sqrt(sums[0, 27] / sums[0, 20])) < 1e-12


def test_refine_solve_recovers_gain_and_offset():
    truth = (0.30, -0.20, 0.004, -0.003)
    gamma, o = 1.0 / 0.7 - 1.0, -60.0
    A, B = _synthetic_pair(*truth, gamma, o)
    sums = np.array([refine_sums_oracle(A, B, 96, 96, 1)], dtype=np.int64)
    table = _pairs([(0, 1, 96, 96, 0.0, 0.0)])
    out = tiling.refine_solve(sums, table, exposure=True)
    print("gain and offset:", out["param"][0].tolist())
    assert out["accepted"].all()
    # gamma and o come with the curvature terms above and with the geometry's bias below: bounds of 0.01 (a fortieth of gamma)
    # and 1.5 grey levels.  Measured here: 0.4223 for 0.4286, -59.18 for -60
    assert abs(out["param"][0, 4] - gamma) < 0.01 and abs(out["param"][0, 5] - o) < 1.5
    # the linearisation drops the product gamma * (grad B . d): the geometry comes out (1 + gamma) times the truth, which the
    # next iteration of refine() removes (it contracts by |gamma| per step); the same tenth of each parameter as above
    scaled = (1.0 + gamma) * np.array(truth)
    err = np.abs(out["param"][0, :4] - scaled)
    print("errors against (1 + gamma) * truth:", err.tolist())
    assert err[0] < 0.03 * (1 + gamma) and err[1] < 0.02 * (1 + gamma) and err[2] < 4e-4 * (1 + gamma) and err[3] < 3e-4 * (1 + gamma)


# ---- CPU: adjust_similarity ------------------------------------------------------------------------------------------

def _consistent(ab, cp, cf, t, th, sg):
    """The (dx, dy, theta, sigma) every pair would measure for per-frame similarities (t, th, sg)."""
    a, b = ab[:, 0], ab[:, 1]
    lin = lambda f, v: np.stack([sg[f] * v[:, 0] - th[f] * v[:, 1], th[f] * v[:, 0] + sg[f] * v[:, 1]], axis=1)
    d = -((t[b] - t[a]) + lin(b, cp - cf[b]) - lin(a, cp - cf[a]))
    return np.concatenate([d, -(th[b] - th[a])[:, None], -(sg[b] - sg[a])[:, None]], axis=1)


def test_adjust_similarity_returns_consistent_measurements():
    rng = np.random.default_rng(4)
    cf = rng.uniform(-100, 100, size=(5, 2)) + np.array([500000.0, 6000000.0])
    t = np.array([[0.3, -0.2], [-0.4, 0.1], [0.2, 0.3], [-0.15, -0.225], [0.05, 0.025]])
    th = np.array([0.004, -0.006, 0.002, 0.003, -0.003])
    sg = np.array([0.002, 0.001, -0.004, 0.003, -0.002])
    assert np.abs(t.mean(axis=0)).max() < 1e-15 and abs(th.mean()) < 1e-15 and abs(sg.mean()) < 1e-15
    ab = np.array([(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 3)])
    cp = 0.5 * (cf[ab[:, 0]] + cf[ab[:, 1]]) + rng.uniform(-5, 5, size=(6, 2))
    m = _consistent(ab, cp, cf, t, th, sg)
    w = np.array([4096.0, 10000.0, 512.0, 7.0, 30000.0, 1.0])
    out = tiling.adjust_similarity(5, ab, cp, cf, m, w)
    # double rounding of such a system sits near 1e-13 at these coordinates; 1e-9 is adjust()'s bound, slack, not measured
    assert np.abs(out["shift"] - t).max() < 1e-9 and np.abs(out["yaw"] - th).max() < 1e-9 and np.abs(out["scale"] - sg).max() < 1e-9
    assert np.abs(out["residual"]).max() < 1e-9 and out["residual"].shape == (6, 4)
    assert out["component"].tolist() == [0, 0, 0, 0, 0]
    # the gauge: the means of a component without a fixed frame are zero
    assert np.abs(out["shift"].mean(axis=0)).max() < 1e-9 and abs(out["yaw"].mean()) < 1e-9 and abs(out["scale"].mean()) < 1e-9
    table = _pairs([(a, b, 8, 8, 0.0, 0.0) for a, b in ab])
    again = tiling.adjust_similarity(5, table, cp, cf, m, w)
    for k in out:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    # fixed frames stay: the others are what they are relative to frame 1
    rel = tiling.adjust_similarity(5, ab, cp, cf, m, w, fixed=[1])
    assert (rel["shift"][1] == 0).all() and rel["yaw"][1] == 0 and rel["scale"][1] == 0
    assert np.abs(rel["yaw"] - (th - th[1])).max() < 1e-9 and np.abs(rel["scale"] - (sg - sg[1])).max() < 1e-9
    want = _consistent(ab, cp, cf, rel["shift"], rel["yaw"], rel["scale"])          # the same field between every two frames
    assert np.abs(want - m).max() < 1e-9


def test_adjust_similarity_components_and_a_frame_without_pairs():
    rng = np.random.default_rng(5)
    cf = rng.uniform(-50, 50, size=(6, 2))
    ab = np.array([(0, 1), (1, 2), (4, 5), (2, 4)])                                  # 0-1-2 and 4-5; 3 alone; (2, 4) has weight 0
    cp = rng.uniform(-20, 20, size=(4, 2))
    t, th, sg = np.zeros((6, 2)), np.zeros(6), np.zeros(6)
    t[[0, 1, 2]] = [[-0.2, 0.1], [0.0, -0.3], [0.2, 0.2]]
    th[[0, 1, 2]] = [0.002, -0.003, 0.001]
    sg[[4, 5]] = [0.004, -0.004]
    t[[4, 5]] = [[0.0, 0.3], [0.0, -0.3]]
    m = _consistent(ab, cp, cf, t, th, sg)
    m[3] = (100.0, 100.0, 1.0, 1.0)
    out = tiling.adjust_similarity(6, ab, cp, cf, m, [10.0, 10.0, 5.0, 0.0])
    assert out["component"].tolist() == [0, 0, 0, -1, 4, 4]
    assert np.abs(out["shift"] - t).max() < 1e-9 and np.abs(out["yaw"] - th).max() < 1e-9 and np.abs(out["scale"] - sg).max() < 1e-9
    assert (out["shift"][3] == 0).all() and out["yaw"][3] == 0 and out["scale"][3] == 0   # no pair: the identity
    for comp in ([0, 1, 2], [4, 5]):                                                  # every component's gauge means are zero
        assert np.abs(out["shift"][comp].mean(axis=0)).max() < 1e-9 and abs(out["yaw"][comp].mean()) < 1e-9
        assert abs(out["scale"][comp].mean()) < 1e-9
    assert np.abs(out["residual"][:3]).max() < 1e-9 and np.abs(out["residual"][3]).min() > 0.5
    empty = tiling.adjust_similarity(3, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2)), np.zeros((3, 2)), np.zeros((0, 4)), np.zeros(0))
    assert (empty["shift"] == 0).all() and empty["component"].tolist() == [-1, -1, -1] and empty["residual"].shape == (0, 4)
    with pytest.raises(ValueError, match="measured"):
        tiling.adjust_similarity(6, ab, cp, cf, m[:, :2], [1.0] * 4)
    with pytest.raises(ValueError, match="frame_centres"):
        tiling.adjust_similarity(6, ab, cp, cf[:5], m, [1.0] * 4)
    with pytest.raises(ValueError, match="fixed"):
        tiling.adjust_similarity(6, ab, cp, cf, m, [1.0] * 4, fixed=[6])


# ---- the analytic scene (register_cases.py) and tiling.refine's loop on the oracles (pyramid_cases.py) ----------------

def _near(exposure_changes=False):
    """The name of the near scene in register_cases.ANALYTIC_SCENES: frames of one exposure, or of EXPOSURE's four."""
    return "near_exposure" if exposure_changes else "near"


def test_analytic_scene_is_what_the_issue_describes():
    frames, true, pert = analytic_scene("near")
    first = _corner_error(pert, true)
    print("initial worst corner error:", first)
    assert 1.4 < first < 1.8 and (pert[0] == true[0]).all()                        # the prototype's 1.62 m, frame 0 true
    table = tiling.register_pairs(pert, SIZES, CELL, 1, SIDE, 4096)
    assert len(table) == 6 and (table["gx"] == SIDE).all() and (table["gy"] == SIDE).all()


@pytest.mark.parametrize("exposure_changes", (False, True))
def test_whole_loop_on_the_oracle(exposure_changes):
    frames, true, pert = analytic_scene(_near(exposure_changes))
    first = _corner_error(pert, true)
    loop = oracle_loop(_near(exposure_changes), 0, 3, exposure_changes)
    print("worst corner error per iteration:", first, loop["errors"], "accepted:", [s["accepted"].tolist() for s in loop["steps"]])
    # the issue's bound: a quarter of a cell, and a quarter of where it started.  Measured here: 1.678 m -> 0.064, 0.0142,
    # 0.0141 m; with the exposure changes and exposure=True 0.640, 0.196, 0.0330 m (the gain's bias takes an iteration more)
    assert loop["errors"][-1] <= 0.25 * CELL and loop["errors"][-1] <= 0.25 * first
    assert (loop["georef"][0] == true[0]).all()                                      # the fixed frame has not moved, to the bit
    assert loop["steps"][-1]["accepted"].all()


def test_exposure_changes_need_the_exposure_terms():
    frames, true, pert = analytic_scene("near_exposure")
    with_terms, without = oracle_loop("near_exposure", 0, 3, True), oracle_loop("near_exposure", 0, 3, False)
    print("exposure changes: with the terms", with_terms["errors"], "without", without["errors"])
    # measured here: 0.033 m with the terms, 1.35 m without (1.40, 1.35, 1.35 over the iterations: it does not converge)
    assert without["errors"][-1] > with_terms["errors"][-1]


def test_lattice_trap_planes_coincide_while_the_georef_is_off():
    """cell = gsd = the scene's pixel and frames aligned with the axes: nearest sampling snaps every plane onto one lattice, so
    a georeference 0.3 m off renders the planes of the true one and the step sees nothing."""
    frames, true, _ = _survey()
    off = true.copy()
    off[:, 0, 2] += np.array([0.3, -0.3, 0.3, -0.3])
    off[:, 1, 2] += np.array([-0.3, 0.3, 0.3, -0.3])
    sizes = [(160, 200)] * 4
    table = tiling.register_pairs(off, sizes, 1.0, 1, 256, 4096)
    assert len(table) == 6
    sums = _oracle_sums(frames, off, sizes, table, 1.0, 256)
    assert (sums[:, 20] >= 4096).all() and (sums[:, 21:] == 0).all()               # R == 0 and sum r^2 == 0: identical planes
    step = tiling.refine_step(off, sizes, table, sums, 1.0)
    assert step["accepted"].all() and (step["param"] == 0).all()
    np.testing.assert_array_equal(step["georef"], off)                              # still 0.42 m off, and it does not move
    assert step["max_corner"] == 0.0 and step["weighted_rms"] == 0.0


# ---- CPU: argument errors, header, binding, library --------------------------------------------------------------------

def test_refine_python_argument_errors_before_device_work():
    g = np.stack([tiling.nadir_affine(80, 100, (50.0, 40.0), 1.0, 0.0), tiling.nadir_affine(80, 100, (60.0, 50.0), 1.0, 0.0)])
    sizes = [(80, 100), (80, 100)]
    imgs = [np.zeros((80, 100, 3), dtype=np.uint8)] * 2
    lazy = _Lazy(imgs)
    for name, bads in (("side", (0, 513, 1.5, "64", None, True)), ("min_cells", (0, -3, 2.5, None, "1", 2 ** 31)),
                       ("iters", (0, -1, 1.5, "3", None, True)), ("pair_chunk", (0, -1, 2.5, "8", None, True, 65536)),
                       ("max_step", (0, -1.0, NAN, INF, "far", None, True)), ("exposure", (1, 0, "yes", None)),
                       ("cell", (0, -1.0, NAN, INF, "wide", None)), ("fixed", ([2], [-1], [0.5], "0", 7))):
        for bad in bads:
            args = {"cell": 1.0, name: bad}
            with pytest.raises(ValueError, match=name):
                tiling.refine(lazy, g, args.pop("cell"), sizes=sizes, **args)
    for bad in (-1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="refine"):
            tiling.register(lazy, g, 1.0, sizes=sizes, refine=bad)
    with pytest.raises(ValueError, match="sizes is required"):
        tiling.refine(lazy, g, 1.0)
    with pytest.raises(ValueError, match="indexed"):
        tiling.refine(iter(imgs), g, 1.0, sizes=sizes)
    with pytest.raises(ValueError, match="1 frames for 2 georeferences"):
        tiling.refine(_Lazy(imgs[:1]), g, 1.0, sizes=sizes)
    with pytest.raises(ValueError, match="georef"):
        tiling.refine(lazy, np.zeros((2, 3, 2)), 1.0, sizes=sizes)
    for bad in ([(0, 1, 8, 8, 0.0, 0.0)], _pairs([(0, 2, 8, 8, 0.0, 0.0)]), _pairs([(0, 1, 8, 65, 0.0, 0.0)]), _pairs([(0, 1, 8, 8, NAN, 0.0)])):
        with pytest.raises(ValueError, match="pairs"):
            tiling.refine(lazy, g, 1.0, sizes=sizes, side=64, pairs=bad)
    table = _pairs([(0, 1, 8, 8, 0.0, 0.0)])
    for bad in (np.zeros((1, 27), dtype=np.int64), np.zeros((1, SUMS)), np.zeros(SUMS, dtype=np.int64)):
        with pytest.raises(ValueError, match="sums"):
            tiling.refine_solve(bad, table)
        with pytest.raises(ValueError, match="sums"):
            tiling.refine_step(g, sizes, table, bad, 1.0)
    with pytest.raises(ValueError, match="pairs"):
        tiling.refine_solve(np.zeros((2, SUMS), dtype=np.int64), table)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device tensor"):              # no CPU fallback
            tiling.refine(lazy, g, 1.0, sizes=sizes, min_cells=1)
    assert lazy.asked == []                                                     # nothing was loaded on the way to an error
    # no pair at all needs no device: every frame keeps its georeference
    far = np.stack([g[0], tiling.nadir_affine(80, 100, (5000.0, 40.0), 1.0, 0.0)])
    out = tiling.refine(lazy, far, 1.0, sizes=sizes)
    assert out["pairs"].shape == (0,) and np.array_equal(out["georef"], far) and lazy.asked == [] and out["history"] == []
    assert (out["yaw"] == 0).all() and (out["scale"] == 0).all() and (out["shift"] == 0).all() and out["param"].shape == (0, 6)


def _abi_refine(n_pairs=3, search=4, side=64, a=0x5001, b=0x6001, pairs=0x4000, sums=0x8000):
    """wm_register_refine with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_register_refine(_p(a), _p(b), _p(pairs), n_pairs, search, side, _p(sums), None)


def test_refine_abi_argument_errors_without_gpu():
    err = last_error
    assert _abi_refine(n_pairs=-1) < 0 and "n_pairs" in err()
    assert _abi_refine(n_pairs=N.REGISTER_MAX_PAIRS + 1) < 0 and "n_pairs" in err()
    for bad in (0, -1, N.REGISTER_MAX_SEARCH + 1):
        assert _abi_refine(search=bad) < 0 and "search" in err() and "wm_register_refine" in err()
    assert _abi_refine(side=0) < 0 and "side" in err()
    assert _abi_refine(side=N.REGISTER_MAX_SIDE + 1) < 0 and "side" in err()
    assert _abi_refine(pairs=0) < 0 and "pairs_dev" in err()
    assert _abi_refine(pairs=0x4004) < 0 and "pairs_dev" in err() and "aligned" in err()
    assert _abi_refine(a=0) < 0 and "a_dev" in err()
    assert _abi_refine(b=0) < 0 and "b_dev" in err()
    assert _abi_refine(sums=0) < 0 and "sums_dev" in err()
    for off in (1, 2, 4, 7):
        assert _abi_refine(sums=0x8000 + off) < 0 and "sums_dev" in err() and "aligned" in err()
    # n_pairs == 0 returns 0 before looking at anything
    assert _abi_refine(n_pairs=0, pairs=0, a=0, b=0, sums=0, search=0, side=0) == 0


def test_refine_symbol_constant_and_abi_13():
    hdr = header()
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey registration, refinement" in hdr and len(re.findall("13, additive", hdr)) == 5
    assert re.search(r"13, additive: wm_register_refine", hdr)
    assert entry_is_whole("wm_register_refine")
    kern = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "register_refine_kernels.h")).read()
    assert macro("WM_REGISTER_REFINE_SUMS") == N.REGISTER_REFINE_SUMS == tiling.REGISTER_REFINE_SUMS == SUMS
    assert int(re.search(r"constexpr int REFINE_SUMS = (\d+);", kern).group(1)) == SUMS and "asm" not in kern
    assert "static_assert(REFINE_SUMS == WM_REGISTER_REFINE_SUMS" in kern


# ---- GPU: equality of all 28 sums with the oracle ----------------------------------------------------------------------

POISON = -0x5A5A5A5A5A5A5A5A


def device_sums(a, b, table, search, side):
    """wm_register_refine on device planes a (P, side, side), b (P, E, E), the sums pre-filled with a poison value."""
    n = len(table)
    pairs = _up(table.view(np.uint8).reshape(n, 32))
    sums = torch.full((n, SUMS), POISON, device=DEV, dtype=torch.int64)
    N.check(N.lib().wm_register_refine(N.ptr(a), N.ptr(b), N.ptr(pairs), n, search, side, N.ptr(sums), N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def _check_planes(A, B, table, search):
    """Hand-built planes (lists of (side, side) and (E, E) uint8): the device's sums equal the oracle's."""
    side = A[0].shape[0]
    got = device_sums(_up(np.stack(A)), _up(np.stack(B)), table, search, side)
    want = _oracle_table(A, B, table, search)
    np.testing.assert_array_equal(got, want)
    return got


# gx, gy, search, side: the issue's list (SHAPES' idea, search >= 1), then one cell either side of the kernel's 64 x 32 tile
REFINE_SHAPES = {
    "1x1_s1_side1": (1, 1, 1, 1), "1x1_s1_side4": (1, 1, 1, 4), "3x5_s1": (3, 5, 1, 8), "4x4_s5": (4, 4, 5, 4), "63x65_s5": (63, 65, 5, 65),
    "64x64_s1": (64, 64, 1, 64), "65x63_s5_side80": (65, 63, 5, 80), "1x65_s5": (1, 65, 5, 65), "64x1_s1": (64, 1, 1, 64),
    "70x19_s5": (70, 19, 5, 70), "257x65_s5_side300": (257, 65, 5, 300), "33x37_s64": (33, 37, 64, 40),
    "63x31_s1": (63, 31, 1, 64), "64x32_s1": (64, 32, 1, 64), "65x33_s2": (65, 33, 2, 66), "128x33_s1": (128, 33, 1, 129), "129x31_s1": (129, 31, 1, 130)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFINE_SHAPES))
def test_gpu_smallest_shapes(name):
    gx, gy, search, side = REFINE_SHAPES[name]
    rng = np.random.default_rng(sorted(REFINE_SHAPES).index(name))
    A = rng.integers(1, 256, size=(side, side), dtype=np.uint8)                     # non-zero past gx, gy too: must not count
    B = rng.integers(1, 256, size=(side + 2 * search, side + 2 * search), dtype=np.uint8)
    got = _check_planes([A], [B], _pairs([(0, 1, gx, gy, 0.0, 0.0)]), search)
    assert got[0, 20] == gx * gy and got[0, 27] > 0


def test_oracle_at_the_overflow_bound():
    want = _overflow_case()[2]
    assert want[20] == 512 * 512 and want[0] == want[6] == 254 * 254 * 512 * 512
    # sum c2^2 = sum (x gyv - y gxv)^2 with |gxv| = |gyv| = 254: sum (x^2 + y^2) * 254^2 -+ 2 x y gxv gyv; the largest entries
    assert max(want[11], want[15]) > 1.4e15 and max(abs(v) for v in want) < 2 ** 63


_OVERFLOW = []


def _overflow_case():
    if not _OVERFLOW:
        A = np.full((512, 512), 255, dtype=np.uint8)
        idx = np.arange(514)
        lev = np.array([1, 1, 255, 255], dtype=np.uint8)
        B = lev[(idx[:, None] + idx[None, :]) % 4]
        # period 4 in both axes: along a row and along a column the values two apart always differ, so e - w and nn - ss are +-254
        assert (np.abs(B[1:-1, 2:].astype(int) - B[1:-1, :-2]) == 254).all() and (np.abs(B[2:, 1:-1].astype(int) - B[:-2, 1:-1]) == 254).all()
        _OVERFLOW.append((A, B, refine_sums_oracle(A, B, 512, 512, 1)))
    return _OVERFLOW[0]


@pytest.mark.gpu
def test_gpu_512x512_at_the_overflow_bound():
    A, B, want = _overflow_case()
    got = device_sums(_up(A[None]), _up(B[None]), _pairs([(0, 1, 512, 512, 0.0, 0.0)]), 1, 512)
    np.testing.assert_array_equal(got[0], np.array(want, dtype=np.int64))


@pytest.mark.gpu
def test_gpu_sprinkled_zeros_and_a_plane_that_sees_nothing():
    A, B = per_k_planes()                                                           # 72 x 72 against 82 x 82: 20 % / 30 % not seen
    table = _pairs([(0, 1, 70, 45, 0.0, 0.0), (0, 1, 72, 72, 0.0, 0.0), (0, 1, 70, 45, 0.0, 0.0), (0, 1, 70, 45, 0.0, 0.0)])
    got = _check_planes([A, A, A, np.zeros_like(A)], [B, B, np.zeros_like(B), B], table, 5)
    assert 0 < got[0, 20] < 70 * 45 // 4 and (got[2:] == 0).all()                    # 0.8 * 0.7^5: about 13 % of the cells count


@pytest.mark.gpu
def test_gpu_several_pairs_bad_pairs_and_the_real_render():
    case = _several_pairs()                                                         # search 6, side 72; pair 3's A is a yawed frame
    a, b = _planes(case)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    _render(case, a, b, status, list(range(len(case["images"]))))
    assert status.item() == 0
    A, B = list(a.cpu().numpy()), list(b.cpu().numpy())
    got = device_sums(a, b, case["pairs"], case["search"], case["side"])
    want = _oracle_table(A, B, case["pairs"], case["search"])
    np.testing.assert_array_equal(got, want)
    assert 0 < got[3, 20] < 72 * 72 and (got[:4, 20] > 0).all()                      # the diagonal mask edge cuts pair 3's patch
    # gx or gy outside [1, side]: all-zero sums, and the other pairs of the launch are still exact
    bad = case["pairs"].copy()
    bad["gx"][0], bad["gy"][2], bad["gx"][4] = 0, case["side"] + 1, -3
    got = device_sums(a, b, bad, case["search"], case["side"])
    assert (got[[0, 2, 4]] == 0).all()
    np.testing.assert_array_equal(got[[1, 3]], want[[1, 3]])


@pytest.mark.gpu
def test_gpu_diagonal_mask_edge_and_planes_of_search_5_and_search_1_agree():
    x0, y0, cell = 300.0, 400.0, 1.0
    small = _content(40, 40, 21), tiling.nadir_affine(40, 40, (x0 + 30.0, y0 + 30.0), 1.0, 45.0)     # a diamond inside the patch
    full = _cover(60, 60, 5, x0, y0, cell, 22)
    rows = [(0, 1, 60, 60, x0, y0), (1, 0, 60, 60, x0, y0)]
    sums = {}
    for search in (5, 1):
        case = _case([small, full], rows, cell, search, 64, 100)
        a, b = _planes(case)
        status = torch.zeros(1, device=DEV, dtype=torch.int32)
        _render(case, a, b, status, [0, 1])
        assert status.item() == 0
        sums[search] = device_sums(a, b, case["pairs"], search, 64)
        np.testing.assert_array_equal(sums[search], _oracle_table(list(a.cpu().numpy()), list(b.cpu().numpy()), case["pairs"], search))
    np.testing.assert_array_equal(sums[5], sums[1])
    assert 0 < sums[1][0, 20] < 60 * 60 and 0 < sums[1][1, 20] < sums[1][0, 20]      # B's mask also loses the cells beside its edge


# ---- GPU: end to end -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("exposure_changes", (False, True))
def test_gpu_refine_equals_the_oracle_loop(exposure_changes):
    frames, true, pert = analytic_scene(_near(exposure_changes))
    want = oracle_loop(_near(exposure_changes), 0, 3, exposure_changes)
    out = tiling.refine(frames, pert, CELL, side=SIDE, iters=3, exposure=exposure_changes, fixed=[0])
    np.testing.assert_array_equal(out["pairs"], want["table"])
    assert np.abs(out["georef"] - want["georef"]).max() < 1e-9                      # the same integers into the same host code
    last = want["steps"][-1]
    np.testing.assert_array_equal(out["cells"], last["cells"])
    np.testing.assert_array_equal(out["accepted"], last["accepted"])
    first, err = _corner_error(pert, true), _corner_error(out["georef"], true)
    print("device: worst corner error", first, "->", err, "history", out["history"])
    assert err <= 0.25 * CELL and err <= 0.25 * first
    assert len(out["history"]) == 3 and out["history"][-1]["max_corner"] < out["history"][0]["max_corner"]
    assert (out["georef"][0] == true[0]).all() and out["yaw"][0] == 0 and out["scale"][0] == 0
    # the whole correction undoes the perturbation: two opposite corners are 256 m apart and each is within 0.25 m, so what is
    # left of yaw and scale is at most 0.5 / 256 = 1.96e-3 (radians; the perturbation's scale enters at second order, 2e-5)
    for f in range(1, 4):
        assert abs(out["yaw"][f] + np.radians(NEAR[f][2])) < 2e-3 and abs((1 + out["scale"][f]) * (1 + NEAR[f][3]) - 1) < 2e-3


@pytest.mark.gpu
def test_gpu_lazy_frames_chunks_and_register_without_refine():
    frames, true, pert = analytic_scene("near")
    whole = tiling.refine(frames, pert, CELL, side=SIDE, iters=2, fixed=[0])
    lazy = _Lazy(frames)
    again = tiling.refine(lazy, pert, CELL, sizes=SIZES, side=SIDE, iters=2, fixed=[0], pair_chunk=2)
    for key in ("georef", "yaw", "scale", "shift", "pairs", "param", "cells", "rms", "accepted"):
        np.testing.assert_array_equal(again[key], whole[key], err_msg=key)
    assert again["history"] == whole["history"]
    assert lazy.asked == [0, 1, 2, 0, 1, 2, 3, 1, 2, 3] * 2                          # chunks (0,1)(0,2) | (0,3)(1,2) | (1,3)(2,3), twice
    # register(refine=0) is register(): the same keys, the same arrays, and no frame asked for a refinement
    s_frames, s_true, displaced = _survey()
    lazy = _Lazy(s_frames)
    plain = tiling.register(lazy, displaced, 1.0, sizes=[(160, 200)] * 4, search=8, side=256, min_cells=4096)
    asked = list(lazy.asked)
    zero = tiling.register(lazy, displaced, 1.0, sizes=[(160, 200)] * 4, search=8, side=256, min_cells=4096, refine=0)
    assert sorted(plain) == sorted(zero) == sorted(["georef", "shift", "pairs", "offset", "cells", "mean", "runner_up", "accepted", "residual",
                                                   "component", "corr"])
    for key in plain:
        np.testing.assert_array_equal(zero[key], plain[key], err_msg=key)
    assert lazy.asked == asked * 2 and asked == [0, 1, 2, 3]
    ab = [(int(p["frame_a"]), int(p["frame_b"])) for p in plain["pairs"]]
    np.testing.assert_array_equal(plain["offset"], np.array([DISPLACED[b] - DISPLACED[a] for a, b in ab], dtype=np.int64))
    assert np.abs(plain["georef"] - s_true).max() < 1e-9


@pytest.mark.gpu
def test_gpu_register_zncc_with_refine_fits_the_exposures():
    """metric="zncc" hands exposure=True to the refinement: a gain and an offset per frame, whole cells and the perturbation."""
    frames, true, pert = analytic_scene("near_exposure")
    displaced = pert.copy()
    displaced[:, 0, 2] += WHOLE_CELLS[:, 0] * CELL
    displaced[:, 1, 2] += WHOLE_CELLS[:, 1] * CELL
    out = tiling.register(frames, displaced, CELL, search=8, side=SIDE, metric="zncc", refine=3, fixed=[0])
    coarse, fine = _corner_error(out["georef"], true), _corner_error(out["refine"]["georef"], true)
    print("zncc: worst corner error after the search", coarse, "after the refinement", fine, "param", out["refine"]["param"].tolist())
    assert out["accepted"].all() and out["refine"]["accepted"].all()
    assert fine <= 0.25 * CELL and fine <= 0.25 * _corner_error(pert, true)          # the oracle's loop from here: 0.030 m
    # pair (0, 1) sees gain 1 / 0.7 and offset -30 / 0.7 between its frames: the last iteration's fit is within about a tenth
    # of both (0.05 of 0.43, 5 of 42.9 grey levels; the synthetic pair above came within a seventieth at one linearisation)
    gamma, o = out["refine"]["param"][0, 4:]
    assert abs(gamma - (1.0 / 0.7 - 1.0)) < 0.05 and abs(o + 30.0 / 0.7) < 5.0


WHOLE_CELLS = np.array([(0, 0), (-4, 1), (2, 3), (-1, -2)], dtype=F64)                # frame 0 is true and fixed
# 12 animals in the ground all four frames see, 12 m apart
ANIMALS_AT = np.array([(x, y) for y in (2002.0, 2014.0, 2026.0) for x in (1004.0, 1016.0, 1028.0, 1040.0)])


def _detections_through(true):
    """Every animal boxed in each frame that sees it through the TRUE georeference."""
    g2p = tiling.ground_to_pixel(true)
    out = []
    for f in range(len(true)):
        u = g2p[f, 0, 0] * ANIMALS_AT[:, 0] + g2p[f, 0, 1] * ANIMALS_AT[:, 1] + g2p[f, 0, 2]
        v = g2p[f, 1, 0] * ANIMALS_AT[:, 0] + g2p[f, 1, 1] * ANIMALS_AT[:, 1] + g2p[f, 1, 2]
        ok = (u >= 4) & (u < FRAME_W - 4) & (v >= 4) & (v < FRAME_H - 4)
        boxes = np.stack([u - 3, v - 3, u + 3, v + 3], axis=1)[ok].astype(np.float32)
        out.append({"boxes": _up(boxes), "scores": _up(np.linspace(0.9, 0.5, ok.sum()).astype(np.float32)),
                    "labels": torch.ones(int(ok.sum()), device=DEV, dtype=torch.int64)})
    return out


@pytest.mark.gpu
def test_gpu_register_with_refine_corrects_the_census():
    frames, true, pert = analytic_scene("near")
    displaced = pert.copy()
    displaced[:, 0, 2] += WHOLE_CELLS[:, 0] * CELL
    displaced[:, 1, 2] += WHOLE_CELLS[:, 1] * CELL
    first = _corner_error(displaced, true)
    out = tiling.register(frames, displaced, CELL, search=8, side=SIDE, refine=3, fixed=[0])
    assert sorted(out) == sorted(["georef", "shift", "pairs", "offset", "cells", "mean", "runner_up", "accepted", "residual", "component",
                                  "corr", "refine"])
    coarse, fine = _corner_error(out["georef"], true), _corner_error(out["refine"]["georef"], true)
    print("worst corner error: displaced", first, "after the search", coarse, "after the refinement", fine, "accepted", out["accepted"].tolist())
    assert first > 4.0 and out["accepted"].any()
    assert fine <= 0.25 * CELL and fine <= 0.25 * _corner_error(pert, true)
    np.testing.assert_array_equal(out["refine"]["pairs"], out["pairs"])            # the same pair table
    assert (out["refine"]["georef"][0] == true[0]).all()
    dets = _detections_through(true)
    assert sum(len(d["boxes"]) for d in dets) >= 3 * len(ANIMALS_AT)
    assert tiling.census(dets, out["refine"]["georef"], 0.5)["count"] == len(ANIMALS_AT) == 12
    assert tiling.census(dets, out["georef"], 0.5)["count"] > len(ANIMALS_AT)         # whole cells alone still split animals
