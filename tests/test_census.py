"""Survey census (include/wm_hip.h "Survey census", tiling.census): the detections of overlapping frames grouped into
individuals on the ground.  The rule has no reference behaviour; census_oracle (tests/ground_oracle.py) restates it
sequentially -- numpy float64, the header's operation order, one detection at a time -- and the device result must equal it
exactly: integers as integers, ground points bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from ground_cases import entry_is_whole, macro
from ground_oracle import census_oracle
from survey_util import ROOT
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


def _pt_boxes(xy):
    """Boxes (n,4) fp32 whose centres are the given pixel positions (exact for multiples of 1/4 below 2^20)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.concatenate([xy - (2.0, 3.0), xy + (2.0, 3.0)], axis=1).astype(np.float32)


def _case(xy, frame, scores=None, labels=None, georef=None, radius=1.0, same_class=False):
    n = len(frame)
    return {"boxes": _pt_boxes(xy), "scores": np.asarray(scores if scores is not None else np.linspace(0.9, 0.5, n), dtype=np.float32),
            "labels": np.asarray(labels if labels is not None else np.zeros(n), dtype=np.int32),
            "frame": np.asarray(frame, dtype=np.int32),
            "georef": np.asarray(georef if georef is not None else [IDENT] * (max(frame) + 1), dtype=np.float64),
            "radius": radius, "same_class": same_class}


def _oracle(case):
    return census_oracle(case["boxes"], case["scores"], case["labels"], case["frame"], case["georef"], case["radius"], case["same_class"])


# name -> (case, expected individual, expected members)
def _hand_cases():
    inf, nan = np.inf, np.nan
    cases = {}
    cases["one_animal_two_frames"] = (_case([(10, 10), (10.25, 10)], [0, 1]), [0, 0], [2])
    # herd: two animals 1.0 m apart, both seen by frames 0 and 1, radius 1.5: absorbing everything in range would give 1
    cases["herd"] = (_case([(10, 10), (11, 10), (10, 10.25), (11, 10.25)], [0, 0, 1, 1], radius=1.5), [0, 1, 0, 1], [2, 2])
    cases["same_frame_never_joins"] = (_case([(5, 5), (5.1, 5)], [0, 0]), [0, 1], [1, 1])
    # a third frame's detection between two individuals joins the nearer one
    cases["third_joins_nearer"] = (_case([(0, 0), (1.5, 0), (1.0, 0)], [0, 1, 2]), [0, 1, 1], [1, 2])
    cases["tie_to_earlier"] = (_case([(0, 0), (1.5, 0), (0.75, 0)], [0, 1, 2]), [0, 1, 0], [2, 1])
    cases["d2_equals_r2_inside"] = (_case([(0, 0), (3, 4), (6, 8.25)], [0, 1, 2], radius=5.0), [0, 0, 1], [2, 1])
    cases["same_class"] = (_case([(0, 0), (0.25, 0), (0.5, 0)], [0, 1, 2], labels=[3, 4, 3], same_class=True), [0, 1, 0], [2, 1])
    cases["class_agnostic"] = (_case([(0, 0), (0.25, 0), (0.5, 0)], [0, 1, 2], labels=[3, 4, 3]), [0, 0, 0], [3])
    c = _case([(0, 0), (0.25, 0), (0.5, 0), (0.25, 0.25), (0, 0.25)], [0, 1, 1, 2, 3], scores=[0.9, 0.8, inf, 0.7, 0.6],
              georef=[IDENT, IDENT, [[1, 0, 0], [0, inf, 0]], IDENT])
    c["boxes"][1, 2] = nan
    c["frame"][4] = 4                                                    # == F
    cases["invalid"] = (c, [0, -1, -1, -1, -1], [1])
    # -0 and +0 tie: the input index decides, so detection 0 (score -0) founds before detection 1 (score +0)
    cases["signed_zero_tie"] = (_case([(0, 0), (5, 0), (0.25, 0)], [0, 0, 1], scores=[-0.0, 0.0, -1.0]), [0, 1, 0], [2, 1])
    return cases


HAND = _hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_hand_cases(name):
    case, individual, members = HAND[name]
    got = _oracle(case)
    assert got["individual"].tolist() == individual
    assert got["members"].tolist() == members
    assert got["count"] == len(members)
    bad = np.array(individual) < 0
    assert np.isnan(got["points"][bad]).all() and np.isfinite(got["points"][~bad]).all()
    # keepers are the first member of each individual in priority order
    for k, i in enumerate(got["keeper"]):
        assert got["individual"][i] == k


def test_oracle_keeper_point_not_mean():
    """The distance is to the keeper's point: a chain 0 - 0.75 - 1.5 does not walk."""
    got = _oracle(_case([(0, 0), (0.75, 0), (1.5, 0)], [0, 1, 2]))
    assert got["individual"].tolist() == [0, 0, 1]


def test_nadir_affine_hand_values():
    H, W, E, Nn, gsd = 4000, 6000, 500000.0, 6000000.0, 0.025
    s37, c37 = 0.6018150231520483, 0.7986355100472928                            # sin, cos of 37 degrees
    want = {0.0: (gsd, 0.0, 0.0, -gsd), 90.0: (0.0, -gsd, -gsd, 0.0), 180.0: (-gsd, 0.0, 0.0, gsd),
            37.0: (gsd * c37, -gsd * s37, -gsd * s37, -gsd * c37)}
    for yaw, (a0, a1, a3, a4) in want.items():
        g = tiling.nadir_affine(H, W, (E, Nn), gsd, yaw)
        assert g.shape == (2, 3) and g.dtype == np.float64
        np.testing.assert_allclose(g[:, :2], [[a0, a1], [a3, a4]], rtol=1e-9, atol=gsd * 1e-9)
        centre = g[:, :2] @ np.array([W / 2, H / 2]) + g[:, 2]
        np.testing.assert_allclose(centre, [E, Nn], rtol=1e-9)
    g0, g90 = tiling.nadir_affine(H, W, (E, Nn), gsd), tiling.nadir_affine(H, W, (E, Nn), gsd, 90.0)
    right, down, up = np.array([1.0, 0.0]), np.array([0.0, 1.0]), np.array([0.0, -1.0])
    np.testing.assert_allclose(g0[:, :2] @ right, [gsd, 0.0], atol=gsd * 1e-9)       # yaw 0: right is east
    np.testing.assert_allclose(g0[:, :2] @ down, [0.0, -gsd], atol=gsd * 1e-9)       # and down is south
    np.testing.assert_allclose(g90[:, :2] @ up, [gsd, 0.0], atol=gsd * 1e-9)         # yaw 90: up is east
    with pytest.raises(ValueError):
        tiling.nadir_affine(H, W, (E, Nn), 0.0)


def _cpu_results(ks):
    return [{"boxes": torch.zeros((k, 4)), "scores": torch.zeros(k), "labels": torch.zeros(k, dtype=torch.int64)} for k in ks]


def test_census_python_argument_errors_before_device_work():
    res = _cpu_results([2, 1])
    g = [IDENT, IDENT]
    for bad in (-1.0, float("nan"), float("inf"), 1e200, "wide", None):
        with pytest.raises(ValueError, match="radius"):
            tiling.census(res, g, bad)
    with pytest.raises(ValueError, match="georef"):
        tiling.census(res, np.zeros((2, 3, 2)), 1.0)
    with pytest.raises(ValueError, match="georeferences"):
        tiling.census(res, [IDENT], 1.0)
    with pytest.raises(ValueError, match="georeferences"):
        tiling.census(iter(res), [IDENT] * 3, 1.0)
    with pytest.raises(ValueError, match="result 0"):
        tiling.census([{"boxes": torch.zeros((2, 4))}], [IDENT], 1.0)
    with pytest.raises(ValueError, match="exceed"):
        tiling.census(_cpu_results([N.CENSUS_MAX_DETS, 1]), g, 1.0)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):          # no CPU fallback
        tiling.census(res, g, 1.0)


def test_census_python_n0():
    for res, g in (([], []), ([], np.zeros((0, 2, 3))), (_cpu_results([0, 0]), [IDENT, IDENT])):
        out = tiling.census(iter(res), g, 1.0)
        assert out["count"] == 0 and out["det_offsets"] == [0] * (len(res) + 1)
        assert out["individual"].shape == (0,) and out["individual"].dtype == torch.int64
        assert out["points"].shape == (0, 2) and out["det_points"].dtype == torch.float64
        assert out["class_counts"].tolist() == [0] * 7
        assert set(out) == {"individual", "keeper", "points", "det_points", "scores", "labels", "frame", "members", "det_frame",
                            "det_offsets", "count", "class_counts"}


def _abi_call(n, radius=1.0, flags=0, scratch=0x1000, scratch_bytes=None, n_frames=1, buf=0x2000):
    """wm_census with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    lib = N.lib()
    p = C.c_void_p(buf)
    if scratch_bytes is None:
        scratch_bytes = max(lib.wm_census_scratch_bytes(min(max(n, 0), N.CENSUS_MAX_DETS)), 0)
    return lib.wm_census(p, p, p, p, n, p, n_frames, radius, flags, C.c_void_p(scratch), scratch_bytes, p, p, p, p, p, None)


def test_census_abi_argument_errors_without_gpu():
    lib = N.lib()
    err = lambda: lib.wm_last_error().decode()
    assert lib.wm_census_scratch_bytes(0) >= 0
    assert lib.wm_census_scratch_bytes(1000) > lib.wm_census_scratch_bytes(999) > 0
    assert lib.wm_census_scratch_bytes(N.CENSUS_MAX_DETS) > 0
    assert lib.wm_census_scratch_bytes(N.CENSUS_MAX_DETS + 1) < 0 and "wm_census_scratch_bytes" in err()
    assert lib.wm_census_scratch_bytes(-1) < 0
    assert _abi_call(10, radius=-1.0) < 0 and "radius" in err()
    assert _abi_call(10, radius=float("nan")) < 0 and "radius" in err()
    assert _abi_call(10, radius=float("inf")) < 0 and "radius" in err()
    assert _abi_call(10, radius=1e200) < 0 and "square" in err()
    assert _abi_call(N.CENSUS_MAX_DETS + 1) < 0 and "outside" in err()
    assert _abi_call(-1) < 0
    assert _abi_call(10, scratch_bytes=lib.wm_census_scratch_bytes(10) - 1) < 0 and "scratch of" in err()
    assert _abi_call(10, scratch=0x1008) < 0 and "aligned" in err()
    assert _abi_call(10, n_frames=0) < 0 and "n_frames" in err()
    assert _abi_call(10, flags=2) < 0 and "flags" in err()
    assert _abi_call(10, buf=0) < 0 and "null" in err()
    # n == 0 returns 0 before looking at any pointer or argument
    assert lib.wm_census(None, None, None, None, 0, None, 0, -1.0, 0, None, 0, None, None, None, None, None, None) == 0


def test_census_abi_13_and_symbols():
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert entry_is_whole("wm_census") and entry_is_whole("wm_census_scratch_bytes", returns="int64_t")
    for name, val in (("WM_CENSUS_MAX_DETS", N.CENSUS_MAX_DETS), ("WM_CENSUS_SAME_CLASS", N.CENSUS_SAME_CLASS),
                      ("WM_CENSUS_UNSOLVED", N.CENSUS_UNSOLVED)):
        assert macro(name) == val, name
    assert tiling.CENSUS_MAX_DETS == 262144


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _lds_sort_capacity():
    src = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "survey_kernels.h")).read()
    return int(re.search(r"MF_LDS_SORT = (\d+)", src).group(1))


def _device_abi(case):
    """wm_census through the C-ABI -> numpy results, the status word and the rounds taken."""
    dev = torch.device("cuda:0")
    n = case["boxes"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, scores, labels, frame = up(case["boxes"]), up(case["scores"]), up(case["labels"]), up(case["frame"])
    g = up(case["georef"].reshape(-1, 6))
    lib = N.lib()
    nbytes = lib.wm_census_scratch_bytes(n)
    assert nbytes > 0
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    points = torch.full((n, 2), 7.0, device=dev, dtype=torch.float64)
    individual, keeper, members = (torch.full((n,), -7, device=dev, dtype=torch.int32) for _ in range(3))
    count = torch.full((2,), -7, device=dev, dtype=torch.int32)
    N.check(lib.wm_census(N.ptr(boxes), N.ptr(scores), N.ptr(labels), N.ptr(frame), n, N.ptr(g), g.shape[0], float(case["radius"]),
                          N.CENSUS_SAME_CLASS if case["same_class"] else 0, N.ptr(scratch), nbytes, N.ptr(points), N.ptr(individual),
                          N.ptr(keeper), N.ptr(members), N.ptr(count), N.stream_ptr(dev)))
    k, status = count.cpu().tolist()
    return {"points": points.cpu().numpy(), "individual": individual.cpu().numpy().astype(np.int64),
            "keeper": keeper[:k].cpu().numpy().astype(np.int64), "members": members[:k].cpu().numpy().astype(np.int64),
            "count": k, "status": status, "rounds": int(scratch[:4].view(torch.int32).item())}


def _assert_same(got, want):
    assert got["count"] == want["count"]
    for key in ("individual", "keeper", "members"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    gp, wp = got["points"], want["points"]
    bad = np.isnan(wp).any(axis=1)
    assert np.isnan(gp[bad]).all()
    np.testing.assert_array_equal(gp[~bad].view(np.int64), wp[~bad].view(np.int64))      # bit for bit


def _check_properties(case, got):
    """What every census result must satisfy, checked without the oracle."""
    ind, pts, fr, sc = got["individual"], got["points"], case["frame"], case["scores"]
    valid = ind >= 0
    assert got["status"] == 0
    assert got["members"].sum() == valid.sum() and (got["members"] >= 1).all()
    np.testing.assert_array_equal(np.bincount(ind[valid], minlength=got["count"]), got["members"])
    pairs = np.stack([ind[valid], fr[valid].astype(np.int64)], axis=1)
    assert len(np.unique(pairs, axis=0)) == len(pairs)                           # no individual has two members of one frame
    kp = pts[got["keeper"]][ind[valid]]
    d = pts[valid] - kp
    r2 = np.float64(case["radius"]) * np.float64(case["radius"])
    assert (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= r2).all()                   # every member within the radius of its keeper
    np.testing.assert_array_equal(ind[got["keeper"]], np.arange(got["count"]))
    ks = sc[got["keeper"]].astype(np.float64) + 0.0
    prio = list(zip((-ks).tolist(), got["keeper"].tolist()))
    assert prio == sorted(prio)                                                  # keepers in priority order
    if case["same_class"]:
        np.testing.assert_array_equal(case["labels"][valid], case["labels"][got["keeper"]][ind[valid]])


def _run_and_check(case):
    want = _oracle(case)
    got = _device_abi(case)
    _assert_same(got, want)
    _check_properties(case, got)
    again = _device_abi(case)                                                    # determinism
    for key in ("individual", "keeper", "members"):
        np.testing.assert_array_equal(again[key], got[key])
    np.testing.assert_array_equal(again["points"].view(np.int64), got["points"].view(np.int64))
    assert (again["count"], again["status"]) == (got["count"], got["status"])
    return got, want


def _herd_case(n, F, side_m, seed, radius=1.0):
    """n detections of animals on a 0.25 m lattice in a side_m square, each seen by 1-4 of F frames with a jitter from
    {0, +-0.25} m; scores from 16 values; detections grouped by frame (as tiling.census concatenates them)."""
    rng = np.random.default_rng(seed)
    levels = np.linspace(0.2, 0.95, 16).astype(np.float32)
    cells = int(side_m * 4)
    pos, frs = [], []
    while len(pos) < n:
        a = rng.integers(0, cells + 1, 2)
        for f in rng.choice(F, size=int(rng.integers(1, 5)), replace=False):
            pos.append(a + rng.integers(-1, 2, 2))
            frs.append(f)
    pos, frs = np.array(pos[:n]), np.array(frs[:n])
    order = np.argsort(frs, kind="stable")
    pos, frs = pos[order], frs[order]
    org = rng.integers(-400, 400, (F, 2))                                        # frame origins, lattice units
    georef = np.array([[[0.25, 0, 0.25 * ox], [0, -0.25, -0.25 * oy]] for ox, oy in org])
    px = np.stack([pos[:, 0] - org[frs, 0], -pos[:, 1] - org[frs, 1]], axis=1)     # X = 0.25 * pos_x, Y = 0.25 * pos_y exactly
    c = _case(px, frs, scores=rng.choice(levels, n), labels=rng.integers(0, 7, n), georef=georef, radius=radius)
    return c


def _as_results(case, dev):
    """The case as detect_frames-style dicts, one per frame (the case's detections are grouped by frame)."""
    F = case["georef"].shape[0]
    assert (np.diff(case["frame"]) >= 0).all()
    out = []
    for f in range(F):
        m = case["frame"] == f
        out.append({"boxes": torch.from_numpy(case["boxes"][m]).to(dev), "scores": torch.from_numpy(case["scores"][m]).to(dev),
                    "labels": torch.from_numpy(case["labels"][m].astype(np.int64)).to(dev)})
    return out


def _check_python(case, want):
    """tiling.census on the same detections: every key, against the oracle."""
    dev = torch.device("cuda:0")
    out = tiling.census(iter(_as_results(case, dev)), case["georef"].reshape(-1, 2, 3), case["radius"], case["same_class"])
    n, k = case["boxes"].shape[0], want["count"]
    assert out["count"] == k and isinstance(out["count"], int)
    np.testing.assert_array_equal(out["individual"].cpu().numpy(), want["individual"])
    np.testing.assert_array_equal(out["keeper"].cpu().numpy(), want["keeper"])
    np.testing.assert_array_equal(out["members"].cpu().numpy(), want["members"])
    assert out["individual"].dtype == out["keeper"].dtype == out["members"].dtype == out["det_frame"].dtype == torch.int64
    dp = out["det_points"].cpu().numpy()
    bad = np.isnan(want["points"]).any(axis=1)
    np.testing.assert_array_equal(dp[~bad].view(np.int64), want["points"][~bad].view(np.int64))
    np.testing.assert_array_equal(out["points"].cpu().numpy().view(np.int64), want["points"][want["keeper"]].view(np.int64))
    np.testing.assert_array_equal(out["scores"].cpu().numpy(), case["scores"][want["keeper"]])
    np.testing.assert_array_equal(out["labels"].cpu().numpy(), case["labels"][want["keeper"]])
    np.testing.assert_array_equal(out["frame"].cpu().numpy(), case["frame"][want["keeper"]])
    np.testing.assert_array_equal(out["det_frame"].cpu().numpy(), case["frame"])
    assert out["det_offsets"] == [int((case["frame"] < f).sum()) for f in range(case["georef"].shape[0] + 1)] and out["det_offsets"][-1] == n
    np.testing.assert_array_equal(out["class_counts"].cpu().numpy(), np.bincount(case["labels"][want["keeper"]], minlength=7))
    assert out["points"].dtype == out["det_points"].dtype == torch.float64


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_cases(name):
    case, individual, members = HAND[name]
    got, _ = _run_and_check(case)
    assert got["individual"].tolist() == individual and got["members"].tolist() == members


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 65, 1023, 1025, 1500])
def test_gpu_random_herds(n):
    case = _herd_case(n, F=12, side_m=max(3.0, math.sqrt(n / 2.5)), seed=100 + n)
    got, want = _run_and_check(case)
    if n >= 63:
        assert (want["members"] > 1).any() and want["count"] < n
    _check_python(case, want)
    both = dict(case, same_class=True)
    _run_and_check(both)


@pytest.mark.gpu
def test_gpu_dense_herd_few_frames():
    """600 detections of 4 frames in 5 x 5 m: a detection has more same-frame neighbours within 2 * radius than the kernel
    keeps in registers, so its rescan of the window decides which individuals its frame already gave to."""
    case = _herd_case(600, F=4, side_m=5.0, seed=3)
    got, want = _run_and_check(case)
    assert (want["members"] > 1).any()
    _run_and_check(dict(case, same_class=True))


@pytest.mark.gpu
def test_gpu_past_lds_sort_capacity():
    """The smallest n at which the sorts run in global scratch and the rank scan takes several passes."""
    n = _lds_sort_capacity() + 4
    case = _herd_case(n, F=12, side_m=300.0, seed=7)
    got, want = _run_and_check(case)
    assert (want["members"] > 1).any()


@pytest.mark.gpu
def test_gpu_long_dependency_chain():
    """600 points 0.9 m apart on a line, frames cycling 0, 1, 2, scores falling along the line: every decision waits for
    the one before it.  Must equal the oracle and finish with status 0 (the round loop is bounded by n)."""
    n = 600
    xy = np.stack([0.9 * np.arange(n), np.zeros(n)], axis=1)
    case = _case(xy, np.arange(n) % 3, scores=np.linspace(0.99, 0.01, n), radius=1.0)
    assert (np.diff(case["scores"]) < 0).all()
    got, want = _run_and_check(case)
    assert got["status"] == 0 and 1 <= got["rounds"] <= n
    assert 1 < want["count"] < n


@pytest.mark.gpu
def test_gpu_yawed_frames_large_coordinates():
    """Georeferences from nadir_affine (yaw 0, 180, 3.5 degrees, gsd 0.02-0.03 m, UTM-sized coordinates): the ground points and
    every association are exact against the oracle, which only double arithmetic without contraction can be."""
    rng = np.random.default_rng(5)
    H, W = 4000, 6000
    E0, N0 = 5.0e5 + 123.4, 6.0e6 + 567.8
    frames = [(0.0, 0.02, (E0, N0)), (180.0, 0.025, (E0 + 30.0, N0 + 5.0)), (3.5, 0.03, (E0 + 15.0, N0 - 20.0)),
              (3.5, 0.021, (E0 - 10.0, N0 + 10.0))]
    georef = np.stack([tiling.nadir_affine(H, W, c, gsd, yaw) for yaw, gsd, c in frames])
    animals = np.stack([E0 + rng.uniform(-40, 60, 260), N0 + rng.uniform(-40, 40, 260)], axis=1)
    animals = np.concatenate([animals, animals[:60] + rng.uniform(0.3, 1.2, (60, 2))])     # close neighbours
    px, fr = [], []
    for f, g in enumerate(georef):
        p = np.linalg.solve(g[:, :2], (animals - g[:, 2]).T).T + rng.normal(0, 4.0, animals.shape)       # ~0.1 m of noise
        inside = (p[:, 0] > 0) & (p[:, 0] < W) & (p[:, 1] > 0) & (p[:, 1] < H)
        px.append(p[inside])
        fr.append(np.full(int(inside.sum()), f))
    px, fr = np.concatenate(px), np.concatenate(fr)
    n = len(fr)
    assert n > 400 and all((fr == f).sum() > 20 for f in range(4))
    half = rng.uniform(8, 30, (n, 2))
    case = _case(px, fr, scores=rng.uniform(0.1, 1.0, n), labels=rng.integers(0, 7, n), georef=georef, radius=0.5)
    case["boxes"] = np.concatenate([px - half, px + half], axis=1).astype(np.float32)
    got, want = _run_and_check(case)
    assert (want["members"] > 1).sum() > 50
    _check_python(case, want)


@pytest.mark.gpu
def test_gpu_end_to_end_same_frame_twice():
    """One 1500 x 1300 frame through detect_frames twice, as a two-frame survey with one georeference: every frame-0
    detection keeps its own individual and its frame-1 twin (equal score, later index, distance 0) joins it."""
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    m._hub.set_precision("fp16")
    rng = np.random.default_rng(16)                                              # test_survey.py's seed for its frames
    frame = torch.from_numpy(rng.integers(0, 256, (1500, 1300, 3), dtype=np.uint8)).to(dev)
    g = tiling.nadir_affine(1500, 1300, (5.0e5, 6.0e6), 0.02, 3.5)
    results = list(tiling.detect_frames(m, [frame, frame], overlap=128, batch=4))
    m._hub.close()
    k0 = results[0]["boxes"].shape[0]
    assert k0 > 0 and results[1]["boxes"].shape[0] == k0
    assert torch.equal(results[0]["boxes"], results[1]["boxes"])
    out = tiling.census(iter(results), [g, g], radius=0.5)
    assert out["count"] == k0
    assert out["members"].tolist() == [2] * k0
    assert out["frame"].tolist() == [0] * k0
    assert out["det_offsets"] == [0, k0, 2 * k0]
    case = {"boxes": torch.cat([r["boxes"] for r in results]).cpu().numpy(), "scores": torch.cat([r["scores"] for r in results]).cpu().numpy(),
            "labels": torch.cat([r["labels"] for r in results]).cpu().numpy().astype(np.int32),
            "frame": np.repeat(np.arange(2, dtype=np.int32), k0), "georef": np.stack([g, g]), "radius": 0.5, "same_class": False}
    want = _oracle(case)
    np.testing.assert_array_equal(out["individual"].cpu().numpy(), want["individual"])
    np.testing.assert_array_equal(out["keeper"].cpu().numpy(), want["keeper"])
    np.testing.assert_array_equal(out["members"].cpu().numpy(), want["members"])
    np.testing.assert_array_equal(out["det_points"].cpu().numpy().view(np.int64), want["points"].view(np.int64))
