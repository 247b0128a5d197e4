"""Survey mosaic (include/wm_hip.h "Survey mosaic", tiling.mosaic): the frames of a survey laid onto the ground grid.  The rule
has no reference behaviour; mosaic_oracle (tests/ground_oracle.py) restates it sequentially -- one cell at a time, numpy
float64, vectorised over the frames only, the header's operation order -- and the device result must equal it exactly: sources
are integers and pixels are uint8 behind arithmetic that is rounded once per operation, so every comparison is
assert_array_equal and there is no tolerance anywhere."""
import os
import re

import numpy as np
import pytest
import torch

from ground_cases import (FRAME_A, FRAME_B, FRAME_SWEEP, GRID_SWEEP, INF, NAN, ORIGIN_CELL_SWEEP, RESIDENT_SWEEP, _case, _mosaic_gpu_case,
                          _mosaic_oracle, _mosaic_python_case, _p, entry_is_whole, header, last_error, macro)
from ground_oracle import MODES, SENTINEL, mosaic_oracle, mosaic_oracle_by_frame, uv
from survey_util import DEV, ROOT, _kernel_constants, _Lazy, _up, _yawed_90
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling
from wildlifemapper_amd._survey import _frame_descs

# Pixel (y, x) of frame A and of frame B (ground_cases.py: u = 2 X, v = 4 - 2 Y; B 2 m further east) holds (16 y + x, 100 + x, 200 - y).
RAMP = np.array([[(16 * y + x, 100 + x, 200 - y) for x in range(8)] for y in range(4)], dtype=np.uint8)
# 2 x 1 px holding 10 and 13 in every channel, 1 m pixels: u = X, v = 1 - Y
FRAME_PAIR = ([1, 0, 0, 0, -1, 1], 1, 2)
PAIR = np.array([[(10, 10, 10), (13, 13, 13)]], dtype=np.uint8)


def _singular():
    return (tiling.ground_to_pixel(np.array([[1.0, 2.0, 5.0], [2.0, 4.0, 7.0]])), 4, 8)             # det == 0: a row of NaN


# name -> (case, expected source rows from j = 0 (south) upwards)
def _seam_cases():
    cases = {}
    none5 = [-1] * 5
    one = [[0, 0, 0, 0, -1], [0, 0, 0, 0, -1], none5]
    cases["one_frame"] = (_case([FRAME_A], 0, 0, 1, 5, 3, images=[RAMP]), one)
    # centres at X = 1..6: A sees 1, 2, 3; B sees 2..5.  At X = 3 both are 2 px from their centre column (u = 6 and u = 2,
    # centre 4) on the same row: the two e are the same number, and the lower index wins
    cases["two_frames_2m_apart"] = (_case([FRAME_A, FRAME_B], 0.5, 0, 1, 6, 3, images=[RAMP, RAMP]),
                                    [[0, 0, 0, 1, 1, -1], [0, 0, 0, 1, 1, -1], [-1] * 6])
    cases["two_frames_2m_apart_swapped"] = (_case([FRAME_B, FRAME_A], 0.5, 0, 1, 6, 3, images=[RAMP, RAMP]),
                                            [[1, 1, 0, 0, 0, -1], [1, 1, 0, 0, 0, -1], [-1] * 6])
    cases["identical_georeferences"] = (_case([FRAME_A, FRAME_A], 0, 0, 1, 5, 3, images=[RAMP, RAMP[::-1].copy()]), one)
    side = [-1, 0, 0, -1]
    cases["yawed_90"] = (_case([_yawed_90()], 8, 17, 1, 4, 6, images=[RAMP]), [[-1] * 4, side, side, side, side, [-1] * 4])
    five = [[5, 5, 5, 5, -1], [5, 5, 5, 5, -1], none5]
    never = [([2, NAN, 0, 0, -2, 4], 4, 8), ([2, 0, 0, 0, -2, INF], 4, 8), _singular(), ([2, 0, 0, 0, -2, 4], 0, 8), ([2, 0, 0, 0, -2, 4], 4, -3)]
    cases["never_a_source"] = (_case(never + [FRAME_A], 0, 0, 1, 5, 3, images=[RAMP, RAMP, RAMP, None, None, RAMP]), five)
    return cases


SEAM = _seam_cases()


# name -> (case, mode or None for both, expected channel 0 rows from j = 0 upwards)
def _pixel_cases():
    cases = {}
    # centres at X = 0.25 + 0.5 i, Y = 0.25 + 0.5 j: u = i + 0.5, v = 3.5 - j, every centre on a pixel centre
    cases["on_pixel_centres"] = (_case([FRAME_A], 0, 0, 0.5, 8, 4, images=[RAMP]), None, RAMP[::-1, :, 0].tolist())
    # u = 1 exactly (column 1, not 0), v = 3 exactly (row 3): cell (0, 0) of the 1 m grid
    cases["nearest_at_integer_u"] = (_case([FRAME_A], 0, 0, 1, 5, 3, images=[RAMP]), "nearest",
                                     [[49, 51, 53, 55, SENTINEL[0]], [17, 19, 21, 23, SENTINEL[0]], [SENTINEL[0]] * 5])
    # the same cells, bilinear: half way between columns and rows, (32 + 33 + 48 + 49) / 4 = 40.5 -> 41
    cases["bilinear_between_four"] = (_case([FRAME_A], 0, 0, 1, 5, 3, images=[RAMP]), "bilinear",
                                      [[41, 43, 45, 47, SENTINEL[0]], [9, 11, 13, 15, SENTINEL[0]], [SENTINEL[0]] * 5])
    # u = 1.0: half way between 10 and 13, 11.5 rounds up
    cases["bilinear_half_way"] = (_case([FRAME_PAIR], 0.5, 0, 1, 1, 1, images=[PAIR]), "bilinear", [[12]])
    # u = 0.25, 0.75, 1.25, 1.75: the first and the last lie within half a pixel of the edge and replicate it
    cases["bilinear_edge_replicate"] = (_case([FRAME_PAIR], 0, 0.25, 0.5, 4, 1, images=[PAIR]), "bilinear", [[10, 11, 12, 13]])
    return cases


PIXEL = _pixel_cases()


@pytest.mark.parametrize("name", sorted(SEAM))
def test_oracle_seam_hand_cases(name):
    case, rows = SEAM[name]
    got = _mosaic_oracle(case)
    assert got["source"].tolist() == rows
    flat = [f for r in rows for f in r]
    assert got["won"].tolist() == [flat.count(f) for f in range(case["g2p"].shape[0])]
    assert got["stats"].tolist() == [len(flat) - flat.count(-1), flat.count(-1)]


def test_oracle_two_frames_tie_is_exact():
    case, _ = SEAM["two_frames_2m_apart"]
    b, Xc, Yc = case["g2p"], np.float64(3.0), np.float64(0.5)
    u, v = uv(b, Xc, Yc)
    e = (u - 4.0) * (u - 4.0) + (v - 2.0) * (v - 2.0)
    assert u.tolist() == [6.0, 2.0] and e[0] == e[1] == 5.0


@pytest.mark.parametrize("name", sorted(PIXEL))
def test_oracle_pixel_hand_cases(name):
    case, mode, rows = PIXEL[name]
    got = _mosaic_oracle(case)
    for m in ([mode] if mode else sorted(MODES)):
        assert got[m][:, :, 0].tolist() == rows, m
    if name == "on_pixel_centres":
        np.testing.assert_array_equal(got["bilinear"], RAMP[::-1])
        np.testing.assert_array_equal(got["nearest"], RAMP[::-1])
    if name == "nearest_at_integer_u":
        assert got["nearest"][0, 0].tolist() == [16 * 3 + 1, 101, 197]


@pytest.mark.parametrize("name", sorted(SEAM) + sorted(PIXEL) + ["grid_70x19", "past_one_chunk", "mixed_sizes_in_one_chunk", "random_survey"])
def test_oracle_by_frame_equals_oracle(name):
    if name in SEAM or name in PIXEL:
        case = (SEAM.get(name) or PIXEL.get(name))[0]
        want = _mosaic_oracle(case)
    else:
        case, want = _mosaic_gpu_case(name)
    got = mosaic_oracle_by_frame(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"], case["images"])
    assert set(got) == set(want)
    for key in want:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_resampled_georef():
    H, W = 8, 16
    a = tiling.nadir_affine(H, W, (512.0, 1024.0), 0.5, 90.0)
    a2 = tiling.resampled_georef(a, (H, W), (H // 2, W // 2))
    assert a2.shape == (2, 3) and a2.dtype == np.float64
    for x, y in ((0.0, 0.0), (4.0, 2.0), (16.0, 8.0), (5.5, 1.25)):
        np.testing.assert_array_equal(a2[:, :2] @ np.array([x / 2, y / 2]) + a2[:, 2], a[:, :2] @ np.array([x, y]) + a[:, 2])
    g = np.array([[[0.5, 0.25, 7.0], [0.125, -0.5, 9.0]], [[2.0, 0.0, 1.0], [0.0, -2.0, 3.0]]])
    out = tiling.resampled_georef(g, [(8, 16), (6, 4)], [(4, 4), (12, 8)])
    np.testing.assert_array_equal(out, [[[2.0, 0.5, 7.0], [0.5, -1.0, 9.0]], [[1.0, 0.0, 1.0], [0.0, -1.0, 3.0]]])
    np.testing.assert_array_equal(tiling.resampled_georef(torch.from_numpy(g), (8, 16), (4, 8)), g * [[[2.0, 2.0, 1.0]]])
    np.testing.assert_array_equal(tiling.resampled_georef(g, (8, 16), (8, 16)), g)
    with pytest.raises(ValueError, match="georef"):
        tiling.resampled_georef(np.zeros((3, 2)), (8, 16), (4, 8))
    with pytest.raises(ValueError, match="georef"):
        tiling.resampled_georef("georef", (8, 16), (4, 8))
    for bad in ((8,), (8, 16, 3), [(8, 16)] * 3, (0, 16), (8.5, 16), "size", None):
        with pytest.raises(ValueError, match="size"):
            tiling.resampled_georef(g, bad, (4, 8))
        with pytest.raises(ValueError, match="new_size"):
            tiling.resampled_georef(g, (8, 16), bad)


def test_mosaic_python_argument_errors_before_device_work():
    g = [[[0.5, 0, 0.0], [0, -0.5, 2.0]]] * 2
    sizes = [(4, 8), (4, 8)]
    frames = [RAMP, RAMP]
    lazy = _Lazy(frames)
    for bad in ("cubic", None, 1, b"nearest"):
        with pytest.raises(ValueError, match="sample"):
            tiling.mosaic(frames, g, 1.0, sample=bad)
    for bad in ((0, 0), (0, 0, 256), (0, -1, 0), (0.5, 0, 0), "red", None, 7):
        with pytest.raises(ValueError, match="fill"):
            tiling.mosaic(frames, g, 1.0, fill=bad)
    for bad in (0, -1, 2.5, "8", None, True, NAN):
        with pytest.raises(ValueError, match="chunk"):
            tiling.mosaic(frames, g, 1.0, chunk=bad)
    with pytest.raises(ValueError, match="marker"):
        tiling.mosaic(frames, g, 1.0, marker=3)
    k = 3
    cen = {"points": torch.zeros((k, 2), dtype=torch.float64), "labels": torch.zeros(k, dtype=torch.int64)}
    with pytest.raises(ValueError, match="marker"):
        tiling.mosaic(frames, g, 1.0, census=cen)
    for bad in (0, -2, 1.5, "3", True):
        with pytest.raises(ValueError, match="marker"):
            tiling.mosaic(frames, g, 1.0, census=cen, marker=bad)
    with pytest.raises(ValueError, match="'points'"):
        tiling.mosaic(frames, g, 1.0, census={"labels": cen["labels"]}, marker=3)
    with pytest.raises(ValueError, match="census"):
        tiling.mosaic(frames, g, 1.0, census=dict(cen, points=torch.zeros((k, 2))), marker=3)            # float32 points
    with pytest.raises(ValueError, match="width"):
        tiling.mosaic(frames, g, 1.0, census=cen, marker=3, width=0)
    with pytest.raises(ValueError, match="palette"):
        tiling.mosaic(frames, g, 1.0, census=cen, marker=3, palette=np.zeros((3, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="sizes is required"):
        tiling.mosaic(lazy, g, 1.0)
    with pytest.raises(ValueError, match="sizes is required"):
        tiling.mosaic([RAMP, "frame_0002.jpg"], g, 1.0)
    with pytest.raises(ValueError, match="indexed"):
        tiling.mosaic(iter(frames), g, 1.0, sizes=sizes)
    with pytest.raises(ValueError, match="sizes for 2 georeferences"):
        tiling.mosaic(lazy, g, 1.0, sizes=[(4, 8)])
    with pytest.raises(ValueError, match="1 frames for 2 georeferences"):
        tiling.mosaic(_Lazy([RAMP]), g, 1.0, sizes=sizes)
    with pytest.raises(ValueError, match="georeferences"):
        tiling.mosaic([RAMP], g, 1.0)
    for bad in (0, -1.0, NAN, INF, "wide", None):
        with pytest.raises(ValueError, match="cell"):
            tiling.mosaic(lazy, g, bad, sizes=sizes)
        with pytest.raises(ValueError, match="cell"):
            tiling.mosaic_plan(g, sizes, bad)
    with pytest.raises(ValueError, match="georef"):
        tiling.mosaic_plan(np.zeros((2, 3, 2)), sizes, 1.0)
    with pytest.raises(ValueError, match="sizes"):
        tiling.mosaic_plan(g, [(4.5, 8), (4, 8)], 1.0)
    for call in (lambda **kw: tiling.mosaic(lazy, g, 1.0, sizes=sizes, **kw), lambda **kw: tiling.mosaic_plan(g, sizes, 1.0, **kw)):
        with pytest.raises(ValueError, match="larger cell"):
            call(bounds=(0.0, 0.0, N.COVERAGE_MAX_SIDE + 1, 1))
        for bad in ((0.0, 0.0, 0, 1), (NAN, 0.0, 5, 5), (0.0, 0.0, 5.5, 5), (0.0, 0.0, 5), "grid"):
            with pytest.raises(ValueError, match="bounds"):
                call(bounds=bad)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):              # no CPU fallback
        tiling.mosaic(lazy, g, 1.0, sizes=sizes, census=cen, marker=3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm device tensor"):
            tiling.mosaic(lazy, g, 1.0, sizes=sizes)
        with pytest.raises(RuntimeError, match="ROCm device tensor"):
            tiling.mosaic_plan(g, sizes, 1.0)
    assert lazy.asked == []                                                     # nothing was loaded on the way to an error


def _abi_plan(n_frames=2, x0=0.0, y0=0.0, cell=1.0, gx=5, gy=3, g2p=0x2000, size=0x3000, source=0x4000, won=0x5000, stats=0x6000):
    """wm_mosaic_plan with fake, never dereferenced device pointers: only paths that return before any HIP call."""
    return N.lib().wm_mosaic_plan(_p(g2p), _p(size), n_frames, x0, y0, cell, gx, gy, _p(source), _p(won), _p(stats), None)


def _abi_fill(n_frames=2, n_resident=2, x0=0.0, y0=0.0, cell=1.0, gx=5, gy=3, mode=N.MOSAIC_BILINEAR, flags=0, frames=0x1000, slot=0x7000,
              g2p=0x2000, size=0x3000, source=0x4000, mosaic=0x8000, status=0x9000):
    return N.lib().wm_mosaic_fill_u8(_p(frames), n_resident, _p(slot), _p(g2p), _p(size), n_frames, x0, y0, cell, gx, gy, _p(source), mode, flags,
                                     _p(mosaic), _p(status), None)


def test_mosaic_abi_argument_errors_without_gpu():
    err = last_error
    for call in (_abi_plan, _abi_fill):
        for kwargs, word in GRID_SWEEP + FRAME_SWEEP + ORIGIN_CELL_SWEEP:
            assert call(**kwargs) < 0 and word in err(), (call.__name__, kwargs, word, err())
        assert call(source=0) < 0 and "source_dev" in err()
        assert call(source=0x4002) < 0 and "aligned" in err()
    assert _abi_plan(won=0) < 0 and "won_dev" in err()
    assert _abi_plan(stats=0) < 0 and "stats_dev" in err()
    assert _abi_plan(won=0x5002) < 0 and "aligned" in err()
    assert _abi_plan(stats=0x6004) < 0 and "aligned" in err()
    for kwargs, word in RESIDENT_SWEEP:
        assert _abi_fill(**kwargs) < 0 and word in err(), ("_abi_fill", kwargs, word, err())
    for bad in (-1, 2, 7):
        assert _abi_fill(mode=bad) < 0 and "mode" in err()
    for bad in (2, 4, 3, -2):
        assert _abi_fill(flags=bad) < 0 and "flags" in err()
    assert _abi_fill(frames=0) < 0 and "frames_dev" in err()
    assert _abi_fill(slot=0) < 0 and "slot_dev" in err()
    assert _abi_fill(mosaic=0) < 0 and "mosaic_dev" in err()
    assert _abi_fill(status=0) < 0 and "status_dev" in err()
    assert _abi_fill(frames=0x1004) < 0 and "aligned" in err()
    assert _abi_fill(slot=0x7002) < 0 and "aligned" in err()
    assert _abi_fill(status=0x9002) < 0 and "aligned" in err()
    # nothing can be resident: returns 0 after the checks, before any HIP call
    assert _abi_fill(n_resident=0, frames=0, slot=0) == 0
    assert _abi_fill(n_frames=0, g2p=0, size=0, frames=0, slot=0) == 0
    assert _abi_fill(n_resident=0, mode=5) < 0 and "mode" in err()


def test_mosaic_symbols_and_abi_13():
    assert macro("WM_ABI_VERSION") == 13 == N.ABI_VERSION == N.lib().wm_abi_version()
    assert "Survey mosaic" in header() and len(re.findall("13, additive", header())) >= 2
    for name in ("wm_mosaic_plan", "wm_mosaic_fill_u8"):
        assert entry_is_whole(name), name
    for name, val in (("WM_MOSAIC_NEAREST", N.MOSAIC_NEAREST), ("WM_MOSAIC_BILINEAR", N.MOSAIC_BILINEAR), ("WM_MOSAIC_NORTH_UP", N.MOSAIC_NORTH_UP),
                      ("WM_MOSAIC_BAD_SLOT", N.MOSAIC_BAD_SLOT), ("WM_MOSAIC_BAD_SIZE", N.MOSAIC_BAD_SIZE), ("WM_MOSAIC_BAD_SOURCE", N.MOSAIC_BAD_SOURCE)):
        assert macro(name) == val, name
    assert MODES == {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}              # ground_oracle.py holds the two integers
    assert N.MOSAIC_NEAREST != N.MOSAIC_BILINEAR and tiling.MOSAIC_SAMPLES == MODES
    kern = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "mosaic_kernels.h")).read()
    shared = ("cov_stage(", "cov_load_frame(", ".may_touch(", "cov_uv(", "cov_inside(")        # the cull is behind CovBlock::may_touch
    assert '#include "coverage_kernels.h"' in kern and "CovBlock blk(" in kern and all(call in kern for call in shared)    # shared, not copied
    assert "cov_stage(CovFrames" not in kern and "struct CovBlock" not in kern and "asm" not in kern
    assert not re.search(r"(int|bool|void|double)\s+(cov_\w+|may_touch)\s*\(", kern)               # none of them is defined here
    reg = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "register_kernels.h")).read()
    assert not any(re.search(r"\+\s*b1\s*\*\s*\w+\s*\)\s*\+\s*b2", src) for src in (kern, reg))    # the (u, v) expression lives in coverage_kernels.h only


# ---- GPU -------------------------------------------------------------------------------------------------------------


def _plan(case):
    """wm_mosaic_plan through the C-ABI, every output pre-filled with a poison value."""
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    g = _up(case["g2p"]) if F else None
    s = _up(case["size"]) if F else None
    source = torch.full((gy, gx), -77, device=DEV, dtype=torch.int32)
    won = torch.full((F,), -7, device=DEV, dtype=torch.int32) if F else None
    stats = torch.full((2,), -7, device=DEV, dtype=torch.int64)
    N.check(N.lib().wm_mosaic_plan(N.ptr(g), N.ptr(s), F, case["x0"], case["y0"], case["cell"], gx, gy, N.ptr(source), N.ptr(won), N.ptr(stats),
                                   N.stream_ptr(torch.device(DEV))))
    return {"g": g, "s": s, "source_dev": source, "source": source.cpu().numpy().astype(np.int64),
            "won": won.cpu().numpy().astype(np.int64) if F else np.zeros(0, dtype=np.int64), "stats": stats.cpu().numpy()}


def _fill(case, plan, mode, picture, status, resident, flags=0, descs=None, slot=None):
    """One wm_mosaic_fill_u8 call with the frames `resident` (survey indices) on the device, in that order."""
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    tensors = [_up(case["images"][f]) for f in resident]
    if descs is None:
        descs = _frame_descs(tensors, torch.device(DEV)) if tensors else None
    if slot is None:
        slot = np.full(F, -1, dtype=np.int32)
        slot[list(resident)] = np.arange(len(resident), dtype=np.int32)
    slot_d = _up(slot) if F else None
    N.check(N.lib().wm_mosaic_fill_u8(N.ptr(descs), len(resident), N.ptr(slot_d), N.ptr(plan["g"]), N.ptr(plan["s"]), F, case["x0"], case["y0"],
                                      case["cell"], gx, gy, N.ptr(plan["source_dev"]), MODES[mode], flags, N.ptr(picture), N.ptr(status),
                                      N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return tensors


def _sentinel_picture(case):
    return _up(np.asarray(SENTINEL, dtype=np.uint8)).expand(case["gy"], case["gx"], 3).contiguous()


def _device(case):
    """The plan, and both pictures with every frame that has pixels resident in one call."""
    plan = _plan(case)
    out = {k: plan[k] for k in ("source", "won", "stats")}
    resident = [f for f, im in enumerate(case["images"]) if im is not None]
    for mode in MODES:
        pic, status = _sentinel_picture(case), torch.zeros(1, device=DEV, dtype=torch.int32)
        _fill(case, plan, mode, pic, status, resident)
        assert status.item() == 0, mode
        out[mode] = pic.cpu().numpy()
    return out, plan


def _assert_same(got, want):
    assert set(got) == set(want)
    for key in got:
        assert got[key].shape == want[key].shape, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def _run_and_check(case, want=None):
    want = _mosaic_oracle(case) if want is None else want
    got, plan = _device(case)
    _assert_same(got, want)
    assert got["stats"].sum() == case["gx"] * case["gy"] and got["won"].sum() == got["stats"][0]
    return got, want, plan


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEAM))
def test_gpu_seam_hand_cases(name):
    case, rows = SEAM[name]
    got, _, _ = _run_and_check(case)
    assert got["source"].tolist() == rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PIXEL))
def test_gpu_pixel_hand_cases(name):
    case, mode, rows = PIXEL[name]
    got, _, _ = _run_and_check(case)
    for m in ([mode] if mode else sorted(MODES)):
        assert got[m][:, :, 0].tolist() == rows, m


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_1x1", "grid_70x19", "grid_257x65", "no_frames", "one_1x1_px_frame", "past_one_chunk",
                                  "mixed_sizes_in_one_chunk"])
def test_gpu_smallest_shapes(name):
    case, want = _mosaic_gpu_case(name)
    got, _, _ = _run_and_check(case, want)
    src = got["source"]
    if name == "no_frames":
        assert (src == -1).all() and got["stats"].tolist() == [0, 70 * 19]
        assert (got["bilinear"] == np.asarray(SENTINEL, dtype=np.uint8)).all()
    if name == "one_1x1_px_frame":
        assert got["won"].tolist() == [30] and (got["bilinear"][src == 0] == case["images"][0][0, 0]).all()
    if name == "past_one_chunk":
        ch = _kernel_constants()["chunk"]
        assert case["g2p"].shape[0] == ch + 3
        np.testing.assert_array_equal(case["g2p"][ch], case["g2p"][10])            # the tie across the chunk boundary
        assert got["won"][10] > 0 and got["won"][ch] == 0 and got["won"][ch + 1] > 0 and got["won"][ch + 2] > 0
        both = dict(case, g2p=case["g2p"][[10, ch + 1]], size=case["size"][[10, ch + 1]], images=None)
        o = mosaic_oracle(both["g2p"], both["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"])
        assert (o["won"] > 0).all() and o["won"].sum() < (src >= 0).sum()         # frame 10 and the second chunk's frame share ground
        assert got["won"][:ch].sum() == got["won"][10]
    if name == "mixed_sizes_in_one_chunk":
        assert (got["won"] > 0).all() and len({tuple(s) for s in case["size"].tolist()}) == 5
    if name.startswith("grid_") and name != "grid_1x1":
        assert want["stats"][1] > 0 and (want["won"] > 0).sum() >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cull_tiny_frame", "cull_thin_between_rows", "cull_thin_on_one_row", "cull_yaw_45", "cover_all", "block_edges"])
def test_gpu_aimed_at_the_cull(name):
    case, want = _mosaic_gpu_case(name)
    got, _, _ = _run_and_check(case, want)
    src = got["source"]
    k = _kernel_constants()
    bx, by = k["block_x"], k["block_y"]
    if name == "cull_tiny_frame":
        assert (src >= 0).sum() == 1 and src[40, 100] == 0
    elif name == "cull_thin_between_rows":
        assert (src == -1).all()
    elif name == "cull_thin_on_one_row":
        assert (src >= 0).sum() == 257 and (src[40] == 0).all()
    elif name == "cull_yaw_45":
        assert 0 < (src >= 0).sum() < 1200 and (got["won"] > 0).all()
        blocks = {(j // by, i // bx) for j, i in zip(*np.nonzero(src >= 0))}
        assert 2 <= len(blocks) < ((257 + bx - 1) // bx) * ((65 + by - 1) // by)
    elif name == "cover_all":
        assert (src >= 0).all() and (got["won"] > 0).all() and got["stats"].tolist() == [257 * 65, 0]
    elif name == "block_edges":
        want_src = np.full((65, 257), -1, dtype=np.int64)
        want_src[by:2 * by, bx:2 * bx] = 0
        want_src[0:by, 0:bx] = 1
        want_src[by:2 * by, 2 * bx:4 * bx] = 2
        corner = src[by - 1:by + 1, bx - 1:bx + 1]
        want_src[by - 1:by + 1, bx - 1:bx + 1] = corner                            # decided by distance: the oracle's word
        np.testing.assert_array_equal(src, want_src)
        assert set(corner.ravel().tolist()) <= {0, 1, 3} and 3 in corner


@pytest.mark.gpu
def test_gpu_random_survey_invariants():
    case, want = _mosaic_gpu_case("random_survey")
    got, _, plan = _run_and_check(case, want)
    src = got["source"]
    F, gx, gy = 40, case["gx"], case["gy"]
    cov = torch.full((gy, gx), 0x7777, device=DEV, dtype=torch.int16)
    cstats = torch.empty(16, device=DEV, dtype=torch.int64)
    N.check(N.lib().wm_coverage_raster(N.ptr(plan["g"]), N.ptr(plan["s"]), F, case["x0"], case["y0"], case["cell"], gx, gy, N.ptr(cov), N.ptr(cstats),
                                       N.stream_ptr(torch.device(DEV))))
    cov = cov.cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(src >= 0, cov > 0)
    np.testing.assert_array_equal(got["won"], np.bincount(src[src >= 0], minlength=F))
    assert got["stats"].tolist() == [int((src >= 0).sum()), int((src == -1).sum())]
    assert got["stats"][1] > 0 and (cov >= 3).any() and (got["won"] > 0).sum() >= 30          # gaps, overlaps, many winners
    assert (got["nearest"] != got["bilinear"]).any()


@pytest.mark.gpu
def test_gpu_fill_is_order_free():
    case, want = _mosaic_gpu_case("random_survey")
    plan = _plan(case)
    src = plan["source"]
    sentinel = np.asarray(SENTINEL, dtype=np.uint8)
    for mode in MODES:
        pic, status = _sentinel_picture(case), torch.zeros(1, device=DEV, dtype=torch.int32)
        done = np.zeros(src.shape, dtype=bool)
        for f in range(39, -1, -1):                                               # one frame per call, descending
            _fill(case, plan, mode, pic, status, [f])
            done |= src == f
            now = pic.cpu().numpy()                                               # after EVERY call
            assert (now[~done] == sentinel).all(), f                             # every cell of a source not yet resident
            np.testing.assert_array_equal(now[done], want[mode][done], err_msg=str(f))
        assert status.item() == 0
        np.testing.assert_array_equal(pic.cpu().numpy(), want[mode])


@pytest.mark.gpu
def test_gpu_bad_residency_is_reported_and_skipped():
    case, want = _mosaic_gpu_case("mixed_sizes_in_one_chunk")
    plan = _plan(case)
    src = plan["source"]
    sentinel = np.asarray(SENTINEL, dtype=np.uint8)
    F = case["g2p"].shape[0]
    good = np.arange(F, dtype=np.int32)

    def run(slot, images=None):
        c = dict(case, images=images or case["images"])
        pic, status = _sentinel_picture(case), torch.zeros(1, device=DEV, dtype=torch.int32)
        _fill(c, plan, "bilinear", pic, status, list(range(F)), slot=slot)
        return pic.cpu().numpy(), status.item()

    # frame 2's slot points past the resident list
    slot = good.copy()
    slot[2] = F
    pic, status = run(slot)
    assert status == N.MOSAIC_BAD_SLOT
    assert (pic[src == 2] == sentinel).all() and (src == 2).any()
    np.testing.assert_array_equal(pic[src != 2], want["bilinear"][src != 2])
    # frame 1's slot holds frame 3's descriptor (a smaller frame: its size is not size_dev[1]); frame 3 itself is fine
    slot = good.copy()
    slot[1] = 3
    pic, status = run(slot)
    assert status == N.MOSAIC_BAD_SIZE
    assert (pic[src == 1] == sentinel).all() and (src == 1).any()
    np.testing.assert_array_equal(pic[src != 1], want["bilinear"][src != 1])
    # a resident frame one row short of what size_dev says
    images = list(case["images"])
    images[0] = images[0][:-1].copy()
    pic, status = run(good, images)
    assert status == N.MOSAIC_BAD_SIZE and (pic[src == 0] == sentinel).all()
    # both at once; a negative slot is simply not resident
    slot = good.copy()
    slot[2], slot[1], slot[4] = F + 5, 3, -1
    pic, status = run(slot)
    assert status == N.MOSAIC_BAD_SLOT | N.MOSAIC_BAD_SIZE
    assert (pic[(src == 1) | (src == 2) | (src == 4) | (src == -1)] == sentinel).all()
    # a source raster that is not the plan's: a frame index past the survey, and a frame that does not see the cell
    bogus = dict(plan, source_dev=plan["source_dev"].clone())
    bogus["source_dev"][0, 0] = F
    far = np.argwhere(src == -1)[0]
    bogus["source_dev"][far[0], far[1]] = 0
    pic2, st2 = _sentinel_picture(case), torch.zeros(1, device=DEV, dtype=torch.int32)
    _fill(case, bogus, "nearest", pic2, st2, list(range(F)))
    assert st2.item() == N.MOSAIC_BAD_SOURCE
    pic2 = pic2.cpu().numpy()
    assert (pic2[0, 0] == sentinel).all() and (pic2[far[0], far[1]] == sentinel).all()


@pytest.mark.gpu
def test_gpu_north_up_flips_the_picture_only():
    case, want = _mosaic_gpu_case("grid_70x19")
    plan = _plan(case)
    before = plan["source_dev"].clone()
    resident = [f for f, im in enumerate(case["images"]) if im is not None]
    for mode in MODES:
        pic, status = _sentinel_picture(case), torch.zeros(1, device=DEV, dtype=torch.int32)
        _fill(case, plan, mode, pic, status, resident, flags=N.MOSAIC_NORTH_UP)
        assert status.item() == 0
        np.testing.assert_array_equal(pic.cpu().numpy(), want[mode][::-1])
        np.testing.assert_array_equal(pic.flip(0).cpu().numpy(), want[mode])
    assert torch.equal(plan["source_dev"], before)
    np.testing.assert_array_equal(before.cpu().numpy(), want["source"])


PLAN_KEYS = {"source", "won", "origin", "cell", "shape", "gap_cells"}


@pytest.mark.gpu
def test_gpu_python_mosaic_end_to_end():
    georef, sizes, images = _mosaic_python_case()
    cell, fill = 0.08, (9, 8, 250)
    x0, y0, gx, gy = tiling.footprint_bounds(georef, sizes, cell)
    g2p = tiling.ground_to_pixel(georef)
    want = mosaic_oracle(g2p, sizes, x0, y0, cell, gx, gy, images, fill)
    mixed = [images[0], torch.from_numpy(images[1]), torch.from_numpy(images[2]).to(DEV), images[3]]          # numpy, host, device
    plan = tiling.mosaic_plan(georef, sizes, cell)
    assert set(plan) == PLAN_KEYS and plan["source"].dtype == torch.int32 and plan["won"].dtype == torch.int64
    np.testing.assert_array_equal(plan["source"].cpu().numpy(), want["source"])
    np.testing.assert_array_equal(plan["won"].cpu().numpy(), want["won"])
    assert plan["origin"] == (x0, y0) and plan["cell"] == cell and plan["shape"] == (gy, gx)
    assert plan["gap_cells"] == int(want["stats"][1]) > 0 and isinstance(plan["gap_cells"], int)
    for sample in MODES:
        out = tiling.mosaic(mixed, georef, cell, sample=sample, fill=fill)                                      # sizes from the shapes
        assert set(out) == PLAN_KEYS | {"mosaic", "north_up"} and out["north_up"] is True
        assert out["mosaic"].dtype == torch.uint8 and out["mosaic"].is_cuda and tuple(out["mosaic"].shape) == (gy, gx, 3)
        np.testing.assert_array_equal(out["mosaic"].cpu().numpy(), want[sample][::-1])
        np.testing.assert_array_equal(out["source"].cpu().numpy(), want["source"])                             # never flipped
        south = tiling.mosaic(mixed, georef, cell, sizes=sizes, sample=sample, fill=fill, north_up=False, chunk=1)
        np.testing.assert_array_equal(south["mosaic"].cpu().numpy(), want[sample])
        assert south["north_up"] is False
    gaps = want["source"] == -1
    assert (out["mosaic"].flip(0).cpu().numpy()[gaps] == np.asarray(fill, dtype=np.uint8)).all() and gaps.any()
    assert tiling.mosaic(mixed, georef, cell)["mosaic"].cpu().numpy()[::-1][gaps].max() == 0                   # the default fill is black

    # a lazy sequence over a corner of the survey: frame 3 (off to the east) wins nothing there and is never asked for
    bounds = (x0, y0, 150, gy)
    want_b = mosaic_oracle(g2p, sizes, x0, y0, cell, 150, gy, images, fill)
    assert want_b["won"][3] == 0 and (want_b["won"][:3] > 0).all() and want["won"][3] > 0
    for chunk in (1, 2, 8):
        lazy = _Lazy(mixed)
        out = tiling.mosaic(lazy, georef, cell, sizes=sizes, bounds=bounds, fill=fill, chunk=chunk)
        assert lazy.asked == [0, 1, 2], chunk
        np.testing.assert_array_equal(out["mosaic"].cpu().numpy(), want_b["bilinear"][::-1])
        assert out["shape"] == (gy, 150) and out["gap_cells"] == int(want_b["stats"][1])
    # a frame whose shape is not what sizes says is named, before its chunk is launched
    wrong = list(mixed)
    wrong[1] = images[1][:, :-1].copy()
    with pytest.raises(ValueError, match="frame 1 is"):
        tiling.mosaic(_Lazy(wrong), georef, cell, sizes=sizes, fill=fill)
    wrong[1] = images[1].astype(np.float32)
    with pytest.raises(RuntimeError, match="^mosaic: frame 1: expected"):
        tiling.mosaic(_Lazy(wrong), georef, cell, sizes=sizes, fill=fill)
    # no frames at all: a 1 x 1 grid of the fill colour
    out = tiling.mosaic([], np.zeros((0, 2, 3)), 1.0, fill=fill)
    assert out["shape"] == (1, 1) and out["mosaic"].cpu().tolist() == [[list(fill)]] and out["gap_cells"] == 1 and tuple(out["won"].shape) == (0,)


@pytest.mark.gpu
def test_gpu_python_mosaic_markers():
    georef, sizes, images = _mosaic_python_case()
    cell = 0.08
    x0, y0, gx, gy = tiling.footprint_bounds(georef, sizes, cell)
    pts = np.array([[x0 + 5.0, y0 + 3.0], [x0 + 0.04, y0 + 0.04], [NAN, y0 + 1.0], [x0 - 0.5, y0 + 1.0], [x0 + 2.0, y0 + gy * cell + 0.01],
                    [x0 + 8.26, y0 + 4.1], [x0 + 3.0, INF], [x0 + gx * cell - 0.01, y0 + gy * cell - 0.01]])
    labels = np.array([0, 3, 1, 1, 2, 6, 2, 99])                                 # 99: outside the palette, draws nothing
    cen = {"points": torch.from_numpy(pts).to(DEV), "labels": torch.from_numpy(labels).to(DEV)}
    plain = tiling.mosaic(images, georef, cell)
    for north_up in (True, False):
        out = tiling.mosaic(images, georef, cell, north_up=north_up, census=cen, marker=9, width=2)
        assert set(out) == PLAN_KEYS | {"mosaic", "north_up", "marker_boxes", "marker_index"}
        assert out["marker_index"].cpu().tolist() == [0, 1, 5, 7]                   # finite and inside the grid
        boxes = out["marker_boxes"]
        assert boxes.dtype == torch.float32 and tuple(boxes.shape) == (4, 4) and boxes.is_cuda
        cx, cy = (pts[[0, 1, 5, 7], 0] - x0) / cell, (pts[[0, 1, 5, 7], 1] - y0) / cell
        cy = gy - cy if north_up else cy
        np.testing.assert_array_equal(boxes.cpu().numpy(), np.stack([cx - 4.5, cy - 4.5, cx + 4.5, cy + 4.5], axis=1).astype(np.float32))
        base = tiling.mosaic(images, georef, cell, north_up=north_up)["mosaic"]
        drawn = tiling.draw_boxes(base.clone(), boxes, cen["labels"][out["marker_index"]], width=2)
        assert torch.equal(out["mosaic"], drawn)
        changed = (out["mosaic"] != base).any(dim=2)
        assert 0 < int(changed.sum()) <= 3 * (100 - 36)                           # three outlines at most 10 x 10 with a 6 x 6 hole; the fourth has no colour
    assert torch.equal(plain["mosaic"], tiling.mosaic(images, georef, cell)["mosaic"])
    # a census without individuals in the grid draws nothing
    none = {"points": cen["points"][[2, 3, 6]], "labels": cen["labels"][[2, 3, 6]]}
    out = tiling.mosaic(images, georef, cell, census=none, marker=3)
    assert tuple(out["marker_boxes"].shape) == (0, 4) and torch.equal(out["mosaic"], plain["mosaic"])
