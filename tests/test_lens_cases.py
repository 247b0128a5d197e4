"""Survey lens on the CPU: the rule's restatement (tests/lens_cases.py: lens_oracle) held against what a lens correction must
do -- identity, direction, teeth against seven wrong rules -- and the host layer (wildlifemapper_amd.lens: lens_plan,
distort_points, undistort_points, lens_points) and the argument checks of wm_undistort_u8 held against the restatement.
The device is held against the same restatement in tests/test_lens.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lens_cases as LC
from survey_util import ROOT, _lib
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import lens, preprocess, tiling


def test_identity_returns_the_frame_byte_for_byte():
    """Zero coefficients, f_out = fx = fy and the principal point at the centre: the input, in both modes, nothing filled.
    The focal lengths are not dyadic, so x / f * f is not exact; the sample still lands on the pixel centre's own pixel
    (nearest) and within 2^-40 px of it (bilinear: weights whose product with 255 rounds away)."""
    for k, size in enumerate(LC.IDENTITY_SIZES):
        f = 0.83 * size[1] + 0.1 * k
        cam = LC.camera(size, f=f)
        img = np.random.default_rng(k).integers(0, 256, (*size, 3), dtype=np.uint8)
        got = LC.lens_oracle(img, cam, size, f)
        assert got["filled"] == 0, size
        for m in LC.MODES:
            assert np.array_equal(got[m], img), (size, m)
        assert lens.lens_plan(cam, size)["out_size"] == size            # and keep='valid' of the identity is the frame


def _line_distance(pts, a, b):
    """Distance of the points (n,2) from the line through a and b."""
    d = (b - a) / np.hypot(*(b - a))
    r = pts - a
    return np.abs(r[:, 0] * d[1] - r[:, 1] * d[0])


def test_direction_a_straight_line_comes_out_straight():
    """A straight world line, drawn into the raw frame through distort_points (the closed form), is straight again in the
    undistorted picture: every bright pixel within 2 px of the true line.  With the restatement and these three lines the
    right camera gives at most 1.22 px, zeroed coefficients 9.1-16.6 px and flipped signs 14.6-26.1 px, so the bound cannot
    hide a wrong direction."""
    size, f = (240, 320), 260.0
    cam = LC.camera(size, f=f, **LC.FIVE)
    cu, cv = cam[2] + 0.5, cam[3] + 0.5
    lines = [((-150.0, -100.0), (150.0, -60.0)), ((-150.0, 100.0), (150.0, 70.0)), ((130.0, -110.0), (145.0, 110.0))]   # px from the centre
    worst = {}
    for n, (a, b) in enumerate(lines):
        a, b = np.array(a), np.array(b)
        t = np.linspace(0.0, 1.0, 4000)[:, None]
        raw = lens.distort_points(cam, (a + t * (b - a)) + np.array([cu, cv]))        # pinhole positions of the same intrinsics
        img = np.zeros((*size, 3), dtype=np.uint8)
        ok = (raw[:, 0] >= 0) & (raw[:, 0] < size[1]) & (raw[:, 1] >= 0) & (raw[:, 1] < size[0])
        assert ok.sum() > 2000                                            # most of the line is in the frame
        img[np.floor(raw[ok, 1]).astype(int), np.floor(raw[ok, 0]).astype(int)] = 255
        for name, c in (("right", cam), ("zeroed", LC.camera(size, f=f)), ("flipped", np.concatenate([cam[:4], -cam[4:]]))):
            pic = LC.lens_oracle(img, c, size, f, modes=("nearest",))["nearest"]
            jj, ii = np.nonzero(pic[..., 0] == 255)
            assert len(jj) > 100, (n, name)                               # a line, not a few stray pixels
            pos = np.stack([(ii + 0.5) - 0.5 * size[1], (jj + 0.5) - 0.5 * size[0]], axis=1)        # px from the picture's centre
            worst[(n, name)] = _line_distance(pos, a, b).max()
    print("direction: worst distance from the true line, px:", {k: round(float(v), 2) for k, v in worst.items()})
    for n in range(len(lines)):
        assert worst[(n, "right")] <= 2.0, worst
        assert worst[(n, "zeroed")] > 2.0 and worst[(n, "flipped")] > 2.0, worst      # the same bound refuses the wrong cameras


def test_every_mutant_changes_a_byte():
    """Each deliberately wrong rule differs from the right one in at least one byte of at least one case."""
    caught = {}
    for mutant in LC.MUTANTS:
        for name in LC.CASE_NAMES:
            pl, img, want = LC.expected(name)
            got = LC.lens_oracle(img, pl["camera"], pl["out_size"], pl["f_out"], mutant=mutant)
            if any(not np.array_equal(got[m], want[m]) for m in LC.MODES):
                caught[mutant] = name
                break
    assert set(caught) == set(LC.MUTANTS), sorted(set(LC.MUTANTS) - set(caught))


def test_cases_cover_the_sizes_the_kernel_branches_on():
    sizes = {tuple(LC.expected(n)[0]["out_size"]) for n in LC.CASE_NAMES}
    assert {s[1] for s in sizes} >= set(LC.OUT_WIDTHS) and {s[0] for s in sizes} >= set(LC.OUT_HEIGHTS)
    assert {c["size"] for c in LC.CASES} == set(LC.SOURCE_SIZES)
    assert any(3 * ow % 4 for _, ow in sizes) and any(ow > 64 and ow % 64 for _, ow in sizes) and any(oh % 16 for oh, _ in sizes)


def test_keep_all_cases_both_fill_and_fetch():
    """Over the keep='all' cases with distortion, filled and fetched pixels are each at least 5 % of the output."""
    names = [c["name"] for c in LC.CASES if c["keep"] == "all"]
    assert len(names) >= 3
    for name in names:
        pl, _, want = LC.expected(name)
        total = pl["out_size"][0] * pl["out_size"][1]
        print(name, pl["out_size"], "filled", want["filled"], "of", total)
        assert want["filled"] >= 0.05 * total and total - want["filled"] >= 0.05 * total, (name, want["filled"], total)


def test_keep_valid_is_the_largest_picture_without_a_filled_pixel():
    names = [c["name"] for c in LC.CASES if c["keep"] == "valid"]
    assert len(names) >= 3
    for name in names:
        pl, img, want = LC.expected(name)
        oh, ow = pl["out_size"]
        assert want["filled"] == 0, name
        for grown in ((oh + 2, ow), (oh, ow + 2)):
            assert LC.lens_oracle(img, pl["camera"], grown, pl["f_out"], modes=())["filled"] >= 1, (name, grown)


def test_keep_all_holds_every_border_pixel_of_the_frame():
    for name in [c["name"] for c in LC.CASES if c["keep"] == "all"]:
        pl = LC.expected(name)[0]
        (h, w), (oh, ow) = pl["size"], pl["out_size"]
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        border = (jj == 0) | (jj == h - 1) | (ii == 0) | (ii == w - 1)
        pts = np.stack([ii[border] + 0.5, jj[border] + 0.5], axis=1)
        got = lens.lens_points(pl, pts, to="undistorted")
        assert np.isfinite(got).all(), name
        assert (got[:, 0] >= 0).all() and (got[:, 0] < ow).all() and (got[:, 1] >= 0).all() and (got[:, 1] < oh).all(), name
        # and it is the smallest: a picture two pixels narrower or lower loses one
        assert got[:, 0].min() < 1 or got[:, 0].max() >= ow - 1, name
        assert got[:, 1].min() < 1 or got[:, 1].max() >= oh - 1, name


def test_points_round_trip():
    """distort(undistort(p)) == p within 1e-9 px on a grid over each case's frame, and through a plan's geometry too."""
    for c in LC.CASES:
        h, w = c["size"]
        xs, ys = np.meshgrid(np.linspace(0, w, 23), np.linspace(0, h, 19))
        p = np.stack([xs.ravel(), ys.ravel()], axis=1)
        q = lens.undistort_points(c["camera"], p)
        assert np.isfinite(q).all(), c["name"]
        assert np.abs(lens.distort_points(c["camera"], q) - p).max() <= 1e-9, c["name"]
        pl = LC.expected(c["name"])[0]
        back = lens.lens_points(pl, lens.lens_points(pl, p, to="undistorted"), to="raw")
        assert np.abs(back - p).max() <= 1e-9, c["name"]


def test_lens_points_raw_is_the_rule_at_pixel_centres():
    """to='raw' of a pixel centre is the kernel's (u, v): nearest sampling through it reproduces the oracle's picture."""
    pl, img, want = LC.expected("five_33x129")
    oh, ow = pl["out_size"]
    jj, ii = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    uv = lens.lens_points(pl, np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], axis=1), to="raw")
    h, w = pl["size"]
    sees = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    pic = np.empty((oh * ow, 3), np.uint8)
    pic[:] = LC.FILL
    pic[sees] = img[np.floor(uv[sees, 1]).astype(int), np.floor(uv[sees, 0]).astype(int)]
    assert np.array_equal(pic.reshape(oh, ow, 3), want["nearest"])


def test_a_folding_camera_raises():
    size = (240, 320)
    cam = LC.camera(size, f=260.0, k1=-2.0)
    for kw in (dict(keep="valid"), dict(keep="all"), dict(out_size=size)):
        with pytest.raises(ValueError, match="folds over"):
            lens.lens_plan(cam, size, **kw)
    lens.lens_plan(cam, size, out_size=(120, 160))                        # inside the fold radius (106 px) the model is a lens
    assert np.isnan(lens.undistort_points(cam, [[0.5, 0.5]])).all()       # the corner has no undistorted position


def test_lens_plan_rejects_bad_arguments():
    size, cam = (37, 53), LC.camera((37, 53), **LC.BARREL)
    bad_cam = lambda k, v: np.concatenate([cam[:k], [v], cam[k + 1:]])
    for args, kw, msg in [
            ((cam[:8], size), {}, "expected 9 numbers"), (("abc", size), {}, "not an array of numbers"),
            ((bad_cam(4, np.nan), size), {}, "camera k1"), ((bad_cam(0, 0.0), size), {}, "camera fx"),
            ((bad_cam(1, -3.0), size), {}, "camera fy"), ((bad_cam(2, np.inf), size), {}, "camera cx"),
            ((cam, (37,)), {}, "expected (height, width)"), ((cam, (0, 53)), {}, "size height"), ((cam, (37, 65537)), {}, "size width"),
            ((cam, (37.5, 53)), {}, "size height"), ((cam, size), dict(keep="most"), "keep"), ((cam, size), dict(f_out=0.0), "f_out"),
            ((cam, size), dict(f_out=float("nan")), "f_out"), ((cam, size), dict(f_out="x"), "f_out"),
            ((cam, size), dict(out_size=(0, 5)), "out_size height"), ((cam, size), dict(out_size=(5, True)), "out_size width")]:
        with pytest.raises(ValueError, match=re.escape(msg)):
            lens.lens_plan(*args, **kw)
    with pytest.raises(ValueError, match="empty"):                        # the principal point is outside the frame
        lens.lens_plan(LC.camera(size, off=(40.0, 0.0)), size, keep="valid")
    pl = lens.lens_plan(cam, size, out_size=(10, 12), f_out=30.0)
    assert pl["out_size"] == (10, 12) and pl["f_out"] == 30.0 and pl["size"] == size and np.array_equal(pl["camera"], cam)
    assert lens.lens_plan(cam, size)["f_out"] == cam[0]                   # f_out defaults to fx
    assert tiling.lens_plan is lens.lens_plan and tiling.undistorted is lens.undistorted and tiling.lens_points is lens.lens_points


def test_lens_points_and_wrappers_reject_bad_arguments():
    pl = LC.expected("valid_barrel")[0]
    for args, kw, msg in [((pl, np.zeros((3, 3))), {}, "expected (n, 2)"), ((pl, "abc"), {}, "not an array of numbers"),
                          ((pl, np.zeros((3, 2))), dict(to="up"), "to 'up'"), (({"camera": pl["camera"]}, np.zeros((3, 2))), {}, "plan must be"),
                          ((dict(pl, f_out=-1.0), np.zeros((3, 2))), {}, "f_out"), ((dict(pl, out_size=(0, 4)), np.zeros((3, 2))), {}, "out_size")]:
        with pytest.raises(ValueError, match=re.escape(msg)):
            lens.lens_points(*args, **kw)
    assert lens.lens_points(pl, np.zeros((0, 2))).shape == (0, 2)
    for f in (lens.distort_points, lens.undistort_points):
        with pytest.raises(ValueError, match="expected"):
            f(pl["camera"], np.zeros(5))
        with pytest.raises(ValueError, match="expected 9 numbers"):
            f(np.zeros(4), np.zeros((1, 2)))
    frames = [np.zeros((37, 53, 3), np.uint8)]
    for args, kw, msg in [((iter(frames), pl), {}, "sequence"), ((frames, {"size": 1}), {}, "plan must be"),
                          ((frames, pl), dict(sample="cubic"), "sample"), ((frames, pl), dict(fill=(1, 2)), "fill"),
                          ((frames, pl), dict(fill=(1, 2, 256)), "fill")]:
        with pytest.raises(ValueError, match=msg):
            tiling.undistorted(*args, **kw)
    u = tiling.undistorted(frames * 3, pl)                                # no device work: nothing is indexed yet
    assert len(u) == 3 and u.sizes.shape == (3, 2) and u.sizes.dtype == np.int64 and (u.sizes == pl["out_size"]).all()
    with pytest.raises(IndexError):
        u[3]
    import torch
    with pytest.raises(ValueError, match="plan must be"):
        preprocess.undistort_u8(torch.zeros((37, 53, 3), dtype=torch.uint8), {})
    with pytest.raises(RuntimeError, match="ROCm tensor"):              # a host tensor is refused, not processed on the host
        preprocess.undistort_u8(torch.zeros((37, 53, 3), dtype=torch.uint8), pl)


def test_undistort_abi_rejects_bad_arguments():
    L = _lib()
    p, q = C.c_void_p(1 << 20), C.c_void_p(1 << 24)      # never dereferenced: every call below fails validation before any HIP call
    cam = lambda **kw: (C.c_double * 9)(*[kw.get(n, v) for n, v in zip(lens.CAMERA_ENTRIES, (50.0, 50.0, 26.0, 18.0, -0.1, 0.0, 0.0, 0.0, 0.0))])
    fill = (C.c_uint8 * 3)(9, 8, 7)
    ok = dict(in_dev=p, height=37, width=53, camera=cam(), out_dev=q, out_height=30, out_width=40, f_out=50.0, mode=N.MOSAIC_BILINEAR,
              fill_rgb=fill, stats_dev=None)
    nan, inf = float("nan"), float("inf")
    for change, msg in [(dict(in_dev=None), b"null in_dev"), (dict(out_dev=None), b"null out_dev"), (dict(camera=None), b"null camera"),
                        (dict(fill_rgb=None), b"null fill_rgb"), (dict(height=0), b"1..65536"), (dict(width=65537), b"1..65536"),
                        (dict(out_height=-1), b"1..65536"), (dict(out_width=0), b"1..65536"), (dict(out_width=65537), b"1..65536"),
                        (dict(camera=cam(k1=nan)), b"camera k1"), (dict(camera=cam(cx=inf)), b"camera cx"), (dict(camera=cam(k3=-inf)), b"camera k3"),
                        (dict(camera=cam(p2=nan)), b"camera p2"), (dict(camera=cam(fx=0.0)), b"camera fx"), (dict(camera=cam(fy=-1.0)), b"camera fy"),
                        (dict(camera=cam(fx=nan)), b"camera fx"), (dict(f_out=0.0), b"f_out"), (dict(f_out=-2.0), b"f_out"), (dict(f_out=nan), b"f_out"),
                        (dict(f_out=inf), b"f_out"), (dict(mode=2), b"mode 2"), (dict(mode=-1), b"mode -1"),
                        (dict(stats_dev=C.c_void_p(12)), b"stats_dev"), (dict(out_dev=p), b"overlap"),
                        (dict(out_dev=C.c_void_p((1 << 20) + 37 * 53 * 3 - 1)), b"overlap"),
                        (dict(out_dev=C.c_void_p((1 << 20) - 30 * 40 * 3 + 1)), b"overlap")]:
        a = dict(ok, **change)
        assert L.wm_undistort_u8(*a.values(), None) < 0, change
        assert msg in L.wm_last_error(), (change, L.wm_last_error())


def test_abi_version_and_export():
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    assert int(re.search(r"#define WM_ABI_VERSION (\d+)", hdr).group(1)) == 13 == N.ABI_VERSION == _lib().wm_abi_version()
    assert "wm_undistort_u8" in N.SYMBOLS and hasattr(_lib(), "wm_undistort_u8")
    assert re.search(r"\bint wm_undistort_u8\(", hdr) and "13, also additive: wm_undistort_u8" in hdr


def test_kernel_includes_the_ground_rules_it_shares():
    """From the sources: the inside test, the sampling and the row store are the mosaic's, included, not copied."""
    csrc = os.path.join(ROOT, "wildlifemapper_amd", "csrc")
    kern = open(os.path.join(csrc, "lens_kernels.h")).read()
    assert '#include "mosaic_kernels.h"' in kern
    for shared in ("cov_inside(", "mos_sample<MODE>(", "mos_store_row("):
        assert shared in kern, shared
    assert "fp contract(off)" in kern and "floor(" not in kern and "atomicAdd(stats" in kern
    everything = "\n".join(open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip")))
    assert len(re.findall(r"void mos_sample\(", everything)) == 1 and len(re.findall(r"void mos_store_row\(", everything)) == 1
