"""Survey attitude on the GPU: wm_rectify_u8 equals the rule's restatement (tests/attitude_cases.py: attitude_oracle) byte for
byte, with the filled count, for every case in both modes at every byte offset of the output; with the identity rotation it
equals wm_undistort_u8's own output on every lens case; and preprocess.rectify_u8 and tiling.rectified hand those bytes to
mosaic unchanged.  The census at the end is wrong without the feature and exact with it.  The cases, the oracle, the mutants
and the CPU proof that the census scene is what it claims are in tests/attitude_cases.py and tests/test_attitude_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import attitude_cases as AC
import lens_cases as LC
from survey_util import DEV, _guarded, _Lazy, _lib, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import preprocess, tiling

pytestmark = pytest.mark.gpu
MODE = {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}


def _rectify_at(pl, img, mode, out_off, in_off, fill=AC.FILL, out_buf=None):
    """wm_rectify_u8 -- wm_undistort_u8 for a plan without a rotation -- with the input in_off and the output out_off bytes past
    an aligned allocation, both inside guard bytes (survey_util._guarded: 255 all round).  Returns (picture, filled, the
    output's whole buffer)."""
    lib = _lib()
    (h, w), (oh, ow) = pl["size"], pl["out_size"]
    _, src = _guarded(img, in_off, DEV)
    if out_buf is None:
        out_buf = _guarded(np.full((oh, ow, 3), 171, np.uint8), out_off, DEV)[0]
    stats = torch.full((1,), -5, dtype=torch.int64, device=DEV)
    cam = (C.c_double * 9)(*np.asarray(pl["camera"]).tolist())
    tail = (C.c_void_p(out_buf.data_ptr() + out_off), oh, ow, pl["f_out"], MODE[mode], (C.c_uint8 * 3)(*fill), N.ptr(stats), N.stream_ptr(torch.device(DEV)))
    if "rotation" in pl:
        rot = (C.c_double * 9)(*np.asarray(pl["rotation"]).reshape(9).tolist())
        N.check(lib.wm_rectify_u8(C.c_void_p(src.data_ptr()), h, w, cam, rot, *tail))
    else:
        N.check(lib.wm_undistort_u8(C.c_void_p(src.data_ptr()), h, w, cam, *tail))
    got = out_buf.cpu().numpy()
    n = oh * ow * 3
    assert (got[:out_off] == 255).all() and (got[out_off + n:] == 255).all(), "the kernel wrote outside its output"
    return got[out_off:out_off + n].reshape(oh, ow, 3), int(stats.item()), out_buf


@pytest.mark.parametrize("name", AC.CASE_NAMES)
def test_rectify_equals_the_oracle_byte_for_byte(name):
    pl, img, want = AC.expected(name)
    for mode in AC.MODES:
        for off in range(4):                                              # the output 0..3 bytes past a dword; the input offset too
            got, filled, _ = _rectify_at(pl, img, mode, off, (off + 1) % 4)
            diff = int((got != want[mode]).sum())
            assert diff == 0, (name, mode, off, diff, np.argwhere((got != want[mode]).any(axis=2))[:4].tolist())
            assert filled == want["filled"], (name, mode, off)


def test_identity_rotation_equals_undistort_on_every_lens_case():
    """With rot the identity the rule is wm_undistort_u8's: the existing kernel is an independent check of the new one."""
    for name in LC.CASE_NAMES:
        pl, img, _ = LC.expected(name)
        for mode in LC.MODES:
            want, want_filled, _ = _rectify_at(pl, img, mode, 1, 2, fill=LC.FILL)
            got, filled, _ = _rectify_at(dict(pl, rotation=AC.IDENTITY), img, mode, 1, 2, fill=LC.FILL)
            assert np.array_equal(got, want) and filled == want_filled, (name, mode)


def test_quarter_turn_through_the_kernel_is_rot90():
    pl, img, _ = AC.expected("quarter_turn_32x32")
    for mode in AC.MODES:
        got, filled, _ = _rectify_at(pl, img, mode, 0, 0)
        assert np.array_equal(got, np.rot90(img, 1)) and filled == 0, mode


def test_a_second_call_overwrites_every_byte():
    for name in ("all_both_five", AC.Z_CASE):
        pl, img, want = AC.expected(name)
        for mode in AC.MODES:
            _, _, buf = _rectify_at(pl, img, mode, 1, 0, fill=(200, 100, 50))
            got, filled, _ = _rectify_at(pl, img, mode, 1, 0, out_buf=buf)
            assert np.array_equal(got, want[mode]) and filled == want["filled"], (name, mode)


def test_no_stats_pointer_is_accepted():
    pl, img, want = AC.expected("both_five_33x65")
    out = torch.empty((*pl["out_size"], 3), dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(img).to(DEV)
    N.check(_lib().wm_rectify_u8(N.ptr(src), *pl["size"], (C.c_double * 9)(*pl["camera"].tolist()), (C.c_double * 9)(*pl["rotation"].reshape(9).tolist()),
                                 N.ptr(out), *pl["out_size"], pl["f_out"], N.MOSAIC_BILINEAR, (C.c_uint8 * 3)(*AC.FILL), None,
                                 N.stream_ptr(torch.device(DEV))))
    assert np.array_equal(out.cpu().numpy(), want["bilinear"])


def _per_frame():
    """Three frames of one camera and size, each with its own attitude: (camera, size, rotations (3,2), frames, oracle dicts)."""
    size = (64, 129)
    cam = LC.camera(size, **LC.FIVE)
    rots = np.array([(4.0, 3.0), (-5.0, 5.0), (0.0, -6.0)])
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (*size, 3), dtype=np.uint8) for _ in rots]
    return cam, size, rots, frames


def test_wrappers_return_the_oracles_bytes():
    """preprocess.rectify_u8 and tiling.rectified, device and host frames, a plan and a size per frame; a lazy source is
    indexed once per access."""
    _lib()
    pl, img, want = AC.expected("all_both_five")
    dev_frame = torch.from_numpy(img).to(DEV)
    for mode in AC.MODES:
        got, filled = preprocess.rectify_u8(dev_frame, pl, sample=mode, fill=AC.FILL, count=True)
        assert got.shape == (*pl["out_size"], 3) and got.dtype == torch.uint8 and got.device == dev_frame.device
        assert filled.dtype == torch.int64 and filled.is_cuda and int(filled.item()) == want["filled"]
        assert np.array_equal(got.cpu().numpy(), want[mode]), mode
    assert np.array_equal(preprocess.rectify_u8(dev_frame, pl, fill=AC.FILL).cpu().numpy(), want["bilinear"])
    with pytest.raises(ValueError, match="the plan was made for"):
        preprocess.rectify_u8(dev_frame[:-1], pl)
    cam, size, rots, frames = _per_frame()
    src = _Lazy([torch.from_numpy(frames[0]).to(DEV), frames[1], torch.from_numpy(frames[2])])       # a device tensor, a numpy array, a CPU tensor
    r = tiling.rectified(src, cam, rots, keep="all", sample="nearest", fill=AC.FILL, size=size)
    assert len(r) == 3 and src.asked == [] and r.sizes.shape == (3, 2) and len({tuple(s) for s in r.sizes}) == 3
    wants = [AC.attitude_oracle(f, cam, p["rotation"], p["out_size"], p["f_out"], modes=("nearest",))["nearest"] for f, p in zip(frames, r.plans)]
    for i in (2, 0, 1):
        got = r[i]
        assert got.is_cuda and tuple(got.shape[:2]) == tuple(r.sizes[i]) and np.array_equal(got.cpu().numpy(), wants[i]), i
    assert src.asked == [2, 0, 1]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(r, wants)) and src.asked == [2, 0, 1, 0, 1, 2]
    same = tiling.rectified(frames, cam, tiling.attitude_rotation(rots[:, 0], rots[:, 1]), keep="all", size=size)      # (n, 3, 3)
    assert np.array_equal(same.sizes, r.sizes)
    with pytest.raises(ValueError, match="the plan was made for"):
        tiling.rectified([frames[0][:, :-1]], cam, rots[:1], size=size)[0]


def test_mosaic_of_rectified_frames_equals_mosaic_of_the_oracles_pictures():
    _lib()
    cam, size, rots, frames = _per_frame()
    src = _Lazy(frames)
    r = tiling.rectified(src, cam, rots, keep="valid", sample="bilinear", size=size)
    georef = np.stack([tiling.nadir_affine(oh, ow, (100.0 + 25.0 * k, 200.0 + 9.0 * k), 0.5, 20.0 * k) for k, (oh, ow) in enumerate(r.sizes)])
    got = tiling.mosaic(r, georef, 0.4, sizes=r.sizes)
    pictures = [AC.attitude_oracle(f, cam, p["rotation"], p["out_size"], p["f_out"], fill=(0, 0, 0), modes=("bilinear",))["bilinear"]
                for f, p in zip(frames, r.plans)]
    want = tiling.mosaic(pictures, georef, 0.4)
    assert torch.equal(got["mosaic"], want["mosaic"]) and torch.equal(got["source"], want["source"])
    assert sorted(src.asked) == torch.nonzero(want["won"] > 0).flatten().tolist() and len(src.asked) >= 2       # the winners, once each


def _census_results(centres):
    """One detect_frames-like result per frame: a 6 x 6 px box about each centre (n,2)."""
    out = []
    for c in centres:
        boxes = np.concatenate([c - 3.0, c + 3.0], axis=1).astype(np.float32)
        out.append({"boxes": _up(boxes), "scores": _up(np.linspace(0.9, 0.5, len(c)).astype(np.float32)),
                    "labels": torch.ones(len(c), device=DEV, dtype=torch.int64)})
    return out


def test_census_counts_each_animal_once_only_after_the_attitude_correction():
    """Two frames banked opposite ways over a dozen animals (attitude_cases.census_scene, proved on the CPU to be more than the
    radius wrong raw and within 1e-6 m corrected).  With nadir_affine on the raw centres the census finds more individuals
    than animals; with the centres through attitude_points, widths and heights kept, and the rectified georeference, it finds
    exactly the animals, two members each.  Without the feature there is no attitude_points, and only the first count exists."""
    _lib()
    sc = AC.census_scene()
    n = len(sc["animals"])
    raw = tiling.census(_census_results([f["raw"] for f in sc["frames"]]), np.stack([f["raw_georef"] for f in sc["frames"]]), radius=AC.CENSUS_RADIUS)
    assert raw["count"] > n, raw["count"]
    fixed = tiling.census(_census_results([tiling.attitude_points(f["plan"], f["raw"], to="rectified") for f in sc["frames"]]),
                          np.stack([f["georef"] for f in sc["frames"]]), radius=AC.CENSUS_RADIUS)
    assert fixed["count"] == n == 12 and fixed["members"].tolist() == [2] * n
    who = [int(v) for v in fixed["individual"]]                            # detections in frame order: animal k is k and n + k
    assert who[:n] == who[n:] and len(set(who[:n])) == n
