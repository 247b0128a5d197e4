"""Survey lens on the GPU: wm_undistort_u8 equals the rule's restatement (tests/lens_cases.py: lens_oracle) byte for byte,
with the filled count, for every case in both modes at every byte offset of the output; and preprocess.undistort_u8 and
tiling.undistorted hand those bytes to detect_frames and mosaic unchanged.  The cases, the oracle and the mutants that show
the cases have teeth are in tests/lens_cases.py and tests/test_lens_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import lens_cases as LC
from survey_util import DEV, _animals, _guarded, _Lazy, _lib, _StubModel
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import preprocess, tiling

pytestmark = pytest.mark.gpu
MODE = {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}


def _undistort_at(pl, img, mode, out_off, in_off, fill=LC.FILL, out_buf=None):
    """wm_undistort_u8 with the input in_off and the output out_off bytes past an aligned allocation, both inside guard
    bytes (survey_util._guarded: 255 all round).  Returns (picture, filled, the output's whole buffer)."""
    lib = _lib()
    (h, w), (oh, ow) = pl["size"], pl["out_size"]
    _, src = _guarded(img, in_off, DEV)
    if out_buf is None:
        out_buf = _guarded(np.full((oh, ow, 3), 171, np.uint8), out_off, DEV)[0]
    stats = torch.full((1,), -5, dtype=torch.int64, device=DEV)
    cam = (C.c_double * 9)(*pl["camera"].tolist())
    N.check(lib.wm_undistort_u8(C.c_void_p(src.data_ptr()), h, w, cam, C.c_void_p(out_buf.data_ptr() + out_off), oh, ow, pl["f_out"],
                                MODE[mode], (C.c_uint8 * 3)(*fill), N.ptr(stats), N.stream_ptr(torch.device(DEV))))
    got = out_buf.cpu().numpy()
    n = oh * ow * 3
    assert (got[:out_off] == 255).all() and (got[out_off + n:] == 255).all(), "wm_undistort_u8 wrote outside its output"
    return got[out_off:out_off + n].reshape(oh, ow, 3), int(stats.item()), out_buf


@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_undistort_equals_the_oracle_byte_for_byte(name):
    pl, img, want = LC.expected(name)
    for mode in LC.MODES:
        for off in range(4):                                              # the output 0..3 bytes past a dword; the input offset too
            got, filled, _ = _undistort_at(pl, img, mode, off, (off + 1) % 4)
            diff = int((got != want[mode]).sum())
            assert diff == 0, (name, mode, off, diff, np.argwhere((got != want[mode]).any(axis=2))[:4].tolist())
            assert filled == want["filled"], (name, mode, off)


def test_a_second_call_overwrites_every_byte():
    """Every output byte is written by every call: a second call into the same buffer with another fill leaves nothing of the first."""
    for name in ("all_barrel", "fx_ne_fy_15x200"):
        pl, img, want = LC.expected(name)
        for mode in LC.MODES:
            _, _, buf = _undistort_at(pl, img, mode, 1, 0, fill=(200, 100, 50))
            got, filled, _ = _undistort_at(pl, img, mode, 1, 0, out_buf=buf)
            assert np.array_equal(got, want[mode]) and filled == want["filled"], (name, mode)


def test_identity_through_the_kernel():
    for k, size in enumerate(LC.IDENTITY_SIZES):
        f = 0.83 * size[1] + 0.1 * k
        pl = tiling.lens_plan(LC.camera(size, f=f), size, out_size=size, f_out=f)
        img = np.random.default_rng(k).integers(0, 256, (*size, 3), dtype=np.uint8)
        for mode in LC.MODES:
            got, filled, _ = _undistort_at(pl, img, mode, 0, 0)
            assert np.array_equal(got, img) and filled == 0, (size, mode)


def test_no_stats_pointer_is_accepted():
    pl, img, want = LC.expected("five_33x129")
    out = torch.empty((*pl["out_size"], 3), dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(img).to(DEV)
    N.check(_lib().wm_undistort_u8(N.ptr(src), *pl["size"], (C.c_double * 9)(*pl["camera"].tolist()), N.ptr(out), *pl["out_size"], pl["f_out"],
                                   N.MOSAIC_BILINEAR, (C.c_uint8 * 3)(*LC.FILL), None, N.stream_ptr(torch.device(DEV))))
    assert np.array_equal(out.cpu().numpy(), want["bilinear"])


def test_wrappers_return_the_oracles_bytes():
    """preprocess.undistort_u8 and tiling.undistorted, device and host frames; a lazy source is indexed once per access."""
    _lib()
    pl, img, want = LC.expected("all_five_fx_ne_fy")
    dev_frame = torch.from_numpy(img).to(DEV)
    for mode in LC.MODES:
        got, filled = preprocess.undistort_u8(dev_frame, pl, sample=mode, fill=LC.FILL, count=True)
        assert got.shape == (*pl["out_size"], 3) and got.dtype == torch.uint8 and got.device == dev_frame.device
        assert filled.dtype == torch.int64 and filled.is_cuda and int(filled.item()) == want["filled"]
        assert np.array_equal(got.cpu().numpy(), want[mode]), mode
    assert np.array_equal(preprocess.undistort_u8(dev_frame, pl, fill=LC.FILL).cpu().numpy(), want["bilinear"])
    with pytest.raises(ValueError, match="the plan was made for"):
        preprocess.undistort_u8(dev_frame[:-1], pl)
    src = _Lazy([dev_frame, img, torch.from_numpy(img)])                  # a device tensor, a numpy array, a CPU tensor
    u = tiling.undistorted(src, pl, sample="nearest", fill=LC.FILL)
    assert len(u) == 3 and src.asked == [] and (u.sizes == pl["out_size"]).all()
    for i in (2, 0, 1):
        got = u[i]
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want["nearest"]), i
    assert src.asked == [2, 0, 1]
    assert all(np.array_equal(g.cpu().numpy(), want["nearest"]) for g in u) and src.asked == [2, 0, 1, 0, 1, 2]
    with pytest.raises(ValueError, match="the plan was made for"):
        tiling.undistorted([img[:, :-1]], pl)[0]


def test_mosaic_of_undistorted_frames_equals_mosaic_of_the_oracles_pictures():
    _lib()
    size = (64, 129)
    cam = LC.camera(size, **LC.FIVE)
    pl = tiling.lens_plan(cam, size, keep="valid")
    oh, ow = pl["out_size"]
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (*size, 3), dtype=np.uint8) for _ in range(4)]
    georef = np.stack([tiling.nadir_affine(oh, ow, (100.0 + 30.0 * k, 200.0 + 11.0 * k), 0.5, 20.0 * k) for k in range(4)])
    src = _Lazy(frames)
    u = tiling.undistorted(src, pl, sample="bilinear")
    got = tiling.mosaic(u, georef, 0.4, sizes=u.sizes)
    pictures = [LC.lens_oracle(f, cam, (oh, ow), pl["f_out"], fill=(0, 0, 0), modes=("bilinear",))["bilinear"] for f in frames]
    want = tiling.mosaic(pictures, georef, 0.4)
    assert torch.equal(got["mosaic"], want["mosaic"]) and torch.equal(got["source"], want["source"])
    assert sorted(src.asked) == torch.nonzero(want["won"] > 0).flatten().tolist()       # the winners, once each


def test_detect_frames_takes_the_undistorted_sequence():
    """detect_frames(stub, tiling.undistorted(...)) tiles the UNDISTORTED sizes: the stub, built for those sizes, hands out
    all its records, and the results are those of a survey of plain frames of the undistorted size."""
    _lib()
    size = (1100, 1300)
    pl = tiling.lens_plan(LC.camera(size, k1=-0.05), size, keep="valid")
    oh, ow = pl["out_size"]
    assert (oh, ow) != size and ow > 1024 and oh > 1024                   # other sizes than the raw frames', and seams either way
    rng = np.random.default_rng(9)
    frames = [torch.from_numpy(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).to(DEV), rng.integers(0, 256, (*size, 3), dtype=np.uint8)]
    org = tiling.tile_origins(oh, ow)
    ys, xs = sorted({o[0] for o in org}), sorted({o[1] for o in org})
    animals = [_animals(oh, ow, rng, ([y + 1024 for y in ys[:-1]] + ys[1:], [x + 1024 for x in xs[:-1]] + xs[1:])) for _ in frames]
    src = _Lazy(frames)
    stub = _StubModel([(oh, ow)] * 2, animals)
    got = list(tiling.detect_frames(stub, tiling.undistorted(src, pl), batch=4))
    assert stub.pos == stub.records.shape[0] == 2 * len(org) and src.asked == [0, 1]
    plain = [torch.zeros((oh, ow, 3), dtype=torch.uint8, device=DEV)] * 2
    want = list(tiling.detect_frames(_StubModel([(oh, ow)] * 2, animals), plain, batch=4))
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert set(a) == set(b)
        assert a["boxes"].shape[0] >= 12                                  # a property of the animals' table, not of any weights
        for key in a:
            if isinstance(a[key], torch.Tensor):
                assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                                   b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), key
            else:
                assert a[key] == b[key], key
