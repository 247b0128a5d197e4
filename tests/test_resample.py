"""Survey resampling (wm_resample_u8, wm_scaled_size, preprocess.resample_u8): argument checks and the size rule on the
CPU; bit-exactness against Pillow (tests/golden/resample_pil.npz, tools/gen_resample_golden.py) and against the N1
resize path on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from survey_util import _lib
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import preprocess, tiling


def test_resample_abi_rejects_bad_arguments():
    L = _lib()
    p = C.c_void_p(16)                  # never dereferenced: every call below fails validation before any HIP call
    for args, msg in [((None, 10, 10, p, 5, 5), b"null"), ((p, 10, 10, None, 5, 5), b"null"),
                      ((p, 0, 10, p, 5, 5), b"1..65536"), ((p, 10, 0, p, 5, 5), b"1..65536"),
                      ((p, 10, 10, p, 0, 5), b"1..65536"), ((p, 10, 10, p, 5, -1), b"1..65536"),
                      ((p, 65537, 10, p, 5, 5), b"1..65536"), ((p, 10, 10, p, 5, 65537), b"1..65536")]:
        assert L.wm_resample_u8(*args, None) < 0, args
        assert msg in L.wm_last_error(), (args, L.wm_last_error())
    oh, ow = C.c_int(), C.c_int()
    for args, msg in [((0, 10, 0.5), b"outside"), ((10, 65537, 0.5), b"outside"), ((10, 10, 0.0), b"positive"),
                      ((10, 10, -1.0), b"positive"), ((10, 10, float("nan")), b"positive"), ((10, 10, float("inf")), b"positive"),
                      ((65536, 10, 1.5), b"exceeds")]:
        assert L.wm_scaled_size(*args, C.byref(oh), C.byref(ow)) < 0, args
        assert msg in L.wm_last_error(), (args, L.wm_last_error())
    assert L.wm_scaled_size(10, 10, 0.5, None, C.byref(ow)) < 0 and b"null" in L.wm_last_error()


def test_scaled_size_rounding_and_tile_counts():
    _lib()
    # (H, W) = (4000, 6000): a 6000 x 4000 frame
    table = {None: ((4000, 6000), 35), 0.5: ((2000, 3000), 12), 0.25: ((1000, 1500), 2), 0.128: ((512, 768), 1),
             1.0: ((4000, 6000), 35)}
    for s, (size, tiles) in table.items():
        got = (4000, 6000) if s is None else preprocess.scaled_size(4000, 6000, s)
        assert got == size, (s, got)
        assert len(tiling.tile_origins(*got, 1024, 128)) == tiles, s
    assert preprocess.resized_size(4000, 6000, 768, 768) == (512, 768)
    assert tiling.resampled_size(0, 4000, 6000, resize=(768, 768)) == (512, 768)
    assert len(tiling.tile_origins(*tiling.resampled_size(0, 4000, 6000, resize=(768, 768)))) == 1
    assert preprocess.scaled_size(3648, 5472, 0.128) == (467, 700)
    assert preprocess.scaled_size(3, 5, 0.5) == (2, 3)                   # floor(x + 0.5): halves round up
    assert preprocess.scaled_size(1, 1, 1e-3) == (1, 1)                  # never below one pixel
    assert preprocess.scaled_size(2400, 3000, 0.5) == (1200, 1500)
    assert preprocess.scaled_size(100, 100, 1.7) == (170, 170)
    assert tiling.resampled_size(3, 4000, 6000, scale=lambda i, h, w: 0.25 * (i + 1)) == (4000, 6000)
    # the reference geometry packs mixed-size frames 16 to a batch: one tile each
    sizes = [(4000, 6000), (3648, 5472), (5525, 3690), (3000, 4000)] * 8
    counts = [len(tiling.tile_origins(*tiling.resampled_size(i, h, w, resize=(768, 768)))) for i, (h, w) in enumerate(sizes)]
    assert counts == [1] * 32
    plan = list(tiling.plan_batches(counts, 16))
    assert [len(b.completes) for b in plan] == [16, 16]


def test_detect_frames_rejects_bad_scale_before_device_work():
    _lib()
    frame = np.zeros((40, 60, 3), np.uint8)
    for kw in [dict(scale=0.5, resize=(768, 768)), dict(scale=0), dict(scale=0.0), dict(scale=-0.5), dict(scale=float("nan")),
               dict(scale=float("inf")), dict(scale="x"), dict(resize=(0, 768)), dict(scale=lambda i, h, w: 0.0),
               dict(scale=lambda i, h, w: float("nan"))]:
        g = tiling.detect_frames(None, [frame], **kw)                   # a generator: nothing runs before the first next()
        with pytest.raises(ValueError):
            next(g)
    with pytest.raises(ValueError):
        tiling.detect_frame(None, torch.from_numpy(frame), scale=float("nan"))
    with pytest.raises(ValueError):
        tiling.detect_frame(None, torch.from_numpy(frame), scale=1.0, resize=(768, 768))


def test_resample_family_has_one_definition_of_what_it_shares():
    """From the sources: one horizontal streaming kernel, one plan cache, one home for the family, one spelling of the clip."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wildlifemapper_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip"))}
    everything = "\n".join(src.values())
    for gone in ("resize_h_rows_kernel", "g_resize", "ResizePlan", "ResizeDevState", "upload_ints"):
        assert not re.search(r"\b%s\b" % gone, everything), gone
    kern = src["resample_kernels.h"]
    assert re.search(r"constexpr int RESIZE_PREC_BITS\s*=", kern)
    assert len(re.findall(r"constexpr int RESIZE_PREC_BITS\s*=", everything)) == 1
    assert re.findall(r'#include "(\w+\.h)"', kern) == ["wm_common.h"]
    for k in ("preprocess_u8_kernel", "resize_h_u8_kernel", "resample_h_cols_kernel", "resample_v_u8_kernel", "resize_v_normalize_kernel",
              "resize_v_normalize4_kernel"):
        assert [n for n, s in src.items() if re.search(r"__global__[^;{]*\b%s\(" % k, s)] == ["resample_kernels.h"], k
    assert "RESIZE_PREC_BITS" not in src["misc_kernels.h"] and "resiz" not in src["misc_kernels.h"].lower()
    assert everything.count(">> RESIZE_PREC_BITS, 0), 255)") == 1                  # resample_clip8
    assert everything.count("1 << (RESIZE_PREC_BITS - 1)") == 1                    # RESAMPLE_ACC0
    assert '#include "resample_kernels.h"' in src["chip_kernels.h"] and "resample_clip8(" in src["chip_kernels.h"]
    assert everything.count('getenv("WM_RESIZE_GENERIC")') == 1


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _resample_at(img: np.ndarray, oh: int, ow: int, in_off: int, out_off: int) -> np.ndarray:
    """wm_resample_u8 with the input and output starting in_off / out_off bytes past an aligned allocation, and 64 guard
    bytes around the output that must stay untouched."""
    dev = torch.device("cuda:0")
    h, w, _ = img.shape
    src = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device=dev)
    src[in_off:in_off + img.size] = torch.from_numpy(img.reshape(-1)).to(dev)
    n = oh * ow * 3
    dst = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=dev)
    N.check(N.lib().wm_resample_u8(C.c_void_p(src.data_ptr() + in_off), h, w, C.c_void_p(dst.data_ptr() + 64 + out_off), oh, ow,
                                   N.stream_ptr(dev)))
    got = dst.cpu().numpy()
    guard = np.concatenate([got[:64 + out_off], got[64 + out_off + n:]])
    assert (guard == 0xA5).all(), "wm_resample_u8 wrote outside its output"
    return got[64 + out_off:64 + out_off + n].reshape(oh, ow, 3)


@pytest.mark.gpu
def test_resample_u8_bit_exact_vs_pil(golden_dir):
    fx = np.load(os.path.join(golden_dir, "resample_pil.npz"))
    dev = torch.device("cuda:0")
    names = list(fx["names"])
    assert len(names) >= 13
    for i, name in enumerate(names):
        img, want = fx[f"in_{i}"], fx[f"out_{i}"]
        oh, ow = want.shape[:2]
        got = preprocess.resample_u8(torch.from_numpy(img).to(dev), (oh, ow))
        assert got.shape == (oh, ow, 3) and got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), name
        for in_off, out_off in [(1, 3), (2, 1), (3, 2)]:                # unaligned frame and output starts
            assert np.array_equal(_resample_at(img, oh, ow, in_off, out_off), want), (name, in_off, out_off)
    # same size: both passes skipped, a copy
    img = fx["in_0"]
    assert np.array_equal(preprocess.resample_u8(torch.from_numpy(img).to(dev), img.shape[:2]).cpu().numpy(), img)
    # more geometries than the plan cache holds, then the first again
    for k in range(12):
        preprocess.resample_u8(torch.from_numpy(img).to(dev), (20 + k, 30 + k))
    assert np.array_equal(preprocess.resample_u8(torch.from_numpy(img).to(dev), fx["out_0"].shape[:2]).cpu().numpy(), fx["out_0"])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_resample_then_cut_equals_resized_preprocess():
    """The survey's resample + tile cut at the reference geometry is the N1 val-transform path, bit for bit."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(21)
    for h, w in [(4000, 6000), (3648, 5472)]:
        f = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)
        assert preprocess.resized_size(h, w, 768, 768) == (512, 768)
        r = preprocess.resample_u8(f, (512, 768))
        got = tiling.frame_to_tiles(r, torch.zeros((1, 2), dtype=torch.int32, device=dev))
        want = preprocess.tiles_from_u8(f[None], resize=(768, 768))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (h, w)
