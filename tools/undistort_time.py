"""Times of the survey lens correction (wm_undistort_u8) beside the calls it resembles and the host route a caller had before.

  python tools/undistort_time.py [--reps 20] [--skip-host] [--height 4000 --width 6000]
      One 4000 x 6000 frame of random content, a wide lens (fx = fy = 0.8 * width, k1 = -0.1, k2 = 0.02, small p1, p2, k3
      and a principal point 7.25 px off centre), keep='valid', f_out = fx.  HIP-event min and median over --reps
      repetitions, after a warm-up call, of
        undistort_nearest / undistort_bilinear   one wm_undistort_u8 call with the filled count (a memset and a launch);
        resample_same_size      wm_resample_u8 of the frame to its own size: the same bytes moved, by a device copy;
        mosaic_fill_bilinear    one-frame wm_mosaic_fill_u8, bilinear, on a grid whose cell is the frame's ground sampling
                                distance: the same sampler and the same stores, behind an affine instead of the lens model;
      and, unless --skip-host, the wall clock of the 16-thread host route: torch.nn.functional.grid_sample on the CPU
      (float32, bilinear, the sampling grid built once from lens_points and not timed), min of three.
      Bytes are algorithmic: 3 * H * W read and 3 * oh * ow written for the lens, whatever the cache does with the four taps of
      a bilinear sample; with the minimum time that is a rate, printed in GB/s and as a fraction of the 8.0 TB/s of HBM.
      Prints one JSON line.  No figure is a pass mark: the numbers are records.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from wildlifemapper_amd import _native as N  # noqa: E402
from wildlifemapper_amd import tiling  # noqa: E402
from survey_bench_util import timed  # noqa: E402
from wildlifemapper_amd._survey import _frame_descs  # noqa: E402

HBM_PEAK = 8.0e12             # bytes per second
HOST_THREADS = 16


def rate(nbytes, ms):
    return {"bytes": int(nbytes), "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "fraction_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    f = 0.8 * W
    camera = np.array([f, f, (W - 1) / 2 + 7.25, (H - 1) / 2 - 7.25, -0.1, 0.02, 0.0004, -0.0003, -0.002])
    t = time.perf_counter()
    plan = tiling.lens_plan(camera, (H, W), keep="valid")
    plan_s = time.perf_counter() - t
    oh, ow = plan["out_size"]
    out = {"reps": a.reps, "frame": [H, W], "camera": camera.tolist(), "out_size": [oh, ow], "f_out": plan["f_out"], "lens_plan_host_s": round(plan_s, 3)}
    lib, st = N.lib(), N.stream_ptr(dev)
    frame = torch.randint(0, 256, (H, W, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(0))
    cam_c, fill_c = (C.c_double * 9)(*camera.tolist()), (C.c_uint8 * 3)(0, 0, 0)
    pic = torch.empty((oh, ow, 3), device=dev, dtype=torch.uint8)
    stats = torch.zeros(1, device=dev, dtype=torch.int64)
    moved = 3 * H * W + 3 * oh * ow
    for mode, code in (("nearest", N.MOSAIC_NEAREST), ("bilinear", N.MOSAIC_BILINEAR)):
        call = lambda: N.check(lib.wm_undistort_u8(N.ptr(frame), H, W, cam_c, N.ptr(pic), oh, ow, plan["f_out"], code, fill_c, N.ptr(stats), st))
        ms_min, ms_med = timed(call, a.reps)
        out[f"undistort_{mode}"] = dict(ms_min=ms_min, ms_median=ms_med, ns_per_output_pixel=round(ms_min * 1e6 / (oh * ow), 4),
                                        filled=int(stats.item()), **rate(moved, ms_min))

    # the same bytes moved: wm_resample_u8 to the frame's own size (both of Pillow's passes skipped: a device copy)
    same = torch.empty_like(frame)
    ms_min, ms_med = timed(lambda: N.check(lib.wm_resample_u8(N.ptr(frame), H, W, N.ptr(same), H, W, st)), a.reps)
    out["resample_same_size"] = dict(ms_min=ms_min, ms_median=ms_med, ns_per_output_pixel=round(ms_min * 1e6 / (H * W), 4), **rate(6 * H * W, ms_min))

    # the same sampler and stores: one frame laid onto a grid of its own pixels' size
    gsd = 0.02
    georef = tiling.nadir_affine(H, W, (500000.1, 6000000.7), gsd, 0.0)[None]
    x0, y0, gx, gy = tiling.footprint_bounds(georef, [(H, W)], gsd)
    g2p = torch.from_numpy(tiling.ground_to_pixel(georef).reshape(-1, 6)).to(dev)
    size = torch.tensor([[H, W]], dtype=torch.int32, device=dev)
    source = torch.empty((gy, gx), device=dev, dtype=torch.int32)
    won, mstats = torch.empty(1, device=dev, dtype=torch.int32), torch.empty(2, device=dev, dtype=torch.int64)
    N.check(lib.wm_mosaic_plan(N.ptr(g2p), N.ptr(size), 1, x0, y0, gsd, gx, gy, N.ptr(source), N.ptr(won), N.ptr(mstats), st))
    with_src = int(mstats[0].item())
    desc, slot = _frame_descs([frame], dev), torch.zeros(1, device=dev, dtype=torch.int32)
    mpic, status = torch.zeros((gy, gx, 3), device=dev, dtype=torch.uint8), torch.zeros(1, device=dev, dtype=torch.int32)
    call = lambda: N.check(lib.wm_mosaic_fill_u8(N.ptr(desc), 1, N.ptr(slot), N.ptr(g2p), N.ptr(size), 1, x0, y0, gsd, gx, gy, N.ptr(source),
                                                 N.MOSAIC_BILINEAR, 0, N.ptr(mpic), N.ptr(status), st))
    ms_min, ms_med = timed(call, a.reps)
    out["mosaic_fill_bilinear"] = dict(grid=[gy, gx], cells_with_source=with_src, status=int(status.item()), ms_min=ms_min, ms_median=ms_med,
                                       ns_per_output_pixel=round(ms_min * 1e6 / max(with_src, 1), 4), **rate(4 * gx * gy + 6 * with_src, ms_min))
    out["undistort_bilinear_over_fill_per_pixel"] = round(out["undistort_bilinear"]["ns_per_output_pixel"] / out["mosaic_fill_bilinear"]["ns_per_output_pixel"], 3)

    if not a.skip_host:
        torch.set_num_threads(HOST_THREADS)
        jj, ii = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
        uv = tiling.lens_points(plan, np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], axis=1), to="raw")
        grid = torch.from_numpy(np.stack([uv[:, 0] * (2.0 / W) - 1.0, uv[:, 1] * (2.0 / H) - 1.0], axis=1).astype(np.float32)).reshape(1, oh, ow, 2)
        img = frame.cpu().permute(2, 0, 1)[None].float()
        best = float("inf")
        for _ in range(3):
            t = time.perf_counter()
            torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False).round_().clamp_(0, 255).to(torch.uint8)
            best = min(best, time.perf_counter() - t)
        out["host_grid_sample"] = dict(threads=HOST_THREADS, ms_min=round(best * 1e3, 1),
                                       times_undistort_bilinear=round(best * 1e3 / out["undistort_bilinear"]["ms_min"], 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
