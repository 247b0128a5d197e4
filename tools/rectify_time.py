"""Times of the survey attitude rectification (wm_rectify_u8) beside the lens correction it extends (wm_undistort_u8).

  python tools/rectify_time.py [--reps 20] [--height 4000 --width 6000] [--roll 4 --pitch 3]
      The 4000 x 6000 frame of random content and the camera of tools/undistort_time.py (fx = fy = 0.8 * width, k1 = -0.1,
      k2 = 0.02, small p1, p2, k3, the principal point 7.25 px off centre), rolled 4 and pitched 3 degrees, keep='valid',
      f_out = fx.  HIP-event min and median over --reps repetitions, after a warm-up call, in one process, of
        rectify_nearest / rectify_bilinear       one wm_rectify_u8 call with the filled count (a memset and a launch);
        undistort_nearest / undistort_bilinear   one wm_undistort_u8 call on the same frame with the lens plan's own
                                                 keep='valid' picture: the parent's kernel, unchanged.
      The two pictures differ in size (a centred valid picture of a tilted frame is smaller), so the comparison is per output
      pixel: rectify_over_undistort_per_pixel, per mode.  Bytes are algorithmic, as in undistort_time.py.
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
from wildlifemapper_amd import _native as N  # noqa: E402
from wildlifemapper_amd import tiling  # noqa: E402
from survey_bench_util import timed  # noqa: E402
from undistort_time import rate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--roll", type=float, default=4.0)
    ap.add_argument("--pitch", type=float, default=3.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    f = 0.8 * W
    camera = np.array([f, f, (W - 1) / 2 + 7.25, (H - 1) / 2 - 7.25, -0.1, 0.02, 0.0004, -0.0003, -0.002])
    t = time.perf_counter()
    plan = tiling.rectify_plan(camera, (H, W), (a.roll, a.pitch), keep="valid")
    plan_s = time.perf_counter() - t
    lens_plan = tiling.lens_plan(camera, (H, W), keep="valid")
    out = {"reps": a.reps, "frame": [H, W], "camera": camera.tolist(), "roll_deg": a.roll, "pitch_deg": a.pitch,
           "rectify_out_size": list(plan["out_size"]), "undistort_out_size": list(lens_plan["out_size"]), "f_out": plan["f_out"],
           "rectify_plan_host_s": round(plan_s, 3)}
    lib, st = N.lib(), N.stream_ptr(dev)
    frame = torch.randint(0, 256, (H, W, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(0))
    cam_c, fill_c = (C.c_double * 9)(*camera.tolist()), (C.c_uint8 * 3)(0, 0, 0)
    rot_c = (C.c_double * 9)(*plan["rotation"].reshape(9).tolist())
    stats = torch.zeros(1, device=dev, dtype=torch.int64)
    for what, pl in (("rectify", plan), ("undistort", lens_plan)):
        oh, ow = pl["out_size"]
        pic = torch.empty((oh, ow, 3), device=dev, dtype=torch.uint8)
        moved = 3 * H * W + 3 * oh * ow
        for mode, code in (("nearest", N.MOSAIC_NEAREST), ("bilinear", N.MOSAIC_BILINEAR)):
            if what == "rectify":
                call = lambda: N.check(lib.wm_rectify_u8(N.ptr(frame), H, W, cam_c, rot_c, N.ptr(pic), oh, ow, pl["f_out"], code, fill_c, N.ptr(stats), st))
            else:
                call = lambda: N.check(lib.wm_undistort_u8(N.ptr(frame), H, W, cam_c, N.ptr(pic), oh, ow, pl["f_out"], code, fill_c, N.ptr(stats), st))
            ms_min, ms_med = timed(call, a.reps)
            out[f"{what}_{mode}"] = dict(ms_min=ms_min, ms_median=ms_med, ns_per_output_pixel=round(ms_min * 1e6 / (oh * ow), 5),
                                         filled=int(stats.item()), **rate(moved, ms_min))
    for mode in ("nearest", "bilinear"):
        out[f"rectify_over_undistort_per_pixel_{mode}"] = round(out[f"rectify_{mode}"]["ns_per_output_pixel"] /
                                                                out[f"undistort_{mode}"]["ns_per_output_pixel"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
