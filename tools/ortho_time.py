"""Times of the survey orthorectification (wm_ortho_u8) beside the attitude rectification it extends (wm_rectify_u8).

  python tools/ortho_time.py [--reps 20] [--height 4000 --width 6000] [--roll 4 --pitch 3] [--altitude 120]
      The 4000 x 6000 frame of random content and the camera of tools/rectify_time.py (fx = fy = 0.8 * width, k1 = -0.1,
      k2 = 0.02, small p1, p2, k3, the principal point 7.25 px off centre), rolled 4 and pitched 3 degrees, yaw 30, --altitude
      metres above ground on which a Gaussian hill 30 m high (sigma 40 m, its summit 25 m east and 10 m north of the nadir point)
      stands: a DEM of 256 x 256 posts 2 m apart at UTM-sized coordinates.  keep='valid', the default cell and a track-aligned
      grid.  HIP-event min and median over --reps repetitions, after a warm-up call, in one process, of
        ortho_nearest / ortho_bilinear       one wm_ortho_u8 call with both counters (a memset and a launch);
        rectify_nearest / rectify_bilinear   one wm_rectify_u8 call on the same frame with rectify_plan's own keep='valid'
                                             picture: the parent's kernel, unchanged.
      The two pictures differ in size, so the comparison is per output pixel: ortho_over_rectify_per_pixel, per mode.  Bytes
      are algorithmic (the frame read, the picture written, the DEM read once), as in undistort_time.py.
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
    ap.add_argument("--altitude", type=float, default=120.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    f = 0.8 * W
    camera = np.array([f, f, (W - 1) / 2 + 7.25, (H - 1) / 2 - 7.25, -0.1, 0.02, 0.0004, -0.0003, -0.002])
    position, ground, posts, spacing = (512345.5, 9812345.25), 100.0, 256, 2.0
    e0, n0 = position[0] - posts * spacing / 2, position[1] + posts * spacing / 2
    r, c = np.meshgrid(np.arange(posts), np.arange(posts), indexing="ij")
    E, Nn = e0 + (c + 0.5) * spacing, n0 - (r + 0.5) * spacing
    heights = ground + 30.0 * np.exp(-((E - (position[0] + 25.0)) ** 2 + (Nn - (position[1] + 10.0)) ** 2) / (2 * 40.0 ** 2))
    dem = tiling.terrain_grid(heights, (e0, n0), spacing, device=dev)
    pose = tiling.camera_pose(position, ground + a.altitude, 30.0, (a.roll, a.pitch))
    t = time.perf_counter()
    plan = tiling.ortho_plan(camera, (H, W), pose, dem, keep="valid")
    plan_s = time.perf_counter() - t
    rect = tiling.rectify_plan(camera, (H, W), (a.roll, a.pitch), keep="valid")
    out = {"reps": a.reps, "frame": [H, W], "camera": camera.tolist(), "roll_deg": a.roll, "pitch_deg": a.pitch, "altitude_m": a.altitude,
           "dem": [posts, posts], "dem_spacing_m": spacing, "hill_m": 30.0, "ortho_out_size": list(plan["out_size"]), "cell_m": plan["cell"],
           "rectify_out_size": list(rect["out_size"]), "ortho_plan_host_s": round(plan_s, 3)}
    lib, st = N.lib(), N.stream_ptr(dev)
    frame = torch.randint(0, 256, (H, W, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(0))
    cam_c, fill_c = (C.c_double * 9)(*camera.tolist()), (C.c_uint8 * 3)(0, 0, 0)
    pose_c = (C.c_double * 12)(*plan["pose"].tolist())
    dgeo_c = (C.c_double * 3)(e0, n0, spacing)
    ogeo_c = (C.c_double * 6)(*plan["georef"].reshape(6).tolist())
    rot_c = (C.c_double * 9)(*rect["rotation"].reshape(9).tolist())
    stats = torch.zeros(2, device=dev, dtype=torch.int64)
    zs = dem["device_heights"]
    for what, pl in (("ortho", plan), ("rectify", rect)):
        oh, ow = pl["out_size"]
        pic = torch.empty((oh, ow, 3), device=dev, dtype=torch.uint8)
        moved = 3 * H * W + 3 * oh * ow + (4 * posts * posts if what == "ortho" else 0)
        for mode, code in (("nearest", N.MOSAIC_NEAREST), ("bilinear", N.MOSAIC_BILINEAR)):
            if what == "ortho":
                call = lambda: N.check(lib.wm_ortho_u8(N.ptr(frame), H, W, cam_c, pose_c, N.ptr(zs), posts, posts, dgeo_c, N.ptr(pic), oh, ow, ogeo_c, code,
                                                       fill_c, N.ptr(stats), st))
            else:
                call = lambda: N.check(lib.wm_rectify_u8(N.ptr(frame), H, W, cam_c, rot_c, N.ptr(pic), oh, ow, pl["f_out"], code, fill_c, N.ptr(stats), st))
            ms_min, ms_med = timed(call, a.reps)
            counts = stats.tolist()
            out[f"{what}_{mode}"] = dict(ms_min=ms_min, ms_median=ms_med, ns_per_output_pixel=round(ms_min * 1e6 / (oh * ow), 5),
                                         filled=counts[0], **({"no_height": counts[1]} if what == "ortho" else {}), **rate(moved, ms_min))
    for mode in ("nearest", "bilinear"):
        out[f"ortho_over_rectify_per_pixel_{mode}"] = round(out[f"ortho_{mode}"]["ns_per_output_pixel"] / out[f"rectify_{mode}"]["ns_per_output_pixel"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
