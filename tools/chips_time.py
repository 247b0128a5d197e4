"""Time of the review-chip kernel (wm_crop_chips_u8) against the route a caller had without it.

  python tools/chips_time.py [--n 256] [--chip 128] [--side 150] [--reps 20]

One launch cuts --n windows of --side pixels (boxes of side / 1.5 pixels, context 1.5) out of a 4000 x 6000 device frame,
timed with HIP events around the launch alone.  The old route, per detection: slice the device frame and call
preprocess.resample_u8 (a copy of the slice, two launches and a host-computed coefficient upload per new geometry); its
windows have to lie inside the frame, since it cannot pad, so all windows here do.  Both routes must give the same bytes.
Prints one JSON line: both times, the ratio, and the kernel's GB/s over the frame bytes inside the windows plus the chip
bytes written.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wildlifemapper_amd import _native as N, preprocess, tiling  # noqa: E402
from wildlifemapper_amd._survey import _frame_descs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--chip", type=int, default=128)
    ap.add_argument("--side", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, S = 4000, 6000, a.chip
    g = torch.Generator(device=dev).manual_seed(0)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(0)
    m = a.side / 1.5
    cx = rng.uniform(a.side, W - a.side, a.n)
    cy = rng.uniform(a.side, H - a.side, a.n)
    boxes_h = np.stack([cx - m / 2, cy - m / 2, cx + m / 2, cy + m / 2], axis=1).astype(np.float32)
    win = tiling.chip_windows(boxes_h)
    assert (win[:, :2] >= 0).all() and (win[:, 0] + win[:, 2] <= H).all() and (win[:, 1] + win[:, 2] <= W).all()
    boxes = torch.from_numpy(boxes_h).to(dev)
    desc = _frame_descs([frame], dev)
    chips = torch.empty((a.n, S, S, 3), dtype=torch.uint8, device=dev)
    windows = torch.empty((a.n, 3), dtype=torch.int32, device=dev)
    L, s = N.lib(), N.stream_ptr(dev)

    def launch():
        N.check(L.wm_crop_chips_u8(N.ptr(desc), 1, N.ptr(boxes), None, a.n, S, 1.5, 32, 1024, N.ptr(chips), N.ptr(windows), s))

    def old_route():
        return [preprocess.resample_u8(frame[y0:y0 + sd, x0:x0 + sd], (S, S)) for y0, x0, sd in win.tolist()]

    launch()
    ref = torch.stack(old_route())
    torch.cuda.synchronize()
    assert torch.equal(ref, chips) and np.array_equal(windows.cpu().numpy(), win), "the two routes differ"

    def timed(fn):
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.min(ms)), float(np.median(ms))

    k_min, k_med = timed(launch)
    o_min, o_med = timed(old_route)
    nbytes = int((win[:, 2].astype(np.int64) ** 2).sum()) * 3 + a.n * S * S * 3
    print(json.dumps({"n": a.n, "chip": S, "side_mean": round(float(win[:, 2].mean()), 1), "kernel_ms_min": round(k_min, 4),
                      "kernel_ms_median": round(k_med, 4), "old_route_ms_min": round(o_min, 3), "old_route_ms_median": round(o_med, 3),
                      "old_over_kernel": round(o_min / k_min, 1), "bytes": nbytes, "kernel_GBps": round(nbytes / k_min / 1e6, 1)}))


if __name__ == "__main__":
    main()
