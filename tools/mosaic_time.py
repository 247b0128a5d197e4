"""Times of the survey mosaic (wm_mosaic_plan, wm_mosaic_fill_u8) against the host route a caller had before.

  python tools/mosaic_time.py [--reps 20] [--skip-oracle] [--only NAME]
      HIP-event min and median over --reps repetitions of one wm_mosaic_plan call (its two memsets and one launch) and of
      one wm_mosaic_fill_u8 call in each mode with every frame of the survey resident (one launch; buffers and frames are
      allocated once, outside the timed region), and -- once per setting -- the wall clock of the numpy restatement of the
      rule on the same input (tests/ground_oracle.py: mosaic_oracle_by_frame, a frame at a time over the cells around its
      footprint), whose source raster, statistics and pictures the device's must equal.
      Two settings, yawed nadir frames of 400 x 600 px of random content at UTM-sized coordinates, placed so that a cell
      is seen by three to four frames on average:
        f40_512      F = 40 on a 512 x 512 grid;
        f1000_8192   F = 1 000 on a 8192 x 8192 grid.
      Per setting the bytes the fill has to move, counted from the shapes: 4 (source) for every cell, and for every cell
      with a source 3 written and 3 (nearest) or 12 (bilinear: four pixels) read; with the minimum time that is a rate,
      printed as a fraction of the 8.0 TB/s of HBM.  The plan's figure is the 4 bytes per cell it stores.
      Prints one JSON line.  No figure is a pass mark: the numbers are records.
"""
import argparse
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
from survey_bench_util import timed, yawed_survey  # noqa: E402
from wildlifemapper_amd._survey import _frame_descs  # noqa: E402

H, W = 400, 600
OVERLAP = 3.5                 # mean frames per cell, were the frames spread evenly
HBM_PEAK = 8.0e12             # bytes per second


def make(F, g, seed):
    """F yawed frames over a g x g grid whose side is chosen for OVERLAP."""
    return dict(yawed_survey(np.random.default_rng(seed), F, g, H, W, OVERLAP)[0], seed=seed)


def run(case, reps, skip_oracle):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    g, s = up(case["g2p"]), up(case["size"])
    lib = N.lib()
    gen = torch.Generator(device=dev).manual_seed(case["seed"])
    pixels = torch.randint(0, 256, (F, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    frames = [pixels[f] for f in range(F)]
    desc = _frame_descs(frames, dev)
    slot = torch.arange(F, device=dev, dtype=torch.int32)
    source = torch.empty((gy, gx), device=dev, dtype=torch.int32)
    won = torch.empty(F, device=dev, dtype=torch.int32)
    stats = torch.empty(2, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    grid = (case["x0"], case["y0"], case["cell"], gx, gy)
    st = N.stream_ptr(dev)
    plan_min, plan_med = timed(lambda: N.check(lib.wm_mosaic_plan(N.ptr(g), N.ptr(s), F, *grid, N.ptr(source), N.ptr(won), N.ptr(stats), st)), reps)
    with_src, without = (int(v) for v in stats.cpu().tolist())
    cells = gx * gy
    out = {"frames": F, "grid": [gy, gx], "cell_m": round(case["cell"], 4), "cells_with_source": with_src, "gap_cells": without,
           "frames_that_won": int((won > 0).sum().item()), "plan_ms_min": plan_min, "plan_ms_median": plan_med,
           "plan_store_bytes": 4 * cells, "plan_store_fraction_of_hbm_peak": round(4 * cells / (plan_min * 1e-3) / HBM_PEAK, 4)}
    pictures = {}
    for mode, code, read in (("nearest", N.MOSAIC_NEAREST, 3), ("bilinear", N.MOSAIC_BILINEAR, 12)):
        pic = torch.zeros((gy, gx, 3), device=dev, dtype=torch.uint8)
        call = lambda: N.check(lib.wm_mosaic_fill_u8(N.ptr(desc), F, N.ptr(slot), N.ptr(g), N.ptr(s), F, *grid, N.ptr(source), code, 0,
                                                     N.ptr(pic), N.ptr(status), st))
        ms_min, ms_med = timed(call, reps)
        moved = 4 * cells + (3 + read) * with_src
        out[f"fill_{mode}_ms_min"], out[f"fill_{mode}_ms_median"] = ms_min, ms_med
        out[f"fill_{mode}_bytes"] = moved
        out[f"fill_{mode}_bytes_per_won_cell"] = round(moved / max(with_src, 1), 2)
        out[f"fill_{mode}_fraction_of_hbm_peak"] = round(moved / (ms_min * 1e-3) / HBM_PEAK, 4)
        pictures[mode] = pic
    out["fill_status"] = int(status.item())
    if not skip_oracle:
        from ground_oracle import mosaic_oracle_by_frame
        host = pixels.cpu().numpy()
        t = time.perf_counter()
        want = mosaic_oracle_by_frame(case["g2p"], case["size"], *grid, frames=host, fill=(0, 0, 0))
        out["oracle_host_s"] = round(time.perf_counter() - t, 2)
        equal = np.array_equal(want["source"], source.cpu().numpy()) and np.array_equal(want["won"], won.cpu().numpy()) and \
            want["stats"].tolist() == [with_src, without]
        for mode in pictures:
            equal = equal and np.array_equal(want[mode], pictures[mode].cpu().numpy())
        out["equals_oracle"] = bool(equal)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    settings = {"f40_512": (40, 512), "f1000_8192": (1000, 8192)}
    out = {"reps": a.reps}
    for i, (name, (F, g)) in enumerate(settings.items()):
        if a.only in (None, name):
            out[name] = run(make(F, g, i), a.reps, a.skip_oracle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
