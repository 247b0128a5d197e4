"""Times of the survey coverage (wm_coverage_raster, wm_coverage_points) against the host route a caller had before.

  python tools/coverage_time.py [--reps 20] [--skip-oracle] [--only NAME]
      HIP-event min and median over --reps repetitions of one wm_coverage_raster call and, with points, of one
      wm_coverage_points call (their memsets and single launches; buffers are allocated once, outside the timed region),
      and -- once each -- the wall clock of the numpy restatement of the rule on the same input (tests/ground_oracle.py:
      coverage_oracle_by_frame for the raster, a frame at a time over the cells around its footprint; the points part
      of coverage_oracle on a 1 x 1 grid's worth of arithmetic per point), whose result the device's must equal.
      Three settings, yawed nadir frames of 400 x 600 px at UTM-sized coordinates, placed so that a cell is seen by
      three to four frames on average:
        f40_512          F = 40 on a 512 x 512 grid;
        f1000_4096       F = 1 000 on a 4096 x 4096 grid;
        f1000_8192_pts   F = 1 000 on a 8192 x 8192 grid with 20 000 points.
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

H, W = 400, 600
OVERLAP = 3.5                 # mean frames per cell, were the frames spread evenly


def make(F, g, n_points, seed):
    """F yawed frames over a g x g grid whose side is chosen for OVERLAP; n_points ground points in and around it."""
    rng = np.random.default_rng(seed)
    case, side = yawed_survey(rng, F, g, H, W, OVERLAP)
    x0, y0 = case["x0"], case["y0"]
    case.update(points=None, labels=None)
    if n_points:
        case["points"] = np.stack([x0 + rng.uniform(-0.02 * side, 1.02 * side, n_points), y0 + rng.uniform(-0.02 * side, 1.02 * side, n_points)], axis=1)
        case["labels"] = rng.integers(0, 7, n_points).astype(np.int32)
    return case


def run(case, reps, skip_oracle):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    g, s = up(case["g2p"]), up(case["size"])
    lib = N.lib()
    cov = torch.empty((gy, gx), device=dev, dtype=torch.int16)
    stats = torch.empty(16, device=dev, dtype=torch.int64)
    grid = (case["x0"], case["y0"], case["cell"], gx, gy)
    ms_min, ms_med = timed(lambda: N.check(lib.wm_coverage_raster(N.ptr(g), N.ptr(s), F, *grid, N.ptr(cov), N.ptr(stats), N.stream_ptr(dev))), reps)
    st = stats.cpu().numpy()
    out = {"frames": F, "grid": [gy, gx], "cell_m": round(case["cell"], 4), "raster_ms_min": ms_min, "raster_ms_median": ms_med,
           "gap_cells": int(st[0]), "mean_frames_per_cell": round(cov.sum(dtype=torch.int64).item() / (gx * gy), 3)}
    P = 0 if case["points"] is None else case["points"].shape[0]
    if P:
        pts, labels = up(case["points"]), up(case["labels"])
        seen = torch.empty(P, device=dev, dtype=torch.int32)
        cidx = torch.empty((P, 2), device=dev, dtype=torch.int32)
        counts = torch.empty((7, gy, gx), device=dev, dtype=torch.int32)
        pstats = torch.empty(2, device=dev, dtype=torch.int64)
        call = lambda c: N.check(lib.wm_coverage_points(N.ptr(g), N.ptr(s), F, N.ptr(pts), N.ptr(labels), P, *grid, N.ptr(seen), N.ptr(cidx),
                                                        N.ptr(c), N.ptr(pstats), N.stream_ptr(dev)))
        out["points"] = P
        out["points_ms_min"], out["points_ms_median"] = timed(lambda: call(counts), reps)             # with the 7-plane memset
        out["points_no_counts_ms_min"], out["points_no_counts_ms_median"] = timed(lambda: call(None), reps)
        call(counts)
        out["binned"] = int(pstats[0].item())
    if not skip_oracle:
        from ground_oracle import coverage_oracle, coverage_oracle_by_frame
        t = time.perf_counter()
        want = coverage_oracle_by_frame(case["g2p"], case["size"], *grid)
        out["oracle_raster_host_s"] = round(time.perf_counter() - t, 2)
        equal = np.array_equal(want["coverage"], cov.cpu().numpy().view(np.uint16)) and np.array_equal(want["stats"], st)
        if P:
            t = time.perf_counter()
            wp = coverage_oracle(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], 1, 1, case["points"], case["labels"])
            out["oracle_points_host_s"] = round(time.perf_counter() - t, 2)
            equal = equal and np.array_equal(wp["seen_by"], seen.cpu().numpy())
            # the cells, independently of the oracle's 1 x 1 grid: the rule's subtraction, division and floor
            fi = np.floor((case["points"][:, 0] - case["x0"]) / case["cell"])
            fj = np.floor((case["points"][:, 1] - case["y0"]) / case["cell"])
            inside = (fi >= 0) & (fi < gx) & (fj >= 0) & (fj < gy)
            wc = np.where(inside[:, None], np.stack([fj, fi], axis=1), -1).astype(np.int64)
            equal = equal and np.array_equal(wc, cidx.cpu().numpy()) and int(inside.sum()) == out["binned"]
            wcounts = np.zeros((7, gy, gx), dtype=np.int32)
            np.add.at(wcounts, (case["labels"][inside], wc[inside, 0], wc[inside, 1]), 1)
            equal = equal and bool(torch.equal(counts.cpu(), torch.from_numpy(wcounts)))
        out["equals_oracle"] = bool(equal)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    settings = {"f40_512": (40, 512, 0), "f1000_4096": (1000, 4096, 0), "f1000_8192_pts": (1000, 8192, 20000)}
    out = {"reps": a.reps}
    for i, (name, (F, g, P)) in enumerate(settings.items()):
        if a.only in (None, name):
            out[name] = run(make(F, g, P, i), a.reps, a.skip_oracle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
