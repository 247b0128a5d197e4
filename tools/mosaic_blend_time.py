"""Times of the blended survey mosaic (wm_mosaic_blend_plan, wm_mosaic_blend_accum_u8, wm_mosaic_blend_finish_u8) beside the
hard mosaic it replaces (wm_mosaic_plan, wm_mosaic_fill_u8) and the host route.

  python tools/mosaic_blend_time.py [--reps 20] [--band 32] [--skip-oracle] [--only NAME]
      HIP-event min and median over --reps repetitions, in ONE process and alternating (hard plan, blend plan, then per mode
      the hard fill, the accumulate with all frames resident and the accumulate in chunks of 32, then the finish -- and the
      same again), of
        the blend plan (two memsets and one launch), the accumulate in each mode with every frame resident (one launch)
        and in chunks of 32 frames (a launch per chunk over the whole grid, frames ascending; the zeroing of acc is outside
        the timed region), and the finish (one launch);
        wm_mosaic_plan and wm_mosaic_fill_u8 on the same survey: what the blend costs over the hard mosaic;
      and -- once per setting -- the wall clock of the numpy restatement of the rule on the same input
      (tests/ground_oracle.py: blend_oracle_by_frame), whose best, cells, statistics, accumulators and pictures the
      device's must equal.  The settings are those of tools/mosaic_time.py: yawed nadir frames of 400 x 600 px of random
      content at UTM-sized coordinates, three to four frames per cell on average,
        f40_512      F = 40 on a 512 x 512 grid;
        f1000_8192   F = 1 000 on a 8192 x 8192 grid.
      Per setting the bytes the algorithm needs, counted from the shapes and the plan's own counts: per contributing (cell,
      frame) 3 (nearest) or 12 (bilinear) pixel bytes; per touched cell and call 32 accumulator bytes (16 read, 16
      written) and 8 of best; the finish 19 bytes per cell with a weight and 16 per cell without; with the minimum time
      that is a rate, printed as a fraction of the 8.0 TB/s of HBM.
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
from survey_bench_util import once, yawed_survey  # noqa: E402
from wildlifemapper_amd._survey import _frame_descs  # noqa: E402

H, W = 400, 600
OVERLAP = 3.5                 # mean frames per cell, were the frames spread evenly
HBM_PEAK = 8.0e12             # bytes per second
CHUNK = 32
MODES = (("nearest", N.MOSAIC_NEAREST, 3), ("bilinear", N.MOSAIC_BILINEAR, 12))


def run(case, reps, band, skip_oracle):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    F, gx, gy = case["g2p"].shape[0], case["gx"], case["gy"]
    g, s = up(case["g2p"]), up(case["size"])
    lib = N.lib()
    gen = torch.Generator(device=dev).manual_seed(case["seed"])
    pixels = torch.randint(0, 256, (F, H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    desc = _frame_descs([pixels[f] for f in range(F)], dev)
    index = torch.arange(F, device=dev, dtype=torch.int32)
    source = torch.empty((gy, gx), device=dev, dtype=torch.int32)
    won = torch.empty(F, device=dev, dtype=torch.int32)
    hstats = torch.empty(2, device=dev, dtype=torch.int64)
    best = torch.empty((gy, gx), device=dev, dtype=torch.float64)
    cells = torch.empty(F, device=dev, dtype=torch.int32)
    stats = torch.empty(3, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    acc = torch.zeros((gy, gx, 4), device=dev, dtype=torch.int32)
    hard_pic = torch.zeros((gy, gx, 3), device=dev, dtype=torch.uint8)
    pic = torch.zeros((gy, gx, 3), device=dev, dtype=torch.uint8)
    grid = (case["x0"], case["y0"], case["cell"], gx, gy)
    st = N.stream_ptr(dev)

    def accum(code, lo, hi):
        N.check(lib.wm_mosaic_blend_accum_u8(C_ptr(desc, lo * 16), C_ptr(index, lo * 4), hi - lo, N.ptr(g), N.ptr(s), F, None, *grid, band, N.ptr(best),
                                             code, N.ptr(acc), N.ptr(status), st))

    calls = {"hard_plan": lambda: N.check(lib.wm_mosaic_plan(N.ptr(g), N.ptr(s), F, *grid, N.ptr(source), N.ptr(won), N.ptr(hstats), st)),
             "blend_plan": lambda: N.check(lib.wm_mosaic_blend_plan(N.ptr(g), N.ptr(s), F, *grid, band, N.ptr(best), N.ptr(cells), N.ptr(stats), st))}
    for mode, code, _ in MODES:
        calls[f"hard_fill_{mode}"] = lambda code=code: N.check(lib.wm_mosaic_fill_u8(N.ptr(desc), F, N.ptr(index), N.ptr(g), N.ptr(s), F, *grid,
                                                                                      N.ptr(source), code, 0, N.ptr(hard_pic), N.ptr(status), st))
        calls[f"accum_{mode}_resident"] = lambda code=code: accum(code, 0, F)
        calls[f"accum_{mode}_chunks_of_{CHUNK}"] = lambda code=code: [accum(code, lo, min(lo + CHUNK, F)) for lo in range(0, F, CHUNK)]
    calls["finish"] = lambda: N.check(lib.wm_mosaic_blend_finish_u8(N.ptr(acc), gx, gy, 0, N.ptr(pic), st))      # on the accumulators just filled
    ms = {name: [] for name in calls}
    for rep in range(reps + 1):                               # the first round warms up and is dropped
        for name, call in calls.items():
            if name.startswith("accum"):
                acc.zero_()
                torch.cuda.synchronize()
            t = once(call)
            if rep:
                ms[name].append(t)
    seen, gap, blended = (int(v) for v in stats.cpu().tolist())
    contributions = int(cells.sum().item())
    out = {"frames": F, "grid": [gy, gx], "cell_m": round(case["cell"], 4), "band_px": band, "cells_seen": seen, "gap_cells": gap,
           "blended_cells": blended, "contributing_cell_frame_pairs": contributions, "frames_that_contribute": int((cells > 0).sum().item()),
           "status": int(status.item())}
    for name, v in ms.items():
        out[name + "_ms_min"], out[name + "_ms_median"] = round(float(np.min(v)), 4), round(float(np.median(v)), 4)
    # the bytes the algorithm needs.  Chunks: a cell is touched once per chunk that holds a frame contributing to it.
    for mode, _, px in MODES:
        need = px * contributions + (32 + 8) * seen
        out[f"accum_{mode}_resident_bytes"] = need
        out[f"accum_{mode}_resident_fraction_of_hbm_peak"] = round(need / (out[f"accum_{mode}_resident_ms_min"] * 1e-3) / HBM_PEAK, 4)
    need = 19 * seen + 16 * gap
    out["finish_bytes"] = need
    out["finish_fraction_of_hbm_peak"] = round(need / (out["finish_ms_min"] * 1e-3) / HBM_PEAK, 4)
    out["blend_plan_store_fraction_of_hbm_peak"] = round(8 * gx * gy / (out["blend_plan_ms_min"] * 1e-3) / HBM_PEAK, 4)
    for mode, _, _ in MODES:
        hard = out["hard_plan_ms_min"] + out[f"hard_fill_{mode}_ms_min"]
        blend = out["blend_plan_ms_min"] + out[f"accum_{mode}_resident_ms_min"] + out["finish_ms_min"]
        out[f"blend_over_hard_{mode}"] = round(blend / hard, 2)
    if not skip_oracle:
        from ground_oracle import blend_oracle_by_frame
        host = pixels.cpu().numpy()
        t = time.perf_counter()
        want = blend_oracle_by_frame(case["g2p"], case["size"], *grid, band, frames=host, fill=(0, 0, 0))
        out["oracle_host_s"] = round(time.perf_counter() - t, 2)
        equal = np.array_equal(want["best"], best.cpu().numpy()) and np.array_equal(want["cells"], cells.cpu().numpy()) and \
            want["stats"].tolist() == [seen, gap, blended]
        for mode, code, _ in MODES:
            for chunked in (False, True):
                acc.zero_()
                pic.zero_()
                calls[f"accum_{mode}_chunks_of_{CHUNK}" if chunked else f"accum_{mode}_resident"]()
                calls["finish"]()
                equal = equal and np.array_equal(want["acc_" + mode], acc.cpu().numpy().view(np.uint32)) and np.array_equal(want[mode], pic.cpu().numpy())
        out["equals_oracle"] = bool(equal)
    return out


def C_ptr(t, byte_offset):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--band", type=float, default=32.0)
    ap.add_argument("--skip-oracle", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    settings = {"f40_512": (40, 512), "f1000_8192": (1000, 8192)}
    out = {"reps": a.reps}
    for i, (name, (F, g)) in enumerate(settings.items()):
        if a.only in (None, name):
            case = dict(yawed_survey(np.random.default_rng(i), F, g, H, W, OVERLAP)[0], seed=i)
            out[name] = run(case, a.reps, a.band, a.skip_oracle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
