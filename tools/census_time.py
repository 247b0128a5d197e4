"""Times of the survey census (wm_census) against the host route a caller had before.

  python tools/census_time.py [--reps 20] [--skip-oracle]
      HIP-event min and median over --reps repetitions of one wm_census call (its single launch; buffers and scratch are
      allocated once, outside the timed region), the rounds its resolution took, and -- once each -- the wall clock of
      census_oracle (tests/ground_oracle.py: the sequential numpy restatement, the host route) on the same inputs, whose
      result the device's must equal.  Three settings, radius 1 m, every animal seen by 3 frames with 0.15 m of noise:
        survey_2000     n = 2 000, F = 40, 2 animals per 100 m^2;
        survey_50000    n = 50 000, F = 1 000, 2 animals per 100 m^2;
        herd_5000       n = 5 000, F = 12, all in 60 x 60 m.
      Prints one JSON line.
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

GSD = 0.05
RADIUS = 1.0


def make(n, F, side_m, seed):
    """n detections: n / 3 animals uniform in a side_m square, each seen by 3 different frames; boxes in pixels of GSD."""
    rng = np.random.default_rng(seed)
    animals = rng.uniform(0, side_m, (n // 3 + 1, 2))
    pos = np.repeat(animals, 3, axis=0)[:n] + rng.normal(0, 0.15, (n, 2))
    first = rng.integers(0, F, n // 3 + 1)
    frame = ((np.repeat(first, 3)[:n] + np.tile(np.arange(3), n // 3 + 1)[:n] * max(1, F // 7)) % F).astype(np.int32)
    org = rng.uniform(-50, 50, (F, 2))
    georef = np.array([[[GSD, 0, ox], [0, -GSD, oy]] for ox, oy in org])
    px = np.stack([(pos[:, 0] - org[frame, 0]) / GSD, (pos[:, 1] - org[frame, 1]) / -GSD], axis=1)
    half = rng.uniform(8, 30, (n, 2))
    boxes = np.concatenate([px - half, px + half], axis=1).astype(np.float32)
    return {"boxes": boxes, "scores": rng.uniform(0.1, 1.0, n).astype(np.float32), "labels": rng.integers(0, 7, n).astype(np.int32),
            "frame": frame, "georef": georef}


def run(case, reps, skip_oracle):
    dev = torch.device("cuda:0")
    n = case["boxes"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    boxes, scores, labels, frame = up(case["boxes"]), up(case["scores"]), up(case["labels"]), up(case["frame"])
    g = up(case["georef"].reshape(-1, 6))
    lib = N.lib()
    nbytes = lib.wm_census_scratch_bytes(n)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    points = torch.empty((n, 2), device=dev, dtype=torch.float64)
    individual, keeper, members = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(3))
    count = torch.empty(2, device=dev, dtype=torch.int32)

    def call():
        N.check(lib.wm_census(N.ptr(boxes), N.ptr(scores), N.ptr(labels), N.ptr(frame), n, N.ptr(g), g.shape[0], RADIUS, 0,
                              N.ptr(scratch), nbytes, N.ptr(points), N.ptr(individual), N.ptr(keeper), N.ptr(members), N.ptr(count),
                              N.stream_ptr(dev)))
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    k, status = count.cpu().tolist()
    out = {"n": n, "frames": int(g.shape[0]), "individuals": k, "status": status,
           "rounds": int(scratch[:4].view(torch.int32).item()),
           "ms_min": round(float(np.min(ms)), 4), "ms_median": round(float(np.median(ms)), 4)}
    if not skip_oracle:
        from ground_oracle import census_oracle
        t = time.perf_counter()
        want = census_oracle(case["boxes"], case["scores"], case["labels"], case["frame"], case["georef"], RADIUS)
        out["oracle_host_s"] = round(time.perf_counter() - t, 2)
        out["equals_oracle"] = bool(want["count"] == k and np.array_equal(want["individual"], individual.cpu().numpy()) and
                                    np.array_equal(want["keeper"], keeper[:k].cpu().numpy()) and
                                    np.array_equal(want["points"].view(np.int64), points.cpu().numpy().view(np.int64)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-oracle", action="store_true")
    a = ap.parse_args()
    density = 2.0 / 100.0
    settings = {"survey_2000": (2000, 40, (2000 / 3 / density) ** 0.5), "survey_50000": (50000, 1000, (50000 / 3 / density) ** 0.5),
                "herd_5000": (5000, 12, 60.0)}
    out = {"reps": a.reps, "radius_m": RADIUS}
    for i, (name, (n, F, side)) in enumerate(settings.items()):
        out[name] = run(make(n, F, side, i), a.reps, a.skip_oracle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
