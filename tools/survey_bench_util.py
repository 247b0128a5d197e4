"""What tools/*_time.py share: the HIP-event timer and the synthetic yawed survey of coverage_time.py and mosaic_time.py."""
import numpy as np
import torch

from wildlifemapper_amd import tiling


def once(call):
    """Milliseconds of one call() between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(call, reps, warmup=1, together=False):
    """`warmup` untimed calls and a synchronize, then (min, median) ms over `reps` calls timed one by one, rounded to
    0.1 us.  together: one pair of events around all `reps` calls instead, and their mean ms, unrounded."""
    for _ in range(warmup):
        call()
    if warmup:
        torch.cuda.synchronize()
    if together:
        return once(lambda: [call() for _ in range(reps)]) / reps
    ms = [once(call) for _ in range(reps)]
    return round(float(np.min(ms)), 4), round(float(np.median(ms)), 4)


def yawed_survey(rng, F, g, H=400, W=600, overlap=3.5, gsd=0.05, x0=500000.1, y0=6000000.7):
    """F nadir frames of H x W px at random yaw and UTM-sized coordinates over a g x g grid whose side is chosen so that a
    cell is seen by `overlap` frames on average, were they spread evenly.  Draws from rng (centre east, north, yaw per
    frame).  Returns (the case: g2p (F,6), size (F,2) int32, x0, y0, cell, gx, gy; the grid's side in metres)."""
    side = (F * H * W * gsd * gsd / overlap) ** 0.5
    georef = np.stack([tiling.nadir_affine(H, W, (x0 + rng.uniform(0, side), y0 + rng.uniform(0, side)), gsd, rng.uniform(0, 360))
                       for _ in range(F)])
    return {"g2p": tiling.ground_to_pixel(georef).reshape(-1, 6), "size": np.tile(np.array([[H, W]], dtype=np.int32), (F, 1)),
            "x0": x0, "y0": y0, "cell": side / g, "gx": g, "gy": g}, side
