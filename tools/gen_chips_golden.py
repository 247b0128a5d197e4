"""Golden vectors of wm_crop_chips_u8 (tests/test_chips.py): one small seeded uint8 frame, boxes, the windows the chip rule
(include/wm_hip.h) gives them, and the chips Pillow's own bilinear resize (PIL.Image.resize(..., BILINEAR)) makes of the
zero-padded crops.

  python tools/gen_chips_golden.py [--out tests/golden]

The rule is restated here in numpy float32, so the fixture depends on Pillow and numpy only.  The boxes cover windows
inside the frame and hanging off each edge and corner, wholly outside it, around it, the identity (side == chip), up- and
down-scaling, the min_side and max_side clamps, a zero-size box and a NaN box (window (0, 0, 0), zero chip).
"""
import argparse
import os

import numpy as np
import PIL
from PIL import Image

H, W, CHIP = 96, 131, 32
CONTEXT, MIN_SIDE, MAX_SIDE = 1.5, 8, 1024
BOXES = [
    (10.2, 20.7, 30.9, 33.1),        # side 32: the identity
    (-5, -5, 3, 2),                  # off the top-left corner, up-scaled
    (0, 0, 5000, 10),                # max_side: far larger than the frame
    (120, 80, 140, 100),             # off the bottom-right corner
    (60, 40, 61, 41),                # min_side
    (20, 10, 100, 90),               # down by 3.75, past the top and bottom
    (0, 0, 131, 96),                 # around the whole frame
    (65.5, 48, 65.5, 48),            # zero size
    (200, 200, 220, 220),            # wholly outside
    (-100, -100, -80, -90),          # wholly outside, negative
    (50, -20, 80, 20),               # off the top
    (-10, 30, 25, 70),               # off the left
    (100, 30, 150, 60),              # off the right
    (40, 70, 70, 120),               # off the bottom
    (30.5, 30.5, 51.5, 52.0),        # side 33: just below the identity
    (5, 5, 25.5, 25),                # side 31: just above it
    (float("nan"), 0, 10, 10),       # not finite: window (0, 0, 0), zero chip
]


def chip_window(box, context, min_side, max_side):
    f = np.float32
    x0, y0, x1, y1 = (f(v) for v in box)
    if not all(np.isfinite(v) for v in (x0, y0, x1, y1)):
        return (0, 0, 0)
    m = max(f(x1 - x0), f(y1 - y0))
    s = np.ceil(f(m * f(context)))
    side = int(min(max(s, f(min_side)), f(max_side)))
    cx, cy = f(f(x0 + x1) * f(0.5)), f(f(y0 + y1) * f(0.5))
    half = f(f(0.5) * f(side))
    lim = f(2.0 ** 30)
    wx = min(max(np.floor(f(cx - half)), -lim), lim)
    wy = min(max(np.floor(f(cy - half)), -lim), lim)
    return (int(wy), int(wx), side)


def zero_padded_crop(frame, window):
    y0, x0, side = window
    out = np.zeros((side, side, 3), np.uint8)
    ya, yb = max(y0, 0), min(y0 + side, frame.shape[0])
    xa, xb = max(x0, 0), min(x0 + side, frame.shape[1])
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = frame[ya:yb, xa:xb]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    rng = np.random.default_rng(2027)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = np.array(BOXES, dtype=np.float32)
    windows = np.array([chip_window(b, CONTEXT, MIN_SIDE, MAX_SIDE) for b in boxes], dtype=np.int32)
    chips = np.zeros((len(boxes), CHIP, CHIP, 3), np.uint8)
    for i, w in enumerate(windows):
        if w[2] > 0:
            chips[i] = np.asarray(Image.fromarray(zero_padded_crop(frame, w), "RGB").resize((CHIP, CHIP), Image.BILINEAR))
    fx = {"frame": frame, "boxes": boxes, "windows": windows, "chips": chips,
          "params": np.array([CONTEXT, MIN_SIDE, MAX_SIDE, CHIP], dtype=np.float64)}
    path = os.path.join(a.out, "chips_pil.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB (Pillow", PIL.__version__ + ")")
    print(windows.tolist())


if __name__ == "__main__":
    main()
