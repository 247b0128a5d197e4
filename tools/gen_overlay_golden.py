"""Golden vectors of the outline rule behind wm_draw_boxes_u8 (tests/test_overlay.py): what Pillow's own
ImageDraw.rectangle paints.

  python tools/gen_overlay_golden.py [--out tests/golden]

Two parts, Pillow and numpy only:
  * single rectangles on a 20 x 24 frame: widths 1..5, sides from width + 1 (the smallest Pillow-valid side: below it
    Pillow's line code paints outside the box, which the rule does not copy) to 13, at positions inside the frame, on each
    edge, across each edge and each corner, and wholly off the frame.  Stored: the inclusive rectangles (l, t, r, b), the
    widths and the painted masks (bit-packed);
  * a 40 x 56 RGB frame with overlapping outlines of several colours drawn one after another, at widths 2 and 3: the
    painter's order.
"""
import argparse
import os

import numpy as np
import PIL
from PIL import Image, ImageDraw

H, W = 20, 24
SCENE_H, SCENE_W = 40, 56
SCENE_RECTS = [(4, 5, 30, 25), (10, 10, 40, 30), (10, 10, 40, 30), (-3, 18, 12, 44), (25, -2, 58, 12), (28, 22, 33, 27),
               (0, 0, 55, 39), (20, 8, 27, 36), (38, 28, 50, 38), (12, 12, 38, 28)]
SCENE_LABELS = [0, 1, 2, 3, 4, 5, 6, 1, 0, 3]
PALETTE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (250, 250, 10), (10, 250, 250), (250, 10, 250), (128, 128, 128)]


def positions(sw, sh):
    """Top-left corners (l, t) for a box of sw x sh pixels."""
    return [(5, 4), (0, 6), (7, 0), (W - sw, 3), (6, H - sh), (-2, 5), (4, -3), (W - sw + 2, 2), (3, H - sh + 3), (-1, -1),
            (W - sw + 1, H - sh + 1), (W + 3, 4), (5, -sh - 2), (-sw - 1, 2), (2, H + 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    rects, widths, masks = [], [], []
    for width in range(1, 6):
        sides = sorted({width + 1, width + 2, 2 * width, 2 * width + 1, 13} - set(range(0, width + 1)))
        for sw in sides:
            for sh in sides:
                for l, t in positions(sw, sh):
                    r, b = l + sw - 1, t + sh - 1
                    im = Image.new("L", (W, H), 0)
                    ImageDraw.Draw(im).rectangle([l, t, r, b], outline=255, width=width)
                    rects.append((l, t, r, b))
                    widths.append(width)
                    masks.append(np.asarray(im) != 0)
    rects, widths, masks = np.array(rects, np.int32), np.array(widths, np.int32), np.array(masks)
    rng = np.random.default_rng(2028)
    scene = rng.integers(0, 200, (SCENE_H, SCENE_W, 3), dtype=np.uint8)
    painted = []
    for width in (2, 3):
        im = Image.fromarray(scene.copy(), "RGB")
        d = ImageDraw.Draw(im)
        for rc, lab in zip(SCENE_RECTS, SCENE_LABELS):
            d.rectangle(list(rc), outline=PALETTE[lab], width=width)
        painted.append(np.asarray(im))
    fx = {"frame_hw": np.array([H, W], np.int32), "rects": rects, "widths": widths, "masks": np.packbits(masks.reshape(len(masks), -1), axis=1),
          "scene": scene, "scene_rects": np.array(SCENE_RECTS, np.int32), "scene_labels": np.array(SCENE_LABELS, np.int32),
          "scene_palette": np.array(PALETTE, np.uint8), "scene_widths": np.array([2, 3], np.int32), "scene_painted": np.array(painted)}
    path = os.path.join(a.out, "overlay_pil.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB (Pillow", PIL.__version__ + "),", len(rects), "rectangles")


if __name__ == "__main__":
    main()
