"""Golden vectors of wm_resample_u8 (tests/test_resample.py): seeded uint8 frames and what Pillow's own bilinear resize
(PIL.Image.resize(..., BILINEAR), the arithmetic of the reference's val transform, dataloader_coco.py:288) makes of them.

  python tools/gen_resample_golden.py [--out tests/golden]

The geometries cover the library's kernel paths: the column-blocked horizontal pass at 17 taps (the reference scale
0.128) and at few taps, the generic one above 20 taps, outputs wider than 1024 columns, upscaling, an unchanged axis
(Pillow skips that pass), 1-pixel sides, and row lengths that are not a multiple of 4 bytes.  The frames are kept
small: the tap counts and block layouts depend on the ratio and the output width, not on the frame size.
"""
import argparse
import os

import numpy as np
import PIL
from PIL import Image

# (name, (H, W), (oh, ow))
CASES = [
    ("down_0p128_17taps", (64, 125), (8, 16)),
    ("down_27taps_generic", (36, 150), (3, 12)),
    ("wide_17taps_ow1152", (2, 9000), (1, 1152)),
    ("wide_5taps_ow1400_long_rows", (4, 1500), (3, 1400)),
    ("up_1p7", (20, 30), (34, 51)),
    ("rows_unchanged", (10, 120), (10, 31)),
    ("cols_unchanged", (120, 10), (31, 10)),
    ("one_row", (1, 500), (1, 64)),
    ("to_one_column", (300, 7), (37, 1)),
    ("to_one_row", (90, 40), (1, 13)),
    ("from_one_pixel", (1, 1), (5, 3)),
    ("ow_mod4_down", (37, 61), (21, 27)),
    ("ow_mod4_up", (13, 17), (29, 39)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    fx = {"names": np.array([c[0] for c in CASES])}
    for i, (name, (h, w), (oh, ow)) in enumerate(CASES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        fx[f"in_{i}"] = img
        fx[f"out_{i}"] = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR))
        assert fx[f"out_{i}"].shape == (oh, ow, 3), name
    path = os.path.join(a.out, "resample_pil.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, sum(v.nbytes for v in fx.values()) // 1024, "KiB (Pillow", PIL.__version__ + ")")


if __name__ == "__main__":
    main()
