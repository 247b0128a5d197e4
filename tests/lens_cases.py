"""The survey lens rule (include/wm_hip.h "Survey lens") restated for the tests, the cases they share, and the mutants that
show the cases have teeth.  The rule has no reference behaviour: lens_oracle is its restatement in numpy float64, the
header's expression statement for statement -- elementwise numpy arithmetic is one correctly rounded IEEE operation per
element and operator -- and the device must equal it byte for byte.  The inside test and the sampling are the ground
rules' (ground_oracle: inside, _sample_many), imported, not restated.

The host layer under test (wildlifemapper_amd.lens) is used only to turn keep='valid' / keep='all' into a size; every
expected byte comes from lens_oracle.  Nothing here asserts."""
import functools

import numpy as np

from ground_oracle import _sample_many, inside

F64 = np.float64
MODES = ("nearest", "bilinear")
FILL = (9, 8, 7)                      # not zero: a byte that was never written cannot pass for a filled one

SOURCE_SIZES = [(5, 7), (37, 53), (64, 129), (130, 257), (240, 320)]
OUT_WIDTHS = [1, 63, 64, 65, 129, 200]          # a full packed row, a partial last block, rows that start off a dword (3 * ow % 4 != 0)
OUT_HEIGHTS = [1, 15, 16, 17, 33]               # row counts around the 16 rows of a workgroup

BARREL = dict(k1=-0.28, k2=0.09, k3=-0.01)
PINCUSHION = dict(k1=0.2)
TANGENTIAL = dict(p1=0.001, p2=-0.0007)
FIVE = dict(BARREL, **TANGENTIAL)

MUTANTS = ("k1_negated", "p1_p2_swapped", "fx_fy_swapped", "cx_cy_swapped", "half_dropped", "rad_on_tangential", "inside_le")


def camera(size, f=None, fy_over_fx=1.0, off=(0.0, 0.0), k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """fx, fy, cx, cy, k1, k2, p1, p2, k3 for a frame of `size`: the principal point `off` = (dx, dy) pixels from the frame's
    centre ((w - 1) / 2, (h - 1) / 2 in OpenCV's convention), f defaulting to 0.83 of the width (a wide lens, and not dyadic)."""
    h, w = size
    f = 0.83 * w if f is None else f
    return np.array([f, f * fy_over_fx, (w - 1) / 2 + off[0], (h - 1) / 2 + off[1], k1, k2, p1, p2, k3], dtype=F64)


def _spanning(size, out_size, cam, span=1.12):
    """An f_out at which the output looks `span` times as far as the frame reaches along the tighter axis: fill and samples both."""
    (h, w), (oh, ow) = size, out_size
    return float(cam[0] * max(ow / w, oh / h) / span)


def _explicit(name, size, out_size, f_out=None, **cam):
    c = camera(size, **cam)
    return dict(name=name, size=size, camera=c, out_size=out_size, keep=None, f_out=_spanning(size, out_size, c) if f_out is None else f_out)


def _kept(name, size, keep, f_out=None, **cam):
    return dict(name=name, size=size, camera=camera(size, **cam), out_size=None, keep=keep, f_out=f_out)


# Every source size, every output width and height, every camera at least once.  The explicit sizes take an f_out that spans
# the frame (so does 'f_out_differs', by definition); the kept ones take the default, f_out = fx.
CASES = [
    _explicit("zero_1x1", (5, 7), (1, 1), f_out=0.83 * 7),
    _explicit("zero_dyadic_edge", (5, 7), (16, 64), f=64.0, f_out=64.0, off=(0.0, 0.0)),      # u == width and v == height are hit exactly
    _explicit("barrel_15x63", (5, 7), (15, 63), **BARREL),
    _explicit("pincushion_16x64", (37, 53), (16, 64), **PINCUSHION),
    _explicit("tangential_17x65", (37, 53), (17, 65), **TANGENTIAL),
    _explicit("five_33x129", (64, 129), (33, 129), **FIVE),
    _explicit("fx_ne_fy_15x200", (64, 129), (15, 200), fy_over_fx=1.07, **FIVE),
    _explicit("pp_off_33x200", (130, 257), (33, 200), off=(7.25, -7.25), **FIVE),
    _explicit("f_out_differs_17x129", (130, 257), (17, 129), f_out=0.61 * 0.83 * 257, **FIVE),
    _explicit("five_33x65", (240, 320), (33, 65), f=260.0, **FIVE),
    _explicit("barrel_1x200", (240, 320), (1, 200), **BARREL),
    _explicit("pincushion_33x1", (64, 129), (33, 1), **PINCUSHION),
    _kept("all_barrel", (37, 53), "all", **BARREL),
    _kept("all_pincushion", (240, 320), "all", f=0.45 * 320, **PINCUSHION),                # a very wide lens: the corners are well filled
    _kept("all_five_pp_off", (130, 257), "all", off=(7.25, -7.25), **FIVE),
    _kept("all_five_fx_ne_fy", (64, 129), "all", fy_over_fx=1.07, **FIVE),
    _kept("valid_barrel", (37, 53), "valid", **BARREL),
    _kept("valid_pincushion", (64, 129), "valid", **PINCUSHION),
    _kept("valid_five_pp_off", (130, 257), "valid", off=(7.25, -7.25), **FIVE),
    _kept("valid_zero", (5, 7), "valid"),
]
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
IDENTITY_SIZES = [(37, 53), (64, 129), (5, 7)]


def lens_oracle(img, cam, out_size, f_out, fill=FILL, modes=MODES, mutant=None):
    """The rule on a whole picture.  img (H,W,3) uint8, cam the nine numbers, out_size (oh, ow).  Returns {'nearest',
    'bilinear': (oh,ow,3) uint8, 'filled': the pixels that hold the fill colour because they look outside the frame}.
    mutant: one of MUTANTS, a deliberately wrong rule."""
    h, w = img.shape[:2]
    oh, ow = out_size
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (F64(v) for v in cam)
    f_out = F64(f_out)
    half = F64(0.5)
    if mutant == "k1_negated":
        k1 = -k1
    if mutant == "p1_p2_swapped":
        p1, p2 = p2, p1
    if mutant == "fx_fy_swapped":
        fx, fy = fy, fx
    if mutant == "cx_cy_swapped":
        cx, cy = cy, cx
    if mutant == "half_dropped":
        half = F64(0.0)                                        # the + 0.5 that turns OpenCV's cx, cy into pixel positions
    i = np.arange(ow, dtype=F64)[None, :]
    j = np.arange(oh, dtype=F64)[:, None]
    with np.errstate(all="ignore"):
        x = ((i + F64(0.5)) - F64(0.5) * F64(ow)) / f_out
        y = ((j + F64(0.5)) - F64(0.5) * F64(oh)) / f_out
        r2 = x * x + y * y
        rad = F64(1.0) + r2 * (k1 + r2 * (k2 + r2 * k3))
        tx = ((F64(2.0) * p1) * x) * y + p2 * (r2 + F64(2.0) * (x * x))
        ty = p1 * (r2 + F64(2.0) * (y * y)) + ((F64(2.0) * p2) * x) * y
        if mutant == "rad_on_tangential":
            tx, ty = tx * rad, ty * rad
        xd = x * rad + tx
        yd = y * rad + ty
        u = fx * xd + (cx + half)
        v = fy * yd + (cy + half)
        u, v = np.broadcast_to(u, (oh, ow)), np.broadcast_to(v, (oh, ow))
        sees = inside(u, v, h, w)
        if mutant == "inside_le":
            sees = (0 <= u) & (u <= w) & (0 <= v) & (v <= h)
            u, v = np.minimum(u, F64(w) - F64(0.25)), np.minimum(v, F64(h) - F64(0.25))    # the edge itself reads the last pixel
    out = {"filled": int((~sees).sum())}
    for m in modes:
        pic = np.empty((oh, ow, 3), dtype=np.uint8)
        pic[:] = np.asarray(fill, dtype=np.uint8)
        if sees.any():
            pic[sees] = _sample_many(img, u[sees], v[sees], m)
        out[m] = pic
    return out


def resolve(case):
    """(camera, size, out_size, f_out) of a case: keep= goes through lens_plan, the host layer under test."""
    from wildlifemapper_amd import lens
    if case["keep"] is None:
        pl = lens.lens_plan(case["camera"], case["size"], out_size=case["out_size"], f_out=case["f_out"])
    else:
        pl = lens.lens_plan(case["camera"], case["size"], keep=case["keep"], f_out=case["f_out"])
    return pl


def source_image(case):
    """The case's frame: noise, so that a position off by a fraction of a pixel changes bytes."""
    h, w = case["size"]
    return np.random.default_rng(1000 + CASE_NAMES.index(case["name"])).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(plan, frame, lens_oracle's dict) of a case, computed once for all the tests that need it; treat as read-only."""
    case = BY_NAME[name]
    pl = resolve(case)
    img = source_image(case)
    return pl, img, lens_oracle(img, pl["camera"], pl["out_size"], pl["f_out"])
