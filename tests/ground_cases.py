"""What the ground tests (census, coverage, mosaic, blended mosaic) and their tools share as inputs: one case builder, the
hand frames, the named geometries aimed at the kernels' cull, the mosaic's cases that the blend re-uses, the sweeps of bad
arguments that check_coverage_grid / check_coverage_frames / check_n_resident (host_survey.h) must refuse, and a reader of
include/wm_hip.h.  Checkers' inputs only: nothing here asserts.  The rules themselves are in ground_oracle.py."""
import ctypes as C
import functools
import os
import re

import numpy as np

from ground_oracle import mosaic_oracle
from survey_util import ROOT, _axis, _kernel_constants, _some_frames, _yawed
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

F64 = np.float64
NAN = float("nan")
INF = float("inf")

# Frame A: 8 x 4 px (W x H), 0.5 m pixels, footprint [0, 4) x (0, 2] m, u = 2 X, v = 4 - 2 Y; frame B: the same, 2 m further east.
FRAME_A = ([2, 0, 0, 0, -2, 4], 4, 8)
FRAME_B = ([2, 0, -4, 0, -2, 4], 4, 8)


def _content(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _case(frames, x0, y0, cell, gx, gy, points=None, labels=None, images=None, seed=None):
    """frames: a list of (g2p as 6 numbers or (2,3), height, width).  points (P,2) with labels (P,): the coverage's points.
    images: one (H,W,3) uint8 array per frame; with a seed instead, random content for every frame of at least 1 x 1 px and
    None for the others; with neither, no pictures (None)."""
    g2p = np.array([np.asarray(f[0], dtype=F64).reshape(6) for f in frames], dtype=F64).reshape(-1, 6)
    size = np.array([[f[1], f[2]] for f in frames], dtype=np.int32).reshape(-1, 2)
    c = {"g2p": g2p, "size": size, "x0": float(x0), "y0": float(y0), "cell": float(cell), "gx": gx, "gy": gy, "points": None, "labels": None,
         "images": images}
    if points is not None:
        c["points"] = np.asarray(points, dtype=F64).reshape(-1, 2)
        c["labels"] = np.asarray(labels, dtype=np.int32).reshape(-1)
    if images is None and seed is not None:
        c["images"] = [_content(h, w, seed * 100003 + k) if h >= 1 and w >= 1 else None for k, (h, w) in enumerate(size.tolist())]
    return c


@functools.lru_cache(maxsize=None)
def _geometries():
    """name -> (frames, (x0, y0, cell, gx, gy)): the geometries the coverage and the mosaic tests aim at the same code, the
    staging of frames and the cull of blocks (CovBlock::may_touch)."""
    k = _kernel_constants()
    bx, by = k["block_x"], k["block_y"]
    wide = (0.0, 0.0, 1.0, 257, 65)
    c = 0.5
    return {
        "no_frames": ([], (0.0, 0.0, 0.7, 70, 19)),
        "cull_tiny_frame": ([_axis(100.25, 100.75, 40.25, 40.75, 8.0)], wide),          # 0.5 m of footprint around one centre, inside one block
        "cull_thin_between_rows": ([_axis(0.0, 257.0, 40.625, 40.875, 8.0)], wide),     # (40.625, 40.875]: between the rows of centres 40.5 and 41.5
        "cull_thin_on_one_row": ([_axis(0.0, 257.0, 40.375, 40.625, 8.0)], wide),       # (40.375, 40.625] holds the row of centres 40.5
        # a 1.5 m x 150 m strip and a 1 m one across the grid's blocks
        "cull_yaw_45": ([_yawed((128.0, 32.0), 0.05, 45.0, 30, 3000), _yawed((60.3, 30.1), 0.05, 135.0, 3000, 20)], wide),
        # centres at multiples of 0.5 m; footprints whose edges are the centres of the first cells of blocks: the west
        # edge is inside, the east edge outside; the north edge inside, the south edge outside
        "block_edges": ([_axis(bx * c, 2 * bx * c, (by - 1) * c, (2 * by - 1) * c, 2.0),            # columns bx..2bx-1, rows by..2by-1
                         _axis(0.0, bx * c, -c, (by - 1) * c, 2.0),                                   # block (0, 0) exactly
                         _axis(2 * bx * c, 4 * bx * c, (by - 1) * c, (2 * by - 1) * c, 2.0),          # east of the first, to the grid's edge region
                         _axis((bx - 1) * c, (bx + 1) * c, (by - 2) * c, by * c, 2.0)],               # 2 x 2 cells across a block corner
                        (-0.25, -0.25, c, 257, 65)),
    }


# ---- the mosaic's cases, which the blend runs too ------------------------------------------------------------------------

_MOSAIC_SEEDS = {"no_frames": 0, "cull_tiny_frame": 5, "cull_thin_between_rows": 6, "cull_thin_on_one_row": 7, "cull_yaw_45": 8, "block_edges": 10}


def _mosaic_oracle(case):
    return mosaic_oracle(case["g2p"], case["size"], case["x0"], case["y0"], case["cell"], case["gx"], case["gy"], case["images"])


@functools.lru_cache(maxsize=None)
def _mosaic_gpu_case(name):
    """name -> (case, mosaic_oracle's result), computed once."""
    k = _kernel_constants()
    if name in _MOSAIC_SEEDS:
        frames, grid = _geometries()[name]
        case = _case(frames, *grid, seed=_MOSAIC_SEEDS[name])
    elif name.startswith("grid_"):                                              # grid_<gx>x<gy>: none a multiple of the block
        gx, gy = (int(v) for v in name[5:].split("x"))
        case = _case(_some_frames(gx, gy, 0.7, gx, shapes=((30, 40), (17, 23), (40, 30), (9, 64), (33, 33))) + [_axis(-1.0, gx * 0.7 / 2, -1.0, gy, 0.5)], 0.0, 0.0, 0.7, gx, gy, seed=1)
    elif name == "one_1x1_px_frame":                                            # one pixel of 4 m over cells of 0.7 m
        case = _case([_axis(10.0, 14.0, 4.0, 8.0, 0.25)], 0.0, 0.0, 0.7, 70, 19, seed=2)
    elif name == "past_one_chunk":
        # the first COV_CHUNK frames are far away, not finite or without pixels, but for frame 10; of the frames after them,
        # the first has frame 10's georeference (an exact tie across the chunk boundary: 10 wins), the second overlaps frame
        # 10 and is nearer for some cells, the third lies alone
        ch = k["chunk"]
        ten = tiling.nadir_affine(30, 40, (16.0, 6.5), 0.5, 0.0)
        far = [_yawed((5000.0 + 40 * f, -3000.0), 0.1, 7.0 * f, 3, 4) for f in range(ch)]
        far[3] = ([2, NAN, 0, 0, -2, 4], 4, 8)
        far[100] = _axis(0.0, 49.0, 0.0, 13.0, 4.0)[:1] + (0, 196)
        far[10] = (tiling.ground_to_pixel(ten), 30, 40)
        near = [(tiling.ground_to_pixel(ten), 30, 40), _yawed((24.0, 6.5), 0.5, 0.0, 30, 40), _yawed((42.0, 8.0), 0.25, 115.0, 30, 40)]
        case = _case(far + near, 0.0, 0.0, 0.7, 70, 19, seed=3)
    elif name == "mixed_sizes_in_one_chunk":
        frames = [_axis(0.0, 32.0, 0.0, 12.0, 2.0), _axis(8.0, 40.0, 2.0, 10.0, 0.5), _axis(20.0, 49.0, 0.0, 13.0, 1.0),
                  _axis(30.0, 34.0, 4.0, 8.0, 0.25), _yawed((25.0, 6.0), 0.3, 30.0, 7, 90)]
        case = _case(frames, 0.0, 0.0, 0.7, 70, 19, seed=4)
    elif name == "cover_all":
        case = _case([_axis(-10.0, 300.0, -10.0, 100.0, 0.5), _yawed((128.0, 32.0), 2.0, 45.0, 300, 300)], 0.0, 0.0, 1.0, 257, 65, seed=9)
    elif name == "random_survey":
        rng = np.random.default_rng(11)
        x0, y0, cell, gx, gy = 500000.1, 4000000.7, 0.11, 128, 96                # 14.1 m x 10.6 m; a frame is 3.2 m x 2.4 m
        frames = [_yawed((x0 + rng.uniform(0, 14), y0 + rng.uniform(0, 10.5)), 0.05, rng.uniform(0, 360), 48, 64) for _ in range(40)]
        case = _case(frames, x0, y0, cell, gx, gy, seed=11)
    else:
        raise KeyError(name)
    return case, _mosaic_oracle(case)


def _mosaic_python_case():
    """Three overlapping yawed frames and a fourth off to the east, pixel -> ground georeferences."""
    E0, N0 = 500000.0, 4000000.0
    specs = [((E0 + 4.0, N0 + 3.0), 0.1, 10.0, 48, 64), ((E0 + 7.0, N0 + 3.5), 0.1, 40.0, 40, 56), ((E0 + 5.5, N0 + 5.0), 0.125, 200.0, 48, 64),
             ((E0 + 16.0, N0 + 3.0), 0.1, 0.0, 24, 32)]
    georef = np.stack([tiling.nadir_affine(H, W, c, gsd, yaw) for c, gsd, yaw, H, W in specs])
    sizes = np.array([(H, W) for *_, H, W in specs], dtype=np.int32)
    images = [_content(H, W, 50 + k) for k, (H, W) in enumerate(sizes.tolist())]
    return georef, sizes, images


# ---- the C-ABI without a GPU: fake pointers and the arguments every ground entry must refuse ------------------------------

def _p(v):
    """A fake device pointer for the paths that return before any HIP call: never dereferenced.  0 is NULL."""
    return C.c_void_p(v) if v else None


def last_error():
    return N.lib().wm_last_error().decode()


# Each sweep: (keyword arguments of an _abi_* call, a word its message must contain).  The test files loop and assert.
GRID_SWEEP = [({"gx": 0}, "gx"), ({"gx": N.COVERAGE_MAX_SIDE + 1}, "gx"), ({"gy": 0}, "gy"), ({"gy": -4}, "gy"), ({"gy": N.COVERAGE_MAX_SIDE + 1}, "gy"),
              ({"gx": 16384, "gy": 8192}, "gx * gy"), ({"gx": 8192, "gy": 8192 + 1}, "gx * gy")]
FRAME_SWEEP = [({"n_frames": -1}, "n_frames"), ({"n_frames": N.COVERAGE_MAX_FRAMES + 1}, "n_frames"), ({"g2p": 0}, "g2p_dev"), ({"size": 0}, "size_dev"),
               ({"g2p": 0x2004}, "aligned"), ({"size": 0x3002}, "aligned")]
ORIGIN_CELL_SWEEP = ([({k: bad}, k) for bad in (NAN, INF, -INF) for k in ("x0", "y0")] + [({"cell": bad}, "cell") for bad in (0.0, -1.0, NAN, INF)])
RESIDENT_SWEEP = [({"n_resident": -1}, "n_resident"), ({"n_resident": N.COVERAGE_MAX_FRAMES + 1}, "n_resident")]


# ---- include/wm_hip.h ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def header():
    with open(os.path.join(ROOT, "include", "wm_hip.h")) as f:
        return f.read()


def macro(name):
    """The integer value include/wm_hip.h gives the macro, or None."""
    m = re.search(r"#define %s (\d+)" % name, header())
    return int(m.group(1)) if m else None


def entry_is_whole(name, returns="int"):
    """An entry point is declared in the header with its return type, listed in _native.SYMBOLS and exported by the library."""
    return bool(name in N.SYMBOLS and re.search(r"\b%s %s\(" % (returns, name), header()) and getattr(N.lib(), name, None) is not None)
