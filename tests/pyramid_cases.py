"""What tests/test_register_pyramid.py, tests/test_register_refine.py and tools/register_time.py share beyond register_cases.py:
the restatement of the pyramid's rule (include/wm_hip.h "Survey registration, pyramid"), the planes the device tests reduce,
and the loop of tiling.refine(levels=L) -- coarse to fine, levels=0 the plain loop -- on register_cases.py's analytic scene with
the oracles' planes and sums in the device's place.  Nothing here asserts about a device."""
import numpy as np
import torch

from register_cases import CELL, SIDE, SIZES, SUMS, _corner_error, _oracle_sums, analytic_scene, refine_sums_oracle, render_plane
from survey_util import DEV, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling


def reduce_oracle(planes, level):
    """The rule, one level at a time, in int64: (..., ext, ext) -> (..., ext >> level, ext >> level) uint8.  A cell is 0 if any
    of the four under it is 0, else (their sum + 2) >> 2."""
    r = np.asarray(planes).astype(np.int64)
    assert r.shape[-1] == r.shape[-2] and r.shape[-1] % (1 << level) == 0 and level >= 0
    for _ in range(level):
        a, b, c, d = r[..., 0::2, 0::2], r[..., 0::2, 1::2], r[..., 1::2, 0::2], r[..., 1::2, 1::2]
        r = np.where((a == 0) | (b == 0) | (c == 0) | (d == 0), 0, (a + b + c + d + 2) >> 2)
    assert r.min(initial=0) >= 0 and r.max(initial=0) <= 255
    return r.astype(np.uint8)


# ---- the planes of the device tests ------------------------------------------------------------------------------------

REDUCE_SHAPES = ((2, 1), (4, 2), (6, 1), (8, 3), (36, 2), (64, 6), (66, 1), (72, 3), (128, 6), (130, 1), (200, 3), (514, 1), (576, 6),
                 (640, 6))                                                           # (ext, level)


def masked_planes(ext, level, n_planes, masked=True):
    """(n_planes, ext, ext) uint8 of random 1..255, a different plane per index.  masked: plane p is 0 where j > i + p * ext
    // 8 -- a half-plane across a diagonal, a footprint's edge -- and, where the output has at least 4 x 4 cells, at three
    single cells of the seen part below the first row of output cells.  Where the output is one cell per plane, a diagonal
    would zero every plane: there the odd planes stay whole, so a stack of three holds both kinds."""
    rng = np.random.default_rng(1000 * ext + 10 * level + n_planes)
    planes = rng.integers(1, 256, size=(n_planes, ext, ext), dtype=np.uint8)
    if not masked:
        return planes
    out_side, block = ext >> level, 1 << level
    j, i = np.meshgrid(np.arange(ext), np.arange(ext), indexing="ij")
    for p in range(n_planes):
        if out_side == 1 and p % 2:
            continue
        t = p * ext // 8
        planes[p][j > i + t] = 0
        if out_side >= 4:
            for _ in range(3):
                jj = int(rng.integers(block, ext - t - 1))
                ii = int(rng.integers(jj + t, ext))
                planes[p, jj, ii] = 0
    return planes


def device_reduce(planes, level, poison=0x5A, guard=256):
    """wm_register_reduce_u8 on host planes (P, ext, ext): the output sits `guard` bytes into a buffer filled with `poison`, with
    `guard` more bytes behind it.  Returns (out (P, ext >> level, ext >> level), the bytes before, the bytes behind, the input
    as it came back), all host arrays."""
    n, ext = planes.shape[0], planes.shape[1]
    oe = ext >> level
    src = _up(planes)
    buf = torch.full((guard + n * oe * oe + guard,), poison, device=DEV, dtype=torch.uint8)
    out = buf[guard:guard + n * oe * oe]
    N.check(N.lib().wm_register_reduce_u8(N.ptr(src), n, ext, level, N.ptr(out), N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    return host[guard:guard + n * oe * oe].reshape(n, oe, oe), host[:guard], host[guard + n * oe * oe:], src.cpu().numpy()


# ---- the loop of tiling.refine on the oracles ------------------------------------------------------------------------

def coarse_tables(table, level):
    """The pair table of level `level`, restated: gx >> level, gy >> level, same frames, x0 and y0.  Returns (the table whose gx
    and gy the sums are computed for, 0 for a pair that takes no part; the table refine_step is given, 1 in their place)."""
    t = table.copy()
    t["gx"], t["gy"] = table["gx"] >> level, table["gy"] >> level
    gone = (t["gx"] < 1) | (t["gy"] < 1)
    t["gx"][gone], t["gy"][gone] = 0, 0
    h = t.copy()
    h["gx"][gone], h["gy"][gone] = 1, 1
    return t, h


def pyramid_sums_oracle(frames, georef, sizes, table, cell, side, level):
    """The sums of one iteration at `level`: render_plane at search 2^level, reduce_oracle, refine_sums_oracle at search 1."""
    if level == 0:
        return _oracle_sums(frames, georef, sizes, table, cell, side)
    g2p = tiling.ground_to_pixel(georef).reshape(-1, 6)
    s, out = 1 << level, []
    for pr, cpr in zip(table, coarse_tables(table, level)[0]):
        fa, fb, gx, gy = (int(pr[k]) for k in ("frame_a", "frame_b", "gx", "gy"))
        if cpr["gx"] < 1:
            out.append([0] * SUMS)
            continue
        A = render_plane(g2p[fa], sizes[fa], frames[fa], pr["x0"], pr["y0"], cell, gx, gy, 0, side)
        B = render_plane(g2p[fb], sizes[fb], frames[fb], pr["x0"], pr["y0"], cell, gx, gy, s, side + 2 * s)
        out.append(refine_sums_oracle(reduce_oracle(A, level), reduce_oracle(B, level), int(cpr["gx"]), int(cpr["gy"]), 1))
    return np.array(out, dtype=np.int64).reshape(len(table), SUMS)




_LOOPS = {}


def oracle_loop(scene, levels, iters, exposure, table=None, min_cells=4096):
    """tiling.refine(levels=, iters=, exposure=, fixed=[0])'s loop on analytic_scene(scene) with the oracles' planes and sums in
    the device's place; levels=0 is the plain loop.  Computed once per key.  'steps' holds refine_step's result of every
    iteration, 'levels' its level, 'errors' the worst corner error after it."""
    key = (scene, levels, iters, exposure, None if table is None else table.tobytes(), min_cells)
    if key not in _LOOPS:
        frames, true, pert = analytic_scene(scene)
        table = tiling.register_pairs(pert, SIZES, CELL, 1, SIDE, min_cells) if table is None else table
        cur, steps, at = pert, [], []
        for l in range(levels, -1, -1):
            host_table = coarse_tables(table, l)[1]
            for _ in range(iters):
                sums = pyramid_sums_oracle(frames, cur, SIZES, table, CELL, SIDE, l)
                steps.append(tiling.refine_step(cur, SIZES, host_table, sums, CELL * (1 << l), exposure, max(1, min_cells >> (2 * l)), 2.0, [0]))
                at.append(l)
                cur = steps[-1]["georef"]
        _LOOPS[key] = {"georef": cur, "table": table, "steps": steps, "levels": at, "errors": [_corner_error(s["georef"], true) for s in steps]}
    return _LOOPS[key]


def point_sampled_loop(cell, iters):
    """The documented workaround as a record: the plain loop on the far-off scene at a coarser, point-sampled cell (side and
    min_cells scaled with it)."""
    frames, true, pert = analytic_scene("far")
    k = int(round(cell / CELL))
    side, min_cells = SIDE // k, max(1, 4096 // (k * k))
    table = tiling.register_pairs(pert, SIZES, cell, 1, side, min_cells)
    cur, errors = pert, []
    for _ in range(iters):
        cur = tiling.refine_step(cur, SIZES, table, _oracle_sums(frames, cur, SIZES, table, cell, side), cell, False, min_cells, 2.0, [0])["georef"]
        errors.append(_corner_error(cur, true))
    return errors
