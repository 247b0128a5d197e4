"""Survey registration: the georeferences of overlapping frames corrected by matching their pixels.
  * register_pairs: the overlapping pairs of a survey and their ground patches, on the host;
  * register: every pair's two frames rendered onto its patch (wm_register_render_u8) and the offset between them searched
    (wm_register_search: sums of absolute differences; wm_register_search_zncc: zero-mean normalised correlation, which
    survives exposure changes), a chunk of pairs and a few resident frames at a time (rule: include/wm_hip.h "Survey
    registration");
  * adjust: one translation per frame from the accepted pairs' offsets, a weighted least-squares bundle adjustment in
    numpy double;
  * refine: below one cell -- the sub-cell shift, yaw and scale of every frame (and the gain and offset between exposures)
    from the integer normal equations of one Gauss-Newton step per pair (wm_register_refine; rule: include/wm_hip.h "Survey
    registration, refinement"), iterated; its host parts are refine_solve (the 4 x 4 or 6 x 6 solve per pair),
    adjust_similarity (one similarity per frame, two calls of adjust) and refine_step (both, and the corrected georef);
  * reduce_planes: rendered planes reduced by 2 x 2 rounded means (wm_register_reduce_u8; rule: include/wm_hip.h "Survey
    registration, pyramid"); refine(levels=L) runs the same step on them coarse to fine, so it converges from far off;
  * adjust_exposure, exposure_table: one gain and one offset per frame from the pairs' exposure fits, two calls of adjust,
    and the Q12 table of them that mosaic(blend=, exposure=) applies."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

import torch

from . import _native as N
from ._survey import _check_whole, _finite_number, _pinned_upload, _whole_number
from .ground import (COVERAGE_MAX_FRAMES, _check_cell, _check_georef, _check_sizes, _footprint_extent, _frame_sequence, _frame_tables,
                     _resident_chunk, _survey_device)

REGISTER_MAX_SIDE = N.REGISTER_MAX_SIDE       # include/wm_hip.h WM_REGISTER_MAX_SIDE
REGISTER_MAX_SEARCH = N.REGISTER_MAX_SEARCH   # WM_REGISTER_MAX_SEARCH
REGISTER_MAX_PAIRS = N.REGISTER_MAX_PAIRS     # WM_REGISTER_MAX_PAIRS, per launch: register() chunks by pair_chunk
# wm_register_pair, 32 bytes: the patch of a pair is gx x gy cells with south-west corner (x0, y0)
REGISTER_PAIR = np.dtype([("frame_a", "<i4"), ("frame_b", "<i4"), ("gx", "<i4"), ("gy", "<i4"), ("x0", "<f8"), ("y0", "<f8")])
REGISTER_MAX_LEVEL = N.REGISTER_MAX_LEVEL     # WM_REGISTER_MAX_LEVEL: 2 x 2 reductions per wm_register_reduce_u8 call
_REGISTER_FRAMES_RESIDENT = 8                 # frames on the device per render call of register()


def _check_register_shape(search, side, min_cells, what: str):
    search = _check_whole(search, what, "search", 0)
    side = _check_whole(side, what, "side")
    min_cells = _check_whole(min_cells, what, "min_cells")
    if search > REGISTER_MAX_SEARCH:
        raise ValueError(f"{what}: search {search} exceeds {REGISTER_MAX_SEARCH}")
    if side > REGISTER_MAX_SIDE:
        raise ValueError(f"{what}: side {side} exceeds {REGISTER_MAX_SIDE}")
    if min_cells >= 2 ** 31:
        raise ValueError(f"{what}: min_cells {min_cells} does not fit int32")
    return search, side, min_cells


def _check_pair_table(pairs, n_frames: int, side: int, what: str) -> np.ndarray:
    """A (P,) array of REGISTER_PAIR as register_pairs returns it, every entry inside the limits of include/wm_hip.h."""
    if not isinstance(pairs, np.ndarray) or pairs.dtype != REGISTER_PAIR or pairs.ndim != 1:
        raise ValueError(f"{what}: pairs must be a (P,) array of tiling.REGISTER_PAIR, as register_pairs returns it")
    t = np.ascontiguousarray(pairs)
    if t.size:
        a, b = t["frame_a"], t["frame_b"]
        if a.min() < 0 or b.min() < 0 or a.max() >= n_frames or b.max() >= n_frames or np.any(a == b):
            raise ValueError(f"{what}: pairs: frame_a and frame_b must be two different frames in 0..{n_frames - 1}")
        if t["gx"].min() < 1 or t["gy"].min() < 1 or t["gx"].max() > side or t["gy"].max() > side:
            raise ValueError(f"{what}: pairs: gx and gy must lie in 1..side ({side})")
        if not (np.isfinite(t["x0"]).all() and np.isfinite(t["y0"]).all()):
            raise ValueError(f"{what}: pairs: x0 and y0 must be finite")
    return t


def _check_pair_chunk(pair_chunk, what: str) -> int:
    pair_chunk = _check_whole(pair_chunk, what, "pair_chunk")
    if pair_chunk > REGISTER_MAX_PAIRS:
        raise ValueError(f"{what}: pair_chunk {pair_chunk} exceeds {REGISTER_MAX_PAIRS}")
    return pair_chunk


def _pair_frames(pairs, what: str) -> np.ndarray:
    """(frame_a, frame_b) of a REGISTER_PAIR table or a (P,2) array of whole numbers, as (P,2) int64: adjust()'s check of pairs."""
    if isinstance(pairs, np.ndarray) and pairs.dtype == REGISTER_PAIR:
        pairs = np.stack([pairs["frame_a"], pairs["frame_b"]], axis=1) if pairs.size else np.zeros((0, 2), dtype=np.int64)
    try:
        ab = np.asarray(pairs)
        if ab.size == 0:
            ab = ab.reshape(0, 2)
        if ab.dtype.kind not in "iu" or ab.ndim != 2 or ab.shape[1] != 2:
            raise TypeError
        return ab.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: pairs must be a REGISTER_PAIR table or a (P,2) array of whole numbers") from None


def register_pairs(georef, sizes, cell, search: int = 16, side: int = 512, min_cells: int = 4096) -> np.ndarray:
    """The overlapping pairs of a survey and their ground patches, for register().  Host only, in double.  georef (F,2,3)
    float64 as for census(), sizes (F,2) (height, width), cell metres.  A pair (i < j) is proposed when the axis-aligned
    ground bounding boxes of the two footprints (the extent of the corners (0, 0), (W, 0), (0, H), (W, H)) intersect with
    a positive area.  Its patch is that intersection snapped outward to multiples of cell -- i0 = floor(lo / cell), i1 =
    ceil(hi / cell), gx = i1 - i0, x0 = i0 * cell, the same north -- so the patches of all pairs lie on one lattice; a
    patch wider than `side` cells is centre-cropped (i0 += (gx - side) // 2, gx = side); a patch of fewer than min_cells
    cells is dropped.  A frame whose georeference is not finite or whose size is below 1 x 1 is in no pair.  search is
    only validated here (the patch does not depend on it).  Returns a (P,) array of REGISTER_PAIR (frame_a, frame_b, gx,
    gy, x0, y0), ordered by (frame_a, frame_b)."""
    what = "register_pairs"
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    search, side, min_cells = _check_register_shape(search, side, min_cells, what)
    F = g.shape[0]
    ok, X, Y = _footprint_extent(g, s)
    with np.errstate(all="ignore"):
        xl, xh, yl, yh = X.min(axis=1), X.max(axis=1), Y.min(axis=1), Y.max(axis=1)
    out = []
    for i in range(F):
        if not ok[i]:
            continue
        js = np.arange(i + 1, F)
        lo_x, hi_x = np.maximum(xl[i], xl[js]), np.minimum(xh[i], xh[js])
        lo_y, hi_y = np.maximum(yl[i], yl[js]), np.minimum(yh[i], yh[js])
        for k in np.nonzero(ok[js] & (lo_x < hi_x) & (lo_y < hi_y))[0]:
            i0, i1 = math.floor(lo_x[k] / cell), math.ceil(hi_x[k] / cell)
            j0, j1 = math.floor(lo_y[k] / cell), math.ceil(hi_y[k] / cell)
            gx, gy = i1 - i0, j1 - j0
            if gx > side:
                i0, gx = i0 + (gx - side) // 2, side
            if gy > side:
                j0, gy = j0 + (gy - side) // 2, side
            if gx < 1 or gy < 1 or gx * gy < min_cells:
                continue
            out.append((i, int(js[k]), gx, gy, i0 * cell, j0 * cell))
    return np.array(out, dtype=REGISTER_PAIR).reshape(-1)


def adjust(n_frames, pairs, measured, weights, fixed=None) -> Dict[str, np.ndarray]:
    """One translation per frame from pairwise measurements: weighted least squares of t_b - t_a = m_p.  Host only, numpy
    double.  pairs: a REGISTER_PAIR table or a (P,2) array of (frame_a, frame_b); measured (P,2) metres (east, north);
    weights (P,) >= 0 -- register() passes the cells n of an accepted pair and 0 for a rejected one; a pair of weight 0 is
    not part of the system or of the graph.  The system is stacked with rows sqrt(w_p) * (t_b - t_a) = sqrt(w_p) * m_p and
    solved by numpy.linalg.lstsq, whose minimum-norm solution fixes what the measurements leave free: in a connected
    component of the graph without a fixed frame the mean shift of its frames is zero.  fixed: frames that stay at 0 (their
    columns are left out), which pins every component that holds one.  A frame with no pair of positive weight keeps 0.
    Returns 'shift' (n_frames,2) metres, to be added to (a2, a5); 'residual' (P,2) = (t_b - t_a) - m_p for every pair,
    whatever its weight; 'component' (n_frames,) int64, the lowest frame index of the frame's component, -1 for a frame
    with no pair of positive weight."""
    what = "adjust"
    F = _check_whole(n_frames, what, "n_frames", 0)
    ab = _pair_frames(pairs, what)
    P = ab.shape[0]
    if P and (ab.min() < 0 or ab.max() >= F or np.any(ab[:, 0] == ab[:, 1])):
        raise ValueError(f"{what}: pairs: frame_a and frame_b must be two different frames in 0..{F - 1}")
    try:
        m = np.asarray(measured, dtype=np.float64).reshape(-1, 2) if np.size(measured) else np.zeros((0, 2))
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: measured must be (P,2) numbers and weights (P,) numbers") from None
    if m.shape != (P, 2) or w.shape != (P,):
        raise ValueError(f"{what}: {P} pairs, measured of shape {m.shape} and weights of shape {w.shape}: expected ({P}, 2) and ({P},)")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f"{what}: weights must be finite and >= 0")
    used = w > 0
    if not np.isfinite(m[used]).all():
        raise ValueError(f"{what}: measured must be finite where the weight is positive")
    fixed_a = np.zeros(F, dtype=bool)
    if fixed is not None:
        try:
            fx = np.asarray(list(fixed))
            if fx.size and (fx.dtype.kind not in "iu" or fx.ndim != 1 or fx.min() < 0 or fx.max() >= F):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{what}: fixed {fixed!r} must be frame indices in 0..{F - 1}") from None
        fixed_a[fx.astype(np.int64)] = True
    # components of the graph of used pairs: union-find, labelled by their lowest frame
    root = np.arange(F)

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    for a, b in ab[used]:
        ra, rb = find(a), find(b)
        if ra != rb:
            root[max(ra, rb)] = min(ra, rb)
    in_graph = np.zeros(F, dtype=bool)
    in_graph[ab[used].reshape(-1)] = True
    component = np.array([find(f) if in_graph[f] else -1 for f in range(F)], dtype=np.int64).reshape(F)
    shift = np.zeros((F, 2), dtype=np.float64)
    cols = np.nonzero(in_graph & ~fixed_a)[0]
    if cols.size and used.any():
        col_of = np.full(F, -1, dtype=np.int64)
        col_of[cols] = np.arange(cols.size)
        rows = np.nonzero(used)[0]
        sw = np.sqrt(w[rows])
        A = np.zeros((rows.size, cols.size), dtype=np.float64)
        ca, cb = col_of[ab[rows, 0]], col_of[ab[rows, 1]]
        r = np.arange(rows.size)
        A[r[ca >= 0], ca[ca >= 0]] = -sw[ca >= 0]
        A[r[cb >= 0], cb[cb >= 0]] = sw[cb >= 0]
        t = np.linalg.lstsq(A, m[rows] * sw[:, None], rcond=None)[0]
        shift[cols] = t
    with np.errstate(all="ignore"):
        residual = (shift[ab[:, 1]] - shift[ab[:, 0]]) - m
    return {"shift": shift, "residual": residual, "component": component}


REGISTER_METRICS = ("sad", "zncc")


def _decode_sad(best, peak, min_corr):
    """best (P,8) -> has, has2, mean, runner_up, corr, confident: best's third of four is sad (-1: none), the fourth n."""
    sad, n1, sad2, n2 = (best[:, k].astype(np.int64) for k in (2, 3, 6, 7))
    has, has2 = sad >= 0, sad2 >= 0
    mean = np.where(has, sad / np.maximum(n1, 1), np.nan)
    runner = np.where(has2, sad2 / np.maximum(n2, 1), np.nan)
    return has, has2, mean, runner, np.full(best.shape[0], np.nan), has


def _decode_zncc(best, peak, min_corr):
    """best (P,8), peak (P,2) -> the same six: best's third of four is ok (1 / 0), peak holds q (NaN: none)."""
    has, has2 = best[:, 2] == 1, best[:, 6] == 1
    r = np.sign(peak) * np.sqrt(np.abs(peak))
    corr = np.where(has, r[:, 0], np.nan)
    mean = np.where(has, 1.0 - r[:, 0], np.nan)
    runner = np.where(has2, 1.0 - r[:, 1], np.nan)
    return has, has2, mean, runner, corr, has & (corr > min_corr)


# per metric: the entry point, its table's dtype and last dimension, whether it fills a peak buffer, best[2] of "none", the decoder
_REGISTER_METRIC = {"sad": ("wm_register_search", torch.int32, 2, False, -1, _decode_sad),
                    "zncc": ("wm_register_search_zncc", torch.int64, 6, True, 0, _decode_zncc)}


def _render_chunk(lib, frames, chunk, s, g_d, s_d, cell, search, side, status, dev, what):
    """The planes of one chunk of pairs, as register() and refine() render them: the chunk's frames go up a few at a time,
    one wm_register_render_u8 call each, and are released after it.  Returns (pairs_d, plane_a, plane_b) on dev."""
    n, F, E = chunk.shape[0], s.shape[0], side + 2 * search
    pairs_d = _pinned_upload(chunk.view(np.uint8).reshape(n, REGISTER_PAIR.itemsize), dev)
    plane_a = torch.empty((n, side, side), device=dev, dtype=torch.uint8)
    plane_b = torch.empty((n, E, E), device=dev, dtype=torch.uint8)
    needed = sorted(set(chunk["frame_a"].tolist()) | set(chunk["frame_b"].tolist()))
    for f0 in range(0, len(needed), _REGISTER_FRAMES_RESIDENT):
        ids = needed[f0:f0 + _REGISTER_FRAMES_RESIDENT]
        desc, slot_d, resident = _resident_chunk(frames, ids, s, dev, what)
        N.check(lib.wm_register_render_u8(N.ptr(desc), len(ids), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, N.ptr(pairs_d), n,
                                          cell, search, side, N.ptr(plane_a), N.ptr(plane_b), N.ptr(status), N.stream_ptr(dev)))
        del resident, desc, slot_d                    # the stream orders their reuse after the launch
    return pairs_d, plane_a, plane_b


def _rendered_chunks(lib, frames, table, pair_chunk, s, g_d, s_d, cell, search, side, status, dev, what):
    """One pass of register() or refine() over a pair table: yields (c0, n, *_render_chunk(table[c0:c0 + n])) pair_chunk pairs at
    a time, then reads `status` (one device-to-host copy) and refuses planes the renders skipped.  Nothing yielded is kept here:
    the caller lets go of a chunk's planes (del) before it asks for the next, so at most one chunk's planes are alive."""
    for c0 in range(0, table.shape[0], pair_chunk):
        chunk = table[c0:c0 + pair_chunk]
        yield (c0, chunk.shape[0], *_render_chunk(lib, frames, chunk, s, g_d, s_d, cell, search, side, status, dev, what))
    bad = int(status.item())
    if bad:
        raise RuntimeError(f"{what}: wm_register_render_u8 skipped planes (status {bad}): a resident frame did not match its slot or size")


def _check_survey(frames, georef, cell, sizes, pairs, search, side, min_cells, fixed, what):
    """What register() and refine() check of a survey after their own arguments, in this order: frames, cell, georef, sizes, the
    frame count, the pair table (`pairs`, or register_pairs at this search) and fixed=.  Returns (cell, georef, sizes, table)."""
    n_given, sizes = _frame_sequence(frames, sizes, what, "the frames of the current chunk of pairs")
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    F = g.shape[0]
    if F > COVERAGE_MAX_FRAMES:
        raise ValueError(f"{what}: {F} frames exceed {COVERAGE_MAX_FRAMES}")
    if n_given != F:
        raise ValueError(f"{what}: {n_given} frames for {F} georeferences")
    table = register_pairs(g, s, cell, search, side, min_cells) if pairs is None else _check_pair_table(pairs, F, side, what)
    adjust(F, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 2)), np.zeros(0), fixed)         # fixed= validated before device work
    return cell, g, s, table


def _check_levels(levels, side: int, what: str) -> int:
    """levels of refine() and register(): a whole number in 0..REGISTER_MAX_LEVEL (no bool, no float) with side % 2^levels == 0."""
    levels = _whole_number(levels, what, "levels", 0, REGISTER_MAX_LEVEL, must=f"must be a whole number in 0..{REGISTER_MAX_LEVEL}")
    if side % (1 << levels):
        raise ValueError(f"{what}: levels {levels} needs a side that 2^levels = {1 << levels} divides, and side is {side}")
    return levels


def _reduce(lib, planes: torch.Tensor, level: int, dev) -> torch.Tensor:
    """One wm_register_reduce_u8 call on a checked (P, ext, ext) uint8 stack on dev."""
    n, ext = planes.shape[0], planes.shape[1]
    out = torch.empty((n, ext >> level, ext >> level), device=dev, dtype=torch.uint8)
    N.check(lib.wm_register_reduce_u8(N.ptr(planes), n, ext, level, N.ptr(out), N.stream_ptr(dev)))
    return out


def reduce_planes(planes, level) -> torch.Tensor:
    """A stack of rendered planes reduced by 2 x 2 rounded means, `level` times (wm_register_reduce_u8; rule: include/wm_hip.h
    "Survey registration, pyramid").  planes: a contiguous (P, ext, ext) uint8 device tensor, as wm_register_render_u8 writes
    it, ext <= REGISTER_MAX_SIDE + 2 * REGISTER_MAX_SEARCH and P <= REGISTER_MAX_PAIRS; level a whole number in
    1..REGISTER_MAX_LEVEL with ext % 2^level == 0.  Per level a cell is 0 -- not seen -- if any of the four cells under it
    is 0, else (their sum + 2) >> 2, with that rounding at every level.  Everything is validated before any device work.  Runs
    on the planes' device and its current stream.  No CPU fallback.  Returns a new (P, ext >> level, ext >> level) uint8 tensor
    on the same device."""
    what = "reduce_planes"
    level = _whole_number(level, what, "level", 1, REGISTER_MAX_LEVEL, must=f"must be a whole number in 1..{REGISTER_MAX_LEVEL}")
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[1] != planes.shape[2]:
        raise ValueError(f"{what}: planes must be a (P, ext, ext) uint8 tensor, as wm_register_render_u8 writes it")
    P, ext = int(planes.shape[0]), int(planes.shape[1])
    if ext < 1 or ext > REGISTER_MAX_SIDE + 2 * REGISTER_MAX_SEARCH:
        raise ValueError(f"{what}: planes: ext {ext} outside 1..{REGISTER_MAX_SIDE + 2 * REGISTER_MAX_SEARCH}")
    if ext % (1 << level):
        raise ValueError(f"{what}: planes: ext {ext} is not a multiple of 2^level = {1 << level}")
    if P > REGISTER_MAX_PAIRS:
        raise ValueError(f"{what}: planes: {P} planes exceed {REGISTER_MAX_PAIRS}")
    if not planes.is_contiguous():
        raise ValueError(f"{what}: planes must be contiguous")
    if not planes.is_cuda:
        raise RuntimeError(f"{what}: planes is on {planes.device}; the HIP path needs a ROCm device tensor "
                           "(there is no CPU fallback in wildlifemapper_amd)")
    with torch.cuda.device(planes.device):
        return _reduce(N.lib(), planes, level, planes.device)


def register(frames, georef, cell, sizes=None, search: int = 16, side: int = 512, min_cells: int = 4096, min_ratio: float = 1.25,
             pairs=None, fixed=None, pair_chunk: int = 256, metric: str = "sad", min_corr: float = 0.0, refine: int = 0, levels: int = 0) -> Dict[str, object]:
    """Correct the georeferences of a survey by matching the pixels of its overlapping frames (wm_register_render_u8,
    wm_register_search or wm_register_search_zncc; rule: include/wm_hip.h "Survey registration" and "Survey registration,
    correlation search").  frames as mosaic() takes them: a sequence that is
    only indexed -- tensors, arrays, or a lazy sequence that loads frame i when asked; georef (F,2,3) float64 as for
    census(); cell metres; sizes (F,2) may be None only for a list of tensors or arrays.  pairs: the table to use, None for
    register_pairs(georef, sizes, cell, search, side, min_cells).  Everything is validated before any device work.
    The pairs are rendered and searched pair_chunk at a time, so the planes stay bounded (pair_chunk * (side^2 + (side +
    2 * search)^2) bytes); within a chunk its frames go up a few at a time and are released after their render call, so a
    frame is read only while a pair of the current chunk needs it (a frame shared by two chunks is read once per chunk).
    A pair is ACCEPTED iff a best offset exists (some offset has n >= min_cells), |dy| < search and |dx| < search (a peak
    on the window's edge is not a peak), and the runner-up outside the peak's 3 x 3 has a mean absolute difference of at
    least min_ratio times the peak's (sad2 / n2 >= min_ratio * (sad / n), in double); a runner-up that does not exist also
    accepts.  The accepted pairs, each measuring t_b - t_a = -(dx, dy) * cell with weight n, go to adjust(fixed=fixed).
    metric: "sad" (the default) is the rule above, masked sums of absolute differences; it assumes the same exposure in
    both frames of a pair (no gain or offset is fitted).  Where exposure changes between frames -- auto-exposure, cloud
    shadow -- use metric="zncc": the offsets are scored by the zero-mean normalised correlation, which a gain and an offset
    between the two frames do not change.  With r = sign(q) * sqrt(|q|) of the device's signed squared correlation q, a
    pair is then accepted iff a best offset exists (n >= min_cells and neither plane flat), |dy| < search and |dx| <
    search, r > min_corr (finite, in [-1, 1)), and the runner-up does not exist or 1 - r2 >= min_ratio * (1 - r): 1 - r
    takes the part of the mean absolute difference, so min_ratio keeps its meaning.  Both defaults are policy, not
    measurements on real imagery.  A cell coarser than the ground
    sampling distance point-samples, so shrink the frames first (preprocess.resample_u8, resampled_georef).  The search
    itself corrects only a translation per frame, at a resolution of one cell; refine=k > 0 follows it with k iterations of
    refine() on the corrected georef and the same pair table -- the sub-cell shift, the yaw and the scale of every frame,
    with exposure=(metric == "zncc") -- and adds one key, 'refine', its result ('refine'['georef'] is the refined
    georeference).  With refine=0 nothing changes, neither the keys nor the launches.  levels=L > 0 is passed to that refine():
    refine iterations at each of the levels L, L - 1, ... 0 of a pyramid of the planes, for a yaw or a scale that leaves the
    patch corners more than about two cells off; it needs refine > 0 and side % 2^L == 0, else ValueError.
    Runs on the current device's current stream.  No CPU fallback.  Returns host arrays:
      'georef' (F,2,3) float64 corrected (shift added to a2, a5), 'shift' (F,2) metres, 'pairs' the table,
      'offset' (P,2) int64 cells (dx, dy), 'cells' (P,) int64 n at the best offset (0: none), 'mean' (P,) float64 sad / n
      (NaN: none), 'runner_up' (P,) float64 sad2 / n2 (NaN: none), 'accepted' (P,) bool, 'residual' (P,2) metres after
      the adjustment, 'component' (F,) int64 as adjust() gives it, 'corr' (P,) float64 NaN.  Under metric="zncc" 'mean'
      is 1 - r and 'runner_up' 1 - r2 (NaN: none), and 'corr' is r (NaN: none)."""
    what = "register"
    if not isinstance(metric, str) or metric not in REGISTER_METRICS:
        raise ValueError(f"{what}: metric {metric!r} must be one of {REGISTER_METRICS}")
    must = "must be a finite number in [-1, 1)"
    min_corr = _finite_number(min_corr, what, "min_corr", lambda r: -1.0 <= r < 1.0, must, must, refuse=bool, echo_float=True)
    entry, table_dtype, table_last, has_peak, none, decode = _REGISTER_METRIC[metric]
    search, side, min_cells = _check_register_shape(search, side, min_cells, what)
    pair_chunk = _check_pair_chunk(pair_chunk, what)
    refine = _check_whole(refine, what, "refine", 0)
    levels = _check_levels(levels, side, what)
    if levels and not refine:
        raise ValueError(f"{what}: levels {levels} without refine: the pyramid belongs to the refinement, pass refine >= 1")
    must = "must be a finite number >= 0"
    min_ratio = _finite_number(min_ratio, what, "min_ratio", lambda r: r >= 0.0, must, must, echo_float=True)
    cell, g, s, table = _check_survey(frames, georef, cell, sizes, pairs, search, side, min_cells, fixed, what)
    F, P = g.shape[0], table.shape[0]
    best = np.zeros((P, 8), dtype=np.int32)
    peak = np.full((P, 2), np.nan, dtype=np.float64)                 # (q, q2) of the correlation search
    best[:, 2] = best[:, 6] = none
    if P:
        dev = _survey_device(what)
        lib = N.lib()
        with torch.cuda.device(dev):
            g_d, s_d = _frame_tables(g, s, dev)
            status = torch.zeros(1, device=dev, dtype=torch.int32)
            for c0, n, pairs_d, plane_a, plane_b in _rendered_chunks(lib, frames, table, pair_chunk, s, g_d, s_d, cell, search, side, status, dev, what):
                best_d =torch.empty((n, 8), device=dev, dtype=torch.int32)
                score = torch.empty((n, 2 * search + 1, 2 * search + 1, table_last), device=dev, dtype=table_dtype)
                peak_d = torch.empty((n, 2), device=dev, dtype=torch.float64) if has_peak else None
                N.check(getattr(lib, entry)(N.ptr(plane_a), N.ptr(plane_b), N.ptr(pairs_d), n, search, side, min_cells, N.ptr(score),
                                            N.ptr(best_d), *([N.ptr(peak_d)] if has_peak else []), N.stream_ptr(dev)))
                if has_peak:
                    peak[c0:c0 + n] = peak_d.cpu().numpy()
                best[c0:c0 + n] = best_d.cpu().numpy()
                del plane_a, plane_b, score, best_d, peak_d, pairs_d          # before the next chunk renders
    dy, dx, n1 = (best[:, k].astype(np.int64) for k in (0, 1, 3))
    with np.errstate(all="ignore"):
        has, has2, mean, runner, corr, confident = decode(best, peak, min_corr)
        accepted = confident & (np.abs(dy) < search) & (np.abs(dx) < search) & (~has2 | (runner >= min_ratio * mean))
    offset = np.stack([dx, dy], axis=1).reshape(P, 2)
    adj = adjust(F, table, -offset.astype(np.float64) * cell, np.where(accepted, n1, 0).astype(np.float64), fixed)
    out_g = g.copy()
    out_g[:, 0, 2] += adj["shift"][:, 0]
    out_g[:, 1, 2] += adj["shift"][:, 1]
    out = {"georef": out_g, "shift": adj["shift"], "pairs": table, "offset": offset, "cells": np.where(has, n1, 0), "mean": mean,
           "runner_up": runner, "accepted": accepted, "residual": adj["residual"], "component": adj["component"], "corr": corr}
    if refine:
        out["refine"] = _refine(frames, out_g, cell, sizes=s, pairs=table, side=side, min_cells=min_cells, iters=refine,
                                exposure=metric == "zncc", fixed=fixed, pair_chunk=pair_chunk, levels=levels)
    return out


REGISTER_REFINE_SUMS = N.REGISTER_REFINE_SUMS     # include/wm_hip.h WM_REGISTER_REFINE_SUMS
_TRI = [(k, l) for k in range(6) for l in range(k, 6)]           # the order of the 21 products in a pair's sums


def _check_refine_policy(min_cells, max_step, exposure, what: str):
    min_cells = _check_whole(min_cells, what, "min_cells")
    must = "must be a finite number > 0"
    max_step = _finite_number(max_step, what, "max_step", lambda r: r > 0.0, must, must, refuse=bool, echo_float=True)
    if not isinstance(exposure, (bool, np.bool_)):
        raise ValueError(f"{what}: exposure {exposure!r} must be True or False")
    return min_cells, max_step, bool(exposure)


def _check_sums(sums, what: str) -> np.ndarray:
    a = np.asarray(sums)
    if a.size == 0:
        a = a.reshape(0, REGISTER_REFINE_SUMS).astype(np.int64)
    if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != REGISTER_REFINE_SUMS:
        raise ValueError(f"{what}: sums must be a (P, {REGISTER_REFINE_SUMS}) array of whole numbers, as wm_register_refine writes it")
    return a.astype(np.int64)


def refine_solve(sums, pairs, exposure: bool = False, min_cells: int = 4096, max_step: float = 2.0) -> Dict[str, np.ndarray]:
    """The parameters of every pair from its sums (wm_register_refine; rule and signs: include/wm_hip.h "Survey
    registration, refinement").  Host only, numpy double.  sums (P,28) int64; pairs the (P,) REGISTER_PAIR table (gx and gy
    are read).  With N the symmetric matrix of the 21 products and R the six sums c_k * r, N q = R is solved per pair --
    the leading 4 x 4, or all 6 x 6 with exposure=True, which also fits the gain and the offset between the two frames --
    after the symmetric diagonal scaling N_kl / sqrt(N_kk N_ll), which brings the columns (grey-level differences next to
    their products with cell offsets of hundreds) to one magnitude.  A pair is ACCEPTED iff its counted cells n >=
    min_cells, the system solves (a diagonal entry that is not positive, numpy.linalg.LinAlgError or a result that is not
    finite rejects; nothing is raised), and the displacement |d| of the solution at the four corners of the patch is at
    most max_step cells.  max_step = 2.0 is policy -- the basin of one linearisation of planes sampled a cell apart -- not a
    measurement.  Returns 'param' (P,6) float64 (tx, ty in cells, theta radians counter-clockwise, sigma, gamma, o; gamma
    and o are 0 when exposure is false; NaN where nothing was solved), 'cells' (P,) int64 n, 'rms' (P,) float64 sqrt(sum r^2
    / n) of the planes as they are (NaN: n = 0), 'accepted' (P,) bool."""
    what = "refine_solve"
    min_cells, max_step, exposure = _check_refine_policy(min_cells, max_step, exposure, what)
    sm = _check_sums(sums, what)
    P = sm.shape[0]
    if not isinstance(pairs, np.ndarray) or pairs.dtype != REGISTER_PAIR or pairs.shape != (P,):
        raise ValueError(f"{what}: pairs must be the ({P},) array of tiling.REGISTER_PAIR that the sums were computed for")
    m = 6 if exposure else 4
    param = np.full((P, 6), np.nan)
    n = sm[:, 20].copy()
    accepted = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        rms = np.where(n > 0, np.sqrt(sm[:, 27] / np.maximum(n, 1)), np.nan)
    for p in range(P):
        if n[p] < 1:
            continue
        Nm = np.zeros((6, 6))
        for v, (k, l) in zip(sm[p, :21].astype(np.float64), _TRI):
            Nm[k, l] = Nm[l, k] = v
        diag = np.diag(Nm)[:m]
        if not (diag > 0).all():
            continue
        d = 1.0 / np.sqrt(diag)
        try:
            with np.errstate(all="ignore"):
                q = d * np.linalg.solve(Nm[:m, :m] * d[:, None] * d[None, :], d * sm[p, 21:21 + m].astype(np.float64))
        except np.linalg.LinAlgError:
            continue
        if not np.isfinite(q).all():
            continue
        q = np.concatenate([q, np.zeros(6 - m)])
        param[p] = (2.0 * q[0], 2.0 * q[1], 4.0 * q[2], 4.0 * q[3], q[4], q[5])
        tx, ty, th, sg = param[p, :4]
        hx, hy = 0.5 * float(pairs["gx"][p]), 0.5 * float(pairs["gy"][p])
        step = max(math.hypot(tx - th * y + sg * x, ty + th * x + sg * y) for x in (-hx, hx) for y in (-hy, hy))
        accepted[p] = bool(n[p] >= min_cells and step <= max_step)
    return {"param": param, "cells": n, "rms": rms, "accepted": accepted}


def adjust_similarity(n_frames, pairs, patch_centres, frame_centres, measured, weights, fixed=None) -> Dict[str, np.ndarray]:
    """One similarity per frame from pairwise measurements, u_f(X) = t_f + (theta_f J + sigma_f I)(X - c_f) with J = [[0, -1],
    [1, 0]]: the correction of frame f at the ground position X.  Host only, numpy double, in two calls of adjust().
    pairs as adjust() takes them; patch_centres (P,2) the c_p, frame_centres (n_frames,2) the c_f, metres; measured (P,4) =
    (dx, dy, theta, sigma) of the field d(X) = (dx, dy) + (theta J + sigma I)(X - c_p) by which B's content appears
    displaced relative to A's, dx and dy in metres; weights (P,) >= 0.  With u_b(X) - u_a(X) = -d(X):
      first (theta, sigma) from theta_b - theta_a = -theta_m, sigma_b - sigma_a = -sigma_m;
      then t from t_b - t_a = -(dx, dy) - (theta_b J + sigma_b I)(c_p - c_b) + (theta_a J + sigma_a I)(c_p - c_a).
    The gauge is adjust()'s, in both calls: in a component without a fixed frame the mean yaw, the mean scale and the mean
    shift of its frames are zero; fixed frames do not move; a frame with no pair of positive weight keeps the identity.
    Returns 'shift' (n_frames,2) the t_f, 'yaw' (n_frames,) the theta_f, 'scale' (n_frames,) the sigma_f, 'residual' (P,4)
    (the translation's two, then yaw's and scale's) and 'component' as adjust() gives it."""
    what = "adjust_similarity"
    F = _check_whole(n_frames, what, "n_frames", 0)
    try:
        m = np.asarray(measured, dtype=np.float64).reshape(-1, 4) if np.size(measured) else np.zeros((0, 4))
        cp = np.asarray(patch_centres, dtype=np.float64).reshape(-1, 2) if np.size(patch_centres) else np.zeros((0, 2))
        cf = np.asarray(frame_centres, dtype=np.float64).reshape(-1, 2) if np.size(frame_centres) else np.zeros((0, 2))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: measured must be (P,4), patch_centres (P,2) and frame_centres (n_frames,2) numbers") from None
    P = m.shape[0]
    if cp.shape != (P, 2) or cf.shape != (F, 2):
        raise ValueError(f"{what}: measured of shape {m.shape}, patch_centres of shape {cp.shape}, frame_centres of shape {cf.shape}: "
                         f"expected ({P}, 4), ({P}, 2) and ({F}, 2)")
    first = adjust(F, pairs, -m[:, 2:4], weights, fixed)                       # validates pairs, weights and fixed
    yaw, scale = first["shift"][:, 0], first["shift"][:, 1]
    ab = _pair_frames(pairs, what)
    a, b = ab[:, 0], ab[:, 1]

    def linear(f, v):                                                          # (theta_f J + sigma_f I) v
        return np.stack([scale[f] * v[:, 0] - yaw[f] * v[:, 1], yaw[f] * v[:, 0] + scale[f] * v[:, 1]], axis=1)

    with np.errstate(all="ignore"):
        want_t = -m[:, :2] - linear(b, cp - cf[b]) + linear(a, cp - cf[a])
    used = np.asarray(weights, dtype=np.float64).reshape(-1) > 0
    if not np.isfinite(want_t[used]).all():
        raise ValueError(f"{what}: measured, patch_centres and frame_centres must be finite where the weight is positive")
    second = adjust(F, ab, want_t, weights, fixed)
    return {"shift": second["shift"], "yaw": yaw.copy(), "scale": scale.copy(),
            "residual": np.concatenate([second["residual"], first["residual"]], axis=1).reshape(P, 4), "component": second["component"]}


def adjust_exposure(n_frames, pairs, param, weights, fixed=None) -> Dict[str, np.ndarray]:
    """One gain and one offset per frame from the pairwise exposure fits: the exposure analogue of adjust().  Host only,
    numpy double, in two calls of adjust().  pairs as adjust() takes them; param (P,6) as refine_solve(exposure=True) and
    refine(..., exposure=True) return it, of which only gamma = param[:, 4] and o = param[:, 5] are read: the pair model is
    A ~ (1 + gamma) * B + o on luma.  With L'_f = k_f * L_f + c_f the corrected luma of frame f, two frames agree where they
    overlap when k_b = k_a * (1 + gamma) and c_b = c_a + k_a * o:
      first ln k from ln k_b - ln k_a = ln(1 + gamma);
      then c from c_b - c_a = k_a * o, with the solved k.
    weights (P,) >= 0; a pair whose gamma or o is not finite, or whose 1 + gamma <= 0, gets weight 0.  From refine(...,
    exposure=True): weights = np.where(out['accepted'], out['cells'], 0).  The gauge is adjust()'s, in both calls: in a
    component without a fixed frame the mean ln k and the mean c of its frames are zero; fixed frames keep (1, 0); a frame
    without a used pair keeps (1, 0).  Returns 'gain' (n_frames,) the k_f, 'offset' (n_frames,) the c_f in grey levels,
    'residual' (P,2) (ln k's, then c's; NaN for a pair that could not be used) and 'component' as adjust() gives it.
    exposure_table() turns 'gain' and 'offset' into the table mosaic(blend=, exposure=) takes."""
    what = "adjust_exposure"
    F = _check_whole(n_frames, what, "n_frames", 0)
    try:
        par = np.asarray(param, dtype=np.float64)
        if par.size == 0:
            par = par.reshape(0, 6)
        if par.ndim != 2 or par.shape[1] != 6:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: param must be (P,6) numbers, as refine_solve returns it") from None
    P = par.shape[0]
    gamma, o = par[:, 4], par[:, 5]
    with np.errstate(all="ignore"):
        usable = np.isfinite(gamma) & np.isfinite(o) & (1.0 + gamma > 0.0)
        ln_g = np.where(usable, np.log(np.where(usable, 1.0 + gamma, 1.0)), np.nan)
    try:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: weights must be (P,) numbers") from None
    if w.shape != (P,):
        raise ValueError(f"{what}: {P} pairs and weights of shape {w.shape}: expected ({P},)")
    w = np.where(usable, w, np.where(np.isfinite(w) & (w >= 0), 0.0, w))          # a bad weight still reaches adjust()'s check
    first = adjust(F, pairs, np.stack([ln_g, np.zeros(P)], axis=1), w, fixed)     # validates pairs, weights and fixed
    gain = np.exp(first["shift"][:, 0])
    ab = _pair_frames(pairs, what)
    with np.errstate(all="ignore"):
        want_c = np.where(usable, gain[ab[:, 0]] * o, np.nan)
    second = adjust(F, ab, np.stack([want_c, np.zeros(P)], axis=1), w, fixed)
    return {"gain": gain, "offset": second["shift"][:, 0].copy(),
            "residual": np.stack([first["residual"][:, 0], second["residual"][:, 0]], axis=1).reshape(P, 2), "component": second["component"]}


def exposure_table(gain, offset) -> np.ndarray:
    """adjust_exposure()'s gains and offsets as the Q12 table of wm_mosaic_blend_accum_u8 (include/wm_hip.h "Survey mosaic,
    blended"): (F,2) int32 (floor(gain * 4096 + 0.5), floor(offset * 4096 + 0.5)).  gain (F,) finite in [1/16, 16), offset
    (F,) grey levels with |offset| <= 255, else ValueError: beyond them the fit is not an exposure change.  (1, 0) gives
    (4096, 0), the identity."""
    what = "exposure_table"
    try:
        k = np.asarray(gain, dtype=np.float64).reshape(-1) if np.size(gain) else np.zeros(0)
        c = np.asarray(offset, dtype=np.float64).reshape(-1) if np.size(offset) else np.zeros(0)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: gain and offset must be (F,) numbers") from None
    if np.ndim(gain) > 1 or np.ndim(offset) > 1 or k.shape != c.shape:
        raise ValueError(f"{what}: gain of shape {np.shape(gain)} and offset of shape {np.shape(offset)}: expected (F,) and (F,)")
    if not (np.isfinite(k).all() and (k >= 1.0 / 16.0).all() and (k < 16.0).all()):
        raise ValueError(f"{what}: every gain must be finite in [1/16, 16)")
    if not (np.isfinite(c).all() and (np.abs(c) <= 255.0).all()):
        raise ValueError(f"{what}: every offset must be finite with |offset| <= 255")
    return np.stack([np.floor(k * 4096.0 + 0.5), np.floor(c * 4096.0 + 0.5)], axis=1).astype(np.int32).reshape(-1, 2)


def _frame_centres(g: np.ndarray, s: np.ndarray) -> np.ndarray:
    """The ground position of every frame's centre pixel (width / 2, height / 2) under g, (F,2)."""
    u, v = 0.5 * s[:, 1].astype(np.float64), 0.5 * s[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([g[:, 0, 0] * u + g[:, 0, 1] * v + g[:, 0, 2], g[:, 1, 0] * u + g[:, 1, 1] * v + g[:, 1, 2]], axis=1)


def refine_step(georef, sizes, pairs, sums, cell, exposure: bool = False, min_cells: int = 4096, max_step: float = 2.0,
                fixed=None) -> Dict[str, object]:
    """One iteration of refine() on the host, numpy double: refine_solve(sums), then adjust_similarity with the weight n for
    an accepted pair and 0 otherwise, c_f the ground position of frame f's centre pixel under georef and c_p the centre of
    the pair's patch, then the corrected georeference.  With M_f = (1 + sigma_f) * Rot(theta_f), counter-clockwise, the 2 x 2
    part of frame f becomes M_f @ g[:, :2] and its offset M_f @ g[:, 2] + t_f + c_f - M_f @ c_f: the ground moves by u_f about
    the frame's centre.  A frame whose centre is not finite stays as it is.  Returns 'georef' (F,2,3), 'shift' (F,2) metres,
    'yaw' (F,) radians, 'scale' (F,), refine_solve's 'param', 'cells', 'rms', 'accepted', adjust_similarity's 'residual' and
    'component', 'weighted_rms' (the accepted pairs' sqrt(sum of sum r^2 / sum of n), NaN without one) and 'max_corner'
    (metres: the largest displacement this step applies to a corner of a frame)."""
    what = "refine_step"
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    F = g.shape[0]
    sm = _check_sums(sums, what)
    table = _check_pair_table(pairs, F, REGISTER_MAX_SIDE, what)
    sol = refine_solve(sm, table, exposure, min_cells, max_step)
    acc, par = sol["accepted"], sol["param"]
    w = np.where(acc, sol["cells"], 0).astype(np.float64)
    cf = _frame_centres(g, s)
    cp = np.stack([table["x0"] + 0.5 * table["gx"] * cell, table["y0"] + 0.5 * table["gy"] * cell], axis=1).reshape(-1, 2)
    measured = np.where(acc[:, None], np.concatenate([par[:, :2] * cell, par[:, 2:4]], axis=1), 0.0).reshape(-1, 4)
    adj = adjust_similarity(F, table, cp, np.where(np.isfinite(cf), cf, 0.0), measured, w, fixed)
    out_g = g.copy()
    _, X0, Y0 = _footprint_extent(g, s)
    for f in np.nonzero(np.isfinite(cf).all(axis=1))[0]:
        th, k = adj["yaw"][f], 1.0 + adj["scale"][f]
        M = k * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        out_g[f, :, :2] = M @ g[f, :, :2]
        out_g[f, :, 2] = g[f, :, 2] + adj["shift"][f] + (M - np.eye(2)) @ (g[f, :, 2] - cf[f])    # = M g2 + t + c - M c; exact for the identity
    _, X1, Y1 = _footprint_extent(out_g, s)
    with np.errstate(all="ignore"):
        moved = np.hypot(X1 - X0, Y1 - Y0)
        moved = moved[np.isfinite(moved)]
        n_acc = float(sol["cells"][acc].sum())
        wrms = math.sqrt(float(sm[acc, 27].sum()) / n_acc) if n_acc > 0 else float("nan")
    return {"georef": out_g, "shift": adj["shift"], "yaw": adj["yaw"], "scale": adj["scale"], "param": par, "cells": sol["cells"],
            "rms": sol["rms"], "accepted": acc, "residual": adj["residual"], "component": adj["component"], "weighted_rms": wrms,
            "max_corner": float(moved.max()) if moved.size else 0.0}


def _coarse_pairs(table: np.ndarray, level: int):
    """The pair table of refine()'s level `level`: gx >> level, gy >> level, the same frames, x0 and y0.  Returns it twice: as
    wm_register_refine reads it -- a pair whose gx or gy became 0 keeps all-zero sums there -- and as refine_step reads it, with
    1 in the place of such a 0: the pair counts no cell, so it is not accepted and has weight 0 whatever its size.  Level 0
    is the table itself."""
    if not level:
        return table, table
    dev_t = table.copy()
    dev_t["gx"], dev_t["gy"] = table["gx"] >> level, table["gy"] >> level
    gone = (dev_t["gx"] < 1) | (dev_t["gy"] < 1)
    dev_t["gx"][gone], dev_t["gy"][gone] = 0, 0                   # neither axis of such a pair is read
    host_t = dev_t.copy()
    host_t["gx"][gone], host_t["gy"][gone] = 1, 1
    return dev_t, host_t


def refine(frames, georef, cell, sizes=None, pairs=None, side: int = 512, min_cells: int = 4096, iters: int = 3, exposure: bool = False,
           fixed=None, max_step: float = 2.0, pair_chunk: int = 256, levels: int = 0) -> Dict[str, object]:
    """Refine the georeferences of a survey below one cell: the sub-cell shift, the yaw and the scale of every frame, from the
    planes register() searches (wm_register_render_u8 at search 1, wm_register_refine; rule: include/wm_hip.h "Survey
    registration, refinement").  Arguments as for register(); georef is usually register()'s 'georef' -- the step is one
    linearisation and converges from within about max_step cells at the patch corners; farther off in translation, run
    register() first; farther off in yaw or scale, pass levels (below).  pairs: the table to use, None for
    register_pairs(georef, sizes, cell, 1, side, min_cells); it is made once, from the input georef at the fine cell.
    Everything is validated before any device work.  Per iteration, for every chunk of pair_chunk pairs: the planes are rendered at the current georef (frames go up as in register(): a frame is read
    only while a pair of the current chunk needs it), one wm_register_refine call gives the chunk's (n,28) sums, and they
    go to the host; then refine_step() solves every pair (refine_solve), solves one similarity per frame
    (adjust_similarity, fixed=fixed) and corrects the georef.  exposure=True also fits a gain and an offset per pair, for
    frames whose exposure differs.  A survey whose planes coincide cell for cell -- cell = gsd = the scene's pixel and frames
    aligned with the axes, so nearest sampling snaps every plane onto one lattice -- shows the step nothing: the planes are
    identical while the georef is still up to half a cell off.
    levels=L in 1..REGISTER_MAX_LEVEL (side % 2^L == 0, else ValueError) runs `iters` iterations at each level l = L, L - 1,
    ... 0 of a pyramid, (L + 1) * iters in all, which widens the basin to about 2^(L+1) fine cells at the patch corners.  An
    iteration at level l > 0 renders the planes at the fine cell with a ring of 2^l cells (wm_register_render_u8 at search
    2^l), reduces both stacks l times by 2 x 2 rounded means (wm_register_reduce_u8, "Survey registration, pyramid": the
    reduced B is the reduced A's grid grown by one coarse cell), and runs wm_register_refine and refine_step on them with
    search 1, side >> l, every pair's gx >> l and gy >> l (same x0, y0), the cell cell * 2^l and min_cells max(1, min_cells
    >> 2l); a pair whose gx >> l or gy >> l is 0 takes no part at that level (weight 0).  The planes are area means of the
    fine cells, not a point-sampled coarse render, so the ground's fine texture does not alias.  An iteration at level 0 is
    the iteration described above, and levels=0 is exactly that loop.  Runs on the current device's current stream.  No CPU
    fallback.  Returns host values: 'georef' (F,2,3) refined; 'yaw' (F,) radians counter-clockwise, 'scale' (F,) and 'shift'
    (F,2) metres, the whole correction of each frame -- with M = out 2 x 2 @ inverse(in 2 x 2): atan2(M10, M00), sqrt(det M)
    - 1, and the displacement of the frame centre's ground position; 'pairs' the table; the last iteration's 'param',
    'cells', 'rms' and 'accepted' as refine_solve returns them; 'history', per iteration a dict of 'rms' (refine_step's
    'weighted_rms' before the step) and 'max_corner' (metres, the largest corner displacement the step applied), and with
    levels > 0 also 'level'.  'param', 'cells', 'rms' and 'accepted' are then those of the last iteration at level 0."""
    what = "refine"
    side = _check_register_shape(1, side, 1, what)[1]
    levels = _check_levels(levels, side, what)
    min_cells, max_step, exposure = _check_refine_policy(min_cells, max_step, exposure, what)
    if min_cells >= 2 ** 31:
        raise ValueError(f"{what}: min_cells {min_cells} does not fit int32")
    iters = _check_whole(iters, what, "iters")
    pair_chunk = _check_pair_chunk(pair_chunk, what)
    cell, g, s, table = _check_survey(frames, georef, cell, sizes, pairs, 1, side, min_cells, fixed, what)
    F, P = g.shape[0], table.shape[0]
    cur = g.copy()
    step = refine_step(cur, s, table, np.zeros((0, REGISTER_REFINE_SUMS), dtype=np.int64), cell, exposure, min_cells, max_step, fixed) if not P else None
    history = []
    if P:
        dev = _survey_device(what)
        lib = N.lib()
        with torch.cuda.device(dev):
            status = torch.zeros(1, device=dev, dtype=torch.int32)
            for l in [lv for lv in range(levels, -1, -1) for _ in range(iters)]:
                g_d, s_d = _frame_tables(cur, s, dev)
                sums = np.zeros((P, REGISTER_REFINE_SUMS), dtype=np.int64)
                coarse = _coarse_pairs(table, l)                  # (the table the device reads, the one refine_step reads)
                for c0, n, pairs_d, plane_a, plane_b in _rendered_chunks(lib, frames, table, pair_chunk, s, g_d, s_d, cell, 1 << l, side, status, dev, what):
                    if l:
                        plane_a, plane_b = _reduce(lib, plane_a, l, dev), _reduce(lib, plane_b, l, dev)
                        pairs_d = _pinned_upload(coarse[0][c0:c0 + n].view(np.uint8).reshape(n, REGISTER_PAIR.itemsize), dev)
                    sums_d = torch.empty((n, REGISTER_REFINE_SUMS), device=dev, dtype=torch.int64)
                    N.check(lib.wm_register_refine(N.ptr(plane_a), N.ptr(plane_b), N.ptr(pairs_d), n, 1, side >> l, N.ptr(sums_d),
                                                   N.stream_ptr(dev)))
                    sums[c0:c0 + n] = sums_d.cpu().numpy()
                    del plane_a, plane_b, sums_d, pairs_d                 # before the next chunk renders
                step = refine_step(cur, s, coarse[1], sums, cell * (1 << l), exposure, max(1, min_cells >> (2 * l)), max_step, fixed)
                history.append({"rms": step["weighted_rms"], "max_corner": step["max_corner"], **({"level": l} if levels else {})})
                cur = step["georef"]
    with np.errstate(all="ignore"):
        yaw, scale = np.zeros(F), np.zeros(F)
        for f in range(F):
            if (cur[f] == g[f]).all():
                continue                                  # a frame that did not move: exactly 0
            if np.isfinite(g[f]).all() and np.isfinite(cur[f]).all() and abs(np.linalg.det(g[f, :, :2])) > 0:
                M = cur[f, :, :2] @ np.linalg.inv(g[f, :, :2])
                yaw[f], scale[f] = math.atan2(M[1, 0], M[0, 0]), math.sqrt(abs(np.linalg.det(M))) - 1.0
        shift = np.where(np.isfinite(_frame_centres(g, s)), _frame_centres(cur, s) - _frame_centres(g, s), 0.0)
    return {"georef": cur, "yaw": yaw, "scale": scale, "shift": shift, "pairs": table, "param": step["param"], "cells": step["cells"],
            "rms": step["rms"], "accepted": step["accepted"], "history": history}


_refine = refine                                  # register() has a parameter of this name
