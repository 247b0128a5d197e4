"""A survey on the ground: its frames' georeferences, and what is counted, covered and mapped through them.
  * census, nadir_affine: the count a survey is flown for -- the detections of all frames (detect_frames' dicts) go to
    ground coordinates through each frame's georeference and are grouped into individuals, at most one detection of any
    frame per individual (census rule: include/wm_hip.h), by one wm_census launch over the whole survey.
  * coverage, ground_to_pixel, footprint_bounds: the denominator of a density -- a ground grid over the survey, every
    cell with the number of frames that saw its centre (the union of the footprints, its gaps), the census' individuals
    per cell and class, and per individual the number of frames that could have seen it (coverage rule:
    include/wm_hip.h), by wm_coverage_raster and wm_coverage_points.
  * mosaic, mosaic_plan, resampled_georef: the map -- the frames laid onto the coverage's ground grid; every cell takes its
    pixel from the one frame that saw it most vertically (seam rule and sampling: include/wm_hip.h), chosen for all cells
    by one wm_mosaic_plan launch and fetched by wm_mosaic_fill_u8, a chunk of resident frames per launch, so only the
    frames that won a cell are ever loaded; the census' individuals can be outlined on it.  mosaic(blend=band),
    mosaic_blend_plan: instead of one frame per cell, the integer-weighted mean of the exposure-corrected frames that see
    it, every weight falling to zero at the frame's border and away from the seam (include/wm_hip.h "Survey mosaic,
    blended"; wm_mosaic_blend_plan, wm_mosaic_blend_accum_u8 per chunk, wm_mosaic_blend_finish_u8).
The validators of georeferences, sizes, cells and grids, the footprints' extent, the census-dict reader and the resident
chunk of frames are shared with registration.py."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

import torch

from . import _native as N
from ._survey import _as_frame_array, _check_fill, _check_whole, _finite_number, _frame_descs, _frame_index, _pinned_upload
from .review import _check_draw_width, _check_palette, draw_boxes

# ---- census ----------------------------------------------------------------------------------------------------------

CENSUS_MAX_DETS = N.CENSUS_MAX_DETS           # include/wm_hip.h WM_CENSUS_MAX_DETS
CENSUS_CLASSES = 7                            # 'class_counts': the model's labels 0..6 (box_decoder.py:50, 6 + 1 classes)


def _check_radius(radius, what: str) -> float:
    """Validate radius= before any device work: a finite number >= 0 whose square is finite in double."""
    return _finite_number(radius, what, "radius", lambda r: r >= 0.0 and math.isfinite(r * r),
                          "must be finite and >= 0, with a finite square")


def _check_georef(georef, what: str) -> np.ndarray:
    """(F,2,3) float64, C-contiguous: rows (a0, a1, a2) and (a3, a4, a5) of every frame.  Values are not checked: a
    georeference that is not finite makes its frame's detections invalid (the census rule)."""
    if isinstance(georef, torch.Tensor):
        georef = georef.detach().cpu().numpy()
    try:
        g = np.ascontiguousarray(np.asarray(georef, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: georef is not an array of numbers") from None
    if g.size == 0 and g.ndim <= 1:
        g = g.reshape(0, 2, 3)
    if g.ndim != 3 or g.shape[1:] != (2, 3):
        raise ValueError(f"{what}: georef of shape {g.shape}: expected (F, 2, 3)")
    return g


def nadir_affine(height, width, centre, gsd, yaw_deg=0.0) -> np.ndarray:
    """Georeference of a nadir frame, (2,3) float64 for census(): [[a0, a1, a2], [a3, a4, a5]], X = a0*x + a1*y + a2 east
    and Y = a3*x + a4*y + a5 north, in metres, of the pixel position (x, y).  centre = (E, N) is the ground position of pixel
    (width / 2, height / 2), gsd the metres per pixel, yaw_deg the heading of the image's up direction, clockwise from
    north: at 0 right is east and down is south, at 90 up is east.  Host only, in double."""
    H, W, gsd, yaw = float(height), float(width), float(gsd), float(yaw_deg)
    E, Nn = (float(v) for v in centre)
    if not (H > 0 and W > 0 and math.isfinite(H) and math.isfinite(W)):
        raise ValueError(f"nadir_affine: height {height!r}, width {width!r}")
    if not (math.isfinite(gsd) and gsd > 0 and math.isfinite(yaw) and math.isfinite(E) and math.isfinite(Nn)):
        raise ValueError(f"nadir_affine: gsd {gsd!r} must be finite and > 0, centre and yaw_deg finite")
    psi = math.radians(yaw)
    c, sn = math.cos(psi), math.sin(psi)
    a0, a1 = gsd * c, -gsd * sn
    a3, a4 = -gsd * sn, -gsd * c
    return np.array([[a0, a1, E - (a0 * W / 2 + a1 * H / 2)],
                     [a3, a4, Nn - (a3 * W / 2 + a4 * H / 2)]], dtype=np.float64)


def census(results, georef, radius, same_class: bool = False) -> Dict[str, object]:
    """Count each animal once across overlapping frames (wm_census; rule: include/wm_hip.h).  results: an iterable (a
    generator is fine) of the dicts detect_frames yields -- 'boxes' (k,4) fp32, 'scores' (k,), 'labels' (k,) are used as
    they come (union boxes when fusing, source-pixel boxes when resampling); georef (F,2,3) float64, an array or a
    sequence of nadir_affine's results: result i pairs with georef[i].  radius: metres; a detection joins the nearest
    individual within it that has no member of the detection's own frame (same_class: and whose keeper has its label),
    else it founds one.  Everything is concatenated on the device; one wm_census launch on the current stream and one
    small copy of the count (which waits for it).  Returns, with k individuals out of n detections:
      'count' k (int), 'individual' (n,) int64 (-1: invalid detection), 'det_points' (n,2) float64 ground points (NaN:
      invalid), 'det_frame' (n,) int64, 'det_offsets' host list of F + 1 (result i is detections [o[i], o[i+1]));
      per individual, from its keeper (its highest-priority member): 'keeper' (k,) int64 index into the n detections,
      'points' (k,2) float64, 'scores', 'labels', 'frame' (k,); 'members' (k,) int64; 'class_counts' (7,) int64, the
      bincount of the keepers' labels 0..6."""
    what = "census"
    radius = _check_radius(radius, what)
    g = _check_georef(georef, what)
    results = list(results)
    if len(results) != g.shape[0]:
        raise ValueError(f"{what}: {len(results)} results for {g.shape[0]} georeferences")
    dev = None
    for i, res in enumerate(results):
        try:
            b, sc, lb = res["boxes"], res["scores"], res["labels"]
        except (TypeError, KeyError):
            raise ValueError(f"{what}: result {i} has no 'boxes', 'scores' and 'labels'") from None
        if not all(isinstance(t, torch.Tensor) for t in (b, sc, lb)) or b.dim() != 2 or b.shape[1] != 4 or \
                tuple(sc.shape) != (b.shape[0],) or tuple(lb.shape) != (b.shape[0],):
            raise ValueError(f"{what}: result {i}: expected boxes (k,4), scores (k,) and labels (k,) tensors")
        dev = b.device if dev is None else dev
        if b.device != dev or sc.device != dev or lb.device != dev:
            raise ValueError(f"{what}: result {i} is on {b.device}, earlier ones on {dev}")
    ks = [int(res["boxes"].shape[0]) for res in results]
    offs = [0]
    for k in ks:
        offs.append(offs[-1] + k)
    n = offs[-1]
    if n > CENSUS_MAX_DETS:
        raise ValueError(f"{what}: {n} detections exceed {CENSUS_MAX_DETS}")
    dev = torch.device("cpu") if dev is None else dev
    i64 = dict(device=dev, dtype=torch.int64)
    if n == 0:
        return {"count": 0, "individual": torch.empty(0, **i64), "keeper": torch.empty(0, **i64),
                "points": torch.empty((0, 2), device=dev, dtype=torch.float64),
                "det_points": torch.empty((0, 2), device=dev, dtype=torch.float64),
                "scores": torch.empty(0, device=dev, dtype=torch.float32), "labels": torch.empty(0, **i64),
                "frame": torch.empty(0, **i64), "members": torch.empty(0, **i64), "det_frame": torch.empty(0, **i64),
                "det_offsets": offs, "class_counts": torch.zeros(CENSUS_CLASSES, **i64)}
    boxes = torch.cat([res["boxes"] for res in results]).contiguous()
    N.require_cuda(boxes, f"{what}: boxes")
    scores = torch.cat([res["scores"] for res in results]).contiguous()
    N.require_cuda(scores, f"{what}: scores")
    labels_in = torch.cat([res["labels"] for res in results])
    labels = labels_in.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        frame = _frame_index(ks, dev)
        g_d = _pinned_upload(g.reshape(-1, 6), dev)
        nbytes = N.lib().wm_census_scratch_bytes(n)
        if nbytes < 0:
            N.check(-1)
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        points = torch.empty((n, 2), device=dev, dtype=torch.float64)
        individual = torch.empty(n, device=dev, dtype=torch.int32)
        keeper = torch.empty(n, device=dev, dtype=torch.int32)
        members = torch.empty(n, device=dev, dtype=torch.int32)
        count = torch.empty(2, device=dev, dtype=torch.int32)
        N.check(N.lib().wm_census(N.ptr(boxes), N.ptr(scores), N.ptr(labels), N.ptr(frame), n, N.ptr(g_d), g.shape[0], radius,
                                  N.CENSUS_SAME_CLASS if same_class else 0, N.ptr(scratch), nbytes, N.ptr(points),
                                  N.ptr(individual), N.ptr(keeper), N.ptr(members), N.ptr(count), N.stream_ptr(dev)))
        k, status = count.cpu().tolist()
    if status & N.CENSUS_UNSOLVED:
        raise RuntimeError(f"{what}: wm_census left detections undecided (status {status})")
    keeper = keeper[:k].to(torch.int64)
    klab = labels_in[keeper]
    ok = (klab >= 0) & (klab < CENSUS_CLASSES)
    det_frame = frame.to(torch.int64)
    return {"count": k, "individual": individual.to(torch.int64), "keeper": keeper, "points": points[keeper],
            "det_points": points, "scores": scores[keeper], "labels": klab, "frame": det_frame[keeper],
            "members": members[:k].to(torch.int64), "det_frame": det_frame, "det_offsets": offs,
            "class_counts": torch.bincount(klab[ok].to(torch.int64), minlength=CENSUS_CLASSES)}


# ---- coverage --------------------------------------------------------------------------------------------------------

COVERAGE_MAX_SIDE = N.COVERAGE_MAX_SIDE       # include/wm_hip.h WM_COVERAGE_MAX_SIDE
COVERAGE_MAX_CELLS = N.COVERAGE_MAX_CELLS     # WM_COVERAGE_MAX_CELLS
COVERAGE_MAX_FRAMES = N.COVERAGE_MAX_FRAMES   # WM_COVERAGE_MAX_FRAMES


def _check_cell(cell, what: str) -> float:
    """Validate cell= before any device work: a finite number > 0."""
    return _finite_number(cell, what, "cell", lambda c: c > 0.0, "must be finite and > 0", refuse=(str, bytes))


def _check_sizes(sizes, n_frames: int, what: str) -> np.ndarray:
    """(F,2) int32, C-contiguous: (height, width) of every frame, one per georeference."""
    if isinstance(sizes, torch.Tensor):
        sizes = sizes.detach().cpu().numpy()
    try:
        a = np.asarray(sizes)
        if a.size == 0 and a.ndim <= 1:
            a = a.reshape(0, 2)
        if a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and np.all(a == np.floor(a))):
            raise TypeError
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise TypeError
        s = np.ascontiguousarray(a.astype(np.int32))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: sizes is not an array of whole numbers that fit int32") from None
    if s.ndim != 2 or s.shape[1] != 2:
        raise ValueError(f"{what}: sizes of shape {s.shape}: expected (F, 2), (height, width) per frame")
    if s.shape[0] != n_frames:
        raise ValueError(f"{what}: {s.shape[0]} sizes for {n_frames} georeferences")
    return s


def _check_grid(x0, y0, gx, gy, cell: float, what: str, name: str = "bounds"):
    """Validate a grid against the limits of include/wm_hip.h; the message says what to do about a grid that is too large."""
    try:
        fx, fy = float(x0), float(y0)
        ix, iy = int(gx), int(gy)
        if ix != gx or iy != gy:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} {(x0, y0, gx, gy)!r}: expected (x0, y0, gx, gy), two numbers and two whole numbers") from None
    if not (math.isfinite(fx) and math.isfinite(fy)):
        raise ValueError(f"{what}: {name}: origin ({x0!r}, {y0!r}) is not finite")
    if ix < 1 or iy < 1:
        raise ValueError(f"{what}: {name}: a grid of {ix} x {iy} cells; gx and gy must be at least 1")
    if ix > COVERAGE_MAX_SIDE or iy > COVERAGE_MAX_SIDE or ix * iy > COVERAGE_MAX_CELLS:
        raise ValueError(f"{what}: {name}: a grid of {ix} x {iy} cells at cell {cell!r} exceeds {COVERAGE_MAX_SIDE} cells a side "
                         f"or {COVERAGE_MAX_CELLS} cells in all: choose a larger cell")
    return fx, fy, ix, iy


def ground_to_pixel(georef) -> np.ndarray:
    """The inverse of census()'s georeferences: (F,2,3) float64 [[a0, a1, a2], [a3, a4, a5]] (pixel -> ground) gives (F,2,3)
    float64 [[b0, b1, b2], [b3, b4, b5]] (ground -> pixel), x = b0*X + b1*Y + b2, y = b3*X + b4*Y + b5; a single (2,3)
    gives a (2,3).  Host only, in double, in this order: det = a0*a4 - a1*a3; b0 = a4/det, b1 = -a1/det, b3 = -a3/det,
    b4 = a0/det; b2 = -(b0*a2 + b1*a5), b5 = -(b3*a2 + b4*a5).  A frame that is singular (det == 0) or not finite, in
    its input or its inverse, gives a row of NaN: such a frame sees nothing (coverage rule: include/wm_hip.h)."""
    g = np.asarray(georef, dtype=np.float64) if not isinstance(georef, torch.Tensor) else georef.detach().cpu().numpy().astype(np.float64)
    single = g.ndim == 2
    g = _check_georef(g[None] if single else g, "ground_to_pixel")
    a0, a1, a2, a3, a4, a5 = (g[:, r, c] for r in range(2) for c in range(3))
    out = np.empty_like(g)
    with np.errstate(all="ignore"):
        det = a0 * a4 - a1 * a3
        b0, b1, b3, b4 = a4 / det, -a1 / det, -a3 / det, a0 / det
        b2 = -(b0 * a2 + b1 * a5)
        b5 = -(b3 * a2 + b4 * a5)
        out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = b0, b1, b2
        out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = b3, b4, b5
        bad = ~(np.isfinite(g).all(axis=(1, 2)) & np.isfinite(out).all(axis=(1, 2)) & (det != 0.0))
    out[bad] = np.nan
    return out[0] if single else out


def _footprint_extent(g: np.ndarray, s: np.ndarray):
    """The ground positions of every frame's corners (0, 0), (W, 0), (0, H), (W, H), in double: (ok (F,) bool -- the
    georeference is finite and the size at least 1 x 1 -- then X (F,4) east and Y (F,4) north, meaningless where not ok)."""
    ok = np.isfinite(g).all(axis=(1, 2)) & (s >= 1).all(axis=1)
    w, h = s[:, 1].astype(np.float64), s[:, 0].astype(np.float64)
    zero = np.zeros(g.shape[0])
    cx, cy = np.stack([zero, w, zero, w], axis=1), np.stack([zero, zero, h, h], axis=1)
    with np.errstate(all="ignore"):
        X = g[:, 0, 0:1] * cx + g[:, 0, 1:2] * cy + g[:, 0, 2:3]
        Y = g[:, 1, 0:1] * cx + g[:, 1, 1:2] * cy + g[:, 1, 2:3]
    return ok, X, Y


def footprint_bounds(georef, sizes, cell):
    """A grid that holds every frame's footprint: (x0, y0, gx, gy) for coverage(bounds=).  georef (F,2,3) float64 as for
    census(), sizes (F,2) (height, width), cell metres.  The extent of the corners (0, 0), (W, 0), (0, H), (W, H) of every
    frame whose georeference is finite and whose size is at least 1 x 1; x0 and y0 are snapped down to multiples of cell,
    so the grids of two flights of one area line up; gx and gy are at least 1 (no usable frame: (0.0, 0.0, 1, 1)).  Host
    only.  Raises ValueError when the grid would exceed the limits of include/wm_hip.h: choose a larger cell."""
    what = "footprint_bounds"
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    ok, X, Y = _footprint_extent(g, s)
    if not ok.any():
        return 0.0, 0.0, 1, 1
    X, Y = X[ok], Y[ok]
    with np.errstate(all="ignore"):
        x0, y0 = math.floor(X.min() / cell) * cell, math.floor(Y.min() / cell) * cell
        nx, ny = math.ceil((X.max() - x0) / cell), math.ceil((Y.max() - y0) / cell)
    if not all(math.isfinite(v) for v in (x0, y0, nx, ny)):
        raise ValueError(f"{what}: the footprints' extent is not finite at cell {cell!r}")
    _, _, gx, gy = _check_grid(x0, y0, max(int(nx), 1), max(int(ny), 1), cell, what, "the footprints' grid")
    return float(x0), float(y0), gx, gy


def _survey_grid(georef, sizes, cell, bounds, what: str):
    """The frames and the grid of coverage() and mosaic(), validated before any device work: (g (F,2,3) float64, s (F,2) int32,
    cell, x0, y0, gx, gy); bounds None means footprint_bounds(georef, sizes, cell)."""
    cell = _check_cell(cell, what)
    g = _check_georef(georef, what)
    s = _check_sizes(sizes, g.shape[0], what)
    if g.shape[0] > COVERAGE_MAX_FRAMES:
        raise ValueError(f"{what}: {g.shape[0]} frames exceed {COVERAGE_MAX_FRAMES}")
    if bounds is None:
        x0, y0, gx, gy = footprint_bounds(g, s, cell)
    else:
        try:
            bx0, by0, bgx, bgy = bounds
        except (TypeError, ValueError):
            raise ValueError(f"{what}: bounds {bounds!r}: expected (x0, y0, gx, gy)") from None
        x0, y0, gx, gy = _check_grid(bx0, by0, bgx, bgy, cell, what)
    return g, s, cell, x0, y0, gx, gy


def _survey_device(what: str, pts=None) -> torch.device:
    """The device of coverage(), mosaic() and register(): that of the census' points when they are given, else the current one."""
    if pts is not None:
        if not pts.is_cuda:
            raise RuntimeError(f"{what}: census['points'] is on {pts.device}; the HIP path needs a ROCm device tensor "
                               "(there is no CPU fallback in wildlifemapper_amd)")
        return pts.device
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what}: no GPU is present; the HIP path needs a ROCm device tensor "
                           "(there is no CPU fallback in wildlifemapper_amd)")
    return torch.device("cuda", torch.cuda.current_device())


def _frame_tables(g: np.ndarray, s: np.ndarray, dev: torch.device):
    """The kernels' g2p (F,6) float64 and sizes (F,2) int32 on dev, through pinned memory; (None, None) when there is no frame."""
    if not g.shape[0]:
        return None, None
    return _pinned_upload(ground_to_pixel(g).reshape(-1, 6), dev), _pinned_upload(s, dev)


def _frame_sequence(frames, sizes, what: str, indexed_for: str):
    """The frames of mosaic() and register(): a sequence that is only indexed.  Returns (len(frames), sizes); sizes None is
    inferred only from a list or tuple of tensors or arrays, whose shapes cost nothing."""
    if not (hasattr(frames, "__getitem__") and hasattr(frames, "__len__")):
        raise ValueError(f"{what}: frames must be a sequence that can be indexed (frames[i], len), got {type(frames).__name__}")
    if sizes is None:
        if not isinstance(frames, (list, tuple)) or not all(isinstance(fr, (torch.Tensor, np.ndarray)) for fr in frames):
            raise ValueError(f"{what}: sizes is required when frames is not a list of tensors or arrays (a lazy sequence is only "
                             f"indexed for {indexed_for})")
        if any(fr.ndim != 3 for fr in frames):
            raise ValueError(f"{what}: frames: expected (H,W,3) uint8 tensors or arrays")
        sizes = np.array([tuple(fr.shape[:2]) for fr in frames], dtype=np.int64).reshape(-1, 2)
    return len(frames), sizes


def _resident_chunk(frames, ids, s: np.ndarray, dev: torch.device, what: str):
    """Makes the frames `ids` (ascending) resident for one fill or render launch: frames[i] is indexed once each, in that
    order, host frames go up through pinned memory, and a shape that disagrees with s raises ValueError naming the frame.
    Returns (descriptors, the (F,) slot table, the frames), all on dev; the caller drops them after its launch."""
    resident = []
    for i in ids:
        on_dev, on_host = _as_frame_array(frames[i], i, dev, what)
        fr = on_dev if on_dev is not None else _pinned_upload(on_host, dev)
        if tuple(fr.shape[:2]) != tuple(int(v) for v in s[i]):
            raise ValueError(f"{what}: frame {i} is {tuple(fr.shape[:2])}, sizes says {tuple(int(v) for v in s[i])}")
        resident.append(fr)
    slot = np.full(s.shape[0], -1, dtype=np.int32)
    slot[ids] = np.arange(len(ids), dtype=np.int32)
    return _frame_descs(resident, dev), _pinned_upload(slot, dev), resident


def _census_fields(census, keys, what: str, most=None):
    """census[k] for k in keys ('points' first), as coverage() and mosaic() read the dict census() returned: 'points' (k,2)
    float64 and every other field a (k,) tensor on its device.  most: the number of individuals the caller's launch takes;
    with it the count is checked between the shapes and the devices, which then have a message of their own."""
    listed = lambda items: ", ".join(items[:-1]) + " and " + items[-1]
    try:
        fields = [census[k] for k in keys]
    except (TypeError, KeyError):
        raise ValueError(f"{what}: census has no {listed([repr(k) for k in keys])}: pass the dict census() returned") from None
    pts, rest = fields[0], fields[1:]
    shaped = all(isinstance(t, torch.Tensor) for t in fields) and pts.dim() == 2 and pts.shape[1] == 2 and \
        pts.dtype == torch.float64 and all(tuple(t.shape) == (pts.shape[0],) for t in rest)
    together = shaped and all(t.device == pts.device for t in rest)
    expected = listed(["'points' (k,2) float64"] + [f"{k!r} (k,)" for k in keys[1:]])
    if most is None and not together:
        raise ValueError(f"{what}: census: expected {expected} tensors on one device")
    if not shaped:
        raise ValueError(f"{what}: census: expected {expected} tensors")
    if most is not None and pts.shape[0] > most:
        raise ValueError(f"{what}: {pts.shape[0]} individuals exceed {most}")
    if not together:
        raise ValueError(f"{what}: census tensors are on different devices")
    return fields


def coverage(georef, sizes, cell, census=None, bounds=None) -> Dict[str, object]:
    """The ground a survey saw (wm_coverage_raster, wm_coverage_points; rule: include/wm_hip.h).  georef (F,2,3) float64 as
    for census() (pixel -> ground; inverted on the host by ground_to_pixel), sizes (F,2) (height, width) of the frames in
    the pixels the georeferences speak of, cell the side of a ground cell in metres, bounds (x0, y0, gx, gy) or None for
    footprint_bounds(georef, sizes, cell), census the dict census() returned, or None.  Everything is validated before
    any device work; the frames go up through pinned memory to the current device -- torch.cuda.current_device(), or with
    census= the device of its tensors -- and the launches run on its current stream; one small copy of the statistics
    waits for them.  No CPU fallback.  Returns
      'coverage' (gy,gx) int32 on the device: frames that saw each cell's centre.  Row 0 is the SOUTHERNMOST row: a
          north-up picture is coverage.flip(0).  The kernel writes uint16 (F <= 65535); it is widened once to int32
          (a copy of twice the raster's bytes), the narrowest dtype torch indexes, compares and sums on the device;
      'origin' (x0, y0), 'cell', 'shape' (gy, gx); 'multiplicity' (16,) int64 on the device: cells seen by 0, 1, ...,
          14 and by 15 or more frames; 'gap_cells' int = multiplicity[0], the cells no frame saw;
      'area_m2' float = (gx * gy - gap_cells) * cell * cell, the observed ground;
    and with census=, from the individuals' keeper 'points' (k,2) and 'labels' (k,):
      'seen_by' (k,) int64: frames whose footprint holds the individual's point (0: not finite, or seen by none);
      'cell_index' (k,2) int64: its cell (j, i), (-1, -1) when it is not binned (outside the grid, not finite, or a
          label outside 0..6);
      'counts' (7,gy,gx) int32: binned individuals per class and cell; 'class_counts' (7,) int64: their sums;
      'density_per_km2' (7,) float64 = class_counts / (area_m2 / 1e6), divided on the host in double; NaN when the area is 0;
      'detection_rate' float = sum of 'members' / sum of 'seen_by' over the individuals with seen_by >= 1, NaN when
          there is none: of the chances the frames had to detect an individual, the share they took.  A member's own
          ground point differs slightly from its keeper's (the georeferencing error the census radius absorbs), so at a
          frame's edge a member can lie in a frame whose footprint misses the keeper's point: a ratio slightly above 1
          is possible and is not clamped."""
    what = "coverage"
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    F = g.shape[0]
    pts = labels = members = None
    if census is not None:
        pts, labels, members = _census_fields(census, ("points", "labels", "members"), what, CENSUS_MAX_DETS)
    dev = _survey_device(what, pts)
    lib = N.lib()
    with torch.cuda.device(dev):
        g_d, s_d = _frame_tables(g, s, dev)                   # no frames: nothing to upload, an all-zero raster
        cov16 = torch.empty((gy, gx), device=dev, dtype=torch.int16)
        stats = torch.empty(N.COVERAGE_STATS, device=dev, dtype=torch.int64)
        N.check(lib.wm_coverage_raster(N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy, N.ptr(cov16), N.ptr(stats), N.stream_ptr(dev)))
        out = {"coverage": cov16.to(torch.int32) & 0xFFFF, "origin": (x0, y0), "cell": cell, "shape": (gy, gx), "multiplicity": stats}
        gap = int(stats[0].item())
        area = float((gx * gy - gap) * cell * cell)
        out["gap_cells"], out["area_m2"] = gap, area
        if census is None:
            return out
        k = int(pts.shape[0])
        pts = pts.contiguous()
        lab32 = labels.to(torch.int32).contiguous()
        alloc = torch.empty if k else torch.zeros             # k == 0: the entry returns before writing anything
        seen = alloc(k, device=dev, dtype=torch.int32)
        cidx = alloc((k, 2), device=dev, dtype=torch.int32)
        counts = alloc((N.COVERAGE_CLASSES, gy, gx), device=dev, dtype=torch.int32)
        pstats = alloc(2, device=dev, dtype=torch.int64)
        N.check(lib.wm_coverage_points(N.ptr(g_d), N.ptr(s_d), F, N.ptr(pts), N.ptr(lab32), k, x0, y0, cell, gx, gy, N.ptr(seen),
                                       N.ptr(cidx), N.ptr(counts), N.ptr(pstats), N.stream_ptr(dev)))
        seen = seen.to(torch.int64)
        class_counts = counts.sum(dim=(1, 2), dtype=torch.int64)
        could = seen >= 1
        n_seen, n_members = int(seen[could].sum().item()), int(members[could].sum().item())
        # seven divisions, on the host: IEEE double there, where a device division by a scalar may be a multiplication
        density = class_counts.cpu().numpy().astype(np.float64) / (area / 1e6) if area > 0 else np.full(N.COVERAGE_CLASSES, np.nan)
    out.update({"seen_by": seen, "cell_index": cidx.to(torch.int64), "counts": counts, "class_counts": class_counts,
                "density_per_km2": torch.from_numpy(density).to(dev),
                "detection_rate": n_members / n_seen if n_seen > 0 else float("nan")})
    return out


# ---- mosaic ----------------------------------------------------------------------------------------------------------

MOSAIC_SAMPLES = {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}

def _mosaic_plan(g, s, cell, x0, y0, gx, gy, dev):
    """wm_mosaic_plan on validated arguments.  Returns the plan's dict and the device copies of g2p and sizes."""
    F = g.shape[0]
    with torch.cuda.device(dev):
        g_d, s_d = _frame_tables(g, s, dev)                   # no frames: nothing to upload, an all -1 raster
        won = torch.empty(F, device=dev, dtype=torch.int32) if F else None
        source = torch.empty((gy, gx), device=dev, dtype=torch.int32)
        stats = torch.empty(2, device=dev, dtype=torch.int64)
        N.check(N.lib().wm_mosaic_plan(N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy, N.ptr(source), N.ptr(won), N.ptr(stats),
                                       N.stream_ptr(dev)))
        gap = int(stats[1].item())
    won = won.to(torch.int64) if F else torch.zeros(0, device=dev, dtype=torch.int64)
    return {"source": source, "won": won, "origin": (x0, y0), "cell": cell, "shape": (gy, gx), "gap_cells": gap}, g_d, s_d


def mosaic_plan(georef, sizes, cell, bounds=None) -> Dict[str, object]:
    """Which frame shows each ground cell (wm_mosaic_plan; rule: include/wm_hip.h "Survey mosaic").  Geometry only, no
    pixels: georef (F,2,3) float64 as for census() (pixel -> ground), sizes (F,2) (height, width), cell metres, bounds
    (x0, y0, gx, gy) or None for footprint_bounds(georef, sizes, cell) -- the arguments and the validation of coverage(),
    run before any device work.  Among the frames that see a cell's centre the source is the one whose centre pixel is
    nearest to it (the most vertical view), ties to the lowest index.  One launch on the current device's current stream
    and one small copy of the statistics, which waits for it.  No CPU fallback.  Returns
      'source' (gy,gx) int32 on the device: the frame of each cell, -1 where no frame saw it; row 0 is the SOUTHERNMOST;
      'won' (F,) int64 on the device: the cells each frame is the source of;
      'origin' (x0, y0), 'cell', 'shape' (gy, gx); 'gap_cells' int, the cells without a source."""
    what = "mosaic_plan"
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    return _mosaic_plan(g, s, cell, x0, y0, gx, gy, _survey_device(what))[0]


def _check_band(band, what: str, name: str = "band") -> float:
    """Validate band= (mosaic's blend=) before any device work: a finite number > 0 (no bool) whose 256 / band is finite too."""
    must = "must be a finite number > 0"
    return _finite_number(band, what, name, lambda b: b > 0.0 and math.isfinite(256.0 / b), must, must, refuse=(bool, np.bool_, str, bytes))


def _check_exposure(exposure, n_frames: int, what: str) -> np.ndarray:
    """exposure= of mosaic(): the (F,2) int32 table exposure_table() returns, as an array or a tensor."""
    a = exposure.detach().cpu().numpy() if isinstance(exposure, torch.Tensor) else exposure
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != (n_frames, 2):
        raise ValueError(f"{what}: exposure must be the ({n_frames}, 2) int32 table tiling.exposure_table() returns")
    return np.ascontiguousarray(a)


def _mosaic_blend_plan(g_d, s_d, F, cell, x0, y0, gx, gy, band, dev):
    """wm_mosaic_blend_plan on validated arguments and the device copies of g2p and sizes.  Returns the plan's dict."""
    with torch.cuda.device(dev):
        cells = torch.empty(F, device=dev, dtype=torch.int32) if F else None
        best = torch.empty((gy, gx), device=dev, dtype=torch.float64)
        stats = torch.empty(3, device=dev, dtype=torch.int64)
        N.check(N.lib().wm_mosaic_blend_plan(N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy, band, N.ptr(best), N.ptr(cells), N.ptr(stats),
                                             N.stream_ptr(dev)))
        seen, gap, blended = (int(v) for v in stats.cpu().tolist())
    cells = cells.to(torch.int64) if F else torch.zeros(0, device=dev, dtype=torch.int64)
    return {"best": best, "cells": cells, "origin": (x0, y0), "cell": cell, "shape": (gy, gx), "band": band, "seen_cells": seen,
            "gap_cells": gap, "blended_cells": blended}


def mosaic_blend_plan(georef, sizes, cell, band, bounds=None) -> Dict[str, object]:
    """Which frames blend into each ground cell (wm_mosaic_blend_plan; rule: include/wm_hip.h "Survey mosaic, blended").
    Geometry only, no pixels; the arguments and the validation of mosaic_plan(), plus band: the width in SOURCE PIXELS, a
    finite number > 0, over which a frame's weight falls to zero at its own border and away from the seam.  One launch on
    the current device's current stream and one small copy of the statistics, which waits for it.  No CPU fallback.  Returns
      'best' (gy,gx) float64 on the device: the largest distance, in its own pixels, of a frame that sees the cell to that
          frame's nearest border, -1.0 where no frame sees it; row 0 is the SOUTHERNMOST;
      'cells' (F,) int64 on the device: the cells into which each frame blends with a positive weight -- the frames
          mosaic(blend=band) loads are exactly those with cells > 0;
      'origin' (x0, y0), 'cell', 'shape' (gy, gx), 'band'; 'seen_cells', 'gap_cells' and 'blended_cells' int: the cells a
          frame sees, those none sees, and those that mix two or more frames."""
    what = "mosaic_blend_plan"
    band = _check_band(band, what)
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    dev = _survey_device(what)
    with torch.cuda.device(dev):
        g_d, s_d = _frame_tables(g, s, dev)
    return _mosaic_blend_plan(g_d, s_d, g.shape[0], cell, x0, y0, gx, gy, band, dev)


def resampled_georef(georef, size, new_size) -> np.ndarray:
    """The georeference of a frame after resampling: georef (2,3) or (F,2,3) float64 (pixel -> ground) of frames of `size`
    (height, width) gives that of the same frames resampled to `new_size` (H', W') -- a pixel of the new frame spans W / W'
    old pixels across and H / H' down, and pixel (0, 0)'s corner stays where it was: a0' = a0 * (W / W'), a3' = a3 *
    (W / W'), a1' = a1 * (H / H'), a4' = a4 * (H / H'), a2 and a5 unchanged.  size and new_size are one (height, width)
    pair for all frames or (F,2), one pair per frame.  Host only, in double.  With preprocess.resample_u8 this is the
    route to a map coarser than the frames: mosaic() point-samples, so shrink the frames to about the cell size first."""
    what = "resampled_georef"
    g = georef.detach().cpu().numpy() if isinstance(georef, torch.Tensor) else georef
    try:
        g = np.asarray(g, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: georef is not an array of numbers") from None
    single = g.ndim == 2
    g = _check_georef(g[None] if single else g, what)
    F = g.shape[0]

    def pairs(v, name):
        try:
            a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v)
            if a.dtype.kind not in "iuf" or a.shape not in ((2,), (F, 2)) or not np.all(np.isfinite(a)) or not np.all(a == np.floor(a)) \
                    or not np.all(a >= 1):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} {v!r}: expected (height, width) or ({F}, 2), whole numbers >= 1") from None
        return np.broadcast_to(a.astype(np.float64), (F, 2))

    old, new = pairs(size, "size"), pairs(new_size, "new_size")
    sy, sx = old[:, 0] / new[:, 0], old[:, 1] / new[:, 1]
    out = g.copy()
    out[:, 0, 0], out[:, 1, 0] = g[:, 0, 0] * sx, g[:, 1, 0] * sx
    out[:, 0, 1], out[:, 1, 1] = g[:, 0, 1] * sy, g[:, 1, 1] * sy
    return out[0] if single else out


def mosaic(frames, georef, cell, sizes=None, bounds=None, sample: str = "bilinear", fill=(0, 0, 0), north_up: bool = True,
           chunk: int = 8, census=None, marker=None, width: int = 2, palette=None, blend=None, exposure=None) -> Dict[str, object]:
    """The map of a survey: its frames laid onto the ground grid (wm_mosaic_plan, wm_mosaic_fill_u8; rule: include/wm_hip.h
    "Survey mosaic").  frames: a sequence that is only indexed (frames[i], len) -- a list of (H,W,3) uint8 ROCm tensors,
    CPU tensors or numpy arrays as detect_frames accepts them, or a lazy sequence that loads frame i from disk when it is
    asked for; georef (F,2,3) float64 as for census(), cell metres, bounds as for coverage().  sizes (F,2) (height, width)
    may be None only when every item of `frames` is already a tensor or an array (a list or tuple, whose shapes cost
    nothing); a lazy sequence needs it.  Everything is validated before any device work.
    The plan runs first (mosaic_plan).  Only frames that are the source of at least one cell are ever indexed, each
    exactly once, in ascending order, `chunk` at a time: host frames go up through pinned memory, one fill launch per
    chunk, and the chunk's frames are released after it -- a lazy sequence pays for the winners only, and bounds= over a
    corner of a survey touches a handful of frames.  A frame whose shape disagrees with sizes raises ValueError naming
    it, before its chunk is launched.
    sample: 'bilinear' (pixel centres at integer + 0.5, edge replicate) or 'nearest'.  A cell finer than the ground
    sampling distance magnifies; a coarser one point-samples and aliases: for a coarse map shrink the frames first
    (preprocess.resample_u8, PIL-exact) and rescale their georeferences (resampled_georef).  fill: the (r, g, b) of the
    cells no frame saw.  north_up: the picture's row 0 is the NORTHERNMOST (what a viewer expects); False keeps row 0
    south, as 'source' and coverage() always have it.
    census= (the dict census() returned) with marker= (the side of a square in cells, a whole number >= 1): every
    individual whose keeper point is finite and inside the grid is outlined in its class colour by one draw_boxes launch
    on the finished mosaic (width, palette as for draw_boxes); the square is centred on ((X - x0) / cell, (Y - y0) / cell),
    the y mirrored (gy - y) when north_up.
    blend= (None: the hard seams above, untouched) a band in SOURCE PIXELS, a finite number > 0: every cell becomes the
    integer-weighted mean of all the frames that see it, each frame's weight falling to zero at its own border and, over
    the band, away from the seam (wm_mosaic_blend_plan, wm_mosaic_blend_accum_u8, wm_mosaic_blend_finish_u8; rule:
    include/wm_hip.h "Survey mosaic, blended").  The hard plan still runs, so 'source', 'won' and 'gap_cells' keep their
    meaning; then the blend plan; exactly the frames that blend into a cell (mosaic_blend_plan's cells > 0) are indexed,
    each once, ascending, `chunk` at a time; one accumulate launch per chunk and one finish into the fill-coloured
    picture.  The result does not depend on chunk.  Memory: 16 bytes per cell of accumulators plus 8 of 'best' while it
    runs, 1.5 GiB at 8192 x 8192 cells.  Within band pixels of the OUTER rim of the covered ground a step can remain, where
    two frames reach their borders at one point and neither has weight left to fade with.
    exposure= (needs blend=) the (F,2) int32 table exposure_table() makes of adjust_exposure()'s gains and offsets: every
    frame's pixels pass through its gain and offset before they are summed.
    Runs on the current device's current stream (with census=, on its tensors' device).  No CPU fallback.  Returns the
    plan's dict ('source', 'won', 'origin', 'cell', 'shape', 'gap_cells') plus 'mosaic' (gy,gx,3) uint8 on the device and
    'north_up'; with blend= also 'blend_cells' (F,) int64 on the device (the cells each frame blends into) and
    'blended_cells' int (the cells that mix two or more frames); with markers also 'marker_boxes' (k',4) fp32 xyxy in
    picture pixels and 'marker_index' (k',) int64, the individuals they belong to."""
    what = "mosaic"
    if blend is not None:
        blend = _check_band(blend, what, "blend")
    elif exposure is not None:
        raise ValueError(f"{what}: exposure needs blend=: the hard-seam mosaic copies pixels as they are")
    if not isinstance(sample, str) or sample not in MOSAIC_SAMPLES:
        raise ValueError(f"{what}: sample {sample!r} must be 'bilinear' or 'nearest'")
    fill_a = _check_fill(fill, what)
    chunk = _check_whole(chunk, what, "chunk")
    if (census is None) != (marker is None):
        raise ValueError(f"{what}: marker {marker!r} and census go together: pass both (census= the dict census() returned) or neither")
    pts = labels = None
    if census is not None:
        marker = _check_whole(marker, what, "marker")
        width = _check_draw_width(width, what)
        palette = _check_palette(palette, what)
        pts, labels = _census_fields(census, ("points", "labels"), what)
    n_given, sizes = _frame_sequence(frames, sizes, what, "the frames that won a cell")
    g, s, cell, x0, y0, gx, gy = _survey_grid(georef, sizes, cell, bounds, what)
    F = g.shape[0]
    if n_given != F:
        raise ValueError(f"{what}: {n_given} frames for {F} georeferences")
    if exposure is not None:
        exposure = _check_exposure(exposure, F, what)
    dev = _survey_device(what, pts)
    out, g_d, s_d = _mosaic_plan(g, s, cell, x0, y0, gx, gy, dev)
    lib = N.lib()
    mode, flags = MOSAIC_SAMPLES[sample], N.MOSAIC_NORTH_UP if north_up else 0
    with torch.cuda.device(dev):
        picture = torch.from_numpy(fill_a).to(dev).expand(gy, gx, 3).contiguous()
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        if blend is None:
            winners = torch.nonzero(out["won"] > 0).flatten().cpu().tolist()
            for c0 in range(0, len(winners), chunk):
                ids = winners[c0:c0 + chunk]
                desc, slot_d, resident = _resident_chunk(frames, ids, s, dev, what)
                N.check(lib.wm_mosaic_fill_u8(N.ptr(desc), len(ids), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, x0, y0, cell, gx, gy,
                                              N.ptr(out["source"]), mode, flags, N.ptr(picture), N.ptr(status), N.stream_ptr(dev)))
                del resident, desc, slot_d                    # the stream orders their reuse after the launch
            bad = int(status.item()) if winners else 0
            if bad:
                raise RuntimeError(f"{what}: wm_mosaic_fill_u8 skipped cells (status {bad}): a resident frame did not match its slot or size")
        else:
            plan = _mosaic_blend_plan(g_d, s_d, F, cell, x0, y0, gx, gy, blend, dev)
            acc = torch.zeros((gy, gx, 4), device=dev, dtype=torch.int32)       # the entry's uint32, as torch can hold them
            e_d = _pinned_upload(exposure, dev) if exposure is not None and F else None
            users = torch.nonzero(plan["cells"] > 0).flatten().cpu().tolist()
            for c0 in range(0, len(users), chunk):
                ids = users[c0:c0 + chunk]
                desc, _, resident = _resident_chunk(frames, ids, s, dev, what)
                index_d = _pinned_upload(np.asarray(ids, dtype=np.int32), dev)
                N.check(lib.wm_mosaic_blend_accum_u8(N.ptr(desc), N.ptr(index_d), len(ids), N.ptr(g_d), N.ptr(s_d), F, N.ptr(e_d), x0, y0,
                                                     cell, gx, gy, blend, N.ptr(plan["best"]), mode, N.ptr(acc), N.ptr(status),
                                                     N.stream_ptr(dev)))
                del resident, desc, index_d                   # the stream orders their reuse after the launch
            bad = int(status.item()) if users else 0
            if bad:
                raise RuntimeError(f"{what}: wm_mosaic_blend_accum_u8 skipped frames (status {bad}): a resident frame did not match its index or size")
            N.check(lib.wm_mosaic_blend_finish_u8(N.ptr(acc), gx, gy, flags, N.ptr(picture), N.stream_ptr(dev)))
            del acc
            out.update({"blend_cells": plan["cells"], "blended_cells": plan["blended_cells"]})
        out.update({"mosaic": picture, "north_up": bool(north_up)})
        if pts is not None:
            p = pts.detach().cpu().numpy()
            with np.errstate(all="ignore"):
                cx, cy = (p[:, 0] - x0) / cell, (p[:, 1] - y0) / cell
                inside = np.isfinite(p).all(axis=1) & (np.floor(cx) >= 0) & (np.floor(cx) < gx) & (np.floor(cy) >= 0) & (np.floor(cy) < gy)
            idx = np.nonzero(inside)[0]
            cx, cy = cx[idx], cy[idx]
            if north_up:
                cy = gy - cy
            half = marker / 2.0
            boxes = np.stack([cx - half, cy - half, cx + half, cy + half], axis=1).astype(np.float32).reshape(-1, 4)
            boxes_d = torch.from_numpy(boxes).to(dev)
            idx_d = torch.from_numpy(idx.astype(np.int64)).to(dev)
            draw_boxes(picture, boxes_d, labels[idx_d], width=width, palette=palette)
            out.update({"marker_boxes": boxes_d, "marker_index": idx_d})
    return out
