"""Survey lens model: the frames of a survey undistorted by their camera calibration, so that the one affine per frame of
census(), coverage(), mosaic(), register() and refine() is true of them (rule: include/wm_hip.h "Survey lens").

A camera is nine numbers, fx, fy, cx, cy, k1, k2, p1, p2, k3: the Brown-Conrady model in OpenCV's order, as photogrammetry
packages export it.  cx, cy follow OpenCV, pixel centres at integers; every pixel POSITION here has centres at integer +
0.5, as everywhere in the survey API.  The undistorted picture is a pinhole picture with one focal length f_out and its
principal point at its geometric centre, so nadir_affine(oh, ow, centre, gsd, yaw) holds for it with gsd = altitude / f_out.

  * lens_plan: the output geometry of one camera and frame size -- the largest picture without a filled pixel
    (keep='valid'), the smallest that holds the whole frame (keep='all'), or the caller's own;
  * distort_points / undistort_points: pixel positions between the raw frame and the pinhole picture of the SAME intrinsics
    (fx, fy, cx, cy without the five coefficients); lens_points does the same with a plan's output geometry, for detections
    made on raw frames;
  * undistorted: the frames of a survey as a lazy sequence of undistorted device frames (preprocess.undistort_u8,
    wm_undistort_u8), which detect_frames, mosaic, register and refine take as they take any sequence.
The geometry is numpy float64 on the host, in the rule's own expression; only the pixels are touched on the device.

Not here: estimating the coefficients from the survey's own overlaps, vignetting, fisheye and rational (k4..k6) models.
The roll and pitch of near-nadir flight are attitude.py's, which applies them and this model in one resampling; terrain relief
is terrain.py's (ortho_plan, orthorectified), which applies all three over a height grid in one resampling; truly oblique
cameras are covered by none of them."""
from __future__ import annotations

from typing import Dict

import numpy as np

import torch

from ._survey import _as_frame_array, _finite_number, _pinned_upload, _whole_number

CAMERA_ENTRIES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
LENS_MAX_SIDE = 65536                      # wm_undistort_u8's limit, which is wm_resample_u8's
LENS_KEEP = ("valid", "all")
_F = np.float64
_FOLD_GRID = 33                            # the coarse interior grid of the fold test, points per axis
_FOLD_STEPS = 16                           # points between the principal point and a solution at which undistort looks for a fold
_NEWTON_STEPS = 60
_NEWTON_TOL = 1e-9                         # undistort_points' contract, in pixels


# ---- validation ---------------------------------------------------------------------------------------------------------

def _check_camera(camera, what: str) -> np.ndarray:
    """(9,) float64: every entry finite, fx and fy > 0."""
    if isinstance(camera, torch.Tensor):
        camera = camera.detach().cpu().numpy()
    try:
        c = np.asarray(camera, dtype=_F)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: camera is not an array of numbers") from None
    if c.shape != (9,):
        raise ValueError(f"{what}: camera of shape {c.shape}: expected 9 numbers ({', '.join(CAMERA_ENTRIES)})")
    for name, v in zip(CAMERA_ENTRIES, c):
        _finite_number(v, what, f"camera {name}", (lambda x: x > 0.0) if name in ("fx", "fy") else (lambda x: True),
                       "must be finite and > 0" if name in ("fx", "fy") else "must be finite", echo_float=True)
    return np.ascontiguousarray(c)


def _check_size(size, what: str, name: str):
    """(height, width), whole numbers in 1..LENS_MAX_SIDE."""
    try:
        h, w = size
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} {size!r}: expected (height, width)") from None
    must = f"must be a whole number in 1..{LENS_MAX_SIDE}"
    return (_whole_number(h, what, f"{name} height", 1, LENS_MAX_SIDE, must=must, floats=True),
            _whole_number(w, what, f"{name} width", 1, LENS_MAX_SIDE, must=must, floats=True))


def _check_f_out(f_out, what: str) -> float:
    return _finite_number(f_out, what, "f_out", lambda f: f > 0.0, "must be finite and > 0")


def _check_points(pts, what: str) -> np.ndarray:
    if isinstance(pts, torch.Tensor):
        pts = pts.detach().cpu().numpy()
    try:
        p = np.asarray(pts, dtype=_F)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: pts is not an array of numbers") from None
    if p.size == 0 and p.ndim <= 1:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"{what}: pts of shape {p.shape}: expected (n, 2), (x, y) per point")
    return p


def _check_plan(plan, what: str) -> Dict[str, object]:
    """A lens_plan() dict, validated again (a plan is plain data and may have been edited or loaded)."""
    if not isinstance(plan, dict) or any(k not in plan for k in ("camera", "size", "out_size", "f_out")):
        raise ValueError(f"{what}: plan must be the dict lens_plan() returned (camera, size, out_size, f_out)")
    return {"camera": _check_camera(plan["camera"], what), "size": _check_size(plan["size"], what, "size"),
            "out_size": _check_size(plan["out_size"], what, "out_size"), "f_out": _check_f_out(plan["f_out"], what)}


# ---- the model, in normalised coordinates -------------------------------------------------------------------------------

def _distort(cam: np.ndarray, x, y):
    """(x, y) -> (xd, yd): the rule's expression, operation for operation (include/wm_hip.h "Survey lens")."""
    k1, k2, p1, p2, k3 = cam[4], cam[5], cam[6], cam[7], cam[8]
    r2 = x * x + y * y
    rad = _F(1.0) + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + (((_F(2.0) * p1) * x) * y + p2 * (r2 + _F(2.0) * (x * x)))
    yd = y * rad + (p1 * (r2 + _F(2.0) * (y * y)) + ((_F(2.0) * p2) * x) * y)
    return xd, yd


def _jacobian(cam: np.ndarray, x, y):
    """The four partial derivatives of (x, y) -> (xd, yd), and their determinant."""
    k1, k2, p1, p2, k3 = cam[4], cam[5], cam[6], cam[7], cam[8]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3))                  # d rad / d r2
    a = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
    b = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
    d = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
    return a, b, b, d, a * d - b * b


def _undistort(cam: np.ndarray, xd, yd, scale: float):
    """(xd, yd) -> (x, y) with _distort(x, y) == (xd, yd): Newton's iteration from (xd, yd), all points at once.  NaN where
    it has not come within _NEWTON_TOL / scale of the target (scale: pixels per unit, the larger focal length), where it
    left the finite numbers, or where it ended on or beyond a fold: a Jacobian determinant <= 0 at the solution or at one of
    _FOLD_STEPS points of the straight way to it from the principal point."""
    xd, yd = np.asarray(xd, dtype=_F), np.asarray(yd, dtype=_F)
    x, y = xd.copy(), yd.copy()
    tol = 0.1 * _NEWTON_TOL / scale
    with np.errstate(all="ignore"):
        for _ in range(_NEWTON_STEPS):
            ex, ey = _distort(cam, x, y)
            ex, ey = ex - xd, ey - yd
            if not (np.maximum(np.abs(ex), np.abs(ey)) > tol).any():          # NaN compares false: it cannot improve
                break
            a, b, c, d, det = _jacobian(cam, x, y)
            x, y = x - (d * ex - b * ey) / det, y - (a * ey - c * ex) / det
        ex, ey = _distort(cam, x, y)
        ok = (np.abs(ex - xd) <= tol) & (np.abs(ey - yd) <= tol)
        for t in np.linspace(1.0, 0.0, _FOLD_STEPS, endpoint=False):           # beyond a fold the determinant can be positive again
            ok &= _jacobian(cam, t * x, t * y)[4] > 0
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan)


def _source_positions(cam: np.ndarray, oh: int, ow: int, f_out: float, j, i):
    """The rule: the source position (u, v) of the output pixels of rows j and columns i (arrays that broadcast)."""
    f_out = _F(f_out)
    x = ((np.asarray(i, dtype=_F) + _F(0.5)) - _F(0.5) * _F(ow)) / f_out
    y = ((np.asarray(j, dtype=_F) + _F(0.5)) - _F(0.5) * _F(oh)) / f_out
    xd, yd = _distort(cam, x, y)
    return cam[0] * xd + (cam[2] + _F(0.5)), cam[1] * yd + (cam[3] + _F(0.5))


def _border(oh: int, ow: int):
    """(j, i) of the border pixels of an oh x ow picture, each once or twice."""
    js, is_ = np.arange(oh), np.arange(ow)
    j = np.concatenate([np.zeros(ow, np.int64), np.full(ow, oh - 1), js, js])
    i = np.concatenate([is_, is_, np.zeros(oh, np.int64), np.full(oh, ow - 1)])
    return j, i


def _none_filled(cam: np.ndarray, h: int, w: int, oh: int, ow: int, f_out: float) -> bool:
    """No border pixel of the oh x ow picture is filled: the rule's inside test on the rule's (u, v)."""
    if oh > LENS_MAX_SIDE or ow > LENS_MAX_SIDE:
        return False
    with np.errstate(all="ignore"):
        u, v = _source_positions(cam, oh, ow, f_out, *_border(oh, ow))
        return bool(((0 <= u) & (u < w) & (0 <= v) & (v < h)).all())


def _largest(ok, n: int) -> int:
    """The largest m >= n to which ok() holds all the way from n, ok(n) given: doubling, then bisection, then one by one
    until neither m + 1 nor m + 2 passes (an outermost pixel centre only moves outwards with the size)."""
    step = 1
    lo = n
    while lo + step <= LENS_MAX_SIDE and ok(lo + step):
        lo += step
        step *= 2
    hi = min(lo + step, LENS_MAX_SIDE + 1)                                      # ok(lo), not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    while True:
        grown = next((lo + d for d in (1, 2) if lo + d <= LENS_MAX_SIDE and ok(lo + d)), None)
        if grown is None:
            return lo
        lo = grown


def _grow_valid(none_filled, h: int, w: int):
    """keep='valid' given none_filled(oh, ow), which holds of (1, 1): pictures of the frame's own aspect are grown about the
    centre as far as none of their border pixels is filled; then the width, then the height, are grown on their own as far as
    they go, until neither can."""
    m = max(h, w)
    shape = lambda k: (max(1, k * h // m), max(1, k * w // m))
    oh, ow = shape(_largest(lambda k: none_filled(*shape(k)), 1))
    while True:
        ow2 = _largest(lambda n: none_filled(oh, n), ow)
        oh2 = _largest(lambda n: none_filled(n, ow2), oh)
        if (oh2, ow2) == (oh, ow):
            return oh, ow
        oh, ow = oh2, ow2


def _valid_size(cam: np.ndarray, h: int, w: int, f_out: float, what: str):
    """keep='valid': the largest centred picture of which no border pixel is filled (_grow_valid)."""
    if not _none_filled(cam, h, w, 1, 1, f_out):
        raise ValueError(f"{what}: keep='valid' is empty: the principal point ({cam[2]!r}, {cam[3]!r}) does not lie in the "
                         f"{h} x {w} frame, so the picture's centre pixel would already be filled")
    return _grow_valid(lambda oh, ow: _none_filled(cam, h, w, oh, ow, f_out), h, w)


def _size_that_holds(x, y, what: str):
    """The smallest centred (oh, ow) that holds the positions (x, y), pixels from the picture's centre."""
    side = lambda lo, hi: max(int(np.ceil(2.0 * -lo)), int(np.floor(2.0 * hi)) + 1, 1)     # -side / 2 <= lo, hi < side / 2
    oh, ow = side(y.min(), y.max()), side(x.min(), x.max())
    if oh > LENS_MAX_SIDE or ow > LENS_MAX_SIDE:
        raise ValueError(f"{what}: keep='all' needs {oh} x {ow} pixels, more than {LENS_MAX_SIDE} a side: pass a smaller f_out")
    return oh, ow


def _all_size(cam: np.ndarray, h: int, w: int, f_out: float, what: str):
    """keep='all': the smallest centred picture that holds the undistorted position of every border pixel centre."""
    j, i = _border(h, w)
    pts = undistort_points(cam, np.stack([i + 0.5, j + 0.5], axis=1))
    if not np.isfinite(pts).all():
        k = int(np.nonzero(~np.isfinite(pts).all(axis=1))[0][0])
        raise ValueError(f"{what}: the model folds over inside the frame: the border pixel (row {int(j[k])}, column {int(i[k])}) has no "
                         "undistorted position (the iteration did not converge on an orientation-preserving branch)")
    x = (pts[:, 0] - (cam[2] + 0.5)) / cam[0] * f_out
    y = (pts[:, 1] - (cam[3] + 0.5)) / cam[1] * f_out
    return _size_that_holds(x, y, what)


def _check_no_fold(cam: np.ndarray, oh: int, ow: int, f_out: float, what: str, rays=None) -> None:
    """ValueError when the Jacobian determinant of (x, y) -> (xd, yd) is <= 0 (or not finite) on the border of the output or
    on a coarse grid over its inside: the picture would show parts of the frame twice, mirrored.  rays (attitude.py): the
    map (x, y) -> (xn, yn, in front) that comes before the lens; the Jacobian is then taken at (xn, yn), and a point that is
    not in front of the camera, which is filled and never sampled, is not looked at."""
    j, i = _border(oh, ow)
    gj, gi = np.meshgrid(np.linspace(0, oh - 1, _FOLD_GRID), np.linspace(0, ow - 1, _FOLD_GRID), indexing="ij")
    j, i = np.concatenate([j, gj.ravel()]), np.concatenate([i, gi.ravel()])
    x, y = ((i + 0.5) - 0.5 * ow) / f_out, ((j + 0.5) - 0.5 * oh) / f_out
    with np.errstate(all="ignore"):
        front = True
        if rays is not None:
            x, y, front = rays(x, y)
        det = _jacobian(cam, x, y)[4]
    bad = ~(det > 0) & front
    if bad.any():
        idx = np.nonzero(bad)[0]
        k = int(idx[np.argmin((x * x + y * y)[idx])])                       # the nearest to the centre
        raise ValueError(f"{what}: the model folds over inside the {oh} x {ow} output: its Jacobian determinant is {det[k]:.3g} <= 0 at "
                         f"row {j[k]:.0f}, column {i[k]:.0f} ({np.hypot(x[k], y[k]) * f_out:.0f} px from the centre); the coefficients do not "
                         "describe a lens out to there -- pass a smaller out_size, or check k1, k2, k3")


# ---- the public functions ---------------------------------------------------------------------------------------------------

def lens_plan(camera, size, keep: str = "valid", out_size=None, f_out=None) -> Dict[str, object]:
    """The output geometry for undistorting frames of `size` = (height, width) taken with `camera` (fx, fy, cx, cy, k1, k2,
    p1, p2, k3).  Returns {'camera': (9,) float64, 'size': (h, w), 'out_size': (oh, ow), 'f_out': float}: plain data, what
    undistort_u8, undistorted and lens_points take.  Host only, numpy float64.
    f_out: the focal length of the output, default fx, which leaves the resolution at the principal point -- and hence the
    ground sampling distance there -- as it was.
    keep='valid': the largest centred picture of which no pixel is filled, decided by the rule itself -- the rule's (u, v)
    and inside test on the candidate's border pixels (for an orientation-preserving map the inside follows).  Pictures of the
    frame's aspect are grown as far as they pass, then each side on its own, so neither side can grow by one or two.
    keep='all': the smallest centred picture that holds the undistorted position of every border pixel centre of the frame;
    its corners, or its edges' middles, are filled.
    out_size=(oh, ow): the caller's own picture; keep is then not used.
    ValueError: malformed arguments; an empty picture; a picture larger than 65536 a side; and a model that folds over inside
    the output -- the Jacobian determinant of (x, y) -> (xd, yd) is <= 0 on the output's border or on a coarse grid over its
    inside (keep='all': a border pixel of the frame has no undistorted position)."""
    what = "lens_plan"
    cam = _check_camera(camera, what)
    h, w = _check_size(size, what, "size")
    if not isinstance(keep, str) or keep not in LENS_KEEP:
        raise ValueError(f"{what}: keep {keep!r} must be 'valid' or 'all'")
    f = float(cam[0]) if f_out is None else _check_f_out(f_out, what)
    if out_size is not None:
        oh, ow = _check_size(out_size, what, "out_size")
    elif keep == "valid":
        oh, ow = _valid_size(cam, h, w, f, what)
    else:
        oh, ow = _all_size(cam, h, w, f, what)
    _check_no_fold(cam, oh, ow, f, what)
    return {"camera": cam, "size": (h, w), "out_size": (oh, ow), "f_out": f}


def distort_points(camera, pts) -> np.ndarray:
    """(n, 2) pixel positions (x, y) of the pinhole picture with the camera's own fx, fy, cx, cy -> their positions in the raw
    frame: the closed form, u = fx * xd + (cx + 0.5) of x = (px - (cx + 0.5)) / fx.  Host only, float64."""
    what = "distort_points"
    cam, p = _check_camera(camera, what), _check_points(pts, what)
    cu, cv = cam[2] + _F(0.5), cam[3] + _F(0.5)
    with np.errstate(all="ignore"):
        xd, yd = _distort(cam, (p[:, 0] - cu) / cam[0], (p[:, 1] - cv) / cam[1])
        return np.stack([cam[0] * xd + cu, cam[1] * yd + cv], axis=1)


def undistort_points(camera, pts) -> np.ndarray:
    """The inverse of distort_points, by Newton's iteration: (n, 2) raw-frame positions -> positions in the pinhole picture
    of the same fx, fy, cx, cy.  distort_points(undistort_points(p)) == p within 1e-9 px for points inside the frame of a
    camera that lens_plan accepts; NaN, both coordinates, where the iteration does not converge or ends where the model has
    folded over."""
    what = "undistort_points"
    cam, p = _check_camera(camera, what), _check_points(pts, what)
    cu, cv = cam[2] + _F(0.5), cam[3] + _F(0.5)
    x, y = _undistort(cam, (p[:, 0] - cu) / cam[0], (p[:, 1] - cv) / cam[1], float(max(cam[0], cam[1])))
    out = np.stack([cam[0] * x + cu, cam[1] * y + cv], axis=1)
    with np.errstate(all="ignore"):
        back = distort_points(cam, out)
        ok = (np.abs(back - p) <= _NEWTON_TOL).all(axis=1)
    out[~ok] = np.nan
    return out


def lens_points(plan, pts, to: str = "undistorted") -> np.ndarray:
    """(n, 2) pixel positions (x, y) between the raw frame and the plan's undistorted picture.  to='undistorted': raw ->
    undistorted, for detections made on raw frames (NaN where undistort_points gives NaN); to='raw': undistorted -> raw, the
    rule's own (u, v) -- for a pixel centre (i + 0.5, j + 0.5) exactly the position the kernel samples.  Host only."""
    what = "lens_points"
    pl = _check_plan(plan, what)
    p = _check_points(pts, what)
    if not isinstance(to, str) or to not in ("undistorted", "raw"):
        raise ValueError(f"{what}: to {to!r} must be 'undistorted' or 'raw'")
    cam, (oh, ow), f = pl["camera"], pl["out_size"], _F(pl["f_out"])
    cu, cv = cam[2] + _F(0.5), cam[3] + _F(0.5)
    with np.errstate(all="ignore"):
        if to == "raw":
            xd, yd = _distort(cam, (p[:, 0] - _F(0.5) * _F(ow)) / f, (p[:, 1] - _F(0.5) * _F(oh)) / f)
            return np.stack([cam[0] * xd + cu, cam[1] * yd + cv], axis=1)
        x, y = _undistort(cam, (p[:, 0] - cu) / cam[0], (p[:, 1] - cv) / cam[1], float(max(cam[0], cam[1])))
        return np.stack([x * f + _F(0.5) * _F(ow), y * f + _F(0.5) * _F(oh)], axis=1)


class undistorted:
    """The frames of a survey, undistorted: a lazy sequence over `frames` (anything with len() and frames[i]: a list of
    (H,W,3) uint8 ROCm tensors, CPU tensors or numpy arrays, or a sequence that loads frame i when it is asked for).
    u[i] indexes frames[i] once -- never before -- sends a host frame up through pinned memory, and returns the
    (oh, ow, 3) uint8 device frame preprocess.undistort_u8(frames[i], plan, sample, fill) on the current device's current
    stream; nothing is kept.  len(u), iteration and u.sizes, the (n, 2) int64 (oh, ow) of every frame, cost nothing.

    This is the whole integration: detect_frames(model, u) takes it as its iterable, and mosaic(u, georef, cell,
    sizes=u.sizes), register(...) and refine(...) take it with sizes=u.sizes; their georeferences are those of the
    undistorted picture (nadir_affine(oh, ow, centre, altitude / f_out, yaw)).  Every frame must have the plan's size.
    Known limit: detect_frames overlaps a HOST frame's upload with the previous batch on its copy stream; a host frame that
    comes through this wrapper is uploaded and undistorted on the current stream when it is indexed, and is not overlapped."""

    def _take(self, frames, sample, fill) -> None:
        what = type(self).__name__
        if not (hasattr(frames, "__getitem__") and hasattr(frames, "__len__")):
            raise ValueError(f"{what}: frames must be a sequence that can be indexed (frames[i], len), got {type(frames).__name__}")
        from .preprocess import _check_undistort_args
        self.sample, self.fill = sample, fill
        _check_undistort_args(sample, fill, what)
        self.frames = frames

    def __init__(self, frames, plan, sample: str = "bilinear", fill=(0, 0, 0)):
        self._take(frames, sample, fill)
        self.plan = _check_plan(plan, "undistorted")
        self.sizes = np.tile(np.asarray(self.plan["out_size"], dtype=np.int64), (len(frames), 1)).reshape(-1, 2)

    def __len__(self) -> int:
        return len(self.frames)

    def _resample(self, frame, i: int):
        """The device frame i, resampled (attitude.rectified has a plan per frame and another call)."""
        from . import preprocess
        return preprocess.undistort_u8(frame, self.plan, self.sample, self.fill)

    def __getitem__(self, i):
        n, who = len(self.frames), type(self).__name__
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
            raise TypeError(f"{who}: index {i!r} is not a whole number")
        if not -n <= i < n:
            raise IndexError(f"{who}: index {i} of {n} frames")
        i = int(i) % n
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who}: no ROCm device (there is no CPU fallback in wildlifemapper_amd)")
        dev = torch.device("cuda", torch.cuda.current_device())
        on_dev, on_host = _as_frame_array(self.frames[i], i, dev, who)
        fr = on_dev if on_dev is not None else _pinned_upload(on_host, dev)
        return self._resample(fr, i)

    def __iter__(self):
        return (self[i] for i in range(len(self)))
