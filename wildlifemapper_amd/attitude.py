"""Survey attitude: the frames of a survey rectified to nadir by the roll and pitch the flight log records next to each GPS
fix, so that the one affine per frame of census(), coverage(), mosaic(), register() and refine() is true of frames taken by
an aircraft that was not level (rule: include/wm_hip.h "Survey attitude").  The rotation and the lens model of lens.py are
applied in ONE resampling: a frame is neither blurred nor paid for twice.

Convention.  The camera is fixed to the airframe, its optical axis points down, the picture's up direction is the nose and
the picture's right the right wing; yaw stays where it is, in nadir_affine.  Pitch > 0 is nose up: the axis swings towards
the picture's up direction.  Roll > 0 is right wing down: the axis swings towards the picture's left.  Both the level
(nadir) camera and the real one have x to the picture's right, y down the picture and z along the optical axis; with
P = [[1,0,0],[0,cos t,-sin t],[0,sin t,cos t]] (t = pitch) and Q = [[cos p,0,-sin p],[0,1,0],[sin p,0,cos p]] (p = roll),
A = P @ Q maps airframe to level and rot = A.T maps a ray of the level camera into the real one, d_cam = rot @ d_nadir.  The
third column of A, the optical axis in level coordinates, is (-sin p, -sin t cos p, cos t cos p).

  * attitude_rotation: (roll, pitch) in degrees -> rot;
  * rectify_plan: the output geometry of one camera, frame size and rotation -- lens_plan's dict plus 'rotation'.  The
    rectified picture is a pinhole picture with one focal length f_out and its principal point at its geometric centre, so
    nadir_affine(oh, ow, position, altitude / f_out, yaw) holds for it, position being the ground point straight below the
    camera: the GPS fix itself;
  * attitude_points: pixel positions between the raw frame and the rectified picture, for detections made on raw frames;
  * rectified: the frames of a survey as a lazy sequence of rectified device frames (preprocess.rectify_u8, wm_rectify_u8),
    one plan per frame.
The geometry is numpy float64 on the host, in the rule's own expressions; only the pixels are touched on the device.

Not here: truly oblique cameras (a rotation is refused beyond max_tilt_deg, 30 by default), estimating the attitude from the
survey's own overlaps, and a lever arm or boresight misalignment between the log's attitude and the camera (pass the corrected
3 x 3 rotation instead).  The ground is the plane of nadir_affine: over terrain relief use terrain.py instead (ortho_plan,
orthorectified), which takes the same rotation and applies it, the lens model and a height grid in one resampling."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

import torch

from .lens import (LENS_KEEP, LENS_MAX_SIDE, _F, _border, _check_camera, _check_f_out, _check_no_fold, _check_plan, _check_points, _check_size, _distort,
                   _grow_valid, _size_that_holds, _undistort, undistorted)
from ._survey import _finite_number

MAX_TILT_DEG = 30.0                        # near-nadir flight, not oblique cameras
_ORTHONORMAL_TOL = 1e-9


# ---- the rotation ---------------------------------------------------------------------------------------------------------

def attitude_rotation(roll_deg, pitch_deg) -> np.ndarray:
    """rot (..., 3, 3) float64 of roll and pitch in degrees (numbers or arrays that broadcast), in the module's convention:
    rot = (P @ Q).T, d_cam = rot @ d_nadir.  Pitch > 0 is nose up, roll > 0 is right wing down; the optical axis in level
    coordinates, rot[2, :], is (-sin p, -sin t cos p, cos t cos p).  Host only."""
    try:
        p, t = np.broadcast_arrays(np.radians(np.asarray(roll_deg, dtype=_F)), np.radians(np.asarray(pitch_deg, dtype=_F)))
    except (TypeError, ValueError):
        raise ValueError("attitude_rotation: roll_deg and pitch_deg must be numbers or arrays of numbers that broadcast") from None
    if not (np.isfinite(p).all() and np.isfinite(t).all()):
        raise ValueError("attitude_rotation: roll_deg and pitch_deg must be finite")
    P = np.zeros(p.shape + (3, 3), dtype=_F)
    Q = np.zeros(p.shape + (3, 3), dtype=_F)
    P[..., 0, 0] = 1.0
    P[..., 1, 1], P[..., 1, 2], P[..., 2, 1], P[..., 2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    Q[..., 1, 1] = 1.0
    Q[..., 0, 0], Q[..., 0, 2], Q[..., 2, 0], Q[..., 2, 2] = np.cos(p), -np.sin(p), np.sin(p), np.cos(p)
    return np.ascontiguousarray(np.swapaxes(P @ Q, -1, -2))


def _check_rotation(rotation, what: str, max_tilt_deg=MAX_TILT_DEG) -> np.ndarray:
    """(3, 3) float64 of `rotation`: (roll_deg, pitch_deg), or a ready 3 x 3 matrix, which must be orthonormal within 1e-9
    with determinant > 0; either is refused when it tilts the axis by more than max_tilt_deg (rot[2][2] < cos(max_tilt_deg))."""
    tilt = _finite_number(max_tilt_deg, what, "max_tilt_deg", lambda v: 0.0 <= v < 90.0, "must be in [0, 90)")
    if isinstance(rotation, torch.Tensor):
        rotation = rotation.detach().cpu().numpy()
    try:
        r = np.asarray(rotation, dtype=_F)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: rotation is not an array of numbers") from None
    if r.shape == (2,):
        if not np.isfinite(r).all():
            raise ValueError(f"{what}: rotation (roll_deg, pitch_deg) {r.tolist()} must be finite")
        r = attitude_rotation(r[0], r[1])
    if r.shape != (3, 3):
        raise ValueError(f"{what}: rotation of shape {r.shape}: expected (roll_deg, pitch_deg) or a (3, 3) matrix")
    if not np.isfinite(r).all():
        raise ValueError(f"{what}: rotation must be finite")
    off = float(np.abs(r @ r.T - np.eye(3)).max())
    if off > _ORTHONORMAL_TOL or not np.linalg.det(r) > 0:
        raise ValueError(f"{what}: rotation is not a rotation matrix: rot @ rot.T differs from the identity by {off:.3g} (allowed "
                         f"{_ORTHONORMAL_TOL:g}), determinant {np.linalg.det(r):.6g}")
    if r[2, 2] < math.cos(math.radians(tilt)):
        raise ValueError(f"{what}: rotation tilts the optical axis by {math.degrees(math.acos(min(1.0, r[2, 2]))):.2f} degrees, more than "
                         f"max_tilt_deg {tilt:g}: this is for near-nadir flight, not oblique cameras")
    return np.ascontiguousarray(r)


def _check_rectify_plan(plan, what: str) -> Dict[str, object]:
    """A rectify_plan() dict, validated again (a plan is plain data and may have been edited or loaded).  The rotation must be
    a rotation that looks down (tilt < 90 degrees); the limit of max_tilt_deg was rectify_plan's to apply."""
    if not isinstance(plan, dict) or "rotation" not in plan:
        raise ValueError(f"{what}: plan must be the dict rectify_plan() returned (camera, size, out_size, f_out, rotation)")
    return dict(_check_plan(plan, what), rotation=_check_rotation(plan["rotation"], what, max_tilt_deg=89.999))


# ---- the rule, in numpy ----------------------------------------------------------------------------------------------------

def _rays(rot: np.ndarray, x, y):
    """(x, y) of the level picture -> (xn, yn, Z > 0): the rule's expressions, operation for operation."""
    X = (rot[0, 0] * x + rot[0, 1] * y) + rot[0, 2]
    Y = (rot[1, 0] * x + rot[1, 1] * y) + rot[1, 2]
    Z = (rot[2, 0] * x + rot[2, 1] * y) + rot[2, 2]
    return X / Z, Y / Z, Z > 0


def _source_positions(cam: np.ndarray, rot: np.ndarray, oh: int, ow: int, f_out: float, px, py):
    """The rule: (u, v, Z > 0) of the positions (px, py) of the oh x ow rectified picture (pixel centres at integer + 0.5)."""
    f_out = _F(f_out)
    x = (np.asarray(px, dtype=_F) - _F(0.5) * _F(ow)) / f_out
    y = (np.asarray(py, dtype=_F) - _F(0.5) * _F(oh)) / f_out
    xn, yn, front = _rays(rot, x, y)
    xd, yd = _distort(cam, xn, yn)
    return cam[0] * xd + (cam[2] + _F(0.5)), cam[1] * yd + (cam[3] + _F(0.5)), front


def _none_filled(cam, rot, h: int, w: int, oh: int, ow: int, f_out: float) -> bool:
    """No border pixel of the oh x ow picture is filled: the rule's Z > 0 and inside test on the rule's (u, v)."""
    if oh > LENS_MAX_SIDE or ow > LENS_MAX_SIDE:
        return False
    j, i = _border(oh, ow)
    with np.errstate(all="ignore"):
        u, v, front = _source_positions(cam, rot, oh, ow, f_out, i.astype(_F) + _F(0.5), j.astype(_F) + _F(0.5))
        return bool((front & (0 <= u) & (u < w) & (0 <= v) & (v < h)).all())


def _to_rectified(cam, rot, f_out: float, oh: int, ow: int, p: np.ndarray) -> np.ndarray:
    """Raw positions -> positions in the rectified picture: lens inverse (Newton), rot.T, divide, f_out.  NaN where the lens
    inverse is NaN or where the back-rotated z is <= 0."""
    f = _F(f_out)
    with np.errstate(all="ignore"):
        xn, yn = _undistort(cam, (p[:, 0] - (cam[2] + _F(0.5))) / cam[0], (p[:, 1] - (cam[3] + _F(0.5))) / cam[1], float(max(cam[0], cam[1])))
        X = rot[0, 0] * xn + rot[1, 0] * yn + rot[2, 0]
        Y = rot[0, 1] * xn + rot[1, 1] * yn + rot[2, 1]
        Z = rot[0, 2] * xn + rot[1, 2] * yn + rot[2, 2]
        out = np.stack([X / Z * f + _F(0.5) * _F(ow), Y / Z * f + _F(0.5) * _F(oh)], axis=1)
    out[~(Z > 0)] = np.nan
    return out


# ---- the public functions --------------------------------------------------------------------------------------------------

def rectify_plan(camera, size, rotation, keep: str = "valid", out_size=None, f_out=None, max_tilt_deg=MAX_TILT_DEG) -> Dict[str, object]:
    """The output geometry for rectifying frames of `size` = (height, width) taken with `camera` (lens.py's nine numbers) at
    `rotation`: (roll_deg, pitch_deg), or a ready (3, 3) rotation with d_cam = rot @ d_nadir, for example one built from
    omega-phi-kappa (orthonormal within 1e-9, determinant > 0).  Returns lens_plan's dict plus 'rotation', the (3, 3) float64:
    plain data, what rectify_u8, rectified and attitude_points take.  Host only, numpy float64.
    The picture's principal point is at its geometric centre and looks straight down, so nadir_affine(oh, ow, position,
    altitude / f_out, yaw) holds for it with position the ground point below the camera.  f_out defaults to fx.
    keep means what it means in lens_plan, decided by the rule's own (u, v), Z > 0 and inside test on the candidate's border:
    'valid' is the largest CENTRED picture with no filled pixel, 'all' the smallest centred picture that holds the rectified
    position of every border pixel centre of the frame; out_size=(oh, ow) is the caller's own.  The point below the camera
    lies f tan(tilt) from the frame's principal point, so a centred valid picture of a tilted frame is smaller than the frame
    by about 2 f tan(tilt) along the tilt: 460 px of 3648 at 3 degrees and f = 4400.  keep='all' loses nothing, and fills.
    ValueError: malformed arguments; a tilt beyond max_tilt_deg (default 30: near-nadir flight, not oblique cameras); an
    empty picture (the point below the camera is not in the frame); a picture larger than 65536 a side; and a lens model that
    folds over inside the output, its Jacobian taken at the rotated (xn, yn)."""
    what = "rectify_plan"
    cam = _check_camera(camera, what)
    h, w = _check_size(size, what, "size")
    rot = _check_rotation(rotation, what, max_tilt_deg)
    if not isinstance(keep, str) or keep not in LENS_KEEP:
        raise ValueError(f"{what}: keep {keep!r} must be 'valid' or 'all'")
    f = float(cam[0]) if f_out is None else _check_f_out(f_out, what)
    if out_size is not None:
        oh, ow = _check_size(out_size, what, "out_size")
    elif keep == "valid":
        if not _none_filled(cam, rot, h, w, 1, 1, f):
            raise ValueError(f"{what}: keep='valid' is empty: the point straight below the camera does not lie in the {h} x {w} frame, so "
                             "the picture's centre pixel would already be filled")
        oh, ow = _grow_valid(lambda a, b: _none_filled(cam, rot, h, w, a, b, f), h, w)
    else:
        j, i = _border(h, w)
        pts = _to_rectified(cam, rot, f, 0, 0, np.stack([i + 0.5, j + 0.5], axis=1))        # pixels from the picture's centre
        if not np.isfinite(pts).all():
            k = int(np.nonzero(~np.isfinite(pts).all(axis=1))[0][0])
            raise ValueError(f"{what}: the border pixel (row {int(j[k])}, column {int(i[k])}) of the frame has no rectified position: the "
                             "lens model folds over inside the frame, or the pixel looks above the horizon")
        oh, ow = _size_that_holds(pts[:, 0], pts[:, 1], what)
    _check_no_fold(cam, oh, ow, f, what, rays=lambda x, y: _rays(rot, x, y))
    return {"camera": cam, "size": (h, w), "out_size": (oh, ow), "f_out": f, "rotation": rot}


def attitude_points(plan, pts, to: str = "rectified") -> np.ndarray:
    """(n, 2) pixel positions (x, y) between the raw frame and the plan's rectified picture.  to='rectified': raw ->
    rectified, for detections made on raw frames -- lens.undistort_points' Newton iteration, then rot.T, the division and
    f_out; NaN where the lens inverse is NaN or where the back-rotated z is <= 0.  to='raw': rectified -> raw, the rule's own
    (u, v) in closed form -- for a pixel centre (i + 0.5, j + 0.5) exactly the position the kernel samples; NaN where the rule
    has Z <= 0.  Host only."""
    what = "attitude_points"
    pl = _check_rectify_plan(plan, what)
    p = _check_points(pts, what)
    if not isinstance(to, str) or to not in ("rectified", "raw"):
        raise ValueError(f"{what}: to {to!r} must be 'rectified' or 'raw'")
    cam, rot, (oh, ow), f = pl["camera"], pl["rotation"], pl["out_size"], pl["f_out"]
    if to == "rectified":
        return _to_rectified(cam, rot, f, oh, ow, p)
    with np.errstate(all="ignore"):
        u, v, front = _source_positions(cam, rot, oh, ow, f, p[:, 0], p[:, 1])
    out = np.stack([u, v], axis=1)
    out[~front] = np.nan
    return out


class rectified(undistorted):
    """The frames of a survey, rectified to nadir: the lazy sequence lens.undistorted is -- r[i] indexes frames[i] once, never
    before, and returns the device frame preprocess.rectify_u8(frames[i], r.plans[i], sample, fill); nothing is kept -- with
    one plan per frame, because every frame has its own attitude.  rotations: (n, 3, 3), or (n, 2) as (roll_deg, pitch_deg)
    per frame; camera, keep, out_size, f_out and max_tilt_deg as in rectify_plan.  size=(height, width), by keyword, is the size
    every frame must have: the plans are made before any frame is indexed, so it cannot be read off the frames.  r.plans
    is the list of plans, r.sizes the (n, 2) int64 (oh, ow) of every frame, which differ from frame to frame with keep=;
    detect_frames(model, r), mosaic(r, georef, cell, sizes=r.sizes), register(...) and refine(...) take them, with the
    georeferences of the rectified pictures: nadir_affine(oh_i, ow_i, position_i, altitude_i / f_out, yaw_i)."""

    def __init__(self, frames, camera, rotations, keep: str = "valid", out_size=None, f_out=None, sample: str = "bilinear",
                 fill=(0, 0, 0), *, size, max_tilt_deg=MAX_TILT_DEG):
        self._take(frames, sample, fill)
        if isinstance(rotations, torch.Tensor):
            rotations = rotations.detach().cpu().numpy()
        try:
            r = np.asarray(rotations, dtype=_F)
        except (TypeError, ValueError):
            raise ValueError("rectified: rotations is not an array of numbers") from None
        n = len(frames)
        if r.shape not in ((n, 2), (n, 3, 3)):
            raise ValueError(f"rectified: rotations of shape {r.shape} for {n} frames: expected ({n}, 3, 3), or ({n}, 2) as roll, pitch in degrees")
        self.plans = [rectify_plan(camera, size, r[k], keep, out_size, f_out, max_tilt_deg) for k in range(n)]
        self.sizes = np.array([pl["out_size"] for pl in self.plans], dtype=np.int64).reshape(-1, 2)

    def _resample(self, frame, i: int):
        from . import preprocess
        return preprocess.rectify_u8(frame, self.plans[i], self.sample, self.fill)
