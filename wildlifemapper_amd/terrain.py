"""Survey terrain: the frames of a survey orthorectified over a digital elevation model (DEM), so that the one affine per
frame of census(), coverage(), mosaic(), register() and refine() is true of frames taken over ground that is not flat (rule:
include/wm_hip.h "Survey terrain").  lens.py removes the lens and attitude.py roll and pitch, but both take the ground for
the plane of nadir_affine: a point z metres above that plane, d from the nadir point of a camera H above it, is seen at
d * H / (H - z) -- at H = 120 m a 10 m rise moves an animal 40 m out by 3.6 m, away from each frame's own nadir, so two frames
count it twice.  No similarity per frame absorbs that; the orthophoto does.  Lens, attitude, yaw, position and relief are
applied in ONE resampling: a frame is neither blurred nor paid for twice, and where a DEM exists this replaces rectified().

  * terrain_grid: a DEM as plain data -- float32 posts at cell centres, north-up, the east and north of the grid's top-left
    corner and the post spacing; terrain_height: the rule's bilinear height of ground points, NaN off the grid;
  * camera_pose: position, height (in the DEM's datum), yaw and an optional attitude.py rotation -> the rule's pose[12];
  * ortho_plan: the output grid of one frame: nadir_affine(oh, ow, centre, cell, yaw_out), sized by keep= as lens_plan's is;
  * terrain_points: raw-frame pixel positions -> ground (E, N) by intersecting the ray with the DEM, for detections made on
    raw frames; ground -> raw, the rule in closed form; ground -> orthophoto pixel;
  * orthorectified: the frames of a survey as a lazy sequence of orthophotos (preprocess.ortho_u8, wm_ortho_u8), one plan per
    frame, with .georef to hand to census, coverage, mosaic, register and refine.
The geometry is numpy float64 on the host, in the rule's own expressions; only the pixels are touched on the device.

Not here: occlusion (a cell hidden behind a ridge shows the ridge's pixel: no true-ortho visibility); estimating or refining
the DEM, or a pose's height, from the survey's own overlaps; DEM file formats (the caller brings an array); geoid and datum
conversion (the pose's height must be in the DEM's own vertical datum); and coverage() counts a filled orthophoto pixel as
seen -- keep='valid' has none."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

import torch

from ._survey import _finite_number
from .attitude import MAX_TILT_DEG, _check_rotation
from .ground import ground_to_pixel, nadir_affine
from .lens import (LENS_KEEP, LENS_MAX_SIDE, _F, _border, _check_camera, _check_points, _check_size, _distort, _grow_valid, _size_that_holds,
                   _undistort, undistorted)

TERRAIN_MAX_SIDE = 32768                   # wm_ortho_u8's limit on the DEM's sides
TERRAIN_TOL_M = 1e-9                       # terrain_points' stopping rule, metres of height between two steps
TERRAIN_STEPS = 64


# ---- the DEM --------------------------------------------------------------------------------------------------------------

def terrain_grid(heights, origin, cell, device=None) -> Dict[str, object]:
    """A DEM as plain data: {'heights': (dh, dw) float32 on the host, 'origin': (e0, n0), 'cell': dcell, 'device_heights': the
    posts on a ROCm device, or None until to_device() puts them there}.  heights: a (dh, dw) array or tensor, host or device,
    of numbers that float32 holds; row 0 is the NORTHERNMOST, heights are at cell centres, and a post that is not finite is
    nodata.  origin = (e0, n0): east and north of the grid's top-left corner, so post [r][c] stands at (e0 + (c + 0.5) cell,
    n0 - (r + 0.5) cell); cell: the post spacing in metres.  device=: upload the posts now (a device tensor given as heights
    is kept as it is)."""
    what = "terrain_grid"
    dev_t = None
    if isinstance(heights, torch.Tensor):
        if heights.is_cuda and heights.dtype == torch.float32 and heights.dim() == 2:
            dev_t = heights.contiguous()
        heights = heights.detach().cpu().numpy()
    try:
        z = np.asarray(heights)
        if z.dtype.kind not in "iuf":
            raise TypeError
        z = np.ascontiguousarray(z, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: heights is not an array of numbers") from None
    if z.ndim != 2 or not all(2 <= s <= TERRAIN_MAX_SIDE for s in z.shape):
        raise ValueError(f"{what}: heights of shape {z.shape}: expected (rows, columns), each in 2..{TERRAIN_MAX_SIDE}")
    try:
        e0, n0 = origin
    except (TypeError, ValueError):
        raise ValueError(f"{what}: origin {origin!r}: expected (east, north) of the grid's top-left corner") from None
    e0 = _finite_number(e0, what, "origin east", lambda v: True, "must be finite")
    n0 = _finite_number(n0, what, "origin north", lambda v: True, "must be finite")
    dcell = _finite_number(cell, what, "cell", lambda v: v > 0.0, "must be finite and > 0")
    dem = {"heights": z, "origin": (e0, n0), "cell": dcell, "device_heights": dev_t}
    if device is not None:
        to_device(dem, device)
    return dem


def _check_dem(dem, what: str) -> Dict[str, object]:
    """A terrain_grid() dict, validated again (it is plain data and may have been edited or loaded)."""
    if not isinstance(dem, dict) or any(k not in dem for k in ("heights", "origin", "cell")):
        raise ValueError(f"{what}: dem must be the dict terrain_grid() returned (heights, origin, cell)")
    z = dem["heights"]
    if not isinstance(z, np.ndarray) or z.dtype != np.float32 or z.ndim != 2 or not all(2 <= s <= TERRAIN_MAX_SIDE for s in z.shape):
        raise ValueError(f"{what}: dem heights must be a (rows, columns) float32 array, each side in 2..{TERRAIN_MAX_SIDE}: make it with terrain_grid()")
    try:
        e0, n0 = dem["origin"]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: dem origin {dem['origin']!r}: expected (east, north)") from None
    e0 = _finite_number(e0, what, "dem origin east", lambda v: True, "must be finite")
    n0 = _finite_number(n0, what, "dem origin north", lambda v: True, "must be finite")
    dcell = _finite_number(dem["cell"], what, "dem cell", lambda v: v > 0.0, "must be finite and > 0")
    return {"heights": np.ascontiguousarray(z), "origin": (e0, n0), "cell": dcell}


def to_device(dem, device) -> torch.Tensor:
    """The DEM's posts on `device`, a (dh, dw) float32 tensor: uploaded once, then kept in dem['device_heights']."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"to_device: {dev} is no ROCm device (there is no CPU fallback in wildlifemapper_amd)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    have = dem.get("device_heights")
    if not (isinstance(have, torch.Tensor) and have.device == dev and have.dtype == torch.float32 and tuple(have.shape) == dem["heights"].shape):
        have = torch.from_numpy(dem["heights"]).to(dev)
        dem["device_heights"] = have
    return have


def _height(z32: np.ndarray, e0: float, n0: float, dcell: float, E, N):
    """The rule's height: (z, the position has a height) of ground positions (E, N), operation for operation.  z is NaN
    where there is no height."""
    dh, dw = z32.shape
    e0, n0, dcell = _F(e0), _F(n0), _F(dcell)
    a = (E - e0) / dcell - _F(0.5)
    b = (n0 - N) / dcell - _F(0.5)
    has = (0 <= a) & (a <= dw - 1) & (0 <= b) & (b <= dh - 1)
    ia = np.minimum(np.floor(np.where(has, a, 0.0)).astype(np.int64), dw - 2)
    ib = np.minimum(np.floor(np.where(has, b, 0.0)).astype(np.int64), dh - 2)
    ta, tb = a - ia.astype(_F), b - ib.astype(_F)
    z00, z01, z10, z11 = (z32[ib + r, ia + c].astype(_F) for r in (0, 1) for c in (0, 1))
    z = (z00 * (_F(1.0) - ta) + z01 * ta) * (_F(1.0) - tb) + (z10 * (_F(1.0) - ta) + z11 * ta) * tb
    return np.where(has, z, np.nan), has


def terrain_height(dem, points) -> np.ndarray:
    """(n,) float64: the rule's bilinear height of the ground points (n, 2) (east, north); NaN off the grid -- beyond the
    outermost posts' centres -- and where a nodata post takes part.  Host only."""
    what = "terrain_height"
    d, p = _check_dem(dem, what), _check_points(points, what)
    with np.errstate(all="ignore"):
        return _height(d["heights"], *d["origin"], d["cell"], p[:, 0], p[:, 1])[0]


# ---- the pose -------------------------------------------------------------------------------------------------------------

def _level(yaw_deg: float) -> np.ndarray:
    """L(psi): world (east, north, up) -> the level camera whose picture-up heading is psi clockwise from north; its first two
    rows are nadir_affine's (a0, a1) and (a3, a4) over the ground sampling distance."""
    psi = math.radians(yaw_deg)
    c, s = math.cos(psi), math.sin(psi)
    return np.array([[c, -s, 0.0], [-s, -c, 0.0], [0.0, 0.0, -1.0]], dtype=_F)


def camera_pose(position, height, yaw_deg, rotation=None, max_tilt_deg=MAX_TILT_DEG) -> np.ndarray:
    """pose (12,) float64 = Ce, Cn, Cu, m0..m8 of a camera at `position` = (east, north) and `height`, in the DEM's own vertical
    datum, whose picture-up heading is yaw_deg clockwise from north (nadir_affine's yaw).  M = rot @ L(yaw): rotation, as
    rectify_plan takes it, is (roll_deg, pitch_deg) or a ready (3, 3) matrix with d_cam = rot @ d_nadir, refused beyond
    max_tilt_deg; None is a level camera.  Host only."""
    what = "camera_pose"
    try:
        ce, cn = position
    except (TypeError, ValueError):
        raise ValueError(f"{what}: position {position!r}: expected (east, north)") from None
    ce = _finite_number(ce, what, "position east", lambda v: True, "must be finite")
    cn = _finite_number(cn, what, "position north", lambda v: True, "must be finite")
    cu = _finite_number(height, what, "height", lambda v: True, "must be finite")
    yaw = _finite_number(yaw_deg, what, "yaw_deg", lambda v: True, "must be finite")
    M = _level(yaw)
    if rotation is not None:
        M = _check_rotation(rotation, what, max_tilt_deg) @ M
    return np.concatenate([[ce, cn, cu], M.reshape(9)]).astype(_F)


def _check_pose(pose, what: str) -> np.ndarray:
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    try:
        p = np.asarray(pose, dtype=_F)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: pose is not an array of numbers") from None
    if p.shape != (12,) or not np.isfinite(p).all():
        raise ValueError(f"{what}: pose of shape {p.shape}: expected the 12 finite numbers camera_pose() returned (east, north, height, M row-major)")
    return np.ascontiguousarray(p)


def _pose_yaw(pose: np.ndarray) -> float:
    """The heading of the picture's up direction, degrees clockwise from north: of -M[1, :], the camera's up in the world."""
    return math.degrees(math.atan2(-pose[6], -pose[7]))


# ---- the rule, in numpy ---------------------------------------------------------------------------------------------------

def _source_positions(cam: np.ndarray, pose: np.ndarray, z32: np.ndarray, e0: float, n0: float, dcell: float, E, N):
    """The rule from the ground position on: (u, v, not outside before the frame test, has a finite height) of ground
    positions (E, N), operation for operation."""
    ce, cn, cu, m0, m1, m2, m3, m4, m5, m6, m7, m8 = (_F(v) for v in pose)
    z, has = _height(z32, e0, n0, dcell, E, N)
    dE, dN, dU = E - ce, N - cn, z - cu
    X = (m0 * dE + m1 * dN) + m2 * dU
    Y = (m3 * dE + m4 * dN) + m5 * dU
    Z = (m6 * dE + m7 * dN) + m8 * dU
    xd, yd = _distort(cam, X / Z, Y / Z)
    return cam[0] * xd + (cam[2] + _F(0.5)), cam[1] * yd + (cam[3] + _F(0.5)), has & (Z > 0), has & np.isfinite(z)


def _pixel_ground(georef: np.ndarray, px, py):
    """The rule's ground position of the picture positions (px, py)."""
    g = georef.reshape(6)
    return (g[0] * px + g[1] * py) + g[2], (g[3] * px + g[4] * py) + g[5]


def _to_ground(cam: np.ndarray, pose: np.ndarray, d: Dict[str, object], p: np.ndarray) -> np.ndarray:
    """Raw positions -> ground (E, N): lens inverse (Newton), M.T, then the ray is intersected with the DEM by fixed-point
    iteration from the height below the camera."""
    z32, (e0, n0), dcell = d["heights"], d["origin"], d["cell"]
    C, M = pose[:3], pose[3:].reshape(3, 3)
    with np.errstate(all="ignore"):
        xn, yn = _undistort(cam, (p[:, 0] - (cam[2] + _F(0.5))) / cam[0], (p[:, 1] - (cam[3] + _F(0.5))) / cam[1], float(max(cam[0], cam[1])))
        dE = M[0, 0] * xn + M[1, 0] * yn + M[2, 0]
        dN = M[0, 1] * xn + M[1, 1] * yn + M[2, 1]
        dU = M[0, 2] * xn + M[1, 2] * yn + M[2, 2]
        z = np.broadcast_to(_height(z32, e0, n0, dcell, np.array([C[0]]), np.array([C[1]]))[0], xn.shape).copy()
        E, N = np.full_like(xn, np.nan), np.full_like(xn, np.nan)
        done = np.zeros(xn.shape, dtype=bool)
        for _ in range(TERRAIN_STEPS):
            t = (z - C[2]) / dU
            En, Nn = C[0] + t * dE, C[1] + t * dN
            E, N = np.where(done, E, En), np.where(done, N, Nn)
            z_next = _height(z32, e0, n0, dcell, E, N)[0]
            done |= np.abs(z_next - z) <= TERRAIN_TOL_M               # a NaN never converges
            z = np.where(done, z, z_next)
            if done.all():
                break
    out = np.stack([E, N], axis=1)
    out[~(done & (dU < 0))] = np.nan
    return out


# ---- the plan -------------------------------------------------------------------------------------------------------------

def _posts_finite(z32: np.ndarray, e0: float, n0: float, dcell: float, georef: np.ndarray, oh: int, ow: int) -> bool:
    """Every post that can take part in a height under the oh x ow picture is finite: those of the DEM cells its corners span."""
    E, N = _pixel_ground(georef, np.array([0.0, ow, 0.0, ow]), np.array([0.0, 0.0, oh, oh]))
    a, b = (E - e0) / dcell - 0.5, (n0 - N) / dcell - 0.5
    dh, dw = z32.shape
    a0, a1 = int(np.clip(np.floor(a.min()), 0, dw - 1)), int(np.clip(np.floor(a.max()) + 1, 0, dw - 1))
    b0, b1 = int(np.clip(np.floor(b.min()), 0, dh - 1)), int(np.clip(np.floor(b.max()) + 1, 0, dh - 1))
    return bool(np.isfinite(z32[b0:b1 + 1, a0:a1 + 1]).all())


def ortho_plan(camera, size, pose, dem, cell=None, yaw_deg=None, keep: str = "valid", out_size=None, centre=None) -> Dict[str, object]:
    """The output grid for orthorectifying a frame of `size` = (height, width) taken with `camera` (lens.py's nine numbers) at
    `pose` (camera_pose) over `dem` (terrain_grid).  The orthophoto's georeference is nadir_affine(oh, ow, centre, cell,
    yaw_out): centre defaults to the ground point below the camera, (Ce, Cn); yaw_out = yaw_deg defaults to the pose's own
    yaw, a track-aligned grid (a north-up box around a frame flown at 45 degrees is half fill); cell, metres per pixel,
    defaults to (Cu - terrain_height(centre)) / fx, the frame's own resolution on the ground below it.
    keep='valid': the largest centred picture with no filled pixel, decided by the rule's own inside test on the candidate's
    border pixels, and every post under it finite; keep='all': the smallest centred picture that holds the ground position of
    every border pixel centre of the frame; out_size=(oh, ow): the caller's own.  Returns plain data: {'camera', 'size',
    'out_size', 'pose', 'georef' (2, 3), 'cell', 'yaw_deg', 'dem_origin', 'dem_cell', 'dem_size'} -- the DEM's geometry, not its
    posts -- what ortho_u8, orthorectified and terrain_points take.  Host only, numpy float64.
    ValueError: malformed arguments; a camera at or below the terrain under it; a DEM that does not cover centre; an empty
    valid picture; a border pixel of the frame whose ray does not meet the DEM (keep='all'); a picture beyond 65536 a side."""
    what = "ortho_plan"
    cam = _check_camera(camera, what)
    h, w = _check_size(size, what, "size")
    ps = _check_pose(pose, what)
    d = _check_dem(dem, what)
    z32, (e0, n0), dcell = d["heights"], d["origin"], d["cell"]
    if not isinstance(keep, str) or keep not in LENS_KEEP:
        raise ValueError(f"{what}: keep {keep!r} must be 'valid' or 'all'")
    if centre is None:
        ce, cn = float(ps[0]), float(ps[1])
    else:
        try:
            ce, cn = centre
        except (TypeError, ValueError):
            raise ValueError(f"{what}: centre {centre!r}: expected (east, north)") from None
        ce = _finite_number(ce, what, "centre east", lambda v: True, "must be finite")
        cn = _finite_number(cn, what, "centre north", lambda v: True, "must be finite")
    with np.errstate(all="ignore"):
        z_c, z_cam = (float(v) for v in _height(z32, e0, n0, dcell, np.array([ce, ps[0]]), np.array([cn, ps[1]]))[0])
    if not math.isfinite(z_c):
        raise ValueError(f"{what}: the DEM does not cover centre ({ce!r}, {cn!r}): it has no finite height there")
    if ps[2] <= z_cam or ps[2] <= z_c:
        raise ValueError(f"{what}: the camera's height {float(ps[2])!r} is at or below the terrain under it ({max(z_cam, z_c)!r}): the pose's "
                         "height must be in the DEM's own vertical datum")
    gsd = (float(ps[2]) - z_c) / float(cam[0]) if cell is None else _finite_number(cell, what, "cell", lambda v: v > 0.0, "must be finite and > 0")
    yaw = _pose_yaw(ps) if yaw_deg is None else _finite_number(yaw_deg, what, "yaw_deg", lambda v: True, "must be finite")
    georef = lambda oh, ow: nadir_affine(oh, ow, (ce, cn), gsd, yaw)

    def none_filled(oh: int, ow: int) -> bool:
        if oh > LENS_MAX_SIDE or ow > LENS_MAX_SIDE:
            return False
        g = georef(oh, ow)
        j, i = _border(oh, ow)
        with np.errstate(all="ignore"):
            u, v, front, _ = _source_positions(cam, ps, z32, e0, n0, dcell, *_pixel_ground(g, i.astype(_F) + _F(0.5), j.astype(_F) + _F(0.5)))
            return bool((front & (0 <= u) & (u < w) & (0 <= v) & (v < h)).all()) and _posts_finite(z32, e0, n0, dcell, g, oh, ow)

    if out_size is not None:
        oh, ow = _check_size(out_size, what, "out_size")
    elif keep == "valid":
        if not none_filled(1, 1):
            raise ValueError(f"{what}: keep='valid' is empty: the frame does not see the ground at centre ({ce!r}, {cn!r}), so the picture's "
                             "centre pixel would already be filled")
        oh, ow = _grow_valid(none_filled, h, w)
    else:
        j, i = _border(h, w)
        ground = _to_ground(cam, ps, d, np.stack([i + 0.5, j + 0.5], axis=1))
        if not np.isfinite(ground).all():
            k = int(np.nonzero(~np.isfinite(ground).all(axis=1))[0][0])
            raise ValueError(f"{what}: the border pixel (row {int(j[k])}, column {int(i[k])}) of the frame has no ground position: its ray "
                             "leaves the DEM or does not meet it (or the lens model folds over inside the frame)")
        L = _level(yaw)
        off = (ground - np.array([ce, cn])) / gsd
        try:
            oh, ow = _size_that_holds(L[0, 0] * off[:, 0] + L[0, 1] * off[:, 1], L[1, 0] * off[:, 0] + L[1, 1] * off[:, 1], what)
        except ValueError:
            raise ValueError(f"{what}: keep='all' at cell {gsd!r} needs more than {LENS_MAX_SIDE} pixels a side: pass a larger cell") from None
    return {"camera": cam, "size": (h, w), "out_size": (oh, ow), "pose": ps, "georef": georef(oh, ow), "cell": gsd, "yaw_deg": yaw,
            "dem_origin": (e0, n0), "dem_cell": dcell, "dem_size": tuple(z32.shape)}


def _check_ortho_plan(plan, dem, what: str):
    """(plan, dem), both validated again; the DEM must be the one the plan was made over."""
    if not isinstance(plan, dict) or any(k not in plan for k in ("camera", "size", "out_size", "pose", "georef", "dem_origin", "dem_cell", "dem_size")):
        raise ValueError(f"{what}: plan must be the dict ortho_plan() returned (camera, size, out_size, pose, georef, cell, and the DEM's geometry)")
    d = _check_dem(dem, what)
    try:
        g = np.ascontiguousarray(np.asarray(plan["georef"], dtype=_F))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: plan georef is not an array of numbers") from None
    if g.shape != (2, 3) or not np.isfinite(g).all():
        raise ValueError(f"{what}: plan georef of shape {g.shape}: expected a finite (2, 3) pixel-to-ground affine")
    if tuple(plan["dem_size"]) != d["heights"].shape or tuple(plan["dem_origin"]) != d["origin"] or plan["dem_cell"] != d["cell"]:
        raise ValueError(f"{what}: the plan was made over a DEM of {tuple(plan['dem_size'])} posts at {tuple(plan['dem_origin'])}, spacing "
                         f"{plan['dem_cell']!r}; this one has {d['heights'].shape} at {d['origin']}, spacing {d['cell']!r}")
    pl = {"camera": _check_camera(plan["camera"], what), "size": _check_size(plan["size"], what, "size"),
          "out_size": _check_size(plan["out_size"], what, "out_size"), "pose": _check_pose(plan["pose"], what), "georef": g}
    return pl, d


def terrain_points(plan, dem, pts, to: str = "ground") -> np.ndarray:
    """(n, 2) positions between the raw frame, the ground and the plan's orthophoto.  Host only.
    to='ground': raw-frame pixel positions -> ground (east, north), for detections made on raw frames: lens._undistort's
    Newton iteration, M.T, then the ray C + t d is intersected with the DEM by fixed-point iteration -- z_0 the height below
    the camera, t = (z_k - Cu) / d_U, (E, N) = C + t d, z_{k+1} = terrain_height(E, N), until |z_{k+1} - z_k| <= 1e-9 m, at
    most 64 steps.  The iteration contracts where the terrain's slope times the tangent of the ray's off-nadir angle is below
    1 (a ray less steep than the slope it meets may not converge, or may meet the ground twice).  NaN where the lens inverse
    is NaN, where the ray does not look down (d_U >= 0), where it leaves the grid, and where 64 steps do not converge.  M is
    taken for orthonormal, as camera_pose makes it.
    to='raw': ground (east, north) -> the raw frame, the rule in closed form -- for an output pixel centre pushed through
    plan['georef'] exactly the position the kernel samples; NaN where the point has no height or lies behind the camera.
    to='picture': ground -> orthophoto pixel positions, through ground_to_pixel(plan['georef'])."""
    what = "terrain_points"
    pl, d = _check_ortho_plan(plan, dem, what)
    p = _check_points(pts, what)
    if not isinstance(to, str) or to not in ("ground", "raw", "picture"):
        raise ValueError(f"{what}: to {to!r} must be 'ground', 'raw' or 'picture'")
    if to == "ground":
        return _to_ground(pl["camera"], pl["pose"], d, p)
    if to == "picture":
        b = ground_to_pixel(pl["georef"])
        return np.stack([(b[0, 0] * p[:, 0] + b[0, 1] * p[:, 1]) + b[0, 2], (b[1, 0] * p[:, 0] + b[1, 1] * p[:, 1]) + b[1, 2]], axis=1)
    with np.errstate(all="ignore"):
        u, v, front, _ = _source_positions(pl["camera"], pl["pose"], d["heights"], *d["origin"], d["cell"], p[:, 0], p[:, 1])
    out = np.stack([u, v], axis=1)
    out[~front] = np.nan
    return out


class orthorectified(undistorted):
    """The frames of a survey, orthorectified: the lazy sequence lens.undistorted is -- o[i] indexes frames[i] once, never
    before, and returns the device frame preprocess.ortho_u8(frames[i], o.plans[i], dem, sample, fill); nothing is kept -- with
    one plan per frame, because every frame has its own pose.  poses: (n, 12), camera_pose's; camera, dem, cell, yaw_deg, keep,
    out_size and centre as in ortho_plan, the same for every frame (centre=None: each frame's own nadir point).
    size=(height, width), by keyword, is the size every frame must have: the plans are made before any frame is indexed.
    o.plans is the list of plans, o.sizes the (n, 2) int64 (oh, ow) of every frame, and o.georef the (n, 2, 3) float64
    georeferences of the orthophotos: detect_frames(model, o), census(results, o.georef, radius), coverage, mosaic(o, o.georef,
    cell, sizes=o.sizes), register(...) and refine(...) take them as they are.  The DEM's posts are uploaded once, when the
    first frame is indexed."""

    def __init__(self, frames, camera, poses, dem, cell=None, yaw_deg=None, keep: str = "valid", out_size=None, centre=None,
                 sample: str = "bilinear", fill=(0, 0, 0), *, size):
        self._take(frames, sample, fill)
        if isinstance(poses, torch.Tensor):
            poses = poses.detach().cpu().numpy()
        try:
            p = np.asarray(poses, dtype=_F)
        except (TypeError, ValueError):
            raise ValueError("orthorectified: poses is not an array of numbers") from None
        n = len(frames)
        if p.shape != (n, 12):
            raise ValueError(f"orthorectified: poses of shape {p.shape} for {n} frames: expected ({n}, 12), camera_pose() of every frame")
        _check_dem(dem, "orthorectified")
        self.dem = dem
        self.plans = [ortho_plan(camera, size, p[k], dem, cell, yaw_deg, keep, out_size, centre) for k in range(n)]
        self.sizes = np.array([pl["out_size"] for pl in self.plans], dtype=np.int64).reshape(-1, 2)
        self.georef = np.array([pl["georef"] for pl in self.plans], dtype=_F).reshape(-1, 2, 3)

    def _resample(self, frame, i: int):
        from . import preprocess
        return preprocess.ortho_u8(frame, self.plans[i], self.dem, self.sample, self.fill)
