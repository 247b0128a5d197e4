"""What tests/test_register_pyramid.py and tools/register_time.py share: the restatement of the pyramid's rule (include/wm_hip.h
"Survey registration, pyramid"), the planes the device tests reduce, the far-off analytic scene and the coarse-to-fine loop of
tiling.refine(levels=L) with the oracles' planes and sums in the device's place.  Nothing here asserts about a device."""
import numpy as np
import torch

from register_cases import F64, SUMS, _oracle_sums, refine_sums_oracle, render_plane
from survey_util import DEV, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

# The analytic scene of tests/test_register_refine.py, restated (no test or tool imports a test module: test_survey_checkers.py):
# four yawed frames about 40 m apart over a ground of sinusoids, gsd 0.5 m, cell 1 m, patches of 128 cells.
FRAME_H, FRAME_W, GSD, CELL, SIDE = 320, 400, 0.5, 1.0, 128
YAWS = (10.0, -20.0, 170.0, 95.0)
CENTRES = ((1000.3, 2000.7), (1039.1, 2006.4), (1007.8, 2041.2), (1044.6, 2043.9))
SIZES = [(FRAME_H, FRAME_W)] * 4
NEAR = ((0.0, 0.0, 0.0, 0.0), (0.4, -0.3, 0.5, -0.004), (-0.3, 0.4, -0.4, 0.003), (0.35, 0.4, 0.3, 0.004))   # that file's PERTURB


def _scene_value(X, Y):
    """24 sinusoids of wave numbers drawn with sigma 0.08 rad/m, at continuous ground coordinates: within about [70, 190]."""
    rng = np.random.default_rng(24)
    k = rng.normal(0.0, 0.08, size=(24, 2))
    ph = rng.uniform(0, 2 * np.pi, size=24)
    amp = rng.uniform(0.5, 1.0, size=24)
    v = np.zeros_like(X)
    for (kx, ky), p, a in zip(k, ph, amp):
        v += a * np.sin(kx * (X - 1000.0) + ky * (Y - 2000.0) + p)
    return 130.0 + v * (60.0 / amp.sum() * 2.2)


def _corner_error(g, true):
    """The worst ground distance, over every frame's corners, between the georeference g and the true one: metres."""
    corners = np.array([[0, 0, 1], [FRAME_W, 0, 1], [0, FRAME_H, 1], [FRAME_W, FRAME_H, 1]], dtype=F64)
    return float(np.linalg.norm(np.einsum("fij,cj->fci", g - true, corners), axis=2).max())


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


# ---- the far-off scene: test_register_refine's frames with fine texture, georeferences off by metres, degrees and percents ---

FAR = ((0.0, 0.0, 0.0, 0.0), (3.2, -2.4, 2.5, -0.015), (-2.6, 3.1, -2.0, 0.012), (2.8, 3.0, 1.5, 0.015))    # east m, north m, yaw deg, scale
_FAR = []


def _fine_value(X, Y):
    """A second bank of 24 sinusoids, wave numbers drawn with sigma 0.9 rad/m: texture a coarse point-sampled cell aliases."""
    rng = np.random.default_rng(7)
    k = rng.normal(0, 0.9, (24, 2))
    ph = rng.uniform(0, 2 * np.pi, 24)
    v = np.zeros_like(X)
    for (kx, ky), p in zip(k, ph):
        v += np.sin(kx * (X - 1000.0) + ky * (Y - 2000.0) + p)
    return v


def _perturbed(true, f, errors):
    """The georeference of frame f with errors[f] = (east m, north m, yaw degrees, scale): a similarity about the frame
    centre's ground position, then a shift."""
    dx, dy, yaw, sc = errors[f]
    c = true[f] @ np.array([FRAME_W / 2, FRAME_H / 2, 1.0])
    th = np.radians(yaw)
    M = (1.0 + sc) * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    g = np.empty((2, 3))
    g[:, :2] = M @ true[f][:, :2]
    g[:, 2] = M @ (true[f][:, 2] - c) + c + np.array([dx, dy])
    return g


def _frames_of(value):
    """The four frames (grey, so the luma is the value) of the ground value(X, Y), and their true georeferences."""
    true = np.stack([tiling.nadir_affine(FRAME_H, FRAME_W, c, GSD, yaw) for c, yaw in zip(CENTRES, YAWS)])
    vv, uu = np.meshgrid(np.arange(FRAME_H) + 0.5, np.arange(FRAME_W) + 0.5, indexing="ij")
    frames = []
    for g in true:
        pix = lambda r: r[0] * uu + r[1] * vv + r[2]                                  # a ground coordinate of every pixel centre
        val = np.rint(value(pix(g[0]), pix(g[1])))
        frames.append(np.repeat(np.clip(val, 2, 254).astype(np.uint8)[:, :, None], 3, axis=2))
    return frames, true


def far_scene():
    """frames, the true georeferences and the far-off ones: the smooth scene at 0.7 of its contrast plus the fine texture.
    Built once."""
    if not _FAR:
        frames, true = _frames_of(lambda X, Y: 128.0 + 0.7 * (_scene_value(X, Y) - 130.0) + _fine_value(X, Y) * 25.0 / np.sqrt(12.0))
        _FAR.append((frames, true, np.stack([_perturbed(true, f, FAR) for f in range(4)])))
    return _FAR[0]


_NEAR = []


def near_scene():
    """The smooth scene alone with the small errors NEAR: what test_register_refine.py calls _analytic().  Built once."""
    if not _NEAR:
        frames, true = _frames_of(_scene_value)
        _NEAR.append((frames, true, np.stack([_perturbed(true, f, NEAR) for f in range(4)])))
    return _NEAR[0]


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


def pyramid_loop(levels, iters, exposure=False, table=None, key=None, min_cells=4096):
    """tiling.refine(levels=, iters=, fixed=[0])'s loop on the far-off scene with the oracles in the device's place.  Computed
    once per key.  'steps' holds refine_step's result of every iteration, 'levels' its level, 'errors' the worst corner error
    after it."""
    key = (levels, iters, exposure) if key is None else key
    if key not in _LOOPS:
        frames, true, pert = far_scene()
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
    """The documented workaround as a record: the plain loop at a coarser, point-sampled cell (side and min_cells scaled with it)."""
    frames, true, pert = far_scene()
    k = int(round(cell / CELL))
    side, min_cells = SIDE // k, max(1, 4096 // (k * k))
    table = tiling.register_pairs(pert, SIZES, cell, 1, side, min_cells)
    cur, errors = pert, []
    for _ in range(iters):
        cur = tiling.refine_step(cur, SIZES, table, _oracle_sums(frames, cur, SIZES, table, cell, side), cell, False, min_cells, 2.0, [0])["georef"]
        errors.append(_corner_error(cur, true))
    return errors
