"""What the registration tests (tests/test_register.py, test_register_zncc.py, test_register_refine.py, test_register_pyramid.py)
and tools/register_time.py share: the sequential oracles of the registration rules (render, search and pick; the correlation
search; the refinement's sums -- include/wm_hip.h "Survey registration" and the two sections after it), the cases the files
build, the thin calls of the C-ABI entry points, the end-to-end scene of the search and the analytic scene of the refinement
and the pyramid (near, near with exposure changes, far off).  The ground rule of render_plane is ground_oracle.py's.  Nothing
here asserts about a device."""
import numpy as np
import torch

from ground_oracle import inside, uv
from survey_util import DEV, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling
from wildlifemapper_amd._survey import _frame_descs

F64 = np.float64
NAN = float("nan")
INF = float("inf")
POISON_A, POISON_B = 0xA5, 0x5A


def luma(px):
    """max(1, (77 R + 150 G + 29 B + 128) >> 8) of (..., 3) uint8 pixels, in int64."""
    p = np.asarray(px).astype(np.int64)
    return np.maximum(1, (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8)


def render_plane(b6, hw, img, x0, y0, cell, nx, ny, s, ext):
    """One plane of the rule, ext x ext uint8: cell (j, i) has centre x0 + ((i - s) + 0.5) * cell; cells with i >= nx + 2 s
    or j >= ny + 2 s are 0; a cell its frame does not see is 0; else the luma of the nearest pixel."""
    h, w = int(hw[0]), int(hw[1])
    b = np.asarray(b6, dtype=F64).reshape(6)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    idx = np.arange(ext, dtype=np.int64)
    with np.errstate(all="ignore"):
        Xc = (x0 + ((idx - s).astype(F64) + F64(0.5)) * cell)[None, :]
        Yc = (y0 + ((idx - s).astype(F64) + F64(0.5)) * cell)[:, None]
        u, v = uv(b, Xc, Yc)
        sees = inside(u, v, h, w)
    sees = sees & (idx[None, :] < nx + 2 * s) & (idx[:, None] < ny + 2 * s)
    out = np.zeros((ext, ext), dtype=np.uint8)
    if sees.any():
        out[sees] = luma(img[np.floor(v[sees]).astype(np.int64), np.floor(u[sees]).astype(np.int64)]).astype(np.uint8)
    return out


def search_oracle(A, B, gx, gy, S):
    """score (2S+1, 2S+1, 2) int64 = (sad, n), one offset at a time."""
    a = A[:gy, :gx].astype(np.int64)
    score = np.zeros((2 * S + 1, 2 * S + 1, 2), dtype=np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            bb = B[S + dy:S + dy + gy, S + dx:S + dx + gx].astype(np.int64)
            both = (a != 0) & (bb != 0)
            score[dy + S, dx + S] = (np.abs(a - bb)[both].sum(), both.sum())
    return score


def beats(p, q):
    """Offset p = (sad, n, dy, dx) beats q: the cross products in Python integers, then (dy^2 + dx^2, dy, dx)."""
    l, r = p[0] * q[1], q[0] * p[1]
    if l != r:
        return l < r
    return (p[2] * p[2] + p[3] * p[3], p[2], p[3]) < (q[2] * q[2] + q[3] * q[3], q[2], q[3])


def pick_two(S, candidate, beats):
    """The pick of both searches, sequentially: the best offset, then the best outside its 3 x 3 (None where there is none).
    candidate(dy, dx) is the offset's (score, n, dy, dx) or None; beats(p, q) the metric's order."""
    def top(excluded):
        best = None
        for dy in range(-S, S + 1):
            for dx in range(-S, S + 1):
                if excluded is not None and max(abs(dy - excluded[2]), abs(dx - excluded[3])) < 2:
                    continue
                cand = candidate(dy, dx)
                if cand is not None and (best is None or beats(cand, best)):
                    best = cand
        return best
    first = top(None)
    return first, (top(first) if first is not None else None)


def pick_oracle(score, S, min_cells):
    """best (8,) int64 from a score table, sequentially."""
    def candidate(dy, dx):
        sad, n = (int(v) for v in score[dy + S, dx + S])
        return (sad, n, dy, dx) if n >= min_cells else None
    first, second = pick_two(S, candidate, beats)
    four = lambda c: [0, 0, -1, 0] if c is None else [c[2], c[3], c[0], c[1]]
    return np.array(four(first) + four(second), dtype=np.int64)


# ---- the correlation search: six moments per offset, the score in three float64 operations ----------------------------------

def zncc_search_oracle(A, B, gx, gy, S):
    """moments (2S+1, 2S+1, 6) int64 = (n, Sa, Sb, Saa, Sbb, Sab) over the cells both planes see, one offset at a time."""
    a = A[:gy, :gx].astype(np.int64)
    out = np.zeros((2 * S + 1, 2 * S + 1, 6), dtype=np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            bb = B[S + dy:S + dy + gy, S + dx:S + dx + gx].astype(np.int64)
            both = (a != 0) & (bb != 0)
            x, y = a[both], bb[both]
            out[dy + S, dx + S] = (both.sum(), x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum())
    return out


def zncc_q(m):
    """The score of one offset from its six moments, or None where a plane is flat: c, va, vb in Python integers, then
    q = (c * |c|) / (va * vb) in three float64 operations."""
    n, sa, sb, saa, sbb, sab = (int(v) for v in m)
    c, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    if va <= 0 or vb <= 0:
        return None
    assert max(abs(c), va, vb, n * sab, sa * sb, n * saa, n * sbb) < 2 ** 53           # the conversions are exact
    cf = F64(c)
    return (cf * np.abs(cf)) / (F64(va) * F64(vb))


def zncc_beats(p, q):
    """Offset p = (q, n, dy, dx) beats q: the larger score, then the smaller (dy^2 + dx^2, dy, dx)."""
    if p[0] != q[0]:
        return p[0] > q[0]
    return (p[2] * p[2] + p[3] * p[3], p[2], p[3]) < (q[2] * q[2] + q[3] * q[3], q[2], q[3])


def zncc_pick_oracle(moments, S, min_cells):
    """(best (8,) int64, peak (2,) float64) from a moments table, sequentially."""
    def candidate(dy, dx):
        m = moments[dy + S, dx + S]
        q = zncc_q(m) if int(m[0]) >= min_cells else None
        return None if q is None else (q, int(m[0]), dy, dx)
    first, second = pick_two(S, candidate, zncc_beats)
    four = lambda c: [0, 0, 0, 0] if c is None else [c[2], c[3], 1, c[1]]
    peak = np.array([NAN if c is None else c[0] for c in (first, second)], dtype=F64)
    return np.array(four(first) + four(second), dtype=np.int64), peak


def same_bytes(got, want):
    return np.ascontiguousarray(got, dtype=F64).tobytes() == np.ascontiguousarray(want, dtype=F64).tobytes()


# ---- refinement: the 28 integer sums of one Gauss-Newton step per pair ---------------------------------------------------

SUMS = 28
TRI = [(k, l) for k in range(6) for l in range(k, 6)]


def refine_sums_oracle(A, B, gx, gy, search):
    """The 28 sums of one pair as a list of Python integers.  A (side, side), B (side + 2 search, side + 2 search) uint8."""
    S = search
    a = A[:gy, :gx].astype(np.int64)
    sl = lambda dj, di: B[S + dj:S + dj + gy, S + di:S + di + gx].astype(np.int64)
    b, e, w, nn, ss = sl(0, 0), sl(0, 1), sl(0, -1), sl(1, 0), sl(-1, 0)
    counts = (a != 0) & (b != 0) & (e != 0) & (w != 0) & (nn != 0) & (ss != 0)
    r, gxv, gyv = a - b, e - w, nn - ss
    x = (2 * np.arange(gx, dtype=np.int64) + 1 - gx)[None, :] + np.zeros((gy, 1), dtype=np.int64)
    y = (2 * np.arange(gy, dtype=np.int64) + 1 - gy)[:, None] + np.zeros((1, gx), dtype=np.int64)
    c = [gxv, gyv, x * gyv - y * gxv, x * gxv + y * gyv, b, np.ones_like(b)]
    total = lambda v: int(v[counts].astype(object).sum()) if counts.any() else 0       # Python integers
    return [total(c[k] * c[l]) for k, l in TRI] + [total(c[k] * r) for k in range(6)] + [total(r * r)]


def _oracle_sums(frames, georef, sizes, table, cell, side, search=1):
    g2p = tiling.ground_to_pixel(georef).reshape(-1, 6)
    out = []
    for pr in table:
        fa, fb, gx, gy = (int(pr[k]) for k in ("frame_a", "frame_b", "gx", "gy"))
        A = render_plane(g2p[fa], sizes[fa], frames[fa], pr["x0"], pr["y0"], cell, gx, gy, 0, side)
        B = render_plane(g2p[fb], sizes[fb], frames[fb], pr["x0"], pr["y0"], cell, gx, gy, search, side + 2 * search)
        out.append(refine_sums_oracle(A, B, gx, gy, search))
    return np.array(out, dtype=np.int64).reshape(len(table), SUMS)


# ---- the whole rule for a pair table -------------------------------------------------------------------------------------

def register_oracle(g2p, size, images, pairs, cell, search, side, min_cells):
    """The whole rule for a pair table: A (P,side,side), B (P,E,E) uint8, score (P,2S+1,2S+1,2) and best (P,8) int64.  A
    pair outside the rule (a frame index out of range, gx or gy outside [1, side]) has no planes here (None)."""
    E = side + 2 * search
    out = {"a": [], "b": [], "score": [], "best": []}
    nf = len(size)
    for pr in pairs:
        fa, fb, gx, gy = (int(pr[k]) for k in ("frame_a", "frame_b", "gx", "gy"))
        if not (0 <= fa < nf and 0 <= fb < nf and 1 <= gx <= side and 1 <= gy <= side):
            for k in out:
                out[k].append(None)
            continue
        A = render_plane(g2p[fa], size[fa], images[fa], pr["x0"], pr["y0"], cell, gx, gy, 0, side)
        B = render_plane(g2p[fb], size[fb], images[fb], pr["x0"], pr["y0"], cell, gx, gy, search, E)
        score = search_oracle(A, B, gx, gy, search)
        out["a"].append(A)
        out["b"].append(B)
        out["score"].append(score)
        out["best"].append(pick_oracle(score, search, min_cells))
    return out


def _pairs(rows):
    return np.array([tuple(r) for r in rows], dtype=tiling.REGISTER_PAIR).reshape(-1)


def _axis_frame(img, x_west, y_north, gsd):
    """A north-up frame: pixel (0, 0)'s corner at (x_west, y_north), gsd metres per pixel.  Returns (img, georef)."""
    return img, np.array([[gsd, 0.0, x_west], [0.0, -gsd, y_north]], dtype=F64)


def _content(h, w, seed, lo=0):
    return np.random.default_rng(seed).integers(lo, 256, size=(h, w, 3), dtype=np.uint8)


HAND_A = np.array([[1, 2], [3, 4]], dtype=np.uint8)
HAND_B = np.array([[0, 0, 0, 0], [0, 1, 2, 0], [0, 3, 4, 0], [0, 0, 0, 0]], dtype=np.uint8)


def _north_up(x_west, y_south, w, h, gsd=1.0):
    return np.array([[gsd, 0.0, x_west], [0.0, -gsd, y_south + h * gsd]], dtype=F64)


def _case(frames, pairs, cell, search, side, min_cells):
    """frames: a list of (img (H,W,3) uint8, georef (2,3)); pairs: rows of (frame_a, frame_b, gx, gy, x0, y0)."""
    georef = np.stack([f[1] for f in frames])
    return {"images": [f[0] for f in frames], "g2p": tiling.ground_to_pixel(georef).reshape(-1, 6),
            "size": np.array([f[0].shape[:2] for f in frames], dtype=np.int32), "pairs": _pairs(pairs), "cell": cell, "search": search,
            "side": side, "min_cells": min_cells}


def _oracle(case):
    return register_oracle(case["g2p"], case["size"], case["images"], case["pairs"], case["cell"], case["search"], case["side"],
                           case["min_cells"])


def _cover(gx, gy, search, x0, y0, cell, seed, gsd_cells=1.5, yaw=0.0, margin=2):
    """A frame of random pixels that sees the whole patch and its search margin: gsd = gsd_cells * cell."""
    gsd = gsd_cells * cell
    span = max(gx, gy) + 2 * search + 2 * margin
    n = int(np.ceil(span / gsd_cells * (1.5 if yaw else 1.0))) + 2
    centre = (x0 + 0.5 * gx * cell, y0 + 0.5 * gy * cell)
    return _content(n, n + 1, seed), tiling.nadir_affine(n, n + 1, centre, gsd, yaw)


def _shape_case(gx, gy, search, side, seed=0, min_cells=1):
    x0, y0, cell = 500000.0 + 0.25 * seed, 6000000.0 - 0.5 * seed, 0.25
    fa = _cover(gx, gy, search, x0, y0, cell, 2 * seed)
    fb = _cover(gx, gy, search, x0, y0, cell, 2 * seed + 1, gsd_cells=1.25)
    return _case([fa, fb], [(0, 1, gx, gy, x0, y0)], cell, search, side, min_cells)


SHAPES = {  # gx, gy, search, side
    "1x1_s0": (1, 1, 0, 1), "1x1_s1_side4": (1, 1, 1, 4), "3x5_s1": (3, 5, 1, 8), "4x4_s5": (4, 4, 5, 4), "5x3_s5": (5, 3, 5, 16),
    "63x65_s5": (63, 65, 5, 65), "64x64_s1": (64, 64, 1, 64), "65x63_s5": (65, 63, 5, 80), "1x65_s5": (1, 65, 5, 65),
    "64x1_s0": (64, 1, 0, 64), "70x19_s5": (70, 19, 5, 70), "257x65_s5": (257, 65, 5, 300), "96x80_s64": (96, 80, 64, 96),
    "512x512_s4": (512, 512, 4, 512), "65x33_s16": (65, 33, 16, 67), "40x40_s33": (40, 40, 33, 41),
    "33x37_s62": (33, 37, 62, 40), "33x37_s63": (33, 37, 63, 40)}             # the last search with 32-row tiles, the first with 16


def _several_pairs():
    """Pairs of different sizes in one launch, sharing frames, patches at different places, one yawed 45 degrees."""
    x0, y0, cell = 1000.0, 2000.0, 0.5
    diamond = _content(90, 90, 13), tiling.nadir_affine(90, 90, (x0 + 17.5, y0 + 17.5), 0.5, 45.0)       # 45 m a side, yawed
    frames = [_cover(70, 70, 6, x0, y0, cell, 11), _cover(70, 70, 6, x0, y0, cell, 12, gsd_cells=1.25), diamond,
              _cover(30, 30, 6, x0 + 10.0, y0 + 10.0, cell, 14, gsd_cells=0.75)]
    pairs = [(0, 1, 70, 19, x0, y0), (1, 2, 5, 66, x0 + 3.0, y0 + 1.5), (0, 3, 33, 30, x0 + 9.5, y0 + 8.0), (2, 3, 72, 72, x0 - 4.0, y0 - 4.0),
             (0, 2, 1, 1, x0 + 7.0, y0 + 7.0)]
    return _case(frames, pairs, cell, 6, 72, 40)


def _planes(case):
    n, side, E = len(case["pairs"]), case["side"], case["side"] + 2 * case["search"]
    return (torch.full((n, side, side), POISON_A, device=DEV, dtype=torch.uint8), torch.full((n, E, E), POISON_B, device=DEV, dtype=torch.uint8))


def _render(case, a, b, status, resident, slot=None, images=None):
    """One wm_register_render_u8 call with the frames `resident` (survey indices) on the device, in that order."""
    F = case["g2p"].shape[0]
    images = case["images"] if images is None else images
    tensors = [_up(images[f]) for f in resident]
    descs = _frame_descs(tensors, torch.device(DEV)) if tensors else None
    if slot is None:
        slot = np.full(F, -1, dtype=np.int32)
        slot[list(resident)] = np.arange(len(resident), dtype=np.int32)
    pairs = _up(case["pairs"].view(np.uint8).reshape(len(case["pairs"]), 32))
    slot_d, g_d, s_d = _up(slot), _up(case["g2p"]), _up(case["size"])                # held until the launch has run
    N.check(N.lib().wm_register_render_u8(N.ptr(descs), len(resident), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F,
                                          N.ptr(pairs), len(case["pairs"]), case["cell"], case["search"], case["side"], N.ptr(a), N.ptr(b),
                                          N.ptr(status), N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()


def device_search(metric, a, b, table, S, side, min_cells):
    """wm_register_search ("sad") or wm_register_search_zncc ("zncc") on device planes a (P, side, side), b (P, E, E) and a
    pair table, every output pre-filled with a poison value.  Returns the offsets' table (P, 2S+1, 2S+1, 2 or 6) and best
    (P, 8) as int64, and peak (P, 2) float64 (None for "sad")."""
    zncc = metric == "zncc"
    n, w1 = len(table), 2 * S + 1
    pairs = _up(table.view(np.uint8).reshape(n, 32))
    score = torch.full((n, w1, w1, 6 if zncc else 2), -77, device=DEV, dtype=torch.int64 if zncc else torch.int32)
    best = torch.full((n, 8), -77, device=DEV, dtype=torch.int32)
    peak = torch.full((n, 2), 123.0, device=DEV, dtype=torch.float64) if zncc else None
    entry = N.lib().wm_register_search_zncc if zncc else N.lib().wm_register_search
    N.check(entry(N.ptr(a), N.ptr(b), N.ptr(pairs), n, S, side, min_cells, N.ptr(score), N.ptr(best), *([N.ptr(peak)] if zncc else []),
                  N.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    return score.cpu().numpy().astype(np.int64), best.cpu().numpy().astype(np.int64), peak.cpu().numpy() if zncc else None


def _search(case, a, b, min_cells=None):
    """The SAD search of a case on device planes.  Returns (score, best) int64."""
    return device_search("sad", a, b, case["pairs"], case["search"], case["side"], case["min_cells"] if min_cells is None else min_cells)[:2]


def per_k_planes():
    """The planes of the offsets-per-thread tests of both searches: 72 x 72 against 82 x 82 (search 5), 20 % / 30 % not seen."""
    rng = np.random.default_rng(17)
    A = np.where(rng.random((72, 72)) < 0.2, 0, rng.integers(1, 256, size=(72, 72))).astype(np.uint8)
    B = np.where(rng.random((82, 82)) < 0.3, 0, rng.integers(1, 256, size=(82, 82))).astype(np.uint8)
    return A, B


SCENE_H, SCENE_W = 400, 500
DISPLACED = np.array([(3, -2), (-4, 1), (2, 3), (-1, -2)], dtype=F64)                  # whole cells (east, north), zero mean
ANIMALS = np.array([(x, y) for y in (150.0, 180.0, 210.0) for x in (190.0, 215.0, 240.0, 265.0)])   # 12, >= 25 m apart


def _detections(true):
    """Every animal boxed in each frame that sees it through the TRUE georeference."""
    g2p = tiling.ground_to_pixel(true)
    out = []
    for f in range(len(true)):
        u = g2p[f, 0, 0] * ANIMALS[:, 0] + g2p[f, 0, 1] * ANIMALS[:, 1] + g2p[f, 0, 2]
        v = g2p[f, 1, 0] * ANIMALS[:, 0] + g2p[f, 1, 1] * ANIMALS[:, 1] + g2p[f, 1, 2]
        ok = (u >= 4) & (u < 196) & (v >= 4) & (v < 156)
        boxes = np.stack([u - 3, v - 3, u + 3, v + 3], axis=1)[ok].astype(np.float32)
        out.append({"boxes": _up(boxes), "scores": _up(np.linspace(0.9, 0.5, ok.sum()).astype(np.float32)),
                    "labels": torch.ones(int(ok.sum()), device=DEV, dtype=torch.int64)})
    return out


def _scene(seed=3):
    """A multi-scale texture: independent uniform fields at 1, 4 and 16 px, mixed per channel."""
    rng = np.random.default_rng(seed)
    out = np.zeros((SCENE_H, SCENE_W, 3), dtype=F64)
    for k, wt in ((1, 0.3), (4, 0.3), (16, 0.4)):
        field = rng.random((SCENE_H // k + 1, SCENE_W // k + 1, 3))
        out += wt * np.kron(field, np.ones((k, k, 1)))[:SCENE_H, :SCENE_W]
    return np.clip(out * 255.0, 0, 255).astype(np.uint8)


def _survey():
    """Four 160 x 200 frames cut from the scene (1 m per pixel; scene pixel (r, c) is the ground [c, c + 1) x [399 - r, 400 - r))
    through their TRUE georeferences, at yaw 0 / 0 / 180 / 90.  Returns frames, true georef, displaced georef."""
    scene = _scene()
    true = np.stack([tiling.nadir_affine(160, 200, c, 1.0, yaw) for c, yaw in
                     (((200.0, 200.0), 0.0), ((280.0, 220.0), 0.0), ((240.0, 170.0), 180.0), ((250.0, 210.0), 90.0))])
    yy, xx = np.meshgrid(np.arange(160) + 0.5, np.arange(200) + 0.5, indexing="ij")
    frames = []
    for g in true:
        X = g[0, 0] * xx + g[0, 1] * yy + g[0, 2]
        Y = g[1, 0] * xx + g[1, 1] * yy + g[1, 2]
        frames.append(scene[SCENE_H - 1 - np.floor(Y).astype(np.int64), np.floor(X).astype(np.int64)].copy())
    displaced = true.copy()
    displaced[:, 0, 2] += DISPLACED[:, 0]
    displaced[:, 1, 2] += DISPLACED[:, 1]
    return frames, true, displaced


# ---- the analytic scene of the refinement and of the pyramid: four yawed frames over a ground of sinusoids ------------------

FRAME_H, FRAME_W, GSD, CELL, SIDE = 320, 400, 0.5, 1.0, 128
YAWS = (10.0, -20.0, 170.0, 95.0)
CENTRES = ((1000.3, 2000.7), (1039.1, 2006.4), (1007.8, 2041.2), (1044.6, 2043.9))     # about 40 m apart, off every lattice
SIZES = [(FRAME_H, FRAME_W)] * 4
# (east m, north m, yaw degrees, scale) of the error of each georeference; frame 0 is true
NEAR = ((0.0, 0.0, 0.0, 0.0), (0.4, -0.3, 0.5, -0.004), (-0.3, 0.4, -0.4, 0.003), (0.35, 0.4, 0.3, 0.004))
FAR = ((0.0, 0.0, 0.0, 0.0), (3.2, -2.4, 2.5, -0.015), (-2.6, 3.1, -2.0, 0.012), (2.8, 3.0, 1.5, 0.015))
EXPOSURE = ((1.0, 0.0), (0.7, 30.0), (1.2, -25.0), (0.85, 12.0))                       # gain and offset of each frame


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


def _fine_value(X, Y):
    """A second bank of 24 sinusoids, wave numbers drawn with sigma 0.9 rad/m: texture a coarse point-sampled cell aliases."""
    rng = np.random.default_rng(7)
    k = rng.normal(0, 0.9, (24, 2))
    ph = rng.uniform(0, 2 * np.pi, 24)
    v = np.zeros_like(X)
    for (kx, ky), p in zip(k, ph):
        v += np.sin(kx * (X - 1000.0) + ky * (Y - 2000.0) + p)
    return v


def _far_value(X, Y):
    """The smooth scene at 0.7 of its contrast plus the fine texture."""
    return 128.0 + 0.7 * (_scene_value(X, Y) - 130.0) + _fine_value(X, Y) * 25.0 / np.sqrt(12.0)


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


# name: the ground's value, the georeferences' errors, each frame's (gain, offset), whether grey levels outside 2..254 are clipped
# (the fine texture's tails) or refused
ANALYTIC_SCENES = {"near": (_scene_value, NEAR, ((1.0, 0.0),) * 4, False), "near_exposure": (_scene_value, NEAR, EXPOSURE, False),
                   "far": (_far_value, FAR, ((1.0, 0.0),) * 4, True)}
_ANALYTIC = {}


def analytic_scene(name):
    """frames (grey, so the luma is the value), the true georeferences and the perturbed ones of ANALYTIC_SCENES[name].  Built
    once per name."""
    if name not in _ANALYTIC:
        value, errors, exposure, clip = ANALYTIC_SCENES[name]
        true = np.stack([tiling.nadir_affine(FRAME_H, FRAME_W, c, GSD, yaw) for c, yaw in zip(CENTRES, YAWS)])
        vv, uu = np.meshgrid(np.arange(FRAME_H) + 0.5, np.arange(FRAME_W) + 0.5, indexing="ij")
        frames = []
        for g, (gain, off) in zip(true, exposure):
            val = value(g[0, 0] * uu + g[0, 1] * vv + g[0, 2], g[1, 0] * uu + g[1, 1] * vv + g[1, 2])    # at every pixel centre
            val = np.rint(gain * val + off)
            if clip:
                val = np.clip(val, 2, 254)
            assert val.min() >= 2 and val.max() <= 254
            frames.append(np.repeat(val.astype(np.uint8)[:, :, None], 3, axis=2))
        _ANALYTIC[name] = (frames, true, np.stack([_perturbed(true, f, errors) for f in range(4)]))
    return _ANALYTIC[name]


def _corner_error(g, true):
    """The worst ground distance, over every frame's corners, between the georeference g and the true one: metres."""
    corners = np.array([[0, 0, 1], [FRAME_W, 0, 1], [0, FRAME_H, 1], [FRAME_W, FRAME_H, 1]], dtype=F64)
    return float(np.linalg.norm(np.einsum("fij,cj->fci", g - true, corners), axis=2).max())
