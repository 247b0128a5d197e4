"""The ground rules of the survey (include/wm_hip.h "Survey census", "Survey coverage", "Survey mosaic", "Survey mosaic,
blended"), restated once for every test and tool that checks the kernels against them.  None of these rules has a reference
behaviour: the oracles below are their sequential restatement -- one cell, one point or one detection at a time, numpy
float64, the header's operation order -- and the device must equal them exactly, so every operation here stays an
np.float64 operation in the order written.  Elementwise numpy arithmetic is one correctly rounded IEEE operation per
element and operator.  The *_by_frame forms are the same rules one frame at a time over the window of cells around its
footprint, held equal to the sequential ones by the tests and fast enough for the grids the tools time.

Pure numpy: nothing else is imported, so a tool or a CPU session can use it without the library.  Nothing here asserts
about a device."""
import numpy as np

F64 = np.float64
MODES = {"nearest": 0, "bilinear": 1}            # WM_MOSAIC_NEAREST, WM_MOSAIC_BILINEAR: tests/test_mosaic.py holds them equal
SENTINEL = (7, 201, 77)


# ---- the geometry every ground kernel shares (coverage_kernels.h) ------------------------------------------------------

def centre(o, cell, i):
    """The centre of cell i along one axis of a grid with origin o: o + (i + 0.5) * cell.  i: an index or an array of them."""
    return o + (np.asarray(i, dtype=F64) + F64(0.5)) * cell


def uv(b, X, Y):
    """The position (u, v) of the point (X, Y) under the affine b (..., 6), broadcast over whatever shapes it is given:
    (b0 * X + b1 * Y) + b2 and (b3 * X + b4 * Y) + b5.  Ground -> pixel with a frame's g2p, pixel -> ground with its georeference."""
    u = (b[..., 0] * X + b[..., 1] * Y) + b[..., 2]
    v = (b[..., 3] * X + b[..., 4] * Y) + b[..., 5]
    return u, v


def inside(u, v, h, w):
    """sees: the position (u, v) lies in a frame of h x w pixels, half open; a frame without pixels sees nothing."""
    return (h >= 1) & (w >= 1) & (0 <= u) & (u < w) & (0 <= v) & (v < h)


def window(bf, h, w, x0, y0, cell, gx, gy):
    """The cells (i0, i1, j0, j1) around the footprint of a frame with g2p bf (6,) and h x w pixels: its corners through the
    numerically inverted 2 x 2, two cells of margin, clipped to the grid; the whole grid where that cannot be told; None
    for a frame that sees nothing (no pixels, or a coefficient that is not finite)."""
    if h < 1 or w < 1 or not np.isfinite(bf).all():
        return None
    i0, i1, j0, j1 = 0, gx, 0, gy
    A = np.array([[bf[0], bf[1]], [bf[3], bf[4]]])
    if abs(np.linalg.det(A)) > 0:
        corners = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=F64) - bf[[2, 5]]
        ground = np.linalg.solve(A, corners.T).T
        if np.isfinite(ground).all():
            i0 = int(np.clip(np.floor((ground[:, 0].min() - x0) / cell) - 2, 0, gx))
            i1 = int(np.clip(np.ceil((ground[:, 0].max() - x0) / cell) + 2, 0, gx))
            j0 = int(np.clip(np.floor((ground[:, 1].min() - y0) / cell) - 2, 0, gy))
            j1 = int(np.clip(np.ceil((ground[:, 1].max() - y0) / cell) + 2, 0, gy))
    return i0, i1, j0, j1


def _tables(g2p, size):
    return np.asarray(g2p, dtype=F64).reshape(-1, 6), np.asarray(size, dtype=np.int64).reshape(-1, 2)


# ---- census ------------------------------------------------------------------------------------------------------------

def census_oracle(boxes, scores, labels, frame, georef, radius, same_class=False):
    """The census rule, sequentially.  Returns points (n,2) float64, individual (n,) int64, keeper (k,) int64,
    members (k,) int64 and count."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    frame = np.asarray(frame, dtype=np.int64).reshape(-1)
    g = np.asarray(georef, dtype=np.float64).reshape(-1, 6)
    n, F = boxes.shape[0], g.shape[0]
    pts = np.full((n, 2), np.nan, dtype=np.float64)
    valid = []
    with np.errstate(all="ignore"):
        for i in range(n):
            if not (np.isfinite(boxes[i]).all() and np.isfinite(scores[i]) and 0 <= frame[i] < F):
                continue
            x0, y0, x1, y1 = (np.float64(v) for v in boxes[i])
            cx = (x0 + x1) * np.float64(0.5)
            cy = (y0 + y1) * np.float64(0.5)
            X, Y = uv(g[frame[i]], cx, cy)
            if np.isfinite(X) and np.isfinite(Y):
                pts[i] = (X, Y)
                valid.append(i)
        order = sorted(valid, key=lambda i: (-float(scores[i]), i))        # -0.0 == 0.0: the index breaks the tie
        r2 = np.float64(radius) * np.float64(radius)
        individual = np.full(n, -1, dtype=np.int64)
        kx, ky = np.empty(len(order)), np.empty(len(order))
        klabel = np.empty(len(order), dtype=np.int64)
        kframes = np.zeros((len(order), max(F, 1)), dtype=bool)           # kframes[q, f]: individual q has a member of frame f
        keeper, members = [], []
        for p in order:
            k = len(keeper)
            dx, dy = pts[p, 0] - kx[:k], pts[p, 1] - ky[:k]
            d2 = dx * dx + dy * dy
            ok = (d2 <= r2) & ~kframes[:k, frame[p]]
            if same_class:
                ok &= klabel[:k] == labels[p]
            if ok.any():
                q = int(np.argmin(np.where(ok, d2, np.inf)))                # first minimum: the individual founded earlier
                members[q] += 1
            else:
                q = k
                kx[q], ky[q], klabel[q] = pts[p, 0], pts[p, 1], labels[p]
                keeper.append(p)
                members.append(1)
            kframes[q, frame[p]] = True
            individual[p] = q
    return {"points": pts, "individual": individual, "keeper": np.array(keeper, dtype=np.int64),
            "members": np.array(members, dtype=np.int64), "count": len(keeper)}


# ---- coverage ----------------------------------------------------------------------------------------------------------

def coverage_oracle(g2p, size, x0, y0, cell, gx, gy, points=None, labels=None):
    """The coverage rule, one cell and one point at a time.  Returns coverage (gy,gx) int64 and stats (16,) int64, and
    with points also seen_by (P,), cell (P,2), counts (7,gy,gx) and pstats (2,), all int64."""
    b, size = _tables(g2p, size)
    h, w = size[:, 0], size[:, 1]
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    cov = np.zeros((gy, gx), dtype=np.int64)
    stats = np.zeros(16, dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(gy):
            Yc = centre(y0, cell, j)
            for i in range(gx):
                Xc = centre(x0, cell, i)
                m = int(inside(*uv(b, Xc, Yc), h, w).sum())
                cov[j, i] = m
                stats[min(m, 15)] += 1
        out = {"coverage": cov, "stats": stats}
        if points is None:
            return out
        pts = np.asarray(points, dtype=F64).reshape(-1, 2)
        labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        P = pts.shape[0]
        seen = np.zeros(P, dtype=np.int64)
        cidx = np.full((P, 2), -1, dtype=np.int64)
        counts = np.zeros((7, gy, gx), dtype=np.int64)
        pstats = np.zeros(2, dtype=np.int64)
        for p in range(P):
            X, Y = pts[p]
            finite = bool(np.isfinite(X) and np.isfinite(Y))
            if finite:
                seen[p] = int(inside(*uv(b, X, Y), h, w).sum())
            fi = np.floor((X - x0) / cell)
            fj = np.floor((Y - y0) / cell)
            if finite and 0 <= fi < gx and 0 <= fj < gy and 0 <= labels[p] < 7:
                cidx[p] = (int(fj), int(fi))
                counts[labels[p], int(fj), int(fi)] += 1
                pstats[0] += 1
            else:
                pstats[1] += 1
    out.update({"seen_by": seen, "cell": cidx, "counts": counts, "pstats": pstats})
    return out


def coverage_oracle_by_frame(g2p, size, x0, y0, cell, gx, gy):
    """The raster part of the rule, one FRAME at a time over its window: the same operations per cell as coverage_oracle."""
    b, size = _tables(g2p, size)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    Xc, Yc = centre(x0, cell, np.arange(gx)), centre(y0, cell, np.arange(gy))
    cov = np.zeros((gy, gx), dtype=np.int64)
    with np.errstate(all="ignore"):
        for f in range(b.shape[0]):
            h, w = size[f]
            win = window(b[f], h, w, x0, y0, cell, gx, gy)
            if win is None:
                continue
            i0, i1, j0, j1 = win
            cov[j0:j1, i0:i1] += inside(*uv(b[f], Xc[None, i0:i1], Yc[j0:j1, None]), h, w)
    stats = np.bincount(np.minimum(cov, 15).ravel(), minlength=16).astype(np.int64)
    return {"coverage": cov, "stats": stats}


# ---- mosaic ------------------------------------------------------------------------------------------------------------

def _sample(img, u, v, mode):
    """One cell from its source frame img (H,W,3) uint8 at the pixel position (u, v), by the header's sampling rule."""
    h, w = img.shape[:2]
    if mode == "nearest":
        return img[int(np.floor(v)), int(np.floor(u))]
    fu, fv = u - F64(0.5), v - F64(0.5)
    xf, yf = np.floor(fu), np.floor(fv)
    tx, ty = fu - xf, fv - yf
    xa, xb = min(max(int(xf), 0), w - 1), min(max(int(xf) + 1, 0), w - 1)
    ya, yb = min(max(int(yf), 0), h - 1), min(max(int(yf) + 1, 0), h - 1)
    p00, p10, p01, p11 = (img[y, x].astype(F64) for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    a = (F64(1.0) - tx) * p00 + tx * p10
    b = (F64(1.0) - tx) * p01 + tx * p11
    val = (F64(1.0) - ty) * a + ty * b
    return np.minimum(np.floor(val + F64(0.5)), F64(255.0)).astype(np.uint8)


def _sample_many(img, u, v, mode):
    """_sample for arrays of positions: the same operations, elementwise."""
    h, w = img.shape[:2]
    if mode == "nearest":
        return img[np.floor(v).astype(np.int64), np.floor(u).astype(np.int64)]
    fu, fv = u - F64(0.5), v - F64(0.5)
    xf, yf = np.floor(fu), np.floor(fv)
    tx, ty = (fu - xf)[:, None], (fv - yf)[:, None]
    xa, xb = np.clip(xf.astype(np.int64), 0, w - 1), np.clip(xf.astype(np.int64) + 1, 0, w - 1)
    ya, yb = np.clip(yf.astype(np.int64), 0, h - 1), np.clip(yf.astype(np.int64) + 1, 0, h - 1)
    p00, p10, p01, p11 = img[ya, xa].astype(F64), img[ya, xb].astype(F64), img[yb, xa].astype(F64), img[yb, xb].astype(F64)
    a = (F64(1.0) - tx) * p00 + tx * p10
    b = (F64(1.0) - tx) * p01 + tx * p11
    val = (F64(1.0) - ty) * a + ty * b
    return np.minimum(np.floor(val + F64(0.5)), F64(255.0)).astype(np.uint8)


def _filled(gy, gx, fill):
    pic = np.empty((gy, gx, 3), dtype=np.uint8)
    pic[:] = np.asarray(fill, dtype=np.uint8)
    return pic


def mosaic_oracle(g2p, size, x0, y0, cell, gx, gy, frames=None, fill=SENTINEL):
    """The mosaic rule, one cell at a time, vectorised over the frames only.  Returns source (gy,gx), won (F,), stats (2,),
    all int64, and with frames (a list of (H,W,3) uint8 arrays, None for a frame without pixels) the pictures 'nearest' and
    'bilinear' (gy,gx,3) uint8, row 0 south, cells without a source holding `fill`.  argmin returns the first, that is the
    lowest, index."""
    b, size = _tables(g2p, size)
    h, w = size[:, 0], size[:, 1]
    cu, cv = F64(0.5) * w.astype(F64), F64(0.5) * h.astype(F64)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    nf = b.shape[0]
    source = np.full((gy, gx), -1, dtype=np.int64)
    pics = {m: _filled(gy, gx, fill) for m in MODES} if frames is not None else {}
    with np.errstate(all="ignore"):
        for j in range(gy):
            Yc = centre(y0, cell, j)
            for i in range(gx):
                if not nf:
                    continue
                u, v = uv(b, centre(x0, cell, i), Yc)
                sees = inside(u, v, h, w)
                if not sees.any():
                    continue
                du, dv = u - cu, v - cv
                e = du * du + dv * dv
                f = int(np.argmin(np.where(sees, e, np.inf)))
                source[j, i] = f
                for m, p in pics.items():
                    p[j, i] = _sample(frames[f], u[f], v[f], m)
    seen = source >= 0
    out = {"source": source, "won": np.bincount(source[seen], minlength=nf).astype(np.int64),
           "stats": np.array([seen.sum(), (~seen).sum()], dtype=np.int64)}
    out.update(pics)
    return out


def mosaic_oracle_by_frame(g2p, size, x0, y0, cell, gx, gy, frames=None, fill=SENTINEL, modes=tuple(MODES)):
    """The same rule one FRAME at a time over its window, with a running best e per cell: frames in ascending order and a
    strict <, so the lowest index keeps a tie.  The same operations per cell as mosaic_oracle."""
    b, size = _tables(g2p, size)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    Xc, Yc = centre(x0, cell, np.arange(gx)), centre(y0, cell, np.arange(gy))
    best = np.full((gy, gx), np.inf, dtype=F64)
    source = np.full((gy, gx), -1, dtype=np.int64)
    windows = {}
    with np.errstate(all="ignore"):
        for f in range(b.shape[0]):
            h, w = size[f]
            win = window(b[f], h, w, x0, y0, cell, gx, gy)
            if win is None:
                continue
            windows[f] = i0, i1, j0, j1 = win
            u, v = uv(b[f], Xc[None, i0:i1], Yc[j0:j1, None])
            du, dv = u - F64(0.5) * F64(w), v - F64(0.5) * F64(h)
            e = du * du + dv * dv
            better = inside(u, v, h, w) & (e < best[j0:j1, i0:i1])
            best[j0:j1, i0:i1][better] = e[better]
            source[j0:j1, i0:i1][better] = f
        seen = source >= 0
        out = {"source": source, "won": np.bincount(source[seen], minlength=b.shape[0]).astype(np.int64),
               "stats": np.array([seen.sum(), (~seen).sum()], dtype=np.int64)}
        if frames is None:
            return out
        for m in modes:
            out[m] = _filled(gy, gx, fill)
        for f, (i0, i1, j0, j1) in windows.items():
            jj, ii = np.nonzero(source[j0:j1, i0:i1] == f)
            if not len(jj):
                continue
            u, v = uv(b[f], Xc[i0 + ii], Yc[j0 + jj])
            for m in modes:
                out[m][j0 + jj, i0 + ii] = _sample_many(frames[f], u, v, m)
    return out


# ---- mosaic, blended ---------------------------------------------------------------------------------------------------

def _weight(m, best, band):
    """q of the header, elementwise, for frames that see the cell: m their border distance, best the cell's m*."""
    band = F64(band)
    k = F64(256.0) / band
    top = m >= best
    edge = np.minimum(m * k, F64(256.0))
    seam = np.where(top, F64(256.0), np.minimum(np.maximum(((m - best) + band) * k, F64(0.0)), F64(255.0)))
    q = np.floor(np.minimum(seam, edge)).astype(np.int64)
    return np.where(top, np.maximum(q, 1), q)


def _expose(p, ab):
    """p' of the header: uint8 pixels p through the Q12 (A, B), in int64; // is floor."""
    if ab is None:
        return p.astype(np.int64)
    return np.clip((np.int64(ab[0]) * p.astype(np.int64) + np.int64(ab[1]) + 2048) // 4096, 0, 255)


def _finish(acc, fill):
    """The picture of the header from acc (gy,gx,4) uint64: (acc_c + (wsum >> 1)) // wsum where wsum > 0, else fill."""
    pic = _filled(acc.shape[0], acc.shape[1], fill)
    has = acc[..., 3] > 0
    ws = acc[..., 3][has]
    pic[has] = ((acc[..., :3][has] + (ws >> np.uint64(1))[:, None]) // ws[:, None]).astype(np.uint8)
    return pic


def _blend_out(best, cells, nq, acc, fill):
    seen = best >= 0
    out = {"best": best, "cells": cells, "stats": np.array([seen.sum(), (~seen).sum(), (nq >= 2).sum()], dtype=np.int64)}
    for mode, a in acc.items():
        assert a.max(initial=0) < 2 ** 32
        out["acc_" + mode] = a.astype(np.uint32)
        out[mode] = _finish(a, fill)
    return out


def blend_oracle(g2p, size, x0, y0, cell, gx, gy, band, frames=None, exposure=None, fill=SENTINEL, resident=None):
    """The blend rule, one cell at a time, vectorised over the frames only.  Returns best (gy,gx) float64, cells (F,) and
    stats (3,) int64, and with frames (a list of (H,W,3) uint8 arrays, None for a frame without pixels) 'acc_nearest' /
    'acc_bilinear' (gy,gx,4) uint32 and the pictures 'nearest' / 'bilinear' (gy,gx,3) uint8, row 0 south, cells without a
    weight holding `fill`.  exposure: (F,2) int32 or None.  resident: the frames that are accumulated (None: all with
    pixels); best, cells and stats are the whole survey's whatever it says."""
    b, size = _tables(g2p, size)
    h, w = size[:, 0], size[:, 1]
    fw, fh = w.astype(F64), h.astype(F64)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    nf = b.shape[0]
    best = np.full((gy, gx), -1.0, dtype=F64)
    cells = np.zeros(nf, dtype=np.int64)
    nq = np.zeros((gy, gx), dtype=np.int64)
    acc = {m: np.zeros((gy, gx, 4), dtype=np.uint64) for m in MODES} if frames is not None else {}
    take = set(range(nf)) if resident is None else set(resident)
    with np.errstate(all="ignore"):
        for j in range(gy):
            Yc = centre(y0, cell, j)
            for i in range(gx):
                if not nf:
                    continue
                u, v = uv(b, centre(x0, cell, i), Yc)
                sees = inside(u, v, h, w)
                if not sees.any():
                    continue
                fs = np.nonzero(sees)[0]
                us, vs = u[fs], v[fs]
                m = np.minimum(np.minimum(us, fw[fs] - us), np.minimum(vs, fh[fs] - vs))
                best[j, i] = m.max()
                q = _weight(m, best[j, i], band)
                cells[fs[q > 0]] += 1
                nq[j, i] = (q > 0).sum()
                for f, qf, uf, vf in zip(fs.tolist(), q.tolist(), us, vs):
                    if qf > 0 and f in take and frames is not None and frames[f] is not None:
                        for mode, a in acc.items():
                            p = _expose(_sample(frames[f], uf, vf, mode), None if exposure is None else exposure[f])
                            a[j, i, :3] += (qf * p).astype(np.uint64)
                            a[j, i, 3] += np.uint64(qf)
    return _blend_out(best, cells, nq, acc, fill)


def blend_oracle_by_frame(g2p, size, x0, y0, cell, gx, gy, band, frames=None, exposure=None, fill=SENTINEL, modes=tuple(MODES)):
    """The same rule one FRAME at a time over its window, in two walks as the plan kernel makes them: first the running
    maximum m*, then every frame's weights against the finished m* and its sums.  The same operations per cell as blend_oracle."""
    b, size = _tables(g2p, size)
    x0, y0, cell = F64(x0), F64(y0), F64(cell)
    Xc, Yc = centre(x0, cell, np.arange(gx)), centre(y0, cell, np.arange(gy))
    nf = b.shape[0]
    best = np.full((gy, gx), -1.0, dtype=F64)
    cells = np.zeros(nf, dtype=np.int64)
    nq = np.zeros((gy, gx), dtype=np.int64)
    acc = {m: np.zeros((gy, gx, 4), dtype=np.uint64) for m in modes} if frames is not None else {}

    def geometry(f):
        """Frame f's window (i0, j0) and, on it, u, v, inside and m; None for a frame that sees nothing."""
        h, w = size[f]
        win = window(b[f], h, w, x0, y0, cell, gx, gy)
        if win is None:
            return None
        i0, i1, j0, j1 = win
        u, v = uv(b[f], Xc[None, i0:i1], Yc[j0:j1, None])
        return i0, j0, u, v, inside(u, v, h, w), np.minimum(np.minimum(u, F64(w) - u), np.minimum(v, F64(h) - v))

    with np.errstate(all="ignore"):
        for f in range(nf):
            geo = geometry(f)
            if geo is not None:
                i0, j0, u, v, sees, m = geo
                sub = best[j0:j0 + m.shape[0], i0:i0 + m.shape[1]]
                upd = sees & (m > sub)
                sub[upd] = m[upd]
        for f in range(nf):
            geo = geometry(f)                                   # computed again, not kept: a survey of 1 000 frames stays small
            if geo is None:
                continue
            i0, j0, u, v, sees, m = geo
            jj, ii = np.nonzero(sees)
            if not len(jj):
                continue
            q = _weight(m[jj, ii], best[j0 + jj, i0 + ii], band)
            pos = q > 0
            jj, ii, q = jj[pos], ii[pos], q[pos]
            cells[f] = len(q)
            nq[j0 + jj, i0 + ii] += 1
            if frames is None or frames[f] is None:
                continue
            for mode, a in acc.items():
                p = _expose(_sample_many(frames[f], u[jj, ii], v[jj, ii], mode), None if exposure is None else exposure[f])
                a[j0 + jj, i0 + ii, :3] += (q[:, None] * p).astype(np.uint64)
                a[j0 + jj, i0 + ii, 3] += q.astype(np.uint64)
    return _blend_out(best, cells, nq, acc, fill)
