"""Survey merge, fuse policy (tiling.merge_frames / detect_frames(fuse_thr=...), wm_merge_frames_fuse): detections of one
animal split by tile seams become one detection with the union box.  The numpy restatement of the rule lives here
(fuse_oracle); CPU tests pin it on hand-worked cases and a perfect-detector seam simulation, GPU tests pin the kernel
against it bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from survey_util import _records, model  # noqa: F401 (model: a fixture)
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

NQ = 51


# ---- the definition -------------------------------------------------------------------------------------------------

def frame_boxes(boxes, origins):
    """boxes (n,51,4) tile pixels -> (n*51,4) fp32 frame boxes: the kernel's fp32 box + origin."""
    shift = np.array([[x0, y0, x0, y0] for (y0, x0) in origins], dtype=np.float32)[:, None, :]
    return (boxes.astype(np.float32) + shift).reshape(-1, 4)


def fuse_oracle(fb, scores, cand, fuse_thr=0.5):
    """Sequential greedy absorption on one frame.  fb (n*51,4) fp32 frame boxes, scores (n*51,), cand (n*51,) bool (the
    slots with FLAG_NMS).  Candidates in priority order (score descending, flat slot ascending); an unabsorbed one becomes
    a keeper and absorbs every later unabsorbed candidate of another tile with inter / min(area_keeper, area_other) >
    fuse_thr (fp32, inter as postprocess_nms_kernel computes it).  Returns (keeper slots in list order, union boxes (k,4),
    members (k,), slot_det (n*51,) list index of each candidate's detection, -1 elsewhere)."""
    fb = np.asarray(fb, np.float32)
    idx = np.nonzero(np.asarray(cand).reshape(-1))[0]
    sc = np.asarray(scores, np.float32).reshape(-1)[idx]
    order = idx[np.argsort(-sc, kind="stable")]
    b = fb[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    tile = order // NQ
    thr = np.float32(fuse_thr)
    owner = np.full(len(order), -1, np.int64)          # keeper's list index
    keepers, unions, members = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(order)):
            if owner[i] >= 0:
                continue
            k = len(keepers)
            owner[i] = k
            rest = np.arange(i + 1, len(order))
            rest = rest[owner[rest] < 0]
            iw = np.maximum(np.float32(0), np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0]))
            ih = np.maximum(np.float32(0), np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1]))
            inter = iw * ih
            ios = inter / np.minimum(area[i], area[rest])
            got = rest[(ios > thr) & (tile[rest] != tile[i])]
            owner[got] = k
            mb = np.concatenate([b[i:i + 1], b[got]])
            keepers.append(order[i])
            unions.append(np.concatenate([mb[:, :2].min(0), mb[:, 2:].max(0)]))
            members.append(1 + len(got))
    slot_det = np.full(fb.shape[0], -1, np.int64)
    slot_det[order] = owner
    return (np.array(keepers, np.int64), np.array(unions, np.float32).reshape(-1, 4), np.array(members, np.int64),
            slot_det)


def _iou_ios(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    iw = np.maximum(np.float32(0), np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    ih = np.maximum(np.float32(0), np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    inter = iw * ih
    aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    ab = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (aa + ab - inter), inter / np.minimum(aa, ab)


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _views(frame_boxes_per_tile, origins):
    """[(tile, frame box, score)] -> per-tile arrays (boxes in tile pixels, scores, cand), slots filled in order."""
    n = len(origins)
    boxes = np.zeros((n, NQ, 4), np.float32)
    scores = np.zeros((n, NQ), np.float32)
    cand = np.zeros((n, NQ), bool)
    fill = [0] * n
    for t, box, s in frame_boxes_per_tile:
        y0, x0 = origins[t]
        j = fill[t]
        fill[t] += 1
        boxes[t, j] = np.asarray(box, np.float32) - np.array([x0, y0, x0, y0], np.float32)
        scores[t, j] = s
        cand[t, j] = True
    return boxes, scores, cand


def seam_simulation(rng, H, W, n_animals, lo, hi, min_px=4):
    """Perfect detector on an H x W frame: each animal (random size in [lo, hi) px, random position, no two touching) is
    seen by every tile where at least min_px of it shows on both axes; the tile's box is the animal's box clipped to the
    tile, its score grows with the visible fraction.  Returns origins, per-tile (boxes, scores, cand) and the animals'
    boxes (fp32)."""
    org = tiling.tile_origins(H, W)
    animals = np.zeros((0, 4), np.float32)
    while len(animals) < n_animals:          # apart from each other: what merges is one animal's views
        wh = rng.uniform(lo, hi, 2)
        xy = rng.uniform(0, 1, 2) * (np.array([W, H]) - wh)
        a = np.concatenate([xy, xy + wh]).astype(np.float32)
        if not ((a[:2] < animals[:, 2:] + 1) & (animals[:, :2] < a[2:] + 1)).all(1).any():
            animals = np.concatenate([animals, a[None]])
    views = []
    for a in animals:
        area = (a[2] - a[0]) * (a[3] - a[1])
        for t, (y0, x0) in enumerate(org):
            c = np.array([max(a[0], x0), max(a[1], y0), min(a[2], x0 + 1024), min(a[3], y0 + 1024)], np.float32)
            if c[2] - c[0] >= min_px and c[3] - c[1] >= min_px:
                frac = (c[2] - c[0]) * (c[3] - c[1]) / area
                views.append((t, c, np.float32(0.5 + 0.45 * frac + rng.uniform(0, 0.01))))
    boxes, scores, cand = _views(views, org)
    return org, boxes, scores, cand, animals


def synth_seams(rng, H, W, p_cand=0.15, ties=False):
    """Random per-tile records of one frame plus seam views: objects near a seam are clipped to each tile that holds part of
    them, as a detector that only sees its tile reports them."""
    org = tiling.tile_origins(H, W)
    n = len(org)
    c = rng.random((n, NQ, 2)) * 1000 + 12
    wh = rng.random((n, NQ, 2)) * 150 + 5
    boxes = np.clip(np.concatenate([c - wh / 2, c + wh / 2], axis=-1), 0, 1024).astype(np.float32)
    scores = rng.random((n, NQ)).astype(np.float32)
    if ties:
        scores = np.array([0.5, 0.75, 0.9], np.float32)[rng.integers(0, 3, scores.shape)]
    cand = rng.random((n, NQ)) < p_cand
    for t in range(n):                       # the last 10 slots of each tile: clipped views of objects across its seams
        y0, x0 = org[t]
        for s in range(NQ - 10, NQ):
            o = rng.integers(0, n)
            oy, ox = org[o]
            if abs(oy - y0) > 1024 or abs(ox - x0) > 1024:
                continue
            ctr = np.array([ox + rng.uniform(0, 1024), oy + rng.uniform(0, 1024)])
            half = rng.uniform(20, 200, 2)
            a = np.concatenate([ctr - half, ctr + half])
            v = np.array([max(a[0], x0), max(a[1], y0), min(a[2], x0 + 1024), min(a[3], y0 + 1024)])
            if v[2] - v[0] >= 4 and v[3] - v[1] >= 4:
                boxes[t, s] = (v - np.array([x0, y0, x0, y0])).astype(np.float32)
                cand[t, s] = True
    return org, boxes, scores, cand


# ---- CPU: the definition on worked cases ----------------------------------------------------------------------------

def _run(views, org, thr=0.5):
    boxes, scores, cand = _views(views, org)
    fb = frame_boxes(boxes, org)
    return fuse_oracle(fb, scores.reshape(-1), cand.reshape(-1), thr), (boxes, scores, cand)


def test_sliver_inside_full_view():
    org = [(0, 0), (0, 896)]
    # animal [990, 1100] x [100, 160]: tile 0 sees x up to 1024 (a 34 px sliver), tile 1 sees all of it
    (keep, union, mem, sd), (boxes, scores, cand) = _run([(0, [990, 100, 1024, 160], 0.6), (1, [990, 100, 1100, 160], 0.9)], org)
    iou, ios = _iou_ios([990, 100, 1024, 160], [990, 100, 1100, 160])
    assert iou < 0.4 and ios == 1.0                        # the NMS merge keeps both
    from oracle import tiling_oracle as TO
    assert len(TO.merge(boxes, scores, cand, org, 0.4)[1]) == 2
    assert keep.tolist() == [NQ] and mem.tolist() == [2]
    assert union.tolist() == [[990, 100, 1100, 160]]
    assert sd[0] == 0 and sd[NQ] == 0 and (sd[1:NQ] == -1).all()


def test_animal_across_two_and_four_tiles():
    # 2 tiles, an animal wider than the overlap: no view covers it, the union does
    (keep, union, mem, _), _ = _run([(0, [800, 200, 1024, 260], 0.7), (1, [896, 200, 1200, 260], 0.8)], [(0, 0), (0, 896)])
    assert keep.tolist() == [NQ] and mem.tolist() == [2] and union.tolist() == [[800, 200, 1200, 260]]
    # 4 tiles around one corner: the animal [850, 1150]^2 is cut into four views; the largest absorbs the other three
    org = [(0, 0), (0, 896), (896, 0), (896, 896)]
    a = np.array([850, 850, 1150, 1150], np.float32)
    views = []
    for t, (y0, x0) in enumerate(org):
        v = [max(a[0], x0), max(a[1], y0), min(a[2], x0 + 1024), min(a[3], y0 + 1024)]
        views.append((t, v, 0.5 + 1e-6 * (v[2] - v[0]) * (v[3] - v[1])))
    (keep, union, mem, sd), _ = _run(views, org)
    assert keep.tolist() == [3 * NQ] and mem.tolist() == [4]
    assert np.array_equal(union[0], a)
    assert [sd[t * NQ] for t in range(4)] == [0, 0, 0, 0]


def test_touching_animals_stay_apart():
    org = [(0, 0), (0, 896)]
    # same tile: a calf inside its mother's box (IoS 1) and a neighbour overlapping it -- the tile's own NMS decided them
    views = [(0, [100, 100, 300, 300], 0.9), (0, [150, 150, 200, 200], 0.8), (0, [280, 100, 480, 300], 0.85)]
    # different tiles, two animals standing edge to edge across the seam: inter 0, never a match
    views += [(0, [900, 500, 960, 560], 0.7), (1, [960, 500, 1020, 560], 0.75)]
    (keep, union, mem, _), (boxes, _, _) = _run(views, org)
    assert len(keep) == 5 and (mem == 1).all()
    assert np.array_equal(union, frame_boxes(boxes, org)[keep])


def test_chain_greedy_order_decides_the_absorber():
    org = [(0, 0), (0, 896), (896, 0)]
    # K1 (tile 0) and K2 (tile 1) do not match each other; X (tile 2) matches both (IoS 0.8): the first keeper, K1,
    # absorbs it
    views = [(0, [0, 0, 100, 100], 0.9), (1, [100, 0, 200, 100], 0.8), (2, [20, 0, 180, 100], 0.7)]
    (keep, union, mem, sd), _ = _run(views, org)
    assert keep.tolist() == [0, NQ] and mem.tolist() == [2, 1]
    assert union.tolist() == [[0, 0, 180, 100], [100, 0, 200, 100]]
    assert sd[2 * NQ] == 0
    # A absorbs B; B matches C but an absorbed box absorbs nothing, and A's union (which would match C) is not used for
    # matching: C is a keeper
    views = [(0, [0, 0, 100, 100], 0.9), (1, [40, 0, 140, 100], 0.8), (2, [80, 0, 180, 100], 0.7)]
    (keep, union, mem, sd), _ = _run(views, org)
    _, ios_ab = _iou_ios([0, 0, 100, 100], [40, 0, 140, 100])
    _, ios_bc = _iou_ios([40, 0, 140, 100], [80, 0, 180, 100])
    _, ios_ac = _iou_ios([0, 0, 100, 100], [80, 0, 180, 100])
    _, ios_uc = _iou_ios([0, 0, 140, 100], [80, 0, 180, 100])
    assert ios_ab > 0.5 and ios_bc > 0.5 and ios_ac <= 0.5 and ios_uc > 0.5
    assert keep.tolist() == [0, 2 * NQ] and mem.tolist() == [2, 1]
    assert union.tolist() == [[0, 0, 140, 100], [80, 0, 180, 100]]
    assert [sd[0], sd[NQ], sd[2 * NQ]] == [0, 0, 1]


@pytest.mark.parametrize("lo,hi", [(20, 60), (40, 120), (80, 250)])
def test_seam_simulation_one_detection_per_animal(lo, hi):
    """6000 x 4000 frame, 35 tiles at the default overlap, a perfect detector: fuse gives one detection per animal, with
    the animal's box wherever each of its cut-off parts was seen; the NMS merge (tiling_oracle.merge) counts more."""
    from oracle import tiling_oracle as TO
    nms_total = fuse_total = animals_total = 0
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        org, boxes, scores, cand, animals = seam_simulation(rng, 4000, 6000, 60, lo, hi)
        assert len(org) == 35
        fb = frame_boxes(boxes, org)
        keep, union, mem, sd = fuse_oracle(fb, scores.reshape(-1), cand.reshape(-1), 0.5)
        nms_total += len(TO.merge(boxes, scores, cand, org, 0.4)[1])
        fuse_total += len(keep)
        animals_total += len(animals)
        assert mem.sum() == cand.sum() and (sd[cand.reshape(-1)] >= 0).all()
        # every detection lies inside one animal's box; most are the whole animal
        inside = (union[:, None, :2] >= animals[None, :, :2]).all(-1) & (union[:, None, 2:] <= animals[None, :, 2:]).all(-1)
        assert inside.any(1).all()
        whole = (np.abs(union[:, None, :] - animals[None]) <= 0.01).all(-1).any(1)
        assert whole.mean() > 0.95
    assert fuse_total == animals_total
    assert nms_total > fuse_total


def test_iou_above_041_implies_ios_above_half():
    """IoS <= t implies IoU <= t / (2 - t); at t = 0.5 every pair with IoU > 0.41 has IoS > 0.5, so on cross-tile pairs the
    fuse policy merges everything the NMS merge (IoU > 0.4) suppresses."""
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.uniform(0, 1000, (200000, 2)), np.zeros((200000, 2))], axis=1)
    a[:, 2:] = a[:, :2] + rng.uniform(1, 300, (200000, 2))
    b = a + rng.normal(0, 1, (200000, 4)) * np.concatenate([a[:, 2:] - a[:, :2]] * 2, axis=1) * 0.3
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 0.5)
    a, b = a.astype(np.float32), b.astype(np.float32)
    iou, ios = _iou_ios(a, b)
    sel = iou > 0.41
    assert sel.sum() > 10000
    assert (ios[sel] > np.float32(0.5)).all()
    assert (iou[ios <= 0.5] <= 0.5 / 1.5 + 1e-6).all()
    # the same on the oracle: cross-tile pairs with IoU > 0.41 always become one detection
    org = [(0, 0), (0, 896)]
    for i in np.nonzero(sel)[0][:200]:
        (keep, _, mem, _), _ = _run([(0, a[i], 0.9), (1, b[i], 0.8)], org)
        assert mem.tolist() == [2], i


def test_bad_fuse_thr_raises_before_device_work():
    rec = torch.zeros((1, NQ, 8))              # CPU records: a device call would raise RuntimeError, not ValueError
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), "half", [0.5]):
        with pytest.raises(ValueError, match="fuse_thr"):
            tiling.merge_frames(rec, torch.zeros((1, 2), dtype=torch.int32), [0, 1], fuse_thr=bad)
        with pytest.raises(ValueError, match="fuse_thr"):
            next(tiling.detect_frames(None, [np.zeros((10, 10, 3), np.uint8)], fuse_thr=bad))
        with pytest.raises(ValueError, match="fuse_thr"):
            tiling.detect_frame(None, np.zeros((10, 10, 3), np.uint8), fuse_thr=bad)


def test_fuse_entry_rejects_bad_arguments():
    import __graft_entry__ as g
    g.build()
    L = N.lib()
    p = C.c_void_p(16)                  # never dereferenced: every call below fails validation before any launch
    offs = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    good = dict(rec=p, org=p, offs=offs(0, 2, 5), nf=2, thr=0.5, scratch=p, nbytes=1 << 30, out=p, det=p, dt=p, dc=p, dm=p, sd=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.wm_merge_frames_fuse(a["rec"], a["org"], a["offs"], a["nf"], a["thr"], a["scratch"], a["nbytes"], a["out"],
                                      a["det"], a["dt"], a["dc"], a["dm"], a["sd"], None)
    for kw, msg in [(dict(rec=None), b"null"), (dict(dm=None), b"null"), (dict(sd=None), b"null"), (dict(nf=0), b"n_frames"),
                    (dict(thr=-0.1), b"fuse_thr"), (dict(thr=1.0), b"fuse_thr"), (dict(thr=float("nan")), b"fuse_thr"),
                    (dict(thr=float("inf")), b"fuse_thr"), (dict(offs=offs(1, 2, 5)), b"offsets"),
                    (dict(offs=offs(0, 3, 2)), b"strictly"), (dict(nbytes=100), b"scratch"),
                    (dict(scratch=C.c_void_p(24)), b"aligned")]:
        assert call(**kw) < 0, kw
        assert msg in L.wm_last_error() and b"wm_merge_frames_fuse" in L.wm_last_error(), (kw, L.wm_last_error())


# ---- GPU --------------------------------------------------------------------------------------------------------------


def _fuse(frames, thr=0.5):
    """frames: list of (org, boxes, scores, cand, records) -> one merge_frames(fuse_thr=thr) call, results on the CPU."""
    dev = torch.device("cuda:0")
    rec = torch.cat([f[4] for f in frames]).to(dev)
    org = torch.tensor([o for f in frames for o in f[0]], dtype=torch.int32)
    offs = np.cumsum([0] + [len(f[0]) for f in frames])
    out = tiling.merge_frames(rec, org, offs, fuse_thr=thr)
    assert set(out) == {"merged", "det", "det_tile", "det_count", "det_members", "slot_det"}
    return {k: v.cpu() for k, v in out.items()}, offs


def _check_frame(out, offs, f, frame, thr=0.5):
    """Every output of frame f against fuse_oracle, bit for bit; score, label and the other flag bits as given."""
    from wildlifemapper_amd.engine import split_records
    org, boxes, scores, cand, rec = frame
    a, b = offs[f], offs[f + 1]
    s0, ns = a * NQ, (b - a) * NQ
    fb = frame_boxes(boxes, org)
    keep, union, mem, sd = fuse_oracle(fb, scores.reshape(-1), cand.reshape(-1), thr)
    k = len(keep)
    merged = out["merged"][a:b]
    r = split_records(merged)
    assert np.array_equal(r["boxes"].reshape(-1, 4).numpy(), fb)
    got, given = merged.view(torch.int32), rec.view(torch.int32)
    assert torch.equal(got[..., 4:6], given[..., 4:6])                                          # score bits, label
    assert torch.equal(got[..., 6] & ~N.FLAG_MERGED, given[..., 6] & ~N.FLAG_MERGED)
    rank = np.full(ns, -1, np.int32)
    rank[keep] = np.arange(k)
    assert np.array_equal(got[..., 7].reshape(-1).numpy(), rank)
    assert np.array_equal(((got[..., 6] & N.FLAG_MERGED) != 0).reshape(-1).numpy(), rank >= 0)
    assert int(out["det_count"][f]) == k
    d = out["det"][s0:s0 + k]
    dint = d.view(torch.int32)
    assert np.array_equal(d[:, 0:4].numpy(), union)
    assert torch.equal(dint[:, 4:8], got.reshape(-1, 8)[torch.from_numpy(keep)][:, 4:8])     # the keeper's record
    assert np.array_equal(out["det_tile"][s0:s0 + k].numpy(), keep // NQ)
    assert np.array_equal(out["det_members"][s0:s0 + k].numpy(), mem)
    assert np.array_equal(out["slot_det"][s0:s0 + ns].numpy(), sd)
    assert int(mem.sum()) == int(cand.sum())
    return keep, mem


@pytest.mark.gpu
def test_fuse_seam_frames_bit_exact():
    rng = np.random.default_rng(41)
    frames = []
    for lo, hi in [(20, 60), (80, 250)]:
        org, boxes, scores, cand, _ = seam_simulation(rng, 4000, 6000, 60, lo, hi)
        frames.append((org, boxes, scores, cand, _records(boxes, scores, cand, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True)))
    for H, W, pc in [(4000, 6000, 0.3), (3648, 5472, 0.15), (1024, 1024, 0.5)]:
        org, boxes, scores, cand = synth_seams(rng, H, W, pc)
        frames.append((org, boxes, scores, cand, _records(boxes, scores, cand, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True)))
    out, offs = _fuse(frames)
    absorbed = 0
    for f, fr in enumerate(frames):
        keep, mem = _check_frame(out, offs, f, fr)
        absorbed += int((mem - 1).sum())
        if f < 2:
            assert len(keep) == 60
    assert absorbed > 100


@pytest.mark.gpu
def test_fuse_above_4096_candidates_global_keys():
    rng = np.random.default_rng(42)
    org, boxes, scores, cand = synth_seams(rng, 14000, 18000, 0.25)
    assert int(cand.sum()) > 4096
    fr = (org, boxes, scores, cand, _records(boxes, scores, cand, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True))
    out, offs = _fuse([fr])
    keep, mem = _check_frame(out, offs, 0, fr)
    assert (mem > 1).sum() > 50


@pytest.mark.gpu
def test_fuse_many_frames_one_call():
    """70 frames (two launches of at most 64) of mixed sizes, thresholds 0.5 and 0."""
    rng = np.random.default_rng(43)
    sizes = [(4000, 6000), (700, 900), (3648, 5472), (1024, 3000), (2000, 2000)] + [(600, 800)] * 60 + [(2200, 2200)] * 5
    frames = []
    for H, W in sizes:
        org, boxes, scores, cand = synth_seams(rng, H, W, 0.1)
        frames.append((org, boxes, scores, cand, _records(boxes, scores, cand, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True)))
    for thr in (0.5, 0.0):
        out, offs = _fuse(frames, thr)
        for f, fr in enumerate(frames):
            _check_frame(out, offs, f, fr, thr)


@pytest.mark.gpu
def test_fuse_adversarial():
    rng = np.random.default_rng(44)
    frames = []
    # exact score ties across tiles
    frames.append(synth_seams(rng, 4000, 14000, 0.08, ties=True))
    # a domino chain along a row of tiles: box k in tile k % n, each overlapping the next with IoS 0.75 and descending
    # scores; box k and k + 2 share no tile only every n-th step -- the rounds walk the whole chain
    org = tiling.tile_origins(1024, 12000)
    n = len(org)
    views = []
    for k, x in enumerate(np.arange(0.0, 11900.0, 25.0)):
        views.append((k % n, [x, 500, x + 100, 600], 1.0 - k * 1e-4))
    boxes, scores, cand = _views(views, org)
    frames.append((org, boxes, scores, cand))
    # all 51 slots of every tile are candidates, boxes reaching 512 px outside their tile
    org = tiling.tile_origins(2000, 2000)
    c = rng.random((len(org), NQ, 2)) * 1848 - 412
    wh = rng.random((len(org), NQ, 2)) * 300 + 5
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=-1).astype(np.float32)
    frames.append((org, boxes, rng.random((len(org), NQ)).astype(np.float32), np.ones((len(org), NQ), bool)))
    recs = [(o, b, s, c, _records(b, s, c, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True)) for o, b, s, c in frames]
    out, offs = _fuse(recs)
    for f, fr in enumerate(recs):
        keep, mem = _check_frame(out, offs, f, fr)
        if f == 1:                              # keepers are every second box, each absorbing the next
            assert len(keep) * 2 >= int(fr[3].sum()) and (mem <= 2).all()


@pytest.mark.gpu
def test_nms_entry_unchanged():
    from oracle import tiling_oracle as TO
    from wildlifemapper_amd.engine import split_records
    rng = np.random.default_rng(45)
    frames = []
    for H, W in [(4000, 6000), (14000, 18000)]:
        org, boxes, scores, cand = synth_seams(rng, H, W, 0.2)
        frames.append((org, boxes, scores, cand, _records(boxes, scores, cand, rng, N.FLAG_CONF | N.FLAG_MERGED, stray_bit=True)))
    dev = torch.device("cuda:0")
    rec = torch.cat([f[4] for f in frames]).to(dev)
    org = torch.tensor([o for f in frames for o in f[0]], dtype=torch.int32)
    offs = np.cumsum([0] + [len(f[0]) for f in frames])
    plain = tiling.merge_frames(rec, org, offs)
    _fuse(frames)
    none = tiling.merge_frames(rec, org, offs, 0.4, fuse_thr=None)
    assert set(none) == set(plain) == {"merged", "det", "det_tile", "det_count"}
    plain, none = {k: v.cpu() for k, v in plain.items()}, {k: v.cpu() for k, v in none.items()}
    assert torch.equal(plain["merged"].view(torch.int32), none["merged"].view(torch.int32))
    assert torch.equal(plain["det_count"], none["det_count"])
    for f in range(len(frames)):                    # the listed detections of each frame (the rest is not written)
        s0, k = offs[f] * NQ, int(plain["det_count"][f])
        assert torch.equal(plain["det"][s0:s0 + k].view(torch.int32), none["det"][s0:s0 + k].view(torch.int32))
        assert torch.equal(plain["det_tile"][s0:s0 + k], none["det_tile"][s0:s0 + k])
    for f, (o, boxes, scores, cand, _) in enumerate(frames):
        r = split_records(plain["merged"][offs[f]:offs[f + 1]])
        fb, keep = TO.merge(boxes, scores, cand, o, 0.4)
        got = torch.nonzero((r["flags"].reshape(-1) & N.FLAG_MERGED) != 0).flatten()
        got = got[torch.argsort(r["nms_rank"].reshape(-1)[got])].numpy()
        assert np.array_equal(got, keep) and int(plain["det_count"][f]) == len(keep)


# ---- GPU end to end ---------------------------------------------------------------------------------------------------


def _per_tile_fuse(model, frame_dev, thr, ext=None):
    """model.detect on the frame's tiles in batches of 4 (the last one shorter), then fuse_oracle."""
    from wildlifemapper_amd.engine import split_records
    org = tiling.tile_origins(frame_dev.shape[0], frame_dev.shape[1])
    x = tiling.frame_to_tiles(frame_dev, torch.tensor(org, dtype=torch.int32))
    recs = []
    for i in range(0, len(org), 4):
        ts = None if ext is None else torch.tensor(ext[i:i + 4], dtype=torch.float32, device=frame_dev.device)
        recs.append(model.detect(x[i:i + 4], ts)["records"] if ts is not None else model.detect(x[i:i + 4])["records"])
    r = split_records(torch.cat(recs).cpu())
    cand = ((r["flags"] & N.FLAG_NMS) != 0).numpy()
    fb = frame_boxes(r["boxes"].numpy(), org)
    return fuse_oracle(fb, r["scores"].numpy().reshape(-1), cand.reshape(-1), thr), r, cand


def _check_e2e(res, want, r, cand, n_tiles, sxy=None):
    keep, union, mem, sd = want
    k = len(keep)
    boxes = torch.from_numpy(union)
    if sxy is not None:
        boxes = torch.empty_like(boxes)
        boxes[:, 0::2] = torch.from_numpy(union[:, 0::2]) * sxy[0]
        boxes[:, 1::2] = torch.from_numpy(union[:, 1::2]) * sxy[1]
    assert res["boxes"].shape == (k, 4) and torch.equal(res["boxes"].cpu().view(torch.int32), boxes.view(torch.int32))
    assert torch.equal(res["scores"].cpu().view(torch.int32), r["scores"].reshape(-1)[keep].contiguous().view(torch.int32))
    assert torch.equal(res["labels"].cpu(), r["labels"].reshape(-1)[keep])
    assert np.array_equal(res["tile"].cpu().numpy(), keep // NQ)
    assert res["members"].dtype == torch.int64 and np.array_equal(res["members"].cpu().numpy(), mem)
    assert res["slot_det"].dtype == torch.int64 and res["slot_det"].shape == (n_tiles, NQ)
    assert np.array_equal(res["slot_det"].cpu().numpy().reshape(-1), sd)
    assert int(res["members"].sum()) == int(cand.sum())
    assert res["records"].shape == (n_tiles, NQ, 8)


@pytest.mark.gpu
def test_detect_frames_fuse_end_to_end(model):
    """ViT-B fp16 survey at batch 4 over device and host frames (tile counts 12, 1, 5, 5, 1: every batch of the survey and
    of the per-tile reference holds 4 tiles or 1, sizes at which the engine's records are bit-identical) equals
    fuse_oracle of per-tile model.detect records."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(46)
    shapes = [(2048, 3000), (600, 800), (1000, 4600), (1024, 4200), (700, 500)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    inputs = [torch.from_numpy(host[0]).to(dev), host[1], torch.from_numpy(host[2]), torch.from_numpy(host[3]).to(dev), host[4]]
    results = list(tiling.detect_frames(model, iter(inputs), batch=4, fuse_thr=0.5))
    assert len(results) == len(shapes)
    total = 0
    for i, (res, fr) in enumerate(zip(results, host)):
        want, r, cand = _per_tile_fuse(model, torch.from_numpy(fr).to(dev), 0.5)
        _check_e2e(res, want, r, cand, len(tiling.tile_origins(*shapes[i])))
        total += len(want[0])
    assert total > 0
    # the NMS survey of the same frames: same keys minus the fuse ones
    nms = next(tiling.detect_frames(model, [inputs[0]], batch=4))
    assert set(results[0]) - set(nms) == {"members", "slot_det"}


@pytest.mark.gpu
def test_detect_frames_fuse_scaled(model):
    """scale=0.5: tiles of the resampled frame with their content extents as target sizes, union boxes mapped back to
    source pixels by the fp32 multiply of the NMS path."""
    from wildlifemapper_amd import preprocess
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(47)
    f = rng.integers(0, 256, (3000, 2400, 3), dtype=np.uint8)
    oh, ow = preprocess.scaled_size(3000, 2400, 0.5)
    org = tiling.tile_origins(oh, ow)
    assert len(org) == 4
    ext = [(min(1024, ow - x0), min(1024, oh - y0)) for y0, x0 in org]
    want, r, cand = _per_tile_fuse(model, preprocess.resample_u8(torch.from_numpy(f).to(dev), (oh, ow)), 0.5, ext)
    sxy = (float(np.float32(2400 / ow)), float(np.float32(3000 / oh)))
    for res in (tiling.detect_frame(model, torch.from_numpy(f).to(dev), batch=4, scale=0.5, fuse_thr=0.5),
                next(tiling.detect_frames(model, [f], batch=4, scale=0.5, fuse_thr=0.5))):
        assert res["resampled_size"] == (oh, ow)
        _check_e2e(res, want, r, cand, 4, sxy)
