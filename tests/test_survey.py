"""Survey front end (tiling.detect_frames): batch plan and C-ABI validation on the CPU; the segmented merge
(wm_merge_frames_nms), the multi-frame tile cut (wm_tile_frames_u8) and detect_frames on the GPU against
oracle/tiling_oracle.py and the single-frame path."""
import ctypes as C

import numpy as np
import pytest
import torch

from survey_util import _records
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

NQ = 51


def _check_plan(counts, batch):
    plan = list(tiling.plan_batches(iter(counts), batch))
    seen = [(f, t) for b in plan for f, t0, t1 in b.segments for t in range(t0, t1)]
    assert seen == [(f, t) for f, n in enumerate(counts) for t in range(n)]          # every tile once, in frame order
    sizes = [sum(t1 - t0 for _, t0, t1 in b.segments) for b in plan]
    assert all(s == batch for s in sizes[:-1]) and 0 < sizes[-1] <= batch
    assert sum(sizes) == sum(counts)
    done = [f for b in plan for f in b.completes]
    assert done == list(range(len(counts)))
    for bi, b in enumerate(plan):                        # a frame completes in the batch holding its last tile
        for f in b.completes:
            last = max(i for i, bb in enumerate(plan) for ff, _, t1 in bb.segments if ff == f and t1 == counts[f])
            assert last == bi
    return plan


def test_plan_batches_mixed_sizes():
    sizes = [(500, 700), (1, 5000), (4000, 6000), (5472, 3648), (3648, 5472), (1024, 1024), (30, 1), (1025, 1025),
             (15000, 20000)]
    counts = [len(tiling.tile_origins(h, w)) for h, w in sizes]
    assert counts[:6] == [1, 6, 35, 24, 24, 1] and counts[-1] == 391
    for batch in (1, 3, 4, 16, 17, 1000):
        _check_plan(counts, batch)
    plan = _check_plan([1, 6, 35], 16)
    assert [b.completes for b in plan] == [[0, 1], [], [2]]        # 1 + 6 + 9 | 16 | 10 (last, short)
    assert plan[0].segments == [(0, 0, 1), (1, 0, 6), (2, 0, 9)]
    with pytest.raises(ValueError):
        list(tiling.plan_batches([3, 0], 4))
    with pytest.raises(ValueError):
        list(tiling.plan_batches([3], 0))


def test_plan_batches_is_lazy():
    pulled = []

    def counts():
        for f, n in enumerate([5, 5, 5]):
            pulled.append(f)
            yield n
    it = tiling.plan_batches(counts(), 4)
    b = next(it)
    assert b.segments == [(0, 0, 4)] and pulled == [0]


def _offs(*vals):
    a = (C.c_int32 * len(vals))(*vals)
    return a


def test_merge_frames_rejects_bad_arguments():
    import __graft_entry__ as g
    g.build()
    L = N.lib()
    p = C.c_void_p(16)                  # never dereferenced: every call below fails validation before any launch
    good = dict(rec=p, org=p, offs=_offs(0, 2, 5), nf=2, thr=0.4, scratch=p, nbytes=1 << 30, out=p, det=p, dt=p, dc=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.wm_merge_frames_nms(a["rec"], a["org"], a["offs"], a["nf"], a["thr"], a["scratch"], a["nbytes"], a["out"], a["det"],
                                     a["dt"], a["dc"], None)
    for kw, msg in [(dict(rec=None), b"null"), (dict(offs=None), b"null"), (dict(dc=None), b"null"), (dict(scratch=None), b"null"),
                    (dict(nf=0), b"n_frames"), (dict(nf=-3), b"n_frames"),
                    (dict(thr=-0.1), b"iou_thr"), (dict(thr=1.0), b"iou_thr"), (dict(thr=float("nan")), b"iou_thr"),
                    (dict(offs=_offs(1, 2, 5)), b"offsets"), (dict(offs=_offs(0, 2, 2)), b"strictly"),
                    (dict(offs=_offs(0, 3, 2)), b"strictly"), (dict(nbytes=100), b"scratch"), (dict(scratch=C.c_void_p(24)), b"aligned")]:
        assert call(**kw) < 0, kw
        assert msg in L.wm_last_error(), (kw, L.wm_last_error())
    assert L.wm_merge_frames_scratch_bytes(5) == 5 * NQ * 36
    assert L.wm_merge_frames_scratch_bytes(0) < 0
    assert L.wm_tile_frames_u8(None, 1, p, p, 4, None) < 0 and b"null" in L.wm_last_error()
    assert L.wm_tile_frames_u8(p, 0, p, p, 4, None) < 0 and b"n_frames" in L.wm_last_error()
    assert L.wm_tile_frames_u8(p, 2, p, p, 0, None) < 0 and b"n_tiles" in L.wm_last_error()
    with pytest.raises(RuntimeError, match="uint8"):
        next(tiling.detect_frames(None, [np.zeros((10, 10), np.uint8)]))
    with pytest.raises(RuntimeError, match="uint8"):
        next(tiling.detect_frames(None, [np.zeros((10, 10, 3), np.float32)]))


# ---- GPU --------------------------------------------------------------------------------------------------------------


def _synth_frame(H, W, rng, p_cand=0.15, dup=4, wide=False):
    """Random per-tile records of one H x W frame: boxes in tile pixels, some duplicated in the right-hand neighbour
    (same frame box, score tie or slightly lower), optionally reaching up to 512 px outside their tile."""
    org = tiling.tile_origins(H, W)
    n = len(org)
    lo, hi = (-512.0, 1536.0) if wide else (0.0, 1024.0)
    c = rng.random((n, NQ, 2)) * (hi - lo - 200) + lo + 100
    wh = rng.random((n, NQ, 2)) * (300 if wide else 90) + 5
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=-1).astype(np.float32)
    boxes = np.clip(boxes, lo, hi)
    scores = rng.random((n, NQ)).astype(np.float32)
    cand = rng.random((n, NQ)) < p_cand
    if dup:
        for t in range(n - 1):
            if org[t][0] == org[t + 1][0]:
                dx = org[t + 1][1] - org[t][1]
                for s in range(dup):
                    boxes[t + 1, s] = boxes[t, s] - np.array([dx, 0, dx, 0], np.float32)
                    scores[t + 1, s] = scores[t, s] * (0.99 if s % 2 else 1.0)
                    cand[t, s] = cand[t + 1, s] = True
    return org, boxes, scores, cand


def _check_against_oracle(merged, det, det_tile, count, boxes, scores, cand, org, thr=0.4):
    from oracle import tiling_oracle as TO
    from wildlifemapper_amd.engine import split_records
    r = split_records(merged)
    fb, keep = TO.merge(boxes, scores, cand, org, thr)
    assert np.array_equal(r["boxes"].reshape(-1, 4).numpy(), fb)
    flags, rank = r["flags"].reshape(-1), r["nms_rank"].reshape(-1)
    got = torch.nonzero((flags & N.FLAG_MERGED) != 0).flatten()
    got = got[torch.argsort(rank[got])].numpy()
    assert np.array_equal(got, keep)
    assert np.array_equal(rank.numpy()[keep], np.arange(len(keep)))
    assert int((rank >= 0).sum()) == len(keep)
    assert count == len(keep)
    d = split_records(det[:count].view(count, 1, 8))
    assert np.array_equal(d["boxes"].reshape(-1, 4).numpy(), fb[keep])
    assert np.array_equal(d["nms_rank"].reshape(-1).numpy(), np.arange(len(keep)))
    assert np.array_equal(det_tile[:count].numpy(), keep // NQ)
    return keep


def _merge(frames, thr=0.4):
    """frames: list of (org, boxes, scores, cand, rng-made records) -> one wm_merge_frames_nms launch, results on the CPU."""
    dev = torch.device("cuda:0")
    rec = torch.cat([f[4] for f in frames]).to(dev)
    org = torch.tensor([o for f in frames for o in f[0]], dtype=torch.int32)
    offs = np.cumsum([0] + [len(f[0]) for f in frames])
    out = tiling.merge_frames(rec, org, offs, thr)
    return {k: v.cpu() for k, v in out.items()}, offs


@pytest.mark.gpu
def test_merge_frames_single_frame_300_plus_tiles():
    rng = np.random.default_rng(11)
    org, boxes, scores, cand = _synth_frame(14000, 18000, rng, p_cand=0.015, dup=1)
    assert len(org) >= 300
    rec = _records(boxes, scores, cand, rng)
    out, _ = _merge([(org, boxes, scores, cand, rec)])
    keep = _check_against_oracle(out["merged"], out["det"], out["det_tile"], int(out["det_count"][0]), boxes, scores, cand, org)
    assert 0 < len(keep) < int(cand.sum())
    # merge_tile_records is this merge on a one-frame survey, at any tile count
    m = tiling.merge_tile_records(rec.to("cuda:0"), torch.tensor(org, dtype=torch.int32), 0.4).cpu()
    assert torch.equal(m.view(torch.int32), out["merged"].view(torch.int32))


@pytest.mark.gpu
def test_merge_frames_many_frames_one_launch():
    rng = np.random.default_rng(12)
    frames = []
    for H, W in [(4000, 6000), (700, 900), (3648, 5472), (9000, 9000), (1024, 3000), (2000, 2000)]:
        org, boxes, scores, cand = _synth_frame(H, W, rng, p_cand=0.04, dup=2, wide=(H == 3648))
        frames.append((org, boxes, scores, cand, _records(boxes, scores, cand, rng)))
    out, offs = _merge(frames)
    for f, (org, boxes, scores, cand, _) in enumerate(frames):
        a, b = offs[f], offs[f + 1]
        _check_against_oracle(out["merged"][a:b], out["det"][a * NQ:], out["det_tile"][a * NQ:], int(out["det_count"][f]),
                              boxes, scores, cand, org)


@pytest.mark.gpu
def test_merge_frames_up_to_80_tiles_every_field():
    """One frame per merge at common frame sizes (1 to 72 tiles): every field of every record pinned -- boxes, survivors,
    nms_rank, the count and the compacted list against the oracle; score, label and the flag bits other than
    FLAG_MERGED as given."""
    rng = np.random.default_rng(13)
    for H, W, pc in [(4000, 6000, 0.4), (1024, 1024, 1.0), (7000, 8000, 0.3), (3000, 2000, 0.0)]:
        org, boxes, scores, cand = _synth_frame(H, W, rng, p_cand=pc, dup=4 if pc > 0 else 0, wide=True)
        assert len(org) <= 80
        rec = _records(boxes, scores, cand, rng)
        out, _ = _merge([(org, boxes, scores, cand, rec)])
        keep = _check_against_oracle(out["merged"], out["det"], out["det_tile"], int(out["det_count"][0]), boxes, scores, cand,
                                     org)
        got, given = out["merged"].view(torch.int32), rec.view(torch.int32)
        assert torch.equal(got[..., 4:6], given[..., 4:6]), (H, W, pc)                       # score bits, label
        assert torch.equal(got[..., 6] & ~N.FLAG_MERGED, given[..., 6] & ~N.FLAG_MERGED), (H, W, pc)
        rank = np.full(len(org) * NQ, -1, np.int32)
        rank[keep] = np.arange(len(keep))
        assert np.array_equal(got[..., 7].reshape(-1).numpy(), rank), (H, W, pc)


@pytest.mark.gpu
def test_merge_frames_adversarial():
    rng = np.random.default_rng(14)
    frames = []
    # exact score ties across tiles: every candidate of the frame has one of three scores
    org, boxes, scores, cand = _synth_frame(4000, 14000, rng, p_cand=0.08, dup=2)
    scores[:] = np.array([0.5, 0.75, 0.9], np.float32)[rng.integers(0, 3, scores.shape)]
    frames.append((org, boxes, scores, cand))
    # a domino chain: along a row of tiles, boxes each overlapping the next (IoU 0.6) with descending scores -- greedy keeps
    # every second one, the rounds have to walk the whole chain
    org = tiling.tile_origins(1024, 12000)
    n = len(org)
    boxes = np.zeros((n, NQ, 4), np.float32)
    scores = np.zeros((n, NQ), np.float32)
    cand = np.zeros((n, NQ), bool)
    x, k = 0.0, 0
    while x + 100 < 12000:
        t = min(int(x // (1024 - 128)), n - 1)
        while org[t][1] + 1024 < x + 100:
            t += 1
        s = k % NQ
        boxes[t, s] = [x - org[t][1], 500, x + 100 - org[t][1], 600]
        scores[t, s] = 1.0 - k * 1e-4
        cand[t, s] = True
        x += 25.0
        k += 1
    frames.append((org, boxes, scores, cand))
    # all 51 slots of every tile are candidates, boxes reaching 512 px outside their tile
    org, boxes, scores, cand = _synth_frame(2000, 2000, rng, p_cand=1.0, wide=True)
    frames.append((org, boxes, scores, cand))
    recs = [(o, b, s, c, _records(b, s, c, rng)) for o, b, s, c in frames]
    out, offs = _merge(recs)
    for f, (org, boxes, scores, cand, _) in enumerate(recs):
        a = offs[f]
        keep = _check_against_oracle(out["merged"][a:offs[f + 1]], out["det"][a * NQ:], out["det_tile"][a * NQ:], int(out["det_count"][f]),
                                     boxes, scores, cand, org)
        if f == 1:
            assert len(keep) * 2 >= int(cand.sum()) - 1 and len(keep) < int(cand.sum())


@pytest.mark.gpu
def test_tile_frames_u8_three_frames_bit_exact():
    from oracle import tiling_oracle as TO
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(15)
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(1500, 2300, 3), (700, 500, 3), (1100, 1024, 3)]]
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    orgs = [tiling.tile_origins(f.shape[0], f.shape[1]) for f in frames]
    rows = [(1, 0, 0), (0, *orgs[0][2]), (2, *orgs[2][1]), (0, *orgs[0][5]), (2, *orgs[2][0]), (0, -100, -50)]
    desc = np.zeros((3, 2), np.int64)
    for j, d in enumerate(dframes):
        desc[j, 0] = d.data_ptr()
        desc[j, 1] = np.array([d.shape[0], d.shape[1]], np.int32).view(np.int64)[0]
    desc_d = torch.from_numpy(desc).to(dev)
    tiles_d = torch.tensor(rows, dtype=torch.int32, device=dev)
    out = torch.empty((len(rows), 3, 1024, 1024), device=dev)
    N.check(N.lib().wm_tile_frames_u8(N.ptr(desc_d), 3, N.ptr(tiles_d), N.ptr(out), len(rows), N.stream_ptr(dev)))
    got = out.cpu().numpy()
    for i, (f, y, x) in enumerate(rows[:-1]):
        assert np.array_equal(got[i], TO.cut_tiles(frames[f], [(y, x)])[0]), i
    first = TO.cut_tiles(frames[0], [(0, 0)])[0]                                 # the tile reaching past the top-left corner
    assert not got[-1][:, :100, :].any() and not got[-1][:, :, :50].any()
    assert np.array_equal(got[-1][:, 100:, 50:], first[:, : 1024 - 100, : 1024 - 50])


@pytest.mark.gpu
def test_detect_frames_equals_detect_frame():
    """ViT-B fp16 survey at batch 4 over device and host frames, one above 80 tiles: every frame's result bit-identical to
    detect_frame on that frame alone; the large frame's merge equals the oracle merge of its per-tile records.  Tile counts
    (12, 1, 81, 5, 5) keep every batch of both paths at B = 1 or 4, sizes the engine's records are bit-identical across
    (B = 1, 4, 5, 16); at B = 2 the boxes differ from B = 4 in the last bits."""
    from oracle import tiling_oracle as TO
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.engine import split_records
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    m._hub.set_precision("fp16")
    rng = np.random.default_rng(16)
    shapes = [(2048, 3000), (600, 800), (7400, 8000), (1000, 4600), (1024, 4200)]
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    inputs = [torch.from_numpy(host[0]).to(dev), host[1], torch.from_numpy(host[2]), torch.from_numpy(host[3]).to(dev), host[4]]
    assert len(tiling.tile_origins(*shapes[2])) > 80
    results = list(tiling.detect_frames(m, iter(inputs), overlap=128, batch=4))
    assert len(results) == len(shapes)
    for i, (res, fr) in enumerate(zip(results, host)):
        want = tiling.detect_frame(m, torch.from_numpy(fr).to(dev), overlap=128, batch=4)
        assert set(res) == set(want)
        for k in want:
            assert res[k].dtype == want[k].dtype and res[k].device == want[k].device, (i, k)
            a, b = res[k].cpu(), want[k].cpu()
            if a.dtype == torch.float32:
                a, b = a.view(torch.int32), b.view(torch.int32)
            assert torch.equal(a, b), (i, k)
    org = tiling.tile_origins(*shapes[2])
    tiles = torch.from_numpy(TO.cut_tiles(host[2], org))
    rec = torch.cat([m.detect(tiles[i:i + 4].to(dev))["records"] for i in range(0, len(org), 4)]).cpu()
    r = split_records(rec)
    fb, keep = TO.merge(r["boxes"].numpy(), r["scores"].numpy(), ((r["flags"] & N.FLAG_NMS) != 0).numpy(), org, 0.4)
    assert len(keep) > 0
    np.testing.assert_array_equal(results[2]["boxes"].cpu().numpy(), fb[keep])
    np.testing.assert_array_equal(results[2]["tile"].cpu().numpy(), keep // NQ)
    m._hub.close()
