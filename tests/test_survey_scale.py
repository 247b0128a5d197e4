"""Survey detection at the model's training scale (tiling.detect_frame / detect_frames with scale= or resize=), ViT-B
fp16 on the GPU: every result equals the single-frame computation it stands for -- the N1 val-transform path at the
reference geometry, native tiling of the resampled frame above one tile, and model.detect with the tile's content
extent as target size.  Batches hold 1 or 4 tiles, sizes at which the engine's records are bit-identical."""
import numpy as np
import pytest
import torch

from survey_util import model  # noqa: F401 (a fixture)
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import preprocess, tiling

NQ = 51


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _one_tile_detections(model, x, w, h):
    """model.detect on one tile with target size (w, h), merged as a one-tile frame at origin (0, 0): detect_frame's keys."""
    from wildlifemapper_amd.engine import split_records
    dev = x.device
    rec = model.detect(x, torch.tensor([[w, h]], dtype=torch.float32, device=dev))["records"]
    merged = tiling.merge_tile_records(rec, torch.zeros((1, 2), dtype=torch.int32, device=dev), 0.4)
    r = split_records(merged)
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in r.items()}
    kept = torch.nonzero((flat["flags"] & N.FLAG_MERGED) != 0).flatten()
    kept = kept[torch.argsort(flat["nms_rank"][kept])]
    return {"boxes": flat["boxes"][kept], "scores": flat["scores"][kept], "labels": flat["labels"][kept],
            "tile": kept // NQ, "records": merged}


def _to_source(boxes, h, w, oh, ow):
    sx, sy = float(np.float32(w / ow)), float(np.float32(h / oh))
    out = torch.empty_like(boxes)
    out[:, 0::2] = boxes[:, 0::2] * sx
    out[:, 1::2] = boxes[:, 1::2] * sy
    return out


@pytest.mark.gpu
def test_detect_frames_reference_geometry_equals_val_transform_path(model):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    shapes = [(4000, 6000), (3648, 5472), (5525, 3690), (4000, 6000)]        # (H, W); the third is portrait
    host = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    inputs = [torch.from_numpy(host[0]).to(dev), host[1], torch.from_numpy(host[2]), torch.from_numpy(host[3]).to(dev)]
    results = list(tiling.detect_frames(model, iter(inputs), batch=4, resize=(768, 768)))
    assert len(results) == 4
    assert preprocess.resized_size(5525, 3690, 768, 768) == (768, 513)
    assert sum(r["boxes"].shape[0] for r in results) > 0
    for i, (res, f) in enumerate(zip(results, host)):
        h, w = shapes[i]
        oh, ow = preprocess.resized_size(h, w, 768, 768)
        assert res["resampled_size"] == (oh, ow)
        x = preprocess.tiles_from_u8(torch.from_numpy(f).to(dev)[None], resize=(768, 768))
        want = _one_tile_detections(model, x, ow, oh)
        assert _eq(res["boxes"], _to_source(want["boxes"], h, w, oh, ow)), i
        for k in ("scores", "labels", "tile", "records"):
            assert _eq(res[k], want[k]), (i, k)
        assert _eq(res["origins"], torch.zeros((1, 2), dtype=torch.int32, device=dev)), i


@pytest.mark.gpu
def test_scale_half_equals_native_tiling_of_resampled_frame(model):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(32)
    f = rng.integers(0, 256, (3000, 2400, 3), dtype=np.uint8)            # a 2400 x 3000 frame -> 1200 x 1500, 4 tiles
    oh, ow = preprocess.scaled_size(3000, 2400, 0.5)
    assert (oh, ow) == (1500, 1200) and len(tiling.tile_origins(oh, ow)) == 4
    native = tiling.detect_frame(model, preprocess.resample_u8(torch.from_numpy(f).to(dev), (oh, ow)), batch=4)
    for res in (tiling.detect_frame(model, torch.from_numpy(f).to(dev), batch=4, scale=0.5),
                next(tiling.detect_frames(model, [f], batch=4, scale=0.5))):
        assert res["resampled_size"] == (1500, 1200)
        for k in ("records", "origins", "tile", "scores", "labels"):
            assert _eq(res[k], native[k]), k
        assert _eq(res["boxes"], _to_source(native["boxes"], 3000, 2400, oh, ow))


@pytest.mark.gpu
def test_per_frame_scale_survey(model):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(33)
    # (H, W), scale, tiles after resampling: 4 + 1 + 1 + 4 + 1 + 1 = 12, three full batches of 4 in the survey
    spec = [((3000, 2400), 0.5, 4), ((600, 800), 1.0, 1), ((4000, 6000), 0.128, 1), ((1100, 1300), 1.0, 4),
            ((2000, 1800), 0.5, 1), ((700, 500), 1.0, 1)]
    host = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s, _, _ in spec]
    inputs = [torch.from_numpy(host[0]).to(dev), host[1], torch.from_numpy(host[2]), torch.from_numpy(host[3]).to(dev),
              torch.from_numpy(host[4]).to(dev), host[5]]
    calls = []

    def gsd(i, h, w):
        calls.append((i, h, w))
        return spec[i][1]
    results = list(tiling.detect_frames(model, iter(inputs), batch=4, scale=gsd))
    assert calls == [(i, *s) for i, (s, _, _) in enumerate(spec)]
    assert len(results) == len(spec) and sum(r["boxes"].shape[0] for r in results) > 0
    for i, (res, (shape, s, tiles)) in enumerate(zip(results, spec)):
        oh, ow = preprocess.scaled_size(*shape, s)
        assert res["resampled_size"] == (oh, ow) and res["origins"].shape[0] == tiles, i
        alone = next(tiling.detect_frames(model, [torch.from_numpy(host[i]).to(dev)], batch=4, scale=s))
        assert set(alone) == set(res)
        for k in res:
            if k != "resampled_size":
                assert _eq(res[k], alone[k]), (i, k)
    # scale 1.0 on a frame of at least one tile: the unscaled path, on every key the two share
    native = tiling.detect_frame(model, torch.from_numpy(host[3]).to(dev), batch=4)
    assert set(native) < set(results[3])
    for k in native:
        assert _eq(results[3][k], native[k]), k
    # scale 1.0 on a 600 x 800 frame: the tile's target size is its content, (w, h) = (800, 600)
    want = _one_tile_detections(model, preprocess.tiles_from_u8(torch.from_numpy(host[1]).to(dev)[None]), 800, 600)
    for k in want:
        assert _eq(results[1][k], want[k]), k
    # the 2000 x 1800 frame at 0.5 is 1000 x 900: not square, so width-first target sizes are told apart from height-first
    oh, ow = 1000, 900
    x = tiling.frame_to_tiles(preprocess.resample_u8(torch.from_numpy(host[4]).to(dev), (oh, ow)),
                              torch.zeros((1, 2), dtype=torch.int32, device=dev))
    want = _one_tile_detections(model, x, ow, oh)
    assert _eq(results[4]["records"], want["records"])
    assert _eq(results[4]["boxes"], _to_source(want["boxes"], 2000, 1800, oh, ow))
