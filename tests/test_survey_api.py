"""The survey API's public surface and its argument errors, pinned before tiling.py was split by concern.

CPU: every public name wildlifemapper_amd.tiling had before the split is still there and is the object of the module that
now holds it; and one table of calls with a bad argument, each with the exception type and the FULL message it raised.
The strings were recorded from the commit before the split (the parent of the one that added this file), not written by
hand: the validators behind them were merged, and the texts, the types and the order in which arguments are looked at
are behaviour that callers match on.  Every call raises before any device work, so the table runs without a GPU.
GPU: the one rule the box launches' shared validator is parametrised by -- crop_chips copies a strided frame, draw_boxes
refuses it because it draws in place -- and the one staging body of detect_frames, host route against device route."""
import numpy as np
import pytest
import torch

from survey_util import _StubModel
from wildlifemapper_amd import ground, registration, review
from wildlifemapper_amd import tiling as T

# ---- public surface --------------------------------------------------------------------------------------------------

SURFACE = {
    T: ["tile_origins", "frame_to_tiles", "merge_frames", "merge_tile_records", "resampled_size", "detect_frame", "SurveyBatch",
        "plan_batches", "detect_frames"],
    review: ["CHIP_MAX_SIDE", "chip_windows", "crop_chips", "DRAW_MAX_WIDTH", "DRAW_MAX_PALETTE", "OVERLAY_MIN", "OVERLAY_MAX",
             "DEFAULT_PALETTE", "outline_rects", "draw_boxes", "overlay_size"],
    ground: ["CENSUS_MAX_DETS", "CENSUS_CLASSES", "nadir_affine", "census", "COVERAGE_MAX_SIDE", "COVERAGE_MAX_CELLS",
             "COVERAGE_MAX_FRAMES", "ground_to_pixel", "footprint_bounds", "coverage", "MOSAIC_SAMPLES", "mosaic_plan",
             "resampled_georef", "mosaic"],
    registration: ["REGISTER_MAX_SIDE", "REGISTER_MAX_SEARCH", "REGISTER_MAX_PAIRS", "REGISTER_PAIR", "register_pairs", "adjust",
                   "REGISTER_METRICS", "register"],
}


@pytest.mark.parametrize("home,name", [(home, name) for home, names in SURFACE.items() for name in names],
                         ids=lambda v: v if isinstance(v, str) else v.__name__.rpartition(".")[2])
def test_tiling_keeps_its_public_names(home, name):
    assert getattr(T, name) is getattr(home, name)
    if callable(getattr(T, name)) and not isinstance(getattr(T, name), type):
        assert getattr(T, name).__module__ == home.__name__


def test_surface_is_whole_and_messages_that_name_tiling_stay_true():
    listed = [name for names in SURFACE.values() for name in names]
    assert len(listed) == len(set(listed)) == 42           # the public names tiling.py defined before the split
    with pytest.raises(ValueError, match=r"tiling\.REGISTER_PAIR"):
        T.register([], np.zeros((0, 2, 3)), 1.0, pairs=[])
    assert T.REGISTER_PAIR is registration.REGISTER_PAIR


# ---- argument errors -------------------------------------------------------------------------------------------------

G2 = np.array([[[1.0, 0, 0], [0, -1.0, 8]], [[1.0, 0, 4], [0, -1.0, 8]]])      # two 8 x 8 frames, 4 m apart
S2 = [(8, 8), (8, 8)]
FR2 = [np.zeros((8, 8, 3), np.uint8)] * 2
PTS = torch.zeros((2, 2), dtype=torch.float64)
LAB = torch.zeros(2, dtype=torch.int64)
CENSUS = {"points": PTS, "labels": LAB, "members": LAB}


def _survey(**kw):
    return lambda: next(T.detect_frames(None, [], **kw))


def _less(d, key):
    return {k: v for k, v in d.items() if k != key}


ERRORS = [
    # the eight scalar validators
    ('fuse_thr-text', lambda: T.merge_frames(None, None, None, fuse_thr="x"),
     ValueError, "merge_frames: fuse_thr 'x' is not a number"),
    ('fuse_thr-one', lambda: T.merge_frames(None, None, None, fuse_thr=1.0),
     ValueError, 'merge_frames: fuse_thr 1.0 must be in [0, 1) in fp32'),
    ('fuse_thr-rounds-to-one', lambda: T.merge_frames(None, None, None, fuse_thr=1.0 - 2.0 ** -30),
     ValueError, 'merge_frames: fuse_thr 0.9999999990686774 must be in [0, 1) in fp32'),
    ('fuse_thr-nan', _survey(fuse_thr=float("nan")),
     ValueError, 'detect_frames: fuse_thr nan must be in [0, 1) in fp32'),
    ('fuse_thr-negative', lambda: T.detect_frame(None, None, fuse_thr=-0.5),
     ValueError, 'detect_frames: fuse_thr -0.5 must be in [0, 1) in fp32'),
    ('scale-text', _survey(scale="a"),
     ValueError, "detect_frames: scale 'a' is not a number"),
    ('scale-zero', _survey(scale=0),
     ValueError, 'detect_frames: scale 0 must be positive and finite'),
    ('scale-inf', _survey(scale=float("inf")),
     ValueError, 'detect_frames: scale inf must be positive and finite'),
    ('scale-per-frame', lambda: T.resampled_size(3, 10, 10, scale=lambda i, h, w: -1.0),
     ValueError, 'frame 3: scale -1.0 must be positive and finite'),
    ('scale-per-frame-none', lambda: T.resampled_size(3, 10, 10, scale=lambda i, h, w: None),
     ValueError, 'frame 3: scale None is not a number'),
    ('chip-bool', lambda: T.crop_chips(None, None, chip=True),
     ValueError, 'crop_chips: chip size True is not an integer'),
    ('chip-float', lambda: T.crop_chips(None, None, chip=64.0),
     ValueError, 'crop_chips: chip size 64.0 is not an integer'),
    ('chip-not-multiple', lambda: T.crop_chips(None, None, chip=18),
     ValueError, 'crop_chips: chip size 18 must be a multiple of 4 in 16..256'),
    ('chip-small', lambda: T.crop_chips(None, None, chip=12),
     ValueError, 'crop_chips: chip size 12 must be a multiple of 4 in 16..256'),
    ('chip-large', _survey(chips=260),
     ValueError, 'detect_frames: chip size 260 must be a multiple of 4 in 16..256'),
    ('width-bool', lambda: T.draw_boxes(None, None, None, width=True),
     ValueError, 'draw_boxes: width True is not an integer'),
    ('width-float', lambda: T.draw_boxes(None, None, None, width=2.0),
     ValueError, 'draw_boxes: width 2.0 is not an integer'),
    ('width-zero', lambda: T.draw_boxes(None, None, None, width=0),
     ValueError, 'draw_boxes: width 0 must be in 1..16'),
    ('width-large', _survey(overlay=128, overlay_width=17),
     ValueError, 'detect_frames: width 17 must be in 1..16'),
    ('width-mosaic', lambda: T.mosaic(FR2, G2, 1.0, census=CENSUS, marker=3, width=0),
     ValueError, 'mosaic: width 0 must be in 1..16'),
    ('overlay-bool', _survey(overlay=True),
     ValueError, 'detect_frames: overlay size True is not an integer'),
    ('overlay-float', _survey(overlay=512.0),
     ValueError, 'detect_frames: overlay size 512.0 is not an integer'),
    ('overlay-small', _survey(overlay=63),
     ValueError, 'detect_frames: overlay size 63 must be in 64..8192'),
    ('overlay-large', _survey(overlay=8193),
     ValueError, 'detect_frames: overlay size 8193 must be in 64..8192'),
    ('radius-text', lambda: T.census([], [], "r"),
     ValueError, "census: radius 'r' is not a number"),
    ('radius-negative', lambda: T.census([], [], -1),
     ValueError, 'census: radius -1 must be finite and >= 0, with a finite square'),
    ('radius-nan', lambda: T.census([], [], float("nan")),
     ValueError, 'census: radius nan must be finite and >= 0, with a finite square'),
    ('radius-square-overflows', lambda: T.census([], [], 1e200),
     ValueError, 'census: radius 1e+200 must be finite and >= 0, with a finite square'),
    ('cell-text', lambda: T.footprint_bounds(G2, S2, "1"),
     ValueError, "footprint_bounds: cell '1' is not a number"),
    ('cell-none', lambda: T.footprint_bounds(G2, S2, None),
     ValueError, 'footprint_bounds: cell None is not a number'),
    ('cell-zero', lambda: T.coverage(G2, S2, 0),
     ValueError, 'coverage: cell 0 must be finite and > 0'),
    ('cell-nan', lambda: T.mosaic_plan(G2, S2, float("nan")),
     ValueError, 'mosaic_plan: cell nan must be finite and > 0'),
    ('cell-inf', lambda: T.register_pairs(G2, S2, float("inf")),
     ValueError, 'register_pairs: cell inf must be finite and > 0'),
    ('cell-register', lambda: T.register(FR2, G2, -1.0),
     ValueError, 'register: cell -1.0 must be finite and > 0'),
    ('chunk-zero', lambda: T.mosaic(FR2, G2, 1.0, chunk=0),
     ValueError, 'mosaic: chunk 0 must be a whole number >= 1'),
    ('chunk-fraction', lambda: T.mosaic(FR2, G2, 1.0, chunk=1.5),
     ValueError, 'mosaic: chunk 1.5 must be a whole number >= 1'),
    ('chunk-bool', lambda: T.mosaic(FR2, G2, 1.0, chunk=True),
     ValueError, 'mosaic: chunk True must be a whole number >= 1'),
    ('marker-zero', lambda: T.mosaic(FR2, G2, 1.0, census=CENSUS, marker=0),
     ValueError, 'mosaic: marker 0 must be a whole number >= 1'),
    ('search-negative', lambda: T.register_pairs(G2, S2, 1.0, search=-1),
     ValueError, 'register_pairs: search -1 must be a whole number >= 0'),
    ('side-zero', lambda: T.register_pairs(G2, S2, 1.0, side=0),
     ValueError, 'register_pairs: side 0 must be a whole number >= 1'),
    ('min_cells-text', lambda: T.register_pairs(G2, S2, 1.0, min_cells="4"),
     ValueError, "register_pairs: min_cells '4' must be a whole number >= 1"),
    ('pair_chunk-inf', lambda: T.register(FR2, G2, 1.0, pair_chunk=float("inf")),
     ValueError, 'register: pair_chunk inf must be a whole number >= 1'),
    ('n_frames-negative', lambda: T.adjust(-1, [], [], []),
     ValueError, 'adjust: n_frames -1 must be a whole number >= 0'),
    # register's min_corr and min_ratio
    ('min_corr-bool', lambda: T.register(FR2, G2, 1.0, min_corr=True),
     ValueError, 'register: min_corr True must be a finite number in [-1, 1)'),
    ('min_corr-text', lambda: T.register(FR2, G2, 1.0, min_corr="x"),
     ValueError, "register: min_corr 'x' must be a finite number in [-1, 1)"),
    ('min_corr-one', lambda: T.register(FR2, G2, 1.0, min_corr=1),
     ValueError, 'register: min_corr 1.0 must be a finite number in [-1, 1)'),
    ('min_corr-nan', lambda: T.register(FR2, G2, 1.0, min_corr=float("nan")),
     ValueError, 'register: min_corr nan must be a finite number in [-1, 1)'),
    ('min_ratio-text', lambda: T.register(FR2, G2, 1.0, min_ratio="x"),
     ValueError, "register: min_ratio 'x' must be a finite number >= 0"),
    ('min_ratio-none', lambda: T.register(FR2, G2, 1.0, min_ratio=None),
     ValueError, 'register: min_ratio None must be a finite number >= 0'),
    ('min_ratio-negative', lambda: T.register(FR2, G2, 1.0, min_ratio=-1),
     ValueError, 'register: min_ratio -1.0 must be a finite number >= 0'),
    ('min_ratio-inf', lambda: T.register(FR2, G2, 1.0, min_ratio=float("inf")),
     ValueError, 'register: min_ratio inf must be a finite number >= 0'),
    # the census dict, as coverage reads it and as mosaic reads it
    ('coverage-census-not-a-dict', lambda: T.coverage(G2, S2, 1.0, census=3),
     ValueError, "coverage: census has no 'points', 'labels' and 'members': pass the dict census() returned"),
    ('coverage-census-no-members', lambda: T.coverage(G2, S2, 1.0, census=_less(CENSUS, "members")),
     ValueError, "coverage: census has no 'points', 'labels' and 'members': pass the dict census() returned"),
    ('coverage-census-points-fp32', lambda: T.coverage(G2, S2, 1.0, census=dict(CENSUS, points=PTS.float())),
     ValueError, "coverage: census: expected 'points' (k,2) float64, 'labels' (k,) and 'members' (k,) tensors"),
    ('coverage-census-labels-short', lambda: T.coverage(G2, S2, 1.0, census=dict(CENSUS, labels=LAB[:1])),
     ValueError, "coverage: census: expected 'points' (k,2) float64, 'labels' (k,) and 'members' (k,) tensors"),
    ('coverage-census-members-list', lambda: T.coverage(G2, S2, 1.0, census=dict(CENSUS, members=[1, 1])),
     ValueError, "coverage: census: expected 'points' (k,2) float64, 'labels' (k,) and 'members' (k,) tensors"),
    ('coverage-census-too-many', lambda: T.coverage(G2, S2, 1.0, census={
        "points": torch.zeros((T.CENSUS_MAX_DETS + 1, 2), dtype=torch.float64),
        "labels": torch.zeros(T.CENSUS_MAX_DETS + 1, dtype=torch.int64),
        "members": torch.zeros(T.CENSUS_MAX_DETS + 1, dtype=torch.int64)}),
     ValueError, 'coverage: 262145 individuals exceed 262144'),
    ('coverage-census-other-device', lambda: T.coverage(G2, S2, 1.0, census=dict(CENSUS, members=LAB.to("meta"))),
     ValueError, 'coverage: census tensors are on different devices'),
    ('mosaic-census-not-a-dict', lambda: T.mosaic(FR2, G2, 1.0, census=3, marker=3),
     ValueError, "mosaic: census has no 'points' and 'labels': pass the dict census() returned"),
    ('mosaic-census-no-labels', lambda: T.mosaic(FR2, G2, 1.0, census=_less(CENSUS, "labels"), marker=3),
     ValueError, "mosaic: census has no 'points' and 'labels': pass the dict census() returned"),
    ('mosaic-census-points-fp32', lambda: T.mosaic(FR2, G2, 1.0, census=dict(CENSUS, points=PTS.float()), marker=3),
     ValueError, "mosaic: census: expected 'points' (k,2) float64 and 'labels' (k,) tensors on one device"),
    ('mosaic-census-labels-short', lambda: T.mosaic(FR2, G2, 1.0, census=dict(CENSUS, labels=LAB[:1]), marker=3),
     ValueError, "mosaic: census: expected 'points' (k,2) float64 and 'labels' (k,) tensors on one device"),
    ('mosaic-census-other-device', lambda: T.mosaic(FR2, G2, 1.0, census=dict(CENSUS, labels=LAB.to("meta")), marker=3),
     ValueError, "mosaic: census: expected 'points' (k,2) float64 and 'labels' (k,) tensors on one device"),
    # the box launches' frames, as far as a host without a device reaches
    ('crop_chips-no-frames', lambda: T.crop_chips([], None),
     RuntimeError, 'crop_chips: no frames'),
    ('crop_chips-frame-on-host', lambda: T.crop_chips(torch.zeros((8, 8, 3), dtype=torch.uint8), None),
     RuntimeError, 'crop_chips: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('crop_chips-frame-dtype', lambda: T.crop_chips([torch.zeros((8, 8, 3))], None),
     RuntimeError, 'crop_chips: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('crop_chips-frame-shape', lambda: T.crop_chips([torch.zeros((8, 8, 4), dtype=torch.uint8)], None),
     RuntimeError, 'crop_chips: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('crop_chips-frame-array', lambda: T.crop_chips([np.zeros((8, 8, 3), np.uint8)], None),
     RuntimeError, 'crop_chips: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('draw_boxes-no-frames', lambda: T.draw_boxes([], None, None),
     RuntimeError, 'draw_boxes: no frames'),
    ('draw_boxes-frame-on-host', lambda: T.draw_boxes(torch.zeros((8, 8, 3), dtype=torch.uint8), None, None),
     RuntimeError, 'draw_boxes: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('draw_boxes-frame-dtype', lambda: T.draw_boxes([torch.zeros((8, 8, 3))], None, None),
     RuntimeError, 'draw_boxes: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    ('draw_boxes-frame-shape', lambda: T.draw_boxes([torch.zeros((8, 8), dtype=torch.uint8)], None, None),
     RuntimeError, 'draw_boxes: frame 0: expected an (H,W,3) uint8 ROCm tensor'),
    # which error wins when several arguments are bad, in the order each public function validates them
    ('first-merge_frames', lambda: T.merge_frames(torch.zeros((1, 51, 8)), None, [0, 1], fuse_thr=2),
     ValueError, 'merge_frames: fuse_thr 2 must be in [0, 1) in fp32'),
    ('first-resampled_size', lambda: T.resampled_size(0, 10, 10, scale="a", resize=(0, 0)),
     RuntimeError, 'wm_hip: wm_resized_size: bad argument'),
    ('first-chip_windows', lambda: T.chip_windows([[0, 0, 1, 1]], context=9.0, min_side=0),
     ValueError, 'chip_windows: context 9.0 must be in [1, 8]'),
    ('first-crop_chips', lambda: T.crop_chips([], None, chip=18, context=0.5),
     ValueError, 'crop_chips: chip size 18 must be a multiple of 4 in 16..256'),
    ('first-crop_chips-frames', lambda: T.crop_chips([], None, context=0.5),
     ValueError, 'crop_chips: context 0.5 must be in [1, 8]'),
    ('first-draw_boxes', lambda: T.draw_boxes([], None, None, width=0, palette=np.zeros((2, 3))),
     ValueError, 'draw_boxes: width 0 must be in 1..16'),
    ('first-draw_boxes-frames', lambda: T.draw_boxes([], None, None, palette=np.zeros((2, 3))),
     ValueError, 'draw_boxes: palette must be a (P,3) uint8 table with P in 1..256, got float64 (2, 3)'),
    ('first-detect_frame', lambda: T.detect_frame(None, None, batch=0, scale=-1),
     ValueError, 'detect_frames: batch 0'),
    ('first-detect_frames-scale', _survey(scale=-1, fuse_thr=2),
     ValueError, 'detect_frames: scale -1 must be positive and finite'),
    ('first-detect_frames-fuse_thr', _survey(fuse_thr=2, chips=18),
     ValueError, 'detect_frames: fuse_thr 2 must be in [0, 1) in fp32'),
    ('first-detect_frames-chips', _survey(chips=18, overlay=1),
     ValueError, 'detect_frames: chip size 18 must be a multiple of 4 in 16..256'),
    ('first-detect_frames-chip-rule', _survey(chips=64, chip_context=0.5, overlay=1),
     ValueError, 'detect_frames: context 0.5 must be in [1, 8]'),
    ('first-detect_frames-overlay', _survey(overlay=1, overlay_width=0),
     ValueError, 'detect_frames: overlay size 1 must be in 64..8192'),
    ('first-detect_frames-width', _survey(overlay=128, overlay_width=0, overlay_palette=np.zeros((2, 3))),
     ValueError, 'detect_frames: width 0 must be in 1..16'),
    ('first-census', lambda: T.census([], np.zeros((1, 2, 2)), -1),
     ValueError, 'census: radius -1 must be finite and >= 0, with a finite square'),
    ('first-census-georef', lambda: T.census([{}], np.zeros((1, 2, 2)), 1.0),
     ValueError, 'census: georef of shape (1, 2, 2): expected (F, 2, 3)'),
    ('first-footprint_bounds', lambda: T.footprint_bounds(np.zeros((1, 2, 2)), [(8, 8, 8)], 0),
     ValueError, 'footprint_bounds: cell 0 must be finite and > 0'),
    ('first-footprint_bounds-georef', lambda: T.footprint_bounds(np.zeros((1, 2, 2)), [(8, 8, 8)], 1.0),
     ValueError, 'footprint_bounds: georef of shape (1, 2, 2): expected (F, 2, 3)'),
    ('first-coverage', lambda: T.coverage(G2, S2[:1], 0, census=3),
     ValueError, 'coverage: cell 0 must be finite and > 0'),
    ('first-coverage-sizes', lambda: T.coverage(G2, S2[:1], 1.0, census=3),
     ValueError, 'coverage: 1 sizes for 2 georeferences'),
    ('first-coverage-bounds', lambda: T.coverage(G2, S2, 1.0, census=3, bounds=(0, 0, 0, 1)),
     ValueError, 'coverage: bounds: a grid of 0 x 1 cells; gx and gy must be at least 1'),
    ('first-mosaic_plan', lambda: T.mosaic_plan(G2, S2, 1.0e-9, bounds=(0, 0, 1.5, 1)),
     ValueError, 'mosaic_plan: bounds (0, 0, 1.5, 1): expected (x0, y0, gx, gy), two numbers and two whole numbers'),
    ('first-mosaic', lambda: T.mosaic(FR2, G2, 0, sample="cubic", fill=(0, 0), chunk=0),
     ValueError, "mosaic: sample 'cubic' must be 'bilinear' or 'nearest'"),
    ('first-mosaic-fill', lambda: T.mosaic(FR2, G2, 0, fill=(0, 0), chunk=0),
     ValueError, 'mosaic: fill (0, 0) must be three whole numbers in 0..255'),
    ('first-mosaic-chunk', lambda: T.mosaic(FR2, G2, 0, chunk=0, marker=3),
     ValueError, 'mosaic: chunk 0 must be a whole number >= 1'),
    ('first-mosaic-marker', lambda: T.mosaic(FR2, G2, 0, marker=3),
     ValueError, 'mosaic: marker 3 and census go together: pass both (census= the dict census() returned) or neither'),
    ('first-mosaic-census', lambda: T.mosaic(iter(FR2), G2, 0, census=3, marker=0, width=0),
     ValueError, 'mosaic: marker 0 must be a whole number >= 1'),
    ('first-mosaic-width', lambda: T.mosaic(iter(FR2), G2, 0, census=3, marker=3, width=0, palette=np.zeros((2, 3))),
     ValueError, 'mosaic: width 0 must be in 1..16'),
    ('first-mosaic-palette', lambda: T.mosaic(iter(FR2), G2, 0, census=3, marker=3, palette=np.zeros((2, 3))),
     ValueError, 'mosaic: palette must be a (P,3) uint8 table with P in 1..256, got float64 (2, 3)'),
    ('first-mosaic-frames', lambda: T.mosaic(iter(FR2), G2, 0),
     ValueError, 'mosaic: frames must be a sequence that can be indexed (frames[i], len), got list_iterator'),
    ('first-mosaic-count', lambda: T.mosaic(FR2[:1], G2, 1.0, sizes=S2, bounds=(0, 0, 0, 1)),
     ValueError, 'mosaic: bounds: a grid of 0 x 1 cells; gx and gy must be at least 1'),
    ('first-resampled_georef', lambda: T.resampled_georef(np.zeros((2, 2)), (0, 8), (8, 0)),
     ValueError, 'resampled_georef: georef of shape (1, 2, 2): expected (F, 2, 3)'),
    ('first-resampled_georef-size', lambda: T.resampled_georef(G2, (0, 8), (8, 0)),
     ValueError, 'resampled_georef: size (0, 8): expected (height, width) or (2, 2), whole numbers >= 1'),
    ('first-register_pairs', lambda: T.register_pairs(G2, S2[:1], 0, search=-1),
     ValueError, 'register_pairs: cell 0 must be finite and > 0'),
    ('first-register_pairs-sizes', lambda: T.register_pairs(G2, S2[:1], 1.0, search=-1),
     ValueError, 'register_pairs: 1 sizes for 2 georeferences'),
    ('first-register_pairs-shape', lambda: T.register_pairs(G2, S2, 1.0, search=T.REGISTER_MAX_SEARCH + 1, side=T.REGISTER_MAX_SIDE + 1),
     ValueError, 'register_pairs: search 65 exceeds 64'),
    ('first-adjust', lambda: T.adjust(1.5, "pairs", [1], [-1.0]),
     ValueError, 'adjust: n_frames 1.5 must be a whole number >= 0'),
    ('first-adjust-pairs', lambda: T.adjust(2, [(0, 0)], [1], [-1.0]),
     ValueError, 'adjust: pairs: frame_a and frame_b must be two different frames in 0..1'),
    ('first-adjust-weights', lambda: T.adjust(2, [(0, 1)], [(1.0, 1.0)], [-1.0], fixed=[7]),
     ValueError, 'adjust: weights must be finite and >= 0'),
    ('first-register', lambda: T.register(iter(FR2), G2, 0, metric="ssd", min_corr=2, search=-1),
     ValueError, "register: metric 'ssd' must be one of ('sad', 'zncc')"),
    ('first-register-min_corr', lambda: T.register(iter(FR2), G2, 0, min_corr=2, search=-1),
     ValueError, 'register: min_corr 2.0 must be a finite number in [-1, 1)'),
    ('first-register-search', lambda: T.register(iter(FR2), G2, 0, search=-1, pair_chunk=0),
     ValueError, 'register: search -1 must be a whole number >= 0'),
    ('first-register-pair_chunk', lambda: T.register(iter(FR2), G2, 0, pair_chunk=T.REGISTER_MAX_PAIRS + 1, min_ratio=-1),
     ValueError, 'register: pair_chunk 65536 exceeds 65535'),
    ('first-register-min_ratio', lambda: T.register(iter(FR2), G2, 0, min_ratio=-1),
     ValueError, 'register: min_ratio -1.0 must be a finite number >= 0'),
    ('first-register-frames', lambda: T.register(iter(FR2), G2, 0),
     ValueError, 'register: frames must be a sequence that can be indexed (frames[i], len), got list_iterator'),
    ('first-register-pairs', lambda: T.register(FR2, G2, 1.0, pairs=[(0, 1)], fixed=[9]),
     ValueError, 'register: pairs must be a (P,) array of tiling.REGISTER_PAIR, as register_pairs returns it'),
    ('first-register-fixed', lambda: T.register(FR2, G2, 1.0, fixed=[9]),
     ValueError, 'adjust: fixed [9] must be frame indices in 0..1'),

]


@pytest.mark.parametrize("call,exc,message", [c[1:] for c in ERRORS], ids=[c[0] for c in ERRORS])
def test_argument_error_is_the_recorded_one(call, exc, message):
    import __graft_entry__ as g
    g.build()
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == message


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.gpu
def test_strided_frame_is_copied_by_crop_chips_and_refused_by_draw_boxes():
    dev = torch.device("cuda:0")
    big = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (48, 128, 3), dtype=np.uint8)).to(dev)
    view = big[:, ::2]
    assert tuple(view.shape) == (48, 64, 3) and not view.is_contiguous()
    boxes = torch.tensor([(5.0, 6.0, 25.0, 20.0), (30.5, 10.25, 44.0, 40.0), (55.0, 38.0, 75.0, 52.0)], device=dev)      # the last straddles two edges
    chips, windows = T.crop_chips(view, boxes, chip=16)
    want_chips, want_windows = T.crop_chips(view.contiguous(), boxes, chip=16)
    assert chips.shape == (3, 16, 16, 3) and torch.equal(chips, want_chips) and torch.equal(windows, want_windows)
    assert chips.any() and int(windows[2, 1] + windows[2, 2]) > 64 and int(windows[2, 0] + windows[2, 2]) > 48
    before = big.clone()
    with pytest.raises(RuntimeError, match="not contiguous"):
        T.draw_boxes(view, boxes, torch.zeros(3, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(big, before)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [None, 0.5])
def test_detect_frames_stages_host_and_device_frames_alike(scale):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(13)
    H, W = 40, 56
    src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    th, tw = (H, W) if scale is None else (int(H * scale), int(W * scale))
    animals = [[(2.0, 3.0, 14.0, 12.0), (float(tw - 9), float(th - 8), float(tw), float(th))]]
    kw = {} if scale is None else dict(scale=scale)
    host, device = (list(T.detect_frames(_StubModel([(th, tw)], animals), [fr], **kw)) for fr in (src, torch.from_numpy(src).to(dev)))
    assert len(host) == len(device) == 1
    a, b = host[0], device[0]
    assert set(a) == set(b) and ("resampled_size" in a) == (scale is not None)
    for key in ("boxes", "records", "origins"):
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and torch.equal(_bits(a[key]), _bits(b[key])), key
    assert a["boxes"].shape[0] == 2 and a["records"].shape == (1, 51, 8) and a["origins"].tolist() == [[0, 0]]
    if scale is not None:
        assert a["resampled_size"] == b["resampled_size"] == (th, tw)
