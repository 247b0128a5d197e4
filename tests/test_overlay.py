"""Survey overlays (wm_box_outline_rect, wm_draw_boxes_u8, wm_plot_image_u8, tiling.draw_boxes / outline_rects,
detect_frames(overlay=...), visualize.plot_points).

CPU: the outline rule restated in numpy with a sequential painter, pinned by what Pillow's ImageDraw.rectangle painted
(tests/golden/overlay_pil.npz, tools/gen_overlay_golden.py); wm_box_outline_rect against a numpy-float32 restatement; every
argument check; the plot image's numpy restatement on hand-worked values.  GPU: the kernels against those restatements, bit
for bit (every comparison is array_equal), frames inside larger allocations filled with 255 whose guard bytes must stay
untouched, and detect_frames with a stub model whose detections are certain."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle.pil_resize import resize_bilinear_u8
from survey_util import _StubModel, _animals, _guarded, _lib, _random_boxes
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling, visualize
from wildlifemapper_amd._survey import _frame_descs

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule, restated ----------------------------------------------------------------------------------------------

def _rects(boxes):
    """The rule's first step in numpy float32: (n,4) xyxy -> ((n,4) int64 (l, t, r, b), (n,) drawn)."""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    finite = np.isfinite(b).all(axis=1)
    with np.errstate(all="ignore"):
        c = np.clip(np.where(np.isfinite(b), b, 0), F(-2.0 ** 30), F(2.0 ** 30))
    r = np.trunc(c).astype(np.int64)
    drawn = finite & (r[:, 2] >= r[:, 0]) & (r[:, 3] >= r[:, 1])
    r[~drawn] = 0
    return r, drawn


def _paint_one(img, l, t, r, b, width, colour):
    """Every pixel of the frame inside [l, r] x [t, b] within `width` of one of the box's sides gets `colour`."""
    H, W = img.shape[:2]
    y0, y1, x0, x1 = max(t, 0), min(b, H - 1), max(l, 0), min(r, W - 1)
    if y0 > y1 or x0 > x1:
        return
    ys, xs = np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64)
    my = (ys - t < width) | (b - ys < width)
    mx = (xs - l < width) | (r - xs < width)
    img[y0:y1 + 1, x0:x1 + 1][my[:, None] | mx[None, :]] = colour


def _painter(frames, boxes, labels, box_frame, palette, width):
    """Draw the boxes one after another in index order onto copies of the frames."""
    out = [f.copy() for f in frames]
    rects, drawn = _rects(boxes)
    bf = np.zeros(len(rects), np.int64) if box_frame is None else np.asarray(box_frame)
    for i in range(len(rects)):
        if drawn[i] and 0 <= bf[i] < len(out) and 0 <= labels[i] < len(palette):
            _paint_one(out[int(bf[i])], *(int(v) for v in rects[i]), width, palette[int(labels[i])])
    return out


def _plot_ref(x):
    """visualize_prediction.py:120-124 in numpy: x (3,H,W) float32 -> (H,W,3) uint8."""
    a = np.asarray(x, dtype=F).transpose(1, 2, 0)[..., ::-1].copy()
    a -= a.min()
    if a.max() == 0:
        return np.zeros(a.shape, np.uint8)
    a /= a.max()
    v = np.int32(a * 255)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


# ---- CPU -------------------------------------------------------------------------------------------------------------

def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "overlay_pil.npz"))


def test_outline_rule_reproduces_pillow_fixture(golden_dir):
    fx = _fixture(golden_dir)
    H, W = (int(v) for v in fx["frame_hw"])
    rects, widths = fx["rects"], fx["widths"]
    masks = np.unpackbits(fx["masks"], axis=1)[:, :H * W].reshape(-1, H, W).astype(bool)
    assert len(rects) >= 1000 and set(widths.tolist()) == {1, 2, 3, 4, 5}
    sides = np.minimum(rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]) + 1
    assert (sides > widths).all() and (sides == widths + 1).any()           # every case Pillow-valid, the smallest included
    off = (rects[:, 0] >= W) | (rects[:, 2] < 0) | (rects[:, 1] >= H) | (rects[:, 3] < 0)
    assert off.any() and (rects[:, 0] < 0).any() and (rects[:, 1] < 0).any() and (rects[:, 2] >= W).any() and (rects[:, 3] >= H).any()
    for i, (rc, w) in enumerate(zip(rects, widths)):
        img = np.zeros((H, W), np.uint8)
        _paint_one(img, *(int(v) for v in rc), int(w), 1)
        assert np.array_equal(img.astype(bool), masks[i]), (i, rc, w)
        assert masks[i].any() != bool(off[i])
    # the painter's order: overlapping outlines, later over earlier
    scene, pal = fx["scene"], fx["scene_palette"]
    for k, w in enumerate(fx["scene_widths"]):
        got = _painter([scene], fx["scene_rects"].astype(F), fx["scene_labels"], None, pal, int(w))[0]
        assert np.array_equal(got, fx["scene_painted"][k]), w
    rev = _painter([scene], fx["scene_rects"][::-1].astype(F), fx["scene_labels"][::-1], None, pal, 2)[0]
    assert not np.array_equal(rev, fx["scene_painted"][0])


def test_outline_rule_stays_inside_small_boxes():
    """Sides <= width, where Pillow's line code paints outside the box: the rule fills the box and nothing else."""
    H, W = 20, 24
    n = 0
    for width in (1, 2, 3, 5, 16):
        for sw in range(1, width + 2):
            for sh in (1, 2, width, width + 1, 13):
                for l, t in [(5, 4), (0, 0), (-1, 3), (W - 1, H - 1), (W - sw + 1, 2), (W + 2, 3)]:
                    r, b = l + sw - 1, t + sh - 1
                    img = np.zeros((H, W), np.uint8)
                    _paint_one(img, l, t, r, b, width, 1)
                    box = np.zeros((H, W), bool)
                    box[max(t, 0):max(b + 1, 0), max(l, 0):max(r + 1, 0)] = True
                    assert not (img.astype(bool) & ~box).any(), (width, l, t, r, b)
                    if min(sw, sh) <= 2 * width:
                        assert np.array_equal(img.astype(bool), box), (width, l, t, r, b)
                    n += 1
    assert n > 500


WORKED = [((10.9, 20.2, 30.99, 33.0), (10, 20, 30, 33), True), ((-0.9, -1.5, 0.5, 2.7), (0, -1, 0, 2), True),
          ((5, 5, 4.5, 9), (0, 0, 0, 0), False), ((-3e9, -5, 3e9, 1e20), (-2 ** 30, -5, 2 ** 30, 2 ** 30), True),
          ((1, 2, float("nan"), 4), (0, 0, 0, 0), False), ((1, 2, float("inf"), 4), (0, 0, 0, 0), False), ((7.2, 7.9, 7.8, 7.1), (7, 7, 7, 7), True)]


def test_box_outline_rect_rule():
    L = _lib()
    for box, want, drawn in WORKED:
        r, d = _rects([box])
        assert tuple(r[0]) == want and bool(d[0]) == drawn, box
        r, d = tiling.outline_rects(np.array([box], F))
        assert tuple(r[0]) == want and bool(d[0]) == drawn, box
    rng = np.random.default_rng(6)
    boxes = _random_boxes(rng, 10000, 0.0003)
    got, drawn = tiling.outline_rects(boxes)
    assert got.shape == (10000, 4) and got.dtype == np.int32 and drawn.dtype == bool
    want, wdrawn = _rects(boxes)
    assert np.array_equal(drawn, wdrawn), np.nonzero(drawn != wdrawn)[0][:10]
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]
    assert (~drawn).sum() >= 1500 and drawn.sum() >= 5000 and (np.abs(got.astype(np.int64)) == 2 ** 30).any()
    assert tiling.outline_rects(np.zeros((0, 4), F))[0].shape == (0, 4)
    box, out = (C.c_float * 4)(0, 0, 10, 10), (C.c_int32 * 4)()
    assert L.wm_box_outline_rect(box, out) == 0 and list(out) == [0, 0, 10, 10]
    assert L.wm_box_outline_rect((C.c_float * 4)(3, 0, 2, 10), out) == 1 and list(out) == [0, 0, 0, 0]
    for args in [(None, out), (box, None)]:
        assert L.wm_box_outline_rect(*args) < 0 and b"null" in L.wm_last_error()


def test_overlay_abi_rejects_bad_arguments():
    L = _lib()
    p = C.c_void_p(16)                  # never dereferenced: every call below fails validation before any HIP call
    good = dict(frames=p, nf=1, boxes=p, labels=p, bf=p, n=3, pal=p, P=9, width=2)

    def draw(**kw):
        a = dict(good, **kw)
        return L.wm_draw_boxes_u8(a["frames"], a["nf"], a["boxes"], a["labels"], a["bf"], a["n"], a["pal"], a["P"], a["width"], None)
    for kw, msg in [(dict(frames=None), b"null"), (dict(boxes=None), b"null"), (dict(labels=None), b"null"), (dict(pal=None), b"null"),
                    (dict(nf=0), b"n_frames"), (dict(nf=-1), b"n_frames"), (dict(n=-1), b"n -1"),
                    (dict(width=0), b"width 0"), (dict(width=17), b"width 17"), (dict(width=-2), b"width -2"),
                    (dict(P=0), b"palette_size 0"), (dict(P=257), b"palette_size 257"), (dict(P=-1), b"palette_size -1")]:
        assert draw(**kw) < 0, kw
        assert msg in L.wm_last_error(), (kw, L.wm_last_error())
    assert L.wm_draw_boxes_u8(None, 0, None, None, None, 0, None, 0, 0, None) == 0       # n == 0: before any pointer or argument

    goodp = dict(inp=p, B=2, H=8, W=8, out=p, scratch=p, sb=2 * 1024)

    def plot(**kw):
        a = dict(goodp, **kw)
        return L.wm_plot_image_u8(a["inp"], a["B"], a["H"], a["W"], a["out"], a["scratch"], a["sb"], None)
    for kw, msg in [(dict(inp=None), b"null"), (dict(out=None), b"null"), (dict(scratch=None), b"null"), (dict(B=-1), b"batch -1"),
                    (dict(B=70000, sb=70000 * 1024), b"batch 70000"), (dict(H=0), b"height 0"), (dict(W=-3), b"width -3"),
                    (dict(sb=2047), b"scratch of 2047"), (dict(sb=0), b"scratch of 0"), (dict(inp=C.c_void_p(18)), b"aligned"),
                    (dict(scratch=C.c_void_p(17)), b"aligned")]:
        assert plot(**kw) < 0, kw
        assert msg in L.wm_last_error(), (kw, L.wm_last_error())
    assert L.wm_plot_image_u8(None, 0, 0, 0, None, None, 0, None) == 0                   # batch == 0


def test_overlay_python_rejects_bad_arguments_before_device_work():
    _lib()
    frame = np.zeros((40, 60, 3), np.uint8)
    for bad in [0, 63, 8193, "x", 1024.0, -512, True]:
        with pytest.raises(ValueError):
            next(tiling.detect_frames(None, [frame], overlay=bad))
        with pytest.raises(ValueError):
            tiling.detect_frame(None, torch.from_numpy(frame), overlay=bad)
    for kw in [dict(overlay_width=0), dict(overlay_width=17), dict(overlay_width=2.0), dict(overlay_width=True),
               dict(overlay_palette=np.zeros((3, 4), np.uint8)), dict(overlay_palette=np.zeros((0, 3), np.uint8)),
               dict(overlay_palette=np.zeros((257, 3), np.uint8)), dict(overlay_palette=np.zeros((9, 3), np.int32))]:
        with pytest.raises(ValueError):
            next(tiling.detect_frames(None, [frame], overlay=512, **kw))
    f, b, l = torch.from_numpy(frame), torch.zeros((1, 4)), torch.zeros(1, dtype=torch.int64)
    for kw in [dict(width=0), dict(width=17), dict(width="2"), dict(palette=np.zeros((2, 2), np.uint8)), dict(palette=[[0.5, 1, 2]])]:
        with pytest.raises(ValueError):
            tiling.draw_boxes(f, b, l, **kw)
    with pytest.raises(RuntimeError, match="ROCm"):
        tiling.draw_boxes(f, b, l)                                               # a host frame: there is no CPU path
    with pytest.raises(RuntimeError, match="no frames"):
        tiling.draw_boxes([], b, l)
    with pytest.raises(RuntimeError):
        visualize.plot_points(torch.zeros((3, 8, 8)), l, b)
    with pytest.raises(ValueError):
        visualize.plot_points(torch.zeros((3, 8, 8)), l, b, width=0)
    with pytest.raises(ValueError):
        visualize.visualize_predictions(None, None, [], "unused", sizes="tile")
    with pytest.raises(ValueError):
        visualize.save_plot("unused.jpg", np.zeros((4, 4), np.uint8))
    assert tiling.DEFAULT_PALETTE.shape == (9, 3) and tiling.DEFAULT_PALETTE.dtype == np.uint8
    assert len({tuple(c) for c in tiling.DEFAULT_PALETTE.tolist()}) == 9
    assert tiling.overlay_size(4000, 6000, 1536) == (1024, 1536) and tiling.overlay_size(600, 800, 1024) == (600, 800)


def test_overlay_symbols_agree():
    """The header, the library and the binding agree on the new symbols and constants."""
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    for name in ("wm_box_outline_rect", "wm_draw_boxes_u8", "wm_plot_image_u8"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in N.SYMBOLS and hasattr(L, name), name
    assert int(re.search(r"#define WM_ABI_VERSION (\d+)", hdr).group(1)) == N.ABI_VERSION == L.wm_abi_version() >= 12
    consts = {k: int(v) for k, v in re.findall(r"#define (WM_DRAW_MAX_WIDTH|WM_DRAW_MAX_PALETTE|WM_PLOT_SCRATCH_BYTES) (\d+)", hdr)}
    assert consts == {"WM_DRAW_MAX_WIDTH": tiling.DRAW_MAX_WIDTH, "WM_DRAW_MAX_PALETTE": tiling.DRAW_MAX_PALETTE,
                      "WM_PLOT_SCRATCH_BYTES": visualize.PLOT_SCRATCH_BYTES}


def test_plot_reference_on_hand_worked_values(tmp_path):
    # min -1, range 5: (v + 1) / 5 * 255 in fp32 = 51, 102, 153, 204, 255, 0; channels 0 and 2 change places
    x = np.array([[[0, 1]], [[2, 3]], [[4, -1]]], F)
    assert _plot_ref(x).tolist() == [[[255, 153, 51], [0, 204, 102]]]
    assert _plot_ref(np.full((3, 2, 2), 7.5, F)).tolist() == np.zeros((2, 2, 3), int).tolist()        # constant: zeros
    # truncation, not rounding: 0.999 * 255 = 254.7 -> 254
    assert _plot_ref(np.array([[[0.0]], [[0.999]], [[1.0]]], F)).tolist() == [[[255, 254, 0]]]
    # save_plot reverses the channels and writes what PIL reads back (PNG: lossless)
    pic = np.zeros((4, 5, 3), np.uint8)
    pic[..., 0], pic[..., 2] = 10, 200
    visualize.save_plot(str(tmp_path / "p.png"), torch.from_numpy(pic))
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "p.png"))), pic[..., ::-1])


# ---- GPU -------------------------------------------------------------------------------------------------------------


def _draw(frames, boxes, labels, box_frame, palette, width):
    """wm_draw_boxes_u8 on numpy frames, each at an odd byte offset inside a 255-filled allocation whose guard bytes are
    checked.  Returns the drawn frames as numpy arrays."""
    dev = torch.device("cuda:0")
    offs = [61 + 2 * j for j in range(len(frames))]
    keep = [_guarded(f, o, dev) for f, o in zip(frames, offs)]
    views = [v.view(f.shape) for (_, v), f in zip(keep, frames)]
    desc = _frame_descs(views, dev)
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=F).reshape(-1, 4)).to(dev)
    lab = torch.from_numpy(np.asarray(labels, dtype=np.int32)).to(dev)
    bf = None if box_frame is None else torch.from_numpy(np.asarray(box_frame, dtype=np.int32)).to(dev)
    pal = torch.from_numpy(np.ascontiguousarray(palette, dtype=np.uint8)).to(dev)
    N.check(N.lib().wm_draw_boxes_u8(N.ptr(desc), len(frames), N.ptr(b), N.ptr(lab), N.ptr(bf), b.shape[0], N.ptr(pal), len(palette),
                                     width, N.stream_ptr(dev)))
    torch.cuda.synchronize()
    out = []
    for (buf, _), f, o in zip(keep, frames, offs):
        h = buf.cpu().numpy()
        assert (h[:o] == 255).all() and (h[o + f.size:] == 255).all(), "wm_draw_boxes_u8 wrote outside a frame"
        out.append(h[o:o + f.size].reshape(f.shape))
    return out


PALETTE = np.array([(250, 10, 20), (10, 240, 30), (20, 30, 230), (200, 200, 0), (0, 200, 200), (1, 2, 3)], np.uint8)


def _case_boxes(H, W):
    """(box, label) pairs: interior, on and across each edge, off the frame, 1-pixel, small sides, inverted, non-finite, huge."""
    nan, inf = float("nan"), float("inf")
    return [((5.7, 6.2, 20.9, 18.1), 0), ((8, 9, 30, 25), 1),                                     # interior, overlapping
            ((0, 10, 12, 20), 2), ((14, 0, 26, 9), 3), ((W - 10, 5, W - 1, 15), 4), ((3, H - 8, 15, H - 1), 0),      # on each edge
            ((-4, 12, 6, 22), 1), ((18, -5, 28, 4), 2), ((W - 6, 20, W + 5, 30), 3), ((22, H - 5, 33, H + 7), 4),    # across each edge
            ((-6, -6, 5, 5), 5), ((W - 4, H - 4, W + 9, H + 9), 0),                               # across two corners
            ((W + 2, 3, W + 12, 9), 1), ((-20, 3, -2, 9), 2), ((4, -15, 9, -1), 3), ((4, H, 9, H + 5), 4),          # wholly off
            ((11.2, 13.9, 11.8, 13.1), 0), ((0.5, 0.5, 0.9, 0.9), 1), ((W - 1, H - 1, W - 1, H - 1), 2),            # 1 pixel
            ((30, 10, 31, 30), 3), ((12, 28, 34, 30), 4), ((2, 22, 6, 24), 5), ((16, 14, 31, 29), 2),               # sides <= width
            ((20, 5, 19, 9), 0), ((5, 20, 9, 19.5), 1), ((9, 9, 8.9, 8.9), 2),                    # r < l, b < t ((9,9,8,8) is inverted after truncation)
            ((nan, 1, 9, 9), 3), ((1, 1, inf, 9), 4), ((-inf, 1, 9, 9), 0),                       # not finite
            ((-1e30, -1e30, 1e30, 1e30), 1), ((-3e9, 7, 3e9, 11), 3), ((2, -2e10, 5, 2e10), 4),    # huge: around the frame, a band, a column
            ((-1e12, 16, 3, 1e12), 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2, 3, 5, 16])
def test_draw_boxes_cases(width):
    _lib()
    rng = np.random.default_rng(40 + width)
    shapes = [(37, 53), (64, 40)]
    frames = [rng.integers(0, 200, s + (3,), dtype=np.uint8) for s in shapes]
    boxes, labels, bf = [], [], []
    for f, (H, W) in enumerate(shapes):
        for b, l in _case_boxes(H, W):
            boxes.append(b), labels.append(l), bf.append(f)
    boxes += [(3, 3, 20, 20), (3, 3, 20, 20), (3, 3, 20, 20), (6, 6, 25, 25), (6, 6, 25, 25), (1, 1, 9, 9)]
    labels += [0, 1, 0, 6, -1, 2]                    # frame index out of range (twice), label out of range (twice), then drawn
    bf += [2, -1, 0, 0, 1, 0]
    order = rng.permutation(len(boxes))              # mixed frame indices, not grouped by frame
    boxes, labels, bf = np.array(boxes, F)[order], np.array(labels, np.int32)[order], np.array(bf, np.int32)[order]
    got = _draw(frames, boxes, labels, bf, PALETTE, width)
    want = _painter(frames, boxes, labels, bf, PALETTE, width)
    for f in range(2):
        assert np.array_equal(got[f], want[f]), (width, f, np.argwhere((got[f] != want[f]).any(axis=2))[:8].tolist())
        assert (got[f] != frames[f]).any()
    # box_frame = NULL is an explicit all-zero index; n = 0 draws nothing; the Python entry point draws the same
    b0, l0 = boxes[bf == 0], labels[bf == 0]
    a = _draw(frames[:1], b0, l0, None, PALETTE, width)[0]
    assert np.array_equal(a, _draw(frames[:1], b0, l0, np.zeros(len(b0), np.int32), PALETTE, width)[0])
    assert np.array_equal(a, _painter(frames[:1], b0, l0, None, PALETTE, width)[0])
    assert np.array_equal(_draw(frames, np.zeros((0, 4), F), np.zeros(0, np.int32), None, PALETTE, width)[0], frames[0])
    dev = torch.device("cuda:0")
    fr = [torch.from_numpy(f).to(dev) for f in frames]
    ret = tiling.draw_boxes(fr, torch.from_numpy(boxes).to(dev), torch.from_numpy(labels.astype(np.int64)).to(dev), bf, width, PALETTE)
    assert ret[0] is fr[0] and all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(fr, want))


@pytest.mark.gpu
def test_draw_boxes_painters_order():
    """Two overlapping outlines of different labels in both index orders, and identical boxes with different labels."""
    _lib()
    frame = np.full((37, 53, 3), 100, np.uint8)
    pair = np.array([(5, 5, 30, 25), (15, 12, 45, 33)], F)
    ab = _draw([frame], pair, [0, 1], None, PALETTE, 3)[0]
    ba = _draw([frame], pair[::-1], [1, 0], None, PALETTE, 3)[0]
    assert not np.array_equal(ab, ba)
    assert np.array_equal(ab, _painter([frame], pair, [0, 1], None, PALETTE, 3)[0])
    assert np.array_equal(ba, _painter([frame], pair[::-1], [1, 0], None, PALETTE, 3)[0])
    same = np.array([(8, 8, 28, 28)] * 3, F)
    for labels in ([0, 1, 2], [2, 1, 0], [1, 7, 0], [1, 0, 7]):                   # an out-of-range label in front of or behind the last
        got = _draw([frame], same, labels, None, PALETTE, 2)[0]
        assert np.array_equal(got, _painter([frame], same, labels, None, PALETTE, 2)[0]), labels
        last = [l for l in labels if l < len(PALETTE)][-1]
        assert tuple(got[8, 8]) == tuple(PALETTE[last])


@pytest.mark.gpu
def test_draw_boxes_order_at_scale(golden_dir):
    """3000 random boxes of 6 labels on one 256 x 256 frame, 3 more on a second frame: several LDS chunks of later boxes."""
    _lib()
    rng = np.random.default_rng(41)
    frames = [rng.integers(0, 200, (256, 256, 3), dtype=np.uint8), rng.integers(0, 200, (30, 44, 3), dtype=np.uint8)]
    c = rng.uniform(-10, 266, (3000, 2))
    wh = rng.uniform(0, 90, (3000, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F)
    labels = rng.integers(0, 6, 3000).astype(np.int32)
    bf = np.zeros(3000, np.int32)
    extra = np.array([(2, 2, 20, 20), (10, 8, 40, 28), (2, 2, 20, 20)], F)
    at = [100, 1500, 2999]
    boxes, labels, bf = np.insert(boxes, at, extra, axis=0), np.insert(labels, at, [3, 4, 5]), np.insert(bf, at, 1)
    want = _painter(frames, boxes, labels, bf, PALETTE, 2)
    got = _draw(frames, boxes, labels, bf, PALETTE, 2)
    again = _draw(frames, boxes, labels, bf, PALETTE, 2)
    for f in range(2):
        assert np.array_equal(got[f], want[f]), (f, int((got[f] != want[f]).any(axis=2).sum()))
        assert np.array_equal(got[f], again[f])
    # the fixture's scene: the kernel against Pillow itself
    fx = _fixture(golden_dir)
    for k, w in enumerate(fx["scene_widths"]):
        g = _draw([fx["scene"]], fx["scene_rects"].astype(F), fx["scene_labels"], None, fx["scene_palette"], int(w))[0]
        assert np.array_equal(g, fx["scene_painted"][k]), w


def _plot_inputs():
    rng = np.random.default_rng(42)
    a = rng.normal(0, 1.5, (3, 50, 70)).astype(F)                   # the minimum at the last element, the maximum at the first
    a[0, 0, 0], a[2, 49, 69] = 9.25, -7.5
    big = rng.normal(0.3, 1.0, (3, 1024, 1024)).astype(F)
    big[0, 0, 0], big[2, 1023, 1023] = 6.0, -6.5
    neg = -rng.random((3, 50, 70)).astype(F) * 40 - 3              # all negative
    const = np.full((3, 50, 70), -2.75, F)
    steps = (rng.integers(0, 256, (3, 50, 70)) / 255.0 * 51.0).astype(F)        # k / 5 of range 51: products on and around integers
    steps[1, 0, :2] = (0.0, 51.0)
    odd = rng.normal(0, 1, (3, 37, 53)).astype(F)                  # H * W odd: the unvectorised path
    return a, big, neg, const, steps, odd


@pytest.mark.gpu
def test_plot_image_bit_exact_vs_numpy():
    _lib()
    dev = torch.device("cuda:0")
    a, big, neg, const, steps, odd = _plot_inputs()
    assert np.argmin(a) == a.size - 1 and np.argmax(a) == 0 and np.argmin(big) == big.size - 1 and np.argmax(big) == 0
    assert neg.max() < 0
    s = _plot_ref(steps).astype(np.int64)
    q = ((steps.transpose(1, 2, 0)[..., ::-1] - steps.min()) / (steps.max() - steps.min())).astype(np.float64) * 255
    assert (np.abs(q - np.round(q)) < 1e-4).sum() > 1000 and s.max() == 255 and s.min() == 0     # many values on an integer boundary
    for name, x in [("a", a), ("big", big), ("neg", neg), ("const", const), ("steps", steps), ("odd", odd)]:
        got = visualize.plot_image(torch.from_numpy(x).to(dev))
        assert got.shape == x.shape[1:] + (3,) and got.dtype == torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), _plot_ref(x)), name
    assert not visualize.plot_image(torch.from_numpy(const).to(dev)).any()
    batch = np.stack([a, neg, const, steps])                         # different ranges, one launch pair
    got = visualize.plot_image(torch.from_numpy(batch).to(dev)).cpu().numpy()
    for j in range(4):
        assert np.array_equal(got[j], _plot_ref(batch[j])), j
    # output and scratch inside guarded allocations, the input at a 4-byte (not 16-byte) aligned address
    x = torch.from_numpy(np.concatenate([np.zeros(1, F), batch[:2].reshape(-1)])).to(dev)[1:]
    nout = 2 * 50 * 70 * 3
    obuf = torch.full((nout + 128,), 255, dtype=torch.uint8, device=dev)
    sbuf = torch.full((2 * 1024 + 128,), 255, dtype=torch.uint8, device=dev)
    N.check(N.lib().wm_plot_image_u8(N.ptr(x), 2, 50, 70, C.c_void_p(obuf.data_ptr() + 64), C.c_void_p(sbuf.data_ptr() + 64), 2 * 1024,
                                     N.stream_ptr(dev)))
    torch.cuda.synchronize()
    o, sc = obuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (o[:64] == 255).all() and (o[64 + nout:] == 255).all() and (sc[:64] == 255).all() and (sc[64 + 2048:] == 255).all()
    assert np.array_equal(o[64:64 + nout].reshape(2, 50, 70, 3), got[:2])


@pytest.mark.gpu
def test_plot_points_draws_on_the_prepared_image():
    _lib()
    dev = torch.device("cuda:0")
    a, _, neg, _, _, _ = _plot_inputs()
    boxes = [np.array([(3, 4, 30, 20), (10, 10, 69, 49), (-5, 30, 8, 60)], F), np.zeros((0, 4), F)]
    labels = [np.array([1, 8, 3]), np.zeros(0, np.int64)]
    pal = np.ascontiguousarray(tiling.DEFAULT_PALETTE[:, ::-1])
    one = visualize.plot_points(torch.from_numpy(a).to(dev), torch.from_numpy(labels[0]), boxes[0])
    want0 = _painter([_plot_ref(a)], boxes[0], labels[0], None, pal, 2)[0]
    assert np.array_equal(one.cpu().numpy(), want0)
    both = visualize.plot_points(torch.from_numpy(np.stack([a, neg])).to(dev), labels, boxes, width=3, palette=PALETTE)
    assert both.shape == (2, 50, 70, 3)
    assert np.array_equal(both[0].cpu().numpy(), _painter([_plot_ref(a)], boxes[0], labels[0], None, PALETTE, 3)[0])    # label 8: outside PALETTE
    assert np.array_equal(both[1].cpu().numpy(), _plot_ref(neg))


class _Nested:
    def __init__(self, tensors):
        self.tensors = tensors

    def to(self, device):
        return _Nested(self.tensors.to(device))


class _StubPost:
    """forward_with_nms of a post-processor: records the target sizes it is given, returns fixed detections."""

    def __init__(self):
        self.seen = []

    def forward_with_nms(self, outputs, target_sizes, score_threshold, iou_threshold):
        self.seen.append((target_sizes.cpu().tolist(), score_threshold, iou_threshold))
        dev = target_sizes.device
        return [{"scores": torch.tensor([0.9, 0.8], device=dev), "labels": torch.tensor([1, 4], device=dev),
                 "boxes": torch.tensor([[3.5, 4.0, 30.2, 20.9], [10, 10, 47, 39]], device=dev)}] * len(target_sizes)


class _StubNet:
    def eval(self):
        return self

    def __call__(self, image, boxes_np):
        assert boxes_np.tolist() == [[0, 0, 40, 48]] * image.tensors.shape[0]
        return {}


@pytest.mark.gpu
def test_visualize_predictions_loop(tmp_path):
    """The reference's loop with stubs for the model and the post-processor: one picture per batch, of its first image,
    named by image_id; max_steps; the target sizes of both sizes= modes; the picture is plot_points' (JPEG: size only)."""
    _lib()
    from PIL import Image
    rng = np.random.default_rng(44)
    batches = []
    for step in range(4):
        x = torch.from_numpy(rng.normal(0, 1, (2, 3, 40, 48)).astype(F))
        targets = [{"image_id": torch.tensor([100 + 2 * step + j]), "orig_size": torch.tensor([400, 600])} for j in range(2)]
        batches.append((_Nested(x), targets))
    post = _StubPost()
    paths = visualize.visualize_predictions(_StubNet(), {"bbox": post}, batches, str(tmp_path / "plots"), max_steps=3)
    assert [os.path.basename(p) for p in paths] == ["100.jpg", "102.jpg", "104.jpg"]
    assert post.seen == [([[400, 600], [400, 600]], 0.5, 0.4)] * 3
    assert all(Image.open(p).size == (48, 40) for p in paths)
    post2 = _StubPost()
    visualize.visualize_predictions(_StubNet(), {"bbox": post2}, batches[:1], str(tmp_path / "plots2"), threshold=0.3, iou_thr=0.6,
                                    sizes="canvas")
    assert post2.seen == [([[40, 48], [40, 48]], 0.3, 0.6)]
    res = post.forward_with_nms(None, torch.zeros((1, 2), device="cuda:0"), 0, 0)[0]
    pic = visualize.plot_points(batches[0][0].tensors[0].to("cuda:0"), res["labels"], res["boxes"])
    pal = np.ascontiguousarray(tiling.DEFAULT_PALETTE[:, ::-1])
    want = _painter([_plot_ref(batches[0][0].tensors[0].numpy())], res["boxes"].cpu().numpy(), [1, 4], None, pal, 2)[0]
    assert np.array_equal(pic.cpu().numpy(), want)


# ---- end to end with a stub model ------------------------------------------------------------------------------------

def _overlay_size(H, W, L):
    m = max(H, W)
    if m <= L:
        return H, W
    s = L / m
    return max(1, int(np.floor(H * s + 0.5))), max(1, int(np.floor(W * s + 0.5)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "fuse", "scale", "chips"])
def test_detect_frames_overlay_with_stub_model(mode):
    _lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(33)
    if mode == "scale":
        sizes, kw, scale, L = [(1100, 1300), (1200, 1600)], dict(scale=0.5), 0.5, 1400
    else:
        sizes, scale, L = [(1100, 1300), (600, 800)], 1.0, 1024
        kw = dict(fuse_thr=0.5) if mode == "fuse" else dict(chips=32) if mode == "chips" else {}
    src = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    frames = [torch.from_numpy(src[0]).to(dev), src[1]]                         # a device frame and a host frame
    tiled = [(int(h * scale), int(w * scale)) for h, w in sizes]
    animals = []
    for h, w in tiled:
        org = tiling.tile_origins(h, w)
        ys, xs = sorted({o[0] for o in org}), sorted({o[1] for o in org})
        animals.append(_animals(h, w, rng, ([y + 1024 for y in ys[:-1]] + ys[1:], [x + 1024 for x in xs[:-1]] + xs[1:])))
    plain = list(tiling.detect_frames(_StubModel(tiled, animals), frames, batch=4, **kw))
    pal = PALETTE if mode == "fuse" else None
    width = 3 if mode == "fuse" else 2
    okw = dict(overlay=L) if mode != "fuse" else dict(overlay=L, overlay_width=3, overlay_palette=PALETTE)
    with_ov = list(tiling.detect_frames(_StubModel(tiled, animals), frames, batch=4, **kw, **okw))
    assert len(plain) == len(with_ov) == 2
    resized = []
    for f, (a, b) in enumerate(zip(plain, with_ov)):
        assert "overlay" not in a and "overlay_boxes" not in a
        assert set(b) == set(a) | {"overlay", "overlay_boxes"}
        for key in a:                                                           # every other key is bit-identical
            if isinstance(a[key], torch.Tensor):
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
                assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                                   b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), (f, key)
            else:
                assert a[key] == b[key], key
        H, W = sizes[f]
        oh, ow = _overlay_size(H, W, L)
        resized.append((oh, ow) != (H, W))
        boxes = b["boxes"].cpu().numpy()
        k = boxes.shape[0]
        assert k >= 6
        assert b["overlay"].shape == (oh, ow, 3) and b["overlay"].dtype == torch.uint8 and b["overlay"].is_cuda
        want_ob = boxes.copy()
        want_ob[:, 0::2] = boxes[:, 0::2] * F(ow / W)
        want_ob[:, 1::2] = boxes[:, 1::2] * F(oh / H)
        ob = b["overlay_boxes"].cpu().numpy()
        assert ob.dtype == F and np.array_equal(ob, want_ob), f
        base = resize_bilinear_u8(src[f], oh, ow) if resized[-1] else src[f]
        labels = b["labels"].cpu().numpy()
        want = _painter([base], ob, labels, None, tiling.DEFAULT_PALETTE if pal is None else pal, width)[0]
        assert np.array_equal(b["overlay"].cpu().numpy(), want), (mode, f)
        assert (want != base).any()
        if isinstance(frames[f], torch.Tensor):                                  # the caller's frame was only read
            assert np.array_equal(frames[f].cpu().numpy(), src[f])
    assert resized == ([True, False] if mode != "scale" else [False, True])


@pytest.mark.gpu
def test_detect_frames_overlay_without_detections():
    _lib()
    dev = torch.device("cuda:0")
    frame = torch.full((300, 500, 3), 9, dtype=torch.uint8, device=dev)
    res = list(tiling.detect_frames(_StubModel([(300, 500)], [[]]), [frame], overlay=128))
    assert len(res) == 1 and res[0]["boxes"].shape == (0, 4) and res[0]["overlay_boxes"].shape == (0, 4)
    assert res[0]["overlay"].shape == (77, 128, 3) and (res[0]["overlay"] == 9).all()
    keys = set(next(tiling.detect_frames(_StubModel([(300, 500)], [[]]), [frame])))
    assert keys == {"boxes", "scores", "labels", "tile", "origins", "records"}       # overlay=None: exactly today's keys
