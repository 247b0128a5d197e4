"""Survey review chips (wm_chip_window, wm_crop_chips_u8, tiling.chip_windows / crop_chips, detect_frames(chips=...)).

CPU: the chip rule against a numpy-float32 restatement, the argument checks, and the test's own chip oracle --
oracle.pil_resize.resize_bilinear_u8 of the zero-padded crop -- pinned by what Pillow made (tests/golden/chips_pil.npz,
tools/gen_chips_golden.py).  GPU: the kernel against that oracle, bit for bit (every comparison is array_equal), with
frames and outputs inside larger allocations filled with 255 whose guard bytes must stay untouched, and detect_frames with
a stub model whose detections are certain."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle.pil_resize import resize_bilinear_u8
from survey_util import _StubModel, _animals, _guarded, _lib, _random_boxes
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling
from wildlifemapper_amd._survey import _frame_descs

F = np.float32


# ---- the rule and the oracle, restated -------------------------------------------------------------------------------

def _rule(boxes, context=1.5, min_side=32, max_side=1024):
    """The chip rule in numpy float32, every operation rounded on its own: (n,4) xyxy -> (n,3) int32 (y0, x0, side)."""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        x0, y0, x1, y1 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        ok = np.isfinite(b).all(axis=1)
        m = np.maximum((x1 - x0).astype(F), (y1 - y0).astype(F))
        s = np.ceil((m * F(context)).astype(F))
        s = np.minimum(np.maximum(s, F(min_side)), F(max_side))
        side = np.where(ok, s, 0).astype(np.int32)
        cx = ((x0 + x1).astype(F) * F(0.5)).astype(F)
        cy = ((y0 + y1).astype(F) * F(0.5)).astype(F)
        half = (F(0.5) * side.astype(F)).astype(F)
        lim = F(2.0 ** 30)
        wx = np.clip(np.floor((cx - half).astype(F)), -lim, lim)
        wy = np.clip(np.floor((cy - half).astype(F)), -lim, lim)
        wx = np.where(ok, wx, 0).astype(np.int64).astype(np.int32)
        wy = np.where(ok, wy, 0).astype(np.int64).astype(np.int32)
    return np.stack([wy, wx, side], axis=1)


def _zero_padded_crop(frame, window):
    y0, x0, side = (int(v) for v in window)
    out = np.zeros((side, side, 3), np.uint8)
    ya, yb = max(y0, 0), min(y0 + side, frame.shape[0])
    xa, xb = max(x0, 0), min(x0 + side, frame.shape[1])
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = frame[ya:yb, xa:xb]
    return out


def _oracle_chip(frame, window, S):
    if frame is None or window[2] <= 0:
        return np.zeros((S, S, 3), np.uint8)
    return resize_bilinear_u8(_zero_padded_crop(frame, window), S, S)


def _oracle_chips(frames, windows, box_frame, S):
    out = np.zeros((len(windows), S, S, 3), np.uint8)
    for i, w in enumerate(windows):
        f = int(box_frame[i])
        out[i] = _oracle_chip(frames[f] if 0 <= f < len(frames) else None, w, S)
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------

WORKED = [((10.2, 20.7, 30.9, 33.1), (10, 4, 32)), ((-5, -5, 3, 2), (-18, -17, 32)), ((0, 0, 5000, 10), (-507, 1988, 1024))]


def test_chip_window_rule():
    _lib()
    for box, want in WORKED:
        assert tuple(_rule([box])[0]) == want, box
        assert tuple(tiling.chip_windows(np.array([box], F))[0]) == want, box
    rng = np.random.default_rng(5)
    boxes = _random_boxes(rng, 10000, 0.01, far=True)
    got = tiling.chip_windows(boxes)
    assert got.shape == (10000, 3) and got.dtype == np.int32
    want = _rule(boxes)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]
    bad = ~np.isfinite(boxes).all(axis=1)
    assert bad.sum() >= 1000 and (got[bad] == 0).all() and (got[~bad, 2] >= 32).all() and (got[:, 2] <= 1024).all()
    assert (np.abs(got[:, :2].astype(np.int64)) == 2 ** 30).any()                                # the origin clamp was reached
    for ctx, lo, hi in [(1.0, 1, 1024), (8.0, 7, 300), (2.25, 64, 64)]:
        sub = boxes[::7]
        assert np.array_equal(tiling.chip_windows(sub, ctx, lo, hi), _rule(sub, ctx, lo, hi)), (ctx, lo, hi)
    assert tiling.chip_windows(np.zeros((0, 4), F)).shape == (0, 3)
    L = N.lib()
    box, out = (C.c_float * 4)(0, 0, 10, 10), (C.c_int32 * 3)()
    for args, msg in [((None, 1.5, 32, 1024, out), b"null"), ((box, 1.5, 32, 1024, None), b"null"), ((box, 0.99, 32, 1024, out), b"context"),
                      ((box, 8.5, 32, 1024, out), b"context"), ((box, float("nan"), 32, 1024, out), b"context"),
                      ((box, 1.5, 0, 1024, out), b"min_side"), ((box, 1.5, 33, 32, out), b"min_side"), ((box, 1.5, 32, 1025, out), b"min_side")]:
        assert L.wm_chip_window(*args) < 0, args
        assert msg in L.wm_last_error(), (args, L.wm_last_error())


def test_crop_chips_abi_rejects_bad_arguments():
    L = _lib()
    p = C.c_void_p(16)                  # never dereferenced: every call below fails validation before any HIP call
    good = dict(frames=p, nf=1, boxes=p, bf=p, n=3, chip=128, ctx=1.5, lo=32, hi=1024, chips=p, win=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.wm_crop_chips_u8(a["frames"], a["nf"], a["boxes"], a["bf"], a["n"], a["chip"], a["ctx"], a["lo"], a["hi"], a["chips"],
                                  a["win"], None)
    for kw, msg in [(dict(frames=None), b"null"), (dict(boxes=None), b"null"), (dict(chips=None), b"null"),
                    (dict(nf=0), b"n_frames"), (dict(nf=-2), b"n_frames"), (dict(n=-1), b"n -1"),
                    (dict(chip=12), b"chip 12"), (dict(chip=15), b"chip 15"), (dict(chip=18), b"chip 18"), (dict(chip=258), b"chip 258"),
                    (dict(chip=260), b"chip 260"), (dict(chip=0), b"chip 0"),
                    (dict(chips=C.c_void_p(18)), b"aligned"), (dict(chips=C.c_void_p(17)), b"aligned"),
                    (dict(ctx=0.5), b"context"), (dict(ctx=8.01), b"context"), (dict(ctx=float("nan")), b"context"),
                    (dict(ctx=float("inf")), b"context"),
                    (dict(lo=0), b"min_side"), (dict(lo=-4), b"min_side"), (dict(lo=65, hi=64), b"min_side"), (dict(hi=1025), b"min_side"),
                    (dict(lo=2000, hi=2000), b"min_side")]:
        assert call(**kw) < 0, kw
        assert msg in L.wm_last_error(), (kw, L.wm_last_error())
    # n == 0 returns 0 before it looks at any pointer or any other argument
    assert L.wm_crop_chips_u8(None, 0, None, None, 0, 128, 1.5, 32, 1024, None, None, None) == 0
    assert L.wm_crop_chips_u8(None, 0, None, None, 0, 7, 0.0, 0, 0, None, None, None) == 0


def test_detect_frames_rejects_bad_chips_before_device_work():
    _lib()
    frame = np.zeros((40, 60, 3), np.uint8)
    for bad in [0, 15, 18, 260, "x", 64.0, -128, True]:
        g = tiling.detect_frames(None, [frame], chips=bad)              # a generator: nothing runs before the first next()
        with pytest.raises(ValueError):
            next(g)
        with pytest.raises(ValueError):
            tiling.detect_frame(None, torch.from_numpy(frame), chips=bad)
    for kw in [dict(chip_context=0.5), dict(chip_context=9), dict(chip_context="x"), dict(chip_min_side=0), dict(chip_min_side=1025)]:
        with pytest.raises(ValueError):
            next(tiling.detect_frames(None, [frame], chips=64, **kw))


def _fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "chips_pil.npz"))
    context, min_side, max_side, S = fx["params"]
    return fx["frame"], fx["boxes"], fx["windows"], fx["chips"], float(context), int(min_side), int(max_side), int(S)


def test_oracle_reproduces_pillow_fixture(golden_dir):
    """The oracle the GPU tests compare against -- the numpy rule, then resize_bilinear_u8 of the zero-padded crop -- is what
    Pillow itself made of the same crops."""
    _lib()
    frame, boxes, windows, chips, context, min_side, max_side, S = _fixture(golden_dir)
    assert len(boxes) >= 16 and chips.shape == (len(boxes), S, S, 3)
    assert np.array_equal(_rule(boxes, context, min_side, max_side), windows)
    assert np.array_equal(tiling.chip_windows(boxes, context, min_side, max_side), windows)
    for i, w in enumerate(windows):
        assert np.array_equal(_oracle_chip(frame, w, S), chips[i]), (i, w)
    sides = set(windows[:, 2].tolist())
    assert 0 in sides and S in sides and min(sides - {0}) < S < max(sides)        # zero chip, identity, up and down


# ---- GPU -------------------------------------------------------------------------------------------------------------


def _crop(frames, boxes, box_frame, S, context, min_side, max_side, windows_out=True):
    """wm_crop_chips_u8 on numpy frames: every frame at an odd byte offset inside a 255-filled allocation, chips and
    windows inside 255-filled allocations whose guard bytes are checked.  Returns (chips, windows) as numpy arrays."""
    dev = torch.device("cuda:0")
    keep = [_guarded(f, 61 + 2 * j, dev) for j, f in enumerate(frames)]
    views = [v.view(f.shape) for (_, v), f in zip(keep, frames)]
    desc = _frame_descs(views, dev)
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=F)).to(dev)
    n = b.shape[0]
    bf = None if box_frame is None else torch.from_numpy(np.asarray(box_frame, dtype=np.int32)).to(dev)
    nc, nw = n * S * S * 3, n * 12
    cbuf = torch.full((nc + 128,), 255, dtype=torch.uint8, device=dev)
    wbuf = torch.full((nw + 128,), 255, dtype=torch.uint8, device=dev)
    N.check(N.lib().wm_crop_chips_u8(N.ptr(desc), len(frames), N.ptr(b), N.ptr(bf), n, S, context, min_side, max_side,
                                     C.c_void_p(cbuf.data_ptr() + 64), C.c_void_p(wbuf.data_ptr() + 64) if windows_out else None,
                                     N.stream_ptr(dev)))
    torch.cuda.synchronize()
    c, w = cbuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (c[:64] == 255).all() and (c[64 + nc:] == 255).all(), "wm_crop_chips_u8 wrote outside chips_dev"
    assert (w[:64] == 255).all() and (w[64 + nw:] == 255).all(), "wm_crop_chips_u8 wrote outside windows_dev"
    if not windows_out:
        assert (w == 255).all()
    for (buf, _), f in zip(keep, frames):                                    # the frames were only read
        assert int((buf != 255).sum().item()) == int((f != 255).sum()), "a frame's allocation changed"
    return c[64:64 + nc].reshape(n, S, S, 3), w[64:64 + nw].copy().view(np.int32).reshape(n, 3)


def _check(frames, boxes, box_frame, S, context, min_side, max_side, what):
    got, win = _crop(frames, boxes, box_frame, S, context, min_side, max_side)
    bf = np.zeros(len(boxes), np.int32) if box_frame is None else np.asarray(box_frame)
    want_win = _rule(boxes, context, min_side, max_side)
    want_win[(bf < 0) | (bf >= len(frames))] = 0
    assert np.array_equal(win, want_win), what
    want = _oracle_chips(frames, want_win, bf, S)
    if not np.array_equal(got, want):
        wrong = np.nonzero((got != want).reshape(len(boxes), -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(wrong)} of {len(boxes)} chips differ, first windows {want_win[wrong[:8]].tolist()}")
    return got, win


def _boxes_of_windows(windows):
    """Boxes with integer corners whose window under context 1, min_side 1 is exactly (y0, x0, side)."""
    w = np.asarray(windows, dtype=np.int64)
    y0, x0, side = w[:, 0], w[:, 1], w[:, 2]
    h = side - (np.arange(len(w)) % 3) * 2                                   # a height of the same parity, up to 4 less
    h = np.where(h >= 0, h, side)
    cy2 = 2 * y0 + side                                                      # twice the centre
    return np.stack([x0, (cy2 - h) // 2, x0 + side, (cy2 + h) // 2], axis=1).astype(F)


@pytest.mark.gpu
def test_chips_fixture_bit_exact_vs_pil(golden_dir):
    frame, boxes, windows, chips, context, min_side, max_side, S = _fixture(golden_dir)
    got, win = _crop([frame], boxes, None, S, context, min_side, max_side)
    assert np.array_equal(win, windows)
    for i in range(len(boxes)):
        assert np.array_equal(got[i], chips[i]), (i, windows[i])
    # the Python entry point, windows not asked for at the C level
    dev = torch.device("cuda:0")
    c2, w2 = tiling.crop_chips(torch.from_numpy(frame).to(dev), torch.from_numpy(boxes).to(dev), None, S, context, min_side, max_side)
    assert c2.shape == (len(boxes), S, S, 3) and c2.dtype == torch.uint8 and w2.dtype == torch.int32 and c2.is_cuda
    assert np.array_equal(c2.cpu().numpy(), chips) and np.array_equal(w2.cpu().numpy(), windows)
    got3, _ = _crop([frame], boxes, None, S, context, min_side, max_side, windows_out=False)
    assert np.array_equal(got3, chips)


@pytest.mark.gpu
def test_chips_geometry_sweep():
    """Every window side 1..300 in one launch at S = 32 (up from one pixel, the identity at 32, down by 9.4 with 21 taps),
    origins negative and past the far edges; then S = 128, 16 and 256 up to side 1024 on a frame larger than the windows."""
    rng = np.random.default_rng(11)
    H, W = 211, 307
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sides = np.arange(1, 301)
    kind = np.arange(300) % 6                # inside where it fits | off the top | bottom | left | right | anywhere, some wholly outside
    y0 = np.where(kind == 1, -rng.integers(0, sides), np.where(kind == 2, H - rng.integers(1, sides + 1), rng.integers(-sides + 1, H)))
    x0 = np.where(kind == 3, -rng.integers(0, sides), np.where(kind == 4, W - rng.integers(1, sides + 1), rng.integers(-sides + 1, W)))
    inside = (kind == 0) & (sides <= H)
    y0 = np.where(inside, rng.integers(0, np.maximum(H - sides, 0) + 1), y0)
    x0 = np.where(inside, rng.integers(0, np.maximum(W - sides, 0) + 1), x0)
    x0 = np.where((kind == 5) & (sides % 4 == 0), W + rng.integers(0, 40, 300), x0)             # past the far edge: zero chips
    windows = np.stack([y0, x0, sides], axis=1)
    boxes = _boxes_of_windows(windows)
    assert np.array_equal(_rule(boxes, 1.0, 1, 1024), windows)
    assert (x0 >= W).any() and (y0 < 0).any() and (x0 < 0).any() and (y0 + sides > H).any() and (x0 + sides > W).any() and inside.sum() >= 30
    _check([frame], boxes, None, 32, 1.0, 1, 1024, "sides 1..300 at S=32")

    H, W = 1100, 1150
    big = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for S, side_list in [(128, [1, 2, 127, 128, 129, 255, 256, 300, 512, 1024]), (16, [16, 256, 1024]), (256, [16, 256, 1024])]:
        wins = []
        for i, s in enumerate(side_list):
            wins.append((int(rng.integers(0, H - s + 1)), int(rng.integers(0, W - s + 1)), s))           # inside
            wins.append((H - s // 2 - 1, -(s // 3), s) if i % 2 else (-(s // 2), W - s // 3 - 1, s))       # off two edges
        wins = np.array(wins)
        boxes = _boxes_of_windows(wins)
        assert np.array_equal(_rule(boxes, 1.0, 1, 1024), wins)
        _check([big], boxes, None, S, 1.0, 1, 1024, f"S={S}")


@pytest.mark.gpu
def test_chips_many_frames_and_degenerate_boxes():
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in [(97, 131), (64, 33), (211, 307)]]      # odd row lengths
    S, ctx, lo, hi = 32, 1.5, 8, 1024
    boxes, bf = [], []
    for f, fr in enumerate(frames):
        H, W = fr.shape[:2]
        for _ in range(6):
            c = rng.random(2) * (W, H)
            wh = rng.random(2) * 60 + 1
            boxes.append((c[0] - wh[0] / 2, c[1] - wh[1] / 2, c[0] + wh[0] / 2, c[1] + wh[1] / 2))
            bf.append(f)
    special = len(boxes)
    boxes += [(np.nan, 1, 20, 20), (5, 5, 30, 30), (5, 5, 30, 30), (500, 500, 520, 520), (-0.5, 10.75, 33.5, 53.25), (1, 2, 3, np.inf)]
    bf += [0, -1, 3, 1, 1, 2]
    order = rng.permutation(len(boxes))                                       # mixed frame indices, not grouped by frame
    boxes, bf = np.array(boxes, dtype=F)[order], np.array(bf, dtype=np.int32)[order]
    got, win = _check(frames, boxes, bf, S, ctx, lo, hi, "three frames")
    pos = {int(o): i for i, o in enumerate(order)}
    for k in (0, 1, 2, 5):                                                     # NaN box, frame -1, frame 3, inf box
        assert (win[pos[special + k]] == 0).all() and (got[pos[special + k]] == 0).all(), k
    outside = pos[special + 3]                                                 # a window wholly outside frame 1
    assert tuple(win[outside]) == (495, 495, 30) and (got[outside] == 0).all()
    cover = pos[special + 4]                                                   # a window covering all of frame 1 (64 rows x 33 columns)
    assert tuple(win[cover]) == (0, -16, 64) and got[cover].any()
    # box_frame_dev = NULL with one frame is an explicit all-zero index
    b0 = boxes[bf == 2]
    a, wa = _crop([frames[2]], b0, None, S, ctx, lo, hi)
    b, wb = _crop([frames[2]], b0, np.zeros(len(b0), np.int32), S, ctx, lo, hi)
    assert np.array_equal(a, b) and np.array_equal(wa, wb)
    assert tiling.crop_chips(torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda:0"),
                             torch.zeros((0, 4), device="cuda:0"))[0].shape == (0, 128, 128, 3)


# ---- end to end with a stub model (survey_util._StubModel) -----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "fuse", "scale"])
def test_detect_frames_chips_with_stub_model(mode):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    S = 64
    if mode == "scale":
        sizes, kw, scale = [(1100, 1300), (1200, 1600)], dict(scale=0.5), 0.5
    else:
        sizes, kw, scale = [(1100, 1300), (600, 800)], (dict(fuse_thr=0.5) if mode == "fuse" else {}), 1.0
    src = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    frames = [torch.from_numpy(src[0]).to(dev), src[1]]                         # a device frame and a host frame
    tiled = [(int(h * scale), int(w * scale)) for h, w in sizes]
    animals = []
    for h, w in tiled:
        org = tiling.tile_origins(h, w)
        ys, xs = sorted({o[0] for o in org}), sorted({o[1] for o in org})
        animals.append(_animals(h, w, rng, ([y + 1024 for y in ys[:-1]] + ys[1:], [x + 1024 for x in xs[:-1]] + xs[1:])))
    plain = list(tiling.detect_frames(_StubModel(tiled, animals), frames, batch=4, **kw))
    with_chips = list(tiling.detect_frames(_StubModel(tiled, animals), frames, batch=4, chips=S, **kw))
    assert len(plain) == len(with_chips) == 2
    total = 0
    for f, (a, b) in enumerate(zip(plain, with_chips)):
        assert set(b) == set(a) | {"chips", "chip_windows", "chip_boxes"}
        for key in a:                                                           # every other key is bit-identical
            if isinstance(a[key], torch.Tensor):
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
                assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                                   b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), (f, key)
            else:
                assert a[key] == b[key], key
        boxes = b["boxes"].cpu().numpy()
        k = boxes.shape[0]
        total += k
        assert b["chips"].shape == (k, S, S, 3) and b["chips"].dtype == torch.uint8 and b["chips"].is_cuda
        assert b["chip_windows"].shape == (k, 3) and b["chip_windows"].dtype == torch.int32
        assert b["chip_boxes"].shape == (k, 4) and b["chip_boxes"].dtype == torch.float32
        win = _rule(boxes)
        assert np.array_equal(b["chip_windows"].cpu().numpy(), win), f
        got = b["chips"].cpu().numpy()
        for i in range(k):                                                      # cut from the SOURCE frame at the returned boxes
            assert np.array_equal(got[i], _oracle_chip(src[f], win[i], S)), (f, i, win[i])
        org = win[:, [1, 0, 1, 0]].astype(F)
        want_cb = ((boxes - org).astype(F) * (S / win[:, 2].astype(np.float64)).astype(F)[:, None]).astype(F)
        assert np.array_equal(b["chip_boxes"].cpu().numpy(), want_cb), f
        H, W = sizes[f]
        assert (win[:, 0] < 0).any() and (win[:, 1] < 0).any() and (win[:, 0] + win[:, 2] > H).any() and (win[:, 1] + win[:, 2] > W).any()
    assert total >= 12                  # a property of the table above, not of any weights
    if mode != "scale":                 # the first frame has seams: the seam animals came back once (fuse) or cut in parts (NMS)
        assert plain[0]["origins"].shape[0] == 4


@pytest.mark.gpu
def test_detect_frames_chips_without_detections():
    dev = torch.device("cuda:0")
    frame = torch.zeros((300, 500, 3), dtype=torch.uint8, device=dev)
    res = list(tiling.detect_frames(_StubModel([(300, 500)], [[]]), [frame], chips=32))
    assert len(res) == 1 and res[0]["boxes"].shape == (0, 4)
    assert res[0]["chips"].shape == (0, 32, 32, 3) and res[0]["chips"].dtype == torch.uint8
    assert res[0]["chip_windows"].shape == (0, 3) and res[0]["chip_boxes"].shape == (0, 4)
