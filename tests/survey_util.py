"""What the survey tests share (chips, overlays, census, coverage, mosaic, registration, the survey front end): the built
library, guarded device buffers, generators of boxes, frames and per-tile records, and the stub model whose detections
are certain.  Checkers' inputs only: nothing here asserts."""
import os
import re
import socket

import numpy as np
import pytest
import torch

from wildlifemapper_amd import _native as N
from wildlifemapper_amd import tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NQ = 51
F = np.float32


def _lib():
    import __graft_entry__ as g
    g.build()
    return N.lib()


def _kernel_constants():
    src = open(os.path.join(ROOT, "wildlifemapper_amd", "csrc", "coverage_kernels.h")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    threads, rows = get("COV_THREADS"), get("COV_ROWS")
    return {"chunk": get("COV_CHUNK"), "block_x": get("COV_BLOCK_X"), "block_y": threads // 64 * rows}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(arr: np.ndarray, offset: int, dev):
    """A device copy of `arr` starting `offset` bytes into a larger uint8 allocation filled with 255."""
    flat = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.full((flat.size + 256,), 255, dtype=torch.uint8, device=dev)
    buf[offset:offset + flat.size] = torch.from_numpy(flat).to(dev)
    return buf, buf[offset:offset + flat.size]


class _Lazy:
    """A sequence that is only indexed, and records what was asked of it."""

    def __init__(self, items):
        self.items, self.asked = items, []

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.asked.append(i)
        return self.items[i]


def _random_boxes(rng, n, tiny, far=False):
    """(n,4) fp32 boxes, a twentieth each of: negative sizes, beyond +-2^30, overflowing, NaN, +inf, -inf, integer corners,
    scaled by `tiny`; then far: one corner, then the whole box, beyond 2^30 -- else: boxes of less than a pixel."""
    c = rng.normal(0, 3000, (n, 2))
    wh = np.abs(rng.normal(0, 120, (n, 2)))
    b = np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F)
    k = n // 20
    b[0 * k:1 * k, 2:] = b[0 * k:1 * k, :2] - rng.random((k, 2)).astype(F) * 50               # negative width and height
    b[1 * k:2 * k] *= F(1e6)                                                                   # huge, centre beyond +-2^30
    with np.errstate(over="ignore"):
        b[2 * k:3 * k] = (rng.normal(0, 1, (k, 4)) * 1e38).astype(F)                           # sums and differences overflow
    b[3 * k:4 * k, rng.integers(0, 4, k)] = np.nan
    b[4 * k:5 * k, rng.integers(0, 4, k)] = np.inf
    b[5 * k:6 * k, rng.integers(0, 4, k)] = -np.inf
    b[6 * k:7 * k] = np.round(b[6 * k:7 * k])                                                    # integers: centres on .0 and .5
    b[7 * k:8 * k] = b[7 * k:8 * k] * F(tiny)
    if far:
        b[8 * k:9 * k, :2] += F(3e9)                                                             # one corner beyond 2^30
        b[9 * k:10 * k] += F(-2.5e9)
    else:
        b[8 * k:9 * k, 2:] = b[8 * k:9 * k, :2] + rng.random((k, 2)).astype(F)                   # less than a pixel
    return b


# ---- frames on the ground: (ground -> pixel as 6 numbers or (2,3), height, width) ------------------------------------

def _axis(xw, xe, ys, yn, px):
    """An axis-aligned frame with footprint [xw, xe) x (ys, yn] m at px pixels per metre (exact for the binary fractions used)."""
    return ([px, 0, -px * xw, 0, -px, px * yn], int(round((yn - ys) * px)), int(round((xe - xw) * px)))


def _yawed(centre, gsd, yaw, H, W):
    return (tiling.ground_to_pixel(tiling.nadir_affine(H, W, centre, gsd, yaw)), H, W)


def _yawed_90():
    return _yawed((10.0, 20.0), 0.5, 90.0, 4, 8)         # up is east: 2 m east-west (9..11), 4 m north-south (18..22)


def _some_frames(gx, gy, cell, seed, n=5, shapes=((300, 400),)):
    """n yawed frames, frame k of shapes[k % len(shapes)], spread over the grid [0, gx * cell) x [0, gy * cell), each about
    a third of it."""
    rng = np.random.default_rng(seed)
    ex, ey = gx * cell, gy * cell
    side = max(ex, ey) / 3 + cell
    pick = lambda k: shapes[k % len(shapes)]
    return [_yawed((rng.uniform(0, ex), rng.uniform(0, ey)), side / max(pick(k)), rng.uniform(0, 360), *pick(k)) for k in range(n)]


# ---- per-tile records and the stub model -----------------------------------------------------------------------------

def _records(boxes, scores, cand, rng, other=N.FLAG_CONF, stray_bit=False):
    """(n,51,8) raw per-tile records on the host: candidates carry CONF | SCORE | NMS (stray_bit: and, at random, a bit no
    kernel defines), every other slot `other`; labels 0..6 and nms ranks -1..50 at random."""
    n = boxes.shape[0]
    rec = torch.zeros((n, NQ, 8), dtype=torch.float32)
    rec[..., 0:4] = torch.from_numpy(boxes)
    rec[..., 4] = torch.from_numpy(scores)
    ints = rec.view(torch.int32)
    ints[..., 5] = torch.from_numpy(rng.integers(0, 7, (n, NQ)).astype(np.int32))
    stray = rng.integers(0, 2, cand.shape) * 16 if stray_bit else 0
    ints[..., 6] = torch.from_numpy(np.where(cand, N.FLAG_CONF | N.FLAG_SCORE | N.FLAG_NMS | stray, other).astype(np.int32))
    ints[..., 7] = torch.from_numpy(rng.integers(-1, 51, (n, NQ)).astype(np.int32))
    return rec


class _StubModel:
    """detect() hands out hand-built per-tile records in the order detect_frames asks for tiles: frame by frame, tile by
    tile.  An animal is a box in frame pixels; every tile that sees at least 6 px of it reports the part it sees, in tile
    pixels, as a candidate."""

    def __init__(self, tiled_sizes, animals, overlap=128):
        rng = np.random.default_rng(3)
        recs = []
        for (h, w), boxes in zip(tiled_sizes, animals):
            for oy, ox in tiling.tile_origins(h, w, 1024, overlap):
                b = np.zeros((NQ, 4), F)
                score = (rng.random(NQ) * 0.5).astype(F)
                cand = np.zeros(NQ, bool)
                q = 0
                for (x0, y0, x1, y1) in boxes:
                    vx0, vy0 = max(x0, ox), max(y0, oy)
                    vx1, vy1 = min(x1, ox + 1024, w), min(y1, oy + 1024, h)
                    if vx1 - vx0 >= 6 and vy1 - vy0 >= 6:
                        b[q] = (vx0 - ox, vy0 - oy, vx1 - ox, vy1 - oy)
                        score[q] = F(0.5 + 0.5 * rng.random())
                        cand[q] = True
                        q += 3
                recs.append((b, score, cand))
        self.records = _records(*(np.stack([r[k] for r in recs]) for k in range(3)), rng).to(DEV)
        self.pos = 0

    def detect(self, x, target_sizes=None):
        n = x.shape[0]
        assert self.pos + n <= self.records.shape[0]
        out = self.records[self.pos:self.pos + n]
        self.pos += n
        return {"records": out}


def _animals(h, w, rng, seams):
    """Boxes in frame pixels: on each frame border, in each corner, across the tile seams, and a few inside."""
    a = [(0, 40, 30, 75), (w - 25, 60, w, 100), (200, 0, 260, 22), (300, h - 18, 345, h), (0, 0, 28, 24), (w - 31, h - 27, w, h)]
    for sx in seams[1]:
        a.append((sx - 35, 300, sx + 45, 352))                                 # cut by a vertical seam
    for sy in seams[0]:
        a.append((420, sy - 30, 470, sy + 50))                                 # cut by a horizontal seam
    for _ in range(4):
        cx, cy = rng.integers(60, w - 60), rng.integers(120, h - 60)
        a.append((cx - 20, cy - 14, cx + 23, cy + 19))
    return [tuple(float(v) for v in b) for b in a]


@pytest.fixture(scope="module")
def model():
    """ViT-B with synthetic weights in fp16 mode, one per test module that imports this fixture."""
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    m._hub.set_precision("fp16")
    yield m
    m._hub.close()
