"""The folded-LayerNorm consumer GEMM with workgroups that walk several column tiles (csrc/gemm16_v5.h "Column walk").

Per tile the arithmetic, the accumulation order, the epilogue and the bytes written are those of one tile per workgroup; only which
workgroup computes a tile, and when, differs.  So every case runs wm_op_gemm16_folded_walk twice on the same buffers, with walk = 1 and
with walk = T, and asserts torch.equal on the whole 16-bit output, row-major and in LDS-image order.  The shapes are the smallest at
which each part can go wrong (two K-steps: the second tile's ring fill covers its whole K and lands in the LDS the last epilogue pass was
staged in; three: the ring wraps; K = 1280: the block shape's loop and four statistics tiles; two and nine row tiles; qkv's and lin1's
column counts).  The tile order (walk_tile_origin, csrc/gemm_common.h) is restated here in Python, checked on the host to visit every
tile once, and compared with the device's through a GEMM whose output shows which tile wrote where."""
import math

import pytest
import torch

import gpu_util as G
from wildlifemapper_amd import _native as N

BM, BN, GROUP_M = 256, 320, 8


# ---------------------------------------------------------------------------
# the tile order, restated (csrc/wm_common.h xcd_remap, csrc/gemm_common.h grouped_tile_origin / walk_tile_origin)
# ---------------------------------------------------------------------------
def xcd_remap(bid, nwg):
    q, r = nwg >> 3, nwg & 7
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def grouped_origin(tiles_m, tiles_n, wg, nwg, gm=GROUP_M):
    """(row tile, column tile) of workgroup wg among tiles_m x tiles_n."""
    t = xcd_remap(wg, nwg)
    per_group = gm * tiles_n
    group = t // per_group
    first_m = group * gm
    gsz = min(gm, tiles_m - first_m)
    in_group = t - group * per_group
    return first_m + in_group % gsz, in_group // gsz


def walk_tiles(tiles_m, tiles_n, walk, wg):
    """The (row tile, column tile) pairs workgroup wg of tiles_m * tiles_n / walk computes, in walk order."""
    nwg = tiles_m * tiles_n // walk
    row, slot = grouped_origin(tiles_m, tiles_n // walk, wg, nwg)
    return [(row, ((slot >> 2) * walk + t) * 4 + (slot & 3)) for t in range(walk)]


def walk_for(tiles_n, asked):
    """The launcher's fall-back (csrc/host_gemm.h gemm16_walk_for) for a T the caller names."""
    return 1 if asked > 1 and (tiles_n % 4 or (tiles_n // 4) % asked) else asked


@pytest.mark.parametrize("tiles_m,tiles_n,walk", [(1, 8, 2), (2, 12, 3), (9, 16, 2), (9, 16, 4), (256, 12, 3), (256, 16, 4)])
def test_walk_order_visits_every_tile_once(tiles_m, tiles_n, walk):
    assert walk_for(tiles_n, walk) == walk
    nwg = tiles_m * tiles_n // walk
    seen = {}
    for wg in range(nwg):
        tiles = walk_tiles(tiles_m, tiles_n, walk, wg)
        assert len({r for r, _ in tiles}) == 1                                  # a workgroup keeps its row tile
        assert [c for _, c in tiles] == [tiles[0][1] + 4 * t for t in range(walk)]   # and moves on by four column tiles
        for rc in tiles:
            assert rc not in seen, (rc, wg, seen[rc])
            seen[rc] = wg
    assert len(seen) == tiles_m * tiles_n and all(0 <= r < tiles_m and 0 <= c < tiles_n for r, c in seen)
    # at every step the 32 workgroups that share an XCD at a time (consecutive slots behind the XCD remap) cover 8 row tiles x 4
    # neighbouring column tiles, where the launch has whole groups of 8 row tiles
    if tiles_m % GROUP_M == 0:
        by_slot = sorted(range(nwg), key=lambda wg: xcd_remap(wg, nwg))
        for first in range(0, nwg - 31, 32):
            for t in range(walk):
                block = [walk_tiles(tiles_m, tiles_n, walk, wg)[t] for wg in by_slot[first:first + 32]]
                rows, cols = sorted({r for r, _ in block}), sorted({c for _, c in block})
                assert len(rows) == 8 and rows[-1] - rows[0] == 7 and len(cols) == 4 and cols[-1] - cols[0] == 3, (first, t, rows, cols)


def test_walk_one_is_the_grouped_order():
    for tiles_m, tiles_n in [(1, 8), (9, 16), (5, 6), (64, 12)]:
        nwg = tiles_m * tiles_n
        assert [walk_tiles(tiles_m, tiles_n, 1, wg) for wg in range(nwg)] == [[grouped_origin(tiles_m, tiles_n, wg, nwg)] for wg in range(nwg)]


def test_launcher_fallback_rule():
    assert [walk_for(6, t) for t in (1, 2, 3, 4)] == [1, 1, 1, 1]               # N = 1920: 6 column tiles, no block of 4 T
    assert [walk_for(8, t) for t in (1, 2, 3, 4)] == [1, 2, 1, 1]
    assert [walk_for(12, t) for t in (1, 2, 3, 4)] == [1, 1, 3, 1]
    assert [walk_for(16, t) for t in (1, 2, 3, 4)] == [1, 2, 1, 4]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _folded_walk(x16, wf, c1, c2, stats, act, prec, walk, out_packed=False):
    code, dt = G.PRECS[prec]
    M, K = x16.shape
    Nn = wf.shape[0]
    out = torch.full((M, Nn), float("nan"), device=x16.device, dtype=dt)          # an unwritten tile shows
    N.gemm_variant_counts(reset=True)
    N.check(N.lib().wm_op_gemm16_folded_walk(N.ptr(x16), N.ptr(wf), N.ptr(c1), N.ptr(c2), N.ptr(stats), 1e-6, N.ptr(out), M, Nn, K,
                                             act | (N.GEMM_OUT_PACKED if out_packed else 0), walk, code, G.sp()))
    torch.cuda.synchronize()
    return out, {k: v for k, v in N.gemm_variant_counts().items() if v}


_INPUTS = {}


@pytest.fixture(scope="module", autouse=True)
def _own_memory_pool():
    """This module's device buffers live in a memory pool of their own, released at its end: the blocks they would leave in the
    caching allocator's free lists change which addresses later modules' allocations get, and a module that relies on a freed and
    re-uploaded tensor coming back at its old address then reads something else."""
    if not torch.cuda.is_available():
        yield
        return
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    _INPUTS.clear()
    torch.cuda.synchronize()
    del pool


def _inputs(M, Nn, K, prec):
    """The folded GEMM's inputs as the existing tests build them: x16 and the row statistics from wm_op_ln_stats16 (a K shorter than a
    statistics tile is one tile: (mean, M2) over the row, in torch), the folded weight and c1 / c2 from wm_op_fold_weight16."""
    key = (M, Nn, K, prec)
    if key not in _INPUTS:
        dev = G.dev()
        g = torch.Generator(device=dev).manual_seed(1000 + M + Nn + K)
        x = torch.randn(M, K, device=dev, generator=g) * 1.5 + 0.3 * torch.randn(M, 1, device=dev, generator=g)
        if K >= 256:
            stats, x16 = G.ln_stats16(x, prec)
        else:
            mean = x.mean(1, keepdim=True)
            stats = torch.stack([mean[:, 0], ((x - mean) ** 2).sum(1)], 1).view(M, 1, 2).contiguous()
            x16 = G.pack16(G.to16(x, prec))
        w = G.to16(torch.randn(Nn, K, device=dev, generator=g) / math.sqrt(K), prec)
        gam = 1 + 0.2 * torch.randn(K, device=dev, generator=g)
        bet = 0.1 * torch.randn(K, device=dev, generator=g)
        bias = torch.randn(Nn, device=dev, generator=g)
        wf, c1, c2 = G.fold_weight16(w, gam, bet, bias, prec)
        c1 = c1 + torch.randn(Nn, device=dev, generator=g)                       # random c1 / c2: a tile that took another tile's shows
        c2 = c2 + torch.randn(Nn, device=dev, generator=g)
        _INPUTS.clear()                                                          # one shape's buffers at a time
        _INPUTS[key] = (x16, wf, c1.contiguous(), c2.contiguous(), stats)
    return _INPUTS[key]


SHAPES = [(256, 2560, 64, 2),        # one row tile, 8 column tiles, two K-steps: the second tile's fill is its whole K
          (256, 2560, 96, 2),        # three K-steps: the ring wraps, the counted waits of steps 0 and 1 take their two forms
          (256, 2560, 1280, 2),      # the block shape's K, four statistics tiles
          (512, 3840, 96, 3),        # qkv's column count, two row tiles
          (512, 3840, 96, 1),
          (2304, 5120, 64, 2),       # lin1's column count, 9 row tiles: the last group of the grouped order holds one
          (2304, 5120, 64, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,Nn,K,walk", SHAPES)
def test_walk_is_bit_identical_to_one_tile_per_workgroup(M, Nn, K, walk, act, prec):
    x16, wf, c1, c2, stats = _inputs(M, Nn, K, prec)
    want, v1 = _folded_walk(x16, wf, c1, c2, stats, act, prec, 1)
    got, vt = _folded_walk(x16, wf, c1, c2, stats, act, prec, walk)
    assert v1 == {"v5_320": 1}, v1
    assert vt == ({"v5_320": 1, "v5_320_walk": 1} if walk > 1 else {"v5_320": 1}), vt
    assert not torch.isnan(want.float()).any()
    assert torch.equal(got, want)
    want_p, _ = _folded_walk(x16, wf, c1, c2, stats, act, prec, 1, out_packed=True)
    got_p, _ = _folded_walk(x16, wf, c1, c2, stats, act, prec, walk, out_packed=True)
    assert torch.equal(got_p, want_p)
    assert torch.equal(G.unpack16_torch(want_p), want)


@pytest.mark.gpu
def test_walk_falls_back_where_t_does_not_divide_the_column_blocks():
    """N = 1920 is 6 column tiles: no T > 1 divides 6 / 4, the launch runs one tile per workgroup and counts as such."""
    x16, wf, c1, c2, stats = _inputs(256, 1920, 64, "fp16")
    want, v1 = _folded_walk(x16, wf, c1, c2, stats, 0, "fp16", 1)
    got, v4 = _folded_walk(x16, wf, c1, c2, stats, 0, "fp16", 4)
    assert v1 == {"v5_320": 1} and v4 == {"v5_320": 1}, (v1, v4)
    assert torch.equal(got, want) and not torch.isnan(want.float()).any()


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,walk", [(256, 2560, 2), (512, 3840, 3), (2304, 5120, 2), (2304, 5120, 4)])
def test_device_tile_order_is_the_restated_one(M, Nn, walk):
    """A has one non-zero row per row tile and W one non-zero row per column tile, so A W^T is non-zero in exactly one element of
    every tile, with a value that names the column tile; c1 = 0 and c2 carries the column tile's index.  The output, prefilled with
    NaN, then shows which operands the tile written at (row tile, column tile) was computed from: every tile the restated order lists
    is written, from its own A rows, W rows and c2, and nothing else is (a tile computed twice by the device would leave another one
    NaN)."""
    prec, K = "fp16", 64
    dev = G.dev()
    tiles_m, tiles_n = M // BM, Nn // BN
    a = torch.zeros(M, K, device=dev)
    w = torch.zeros(Nn, K, device=dev)
    for r in range(tiles_m):
        a[r * BM + 3 + r, :] = 1.0
    for c in range(tiles_n):
        w[c * BN + 5 + c, :] = 1.0 + c
    x16 = G.pack16(G.to16(a, prec))
    wf = G.pack16(G.to16(w, prec))
    # mean 0, M2 = K (rstd = 1 up to eps): out = acc + c2
    stats = torch.tensor([0.0, float(K)], device=dev).repeat(M, 1).view(M, 1, 2).contiguous()
    c1 = torch.zeros(Nn, device=dev)
    c2 = torch.arange(tiles_n, device=dev, dtype=torch.float32).repeat_interleave(BN).contiguous()
    got, var = _folded_walk(x16, wf, c1, c2, stats, 0, prec, walk)
    assert var == {"v5_320": 1, "v5_320_walk": 1}, var
    want = c2.repeat(M, 1)
    for r in range(tiles_m):
        for c in range(tiles_n):
            want[r * BM + 3 + r, c * BN + 5 + c] += K * (1.0 + c)
    assert torch.equal(got.float(), want)
    nwg = tiles_m * tiles_n // walk
    listed = sorted(rc for wg in range(nwg) for rc in walk_tiles(tiles_m, tiles_n, walk, wg))
    assert listed == [(r, c) for r in range(tiles_m) for c in range(tiles_n)]
