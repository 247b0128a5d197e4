"""Times of the survey registration: the render (wm_register_render_u8) and both searches (wm_register_search, SAD, and
wm_register_search_zncc, the correlation) on the same planes, against the host route a caller had before.

  python tools/register_time.py [--reps 20] [--oracle-pairs 4] [--zncc-oracle-pairs 2] [--refine-oracle-pairs 2] [--only NAME]
      HIP-event min and median over --reps repetitions of one wm_register_render_u8 call with every frame of the chunk
      resident (one launch) and of one search call (one memset, the search launch, the pick launch) on ONE CHUNK of
      pairs, as tiling.register issues them (pair_chunk pairs at a time; buffers and frames are allocated once, outside
      the timed region).  The SAD search is timed in a run of its own (search_ms_*), and then, in the same process,
      --reps rounds of one SAD call and one correlation call, alternating, each between two HIP events (sad_ms_*,
      zncc_ms_*, and the ratio zncc / sad of the minima and of the medians).  The refinement's sums (wm_register_refine: one
      memset and one launch, one pass over the same planes, of which it uses the centre offset alone) are timed the same
      way, alternating with the SAD search (refine_ms_*, sad_beside_refine_ms_min and the ratio sad / refine of the minima);
      for the first --refine-oracle-pairs pairs they must equal tests/register_cases.py's refine_sums_oracle.
      Two settings, nadir frames of 400 x 600 px (20 x 30 m at 0.05 m) of random content at UTM-sized coordinates on
      flight lines with 55 % forward overlap and 30 % sidelap, a little jitter in position and heading, cell = 0.05 m:
        f40      F = 40 (4 lines of 10), side 256, search 16, pair_chunk 64;
        f1000    F = 1 000 (25 lines of 40), side 512, search 32, pair_chunk 256: about 4 pairs per frame.
      The searches' work is counted from the shapes: (2 S + 1)^2 * gx * gy cell pairs (byte differences) per pair of
      frames.  With the minimum time that is a rate, printed against the VALU bound of each inner loop: per 4 cells and
      offset SAD issues 7 vector instructions (two v_alignbyte_b32, three v_and_b32, v_sad_u8, v_bcnt_u32_b32), the
      correlation 11 (two v_alignbyte_b32, three v_and_b32, two v_sad_u8, three v_dot4_u32_u8, v_bcnt_u32_b32); 256 CUs
      x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-instructions per second (MI355X_MICROARCH: a wave64
      VALU instruction issues over 2 cycles on a SIMD-32), so 44.9e12 and 28.6e12 cell pairs per second.
      Each search is also timed with each of the offsets-per-thread variants K = 1, 2, 4 (WM_REGISTER_K; the result does
      not depend on K), alternating, twice, next to the default choice.
      For the first --oracle-pairs pairs of the chunk the wall clock of the numpy restatement of the SAD rule on the same
      input (tests/register_cases.py: register_oracle), whose planes, score table and best the device's must equal; it
      costs seconds per pair at the survey setting, so it runs on a sample and its time for the survey is the sample's
      mean per byte difference times the survey's byte differences.  For the first --zncc-oracle-pairs pairs the device's
      moments, best and peak must equal the restatement of the correlation rule (tests/register_cases.py:
      zncc_search_oracle, zncc_pick_oracle) on the device's planes, peak by its bytes.  The tool asserts both;
      equals_oracle is true where every comparison that ran held.
  python tools/register_time.py --only pyramid [--reps 20]
      The pyramid's reduce (wm_register_reduce_u8, one launch): HIP-event min and median of one call on stacks of 64 and 256
      planes of 512 x 512 (plane A of side 512) and 520 x 520 (plane B of side 512 at search 4) of random 1..255 at levels
      1, 3 and 6 -- 2^6 does not divide 520, so level 6 runs on 512 x 512 and on 640 x 640, the B plane of search 64 -- with
      the bytes it must move, n * ext^2 * (1 + 4^-level), as a rate and as a fraction of the 8 TB/s HBM peak (and 1 152
      planes of 512 x 512 at levels 1 and 3, 302 MB: the stacks above fit the 256 MiB Infinity Cache, this one does not), and
      the output compared with tests/pyramid_cases.py's reduce_oracle on the first two planes.  Then, on one chunk of 64 and of
      256 pairs of the f1000 survey at side 512 and search 4, in the same process and alternating: one
      wm_register_render_u8 call (which writes the very bytes the reduce reads), the reduce of both of its planes by 1 and
      by 2 (two launches), and one wm_register_refine call on the planes reduced by 2 (search 1, side 128) and on the
      fine ones; the ratios reduce / render and reduce / refine of the minima.  Last, end to end on test_register_pyramid's
      far-off scene: the wall clock of tiling.refine(levels=3, iters=3) against tiling.refine(levels=0, iters=12), twelve
      iterations each, the best of three after one warm-up.
      Prints one JSON line.  No figure is a pass mark: the numbers are records.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from wildlifemapper_amd import _native as N  # noqa: E402
from survey_bench_util import once, timed  # noqa: E402
from wildlifemapper_amd import tiling  # noqa: E402
from wildlifemapper_amd._survey import _frame_descs  # noqa: E402

H, W, GSD = 400, 600, 0.05
MIN_CELLS = 4096
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9          # lane-instructions per second
LOOP_VALU_PER_4_CELLS = {"sad": 7, "zncc": 11}


def make(lines, per_line, seed):
    rng = np.random.default_rng(seed)
    x0, y0 = 500000.1, 6000000.7
    dx, dy = W * GSD * 0.7, H * GSD * 0.45
    georef = np.stack([tiling.nadir_affine(H, W, (x0 + l * dx + rng.uniform(-0.5, 0.5), y0 + k * dy + rng.uniform(-0.5, 0.5)), GSD,
                                           rng.uniform(-3.0, 3.0)) for l in range(lines) for k in range(per_line)])
    return georef, np.tile(np.array([[H, W]], dtype=np.int32), (lines * per_line, 1))


def by_offsets_per_thread(call, reps):
    """Minimum time of `call` with K = 1, 2, 4 forced through WM_REGISTER_K, alternating, twice."""
    by_k = {}
    for rnd in range(2):
        for k in (1, 2, 4):
            os.environ["WM_REGISTER_K"] = str(k)
            by_k.setdefault(f"k{k}", []).append(timed(call, reps)[0])
    del os.environ["WM_REGISTER_K"]
    return by_k


def run(lines, per_line, side, search, pair_chunk, seed, reps, oracle_pairs, zncc_oracle_pairs, refine_oracle_pairs=2):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    georef, size = make(lines, per_line, seed)
    F = georef.shape[0]
    table = tiling.register_pairs(georef, size, GSD, search, side, MIN_CELLS)
    w1 = 2 * search + 1
    diffs_all = int((table["gx"].astype(np.int64) * table["gy"]).sum()) * w1 * w1
    chunk = table[:pair_chunk]
    n = chunk.shape[0]
    diffs = int((chunk["gx"].astype(np.int64) * chunk["gy"]).sum()) * w1 * w1
    needed = sorted(set(chunk["frame_a"].tolist()) | set(chunk["frame_b"].tolist()))
    gen = torch.Generator(device=dev).manual_seed(seed)
    pixels = torch.randint(0, 256, (len(needed), H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    frames = [pixels[k] for k in range(len(needed))]
    desc = _frame_descs(frames, dev)
    slot = np.full(F, -1, dtype=np.int32)
    slot[needed] = np.arange(len(needed), dtype=np.int32)
    g2p = tiling.ground_to_pixel(georef).reshape(-1, 6)
    g_d, s_d, slot_d = up(g2p), up(size), up(slot)
    pairs_d = up(chunk.view(np.uint8).reshape(n, 32))
    E = side + 2 * search
    a = torch.zeros((n, side, side), device=dev, dtype=torch.uint8)
    b = torch.zeros((n, E, E), device=dev, dtype=torch.uint8)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    score = torch.empty((n, w1, w1, 2), device=dev, dtype=torch.int32)
    best_sad = torch.empty((n, 8), device=dev, dtype=torch.int32)
    moments = torch.empty((n, w1, w1, 6), device=dev, dtype=torch.int64)
    best = torch.empty((n, 8), device=dev, dtype=torch.int32)
    peak = torch.empty((n, 2), device=dev, dtype=torch.float64)
    lib, st = N.lib(), N.stream_ptr(dev)
    render = lambda: N.check(lib.wm_register_render_u8(N.ptr(desc), len(needed), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, N.ptr(pairs_d), n, GSD,
                                                       search, side, N.ptr(a), N.ptr(b), N.ptr(status), st))
    sad = lambda: N.check(lib.wm_register_search(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, MIN_CELLS, N.ptr(score), N.ptr(best_sad), st))
    zncc = lambda: N.check(lib.wm_register_search_zncc(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, MIN_CELLS, N.ptr(moments),
                                                       N.ptr(best), N.ptr(peak), st))
    r_min, r_med = timed(render, reps)
    s_min, s_med = timed(sad, reps)
    rate = diffs / (s_min * 1e-3)
    bound = VALU_LANE_OPS / LOOP_VALU_PER_4_CELLS["sad"] * 4
    out = {"frames": F, "pairs": int(table.shape[0]), "pairs_per_frame": round(table.shape[0] / F, 2), "side": side, "search": search,
           "chunk_pairs": n, "chunk_frames": len(needed), "mean_patch_cells": int((chunk["gx"].astype(np.int64) * chunk["gy"]).mean()),
           "render_ms_min": r_min, "render_ms_median": r_med, "render_cells": n * (side * side + E * E),
           "search_ms_min": s_min, "search_ms_median": s_med, "search_byte_differences": diffs,
           "search_byte_differences_per_s": float(f"{rate:.4g}"), "valu_bound_byte_differences_per_s": float(f"{bound:.4g}"),
           "search_fraction_of_valu_bound": round(rate / bound, 4), "survey_byte_differences": diffs_all,
           "survey_search_s_at_this_rate": round(diffs_all / rate, 4), "render_status": int(status.item()), "cell_pairs": diffs}
    sad(), zncc()
    torch.cuda.synchronize()
    ms = {"sad": [], "zncc": []}
    for _ in range(reps):                                     # alternating, in one process
        ms["sad"].append(once(sad))
        ms["zncc"].append(once(zncc))
    a_min, a_med = float(np.min(ms["sad"])), float(np.median(ms["sad"]))
    z_min, z_med = float(np.min(ms["zncc"])), float(np.median(ms["zncc"]))
    rate, bound = diffs / (z_min * 1e-3), VALU_LANE_OPS / LOOP_VALU_PER_4_CELLS["zncc"] * 4
    out.update({"sad_ms_min": round(a_min, 4), "sad_ms_median": round(a_med, 4), "zncc_ms_min": round(z_min, 4), "zncc_ms_median": round(z_med, 4),
                "zncc_over_sad_min": round(z_min / a_min, 3), "zncc_over_sad_median": round(z_med / a_med, 3),
                "zncc_cell_pairs_per_s": float(f"{rate:.4g}"), "valu_bound_cell_pairs_per_s": float(f"{bound:.4g}"),
                "zncc_fraction_of_valu_bound": round(rate / bound, 4)})
    sums = torch.empty((n, N.REGISTER_REFINE_SUMS), device=dev, dtype=torch.int64)
    refine = lambda: N.check(lib.wm_register_refine(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, N.ptr(sums), st))
    sad(), refine()
    torch.cuda.synchronize()
    ms = {"sad": [], "refine": []}
    for _ in range(reps):                                     # alternating, in one process, on the same planes
        ms["sad"].append(once(sad))
        ms["refine"].append(once(refine))
    f_min, f_med, b_min = float(np.min(ms["refine"])), float(np.median(ms["refine"])), float(np.min(ms["sad"]))
    cells = diffs // (w1 * w1)
    out.update({"refine_ms_min": round(f_min, 4), "refine_ms_median": round(f_med, 4), "sad_beside_refine_ms_min": round(b_min, 4),
                "sad_over_refine_min": round(b_min / f_min, 1), "refine_cells": cells, "refine_cells_per_s": float(f"{cells / (f_min * 1e-3):.4g}"),
                "refine_plane_bytes_per_s": float(f"{n * (side * side + E * E) / (f_min * 1e-3):.4g}")})
    out["search_ms_min_by_offsets_per_thread"] = by_offsets_per_thread(sad, reps)
    out["zncc_ms_min_by_offsets_per_thread"] = by_offsets_per_thread(zncc, reps)
    sad(), zncc()
    torch.cuda.synchronize()
    equal = []
    if oracle_pairs > 0:
        from register_cases import register_oracle
        m = min(oracle_pairs, n)
        host = pixels.cpu().numpy()
        images = {f: host[k] for k, f in enumerate(needed)}
        t = time.perf_counter()
        want = register_oracle(g2p, size, images, chunk[:m], GSD, search, side, MIN_CELLS)
        took = time.perf_counter() - t
        sample = int((chunk["gx"][:m].astype(np.int64) * chunk["gy"][:m]).sum()) * w1 * w1
        out["oracle_pairs"], out["oracle_host_s"] = m, round(took, 2)
        out["oracle_host_s_for_the_survey_extrapolated"] = round(took / sample * diffs_all, 1)
        got_a, got_b = a[:m].cpu().numpy(), b[:m].cpu().numpy()
        got_s, got_best = score[:m].cpu().numpy(), best_sad[:m].cpu().numpy()
        equal.append(all(np.array_equal(got_a[p], want["a"][p]) and np.array_equal(got_b[p], want["b"][p]) and
                         np.array_equal(got_s[p], want["score"][p]) and np.array_equal(got_best[p], want["best"][p]) for p in range(m)))
        out["sad_equals_oracle"] = bool(equal[-1])
    if zncc_oracle_pairs > 0:
        from register_cases import same_bytes, zncc_pick_oracle, zncc_search_oracle
        m = min(zncc_oracle_pairs, n)
        A, B = a[:m].cpu().numpy(), b[:m].cpu().numpy()
        got_m, got_b, got_p = moments[:m].cpu().numpy(), best[:m].cpu().numpy(), peak[:m].cpu().numpy()
        t = time.perf_counter()
        ok = True
        for p in range(m):
            mo = zncc_search_oracle(A[p], B[p], int(chunk["gx"][p]), int(chunk["gy"][p]), search)
            wb, wp = zncc_pick_oracle(mo, search, MIN_CELLS)
            ok = ok and np.array_equal(got_m[p], mo) and np.array_equal(got_b[p], wb) and same_bytes(got_p[p], wp)
        equal.append(ok)
        out["zncc_oracle_pairs"], out["zncc_oracle_host_s"], out["zncc_equals_oracle"] = m, round(time.perf_counter() - t, 2), bool(ok)
        out["sampled_peaks_r"] = [round(float(np.sign(q) * np.sqrt(abs(q))), 4) for q in got_p[:, 0]]
    if refine_oracle_pairs > 0:
        from register_cases import refine_sums_oracle
        m = min(refine_oracle_pairs, n)
        refine()
        torch.cuda.synchronize()
        A, B, got = a[:m].cpu().numpy(), b[:m].cpu().numpy(), sums[:m].cpu().numpy()
        ok = all(got[p].tolist() == refine_sums_oracle(A[p], B[p], int(chunk["gx"][p]), int(chunk["gy"][p]), search) for p in range(m))
        equal.append(ok)
        out["refine_oracle_pairs"], out["refine_equals_oracle"] = m, bool(ok)
    if equal:
        out["equals_oracle"] = bool(all(equal))
        assert all(equal), "the device result differs from the oracle: sad %s, zncc %s" % (out.get("sad_equals_oracle"), out.get("zncc_equals_oracle"))
    return out


HBM_PEAK = 8.0e12                                  # bytes per second, MI355X


def run_pyramid(reps):
    from pyramid_cases import reduce_oracle
    from register_cases import CELL, SIDE, analytic_scene
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lib, st = N.lib(), N.stream_ptr(dev)
    out = {"stacks": {}, "beside_render_and_refine": {}}
    gen = torch.Generator(device=dev).manual_seed(5)
    equal = True
    shapes = ((512, (1, 3, 6)), (520, (1, 3)), (640, (6,)))
    for n, of in ((64, shapes), (256, shapes), (1152, ((512, (1, 3)),))):     # the last: 302 MB, past the 256 MiB Infinity Cache
        for ext, levels in of:
            src = torch.randint(1, 256, (n, ext, ext), device=dev, dtype=torch.uint8, generator=gen)
            src[:, ext // 3, ::7] = 0
            for level in levels:
                oe = ext >> level
                dst = torch.empty((n, oe, oe), device=dev, dtype=torch.uint8)
                call = lambda: N.check(lib.wm_register_reduce_u8(N.ptr(src), n, ext, level, N.ptr(dst), st))
                t_min, t_med = timed(call, reps, warmup=3)
                moved = n * ext * ext + n * oe * oe
                ok = bool(np.array_equal(dst[:2].cpu().numpy(), reduce_oracle(src[:2].cpu().numpy(), level)))
                equal = equal and ok
                out["stacks"][f"n{n}_ext{ext}_level{level}"] = {
                    "ms_min": t_min, "ms_median": t_med, "bytes": moved, "bytes_per_s": float(f"{moved / (t_min * 1e-3):.4g}"),
                    "fraction_of_hbm_peak": round(moved / (t_min * 1e-3) / HBM_PEAK, 4), "equals_oracle": ok}
            del src
    # the parent's kernels on the same chunk, in the same process
    side, search = 512, 4
    georef, size = make(25, 40, 1)
    F = georef.shape[0]
    table = tiling.register_pairs(georef, size, GSD, search, side, MIN_CELLS)
    g2p = tiling.ground_to_pixel(georef).reshape(-1, 6)
    for n in (64, 256):
        chunk = table[:n]
        needed = sorted(set(chunk["frame_a"].tolist()) | set(chunk["frame_b"].tolist()))
        pixels = torch.randint(0, 256, (len(needed), H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
        desc = _frame_descs([pixels[k] for k in range(len(needed))], dev)
        slot = np.full(F, -1, dtype=np.int32)
        slot[needed] = np.arange(len(needed), dtype=np.int32)
        g_d, s_d, slot_d = up(g2p), up(size), up(slot)
        pairs_d = up(chunk.view(np.uint8).reshape(n, 32))
        coarse = chunk.copy()
        coarse["gx"], coarse["gy"] = chunk["gx"] >> 2, chunk["gy"] >> 2
        coarse_d = up(coarse.view(np.uint8).reshape(n, 32))
        E = side + 2 * search
        a = torch.zeros((n, side, side), device=dev, dtype=torch.uint8)
        b = torch.zeros((n, E, E), device=dev, dtype=torch.uint8)
        ra = {l: torch.empty((n, side >> l, side >> l), device=dev, dtype=torch.uint8) for l in (1, 2)}
        rb = {l: torch.empty((n, E >> l, E >> l), device=dev, dtype=torch.uint8) for l in (1, 2)}
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        sums = torch.empty((n, N.REGISTER_REFINE_SUMS), device=dev, dtype=torch.int64)
        render = lambda: N.check(lib.wm_register_render_u8(N.ptr(desc), len(needed), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, N.ptr(pairs_d), n,
                                                           GSD, search, side, N.ptr(a), N.ptr(b), N.ptr(status), st))

        def reduce_both(l):
            N.check(lib.wm_register_reduce_u8(N.ptr(a), n, side, l, N.ptr(ra[l]), st))
            N.check(lib.wm_register_reduce_u8(N.ptr(b), n, E, l, N.ptr(rb[l]), st))

        calls = {"render": render, "reduce_by_1": lambda: reduce_both(1), "reduce_by_2": lambda: reduce_both(2),
                 "refine_fine": lambda: N.check(lib.wm_register_refine(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, N.ptr(sums), st)),
                 "refine_reduced_by_2": lambda: N.check(lib.wm_register_refine(N.ptr(ra[2]), N.ptr(rb[2]), N.ptr(coarse_d), n, 1, side >> 2,
                                                                                N.ptr(sums), st))}
        for c in calls.values():
            c(), c()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(reps):                                     # alternating, in one process, on the same chunk
            for k, c in calls.items():
                ms[k].append(once(c))
        mins = {k: float(np.min(v)) for k, v in ms.items()}
        rec = {f"{k}_ms_min": round(mins[k], 4) for k in calls}
        rec.update({f"{k}_ms_median": round(float(np.median(v)), 4) for k, v in ms.items()})
        rec.update({"chunk_frames": len(needed), "plane_bytes": n * (side * side + E * E), "render_status": int(status.item()),
                    "reduce_by_1_over_render": round(mins["reduce_by_1"] / mins["render"], 3),
                    "reduce_by_2_over_render": round(mins["reduce_by_2"] / mins["render"], 3),
                    "reduce_by_1_over_refine_fine": round(mins["reduce_by_1"] / mins["refine_fine"], 3),
                    "reduce_by_2_over_refine_fine": round(mins["reduce_by_2"] / mins["refine_fine"], 3)})
        ok = bool(np.array_equal(rb[2][:2].cpu().numpy(), reduce_oracle(b[:2].cpu().numpy(), 2)))
        equal = equal and ok
        rec["equals_oracle"] = ok
        out["beside_render_and_refine"][f"n{n}"] = rec
        del pixels, desc, a, b, ra, rb
    # end to end on the far-off scene of tests/test_register_pyramid.py (tests/register_cases.py: analytic_scene)
    frames, true, pert = analytic_scene("far")
    wall = {}
    for name, kw in (("levels3_iters3", {"levels": 3, "iters": 3}), ("levels0_iters12", {"levels": 0, "iters": 12})):
        took = []
        for _ in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            tiling.refine(frames, pert, CELL, side=SIDE, fixed=[0], **kw)
            took.append(time.perf_counter() - t)
        wall[name + "_s"] = round(min(took[1:]), 4)
    wall["pyramid_over_plain"] = round(wall["levels3_iters3_s"] / wall["levels0_iters12_s"], 3)
    out["end_to_end_far_scene"] = wall
    out["equals_oracle"] = equal
    assert equal, "the device result differs from reduce_oracle"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle-pairs", type=int, default=4)
    ap.add_argument("--zncc-oracle-pairs", type=int, default=2)
    ap.add_argument("--refine-oracle-pairs", type=int, default=2)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    settings = {"f40": (4, 10, 256, 16, 64), "f1000": (25, 40, 512, 32, 256)}
    out = {"reps": a.reps}
    for i, (name, (lines, per_line, side, search, chunk)) in enumerate(settings.items()):
        if a.only in (None, name):
            out[name] = run(lines, per_line, side, search, chunk, i, a.reps, a.oracle_pairs, a.zncc_oracle_pairs, a.refine_oracle_pairs)
    if a.only == "pyramid":                                       # asked for by name: the two settings above keep their output
        out["pyramid"] = run_pyramid(a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
