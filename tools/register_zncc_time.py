"""Times of the correlation search (wm_register_search_zncc) next to the SAD search (wm_register_search) on the same planes.

  python tools/register_zncc_time.py [--reps 20] [--oracle-pairs 2] [--only NAME]
      The two settings, frames and chunks of tools/register_time.py (f40: F = 40, side 256, search 16, 64 pairs; f1000:
      F = 1 000, side 512, search 32, 256 pairs), rendered once by wm_register_render_u8.  Then, in one process, --reps
      rounds of one wm_register_search call and one wm_register_search_zncc call, alternating, each between two HIP
      events (a call is its memset, the search launch and the pick launch; buffers are allocated once, outside the
      timed region): min and median of each and the ratio zncc / sad of the minima and of the medians.
      The correlation search is also timed with each of the offsets-per-thread variants K = 1, 2, 4 (WM_REGISTER_K; the
      result does not depend on K), alternating, twice, next to the default choice.
      Work is counted from the shapes, (2 S + 1)^2 * gx * gy cell pairs per pair of frames, and the rate is printed against
      the VALU bound of the new inner loop, counted as tools/register_time.py counts the SAD loop's: 11 vector
      instructions per 4 cells and offset (two v_alignbyte_b32, three v_and_b32, two v_sad_u8, three v_dot4_u32_u8,
      v_bcnt_u32_b32) against 78.6e12 lane-instructions per second, so 28.6e12 cell pairs per second.
      For the first --oracle-pairs pairs of the chunk the device's moments, best and peak must equal the numpy restatement
      of the rule (tests/test_register_zncc.py: zncc_search_oracle, zncc_pick_oracle) on the device's planes, peak by its
      bytes; the tool asserts it.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from wildlifemapper_amd import _native as N  # noqa: E402
from wildlifemapper_amd import tiling  # noqa: E402
from register_time import GSD, H, VALU_LANE_OPS, W, make, timed  # noqa: E402

LOOP_VALU_PER_4_CELLS = 11
MIN_CELLS = 4096


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(lines, per_line, side, search, pair_chunk, seed, reps, oracle_pairs):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    georef, size = make(lines, per_line, seed)
    F = georef.shape[0]
    table = tiling.register_pairs(georef, size, GSD, search, side, MIN_CELLS)
    w1 = 2 * search + 1
    chunk = table[:pair_chunk]
    n = chunk.shape[0]
    pairs_of_cells = int((chunk["gx"].astype(np.int64) * chunk["gy"]).sum()) * w1 * w1
    needed = sorted(set(chunk["frame_a"].tolist()) | set(chunk["frame_b"].tolist()))
    gen = torch.Generator(device=dev).manual_seed(seed)
    pixels = torch.randint(0, 256, (len(needed), H, W, 3), device=dev, dtype=torch.uint8, generator=gen)
    desc = tiling._frame_descs([pixels[k] for k in range(len(needed))], dev)
    slot = np.full(F, -1, dtype=np.int32)
    slot[needed] = np.arange(len(needed), dtype=np.int32)
    g_d, s_d, slot_d = up(tiling.ground_to_pixel(georef).reshape(-1, 6)), up(size), up(slot)
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
    N.check(lib.wm_register_render_u8(N.ptr(desc), len(needed), N.ptr(slot_d), N.ptr(g_d), N.ptr(s_d), F, N.ptr(pairs_d), n, GSD, search, side,
                                      N.ptr(a), N.ptr(b), N.ptr(status), st))
    sad = lambda: N.check(lib.wm_register_search(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, MIN_CELLS, N.ptr(score), N.ptr(best_sad), st))
    zncc = lambda: N.check(lib.wm_register_search_zncc(N.ptr(a), N.ptr(b), N.ptr(pairs_d), n, search, side, MIN_CELLS, N.ptr(moments),
                                                       N.ptr(best), N.ptr(peak), st))
    sad(), zncc()
    torch.cuda.synchronize()
    ms = {"sad": [], "zncc": []}
    for _ in range(reps):                                     # alternating, in one process
        ms["sad"].append(once(sad))
        ms["zncc"].append(once(zncc))
    s_min, s_med = float(np.min(ms["sad"])), float(np.median(ms["sad"]))
    z_min, z_med = float(np.min(ms["zncc"])), float(np.median(ms["zncc"]))
    rate, bound = pairs_of_cells / (z_min * 1e-3), VALU_LANE_OPS / LOOP_VALU_PER_4_CELLS * 4
    out = {"frames": F, "side": side, "search": search, "chunk_pairs": n, "chunk_frames": len(needed),
           "mean_patch_cells": int((chunk["gx"].astype(np.int64) * chunk["gy"]).mean()), "cell_pairs": pairs_of_cells,
           "sad_ms_min": round(s_min, 4), "sad_ms_median": round(s_med, 4), "zncc_ms_min": round(z_min, 4), "zncc_ms_median": round(z_med, 4),
           "zncc_over_sad_min": round(z_min / s_min, 3), "zncc_over_sad_median": round(z_med / s_med, 3),
           "zncc_cell_pairs_per_s": float(f"{rate:.4g}"), "valu_bound_cell_pairs_per_s": float(f"{bound:.4g}"),
           "zncc_fraction_of_valu_bound": round(rate / bound, 4), "render_status": int(status.item())}
    by_k = {}
    for rnd in range(2):                                      # K = 1, 2, 4 alternating, twice
        for k in (1, 2, 4):
            os.environ["WM_REGISTER_K"] = str(k)
            by_k.setdefault(f"k{k}", []).append(timed(zncc, reps)[0])
    del os.environ["WM_REGISTER_K"]
    out["zncc_ms_min_by_offsets_per_thread"] = by_k
    zncc()
    torch.cuda.synchronize()
    if oracle_pairs > 0:
        from test_register_zncc import same_bytes, zncc_pick_oracle, zncc_search_oracle
        m = min(oracle_pairs, n)
        A, B = a[:m].cpu().numpy(), b[:m].cpu().numpy()
        got_m, got_b, got_p = moments[:m].cpu().numpy(), best[:m].cpu().numpy(), peak[:m].cpu().numpy()
        t = time.perf_counter()
        equal = True
        for p in range(m):
            mo = zncc_search_oracle(A[p], B[p], int(chunk["gx"][p]), int(chunk["gy"][p]), search)
            wb, wp = zncc_pick_oracle(mo, search, MIN_CELLS)
            equal = equal and np.array_equal(got_m[p], mo) and np.array_equal(got_b[p], wb) and same_bytes(got_p[p], wp)
        out["oracle_pairs"], out["oracle_host_s"], out["equals_oracle"] = m, round(time.perf_counter() - t, 2), bool(equal)
        out["sampled_peaks_r"] =[round(float(np.sign(q) * np.sqrt(abs(q))), 4) for q in got_p[:, 0]]
        assert equal, "the device result differs from the zncc oracle"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle-pairs", type=int, default=2)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    settings = {"f40": (4, 10, 256, 16, 64), "f1000": (25, 40, 512, 32, 256)}
    out = {"reps": a.reps}
    for i, (name, (lines, per_line, side, search, chunk)) in enumerate(settings.items()):
        if a.only in (None, name):
            out[name] = run(lines, per_line, side, search, chunk, i, a.reps, a.oracle_pairs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
