#!/usr/bin/env python3
"""Dev tool: the folded-LayerNorm consumer GEMM at the block shapes (qkv, lin1), one column tile per workgroup against T tiles per
workgroup (csrc/gemm16_v5.h "Column walk").

  default       A/B in one process: per iteration one launch of every arm in turn (so all arms see the same clocks), each between two
                events; medians per arm, for two passes over the same arms (the spread of an arm against itself is the noise a
                difference has to beat).  --parent-lib PATH adds the parent commit's library (its wm_op_gemm16_folded) as an arm, loaded
                beside this tree's.  The outputs of all arms are compared bit for bit.
  --boundary    with WM_HIP_LIB=build/ab/libwm_dev.so WM_GEMM_DBG=1 (tools/build_dev.sh): 31 back-to-back launches per (shape, T); the
                library prints the in-kernel stamps of the 31st to stderr (host_dev_timeline.h)."""
import argparse, ctypes as C, math, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch
import gpu_util as G
from wildlifemapper_amd import _native as N

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=24)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--prec", default="fp16")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--boundary", action="store_true")
a = ap.parse_args()
M, K = a.batch * 4096, 1280
SHAPES = {"qkv": (3840, 0, False, (1, 3)), "lin1": (5120, 1, True, (1, 2, 4))}      # N, act, out_packed, candidate T
dev = G.dev()
code, dt = G.PRECS[a.prec]
_P, _I, _F = C.c_void_p, C.c_int, C.c_float
parent = None
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.wm_op_gemm16_folded.restype = _I
    parent.wm_op_gemm16_folded.argtypes = [_P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P]

for name, (Nn, act, packed, cands) in SHAPES.items():
    x = torch.randn(M, K, device=dev) * 1.5 + 0.2
    stats, x16 = G.ln_stats16(x, a.prec)
    w = G.to16(torch.randn(Nn, K, device=dev) / math.sqrt(K), a.prec)
    wf, c1, c2 = G.fold_weight16(w, 1 + 0.2 * torch.randn(K, device=dev), 0.1 * torch.randn(K, device=dev), torch.randn(Nn, device=dev), a.prec)
    flags = act | (N.GEMM_OUT_PACKED if packed else 0)
    outs = {}

    def launch(arm):
        out = outs.setdefault(arm, torch.empty((M, Nn), device=dev, dtype=dt))
        if arm == "parent":
            N.check(parent.wm_op_gemm16_folded(N.ptr(x16), N.ptr(wf), N.ptr(c1), N.ptr(c2), N.ptr(stats), 1e-6, N.ptr(out), M, Nn, K, flags, code, G.sp()))
        else:
            N.check(N.lib().wm_op_gemm16_folded_walk(N.ptr(x16), N.ptr(wf), N.ptr(c1), N.ptr(c2), N.ptr(stats), 1e-6, N.ptr(out), M, Nn, K, flags,
                                                     arm, code, G.sp()))

    if a.boundary:
        for t in cands:
            for _ in range(31):
                launch(t)
            torch.cuda.synchronize()
        continue
    arms = (["parent"] if parent else []) + list(cands)
    for arm in arms:
        for _ in range(3):
            launch(arm)
    torch.cuda.synchronize()
    ref = outs[arms[0]]
    same = {arm: bool(torch.equal(outs[arm], ref)) for arm in arms}
    for rep in range(2):
        ev = {arm: [] for arm in arms}
        for _ in range(a.iters):
            for arm in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(arm)
                e1.record()
                ev[arm].append((e0, e1))
        torch.cuda.synchronize()
        for arm in arms:
            us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[arm])
            label = arm if arm == "parent" else f"T={arm}"
            print(f"{name:5s} M={M} N={Nn} K={K} pass {rep} {label:7s}: median {statistics.median(us):8.1f} us  min {us[0]:8.1f}  max {us[-1]:8.1f}  "
                  f"n={len(us)}  bits equal to {arms[0] if arms[0] == 'parent' else 'T=' + str(arms[0])}: {same[arm]}", flush=True)
