"""Survey throughput and merge timing (tiling.detect_frames, wm_merge_frames_nms).

  python tools/survey_time.py rate  [--model vit_h] [--batch 16]
      tiles/s of detect_frames over a mixed survey (8 x 6000x4000, 8 x 3648x5472, 1 x 20000x15000) with device-resident
      frames and with host frames, against model.detect on resident tiles at the same batch, in one process.
  python tools/survey_time.py rate --resize 768 768 | --scale 0.25  [--repeat 8]
      the same survey resampled first (detect_frames(resize=...) / (scale=...)), --repeat times over; the resident
      baseline runs model.detect on the same batch sizes with the tiles' content extents as target sizes, and frames/s
      are printed next to tiles/s.
  python tools/survey_time.py rate --chips 128
      the same survey (any of the forms above) with a review chip per detection (detect_frames(chips=...)); the JSON
      line gains the detections of one pass, so the added time per frame and per chip follows from a run without --chips.
  python tools/survey_time.py resample [--reps 20]
      wm_resample_u8 of a 6000 x 4000 frame to 768 x 512 and to 3000 x 2000; run under `rocprofv3 --kernel-trace --stats`
      for the per-kernel times; the algorithmic bytes of each pass are printed.
  python tools/survey_time.py merge [--reps 20] [--fuse [--fuse-thr 0.5]]
      synthetic per-tile records, wm_merge_frames_nms at 35 tiles and at 391; run under `rocprofv3 --kernel-trace --stats`
      for the per-kernel times (wall times printed here include the launch).  --fuse: wm_merge_frames_fuse on the same
      records too (merge_frames_nms_kernel<1>; the NMS is <0>), each mode's calls back to back, and the detection counts.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wildlifemapper_amd import _native as N, synth, tiling  # noqa: E402

SURVEY = [(4000, 6000)] * 8 + [(3648, 5472)] * 8 + [(15000, 20000)]


def make_model(model_type, prec):
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(model_type).items()}
    sam, _, _ = sam_model_registry[model_type](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    m._hub.set_precision(prec)
    return m


def rate(args):
    dev = torch.device("cuda:0")
    m = make_model(args.model, args.prec)
    g = torch.Generator(device=dev).manual_seed(0)
    dframes = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=g) for h, w in SURVEY]
    hframes = [f.cpu().numpy() for f in dframes]
    shapes = SURVEY * args.repeat
    dframes, hframes = dframes * args.repeat, hframes * args.repeat
    resampling = args.scale is not None or args.resize is not None
    kw = dict(scale=args.scale, resize=tuple(args.resize) if args.resize else None) if resampling else {}
    sizes = [tiling.resampled_size(i, h, w, **kw) for i, (h, w) in enumerate(shapes)] if resampling else shapes
    origins = [tiling.tile_origins(h, w) for h, w in sizes]
    n_tiles = sum(len(o) for o in origins)
    x = tiling.frame_to_tiles(dframes[0], torch.tensor(tiling.tile_origins(4000, 6000)[:args.batch], dtype=torch.int32))
    n_batches = -(-n_tiles // args.batch)
    if resampling:                            # the survey's own batch sizes and content-extent target sizes
        ext = torch.tensor([(min(1024, w - x0), min(1024, h - y0)) for (h, w), org in zip(sizes, origins) for y0, x0 in org],
                           dtype=torch.float32, device=dev)
        batches = [(x[:min(args.batch, n_tiles - i)], ext[i:i + args.batch]) for i in range(0, n_tiles, args.batch)]

    def resident():
        if resampling:
            for xb, tb in batches:
                m.detect(xb, tb)
            return
        for _ in range(n_batches):
            m.detect(x)

    ckw = dict(chips=args.chips) if args.chips else {}
    detections = [0]

    def survey(frames):
        def run():
            detections[0] = 0
            for r in tiling.detect_frames(m, frames, batch=args.batch, **kw, **ckw):
                detections[0] += r["boxes"].shape[0]
        return run

    res = {}
    for name, fn in [("resident_tiles", resident), ("device_frames", survey(dframes)), ("host_frames", survey(hframes))]:
        fn()                                     # warm-up (handle, pinned buffer, allocator)
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        res[name] = (n_tiles if resampling or name != "resident_tiles" else n_batches * args.batch) / best
        if resampling:
            res[name.split("_")[0] + "_frames_per_s"] = len(shapes) / best
        print(f"{name}: {res[name]:.2f} tiles/s (best of {args.reps}, {best:.3f} s)", flush=True)
    res["device_over_resident"] = res["device_frames"] / res["resident_tiles"]
    res["host_over_resident"] = res["host_frames"] / res["resident_tiles"]
    extra = {"scale": args.scale, "resize": args.resize} if resampling else {}
    if args.chips:
        extra.update(chips=args.chips, detections=detections[0])
    print(json.dumps({"survey_tiles": n_tiles, "frames": len(shapes), "model": args.model, "precision": args.prec, "batch": args.batch,
                      **extra, **{k: round(v, 4) for k, v in res.items()}}))


def resample(args):
    from wildlifemapper_amd import preprocess
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    f = torch.randint(0, 256, (4000, 6000, 3), dtype=torch.uint8, device=dev, generator=g)
    out = {}
    for oh, ow in [(512, 768), (2000, 3000)]:
        preprocess.resample_u8(f, (oh, ow))
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.reps):
            preprocess.resample_u8(f, (oh, ow))
        torch.cuda.synchronize()
        key = f"{ow}x{oh}"
        out[f"{key}_ms_wall"] = round((time.perf_counter() - t) / args.reps * 1e3, 4)
        # horizontal pass: H*W*3 read, H*ow*3 written; vertical pass: H*ow*3 read, oh*ow*3 written
        out[f"{key}_h_bytes"] = 4000 * 6000 * 3 + 4000 * ow * 3
        out[f"{key}_v_bytes"] = 4000 * ow * 3 + oh * ow * 3
    print(json.dumps(out))


def synth_records(H, W, rng, p_cand=0.1):
    """Per-tile records: a few candidates per tile, objects seen by two horizontally neighbouring tiles duplicated."""
    org = tiling.tile_origins(H, W)
    n = len(org)
    c = rng.random((n, 51, 2)) * 1000 + 12
    wh = rng.random((n, 51, 2)) * 80 + 10
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=-1).astype(np.float32)
    scores = rng.random((n, 51)).astype(np.float32)
    cand = rng.random((n, 51)) < p_cand
    for t in range(n - 1):
        if org[t][0] == org[t + 1][0]:
            dx = org[t + 1][1] - org[t][1]
            boxes[t + 1, 0] = boxes[t, 0] - np.array([dx, 0, dx, 0], np.float32)
            cand[t, 0] = cand[t + 1, 0] = True
    rec = torch.zeros((n, 51, 8), dtype=torch.float32)
    rec[..., 0:4] = torch.from_numpy(boxes)
    rec[..., 4] = torch.from_numpy(scores)
    rec.view(torch.int32)[..., 6] = torch.from_numpy(np.where(cand, N.FLAG_NMS | N.FLAG_SCORE | N.FLAG_CONF, N.FLAG_CONF).astype(np.int32))
    rec.view(torch.int32)[..., 7] = -1
    return rec, torch.tensor(org, dtype=torch.int32), int(cand.sum())


def merge(args):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    out = {}
    for label, (H, W) in [("35_tiles", (4000, 6000)), ("391_tiles", (15000, 20000))]:
        rec, org, ncand = synth_records(H, W, rng)
        rec, org = rec.to(dev), org.to(dev)
        n = rec.shape[0]
        modes = [("merge", None)] + ([("fuse", args.fuse_thr)] if args.fuse else [])
        for name, fuse_thr in modes:
            res = tiling.merge_frames(rec, org, [0, n], 0.4, fuse_thr=fuse_thr)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                tiling.merge_frames(rec, org, [0, n], 0.4, fuse_thr=fuse_thr)
            torch.cuda.synchronize()
            out[f"{name}_{label}_ms_wall"] = round((time.perf_counter() - t) / args.reps * 1e3, 4)
            if args.fuse:
                out[f"{name}_{label}_detections"] = int(res["det_count"][0])
        out[f"candidates_{label}"] = ncand
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("rate", "merge", "resample"))
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--prec", default="fp16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=None, help="rate: resample every frame by this factor first")
    ap.add_argument("--resize", type=int, nargs=2, default=None, metavar=("SIZE", "MAX_SIZE"),
                    help="rate: resample every frame to the val transform's geometry first, e.g. 768 768")
    ap.add_argument("--chips", type=int, default=None, help="rate: cut a review chip of this size for every detection")
    ap.add_argument("--repeat", type=int, default=1, help="rate: the survey this many times over")
    ap.add_argument("--fuse", action="store_true", help="merge: time wm_merge_frames_fuse on the same records too")
    ap.add_argument("--fuse-thr", type=float, default=0.5, help="merge --fuse: the fuse threshold")
    args = ap.parse_args()
    {"rate": rate, "merge": merge, "resample": resample}[args.mode](args)


if __name__ == "__main__":
    main()
