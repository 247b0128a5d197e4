"""Times of the overlay kernels (wm_draw_boxes_u8, wm_plot_image_u8) and the kernel list of one survey.

  python tools/overlay_time.py kernels [--reps 20]
      HIP-event times, each around one Python call (its small uploads and its launches), on a 6000 x 4000 device frame:
        draw_full_50 / draw_full_2000      wm_draw_boxes_u8 of 50 / 2000 boxes on the frame itself;
        overlay_1536_50 / overlay_1536_2000  what detect_frames(overlay=1536) queues per frame: wm_resample_u8 to
                                           1024 x 1536, then wm_draw_boxes_u8 of the scaled boxes; the draw alone beside it;
        plot_image_b16                     wm_plot_image_u8 of 16 tiles of 1024 x 1024 (201 MB read twice, 50 MB written);
        host_route_2000                    the route a caller had before: frame.cpu(), PIL resize to 1536 x 1024 and an
                                           ImageDraw.rectangle loop (host wall clock, once).
      Boxes are 20..120 px animals at random places, 7 labels.  The device pictures are checked against the PIL route.
      Prints one JSON line.
  python tools/overlay_time.py survey [--overlay 1536] [--frames 2]
      One survey of --frames 6000 x 4000 device frames with the synthetic ViT-B, with or without overlay=: run it under
      `rocprofv3 --kernel-trace --stats` for the kernel list.  Prints the detections.
"""
import argparse
import functools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import survey_bench_util  # noqa: E402
from wildlifemapper_amd import preprocess, synth, tiling  # noqa: E402

H, W = 4000, 6000


def boxes_for(n, rng):
    c = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1)
    wh = rng.uniform(20, 120, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(np.float32), rng.integers(0, 7, n)


timed = functools.partial(survey_bench_util.timed, warmup=0)          # every call site below warms up itself


def kernels(args):
    from PIL import Image, ImageDraw
    from wildlifemapper_amd import visualize
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    rng = np.random.default_rng(0)
    oh, ow = tiling.overlay_size(H, W, 1536)
    out = {"frame": [H, W], "overlay": [oh, ow], "reps": args.reps}
    for n in (50, 2000):
        bh, lh = boxes_for(n, rng)
        b, l = torch.from_numpy(bh).to(dev), torch.from_numpy(lh).to(dev)
        ob = b * torch.tensor([ow / W, oh / H, ow / W, oh / H], dtype=torch.float32, device=dev)
        work = frame.clone()
        tiling.draw_boxes(work, b, l)                                  # warm-up
        out[f"draw_full_{n}_ms"] = timed(lambda: tiling.draw_boxes(work, b, l), args.reps)
        pic = [None]

        def overlay():
            pic[0] = preprocess.resample_u8(frame, (oh, ow))
            tiling.draw_boxes(pic[0], ob, l)
        overlay()
        out[f"overlay_1536_{n}_ms"] = timed(overlay, args.reps)
        small = preprocess.resample_u8(frame, (oh, ow))
        out[f"draw_1536_{n}_ms"] = timed(lambda: tiling.draw_boxes(small, ob, l), args.reps)
        if n == 2000:                                                   # the host route, and the same picture from both
            torch.cuda.synchronize()
            t = time.perf_counter()
            im = Image.fromarray(frame.cpu().numpy(), "RGB").resize((ow, oh), Image.BILINEAR)
            d = ImageDraw.Draw(im)
            rects, drawn = tiling.outline_rects(ob)
            for rc, ok, lab in zip(rects.tolist(), drawn.tolist(), lh.tolist()):
                if ok:
                    d.rectangle(rc, outline=tuple(int(v) for v in tiling.DEFAULT_PALETTE[lab]), width=2)
            out["host_route_2000_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            big = (rects[:, 2] - rects[:, 0] >= 2) & (rects[:, 3] - rects[:, 1] >= 2)         # Pillow-valid sides only
            out["same_as_pil"] = bool(big.all()) and bool(np.array_equal(np.asarray(im), pic[0].cpu().numpy()))
    x = torch.randn((16, 3, 1024, 1024), device=dev, generator=g)
    visualize.plot_image(x)
    out["plot_image_b16_ms"] = timed(lambda: visualize.plot_image(x), args.reps)
    mn, md = out["plot_image_b16_ms"]
    out["plot_image_b16_GBps"] = round((2 * x.numel() * 4 + x.numel()) / mn / 1e6, 1)
    print(json.dumps(out))


def survey(args):
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(args.frames)]
    kw = dict(overlay=args.overlay) if args.overlay else {}
    dets = 0
    for r in tiling.detect_frames(m, frames, batch=16, **kw):
        dets += r["boxes"].shape[0]
    torch.cuda.synchronize()
    print(json.dumps({"frames": args.frames, "overlay": args.overlay, "detections": dets}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "survey"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--overlay", type=int, default=None)
    ap.add_argument("--frames", type=int, default=2)
    a = ap.parse_args()
    kernels(a) if a.mode == "kernels" else survey(a)


if __name__ == "__main__":
    main()
