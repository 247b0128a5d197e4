#!/usr/bin/env python3
"""Throughput bench of the WildlifeMapper inference hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N>1: launched by torch.distributed.run)

A "step" is one pass of the hot path over one batch of synthetic 1024x1024 tiles that is already
resident in HBM: FFT high-pass -> ViT-H encoder -> detection decoder -> PostProcess + NMS
(`--workload full`, the default), or the encoder alone (`--workload encoder`).  Default batch is
16 tiles per GPU = BASELINE.json configs[2], the largest single-GPU configuration (and configs[3]'s
per-GPU share: 128 tiles over 8 GPUs); `--batch 4 --workload encoder --precision bf16` is configs[1] literally,
`--precision fp8` configs[4].  Default operand type: fp16 (same MFMA rate as bf16; the mode that meets the 1e-3 logits bar
on every weight set tried); `--precision bf16` is +3.9 % tiles/s.  With N > 1 tiles shard data-parallel, one process per GPU, and every
step ends with the single fixed-size RCCL all-gather of box records (dist.py); per-GPU work is
constant -> weak scaling.  `--gpus N` without a torch.distributed.run environment starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child process (before this
process touches the GPU) and exits with its return code.

One JSON line on rank 0.  A plain run sets up, warms up, times the K steps (`value` in tiles/s, `ms_per_step`), writes the
last timed step's outputs if `--dump-outputs DIR` is given (inputs and weights are seeded: the same arguments give the same
inputs in every run) and prints the line; `roofline`, `kernel_classes`, `cpu_baseline` and `map_vs_cpu_ref` are null there.
Everything below needs `--full` (the `--no-*` switches then drop single parts of it).

`roofline` is for the dominant kernel class (the 16-bit MFMA GEMM):
algorithmic FLOPs of its launches / their summed duration, measured with HIP events on the
launch stream in a second pass of the same steps (so the headline timing carries no event overhead).
`cpu_baseline` times the CPU oracle (fp32 torch port of the reference) on ONE ViT-H tile: warm-up, 3 timed forwards, median,
on the host's physical cores (count and CPU model in the record).  `parity_vs_reference` scores tiles 0..4 of the timed batch
against the outputs the reference's own modules produced for them (tests/golden); `other_configs` holds short timed runs of
the other BASELINE.json configurations (configs[1] literally, bf16 at B = 16, configs[4] fp8) in the same process.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)



def _self_launch_if_needed() -> None:
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks as a CHILD process group
    (never exec: this process may not replace itself once a GPU runtime is loaded) and leave with the child's code."""
    if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    n = 1
    for i, tok in enumerate(sys.argv):
        if tok == "--gpus" and i + 1 < len(sys.argv):
            n = int(sys.argv[i + 1])
        elif tok.startswith("--gpus="):
            n = int(tok.split("=", 1)[1])
    if n <= 1:
        return
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: launching " + " ".join(cmd), file=sys.stderr, flush=True)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    rc = subprocess.call(cmd, env=env)
    sys.exit(rc if rc >= 0 else 1)


if __name__ == "__main__":
    _self_launch_if_needed()          # before torch / HIP are imported

import torch
import torch.distributed as dist

from wildlifemapper_amd import _native as N_
from wildlifemapper_amd import dist as wdist
from wildlifemapper_amd import synth

# algorithmic FLOPs per tile (useful work only)
FLOPS_FULL = {"vit_h": 5797.8e9, "vit_b": 1115.96e9 + 3.55e9}
FLOPS_ENC = {"vit_h": 5794.3e9, "vit_b": 1115.96e9}
PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp8": 5000.0}      # MI355X dense MFMA peaks (MI355X_MICROARCH.md)


def _state_dict(model_type: str) -> dict:
    """synth.make_state_dict(model_type) with the tensors filled on a thread pool: every tensor is its own counter stream, so
    the values are bit-identical; numpy's integer ufuncs run without the GIL, so ViT-H takes seconds instead of ~20 s."""
    from concurrent.futures import ThreadPoolExecutor
    shapes = synth.weight_shapes(model_type)
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    with ThreadPoolExecutor(max(1, min(16, cpus))) as ex:
        vals = list(ex.map(lambda kv: synth.make_weight(kv[0], kv[1]), shapes.items()))
    return {k: torch.from_numpy(v) for k, v in zip(shapes, vals)}


def build_model(model_type: str, precision: str, device: torch.device):
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    sam, _, post = sam_model_registry[model_type](None, None)
    model = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    sd = _state_dict(model_type)
    model.load_state_dict(sd, strict=True)
    model._hub.set_precision(precision)
    return model, sd


DUMP_BYTES = 64 << 20


def dump_outputs(d: str, outs: dict) -> None:
    """--dump-outputs: what the last timed step returned, one DIR/<name>.npy per array.  Box records are split into their
    fields (the int fields as float64, exact).  An output larger than its share of the 64 MB budget is written as a fixed
    sample (numpy seed 0, sorted flat indices) next to DIR/<name>_index.npy holding those indices (float64, exact); the two
    files together stay within the share."""
    import numpy as np
    from wildlifemapper_amd.engine import split_records
    arrays = {}
    for k, v in outs.items():
        if k == "records":
            for f, t in split_records(v).items():
                arrays[f"records_{f}"] = t.numpy().astype(np.float32 if t.is_floating_point() else np.float64)
        else:
            arrays[k] = v.float().numpy()
    os.makedirs(d, exist_ok=True)
    share = DUMP_BYTES // len(arrays) - 4096          # room for the .npy headers
    for k, v in arrays.items():
        if v.nbytes > share:
            n = share // (v.itemsize + 8)
            idx = np.sort(np.random.default_rng(0).choice(v.size, size=n, replace=False))
            np.save(os.path.join(d, f"{k}_index.npy"), idx.astype(np.float64))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(d, f"{k}.npy"), np.ascontiguousarray(v))


def _host_cpu() -> tuple:
    """(model string, physical cores) from /proc/cpuinfo."""
    model, cores = "unknown", set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "model name" and model == "unknown":
                    model = v
                elif k == "physical id":
                    phys = v
                elif k == "core id":
                    core = v
                elif not k and phys is not None:
                    cores.add((phys, core))
                    phys = core = None
        if phys is not None:
            cores.add((phys, core))
    except OSError:
        pass
    return model, (len(cores) or (os.cpu_count() or 1))


def _dets(rec, b: int) -> dict:
    kept = (rec["flags"][b] & 4) != 0
    order = torch.argsort(rec["nms_rank"][b][kept])
    return {"boxes": rec["boxes"][b][kept][order].numpy(), "scores": rec["scores"][b][kept][order].numpy(),
            "labels": rec["labels"][b][kept][order].numpy()}


def _nms_positions(rec, b: int) -> list:
    """NMS index list as visualize_prediction.py:150-154 produces it: positions among the score-filtered candidates."""
    flags, rank = rec["flags"][b], rec["nms_rank"][b]
    pos = torch.cumsum(((flags & 2) != 0).long(), 0) - 1
    slots = torch.nonzero((flags & 4) != 0).flatten()
    slots = slots[torch.argsort(rank[slots])]
    return pos[slots].tolist()


def parity_vs_reference_fixtures(model_type: str, out: dict, first_tile: int, weight_seed: int = 0):
    """Tiles of THE TIMED BATCH whose outputs the reference's own modules produced in the build container (tests/golden/
    e2e_vit_h.npz = tile 0, e2e_vit_h_tiles1to4.npz = tiles 1..4; oracle/gen_golden.py): logits rel-L2 per tile, NMS index
    lists, and mAP of the GPU detections with the reference-derived detections as ground truth.  Checker code (oracle
    PostProcess is pinned to the reference's; its NMS restates torchvision's and is unpinned)."""
    import numpy as np
    from oracle import wm_oracle as O
    from wildlifemapper_amd.coco_eval import map_vs_reference
    from wildlifemapper_amd.engine import split_records
    gold = os.path.join(ROOT, "tests", "golden")
    if model_type != "vit_h" or first_tile != 0 or weight_seed != 0:
        return None
    ref_lg, ref_bx, nms = {}, {}, {}
    for name in ("e2e_vit_h.npz", "e2e_vit_h_tiles1to4.npz"):
        path = os.path.join(gold, name)
        if not os.path.exists(path):
            continue
        fx = np.load(path)
        f0, n = int(fx["first_tile"]), int(fx["n_tiles"])
        for t in range(n):
            ref_lg[f0 + t], ref_bx[f0 + t] = fx["pred_logits"][t], fx["pred_boxes"][t]
            nms[f0 + t] = fx[f"pp{t}_nms_index"].tolist()
    B = out["pred_logits"].shape[0]
    tiles = [t for t in sorted(ref_lg) if t < B]
    if not tiles:
        return None
    lg = out["pred_logits"].cpu().numpy()
    rec = split_records(out["records"].cpu())
    errs, same, pred, gt = [], [], {}, {}
    for t in tiles:
        errs.append(float(np.linalg.norm(lg[t] - ref_lg[t]) / np.linalg.norm(ref_lg[t])))
        same.append(_nms_positions(rec, t) == nms[t])
        pred[t] = _dets(rec, t)
        d = O.detect(O.postprocess(torch.from_numpy(ref_lg[t][None]), torch.from_numpy(ref_bx[t][None]), torch.tensor([[1024, 1024]]))[0])
        gt[t] = {"boxes": d["boxes"].numpy(), "scores": d["scores"].numpy(), "labels": d["labels"].numpy()}
    m = map_vs_reference(pred, gt)
    return {"tiles": tiles, "source": "reference modules' outputs (tests/golden/e2e_vit_h*.npz), tiles of the timed batch",
            "logits_rel_l2": [round(e, 6) for e in errs], "logits_rel_l2_max": round(max(errs), 6),
            "nms_lists_identical": int(sum(same)), "nms_lists_total": len(same),
            "mAP": round(m["mAP"], 4), "mAP50": round(m["mAP50"], 4),
            "detections_gpu": [int(len(pred[t]["scores"])) for t in tiles], "detections_ref": [int(len(gt[t]["scores"])) for t in tiles]}


def cpu_baseline(model_type: str, sd, model, device, x_batch, ts_batch, first_tile: int, out_batch: dict, budget_s: float = 200.0) -> tuple:
    """Oracle (CPU port of the reference, fp32) timed on the host: one warm-up forward (ViT-B: thread pool, allocator and
    oneDNN primitives), then up to 3 timed forwards of ONE tile of the benched model, median, inside a
    time budget so that the default run stays bounded.  And the BASELINE metric's second half, "mAP vs CPU ref": the GPU
    path's detections on tile 0 OF THE TIMED BATCH (`out_batch`: one more pass over that resident batch, same kernel
    instances as the timed steps) scored against the CPU detections as ground truth (own COCO-style evaluator,
    wildlifemapper_amd/coco_eval.py).  Checker code, used here only as a baseline."""
    from oracle import wm_oracle as O
    from wildlifemapper_amd.coco_eval import map_vs_reference
    from wildlifemapper_amd.engine import split_records
    x = torch.from_numpy(synth.make_batch(first_tile, 1))
    assert torch.equal(x[0], x_batch[0].cpu()), "timed batch does not start with the checked tile"
    cfg = O.OracleCfg.from_model_type(model_type)
    cpu_model, phys = _host_cpu()
    torch.set_num_threads(max(1, phys))
    threads = torch.get_num_threads()
    t0 = time.time()
    if model_type != "vit_b":
        sdb = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
        O.model_forward(x, sdb, O.OracleCfg.from_model_type("vit_b"))
        del sdb
        warm = "1 vit_b tile"
    else:
        O.model_forward(x, sd, cfg)
        warm = "1 tile"
    warm_s = time.time() - t0
    times, ref = [], None
    t_start = time.time()
    for _ in range(3):
        t1 = time.time()
        ref = O.model_forward(x, sd, cfg)
        times.append(time.time() - t1)
        if time.time() - t_start + times[-1] > budget_s:          # the next forward would leave the budget
            break
    times.sort()
    med = times[len(times) // 2] if len(times) % 2 else 0.5 * (times[len(times) // 2 - 1] + times[len(times) // 2])
    base = {"value": round(1.0 / med, 5), "unit": "tiles/s", "cores": threads, "kind": "port", "cpu_model": cpu_model,
            "physical_cores": phys, "logical_cpus": os.cpu_count(),
            "sample": f"warm-up {warm} ({warm_s:.1f} s), then {len(times)} timed forward(s) of 1 {model_type} tile, full path fp32 "
                      f"(fft+encoder+decoder): {', '.join(f'{t:.1f}' for t in times)} s, median {med:.1f} s; torch CPU, {threads} threads "
                      f"= physical cores of {cpu_model}"}
    ts = torch.tensor([[1024, 1024]])
    det_ref = O.detect(O.postprocess(ref["pred_logits"], ref["pred_boxes"], ts)[0])
    out = {k: v[:1] for k, v in out_batch.items()}
    rec = split_records(out["records"].cpu())
    pred = {0: _dets(rec, 0)}
    kept = (rec["flags"][0] & 4) != 0
    gt = {0: {"boxes": det_ref["boxes"].numpy(), "scores": det_ref["scores"].numpy(), "labels": det_ref["labels"].numpy()}}
    m = map_vs_reference(pred, gt)
    lg = out["pred_logits"].cpu()
    parity = {"mAP": round(m["mAP"], 4), "mAP50": round(m["mAP50"], 4), "tiles": 1, "tile": f"tile 0 of the timed batch of {x_batch.shape[0]}",
              "detections_gpu": int(kept.sum()), "detections_cpu": int(len(det_ref["scores"])),
              "logits_rel_l2": float(((lg - ref["pred_logits"]).norm() / ref["pred_logits"].norm()).item()),
              "evaluator": "own COCO-style bbox AP@[.5:.95], CPU-reference detections as ground truth"}
    return base, parity


def time_config(model, x, ts, precision: str, workload: str, batch: int, steps: int, warmup: int, device, fp8_gemms: int = 0,
                fold_ln=None, fp8_bf16_head_tail=(0, 0), gemm_rate: bool = False) -> dict:
    """A short timed run of another BASELINE.json configuration in this same process (same model object, weights re-packed
    for the precision): W warm-up steps, K timed steps between device synchronisations, inputs resident.  gemm_rate: one more
    pass of the K steps with per-kernel HIP events for the GEMM class's TFLOP/s."""
    hub = model._hub
    hub.set_precision(precision)
    hub.set_fp8_gemms(fp8_gemms)
    if fold_ln is not None and fold_ln != hub.fold_ln:
        hub.fold_ln = fold_ln
        hub.close()
    os.environ["WM_FP8_BF16_HEAD"], os.environ["WM_FP8_BF16_TAIL"] = str(fp8_bf16_head_tail[0]), str(fp8_bf16_head_tail[1])
    if precision == "fp8":
        hub.close()                                   # the head / tail dials are read when the handle is created
    xb, tb = x[:batch].contiguous(), ts[:batch].contiguous()
    hfc = model.fft(xb) if workload == "encoder" else None

    def step():
        if workload == "encoder":
            return model.image_encoder(xb, hfc)
        return model.detect(xb, tb)

    with torch.no_grad():
        for _ in range(warmup):
            out = step()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
    r = {"precision": precision, "workload": workload, "batch": batch, "steps": steps, "warmup": warmup,
         "tiles_per_s": round(batch * steps / dt, 3), "ms_per_step": round(dt / steps * 1e3, 3)}
    if gemm_rate:
        hub.profile_enable(True)
        hub.profile_reset()
        with torch.no_grad():
            for _ in range(steps):
                step()
        torch.cuda.synchronize(device)
        st = hub.profile_read()
        hub.profile_enable(False)
        g = st["gemm16"]
        r["gemm_class_tflops"] = round(g["flops"] / (g["ms"] * 1e-3) / 1e12, 1) if g["ms"] > 0 else None
        r["gemm_class_frac_of_peak"] = round(r["gemm_class_tflops"] / PEAK_TFLOPS[precision], 4) if r["gemm_class_tflops"] else None
        r["kernel_classes_ms_per_step"] = {k: round(v["ms"] / steps, 3) for k, v in st.items()}
    if precision == "fp8":
        r["fp8_gemms"] = {0: "all (qkv, proj, lin1, lin2)", 4: "lin1 + lin2", 5: "qkv + lin1 + lin2", 6: "proj + lin1 + lin2", 7: "all"}.get(fp8_gemms, str(fp8_gemms))
        r["fp8_bf16_head_tail_blocks"] = list(fp8_bf16_head_tail)
    if workload == "full":
        par = parity_vs_reference_fixtures("vit_h", out, 0)
        if par:
            r["parity"] = {k: par[k] for k in ("tiles", "logits_rel_l2_max", "nms_lists_identical", "nms_lists_total", "mAP", "mAP50")}
    return r


def frontend_configs(model, device, B: int, headline_tiles_per_s: float) -> list:
    """SURVEY.md section 8(f) rows N1 and N3, timed with the headline's discipline (inputs resident in HBM, warm-up, device
    synchronisation on both sides of the timed region):
      (a) N1  wm_preprocess_u8_resized: 16 resident 3648 x 5472 uint8 frames (the val set's size) -> PIL-bilinear resize to
              512 x 768 -> ToTensor -> Normalize -> zero-padded 1024 x 1024 fp32 tiles; algorithmic bytes per frame = the
              frame read once + the tile written once;
      (b) N3  tiling.detect_frame on one resident 6000 x 4000 frame (7 x 5 overlapping tiles): frames/s and the split
              tile cut / path / merge NMS (each stage timed alone);
      (c) the chain frames -> N1 -> path -> records at the headline batch: what the input side costs a step."""
    from wildlifemapper_amd import preprocess, tiling
    from wildlifemapper_amd.engine import split_records
    out = []

    def timed(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) / reps, r

    with torch.no_grad():
        # (a) N1
        h, w = 3648, 5472
        torch.manual_seed(7)
        frames = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device=device)
        oh, ow = preprocess.resized_size(h, w, 768, 768)
        dt, tiles = timed(lambda: preprocess.tiles_from_u8(frames, resize=(768, 768)), 2, 10)
        bytes_frame = h * w * 3 + 3 * 1024 * 1024 * 4
        out.append({"config": "SURVEY 8(f) N1: wm_preprocess_u8_resized, %d resident %dx%d uint8 frames -> %dx%d content on 1024x1024 fp32 tiles" % (B, h, w, oh, ow),
                    "frames": B, "us_per_frame": round(dt / B * 1e6, 1), "frames_per_s": round(B / dt, 1),
                    "algorithmic_bytes_per_frame": bytes_frame, "algorithmic_gbps": round(bytes_frame * B / dt / 1e9, 1),
                    "frac_of_8TBps": round(bytes_frame * B / dt / 8e12, 4), "bound": "hbm",
                    "share_of_a_step_at_headline_rate": round((dt / B) * headline_tiles_per_s, 4)})
        # (c) chain: frames -> tiles -> path -> records
        ts = torch.full((B, 2), 1024.0, device=device)

        def chain():
            return model.detect(preprocess.tiles_from_u8(frames, resize=(768, 768)), ts)["records"]
        dtc, _ = timed(chain, 2, 5)
        out.append({"config": "frames -> N1 -> full path -> records, batch=%d (the input side inside the step)" % B,
                    "tiles_per_s": round(B / dtc, 3), "ms_per_step": round(dtc * 1e3, 3),
                    "vs_headline_resident_tiles": round((B / dtc) / headline_tiles_per_s, 4),
                    "note": "content is a 512 x 768 image on a zero canvas, as the val pipeline feeds the model (dataloader_coco.py:288); the path's time does not depend on content"})
        del frames, tiles
        # (b) N3
        H, W = 4000, 6000
        frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=device)
        org = torch.tensor(tiling.tile_origins(H, W, 1024, 128), dtype=torch.int32, device=device)
        n = int(org.shape[0])
        dt_all, det = timed(lambda: tiling.detect_frame(model, frame, batch=B), 1, 3)
        dt_cut, xt = timed(lambda: tiling.frame_to_tiles(frame, org), 2, 10)
        def path():
            return torch.cat([model.detect(xt[i:i + B])["records"] for i in range(0, n, B)], dim=0)
        dt_path, rec = timed(path, 1, 3)
        dt_merge, _ = timed(lambda: tiling.merge_tile_records(rec, org, 0.4), 2, 10)
        cut_bytes = H * W * 3 + n * 3 * 1024 * 1024 * 4
        out.append({"config": "SURVEY 8(f) N3: tiling.detect_frame, one resident %dx%d uint8 frame -> %d overlapping 1024x1024 tiles (batches of %d) -> merge NMS" % (W, H, n, B),
                    "frames_per_s": round(1.0 / dt_all, 3), "ms_per_frame": round(dt_all * 1e3, 2), "tiles_per_frame": n,
                    "tiles_per_s": round(n / dt_all, 2),
                    "split_ms": {"tile_cut": round(dt_cut * 1e3, 3), "path": round(dt_path * 1e3, 2), "merge_nms": round(dt_merge * 1e3, 3)},
                    "tile_cut_algorithmic_gbps": round(cut_bytes / dt_cut / 1e9, 1), "tile_cut_frac_of_8TBps": round(cut_bytes / dt_cut / 8e12, 4),
                    "merged_detections": int(det["scores"].numel()),
                    "note": "35 tiles = batches of 16 + 16 + 3: the last batch runs the small-batch kernel instances"})
    return out


def _committed_profile(a, B: int, hub):
    """Counter-derived numbers of the dominant kernel class from the rocprofv3 --pmc passes committed under profiles/ (newest
    round first).  Used only for the workload they were collected on; every value is labelled with its file."""
    if not (a.model == "vit_h" and a.workload == "full"):
        return None
    prof = os.path.join(ROOT, "profiles")
    for tag in ("r4_final", "r3_final", "r3"):
        tname = f"{tag}_{a.precision}_pmc_traffic.json"
        try:
            with open(os.path.join(prof, tname)) as f:
                t = json.load(f)
            if int(t.get("batch", 4)) != B or t.get("precision", "bf16") != a.precision:
                continue
            out = {"traffic_file": tname, "collected": t.get("collected", "see git log of the file"),
                   "hbm_bytes_per_launch": t["classes"]["gemm16"]["hbm_bytes_per_launch"],
                   "caveat": "counters from the builder's box under the profiler's clock; only the division by the live launch time uses this run"}
            uname = tname.replace("pmc_traffic.json", "pmc_util.txt")
            try:
                sect, vals = None, {}
                for ln in open(os.path.join(prof, uname)):
                    if ln.startswith("=="):
                        sect = ln.split()[1]
                    elif sect in ("gemm16v5_kernel", "gemm8_kernel") and "avg=" in ln:
                        vals.setdefault(sect, {})[ln.split()[0]] = float(ln.split("avg=")[1])
                v = vals.get("gemm8_kernel" if a.precision == "fp8" else "gemm16v5_kernel")
                if v and v.get("GRBM_GUI_ACTIVE"):
                    out["mfma_busy_pct"] = round(100.0 * v["SQ_VALU_MFMA_BUSY_CYCLES"] / (v["GRBM_GUI_ACTIVE"] * 128.0), 1)
                    out["mfma_busy_note"] = "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 128 SIMDs per XCD), tools/pmc_kernel.py"
                    out["util_file"] = uname
            except OSError:
                pass
            return out
        except (OSError, KeyError, ValueError):
            continue
    return None


def _config_name(a, B: int, world: int) -> str:
    """Which BASELINE.json config this run is, derived from what actually runs."""
    if a.model != "vit_h":
        return "not a BASELINE.json config"
    if a.precision == "fp8":
        return "BASELINE.json configs[4]" if (B == 16 and world == 1 and a.workload == "full") else "fp8 variant, not the configs[4] batch"
    if a.workload == "encoder":
        if B == 4 and world == 1:
            return "BASELINE.json configs[1]" if a.precision == "bf16" else "configs[1]'s shape with fp16 operands (configs[1] names bf16: --precision bf16)"
        return "encoder only, not the configs[1] batch"
    if B == 16:
        return "BASELINE.json configs[2]" if world == 1 else (f"BASELINE.json configs[3]: {16 * world} tiles over {world} GPUs" if world == 8
                                                               else f"configs[2] per GPU, {world} GPUs")
    return "full path, not a BASELINE.json batch"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="tiles per GPU per step (16 = BASELINE.json configs[2])")
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--precision", default=os.environ.get("WM_PRECISION", "fp16"), choices=["bf16", "fp16", "fp8"],
                    help="operand type of the MFMA GEMMs / attention: fp16 (default: meets the 1e-3 logits bar on every weight set tried) | "
                         "bf16 (the type BASELINE.json configs[1] names; same MFMA rate, +3.9 %% tiles/s, logits 0.7e-3 .. 2.0e-3 depending on "
                         "the weights) | fp8 (configs[4]; tolerance re-stated, see config.tolerance)")
    ap.add_argument("--workload", default="full", choices=["full", "encoder"])
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the HIP-event pass (roofline, kernel_classes), parity_vs_reference, other_configs, "
                         "frontend_configs and the CPU baseline; a plain run times the steps and prints the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the HIP-event pass")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip the short timed runs of the other BASELINE.json configurations")
    ap.add_argument("--backend", default="nccl", help="nccl (RCCL, default) | gloo (single-GPU rehearsal of the N>1 path)")
    ap.add_argument("--same-device", action="store_true", help="rehearsal: every rank uses cuda:0")
    a = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm device (no CPU fallback)")
    rank, world, local = wdist.init_from_env(a.backend)
    if a.same_device:
        local = 0
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a ROCm device"
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)

    model, sd = build_model(a.model, a.precision, device)
    hub = model._hub
    B = a.batch
    n_tiles = B * world
    first, _ = wdist.shard_range(n_tiles, rank, world)
    x = torch.from_numpy(synth.make_batch(first, B)).to(device)         # resident before timing
    ts = torch.full((B, 2), 1024.0, device=device)
    hfc = model.fft(x) if a.workload == "encoder" else None

    def step():
        """The timed path; returns what its caller receives (a dict of tensors)."""
        if a.workload == "encoder":
            return {"image_embeddings": model.image_encoder(x, hfc)}
        out = model.detect(x, ts)
        if world > 1:
            out["records"] = wdist.all_gather_records(out["records"], n_tiles, rank, world)
        return out

    def sync():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    last = None
    with torch.no_grad():
        for _ in range(a.warmup):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            last = step()
        sync()
        elapsed = time.perf_counter() - t0
    if a.dump_outputs and rank == 0 and last is not None:
        dump_outputs(a.dump_outputs, {k: v.cpu() for k, v in last.items()})
    del last
    tmax = torch.tensor([elapsed], device=device if a.backend == "nccl" else "cpu", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax.item())
    tiles_per_s = n_tiles * a.steps / elapsed

    roofline = None
    classes = None
    if a.full and not a.no_roofline:
        # second pass of the same steps with per-kernel HIP events on rank 0; every rank runs the steps because
        # a step of the N > 1 path contains the all-gather
        if rank == 0:
            hub.profile_enable(True)
            hub.profile_reset()
            N_.gemm_variant_counts(reset=True)
        with torch.no_grad():
            sync()
            t1 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize(device)
            prof_elapsed = time.perf_counter() - t1
        if rank == 0:
            st = hub.profile_read()
            hub.profile_enable(False)
            gemm_instances = {k: v // a.steps for k, v in N_.gemm_variant_counts().items() if v}
            g = st["gemm16"]
            achieved = g["flops"] / (g["ms"] * 1e-3) / 1e12 if g["ms"] > 0 else 0.0
            peak = PEAK_TFLOPS[a.precision if a.precision in PEAK_TFLOPS else "bf16"]
            # Live numbers (this run, HIP events on the launch stream): achieved, frac, avg_launch_us, launches, FLOPs and the
            # ALGORITHMIC bytes per launch (operands + residual + outputs as the launcher's byte model counts them).
            # Counter-derived numbers come from rocprofv3 --pmc passes committed under profiles/ (another box, another day):
            # they sit under `from_committed_profile` with their file names; `traffic` (the contract's key) repeats the PMC bytes
            # per launch of that file and `traffic_source` says so.
            avg_launch_s = g["ms"] * 1e-3 / max(g["launches"], 1)
            alg_bytes = g["bytes"] / max(g["launches"], 1)
            committed = _committed_profile(a, B, hub)
            traffic = committed["hbm_bytes_per_launch"] if committed else None
            if committed:
                committed["hbm_gbps_at_live_launch_time"] = round(traffic / avg_launch_s / 1e9, 1) if avg_launch_s > 0 else None
                committed["hbm_frac_of_8TBps"] = round(committed["hbm_gbps_at_live_launch_time"] / 8000.0, 4) if committed["hbm_gbps_at_live_launch_time"] else None
                committed["traffic_over_algorithmic"] = round(traffic / alg_bytes, 3) if alg_bytes > 0 else None
            folded = (bool(hub.fold_ln) and a.precision == "fp16") or (hub.fold_ln == "all" and a.precision == "bf16")
            roofline = {"bound": "mfma", "kernel": ("gemm8_kernel (fp8 block-scaled MFMA, the blocks' 4 projections) + the stem / neck fp16 GEMMs" if a.precision == "fp8"
                                                    else "gemm16v5_kernel<T,320|256,3> (all 16-bit MFMA GEMM launches)"),
                        "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                        "traffic": traffic,
                        "traffic_source": (f"NOT measured in this run: rocprofv3 PMC pass committed as profiles/{committed['traffic_file']} "
                                           f"(FETCH_SIZE x 2 + WRITE_SIZE per launch, tools/pmc_summarize.py)") if committed else None,
                        "measured_live": "achieved, frac, avg_launch_us, launches_per_step, gflop_per_launch, ms_per_step_with_events: HIP events on the launch stream, this run",
                        "avg_launch_us": round(g["ms"] * 1e3 / max(g["launches"], 1), 2),
                        "launches_per_step": g["launches"] // a.steps,
                        "gflop_per_launch": round(g["flops"] / max(g["launches"], 1) / 1e9, 3),
                        "algorithmic_bytes_per_launch": round(alg_bytes),
                        "algorithmic_bytes_note": "operands (A, W: 2 B per element), residual and outputs per launch as the launchers count them (csrc/wm_api.hip Bracket), averaged over the class",
                        "algorithmic_gbps": round(alg_bytes / avg_launch_s / 1e9, 1) if avg_launch_s > 0 else None,
                        "ms_per_step_with_events": round(prof_elapsed / a.steps * 1e3, 3),
                        "from_committed_profile": committed,
                        "folded_layernorm": folded,
                        "note": ("with the folded LayerNorm (default) the GEMM launches also carry the blocks' LayerNorms -- row statistics and the 16-bit "
                                 "plane(s) of the stream in the residual GEMMs' epilogues, the normalisation in the qkv / lin1 epilogues; "
                                 "other_configs holds the same step with the LayerNorm as its own kernel") if folded else None,
                        "sustained_clock_note": "power-limited: in-kernel s_memtime / wall clock (dev build, WM_GEMM_DBG=1) reads ~1.5 GHz "
                                                "at the 31st 16-bit GEMM of a step (1.79 GHz isolated) and 1.6-1.9 GHz in the fp8 GEMM; "
                                                "DESIGN.md section 5",
                        "gemm_instances_per_step": gemm_instances}
            classes = {k: {"ms_per_step": round(v["ms"] / a.steps, 3), "launches_per_step": v["launches"] // a.steps,
                           "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 and v["flops"] > 0 else None}
                       for k, v in st.items()}
    if world > 1:
        dist.barrier()

    if rank == 0:
        flops_tile = (FLOPS_ENC if a.workload == "encoder" else FLOPS_FULL).get(a.model)
        line = {
            "metric": "1024x1024 tiles/sec (whole node)", "value": round(tiles_per_s, 3), "unit": "tiles/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.precision, "data": "synthetic",
            "config": {"workload": (f"{a.model} {'encoder only' if a.workload == 'encoder' else 'full path fft+encoder+decoder+PostProcess/NMS'}"
                                    f", {a.precision} MFMA, batch={B} tiles/GPU of 1024x1024x3 ({_config_name(a, B, world)})"),
                       "tiles_per_step": n_tiles, "parallelism": f"dp{world} tile shard" + (f", {'RCCL' if a.backend == 'nccl' else a.backend} all-gather of box records" if world > 1 and a.workload == "full" else ""),
                       "weights": "seed 0 synthetic (random init)",
                       "tolerance": ("re-stated for fp8 (DESIGN.md section 3): logits within 5e-2 relative of the fp32 CPU forward, mAP50 vs the CPU "
                                     "reference's detections >= 0.8" if a.precision == "fp8"
                                     else ("logits within 1e-3 relative of the fp32 CPU forward, identical NMS index lists" if a.precision == "fp16"
                                           else "bf16 operands: logits within 1e-3 relative of the fp32 CPU forward on synth weight seed 0 (7.2-8.2e-4), "
                                                "2.0e-3 on seed 1; identical NMS index lists on both (DESIGN.md section 3)"))},
            "model_tflops": round(tiles_per_s * flops_tile / 1e12, 1) if flops_tile else None,
            "frac_of_mfma_peak_whole_path": round(tiles_per_s * flops_tile / 1e12 / (PEAK_TFLOPS.get(a.precision, 2500.0) * world), 4) if flops_tile else None,
            "roofline": roofline, "kernel_classes": classes,
        }
        if a.full:
            full_extras(a, line, model, sd, hub, x, ts, B, first, world, device, tiles_per_s)
        else:
            line["cpu_baseline"], line["map_vs_cpu_ref"] = None, None
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def full_extras(a, line: dict, model, sd, hub, x, ts, B: int, first: int, world: int, device, tiles_per_s: float) -> None:
    """--full, rank 0, after the headline: parity of the timed batch against the reference fixtures, the other BASELINE.json
    configurations, the frontend rows and the CPU baseline, each written into `line`."""
    out_batch = None
    if world == 1 and a.workload == "full":
        with torch.no_grad():
            out_batch = model.detect(x, ts)                       # one more pass over the timed, resident batch
        torch.cuda.synchronize(device)
        line["parity_vs_reference"] = parity_vs_reference_fixtures(a.model, out_batch, first)
    # The other BASELINE.json configurations, timed in this process so that the driver's one command covers them:
    # configs[1] literally (ViT-H encoder, bf16, B = 4), bf16 at the headline batch, configs[4] (fp8, all GEMMs) and the
    # fp8 mix that keeps the reference's detections.  Short runs (5 steps): indicative, the headline is `value`.
    if world == 1 and a.model == "vit_h" and not a.no_other_configs and B >= 4:
        others = []
        fold_default = hub.fold_ln
        try:
            others.append(dict(time_config(model, x, ts, "bf16", "encoder", 4, 5, 2, device), config="BASELINE.json configs[1]: ViT-H encoder bf16, batch=4"))
            if B >= 16:
                others.append(dict(time_config(model, x, ts, "bf16", "full", 16, 5, 2, device, fold_ln=fold_default, gemm_rate=True),
                                   config="configs[2] with bf16 operands (bf16 default: LayerNorm as its own kernel, fp32 residual stream)"))
                others.append(dict(time_config(model, x, ts, "bf16", "full", 16, 5, 2, device, fold_ln="all", gemm_rate=True),
                                   config="configs[2] with bf16 operands, LayerNorm folded + split residual stream (WM_LN_FOLD=2, opt-in: another draw of bf16's "
                                          "~1e-3 logits error, include/wm_hip.h WM_CFG_FOLD_LN)"))
                others.append(dict(time_config(model, x, ts, "fp16", "full", 16, 5, 2, device, fold_ln=False, gemm_rate=True),
                                   config="configs[2], fp16 operands, LayerNorm as its own kernel (WM_LN_FOLD=0): the GEMM class without the folded "
                                          "LayerNorm's statistics / 16-bit-copy / normalisation work in its epilogues"))
                others.append(dict(time_config(model, x, ts, "fp8", "full", 16, 5, 2, device, fold_ln=fold_default, gemm_rate=True),
                                   config="BASELINE.json configs[4]: fp8, all four GEMMs of every block"))
                others.append(dict(time_config(model, x, ts, "fp8", "full", 16, 5, 2, device, fp8_gemms=N_.FP8_MLP, fp8_bf16_head_tail=(8, 8)),
                                   config="configs[4] variant closest to the reference's detections in the sweep (profiles/r3_fp8_gemm_mask_sweep.txt): fp8 MLP "
                                          "pair only, first / last 8 blocks bf16"))
        finally:
            os.environ["WM_FP8_BF16_HEAD"], os.environ["WM_FP8_BF16_TAIL"] = "0", "0"
            hub.set_fp8_gemms(0)
            hub.set_precision(a.precision)
            if hub.fold_ln != fold_default:
                hub.fold_ln = fold_default
                hub.close()
        line["other_configs"] = others
    # the rows either side of the path (N1 input pipeline, N3 large-frame tiling), measured
    if world == 1 and a.model == "vit_h" and a.workload == "full" and not a.no_other_configs and B >= 4:
        line["frontend_configs"] = frontend_configs(model, device, B, tiles_per_s)
    if not a.no_cpu_baseline and world == 1 and a.workload == "full":
        line["cpu_baseline"], line["map_vs_cpu_ref"] = cpu_baseline(a.model, sd, model, device, x, ts, first, {k: v.cpu() for k, v in out_batch.items()})
    else:
        line["cpu_baseline"], line["map_vs_cpu_ref"] = None, None


if __name__ == "__main__":
    main()
