"""The encoder's stage-by-stage parity cases: what tests/test_gpu_encoder_stages.py and tests/test_encoder_mutants.py share.  Plain
module (torch on the CPU only): the stages, the three input tiles, the metrics, the bar rule and the launch-plan table.

A STAGE is one step of host_encoder.h's path, checked alone: it is fed what the GPU itself produced for the previous stage (teacher
forcing), so its error is its own.

  stage      oracle input (from the GPU)        compared with
  hfc        the tile                           m.fft(x), the whole 1024 x 1024
  patch      the tile                           tap -3
  adaptor    tap -3 and m.fft(x)                tap -1 minus tap -3
  block<i>   tap i-1 (tap -1 for i = 0)         tap i minus its input
  neck       tap depth-1                        the embedding, as (64, 64, 256)

For adaptor and block<i> the stage's own contribution is compared, not the stream (whose norm would hide the stage's error).

METRICS (float64, err = got - ref): relative L2 over the whole tensor; max-abs over the largest reference magnitude; the worst
relative L2 over every channel, every grid row, every grid column, every token (hfc: image rows and image columns).  A slice whose
reference norm is zero is compared by absolute error against the largest slice norm of its family.

BARS come from the oracle alone, per stage, input and metric, in the same test run:
    bar = 2 x metric(oracle with cfg.rnd = the stage's operand rounding and float64 accumulation, against the exact float64 oracle)
on the same teacher-forced input.  The rounding is fp16 for patch, adaptor and neck in every mode and fp16 or bf16 for the blocks.
The factor 2 is for the roundings the kernels do and cfg.rnd does not model (16-bit copies between GEMMs, gamma (.) W rounded once,
softmax in the log2 domain, the fast GELU).  hfc has no operand rounding: its bar is 4 x the error of the fp32 CPU oracle against
the float64 one (the margin is for the kernel's different FFT factorisation).
"""
from __future__ import annotations

import dataclasses

import torch

from oracle import wm_oracle as O
from wildlifemapper_amd import synth

ROUND = {"fp16": O.fp16_round, "bf16": O.bf16_round}
BAR_FACTOR, HFC_BAR_FACTOR = 2.0, 4.0

# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: three tiles chosen for the edges
# ---------------------------------------------------------------------------------------------------------------------------------
TILES = ("textured", "padded", "spike")
PADDED = (768, 700)                 # content rows x columns of `padded`; the rest is zero, as the collation pads a short image
SPIKE = (63, 63, 30.0)              # grid row, grid column, factor of the one bright 16 x 16 patch of `spike`: the 64 -> 70 grid's
                                    # last, partly padded window (4 of its 14 rows and columns are real tokens)
_TILE_SEED = {"textured": 3, "padded": 4, "spike": 5}


def tile(kind: str) -> torch.Tensor:
    """(1, 3, 1024, 1024) fp32, normalised as the dataloader does.  textured: block pattern + noise (pass-band and stop-band energy
    for the high-pass); padded: 768 x 700 of content, zero elsewhere (whole windows and the neck's border rows see constant tokens);
    spike: textured with the patch of grid cell (63, 63) scaled by 30."""
    x = torch.from_numpy(synth.make_batch(_TILE_SEED[kind], 1, smooth=True))
    if kind == "padded":
        h, w = PADDED
        x[:, :, h:, :] = 0
        x[:, :, :, w:] = 0
    elif kind == "spike":
        r, c, f = SPIKE
        x[:, :, 16 * r:16 * r + 16, 16 * c:16 * c + 16] *= f
    elif kind != "textured":
        raise KeyError(kind)
    return x


def batch(kind: str, n: int) -> torch.Tensor:
    """n tiles with tile(kind) LAST (the oracle checks the last tile only: a wrong batch offset shows); the others are noise tiles."""
    if n == 1:
        return tile(kind)
    return torch.cat([torch.from_numpy(synth.make_batch(10, n - 1)), tile(kind)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plan: which batch sizes the GPU test runs, and which GEMM kernel instances a forward of that size must take
# ---------------------------------------------------------------------------------------------------------------------------------
# gemm16_takes_v5 (host_gemm.h) picks the 256-row-tile kernel or a half-width one per GEMM from M = 4096 x batch; the folded LayerNorm
# needs qkv and lin1 on the 256-row-tile kernel, the split stream needs proj and lin2 on it.  For ViT-B (D = 768) that gives:
#   batch 1   qkv, lin1 on the 256-row-tile kernel, every other GEMM half-width: folded LayerNorm (fp16 blocks), fp32 stream
#   batch 2   every encoder GEMM half-width except the adaptor's k/v: no fold, standalone LayerNorm kernels
#   batch 3   every encoder GEMM on the 256-row-tile kernel except the adaptor's k/v and the neck: fold + split stream (fp16 blocks)
# and for ViT-H (D = 1280): 1 tile = fold with the fp32 stream, 2 tiles = no fold, 3 and 4 tiles = fold + split stream (the test runs
# 1 and 4).
# PLAN[(model, mode, batch)] = the non-zero wm_debug_gemm_variant_counts of ONE image_encoder forward.  Asserted by the GPU test, so
# that a change of the dispatch shows as a failing test and not as lost coverage.  (v2_*: the half-width kernels; v5_*: the 256-row-tile
# kernel, _res with an fp32 residual, _foldp the statistics-producing form, _split the split stream's residual GEMM.  The folded
# LayerNorm's CONSUMER counts as the plain v5 instance it is, so fold against no fold shows at batch 1 only through the numbers; at
# batch 3 / 4 tiles the 24 / 64 _split launches and the _foldp launch of proj_back are the fold + split-stream regime itself.)
_B1 = {"v2_128": 33, "v3_conv3x3": 1, "v5_256": 24, "v3_patch_embed": 2}
_B2 = {"v2_128": 56, "v3_conv3x3": 1, "v5_256": 1, "v3_patch_embed": 2}
PLAN = {
    ("vit_b", "fp16", 1): _B1,
    ("vit_b", "fp16", 2): _B2,
    ("vit_b", "fp16", 3): {"v2_128": 2, "v3_conv3x3": 1, "v5_256": 27, "v5_256_res": 3, "v5_256_foldp": 1, "v5_256_split": 24, "v3_patch_embed": 2},
    ("vit_b", "bf16", 1): _B1,
    ("vit_b", "bf16", 2): _B2,
    ("vit_b", "bf16", 3): {"v2_128": 2, "v3_conv3x3": 1, "v5_256": 27, "v5_256_res": 28, "v3_patch_embed": 2},
    ("vit_h", "fp16", 1): {"v2_160": 65, "v2_128": 8, "v3_conv3x3": 1, "v5_320": 64, "v3_patch_embed": 2},
    ("vit_h", "fp16", 4): {"v2_128": 1, "v3_conv3x3": 1, "v5_320": 64, "v5_256": 4, "v5_256_res": 3, "v5_320_foldp": 1, "v5_320_split": 64,
                           "v3_patch_embed": 2},
}


def takes_v5(M: int, N: int, K: int) -> bool:
    """gemm16_takes_v5's rule restated (host_gemm.h), for the table above and its CPU check."""
    if M <= 0 or M % 256 or K % 32 or K // 32 < 2:
        return False

    def prefer_half(bn):
        t = (M // 256) * (N // bn)
        return ((2 * t + 255) // 256) * 0.6 < ((t + 255) // 256)
    if N % 320 == 0:
        return not prefer_half(320)
    if N % 256 == 0:
        return not prefer_half(256)
    return False


def regime(D: int, n: int) -> str:
    """The fp16 blocks' regime of a call of n tiles: 'fold' (folded LayerNorm, fp32 stream), 'split' (fold + split stream), 'plain'."""
    M = 4096 * n
    fold = takes_v5(M, 3 * D, D) and takes_v5(M, 4 * D, D)
    split = takes_v5(M, D, D) and takes_v5(M, D, 4 * D)
    return "split" if fold and split else "fold" if fold else "plain"


VIT_B_BATCHES = (1, 2, 3)            # fold, plain, split (regime(768, n))
VIT_H_BATCHES = (1, 4)               # fold, split (regime(1280, n))


# ---------------------------------------------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------------------------------------------
def vit_b_stages(depth: int = 12):
    return ("hfc", "patch", "adaptor", "block0", "block1", "block2", f"block{depth - 1}", "neck")


def stage_taps(stage: str, depth: int):
    """(taps read for the oracle's input, taps read for the GPU's result).  'x', 'hfc', 'emb' are not taps but travel with them."""
    if stage == "hfc":
        return ("x",), ("hfc",)
    if stage == "patch":
        return ("x",), (-3,)
    if stage == "adaptor":
        return (-3, "hfc"), (-1, -3)
    if stage == "neck":
        return (depth - 1,), ("emb",)
    i = int(stage[5:])
    return (i - 1,), (i, i - 1)


def stage_weights(W: dict, stage: str) -> dict:
    e = "image_encoder."
    pre = {"hfc": (), "patch": (e + "patch_embed.", e + "pos_embed"), "adaptor": (e + "hfc_embed.", e + "hfc_attn."),
           "neck": (e + "neck.",)}.get(stage) or (f"{e}blocks.{int(stage[5:])}.",)
    return {k: v for k, v in W.items() if k.startswith(pre)} if pre else {}


def oracle_stage(stage: str, cfg: O.OracleCfg, W: dict, ins: dict) -> torch.Tensor:
    """The stage in the dtype of W and ins: x (1, 3, 1024, 1024), hfc (1, 1, 1024, 1024), t (1, 64, 64, D).  Returns what the table
    at the top compares: hfc (1024, 1024); patch, adaptor, block<i> (64, 64, D); neck (64, 64, 256)."""
    e = "image_encoder."
    with torch.no_grad():
        if stage == "hfc":
            return O.hfc_fft(ins["x"])[0, 0]
        if stage == "patch":
            t = O.conv_embed(ins["x"], W[e + "patch_embed.proj.weight"], W[e + "patch_embed.proj.bias"], cfg.patch, cfg)
            return (t + W[e + "pos_embed"])[0]
        if stage == "adaptor":
            h = O.conv_embed(ins["hfc"], W[e + "hfc_embed.proj.weight"], W[e + "hfc_embed.proj.bias"], cfg.patch, cfg)
            return O.hfc_adaptor(h, ins["t"], W, cfg)[0]
        if stage == "neck":
            return O.neck(ins["t"], W, cfg)[0].permute(1, 2, 0).contiguous()
        t = ins["t"]
        return (O.encoder_block(t, W, int(stage[5:]), cfg) - t)[0]


def to64(d: dict) -> dict:
    return {k: v.double() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics and bars
# ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"channel": (0, 1), "row": (1, 2), "col": (0, 2), "token": (2,)}       # of a (64, 64, C) tensor: the dims summed over
IMAGE_FAMILIES = {"row": (1,), "col": (0,)}                                       # of the (1024, 1024) hfc image


def metrics(got: torch.Tensor, ref: torch.Tensor) -> dict:
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = got - ref
    out = {"rel_l2": (err.norm() / ref.norm()).item(), "max_rel": (err.abs().max() / ref.abs().max()).item()}
    for name, dims in (IMAGE_FAMILIES if ref.dim() == 2 else FAMILIES).items():
        en, rn = err.pow(2).sum(dims).sqrt(), ref.pow(2).sum(dims).sqrt()
        scale = torch.where(rn > 0, rn, rn.max())            # a zero slice: absolute error against the family's largest norm
        out[name] = (en / scale).max().item()
    return out


def zero_slices(ref: torch.Tensor) -> dict:
    ref = ref.double()
    return {name: int((ref.pow(2).sum(dims) == 0).sum()) for name, dims in (IMAGE_FAMILIES if ref.dim() == 2 else FAMILIES).items()}


def study(stage: str, cfg: O.OracleCfg, W32: dict, ins32: dict, prec: str = "fp16"):
    """(the exact float64 result, the bars) of one stage on one teacher-forced input.  `prec` matters for block<i> only."""
    ins64 = to64(ins32)
    if stage == "hfc":
        exact = oracle_stage(stage, cfg, {}, ins64)
        emul, factor = oracle_stage(stage, cfg, {}, ins32), HFC_BAR_FACTOR
    else:
        W64 = to64(stage_weights(W32, stage))
        exact = oracle_stage(stage, cfg, W64, ins64)
        rnd = ROUND[prec if stage.startswith("block") else "fp16"]
        emul, factor = oracle_stage(stage, dataclasses.replace(cfg, rnd=rnd), W64, ins64), BAR_FACTOR
    assert exact.dtype == torch.float64 and emul.dtype in (torch.float64, torch.float32)
    return exact, {k: factor * v for k, v in metrics(emul, exact).items()}


def line(name: str, m: dict, bars: dict) -> str:
    return f"encoder stage {name}: " + "  ".join(f"{k} {m[k]:.2e} ({bars[k]:.1e})" for k in m)


def check(name: str, got: torch.Tensor, exact: torch.Tensor, bars: dict) -> dict:
    """Prints the figures with their bars, then asserts every one."""
    m = metrics(got, exact)
    print(line(name, m, bars))
    assert torch.isfinite(got).all(), name
    over = {k: (m[k], bars[k]) for k in m if not m[k] < bars[k]}
    assert not over, (name, over)
    return m
