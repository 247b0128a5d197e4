"""The box decoder's parity cases: what oracle/gen_golden.py --only decoder, tests/test_oracle_small.py, tests/test_decoder_mutants.py
and tests/test_gpu_decoder.py share.  Plain module (torch on the CPU only): the case table, the seeded embedding generator, the
synthetic decoder weights and the tolerance table the GPU test asserts.

tests/golden/decoder_ref.npz holds only the reference's float64 outputs of these cases; the embeddings are made here.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

PROFILES = ("baseline", "sensitive")
EMBEDDINGS = ("unit", "small", "large", "smooth", "const", "spike")
SPIKE = (1, 17, 41, 1.0e3)          # tile, grid row, grid column, factor of the `spike` case

# case name -> (embedding kind, batch, weight seed)
CASES = {k: (k, 2, 0) for k in EMBEDDINGS}
CASES["unit_seed1"] = ("unit", 2, 1)
CASES["unit_b3"] = ("unit", 3, 0)    # Mq = 153: a ragged last GEMM tile
TABLE = [(p, c) for p in PROFILES for c in CASES]


def fixture_key(profile: str, case: str) -> str:
    return f"{profile}__{case}"


def embedding(kind: str, batch: int = 2, seed: int = 0) -> torch.Tensor:
    """(batch, 256, 64, 64) fp32.  unit: randn; small: randn * 1e-2 (the low range of the split GEMM); large: randn * 30 (a peaky
    token-to-image softmax); smooth: an 8 x 8 random grid, bilinear to 64 x 64; const: one random vector at all 4096 positions
    (every key equal: a uniform softmax); spike: unit with one token of one tile scaled by 1e3."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(batch, 256, 64, 64, generator=g)
    if kind == "unit":
        return e
    if kind == "small":
        return e * 1e-2
    if kind == "large":
        return e * 30
    if kind == "smooth":
        return F.interpolate(torch.randn(batch, 256, 8, 8, generator=g), size=64, mode="bilinear").contiguous()
    if kind == "const":
        return torch.randn(batch, 256, 1, 1, generator=g).expand(batch, 256, 64, 64).contiguous()
    if kind == "spike":
        b, y, x, f = SPIKE
        e[b % batch, :, y, x] *= f
        return e
    raise KeyError(kind)


def case_embedding(case: str) -> torch.Tensor:
    kind, batch, _ = CASES[case]
    return embedding(kind, batch)


def decoder_weights(profile: str, seed: int = 0) -> dict:
    """Synthetic ViT-B decoder-side weights (mask_decoder.* and the prompt encoder's gaussian matrix) as fp32 torch tensors."""
    from wildlifemapper_amd import synth
    sd = {}
    for pre in ("mask_decoder.", "prompt_encoder."):
        sd.update(synth.make_state_dict("vit_b", seed, only_prefix=pre, profile=profile))
    return {k: torch.from_numpy(v.copy()) for k, v in sd.items()}


def case_weights(profile: str, case: str) -> dict:
    return decoder_weights(profile, CASES[case][2])


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def max_rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """max-abs difference relative to the largest reference value."""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def max_abs(a: torch.Tensor, b: torch.Tensor) -> float:
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# What tests/test_gpu_decoder.py asserts: (logits relative L2, logits max-abs relative to the largest logit, boxes max-abs) of
# wm_decoder_forward against the float64 fixture.  Each bar is 4 x the error measured on the MI355X for that (profile, case), rounded
# up to one significant digit (the measured values are in tests/test_gpu_decoder.py's docstring and profiles/decoder_parity/).
# tests/test_decoder_mutants.py checks that every structural mutant moves the float64 logits by at least 3 x the first bar in at
# least one case, and that the fp32 CPU oracle stays under every bar.
# ---------------------------------------------------------------------------------------------------------------------------------
DEC_TOL = {                                                   # measured on the MI355X (same three figures)
    ("baseline", "unit"): (2e-06, 3e-06, 9e-07),              # 3.92e-07 5.25e-07 2.21e-07
    ("baseline", "small"): (2e-06, 3e-06, 9e-07),             # 4.08e-07 5.37e-07 2.12e-07
    ("baseline", "large"): (7e-06, 2e-05, 6e-06),             # 1.65e-06 2.76e-06 1.30e-06
    ("baseline", "smooth"): (2e-06, 3e-06, 9e-07),            # 3.70e-07 5.22e-07 2.21e-07
    ("baseline", "const"): (2e-06, 3e-06, 8e-07),             # 4.17e-07 5.30e-07 1.84e-07
    ("baseline", "spike"): (3e-06, 2e-05, 5e-06),             # 6.51e-07 3.45e-06 1.07e-06
    ("baseline", "unit_seed1"): (2e-06, 3e-06, 8e-07),        # 4.36e-07 5.16e-07 1.76e-07
    ("baseline", "unit_b3"): (2e-06, 3e-06, 9e-07),           # 3.94e-07 5.32e-07 2.21e-07
    ("sensitive", "unit"): (2e-06, 3e-06, 8e-07),             # 4.77e-07 6.42e-07 1.96e-07
    ("sensitive", "small"): (2e-06, 3e-06, 8e-07),            # 3.62e-07 5.47e-07 1.97e-07
    ("sensitive", "large"): (2e-05, 4e-05, 2e-05),            # 3.12e-06 8.38e-06 3.55e-06
    ("sensitive", "smooth"): (2e-06, 2e-06, 1e-06),           # 3.89e-07 4.97e-07 2.29e-07
    ("sensitive", "const"): (2e-06, 2e-06, 9e-07),            # 3.24e-07 4.68e-07 2.16e-07
    ("sensitive", "spike"): (2e-06, 3e-06, 8e-07),            # 4.59e-07 5.46e-07 1.91e-07
    ("sensitive", "unit_seed1"): (2e-06, 4e-06, 8e-07),       # 4.59e-07 7.85e-07 1.88e-07
    ("sensitive", "unit_b3"): (2e-06, 3e-06, 9e-07),          # 4.80e-07 6.22e-07 2.09e-07
}

# the same with WM_GEMM32_F32=1 (the fp32-MFMA GEMMs the overflow warning names as the remedy), for the two cases its test runs
DEC_TOL_F32 = {
    ("baseline", "unit"): (3e-06, 4e-06, 2e-06),              # 7.42e-07 8.47e-07 3.61e-07
    ("sensitive", "large"): (2e-05, 4e-05, 3e-05),            # 4.84e-06 8.74e-06 5.45e-06
}

# WM_GEMM32_F32=1 on overflow_embedding(), against the live float64 oracle.  Not a measured bar: the fp32 CPU oracle is 3.1e-6 /
# 2.3e-5 / 4.6e-6 from float64 on that input (the 7e4 token makes some softmaxes one-hot); 4 x that, rounded up to one digit.
DEC_TOL_F32_OVERFLOW = (2e-5, 1e-4, 2e-5)


def overflow_embedding() -> torch.Tensor:
    """`unit` with one value of 7e4: outside fp16's range (65504), so the fp16-split GEMMs cannot take it as an operand; the fp32-MFMA
    GEMMs (WM_GEMM32_F32=1) can.  Not in the fixture: checked against the live float64 oracle."""
    e = embedding("unit", 2)
    e[0, 5, 10, 10] = 7.0e4
    return e
