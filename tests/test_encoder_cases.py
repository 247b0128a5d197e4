"""CPU checks of what the encoder's stage tests stand on: the oracle's encoder path stays in float64, its rounding helpers keep their
fp32 bits, the metrics treat zero slices as written, the launch-plan table agrees with gemm16_takes_v5's rule."""
import dataclasses

import pytest
import torch

from oracle import wm_oracle as O
from wildlifemapper_amd import synth
import encoder_cases as EC


def _tiny():
    """A 2-block encoder (window, global) of width 64 on the real grid and image size; the weights of every stage, fp32."""
    cfg = O.OracleCfg(embed_dim=64, depth=2, num_heads=2, global_attn_indexes=(1,))
    e, a = "image_encoder.", "image_encoder.hfc_attn."
    D, H, G = 64, cfg.hfc_dim, cfg.grid
    shapes = {e + "pos_embed": (1, G, G, D), e + "patch_embed.proj.weight": (D, 3, 16, 16), e + "patch_embed.proj.bias": (D,),
              e + "hfc_embed.proj.weight": (H, 1, 16, 16), e + "hfc_embed.proj.bias": (H,), a + "pos_embed": (1, H, G, G),
              a + "proj_hfc.weight": (H, H, 1, 1), a + "proj_hfc.bias": (H,), a + "proj_patch.weight": (H, D, 1, 1),
              a + "proj_patch.bias": (H,), a + "cross_attn.in_proj_weight": (3 * H, H), a + "cross_attn.in_proj_bias": (3 * H,),
              a + "cross_attn.out_proj.weight": (H, H), a + "cross_attn.out_proj.bias": (H,), a + "proj_back.weight": (D, H, 1, 1),
              a + "proj_back.bias": (D,), e + "neck.0.weight": (256, D, 1, 1), e + "neck.1.weight": (256,), e + "neck.1.bias": (256,),
              e + "neck.2.weight": (256, 256, 3, 3), e + "neck.3.weight": (256,), e + "neck.3.bias": (256,)}
    for nm in ("linear1", "linear2"):
        shapes[a + nm + ".weight"], shapes[a + nm + ".bias"] = (H, H), (H,)
    for nm in ("norm1", "norm2"):
        shapes[a + nm + ".weight"], shapes[a + nm + ".bias"] = (H,), (H,)
    for i, size in ((0, cfg.window), (1, G)):
        b = f"{e}blocks.{i}."
        shapes.update({b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.rel_pos_h": (2 * size - 1, D // 2),
                       b + "attn.rel_pos_w": (2 * size - 1, D // 2), b + "attn.qkv.weight": (3 * D, D), b + "attn.qkv.bias": (3 * D,),
                       b + "attn.proj.weight": (D, D), b + "attn.proj.bias": (D,), b + "norm2.weight": (D,), b + "norm2.bias": (D,),
                       b + "mlp.lin1.weight": (4 * D, D), b + "mlp.lin1.bias": (4 * D,), b + "mlp.lin2.weight": (D, 4 * D),
                       b + "mlp.lin2.bias": (D,)})
    return cfg, {k: torch.from_numpy(synth.make_weight(k, s)) for k, s in shapes.items()}


@pytest.mark.parametrize("rnd", [None, "fp16", "bf16"])
def test_every_encoder_stage_stays_in_float64(rnd):
    """float64 inputs and weights give float64 out of every stage function, with and without emulated operand rounding, and the
    float64 result is the fp32 one to fp32's precision (so nothing inside fell back to fp32 and was widened again)."""
    cfg, W = _tiny()
    if rnd:
        cfg = dataclasses.replace(cfg, rnd=EC.ROUND[rnd])
    W64 = EC.to64(W)
    x = EC.tile("spike")
    with torch.no_grad():
        hfc = O.hfc_fft(x)
        t = torch.from_numpy(synth.fill_normal(0, "tiny.stream", (1, 64, 64, 64), 1.0))
        feeds = {"hfc": {"x": x}, "patch": {"x": x}, "adaptor": {"hfc": hfc, "t": t}, "block0": {"t": t}, "block1": {"t": t}, "neck": {"t": t}}
        for stage, feed in feeds.items():
            if rnd and stage in ("hfc", "adaptor", "block1"):          # the rounding helpers are the same in every stage
                continue
            got = EC.oracle_stage(stage, cfg, W64, EC.to64(feed))
            assert got.dtype == torch.float64, stage
            if rnd is None:
                ref = EC.oracle_stage(stage, cfg, W, feed)
                assert ref.dtype == torch.float32
                assert EC.metrics(ref, got)["rel_l2"] < 2e-6, stage
        if rnd is None:
            assert O.encoder_forward(x.double(), hfc.double(), W64, cfg).dtype == torch.float64


def test_rounding_helpers_keep_dtype_and_fp32_bits():
    g = torch.Generator().manual_seed(0)
    t = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 7e4, -7e4, 500.0, 65504.0, 1e-8])])
    old = {"bf16": t.to(torch.bfloat16).to(torch.float32), "fp16": t.clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32),
           "e4m3": t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)}
    for name, fn in (("bf16", O.bf16_round), ("fp16", O.fp16_round), ("e4m3", O.e4m3_round)):
        got = fn(t)
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), old[name].view(torch.int32)), name
        wide = fn(t.double())
        assert wide.dtype == torch.float64 and torch.equal(wide, old[name].double()), name      # fp32 values: one rounding either way


def test_metrics_zero_slice_and_families():
    ref = torch.zeros(64, 64, 8, dtype=torch.float64)
    ref[:, :, 0] = 3.0                                        # channels 1..7 are zero slices; every row, column, token is not
    got = ref.clone()
    got[5, 63, 2] += 0.3                                      # an error in a zero channel, the last column
    m = EC.metrics(got, ref)
    chan_norm = 3.0 * 64
    assert EC.zero_slices(ref) == {"channel": 7, "row": 0, "col": 0, "token": 0}
    assert m["channel"] == pytest.approx(0.3 / chan_norm)    # absolute error against the family's largest norm
    assert m["token"] == pytest.approx(0.1) and m["max_rel"] == pytest.approx(0.1)
    assert m["col"] == pytest.approx(0.3 / (3.0 * 8)) and m["row"] == pytest.approx(0.3 / (3.0 * 8))
    assert m["rel_l2"] == pytest.approx(0.3 / (3.0 * 64))
    img = EC.metrics(torch.ones(16, 16), torch.ones(16, 16) * 2)
    assert set(img) == {"rel_l2", "max_rel", "row", "col"} and img["row"] == pytest.approx(0.5)


def test_launch_plan_batches_follow_the_dispatch_rule():
    """The batch sizes of the GPU test are the smallest of each regime of gemm16_takes_v5's rule."""
    assert [EC.regime(768, n) for n in (1, 2, 3)] == ["fold", "plain", "split"] and EC.VIT_B_BATCHES == (1, 2, 3)
    assert [EC.regime(1280, n) for n in (1, 2, 3, 4)] == ["fold", "plain", "split", "split"] and EC.VIT_H_BATCHES == (1, 4)
    for key in [("vit_b", p, n) for p in ("fp16", "bf16") for n in EC.VIT_B_BATCHES] + [("vit_h", "fp16", n) for n in EC.VIT_H_BATCHES]:
        assert key in EC.PLAN, key
    # the rule against the library's own answer, where the library is built
    from wildlifemapper_amd import _native as N
    lib = N.lib()
    for M in (4096, 8192, 12288, 16384):
        for Nn, K in ((2304, 768), (3072, 768), (768, 768), (768, 3072), (1024, 1024), (2048, 1024), (256, 768), (3840, 1280), (1280, 5120)):
            assert bool(lib.wm_op_gemm16_takes_packed(M, Nn, K)) == EC.takes_v5(M, Nn, K), (M, Nn, K)


def test_tiles_are_what_the_cases_say():
    pad, spike, tex = EC.tile("padded"), EC.tile("spike"), EC.tile("textured")
    h, w = EC.PADDED
    assert pad[:, :, h:, :].abs().max() == 0 and pad[:, :, :, w:].abs().max() == 0 and pad[:, :, :h, :w].abs().min() > 0
    r, c, f = EC.SPIKE
    assert (r, c) == (63, 63) and spike[:, :, 1008:, 1008:].abs().max() > 0.5 * f * tex.abs().max()
    b = EC.batch("spike", 3)
    assert b.shape == (3, 3, 1024, 1024) and torch.equal(b[2:], spike) and not torch.equal(b[0], b[1])
