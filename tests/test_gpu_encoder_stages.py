"""Every encoder stage alone (-m gpu): the path host_encoder.h builds -- FFT front, patch embed, HFC adaptor with its scramble, window
and global blocks with the folded LayerNorm / split-stream state machine, neck -- against the CPU oracle in float64, over the WHOLE
tensor of each stage, sliced by channel, grid row, grid column and token (tests/encoder_cases.py: stages, teacher forcing, metrics).

Every bar is computed in the test run from the oracle alone: 2 x the error of the oracle with the stage's operand rounding (fp16 /
bf16, float64 accumulation) against the exact float64 oracle on the same input; for the FFT 4 x the error of the fp32 CPU oracle.
tests/test_encoder_mutants.py shows on the CPU which structural mistakes these bars see.

ViT-B: hfc, patch, adaptor, blocks 0 and 1 (window), 2 (global), 11 (last), neck; blocks and neck in fp16 and bf16 mode; three tiles
(textured, padded 768 x 700, a bright patch in grid cell (63, 63)); batches 1, 2, 3 -- the three launch plans of encoder_cases.PLAN
(fold with the fp32 stream, no fold, fold + split stream), each asserted on the GEMM variant counters.  In a batch the checked tile
is the last.  ViT-H (N % 320, head dim 80): adaptor, block 6 (window), block 7 (global), neck, fp16, 1 and 4 tiles, last in the file.
One tap is read per forward; a repeated forward must repeat the tap's bits, which makes pairing taps of different forwards sound.

Measured figures: profiles/encoder_stages/ (README.md, gpu_tests.txt).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import wm_oracle as O          # checker only
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import synth
from wildlifemapper_amd.segment_anything import sam_model_registry
from wildlifemapper_amd.segment_anything.network import MedSAM
from wildlifemapper_amd.segment_anything.utils.misc import NestedTensor
import encoder_cases as EC
import gpu_util as G

MAX_BATCH = {"vit_b": max(EC.VIT_B_BATCHES), "vit_h": max(EC.VIT_H_BATCHES)}
_MODELS = {}
_TAPS = {}                                   # the taps of the latest (model, mode, tile, batch) only


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()
    yield
    _TAPS.clear()
    for k in list(_MODELS):
        _MODELS.pop(k)[0]._hub.close()


def _model(mt, prec):
    """(model, its encoder weights on the CPU); one model type resident at a time, as in test_gpu_e2e.py."""
    if mt not in _MODELS:
        for k in list(_MODELS):
            _MODELS.pop(k)[0]._hub.close()
        _TAPS.clear()
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(mt).items()}
        sam, _, _ = sam_model_registry[mt](None, None)
        m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
        m.load_state_dict(sd, strict=True)
        m._hub.max_batch = MAX_BATCH[mt]                    # one workspace for every batch size: the handle (and its tap) stays
        _MODELS[mt] = (m, {k: v for k, v in sd.items() if k.startswith("image_encoder.")})
    m, W = _MODELS[mt]
    m._hub.set_precision(prec)
    return m, W


def _forward_tap(m, x, hfc, which):
    """The last tile of tap `which` (or of the embedding, which = 'emb') of one image_encoder forward, on the CPU."""
    hub = m._hub
    n = x.shape[0]
    hub.set_tap(-2 if which == "emb" else which)
    with torch.no_grad():
        emb = m.image_encoder(x, hfc)
    out = emb[n - 1].permute(1, 2, 0) if which == "emb" else hub.read_tap(n)[n - 1]
    hub.set_tap(-2)
    return out.contiguous().cpu()


def _taps(mt, prec, kind, n, which):
    """{'x', 'hfc', 'emb', tap index: the LAST tile's tensor on the CPU} of a batch of n tiles; every tap is read from two forwards of
    the same input, which must agree bit for bit."""
    key = (mt, prec, kind, n)
    if key not in _TAPS:
        _TAPS.clear()
        m, _ = _model(mt, prec)
        x = EC.batch(kind, n).to(G.dev())
        m._hub.handle(x.device, n)
        hfc = m.fft(x)
        assert torch.equal(hfc, m.fft(x))
        _TAPS[key] = {"x": x[n - 1:].cpu(), "hfc": hfc[n - 1:].cpu(), "_dev": (x, hfc)}
    have = _TAPS[key]
    m, _ = _model(mt, prec)
    x, hfc = have["_dev"]
    m._hub.handle(x.device, n)                              # a mode switch in between closed the handle
    for w in which:
        if w not in have:
            have[w] = _forward_tap(m, x, hfc, w)
            assert torch.equal(have[w], _forward_tap(m, x, hfc, w)), f"tap {w} of a repeated forward differs"
    return have


def _run_stage(mt, prec, kind, n, stage):
    cfg = O.OracleCfg.from_model_type(mt)
    _, W = _model(mt, prec)
    ins, outs = EC.stage_taps(stage, cfg.depth)
    t = _taps(mt, prec, kind, n, tuple(k for k in ins + outs if k not in ("x", "hfc")))
    feed = {}
    for k in ins:
        if k in ("x", "hfc"):
            feed[k] = t[k]
        else:
            feed["t"] = t[k][None]
    if stage == "hfc":
        got = t["hfc"][0, 0].double()
    elif len(outs) == 2:
        got = t[outs[0]].double() - t[outs[1]].double()
    else:
        got = t[outs[0]].double()
    exact, bars = EC.study(stage, cfg, W, feed, prec)
    zeros = EC.zero_slices(exact)
    assert not any(zeros.values()), (stage, kind, zeros)     # the inputs are chosen so that no reference slice is zero
    EC.check(f"{mt}/{prec}/{kind}/b{n}/{stage}", got, exact, bars)


def _count_forward(mt, prec, n):
    m, _ = _model(mt, prec)
    x = EC.batch("textured", n).to(G.dev())
    m._hub.handle(x.device, n)
    hfc = m.fft(x)
    torch.cuda.synchronize()
    N.gemm_variant_counts(reset=True)
    with torch.no_grad():
        m.image_encoder(x, hfc)
    torch.cuda.synchronize()
    return {k: v for k, v in N.gemm_variant_counts(reset=True).items() if v}


# ---------------------------------------------------------------------------
# ViT-B
# ---------------------------------------------------------------------------
B_STAGES = EC.vit_b_stages()
B_FRONT = [(s, "fp16") for s in B_STAGES if not s.startswith("block") and s != "neck"]
B_MODAL = [(s, p) for p in ("fp16", "bf16") for s in B_STAGES if s.startswith("block") or s == "neck"]
# ordered so that the cases of one (mode, batch, tile) are neighbours: its taps are read once
B_TABLE = [(p, n, kind, s) for p in ("fp16", "bf16") for n in EC.VIT_B_BATCHES for kind in EC.TILES
           for s, sp in B_FRONT + B_MODAL if sp == p]


@pytest.mark.parametrize("prec,n", [(p, n) for p in ("fp16", "bf16") for n in EC.VIT_B_BATCHES])
def test_vit_b_launch_plan_is_the_recorded_one(prec, n):
    got = _count_forward("vit_b", prec, n)
    print(f"encoder launch plan vit_b/{prec}/b{n}: {got}")
    assert got == EC.PLAN[("vit_b", prec, n)]


@pytest.mark.parametrize("prec,n,kind,stage", B_TABLE)
def test_vit_b_stage_vs_float64_oracle(prec, n, kind, stage):
    _run_stage("vit_b", prec, kind, n, stage)


# ---------------------------------------------------------------------------
# the fused path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.VIT_B_BATCHES)
def test_fused_forward_taps_equal_the_two_call_path(n):
    """Taps -3 and -1 of m.detect (wm_forward: the FFT's last pass writes the 16-bit copies the patch embeds read) against m.fft
    followed by m.image_encoder (cvt_f32_to_16_kernel writes them): the same fp32 values through the same conversion, so the same
    bits."""
    m, _ = _model("vit_b", "fp16")
    hub = m._hub
    x = EC.batch("textured", n).to(G.dev())
    hub.handle(x.device, n)
    hfc = m.fft(x)
    sizes = torch.tensor([[1024, 1024]] * n)
    for which in (-3, -1):
        hub.set_tap(which)
        with torch.no_grad():
            m.image_encoder(x, hfc)
        two_call = hub.read_tap(n).clone()
        m.detect(NestedTensor(x, None), sizes)
        fused = hub.read_tap(n).clone()
        hub.set_tap(-2)
        same = torch.equal(two_call, fused)
        diff = (two_call.double() - fused.double()).abs().max().item()
        print(f"fused vs two-call tap {which} b{n}: identical {same}, max-abs difference {diff:.2e}")
        assert same, (which, n, diff)


# ---------------------------------------------------------------------------
# ViT-H, the product shape.  Last in the file: the resident model is replaced.
# ---------------------------------------------------------------------------
H_STAGES = ("adaptor", "block6", "block7", "neck")


@pytest.mark.parametrize("n", EC.VIT_H_BATCHES)
def test_vit_h_launch_plan_is_the_recorded_one(n):
    got = _count_forward("vit_h", "fp16", n)
    print(f"encoder launch plan vit_h/fp16/b{n}: {got}")
    assert got == EC.PLAN[("vit_h", "fp16", n)]


@pytest.mark.parametrize("n,stage", [(n, s) for n in EC.VIT_H_BATCHES for s in H_STAGES])
def test_vit_h_stage_vs_float64_oracle(n, stage):
    _run_stage("vit_h", "fp16", "textured", n, stage)
