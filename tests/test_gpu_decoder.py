"""The box decoder alone (-m gpu): wm_decoder_forward through a standalone drop-in MaskDecoder (a decoder-only native handle: no
encoder weights, no encoder run) against the reference's own decoder in float64 (tests/golden/decoder_ref.npz, written by
oracle/gen_golden.py --only decoder), on the cases of tests/decoder_cases.py.

The end-to-end tests hold the decoder only to the encoder's 16-bit operand rounding (2e-4 .. 9.8e-4 on the logits); the decoder is
fp32 throughout and is held here to DEC_TOL (tests/decoder_cases.py): per case 4 x the error measured on the MI355X, rounded up to
one significant digit.  tests/test_decoder_mutants.py shows on the CPU that every structural mistake (eps, a PE added or left out,
a stale keys + key_pe, x / y or sin / cos swapped, the wrong head dimension or head split) moves the logits by at least 3 x such a
bar in at least one case, and that a correct fp32 implementation (the CPU oracle) stays under every bar.

MEASURED on the MI355X (profiles/decoder_parity/gpu_tests.txt; the figures of every case stand beside its bars in
tests/decoder_cases.py), as logits relative L2 / logits max-abs relative to the largest logit / boxes max-abs:
  the 12 cases at unit, small, smooth, const scale (both profiles, seed 1, B = 3)   3.2e-7 .. 4.8e-7 / 4.7e-7 .. 7.9e-7 / 1.8e-7 .. 2.3e-7
                                                                 -> bars 2e-6 / 2e-6 .. 4e-6 / 8e-7 .. 1e-6
  baseline/spike     6.5e-7 / 3.5e-6 / 1.1e-6 -> 3e-6 / 2e-5 / 5e-6     sensitive/spike    4.6e-7 / 5.5e-7 / 1.9e-7 -> 2e-6 / 3e-6 / 8e-7
  baseline/large     1.7e-6 / 2.8e-6 / 1.3e-6 -> 7e-6 / 2e-5 / 6e-6     sensitive/large    3.1e-6 / 8.4e-6 / 3.6e-6 -> 2e-5 / 4e-5 / 2e-5
  WM_GEMM32_F32=1:  baseline/unit 7.4e-7 / 8.5e-7 / 3.6e-7 -> 3e-6 / 4e-6 / 2e-6;  sensitive/large 4.8e-6 / 8.7e-6 / 5.5e-6 -> 2e-5 / 4e-5 / 3e-5;
                    the 7e4 activation against the live float64 oracle 1.3e-6 / 7.7e-6 / 1.5e-6 (bar from the fp32 CPU oracle: 2e-5 / 1e-4 / 2e-5)
The split-GEMM decoder is closer to float64 than the fp32 CPU oracle (7.1e-7 .. 8.8e-7, `large` 2.6e-6 and 4.9e-6, baseline/spike
1.6e-6) and than the fp32-MFMA kernel; the smallest mutant effect in any case that counts it is 8 x its bar (stale keys + key_pe on
baseline/small: 1.6e-5 against 2e-6), LayerNorm eps 1e-6 is 21 x (4.3e-5 .. 5.4e-5 at unit scale).  No case needed investigation:
every case satisfies both the 4 x rule and the one-third rule.

Bit-for-bit checks need no tolerance: a tile's result does not depend on its batch neighbours or position; batches that grow and
shrink on one handle (the key-split attention's partials are reallocated when the batch grows) equal fresh handles; a repeated call
repeats and the input is left alone; the standalone decoder equals the mask_decoder of a full model whose encoder ran first on the
same handle (keys + key_pe lives in the neck's scratch); a decoder-side weight changed in place is followed by everything the handle
derives from it (the cached fp16 planes of the split GEMM, keyed by device address, and the dense PE built from the gaussian matrix).

The range watch: an activation outside fp16's range raises the decoder's overflow bit (wm_stream_overflow bit 2) and the drop-in
warns at the next call; the remedy the warning names (WM_GEMM32_F32=1, read once per process: a child process) runs the decoder on
the fp32-MFMA GEMMs, meets its own bars on the fixture and takes that activation without an overflow.
"""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import wm_oracle as O          # checker only
from wildlifemapper_amd.segment_anything.modeling import MaskDecoder, PromptEncoder, TwoWayTransformer
import decoder_cases as DC
import gpu_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = O.OracleCfg.from_model_type("vit_b")
MAX_BATCH = 4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()
    yield
    for dec, _ in _DECODERS.values():
        if dec._hub is not None:
            dec._hub.close()
    _DECODERS.clear()


@pytest.fixture(scope="module")
def ref(golden_dir):
    fx = np.load(os.path.join(golden_dir, "decoder_ref.npz"))
    assert int(fx["pinned"]) == 1
    return fx


def build_decoder(profile, seed=0):
    """A standalone MaskDecoder + PromptEncoder of the drop-in package with the synthetic decoder weights only."""
    dec = MaskDecoder(num_multimask_outputs=50, transformer=TwoWayTransformer(depth=2, embedding_dim=256, mlp_dim=2048, num_heads=8),
                      transformer_dim=256, iou_head_depth=3, iou_head_hidden_dim=256).eval()
    pe = PromptEncoder(embed_dim=256, image_embedding_size=(64, 64), input_image_size=(1024, 1024), mask_in_chans=16).eval()
    W = DC.decoder_weights(profile, seed)
    dec.load_state_dict({k[len("mask_decoder."):]: v for k, v in W.items() if k.startswith("mask_decoder.")}, strict=True)
    pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in W.items() if k.startswith("prompt_encoder.")}, strict=True)
    dec._ensure_hub(pe.get_dense_pe()).max_batch = MAX_BATCH          # one workspace for every batch size the tests use
    return dec, pe


_DECODERS = {}


def decoder(profile, seed=0):
    if (profile, seed) not in _DECODERS:
        _DECODERS[(profile, seed)] = build_decoder(profile, seed)
    return _DECODERS[(profile, seed)]


def run(dec, pe, emb):
    """(logits, boxes) of one mask_decoder call, as clones."""
    with torch.no_grad():
        out = dec(image_embeddings=emb.to(G.dev()), image_pe=pe.get_dense_pe(), sparse_prompt_embeddings=None,
                  dense_prompt_embeddings=None, multimask_output=False, hfc_embed=None)
    return out["pred_logits"].clone(), out["pred_boxes"].clone()


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def errors(got, lg, bx):
    return DC.rel_l2(got[0], lg), DC.max_rel(got[0], lg), DC.max_abs(got[1], bx)


def live_oracle64(dec, pe, emb):
    """The float64 oracle on the modules' current weights."""
    W = {"mask_decoder." + k: v.detach().cpu().double() for k, v in dec.state_dict().items()}
    W.update({"prompt_encoder." + k: v.detach().cpu().double() for k, v in pe.state_dict().items()})
    with torch.no_grad():
        out = O.decoder_forward(emb.double(), W, CFG)
    return out["pred_logits"], out["pred_boxes"]


def check(name, got, lg, bx, tol):
    el, em, eb = errors(got, lg, bx)
    print(f"decoder parity {name}: logits rel-L2 {el:.2e} max-rel {em:.2e} boxes max-abs {eb:.2e}  (bars {tol[0]:.0e} {tol[1]:.0e} {tol[2]:.0e})")
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), name
    assert el < tol[0] and em < tol[1] and eb < tol[2], (name, el, em, eb, tol)


# ---------------------------------------------------------------------------
# parity with the reference in float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("profile,case", DC.TABLE)
def test_decoder_vs_float64_reference(profile, case, ref):
    dec, pe = decoder(profile, DC.CASES[case][2])
    key = DC.fixture_key(profile, case)
    got = run(dec, pe, DC.case_embedding(case))
    assert dec._hub._handle is not None and set(dec._hub._sources) == {"mask_decoder.", "prompt_encoder."}      # decoder-only handle
    check(f"{profile}/{case}", got, torch.from_numpy(ref[key + "_logits"]), torch.from_numpy(ref[key + "_boxes"]),
          DC.DEC_TOL[(profile, case)])


# ---------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------
def test_tile_result_does_not_depend_on_batch_or_position():
    dec, pe = decoder("baseline")
    e = DC.embedding("unit", 4)
    alone = run(dec, pe, e[1:2])
    first3 = run(dec, pe, torch.stack([e[1], e[0], e[2]]))
    last4 = run(dec, pe, torch.stack([e[0], e[2], e[3], e[1]]))
    assert torch.equal(alone[0][0], first3[0][0]) and torch.equal(alone[1][0], first3[1][0])
    assert torch.equal(alone[0][0], last4[0][3]) and torch.equal(alone[1][0], last4[1][3])
    assert not torch.equal(alone[0][0], first3[0][1])


def test_growing_batches_on_one_handle_equal_fresh_handles():
    """Call sizes 1, 4, 2, 3 on one handle (launch_mha32 reallocates the key-split partials when the batch grows) against a fresh
    handle per size."""
    dec, pe = build_decoder("baseline")
    hub = dec._hub
    try:
        e = DC.embedding("unit", 4)
        sizes = (1, 4, 2, 3)
        live, handles = [], set()
        for n in sizes:
            live.append(run(dec, pe, e[:n]))
            handles.add(hub._handle.value)
        assert len(handles) == 1 and hub.max_batch == MAX_BATCH          # one handle served all four
        for n, got in zip(sizes, live):
            hub.close()
            assert same_bits(run(dec, pe, e[:n]), got), n
    finally:
        hub.close()


def test_repeat_gives_same_bits_and_input_is_unchanged():
    dec, pe = decoder("sensitive")
    e = DC.embedding("large", 2).to(G.dev())
    keep = e.clone()
    a = run(dec, pe, e)
    b = run(dec, pe, e)
    assert same_bits(a, b)
    assert torch.equal(e, keep)


def test_standalone_decoder_equals_full_model_decoder():
    """The same embedding through the mask_decoder of a full ViT-B MedSAM, after that model's encoder and fused forward ran on the
    same handle (keys + key_pe lives in the neck's scratch), and through the standalone decoder: the same bits."""
    from wildlifemapper_amd import synth
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    from wildlifemapper_amd.segment_anything.utils.misc import NestedTensor
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict("vit_b").items()}
    sam, _, _ = sam_model_registry["vit_b"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    m.load_state_dict(sd, strict=True)
    try:
        x = torch.from_numpy(synth.make_batch(0, 2)).to(G.dev())
        with torch.no_grad():
            emb_model = m.image_encoder(x, m.fft(x))
            fused = m(NestedTensor(x, None), None)
        assert torch.isfinite(fused["pred_logits"]).all()
        dec, pe = decoder("baseline")
        for emb in (DC.embedding("unit", 2), emb_model.cpu()):
            full = run(m.mask_decoder, m.prompt_encoder, emb)
            assert same_bits(run(dec, pe, emb), full)
        assert torch.equal(full[0], fused["pred_logits"])
    finally:
        m._hub.close()


def test_partial_reupload_of_decoder_weights_matches_fresh_handle():
    """Decoder-side tensors changed in place, one after another: a GEMM weight (its cached fp16 planes are keyed by device address),
    the token table (tokens and query PE), a LayerNorm gamma, and the gaussian matrix alone (the dense PE is rebuilt only when it is
    staged).  After each the live handle equals a fresh one bit for bit, meets the live float64 oracle on the changed weights within
    DEC_TOL of (baseline, unit), and differs from the result before the change."""
    dec, pe = build_decoder("baseline")
    hub = dec._hub
    tr = dec.transformer
    gauss = pe.pe_layer.positional_encoding_gaussian_matrix
    steps = [("k_proj", tr.layers[1].cross_attn_image_to_token.k_proj.weight, lambda t: t.mul_(1.5)),
             ("mask_tokens", dec.mask_tokens.weight, lambda t: t.mul_(1.1)),
             ("norm3", tr.layers[0].norm3.weight, lambda t: t.mul_(1.2)),
             ("gaussian", gauss, lambda t: t.mul_(1.25))]
    saved = [t.detach().clone() for _, t, _ in steps]
    emb = DC.embedding("unit", 2)
    tol = DC.DEC_TOL[("baseline", "unit")]
    try:
        before = run(dec, pe, emb)
        first = before
        handle = hub._handle.value
        for name, t, change in steps:
            with torch.no_grad():
                change(t)
            again = run(dec, pe, emb)                                  # partial re-upload into the live handle
            assert hub._handle.value == handle, name
            assert not torch.equal(again[0], before[0]), name
            check(f"re-upload {name}", again, *live_oracle64(dec, pe, emb), tol)
            hub.close()                                                # fresh handle, full upload of the same weights
            fresh = run(dec, pe, emb)
            assert same_bits(again, fresh), name
            handle = hub._handle.value
            before = again
    finally:
        with torch.no_grad():
            for (_, t, _), s0 in zip(steps, saved):
                t.copy_(s0)
        hub.close()
    assert same_bits(run(dec, pe, emb), first)
    hub.close()


# ---------------------------------------------------------------------------
# the range watch and its remedy
# ---------------------------------------------------------------------------
def test_activation_outside_fp16_range_is_loud():
    dec, pe = decoder("baseline")
    hub = dec._hub
    emb = DC.embedding("unit", 2)
    run(dec, pe, emb)
    torch.cuda.synchronize()
    hub.stream_overflow(reset=True)
    clean = run(dec, pe, emb)
    torch.cuda.synchronize()
    assert hub.stream_overflow(reset=True) == 0
    run(dec, pe, DC.overflow_embedding())
    torch.cuda.synchronize()
    assert hub.stream_overflow() & 2
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        again = run(dec, pe, emb)
    assert any("WM_GEMM32_F32" in str(i.message) for i in w), [str(i.message) for i in w]
    torch.cuda.synchronize()
    assert hub.stream_overflow(reset=True) == 0 and same_bits(again, clean)


REMEDY_CASES = (("baseline", "unit"), ("sensitive", "large"))


def remedy_child(golden_dir):
    """Runs in a child process started with WM_GEMM32_F32=1: prints every figure, then one 'remedy ok' line per check that held;
    exits non-zero if one did not."""
    assert os.environ.get("WM_GEMM32_F32") == "1"
    fx = np.load(os.path.join(golden_dir, "decoder_ref.npz"))
    bad = []

    def held(name, *args):
        try:
            check("fp32-MFMA " + name, *args)
            print(f"remedy ok {name}")
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])

    for profile, case in REMEDY_CASES:
        dec, pe = decoder(profile)
        key = DC.fixture_key(profile, case)
        held(f"{profile}/{case}", run(dec, pe, DC.case_embedding(case)), torch.from_numpy(fx[key + "_logits"]),
             torch.from_numpy(fx[key + "_boxes"]), DC.DEC_TOL_F32[(profile, case)])
    dec, pe = decoder("baseline")
    hub = dec._hub
    torch.cuda.synchronize()
    hub.stream_overflow(reset=True)
    emb = DC.overflow_embedding()
    got = run(dec, pe, emb)
    torch.cuda.synchronize()
    print(f"fp32-MFMA overflow word {hub.stream_overflow(reset=True)}")
    held("7e4 activation", got, *live_oracle64(dec, pe, emb), DC.DEC_TOL_F32_OVERFLOW)
    for d, _ in _DECODERS.values():
        d._hub.close()
    assert not bad, bad


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_decoder as T
T.remedy_child(sys.argv[1] + "/tests/golden")
"""


def test_fp32_mfma_remedy_in_child_process():
    """WM_GEMM32_F32=1 is read once per process: one fresh child runs the decoder on the fp32-MFMA GEMMs against the fixture
    (DEC_TOL_F32, measured with that kernel) and on the 7e4 activation (finite, no overflow bit, the live float64 oracle)."""
    env = dict(os.environ, WM_GEMM32_F32="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=180)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2000:]
    for profile, case in REMEDY_CASES:
        assert f"remedy ok {profile}/{case}" in r.stdout
    assert "fp32-MFMA overflow word 0" in r.stdout and "remedy ok 7e4 activation" in r.stdout
