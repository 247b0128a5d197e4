"""What the decoder's parity bars can see (CPU only).

tests/test_gpu_decoder.py holds wm_decoder_forward to DEC_TOL (tests/decoder_cases.py) against the reference in float64.  Here the
two-way transformer is restated with a `mutant` switch, one structural mistake per mutant -- the mistakes a rework of the decoder's
launch chain could make -- and each is measured, in float64, on every (profile, case) of the table: the relative L2 change of the
logits.  A mutant counts as visible in a case when it moves the logits by at least 3 x that case's DEC_TOL; every mutant must be
visible in at least one case.  ("At least one" is the rule: on `const` every key is equal, so swapping x and y changes nothing and a
stale keys + key_pe hardly anything.)  The fp32 CPU oracle must stay under DEC_TOL in every case: the bars are reachable by a
correct fp32 implementation.  With mutant=None the restatement equals O.decoder_forward bit for bit in fp32.
"""
import math

import pytest
import torch

from oracle import wm_oracle as O
import decoder_cases as DC

CFG = O.OracleCfg.from_model_type("vit_b")
HEADS = CFG.dec_heads

MUTANTS = {
    "eps": "LayerNorm eps 1e-6 instead of 1e-5",
    "l0_pe": "layer-0 self-attention with the query PE",
    "l0_res": "layer-0 self-attention with a residual",
    "l1_nope": "layer-1 self-attention without PE",
    "v_pe_self": "v with PE in the layer-1 self-attention",
    "v_pe": "v with PE in the token-to-image attentions",
    "stale_kpe": "keys + key_pe not rebuilt after the keys change",
    "i2t_nope": "image-to-token keys without the query PE",
    "pe_xy": "dense PE with x and y swapped",
    "pe_sincos": "dense PE with sin and cos swapped",
    "scale_hd": "attention scale 1/sqrt(E/8) where internal/8 belongs",
    "heads_interleaved": "heads split interleaved instead of blocked",
}


def attention(q, k, v, W, pre, mutant, embed_dim, chunk=1024):
    """transformer.py:217-240 (the oracle's dec_attention + mha_core, same operation order)."""
    lin = lambda x, n: x @ W[pre + n + ".weight"].t() + W[pre + n + ".bias"]
    q, k, v = lin(q, "q_proj"), lin(k, "k_proj"), lin(v, "v_proj")
    B, Nq, C = q.shape
    hd = C // HEADS
    if mutant == "heads_interleaved":                   # head h = channels h, h + 8, ...
        split = lambda x: x.reshape(B, -1, hd, HEADS).permute(0, 3, 1, 2)
    else:
        split = lambda x: x.reshape(B, -1, HEADS, hd).permute(0, 2, 1, 3)
    qh, kh, vh = split(q), split(k), split(v)
    scale = 1.0 / math.sqrt(embed_dim // HEADS if mutant == "scale_hd" else hd)
    outs = []
    for s in range(0, Nq, chunk):
        a = (qh[:, :, s:s + chunk] @ kh.transpose(-1, -2)) * scale
        outs.append(a.softmax(-1) @ vh)
    o = torch.cat(outs, dim=2)
    o = o.permute(0, 2, 3, 1).reshape(B, Nq, C) if mutant == "heads_interleaved" else o.permute(0, 2, 1, 3).reshape(B, Nq, C)
    return lin(o, "out_proj")


def decoder(emb, W, mutant=None):
    """box_decoder.py:96-147 + transformer.py:62-106 in the dtype of W, with one mistake if `mutant` names it."""
    assert mutant is None or mutant in MUTANTS
    dt = W["mask_decoder.mask_tokens.weight"].dtype
    pe = O.dense_pe(W["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"], CFG.grid, dtype=dt)
    if mutant == "pe_xy":
        pe = pe.transpose(2, 3).contiguous()
    if mutant == "pe_sincos":
        pe = torch.cat([pe[:, 128:], pe[:, :128]], 1)
    B, E = emb.shape[0], emb.shape[1]
    tokens = W["mask_decoder.mask_tokens.weight"].unsqueeze(0).expand(B, -1, -1)
    keys = emb.flatten(2).transpose(1, 2)
    kpe = pe.flatten(2).transpose(1, 2)
    queries, qpe = tokens, tokens
    t = "mask_decoder.transformer."
    eps = 1e-6 if mutant == "eps" else 1e-5
    ln = lambda x, n: O.layer_norm(x, W[n + ".weight"], W[n + ".bias"], eps)
    att = lambda q, k, v, p: attention(q, k, v, W, p, mutant, E)
    lin = lambda x, n: x @ W[n + ".weight"].t() + W[n + ".bias"]
    kpe_sum0 = keys + kpe
    for i in range(2):
        L = f"{t}layers.{i}."
        if i == 0:
            if mutant == "l0_pe":
                queries = att(queries + qpe, queries + qpe, queries, L + "self_attn.")
            elif mutant == "l0_res":
                queries = queries + att(queries, queries, queries, L + "self_attn.")
            else:
                queries = att(queries, queries, queries, L + "self_attn.")
        else:
            qq = queries if mutant == "l1_nope" else queries + qpe
            queries = queries + att(qq, qq, qq if mutant == "v_pe_self" else queries, L + "self_attn.")
        queries = ln(queries, L + "norm1")
        kk = kpe_sum0 if mutant == "stale_kpe" else keys + kpe
        queries = queries + att(queries + qpe, kk, kk if mutant == "v_pe" else keys, L + "cross_attn_token_to_image.")
        queries = ln(queries, L + "norm2")
        m = lin(torch.relu(lin(queries, L + "mlp.lin1")), L + "mlp.lin2")
        queries = ln(queries + m, L + "norm3")
        kq = queries if mutant == "i2t_nope" else queries + qpe
        keys = keys + att(keys + kpe, kq, queries, L + "cross_attn_image_to_token.")
        keys = ln(keys, L + "norm4")
    kk = kpe_sum0 if mutant == "stale_kpe" else keys + kpe
    queries = queries + att(queries + qpe, kk, kk if mutant == "v_pe" else keys, t + "final_attn_token_to_image.")
    queries = ln(queries, t + "norm_final_attn")

    def head(x, pre):
        for j in range(3):
            x = lin(x, f"{pre}layers.{j}")
            if j < 2:
                x = torch.relu(x)
        return x
    return head(queries, "mask_decoder.class_embed."), head(queries, "mask_decoder.bbox_embed.").sigmoid()


@pytest.fixture(scope="module")
def study():
    """Per (profile, case): the float64 logits, the fp32 CPU oracle's errors against them, every mutant's effect.  Computed once."""
    out = {}
    weights = {}
    with torch.no_grad():
        for profile, case in DC.TABLE:
            seed = DC.CASES[case][2]
            if (profile, seed) not in weights:
                W = DC.decoder_weights(profile, seed)
                weights[(profile, seed)] = (W, {k: v.double() for k, v in W.items()})
            W32, W64 = weights[(profile, seed)]
            emb = DC.case_embedding(case)
            lg64, bx64 = decoder(emb.double(), W64)
            ref32 = O.decoder_forward(emb, W32, CFG)
            mine32 = decoder(emb, W32)
            out[(profile, case)] = {
                "exact": torch.equal(mine32[0], ref32["pred_logits"]) and torch.equal(mine32[1], ref32["pred_boxes"]),
                "fp32": (DC.rel_l2(ref32["pred_logits"], lg64), DC.max_rel(ref32["pred_logits"], lg64), DC.max_abs(ref32["pred_boxes"], bx64)),
                "mutants": {m: DC.rel_l2(decoder(emb.double(), W64, m)[0], lg64) for m in MUTANTS},
            }
    return out


def test_restatement_equals_the_oracle_in_fp32(study):
    assert all(v["exact"] for v in study.values()), [k for k, v in study.items() if not v["exact"]]


def test_restatement_in_float64_equals_the_reference_fixture(golden_dir):
    """The mutants are measured against the restatement's own float64 result; that result is the reference's (1e-9, as in
    tests/test_oracle_small.py), here on one case."""
    import os
    import numpy as np
    fx = np.load(os.path.join(golden_dir, "decoder_ref.npz"))
    W64 = {k: v.double() for k, v in DC.decoder_weights("sensitive").items()}
    with torch.no_grad():
        lg, bx = decoder(DC.case_embedding("large").double(), W64)
    key = DC.fixture_key("sensitive", "large")
    assert DC.rel_l2(lg, torch.from_numpy(fx[key + "_logits"])) < 1e-9 and DC.max_abs(bx, torch.from_numpy(fx[key + "_boxes"])) < 1e-10


def test_fp32_cpu_oracle_is_under_every_bar(study):
    """A correct fp32 implementation reaches DEC_TOL (and, on the 7e4 activation, the bar the fp32-MFMA remedy is held to)."""
    bad = []
    for key in DC.TABLE:
        e, tol = study[key]["fp32"], DC.DEC_TOL[key]
        print(f"fp32 CPU oracle vs float64 {key[0]}/{key[1]}: logits rel-L2 {e[0]:.2e} max-rel {e[1]:.2e} boxes max-abs {e[2]:.2e}"
              f"  (bars {tol[0]:.0e} {tol[1]:.0e} {tol[2]:.0e})")
        if not (e[0] < tol[0] and e[1] < tol[1] and e[2] < tol[2]):
            bad.append((key, e, tol))
    for key, tol in DC.DEC_TOL_F32.items():
        e = study[key]["fp32"]
        if not (e[0] < tol[0] and e[1] < tol[1] and e[2] < tol[2]):
            bad.append((key, "fp32-MFMA bars", e, tol))
    W = DC.decoder_weights("baseline")
    emb = DC.overflow_embedding()
    with torch.no_grad():
        r32 = O.decoder_forward(emb, W, CFG)
        r64 = O.decoder_forward(emb.double(), {k: v.double() for k, v in W.items()}, CFG)
    e = (DC.rel_l2(r32["pred_logits"], r64["pred_logits"]), DC.max_rel(r32["pred_logits"], r64["pred_logits"]), DC.max_abs(r32["pred_boxes"], r64["pred_boxes"]))
    print(f"fp32 CPU oracle vs float64, 7e4 activation: {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
    if not all(x < t for x, t in zip(e, DC.DEC_TOL_F32_OVERFLOW)):
        bad.append(("overflow", e, DC.DEC_TOL_F32_OVERFLOW))
    assert not bad, bad


def test_every_mutant_shows_in_at_least_one_case(study):
    """The matrix: relative L2 change of the float64 logits per mutant and case, '*' where it is at least 3 x that case's DEC_TOL."""
    print("\n" + " " * 22 + " ".join(f"{m[:10]:>10}" for m in MUTANTS))
    seen = {m: [] for m in MUTANTS}
    for key in DC.TABLE:
        row = []
        for m in MUTANTS:
            eff = study[key]["mutants"][m]
            vis = eff >= 3 * DC.DEC_TOL[key][0]
            if vis:
                seen[m].append(key)
            row.append(f"{eff:9.1e}{'*' if vis else ' '}")
        print(f"{key[0] + '/' + key[1]:<20}  " + " ".join(row) + f"   bar {DC.DEC_TOL[key][0]:.0e}")
    for m, where in seen.items():
        print(f"{m:<18} visible in {len(where):2d} of {len(DC.TABLE)} cases  ({MUTANTS[m]})")
    hidden = [m for m, where in seen.items() if not where]
    assert not hidden, f"no case shows: {hidden}"
