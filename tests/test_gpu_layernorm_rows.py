"""The LayerNorm family row by row on hard row statistics (-m gpu).

Every kernel that computes or consumes LayerNorm statistics -- layernorm_kernel, layernorm_tiled_kernel, ln_stats_x16_kernel, the
FOLDP / SPLIT producers and the FOLDC consumer of gemm16_v5.h, layernorm_plane_fp8_kernel -- on the row families of
tests/layernorm_cases.py (|mean| / std from 0 to 3e5, std from 0 to 800, exact rows, spikes at the statistics tiles' edges), judged
per row against float64 computed with torch on the device.  Every bar is computed in the run from the oracle and the emulations of
layernorm_cases.py (its docstring has the rules and the derivations); each test prints one line of per-family worst rows and names
the families and rows that stand over their bars.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util as G
import encoder_cases as EC
import layernorm_cases as LC
from wildlifemapper_amd import _native as Nn
from wildlifemapper_amd import synth

EPS_OF = {256: 1e-5, 768: 1e-6, 1024: 1e-5, 1280: 1e-6}       # the neck's and the blocks' eps
GUARD = 8                                                     # poisoned rows before and after an output


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()
    torch.manual_seed(0)


@functools.lru_cache(maxsize=4)
def _case(C, n_rows, block):
    x, fam = LC.rows(C, n_rows, seed=C + n_rows, block=block)
    return x.to(G.dev()), fam


def _variants_run(fn):
    """Run fn() and return (its result, {GEMM kernel instance: launches}) from wm_debug_gemm_variant_counts, as test_gpu_ops.py does."""
    Nn.gemm_variant_counts(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v for k, v in Nn.gemm_variant_counts().items() if v}


def _weights(C, N, prec):
    return tuple(t.to(G.dev()) for t in LC.params(C, N, prec))


def _guarded(rows, C, dtype):
    """(the whole buffer, its interior [rows, C]): NaN guard rows around an output, the interior 16-byte aligned."""
    big = torch.full((rows + 2 * GUARD, C), float("nan"), device=G.dev(), dtype=dtype)
    out = big[GUARD:GUARD + rows]
    assert out.data_ptr() % 16 == 0 and out.is_contiguous()
    return big, out


def _guards_untouched(big, rows):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + rows:]).all())


def _layernorm_guarded(x, g, b, eps, prec, want32, want16, packed=False):
    code, dt = G.PRECS[prec]
    rows, C = x.shape
    b32, o32 = _guarded(rows, C, torch.float32) if want32 else (None, None)
    b16, o16 = _guarded(rows, C, dt) if want16 else (None, None)
    Nn.check(Nn.lib().wm_op_layernorm(Nn.ptr(x), Nn.ptr(g), Nn.ptr(b), eps, Nn.ptr(o32), Nn.ptr(o16), rows, C,
                                      code | (Nn.LAYOUT_PACKED if packed else 0), G.sp()))
    torch.cuda.synchronize()
    for big in (b32, b16):
        assert big is None or _guards_untouched(big, rows), f"a guard row was written (rows={rows} C={C} {prec} packed={packed})"
    return o32, o16


# ---------------------------------------------------------------------------
# the LayerNorm op: layernorm_kernel (fp32 and fp32 + 16-bit outputs), layernorm_tiled_kernel (16-bit only, row-major and packed)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("C", [256, 768, 1024, 1280])
def test_layernorm_op_rows(C, prec):
    """fp32 output: 4 x the fp32 emulation's worst error in the row's family, const and zero rows exactly beta.  16-bit outputs (the
    fp32 + 16-bit form of layernorm_kernel and the blocks' column-tiled kernel): 2 x the error of round16(float64 LayerNorm) on the
    row.  Tail rows: 1, 51, 153 and 1021 rows in family blocks of 3; the full table at 512 rows, where the packed output must be
    the row-major one permuted.  Every output lies between NaN guard rows."""
    eps = EPS_OF[C]
    g, b, _, _ = _weights(C, 16, prec)
    bad = {}
    for n_rows, block in ((1, 3), (51, 3), (153, 3), (1021, 3), (512, 16)):
        x, fam = _case(C, n_rows, block)
        tag = f"layernorm C={C} {prec} rows={n_rows}"
        ref, bar32 = LC.bar_out32(x, g, b, eps, fam)
        _, bar16 = LC.bar_out16(x, g, b, eps, prec, fam)
        o32, o16 = _layernorm_guarded(x, g, b, eps, prec, True, True)
        only32, _ = _layernorm_guarded(x, g, b, eps, prec, True, False)
        _, tiled = _layernorm_guarded(x, g, b, eps, prec, False, True)
        assert torch.equal(o32, only32), tag
        exact = ((fam == LC.FID["const"]) | (fam == LC.FID["zero"])).to(x.device)
        assert torch.equal(o32[exact], b.expand_as(o32)[exact]), f"{tag}: const / zero rows are not beta exactly"
        assert torch.isfinite(o32).all() and torch.isfinite(o16.float()).all() and torch.isfinite(tiled.float()).all(), tag
        for name, got, bar in (("fp32", o32, bar32), ("16 (with fp32)", o16, bar16), ("16 (tiled)", tiled, bar16)):
            pf = LC.per_family(LC.row_err(got, ref, fam), bar, fam)
            print(LC.line(f"{tag} {name}", pf))
            if LC.failures(pf):
                bad[f"rows={n_rows} {name}"] = LC.failures(pf)
        if n_rows % 16 == 0:
            _, packed = _layernorm_guarded(x, g, b, eps, prec, False, True, packed=True)
            assert torch.equal(G.unpack16_torch(packed), tiled) and torch.equal(packed, G.pack16(tiled.contiguous())), tag
    assert not bad, f"layernorm C={C} {prec}: over the bar {{case: {{family: (error, bar, row)}}}} {bad}"


# ---------------------------------------------------------------------------
# statistics and planes: ln_stats_x16_kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("C", [768, 1024, 1280])
def test_statistics_and_planes_rows(C, prec):
    """Per row and tile (mean, M2) against float64 (4 x the fp32 emulation's worst error in the row's family, floored at one ulp of
    the row's largest |x| / that squared times C); hi, lo and the rewritten rows bit-equal to their torch statement; x = hi + lo to
    2^-20 (fp16 hi) / 2^-18 (bf16 hi) relative plus 2^-24."""
    x, fam = _case(C, 512, 16)
    ref, bar = LC.bar_stats(x, fam)
    st0, x16 = G.ln_stats16(x, prec)
    stats, hi, lo, xr = G.ln_stats16_split(x, prec)
    assert torch.equal(stats, st0) and torch.equal(hi, x16)
    hi_rm, lo_rm = G.unpack16(hi), G.unpack16(lo)
    assert torch.equal(hi_rm, G.unpack16_torch(hi)) and torch.equal(hi_rm, x.to(G.PRECS[prec][1]))
    assert torch.equal(lo_rm, (x - hi_rm.float()).to(torch.float16))
    assert torch.equal(xr, hi_rm.float() + lo_rm.float())
    assert torch.equal(G.stream_merge(hi, lo, prec), xr)
    bound = x.abs() * (2.0 ** -18 if prec == "bf16" else 2.0 ** -20) + 2.0 ** -24
    over = (xr - x).abs() - bound
    r = int(over.amax(1).argmax())
    assert bool((over <= 0).all()), f"hi + lo misses x by {over.max().item():.2e} over the bound in family {LC.FAMILIES[fam[r]]}, row {r}"
    LC.check(f"ln_stats16 C={C} {prec} (mean, M2)", (stats.double() - ref).abs(), bar, fam)


# ---------------------------------------------------------------------------
# the folded consumer (FOLDC epilogue) and the classic route on the same rows
# ---------------------------------------------------------------------------
FOLDED_SHAPES = [(2816, 3840, 1280), (2816, 3072, 1024), (3840, 2304, 768)]      # the fewest 256-row tiles the 256-row kernel takes


@functools.lru_cache(maxsize=None)
def _folded_run(M, N, K, prec, act):
    """Per-family verdicts of G.gemm16_folded and of G.layernorm -> G.gemm16 on the family rows: computed once per case."""
    assert EC.takes_v5(M, N, K)
    x, fam = _case(K, M, 16)
    g, b, w16, bias = _weights(K, N, prec)
    eps = 1e-6
    ref, bar_f, emu, noise = LC.bar_folded(x, g, b, eps, w16, bias, act, prec, fam)
    _, bar_c = LC.bar_classic(x, g, b, eps, w16, bias, act, prec, fam)
    stats, x16 = G.ln_stats16(x, prec)
    wf, c1, c2 = G.fold_weight16(w16, g, b, bias, prec)
    got, var = _variants_run(lambda: G.gemm16_folded(x16, wf, c1, c2, stats, eps, act, prec))
    got_p = G.gemm16_folded(x16, wf, c1, c2, stats, eps, act, prec, out_packed=True)
    _, xn16 = G.layernorm(x, g, b, eps, prec, want32=False, want16=True)
    _, cl = G.gemm16(xn16, w16, bias, None, 0, act, prec, want32=False, want16=True)
    tag = f"M={M} N={N} K={K} {prec} act={act}"
    out = {
        "variant": var, "packed_equal": torch.equal(G.unpack16_torch(got_p), got),
        "finite": bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(cl.float()).all()),
        "folded": LC.per_family(LC.row_err(got, ref, fam), bar_f, fam),
        "classic": LC.per_family(LC.row_err(cl, ref, fam), bar_c, fam),
        "emulation": LC.per_family(emu, bar_f, fam), "noise": LC.per_family(noise, bar_f, fam),
    }
    print(LC.line(f"folded GEMM {tag} kernel", out["folded"]))
    print(LC.line(f"folded GEMM {tag} emulation", out["emulation"]))
    print(LC.line(f"folded GEMM {tag} fp32-noise term", out["noise"]))
    print(LC.line(f"classic route {tag} kernel", out["classic"]))
    return out


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", FOLDED_SHAPES)
def test_folded_consumer_rows(M, N, K, act, prec):
    """G.gemm16_folded per row under 2 x err(folded emulation) + the fp32 accumulation noise times rstd, the classic route on the
    same rows under 2 x err(classic emulation); out_packed bit-equal to the plain output; all outputs finite."""
    r = _folded_run(M, N, K, prec, act)
    assert r["variant"] == {("v5_320" if N % 320 == 0 else "v5_256"): 1}, r["variant"]
    assert r["packed_equal"] and r["finite"]
    bad = {k: LC.failures(r[k]) for k in ("folded", "classic") if LC.failures(r[k])}
    assert not bad, f"M={M} N={N} K={K} {prec} act={act}: over the bar {{route: {{family: (error, bar, row)}}}} {bad}"


# ---------------------------------------------------------------------------
# the producers (FOLDP, SPLIT epilogues) with the family rows as the residual
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("scale", [1e-3, 1.0])
@pytest.mark.parametrize("M,N", [(8448, 1280), (8448, 1024), (11008, 768)])
def test_producers_rows(M, N, scale, prec):
    """gemm16_stats / gemm16_split with K = 64 and a w^T of size `scale`: bit identity with the standalone kernel on the rows they
    wrote, and those statistics against float64 under the statistics bar."""
    K = 64
    dev = G.dev()
    assert EC.takes_v5(M, N, K)
    r, fam = _case(N, M, 16)
    gen = torch.Generator(device=dev).manual_seed(M + N)
    a = G.to16(torch.randn(M, K, device=dev, generator=gen) * scale, prec)
    w = G.to16(torch.randn(N, K, device=dev, generator=gen) / math.sqrt(K), prec)
    bias = torch.randn(N, device=dev, generator=gen) * scale
    base32, _ = G.gemm16(a, w, bias, r, 0, 0, prec, want32=True, want16=False)
    (out32, x16, stats), var = _variants_run(lambda: G.gemm16_stats(a, w, bias, r, prec))
    assert var == {("v5_320_foldp" if N % 320 == 0 else "v5_256_foldp"): 1}, var
    assert torch.equal(out32, base32)
    st2, x2 = G.ln_stats16(out32, prec)
    assert torch.equal(stats, st2) and torch.equal(x16, x2)
    ref, bar = LC.bar_stats(out32, fam)
    LC.check(f"gemm16_stats M={M} N={N} scale={scale} {prec} (mean, M2)", (stats.double() - ref).abs(), bar, fam)
    # the split stream: planes in, planes out
    _, hi, lo, xr = G.ln_stats16_split(r, prec)
    v32, _ = G.gemm16(a, w, bias, xr, 0, 0, prec, want32=True, want16=False)
    st_ref, hi_ref, lo_ref, _ = G.ln_stats16_split(v32, prec)
    (hi2, lo2, st3), var = _variants_run(lambda: G.gemm16_split(a, w, bias, hi, lo, prec))
    assert var == {("v5_320_split" if N % 320 == 0 else "v5_256_split"): 1}, var
    assert torch.equal(st3, st_ref) and torch.equal(hi2, hi_ref) and torch.equal(lo2, lo_ref)


# ---------------------------------------------------------------------------
# e4m3 LayerNorm: on the hi plane (layernorm_plane_fp8_kernel) and on fp32 rows (layernorm_tiled_kernel's e4m3 form)
# ---------------------------------------------------------------------------
def _e4m3_index(code):
    """Signed position of an e4m3 byte on the number line (+-0 -> 0): adjacent values differ by 1."""
    mag = (code & 0x7f).long()
    return torch.where(code >= 0x80, -mag, mag)


def _fp8_verdict(tag, got, ref64, emu32, fam):
    """got: e4m3 bytes; ref64: the float64 LayerNorm; emu32: the fp32 emulation.  No element more than one e4m3 step from e4m3(ref);
    per family the share of elements that differ at all <= max(2 x the emulation's share, 2e-3)."""
    want, emu = G.to_fp8(ref64.float()), G.to_fp8(emu32)
    step = (_e4m3_index(got) - _e4m3_index(want)).abs()
    fam_d = fam.to(got.device)
    bad, parts = {}, []
    for f in torch.unique(fam).tolist():
        m = fam_d == f
        share, emu_share = (got[m] != want[m]).float().mean().item(), (emu[m] != want[m]).float().mean().item()
        far = int(step[m].max())
        bar = max(2 * emu_share, 2e-3)
        parts.append(f"{LC.FAMILIES[f]} {share:.1e}({bar:.1e})")
        if far > 1 or not share <= bar:
            rows_at = torch.nonzero(m).flatten()
            bad[LC.FAMILIES[f]] = (share, bar, far, int(rows_at[int(step[m].amax(1).argmax())]))
    print(f"{tag} share of differing e4m3 elements: " + "  ".join(parts))
    return bad


@pytest.mark.parametrize("C", [768, 1024, 1280])
def test_layernorm_fp8_rows(C):
    """Against e4m3 of the float64 LayerNorm of float(hi), per family, for both hi-plane types; and the fp32-rows e4m3 form of the
    blocks' LayerNorm against e4m3 of the float64 LayerNorm of the rows."""
    x, fam = _case(C, 512, 16)
    g, b, _, _ = _weights(C, 16, "fp16")
    pos = G.plane_pos(C, x.device)
    bad = {}
    for prec in ("bf16", "fp16"):
        hi, _ = G.stream_rows_split(x, prec)
        xh = hi[:, pos].float().contiguous()
        got = G.layernorm_fp8_plane(hi, g, b, 1e-6, prec)[:, pos].contiguous()
        v = _fp8_verdict(f"layernorm_fp8_plane C={C} hi={prec}", got, LC.ln64(xh, g, b, 1e-6), LC.ln32(xh, g, b, 1e-6), fam)
        if v:
            bad[f"plane {prec}"] = v
    v = _fp8_verdict(f"layernorm e4m3 of fp32 rows C={C}", G.layernorm_fp8(x, g, b, 1e-6), LC.ln64(x, g, b, 1e-6), LC.ln32(x, g, b, 1e-6), fam)
    if v:
        bad["rows"] = v
    assert not bad, f"C={C}: {{form: {{family: (share, bar, steps, row)}}}} {bad}"


# ---------------------------------------------------------------------------
# the model's own rows lie inside what was tested
# ---------------------------------------------------------------------------
def _row_figures(t, eps=1e-6):
    """(|mean| / std, std) per row of a [.., D] tensor, float64."""
    v = t.reshape(-1, t.shape[-1]).double()
    mean = v.mean(-1)
    std = ((v - mean[:, None]) ** 2).mean(-1).sqrt()
    return mean.abs() / std, std


def _tap_figures(m, x, taps):
    hub = m._hub
    n = x.shape[0]
    hub.handle(x.device, n)
    hfc = m.fft(x)
    ratio, std = [], []
    for which in taps:
        hub.set_tap(which)
        with torch.no_grad():
            m.image_encoder(x, hfc)
        r, s = _row_figures(hub.read_tap(n))
        ratio.append(r)
        std.append(s)
    hub.set_tap(-2)
    return torch.cat(ratio), torch.cat(std)


def _envelope(K, prec="fp16"):
    """(largest |mean| / std, smallest and largest std) among the families on which the folded consumer met its bar at this K."""
    M, N, _ = next(s for s in FOLDED_SHAPES if s[2] == K)
    ok = set(LC.FAMILIES)
    for act in (0, 1):
        ok -= set(LC.failures(_folded_run(M, N, K, prec, act)["folded"]))
    x, fam = _case(K, M, 16)
    ratio, std = _row_figures(x)
    rmax, smin, smax = 0.0, float("inf"), 0.0
    for f in ok - {"const", "zero"}:
        m = (fam == LC.FID[f]).to(x.device)
        rmax, smin, smax = max(rmax, ratio[m].median().item()), min(smin, std[m].median().item()), max(smax, std[m].median().item())
    return sorted(ok), rmax, smin, smax


def _inside(name, ratio, std, K):
    ok, rmax, smin, smax = _envelope(K)
    q = torch.tensor([0.5, 0.999], dtype=torch.float64, device=ratio.device)
    rq, sq = torch.quantile(ratio, q).tolist(), torch.quantile(std, 1 - q).tolist()
    print(f"{name}: {ratio.numel()} rows  |mean|/std max {ratio.max().item():.3g} p99.9 {rq[1]:.3g} median {rq[0]:.3g}   "
          f"std min {std.min().item():.3g} p0.1 {sq[1]:.3g} median {sq[0]:.3g} max {std.max().item():.3g}   "
          f"std/sqrt(eps) min {std.min().item() / 1e-3:.3g}   "
          f"tested: |mean|/std <= {rmax:.3g}, {smin:.3g} <= std <= {smax:.3g} ({len(ok)} of {len(LC.FAMILIES)} families met the folded bar)")
    assert ratio.max().item() <= rmax and smin <= std.min().item() and std.max().item() <= smax, \
        f"{name}: the stream leaves the tested families: extend layernorm_cases.FAMILIES"


def test_vit_b_stream_rows_lie_inside_the_tested_families():
    """ViT-B fp16 on the three tiles of encoder_cases.TILES: taps -1 and every block."""
    m, _ = G._model("vit_b", "fp16")
    ratio, std = [], []
    for kind in EC.TILES:
        r, s = _tap_figures(m, EC.tile(kind).to(G.dev()), [-1] + list(range(12)))
        ratio.append(r)
        std.append(s)
    _inside("vit_b fp16 stream, 3 tiles x 13 taps", torch.cat(ratio), torch.cat(std), 768)


def test_vit_h_outlier_profile_stream_rows_lie_inside_the_tested_families():
    """One tile of the ViT-H outlier weight profile (the encoder of test_gpu_e2e.py's outlier test): taps -1, 0, 7, 15, 23, 31."""
    from wildlifemapper_amd.segment_anything import sam_model_registry
    from wildlifemapper_amd.segment_anything.network import MedSAM
    sam, _, _ = sam_model_registry["vit_h"](None, None)
    m = MedSAM(sam.image_encoder, sam.mask_decoder, sam.prompt_encoder).eval()
    sd = synth.make_state_dict("vit_h", 0, only_prefix="image_encoder.", profile="outlier")      # the decoder is not run
    missing = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if k.startswith("image_encoder.")]
    m._hub.set_precision("fp16")
    try:
        x = torch.from_numpy(synth.make_batch(0, 1)).to(G.dev())
        ratio, std = _tap_figures(m, x, [-1, 0, 7, 15, 23, 31])
    finally:
        m._hub.close()
    _inside("vit_h fp16 outlier profile stream, 1 tile x 6 taps", ratio, std, 1280)
