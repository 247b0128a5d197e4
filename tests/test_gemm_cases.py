"""The GEMM element cases on the reference alone (-m "not gpu"): the conditions every case of tests/gemm_cases.py relies on, the
emulation passing every case, and the mutant study -- for each mutant of the emulation the first case that sees it, and whether the
old criterion (one relative L2 on Gaussian operands at test_gpu_ops.py's tolerances) does.  Run with -s for the study;
profiles/gemm_elements/mutants.txt is that output."""
import math

import pytest
import torch

import gemm_cases as C

# (instance, row tile, column tile): the tiles the probes are built on (host_gemm.h)
TILES = {"v1_128": (128, 128), "v2_128": (256, 128), "v2_160": (256, 160), "v5_320": (256, 320), "v5_256": (256, 256), "gemm32": (64, 64), "fp8_256": (256, 256)}
OPMAX = {"bf16": 255, "fp16": 2047, "fp8": 8}


def _representable(t, prec):
    if prec == "fp32":
        return True
    dt = torch.float8_e4m3fn if prec == "fp8" else C.DT[prec]
    return bool((t.to(dt).float() == t).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# probe
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst,M,N,K,prec", [("v1_128", 384, 256, 64, "bf16"), ("v1_128", 384, 256, 320, "fp16"), ("v2_128", 768, 512, 192, "bf16"),
                                             ("v2_160", 256, 640, 64, "fp16"), ("v5_320", 1024, 640, 160, "bf16"), ("v5_256", 512, 512, 5120, "fp16"),
                                             ("gemm32", 153, 14, 96, "fp32"), ("fp8_256", 512, 256, 256, "fp8")])
def test_probe_covers_every_k_in_every_tile_and_codes_are_exact(inst, M, N, K, prec):
    tile = TILES[inst]
    for side, rows, t in (("w", M, tile[0]), ("a", N, tile[1])):
        J = C.probe_launches(K, t)
        pis = torch.stack([C.probe_pi(rows, K, t, j) for j in range(J)])               # [J, rows]
        for r0 in range(0, rows - t + 1, t):                                            # every whole tile
            assert len(torch.unique(pis[:, r0:r0 + t])) == K, (side, r0)
        if rows >= 2 * t:
            assert not torch.equal(pis[0, :t], pis[0, t:2 * t])                         # neighbouring tiles: another map
        c = C.make_probe(M, N, K, prec, tile, side=side, j=J - 1, bias=True, res_rows=min(M, 256))
        assert c.a.abs().max() <= OPMAX.get(prec, 2047) and c.w.abs().max() <= OPMAX.get(prec, 2047)
        assert _representable(c.a, prec) and _representable(c.w, prec)
        y = C.ref64(c)
        plain = y - c.bias.double() - C.res_rows_of(c)
        assert torch.equal(plain, C.probe_answer(c))                                    # the float64 product IS the gather
        assert C.is_exact32(y) and C.is_exact32(plain + c.bias.double())                # (acc + bias) + res: exact at every step
        assert len(torch.unique(c.bias)) == N and len(torch.unique(c.res[:, 0])) == c.res.shape[0]


@pytest.mark.parametrize("fp8", [False, True])
def test_code_is_injective_under_structure_shifts(fp8):
    """Two positions carry the same code only if their rows differ by a multiple of MOD_R and their k by a multiple of MOD_K (fp8: 3
    and 5); no structure shift is such a multiple, so no shift in n, in k or in both maps a position onto an equal code."""
    mr, mk = (3, 5) if fp8 else (C.MOD_R, C.MOD_K)
    r, k = torch.arange(mr)[:, None], torch.arange(mk)[None, :]
    window = C.code(r, k, fp8)
    assert len(torch.unique(window)) == mr * mk                                          # injective on a MOD_R x MOD_K window
    assert window.abs().max() <= (7 if fp8 else 218)
    big = C.code(torch.arange(700)[:, None], torch.arange(700)[None, :], fp8)
    assert torch.equal(big, window[torch.arange(700) % mr][:, torch.arange(700) % mk])   # and periodic with exactly those periods
    shifts = C.structure_shifts(1 << 16, fp8)
    assert {16, 32, 64, 128, 256, 4096} <= set(shifts) and (fp8 or {160, 320, 96, 192, 1280, 5120} <= set(shifts))
    assert all(s % mr and s % mk for s in shifts)
    # spelled out on a tile: shifting n, k or both by any structure shift changes the code everywhere
    for dn in [0] + [s for s in shifts if s <= 320]:
        for dk in [0] + [s for s in shifts if s <= 128]:
            if dn or dk:
                assert bool((big[:320, :128] != big[dn:320 + dn, dk:128 + dk]).all()), (dn, dk)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("K,res_rows,act", [(64, 0, 0), (320, 256, 0), (320, 0, 2), (5120, 128, 0)])
def test_exact_case_is_exact_and_full_of_ties(prec, K, res_rows, act):
    c = C.make_exact(256, 256, K, prec, (128, 128), seed=K, res_rows=res_rows, act=act)
    assert C.exact_bound(c) < 65504 < 2 ** 24                        # no fp16 clamp; every partial sum an integer below 2^24
    assert _representable(c.a, prec) and _representable(c.w, prec) and c.a.abs().max() == 3
    y = C.ref64(c)
    assert C.is_exact32(y) and y.abs().max() <= C.exact_bound(c) and bool((y == y.round()).all())
    census = C.tie_census(y, prec)
    binades = len(torch.unique(torch.floor(torch.log2(y.abs().clamp_min(1)))))
    print(f"exact {prec} K={K} res_rows={res_rows} act={act}: |y| <= {y.abs().max().item():.0f} over {binades} binades, {census}")
    assert census["ties_up"] >= 20 and census["ties_down"] >= 20 and census["near"] >= 20 and binades >= 8
    # the three wrong roundings differ from round-to-nearest-even on this very tensor
    rne = C.round16(y, prec)
    for mode in ("trunc", "away") + (("via_fp16",) if prec == "bf16" else ()):
        assert int((C.round16(y, prec, mode).float() != rne.float()).sum()) > 0, mode
    hi, lo = C.planes(y.float(), prec)
    assert torch.equal(hi.double() + lo.double(), y)                 # hi + lo holds these integers exactly


def test_exact_saturating_variant_saturates_the_designed_set_only():
    c = C.make_exact(256, 512, 320, "fp16", (128, 128), seed=3, saturate=True)
    y = C.ref64(c)
    over = y.abs() > 65504
    assert torch.equal(over, c.sat_cols[None, :].expand_as(over)) and int(c.sat_cols.sum()) >= 10
    assert y[:, c.sat_cols].abs().min() > 65520 and C.is_exact32(y)
    want = C.round16(y, "fp16")
    assert bool((want[:, c.sat_cols].float().abs() == 65504).all()) and bool(torch.isfinite(want.float()).all())
    assert (want[:, c.sat_cols].float() > 0).any() and (want[:, c.sat_cols].float() < 0).any()


def test_exact_fp8_case_has_ties_and_saturation_of_e4m3():
    c = C.make_exact(256, 256, 256, "fp8", (256, 256), seed=5, amp=100)
    assert _representable(c.a, "fp8") and _representable(c.w, "fp8") and set(c.wscale.tolist()) == {0.5, 1.0, 2.0}
    y = C.ref64(c)
    assert C.is_exact32(y)
    census = C.tie_census(y, "fp8")
    print(f"exact fp8: |y| <= {y.abs().max().item():.1f}, {census}, {int((y.abs() > 448).sum())} beyond 448")
    assert census["ties_up"] >= 20 and census["ties_down"] >= 20 and int((y.abs() > 448).sum()) >= 20
    assert bool((C.round8(y).float().abs() <= 448).all())


def test_small_integers_split_exactly_into_fp16_hi_and_lo():
    """The split fp32 form carries x as hi + 2^-11 lo (fp16 each): the probe's codes and the exact case's integers have lo = 0."""
    for t in (C.make_probe(153, 14, 96, "fp32", (64, 64)).w, C.make_exact(70, 14, 96, "fp32", (64, 64)).a):
        hi = t.to(torch.float16)
        assert torch.equal(hi.float(), t) and t.abs().max() <= 2048


# ---------------------------------------------------------------------------------------------------------------------------------
# gelu, sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", C.GELU_SHAPES, ids=lambda v: str(v))
def test_gelu_case_sweeps_exact_pre_activations(M, N, K, prec):
    """At every (M, N, K) a gelu case is launched with (the GPU module takes its shapes from C.GELU_SHAPES and asserts the same per
    launch): [-9, 9] end to end with no gap above 1 / 16, 0 and its neighbourhood, both sides of both clamp points, the underflowing
    tail, one non-zero k per row, everything exact."""
    c = C.make_gelu(M, N, K, prec, (64, 64))
    assert _representable(c.a, prec) and _representable(c.w, prec)
    x = c.a.double() @ c.w.double().t()
    assert torch.equal((c.a @ c.w.t()).double(), x)                                      # exact in fp32
    s = C.gelu_sweep(c)
    print(f"gelu sweep {M}x{N}x{K} {prec}: {vars(s)}")
    assert C.gelu_sweep_ok(s), vars(s)
    assert s.lo == -9 and s.hi == 9 and s.gap <= 1 / 16 and s.near0 >= 4 and s.clamp < 0.02 and s.tail >= 100       # (spelled out once more)
    y = C.gelu64(x)
    assert bool((y[x < 0] <= 0).all()) and bool((y[x < -8.9] < 0).all())                 # the oracle keeps the sign of the tail
    # the fast form restated passes its own stated accuracy on this sweep; the two GELU mutants do not
    assert (C.gelu_fast32(x.float()).double() - y).abs().max() < C.GELU_BAR
    assert (C.gelu_fast32(x.float(), 3.2).double() - y).abs().max() > C.GELU_BAR


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_sums_case_has_the_rows_and_columns_it_claims(prec):
    c = C.make_sums(256, 256, 320, prec, (128, 128), seed=1, bias=True, res_rows=128)
    assert _representable(c.a, prec) and _representable(c.w, prec)
    plain = C.make_sums(256, 256, 320, prec, (128, 128), seed=1)
    y, s = C.ref64(plain, want_s=True)
    cancel = (y.abs() / s)[3::8, 5::8]
    rowsize = plain.a.norm(dim=1)
    print(f"sums {prec}: cancellation block |sum| / sum|.| <= {cancel.max().item():.2e}, elsewhere median {(y.abs() / s).median().item():.2e}; "
          f"row norms {rowsize.min().item():.2f} .. {rowsize.max().item():.1f}")
    assert cancel.max() < 2e-2 and (y.abs() / s).median() > 0.03
    assert s[3::8, 5::8].median() > 1
    assert rowsize.max() / rowsize.min() > 30
    # the float32 CPU product sits inside the hard bound
    rho = ((plain.a @ plain.w.t()).double() - y).abs() / (C.U32 * s)
    assert rho.max() <= C.hard_bound(plain, "mfma32" if prec == "fp32" else "mfma16")


# ---------------------------------------------------------------------------------------------------------------------------------
# the implicit forms' gathers and the packed order
# ---------------------------------------------------------------------------------------------------------------------------------
def test_conv_and_patch_gathers_equal_torch_convolutions():
    c = C.make_conv("exact", 2, 32, 256, "fp16", seed=2)
    ref = torch.nn.functional.conv2d(c.x.permute(0, 3, 1, 2).double(), c.w.view(256, 3, 3, 32).permute(0, 3, 1, 2).double(), padding=1)
    assert torch.equal(C.ref64(c), ref.permute(0, 2, 3, 1).reshape(2 * 4096, 256))
    p = C.make_patch("exact", 1, 3, 256, "bf16", seed=4)
    ref = torch.nn.functional.conv2d(p.x.double(), p.w.view(256, 3, 16, 16).double(), p.bias.double(), stride=16)
    assert torch.equal(C.ref64(p), ref.permute(0, 2, 3, 1).reshape(4096, 256))


def test_conv_probe_reaches_every_tap_at_every_border_class():
    """W one-hot on (tap, ci): over the launches every k = (tap, ci) is some output channel's choice, and the answer of a border pixel is
    an exact zero for the taps outside the grid and the neighbour's code inside."""
    Cin, N = 32, 256
    J = C.probe_launches(9 * Cin, 256)
    seen = set()
    for j in range(J):
        c = C.make_conv("probe", 1, Cin, N, "bf16", j=j)
        seen |= set(c.pi.tolist())
        y = C.ref64(c)
        assert torch.equal(y, C.probe_answer(c)) and C.is_exact32(y)
        tap = c.pi // Cin
        dy, dx = tap // 3 - 1, tap % 3 - 1
        for (py, px) in ((0, 0), (0, 63), (63, 0), (63, 63), (0, 17), (40, 0), (63, 5), (22, 63), (31, 31)):      # corners, edges, interior
            outside = (py + dy < 0) | (py + dy > 63) | (px + dx < 0) | (px + dx > 63)
            row = y[py * 64 + px]
            assert bool((row[outside] == 0).all())
            inside_want = C.code((py + dy) * 64 + (px + dx), c.pi % Cin, nonzero=True).double()
            assert torch.equal(row[~outside], inside_want[~outside])
        assert bool((c.x != 0).all())                   # no code is the zero page's value
    assert seen == set(range(9 * Cin))


def test_image_order_is_the_documented_permutation():
    t = torch.arange(48 * 96, dtype=torch.int32).view(48, 96)
    p = C.pack16_image(t)
    assert torch.equal(C.unpack16_image(p), t) and not torch.equal(p, t)
    l = 37                                          # position l of block (1, 2): row l >> 2, chunk (l & 3) ^ ((-(l >> 4)) & 3)
    row, ch = l >> 2, (l & 3) ^ ((-(l >> 4)) & 3)
    blk = p.view(3, 3, 64, 8)[1, 2, l]
    assert torch.equal(blk, t[16 + row, 64 + ch * 8:64 + ch * 8 + 8])


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation passes every case; every mutant is seen by one
# ---------------------------------------------------------------------------------------------------------------------------------
TILE, M0, N0, K0 = (128, 128), 512, 256, 128            # 4 x 2 tiles in rounds of 4: the second round is tiles (2, 0) .. (3, 1)


def _study_cases(prec):
    """(name, case, outputs) in the order the study tries them."""
    yield "probe W coded", C.make_probe(M0, N0, K0, prec, TILE, "w", bias=True, res_rows=256), ("f32", "o16")
    yield "probe A coded", C.make_probe(M0, N0, K0, prec, TILE, "a", bias=True, res_rows=256), ("f32", "o16")
    yield "exact", C.make_exact(M0, N0, K0, prec, TILE, seed=1, res_rows=256), ("f32", "o16")
    yield "exact planes", C.make_exact(M0, N0, K0, prec, TILE, seed=2, res_rows=M0), ("hi", "lo")
    yield "conv probe", C.make_conv("probe", 1, 32, 256, prec), ("f32",)
    yield "gelu", C.make_gelu(M0, N0, K0, prec, TILE), ("f32", "o16")
    yield "sums", C.make_sums(M0, N0, K0, prec, TILE, seed=3, bias=True, res_rows=256), ("f32", "o16")


def _judge(c, got, outs):
    """(seen, text) of one case on the outputs `got`."""
    if c.kind == "sums":                                # the hard bound and the measured bar, per element, as the GPU run asserts them
        y, s = C.ref64(c, want_s=True)
        cpu32 = C.cpu_product32(c, C.CHAIN["mfma16"])
        figs = {o: C.sums_figures(c, got[o], y, s, cpu32, None if o == "f32" else C.out_prec(c)) for o in outs}
        o, f = max(figs.items(), key=lambda kv: kv[1].worst)
        return any(f_.over for f_ in figs.values()), (f"{o} rho {f.worst:.3g} against hard bound {f.hard} and bar {C.BAR_FACTOR * f.worst_cpu:.3g}, "
                                                      f"{f.n_over} elements over")
    y = C.ref64(c)
    if c.kind in ("probe", "exact"):
        want = C.expected(c, y, outs)
        bad = {o: C.mismatches(got[o], want[o])[0] for o in outs}
        return any(bad.values()), "exact mismatch, " + " / ".join(f"{n} elements of {o}" for o, n in bad.items() if n)
    f32, f16 = C.gelu_figures(c, got["f32"], y), C.gelu_figures(c, got["o16"], y, C.out_prec(c))
    worst = max((f32, f16), key=lambda f: f.ratio)
    return worst.ratio > 1 or worst.pos_over > 0 or worst.nans > 0, f"|err| {worst.err:.2e} at x = {worst.x:.4f}, x{worst.ratio:.2f} of its bar {worst.bar:.2e}"


def _old_criterion_sees(prec, mutant):
    """Relative L2 on Gaussian operands against the product, at test_gpu_ops.py's tolerances (fp32 2e-5, fp16 7e-4, bf16 5e-3)."""
    if mutant == "conv_tap":
        c = C.make_conv("exact", 1, 32, 256, prec)
        g = torch.Generator().manual_seed(9)
        c.x, c.w = torch.randn(c.x.shape, generator=g).to(C.DT[prec]).float(), (torch.randn(c.w.shape, generator=g) / 17).to(C.DT[prec]).float()
        outs = ("f32",)
    else:                                           # 4096 x 1280: a quarter of the smallest output the old tests give the wide kernels
        M, N = 4096, 1280
        c = C.make_sums(M, N, K0, prec, TILE, seed=9, bias=True, res_rows=M if mutant == "lo_unrounded" else 256)
        c.act = 1 if mutant.startswith("gelu") else 0
        outs = ("hi", "lo") if mutant == "lo_unrounded" else ("f32", "o16")
    y = C.ref64(c)
    got = C.emulate(c, outs, mutant)
    rel = lambda t: ((t.double() - y).norm() / y.norm()).item()
    if outs == ("hi", "lo"):
        return {"hi + lo": rel(got["hi"].double() + got["lo"].double()) >= 1e-5}
    base = C.emulate(c, outs)                          # an output the mutant leaves as it is has nothing to see
    tol32 = C.OLD_TOL["fp32_act" if c.act else "fp32"]
    return {o: rel(got[o]) >= (tol32 if o == "f32" else C.OLD_TOL[prec]) for o in outs if not torch.equal(got[o], base[o])}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_emulation_passes_and_every_mutant_is_seen(prec):
    cases = list(_study_cases(prec))
    print(f"\n{prec}: the emulation, {M0} x {N0} x {K0} in {TILE[0]} x {TILE[1]} tiles, K-steps of 32, rounds of 4 tiles")
    for name, c, outs in cases:
        seen, text = _judge(c, C.emulate(c, outs), outs)
        print(f"  baseline      {name:14s} {'FAILS: ' + text if seen else 'passes'}")
        assert not seen, (name, text)
    blind = []
    for mutant, what in C.MUTANTS.items():
        if mutant == "double_round" and prec != "bf16":
            continue
        first = None
        for name, c, outs in cases:
            seen, text = _judge(c, C.emulate(c, outs, mutant), outs)
            if seen:
                first = (name, text)
                break
        old = _old_criterion_sees(prec, mutant)
        blind += [mutant] if not all(old.values()) else []
        verdict = ", ".join(f"{o} {'sees it' if s else 'BLIND'}" for o, s in old.items())
        print(f"  {mutant:13s} {what:98s} {'NOT SEEN' if first is None else first[0] + ': ' + first[1]:82s} old criterion: {verdict}")
        name, c, outs = cases[-1]                       # and what the sums metrics alone make of it
        seen, text = _judge(c, C.emulate(c, outs, mutant), outs)
        print(f"  {'':13s} by the sums case alone: {'seen' if seen else 'not seen'} ({text})")
        assert first is not None, mutant
    print(f"  the old criterion is blind, on some output, to: {', '.join(blind)}")
    # the rounding mutants on either type; the few-element one where the tolerance is bf16's (an fp32 output at 2e-5 does see 16 elements)
    assert {"trunc16", "half_away"} | ({"double_round", "store_shift"} if prec == "bf16" else set()) <= set(blind)
