"""What the LayerNorm row cases are and what their bars can see (CPU only).

tests/test_gpu_layernorm_rows.py holds every kernel of the LayerNorm family to per-row bars computed from the float64 oracle and the
emulations of tests/layernorm_cases.py.  Here: the case builder is deterministic and every 256-row tile holds every family; the
folded emulation reproduces the error growth with |mean| / std that motivated the families (float64 emulation, K = 1280, N = 320,
32 rows per family, no output rounding: x and gamma (.) W each rounded once); and each structural mistake of MUTANTS -- a wrong
variant of the folded emulation, and of the LayerNorm itself for the fp32-output kernel -- exceeds its bar on the family named in
CAUGHT_BY, in fp16 and in bf16, while the unmutated emulation passes every family.
"""
import pytest
import torch

import layernorm_cases as LC

EPS = 1e-6
N_OUT = 320
ROWS = 512                      # 32 rows per family slot

# the emulated worst-row errors the families were chosen on (rows: family, fp16 classic, fp16 folded, bf16 classic, bf16 folded)
CURVE = {
    "base": (1.6e-4, 2.3e-4, 1.4e-3, 1.8e-3),
    "offset10": (1.6e-4, 1.7e-3, 1.4e-3, 1.4e-2),
    "offset100": (1.6e-4, 1.4e-2, 1.4e-3, 1.1e-1),
    "offset1000": (1.6e-4, 1.1e-1, 1.3e-3, 7.3e-1),
    "flat1e-1": (1.6e-4, 4.4e-3, 1.3e-3, 3.5e-2),
    "flat1e-3": (1.3e-4, 3.4e-1, 1.1e-3, 6.1e-1),
    "spike": (3.1e-4, 1.7e-4, 2.5e-3, 2.0e-3),           # one channel at 1e3 or 3e4: the worse of the two families
}
CURVE_FACTOR = 1.5

# mutant -> (the family that catches it in the folded GEMM, the family that catches it in the fp32 LayerNorm or None, C)
CAUGHT_BY = {
    "next_row": ("offset1000", "offset1000", 1280),
    "no_between": ("tilestep", "tilestep", 1280),
    "onepass32": ("flat1e-5", "offset1000", 1280),
    "eps_dropped": ("const", "const", 1280),
    "eps_after_sqrt": ("tiny1e-4", "tiny1e-4", 1280),
    "mean_div4": ("offset10", "offset10", 768),
    "c_shift": ("zero", None, 1280),                      # c1 / c2 exist in the folded GEMM only
}


@pytest.fixture(scope="module")
def study():
    """{(C, prec): everything the tests below read}, computed once."""
    out = {}
    for C in (1280, 768):
        x, fam = LC.rows(C, ROWS, 0)
        for prec in ("fp16", "bf16"):
            g, b, w16, bias = LC.params(C, N_OUT, prec)
            ref, bar, emu, noise = LC.bar_folded(x, g, b, EPS, w16, bias, 0, prec, fam)
            ref32, bar32 = LC.bar_out32(x, g, b, EPS, fam)
            out[C, prec] = dict(x=x, fam=fam, w=(g, b, w16, bias), ref=ref, bar=bar, emu=emu, ref32=ref32, bar32=bar32)
    return out


def test_rows_are_deterministic_and_every_tile_holds_every_family():
    for C in (256, 768, 1024, 1280):
        x, fam = LC.rows(C, 1024, 3)
        x2, fam2 = LC.rows(C, 1024, 3)
        assert torch.equal(x, x2) and torch.equal(fam, fam2)
        assert not torch.equal(x, LC.rows(C, 1024, 4)[0])
        assert x.dtype == torch.float32 and x.abs().max().item() < 65504
        for t in range(4):
            assert set(fam[256 * t:256 * t + 256].tolist()) == set(range(len(LC.FAMILIES))), (C, t)
        assert (x[fam == LC.FID["const"]] == 3.0).all() and (x[fam == LC.FID["zero"]] == 0.0).all()
        # the spikes stand at the first and at the last column of every statistics tile
        bn = LC.fold_bn(C)
        cols = set((x[fam == LC.FID["spike3e4"]] == 3e4).nonzero()[:, 1].tolist())
        assert cols == {t * bn for t in range(C // bn)} | {t * bn + bn - 1 for t in range(C // bn)}, (C, cols)
    # blocks of 3 rows: 51 rows already hold every family, and a four-row workgroup always mixes two
    _, fam = LC.rows(768, 51, 0, block=3)
    assert set(fam.tolist()) == set(range(len(LC.FAMILIES)))
    assert all(len(set(fam[r:r + 4].tolist())) >= 2 for r in range(0, 48, 4))
    # a prefix of a longer case is the same family layout
    assert torch.equal(LC.family_ids(1021, 3)[:153], LC.family_ids(153, 3))


def test_outlier_rows_are_the_rows_test_gpu_ops_used():
    """outlier_rows() moved here from test_gpu_ops.py: the same draws from the global generator, the same two massive channels."""
    torch.manual_seed(0)
    a = LC.outlier_rows(64, 768, "cpu")
    torch.manual_seed(0)
    b = torch.randn(64, 768) * (0.7 + torch.rand(64, 1)) + 0.2 * torch.randn(64, 1)
    b[:, 101] += 190.0
    b[:, 678 % 768] -= 240.0
    assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_folded_emulation_reproduces_the_growth_with_mean_over_std(study, prec):
    s = study[1280, prec]
    g, b, w16, bias = s["w"]
    col = 0 if prec == "fp16" else 2
    ef = LC.row_err(LC.folded(s["x"], g, b, EPS, w16, bias, 0, prec, round_out=False), s["ref"], s["fam"])
    ec = LC.row_err(LC.classic(s["x"], g, b, EPS, w16, bias, 0, prec, round_out=False), s["ref"], s["fam"])
    bad = {}
    for name, want in CURVE.items():
        fams = ("spike1e3", "spike3e4") if name == "spike" else (name,)
        m = sum((s["fam"] == LC.FID[f]) for f in fams).bool()
        got = (ec[m].max().item(), ef[m].max().item())
        print(f"{prec} {name:<11} classic {got[0]:.2e} (table {want[col]:.1e})  folded {got[1]:.2e} (table {want[col + 1]:.1e})")
        for gv, wv in zip(got, want[col:col + 2]):
            if not wv / CURVE_FACTOR <= gv <= wv * CURVE_FACTOR:
                bad[name] = (got, want[col:col + 2])
    assert not bad, bad


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_the_unmutated_emulations_pass_every_family(study, prec):
    for C in (1280, 768):
        s = study[C, prec]
        g, b, w16, bias = s["w"]
        LC.check(f"folded emulation C={C} {prec}", s["emu"], s["bar"], s["fam"])
        e32 = LC.row_err(LC.ln_mutant64(s["x"], g, b, EPS), s["ref32"], s["fam"])
        LC.check(f"tiled-statistics LayerNorm in float64 C={C}", e32, s["bar32"], s["fam"])
        e32 = LC.row_err(LC.ln32(s["x"], g, b, EPS), s["ref32"], s["fam"])
        LC.check(f"fp32 emulation C={C}", e32, s["bar32"], s["fam"])
        st, bar = LC.bar_stats(s["x"], s["fam"])
        LC.check(f"fp32 tiled statistics C={C}", (LC.tile_stats32(s["x"]).double() - st).abs(), bar, s["fam"])


@pytest.mark.parametrize("mutant", list(LC.MUTANTS))
def test_every_mutant_exceeds_its_bar_on_the_named_family(study, mutant):
    fam_gemm, fam_ln, C = CAUGHT_BY[mutant]
    for prec in ("fp16", "bf16"):
        s = study[C, prec]
        g, b, w16, bias = s["w"]
        e = LC.row_err(LC.folded(s["x"], g, b, EPS, w16, bias, 0, prec, mutant), s["ref"], s["fam"])
        caught = LC.failures(LC.per_family(e, s["bar"], s["fam"]))
        print(f"{mutant} ({LC.MUTANTS[mutant]}) C={C} {prec}: folded GEMM over its bar on {sorted(caught)}")
        assert fam_gemm in caught, (mutant, prec, sorted(caught))
        if fam_ln is not None:
            e = LC.row_err(LC.ln_mutant64(s["x"], g, b, EPS, mutant), s["ref32"], s["fam"])
            caught = LC.failures(LC.per_family(e, s["bar32"], s["fam"]))
            print(f"{mutant} C={C}: fp32 LayerNorm over its bar on {sorted(caught)}")
            assert fam_ln in caught, (mutant, sorted(caught))


def test_ln_combine_mutants_show_in_the_statistics_bar():
    """The tiled (mean, M2) bar sees a partial landing in the neighbouring tile's slot or the next row's."""
    x, fam = LC.rows(768, ROWS, 0)
    ref, bar = LC.bar_stats(x, fam)
    assert "tilestep" in LC.failures(LC.per_family((torch.roll(ref, 1, 1) - ref).abs(), bar, fam))
    assert "offset1000" in LC.failures(LC.per_family((torch.roll(ref, -1, 0) - ref).abs(), bar, fam))
