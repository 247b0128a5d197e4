"""CPU checks of tests/attention_cases.py: the oracle against wm_oracle's own attention pieces, the coverage conditions of every
case and shape tests/test_gpu_attention_queries.py runs, the bar code, and the mutant study (run with -s for the table;
profiles/attention_queries/mutants.txt is its output)."""
import pytest
import torch

from oracle import wm_oracle as O
import attention_cases as A

WINDOW_SHAPES = [(prec, hd) for prec in ("fp16", "bf16") for hd in (64, 80)]          # 4 images x 2 heads
WINDOW_B, GLOBAL_B, HEADS = 4, 2, 2
# the plain shapes of the GPU file: (B, heads, hd, nq, nk, prec); B the smallest with B heads nq >= nk
MHA16_SHAPES = [(2, 2, 64, 256, 128, "fp16"), (2, 2, 64, 128, 192, "bf16"), (2, 2, 64, 384, 64, "fp16"), (2, 2, 64, 128, 64, "bf16"),
                (2, 2, 128, 128, 128, "fp16"), (2, 2, 80, 256, 256, "bf16"), (1, 2, 128, 4096, 4096, "fp16")]
MHA32_SHAPES = [(11, 8, 16, 51, 4096, "fp32"), (1, 8, 16, 4096, 51, "fp32"), (8, 2, 16, 65, 1024, "fp32"), (10, 2, 16, 7, 130, "fp32"),
                (2, 8, 32, 51, 51, "fp32")]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.manual_seed(0)


def _item_sums(case, b, h, mutant=None, rows=None, ref=None):
    """(e2 of the emulation (or the mutated emulation), r2, f2, t2) of one item; ref = (out, P, p_noise2) of the exact oracle."""
    kw = {} if rows is None else {"rows": rows}
    ref, _, n2 = A.item(case, b, h, want_p=True, **kw) if ref is None else ref
    got = A.item(case, b, h, emu=A.emu_of(case), mutant=mutant, **kw)
    e2, r2 = A.row_sums(got, ref)
    return e2, r2, A.floor2(ref, case.prec), None if case.prec == "fp32" else A.noise2(n2, case.prec)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle is wm_oracle's
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [14, 0])
def test_oracle_equals_wm_oracle_pieces(window):
    B, heads, hd = 1, 2, 16 if not window else 64
    case = A.make_encoder_case("diffuse", window, B, heads, hd, "fp16", seed=3)
    D, S = heads * hd, 14 if window else 64
    x = case.qkv.double().reshape(B, 64, 64, 3 * D)
    bias = case.bias.double()
    if window:
        xw, n = O.to_windows(x - bias, window)
        xw = xw + bias
    else:
        xw, n = x, 0
    Bp = xw.shape[0]
    t = xw.reshape(Bp, S * S, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    Rh, Rw = O.rel_pos_table(S, case.rel_h.double()), O.rel_pos_table(S, case.rel_w.double())
    rq = q.reshape(Bp, heads, S, S, hd)
    rh = torch.einsum("bnhwc,hkc->bnhwk", rq, Rh)
    rw = torch.einsum("bnhwc,wkc->bnhwk", rq, Rw)
    a = (q @ k.transpose(-1, -2)) * hd ** -0.5
    a = (a.view(Bp, heads, S, S, S, S) + rh[..., :, None] + rw[..., None, :]).view(Bp, heads, S * S, S * S)
    o = (a.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(Bp, S, S, D)
    if window:
        o = O.from_windows(o, window, n, 64)
    want = o.reshape(4096, heads, hd)
    for h in range(heads):
        got = A.enc_item(case, 0, h)
        err = ((got - want[:, h]).norm() / want[:, h].norm()).item()
        print(f"window {window} head {h}: oracle vs wm_oracle pieces rel-L2 {err:.2e}")
        assert err < 1e-13                      # float64 round-off of two summation orders


def test_plain_oracle_equals_mha_core():
    case = A.make_plain_case("diffuse", 2, 3, 16, 51, 130, "fp32", seed=3)
    want = O.mha_core(case.q.double().reshape(2, 51, 48), case.k.double().reshape(2, 130, 48), case.v.double().reshape(2, 130, 48), 3,
                      O.OracleCfg()).view(2, 51, 3, 16)
    for b in range(2):
        for h in range(3):
            got = A.plain_item(case, b, h)
            assert ((got - want[b, :, h]).norm() / want[b, :, h].norm()).item() < 1e-13


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage conditions (of the reference alone)
# ---------------------------------------------------------------------------------------------------------------------------------
def _mass_conditions(case, items):
    lo = []
    for b, h in items:
        ref, p, _ = A.item(case, b, h, want_p=True)
        assert (ref.pow(2).sum(-1) > 0).all(), "a zero reference row"
        if case.kind in ("select", "pair"):
            m = A.designated_mass(case, b, h, p)
            lo.append(m.min().item())
            assert m.min().item() >= (0.99 if case.kind == "select" else 0.49), (case.kind, b, h, m.min().item())
        if case.kind == "pads":
            s = A.pad_share(case, p)
            lo.append(s.min().item()), lo.append(s.max().item())
            assert 0.3 <= s.min().item() and s.max().item() <= 0.7, (b, h, s.min().item(), s.max().item())
    return lo


@pytest.mark.parametrize("prec,hd", WINDOW_SHAPES)
def test_window_cases_meet_the_conditions(prec, hd):
    for kind in ("select", "pair", "pads", "diffuse"):
        case = A.make_encoder_case(kind, 14, WINDOW_B, HEADS, hd, prec)
        lo = _mass_conditions(case, [(b, h) for b in range(WINDOW_B) for h in range(HEADS)])
        msg = f"window {prec} hd {hd} {kind}:"
        if kind in ("select", "pair"):
            cov = A.target_coverage(case)
            assert cov == (0, 0, 0), cov
            assert A.maps_differ(case)
            msg += f" every one of 25 x 196 key slots a target, 27 + 27 table rows used, maps differ, least designated mass {min(lo):.6f}"
        if kind == "pads":
            msg += f" padded share of the edge windows' queries {min(lo):.3f} .. {max(lo):.3f}"
        print(msg)
    # the condition of the multi-item instance (B = CUs // 50 + 1 images, 2 heads x 80, fp16, select): checked for its targets at a B
    # of 6 (256 CUs); the masses do not depend on B
    case = A.make_encoder_case("select", 14, 6, HEADS, 80, "fp16")
    assert A.target_coverage(case) == (0, 0, 0) and A.maps_differ(case)


@pytest.mark.parametrize("prec,hd", WINDOW_SHAPES)
def test_global_cases_meet_the_conditions(prec, hd):
    for kind in ("select", "pair", "diffuse"):
        case = A.make_encoder_case(kind, 0, GLOBAL_B, HEADS, hd, prec)
        lo = _mass_conditions(case, [(b, h) for b in range(GLOBAL_B) for h in range(HEADS)])
        msg = f"global {prec} hd {hd} {kind}:"
        if kind != "diffuse":
            cov = A.target_coverage(case)
            assert cov == (0, 0, 0), cov
            assert A.maps_differ(case)
            msg += f" target maps are permutations, 127 + 127 table rows used, maps differ, least designated mass {min(lo):.6f}"
        print(msg)


@pytest.mark.parametrize("shape", MHA16_SHAPES + MHA32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plain_cases_meet_the_conditions(shape):
    B, heads, hd, nq, nk, prec = shape
    for kind in ("select", "pair", "diffuse"):
        case = A.make_plain_case(kind, B, heads, hd, nq, nk, prec)
        items = [(b, h) for b in range(B) for h in range(heads)]
        lo = _mass_conditions(case, items if nq * nk < 1 << 22 else items[:1] + items[-1:])
        msg = f"plain {shape} {kind}:"
        if kind != "diffuse":
            cov = A.target_coverage(case)
            assert cov == (0,), cov
            assert A.maps_differ(case)
            msg += f" every key a target, maps differ, least designated mass {min(lo):.6f}"
        print(msg)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bar code
# ---------------------------------------------------------------------------------------------------------------------------------
def _one_item_case(case, b, h):
    """A view of `case` as a case of the single item (b, h), for evaluate()."""
    one = A.SimpleNamespace(**vars(case))
    one.B, one.heads = 1, 1
    one.target = None if case.target is None else case.target[b:b + 1, h:h + 1]
    return one


@pytest.mark.parametrize("form", ["window", "plain16", "plain32"])
def test_emulation_passes_its_own_bars(form):
    case = {"window": lambda: A.make_encoder_case("pair", 14, 1, 1, 64, "bf16"),
            "plain16": lambda: A.make_plain_case("pair", 1, 1, 128, 128, 128, "fp16"),
            "plain32": lambda: A.make_plain_case("diffuse", 1, 1, 16, 65, 1024, "fp32")}[form]()
    e2, r2, f2, t2 = _item_sums(case, 0, 0)
    ev, excluded = A.evaluate(case, e2[None, None], e2[None, None], r2[None, None], f2[None, None], None if t2 is None else t2[None, None])
    print(A.line(f"emulation as the kernel, {form}", ev))
    assert excluded == 0 and not A.over(ev)


def test_another_reference_point_is_within_the_bars(monkeypatch):
    """The kernels round P at a reference point of their own (attention_cases.py, EMULATION): the emulation at another one is as
    right as the first, and must sit inside the bars the first gives -- on the diffuse case, where the P rounding is most of a
    row's error, and at head dim 80, whose bars carry no + u."""
    case = A.make_encoder_case("diffuse", 14, 1, 1, 80, "fp16")
    ref = A.item(case, 0, 0, want_p=True)
    ee, r2, f2, t2 = _item_sums(case, 0, 0, ref=ref)
    monkeypatch.setattr(A, "REF_SLACK_SHIFT", 0.437)
    e2 = _item_sums(case, 0, 0, ref=ref)[0]
    ev, _ = A.evaluate(case, e2[None, None], ee[None, None], r2[None, None], f2[None, None], t2[None, None])
    print(A.line("emulation at another reference point, window fp16 hd 80 diffuse", ev))
    own = (e2 / r2).sqrt() / torch.maximum(A.BAR_FACTOR * (ee / r2).sqrt(), (f2 / r2).sqrt())
    print(f"  against {A.BAR_FACTOR:g} x the row's own emulation error alone: worst query x{own.max().item():.2f}, {int((own > 1).sum())} of {own.numel()} over")
    assert not A.over(ev)


# ---------------------------------------------------------------------------------------------------------------------------------
# the mutant study: one image, one head per form; every mutant over a bar on some case
# ---------------------------------------------------------------------------------------------------------------------------------
def _study(make, kinds, mutants, prec, hd, rows=None):
    """Prints and returns {mutant: (case kind, metric, ratio to its bar)} of the first case kind that sees it, and whether the old
    criterion (whole-tensor relative L2 on the diffuse case below 2 x OUT16_TOL) sees it."""
    seen, old = {}, {}
    base = {}
    for kind in kinds:
        case = make(kind)
        b, h = case.B - 1, case.heads - 1                       # item (1, 1): mutants head_v0 / image_k0 read item 0's rows
        one = _one_item_case(case, b, h)
        if rows is not None:
            one.nq = len(rows)
            one.target = None if one.target is None else one.target[:, :, rows]
        ref = A.item(case, b, h, want_p=True, **({} if rows is None else {"rows": rows}))
        ee, r2, f2, t2 = _item_sums(case, b, h, rows=rows, ref=ref)
        base[kind] = (case, one, ee, r2, f2, t2, ref)
    for mutant in mutants:
        ratios = []
        for kind in kinds:
            case, one, ee, r2, f2, t2, ref = base[kind]
            if kind == "diffuse" or mutant not in seen:
                em = _item_sums(case, case.B - 1, case.heads - 1, mutant=mutant, rows=rows, ref=ref)[0]
                ev, _ = A.evaluate(one, em[None, None], ee[None, None], r2[None, None], f2[None, None], None if t2 is None else t2[None, None])
                metric, ratio = A.worst_ratio(ev)
                ratios.append((kind, metric, ratio))
                if ratio > 1 and mutant not in seen:
                    seen[mutant] = (kind, metric, ratio)
                if kind == "diffuse" and case.prec != "fp32":
                    old[mutant] = (em.sum() / r2.sum()).sqrt().item() >= 2 * A.OLD_OUT16_TOL[case.prec]
        best = seen.get(mutant) or max(ratios, key=lambda r: r[2])
        print(f"  {mutant:14s} {A.MUTANTS[mutant]:68s} {best[0]:8s} {best[1]:7s} x{best[2]:<10.3g} old criterion: "
              f"{'n/a' if mutant not in old else 'sees it' if old[mutant] else 'BLIND'}")
    return seen


def test_window_mutants_exceed_a_bar():
    seen = {}
    for prec, hd in (("fp16", 80), ("bf16", 64)):
        print(f"window kernel form, {prec} hd {hd}, image 1 head 1 of 2 x 2:")
        make = lambda kind: A.make_encoder_case(kind, 14, 2, 2, hd, prec)
        muts = [m for m in A.WINDOW_MUTANTS if m != "den_unrounded" or A.den_rounded(hd)]
        seen[hd] = _study(make, ("select", "pair", "pads", "diffuse"), muts, prec, hd)
        assert set(seen[hd]) == set(muts), sorted(set(muts) - set(seen[hd]))


@pytest.mark.parametrize("prec,hd", [("fp16", 80), ("bf16", 64)])
def test_global_mutants_exceed_a_bar(prec, hd):
    """One (image, head) at a time, on the queries of grid rows 0, 31, 32 and 63 (every column): they reach every row of both tables
    (rows 0, 63, 64, 126 of rel_h through key rows 63, 0 and the query's own)."""
    print(f"global kernel form, {prec} hd {hd}, image 1 head 1 of 2 x 2, query rows 0 / 31 / 32 / 63:")
    rows = torch.cat([torch.arange(64) + 64 * r for r in (0, 31, 32, 63)])
    make = lambda kind: A.make_encoder_case(kind, 0, 2, 2, hd, prec)
    muts = [m for m in A.GLOBAL_MUTANTS if m != "den_unrounded" or A.den_rounded(hd)]
    seen = _study(make, ("select", "pair", "diffuse"), muts, prec, hd, rows=rows)
    assert set(seen) == set(muts), sorted(set(muts) - set(seen))


@pytest.mark.parametrize("shape", [(2, 2, 80, 256, 256, "fp16"), (2, 2, 128, 128, 128, "bf16"), (2, 2, 16, 65, 1024, "fp32")],
                         ids=lambda s: "x".join(map(str, s)))
def test_plain_mutants_exceed_a_bar(shape):
    B, heads, hd, nq, nk, prec = shape
    print(f"plain form {shape}, image 1 head 1:")
    make = lambda kind: A.make_plain_case(kind, B, heads, hd, nq, nk, prec)
    muts = [m for m in A.PLAIN_MUTANTS if m != "den_unrounded" or (prec != "fp32" and A.den_rounded(hd))]
    seen = _study(make, ("select", "pair", "diffuse"), muts, prec, hd)
    assert set(seen) == set(muts), sorted(set(muts) - set(seen))
