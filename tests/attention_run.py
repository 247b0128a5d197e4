"""What tests/test_gpu_attention_queries.py and its 4-wave child process share: a launch into a guarded buffer, repeated; the
figures of one case beside their bars (attention_cases.py); the encoder-form runner.  GPU only, through the C ABI."""
import torch

import attention_cases as A
import gpu_util as G

N = G.N
GUARD = 256                     # bytes on either side of an output
WINDOW_B, GLOBAL_B, HEADS = 4, 2, 2
GLOBAL_CASES = [(prec, hd, kind) for prec in ("fp16", "bf16") for hd in (64, 80) for kind in ("select", "pair", "diffuse")]


def guarded(rows, stride, dt):
    """(the whole uint8 allocation filled with 0xff, its [rows, stride] view of dtype dt behind GUARD bytes)."""
    nbytes = rows * stride * torch.empty((), dtype=dt).element_size()
    buf = torch.full((nbytes + 2 * GUARD,), 255, dtype=torch.uint8, device=G.dev())
    return buf, buf[GUARD:GUARD + nbytes].view(dt).view(rows, stride)


def contained(name, buf, view, cols):
    """Guards and gap columns still hold the sentinel; every output element was written (0xff.. is a NaN no kernel returns)."""
    assert bool((buf[:GUARD] == 255).all()) and bool((buf[-GUARD:] == 255).all()), f"{name}: guard bytes written"
    raw = view.view(torch.int16 if view.element_size() == 2 else torch.int32)
    assert bool((raw[:, cols:] == -1).all()), f"{name}: gap columns written"
    unwritten = (raw[:, :cols] == -1)
    assert not bool(unwritten.any()), f"{name}: {int(unwritten.sum())} output elements never written, first row {int(unwritten.any(1).nonzero()[0])}"


def launch_twice(name, launch, rows, stride, cols, dt):
    buf, view = guarded(rows, stride, dt)
    launch(view)
    torch.cuda.synchronize()
    contained(name, buf, view, cols)
    first = buf.clone()
    launch(view)
    torch.cuda.synchronize()
    assert torch.equal(buf, first), f"{name}: a repeated launch gave other bits"
    return view[:, :cols]


def measure(name, case, got_of_item, vrows_of_item):
    """The conditions on the reference, the kernel's and the emulation's row errors per item, the figures beside their bars."""
    B, heads, nq, dev = case.B, case.heads, case.nq, G.dev()
    e2, ee, r2, f2, t2 = (torch.zeros(B, heads, nq, dtype=torch.float64, device=dev) for _ in range(5))
    least = []
    for b in range(B):
        for h in range(heads):
            ref, p, n2 = A.item(case, b, h, want_p=True)
            assert bool((ref.pow(2).sum(-1) > 0).all()), f"{name}: a zero reference row"
            if case.kind in ("select", "pair"):
                m = A.designated_mass(case, b, h, p).min().item()
                least.append(m)
                assert m >= (0.99 if case.kind == "select" else 0.49), (name, b, h, m)
            if case.kind == "pads":
                s = A.pad_share(case, p)
                least += [s.min().item(), s.max().item()]
                assert 0.3 <= min(least) and max(least) <= 0.7, (name, b, h, least)
            del p
            emu = A.item(case, b, h, emu=A.emu_of(case))
            got = got_of_item(b, h).double()
            assert bool(torch.isfinite(got).all()), f"{name}: non-finite output, image {b} head {h}"
            e2[b, h], r2[b, h] = A.row_sums(got, ref)
            ee[b, h], _ = A.row_sums(emu, ref)
            f2[b, h] = A.floor2(ref, case.prec)
            if case.prec != "fp32":
                t2[b, h] = A.noise2(n2, case.prec)
    ev, excluded = A.evaluate(case, e2, ee, r2, f2, t2)
    cond = "" if not least else (f"  [designated mass >= {min(least):.6f}]" if case.kind != "pads" else f"  [padded share {min(least):.3f} .. {max(least):.3f}]")
    print(A.line(name, ev) + cond)
    assert excluded == 0
    bad = A.over(ev)
    if bad:
        gid = ev["query"][2]
        it, qi = gid // nq, gid % nq
        b, h = it // heads, it % heads
        where = A.describe_query(case, gid, got_of_item(b, h)[qi], vrows_of_item(b, h))
        raise AssertionError(f"{name}: over the bar {bad}; worst query: {where}")
    return ev


def encoder_case(name, kind, window, B, heads, hd, prec):
    case = A.case_to(A.make_encoder_case(kind, window, B, heads, hd, prec), G.dev())
    D = heads * hd
    code, dt = G.PRECS[prec]

    def launch(out):
        N.check(N.lib().wm_op_encoder_attention(N.ptr(case.qkv), N.ptr(case.bias), N.ptr(case.rel_h), N.ptr(case.rel_w), N.ptr(out),
                                                B, heads, hd, window, code, G.sp()))
    out = launch_twice(name, launch, B * A.T, D, D, dt).view(B, A.T, heads, hd)
    x = case.qkv.view(B, A.T, 3, heads, hd)
    bias_v = case.bias.view(3, heads, hd)[2]
    return measure(name, case, lambda b, h: out[b, :, h], lambda b, h: torch.cat([x[b, :, 2, h].double(), bias_v[h][None].double()]))


def run_global_cases_4wave():
    """The child's body: every case of GLOBAL_CASES through whichever global kernel this process selects."""
    G.need_gpu()
    for prec, hd, kind in GLOBAL_CASES:
        encoder_case(f"global 4-wave {prec} hd {hd} {kind}", kind, 0, GLOBAL_B, HEADS, hd, prec)
