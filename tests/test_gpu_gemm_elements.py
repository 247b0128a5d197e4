"""The GEMM family element by element (-m gpu): every kernel instance behind wm_op_gemm16, wm_op_gemm16_stats, wm_op_gemm16_split,
wm_op_conv3x3_16, wm_op_patch_embed16, wm_op_gemm32 and wm_op_gemm8 / wm_op_gemm8_planes, through the C ABI, against the float64
oracle of tests/gemm_cases.py.  probe and exact cases are held to ZERO mismatching elements (the operands are small integers: every
partial sum is exact in fp32 in any order); gelu and sums print every figure beside a bar computed in the same run from the oracle
(gemm_cases.py has the rules).  Each launch writes into buffers with guard bytes on both sides (untouched afterwards), pre-filled
with a NaN pattern (every element written), is repeated (the same bits), and the kernel instance that ran is asserted from
wm_debug_gemm_variant_counts.  Shapes come from the dispatch in host_gemm.h: the smallest that reach each instance.
Run with -s for the figures; profiles/gemm_elements/gpu_tests.txt is that output."""
import re
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_run as R            # the guarded buffer
import gemm_cases as C
import gpu_util as G

N = G.N
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()
    yield
    print(f"\n[gemm elements: {time.time() - T0:.1f} s wall for the module]")


# ---------------------------------------------------------------------------------------------------------------------------------
# one guarded, repeated, counted launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch(name, variant, spec, fn):
    """spec {output: (rows, cols, dtype, initial content or None)}; fn(views) launches once.  Returns the views."""
    bufs = {o: R.guarded(rows, cols, dt) for o, (rows, cols, dt, _) in spec.items()}

    def fill():
        for o, (buf, view) in bufs.items():
            buf.fill_(255)
            if spec[o][3] is not None:
                view.copy_(spec[o][3])
    views = {o: v for o, (_, v) in bufs.items()}
    fill()
    N.gemm_variant_counts(reset=True)
    fn(views)
    torch.cuda.synchronize()
    ran = {k: v for k, v in N.gemm_variant_counts().items() if v}
    assert ran == ({variant: 1} if variant else {}), f"{name}: ran {ran}, wanted {variant}"
    for o, (buf, view) in bufs.items():
        assert bool((buf[:R.GUARD] == 255).all()) and bool((buf[-R.GUARD:] == 255).all()), f"{name}: guard bytes of {o} written"
        if spec[o][3] is None:
            raw = view.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[view.element_size()])
            unwritten = raw == -1
            assert not bool(unwritten.any()), f"{name}: {int(unwritten.sum())} elements of {o} never written, first row {int(unwritten.any(1).nonzero()[0])}"
    first = {o: buf.clone() for o, (buf, _) in bufs.items()}
    fill()
    fn(views)
    torch.cuda.synchronize()
    for o, (buf, _) in bufs.items():
        assert torch.equal(buf, first[o]), f"{name}: a repeated launch gave other bits in {o}"
    return views


def _dev(c):
    return C.case_to(c, G.dev())


def _named_right(name, c):
    """A printed line that names a shape M x N x K names the shape of the case that ran."""
    shape = re.search(r"\d+x\d+x\d+", name)
    assert shape is None or shape.group(0) == f"{c.M}x{c.N}x{c.K}", f"{name}: the case is {c.M}x{c.N}x{c.K}"


def _check_exact(name, c, got):
    """probe / exact: zero mismatching elements against the float64 answer and its defined roundings."""
    _named_right(name, c)
    y = C.ref64(c)
    assert C.is_exact32(y), f"{name}: the reference is not exact in fp32"
    if c.kind == "exact":
        assert C.exact_bound(c) < 2 ** 24
    if c.kind == "probe" and c.bias is None and c.res is None and (c.form == "plain" or c.side == "a"):
        assert torch.equal(y, C.probe_answer(c))
    want = C.expected(c, y, tuple(got))
    parts = []
    for o in got:
        n, where = C.mismatches(got[o], want[o])
        parts.append(f"{o} {n} of {got[o].numel()}")
        assert n == 0, f"{name}: {n} mismatching elements of {o}; " + C.describe(c, got[o], want[o], where)
    extra = ""
    if c.sat_cols is not None:
        sat = got["o16"][:, c.sat_cols].float().abs() == 65504
        assert bool(sat.all()) and torch.equal(y.abs() > 65504, c.sat_cols[None, :].expand_as(y))
        extra = f"  [{int(c.sat_cols.sum()) * c.M} elements saturated at +-65504]"
    print(f"{name:92s} mismatches: {', '.join(parts)}{extra}")


def _assert_sweep(name, c):
    """The launch's own (M, N, K) sweeps what the gelu case claims (and is one of the shapes the CPU test asserts it for)."""
    s = C.gelu_sweep(c)
    assert (c.M, c.N, c.K) in C.GELU_SHAPES and C.gelu_sweep_ok(s), f"{name}: {vars(s)}"
    return f"[x in {s.lo:g} .. {s.hi:g}, largest gap {s.gap:g}, {s.near0} non-zero |x| < 1e-3, clamp point within {s.clamp:.3f}, {s.tail} tail elements]"


def _check_gelu(name, c, got):
    _named_right(name, c)
    print(f"{name:80s} sweep {_assert_sweep(name, c)}")
    y = C.ref64(c)
    for o, t in got.items():
        f = C.gelu_figures(c, t, y, None if o == "f32" else C.out_prec(c))
        print(f"{name:80s} {o}: worst |err| {f.err:.3e} at x = {f.x:+.5f} | bar {f.bar:.3e}  x{f.ratio:.2f}; NaN {f.nans}; largest (value - bar) for x < 0: {f.pos_over:.2e}")
        assert f.nans == 0 and f.ratio <= 1 and f.pos_over <= 0, f"{name} {o}: {vars(f)}"


def _check_sums(name, c, got, form="mfma16", cpu_c=None):
    """cpu_c: the CPU copy of the case (its float32 product by torch on the CPU gives the measured bar)."""
    _named_right(name, c)
    y, s = C.ref64(c, want_s=True)
    if form == "split":
        s = s + C.split_abs_term(c)
    if cpu_c.kind == "sums" and cpu_c.bias is None and cpu_c.res is None:
        block = (y.abs() / s)[3::8, 5::8]
        assert block.max().item() < 2e-2, f"{name}: the cancellation block does not cancel ({block.max().item():.2e})"
    cpu32, blas = C.cpu_product32(cpu_c, C.CHAIN[form]).to(G.dev()), C.cpu_product32(cpu_c).to(G.dev())
    for o, t in got.items():
        f = C.sums_figures(c, t, y, s, cpu32, None if o == "f32" else C.out_prec(c), form, cpu_blas=blas)
        print(f"{name} {o}: " + "\n    ".join(f.lines))
        assert not f.over, f"{name} {o}: over {f.over}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------------
def _op16(t, prec, packed=False):
    t16 = t.to(C.DT[prec])
    assert torch.equal(t16.float(), t)
    return G.pack16_torch(t16).contiguous() if packed else t16.contiguous()


def run_gemm16(name, variant, c, outs="both", layout=0, inplace=False):
    """wm_op_gemm16.  outs f32 | both | 16; inplace: the fp32 residual IS the fp32 output buffer (res rows = M)."""
    code, dt = G.PRECS[c.prec]
    a = _op16(c.a, c.prec, bool(layout & N.GEMM_A_PACKED))
    w = _op16(c.w, c.prec, bool(layout & N.GEMM_W_PACKED))
    spec = {}
    if outs != "16":
        spec["f32"] = (c.M, c.N, torch.float32, c.res if inplace else None)
    if outs != "f32":
        spec["o16"] = (c.M, c.N, dt, None)
    assert not inplace or (c.res.shape[0] == c.M and outs != "16")

    def fn(v):
        res = v["f32"] if inplace else c.res
        N.check(N.lib().wm_op_gemm16(N.ptr(a), N.ptr(w), N.ptr(c.bias), N.ptr(res), 0 if inplace else c.res_mod, N.ptr(v.get("f32")), N.ptr(v.get("o16")),
                                     c.M, c.N, c.K, c.act | layout, code, G.sp()))
    got = dict(_launch(name, variant, spec, fn))
    if layout & N.GEMM_OUT_PACKED:
        got["o16"] = G.unpack16_torch(got["o16"].contiguous())
    return got


def run_stats(name, variant, c, layout=0):
    """wm_op_gemm16_stats (the folded LayerNorm's producer): fp32 rows in place, the 16-bit copy in LDS-image order."""
    code, dt = G.PRECS[c.prec]
    a = _op16(c.a, c.prec, bool(layout & N.GEMM_A_PACKED))
    w = _op16(c.w, c.prec, bool(layout & N.GEMM_W_PACKED))
    spec = {"f32": (c.M, c.N, torch.float32, c.res), "o16": (c.M, c.N, dt, None), "stats": (c.M, c.N // G.fold_bn(c.N) * 2, torch.float32, None)}

    def fn(v):
        N.check(N.lib().wm_op_gemm16_stats(N.ptr(a), N.ptr(w), N.ptr(c.bias), N.ptr(v["f32"]), N.ptr(v["f32"]), N.ptr(v["o16"]), N.ptr(v["stats"]),
                                           c.M, c.N, c.K, layout, code, G.sp()))
    v = _launch(name, variant, spec, fn)
    return {"f32": v["f32"], "o16": G.unpack16_torch(v["o16"].contiguous())}


def run_split(name, variant, c, layout=0):
    """wm_op_gemm16_split: the residual comes in and leaves as the planes (hi, lo) in LDS-image order."""
    code, dt = G.PRECS[c.prec]
    a = _op16(c.a, c.prec, bool(layout & N.GEMM_A_PACKED))
    w = _op16(c.w, c.prec, bool(layout & N.GEMM_W_PACKED))
    hi0, lo0 = C.planes(c.res, c.prec)
    assert torch.equal(hi0.double() + lo0.double(), c.res.double())           # the planes hold the case's residual exactly
    spec = {"hi": (c.M, c.N, dt, G.pack16_torch(hi0)), "lo": (c.M, c.N, torch.float16, G.pack16_torch(lo0)),
            "stats": (c.M, c.N // G.fold_bn(c.N) * 2, torch.float32, None)}

    def fn(v):
        N.check(N.lib().wm_op_gemm16_split(N.ptr(a), N.ptr(w), N.ptr(c.bias), N.ptr(v["hi"]), N.ptr(v["lo"]), N.ptr(v["stats"]), c.M, c.N, c.K, layout, code, G.sp()))
    v = _launch(name, variant, spec, fn)
    return {"hi": G.unpack16_torch(v["hi"].contiguous()), "lo": G.unpack16_torch(v["lo"].contiguous())}


def run_conv(name, c):
    code, dt = G.PRECS[c.prec]
    x, w = _op16(c.x, c.prec), _op16(c.w, c.prec)

    def fn(v):
        N.check(N.lib().wm_op_conv3x3_16(N.ptr(x), N.ptr(w), N.ptr(v["f32"]), c.B, c.N, c.Cin, code, G.sp()))
    return dict(_launch(name, "v3_conv3x3", {"f32": (c.M, c.N, torch.float32, None)}, fn))


def run_patch(name, c, outs="both"):
    code, dt = G.PRECS[c.prec]
    x, w = _op16(c.x, c.prec), _op16(c.w, c.prec)
    spec = {"o16": (c.M, c.N, dt, None)}
    if outs == "both":
        spec["f32"] = (c.M, c.N, torch.float32, None)

    def fn(v):
        N.check(N.lib().wm_op_patch_embed16(N.ptr(x), N.ptr(w), N.ptr(c.bias), N.ptr(v.get("f32")), N.ptr(v["o16"]), c.B, c.N, c.Cin, code, G.sp()))
    return dict(_launch(name, "v3_patch_embed", spec, fn))


GEMM32_FLAG = {"mfma32": 0, "split": N.GEMM32_SPLIT, "presplit": N.GEMM32_PRESPLIT}


def run_gemm32(name, c, mode):
    """wm_op_gemm32: the fp32 MFMA kernel, the split form with W split per K-step, the engine's pre-split form.  (No variant counter
    covers these kernels: the mode is the caller's explicit flag.)"""
    a, w = c.a.contiguous(), c.w.contiguous()

    def fn(v):
        N.check(N.lib().wm_op_gemm32(N.ptr(a), N.ptr(w), N.ptr(c.bias), N.ptr(c.res), N.ptr(v["f32"]), c.M, c.N, c.K, c.act | GEMM32_FLAG[mode], G.sp()))
    return dict(_launch(name, None, {"f32": (c.M, c.N, torch.float32, None)}, fn))


def _e4m3(t):
    b = t.to(torch.float8_e4m3fn)
    assert torch.equal(b.float(), t)
    return b.view(torch.uint8).contiguous()


def run_gemm8(name, c, mode):
    """wm_op_gemm8: mode f32 (residual + fp32 in place), f32+16, 16, 8; wm_op_gemm8_planes: mode planes (row-major planes, plane order)."""
    code, dt = G.PRECS[c.prec16]
    a, w = _e4m3(c.a), _e4m3(c.w)
    if mode == "planes":
        pos = G.plane_pos(c.N, G.dev())
        hi0, lo0 = C.planes(c.res, c.prec16)
        assert torch.equal(hi0.double() + lo0.double(), c.res.double())
        hp, lp = torch.empty_like(hi0), torch.empty_like(lo0)
        hp[:, pos], lp[:, pos] = hi0, lo0
        spec = {"hi": (c.M, c.N, dt, hp), "lo": (c.M, c.N, torch.float16, lp)}

        def fn(v):
            N.check(N.lib().wm_op_gemm8_planes(N.ptr(a), N.ptr(w), N.ptr(c.wscale), N.ptr(c.bias), N.ptr(v["hi"]), N.ptr(v["lo"]), c.M, c.N, c.K, code, G.sp()))
        v = _launch(name, "fp8_256_planes", spec, fn)
        return {"hi": v["hi"][:, pos], "lo": v["lo"][:, pos]}
    spec = {}
    if mode in ("f32", "f32+16"):
        spec["f32"] = (c.M, c.N, torch.float32, c.res)
    if mode in ("16", "f32+16"):
        spec["o16"] = (c.M, c.N, dt, None)
    if mode == "8":
        spec["o8"] = (c.M, c.N, torch.uint8, None)

    def fn(v):
        N.check(N.lib().wm_op_gemm8(N.ptr(a), N.ptr(w), N.ptr(c.wscale), N.ptr(c.bias), N.ptr(v.get("f32")), N.ptr(v.get("f32")), N.ptr(v.get("o16")),
                                    N.ptr(v.get("o8")), c.M, c.N, c.K, c.act, code, G.sp()))
    got = dict(_launch(name, "fp8_256", spec, fn))
    if "o8" in got:
        got["o8"] = got["o8"].view(torch.float8_e4m3fn)
    return got


def _probes(M, N, K, prec, tile, **kw):
    """Both mirror images, every launch that the coverage of all k needs."""
    for side, t in (("w", tile[0]), ("a", tile[1])):
        for j in range(C.probe_launches(K, t)):
            yield f"probe {side} coded j={j}", C.make_probe(M, N, K, prec, tile, side, j, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# v1_128: M % 256 != 0
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_v1_128(prec):
    """gemm16_kernel 128 x 128 x 64: 384 x 256 = three row tiles in a partly filled group; K = 64 (one step) and 320 (five)."""
    M, Nn, tile, V = 384, 256, (128, 128), "v1_128"
    for K in (64, 320):
        tag = f"v1_128 {prec} {M}x{Nn}x{K}"
        for pname, c in _probes(M, Nn, K, prec, tile, bias=True, res_rows=128):
            c = _dev(c)
            _check_exact(f"{tag} {pname} bias res_mod=128 both", c, run_gemm16(tag, V, c, "both"))
        c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K, res_rows=M))
        _check_exact(f"{tag} exact in-place residual both", c, run_gemm16(tag, V, c, "both", inplace=True))
        c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K + 1, res_rows=128, act=2))
        _check_exact(f"{tag} exact ReLU res_mod=128 f32", c, run_gemm16(tag, V, c, "f32"))
        c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K + 2))
        _check_exact(f"{tag} exact bias 16", c, run_gemm16(tag, V, c, "16"))
        c = _dev(C.make_gelu(M, Nn, K, prec, tile))
        _check_gelu(f"{tag} gelu", c, run_gemm16(tag, V, c, "both"))
    if prec == "fp16":
        c = _dev(C.make_exact(M, Nn, 320, prec, tile, seed=7, saturate=True))
        _check_exact(f"{tag} exact saturating both", c, run_gemm16(tag, V, c, "both"))
    cpu = C.make_sums(M, Nn, 320, prec, tile, seed=11)
    _check_sums(f"{tag} sums", _dev(cpu), run_gemm16(tag, V, _dev(cpu), "both"), cpu_c=cpu)


# ---------------------------------------------------------------------------------------------------------------------------------
# v2_128 / v2_160: the half-width kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("Nn,V", [(512, "v2_128"), (640, "v2_160")])
def test_v2(Nn, V, prec):
    """gemm16v2_kernel<128 | 160>, 256-row tiles, K-steps of 64 through a 3-slot ring: K = 64 (one step) and 448 (seven: two ring
    turns and a step); M = 256 and 768; the three output combinations; residual in place and with res_mod."""
    tile = (256, int(V[-3:]))
    for M, K in ((256, 64), (768, 448)):
        tag = f"{V} {prec} {M}x{Nn}x{K}"
        for pname, c in _probes(M, Nn, K, prec, tile, bias=True, res_rows=256):
            c = _dev(c)
            _check_exact(f"{tag} {pname} bias res_mod=256 both", c, run_gemm16(tag, V, c, "both"))
        for outs in ("f32", "both", "16"):
            c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K + len(outs), res_rows=256))
            _check_exact(f"{tag} exact res_mod=256 {outs}", c, run_gemm16(tag, V, c, outs))
        c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K + 5, res_rows=M))
        _check_exact(f"{tag} exact in-place residual both", c, run_gemm16(tag, V, c, "both", inplace=True))
        c = _dev(C.make_exact(M, Nn, K, prec, tile, seed=K + 6, act=2))
        _check_exact(f"{tag} exact ReLU 16", c, run_gemm16(tag, V, c, "16"))
        c = _dev(C.make_gelu(M, Nn, K, prec, tile))
        _check_gelu(f"{tag} gelu", c, run_gemm16(tag, V, c, "both"))
    if prec == "fp16":
        c = _dev(C.make_exact(768, Nn, 64, prec, tile, seed=8, saturate=True))
        tag = f"{V} {prec} {c.M}x{c.N}x{c.K}"
        _check_exact(f"{tag} exact saturating both", c, run_gemm16(tag, V, c, "both"))
    cpu = C.make_sums(768, Nn, 448, prec, tile, seed=12, bias=True, res_rows=256)
    tag = f"{V} {prec} {cpu.M}x{cpu.N}x{cpu.K}"
    _check_sums(f"{tag} sums bias res_mod=256", _dev(cpu), run_gemm16(tag, V, _dev(cpu), "both"), cpu_c=cpu)


# ---------------------------------------------------------------------------------------------------------------------------------
# v5: the 256-row-tile kernel, 129+ tiles (gemm16_takes_v5)
# ---------------------------------------------------------------------------------------------------------------------------------
V5 = [(1280, 320), (1024, 256)]
M5 = 33 * 256                                    # x 4 column tiles = 132 tiles: one partly filled round of 256 workgroups
M5_ROUNDS = 129 * 256                            # x 4 = 516 tiles: two rounds and four tiles (260 .. 384 tiles go to the half-width kernel)
PACKED = N.GEMM_W_PACKED | N.GEMM_A_PACKED | N.GEMM_OUT_PACKED


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("Nn,bn", V5)
def test_v5_probes(Nn, bn, prec):
    """gemm16v5_kernel<320 | 256>: K = 64 (the minimum, two K-steps of 32) and 320 (ten: not a multiple of the three ring slots), both
    mirror images, plain and packed operands, with and without the residual."""
    tile = (256, bn)
    for K in (64, 320):
        tag = f"v5_{bn} {prec} {M5}x{Nn}x{K}"
        for pname, c in _probes(M5, Nn, K, prec, tile, bias=True):
            c = _dev(c)
            _check_exact(f"{tag} {pname} bias both", c, run_gemm16(tag, f"v5_{bn}", c, "both"))
            _check_exact(f"{tag} {pname} bias 16, W A OUT packed", c, run_gemm16(tag, f"v5_{bn}", c, "16", layout=PACKED))
        for pname, c in _probes(M5, Nn, K, prec, tile, bias=True, res_rows=4096):
            c = _dev(c)
            _check_exact(f"{tag} {pname} bias res_mod=4096 both", c, run_gemm16(tag, f"v5_{bn}_res", c, "both"))
    tag = f"v5_{bn} {prec} {M5_ROUNDS}x{Nn}x64"
    c = _dev(C.make_probe(M5_ROUNDS, Nn, 64, prec, tile, "w", bias=True))
    _check_exact(f"{tag} probe w coded bias both (516 tiles: three rounds)", c, run_gemm16(tag, f"v5_{bn}", c, "both"))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("Nn,bn", V5)
def test_v5_exact(Nn, bn, prec):
    tile, K = (256, bn), 320
    tag = f"v5_{bn} {prec} {M5}x{Nn}x{K}"
    V, VR = f"v5_{bn}", f"v5_{bn}_res"
    c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=1))
    _check_exact(f"{tag} exact bias both", c, run_gemm16(tag, V, c, "both"))
    _check_exact(f"{tag} exact bias 16, W packed", c, run_gemm16(tag, V, c, "16", layout=N.GEMM_W_PACKED))
    _check_exact(f"{tag} exact bias 16, A packed", c, run_gemm16(tag, V, c, "16", layout=N.GEMM_A_PACKED))
    _check_exact(f"{tag} exact bias 16, OUT packed", c, run_gemm16(tag, V, c, "16", layout=N.GEMM_OUT_PACKED))
    _check_exact(f"{tag} exact bias 16, W A OUT packed", c, run_gemm16(tag, V, c, "16", layout=PACKED))
    c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=2, act=2))
    _check_exact(f"{tag} exact ReLU both, W A packed", c, run_gemm16(tag, V, c, "both", layout=N.GEMM_W_PACKED | N.GEMM_A_PACKED))
    for outs in ("f32", "both", "16"):
        c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=3 + len(outs), res_rows=4096))
        _check_exact(f"{tag} exact res_mod=4096 {outs}", c, run_gemm16(tag, VR, c, outs))
    c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=9, res_rows=M5))
    _check_exact(f"{tag} exact in-place residual both, W A packed", c, run_gemm16(tag, VR, c, "both", layout=N.GEMM_W_PACKED | N.GEMM_A_PACKED, inplace=True))
    if prec == "fp16":
        c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=10, saturate=True))
        _check_exact(f"{tag} exact saturating both", c, run_gemm16(tag, V, c, "both"))
        _check_exact(f"{tag} exact saturating 16, OUT packed", c, run_gemm16(tag, V, c, "16", layout=N.GEMM_OUT_PACKED))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("Nn,bn", V5)
def test_v5_gelu(Nn, bn, prec):
    tile = (256, bn)
    tag = f"v5_{bn} {prec} {M5}x{Nn}x320"
    c = _dev(C.make_gelu(M5, Nn, 320, prec, tile))
    _check_gelu(f"{tag} gelu", c, run_gemm16(tag, f"v5_{bn}", c, "both"))
    _check_gelu(f"{tag} gelu 16, W A OUT packed", c, run_gemm16(tag, f"v5_{bn}", c, "16", layout=PACKED))


@pytest.mark.parametrize("Nn,bn,prec", [(1280, 320, "fp16"), (1024, 256, "bf16")])
def test_v5_longest_k(Nn, bn, prec):
    """K = 5120, the family's longest: exact (|sum| up to 46080 + bias + residual < 65504) and sums."""
    tile, K = (256, bn), 5120
    tag = f"v5_{bn} {prec} {M5}x{Nn}x{K}"
    c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=21, res_rows=M5))
    _check_exact(f"{tag} exact in-place residual both", c, run_gemm16(tag, f"v5_{bn}_res", c, "both", inplace=True))
    del c
    cpu = C.make_sums(M5, Nn, K, prec, tile, seed=22)
    _check_sums(f"{tag} sums", _dev(cpu), run_gemm16(tag, f"v5_{bn}", _dev(cpu), "both"), cpu_c=cpu)


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream producers: the stream outputs only (row statistics and the consumer: tests/test_gpu_layernorm_rows.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("Nn,bn", V5)
def test_v5_stream_producers(Nn, bn, prec):
    """v5_*_foldp (fp32 rows in place + the 16-bit copy in LDS-image order) and v5_*_split (planes hi = round16(v), lo = fp16(v - hi)
    in and out, LDS-image order)."""
    tile, K = (256, bn), 320
    tag = f"{prec} {M5}x{Nn}x{K}"
    both = N.GEMM_W_PACKED | N.GEMM_A_PACKED
    for pname, c in _probes(M5, Nn, K, prec, tile, bias=True, res_rows=M5):
        c = _dev(c)
        _check_exact(f"v5_{bn}_foldp {tag} {pname} f32 + copy", c, run_stats(tag, f"v5_{bn}_foldp", c))
        _check_exact(f"v5_{bn}_split {tag} {pname} planes", c, run_split(tag, f"v5_{bn}_split", c))
    c = _dev(C.make_exact(M5, Nn, K, prec, tile, seed=31, res_rows=M5))
    _check_exact(f"v5_{bn}_foldp {tag} exact f32 + copy", c, run_stats(tag, f"v5_{bn}_foldp", c))
    _check_exact(f"v5_{bn}_foldp {tag} exact f32 + copy, W A packed", c, run_stats(tag, f"v5_{bn}_foldp", c, both))
    _check_exact(f"v5_{bn}_split {tag} exact planes", c, run_split(tag, f"v5_{bn}_split", c))
    _check_exact(f"v5_{bn}_split {tag} exact planes, W A packed", c, run_split(tag, f"v5_{bn}_split", c, both))


# ---------------------------------------------------------------------------------------------------------------------------------
# the implicit GEMMs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("B,Cin", [(1, 32), (2, 256)])
def test_conv3x3(B, Cin, prec):
    """gemm16v3_kernel<256, Conv3x3>: the probe puts the one-hot on (tap, ci), so every tap at every border pixel, and the zero page,
    are exact statements; its mirror image has one hot channel per pixel and coded weights."""
    tag = f"conv3x3 {prec} B={B} Cin={Cin} N=256"
    for j in range(C.probe_launches(9 * Cin, 256)):
        c = _dev(C.make_conv("probe", B, Cin, 256, prec, j=j))
        assert bool((c.x != 0).all())
        _check_exact(f"{tag} probe x coded j={j}", c, run_conv(tag, c))
    c = _dev(C.make_conv("probe_a", B, Cin, 256, prec))
    _check_exact(f"{tag} probe W coded", c, run_conv(tag, c))
    c = _dev(C.make_conv("exact", B, Cin, 256, prec, seed=B))
    _check_exact(f"{tag} exact", c, run_conv(tag, c))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("B,Cin,Nn", [(1, 1, 256), (2, 3, 320), (3, 3, 640)])
def test_patch_embed(B, Cin, Nn, prec):
    """gemm16v3_kernel<320 | 256, PatchEmbed>: the probe over (ci, ky, kx), both mirror images, with the bias.  (The op-level entry passes
    no residual: the pos-embed add of the engine's call is not reachable here.)"""
    tag = f"patch_embed {prec} B={B} Cin={Cin} N={Nn}"
    K = Cin * 256
    for j in range(C.probe_launches(K, 320 if Nn % 320 == 0 else 256)):
        c = _dev(C.make_patch("probe", B, Cin, Nn, prec, j=j))
        _check_exact(f"{tag} probe image coded j={j}", c, run_patch(tag, c))
    for j in range(C.probe_launches(K, 256)):
        c = _dev(C.make_patch("probe_a", B, Cin, Nn, prec, j=j))
        _check_exact(f"{tag} probe W coded j={j}", c, run_patch(tag, c, "16" if j else "both"))
    c = _dev(C.make_patch("exact", B, Cin, Nn, prec, seed=B))
    _check_exact(f"{tag} exact", c, run_patch(tag, c))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mfma32", "split", "presplit"])
def test_gemm32_exact(mode):
    """gemm32_kernel / gemm32x3_kernel<false | true>, 64 x 64 tiles with ragged edges.  Small integers split exactly into fp16 hi + lo
    (lo = 0), so probe and exact are bit-exact in the split forms too."""
    tile = (64, 64)
    for M, Nn in ((51, 4), (70, 8), (153, 14)):
        for K in (16, 32, 96) if mode == "mfma32" else (32, 96):
            tag = f"gemm32 {mode} {M}x{Nn}x{K}"
            for pname, c in _probes(M, Nn, K, "fp32", tile, bias=True, res_rows=M):
                c = _dev(c)
                _check_exact(f"{tag} {pname} bias res", c, run_gemm32(tag, c, mode))
            for act in (0, 2):
                c = _dev(C.make_exact(M, Nn, K, "fp32", tile, seed=K + act, res_rows=M, act=act))
                _check_exact(f"{tag} exact act={act} bias res", c, run_gemm32(tag, c, mode))


def _check_act32(name, c, got, cpu_c):
    """Sigmoid / GELU of the fp32 forms: |err| <= 4 x the float32 CPU evaluation's own worst error, floored at one fp32 ulp."""
    _named_right(name, c)
    print(f"{name:60s} sweep {_assert_sweep(name, c)}")
    y = C.ref64(c)
    pre = cpu_c.a @ cpu_c.w.t() + cpu_c.bias
    cpu32 = C.activate(pre, cpu_c.act).to(G.dev())
    err, err_cpu = (got["f32"].double() - y).abs(), (cpu32.double() - y).abs()
    bar = torch.maximum(torch.full_like(y, C.BAR_FACTOR * err_cpu.max().item()), C.ulp32(y))
    print(f"{name:60s} worst |err| {err.max().item():.3e} | bar {C.BAR_FACTOR:g} x cpu-fp32 {err_cpu.max().item():.3e} = {C.BAR_FACTOR * err_cpu.max().item():.3e}"
          f"  x{(err / bar).max().item():.2f}")
    assert bool(torch.isfinite(got["f32"]).all()) and bool((err <= bar).all())


@pytest.mark.parametrize("mode", ["mfma32", "split", "presplit"])
def test_gemm32_sums_and_activations(mode):
    tile, form = (64, 64), ("mfma32" if mode == "mfma32" else "split")
    for M, Nn, K in ((153, 14, 96), (70, 8, 32), (816, 256, 2048)):
        tag = f"gemm32 {mode} {M}x{Nn}x{K}"
        cpu = C.make_sums(M, Nn, K, "fp32", tile, seed=K, wsize=0.02)
        _check_sums(f"{tag} sums", _dev(cpu), run_gemm32(tag, _dev(cpu), mode), form=form, cpu_c=cpu)
    for act, what in ((1, "gelu"), (3, "sigmoid")):
        cpu = C.make_gelu(153, 70, 96, "fp16", tile)                      # the gelu case's sweep (its fp16-exact values are fp32 values)
        cpu.prec, cpu.act, cpu.bias = "fp32", act, torch.zeros(70)
        _check_act32(f"gemm32 {mode} 153x70x96 {what}", _dev(cpu), run_gemm32(f"gemm32 {mode} {what}", _dev(cpu), mode), cpu)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp8
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Nn,K", [(256, 256, 256), (1024, 768, 384)])
def test_gemm8(M, Nn, K):
    """gemm8_kernel<256> and its planes form: probe and exact only, operands exact in e4m3, wscale powers of two.  (The fp8 blocks'
    numerics are not emulated here.)"""
    tile = (256, 256)
    tag = f"gemm8 {M}x{Nn}x{K}"
    for pname, c in _probes(M, Nn, K, "fp8", tile, bias=True, res_rows=M):
        c = _dev(c)
        c.prec16 = "bf16"
        _check_exact(f"{tag} {pname} residual f32 + bf16", c, run_gemm8(tag, c, "f32+16"))
    for prec16 in ("bf16", "fp16"):
        c = _dev(C.make_exact(M, Nn, K, "fp8", tile, seed=K, res_rows=M))
        c.prec16 = prec16
        _check_exact(f"{tag} exact residual f32", c, run_gemm8(tag, c, "f32"))
        _check_exact(f"{tag} exact residual f32 + {prec16}", c, run_gemm8(tag, c, "f32+16"))
        _check_exact(f"{tag} exact planes {prec16}", c, run_gemm8(tag, c, "planes"))
        c = _dev(C.make_exact(M, Nn, K, "fp8", tile, seed=K + 1, act=2))
        c.prec16 = prec16
        _check_exact(f"{tag} exact ReLU {prec16} only", c, run_gemm8(tag, c, "16"))
    c = _dev(C.make_exact(M, Nn, K, "fp8", tile, seed=K + 2, amp=100))
    c.prec16 = "bf16"
    assert int((C.ref64(c).abs() > 448).sum()) > 0
    _check_exact(f"{tag} exact e4m3 output (ties, saturation at 448)", c, run_gemm8(tag, c, "8"))
