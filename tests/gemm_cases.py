"""The GEMM family's element cases: what tests/test_gpu_gemm_elements.py and tests/test_gemm_cases.py share.  Plain module (torch
only, any device), asserts nothing: the case builders, the float64 oracle of every form, the expected outputs, the metrics and bar
rules, a tiled emulation and its mutants.  Follows attention_cases.py / layernorm_cases.py.

FORMS.  A case holds a logical product  out[M, N] = act(A[M, K] W[N, K]^T * wscale[n] + bias[n]) + res[m % res_mod, n]
(gemm_common.h: bias, activation, residual in this order; wscale only for the fp8 form).  `form` says how A is stored:
  plain   A is a [M, K] matrix (wm_op_gemm16 / _stats / _split / wm_op_gemm8 / _planes / wm_op_gemm32);
  conv    A is gathered from an NHWC activation x [B, 64, 64, Cin]: k = tap * Cin + ci, tap = 3 (dy + 1) + (dx + 1), the pixel
          (y + dy, x + dx), zero outside the grid (wm_op_conv3x3_16);
  patch   A is gathered from an NCHW image img [B, Cin, 1024, 1024]: m = (b, py, px), k = ci * 256 + ky * 16 + kx, the pixel
          (16 py + ky, 16 px + kx) (wm_op_patch_embed16).
logical_a restates both gathers with explicit index arithmetic (no F.conv2d / unfold), so a mutant is a one-line switch.

ORACLE (ref64).  float64 product of the operands as stored (every case holds only values its operand type represents exactly;
test_gemm_cases.py asserts it), then bias, activation (GELU through erfc, which keeps the far negative tail), residual.

CASES
  probe  which operand element reaches which output element.  A[m, k] = [k == pi(m)], W[n, k] = code(n, k):
         out[m, n] = code(n, pi(m)) (probe_answer: a gather).  pi_j(m) = (11 ((m mod BM) + j BM) + 37 (m div BM)) mod K, BM the
         instance's row tile: gcd(11, K) = 1 for every K used, so over the launches j = 0 .. ceil(K / BM) - 1 the rows of EVERY
         row tile choose every k of 0 .. K - 1 (the arguments (m mod BM) + j BM run over 0 .. J BM - 1 >= K - 1 and x -> 11 x is a
         bijection mod K); neighbouring row tiles are shifted by 37.  The mirror image (side "a") has W one-hot per column,
         sigma_j(n) built the same way on the column tile BN, and A coded: out[m, n] = A[m, sigma(n)].
         code(r, k) = 19 (r mod 23) + (k mod 19) - 218, |code| <= 218: exact in bf16 (<= 255) and fp16; for e4m3
         code8(r, k) = 5 (r mod 3) + (k mod 5) - 7, |code8| <= 7.  Injectivity rule: two positions carry the same code only if
         their row / column indices differ by a multiple of 23 (3) AND their k by a multiple of 19 (5).  The index errors a tiled
         kernel can make are shifts by its structure sizes c 2^i, c in {1, 3, 5} (lanes, 16-element groups, K-steps of 32 / 64 / 128,
         ring slots, tiles of 128 / 160 / 256 / 320, the nine taps times Cin, 4096 tokens): none is a multiple of 23 or 19
         (structure_shifts; for fp8 c = 1 only, and none is a multiple of 3 or 5), so no single such shift in n or k, nor one in
         each, maps a position onto one with the same code.
         Coded bias and residual: bias[n] = (n - N / 2) / 8 and res[r, n] = r / 2 -- every column and every row of a res_mod
         period its own dyadic value; code + bias + res is a multiple of 1 / 8 below 2^14: exact in fp32.
  exact  dense integers, |a|, |w| <= 3, integer bias and residual.  |sum| <= 9 K <= 46080 at the family's longest K = 5120; with
         |bias| <= 2000 and |res| <= 16000 (or |bias| <= 19000 where there is no residual) every partial and final sum is an
         integer below 65504 < 2^24: exact in fp32 IN ANY ORDER, so the float64 answer is the answer bit for bit, its 16-bit
         rounding is one defined value (round16: torch's round-to-nearest-even, fp16 clamped to +-65504 as DESIGN.md section 3
         says), and the split stream's planes are hi = round16(v), lo = fp16(v - hi).  Integers above 2^11 (fp16) / 2^8 (bf16)
         are full of exact ties; tie_census counts those that round up, those that round down, and the values one off a tie.
         ReLU is exact too.  Variant `saturate`: bias +-80000 on the columns n mod 37 == 5; there |v| >= 80000 - 2000 - 9 K >
         65520 for K <= 320, so exactly those columns come out as +-65504 in fp16 and everything else stays exact.
         fp8: the same integers are exact in e4m3; wscale[n] = 2^((n mod 3) - 1), so acc wscale + bias + res is an integer or a
         half-integer below 2^24; the e4m3 output form takes |bias| <= 100 so that most values lie below 448 (ties of e4m3) and
         some beyond (saturation).  The conv's coded activation skips the code 0, the zero page's value.
  gelu   the one inexact epilogue.  One non-zero k per row: x[m, n] = factor[m] g, both with at most 8 significant bits (exact in
         bf16 and fp16), so x is exact in fp32.  g runs over 301 points: [-9, 9] in steps of 1 / 16 and the special values 0,
         +-1 / 32, +-4.5 and +-4.53125 (either side of the clamp point 3.2 sqrt 2 = 4.5255 of gelu_erf_fast4), -9, -8, -7, -6, -5.5
         (the tail: the true value is below fp16's smallest subnormal from x = -5.6 on).  The points are laid over
         ceil(301 / N) depth slots and each row reads one slot, so the sweep is the same at every M and N the tests use
         (make_gelu; GELU_SHAPES lists them and gelu_sweep_ok states the conditions, asserted per launch): the factor 1 gives the
         whole of [-9, 9] with no gap above 1 / 16, 255 / 256 an x 0.012 under the clamp point, 1 / 64 the neighbourhood of 0,
         the other 253 factors j / 256 fill in between.
         Bar per element: |got - gelu64(x)| <= 2e-5 for the fp32 output (the project's own stated accuracy of the fast form,
         test_gelu_fast_accuracy), plus half a unit in the last place of the output type at the reference value for 16-bit outputs
         (ulp16: 2^(e - p + 1), p = 11 / 8 significant bits, floored at fp16's subnormal spacing 2^-24).  Never NaN, and for x < 0
         never above +bar.
  sums   Gaussian operands as test_gpu_ops.py draws them (a ~ N(0, 1), w ~ N(0, 1) / sqrt(K)), rounded to the operand type; rows
         m mod 4 == 1 scaled by exp(1.5 N(0, 1)) (the test_gemm32_split_form recipe); heavy cancellation on the rows m mod 8 == 3
         x columns n mod 8 == 5: a[m, 2 j + 1] = a[m, 2 j], w[n, 2 j + 1] = -w[n, 2 j], then w[n, 1] moved by one part in 64, so
         sum a w is ~ 1e-3 of sum |a w|.
         rho[m, n] = |got - ref64| / (u32 S),  S = sum_k |a_k w_k| + |bias| + |res|,  u32 = 2^-24.
         HARD BOUND.  16-bit operands: every product a_k w_k is exact in fp32 (8 + 8 or 11 + 11 <= 24 bits).  A sum of t terms in
         fp32, in any order and any tree, has |fl(sum) - sum| <= gamma_(t-1) sum |terms|, gamma_j = j u / (1 - j u) (Higham, Accuracy
         and Stability, section 4.2).  K products + bias + residual: K + 1 additions at most, and gamma_(K+1) / u = (K + 1) / (1 - (K + 1) u)
         <= K + 3 for K <= 5120 ((K + 1)^2 u = 1.56 <= 2 (1 - (K + 1) u)): rho <= K + 3.  fp32 operands on the fp32 MFMA: a
         product may be rounded once more: rho <= K + 4.  Split fp32 form (gemm32.h
         gemm32x3_kernel): x = hi + 2^-11 lo to 2^-22 |x| + 2^-36 (include/wm_hip.h), three products hi hi + hi lo + lo hi, the
         lo lo term (<= 2^-22 |a w|) dropped: per product a relative 3 x 2^-22 = 12 u32 plus the absolute term, and 3 K + 2
         additions: rho <= 3 K + 16, with S extended by 2^-12 sum_k (|a_k| + |w_k|) for the absolute term (2^-36 per operand
         value is u32 2^-12; split_abs_term).
         MEASURED BAR.  The worst rho of the kernel is at most BAR_FACTOR (4) x the worst rho of the same product evaluated in
         float32 by torch on the CPU on the same operands (two draws from one error distribution, a worst of 10^7 elements
         compared; the mha32 precedent of profiles/attention_queries/README.md), per element floored at one fp32 ulp of the
         reference.  16-bit outputs: plus half an ulp16 at the reference value (rho then counts the excess over it).  The
         kernel's figure never enters its own bar.
         WHICH float32 evaluation (cpu_product32).  "One distribution" holds only between sums of the same SHAPE.  Every kernel
         of the family keeps ONE fp32 accumulator per output element and adds the matrix instruction's partial product to it,
         K / d links in a row (d = 32 for the 16-bit MFMAs, 2 for v_mfma_f32_32x32x2_f32, 16 for the split form): the error of
         such a chain grows like sqrt(K / d) u |partial sum|.  One torch.matmul on the CPU is a BLAS product that spreads a dot
         product over the lanes and unrolled accumulators of its micro-kernel and over its K blocks: chains tens of times shorter,
         and an error systematically smaller, not another draw (the first GPU run, against the one-matmul product: gemm32_kernel
         at K = 2048, 1024 links, rho 5.1 against 4 x 0.80; the 160-link 16-bit chains at K = 5120 rho 2.3 against 4 x 0.65,
         inside by 10 %; every kernel far inside the hard bound).  So the product is evaluated in float32 by torch on the CPU IN
         THAT ORDER: acc += A[:, k : k + d] W[:, k : k + d]^T for ascending k (CHAIN[form]); the one-matmul figure is printed
         beside it.  The kernel's own output enters neither.
         GROUP FIGURES.  sqrt(sum err^2) / (u32 sqrt(sum S^2)) per row, per column, per output tile of the instance and over the
         whole tensor, each the worst, printed beside 4 x the chained CPU product's same figure (floored likewise); the tile
         figure names a workgroup.  Reported, not asserted: the two conditions above are per element.

EMULATION (emulate).  A tiled GEMM in plain torch with the family's documented structure: BM x BN output tiles walked in rounds of
`slots` workgroups, K-steps of BK with an fp32 accumulator, gemm_common.h's epilogue order, the residual row m mod res_mod, the
fast GELU of wm_common.h restated, round-to-nearest-even outputs (fp16 clamped), the stream planes, and a 16-bit output that is
written in LDS-image order and read back by the definition in include/wm_hip.h (pack16_image / unpack16_image: an identity unless
the writer's order is wrong, which is mutant pack_swizzle).  MUTANTS names the switches; test_gemm_cases.py shows for each
the first case that sees it and whether the old criterion (one relative L2 on Gaussian operands at test_gpu_ops.py's tolerances)
does.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
SIG = {"fp16": 11, "bf16": 8}                    # significant bits
U32 = 2.0 ** -24
BAR_FACTOR = 4.0
GELU_BAR = 2e-5
MOD_R, MOD_K = 23, 19
OLD_TOL = {"fp32": 1e-5, "fp32_act": 2e-5, "fp16": 7e-4, "bf16": 5e-3}        # test_gpu_ops.py (fp32 behind an activation: 2e-5)
GELU_X = 4.525483399593905


# ---------------------------------------------------------------------------------------------------------------------------------
# codes and probes
# ---------------------------------------------------------------------------------------------------------------------------------
def code(r, k, fp8=False, nonzero=False):
    """Integer code of position (row r, depth k); see the docstring for the injectivity rule.  nonzero: the codes >= 0 moved up by
    one, so that none equals the conv's zero page (|code| <= 219)."""
    if fp8:
        return (5 * (r % 3) + (k % 5) - 7).float()
    c = MOD_K * (r % MOD_R) + (k % MOD_K) - 218
    return (c + (c >= 0) if nonzero else c).float()


def structure_shifts(limit, fp8=False):
    """The index shifts a tiled kernel can make: c 2^i with c in {1, 3, 5} (fp8: c = 1), up to `limit`."""
    out = set()
    for c in ((1,) if fp8 else (1, 3, 5)):
        i = 0
        while c << i <= limit:
            out.add(c << i)
            i += 1
    return sorted(out)


def probe_launches(K, tile):
    return -(-K // tile)


def probe_pi(rows, K, tile, j=0):
    """Row (or column) index -> its one hot k in launch j."""
    assert math.gcd(11, K) == 1
    r = torch.arange(rows)
    return (11 * ((r % tile) + j * tile) + 37 * (r // tile)) % K


def _coded_bias_res(c, bias, res_rows):
    if bias:
        c.bias = (torch.arange(c.N, dtype=torch.float32) - c.N // 2) / 8
    if res_rows:
        c.res = (torch.arange(res_rows, dtype=torch.float32) / 2)[:, None].expand(res_rows, c.N).contiguous()
        c.res_mod = res_rows


def _case(kind, prec, M, N, K, tile, **kw):
    c = SimpleNamespace(kind=kind, prec=prec, M=M, N=N, K=K, tile=tile, form="plain", a=None, w=None, bias=None, res=None, res_mod=0,
                        act=0, wscale=None, x=None, Cin=0, B=0, sat_cols=None, side=None, j=0)
    c.__dict__.update(kw)
    return c


def make_probe(M, N, K, prec, tile, side="w", j=0, bias=False, res_rows=0):
    """side "w": A one-hot per row, W coded; side "a": W one-hot per column, A coded."""
    c = _case("probe", prec, M, N, K, tile, side=side, j=j)
    fp8 = prec == "fp8"
    kk = torch.arange(K)
    if side == "w":
        c.pi = probe_pi(M, K, tile[0], j)
        c.a = torch.zeros(M, K)
        c.a[torch.arange(M), c.pi] = 1.0
        c.w = code(torch.arange(N)[:, None], kk[None, :], fp8)
    else:
        c.pi = probe_pi(N, K, tile[1], j)
        c.w = torch.zeros(N, K)
        c.w[torch.arange(N), c.pi] = 1.0
        c.a = code(torch.arange(M)[:, None], kk[None, :], fp8)
    if fp8:
        c.wscale = torch.ones(N)
    _coded_bias_res(c, bias, res_rows)
    return c


def probe_answer(c):
    """The product of a probe case as a gather (no bias / residual)."""
    if c.form == "plain":
        return (c.w[:, c.pi].t() if c.side == "w" else c.a[:, c.pi]).double()
    assert c.side == "a"                     # implicit forms: W one-hot, the answer is the gathered operand's column sigma(n)
    return logical_a(c)[:, c.pi].double()


# ---------------------------------------------------------------------------------------------------------------------------------
# implicit-GEMM forms: the gathers restated
# ---------------------------------------------------------------------------------------------------------------------------------
def logical_a(c, mutant=None):
    if c.form == "plain":
        return c.a
    if c.form == "conv":
        B, Cin = c.B, c.Cin
        xf = c.x.reshape(B * 4096, Cin)
        m = torch.arange(B * 4096, device=xf.device)
        y, x = (m & 4095) >> 6, m & 63
        cols = []
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            inside = (y + dy >= 0) & (y + dy < 64) & (x + dx >= 0) & (x + dx < 64)
            if mutant == "conv_tap" and dx == -1:                # left border: the neighbouring pixel in memory, not the zero page
                inside = inside | ((x == 0) & (y + dy >= 0) & (y + dy < 64) & (m + dy * 64 + dx >= 0))
            src = (m + dy * 64 + dx).clamp(0, B * 4096 - 1)
            cols.append(torch.where(inside[:, None], xf[src], torch.zeros((), dtype=xf.dtype, device=xf.device)))
        return torch.cat(cols, 1)
    if c.form == "patch":
        B, Cin = c.B, c.Cin
        return c.x.reshape(B, Cin, 64, 16, 64, 16).permute(0, 2, 4, 1, 3, 5).reshape(B * 4096, Cin * 256)
    raise ValueError(c.form)


def make_conv(kind, B, Cin, N, prec, j=0, seed=0):
    """3 x 3 conv cases: probe (W one-hot on (tap, ci) per output channel, x coded by (pixel, ci)), probe_a (one hot channel per pixel, W
    coded: every output is a sum of up to nine codes) and exact."""
    M, K = B * 4096, 9 * Cin
    c = _case("probe" if kind.startswith("probe") else kind, prec, M, N, K, (256, 256), form="conv", B=B, Cin=Cin, j=j)
    g = torch.Generator().manual_seed(seed)
    if kind == "probe":
        c.side = "a"
        c.pi = probe_pi(N, K, 256, j)
        c.w = torch.zeros(N, K)
        c.w[torch.arange(N), c.pi] = 1.0
        c.x = code(torch.arange(M)[:, None], torch.arange(Cin)[None, :], nonzero=True).view(B, 64, 64, Cin).contiguous()
    elif kind == "probe_a":
        c.side = "w"
        c.pi = probe_pi(M, Cin, 256, j)
        c.x = torch.zeros(M, Cin)
        c.x[torch.arange(M), c.pi] = 1.0
        c.x = c.x.view(B, 64, 64, Cin)
        c.w = code(torch.arange(N)[:, None], torch.arange(K)[None, :])
    else:
        c.x = torch.randint(-3, 4, (B, 64, 64, Cin), generator=g).float()
        c.w = torch.randint(-3, 4, (N, K), generator=g).float()
    return c


def make_patch(kind, B, Cin, N, prec, j=0, seed=0, bias=True):
    M, K = B * 4096, Cin * 256
    tile = (256, 320 if N % 320 == 0 else 256)
    c = _case("probe" if kind.startswith("probe") else kind, prec, M, N, K, tile, form="patch", B=B, Cin=Cin, j=j)
    g = torch.Generator().manual_seed(seed)
    if kind == "probe":                      # W one-hot per column, the image coded by (patch, k)
        c.side = "a"
        c.pi = probe_pi(N, K, tile[1], j)
        c.w = torch.zeros(N, K)
        c.w[torch.arange(N), c.pi] = 1.0
        a = code(torch.arange(M)[:, None], torch.arange(K)[None, :])
    elif kind == "probe_a":                  # one hot (ci, ky, kx) per patch, W coded
        c.side = "w"
        c.pi = probe_pi(M, K, 256, j)
        a = torch.zeros(M, K)
        a[torch.arange(M), c.pi] = 1.0
        c.w = code(torch.arange(N)[:, None], torch.arange(K)[None, :])
    else:
        a = torch.randint(-3, 4, (M, K), generator=g).float()
        c.w = torch.randint(-3, 4, (N, K), generator=g).float()
    c.x = a.view(B, 64, 64, Cin, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(B, Cin, 1024, 1024).contiguous()    # the inverse gather
    if bias:
        c.bias = (torch.arange(N, dtype=torch.float32) - N // 2) / 8 if c.kind == "probe" else torch.randint(-2000, 2001, (N,), generator=g).float()
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# exact, gelu, sums
# ---------------------------------------------------------------------------------------------------------------------------------
def make_exact(M, N, K, prec, tile, seed=0, bias=True, res_rows=0, act=0, saturate=False, amp=None):
    """amp: the bias amplitude (default 2000 beside a residual, else 19000; the e4m3 output form takes a small one to stay below 448)."""
    c = _case("exact", prec, M, N, K, tile, act=act)
    g = torch.Generator().manual_seed(seed)
    c.a = torch.randint(-3, 4, (M, K), generator=g).float()
    c.w = torch.randint(-3, 4, (N, K), generator=g).float()
    amp = amp if amp is not None else 2000 if res_rows else 19000
    if bias:
        c.bias = torch.randint(-amp, amp + 1, (N,), generator=g).float()
    if res_rows:
        c.res = torch.randint(-16000, 16001, (res_rows, N), generator=g).float()
        c.res_mod = res_rows
    if prec == "fp8":
        c.wscale = 2.0 ** ((torch.arange(N) % 3) - 1).float()
    if saturate:
        assert bias and not res_rows and K <= 320
        c.sat_cols = torch.arange(N) % 37 == 5
        sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
        c.bias = torch.where(c.sat_cols, 80000.0 * sign + c.bias.clamp(-2000, 2000), c.bias)
    return c


def exact_bound(c):
    """The largest magnitude any partial or final sum of an exact case can reach."""
    sc = 1.0 if c.wscale is None else c.wscale.max().item()
    return 9.0 * c.K * sc + (0 if c.bias is None else c.bias.abs().max().item()) + (0 if c.res is None else c.res.abs().max().item())


GELU_SPECIAL = (0.0, 1 / 32, -1 / 32, 4.5, -4.5, 4.53125, -4.53125, -9.0, -8.0, -7.0, -6.0, -5.5)


GELU_POINTS = torch.cat([torch.arange(-144, 145, dtype=torch.float32) / 16, torch.tensor(GELU_SPECIAL)])       # 301 values of g
# row factors / 256, at most 8 significant bits: 1 first (the whole of [-9, 9]), 255 / 256 (just under the clamp point from
# 4.53125), 1 / 64 (around 0), then the rest
GELU_FACTORS = torch.tensor([256, 255, 4] + [j for j in range(254, 0, -1) if j != 4], dtype=torch.float32) / 256
# the (M, N, K) at which tests/test_gpu_gemm_elements.py launches a gelu case; tests/test_gemm_cases.py asserts the sweep on each
GELU_SHAPES = [(384, 256, 64), (384, 256, 320), (256, 512, 64), (768, 512, 448), (256, 640, 64), (768, 640, 448), (8448, 1280, 320), (8448, 1024, 320),
               (153, 70, 96)]


def make_gelu(M, N, K, prec, tile):
    """One non-zero k per row, the same sweep at any M and N: the 301 points are laid over S = ceil(301 / N) depth slots,
    w[n, k_s] = point (s N + n) mod 301, and row m reads slot m mod S alone with the factor GELU_FACTORS[(m div S) mod 256], so
    x[m, n] = factor x point.  Needs M >= 3 S (every slot with the first three factors) and S <= K."""
    c = _case("gelu", prec, M, N, K, tile, act=1)
    P = len(GELU_POINTS)
    S = -(-P // N)
    assert M >= 3 * S and S <= K and math.gcd(11, K) == 1
    slot_k = (5 + 11 * torch.arange(S)) % K                                       # the slots' depths, spread over the K-steps
    m, n = torch.arange(M), torch.arange(N)
    c.a, c.w = torch.zeros(M, K), torch.zeros(N, K)
    c.a[m, slot_k[m % S]] = GELU_FACTORS[(m // S) % len(GELU_FACTORS)]
    for s in range(S):
        c.w[:, slot_k[s]] = GELU_POINTS[(s * N + n) % P]
    return c


def gelu_sweep(c):
    """What the sweep of a gelu case covers: range, largest gap between neighbouring x, non-zero |x| < 1e-3, the distance of the
    nearest x on either side of +-GELU_X, and the elements of the tail whose true value is below fp16's subnormals."""
    x = logical_a(c).double() @ c.w.double().t()
    xs = torch.unique(x)
    d = [s * xs - GELU_X for s in (-1, 1)]
    return SimpleNamespace(lo=xs.min().item(), hi=xs.max().item(), gap=(xs[1:] - xs[:-1]).max().item(), zero=bool((xs == 0).any()),
                           near0=int(((xs != 0) & (xs.abs() < 1e-3)).sum()), clamp=max(max(t[t > 0].min().item(), (-t[t < 0]).min().item()) for t in d),
                           tail=int(((x < -5.6) & (gelu64(x).abs() < 2.0 ** -25)).sum()), one_k=int((logical_a(c) != 0).sum(1).max()))


def gelu_sweep_ok(s):
    """The conditions of the gelu case: [-9, 9] end to end, no gap above 1 / 16, 0 and at least four non-zero |x| < 1e-3, an x within 0.02
    of the clamp point on either side of both signs, at least 100 elements in the underflowing tail, one non-zero k per row."""
    return s.lo == -9 and s.hi == 9 and s.gap <= 1 / 16 and s.zero and s.near0 >= 4 and s.clamp < 0.02 and s.tail >= 100 and s.one_k == 1


def make_sums(M, N, K, prec, tile, seed=0, bias=False, res_rows=0, wsize=None):
    c = _case("sums", prec, M, N, K, tile)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * (wsize if wsize else 1 / math.sqrt(K))
    a[1::4] *= torch.exp(torch.randn(a[1::4].shape[0], 1, generator=g) * 1.5)
    a[3::8, 1::2] = a[3::8, 0::2]
    w[5::8, 1::2] = -w[5::8, 0::2] * (1 + 2.0 ** -6)
    if prec in DT:
        a, w = a.to(DT[prec]).float(), w.to(DT[prec]).float()
    c.a, c.w = a, w
    if bias:
        c.bias = torch.randn(N, generator=g)
    if res_rows:
        c.res, c.res_mod = torch.randn(res_rows, N, generator=g), res_rows
    return c


def case_to(c, device):
    d = SimpleNamespace(**vars(c))
    for k, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(d, k, v.to(device))
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle and expected outputs
# ---------------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def activate(y, act):
    if act == 1:
        return gelu64(y) if y.dtype == torch.float64 else (0.5 * y * (1 + torch.erf(y * 0.70710678118654752440)))
    if act == 2:
        return torch.relu(y)
    if act == 3:
        return torch.sigmoid(y)
    return y


def res_rows_of(c, dtype=torch.float64):
    """The residual as it is added: [M, N], row m from res[m % res_mod]."""
    R = c.res_mod if c.res_mod > 0 else c.M
    return c.res.to(dtype)[torch.arange(c.M, device=c.res.device) % R]


def ref64(c, want_s=False):
    """float64 answer; with want_s also S = sum_k |a_k w_k| (* wscale) + |bias| + |res|."""
    a, w = logical_a(c).double(), c.w.double()
    y = a @ w.t()
    s = a.abs() @ w.abs().t() if want_s else None
    if c.wscale is not None:
        y = y * c.wscale.double()
        s = s * c.wscale.double() if want_s else None
    if c.bias is not None:
        y = y + c.bias.double()
        s = s + c.bias.double().abs() if want_s else None
    y = activate(y, c.act)
    if c.res is not None:
        r = res_rows_of(c)
        y = y + r
        s = s + r.abs() if want_s else None
    return (y, s) if want_s else y


def is_exact32(y64):
    """Every value of y64 is an fp32 number (so fp32 arithmetic that is exact at every step must return it)."""
    return bool((y64.float().double() == y64).all())


def round16(v, prec, mode="rne"):
    """v (values that are fp32 numbers) -> the 16-bit type; mode rne (torch's, with the kernels' fp16 clamp) / trunc / away / via_fp16."""
    x = v.float()
    if prec == "fp16" or mode == "via_fp16":
        x = x.clamp(-65504.0, 65504.0)
    if mode == "via_fp16":
        return x.to(torch.float16).to(DT[prec])
    r = x.to(DT[prec])
    if mode == "rne":
        return r
    t, up = _neighbours(x, r, torch.int16)
    if mode == "trunc":
        return t
    tie = ((x - t.float()).abs() == (up.float() - x).abs()) & (t.float() != x)
    return torch.where(tie, up, r)


def _neighbours(x, r, itype):
    """(the value of r's type next to x toward zero or x itself, the next one away from zero)."""
    bits = r.view(itype)
    t = torch.where(r.float().abs() > x.abs(), (bits - 1).view(r.dtype), r)
    return t, (t.view(itype) + 1).view(r.dtype)


def round8(v):
    return v.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def planes(v32, prec):
    hi = round16(v32, prec)
    return hi, (v32.float() - hi.float()).to(torch.float16)


def tie_census(y64, prec):
    """{ties_up, ties_down, near}: exact ties of the output type that round-to-nearest-even sends away from / toward zero, and values
    one integer step off a tie."""
    x = y64.float()
    if prec == "fp8":
        x = x[x.abs() < 448]
        r, itype = x.to(torch.float8_e4m3fn), torch.int8
    else:
        x = x[x.abs() < 65504]
        r, itype = x.to(DT[prec]), torch.int16
    t, up = _neighbours(x, r, itype)
    lo, hi = (x - t.float()).abs(), (up.float() - x).abs()
    inexact = t.float() != x
    tie = inexact & (lo == hi)
    near = inexact & ((lo - hi).abs() == 2)
    return {"ties_up": int((tie & (r.float() == up.float())).sum()), "ties_down": int((tie & (r.float() == t.float())).sum()), "near": int(near.sum())}


def ulp16(y64, prec):
    """Unit in the last place of the 16-bit type at |y| (fp16: floored at its subnormal spacing 2^-24; bf16: at 2^-133)."""
    e = torch.floor(torch.log2(y64.abs().clamp_min(1e-300)))
    emin = -14.0 if prec == "fp16" else -126.0
    return torch.exp2(e.clamp_min(emin) - (SIG[prec] - 1))


def ulp32(y64):
    e = torch.floor(torch.log2(y64.abs().clamp_min(1e-300)))
    return torch.exp2(e.clamp_min(-126.0) - 23)


def out_prec(c):
    """The 16-bit output type: the operand type, or for fp8 operands the case's prec16."""
    return getattr(c, "prec16", None) or c.prec


def expected(c, y64, outs):
    """{output name: tensor} for the exact kinds.  outs: any of f32, o16, hi, lo, o8."""
    want = {}
    if "f32" in outs:
        want["f32"] = y64.float()
    if "o16" in outs:
        want["o16"] = round16(y64, out_prec(c))
    if "hi" in outs or "lo" in outs:
        want["hi"], want["lo"] = planes(y64.float(), out_prec(c))
        want = {k: v for k, v in want.items() if k in outs}
    if "o8" in outs:
        want["o8"] = round8(y64)
    return want


def mismatches(got, want):
    """(count, first (m, n) or None): value equality (a signed zero equals zero; a NaN equals nothing)."""
    g, w = (got.float() if got.dtype != torch.float32 else got), (want.float() if want.dtype != torch.float32 else want)
    bad = ~(g == w)
    n = int(bad.sum())
    if not n:
        return 0, None
    i = int(bad.flatten().nonzero()[0])
    return n, (i // got.shape[1], i % got.shape[1])


def describe(c, got, want, where):
    m, n = where
    bm, bn = c.tile
    return (f"first at row {m} col {n} (tile {m // bm}, {n // bn}; row in tile {m % bm}, col in tile {n % bn}): got {got[m, n].float().item()!r} "
            f"want {want[m, n].float().item()!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# gelu and sums: figures beside bars
# ---------------------------------------------------------------------------------------------------------------------------------
def gelu_figures(c, got, y64, out16=None):
    """(worst |err| / bar, worst |err|, its bar, x there, count of NaN, worst positive value for x < 0 over its bar)."""
    pre = logical_a(c).double() @ c.w.double().t()
    bar = torch.full_like(y64, GELU_BAR)
    if out16:
        bar = bar + 0.5 * ulp16(y64, out16)
    g = got.double()
    err = (g - y64).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bar)
    i = int(ratio.argmax())
    neg = pre < 0
    pos_over = torch.where(neg, g - bar, torch.full_like(g, -1.0)).max().item()
    return SimpleNamespace(ratio=ratio.flatten()[i].item(), err=err.flatten()[i].item(), bar=bar.flatten()[i].item(), x=pre.flatten()[i].item(),
                           nans=int(torch.isnan(g).sum()), pos_over=pos_over)


def hard_bound(c, form="mfma16"):
    """rho's hard bound (docstring, HARD BOUND)."""
    return {"mfma16": c.K + 3, "mfma32": c.K + 4, "split": 3 * c.K + 16}[form]


def split_abs_term(c):
    """The split fp32 form's absolute representation error 2^-36 per operand value, as an addition to S (in units where u32 S is an
    error): sum_k (|a_k| + |w_k|) 2^-36 / u32."""
    a, w = logical_a(c).double().abs().sum(1), c.w.double().abs().sum(1)
    return (a[:, None] + w[None, :]) * 2.0 ** -12


def _groups(x2, tile):
    """{row, col, tile, whole: the sums of x2 over each group}; the tile sums as a [row tiles, column tiles] matrix."""
    M, N = x2.shape
    bm, bn = tile
    tm, tn = -(-M // bm), -(-N // bn)
    t = torch.nn.functional.pad(x2, (0, tn * bn - N, 0, tm * bm - M)).view(tm, bm, tn, bn).sum((1, 3))
    return {"row": x2.sum(1), "col": x2.sum(0), "tile": t, "whole": x2.sum().view(1)}


CHAIN = {"mfma16": 32, "mfma32": 2, "split": 16}        # the depth of one matrix instruction: the link of the kernels' accumulation chain


def cpu_product32(c, chain=0):
    """The case's operation evaluated in float32 by torch (on the case's device: the CPU for a CPU case).  chain = 0: one matmul, in
    the BLAS's own blocked order; chain = d: the documented order of the kernels, ONE accumulator per output element to which the
    partial products of d consecutive k are added, K / d links long."""
    a, w = logical_a(c).float(), c.w.float()
    if chain:
        y = torch.zeros(a.shape[0], w.shape[0], device=a.device)
        for k in range(0, c.K, chain):
            y += a[:, k:k + chain] @ w[:, k:k + chain].t()
    else:
        y = a @ w.t()
    if c.wscale is not None:
        y = y * c.wscale
    if c.bias is not None:
        y = y + c.bias
    y = activate(y, c.act)
    if c.res is not None:
        y = y + res_rows_of(c, torch.float32)
    return y


def sums_figures(c, got, y64, s, cpu32, out16=None, form="mfma16", cpu_blas=None):
    """The kernel's figures beside their bars; cpu32 = cpu_product32 in the kernels' chain order, cpu_blas = the same as one matmul (shown
    only), both moved to y64's device.  Returns a namespace with .lines (printable), .over (what is over a bar) and the numbers.  The
    element conditions are asserted by the caller; the group figures are reported beside 4 x the chained product's."""
    half = 0.5 * ulp16(y64, out16) if out16 else torch.zeros_like(y64)
    floor = ulp32(y64)
    err = ((got.double() - y64).abs() - half).clamp_min(0)
    err_cpu = (cpu32.double() - y64).abs()
    rho, rho_cpu = err / (U32 * s), err_cpu / (U32 * s)
    worst, worst_cpu = rho.max().item(), rho_cpu.max().item()
    i = int(rho.argmax())
    over_el = err > torch.maximum(BAR_FACTOR * worst_cpu * U32 * s, floor)
    hard = hard_bound(c, form)
    res = SimpleNamespace(worst=worst, worst_cpu=worst_cpu, hard=hard, n_over=int(over_el.sum()), at=(i // y64.shape[1], i % y64.shape[1]), over=[], lines=[])
    blas = "" if cpu_blas is None else f"; as one matmul {((cpu_blas.double() - y64).abs() / (U32 * s)).max().item():.3f}"
    res.lines.append(f"element rho {worst:9.3f} at {res.at}  | hard bound {hard}  | bar {BAR_FACTOR:g} x cpu-fp32 {worst_cpu:.3f} = {BAR_FACTOR * worst_cpu:.3f}"
                     f"  (x{worst / max(BAR_FACTOR * worst_cpu, 1e-30):.2f}; {res.n_over} elements over bar-or-floor{blas})")
    if not worst <= hard:
        res.over.append(("hard", worst, hard))
    if res.n_over:
        res.over.append(("element", worst, BAR_FACTOR * worst_cpu))
    ge, gc, gs, gf = (_groups(t * t, c.tile) for t in (err, err_cpu, s, floor))
    for name in ("row", "col", "tile", "whole"):
        fig, fig_cpu, fl = ((g[name] / gs[name]).sqrt() / U32 for g in (ge, gc, gf))
        bar = torch.maximum(BAR_FACTOR * fig_cpu.max(), fl)     # the CPU product's worst group; a group's floor is its elements' one-ulp floors in quadrature
        ratio = fig / bar
        j = int(ratio.argmax())
        at = (j // fig.shape[1], j % fig.shape[1]) if fig.dim() == 2 else j
        res.lines.append(f"  worst {name:5s} {fig.flatten()[j].item():9.4f} at {at}  | bar {bar.flatten()[j].item():.4f} (cpu-fp32 worst {fig_cpu.max().item():.4f})"
                         f"  x{ratio.flatten()[j].item():.2f}")
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# LDS-image order (include/wm_hip.h): position l of a 16 x 32 block holds row l >> 2, 16-byte chunk (l & 3) ^ ((-(l >> 4)) & 3)
# ---------------------------------------------------------------------------------------------------------------------------------
def _image_index(wrong_swizzle=False):
    l = torch.arange(64)
    return l >> 2, (l & 3) ^ (((l >> 4) if wrong_swizzle else (-(l >> 4))) & 3)


def pack16_image(t, wrong_swizzle=False):
    rows, K = t.shape
    row, ch = _image_index(wrong_swizzle)
    return t.view(rows // 16, 16, K // 32, 4, 8)[:, row, :, ch, :].permute(1, 2, 0, 3).contiguous().view(rows, K)


def unpack16_image(p):
    rows, K = p.shape
    row, ch = _image_index()
    out = torch.empty_like(p).view(rows // 16, 16, K // 32, 4, 8)
    out[:, row, :, ch, :] = p.view(rows // 16, K // 32, 64, 8).permute(2, 0, 1, 3)
    return out.view(rows, K)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tiled emulation and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "trunc16": "output truncated instead of rounded to nearest even",
    "half_away": "output ties rounded away from zero",
    "double_round": "a bf16 output rounded through fp16 first",
    "lo_unrounded": "lo = fp16(v - trunc16(v)) beside hi = round16(v)",
    "kswap_a": "k positions 3 and 17 of every K-step swapped for A only",
    "drop_last_k": "the last K-step dropped for output tile (1, 0)",
    "store_shift": "one 16-element store of one lane lands one row lower",
    "res_m": "the residual read at row m instead of m % res_mod",
    "bias_n1": "the bias of column n + 1",
    "conv_tap": "conv: the left border's dx = -1 taps read the neighbouring pixel, not the zero page",
    "round2_at_1": "the tiles of the second round written at the first round's place",
    "gelu_tanh": "the tanh form of GELU",
    "gelu_clamp": "the GELU tail clamp at 3.2 instead of 3.2 sqrt 2",
    "pack_swizzle": "the packed 16-bit output written with the chunk swizzle (l >> 4) & 3 instead of (-(l >> 4)) & 3",
}
_P = (0.7978911995887756, 0.05407121405005455, 0.007685498800128698, 6.773129280190915e-05)
_Q = (0.2344742864370346, 0.02365594170987606, 0.0011780407512560487)


def gelu_fast32(x, clamp=GELU_X):
    """wm_common.h gelu_erf_fast restated in fp32 torch: erf(x / sqrt 2) as a clamped rational."""
    x = x.float()
    xc = x.clamp(-clamp, clamp)
    t = xc * xc
    p = ((_P[3] * t + _P[2]) * t + _P[1]) * t + _P[0]
    q = ((_Q[2] * t + _Q[1]) * t + _Q[0]) * t + 1.0
    hx = 0.5 * x
    return hx * ((xc * p) / q) + hx


def emulate(c, outs, mutant=None, bk=32, slots=4):
    """{output name: tensor} of the tiled emulation; outs as expected().  Tiles are numbered row-major and walked in rounds of `slots`."""
    bm, bn = c.tile
    a, w = logical_a(c, mutant).float(), c.w.float()
    M, N, K = c.M, c.N, c.K
    if mutant == "kswap_a":
        a = a.clone().view(M, K // bk, bk)
        a[:, :, [3, 17]] = a[:, :, [17, 3]]
        a = a.view(M, K)
    acc = torch.zeros(M, N)
    for s in range(K // bk):
        part = a[:, s * bk:(s + 1) * bk] @ w[:, s * bk:(s + 1) * bk].t()
        if mutant == "drop_last_k" and s == K // bk - 1:
            part[bm:2 * bm, :bn] = 0
        acc = acc + part
    v = acc
    if c.wscale is not None:
        v = v * c.wscale
    if c.bias is not None:
        v = v + (torch.roll(c.bias, -1) if mutant == "bias_n1" else c.bias)
    if c.act == 1:
        if mutant == "gelu_tanh":
            v = 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
        else:
            v = gelu_fast32(v, 3.2 if mutant == "gelu_clamp" else GELU_X)
    elif c.act:
        v = activate(v, c.act)
    if c.res is not None:
        if mutant == "res_m":                                   # rows past the buffer: whatever follows it, here zeros
            R = c.res.shape[0]
            m = torch.arange(M)
            v = v + torch.where((m < R)[:, None], c.res[m.clamp_max(R - 1)], torch.zeros(()))
        else:
            v = v + res_rows_of(c, torch.float32)
    if mutant == "store_shift":
        v = v.clone()
        r0, n0 = bm + 37, 48
        v[r0 + 1, n0:n0 + 16] = v[r0, n0:n0 + 16]
    if mutant == "round2_at_1":
        tn = N // bn
        tiles = [(i // tn, i % tn) for i in range((M // bm) * tn)]
        out = torch.zeros_like(v)
        for i, (tm_, tn_) in enumerate(tiles):
            dm, dn = tiles[i - slots] if slots <= i < 2 * slots else (tm_, tn_)
            out[dm * bm:(dm + 1) * bm, dn * bn:(dn + 1) * bn] = v[tm_ * bm:(tm_ + 1) * bm, tn_ * bn:(tn_ + 1) * bn]
        v = out
    prec = out_prec(c)
    got = {}
    if "f32" in outs:
        got["f32"] = v
    if "o16" in outs:
        mode = {"trunc16": "trunc", "half_away": "away", "double_round": "via_fp16"}.get(mutant, "rne")
        # written in LDS-image order as the kernel's packed output is, read back by the definition as the GPU test reads it
        got["o16"] = unpack16_image(pack16_image(round16(v, prec, mode), wrong_swizzle=mutant == "pack_swizzle"))
    if "hi" in outs:
        got["hi"] = round16(v, prec)
    if "lo" in outs:
        base = round16(v, prec, "trunc") if mutant == "lo_unrounded" else round16(v, prec)
        got["lo"] = (v - base.float()).to(torch.float16)
    return got
