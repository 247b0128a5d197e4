"""The LayerNorm family's row cases: what tests/test_gpu_layernorm_rows.py and tests/test_layernorm_cases.py share.  Plain module
(torch only, any device): the row families, the float64 oracle, the emulations and the bar rules.  Follows encoder_cases.py.

ROW FAMILIES (rows()).  Rows of one family come in blocks of `block` rows (16: the row tile of the LDS-image order), the blocks
interleaved in the fixed cycle CYCLE, so every 256-row GEMM tile and every four-row LayerNorm workgroup at a block boundary holds
rows whose mean and rstd differ by orders of magnitude.  CYCLE has 16 slots for 17 families: `const` and `zero`, the two exact
rows, share one slot (first half const, rest zero), so that 16 blocks of 16 rows -- one GEMM tile -- hold every family.
bn = fold_bn(C), ntile = C / bn, z = randn:

  base                       z
  offset1 .. offset1000      z + r
  flat1e-1 .. flat1e-5       3 + s z
  const / zero               exactly 3.0 / exactly 0
  spike1e3, spike3e4         z with one channel set to the value, in turn at the first and the last column of each statistics tile
  spikes2                    z with +1e3 in tile 0 and -1e3 in the last tile
  tilestep                   tile t of z shifted by (-50, 0, 50, 200)[t]: the between-tile term of ln_combine dominates
  tiny1e-4, tiny1e-7         s z: the variance near and far below eps, the lo plane in fp16's subnormals
  outlier                    outlier_rows(): unit bulk, a row offset of 0.2 sigma, two massive channels

Every value stays below 65504.

ORACLE.  ln64(): float64 LayerNorm of the fp32 rows, biased variance.  gemm64(): that LayerNorm times the 16-bit weight plus the
bias, exact-erf GELU where asked.

EMULATIONS.  classic(): float64 LayerNorm, rounded to 16 bits, GEMM, output rounded.  folded(): wm_common.h / gemm16_v5.h restated
in float64 -- per-tile (mean, M2) of the fp32 rows combined as ln_combine does, x16 = round16(x), wf = round16(gamma (.) W16) with
the product in fp32 as fold_weight_kernel forms it, c1 = sum wf, c2 = beta . W16 + bias, rstd (x16 wf^T - mean c1) + c2, GELU,
output rounded -- with a `mutant` switch (MUTANTS) for tests/test_layernorm_cases.py.  ln32() / tile_stats32(): the two-pass
LayerNorm and the tiled statistics with every operation in float32.

ERRORS are per row: the L2 norm of (got - ref) over the row, over the row's reference norm; a row whose reference norm is zero is
measured against the largest reference norm of its family (row_err()).  Statistics: absolute error per row and tile.

BARS are computed in the same run from the oracle and the emulations alone, per row, and reported per family:

  16-bit LayerNorm output      BAR_FACTOR (2) x the error of round16(ln64) on that row.
  classic route                2 x the error of classic() on that row.
  folded GEMM                  2 x the error of folded() on that row + rstd sqrt(K) 2^-24 || |x16| |wf|^T ||_row / || ref ||_row.
      The second term: an fp32 dot product of K terms carries, by the usual probabilistic bound, an error of about sqrt(K) u
      sum |x_k w_k| with u = 2^-24 per column; over the row's N columns that is sqrt(K) u || |x16| |wf|^T ||, and the epilogue
      multiplies it by rstd.  folded() accumulates in float64 and has none of it, and on const, flat1e-3 and flat1e-5 rows (where
      x16 wf^T - mean c1 cancels to nothing and rstd is 700 .. 1000) that noise is the kernel's whole error.
  fp32 LayerNorm output,       FP32_BAR_FACTOR (4) x the error of ln32() / tile_stats32() against float64, the margin for another
  tiled (mean, M2)             summation order (the factor encoder_cases.py gives the FFT), floored at one fp32 ulp of the row's
      largest |x| for the mean, at that squared times C for M2, and for the output at the mean's floor carried through the
      LayerNorm: ulp rstd || gamma || / || ref ||_row.  The emulation's error is taken as the WORST OVER THE ROW'S FAMILY in the
      run, not the row's own: an fp32 rounding error of one row is a single draw around zero, the ratio of two such draws (the
      kernel's and the emulation's, different summation orders) has a Cauchy tail -- P(ratio > 4) is 15 % -- and the emulation's
      draw is exactly zero on some rows, so a bar from the row's own draw refuses a correct kernel; the family's worst is the
      stable scale of the same quantity.  Each row is still held to its own family's bar: families differ by orders of magnitude.
"""
from __future__ import annotations

import math

import torch

DT16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
BAR_FACTOR, FP32_BAR_FACTOR = 2.0, 4.0
BLOCK = 16
TILESTEP = (-50.0, 0.0, 50.0, 200.0)

FAMILIES = ("base", "offset1", "offset10", "offset100", "offset1000", "flat1e-1", "flat1e-3", "flat1e-5", "const", "zero",
            "spike1e3", "spike3e4", "spikes2", "tilestep", "tiny1e-4", "tiny1e-7", "outlier")
FID = {f: i for i, f in enumerate(FAMILIES)}
# the interleave: 16 slots; families far apart in mean / rstd are neighbours
CYCLE = ("base", "offset1000", "flat1e-5", "spike3e4", "tiny1e-7", "offset100", "const|zero", "tilestep", "flat1e-3", "offset1",
         "spikes2", "tiny1e-4", "offset10", "flat1e-1", "spike1e3", "outlier")
_PARAM = {"offset1": 1.0, "offset10": 10.0, "offset100": 100.0, "offset1000": 1000.0, "flat1e-1": 1e-1, "flat1e-3": 1e-3,
          "flat1e-5": 1e-5, "spike1e3": 1e3, "spike3e4": 3e4, "tiny1e-4": 1e-4, "tiny1e-7": 1e-7}


def fold_bn(C: int) -> int:
    return 320 if C % 320 == 0 else 256


def outlier_rows(M, C, dev, generator=None):
    """Residual-stream-like rows: unit bulk, a per-row offset, two massive channels (~200x) as the outlier weight profile makes."""
    x = torch.randn(M, C, device=dev, generator=generator) * (0.7 + torch.rand(M, 1, device=dev, generator=generator)) \
        + 0.2 * torch.randn(M, 1, device=dev, generator=generator)
    x[:, 101] += 190.0
    x[:, 678 % C] -= 240.0
    return x


def family_ids(n_rows: int, block: int = BLOCK) -> torch.Tensor:
    fam = torch.empty(n_rows, dtype=torch.long)
    for r in range(n_rows):
        slot = CYCLE[(r // block) % len(CYCLE)]
        if slot == "const|zero":
            slot = "const" if r % block < (block + 1) // 2 else "zero"
        fam[r] = FID[slot]
    return fam


def rows(C: int, n_rows: int, seed: int = 0, block: int = BLOCK):
    """(x [n_rows, C] fp32 on the CPU, family id per row [n_rows]); the same for the same arguments."""
    g = torch.Generator().manual_seed(seed)
    bn = fold_bn(C)
    ntile = C // bn
    fam = family_ids(n_rows, block)
    z = torch.randn(n_rows, C, generator=g)
    out = outlier_rows(n_rows, C, "cpu", g)
    x = torch.empty(n_rows, C)
    for name in FAMILIES:
        idx = torch.nonzero(fam == FID[name]).flatten()
        if idx.numel() == 0:
            continue
        zz = z[idx]
        j = torch.arange(idx.numel())                      # the row's number inside its family
        if name == "base":
            v = zz
        elif name.startswith("offset"):
            v = zz + _PARAM[name]
        elif name.startswith("flat"):
            v = 3.0 + _PARAM[name] * zz
        elif name == "const":
            v = torch.full_like(zz, 3.0)
        elif name == "zero":
            v = torch.zeros_like(zz)
        elif name.startswith("spike") and name != "spikes2":
            v = zz.clone()
            at = j % (2 * ntile)
            v[j, (at // 2) * bn + (at % 2) * (bn - 1)] = _PARAM[name]
        elif name == "spikes2":
            v = zz.clone()
            v[j, j % bn] += 1e3
            v[j, (ntile - 1) * bn + (j * 7 + 3) % bn] -= 1e3
        elif name == "tilestep":
            v = (zz.view(-1, ntile, bn) + torch.tensor(TILESTEP[:ntile]).view(1, ntile, 1)).reshape(-1, C)
        elif name.startswith("tiny"):
            v = _PARAM[name] * zz
        else:
            v = out[idx]
        x[idx] = v
    assert x.abs().max().item() < 65504
    return x, fam


def params(C: int, N: int, prec: str, seed: int = 1):
    """(gamma [C], beta [C], W16 [N, C] of the 16-bit type, bias [N]) on the CPU: the weights of the GEMM forms."""
    g = torch.Generator().manual_seed(seed)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    w16 = (torch.randn(N, C, generator=g) / math.sqrt(C)).to(DT16[prec])
    bias = torch.randn(N, generator=g)
    return gamma, beta, w16, bias


def round16(t: torch.Tensor, prec: str) -> torch.Tensor:
    return t.to(DT16[prec]).double()


def gelu64(v: torch.Tensor) -> torch.Tensor:
    return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def stats64(x: torch.Tensor, eps: float):
    """(mean [rows, 1], rstd [rows, 1]) in float64, biased variance."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def ln64(x, gamma, beta, eps):
    mean, rstd = stats64(x, eps)
    return (x.double() - mean) * rstd * gamma.double() + beta.double()


def gemm64(x, gamma, beta, eps, w16, bias, act=0):
    y = ln64(x, gamma, beta, eps) @ w16.double().t() + bias.double()
    return gelu64(y) if act == 1 else y


def tile_stats64(x: torch.Tensor):
    """[rows, ntile, 2] = per-tile (mean, M2) in float64."""
    C = x.shape[1]
    bn = fold_bn(C)
    xt = x.double().view(-1, C // bn, bn)
    mean = xt.mean(-1)
    return torch.stack([mean, ((xt - mean[..., None]) ** 2).sum(-1)], -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# emulations
# ---------------------------------------------------------------------------------------------------------------------------------
def classic(x, gamma, beta, eps, w16, bias, act, prec, round_out=True):
    y = round16(ln64(x, gamma, beta, eps), prec) @ w16.double().t() + bias.double()
    y = gelu64(y) if act == 1 else y
    return round16(y, prec) if round_out else y


MUTANTS = {
    "next_row": "(mean, rstd) taken from the next row",
    "no_between": "ln_combine without the between-tile term (m2 = sum qk)",
    "onepass32": "one-pass variance E[x^2] - mean^2 in float32",
    "eps_dropped": "eps dropped",
    "eps_after_sqrt": "eps added after the square root",
    "mean_div4": "row mean divided by 4 tiles when ntile = 3",
    "c_shift": "c1 and c2 indexed one column off",
}


def combine(st: torch.Tensor, C: int, eps: float, mutant=None):
    """ln_combine (wm_common.h) on [rows, ntile, 2] partials, in their dtype: (mean [rows, 1], rstd [rows, 1])."""
    ntile = st.shape[1]
    bn = C // ntile
    mk, qk = st[..., 0], st[..., 1]
    mean = mk.sum(-1, keepdim=True) / (4 if mutant == "mean_div4" and ntile == 3 else ntile)
    m2 = qk.sum(-1, keepdim=True)
    if mutant != "no_between":
        m2 = m2 + (bn * (mk - mean) ** 2).sum(-1, keepdim=True)
    var = m2 / C
    if mutant == "eps_dropped":
        rstd = 1.0 / torch.sqrt(var)
    elif mutant == "eps_after_sqrt":
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    return mean, rstd


def row_stats(x, eps, mutant=None):
    """The folded form's (mean, rstd) per row in float64, from the tiled statistics of the fp32 rows."""
    if mutant == "onepass32":
        xf = x.float()
        mean = xf.sum(-1, keepdim=True) / x.shape[1]
        var = (xf * xf).sum(-1, keepdim=True) / x.shape[1] - mean * mean
        mean, rstd = mean.double(), (1.0 / torch.sqrt(var + eps)).double()
    else:
        mean, rstd = combine(tile_stats64(x), x.shape[1], eps, mutant)
    if mutant == "next_row":
        mean, rstd = torch.roll(mean, -1, 0), torch.roll(rstd, -1, 0)
    return mean, rstd


def fold_weight(gamma, beta, w16, bias, prec):
    """(wf, c1, c2) in float64; gamma (.) W16 is formed in fp32 and rounded once, as fold_weight_kernel does."""
    wf = (gamma.float()[None, :] * w16.float()).to(DT16[prec]).double()
    return wf, wf.sum(1), w16.double() @ beta.double() + bias.double()


def folded(x, gamma, beta, eps, w16, bias, act, prec, mutant=None, round_out=True):
    mean, rstd = row_stats(x, eps, mutant)
    wf, c1, c2 = fold_weight(gamma, beta, w16, bias, prec)
    if mutant == "c_shift":
        c1, c2 = torch.roll(c1, 1), torch.roll(c2, 1)
    y = rstd * (round16(x, prec) @ wf.t() - mean * c1) + c2
    y = gelu64(y) if act == 1 else y
    return round16(y, prec) if round_out else y


def ln_mutant64(x, gamma, beta, eps, mutant=None):
    """The LayerNorm itself with the folded form's (possibly mutated) statistics, float64: the fp32-output kernel's mutants."""
    mean, rstd = row_stats(x, eps, mutant)
    return (x.double() - mean) * rstd * gamma.double() + beta.double()


def ln32(x, gamma, beta, eps):
    """Two-pass LayerNorm, every operation in float32."""
    x = x.float()
    C = x.shape[1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / C
    return d * (1.0 / torch.sqrt(var + eps)) * gamma.float() + beta.float()


def tile_stats32(x):
    C = x.shape[1]
    bn = fold_bn(C)
    xt = x.float().view(-1, C // bn, bn)
    mean = xt.sum(-1) / bn
    d = xt - mean[..., None]
    return torch.stack([mean, (d * d).sum(-1)], -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# errors and bars
# ---------------------------------------------------------------------------------------------------------------------------------
def row_err(got, ref, fam):
    """Per-row relative L2 of got against ref (float64); a row of zero reference norm against its family's largest norm."""
    got, ref = got.double(), ref.double()
    en, rn = (got - ref).norm(dim=-1), ref.norm(dim=-1)
    scale = rn.clone()
    fam = fam.to(rn.device)
    for f in torch.unique(fam[rn == 0]).tolist():
        m = fam == f
        scale[m & (rn == 0)] = rn[m].max().clamp_min(1e-300)
    e = en / scale
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def family_worst(v: torch.Tensor, fam: torch.Tensor) -> torch.Tensor:
    """v [rows, ...] -> per row the largest v over the rows of its family (same trailing shape)."""
    out = torch.empty_like(v)
    fam = fam.to(v.device)
    for f in torch.unique(fam).tolist():
        m = fam == f
        out[m] = v[m].amax(0, keepdim=True)
    return out


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """One fp32 ulp at |v| (float64 result)."""
    v = v.abs().float().clamp_min(2.0 ** -126)
    return (torch.nextafter(v, torch.full_like(v, float("inf"))) - v).double()


def bar_out16(x, gamma, beta, eps, prec, fam):
    ref = ln64(x, gamma, beta, eps)
    return ref, BAR_FACTOR * row_err(round16(ref, prec), ref, fam)


def bar_out32(x, gamma, beta, eps, fam):
    ref = ln64(x, gamma, beta, eps)
    emu = family_worst(row_err(ln32(x, gamma, beta, eps), ref, fam), fam)
    _, rstd = stats64(x, eps)
    floor = ulp32(x.abs().amax(-1)) * rstd[:, 0] * gamma.double().norm() / ref.norm(dim=-1).clamp_min(1e-300)
    return ref, torch.maximum(FP32_BAR_FACTOR * emu, floor)


def bar_stats(x, fam):
    """(float64 [rows, ntile, 2], bars of the same shape, absolute)."""
    ref = tile_stats64(x)
    emu = family_worst((tile_stats32(x).double() - ref).abs().amax(1, keepdim=True).expand_as(ref).contiguous(), fam)
    u = ulp32(x.abs().amax(-1))
    floor = torch.stack([u, u * u * x.shape[1]], -1)[:, None, :].expand_as(ref)
    return ref, torch.maximum(FP32_BAR_FACTOR * emu, floor)


def bar_classic(x, gamma, beta, eps, w16, bias, act, prec, fam):
    ref = gemm64(x, gamma, beta, eps, w16, bias, act)
    return ref, BAR_FACTOR * row_err(classic(x, gamma, beta, eps, w16, bias, act, prec), ref, fam)


def bar_folded(x, gamma, beta, eps, w16, bias, act, prec, fam, ref=None):
    """(ref, bar per row, the folded emulation's error per row, the fp32-noise term per row)."""
    if ref is None:
        ref = gemm64(x, gamma, beta, eps, w16, bias, act)
    emu = row_err(folded(x, gamma, beta, eps, w16, bias, act, prec), ref, fam)
    _, rstd = row_stats(x, eps)
    wf, _, _ = fold_weight(gamma, beta, w16, bias, prec)
    rn = ref.norm(dim=-1)
    rn = torch.where(rn > 0, rn, rn.max())
    noise = rstd[:, 0] * math.sqrt(x.shape[1]) * 2.0 ** -24 * (round16(x, prec).abs() @ wf.abs().t()).norm(dim=-1) / rn
    return ref, BAR_FACTOR * emu + noise, emu, noise


def per_family(err: torch.Tensor, bar: torch.Tensor, fam: torch.Tensor):
    """{family: (worst error, its bar, row)} with the row that stands highest over its bar (by difference where the bar is zero)."""
    out = {}
    err, bar = err.double().cpu(), bar.double().cpu()
    if err.dim() > 1:
        over = (err / bar.clamp_min(1e-300)).flatten(1)
        k = over.argmax(1)
        pick = torch.arange(err.shape[0])
        err, bar = err.flatten(1)[pick, k], bar.flatten(1)[pick, k]
    fam = fam.cpu()
    for f in torch.unique(fam).tolist():
        idx = torch.nonzero(fam == f).flatten()
        score = torch.where(bar[idx] > 0, err[idx] / bar[idx].clamp_min(1e-300), torch.where(err[idx] > 0, float("inf"), 0.0).double())
        j = int(score.argmax())
        out[FAMILIES[f]] = (err[idx[j]].item(), bar[idx[j]].item(), int(idx[j]))
    return out


def failures(pf: dict) -> dict:
    return {f: v for f, v in pf.items() if not v[0] <= v[1]}


def line(name: str, pf: dict) -> str:
    return f"{name}: " + "  ".join(f"{f} {e:.1e}({b:.1e})" for f, (e, b, _) in pf.items())


def check(name: str, err, bar, fam) -> dict:
    """Prints one line of per-family worst rows with their bars, then asserts every row (error <= bar)."""
    pf = per_family(err, bar, fam)
    print(line(name, pf))
    bad = failures(pf)
    assert not bad, f"{name}: over the bar (family: error, bar, row) {bad}"
    return pf
