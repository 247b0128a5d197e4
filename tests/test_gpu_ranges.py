"""Value-range parity (-m gpu): the attention kernels at logits far from O(1) and the split fp32 GEMM at operand sizes far from 1,
each against a float64 evaluation of the same operation on the same 16-bit-rounded operands (P rounded before P.V like the kernels).

Attention.  A common component on q and k (dimension 0 of every head, zero in the rel-pos tables) moves every logit of a query by the
same constant, which the softmax does not see: the output must match the reference and the same kernel's output on the unshifted
input.  Giving that component to the first 64 keys only puts the first key tile ~200 natural units below the rest, and a large
negative rel_pos_h[63] along it sinks every query's own grid row (for grid row 0 that is the first key tile).  A first key tile whose
log2-domain maximum is below -128 once made the global kernels rescale their empty accumulators by exp2(+inf): NaN rows.

Split fp32 GEMM.  Rows of A spread over 1e-5 .. 1e3 and columns of W over 2e-6 .. 2e-2: the error of every row and every column is
measured relative to that row's or column's own output.  The lo parts of the fp16 split once lay in fp16's subnormals below |x| = 0.25
and lost accuracy in proportion (2e-5 at rows of 1e-3).
"""
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import wm_oracle as O          # checker only
import gpu_util as G

OUT16_TOL = {"bf16": 5e-3, "fp16": 7e-4}
SHIFTS = (-100.0, -300.0, 300.0)
QA = 16.0                                  # q's common component; k's is chosen for the wanted logit shift


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()


def _randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _kcomp(shift, hd, prec):
    """k's component that, against QA on q, moves a logit by ~shift natural units (rounded as the kernel sees it)."""
    return G.rnd16(torch.tensor(shift * math.sqrt(hd) / QA), prec).item()


# ---------------------------------------------------------------------------
# encoder attention (packed qkv, decomposed rel-pos)
# ---------------------------------------------------------------------------
def encoder_case(case, prec, hd, window, heads=2, B=1, seed=0):
    """(qkv16, bias, rel_h, rel_w) for one case: 'base', 'shift<s>', 'first_tile', 'relpos'.  Dimension 0 of each head's q and k is the
    common component (0 in 'base'); the rel-pos tables have 0 there, so it enters the logits only through q.k (or rel_h[63] in 'relpos')."""
    D, S = heads * hd, (window or 64)
    x = _randn(seed, B * 4096, 3 * D) * 0.5
    bias = torch.randn(3 * D, generator=torch.Generator().manual_seed(seed + 1)) * (0.1 if window else 0.0)
    rel_h = _randn(seed + 2, 2 * S - 1, hd) * 0.3
    rel_w = _randn(seed + 3, 2 * S - 1, hd) * 0.3
    qc = torch.arange(heads) * hd
    kc = D + qc
    x[:, qc] = 0.0
    x[:, kc] = 0.0
    bias[qc] = 0.0
    bias[kc] = 0.0
    rel_h[:, 0] = 0.0
    rel_w[:, 0] = 0.0
    if case.startswith("shift"):
        k = _kcomp(float(case[5:]), hd, prec)
        x[:, qc] = QA
        x[:, kc] = k
        bias[qc] = QA                      # padded tokens (window) carry the bias: the same shift
        bias[kc] = k
    elif case == "first_tile":
        x[:, qc] = QA
        first = torch.nonzero((torch.arange(B * 4096) % 4096) < 64).flatten()          # keys 0..63 of each image: the first key tile
        x[first[:, None], kc[None, :]] = _kcomp(-200.0, hd, prec)
    elif case == "relpos":
        x[:, qc] = QA
        rel_h[S - 1, 0] = -200.0 / QA      # own grid row: q . rel_h[63] ~ -200
    else:
        assert case == "base", case
    dev = G.dev()
    return G.to16(x.to(dev), prec), bias.to(dev), rel_h.to(dev), rel_w.to(dev)


def run_encoder_case(case, prec, hd, window, heads=2, B=1):
    qkv, bias, rel_h, rel_w = encoder_case(case, prec, hd, window, heads, B)
    return G.encoder_attention(qkv, bias, rel_h, rel_w, B, heads, hd, window, prec)


def _check_encoder(out, base_out, case, prec, hd, window, heads=2, B=1):
    """out / base_out: the kernel's outputs of `case` and of 'base'."""
    assert torch.isfinite(out.float()).all(), f"{case}: non-finite output ({(~torch.isfinite(out.float())).any(1).sum().item()} rows)"
    qkv, bias, rel_h, rel_w = encoder_case(case, prec, hd, window, heads, B)
    ref = G.ref_encoder_attention(qkv, G.rnd16(bias, prec), rel_h, rel_w, B, heads, hd, window, prec, dtype=torch.float64)
    err = G.rel_l2(out, ref)
    msg = f"{prec} hd {hd} window {window} {case}: rel-L2 {err:.2e} against float64"
    if case.startswith("shift"):
        d = G.rel_l2(out, base_out.double())
        msg += f", {d:.2e} against the unshifted input"
        assert d < 2 * OUT16_TOL[prec], msg
    if case == "relpos":                   # grid row 0 (its own row is the first key tile) on its own
        row0 = ((torch.arange(B * 4096) % 4096) < 64).to(out.device)
        e0 = G.rel_l2(out[row0], ref[row0])
        msg += f", grid row 0 {e0:.2e}"
        assert e0 < 2 * OUT16_TOL[prec], msg
    print(msg)
    assert err < 2 * OUT16_TOL[prec], msg


ENC_CASES = [f"shift{s:g}" for s in SHIFTS] + ["first_tile", "relpos"]


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("hd", [80, 64])
@pytest.mark.parametrize("case", ENC_CASES)
def test_global_attention_extreme_logits(case, prec, hd):
    """The 8-wave global kernel with rel-pos (attn_global8_kernel<REL>), the encoder's global blocks."""
    base = run_encoder_case("base", prec, hd, 0)
    _check_encoder(run_encoder_case(case, prec, hd, 0), base, case, prec, hd, 0)


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_ranges as R
outs = {}
for prec in ("fp16", "bf16"):
    for hd in (80, 64):
        for case in ["base"] + R.ENC_CASES:
            outs[(prec, hd, case)] = R.run_encoder_case(case, prec, hd, 0).cpu()
for case in ["base"] + R.MHA_CASES:
    outs[("hfc", case)] = R.run_mha16_case(case, "fp16", 8, 128, 4096, 4096, 1).cpu()
torch.cuda.synchronize()
torch.save(outs, sys.argv[2] + "/outs.pt")
print("saved", len(outs))
"""


def test_global_attention_extreme_logits_4wave():
    """The same cases through the 4-wave global kernel (attn_global_kernel<REL>, and <!REL> at the HFC geometry), which WM_ATTN_4WAVE=1
    selects for every shape; the switch is read once per process, so the kernel runs in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tempfile.mkdtemp()
    env = dict(os.environ, WM_ATTN_4WAVE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, d], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    outs = torch.load(os.path.join(d, "outs.pt"))
    bad = []
    for prec in ("fp16", "bf16"):
        for hd in (80, 64):
            for case in ENC_CASES:
                try:
                    _check_encoder(outs[(prec, hd, case)].to(G.dev()), outs[(prec, hd, "base")].to(G.dev()), case, prec, hd, 0)
                except AssertionError as e:
                    bad.append(str(e).splitlines()[0])
    for case in MHA_CASES:
        try:
            _check_mha16(outs[("hfc", case)].to(G.dev()), outs[("hfc", "base")].to(G.dev()), case, "fp16", 8, 128, 4096, 4096, 1)
        except AssertionError as e:
            bad.append("hfc " + str(e).splitlines()[0])
    assert not bad, "4-wave kernel: " + "; ".join(bad)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("case", [f"shift{s:g}" for s in SHIFTS])
def test_window_attention_extreme_logits(case, prec):
    """The window kernel (its first half-step never rescales: the form the global kernels now share); padded tokens carry the shift."""
    hd = 80
    base = run_encoder_case("base", prec, hd, 14, heads=2, B=1)
    _check_encoder(run_encoder_case(case, prec, hd, 14), base, case, prec, hd, 14)


# ---------------------------------------------------------------------------
# mha16 (no rel-pos): the HFC cross-attention and the short key counts
# ---------------------------------------------------------------------------
MHA_CASES = [f"shift{s:g}" for s in SHIFTS] + ["first_tile"]


def mha_case(case, prec, heads, hd, nq, nk, B, seed=7):
    D = heads * hd
    q = _randn(seed, B * nq, D)
    k = _randn(seed + 1, B * nk, D)
    v = _randn(seed + 2, B * nk, D)
    qc = torch.arange(heads) * hd
    q[:, qc] = 0.0
    k[:, qc] = 0.0
    if case.startswith("shift"):
        q[:, qc] = QA
        k[:, qc] = _kcomp(float(case[5:]), hd, prec)
    elif case == "first_tile":
        q[:, qc] = QA
        first = torch.nonzero((torch.arange(B * nk) % nk) < 64).flatten()
        k[first[:, None], qc[None, :]] = _kcomp(-200.0, hd, prec)
    else:
        assert case == "base", case
    dev = G.dev()
    return G.to16(q.to(dev), prec), G.to16(k.to(dev), prec), G.to16(v.to(dev), prec)


def run_mha16_case(case, prec, heads, hd, nq, nk, B):
    q, k, v = mha_case(case, prec, heads, hd, nq, nk, B)
    return G.mha16(q, k, v, B, heads, hd, nq, nk, prec)


def _ref_mha(q, k, v, B, heads, hd, nq, nk, prec):
    """float64 softmax(q k^T / sqrt(hd)), P rounded to the 16-bit type, P v; one head at a time."""
    qf = q.double().view(B, nq, heads, hd)
    kf = k.double().view(B, nk, heads, hd)
    vf = v.double().view(B, nk, heads, hd)
    out = torch.empty(B, nq, heads, hd, dtype=torch.float64, device=q.device)
    for h in range(heads):
        p = ((qf[:, :, h] @ kf[:, :, h].transpose(-1, -2)) / math.sqrt(hd)).softmax(-1)
        out[:, :, h] = G.rnd16(p, prec, torch.float64) @ vf[:, :, h]
    return out.view(B * nq, heads * hd)


def _check_mha16(out, base_out, case, prec, heads, hd, nq, nk, B):
    assert torch.isfinite(out.float()).all(), f"{case}: non-finite output ({(~torch.isfinite(out.float())).any(1).sum().item()} rows)"
    ref = _ref_mha(*mha_case(case, prec, heads, hd, nq, nk, B), B, heads, hd, nq, nk, prec)
    err = G.rel_l2(out, ref)
    msg = f"mha16 {prec} ({nq}, {nk}) {heads} x {hd} {case}: rel-L2 {err:.2e} against float64"
    if case.startswith("shift"):
        d = G.rel_l2(out, base_out.double())
        msg += f", {d:.2e} against the unshifted input"
        assert d < 2 * OUT16_TOL[prec], msg
    print(msg)
    assert err < 2 * OUT16_TOL[prec], msg


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("case", MHA_CASES)
def test_mha16_hfc_extreme_logits(case, prec):
    """HFC geometry, 8 heads x 128, 4096 x 4096: the 8-wave kernel without rel-pos (-m through the bias k-step)."""
    args = (prec, 8, 128, 4096, 4096, 1)
    base = run_mha16_case("base", *args)
    _check_mha16(run_mha16_case(case, *args), base, case, *args)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("nq,nk", [(256, 128), (128, 192), (384, 64)])
@pytest.mark.parametrize("case", MHA_CASES)
def test_mha16_short_extreme_logits(case, nq, nk, prec):
    """(256, 128): the 8-wave kernel; (128, 192) and (384, 64): the 4-wave kernel without rel-pos."""
    args = (prec, 2, 80, nq, nk, 2)
    base = run_mha16_case("base", *args)
    _check_mha16(run_mha16_case(case, *args), base, case, *args)


# ---------------------------------------------------------------------------
# mha32 (the decoder's fp32 attention)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nk,heads", [(51, 4096, 8), (65, 1024, 2)])
@pytest.mark.parametrize("shift", [-300.0, 300.0])
def test_mha32_extreme_logits(nq, nk, heads, shift):
    """(51, 4096): the key-split kernels; (65, 1024): the query-group kernel.  Max-abs bar of test_mha32."""
    B, hd, dev = 2, 16, G.dev()
    D = heads * hd
    q, k, v = _randn(21, B, nq, D), _randn(22, B, nk, D), _randn(23, B, nk, D)
    qc = torch.arange(heads) * hd
    q[..., qc] = 0.0
    k[..., qc] = 0.0
    base = G.mha32(q.to(dev), k.to(dev), v.to(dev), heads)
    q[..., qc] = QA
    k[..., qc] = shift * math.sqrt(hd) / QA
    out = G.mha32(q.to(dev), k.to(dev), v.to(dev), heads)
    assert torch.isfinite(out).all()
    ref = O.mha_core(q.double(), k.double(), v.double(), heads, O.OracleCfg())
    err, d = (out.cpu().double() - ref).abs().max().item(), (out - base).abs().max().item()
    print(f"mha32 ({nq}, {nk}) shift {shift:g}: max-abs {err:.2e} against float64, {d:.2e} against the unshifted input")
    assert err < 2e-5 and d < 2e-5, (err, d)


# ---------------------------------------------------------------------------
# split fp32 GEMM
# ---------------------------------------------------------------------------
GEMM32_SHAPES = [(51, 8, 256), (102, 4, 256), (4096, 128, 256), (51, 2048, 256), (153, 256, 2048), (816, 256, 256), (65536, 128, 256),
                 (65536, 256, 128), (64, 64, 32), (70, 14, 96)]


def _gemm32_mode(a, w, mode):
    flag = {"fp32": 0, "split": G.N.GEMM32_SPLIT, "presplit": G.N.GEMM32_PRESPLIT}[mode]
    out = torch.empty((a.shape[0], w.shape[0]), device=a.device, dtype=torch.float32)
    G.N.check(G.N.lib().wm_op_gemm32(G.N.ptr(a), G.N.ptr(w), None, None, G.N.ptr(out), a.shape[0], w.shape[0], a.shape[1], flag, G.sp()))
    return out


@pytest.mark.parametrize("M,N,K", GEMM32_SHAPES)
def test_gemm32_rows_and_columns_of_any_size(M, N, K):
    """Rows of A of size 10^u, u in [-5, 3], columns of W of size 0.02 * 10^v, v in [-4, 0].  The error of each row and each column
    against float64 is measured relative to the size of what it sums, the norm of that row / column of |A| |W|^T: free of cancellation
    (a row's own output norm is not: with N = 4 the fp32-MFMA kernel shows 1.8e-5 on it) and still proportional to the row's scale.
    Bounds: 2e-7 for the rows and columns of size 1e-4 and up, 2e-6 for every row down to 1e-5.  Measured on the MI355X: split form
    5.3e-8 and 3.3e-7 there (columns 5.6e-8), fp32-MFMA kernel 1.0e-7 (columns 1.3e-7).  With the unscaled lo of before, a CPU
    emulation gave 6.9e-7 .. 4.8e-6 on rows of 1e-3 and 5.8e-5 .. 4.8e-4 overall (on the MI355X: 1.5e-5 .. 3.6e-5 at 1e-3 relative
    to the rows' own output norm).
    For the split form with W split per K-step (the op-level entry), with W pre-split by split_w32_kernel (the decoder inside
    wm_forward; the two give the same bits), and the fp32-MFMA kernel as the control.  No bias and no residual: an O(1) term added
    in fp32 would set the floor of a small row's error."""
    dev = G.dev()
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    u = torch.rand(M, 1, generator=g) * 8 - 5
    v = torch.rand(N, 1, generator=g) * 4 - 4
    u[0], u[-1] = -5.0, 3.0
    u[M // 2] = -3.0
    v[0] = -4.0
    a = (torch.randn(M, K, generator=g) * 10.0 ** u).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.02 * 10.0 ** v).to(dev)
    y = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    ru, cv = u.flatten().to(dev), v.flatten().to(dev)
    res = {}
    for mode in ("split", "presplit", "fp32"):
        out = _gemm32_mode(a, w, mode)
        assert torch.isfinite(out).all(), mode
        e = out.double() - y
        rowe = e.norm(dim=1) / mag.norm(dim=1)
        cole = e.norm(dim=0) / mag.norm(dim=0)
        res[mode] = (out, rowe, cole)
        print(f"gemm32 {mode} M={M} N={N} K={K}: rows >= 1e-4 {rowe[ru >= -4].max().item():.2e}, rows >= 1e-3 "
              f"{rowe[ru >= -3].max().item():.2e}, all rows {rowe.max().item():.2e}, columns {cole.max().item():.2e}")
    for mode, (out, rowe, cole) in res.items():
        assert rowe[ru >= -4].max().item() < 2e-7, (mode, rowe[ru >= -4].max().item())
        assert cole[cv >= -4].max().item() < 2e-7, (mode, cole.max().item())
        assert rowe.max().item() < 2e-6, (mode, rowe.max().item())
    assert torch.equal(res["split"][0], res["presplit"][0])
