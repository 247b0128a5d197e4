"""The attention family query by query (-m gpu): every kernel instance behind wm_op_encoder_attention, wm_op_mha16 and wm_op_mha32,
through the C ABI, against the float64 oracle of tests/attention_cases.py on inputs where each query's answer is one chosen key
(select), the mean of two (pair), a known share of the padded keys (pads), or a realistic softmax (diffuse).  Errors are relative L2
per (image, head, query), per window, per target key tile, per head, per image and over the whole tensor; every bar is computed in
the run from the oracle and its emulation (attention_cases.py has the rules).  Each launch writes into a guarded buffer (guards
and the gap columns of a strided output untouched, every output element written) and is repeated (the same bits).
Run with -s for the figures; profiles/attention_queries/gpu_tests.txt is that output."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A
import attention_run as R
import gpu_util as G

N = G.N
WINDOW_B, GLOBAL_B, HEADS, GLOBAL_CASES = R.WINDOW_B, R.GLOBAL_B, R.HEADS, R.GLOBAL_CASES


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    G.need_gpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# encoder form: the window kernel and the global kernels with rel-pos
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["select", "pair", "pads", "diffuse"])
@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_window_attention_queries(prec, hd, kind):
    """attn_window_kernel<T, 64 | 80>: 4 images x 2 heads = 200 items, one per workgroup."""
    R.encoder_case(f"window {prec} hd {hd} {kind}", kind, 14, WINDOW_B, HEADS, hd, prec)


def test_window_attention_queries_multi_item_walk():
    """The persistent loop's back edge per query (the next item's K / V prefetch, the Q hand-over): B = CUs // (25 heads) + 1, the rule of
    test_window_attention_multi_item_walk, so some workgroups walk two items."""
    cus = torch.cuda.get_device_properties(G.dev()).multi_processor_count
    B = cus // (25 * HEADS) + 1
    print(f"multi-item walk: B={B} items={25 * HEADS * B} CUs={cus}")
    R.encoder_case(f"window fp16 hd 80 select B={B}", "select", 14, B, HEADS, 80, "fp16")


@pytest.mark.parametrize("prec,hd,kind", GLOBAL_CASES)
def test_global_attention_queries_8wave(prec, hd, kind):
    """attn_global8_kernel<T, 64 | 80, rel-pos>: 2 images x 2 heads."""
    R.encoder_case(f"global 8-wave {prec} hd {hd} {kind}", kind, 0, GLOBAL_B, HEADS, hd, prec)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import attention_run as R
R.run_global_cases_4wave()
"""


def test_global_attention_queries_4wave():
    """attn_global_kernel<T, 64 | 80, rel-pos>, which WM_ATTN_4WAVE=1 selects; the library reads the switch once per process, so all its
    cases run in one child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root], env=dict(os.environ, WM_ATTN_4WAVE="1"), capture_output=True, text=True, timeout=300)
    print(r.stdout, end="")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("global 4-wave") == len(GLOBAL_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# plain forms
# ---------------------------------------------------------------------------------------------------------------------------------
def _filler(rows, cols, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g).to(dt).to(G.dev())


# (name, B, heads, hd, nq, nk, prec, layout): layout plain / kv (k and v interleaved in one buffer) / strided (q and out rows wider than heads * hd)
MHA16 = [("8-wave", 2, 2, 64, 256, 128, "fp16", "plain"), ("4-wave", 2, 2, 64, 128, 192, "bf16", "plain"), ("4-wave", 2, 2, 64, 384, 64, "fp16", "plain"),
         ("4-wave", 2, 2, 64, 128, 64, "bf16", "plain"), ("4-wave", 2, 2, 128, 128, 128, "fp16", "plain"), ("8-wave", 2, 2, 80, 256, 256, "bf16", "strided"),
         ("8-wave HFC", 1, 2, 128, 4096, 4096, "fp16", "kv")]


@pytest.mark.parametrize("shape", MHA16, ids=lambda s: "-".join(map(str, s)).replace(" ", "_"))
def test_mha16_queries(shape):
    """wm_op_mha16 (no rel-pos): (256, 128) and the HFC geometry take the 8-wave kernel, (128, 192), (384, 64), (128, 64) and (128, 128) at
    head_dim 128 the 4-wave one (host_attn.h: nq % 256 == 0 and nk >= 128)."""
    tag, B, heads, hd, nq, nk, prec, layout = shape
    code, dt = G.PRECS[prec]
    D = heads * hd
    for kind in ("select", "pair", "diffuse"):
        case = A.case_to(A.make_plain_case(kind, B, heads, hd, nq, nk, prec), G.dev())
        name = f"mha16 {tag} {nq}x{nk} hd {hd} {prec} {layout} {kind}"
        q2, k2, v2 = case.q.reshape(B * nq, D), case.k.reshape(B * nk, D), case.v.reshape(B * nk, D)
        qs = os_ = ks = vs = D
        kbuf, vbuf = k2.contiguous(), v2.contiguous()
        kptr, vptr = N.ptr(kbuf), N.ptr(vbuf)
        if layout == "strided":
            qs, os_ = D + 40, D + 24
            q2 = torch.cat([q2, _filler(B * nq, 40, dt, 1)], 1)
        if layout == "kv":
            ks = vs = 2 * D
            kbuf = torch.cat([k2, v2], 1).contiguous()
            kptr, vptr = N.ptr(kbuf), G.C.c_void_p(kbuf.data_ptr() + D * kbuf.element_size())
        q2 = q2.contiguous()

        def launch(out):
            N.check(N.lib().wm_op_mha16(N.ptr(q2), qs, kptr, ks, vptr, vs, N.ptr(out), os_, B, heads, hd, nq, nk, code, G.sp()))
        out = R.launch_twice(name, launch, B * nq, os_, D, dt).reshape(B, nq, heads, hd)
        R.measure(name, case, lambda b, h: out[b, :, h], lambda b, h: case.v[b, :, h].double())


# (B, heads, hd, nq, nk): B the smallest with B heads nq >= nk, so that every key is some query's target
MHA32 = [("key split + merge", 11, 8, 16, 51, 4096), ("few keys", 1, 8, 16, 4096, 51), ("shared KV", 8, 2, 16, 65, 1024),
         ("one query per wave", 10, 2, 16, 7, 130), ("hd 32", 2, 8, 32, 51, 51)]


@pytest.mark.parametrize("shape", MHA32, ids=lambda s: "-".join(map(str, s)).replace(" ", "_"))
def test_mha32_queries(shape):
    """wm_op_mha32's five forms (host_attn.h launch_mha32)."""
    tag, B, heads, hd, nq, nk = shape
    D = heads * hd
    for kind in ("select", "pair", "diffuse"):
        case = A.case_to(A.make_plain_case(kind, B, heads, hd, nq, nk, "fp32"), G.dev())
        name = f"mha32 {tag} {nq}x{nk} hd {hd} {kind}"
        q2, k2, v2 = case.q.reshape(B * nq, D).contiguous(), case.k.reshape(B * nk, D).contiguous(), case.v.reshape(B * nk, D).contiguous()

        def launch(out):
            N.check(N.lib().wm_op_mha32(N.ptr(q2), N.ptr(k2), N.ptr(v2), N.ptr(out), B, heads, hd, nq, nk, G.sp()))
        out = R.launch_twice(name, launch, B * nq, D, D, torch.float32).reshape(B, nq, heads, hd)
        R.measure(name, case, lambda b, h: out[b, :, h], lambda b, h: case.v[b, :, h].double())
