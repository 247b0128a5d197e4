"""The attention family's query cases: what tests/test_gpu_attention_queries.py (with attention_run.py) and tests/test_attention_cases.py share.  Plain module
(torch only, any device), asserts nothing: the cases, the float64 oracle, the emulation, the mutants, the metrics and the bar rule.
Follows encoder_cases.py / layernorm_cases.py.

FORMS.  Encoder form (make_encoder_case / enc_item): packed qkv [B * 4096, 3 D] of the 16-bit type, decomposed rel-pos from the
UNSCALED q, window = 14 (the 70 x 70 padded grid: the last window of each direction holds 8 real rows / columns and 6 padded ones;
a padded token carries the bias row as q / k / v and is NOT masked) or 0 (one 64 x 64 grid).  Plain form (make_plain_case /
plain_item): softmax(q k^T / sqrt(hd)) v, mha16 and mha32.  Everything is evaluated one (image, head) ITEM at a time.

ORACLE (attend, emu=None).  Float64 on the 16-bit-rounded operands the kernel is given (the cases hold only representable values,
tables and bias row included).  The rel-pos term is read through explicit per-(query, key) index tables ih / iw (rel_index), the
window partition through an explicit slot -> token table (window_tokens), so every mutant is a one-line switch.

EMULATION (attend, emu=(prec, den_rounded)).  The same with the roundings the kernels document and float64 accumulation:
  q16s = round16(fp32(q) * c1), c1 = fp32(hd^-0.5) * fp32(log2 e)        scale_q16_kernel, the op entry points' copy of q
  scores (log2 domain) = q16s . k  +  (q16s . round16(table row)) / fp32(hd^-0.5)      both rel-pos terms, from the SCALED copy
  padded rows = round16(bias)
  P = exp2(score - m) rounded to the 16-bit type before P V
  denominator = sum of the ROUNDED P where hd % 32 != 0 (AttnGeom::LSUM_IN_O: hd 80, the V image's pad column of ones rides the
      matrix pipe), else the sum of the UNROUNDED P (hd 64, 128: `ls += pv` in front of the convert) -- den_rounded(hd)
  output rounded to the 16-bit type.
m is the kernels' reference point: the maximum of an EARLIER key tile, moved only when some query of the wave exceeds it by 2^6
(attn_common.h move_reference), so the largest P of a row is 2^d with 0 <= d <= 6, not 1, and its rounding is not exact.  Which d
a query gets depends on its wave's other queries and on fp32 score bits; the emulation takes m = row maximum - d with d a fixed
per-query sequence in [0, 1) (ref_slack): only the position inside the binade matters to a relative rounding.
mha32: the emulation is the whole operation in float32 (plain_item(emu="f32")).

CASES.  A case holds inputs plus `target` [B, heads, nq, T]: the designated key(s) of every query (window form: the slot
14 kh + kw inside the query's window; else the key's token).
  select   every query puts its mass on ONE key.  The tables carry one code per row, rel_h codes in the first half of the head's
           dims, rel_w codes in the second: unit vectors where 2 S - 1 <= hd / 2 (windows), else +-1 codes (the 127-row global
           tables).  The query carries the codes of rows qh - kh* + S - 1 and qw - kw* + S - 1; k is small noise, v is O(1) noise.
           Amplitudes (AMP): 4 for windows (logit 32 against 16 for the target's row / column mates), 3 for global select, 1 for
           global pair.  (A scratch check used 6 for global; the masses are 1 either way, and amplitude 1 keeps the pair's two
           scores -- ~110 log2 units -- where an fp32 accumulator's own rounding, ~2^-17, is far below the 16-bit P rounding: at
           6 they are ~3300 and differ by ~2^-11 between two "equal" keys, a term the float64 emulation lacks.)
           Plain forms: the same selection through q . k, keys = +-a codes (distinct sign vectors), q = a code[target].
  pair     two designated keys of one key row with equal logits: the output is the mean of two value rows (P values and the
           denominator, not only the argmax).  Global: the partner row of rel_w is the one with the largest margin over every
           third row (pair_partner), +-1 codes of length hd / 2 not being orthogonal.
  pads     window only.  q = 1 on the dims no code uses (FREE dims) + small noise, the bias k-row = -beta there, so every padded
           key gets the same logit -0.2 against ~0 for the real ones: in the nine edge windows the padded keys together take
           0.38 (84 of 196 keys) to 0.63 (132 of 196) of the mass.  The bias v-row (+-3 alternating) is far from every real value
           row.  The share moves with how many padded keys there are and with what they hold.
  diffuse  Gaussian inputs, as test_gpu_ops.py draws them.
Target maps: window -- per (window, head) a random permutation perm of the 196 slots, the j-th real query of image b targets
perm[(j + b n_real + 5 b [n_real = 196]) mod 196]: over 4 images the arguments cover every residue (4 x 64 >= 196 in the corner
window), so every key slot, padded ones included, is some real query's target.  Global -- kh = (qh + a[qw]) mod 64, kw = (qw +
b[kh]) mod 64 with a, b random permutations per (image, head): a composition of two shears, so a permutation of the 4096 keys, and
the rows qh = 0 / 63 (qw = 0 / 63) reach every one of the 127 table rows.  Plain -- item n = b heads + h targets
perm[(i + n nq (+ the least shift that no earlier item has, once those have tiled the keys)) mod nk], one perm per case: every key is a target once
B heads nq >= nk, and the items' maps differ.

METRICS (evaluate).  err = got - ref in float64; relative L2 per (image, head, query) over the head's hd channels, worst taken;
per window; per target key tile (global / plain: 64 keys, a grid row; window: the 32-slot MFMA tile of the 14 x 16 slot layout =
key rows 2 t, 2 t + 1, seven tiles of 28 keys -- attn_window.h; the linear count "keys 192..195" of mutant tile7 is not a tile of
this kernel); per head, per image, whole tensor.  No query and no slice is excluded (evaluate returns the excluded count, 0).

BARS, computed in the run from the oracle and the emulation alone (bar16 / bar32):
  16-bit kernels   BAR_FACTOR (2) x the emulation's metric against the exact oracle, floored per query at one unit in the last
                   place of the output type at the row's largest reference magnitude over the row's norm (an fp32 and a float64
                   sum can round an output element to neighbouring 16-bit values); a group's floor is its queries' floors in
                   quadrature.
                   + the P-ROUNDING term u sqrt(sum_i p_i^2 |v_i - o|^2) / |o| of the oracle's own P (p_noise2), u = 2^-11 (fp16) /
                   2^-8 (bf16).  The kernel rounds P = 2^(score - m) at ITS reference point m, the emulation at another, so the
                   two round every P at another place of its binade: independent relative errors d_i, |d_i| <= u, which move the
                   output by sum_i d_i p_i (v_i - o) -- the usual probabilistic bound with u for each |d_i|, as layernorm_cases.py
                   bounds an fp32 dot product.  The emulation's error holds ONE such draw; the kernel's is another, and on a
                   diffuse softmax (|v_i - o| >> |o|) this draw is most of a row's error, so the ratio of the two rows' errors
                   has a tail that 2 x the row's own emulation error cannot hold (first GPU run, hd 80 diffuse: worst query 1.4
                   x over while every group figure sat at half its bar; the emulation itself at another d sequence stands 1.3 x
                   over its own 2 x, and 0.8 under the bar with this term: test_another_reference_point_is_within_the_bars).  The term is ~0 where one key has the mass (select).
                   Instances with the UNROUNDED denominator (hd 64, 128) get + u, u = 2^-11 (fp16) / 2^-8 (bf16):
                   out = sum round(p_i) v_i / sum p_i = [sum round(p_i) v_i / sum round(p_i)] (1 + e), |e| = |sum (round(p_i) -
                   p_i)| / sum p_i <= u, a relative error of the whole row that depends on where 2^d falls in its binade, i.e. on
                   the kernel's reference point, which the emulation's fixed d sequence only samples.  (hd 80: e = 0 exactly.)
  mha32            FP32_BAR_FACTOR (4) x the fp32 emulation's error, the factor encoder_cases.py gives the FFT for another
                   summation order, the emulation's error taken as the worst over the case (layernorm_cases.py has the reason),
                   floored at one fp32 ulp in the same way.

MUTANTS: a `mutant=` switch on the oracle / emulation, for tests/test_attention_cases.py.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

DT16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp16": 10, "bf16": 7, "fp32": 23}
BAR_FACTOR, FP32_BAR_FACTOR = 2.0, 4.0
WS, GRID, NWIN, NTOK, T = 14, 64, 5, 196, 4096
LOG2E = 1.44269504088896340736
AMP = {("window", "select"): 4.0, ("window", "pair"): 4.0, ("window", "pads"): 4.0, ("global", "select"): 3.0, ("global", "pair"): 1.0}
K_NOISE = 0.004
REF_SLACK_SHIFT = 0.0                                # moves ref_slack's sequence: another reference point (test_attention_cases.py)
OLD_OUT16_TOL = {"bf16": 5e-3, "fp16": 7e-4}          # test_gpu_ops.py's whole-tensor criterion, for the mutant table's last column only

MUTANTS = {
    "rel_h_off1": "rel index off by one (h)",
    "rel_w_off1": "rel index off by one (w)",
    "tables_swapped": "rel_h and rel_w swapped",
    "rel_scaled_q": "rel-pos term taken from the scaled q",
    "pad_masked": "window: padded keys masked out",
    "pad_zero": "window: padded keys hold zero rows, not the bias",
    "pad_clamped": "window: padded keys read the clamped edge token",
    "pad_no_rel": "window: padded keys lose their rel-pos term",
    "dead_cols": "window: the dead columns 14, 15 count as keys",
    "tile7": "window: keys 192..195 dropped",
    "tile_first": "the first key tile dropped",
    "tile_last": "the last key tile dropped",
    "v_swap4": "value rows k and k + 4 swapped inside each 8-key group",
    "rows_63_64": "global: table rows 63 and 64 swapped",
    "row126_zero": "global: table row 126 read as zero",
    "head_v0": "head h reads head 0's values",
    "image_k0": "image b reads image 0's keys",
    "den_unrounded": "denominator from the unrounded P, numerator from the rounded P",
}
WINDOW_MUTANTS = ("rel_h_off1", "rel_w_off1", "tables_swapped", "rel_scaled_q", "pad_masked", "pad_zero", "pad_clamped", "pad_no_rel",
                  "dead_cols", "tile7", "tile_first", "tile_last", "v_swap4", "head_v0", "image_k0", "den_unrounded")
GLOBAL_MUTANTS = ("rel_h_off1", "rel_w_off1", "tables_swapped", "rel_scaled_q", "tile_first", "tile_last", "v_swap4", "rows_63_64",
                  "row126_zero", "head_v0", "image_k0", "den_unrounded")
PLAIN_MUTANTS = ("tile_first", "tile_last", "v_swap4", "head_v0", "image_k0", "den_unrounded")


def round16(t: torch.Tensor, prec: str) -> torch.Tensor:
    return t.to(DT16[prec]).double()


def den_rounded(hd: int) -> bool:
    """AttnGeom::LSUM_IN_O: the softmax denominator is the sum of the rounded P (else of the unrounded)."""
    return hd % 32 != 0


def ulp(v: torch.Tensor, prec: str) -> torch.Tensor:
    """One unit in the last place of `prec` at |v| (float64)."""
    _, e = torch.frexp(v.abs().double().clamp_min(2.0 ** -14 if prec == "fp16" else 2.0 ** -126))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), (e - 1 - MANT[prec]).double())


def ref_slack(n: int, dev) -> torch.Tensor:
    """d in [0, 1) per query: how far (log2 units, inside a binade) the emulation's reference point sits below the row maximum."""
    return torch.remainder(torch.arange(n, device=dev, dtype=torch.float64) * 0.6180339887498949 + 0.25 + REF_SLACK_SHIFT, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry: explicit index tables
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _window_tokens(clamped: bool):
    w, s = torch.arange(NWIN * NWIN), torch.arange(NTOK)
    y = (w // NWIN)[:, None] * WS + (s // WS)[None, :]
    x = (w % NWIN)[:, None] * WS + (s % WS)[None, :]
    if clamped:
        return y.clamp_max(GRID - 1) * GRID + x.clamp_max(GRID - 1)
    return torch.where((y < GRID) & (x < GRID), y * GRID + x, torch.full_like(y, -1))


def window_tokens(dev="cpu", clamped=False) -> torch.Tensor:
    """[25, 196]: the token y * 64 + x of slot 14 kh + kw of each window, -1 where the slot is padding (clamped: the edge token)."""
    return _window_tokens(clamped).to(dev)


@functools.lru_cache(None)
def _token_slots():
    tok = _window_tokens(False)
    win = torch.empty(T, dtype=torch.long)
    slot = torch.empty(T, dtype=torch.long)
    w, s = torch.nonzero(tok >= 0, as_tuple=True)
    win[tok[w, s]], slot[tok[w, s]] = w, s
    return win, slot


def token_slots(dev="cpu"):
    """(window [4096], slot [4096]) of every token."""
    return tuple(t.to(dev) for t in _token_slots())


def rel_index(S: int, dev="cpu", rows=None):
    """(ih, iw) [queries, S * S]: the table rows qh - kh + S - 1 and qw - kw + S - 1 of every (query, key) pair."""
    t = torch.arange(S * S, device=dev)
    qt = t if rows is None else rows
    return (qt // S)[:, None] - (t // S)[None, :] + S - 1, (qt % S)[:, None] - (t % S)[None, :] + S - 1


def free_dims(hd: int) -> torch.Tensor:
    """The head dims no window code uses: [27, hd / 2) and [hd / 2 + 27, hd)."""
    half = hd // 2
    return torch.cat([torch.arange(2 * WS - 1, half), torch.arange(half + 2 * WS - 1, hd)])


# ---------------------------------------------------------------------------------------------------------------------------------
# oracle and emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def attend(q, k, v, hd, rel=None, emu=None, mutant=None, key_mask=None, key_norel=None):
    """q [W, nq, hd], k / v [W, nk, hd] float64; rel = (Rh, Rw [L, hd], ih, iw [nq, nk]) or None; key_mask [W, nk]: keys that are
    not there; key_norel [W, nk]: keys without a rel-pos term.  emu: None (exact), (prec, den_rounded) or "f32".
    -> (out [W, nq, hd], P [W, nq, nk], n2 [W, nq]); exact: float64, P the softmax, n2 = sum_i p_i^2 |v_i - out|^2 (p_noise2)."""
    if emu == "f32":                                            # plain form only
        a =(q.float() @ k.float().transpose(-1, -2)) * (1.0 / math.sqrt(hd))
        if key_mask is not None:
            a = a.masked_fill(key_mask[:, None, :], float("-inf"))
        p = a.softmax(-1)
        return (p @ v.float()).double(), p.double(), None
    W = q.shape[0]
    scale32 = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd), dtype=torch.float32))
    if emu is None:
        qq, score_scale, rel_scale = q, hd ** -0.5, 1.0
    else:
        c1 = scale32 * torch.tensor(LOG2E, dtype=torch.float32)
        qq = (q.float() * c1.to(q.device)).to(DT16[emu[0]]).double()
        score_scale, rel_scale = 1.0, (torch.tensor(1.0, dtype=torch.float32) / scale32).item()
    a = (qq @ k.transpose(-1, -2)) * score_scale
    if rel is not None:
        Rh, Rw, ih, iw = rel
        if emu is not None:
            Rh, Rw = round16(Rh, emu[0]), round16(Rw, emu[0])
        if mutant == "tables_swapped":
            Rh, Rw = Rw, Rh
        if mutant == "rows_63_64":
            sw = torch.arange(Rh.shape[0], device=Rh.device)
            sw[63], sw[64] = 64, 63
            Rh, Rw = Rh[sw], Rw[sw]
        if mutant == "row126_zero":
            Rh, Rw = Rh.clone(), Rw.clone()
            Rh[126], Rw[126] = 0, 0
        if mutant == "rel_h_off1":
            ih = (ih - 1).clamp_min(0)
        if mutant == "rel_w_off1":
            iw = (iw - 1).clamp_min(0)
        r = (qq @ Rh.t()).gather(2, ih.expand(W, -1, -1)) + (qq @ Rw.t()).gather(2, iw.expand(W, -1, -1))
        r = r * (rel_scale * (hd ** -0.5 if mutant == "rel_scaled_q" else 1.0))
        if key_norel is not None:
            r = r.masked_fill(key_norel[:, None, :], 0.0)
        a = a + r
    if key_mask is not None:
        a = a.masked_fill(key_mask[:, None, :], float("-inf"))
    if emu is None:
        p = a.softmax(-1)
        out = p @ v
        return out, p, p_noise2(p, v, out)
    prec, den_r = emu
    if mutant == "den_unrounded":
        den_r = False
    m = a.amax(-1, keepdim=True) - ref_slack(a.shape[1], a.device)[None, :, None]
    p = torch.exp2(a - m)
    p16 = round16(p, prec)
    den = (p16 if den_r else p).sum(-1, keepdim=True)
    return round16((p16 @ v) / den, prec), p16 / den, None


def p_noise2(p, v, out):
    """sum_i p_i^2 |v_i - out|^2 per query: with independent relative errors d_i on the p_i, out moves by sum_i d_i p_i (v_i - out)."""
    p2 = p * p
    n2 = (p2 @ v.pow(2).sum(-1, keepdim=True))[..., 0] - 2 * ((p2 @ v) * out).sum(-1) + p2.sum(-1) * out.pow(2).sum(-1)
    return n2.clamp_min(0.0)                                    # the three terms cancel to round-off where one key has the mass


def _tile_mask(nk, W, first, dev, per=64):
    m = torch.zeros(W, nk, dtype=torch.bool, device=dev)
    if first:
        m[:, :per] = True
    else:
        m[:, nk - per:] = True
    return m


def _swap4(n, dev):
    k = torch.arange(n, device=dev)
    return k ^ 4


def enc_item(case, b, h, emu=None, mutant=None, rows=None, want_p=False):
    """One (image, head) of the encoder form -> out [4096 (or len(rows), global form only), hd] float64 (want_p: and P -- window form
    [25, 196, keys] by slot, global form [queries, 4096] -- and the exact oracle's p_noise2 per query)."""
    B, heads, hd, dev = case.B, case.heads, case.hd, case.qkv.device
    x = case.qkv.view(B, T, 3, heads, hd)
    bk_, hv_ = (0 if mutant == "image_k0" else b), (0 if mutant == "head_v0" else h)
    q, k, v = x[b, :, 0, h].double(), x[bk_, :, 1, h].double(), x[b, :, 2, hv_].double()
    Rh, Rw = case.rel_h.double(), case.rel_w.double()
    if not case.window:
        qt = torch.arange(T, device=dev) if rows is None else rows
        ih, iw = rel_index(GRID, dev, qt)
        mask = _tile_mask(T, 1, mutant == "tile_first", dev) if mutant in ("tile_first", "tile_last") else None
        if mutant == "v_swap4":
            v = v[_swap4(T, dev)]
        out, p, n2 = attend(q[qt][None], k[None], v[None], hd, (Rh, Rw, ih, iw), emu, mutant, mask)
        return (out[0], p[0], None if n2 is None else n2[0]) if want_p else out[0]
    bias = case.bias.double().view(3, heads, hd)
    tok = window_tokens(dev)
    pad = tok < 0
    g = tok.clamp_min(0)
    padx = pad[..., None]
    qw_ = torch.where(padx, bias[0, h], q[g])
    kw_ = torch.where(padx, bias[1, h], k[g])
    vw_ = torch.where(padx, bias[2, hv_], v[g])
    if mutant == "pad_zero":
        kw_, vw_ = torch.where(padx, 0.0, kw_), torch.where(padx, 0.0, vw_)
    if mutant == "pad_clamped":
        gc = window_tokens(dev, clamped=True)
        kw_, vw_ = k[gc], v[gc]
    ih, iw = rel_index(WS, dev)
    mask = norel = None
    if mutant == "pad_masked":
        mask = pad
    if mutant == "pad_no_rel":
        norel = pad
    if mutant in ("tile_first", "tile_last", "tile7"):
        mask = torch.zeros_like(pad)
        mask[:, {"tile_first": slice(0, 2 * WS), "tile_last": slice(NTOK - 2 * WS, NTOK), "tile7": slice(192, NTOK)}[mutant]] = True
    if mutant == "v_swap4":
        s = torch.arange(NTOK, device=dev)
        kw4 = (s % WS) ^ 4
        vw_ = vw_[:, torch.where(kw4 < WS, (s // WS) * WS + kw4, s)]
    if mutant == "dead_cols":       # 28 more keys per window: the bias rows, the key row's rel_h term, no rel_w term (a zero table row)
        kh = torch.arange(WS, device=dev).repeat_interleave(2)
        nw = NWIN * NWIN
        kw_ = torch.cat([kw_, bias[1, h].expand(nw, 2 * WS, hd)], 1)
        vw_ = torch.cat([vw_, bias[2, hv_].expand(nw, 2 * WS, hd)], 1)
        qh = torch.arange(NTOK, device=dev) // WS
        ih = torch.cat([ih, qh[:, None] - kh[None, :] + WS - 1], 1)
        iw = torch.cat([iw, torch.full((NTOK, 2 * WS), 2 * WS - 1, device=dev, dtype=torch.long)], 1)
        Rw = torch.cat([Rw, torch.zeros(1, hd, dtype=Rw.dtype, device=dev)])
        Rh = torch.cat([Rh, torch.zeros(1, hd, dtype=Rh.dtype, device=dev)])
    ow, p, n2w = attend(qw_, kw_, vw_, hd, (Rh, Rw, ih, iw), emu, mutant, mask, norel)
    out = torch.empty(T, hd, dtype=torch.float64, device=dev)
    out[tok[~pad]] = ow[~pad]
    if not want_p:
        return out
    n2 = None
    if n2w is not None:
        n2 = torch.empty(T, dtype=torch.float64, device=dev)
        n2[tok[~pad]] = n2w[~pad]
    return out, p, n2


def plain_item(case, b, h, emu=None, mutant=None, want_p=False):
    """One (image, head) of the plain form -> out [nq, hd] float64 (want_p: and P [nq, nk], p_noise2 [nq])."""
    hd, dev = case.hd, case.q.device
    bk_, hv_ = (0 if mutant == "image_k0" else b), (0 if mutant == "head_v0" else h)
    q, k, v = case.q[b, :, h].double(), case.k[bk_, :, h].double(), case.v[b, :, hv_].double()
    mask = _tile_mask(case.nk, 1, mutant == "tile_first", dev) if mutant in ("tile_first", "tile_last") else None
    if mutant == "v_swap4":
        v = v[_swap4(case.nk, dev)]
    out, p, n2 = attend(q[None], k[None], v[None], hd, None, emu, mutant, mask)
    return (out[0], p[0], None if n2 is None else n2[0]) if want_p else out[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _codes(L, n, gen):
    """[L, n] code book: unit vectors where they fit, else +-1."""
    if L <= n:
        return torch.eye(L, n)
    return torch.randint(0, 2, (L, n), generator=gen).float() * 2 - 1


def pair_partner(codes: torch.Tensor) -> torch.Tensor:
    """margin[i, j] of +-1 (or unit) codes: with a query carrying code i + code j, the designated rows' score minus the best third
    row's: (n + G_ij) - max_r (G_ir + G_jr)."""
    G = codes @ codes.t()
    L = G.shape[0]
    s = G[:, None, :] + G[None, :, :]
    eye = torch.eye(L, dtype=torch.bool)
    s = s.masked_fill(eye[:, None, :] | eye[None, :, :], float("-inf"))
    return (G.diagonal()[:, None] + G - s.amax(-1)).masked_fill(eye, float("-inf"))


def make_encoder_case(kind, window, B, heads, hd, prec, seed=0):
    """kind: select / pair / pads (window only) / diffuse.  Tensors on the CPU: qkv [B * 4096, 3 D] of the 16-bit type, bias [3 D],
    rel_h / rel_w [2 S - 1, hd] fp32 holding 16-bit-representable values, target [B, heads, 4096, T] or None."""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * (kind == "pair") + 10 * bool(window) + hd)
    S = WS if window else GRID
    L, half, form = 2 * S - 1, hd // 2, "window" if window else "global"
    rn = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = torch.zeros(B, T, heads, hd), torch.zeros(B, T, heads, hd), rn(B, T, heads, hd)
    bias = torch.zeros(3, heads, hd)
    target = None
    if kind == "diffuse":
        q, k = rn(B, T, heads, hd), rn(B, T, heads, hd)
        bias = rn(3, heads, hd) * 0.5 if window else bias
        rel_h, rel_w = rn(L, hd) * 0.3, rn(L, hd) * 0.3
    else:
        amp = AMP[(form, kind)]
        ch, cw = _codes(L, half, gen), _codes(L, half, gen)
        rel_h, rel_w = torch.zeros(L, hd), torch.zeros(L, hd)
        rel_h[:, :half], rel_w[:, half:] = amp * ch, amp * cw
        k = K_NOISE * rn(B, T, heads, hd)
        bias[0], bias[1], bias[2] = 0.5 * rn(heads, hd), K_NOISE * rn(heads, hd), rn(heads, hd)
    if kind == "pads":
        F = free_dims(hd)
        q = 0.02 * rn(B, T, heads, hd)
        q[..., F] += 1.0
        k = 0.02 * rn(B, T, heads, hd)
        bias[1] = 0.0
        bias[1][:, F] = -0.2 / (len(F) * hd ** -0.5)
        bias[2] = 3.0 * (1 - 2 * (torch.arange(hd) % 2)).float().expand(heads, hd)
    if kind in ("select", "pair"):
        nt = 1 if kind == "select" else 2
        target = torch.empty(B, heads, T, nt, dtype=torch.long)
        if window:
            tok = window_tokens()
            real = tok >= 0
            nreal = real.sum(1)
            j = real.cumsum(1) - 1
            s = torch.arange(NTOK)[None, :].expand(NWIN * NWIN, NTOK)
            for h in range(heads):
                perm = torch.stack([torch.randperm(NTOK, generator=gen) for _ in range(NWIN * NWIN)])
                for b in range(B):
                    arg = (j + b * nreal[:, None] + 5 * b * (nreal[:, None] == NTOK)) % NTOK
                    t = perm.gather(1, arg)
                    ih_, iw_ = s // WS - t // WS + WS - 1, s % WS - t % WS + WS - 1
                    rows, n = tok[real], int(real.sum())
                    qr, ar = torch.zeros(n, hd), torch.arange(n)
                    qr[ar, ih_[real]] = amp
                    qr[ar, half + iw_[real]] = amp
                    target[b, h, rows, 0] = t[real]
                    if kind == "pair":
                        kw2 = (t % WS + 1 + j % (WS - 1)) % WS
                        qr[ar, half + (s % WS - kw2 + WS - 1)[real]] += amp
                        target[b, h, rows, 1] = ((t // WS) * WS + kw2)[real]
                    q[b, rows, h] = qr
        else:
            tq = torch.arange(T)
            qh, qw = tq // GRID, tq % GRID
            margin = pair_partner(cw) if kind == "pair" else None
            for b in range(B):
                for h in range(heads):
                    pa, pb = torch.randperm(GRID, generator=gen), torch.randperm(GRID, generator=gen)
                    kh = (qh + pa[qw]) % GRID
                    kw = (qw + pb[kh]) % GRID
                    ih_, iw_ = qh - kh + GRID - 1, qw - kw + GRID - 1
                    qr = torch.cat([amp * ch[ih_], amp * cw[iw_]], 1)
                    target[b, h, :, 0] = kh * GRID + kw
                    if kind == "pair":
                        r = torch.arange(L)[None, :]
                        ok = (r >= qw[:, None]) & (r <= qw[:, None] + GRID - 1)      # rows whose key column qw + 63 - r exists
                        iw2 = margin[iw_].masked_fill(~ok, float("-inf")).argmax(1)
                        qr[:, half:] += amp * cw[iw2]
                        target[b, h, :, 1] = kh * GRID + (qw + GRID - 1 - iw2)
                    q[b, :, h] = qr
    D = heads * hd
    qkv = torch.stack([q, k, v], 2).reshape(B * T, 3 * D).to(DT16[prec])
    r16 = lambda t: t.to(DT16[prec]).float()
    return SimpleNamespace(form=form, kind=kind, window=window, B=B, heads=heads, hd=hd, prec=prec, nq=T, nk=T, qkv=qkv,
                           bias=r16(bias.reshape(3 * D)), rel_h=r16(rel_h), rel_w=r16(rel_w), target=target)


def plain_amp(hd):
    return {16: 4.0, 32: 3.0}.get(hd, 2.0)


def make_plain_case(kind, B, heads, hd, nq, nk, prec, seed=0):
    """kind: select / pair / diffuse; prec fp16 / bf16 / fp32.  q [B, nq, heads, hd], k / v [B, nk, heads, hd] of that type (CPU)."""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * (kind == "pair") + hd + 7 * nq + 13 * nk)
    rn = lambda *s: torch.randn(*s, generator=gen)
    v, target = rn(B, nk, heads, hd), None
    if kind == "diffuse":
        q, k = rn(B, nq, heads, hd), rn(B, nk, heads, hd)
    else:
        a = plain_amp(hd)
        q, k = torch.empty(B, nq, heads, hd), torch.empty(B, nk, heads, hd)
        target = torch.empty(B, heads, nq, 1 if kind == "select" else 2, dtype=torch.long)
        perm, offs = torch.randperm(nk, generator=gen), set()
        for b in range(B):
            for h in range(heads):
                if hd == 16:                                               # distinct sign vectors
                    bits = torch.randperm(1 << hd, generator=gen)[:nk]
                    codes = ((bits[:, None] >> torch.arange(hd)[None, :]) & 1).float() * 2 - 1
                else:
                    codes = torch.randint(0, 2, (nk, hd), generator=gen).float() * 2 - 1
                off = (b * heads + h) * nq                                 # the first ceil(nk / nq) items tile the keys
                while off >= nk and off % nk in offs:
                    off += 1
                offs.add(off % nk)
                t = perm[(torch.arange(nq) + off) % nk]
                k[b, :, h] = a * codes
                q[b, :, h] = a * codes[t]
                target[b, h, :, 0] = t
                if kind == "pair":
                    G = codes[t] @ codes.t()
                    G[torch.arange(nq), t] = float("-inf")
                    t2 = G.argmax(1)
                    q[b, :, h] += a * codes[t2]
                    target[b, h, :, 1] = t2
    dt = torch.float32 if prec == "fp32" else DT16[prec]
    return SimpleNamespace(form="plain", kind=kind, window=0, B=B, heads=heads, hd=hd, prec=prec, nq=nq, nk=nk,
                           q=q.to(dt), k=k.to(dt), v=v.to(dt), target=target)


def case_to(case, dev):
    out = SimpleNamespace(**vars(case))
    for name, val in vars(case).items():
        if torch.is_tensor(val):
            setattr(out, name, val.to(dev))
    return out


def item(case, b, h, **kw):
    return plain_item(case, b, h, **kw) if case.form == "plain" else enc_item(case, b, h, **kw)


def emu_of(case):
    return "f32" if case.prec == "fp32" else (case.prec, den_rounded(case.hd))


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage conditions: figures of the REFERENCE alone
# ---------------------------------------------------------------------------------------------------------------------------------
def designated_mass(case, b, h, p):
    """[nq (real queries), T]: the oracle's mass on each designated key of every query of item (b, h); p from item(want_p=True)."""
    tg = case.target[b, h]
    if case.form == "window":
        win, slot = token_slots(p.device)
        return p[win, slot].gather(1, tg)
    return p.gather(1, tg)


def pad_share(case, p):
    """(share [n], n) the oracle's mass on padded keys for every real query of the nine edge windows."""
    pad = window_tokens(p.device) < 0
    share = (p * pad[:, None, :]).sum(-1)                       # [25, 196]
    edge = pad.any(1)
    return share[edge][~pad[edge]]


def target_coverage(case):
    """Counts that the conditions name.  window: (key slots of the 25 x 196 that are nobody's target, unused rows of rel_h, rel_w);
    global: ((image, head) maps that are not permutations, unused rows ...); plain: (keys that are nobody's target,)."""
    tg = case.target
    B, heads = case.B, case.heads
    if case.form == "window":
        win, slot = token_slots()
        hit = torch.zeros(NWIN * NWIN, NTOK, dtype=torch.bool)
        uh, uw = torch.zeros(2 * WS - 1, dtype=torch.bool), torch.zeros(2 * WS - 1, dtype=torch.bool)
        for t in range(tg.shape[-1]):
            ts = tg[..., t]                                                        # [B, heads, 4096]
            hit[win.expand_as(ts), ts] = True
            uh[(slot // WS).expand_as(ts) - ts // WS + WS - 1] = True
            uw[(slot % WS).expand_as(ts) - ts % WS + WS - 1] = True
        return int((~hit).sum()), int((~uh).sum()), int((~uw).sum())
    if case.form == "global":
        tq = torch.arange(T)
        notperm = sum(int(tg[b, h, :, 0].unique().numel() != T) for b in range(B) for h in range(heads))
        uh, uw = torch.zeros(2 * GRID - 1, dtype=torch.bool), torch.zeros(2 * GRID - 1, dtype=torch.bool)
        for t in range(tg.shape[-1]):
            ts = tg[..., t]
            uh[(tq // GRID).expand_as(ts) - ts // GRID + GRID - 1] = True
            uw[(tq % GRID).expand_as(ts) - ts % GRID + GRID - 1] = True
        return notperm, int((~uh).sum()), int((~uw).sum())
    hit = torch.zeros(case.nk, dtype=torch.bool)
    hit[tg.flatten()] = True
    return (int((~hit).sum()),)


def maps_differ(case) -> bool:
    """No two (image, head) items share a target map."""
    flat = case.target[..., 0].reshape(case.B * case.heads, -1)
    return all(not torch.equal(flat[i], flat[j]) for i in range(len(flat)) for j in range(i))


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics and bars
# ---------------------------------------------------------------------------------------------------------------------------------
def row_sums(got, ref):
    """(sum err^2, sum ref^2) per query over the channels, float64."""
    got, ref = got.double(), ref.double()
    return (got - ref).pow(2).sum(-1), ref.pow(2).sum(-1)


def floor2(ref, prec):
    """Per query: (one ulp of the output type at the row's largest reference magnitude)^2."""
    return ulp(ref.double().abs().amax(-1), prec).pow(2)


def groups(case, dev="cpu"):
    """{metric: group id per (image, head, query) [B, heads, nq]}; no query is left out of any."""
    B, heads, nq = case.B, case.heads, case.nq
    b = torch.arange(B, device=dev)[:, None, None].expand(B, heads, nq)
    h = torch.arange(heads, device=dev)[None, :, None].expand(B, heads, nq)
    qi = torch.arange(nq, device=dev)[None, None, :].expand(B, heads, nq)
    item_ = b * heads + h
    g = {"query": item_ * nq + qi, "head": h, "image": b, "all": torch.zeros_like(b)}
    if case.form == "window":
        win, _ = token_slots(dev)
        g["window"] = item_ * (NWIN * NWIN) + win[None, None, :]
    if case.target is not None:
        t0 = case.target[..., 0].to(dev)
        tile = t0 // (2 * WS) if case.form == "window" else t0 // 64
        g["tile"] = item_ * 64 + tile
    return g


def _group_rel(num, den, gid):
    n = int(gid.max()) + 1
    a = torch.zeros(n, dtype=torch.float64, device=num.device).index_add_(0, gid.flatten(), num.flatten())
    d = torch.zeros(n, dtype=torch.float64, device=num.device).index_add_(0, gid.flatten(), den.flatten())
    cnt = torch.zeros(n, dtype=torch.float64, device=num.device).index_add_(0, gid.flatten(), torch.ones_like(num.flatten()))
    return torch.sqrt(a / d), cnt > 0, d


def unit_roundoff(prec):
    return 2.0 ** -(MANT[prec] + 1)


def noise2(n2, prec):
    """The squared P-rounding term of a query's bar, absolute: u^2 p_noise2 (module docstring)."""
    return unit_roundoff(prec) ** 2 * n2


def bar16(emu, floor, noise, hd, prec):
    """The 16-bit bar of one figure from the emulation's figure, the P-rounding term and the floor (module docstring)."""
    u = 0.0 if den_rounded(hd) else unit_roundoff(prec)
    return torch.maximum(BAR_FACTOR * emu + noise + u, floor)


def bar32(emu, floor):
    return torch.maximum(FP32_BAR_FACTOR * emu.max(), floor)


def evaluate(case, e2, e2_emu, r2, f2, t2=None):
    """e2 / e2_emu / r2 / f2 / t2 [B, heads, nq]: the kernel's and the emulation's squared row errors, the squared reference row
    norms, the squared ulp floors, the squared P-rounding terms (noise2; 16-bit cases).  -> ({metric: (worst figure, its bar, group
    id)}, excluded count); the worst group is the one highest over its bar."""
    out, excluded = {}, 0
    for name, gid in groups(case, e2.device).items():
        got, used, d = _group_rel(e2, r2, gid)
        emu, _, _ = _group_rel(e2_emu, r2, gid)
        floor, _, _ = _group_rel(f2, r2, gid)
        excluded += int((used & ~(d > 0)).sum())
        got, emu, floor = got[used], emu[used], floor[used]
        if case.prec == "fp32":
            bar = bar32(emu, floor)
        else:
            bar = bar16(emu, floor, _group_rel(t2, r2, gid)[0][used], case.hd, case.prec)
        ratio = torch.where(torch.isfinite(got), got / bar, torch.full_like(got, float("inf")))
        j = int(ratio.argmax())
        out[name] = (got[j].item(), bar[j].item(), int(torch.nonzero(used).flatten()[j]))
    return out, excluded


def line(name, ev):
    return f"{name}: " + "  ".join(f"{k} {v[0]:.2e} ({v[1]:.1e})" for k, v in ev.items())


def over(ev):
    return {k: v for k, v in ev.items() if not v[0] <= v[1]}


def worst_ratio(ev):
    k = max(ev, key=lambda m: ev[m][0] / ev[m][1] if ev[m][1] > 0 else float("inf"))
    return k, ev[k][0] / ev[k][1]


def describe_query(case, gid, got_row, vrows):
    """The failing query's (image, head, query), its target, and the key whose value row is nearest to what the kernel returned."""
    nq = case.nq
    it, qi = gid // nq, gid % nq
    near = int((vrows.double() - got_row.double()[None, :]).norm(dim=1).argmin())
    tg = None if case.target is None else case.target[it // case.heads, it % case.heads, qi].tolist()
    return f"image {it // case.heads} head {it % case.heads} query {qi} target {tg} nearest value row {near}"
