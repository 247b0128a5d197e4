// The image encoder: FFT front, stem, HFC adaptor, transformer blocks (residual-stream state machine), neck.
#pragma once
#include "fft_kernels.h"
#include "host_attn.h"
#include "host_gemm.h"
#include "host_norm.h"
#include "host_weights.h"

namespace {

int tap_alloc(wm_handle* h) {
    if (!h->tap_buf) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, (size_t)h->maxB * T * h->D * 4));
        h->tap_buf = (float*)p;
    }
    return 0;
}
int do_tap(wm_handle* h, hipStream_t s, int which, int batch, const float* src = nullptr) {
    if (h->tap_which != which) return 0;
    WM_TRY(tap_alloc(h));
    HIP_TRY(hipMemcpyAsync(h->tap_buf, src ? src : h->resid, (size_t)batch * T * h->D * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

int fft_impl(wm_handle* h, const float* x, float* out, int B, hipStream_t s, bool copies16 = false) {
    WM_TRY(launch_simple(h, s, (double)B * (12e6 + 3e6), fft_rows_fwd_kernel, dim3(FFT_N, B), dim3(256), x, h->fftR, (const float2*)h->fft_tw));
    WM_TRY(launch_simple(h, s, (double)B * 6e6, fft_cols_kernel, dim3(FFT_L, B), dim3(256), h->fftR, (const float2*)h->fft_tw));
    // copies16: the last pass also leaves fp16 NCHW copies of x and of the result in p16 / h16 (the patch embeds' operands)
    WM_TRY(launch_simple(h, s, (double)B * (12e6 + 3e6 + 4e6 + (copies16 ? 8e6 : 0.0)), fft_rows_inv_kernel<FP16>, dim3(FFT_N, B), dim3(256), x, (const float2*)h->fftR,
                         (const float2*)h->fft_tw, out, copies16 ? (u16*)h->p16 : (u16*)nullptr, copies16 ? (u16*)h->h16 : (u16*)nullptr));
    return 0;
}

int encoder_impl(wm_handle* h, const float* x, const float* hfc, float* out_nchw, int B, hipStream_t s, bool have16 = false) {
    const int D = h->D, M = B * T;
    const int PS = WM_PREC_FP16;      // stem, HFC adaptor and neck: fp16 operands in every mode (see is_stem_or_neck)
    const std::string e = "image_encoder.", a = e + "hfc_attn.";
    // ---- stem: patch / HFC embeds (image_encoder.py:124-128) ----
    // the embeds read 16-bit NCHW copies of x and hfc (p16, h16) -- left there by the FFT's last pass (wm_forward) or made here --
    // through the implicit-GEMM loader (gemm16_v3.h ALoad::PatchEmbed): no im2col buffer
    if (!have16) {
        WM_TRY(launch_simple(h, s, B * 18.9e6, cvt_f32_to_16_kernel<FP16>, dim3(grid_for((int64_t)B * 3 * 1024 * 256)), dim3(256), x, (u16*)h->p16, (int64_t)B * 3 * 1024 * 256));
        WM_TRY(launch_simple(h, s, B * 6.3e6, cvt_f32_to_16_kernel<FP16>, dim3(grid_for((int64_t)B * 1024 * 256)), dim3(256), hfc, (u16*)h->h16, (int64_t)B * 1024 * 256));
    }
    // t = patch_embed(x) + pos_embed  -> tokbase (fp32) and xn16 (16-bit copy for proj_patch)
    WM_TRY(launch_patch_embed16(h, s, PS, h->p16, W16(h, e + "patch_embed.proj.weight"), W32(h, e + "patch_embed.proj.bias"),
                                W32(h, e + "pos_embed"), T, h->tokbase, h->xn16, B, D, 3));
    WM_TRY(do_tap(h, s, -3, B, h->tokbase));
    WM_TRY(launch_patch_embed16(h, s, PS, h->h16, W16(h, e + "hfc_embed.proj.weight"), W32(h, e + "hfc_embed.proj.bias"),
                                nullptr, 0, nullptr, h->he16, B, HFC, 1));
    // ---- HFC adaptor (image_encoder.py:486-516) ----
    WM_TRY(launch_gemm16(h, s, PS, h->he16, W16(h, a + "proj_hfc.weight"), W32(h, a + "proj_hfc.bias"),
                         W32(h, a + "pos_embed"), T, nullptr, h->hp16, M, HFC, HFC, ACT_NONE, GX(W16P(h, a + "proj_hfc.weight"))));                    // :494
    WM_TRY(launch_gemm16(h, s, PS, h->xn16, W16(h, a + "proj_patch.weight"), W32(h, a + "proj_patch.bias"),
                         nullptr, 0, h->pt32, h->pt16, M, HFC, D, ACT_NONE, GX(W16P(h, a + "proj_patch.weight"))));                                       // :495
    const uint16_t* wi = W16(h, a + "cross_attn.in_proj_weight");
    const uint16_t* wip = W16P(h, a + "cross_attn.in_proj_weight");      // same element offsets: 16 rows x K are one contiguous block in both layouts
    const float* bi = W32(h, a + "cross_attn.in_proj_bias");
    WM_TRY(launch_gemm16(h, s, PS, h->pt16, wi, bi, nullptr, 0, nullptr, h->q16, M, HFC, HFC, ACT_NONE, GX(wip)));
    WM_TRY(launch_gemm16(h, s, PS, h->hp16, wi + (size_t)HFC * HFC, bi + HFC, nullptr, 0, nullptr, h->kv16, M, 2 * HFC, HFC, ACT_NONE, GX(wip ? wip + (size_t)HFC * HFC : nullptr)));
    WM_TRY(launch_mha16(h, s, PS, h->q16, HFC, h->kv16, 2 * HFC, h->kv16 + HFC, 2 * HFC, h->aoh16, HFC, B, HFC_HEADS,
                        HFC / HFC_HEADS, T, T, 1));                                                                      // :500-503
    WM_TRY(launch_gemm16(h, s, PS, h->aoh16, W16(h, a + "cross_attn.out_proj.weight"), W32(h, a + "cross_attn.out_proj.bias"),
                         h->pt32, 0, h->y1, nullptr, M, HFC, HFC, ACT_NONE, GX(W16P(h, a + "cross_attn.out_proj.weight"))));                                       // + residual :504
    WM_TRY(launch_layernorm(h, s, PS, h->y1, W32(h, a + "norm1.weight"), W32(h, a + "norm1.bias"), 1e-5f, h->y1n32, h->y1n16, M, HFC));
    WM_TRY(launch_gemm16(h, s, PS, h->y1n16, W16(h, a + "linear1.weight"), W32(h, a + "linear1.bias"), nullptr, 0, nullptr,
                         h->h1_16, M, HFC, HFC, ACT_RELU, GX(W16P(h, a + "linear1.weight"))));
    WM_TRY(launch_gemm16(h, s, PS, h->h1_16, W16(h, a + "linear2.weight"), W32(h, a + "linear2.bias"), h->y1n32, 0, h->z32,
                         nullptr, M, HFC, HFC, ACT_NONE, GX(W16P(h, a + "linear2.weight"))));                                                          // :506-508
    WM_TRY(launch_layernorm(h, s, PS, h->z32, W32(h, a + "norm2.weight"), W32(h, a + "norm2.bias"), 1e-5f, nullptr, h->y2_16, M, HFC));
    // scramble (:512): per tile [4096 tok,1024 ch] re-read as [1024, 4096]; make it the K-contiguous A operand
    WM_TRY(launch_simple(h, s, B * 16.8e6, transpose16_kernel, dim3(T / 64, HFC / 64, B), dim3(256), (const u16*)h->y2_16, (u16*)h->y2t16, HFC, T));
    // x = proj_back(scrambled) + t   (:513-514, :131)
    // Folded LayerNorm (WM_CFG_FOLD_LN; gemm16_v5.h "Folded LayerNorm"): a block whose qkv and lin1 run the 256-row-tile
    // 16-bit kernel takes its two LayerNorms inside those GEMMs.  raw_prec: the 16-bit type in which xn16 holds the copy of the
    // CURRENT residual stream (LDS-image order) with fold_stats its per-row partial statistics, or -1.
    auto fold_block = [&](int i) {
        const int pb = block_prec(h, i);
        const std::string b = e + "blocks." + std::to_string(i) + ".";
        return h->fold && (pb == WM_PREC_FP16 || (pb == WM_PREC_BF16 && h->fold_bf16)) && gemm16_takes_v5(M, 3 * D, D) && gemm16_takes_v5(M, 4 * D, D) &&
               h->wfold.count(b + "attn.qkv.weight") && h->wfold.count(b + "mlp.lin1.weight");
    };
    // Where the residual stream lives.  st_split: as the two 16-bit planes (xn16 = hi of type raw_prec, lo16), fp32 `resid` stale;
    // otherwise in `resid` (fp32), with xn16 / fold_stats its hi plane and statistics iff raw_prec >= 0.  The split form is used by
    // a call whose residual GEMMs run the 256-row-tile kernel (4+ tiles for ViT-H); a smaller call keeps fp32 and rounds the stream
    // to hi + lo in ln_stats_x16_kernel, so both forms carry the same values bit for bit (gemm16_v5.h "Split stream").
    const bool split_call = h->split && gemm16_takes_v5(M, D, D) && gemm16_takes_v5(M, D, 4 * D);
    // st_rows (fp8 blocks): as two planes of rows (x16last = hi bf16, lo16; columns at plane_pos), `resid` stale (gemm8.h PLANES).
    bool st_split = false, st_rows = false;
    int raw_prec = -1;
    auto to_fp32 = [&]() -> int {                           // planes -> resid (type boundaries, non-folded blocks, the bf16 neck input)
        if (st_split) WM_TRY(launch_stream_merge(h, s, raw_prec, h->xn16, h->lo16, h->resid, M, D));
        if (st_rows) WM_TRY(launch_stream_rows(h, s, WM_PREC_BF16, h->resid, h->x16last, h->lo16, M, D, true));
        st_split = st_rows = false;
        return 0;
    };
    auto planes_from_fp32 = [&](int P) -> int {             // resid -> statistics + planes of type P (resid rounded in place unless the call is split)
        WM_TRY(to_fp32());
        WM_TRY(launch_ln_stats16(h, s, P, h->resid, h->fold_stats, h->xn16, M, D, h->lo16, split_call ? nullptr : h->resid, h->overflow));
        raw_prec = P;
        st_split = split_call;
        return 0;
    };
    auto tap = [&](int which) -> int {
        if (h->tap_which != which) return 0;
        if (!st_split && !st_rows) return do_tap(h, s, which, B);
        WM_TRY(tap_alloc(h));
        if (st_rows) return launch_stream_rows(h, s, WM_PREC_BF16, h->tap_buf, h->x16last, h->lo16, M, D, true);
        return launch_stream_merge(h, s, raw_prec, h->xn16, h->lo16, h->tap_buf, M, D);
    };
    // a residual GEMM of a folded block of type P: x += A W^T + b, leaving the stream with planes + statistics of type P
    auto residual_gemm = [&](int P, const void* A, const std::string& wn, int K, int a_packed) -> int {
        GemmExtra x = GX(W16P(h, wn + ".weight"), a_packed);
        if (st_split) {                                     // planes in, planes out (in place), statistics out
            x.st_stats = h->fold_stats; x.res_hi = h->xn16; x.res_lo = h->lo16; x.out_lo = h->lo16; x.overflow = h->overflow;
            return launch_gemm16(h, s, P, A, W16(h, wn + ".weight"), W32(h, wn + ".bias"), nullptr, 0, nullptr, h->xn16, M, D, K, ACT_NONE, x);
        }
        const bool v5 = gemm16_takes_v5(M, D, K);
        if (v5 && !h->split) {                              // fp32 stream (WM_STREAM_SPLIT=0): statistics + 16-bit copy from the GEMM, as in round 3
            x.st_stats = h->fold_stats;
            WM_TRY(launch_gemm16(h, s, P, A, W16(h, wn + ".weight"), W32(h, wn + ".bias"), h->resid, 0, h->resid, h->xn16, M, D, K, ACT_NONE, x));
            raw_prec = P;
            return 0;
        }
        // half-width launch (1-2 tiles per call), or a call whose proj and lin2 disagree about the kernel: fp32 in place, then the
        // standalone statistics kernel, which also rounds the stream to hi + lo
        WM_TRY(launch_gemm16(h, s, P, A, W16(h, wn + ".weight"), W32(h, wn + ".bias"), h->resid, 0, h->resid, nullptr, M, D, K, ACT_NONE, x));
        raw_prec = -1;
        return planes_from_fp32(P);
    };
    {
        GemmExtra xb = GX(W16P(h, a + "proj_back.weight"));
        const bool produce = fold_block(0) && block_prec(h, 0) == PS && gemm16_takes_v5(M, D, HFC) && (split_call || !h->split);
        if (produce) { xb.st_stats = h->fold_stats; xb.overflow = h->overflow; if (split_call) xb.out_lo = h->lo16; }
        WM_TRY(launch_gemm16(h, s, PS, h->y2t16, W16(h, a + "proj_back.weight"), W32(h, a + "proj_back.bias"), h->tokbase, 0,
                             (produce && split_call) ? nullptr : h->resid, produce ? h->xn16 : nullptr, M, D, HFC, ACT_NONE, xb));
        if (produce) { raw_prec = PS; st_split = split_call; }
    }
    WM_TRY(tap(-1));

    // ---- transformer blocks (image_encoder.py:188-204) ----
    // x = x + proj(attn(norm1 x)); x = x + lin2(gelu(lin1(norm2 x))).
    // Per GEMM the operand type is the block's (block_prec) or, in fp8 mode, e4m3 for the GEMMs the handle's fp8 mask names
    // (WM_FP8_QKV | WM_FP8_PROJ | WM_FP8_MLP; lin1 and lin2 go together because lin1's epilogue writes lin2's operand) and
    // bf16 for the rest and for attention.  Each producer writes its consumer's operand type directly (LayerNorm / attention /
    // GELU epilogue -> e4m3 bytes or 16-bit), so no conversion pass exists in any mix.
    bool xn_packed = false;                                 // xn16 (a LayerNorm's output) is in LDS-image order
    for (int i = 0; i < h->depth; ++i) {
        const std::string b = e + "blocks." + std::to_string(i) + ".";
        const int PB = block_prec(h, i);
        const bool f8 = PB == WM_PREC_FP8;
        const int P = f8 ? WM_PREC_BF16 : PB;               // 16-bit type of this block (attention, non-fp8 GEMMs)
        const bool q8 = f8 && (h->fp8_gemms & WM_FP8_QKV), p8 = f8 && (h->fp8_gemms & WM_FP8_PROJ), m8 = f8 && (h->fp8_gemms & WM_FP8_MLP);
        auto W8 = [&](const std::string& n) { return h->w8.at(n); };
        // Activations that feed a 16-bit GEMM on the 256-row-tile kernel are written in LDS-image order by their producer
        // (gemm16_v5.h "Operand layout"): norm1 -> qkv, norm2 -> lin1, lin1's GELU epilogue -> lin2.  (proj's operand, the
        // attention output, stays row-major: a head's 80 columns do not fall on the 32-column pieces.)
        const bool pk_qkv = !h->row_major && !q8 && gemm16_takes_v5(M, 3 * D, D), pk_lin1 = !h->row_major && !m8 && gemm16_takes_v5(M, 4 * D, D);
        const bool pk_lin2 = pk_lin1 && gemm16_takes_v5(M, D, 4 * D);
        if (fold_block(i)) {
            // ---- both LayerNorms folded: statistics (and the stream's hi plane = the operand) from the producing residual GEMM, or
            // from the standalone kernel where that one is a half-width launch or of another operand type; normalisation in the
            // consuming GEMM's epilogue ----
            auto folded = [&](const std::string& wn, int act, int out_packed, void* out, int N) {
                GemmExtra x = GX(h->wfold.at(wn), 1, out_packed);
                x.fold_stats = h->fold_stats; x.fold_c1 = h->fold_c1.at(wn); x.fold_eps = 1e-6f;
                return launch_gemm16(h, s, P, h->xn16, W16(h, wn), h->fold_c2.at(wn), nullptr, 0, nullptr, out, M, N, D, act, x);
            };
            if (raw_prec != P) WM_TRY(planes_from_fp32(P));
            WM_TRY(sat_check(h, s, WM_SAT_LN, h->xn16, (int64_t)M * D, P));
            WM_TRY(folded(b + "attn.qkv.weight", ACT_NONE, 0, h->qkv16, 3 * D));
            WM_TRY(sat_check(h, s, WM_SAT_QKV, h->qkv16, (int64_t)M * 3 * D, P));
            AttnExtra prescaled;
            prescaled.q_prescaled = 1;
            WM_TRY(launch_encoder_attention(h, s, P, h->qkv16, W32(h, b + "attn.qkv.bias"), W32(h, b + "attn.rel_pos_h"),
                                            W32(h, b + "attn.rel_pos_w"), h->ao16, B, h->heads, h->hd, h->is_global[i] ? 0 : 14, prescaled));
            WM_TRY(sat_check(h, s, WM_SAT_ATTN, h->ao16, (int64_t)M * D, P));
            WM_TRY(residual_gemm(P, h->ao16, b + "attn.proj", D, 0));
            WM_TRY(sat_check(h, s, WM_SAT_LN, h->xn16, (int64_t)M * D, P));
            WM_TRY(folded(b + "mlp.lin1.weight", ACT_GELU, pk_lin2, h->hid16, 4 * D));
            WM_TRY(sat_check(h, s, WM_SAT_HID, h->hid16, (int64_t)M * 4 * D, P));
            WM_TRY(residual_gemm(P, h->hid16, b + "mlp.lin2", 4 * D, pk_lin2));
            WM_TRY(tap(i));
            continue;
        }
        // a block whose four GEMMs take e4m3 keeps the stream as planes of rows: proj / lin2 move the same 8 bytes per element, the
        // two LayerNorm passes read the 2-byte hi plane instead of 4-byte rows (their e4m3 output has a 2^-4 step; hi is bf16, 2^-9)
        const bool rows_blk = h->rows8 && q8 && p8 && m8 && D % 256 == 0 && D >= 512 && D <= 1536 && h->w8k.count(b + "attn.qkv.weight") && h->w8k.count(b + "mlp.lin1.weight");
        if (rows_blk && !st_rows) {
            WM_TRY(to_fp32());
            WM_TRY(launch_stream_rows(h, s, P, h->resid, h->x16last, h->lo16, M, D, false));
            st_rows = true;
        } else if (!rows_blk) {
            WM_TRY(to_fp32());
        }
        raw_prec = -1;
        if (st_rows) WM_TRY(launch_layernorm_plane8(h, s, P, h->x16last, W32(h, b + "norm1.weight"), W32(h, b + "norm1.bias"), 1e-6f, h->xn16, M, D));
        else WM_TRY(launch_layernorm_block(h, s, q8 ? WM_PREC_FP8 : P, h->resid, W32(h, b + "norm1.weight"), W32(h, b + "norm1.bias"), 1e-6f, h->xn16, M, D, pk_qkv));
        xn_packed = pk_qkv;
        WM_TRY(sat_check(h, s, WM_SAT_LN, h->xn16, (int64_t)M * D, q8 ? WM_PREC_FP8 : P));
        if (q8)
            WM_TRY(launch_gemm8(h, s, P, h->xn16, st_rows ? h->w8k.at(b + "attn.qkv.weight") : W8(b + "attn.qkv.weight"), W32(h, b + "attn.qkv.weight.wscale"), W32(h, b + "attn.qkv.bias"),
                                nullptr, nullptr, h->qkv16, nullptr, M, 3 * D, D, ACT_NONE));
        else
            WM_TRY(launch_gemm16(h, s, P, h->xn16, W16(h, b + "attn.qkv.weight"), W32(h, b + "attn.qkv.bias"), nullptr, 0, nullptr,
                                 h->qkv16, M, 3 * D, D, ACT_NONE, GX(W16P(h, b + "attn.qkv.weight"), xn_packed)));
        WM_TRY(sat_check(h, s, WM_SAT_QKV, h->qkv16, (int64_t)M * 3 * D, P));
        // the attention kernels write their output as e4m3 when proj consumes e4m3
        AttnExtra to8;
        to8.q_prescaled = 1; to8.out8 = p8 ? h->ao8 : nullptr;
        WM_TRY(launch_encoder_attention(h, s, P, h->qkv16, W32(h, b + "attn.qkv.bias"), W32(h, b + "attn.rel_pos_h"),
                                        W32(h, b + "attn.rel_pos_w"), h->ao16, B, h->heads, h->hd, h->is_global[i] ? 0 : 14, to8));
        if (p8) WM_TRY(sat_check(h, s, WM_SAT_ATTN, h->ao8, (int64_t)M * D, WM_PREC_FP8));
        else WM_TRY(sat_check(h, s, WM_SAT_ATTN, h->ao16, (int64_t)M * D, P));
        if (st_rows) {
            WM_TRY(launch_gemm8(h, s, P, h->ao8, W8(b + "attn.proj.weight"), W32(h, b + "attn.proj.weight.wscale"), W32(h, b + "attn.proj.bias"),
                                nullptr, nullptr, nullptr, nullptr, M, D, D, ACT_NONE, h->x16last, h->lo16));
        } else if (p8) {
            WM_TRY(launch_gemm8(h, s, P, h->ao8, W8(b + "attn.proj.weight"), W32(h, b + "attn.proj.weight.wscale"), W32(h, b + "attn.proj.bias"),
                                h->resid, h->resid, nullptr, nullptr, M, D, D, ACT_NONE));
        } else {
            WM_TRY(launch_gemm16(h, s, P, h->ao16, W16(h, b + "attn.proj.weight"), W32(h, b + "attn.proj.bias"), h->resid, 0,
                                 h->resid, nullptr, M, D, D, ACT_NONE, GX(W16P(h, b + "attn.proj.weight"))));
        }
        if (st_rows) WM_TRY(launch_layernorm_plane8(h, s, P, h->x16last, W32(h, b + "norm2.weight"), W32(h, b + "norm2.bias"), 1e-6f, h->xn16, M, D));
        else WM_TRY(launch_layernorm_block(h, s, m8 ? WM_PREC_FP8 : P, h->resid, W32(h, b + "norm2.weight"), W32(h, b + "norm2.bias"), 1e-6f, h->xn16, M, D, pk_lin1));
        xn_packed = pk_lin1;
        WM_TRY(sat_check(h, s, WM_SAT_LN, h->xn16, (int64_t)M * D, m8 ? WM_PREC_FP8 : P));
        if (m8) {
            WM_TRY(launch_gemm8(h, s, P, h->xn16, st_rows ? h->w8k.at(b + "mlp.lin1.weight") : W8(b + "mlp.lin1.weight"), W32(h, b + "mlp.lin1.weight.wscale"), W32(h, b + "mlp.lin1.bias"),
                                nullptr, nullptr, nullptr, h->hid16, M, 4 * D, D, ACT_GELU));
            WM_TRY(sat_check(h, s, WM_SAT_HID, h->hid16, (int64_t)M * 4 * D, WM_PREC_FP8));
            if (st_rows)
                WM_TRY(launch_gemm8(h, s, P, h->hid16, W8(b + "mlp.lin2.weight"), W32(h, b + "mlp.lin2.weight.wscale"), W32(h, b + "mlp.lin2.bias"),
                                    nullptr, nullptr, nullptr, nullptr, M, D, 4 * D, ACT_NONE, h->x16last, h->lo16));
            else
                WM_TRY(launch_gemm8(h, s, P, h->hid16, W8(b + "mlp.lin2.weight"), W32(h, b + "mlp.lin2.weight.wscale"), W32(h, b + "mlp.lin2.bias"),
                                    h->resid, h->resid, nullptr, nullptr, M, D, 4 * D, ACT_NONE));
        } else {
            WM_TRY(launch_gemm16(h, s, P, h->xn16, W16(h, b + "mlp.lin1.weight"), W32(h, b + "mlp.lin1.bias"), nullptr, 0, nullptr,
                                 h->hid16, M, 4 * D, D, ACT_GELU, GX(W16P(h, b + "mlp.lin1.weight"), xn_packed, pk_lin2)));
            WM_TRY(sat_check(h, s, WM_SAT_HID, h->hid16, (int64_t)M * 4 * D, P));
            WM_TRY(launch_gemm16(h, s, P, h->hid16, W16(h, b + "mlp.lin2.weight"), W32(h, b + "mlp.lin2.bias"), h->resid, 0,
                                 h->resid, nullptr, M, D, 4 * D, ACT_NONE, GX(W16P(h, b + "mlp.lin2.weight"), pk_lin2)));
        }
        WM_TRY(tap(i));
    }

    // ---- neck (image_encoder.py:105-121,136) ----
    // the neck's operand is fp16(x).  With the split stream and fp16 blocks that is the hi plane itself (LDS-image order: the
    // 256-row-tile kernel takes it as it is, a half-width launch gets it unpacked); otherwise fp16 of the fp32 stream.
    const void* neck_a = h->x16last;
    int neck_packed = 0;
    if (h->split && raw_prec == PS) {
        if (gemm16_takes_v5(M, OUTC, D)) { neck_a = h->xn16; neck_packed = 1; }
        else WM_TRY(launch_simple(h, s, B * 21.0e6, unpack16_lds_image_kernel, dim3(grid_for((int64_t)M * D / 8)), dim3(256), (const uint4*)h->xn16, (uint4*)h->x16last, (int64_t)M, D));
    } else if (st_rows) {                                   // the fp8 blocks' planes: one pass to fp16 rows (hid16 is free after the last block)
        neck_a = h->hid16;
        WM_TRY(launch_simple(h, s, B * 31.5e6, stream_rows_to_fp16_kernel<BF16>, dim3(grid_for((int64_t)M * D / 4)), dim3(256), (const u16*)h->x16last, (const u16*)h->lo16,
                             (u16*)h->hid16, (int64_t)M * D / 4, D));
        st_rows = false;
    } else {
        WM_TRY(to_fp32());
        WM_TRY(launch_simple(h, s, B * 31.5e6, cvt_f32_to_16_kernel<FP16>, dim3(grid_for((int64_t)M * D / 4)), dim3(256), (const float*)h->resid, (u16*)h->x16last, (int64_t)M * D / 4));
    }
    WM_TRY(sat_check(h, s, WM_SAT_LAST, neck_a, (int64_t)M * D, PS));
    WM_TRY(launch_gemm16(h, s, PS, neck_a, W16(h, e + "neck.0.weight"), nullptr, nullptr, 0, h->n1, nullptr, M, OUTC, D, ACT_NONE, GX(W16P(h, e + "neck.0.weight"), neck_packed)));
    WM_TRY(launch_layernorm(h, s, PS, h->n1, W32(h, e + "neck.1.weight"), W32(h, e + "neck.1.bias"), 1e-6f, nullptr, h->n1n16, M, OUTC));
    WM_TRY(launch_conv3x3_16(h, s, PS, h->n1n16, W16(h, e + "neck.2.weight"), h->n2, M, OUTC, OUTC));
    WM_TRY(launch_layernorm(h, s, PS, h->n2, W32(h, e + "neck.3.weight"), W32(h, e + "neck.3.bias"), 1e-6f, h->emb_nhwc, nullptr, M, OUTC));
    if (out_nchw)
        WM_TRY(launch_simple(h, s, B * 8.4e6, transpose32_kernel, dim3(OUTC / 64, T / 64, B), dim3(256), (const float*)h->emb_nhwc, out_nchw, T, OUTC));
    return 0;
}

}  // namespace
