// The box decoder (two-way transformer + heads) on fp32 buffers, and the whole path of wm_forward.
#pragma once
#include "dec_kernels.h"
#include "host_encoder.h"

namespace {

// attention block of the decoder (transformer.py:217-240) on fp32 buffers
struct DecAttnW { const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo; int internal; };

DecAttnW dec_w(wm_handle* h, const std::string& p, int internal) {
    return DecAttnW{W32(h, p + "q_proj.weight"), W32(h, p + "q_proj.bias"), W32(h, p + "k_proj.weight"), W32(h, p + "k_proj.bias"),
                    W32(h, p + "v_proj.weight"), W32(h, p + "v_proj.bias"), W32(h, p + "out_proj.weight"), W32(h, p + "out_proj.bias"), internal};
}

int decoder_impl(wm_handle* h, const float* keys_nhwc, float* logits, float* boxes, int B, hipStream_t s) {
    const std::string t = "mask_decoder.transformer.";
    const int E = OUTC, Mk = B * T, Mq = B * NQ;
    const float* tok = W32(h, "mask_decoder.mask_tokens.weight");      // [51,256] = tokens and query PE (box_decoder.py:128-131)
    float* keys = h->dkeys;
    HIP_TRY(hipMemcpyAsync(keys, keys_nhwc, (size_t)Mk * E * 4, hipMemcpyDeviceToDevice, s));
    float* queries = h->dq;
    // every tile starts from the same 51 tokens (one launch; it was one copy per tile)
    WM_TRY(launch_simple(h, s, 0.0, add_bcast_kernel, dim3(grid_for((int64_t)Mq * E / 4)), dim3(256), (const float*)nullptr, tok, queries, (int64_t)Mq, E, NQ));

    auto add_q = [&](float* out) {   // queries + query_pe
        return launch_simple(h, s, 0.0, add_bcast_kernel, dim3(grid_for((int64_t)Mq * E / 4)), dim3(256), (const float*)queries, tok, out, (int64_t)Mq, E, NQ);
    };
    auto add_k = [&](float* out) {   // keys + key_pe
        return launch_simple(h, s, 0.0, add_bcast_kernel, dim3(grid_for((int64_t)Mk * E / 4)), dim3(256), (const float*)keys, (const float*)h->kpe, out, (int64_t)Mk, E, T);
    };
    auto ln = [&](float* x, const std::string& n, int rows) {
        return launch_layernorm(h, s, WM_PREC_FP16, x, W32(h, n + ".weight"), W32(h, n + ".bias"), 1e-5f, x, nullptr, rows, E);   // fp32 in place: the 16-bit type is unused
    };
    // token -> image attention: q from (queries+pe), k from (keys+pe) [kin], v from keys; result added to queries
    auto token_to_image = [&](const DecAttnW& w, const float* kin) -> int {
        WM_TRY(add_q(h->dt_h1));
        WM_TRY(launch_gemm32(h, s, h->dt_h1, w.wq, w.bq, nullptr, h->dt_q, Mq, w.internal, E, ACT_NONE));
        WM_TRY(launch_gemm32(h, s, kin, w.wk, w.bk, nullptr, h->dk_a, Mk, w.internal, E, ACT_NONE));
        WM_TRY(launch_gemm32(h, s, keys, w.wv, w.bv, nullptr, h->dk_b, Mk, w.internal, E, ACT_NONE));
        WM_TRY(launch_mha32(h, s, h->dt_q, h->dk_a, h->dk_b, h->dt_att, B, 8, w.internal / 8, NQ, T));
        WM_TRY(launch_gemm32(h, s, h->dt_att, w.wo, w.bo, queries, queries, Mq, E, w.internal, ACT_NONE));
        return 0;
    };
    float* kpe_sum = h->n1;   // reuse [B*T,256] fp32 scratch of the neck: keys + key_pe

    for (int i = 0; i < 2; ++i) {
        const std::string L = t + "layers." + std::to_string(i) + ".";
        // (1) self attention of the tokens (transformer.py:151-158)
        {
            const DecAttnW w = dec_w(h, L + "self_attn.", E);
            const float* qin = queries;
            if (i != 0) { WM_TRY(add_q(h->dt_h1)); qin = h->dt_h1; }
            WM_TRY(launch_gemm32(h, s, qin, w.wq, w.bq, nullptr, h->dt_q, Mq, E, E, ACT_NONE));
            WM_TRY(launch_gemm32(h, s, qin, w.wk, w.bk, nullptr, h->dt_k, Mq, E, E, ACT_NONE));
            WM_TRY(launch_gemm32(h, s, queries, w.wv, w.bv, nullptr, h->dt_v, Mq, E, E, ACT_NONE));
            WM_TRY(launch_mha32(h, s, h->dt_q, h->dt_k, h->dt_v, h->dt_att, B, 8, E / 8, NQ, NQ));
            // layer 0 replaces the queries (no residual, :155-156); later layers add
            WM_TRY(launch_gemm32(h, s, h->dt_att, w.wo, w.bo, i == 0 ? nullptr : queries, queries, Mq, E, E, ACT_NONE));
            WM_TRY(ln(queries, L + "norm1", Mq));
        }
        // (2) tokens attend to the image (:160-165)
        WM_TRY(add_k(kpe_sum));
        WM_TRY(token_to_image(dec_w(h, L + "cross_attn_token_to_image.", E / 2), kpe_sum));
        WM_TRY(ln(queries, L + "norm2", Mq));
        // (3) MLP (:167-170)
        WM_TRY(launch_gemm32(h, s, queries, W32(h, L + "mlp.lin1.weight"), W32(h, L + "mlp.lin1.bias"), nullptr, h->dt_hid, Mq, DEC_MLP, E, ACT_RELU));
        WM_TRY(launch_gemm32(h, s, h->dt_hid, W32(h, L + "mlp.lin2.weight"), W32(h, L + "mlp.lin2.bias"), queries, queries, Mq, E, DEC_MLP, ACT_NONE));
        WM_TRY(ln(queries, L + "norm3", Mq));
        // (4) image attends to the tokens (:172-178): q = keys+pe, k = queries+pe, v = queries
        {
            const DecAttnW w = dec_w(h, L + "cross_attn_image_to_token.", E / 2);
            WM_TRY(add_q(h->dt_h1));
            WM_TRY(launch_gemm32(h, s, kpe_sum, w.wq, w.bq, nullptr, h->dk_a, Mk, w.internal, E, ACT_NONE));
            WM_TRY(launch_gemm32(h, s, h->dt_h1, w.wk, w.bk, nullptr, h->dt_k, Mq, w.internal, E, ACT_NONE));
            WM_TRY(launch_gemm32(h, s, queries, w.wv, w.bv, nullptr, h->dt_v, Mq, w.internal, E, ACT_NONE));
            WM_TRY(launch_mha32(h, s, h->dk_a, h->dt_k, h->dt_v, h->dk_c, B, 8, w.internal / 8, T, NQ));
            WM_TRY(launch_gemm32(h, s, h->dk_c, w.wo, w.bo, keys, keys, Mk, E, w.internal, ACT_NONE));
            WM_TRY(ln(keys, L + "norm4", Mk));
        }
    }
    // final token -> image attention (transformer.py:100-104)
    WM_TRY(add_k(kpe_sum));
    WM_TRY(token_to_image(dec_w(h, t + "final_attn_token_to_image.", E / 2), kpe_sum));
    WM_TRY(ln(queries, t + "norm_final_attn", Mq));

    // heads (box_decoder.py:102-103)
    const std::string c = "mask_decoder.class_embed.layers.", bb = "mask_decoder.bbox_embed.layers.";
    WM_TRY(launch_gemm32(h, s, queries, W32(h, c + "0.weight"), W32(h, c + "0.bias"), nullptr, h->dt_h1, Mq, E, E, ACT_RELU));
    WM_TRY(launch_gemm32(h, s, h->dt_h1, W32(h, c + "1.weight"), W32(h, c + "1.bias"), nullptr, h->dt_h2, Mq, E, E, ACT_RELU));
    WM_TRY(launch_gemm32(h, s, h->dt_h2, W32(h, c + "2.weight"), W32(h, c + "2.bias"), nullptr, logits, Mq, WM_NUM_LOGITS, E, ACT_NONE));
    WM_TRY(launch_gemm32(h, s, queries, W32(h, bb + "0.weight"), W32(h, bb + "0.bias"), nullptr, h->dt_h1, Mq, E, E, ACT_RELU));
    WM_TRY(launch_gemm32(h, s, h->dt_h1, W32(h, bb + "1.weight"), W32(h, bb + "1.bias"), nullptr, h->dt_h2, Mq, E, E, ACT_RELU));
    WM_TRY(launch_gemm32(h, s, h->dt_h2, W32(h, bb + "2.weight"), W32(h, bb + "2.bias"), nullptr, boxes, Mq, 4, E, ACT_SIGMOID));
    return 0;
}

int forward_impl(wm_handle* h, const float* x_dev, const float* target_sizes_dev, float* logits_dev, float* boxes_dev,
                 wm_box_record* records_dev, int batch, hipStream_t s) {
    WM_TRY(fft_impl(h, x_dev, h->hfc, batch, s, true));                                    // network.py:61 (+ the embeds' 16-bit operands)
    WM_TRY(encoder_impl(h, x_dev, h->hfc, nullptr, batch, s, true));                       // network.py:65
    WM_TRY(decoder_impl(h, h->emb_nhwc, h->logits, h->boxes, batch, s));                   // network.py:79-86
    const float* ts = target_sizes_dev ? target_sizes_dev : h->tsz_default;
    WM_TRY(launch_simple(h, s, 0.0, postprocess_nms_kernel, dim3(batch), dim3(64), (const float*)h->logits, (const float*)h->boxes, ts,
                         0.05f, 0.5f, 0.4f, h->records));
    if (logits_dev) HIP_TRY(hipMemcpyAsync(logits_dev, h->logits, (size_t)batch * NQ * WM_NUM_LOGITS * 4, hipMemcpyDeviceToDevice, s));
    if (boxes_dev) HIP_TRY(hipMemcpyAsync(boxes_dev, h->boxes, (size_t)batch * NQ * 16, hipMemcpyDeviceToDevice, s));
    if (records_dev) HIP_TRY(hipMemcpyAsync(records_dev, h->records, (size_t)batch * NQ * sizeof(wm_box_record), hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace
