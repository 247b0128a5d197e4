// Attention launchers: the encoder's global / window kernels and their instance pickers, the decoder's fp32 attention.
#pragma once
#include "attn_glob4.h"
#include "attn_glob8.h"
#include "attn_window.h"
#include "dec_kernels.h"
#include "misc_kernels.h"
#include "host_core.h"

namespace {

// One attention launch, the same sequence for the three kernels: LDS limit, bracket, dev hook, launch, check.  tl: the dev build's
// timeline of the instance (dev_attn_timeline: tag, waves, stamps per wave), tag null = the kernel has none.
struct AttnTimeline { const char* tag = nullptr; int waves = 0, marks = 0; };
template <auto KERN, class... Extra>
int launch_attn(wm_handle* h, hipStream_t s, int kclass, double flops, AttnTimeline tl, int grid, int block, int lds, const AttnArgs& a, Extra... extra) {
    lds += (tl.tag && WM_DEV_TIMELINE) ? 4096 : 0;         // dev build: room for the phase stamps
    WM_TRY(set_max_lds((const void*)KERN, lds));
    Bracket br(h, s, kclass, flops, 0.0);
    if (tl.tag) WM_DEV_HOOK((dev_attn_timeline<KERN>(tl.tag, tl.waves, tl.marks, dim3(grid), dim3(block), lds, s, a, extra...)));
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(block), lds, s, a, extra...);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class T16, int HD, bool REL>
int launch_attn_global_t(wm_handle* h, hipStream_t s, const AttnArgs& a, int batch, int kclass) {
    // the 8-wave anti-phase kernel (attn_glob8.h); WM_ATTN_4WAVE=1 (read once per process; A/B runs) keeps every shape on the 4-wave one
    static const bool four_wave = getenv("WM_ATTN_4WAVE") && atoi(getenv("WM_ATTN_4WAVE")) != 0;
    const double flops = 4.0 * batch * a.heads * (double)a.nq * a.nk * HD;
    // (head_dim 128, the HFC cross-attention: on the 8-wave kernel since round 4 -- with -m through the bias k-step its phases balance,
    // 1086 vs 1257 us on the 4-wave kernel, profiles/r4_dev/attn_kernels_log2_domain.txt)
    if (a.nq % 256 == 0 && a.nk >= 128 && !four_wave)
        return launch_attn<attn_global8_kernel<T16, HD, REL>>(h, s, kclass, flops, {"g8", 8, 64}, (a.nq / 256) * a.heads * batch, 512, Global8Lds<HD, REL>::TOTAL, a);
    return launch_attn<attn_global_kernel<T16, HD, REL>>(h, s, kclass, flops, {}, (a.nq / 128) * a.heads * batch, 256, GlobalLds<HD, REL>::TOTAL, a);
}

// the built instances: rel-pos for the encoder's head dims, 128 (the HFC cross-attention) without
template <class T16>
int launch_attn_global_p(wm_handle* h, hipStream_t s, const AttnArgs& a, int batch, int hd, bool rel, int kclass) {
    if (a.nq % 128 || a.nk % 64) return fail("attention: nq=%d nk=%d must be multiples of 128/64", a.nq, a.nk);
    if (rel && (a.nq != T || a.nk != T)) return fail("attention: rel-pos path needs 4096 queries and keys");
    auto none = [&] { return fail("attention: head_dim=%d rel=%d not built (64, 80, 128)", hd, (int)rel); };
    if (rel) return by_head_dim<64, 80>(hd, [&](auto d) { return launch_attn_global_t<T16, decltype(d)::value, true>(h, s, a, batch, kclass); }, none);
    return by_head_dim<64, 80, 128>(hd, [&](auto d) { return launch_attn_global_t<T16, decltype(d)::value, false>(h, s, a, batch, kclass); }, none);
}
int launch_attn_global(wm_handle* h, hipStream_t s, int prec, const AttnArgs& a, int batch, int hd, bool rel) {
    return by_type16(prec, [&](auto t) { return launch_attn_global_p<decltype(t)>(h, s, a, batch, hd, rel, WM_KCLASS_ATTN_GLOBAL); });
}

template <class T16, int HD>
int launch_attn_window_t(wm_handle* h, hipStream_t s, const AttnArgs& a, int batch) {
    const int num_cu = num_cus();
    const int nitems = 25 * a.heads * batch;
    const int grid = nitems < num_cu ? nitems : num_cu;
    // (round 4: an 8-wave anti-phase form of this kernel -- key tiles of 64 slots in a 4-slot ring filled by LDS-DMA, SIMD partners one
    // phase apart, ten barriers per item -- was built, is correct and measured 388 vs 274 us per launch: tools/experiments/
    // attn_win8_antiphase_window.h)
    const double flops = 4.0 * batch * a.heads * 4096.0 * 196.0 * HD;      // useful work only
    return launch_attn<attn_window_kernel<T16, HD>>(h, s, WM_KCLASS_ATTN_WIN, flops, {"win", 7, 48}, grid, 448, WindowLds<HD>::TOTAL, a, nitems);
}

// n4 groups of four fp32 values -> the 16-bit type of `prec`, unbracketed (the window attention's bias row, wm_op_cvt_f32_to_16)
int launch_cvt_f32_to_16(hipStream_t s, int prec, const float* in, void* out, int64_t n4) {
    return by_type16(prec, [&](auto t) { return launch_simple(nullptr, s, 0.0, cvt_f32_to_16_kernel<decltype(t)>, dim3(grid_for(n4)), dim3(256), in, (u16*)out, n4); });
}

// The attention kernels take q in the log2 domain, c1 q with c1 = head_dim^-0.5 * log2 e (attn_common.h "Scores").  A caller that holds the
// reference's plain q (the single-op entry points) gets a scaled copy in a scratch buffer: a.q / a.q_stride are redirected to it.
int scale_q_copy(hipStream_t s, int prec, AttnArgs& a, int batch, int cols) {
    const int64_t rows = (int64_t)batch * a.nq;
    void* pb = nullptr;
    WM_TRY(op_scratch(s, 2, (size_t)rows * cols * 2, &pb));
    const float c1 = a.scale * 1.44269504088896340736f;
    const dim3 grid(grid_for(rows * (cols / 8)));
    by_type16(prec, [&](auto t) { hipLaunchKernelGGL(scale_q16_kernel<decltype(t)>, grid, dim3(256), 0, s, a.q, a.q_stride, (u16*)pb, rows, cols, c1); });
    HIP_TRY(hipGetLastError());
    a.q = (const u16*)pb;
    a.q_stride = cols;
    return 0;
}

// What launch_encoder_attention takes beyond the packed-qkv form.
//   out8: write the output as e4m3 bytes there instead of 16-bit to `out` (the A operand of an fp8 proj GEMM);
//   k_sep / v_sep / tok_stride: q / k / v as three tensors of one token stride (`qkv` is then q);
//   q_prescaled: q already carries softmax scale * log2 e (the engine folds it into the q rows of the qkv weight at
//             wm_finalize_weights, attn_common.h "Scores"); 0 for the single-op entry points, whose callers pass the reference's plain q.
struct AttnExtra {
    void* out8 = nullptr;
    const void* k_sep = nullptr;
    const void* v_sep = nullptr;
    int tok_stride = 0;
    int q_prescaled = 0;
};

int launch_encoder_attention(wm_handle* h, hipStream_t s, int prec, const void* qkv, const float* qkv_bias,
                             const float* rel_h, const float* rel_w, void* out, int batch, int heads, int hd, int window,
                             const AttnExtra& x = AttnExtra{}) {
    const int D = heads * hd;
    AttnArgs a{};
    a.out8 = (unsigned char*)x.out8;
    a.q = (const u16*)qkv; a.k = (const u16*)qkv + D; a.v = (const u16*)qkv + 2 * D;
    a.out = (u16*)out;
    a.q_stride = a.k_stride = a.v_stride = 3 * D;
    if (x.k_sep) { a.k = (const u16*)x.k_sep; a.v = (const u16*)x.v_sep; a.q_stride = a.k_stride = a.v_stride = x.tok_stride; }   // q / k / v as three tensors
    a.out_stride = D;
    a.nq = a.nk = T;
    a.scale = 1.0f / sqrtf((float)hd);
    a.rel_h = rel_h; a.rel_w = rel_w; a.qkv_bias = qkv_bias; a.heads = heads;
    if (!x.q_prescaled) WM_TRY(scale_q_copy(s, prec, a, batch, D));
    if (window == 0) return launch_attn_global(h, s, prec, a, batch, hd, true);
    if (window != 14) return fail("attention: window=%d unsupported (14 or 0)", window);
    {   // the bias as a 16-bit row (AttnArgs::qkv_bias16): cached per handle, converted per call without one
        uint16_t* b16 = nullptr;
        bool convert = true;
        if (h) {
            auto it = h->bias16.find({qkv_bias, prec});
            if (it != h->bias16.end()) { b16 = it->second; convert = false; }
            else { WM_TRY(dalloc(h, &b16, (size_t)3 * D * 2)); h->bias16[{qkv_bias, prec}] = b16; }
        } else {
            void* pb = nullptr;
            WM_TRY(op_scratch(s, 0, (size_t)3 * D * 2, &pb));
            b16 = (uint16_t*)pb;
        }
        if (convert) WM_TRY(launch_cvt_f32_to_16(s, prec, qkv_bias, b16, 3 * D / 4));
        a.qkv_bias16 = (const u16*)b16;
    }
    return by_head_dim<64, 80>(hd, [&](auto d) {
        return by_type16(prec, [&](auto t) { return launch_attn_window_t<decltype(t), decltype(d)::value>(h, s, a, batch); });
    }, [&] { return fail("attention: head_dim=%d not built for windows (64, 80)", hd); });
}

int launch_mha16(wm_handle* h, hipStream_t s, int prec, const void* q, int qs, const void* k, int ks, const void* v, int vs,
                 void* out, int os, int batch, int heads, int hd, int nq, int nk, int q_prescaled = 0) {
    AttnArgs a{};
    a.q = (const u16*)q; a.k = (const u16*)k; a.v = (const u16*)v; a.out = (u16*)out;
    a.q_stride = qs; a.k_stride = ks; a.v_stride = vs; a.out_stride = os;
    a.nq = nq; a.nk = nk; a.scale = 1.0f / sqrtf((float)hd); a.heads = heads;
    if (!q_prescaled) WM_TRY(scale_q_copy(s, prec, a, batch, heads * hd));
    return launch_attn_global(h, s, prec, a, batch, hd, false);
}

int launch_mha32(wm_handle* h, hipStream_t s, const float* q, const float* k, const float* v, float* out, int batch,
                 int heads, int hd, int nq, int nk) {
    Bracket br(h, s, WM_KCLASS_OTHER, 4.0 * batch * heads * (double)nq * nk * hd, 0.0);
    // many keys, few queries (token -> image): 4 queries share each K / V row and 4 waves split the keys; otherwise one
    // query per wave
    const bool share = nk >= 1024;
    constexpr int KC = 256;                        // keys per workgroup of the key-split kernel
    if (hd == 16 && nq <= 64 && nk >= 1024 && nk % KC == 0) {
        // token -> image: keys split over workgroups, K / V read once (dec_kernels.h); partials in a scratch buffer of the handle
        // (or, for handle-less op calls, of the process)
        const int nchunk = nk / KC;
        const size_t need = (size_t)batch * heads * nchunk * 64 * (16 + 2) * 4;
        float* part = nullptr;
        if (h) {
            if (h->mha_part_cap < need) {
                if (h->mha_part) dfree(h, h->mha_part);
                h->mha_part = nullptr; h->mha_part_cap = 0;
                WM_TRY(dalloc(h, &h->mha_part, need));
                h->mha_part_cap = need;
            }
            part = h->mha_part;
        } else {
            void* pb = nullptr;
            WM_TRY(op_scratch(s, 1, need, &pb));
            part = (float*)pb;
        }
        hipLaunchKernelGGL((mha32_keysplit_kernel<16, KC>), dim3(nchunk, heads, batch), dim3(256), 0, s, q, k, v, part, nq, nk, heads);
        hipLaunchKernelGGL((mha32_merge_chunks_kernel<16>), dim3(heads, batch), dim3(64 * 4), 0, s, (const float*)part, out, nq, nchunk, heads);
    } else if (hd == 16 && nk == NQ && nq >= 1024)       // image -> token: one thread per query, K / V from scalar loads
        hipLaunchKernelGGL((mha32_fewkeys_kernel<16, NQ>), dim3((nq + 255) / 256, heads, batch), dim3(256), 0, s, q, k, v, out, nq, heads);
    else if (hd == 16 && share) hipLaunchKernelGGL((mha32_kernel<16, 4, 4>), dim3((nq + 3) / 4, heads, batch), dim3(256), 0, s, q, k, v, out, nq, nk, heads);
    else if (hd == 16) hipLaunchKernelGGL((mha32_kernel<16, 1>), dim3(nq, heads, batch), dim3(64), 0, s, q, k, v, out, nq, nk, heads);
    else if (hd == 32) hipLaunchKernelGGL((mha32_kernel<32, 1>), dim3(nq, heads, batch), dim3(64), 0, s, q, k, v, out, nq, nk, heads);
    else return fail("mha32: head_dim=%d not built (16, 32)", hd);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
