// The weight table: expected tensors, host-side conversion to the operand types, uploads, wm_create / wm_finalize_weights.
#pragma once
#include "misc_kernels.h"
#include "fft_kernels.h"
#include "host_core.h"

namespace {

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// ---------------------------------------------------------------------------
// host-side 16-bit conversion (round to nearest even), used by the weight packer
// ---------------------------------------------------------------------------
static inline uint16_t f32_to_bf16_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

static inline uint16_t f32_to_f16_host(float f) {
    _Float16 h = (_Float16)fminf(fmaxf(f, -65504.f), 65504.f);
    uint16_t r;
    memcpy(&r, &h, 2);
    return r;
}

// f32 -> OCP e4m3fn (bias 7, max 448, no infinity, 0x7f = NaN), round to nearest even, saturating; weight packer of WM_PREC_FP8
static inline uint8_t f32_to_e4m3_host(float f) {
    if (f != f) return 0x7f;
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    float a = fabsf(f);
    if (a > 448.0f) a = 448.0f;
    if (a == 0.0f) return sign;
    int e;
    (void)frexpf(a, &e);                                           // a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    int fl = e - 1;
    if (fl < -6) fl = -6;                                          // subnormals share the quantum 2^-9
    const float q = ldexpf(1.0f, fl - 3);
    float v = nearbyintf(a / q) * q;                               // exact scaling; default rounding mode = nearest even
    if (v == 0.0f) return sign;
    if (v > 448.0f) v = 448.0f;
    if (v < ldexpf(1.0f, -6)) return sign | (uint8_t)(int)(v / ldexpf(1.0f, -9));
    (void)frexpf(v, &e);
    const int ex = e - 1;
    const int man = (int)((v / ldexpf(1.0f, ex) - 1.0f) * 8.0f);
    return sign | (uint8_t)(((ex + 7) << 3) | man);
}

// -------- expected weights --------
void add_attn(std::map<std::string, std::vector<int64_t>>& m, const std::string& p, int E, int internal) {
    for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
        m[p + n + ".weight"] = {internal, E};
        m[p + n + ".bias"] = {internal};
    }
    m[p + "out_proj.weight"] = {E, internal};
    m[p + "out_proj.bias"] = {E};
}

void build_expected(wm_handle* h) {
    auto& m = h->expected;
    const int D = h->D, hd = h->hd;
    const std::string e = "image_encoder.";
    m[e + "pos_embed"] = {1, GRID, GRID, D};
    m[e + "patch_embed.proj.weight"] = {D, 3, 16, 16};
    m[e + "patch_embed.proj.bias"] = {D};
    m[e + "hfc_embed.proj.weight"] = {HFC, 1, 16, 16};
    m[e + "hfc_embed.proj.bias"] = {HFC};
    const std::string a = e + "hfc_attn.";
    m[a + "pos_embed"] = {1, HFC, GRID, GRID};
    m[a + "proj_hfc.weight"] = {HFC, HFC, 1, 1};
    m[a + "proj_hfc.bias"] = {HFC};
    m[a + "proj_patch.weight"] = {HFC, D, 1, 1};
    m[a + "proj_patch.bias"] = {HFC};
    m[a + "cross_attn.in_proj_weight"] = {3 * HFC, HFC};
    m[a + "cross_attn.in_proj_bias"] = {3 * HFC};
    m[a + "cross_attn.out_proj.weight"] = {HFC, HFC};
    m[a + "cross_attn.out_proj.bias"] = {HFC};
    for (const char* n : {"linear1", "linear2"}) {
        m[a + n + ".weight"] = {HFC, HFC};
        m[a + n + ".bias"] = {HFC};
    }
    for (const char* n : {"norm1", "norm2"}) {
        m[a + n + ".weight"] = {HFC};
        m[a + n + ".bias"] = {HFC};
    }
    m[a + "proj_back.weight"] = {D, HFC, 1, 1};
    m[a + "proj_back.bias"] = {D};
    for (int i = 0; i < h->depth; ++i) {
        const std::string b = e + "blocks." + std::to_string(i) + ".";
        const int size = h->is_global[i] ? GRID : 14;
        m[b + "norm1.weight"] = {D};
        m[b + "norm1.bias"] = {D};
        m[b + "attn.rel_pos_h"] = {2 * size - 1, hd};
        m[b + "attn.rel_pos_w"] = {2 * size - 1, hd};
        m[b + "attn.qkv.weight"] = {3 * D, D};
        m[b + "attn.qkv.bias"] = {3 * D};
        m[b + "attn.proj.weight"] = {D, D};
        m[b + "attn.proj.bias"] = {D};
        m[b + "norm2.weight"] = {D};
        m[b + "norm2.bias"] = {D};
        m[b + "mlp.lin1.weight"] = {4 * D, D};
        m[b + "mlp.lin1.bias"] = {4 * D};
        m[b + "mlp.lin2.weight"] = {D, 4 * D};
        m[b + "mlp.lin2.bias"] = {D};
    }
    m[e + "neck.0.weight"] = {OUTC, D, 1, 1};
    m[e + "neck.1.weight"] = {OUTC};
    m[e + "neck.1.bias"] = {OUTC};
    m[e + "neck.2.weight"] = {OUTC, OUTC, 3, 3};
    m[e + "neck.3.weight"] = {OUTC};
    m[e + "neck.3.bias"] = {OUTC};
    m["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"] = {2, OUTC / 2};
    const std::string d = "mask_decoder.";
    for (int i = 0; i < 2; ++i) {
        const std::string L = d + "transformer.layers." + std::to_string(i) + ".";
        add_attn(m, L + "self_attn.", OUTC, OUTC);
        add_attn(m, L + "cross_attn_token_to_image.", OUTC, OUTC / 2);
        add_attn(m, L + "cross_attn_image_to_token.", OUTC, OUTC / 2);
        for (const char* n : {"norm1", "norm2", "norm3", "norm4"}) {
            m[L + n + ".weight"] = {OUTC};
            m[L + n + ".bias"] = {OUTC};
        }
        m[L + "mlp.lin1.weight"] = {DEC_MLP, OUTC};
        m[L + "mlp.lin1.bias"] = {DEC_MLP};
        m[L + "mlp.lin2.weight"] = {OUTC, DEC_MLP};
        m[L + "mlp.lin2.bias"] = {OUTC};
    }
    add_attn(m, d + "transformer.final_attn_token_to_image.", OUTC, OUTC / 2);
    m[d + "transformer.norm_final_attn.weight"] = {OUTC};
    m[d + "transformer.norm_final_attn.bias"] = {OUTC};
    m[d + "iou_token.weight"] = {1, OUTC};                 // parameter exists, unused in forward (box_decoder.py:52)
    m[d + "mask_tokens.weight"] = {NQ, OUTC};
    const int cls_dims[4] = {OUTC, OUTC, OUTC, WM_NUM_LOGITS}, box_dims[4] = {OUTC, OUTC, OUTC, 4};
    for (int j = 0; j < 3; ++j) {
        m[d + "class_embed.layers." + std::to_string(j) + ".weight"] = {cls_dims[j + 1], cls_dims[j]};
        m[d + "class_embed.layers." + std::to_string(j) + ".bias"] = {cls_dims[j + 1]};
        m[d + "bbox_embed.layers." + std::to_string(j) + ".weight"] = {box_dims[j + 1], box_dims[j]};
        m[d + "bbox_embed.layers." + std::to_string(j) + ".bias"] = {box_dims[j + 1]};
    }
}

// Stem (patch / HFC embeds), HFC adaptor and neck always run with fp16 operands: they are 2.9 % of the FLOPs,
// their inputs are normalised (|x| of a few units), and in bf16 they alone cost 1e-3 on the logits (DESIGN.md
// "Precision").  The transformer blocks use the handle's precision (bf16 by default).
// precision of transformer block i
static int block_prec(const wm_handle* h, int i) {
    if (h->prec == WM_PREC_FP8) return (i >= h->depth - h->fp8_bf16_tail || i < h->fp8_bf16_head) ? WM_PREC_BF16 : WM_PREC_FP8;
    return (h->prec == WM_PREC_BF16 && i >= h->depth - h->fp16_tail) ? WM_PREC_FP16 : h->prec;
}
static bool is_fp8_block_gemm(const wm_handle* h, const std::string& name) {
    const std::string pre = "image_encoder.blocks.";
    if (h->prec != WM_PREC_FP8 || name.rfind(pre, 0) != 0) return false;
    if (block_prec(h, atoi(name.c_str() + pre.size())) != WM_PREC_FP8) return false;
    const std::pair<const char*, int> sufs[] = {{"attn.qkv.weight", WM_FP8_QKV}, {"attn.proj.weight", WM_FP8_PROJ},
                                                {"mlp.lin1.weight", WM_FP8_MLP}, {"mlp.lin2.weight", WM_FP8_MLP}};
    for (const auto& sf : sufs)
        if (ends_with(name, sf.first)) return (h->fp8_gemms & sf.second) != 0;
    return false;
}
static bool is_fp16_block(const wm_handle* h, const std::string& name) {
    const std::string pre = "image_encoder.blocks.";
    if (name.rfind(pre, 0) != 0) return false;
    return block_prec(h, atoi(name.c_str() + pre.size())) == WM_PREC_FP16;
}

bool is_stem_or_neck(const std::string& name) {
    return name.rfind("image_encoder.patch_embed.", 0) == 0 || name.rfind("image_encoder.hfc_embed.", 0) == 0 ||
           name.rfind("image_encoder.hfc_attn.", 0) == 0 || name.rfind("image_encoder.neck.", 0) == 0;
}

int upload16(wm_handle* h, const std::string& key, const float* src, size_t n) {
    std::vector<uint16_t> tmp(n);
    if (h->prec == WM_PREC_FP16 || is_stem_or_neck(key) || is_fp16_block(h, key)) for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_f16_host(src[i]);
    else for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_host(src[i]);
    uint16_t* d = nullptr;
    WM_TRY(dalloc(h, &d, n * 2));
    HIP_TRY(hipMemcpy(d, tmp.data(), n * 2, hipMemcpyHostToDevice));
    h->w16[key] = d;
    return 0;
}

// [N][K] fp32 -> e4m3 with one fp32 scale per output channel (absmax / 448), gemm8.h
int upload8(wm_handle* h, const std::string& key, const float* src, size_t rows, size_t cols) {
    std::vector<uint8_t> q(rows * cols);
    std::vector<float> sc(rows);
    for (size_t r = 0; r < rows; ++r) {
        float amax = 0.f;
        for (size_t c = 0; c < cols; ++c) amax = fmaxf(amax, fabsf(src[r * cols + c]));
        const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
        sc[r] = scale;
        for (size_t c = 0; c < cols; ++c) q[r * cols + c] = f32_to_e4m3_host(src[r * cols + c] / scale);
    }
    uint8_t* d = nullptr;
    WM_TRY(dalloc(h, &d, rows * cols));
    HIP_TRY(hipMemcpy(d, q.data(), rows * cols, hipMemcpyHostToDevice));
    h->w8[key] = d;
    if (cols % 256 == 0 && (ends_with(key, "attn.qkv.weight") || ends_with(key, "mlp.lin1.weight"))) {
        std::vector<uint8_t> qk(rows * cols);
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < cols; ++c) qk[r * cols + (size_t)plane_pos((int)c)] = q[r * cols + c];
        uint8_t* dk = nullptr;
        WM_TRY(dalloc(h, &dk, rows * cols));
        HIP_TRY(hipMemcpy(dk, qk.data(), rows * cols, hipMemcpyHostToDevice));
        h->w8k[key] = dk;
    }
    float* ds = nullptr;
    WM_TRY(dalloc(h, &ds, rows * 4));
    HIP_TRY(hipMemcpy(ds, sc.data(), rows * 4, hipMemcpyHostToDevice));
    h->w32[key + ".wscale"] = ds;
    return 0;
}

int upload32(wm_handle* h, const std::string& key, const float* src, size_t n) {
    float* d = nullptr;
    WM_TRY(dalloc(h, &d, n * 4));
    HIP_TRY(hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice));
    h->w32[key] = d;
    return 0;
}

const uint16_t* W16(wm_handle* h, const std::string& n) { return h->w16.at(n); }
const uint16_t* W16P(wm_handle* h, const std::string& n) {
    if (h->row_major) return nullptr;
    auto it = h->w16p.find(n);
    return it == h->w16p.end() ? nullptr : it->second;
}
const float* W32(wm_handle* h, const std::string& n) { return h->w32.at(n); }

// gamma (.) W in LDS-image order, c1, c2 of a folded LayerNorm's consumer weight (fold_weight_kernel); w32 = the fp32 weight, or null: from w16
int launch_fold_weight(hipStream_t s, int prec, const void* w16, const float* w32, const float* g, const float* be, const float* bias, void* wf,
                       float* c1, float* c2, int N, int K) {
    return by_type16(prec, [&](auto t) {
        return launch_simple(nullptr, s, 0.0, fold_weight_kernel<decltype(t)>, dim3(N), dim3(256), (const u16*)w16, w32, g, be, bias, (u16*)wf, c1, c2, N, K);
    });
}

// the checked configuration -> a handle with its workspace (wm_create)
int create_impl(const wm_config* cfg, int device, wm_handle** out) {
    HIP_TRY(hipSetDevice(device));
    wm_handle* h = new wm_handle();
    h->cfg = *cfg; h->device = device;
    // bf16 mode: WM_FP16_TAIL=K gives the last K blocks fp16 operands.  Measured (ViT-H, B=16, one box): K = 0 / 8 / 16 / 32 ->
    // logits 8.2e-4 / 7.9e-4 / 6.5e-4 / 2.4e-4 of the reference at 149.9 / 148.6 / 147.1 / 144.8 tiles/s: every block's bf16
    // rounding contributes alike, so the dial buys margin only in proportion to what it costs; default 0 (= north_star's bf16)
    h->fp16_tail = getenv("WM_FP16_TAIL") ? atoi(getenv("WM_FP16_TAIL")) : 0;
    h->fp8_bf16_tail = getenv("WM_FP8_BF16_TAIL") ? atoi(getenv("WM_FP8_BF16_TAIL")) : 0;
    h->fp8_bf16_head = getenv("WM_FP8_BF16_HEAD") ? atoi(getenv("WM_FP8_BF16_HEAD")) : 0;
    h->row_major = getenv("WM_ROW_MAJOR_OPERANDS") && atoi(getenv("WM_ROW_MAJOR_OPERANDS")) != 0;
    h->fold = (cfg->flags & (WM_CFG_FOLD_LN | WM_CFG_FOLD_LN_BF16)) != 0 && !h->row_major;
    h->fold_bf16 = (cfg->flags & WM_CFG_FOLD_LN_BF16) != 0;
    h->fold_from16 = getenv("WM_FOLD_FROM16") && atoi(getenv("WM_FOLD_FROM16")) != 0;
    h->rows8 = !(getenv("WM_FP8_ROWS") && atoi(getenv("WM_FP8_ROWS")) == 0);
    h->split = h->fold && !(getenv("WM_STREAM_SPLIT") && atoi(getenv("WM_STREAM_SPLIT")) == 0);
    h->fp8_gemms = cfg->fp8_gemms ? (cfg->fp8_gemms & WM_FP8_ALL) : (getenv("WM_FP8_GEMMS") ? (atoi(getenv("WM_FP8_GEMMS")) & WM_FP8_ALL) : WM_FP8_ALL);
    if (cfg->precision == WM_PREC_FP8 && h->fp8_gemms == 0) { delete h; return fail("wm_create: fp8_gemms selects no GEMM"); }
    h->D = cfg->embed_dim; h->depth = cfg->depth; h->heads = cfg->num_heads; h->hd = cfg->embed_dim / cfg->num_heads;
    h->prec = cfg->precision; h->maxB = cfg->max_batch;
    for (int i = 0; i < cfg->num_global; ++i) {
        const int g = cfg->global_attn_indexes[i];
        if (g < 0 || g >= cfg->depth) { delete h; return fail("wm_create: global index %d out of range", g); }
        h->is_global[g] = true;
    }
    build_expected(h);

    const size_t B = (size_t)h->maxB, D = (size_t)h->D, BT = B * T;
    int r = 0;
#define A(ptr, bytes) if (!r) r = dalloc(h, &h->ptr, (bytes))
    A(resid, BT * D * 4); A(tokbase, BT * D * 4);
    A(xn16, BT * D * 2); A(ao16, BT * D * 2); A(qkv16, BT * 3 * D * 2); A(hid16, BT * 4 * D * 2);
    A(p16, BT * 768 * 2); A(h16, BT * 256 * 2); A(he16, BT * HFC * 2); A(hp16, BT * HFC * 2); A(pt16, BT * HFC * 2);
    A(q16, BT * HFC * 2); A(kv16, BT * 2 * HFC * 2); A(aoh16, BT * HFC * 2); A(y1n16, BT * HFC * 2); A(h1_16, BT * HFC * 2);
    A(y2_16, BT * HFC * 2); A(y2t16, BT * HFC * 2);
    A(pt32, BT * HFC * 4); A(y1, BT * HFC * 4); A(y1n32, BT * HFC * 4); A(z32, BT * HFC * 4);
    A(n1, BT * OUTC * 4); A(n2, BT * OUTC * 4); A(emb_nhwc, BT * OUTC * 4); A(emb_nchw, BT * OUTC * 4);
    A(n1n16, BT * OUTC * 2); A(x16last, BT * D * 2);
    if (cfg->precision == WM_PREC_FP8) { A(ao8, BT * D); }
    A(dkeys, BT * OUTC * 4); A(dk_a, BT * 128 * 4); A(dk_b, BT * 128 * 4); A(dk_c, BT * 128 * 4);
    A(dq, B * NQ * OUTC * 4); A(dt_q, B * NQ * OUTC * 4); A(dt_k, B * NQ * OUTC * 4); A(dt_v, B * NQ * OUTC * 4);
    A(dt_att, B * NQ * OUTC * 4); A(dt_hid, B * NQ * DEC_MLP * 4); A(dt_h1, B * NQ * OUTC * 4); A(dt_h2, B * NQ * OUTC * 4);
    A(logits, B * NQ * WM_NUM_LOGITS * 4); A(boxes, B * NQ * 4 * 4);
    A(hfc, B * 1024 * 1024 * 4); A(tsz_default, B * 2 * 4);
    A(fftR, B * FFT_N * FFT_L * sizeof(float2)); A(fft_tw, FFT_N * sizeof(float2));
    A(kpe, (size_t)T * OUTC * 4);
    A(records, B * NQ * sizeof(wm_box_record));
    A(sat_counts, WM_SAT_COUNT * sizeof(unsigned long long));
    A(fold_stats, BT * 4 * 2 * 4);
    A(lo16, BT * D * 2);
#undef A
    if (!r) {
        void* pf = nullptr;
        if (hipHostMalloc(&pf, 64, hipHostMallocMapped) != hipSuccess) r = fail("wm_create: hipHostMalloc failed");
        else { h->overflow = (int*)pf; h->overflow[0] = h->overflow[1] = 0; }       // [0] the fp16 stream, [1] the decoder's fp16-split GEMMs
    }
    if (r) { wm_destroy(h); return r; }
    // FFT twiddles exp(-2 pi i k / 1024), computed in double
    {
        std::vector<float2> tw(FFT_N);
        for (int k = 0; k < FFT_N; ++k) {
            const double ang = -2.0 * M_PI * k / FFT_N;
            tw[k] = make_float2((float)cos(ang), (float)sin(ang));
        }
        hipError_t e = hipMemcpy(h->fft_tw, tw.data(), FFT_N * sizeof(float2), hipMemcpyHostToDevice);
        std::vector<float> ts(B * 2, 1024.f);
        if (e == hipSuccess) e = hipMemcpy(h->tsz_default, ts.data(), B * 2 * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(h->sat_counts, 0, WM_SAT_COUNT * sizeof(unsigned long long));
        if (e != hipSuccess) { wm_destroy(h); return fail("wm_create: twiddle upload failed: %s", hipGetErrorString(e)); }
    }
    *out = h;
    return 0;
}

// staged host tensors -> device operands of every kind (wm_finalize_weights)
int finalize_impl(wm_handle* h) {
    HIP_TRY(hipSetDevice(h->device));
    // Two independently loadable groups: the encoder ("image_encoder.*") and the
    // decoder ("mask_decoder.*" + "prompt_encoder.*").  A group is ready when every
    // tensor of it has been loaded; a partially loaded group is an error.
    for (int grp = 0; grp < 2; ++grp) {
        std::string missing;
        int nmiss = 0, nhave = 0;
        for (auto& kv : h->expected) {
            const bool enc = kv.first.rfind("image_encoder.", 0) == 0;
            if ((grp == 0) != enc) continue;
            if (h->staged.count(kv.first) || h->w16.count(kv.first) || h->w32.count(kv.first) || h->w8.count(kv.first)) { ++nhave; continue; }
            if (nmiss < 4) missing += (nmiss ? ", " : "") + kv.first;
            ++nmiss;
        }
        if (nmiss && nhave)
            return fail("wm_finalize_weights: %s group incomplete, %d tensors missing (%s%s)", grp == 0 ? "encoder" : "decoder",
                        nmiss, missing.c_str(), nmiss > 4 ? ", ..." : "");
        if (grp == 0) h->enc_ready = nmiss == 0;
        else h->dec_ready = nmiss == 0;
    }
    if (!h->enc_ready && !h->dec_ready) return fail("wm_finalize_weights: no weights loaded");
    // Attention scores are computed in the log2 domain with the scale inside q (attn_common.h "Scores"): the q rows of every qkv
    // weight and bias (and of the HFC cross-attention's in_proj) are multiplied by head_dim^-0.5 * log2 e here, in fp32, BEFORE the one
    // rounding to the operand type (16-bit, folded gamma (.) W, or e4m3 with its per-channel scale), so q = (c1 q_ref) costs no rounding.
    // Each staged tensor passes here exactly once (the staging area is cleared at the end of this call).
    {
        const float c1_blk = (1.0f / sqrtf((float)h->hd)) * 1.44269504088896340736f;
        const float c1_hfc = (1.0f / sqrtf((float)(HFC / HFC_HEADS))) * 1.44269504088896340736f;
        for (auto& kv : h->staged) {
            const std::string& name = kv.first;
            std::vector<float>& d = kv.second.data;
            float c1 = 0.f;
            size_t nq = 0;                                  // leading elements that belong to q
            if (name.rfind("image_encoder.blocks.", 0) == 0 && ends_with(name, "attn.qkv.weight")) { c1 = c1_blk; nq = (size_t)h->D * h->D; }
            else if (name.rfind("image_encoder.blocks.", 0) == 0 && ends_with(name, "attn.qkv.bias")) { c1 = c1_blk; nq = (size_t)h->D; }
            else if (name == "image_encoder.hfc_attn.cross_attn.in_proj_weight") { c1 = c1_hfc; nq = (size_t)HFC * HFC; }
            else if (name == "image_encoder.hfc_attn.cross_attn.in_proj_bias") { c1 = c1_hfc; nq = (size_t)HFC; }
            for (size_t i = 0; i < nq && i < d.size(); ++i) d[i] *= c1;
        }
    }
    // re-upload: free previous device copies of the tensors being replaced
    auto drop = [&](auto& m, const std::string& key) {
        auto it = m.find(key);
        if (it != m.end()) { dfree(h, it->second); m.erase(it); }
    };
    for (auto& kv : h->staged) {
        drop(h->w16, kv.first); drop(h->w16p, kv.first); drop(h->w32, kv.first); drop(h->wsrc32, kv.first);
        drop(h->w8, kv.first); drop(h->w8k, kv.first); drop(h->w32, kv.first + ".wscale");
    }
    // 16-bit copies of the qkv biases are keyed by the fp32 copy's address: a re-upload may reuse an address for new values
    for (auto& kv : h->bias16) dfree(h, kv.second);
    h->bias16.clear();
    for (auto& kv : h->w32x3) { dfree(h, kv.second.first); dfree(h, kv.second.second); }
    h->w32x3.clear();
    for (auto& kv : h->staged) {
        const std::string& name = kv.first;
        const HostW& w = kv.second;
        const size_t n = w.data.size();
        const bool enc = name.rfind("image_encoder.", 0) == 0;
        const bool is_gemm_w = enc && (ends_with(name, ".weight") || ends_with(name, "in_proj_weight")) && w.shape.size() >= 2;
        if (name == "image_encoder.neck.2.weight") {
            // [co][ci][ky][kx] -> [co][tap][ci]
            std::vector<float> t(n);
            for (int co = 0; co < OUTC; ++co)
                for (int ci = 0; ci < OUTC; ++ci)
                    for (int tap = 0; tap < 9; ++tap)
                        t[((size_t)co * 9 + tap) * OUTC + ci] = w.data[((size_t)co * OUTC + ci) * 9 + tap];
            WM_TRY(upload16(h, name, t.data(), n));
        } else if (name == "image_encoder.hfc_attn.pos_embed") {
            // NCHW (1,1024,64,64) -> token-major [4096,1024] (added after proj_hfc, image_encoder.py:494)
            std::vector<float> t(n);
            for (int c = 0; c < HFC; ++c)
                for (int p = 0; p < T; ++p) t[(size_t)p * HFC + c] = w.data[(size_t)c * T + p];
            WM_TRY(upload32(h, name, t.data(), n));
        } else if (is_gemm_w && is_fp8_block_gemm(h, name)) {
            WM_TRY(upload8(h, name, w.data.data(), (size_t)w.shape[0], n / (size_t)w.shape[0]));
        } else if (is_gemm_w) {
            WM_TRY(upload16(h, name, w.data.data(), n));
            // second copy in LDS-image order for the 256-row-tile kernel (row-major stays for the half-width kernels that
            // small batches take): [N][K] with N % 16 == 0 and K % 32 == 0 (every GEMM weight of the encoder)
            const int64_t rows = w.shape[0], cols = (int64_t)n / rows;
            if (rows % 16 == 0 && cols % 32 == 0) {
                uint16_t* dp = nullptr;
                WM_TRY(dalloc(h, &dp, n * 2));
                hipLaunchKernelGGL(pack16_lds_image_kernel, dim3(grid_for((int64_t)n / 8)), dim3(256), 0, 0, (const uint4*)h->w16.at(name), (uint4*)dp, rows, (int)cols);
                HIP_TRY(hipGetLastError());
                h->w16p[name] = dp;
            }
            // a weight the folded LayerNorm multiplies by gamma: keep the fp32 values on the device (1.47 GB for ViT-H, of 288)
            if (h->fold && name.rfind("image_encoder.blocks.", 0) == 0 && (ends_with(name, "attn.qkv.weight") || ends_with(name, "mlp.lin1.weight"))) {
                float* d32 = nullptr;
                WM_TRY(dalloc(h, &d32, n * 4));
                HIP_TRY(hipMemcpy(d32, w.data.data(), n * 4, hipMemcpyHostToDevice));
                h->wsrc32[name] = d32;
            }
        } else {
            WM_TRY(upload32(h, name, w.data.data(), n));
        }
    }
    // dense positional encoding, token-major (pos_encoder.py:50-70)
    if (h->staged.count("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix")) {
        const HostW& g = h->staged["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"];
        const int F = OUTC / 2;
        std::vector<float> pe((size_t)T * OUTC);
        for (int y = 0; y < GRID; ++y)
            for (int x = 0; x < GRID; ++x) {
                const float cx = 2.0f * ((x + 0.5f) / GRID) - 1.0f, cy = 2.0f * ((y + 0.5f) / GRID) - 1.0f;
                for (int f = 0; f < F; ++f) {
                    float arg = cx * g.data[f] + cy * g.data[F + f];
                    arg = arg * 6.283185307179586f;
                    pe[(size_t)(y * GRID + x) * OUTC + f] = (float)sin((double)arg);
                    pe[(size_t)(y * GRID + x) * OUTC + F + f] = (float)cos((double)arg);
                }
            }
        HIP_TRY(hipMemcpy(h->kpe, pe.data(), pe.size() * 4, hipMemcpyHostToDevice));
    }
    // Folded LayerNorm: gamma (.) W (LDS-image order), c1, c2 of every block's qkv (norm1) and lin1 (norm2), from the DEVICE
    // copies of the fp32 weights (kept above), so a later partial re-upload folds to the same bits as a full one.
    if (h->fold && h->enc_ready) {
        for (int i = 0; i < h->depth; ++i) {
            const std::string b = "image_encoder.blocks." + std::to_string(i) + ".";
            const int P = block_prec(h, i) == WM_PREC_FP8 ? WM_PREC_BF16 : block_prec(h, i);
            const std::pair<const char*, const char*> pairs[] = {{"attn.qkv", "norm1"}, {"mlp.lin1", "norm2"}};
            for (const auto& pr : pairs) {
                const std::string wn = b + pr.first + ".weight";
                if (!h->w16.count(wn)) continue;            // an fp8 GEMM of this block: no 16-bit weight, no fold
                const int N = (int)h->expected.at(wn)[0], K = (int)h->expected.at(wn)[1];
                if (!h->wfold.count(wn)) {
                    uint16_t* wf = nullptr; float *c1 = nullptr, *c2 = nullptr;
                    WM_TRY(dalloc(h, &wf, (size_t)N * K * 2)); WM_TRY(dalloc(h, &c1, (size_t)N * 4)); WM_TRY(dalloc(h, &c2, (size_t)N * 4));
                    h->wfold[wn] = wf; h->fold_c1[wn] = c1; h->fold_c2[wn] = c2;
                }
                const float* g = h->w32.at(b + pr.second + ".weight");
                const float* be = h->w32.at(b + pr.second + ".bias");
                const float* bias = h->w32.at(b + pr.first + ".bias");
                WM_TRY(launch_fold_weight(0, P, h->w16.at(wn), h->fold_from16 ? nullptr : h->wsrc32.at(wn), g, be, bias, h->wfold[wn], h->fold_c1[wn], h->fold_c2[wn], N, K));
            }
        }
    }
    HIP_TRY(hipDeviceSynchronize());        // the pack / fold launches above
    h->staged.clear();
    h->finalized = true;
    return 0;
}

}  // namespace
