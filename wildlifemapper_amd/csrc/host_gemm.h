// GEMM launchers: the 16-bit kernels and their dispatch, fp8, the implicit-GEMM conv / patch embed, the decoder's fp32 forms.
#pragma once
#include "gemm16.h"
#include "gemm16_v2.h"
#include "gemm16_v3.h"
#include "gemm16_v5.h"
#include "gemm32.h"
#include "gemm8.h"
#include "misc_kernels.h"
#include "host_core.h"

namespace {

// algorithmic flops / bytes of a 16-bit GEMM launch as the profile counts them: operands (2 B per element), the outputs, the residual
double gemm16_flops(const Gemm16Args& a) { return 2.0 * a.M * (double)a.N * a.K; }
double gemm16_bytes(const Gemm16Args& a) {
    return 2.0 * ((double)a.M * a.K + (double)a.N * a.K) + (a.out32 ? 4.0 : 0.0) * a.M * a.N + (a.out16 ? 2.0 : 0.0) * a.M * a.N +
           (a.residual ? 4.0 * (double)(a.res_mod > 0 ? a.res_mod : a.M) * a.N : 0.0);
}

// The launch sequence of the family's kernels: raise the kernel's dynamic-LDS limit (once per kernel and device), count the variant
// (variant < 0: the caller has), open the profile bracket, launch, check.
template <class Kern, class Args>
int launch_gemm_kernel(wm_handle* h, hipStream_t s, Kern kern, int grid, int threads, int lds, const Args& a, int variant, double flops, double bytes) {
    WM_TRY(set_max_lds((const void*)kern, lds));
    if (variant >= 0) count_variant(variant);
    Bracket br(h, s, WM_KCLASS_GEMM16, flops, bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <class T16>
int launch_gemm16_t(wm_handle* h, hipStream_t s, const Gemm16Args& a) {
    return launch_gemm_kernel(h, s, gemm16_kernel<T16>, (a.M / G16_BM) * (a.N / G16_BN), 256, G16_LDS_BYTES, a, WM_GEMM_V1_128, gemm16_flops(a), gemm16_bytes(a));
}

template <class T16, int BN>
int launch_gemm16v2_t(wm_handle* h, hipStream_t s, const Gemm16Args& a) {
    return launch_gemm_kernel(h, s, gemm16v2_kernel<T16, BN>, (a.M / 256) * (a.N / BN), 512, G2<BN>::LDS, a, BN == 160 ? WM_GEMM_V2_160 : WM_GEMM_V2_128,
                              gemm16_flops(a), gemm16_bytes(a));
}

// The 256-row-tile kernel (gemm16_v5.h); FOLDP / FOLDC / SPLIT / NSLOT are the kernel's own flags: the folded LayerNorm's producer
// (statistics out; SPLIT: the stream as two 16-bit planes) and consumer (normalisation in the epilogue), ring slots.
// Column tiles per workgroup of the folded-LayerNorm consumer (gemm16_v5.h "Column walk"), by the launch's column tiles: the T that
// measured fastest at the block shapes (profiles/gemm_walk/kernel_ab.txt; qkv has 12 column tiles of 320, lin1 16).
static int gemm16_walk_table(int tilesN) { return tilesN == 12 ? 3 : tilesN == 16 ? 4 : 1; }
// What a launch walks.  `asked` > 0 (the op-level entry) is taken as it is, 0 asks the table, and the table's T holds only while the
// walking grid is still at least two rounds of 256 workgroups (8 ViT-H tiles per call; measured at 16 = four rounds): a smaller call
// keeps one tile per workgroup, so that no CU goes idle, and the launch plans recorded for 1 to 4 tiles per call
// (tests/encoder_cases.py) stay what they are.  Any T that does not divide tilesN / 4 (walk_tile_origin) falls back to 1.
static int gemm16_walk_for(int tilesM, int tilesN, int asked) {
    int t = asked > 0 ? asked : gemm16_walk_table(tilesN);
    if (asked <= 0 && t > 1 && (long)tilesM * tilesN / t < 2 * 256) t = 1;
    if (t > 1 && (tilesN % 4 || (tilesN / 4) % t)) t = 1;
    return t;
}

template <class T16, int BN, bool FOLDP, bool FOLDC, bool SPLIT, int NSLOT = 3>
int launch_gemm16v5_t(wm_handle* h, hipStream_t s, const Gemm16Args& a_in) {
    using G = G3<BN>;
    constexpr int LDS = NSLOT * G::STAGE + 32 * BN * 4;        // ring + the first residual landing buffer
    static_assert(LDS <= 160 * 1024, "LDS");
    WM_TRY(set_max_lds((const void*)gemm16v5_kernel<T16, BN, NSLOT, false, FOLDP, FOLDC, SPLIT>, LDS));
    // (the consumer counts as the 16-bit-output instance it is, with the folded LayerNorm's epilogue)
    count_variant(SPLIT   ? (BN == 320 ? WM_GEMM_V5_320_SPLIT : WM_GEMM_V5_256_SPLIT)
                  : FOLDP ? (BN == 320 ? WM_GEMM_V5_320_FOLDP : WM_GEMM_V5_256_FOLDP)
                  : BN == 320 ? (a_in.residual ? WM_GEMM_V5_320_RES : WM_GEMM_V5_320) : (a_in.residual ? WM_GEMM_V5_256_RES : WM_GEMM_V5_256));
    Gemm16Args a = a_in;
#if WM_DEV_TIMELINE
    dev_group_m(a);
    if (FOLDC) dev_walk(a);
#endif
    a.walk = FOLDC ? gemm16_walk_for(a.M / 256, a.N / BN, a.walk) : 1;
    if (a.walk > 1) count_variant(BN == 320 ? WM_GEMM_V5_320_WALK : WM_GEMM_V5_256_WALK);       // a walking consumer: under its own name too
    const int grid = (a.M / 256) * (a.N / BN) / a.walk;
    // a producer's bytes: operands + the stream in and out (split: 2 + 2 B in, 2 + 2 B out; fp32: 4 in, 4 + 2 out, or 2 + 2 out with a lo plane)
    const double stream_bytes = SPLIT ? 8.0 : 4.0 + (a.out32 ? 4.0 : 0.0) + 2.0 + (a.out_lo ? 2.0 : 0.0);
    Bracket br(h, s, WM_KCLASS_GEMM16, gemm16_flops(a),
               FOLDP ? 2.0 * ((double)a.M * a.K + (double)a.N * a.K) + stream_bytes * a.M * a.N : gemm16_bytes(a));
    WM_DEV_HOOK((dev_gemm16v5_timeline<T16, BN, NSLOT, FOLDP, FOLDC>(s, a, grid, LDS)));     // between bracket and launch: not the helper's sequence
    hipLaunchKernelGGL((gemm16v5_kernel<T16, BN, NSLOT, false, FOLDP, FOLDC, SPLIT>), dim3(grid), dim3(512), LDS, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <bool FOLDP, bool FOLDC, bool SPLIT>
int launch_gemm16v5(wm_handle* h, hipStream_t s, int prec, const Gemm16Args& a) {
    return by_type16(prec, [&](auto t) {
        return by_tile_width(a.N, [&](auto bn) { return launch_gemm16v5_t<decltype(t), decltype(bn)::value, FOLDP, FOLDC, SPLIT>(h, s, a); });
    });
}

// fraction of the last round of workgroup slots that is filled
static double round_eff(long tiles, long slots) { return (double)tiles / (double)(((tiles + slots - 1) / slots) * slots); }

// The staggered 256 x 320 / 256 x 256 kernel (gemm16_v5.h) serves the shape: the only kernel that reads operands in
// LDS-image order and writes its 16-bit output in it.  Few tiles (one or two image tiles per call): the half-width
// 256 x 160 / 128 kernel fills more CUs; cost model from tools/gemm_bench.py --batch 1: rounds of 256 workgroups x (1.0 | 0.6) per tile.
static bool gemm16_v5_serves(int M, int N, int K) {          // what the kernel can run at all
    return M > 0 && M % 256 == 0 && K > 0 && K % 32 == 0 && K / 32 >= 2 && N > 0 && (N % 320 == 0 || N % 256 == 0);
}
static bool gemm16_takes_v5(int M, int N, int K) {
    if (!gemm16_v5_serves(M, N, K) || K % G16_BK) return false;
    auto prefer_half = [&](int bn) {
        const long t = (long)(M / 256) * (N / bn);
        return (double)((2 * t + 255) / 256) * 0.6 < (double)((t + 255) / 256);
    };
    if (N % 320 == 0) return !prefer_half(320);
    if (N % 256 == 0) return !prefer_half(256);
    return false;
}

// Options of a launch that only the gemm16_v5 kernel has (the caller asks gemm16_takes_v5 first; a mismatch is an error):
//   Wp: the weight in LDS-image order (or null); a_packed / out_packed: A is / the 16-bit output shall be in that order;
//   st_stats: folded-LayerNorm PRODUCER (fp32 + residual form): per-row partial statistics out, out16 = 16-bit copy of the
//             rows in LDS-image order;
//   fold_stats / fold_c1 / fold_eps: folded-LayerNorm CONSUMER (16-bit-only form): A = such a copy, W = gamma (.) W, bias = c2;
//             walk: its column tiles per workgroup (0 = the launcher's choice).
//   res_hi / res_lo / out_lo: split stream (gemm16_v5.h "Split stream"): with st_stats, the residual as two 16-bit planes in
//             (res_hi, res_lo; no fp32 residual) and out (out16 = hi, out_lo); out_lo alone: the fp32-residual producer also
//             writes the lo plane (and no fp32 output when out32 is null).
struct GemmExtra {
    const void* Wp = nullptr;
    int a_packed = 0, out_packed = 0;
    float* st_stats = nullptr;
    const float* fold_stats = nullptr;
    const float* fold_c1 = nullptr;
    float fold_eps = 0.f;
    const void* res_hi = nullptr;
    const void* res_lo = nullptr;
    void* out_lo = nullptr;
    int* overflow = nullptr;
    int walk = 0;          // consumer: column tiles per workgroup, 0 = the launcher's table (gemm16_walk_for)
};
static GemmExtra GX(const void* Wp, int a_packed = 0, int out_packed = 0) {
    GemmExtra x;
    x.Wp = Wp; x.a_packed = a_packed; x.out_packed = out_packed;
    return x;
}

int launch_gemm16(wm_handle* h, hipStream_t s, int prec, const void* A, const void* W, const float* bias,
                  const float* res, int res_mod, float* out32, void* out16, int M, int N, int K, int act,
                  const GemmExtra& x = GemmExtra{}) {
    const void* Wp = x.Wp;
    const int a_packed = x.a_packed, out_packed = x.out_packed;
    // a caller that names the consumer's walk (the op-level entry) has chosen the 256-row-tile kernel, whose K-step is 32
    const bool v5_asked = x.walk > 0 && x.fold_stats && gemm16_v5_serves(M, N, K);
    if (!v5_asked && (M <= 0 || N <= 0 || K <= 0 || M % G16_BM || N % G16_BN || K % G16_BK))
        return fail("gemm16: shape M=%d N=%d K=%d must be multiples of %d/%d/%d", M, N, K, G16_BM, G16_BN, G16_BK);
    if (!out32 && !out16) return fail("gemm16: no output");
    Gemm16Args a{};
    a.A = (const u16*)A; a.W = (const u16*)W; a.bias = bias; a.residual = res; a.out32 = out32; a.out16 = (u16*)out16;
    a.M = M; a.N = N; a.K = K; a.res_mod = res_mod; a.act = act;
    if (gemm16_takes_v5(M, N, K) || v5_asked) {         // staggered wave groups (gemm16_v5.h)
        if (Wp) { a.W = (const u16*)Wp; a.w_packed = 1; }
        a.a_packed = a_packed;
        a.out_packed = out_packed;
        if (out_packed && (out32 || res || !out16)) return fail("gemm16: a packed output is the 16-bit-only form (no fp32 output, no residual)");
        if (x.st_stats) {                   // folded LayerNorm, producer
            const bool split = x.res_hi != nullptr;
            if (!out16 || act != ACT_NONE || N / fold_bn_for(N) > 4 || N % 32)
                return fail("gemm16: the statistics-producing form has a 16-bit copy, no activation, at most 4 column tiles");
            if (split ? (res || out32 || !x.res_lo || !x.out_lo || res_mod) : (!res || (!out32 && !x.out_lo)))
                return fail("gemm16: the statistics-producing form takes an fp32 residual (fp32 and / or lo-plane output) or the two planes of a split stream (planes out)");
            a.st_stats = x.st_stats;
            a.res_hi = (const u16*)x.res_hi; a.res_lo = (const u16*)x.res_lo; a.out_lo = (u16*)x.out_lo; a.overflow = x.overflow;
            return split ? launch_gemm16v5<true, false, true>(h, s, prec, a) : launch_gemm16v5<true, false, false>(h, s, prec, a);
        }
        if (x.fold_stats) {                 // folded LayerNorm, consumer
            const int bn = K < 256 ? K : fold_bn_for(K);        // (a K shorter than a statistics tile is one tile: op-level tests of short K loops)
            if (out32 || res || !out16 || !x.fold_c1 || !bias || (act != ACT_NONE && act != ACT_GELU) || K % bn || K / bn > 4 || !Wp || !a_packed)
                return fail("gemm16: the folded-LayerNorm form is 16-bit-only output, act none | GELU, operands in LDS-image order, K a multiple of %d with at most 4 tiles", bn);
            a.fold_stats = x.fold_stats; a.fold_c1 = x.fold_c1; a.fold_ntile = K / bn; a.fold_bn = (float)bn; a.fold_eps = x.fold_eps;
            a.walk = x.walk;
            return launch_gemm16v5<false, true, false>(h, s, prec, a);
        }
        return launch_gemm16v5<false, false, false>(h, s, prec, a);
    }
    if (a_packed || out_packed || x.st_stats || x.fold_stats || x.res_hi || x.out_lo)
        return fail("gemm16: M=%d N=%d K=%d runs on a half-width kernel, which takes row-major operands only", M, N, K);
    if (M % 256 == 0) {
        // half-width tiles: 256 x 160 where N allows and it fills the last round at least as well as 256 x 128
        const bool can160 = N % 160 == 0;
        const bool use160 = can160 && (N % 320 == 0 || round_eff((long)(M / 256) * (N / 160), 256) >= round_eff((long)(M / 256) * (N / 128), 256) - 1e-9);
        return by_type16(prec, [&](auto t) { return use160 ? launch_gemm16v2_t<decltype(t), 160>(h, s, a) : launch_gemm16v2_t<decltype(t), 128>(h, s, a); });
    }
    return by_type16(prec, [&](auto t) { return launch_gemm16_t<decltype(t)>(h, s, a); });
}

// fp8 GEMM (gemm8.h).  prec16 = type of a 16-bit output.  K-step 128 (the 64-byte / 4-slot variant measured equal or
// 1-3 % slower: tools/experiments/gemm8_bk64.h, profiles/r2_dev/gemm8_bench_b16_bk64.txt).
template <class T16, bool PLANES = false>
int launch_gemm8_t(wm_handle* h, hipStream_t s, Gemm8Args a, int grid, double flops, double bytes) {
    WM_DEV_HOOK((dev_gemm8_timeline<T16, PLANES>(s, a, grid)));
    return launch_gemm_kernel(h, s, gemm8_kernel<T16, false, PLANES>, grid, 512, G8::LDS, a, -1, flops, bytes);
}

int launch_gemm8(wm_handle* h, hipStream_t s, int prec16, const void* A, const void* W, const float* wscale, const float* bias,
                 const float* res, float* out32, void* out16, void* out8, int M, int N, int K, int act, void* hi = nullptr, void* lo = nullptr) {
    if (M <= 0 || N <= 0 || K <= 0 || M % G8_BM || N % G8_BN || K % 128 || K < 256)
        return fail("gemm8: shape M=%d N=%d K=%d must be multiples of %d/%d/128 with K >= 256", M, N, K, G8_BM, G8_BN);
    if (!A || !W || !wscale) return fail("gemm8: null operand");
    if (hi || lo) {                                         // the stream's row-major planes, updated in place (gemm8.h PLANES)
        if (!hi || !lo || res || out32 || out16 || out8 || act != ACT_NONE) return fail("gemm8: the plane form takes (hi, lo) and nothing else");
        Gemm8Args a{(const unsigned char*)A, (const unsigned char*)W, wscale, bias, nullptr, nullptr, nullptr, nullptr, M, N, K, act, nullptr,
                    (const u16*)hi, (const u16*)lo, (u16*)hi, (u16*)lo};
        count_variant(WM_GEMM_FP8_256_PLANES);
        const double flops = 2.0 * M * (double)N * K, bytes = (double)M * K + (double)N * K + 8.0 * M * N;
        return by_type16(prec16, [&](auto t) { return launch_gemm8_t<decltype(t), true>(h, s, a, (M / G8_BM) * (N / G8_BN), flops, bytes); });
    }
    const int modes = (res != nullptr) + (out8 != nullptr) + (res == nullptr && out8 == nullptr && out16 != nullptr);
    if (modes != 1 || (res && !out32 && !out16) || (!res && out32)) return fail("gemm8: outputs must be (residual + out32 [+ out16]) | out8 | out16");
    Gemm8Args a{(const unsigned char*)A, (const unsigned char*)W, wscale, bias, res, out32, (u16*)out16, (unsigned char*)out8, M, N, K, act, nullptr,
                nullptr, nullptr, nullptr, nullptr};
    const int grid = (M / G8_BM) * (N / G8_BN);
    count_variant(WM_GEMM_FP8_256);
    const double flops = 2.0 * M * (double)N * K;
    const double bytes = (double)M * K + (double)N * K + (res ? 8.0 : 0.0) * M * N + (out16 ? 2.0 : 0.0) * M * N + (out8 ? 1.0 : 0.0) * M * N;
    return by_type16(prec16, [&](auto t) { return launch_gemm8_t<decltype(t)>(h, s, a, grid, flops, bytes); });
}

// 3x3 / pad 1 convolution over an NHWC [B,64,64,C] 16-bit activation as an implicit GEMM (no im2col buffer):
// out[M = B*4096, N] = conv(A) with W packed [N][tap][C]  (image_encoder.py:113-119)
int launch_conv3x3_16(wm_handle* h, hipStream_t s, int prec, const void* A, const void* W, float* out32, int M, int N, int Cin) {
    if (M % 4096 || N % 256 || Cin % 32) return fail("conv3x3: M=%d N=%d C=%d unsupported (M %% 4096, N %% 256, C %% 32)", M, N, Cin);
    const uint16_t* zero_page = nullptr;       // 256 B of zeros for out-of-image taps (one per device)
    WM_TRY(zero_page_for_device(&zero_page));
    Gemm16Args a{};
    a.A = (const u16*)A; a.W = (const u16*)W; a.out32 = out32; a.M = M; a.N = N; a.K = 9 * Cin; a.act = ACT_NONE; a.conv_c = Cin; a.zero_page = (const u16*)zero_page;
    using G = G3<256>;
    count_variant(WM_GEMM_V3_CONV3X3);
    return by_type16(prec, [&](auto t) {
        return launch_gemm_kernel(h, s, gemm16v3_kernel<decltype(t), 256, ALoad::Conv3x3>, (M / 256) * (N / 256), G::THREADS, G::LDS, a, -1,
                                  2.0 * M * (double)N * 9 * Cin, 2.0 * ((double)M * Cin + 9.0 * N * Cin) + 4.0 * M * N);
    });
}

// 16 x 16 / stride-16 patch embed as an implicit GEMM (gemm16_v3.h ALoad::PatchEmbed): img16 [B][Cin][1024][1024] 16-bit, W [N][Cin * 256]
// row-major, out[M = B * 4096][N] = patches W^T + bias (+ residual[m % res_mod])  (image_encoder.py:386-450)
int launch_patch_embed16(wm_handle* h, hipStream_t s, int prec, const void* img16, const void* W, const float* bias, const float* res, int res_mod,
                         float* out32, void* out16, int B, int N, int Cin) {
    const int M = B * 4096, K = Cin * 256;
    if (B <= 0 || (N % 320 && N % 256) || Cin <= 0) return fail("patch_embed: B=%d N=%d Cin=%d unsupported (N %% 320 or N %% 256)", B, N, Cin);
    if (!out32 && !out16) return fail("patch_embed: no output");
    Gemm16Args a{};
    a.A = (const u16*)img16; a.W = (const u16*)W; a.bias = bias; a.residual = res; a.out32 = out32; a.out16 = (u16*)out16;
    a.M = M; a.N = N; a.K = K; a.res_mod = res_mod; a.act = ACT_NONE; a.conv_c = Cin;
    count_variant(WM_GEMM_V3_PATCH);
    const double bytes = 2.0 * ((double)M * K + (double)N * K) + (out32 ? 4.0 : 0.0) * M * N + (out16 ? 2.0 : 0.0) * M * N;
    return by_type16(prec, [&](auto t) {
        return by_tile_width(N, [&](auto bn) {
            constexpr int BN = decltype(bn)::value;
            using G = G3<BN>;
            return launch_gemm_kernel(h, s, gemm16v3_kernel<decltype(t), BN, ALoad::PatchEmbed>, (M / 256) * (N / BN), G::THREADS, G::LDS, a, -1,
                                      2.0 * M * (double)N * K, bytes);
        });
    });
}

// fp32 GEMM (the decoder).  mode: 0 = the engine's choice (the fp16-split form on the 16-bit matrix pipe, gemm32.h gemm32x3_kernel,
// where K % 32 == 0, with W pre-split once per weight upload; WM_GEMM32_F32=1 keeps the fp32-MFMA kernel: A/B runs), 1 = the fp32-MFMA
// kernel, 2 = the split form with W split per K-step (op-level entry: no handle to cache planes in), 3 = the engine's form without a
// handle: W split by split_w32_kernel into the stream's scratch planes, then gemm32x3_kernel<true> (op-level entry, WM_GEMM32_PRESPLIT)
int launch_gemm32(wm_handle* h, hipStream_t s, const float* A, const float* W, const float* bias, const float* res,
                  float* out, int M, int N, int K, int act, int lda = 0, int mode = 0) {
    if (K % 16) return fail("gemm32: K=%d must be a multiple of 16", K);
    static const bool f32_only = getenv("WM_GEMM32_F32") && atoi(getenv("WM_GEMM32_F32")) != 0;
    if ((mode == 2 || mode == 3) && K % 32) return fail("gemm32 (split form): K=%d must be a multiple of 32", K);
    if (mode == 2 || mode == 3 || (mode == 0 && h && !f32_only && K % 32 == 0)) {
        Gemm32x3Args a{A, W, nullptr, nullptr, bias, res, out, M, N, K, act, lda > 0 ? lda : K, h ? h->overflow + 1 : nullptr};
        if (mode == 3) {                                    // no handle to cache the planes in: the stream's scratch, split on every call
            const size_t n = (size_t)N * K;                 // K % 32 == 0: n % 4 == 0
            void* pb = nullptr;
            WM_TRY(op_scratch(s, 3, n * 4, &pb));
            u16* hi = (u16*)pb;
            hipLaunchKernelGGL(split_w32_kernel, dim3(grid_for((int64_t)n / 4)), dim3(256), 0, s, W, hi, hi + n, (int64_t)n / 4, (int*)nullptr);
            HIP_TRY(hipGetLastError());
            a.Whi = hi; a.Wlo = hi + n;
        }
        if (mode == 0) {                                    // the weight's fp16 planes: made at first use, dropped with the weights
            auto it = h->w32x3.find(W);
            if (it == h->w32x3.end()) {
                uint16_t *hi = nullptr, *lo = nullptr;
                const size_t n = (size_t)N * K;
                if (n % 4) return fail("gemm32: weight of %zu elements", n);
                WM_TRY(dalloc(h, &hi, n * 2)); WM_TRY(dalloc(h, &lo, n * 2));
                hipLaunchKernelGGL(split_w32_kernel, dim3(grid_for((int64_t)n / 4)), dim3(256), 0, s, W, (u16*)hi, (u16*)lo, (int64_t)n / 4, h->overflow + 1);
                HIP_TRY(hipGetLastError());
                it = h->w32x3.emplace(W, std::make_pair(hi, lo)).first;
            }
            a.Whi = (const u16*)it->second.first; a.Wlo = (const u16*)it->second.second;
        }
        Bracket br(h, s, WM_KCLASS_OTHER, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)M * N) + 4.0 * (double)N * K);
        const dim3 grid(((N + 63) / 64) * ((M + 63) / 64));
        if (mode == 0 || mode == 3) hipLaunchKernelGGL(gemm32x3_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(gemm32x3_kernel<false>, grid, dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    Gemm32Args a{A, W, bias, res, out, M, N, K, act, lda > 0 ? lda : K};
    Bracket br(h, s, WM_KCLASS_OTHER, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    hipLaunchKernelGGL(gemm32_kernel, dim3(((N + 63) / 64) * ((M + 63) / 64)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
