// LayerNorm launchers (general, the blocks' column-tiled form, the fp8 planes' form), the folded LayerNorm's standalone
// statistics, the split stream's merge / row passes and the saturation census.
#pragma once
#include "misc_kernels.h"
#include "host_core.h"

namespace {

int launch_layernorm(wm_handle* h, hipStream_t s, int prec, const float* x, const float* g, const float* b, float eps,
                     float* out32, void* out16, int64_t rows, int C, int nchw_hw = 0) {
    if (C % 256 || C > 1280) return fail("layernorm: C=%d unsupported (multiple of 256, <= 1280)", C);
    if (prec != WM_PREC_BF16 && prec != WM_PREC_FP16)
        return fail("layernorm: precision %d has no fp32-output / general form (e4m3 output exists only for the blocks' 16-bit-only form)", prec);
    const dim3 grid((unsigned)((rows + 3) / 4));
    Bracket br(h, s, WM_KCLASS_LAYERNORM, 0.0, (double)rows * C * (4.0 + (out32 ? 4.0 : 0.0) + (out16 ? 2.0 : 0.0)));
    return by_type16(prec, [&](auto t) {
        auto go = [&](auto nv) {
            hipLaunchKernelGGL((layernorm_kernel<decltype(t), decltype(nv)::value>), grid, dim3(256), 0, s, x, g, b, eps, out32, (u16*)out16, rows, nchw_hw);
            HIP_TRY(hipGetLastError());
            return 0;
        };
        switch (C / 256) {
            case 1: return go(int_c<1>{});
            case 2: return go(int_c<2>{});
            case 3: return go(int_c<3>{});
            case 4: return go(int_c<4>{});
            case 5: return go(int_c<5>{});
            default: return fail("layernorm: C=%d", C);
        }
    });
}

// LayerNorm of the transformer blocks (norm1 / norm2, 16-bit output): column-tiled statistics, the same
// statistics arithmetic as the folded LayerNorm's producers (ln_partial16 / ln_combine).
int launch_layernorm_block(wm_handle* h, hipStream_t s, int prec, const float* x, const float* g, const float* b, float eps,
                           void* out16, int64_t rows, int C, int packed = 0) {
    const int bn = fold_bn_for(C);
    const bool tiled = C % bn == 0 && C / bn <= 4;
    if (!tiled && prec == WM_PREC_FP8) return fail("layernorm: C=%d has no e4m3 form", C);
    if (packed && (prec == WM_PREC_FP8 || !tiled || rows % 16 || C % 32))
        return fail("layernorm: no LDS-image-order output for rows=%lld C=%d precision %d", (long long)rows, C, prec);
    if (!tiled) return launch_layernorm(h, s, prec, x, g, b, eps, nullptr, out16, rows, C);
    const dim3 grid((unsigned)((rows + 3) / 4));
    Bracket br(h, s, WM_KCLASS_LAYERNORM, 0.0, (double)rows * C * (prec == WM_PREC_FP8 ? 5.0 : 6.0));
    by_tile_width(C, [&](auto bnc) {
        auto go = [&](auto t) {
            hipLaunchKernelGGL((layernorm_tiled_kernel<decltype(t), decltype(bnc)::value>), grid, dim3(256), 0, s, x, g, b, eps, (u16*)out16, rows, C, packed);
        };
        if (prec == WM_PREC_FP8) go(FP8{});             // e4m3 output (never packed: checked above)
        else by_type16(prec, go);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// LayerNorm of the fp8 blocks on the stream's hi plane: plane order in, e4m3 in plane order out (layernorm_plane_fp8_kernel)
int launch_layernorm_plane8(wm_handle* h, hipStream_t s, int in16, const void* hi, const float* g, const float* b, float eps, void* out8, int64_t rows, int C) {
    if (C % 256 || C > 1536 || C < 512 || (in16 != WM_PREC_BF16 && in16 != WM_PREC_FP16)) return fail("layernorm (plane): C=%d type %d", C, in16);
    const dim3 grid((unsigned)((rows + 3) / 4));
    Bracket br(h, s, WM_KCLASS_LAYERNORM, 0.0, (double)rows * C * 3.0);
    by_type16(in16, [&](auto t) {
        auto go = [&](auto nj) {
            hipLaunchKernelGGL((layernorm_plane_fp8_kernel<decltype(t), decltype(nj)::value, 1>), grid, dim3(256), 0, s, (const u16*)hi, g, b, eps, (unsigned char*)out8, rows, C);
        };
        if (C > 1024) go(int_c<3>{}); else go(int_c<2>{});
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// Folded LayerNorm, standalone producer (ln_stats_x16_kernel): partial statistics + 16-bit copy of `rows` fp32 rows of C channels
int launch_ln_stats16(wm_handle* h, hipStream_t s, int prec, const float* x, float* stats, void* x16, int64_t rows, int C,
                      void* lo16 = nullptr, float* x_rw = nullptr, int* overflow = nullptr) {
    const int bn = fold_bn_for(C);
    if (C % bn || C / bn > 4 || rows % 16 || C % 32 || (prec != WM_PREC_FP16 && prec != WM_PREC_BF16))
        return fail("ln_stats16: rows=%lld C=%d precision %d unsupported", (long long)rows, C, prec);
    const dim3 grid((unsigned)((rows + 3) / 4));
    Bracket br(h, s, WM_KCLASS_LAYERNORM, 0.0, (double)rows * C * (6.0 + (lo16 ? 2.0 : 0.0) + (x_rw ? 4.0 : 0.0)));
    by_type16(prec, [&](auto t) {
        by_tile_width(C, [&](auto bnc) {
            hipLaunchKernelGGL((ln_stats_x16_kernel<decltype(t), decltype(bnc)::value>), grid, dim3(256), 0, s, x, stats, (u16*)x16, rows, C, (u16*)lo16, x_rw, overflow);
        });
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// split stream -> fp32 rows (stream_merge_kernel): out[row][col] = float(hi) + float(lo)
int launch_stream_merge(wm_handle* h, hipStream_t s, int prec, const void* hi, const void* lo, float* out, int64_t rows, int C) {
    if (rows % 16 || C % 32 || (prec != WM_PREC_FP16 && prec != WM_PREC_BF16)) return fail("stream_merge: rows=%lld C=%d precision %d", (long long)rows, C, prec);
    Bracket br(h, s, WM_KCLASS_OTHER, 0.0, (double)rows * C * 8.0);
    const dim3 grid(grid_for(rows * (C / 8)));
    by_type16(prec, [&](auto t) { hipLaunchKernelGGL(stream_merge_kernel<decltype(t)>, grid, dim3(256), 0, s, (const u16*)hi, (const u16*)lo, out, rows, C); });
    HIP_TRY(hipGetLastError());
    return 0;
}

// the fp8 blocks' stream: fp32 rows <-> planes of rows (hi of type prec, lo fp16; column c at wm::plane_pos(c))
int launch_stream_rows(wm_handle* h, hipStream_t s, int prec, float* x32, void* hi, void* lo, int64_t rows, int C, bool merge) {
    if (rows <= 0 || C % 256 || (prec != WM_PREC_FP16 && prec != WM_PREC_BF16)) return fail("stream rows: rows=%lld C=%d precision %d", (long long)rows, C, prec);
    const int64_t n = rows * C;
    Bracket br(h, s, WM_KCLASS_OTHER, 0.0, (double)n * 8.0);
    const dim3 grid(grid_for(n / 4));
    by_type16(prec, [&](auto t) {
        if (merge) hipLaunchKernelGGL(stream_merge_rows_kernel<decltype(t)>, grid, dim3(256), 0, s, (const u16*)hi, (const u16*)lo, x32, n / 4, C);
        else hipLaunchKernelGGL(stream_split_rows_kernel<decltype(t)>, grid, dim3(256), 0, s, (const float*)x32, (u16*)hi, (u16*)lo, n / 4, C);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// opt-in census of clamped values in a 16-bit / e4m3 activation buffer (wm_debug_saturation_enable); prec = element type
int sat_check(wm_handle* h, hipStream_t s, int which, const void* buf, int64_t n_elems, int prec) {
    if (!h->sat_on) return 0;
    const int64_t bytes = n_elems * (prec == WM_PREC_FP8 ? 1 : 2);
    if (bytes % 16) return fail("saturation census: buffer of %lld bytes", (long long)bytes);
    const unsigned thr = prec == WM_PREC_FP8 ? 0x7eu : (prec == WM_PREC_FP16 ? 0x7bffu : 0x7f7fu);
    if (prec == WM_PREC_FP8)
        hipLaunchKernelGGL(saturation_count_kernel<1>, dim3(grid_for(bytes / 16)), dim3(256), 0, s, (const uint4*)buf, bytes / 16, thr, h->sat_counts + which);
    else
        hipLaunchKernelGGL(saturation_count_kernel<2>, dim3(grid_for(bytes / 16)), dim3(256), 0, s, (const uint4*)buf, bytes / 16, thr, h->sat_counts + which);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
