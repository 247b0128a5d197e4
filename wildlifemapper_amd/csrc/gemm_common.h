// What the 16-bit and fp8 MFMA GEMM kernels share (gemm16.h, gemm16_v2.h, gemm16_v3.h, gemm16_v5.h, gemm8.h): the argument block,
// the activation codes, the grouped tile order, the counted vmcnt wait, and the epilogue arithmetic.
//
// The epilogue arithmetic is defined HERE ONLY because a tile's bits must not depend on which kernel its batch size selects
// (tests/test_gpu_ops.py test_gemm16_kernels_agree_bitwise, test_gemm16_v1_128_kernel): every kernel accumulates K in
// ascending 32-wide MFMA steps with the same operand roles and then applies bias, gemm_act, residual in this order.
#pragma once
#include "wm_common.h"

namespace wm {

constexpr int G16_GROUP_M = 8;

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_SIGMOID = 3 };

struct Gemm16Args {
    const u16* A;
    const u16* W;
    const float* bias;       // [N] or null
    const float* residual;   // [res_mod, N] fp32 or null
    float* out32;            // [M,N] or null
    u16* out16;              // [M,N] or null
    int M, N, K;
    int res_mod;             // rows of residual (M, or 4096 for a per-tile broadcast)
    int act;
    // implicit-GEMM A operand (gemm16_v3.h).  Conv3x3: A is an NHWC activation [M = B*64*64, conv_c] and the GEMM's K runs over
    // (tap, channel) of a 3x3 / pad 1 convolution, K = 9 * conv_c; out-of-image taps read `zero_page` (>= 64 B of zeros).
    // PatchEmbed: A is the 16-bit NCHW image with conv_c channels.  Unused (0 / null) for a plain A matrix.
    int conv_c;
    const u16* zero_page;
    // row tiles per group of the grouped tile order (gemm16_v5.h; 0 = G16_GROUP_M): a group's row tiles x all column tiles
    // are consecutive tile ids, so group_m * tilesN ~ the 32 workgroups co-resident on an XCD keeps each A panel to one XCD
    int group_m;
    // gemm16_v5.h only: W / A stored in LDS-image order ([rows / 16][K / 32][64 x 16 B], pack16_lds_image_kernel); out_packed:
    // the 16-bit output is written in that order (it is the next GEMM's A operand; N % 32 == 0)
    int w_packed, a_packed, out_packed;
    // Folded LayerNorm (gemm16_v5.h "Folded LayerNorm").  Producer (FOLDP instance, fp32 + residual epilogue): st_stats
    // [M][N / BN][2] receives each row's (mean, M2) over this tile's columns, out16 the finished rows as 16-bit in LDS-image
    // order.  Consumer (16-bit epilogue): A is such a 16-bit copy x16 and W = gamma (.) W; with fold_stats = the producer's
    // partials over fold_ntile tiles of fold_bn columns (fold_ntile * fold_bn = K), fold_c1[n] = sum_k W[n][k] and
    // bias[n] = sum_k beta[k] W0[n][k] + b[n] the epilogue computes rstd (acc - mean c1) + bias = LayerNorm(x) W0^T + b.
    float* st_stats;
    const float* fold_stats;
    const float* fold_c1;
    int fold_ntile;
    float fold_bn, fold_eps;
    // Split residual stream (gemm16_v5.h "Split stream", round 4): the stream x as two 16-bit planes in LDS-image order,
    // hi = T(x) (the folded LayerNorm's operand) and lo = fp16(x - hi).  SPLIT instance: the residual comes in as
    // (res_hi, res_lo) and leaves as (out16 = hi, out_lo); the FOLDP instance (fp32 residual in) writes out_lo too when it is
    // given and then skips out32 when that is null.  overflow: a host-visible word the producers set to 1 when a value of the
    // stream reaches the fp16 clamp (|x| >= 65504), or null.
    const u16* res_hi;
    const u16* res_lo;
    u16* out_lo;
    int* overflow;
    // Folded-LayerNorm consumer only (gemm16_v5.h "Column walk"): column tiles per workgroup, 0 | 1 = one (the grid is then
    // tilesM * tilesN workgroups, otherwise tilesM * tilesN / walk; walk divides tilesN / 4, see walk_tile_origin)
    int walk;
};

// s_waitcnt vmcnt(N) with N a template argument (the instruction takes an immediate)
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 12, "extend the table");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
}

// Grouped tile order behind the XCD remap: workgroup `wg` of `nwg` -> origin (m0, n0) of its BM x BN tile among tilesM x tilesN.
// `group_m` row tiles (0 = G16_GROUP_M) x all column tiles are consecutive tile ids, so the row tiles of a group share each W
// panel back to back; the last group may hold fewer row tiles.
struct TileOrigin { int m0, n0; };
template <int BM, int BN>
__device__ __forceinline__ TileOrigin grouped_tile_origin(int tilesM, int tilesN, int wg, int nwg, int group_m) {
    const int t = xcd_remap(wg, nwg);
    const int gm = group_m > 0 ? group_m : G16_GROUP_M;
    const int per_group = gm * tilesN;
    const int group = t / per_group;
    const int first_m = group * gm;
    const int gsz = min(gm, tilesM - first_m);
    const int in_group = t - group * per_group;
    return {(first_m + in_group % gsz) * BM, (in_group / gsz) * BN};
}

// The same order for workgroups that each walk `walk` column tiles of one row tile (gemm16_v5.h "Column walk").  The tilesN columns
// are cut into blocks of 4 * walk; a workgroup owns one SLOT = (row tile, column block, lane 0..3 of the block) and its tile at step t of
// the walk is column (block * walk + t) * 4 + lane: n0 advances by 4 BN per step and m0 stays.  The slots are numbered like the tiles
// above with tilesN / walk columns, so at every step the 32 consecutive slots of an XCD still cover group_m = 8 row tiles x 4
// neighbouring column tiles, and over the walk every tile is computed exactly once.  walk == 1 is grouped_tile_origin itself.
// Needs tilesN % (4 * walk) == 0 for walk > 1 (the launcher checks); nwg = tilesM * tilesN / walk.
template <int BM, int BN>
__device__ __forceinline__ TileOrigin walk_tile_origin(int tilesM, int tilesN, int wg, int nwg, int group_m, int walk) {
    const TileOrigin slot = grouped_tile_origin<BM, 1>(tilesM, tilesN / walk, wg, nwg, group_m);
    return {slot.m0, (((slot.n0 >> 2) * walk) * 4 + (slot.n0 & 3)) * BN};
}

// The activation of a GEMM epilogue: GELU (the fast erf form), ReLU or none ...
__device__ __forceinline__ f32x4 gemm_act(f32x4 v, int act) {
    if (act == ACT_GELU) {
        v = gelu_erf_fast4(v);
    } else if (act == ACT_RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    }
    return v;
}
// ... and with the activation known at compile time (gemm16_v5.h: one straight-line epilogue per activation)
template <int ACT> __device__ __forceinline__ f32x4 gemm_act(f32x4 v) { return gemm_act(v, ACT); }

// Direct epilogue, straight from the MFMA layout: the lane holds v = C[m][n .. n + 3].  bias, activation, residual row
// m % res_mod, then the fp32 (16 B) and / or 16-bit (8 B) store.
template <class T>
__device__ __forceinline__ void gemm16_direct_epilogue(const Gemm16Args& p, f32x4 v, int m, int n, int act, int res_mod) {
    if (p.bias) v += *(const f32x4*)(p.bias + n);
    v = gemm_act(v, act);
    if (p.residual) v += *(const f32x4*)(p.residual + (size_t)(m % res_mod) * p.N + n);
    if (p.out32) *(f32x4*)(p.out32 + (size_t)m * p.N + n) = v;
    if (p.out16) {
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = T::from_f32(v[j]);
        *(typename T::vec4*)(p.out16 + (size_t)m * p.N + n) = o;
    }
}

}  // namespace wm
