// HBM-bound helper kernels: LayerNorm, patch gather, transposes, converts.
#pragma once
#include <type_traits>

#include "wm_common.h"

namespace wm {

// ---------------------------------------------------------------------------
// LayerNorm over the last dim of [rows, C] fp32, biased variance, two-pass in
// registers (nn.LayerNorm / LayerNorm2d per pixel: image_encoder.py:173,183,
// common.py:31-43).  One wave per row, C = 256*NV, 16 B per lane per step.
// Outputs: fp32 [rows,C] and/or 16-bit [rows,C]; or, if nchw_hw > 0, fp32 in
// channel-major order out[(row / hw), c, row % hw] (neck output, NHWC -> NCHW).
// ---------------------------------------------------------------------------
template <class T, int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        float* out32, u16* out16, int64_t rows, int nchw_hw) {
    constexpr int C = NV * 256;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    f32x4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = *(const f32x4*)(xr + i * 256 + lane * 4);
        sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(sum) * (1.0f / C);
    // The mean once more, from the residuals: an fp32 mean is off by up to an ulp of itself, which on a row whose spread is 1e-5
    // of its mean is a percent of the normalised value (tests/test_gpu_layernorm_rows.py, family flat1e-5).  x - mean is exact for
    // x within a factor 2 of the mean, so the residuals' own mean is the correction to fp32 accuracy RELATIVE TO THE SPREAD.
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] -= mean;
        rs += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float corr = wave_sum(rs) * (1.0f / C);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[i][j] -= corr;
            sq += v[i][j] * v[i][j];
        }
    const float var = wave_sum(sq) * (1.0f / C);
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c0 = i * 256 + lane * 4;
        const f32x4 g = *(const f32x4*)(gamma + c0);
        const f32x4 b = *(const f32x4*)(beta + c0);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = v[i][j] * rstd * g[j] + b[j];
        if (nchw_hw > 0) {
            const int64_t img = row / nchw_hw, pix = row % nchw_hw;
#pragma unroll
            for (int j = 0; j < 4; ++j) out32[(img * C + c0 + j) * nchw_hw + pix] = y[j];
        } else {
            if (out32) *(f32x4*)(out32 + row * C + c0) = y;
            if (out16) {
                typename T::vec4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = T::from_f32(y[j]);
                *(typename T::vec4*)(out16 + row * C + c0) = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The transformer blocks' LayerNorm with the column-tiled statistics of wm_common.h (ln_partial16 / ln_combine): the
// statistics of the folded LayerNorm's producers (gemm16_v5.h), operation for operation; applied to x - mean with the mean's
// own rounding removed (see below), which the folded form, holding one fp32 mean per row, cannot do.  One wave per row, 16-lane
// group k owns column tile k (C = TN * BN, TN <= 4), 16-bit output.  grid (rows / 4), 256 threads.
// ---------------------------------------------------------------------------
// store 4 consecutive outputs of type T (16-bit) or, for FP8, as packed e4m3 bytes (wm_common.h)
template <class T>
__device__ __forceinline__ void store4_as(void* base, int64_t elem, const f32x4& y) {
    if constexpr (std::is_same<T, FP8>::value) {
        *(unsigned*)((unsigned char*)base + elem) = pack4_e4m3(y);
    } else {
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = T::from_f32(y[j]);
        *(typename T::vec4*)((u16*)base + elem) = o;
    }
}

// row-major [rows][K] 16-bit -> LDS-image order (weights at wm_finalize_weights; tests).  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void pack16_lds_image_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int64_t rows, int K) {
    const int64_t n16 = rows * (K / 8);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / (K / 8);
        const int col = (int)(i - row * (K / 8)) * 8;
        out[lds_image_index(row, col, K) >> 3] = in[i];
    }
}

template <class T, int BN>
__global__ __launch_bounds__(256) void layernorm_tiled_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, u16* __restrict__ out16,
                                                              int64_t rows, int C, int packed) {
    constexpr int CPT = BN / 64;                       // 16-byte chunks per lane (BN / 4 per tile over 16 lanes)
    const int lane = threadIdx.x & 63, k = lane >> 4, l16 = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int ntile = C / BN;
    const bool live = k < ntile;
    const float* xr = x + row * C + k * BN;
    f32x4 v[CPT];
#pragma unroll
    for (int kk = 0; kk < CPT; ++kk) v[kk] = live ? *(const f32x4*)(xr + (l16 + 16 * kk) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    float pm, pq;
    ln_partial16<CPT>(v, 1.0f / BN, pm, pq);
    float mk[8], qk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        mk[i] = i < 4 ? __shfl(pm, i * 16, 64) : 0.f;
        qk[i] = i < 4 ? __shfl(pq, i * 16, 64) : 0.f;
    }
    float rstd;
    const float mean = ln_combine(mk, qk, ntile, (float)BN, (float)C, eps, rstd);
    // the mean's fp32 rounding taken out through the residuals' own mean, as in layernorm_kernel above (the variance feels it in
    // second order only, so rstd stays ln_combine's: the statistics proper are still those of the folded LayerNorm's producers)
    float rs = 0.f;
    if (live) {
#pragma unroll
        for (int kk = 0; kk < CPT; ++kk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[kk][j] -= mean;
            rs += (v[kk][0] + v[kk][1]) + (v[kk][2] + v[kk][3]);
        }
    }
    const float corr = wave_sum(rs) / (float)C;
    if constexpr (!std::is_same<T, FP8>::value) {
        if (packed) {
            // The output is the A operand of a gemm16_v5 launch: LDS-image order (gemm16_v5.h "Operand layout").  A row's 64 bytes
            // of one K-step are contiguous there and the workgroup's 4 consecutive rows make 256 B, so the rows go through LDS and
            // the workgroup stores 16 bytes per thread, 256-byte runs (a wave storing its own row would write 64-byte pieces 1 KiB
            // apart: measured +15 % on this HBM-bound kernel).  rows % 16 == 0: every workgroup is full.
            __shared__ __attribute__((aligned(16))) u16 stage[4][1280];
            const int w = threadIdx.x >> 6;
            if (live) {
#pragma unroll
                for (int kk = 0; kk < CPT; ++kk) {
                    const int c0 = k * BN + (l16 + 16 * kk) * 4;
                    const f32x4 g = *(const f32x4*)(gamma + c0);
                    const f32x4 b = *(const f32x4*)(beta + c0);
                    typename T::vec4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = T::from_f32(ln_apply(v[kk][j], corr, rstd, g[j], b[j]));
                    *(typename T::vec4*)(&stage[w][c0]) = o;
                }
            }
            __syncthreads();
            const int64_t row0 = (int64_t)blockIdx.x * 4;
            const int r0 = (int)(row0 & 15);                               // 0, 4, 8 or 12: the 4 rows share r >> 2, i.e. one swizzle key
            const int key = (0 - (r0 >> 2)) & 3;
            uint4* dst = (uint4*)(out16 + (row0 >> 4) * (int64_t)(C >> 5) * 512) + r0 * 4;      // + kt * 64 + (row in 4) * 4 + position chunk
            for (int i = threadIdx.x; i < (C >> 5) * 16; i += 256) {       // per K-step: 4 rows x 4 chunks = 256 contiguous bytes
                const int kt = i >> 4, rr = (i >> 2) & 3, pc = i & 3;
                dst[kt * 64 + rr * 4 + pc] = *(const uint4*)(&stage[rr][kt * 32 + ((pc ^ key) << 3)]);
            }
            return;
        }
    }
    if (!live) return;
#pragma unroll
    for (int kk = 0; kk < CPT; ++kk) {
        const int c0 = k * BN + (l16 + 16 * kk) * 4;
        const f32x4 g = *(const f32x4*)(gamma + c0);
        const f32x4 b = *(const f32x4*)(beta + c0);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = ln_apply(v[kk][j], corr, rstd, g[j], b[j]);
        store4_as<T>(out16, row * C + c0, y);
    }
}

// The fp8 blocks' LayerNorm on the stream's hi plane (gemm8.h PLANES): position-wise.  Input: the hi plane of rows (16-bit type TIN,
// column c at plane_pos(c)); output: e4m3 rows IN THE SAME ORDER (position p holds LN(x)[plane_col(p)]), consumed by a gemm8 launch whose
// weight has its K columns permuted alike (host_weights.h upload8: a dot product does not care).  So the kernel reads and writes whole
// contiguous runs: a lane owns the 16-byte chunks lane + 64 j of the row (1 KiB per load instruction, 512 B per store instruction;
// the column-tiled kernel above wrote 64-byte pieces 320 columns apart).  Statistics: mean, then the centred second moment, both over
// the wave.  One wave per row, NJ = ceil(C / 512) chunks per lane, grid (rows / 4) x 256 threads.
template <class TIN, int NJ, int RPW>
__global__ __launch_bounds__(256) void layernorm_plane_fp8_kernel(const u16* __restrict__ hi, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float eps, unsigned char* __restrict__ out, int64_t rows, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;       // RPW rows per wave, all loads issued before the first use (1 and 2 measured equal: 1)
    if (row0 >= rows) return;
    const int nch = C >> 3;
    uint4 raw[RPW][NJ];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < nch && row0 + r < rows) raw[r][j] = *(const uint4*)(hi + (row0 + r) * C + (lane + 64 * j) * 8);
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const int64_t row = row0 + r;
        if (row >= rows) break;
        float v[NJ][8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < nch) {
                union { uint4 raw; typename TIN::vec4 h[2]; } u;
                u.raw = raw[r][j];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[j][e] = TIN::to_f32(u.h[e >> 2][e & 3]);
                    s += v[j][e];
                }
            }
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < nch) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[j][e] -= mean;
                    q = fmaf(v[j][e], v[j][e], q);
                }
            }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int p = lane + 64 * j;
            if (p < nch) {
                const int c0 = plane_col(p * 8);              // 8 consecutive positions are 8 consecutive columns
                uint2 o;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const f32x4 g = *(const f32x4*)(gamma + c0 + 4 * hh);
                    const f32x4 b = *(const f32x4*)(beta + c0 + 4 * hh);
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = fmaf(v[j][4 * hh + e] * rstd, g[e], b[e]);
                    (hh ? o.y : o.x) = pack4_e4m3(y);
                }
                *(uint2*)(out + row * C + p * 8) = o;
            }
        }
    }
}

// the stream's planes of rows -> fp16 rows in column order (the neck's operand): out[row][c] = fp16(float(hi) + float(lo))
template <class T>
__global__ __launch_bounds__(256) void stream_rows_to_fp16_kernel(const u16* __restrict__ hi, const u16* __restrict__ lo, u16* __restrict__ out, int64_t n4, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i * 4 / C;
        const int64_t at = row * C + plane_pos((int)(i * 4 - row * C));
        const typename T::vec4 h4 = *(const typename T::vec4*)(hi + at);
        const f16x4 l4 = *(const f16x4*)(lo + at);
        typename FP16::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = FP16::from_f32(T::to_f32(h4[j]) + (float)l4[j]);
        *(typename FP16::vec4*)(out + i * 4) = o;
    }
}

// Folded LayerNorm, weight side (once per wm_finalize_weights): from the weight W [N][K] (row-major), the LayerNorm's
// gamma / beta [K] and the Linear's bias [N]:
//   wf[n][k] = round16(gamma[k] * W[n][k])   written in LDS-image order
//   c1[n] = sum_k wf[n][k]        c2[n] = sum_k beta[k] * W[n][k] + bias[n]
// W is the fp32 weight when `w32` is given (the engine's path since round 4: the folded weight is then rounded ONCE, which is what
// lets bf16-operand blocks fold: rounded twice, bf16 cost 8.7-9.5e-4 against 7.2-8.2e-4 on the ViT-H logits), else the 16-bit
// weight `w16` as packed for the unfolded path (wm_op_fold_weight16: the op-level identity tests against LayerNorm-then-GEMM).
// One workgroup per output row; fixed summation order (thread-strided partials, then a fixed tree): the same bits every time.
template <class T>
__global__ __launch_bounds__(256) void fold_weight_kernel(const u16* __restrict__ w16, const float* __restrict__ w32, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ bias, u16* __restrict__ wf,
                                                          float* __restrict__ c1, float* __restrict__ c2, int N, int K) {
    const int n = blockIdx.x, tid = threadIdx.x;
    __shared__ float red[2][256];
    float s1 = 0.f, s2 = 0.f;
    for (int k4 = tid; k4 < K / 4; k4 += 256) {
        f32x4 wv;
        if (w32) {
            wv = *(const f32x4*)(w32 + (size_t)n * K + k4 * 4);
        } else {
            const typename T::vec4 w = *(const typename T::vec4*)(w16 + (size_t)n * K + k4 * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) wv[j] = T::to_f32(w[j]);
        }
        const f32x4 g = *(const f32x4*)(gamma + k4 * 4), b = *(const f32x4*)(beta + k4 * 4);
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = T::from_f32(g[j] * wv[j]);
            s1 += T::to_f32(o[j]);
            s2 = fmaf(b[j], wv[j], s2);
        }
        *(typename T::vec4*)(wf + lds_image_index(n, k4 * 4, K)) = o;
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { c1[n] = red[0][0]; c2[n] = red[1][0] + (bias ? bias[n] : 0.f); }
}

// Folded LayerNorm (gemm16_v5.h "Folded LayerNorm"), standalone producer: per-row partial statistics over BN-column tiles,
// [rows][C / BN][2] = (mean, M2) -- the same arithmetic, lane assignment and order as the residual GEMM's FOLDP epilogue and
// as layernorm_tiled_kernel above -- and the 16-bit copy of the rows in LDS-image order.  Used where the residual stream was
// not produced by a FOLDP launch: a half-width GEMM (one or two tiles per call), or an operand-type boundary between blocks.
// Split stream (round 4, gemm16_v5.h "Split stream"): with `lo16` the kernel also writes lo = fp16(x - hi) in the same order, and with
// `x_rw` it rewrites the fp32 rows as float(hi) + float(lo) -- the value the SPLIT GEMM instance reconstructs -- so that the
// half-width path (fp32 stream) and the split path carry the same stream bit for bit.  overflow: set to 1 when an fp16 hi clamps.
template <class T, int BN>
__global__ __launch_bounds__(256) void ln_stats_x16_kernel(const float* __restrict__ x, float* __restrict__ stats, u16* __restrict__ x16,
                                                           int64_t rows, int C, u16* __restrict__ lo16 = nullptr, float* x_rw = nullptr,
                                                           int* overflow = nullptr) {
    constexpr int CPT = BN / 64;
    const int lane = threadIdx.x & 63, k = lane >> 4, l16 = lane & 15;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int ntile = C / BN;
    const bool live = k < ntile;
    const float* xr = x + row * C + k * BN;
    f32x4 v[CPT];
#pragma unroll
    for (int kk = 0; kk < CPT; ++kk) v[kk] = live ? *(const f32x4*)(xr + (l16 + 16 * kk) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    float pm, pq;
    ln_partial16<CPT>(v, 1.0f / BN, pm, pq);
    if (!live) return;
    if (l16 == 0) *(float2*)(stats + (row * ntile + k) * 2) = make_float2(pm, pq);
    float amax = 0.f;
#pragma unroll
    for (int kk = 0; kk < CPT; ++kk) {
        typename T::vec4 o;
        f16x4 lo;
        f32x4 back;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = T::from_f32(v[kk][j]);
            lo[j] = FP16::from_f32(v[kk][j] - T::to_f32(o[j]));
            back[j] = T::to_f32(o[j]) + (float)lo[j];
            amax = fmaxf(amax, fabsf(v[kk][j]));
        }
        const int64_t e = lds_image_index(row, k * BN + (l16 + 16 * kk) * 4, C);
        *(typename T::vec4*)(x16 + e) = o;
        if (lo16) *(f16x4*)(lo16 + e) = lo;
        if (x_rw) *(f32x4*)(x_rw + row * C + k * BN + (l16 + 16 * kk) * 4) = back;
    }
    if constexpr (std::is_same<T, FP16>::value) {
        if (amax >= 65504.f && overflow) *(volatile int*)overflow = 1;
    }
}

// Split stream -> fp32 rows: out[row][col] = float(hi) + float(lo), planes in LDS-image order (taps, the neck's input in bf16 mode,
// operand-type boundaries between blocks).  One thread per 16-byte chunk of a plane (8 elements).
template <class T>
__global__ __launch_bounds__(256) void stream_merge_kernel(const u16* __restrict__ hi, const u16* __restrict__ lo, float* __restrict__ out,
                                                           int64_t rows, int C) {
    const int64_t n16 = rows * (C / 8);
    const int kts = C >> 5;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        // chunk i of the image: [row block][K-step][position], position = (row % 16) * 4 + swizzled chunk
        const int pos = (int)(i & 63);
        const int64_t piece = i >> 6;
        const int kt = (int)(piece % kts);
        const int64_t rb = piece / kts;
        const int r = pos >> 2, chunk = (pos & 3) ^ ((0 - (r >> 2)) & 3);
        const typename T::vec8 h = *(const typename T::vec8*)(hi + i * 8);
        const f16x8 l = *(const f16x8*)(lo + i * 8);
        float* dst = out + (rb * 16 + r) * C + kt * 32 + chunk * 8;
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = T::to_f32(h[j]) + (float)l[j];
            b[j] = T::to_f32(h[4 + j]) + (float)l[4 + j];
        }
        *(f32x4*)dst = a;
        *(f32x4*)(dst + 4) = b;
    }
}

// Row forms of the split stream (the fp8 blocks: gemm8.h PLANES; column c of a row sits at plane_pos(c)): fp32 rows -> (hi, lo);
// (hi, lo) -> fp32 rows.  n4 = elements / 4, C % 256 == 0.
template <class T>
__global__ __launch_bounds__(256) void stream_split_rows_kernel(const float* __restrict__ x, u16* __restrict__ hi, u16* __restrict__ lo, int64_t n4, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i * 4 / C;
        const int64_t at = row * C + plane_pos((int)(i * 4 - row * C));
        const f32x4 v = *(const f32x4*)(x + i * 4);
        typename T::vec4 o;
        f16x4 l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = T::from_f32(v[j]);
            l[j] = FP16::from_f32(v[j] - T::to_f32(o[j]));
        }
        *(typename T::vec4*)(hi + at) = o;
        *(f16x4*)(lo + at) = l;
    }
}
template <class T>
__global__ __launch_bounds__(256) void stream_merge_rows_kernel(const u16* __restrict__ hi, const u16* __restrict__ lo, float* __restrict__ out, int64_t n4, int C) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i * 4 / C;
        const int64_t at = row * C + plane_pos((int)(i * 4 - row * C));
        const typename T::vec4 h4 = *(const typename T::vec4*)(hi + at);
        const f16x4 l4 = *(const f16x4*)(lo + at);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = T::to_f32(h4[j]) + (float)l4[j];
        *(f32x4*)(out + i * 4) = v;
    }
}

// LDS-image order -> row-major (the neck's first GEMM where it is a half-width launch: 1-4 tiles per call)
__global__ __launch_bounds__(256) void unpack16_lds_image_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int64_t rows, int K) {
    const int64_t n16 = rows * (K / 8);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / (K / 8);
        const int col = (int)(i - row * (K / 8)) * 8;
        out[i] = in[lds_image_index(row, col, K) >> 3];
    }
}

// ---------------------------------------------------------------------------
// Batched 2-byte transpose: in [batch][R][C] -> out [batch][C][R], 64x64 LDS tiles.
// Used for the HFC adaptor's scramble reshape (image_encoder.py:512): per tile the
// [4096 tok, 1024 ch] buffer re-read as [1024, 4096] must become the K-contiguous
// A operand [4096, 1024] of proj_back.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose16_kernel(const u16* __restrict__ in, u16* __restrict__ out, int R, int C) {
    __shared__ u16 tile[64][66];
    const int64_t boff = (int64_t)blockIdx.z * R * C;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = ty + i * 4;
        tile[r][tx] = in[boff + (int64_t)(r0 + r) * C + c0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int cc = ty + i * 4;
        out[boff + (int64_t)(c0 + cc) * R + r0 + tx] = tile[tx][cc];
    }
}

// fp32 [batch][R][C] -> [batch][C][R] (NCHW <-> NHWC of the 256-channel embedding)
__global__ __launch_bounds__(256) void transpose32_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float tile[64][65];
    const int64_t boff = (int64_t)blockIdx.z * R * C;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = ty + i * 4;
        tile[r][tx] = in[boff + (int64_t)(r0 + r) * C + c0 + tx];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int cc = ty + i * 4;
        out[boff + (int64_t)(c0 + cc) * R + r0 + tx] = tile[tx][cc];
    }
}

template <class T>
__global__ __launch_bounds__(256) void cvt_f32_to_16_kernel(const float* __restrict__ in, u16* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = *(const f32x4*)(in + i * 4);
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = T::from_f32(v[j]);
        *(typename T::vec4*)(out + i * 4) = o;
    }
}

// Opt-in saturation census (wm_debug_saturation_*): elements of a 16-bit buffer whose magnitude bits are >= `thr` (fp16:
// 0x7bff = 65504, the value T::from_f32 clamps to, and inf / NaN above it; bf16: 0x7f7f and above), or of an e4m3 byte
// buffer with magnitude >= 0x7e (448).  One atomic per workgroup.  16 bytes per thread and iteration.
template <int BYTES_PER_ELEM>
__global__ __launch_bounds__(256) void saturation_count_kernel(const uint4* __restrict__ in, int64_t n16, unsigned thr, unsigned long long* __restrict__ counter) {
    unsigned c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const uint4 v = in[i];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (BYTES_PER_ELEM == 2) {
                c += ((w[j] & 0x7fffu) >= thr) + (((w[j] >> 16) & 0x7fffu) >= thr);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) c += (((w[j] >> (8 * b)) & 0x7fu) >= thr);
            }
        }
    }
    c = (unsigned)wave_sum((float)c);                  // <= 64 * 16 * iterations: exact in fp32 for any realistic grid
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counter, (unsigned long long)c);
}

template <class T>
__global__ __launch_bounds__(256) void cvt_16_to_f32_kernel(const u16* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const typename T::elem e = __builtin_bit_cast(typename T::elem, in[i]);
        out[i] = T::to_f32(e);
    }
}

}  // namespace wm
