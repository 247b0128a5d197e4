// The PIL-bilinear resample family: every kernel that filters uint8 HWC pixels with the 8-bit arithmetic of Pillow's
// ImagingResample (separable antialiased triangle filter, 22-bit fixed-point coefficients, a horizontal pass into an 8-bit
// intermediate, then the vertical pass, every output clip8((acc + 2^21) >> 22)).  Integer work: bit-exact with
// PIL.Image.resize.  Its callers are the input pipeline (wm_preprocess_u8, wm_preprocess_u8_resized) and
// the survey resampler (wm_resample_u8), both launched from host_frontend.h.  Index:
//   * the coefficient rule, host and device: resize_axis_of, resize_coeff_row (Pillow's precompute_coeffs +
//     normalize_coeffs_8bpc).  The host tables (host_frontend.h: resize_coeffs) and the tables crop_chips_kernel builds in
//     LDS are both made by it.
//   * the arithmetic, spelled once: RESIZE_PREC_BITS, RESAMPLE_ACC0 (the rounding constant an accumulator starts from),
//     resample_clip8, resample_pack4.
//   * horizontal pass: resample_h_cols_kernel<KMAX,OPT>, column-blocked and row-staged, for <= 20 taps.  Grid (row block,
//     column block): a workgroup owns up to 256 * OPT output columns and stages in LDS, row by row, only the input span
//     those columns read.  Its rows are the rows of one frame or of a batch of frames ([B, h, w, 3] is B * h rows: the
//     pass is per row and does not see the image boundary).  resize_h_u8_kernel is the generic fallback for more taps,
//     one thread per output pixel.
//   * vertical pass, three forms: resample_v_u8_kernel writes uint8 HWC (rows of any byte length and alignment);
//     resize_v_normalize4_kernel writes the fp32 normalised tile, four pixels per thread (output width % 4 == 0, input
//     4-byte aligned); resize_v_normalize_kernel is the generic form of the latter.  preprocess_u8_kernel is the tile
//     without a filter (normalise + pad), which is also what an unchanged height needs.
//   * the review chips (chip_kernels.h: crop_chips_kernel) include this file: both passes in LDS, a table per chip.
#pragma once

#include "wm_common.h"

namespace wm {

constexpr int RESIZE_PREC_BITS = 22;
constexpr int RESAMPLE_ACC0 = 1 << (RESIZE_PREC_BITS - 1);      // every accumulator starts here: >> rounds to nearest

__device__ __forceinline__ unsigned char resample_clip8(int acc) { return (unsigned char)min(max(acc >> RESIZE_PREC_BITS, 0), 255); }

// acc_c += src[3 t + c] * coef[t] over t < n, c = 0..2: the tap loop of the horizontal kernels.  At the column-blocked kernel's
// site n is a constant and coef a register array: the loop unrolls fully there.
__device__ __forceinline__ void resample_taps3(const unsigned char* src, const int* coef, int n, int& a0, int& a1, int& a2) {
    for (int t = 0; t < n; ++t) {
        const int c = coef[t];
        a0 += src[3 * t] * c; a1 += src[3 * t + 1] * c; a2 += src[3 * t + 2] * c;
    }
}

// clip8 of four accumulators packed little-endian.  The clipped bytes pass through an empty asm so that they are packed by
// plain shifts: left to itself the compiler fuses two shift + clamp + pack steps into v_ashr_pk_u8_i32 and ORs the other two
// bytes into its destination, whose upper half that instruction leaves dirty (bytes 2 and 3 of the dword came out wrong).
__device__ __forceinline__ unsigned resample_pack4(const int* acc) {
    unsigned b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        b[i] = resample_clip8(acc[i]);
        asm volatile("" : "+v"(b[i]));
    }
    return (b[0] & 255u) | ((b[1] & 255u) << 8) | ((b[2] & 255u) << 16) | ((b[3] & 255u) << 24);
}

// Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for one axis, bilinear filter (support 1): the one definition
// behind the host tables (host_frontend.h: resize_coeffs) and the tables crop_chips_kernel builds in LDS.  Double
// arithmetic in Pillow's operation order, every operation rounded on its own (no contraction).
struct resize_axis {
    double scale, support, ss;
    int ksize;                 // taps per output: the row length of kk
};

__host__ __device__ inline resize_axis resize_axis_of(int in_size, int out_size) {
#pragma clang fp contract(off)
    resize_axis a;
    a.scale = (double)in_size / out_size;
    const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 1.0 * filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    a.ss = 1.0 / filterscale;
    return a;
}

// Output xx of an axis of in_size inputs: first input *xmin_out, taps *n_out (<= ksize), coefficients kk_row[0 .. taps).
// Pillow keeps the weights in an array between its two loops; here the second loop computes each weight again, the same
// operations on the same values.
__host__ __device__ inline void resize_coeff_row(const resize_axis& a, int in_size, int xx, int* xmin_out, int* n_out, int* kk_row) {
#pragma clang fp contract(off)
    const double center = (xx + 0.5) * a.scale;
    int xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double v = (x + xmin - center + 0.5) * a.ss;
        if (v < 0.0) v = -v;
        ww += v < 1.0 ? 1.0 - v : 0.0;
    }
    for (int x = 0; x < xmax; ++x) {
        double v = (x + xmin - center + 0.5) * a.ss;
        if (v < 0.0) v = -v;
        double wt = v < 1.0 ? 1.0 - v : 0.0;
        if (ww != 0.0) wt /= ww;
        kk_row[x] = wt < 0 ? (int)(-0.5 + wt * (1 << RESIZE_PREC_BITS)) : (int)(0.5 + wt * (1 << RESIZE_PREC_BITS));
    }
    *xmin_out = xmin;
    *n_out = xmax;
}

// ---------------------------------------------------------------------------
// Input pipeline without a resize: uint8 HWC image (h, w <= 1024) -> fp32 CHW tile on the zero
// 1024 x 1024 canvas, top-left aligned: ToTensor (/255), Normalize(ImageNet mean/std) (dataloader_coco.py:286-292,
// augmentation.py:229-249) and the fixed-1024 zero padding of nested_tensor_from_tensor_list
// (utils/misc.py:46-67) in one pass.  in [B,h,w,3] u8, out [B,3,1024,1024] fp32.  One thread per 4 pixels.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                            int B, int h, int w) {
    const int64_t total = (int64_t)B * 1024 * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(i & 255) * 4;
        const int y = (int)((i >> 8) & 1023);
        const int64_t b = i >> 18;
        f32x4 v[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if (y < h) {
            const unsigned char* row = in + ((b * h + y) * (int64_t)w) * 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x4 + j;
                if (x < w) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][j] = normalize_u8(row[x * 3 + c], c);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)(out + ((b * 3 + c) * 1024 + y) * (int64_t)1024 + x4) = v[c];
    }
}

// ---- horizontal pass ----------------------------------------------------------------------------------------------------
// Generic: in [B,h,w,3] u8 -> tmp [B,h,ow,3] u8; bounds [ow][2] = (first input column, taps), kk [ow][ksize].  One thread per
// output pixel, byte loads from global memory: any number of taps.
__global__ __launch_bounds__(256) void resize_h_u8_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ tmp,
                                                          const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                          int B, int h, int w, int ow) {
    const int64_t total = (int64_t)B * h * ow;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xx = (int)(i % ow);
        const int64_t by = i / ow;                                   // b * h + y
        const int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
        const unsigned char* src = in + (by * w + x0) * 3;
        const int* k = kk + (int64_t)xx * ksize;
        int a0 = RESAMPLE_ACC0, a1 = a0, a2 = a0;
        resample_taps3(src, k, n, a0, a1, a2);
        unsigned char* dst = tmp + i * 3;
        dst[0] = resample_clip8(a0); dst[1] = resample_clip8(a1); dst[2] = resample_clip8(a2);
    }
}

// Column-blocked, at streaming rate (the generic kernel: 0.08 of the HBM rate on a 3648 x 5472 frame).
// in [h, w, 3] u8 -> out [h, ow, 3] u8, h the rows of one frame or of a whole batch.  bounds are non-decreasing in both
// entries (Pillow's triangle filter), so the columns [c0, c1) of a block read the input columns
// [bounds[c0].first, bounds[c1-1].first + bounds[c1-1].taps).  A workgroup walks its rows; per row that span is staged in
// LDS by coalesced dword loads, and each thread owns up to OPT output columns whose taps' coefficients it keeps in
// registers for all its rows (KMAX taps, zero beyond the column's count).  LDS: the span of one row + its alignment shift
// + KMAX * 3 bytes of slack for the zero-coefficient taps (a zero coefficient times any staged byte adds nothing).
// The staging reads only aligned dwords that hold at least one byte of the frame, whatever the frame's start and row
// length: the first and last dword of a span may reach up to 3 bytes past the frame's ends, inside the 4-byte granule
// the frame itself occupies.  wm_resample_u8 has always relied on exactly that, and wm_preprocess_u8_resized hands this
// kernel the same kinds of caller buffers (device allocations, and views into them at any byte offset).
template <int KMAX, int OPT>
__global__ __launch_bounds__(256) void resample_h_cols_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                              const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                              int h, int w, int ow, int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned srow[];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * 256 * OPT;
    const int c1 = min(c0 + 256 * OPT, ow);
    const int xs = bounds[2 * c0];
    const int span_bytes = (bounds[2 * (c1 - 1)] + bounds[2 * (c1 - 1) + 1] - xs) * 3;
    int rel[OPT], coef[OPT][KMAX];
    bool valid[OPT];
#pragma unroll
    for (int o = 0; o < OPT; ++o) {
        const int xx = c0 + tid + 256 * o;
        valid[o] = xx < c1;
        const int n = valid[o] ? bounds[2 * xx + 1] : 0;
        rel[o] = valid[o] ? bounds[2 * xx] - xs : 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) coef[o][k] = k < n ? kk[(int64_t)xx * ksize + k] : 0;
    }
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(r0 + rows_per_block, h);
    for (int row = r0; row < r1; ++row) {
        // aligned dwords covering [p, p + span_bytes): each holds at least one byte of the frame, so none leaves its allocation
        const unsigned char* p = in + ((int64_t)row * w + xs) * 3;
        const unsigned* a = (const unsigned*)((uintptr_t)p & ~(uintptr_t)3);
        const int shift = (int)((uintptr_t)p & 3), ndw = (shift + span_bytes + 3) >> 2;
        for (int i = tid; i < ndw; i += 256) srow[i] = a[i];
        __syncthreads();
        const unsigned char* sb = (const unsigned char*)srow + shift;
#pragma unroll
        for (int o = 0; o < OPT; ++o) {
            if (!valid[o]) continue;
            const unsigned char* src = sb + rel[o] * 3;
            int a0 = RESAMPLE_ACC0, a1 = a0, a2 = a0;
            resample_taps3(src, coef[o], KMAX, a0, a1, a2);
            unsigned char* dst = out + ((int64_t)row * ow + c0 + tid + 256 * o) * 3;
            dst[0] = resample_clip8(a0); dst[1] = resample_clip8(a1); dst[2] = resample_clip8(a2);
        }
        __syncthreads();
    }
}

// ---- vertical pass ------------------------------------------------------------------------------------------------------
// uint8 out.  in [h][row_bytes] -> out [oh][row_bytes], row_bytes = ow * 3: the vertical filter treats every byte column
// (pixel and channel) alike.  One output row per workgroup (its taps are wave-uniform); a thread filters 16 contiguous
// bytes of the row.  Output dwords are aligned; the input of a tap row is shifted against them by a wave-uniform 0..3 bytes
// and read as aligned dwords joined by alignbyte, each holding at least one byte of the row (no read leaves the buffer).
// The 0..3 bytes before the first aligned output dword and after the last one are done byte by byte.
__global__ __launch_bounds__(256) void resample_v_u8_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                            int64_t row_bytes) {
    const int yy = blockIdx.x;
    const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
    const int* k = kk + (int64_t)yy * ksize;
    const unsigned char* irow = in + (int64_t)y0 * row_bytes;
    unsigned char* orow = out + (int64_t)yy * row_bytes;
    const int64_t head = min((int64_t)((4 - ((uintptr_t)orow & 3)) & 3), row_bytes);
    const int64_t body_end = head + ((row_bytes - head) & ~(int64_t)3);
    const int64_t n_edge = head + (row_bytes - body_end);
    for (int64_t e = threadIdx.x; e < n_edge; e += 256) {
        const int64_t j = e < head ? e : body_end + (e - head);
        int acc = RESAMPLE_ACC0;
        for (int y = 0; y < n; ++y) acc += irow[(int64_t)y * row_bytes + j] * k[y];
        orow[j] = resample_clip8(acc);
    }
    for (int64_t j = head + (int64_t)threadIdx.x * 16; j < body_end; j += 256 * 16) {
        const int nd = (int)min((int64_t)4, (body_end - j) >> 2);           // output dwords of this thread, 1..4
        int acc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = RESAMPLE_ACC0;
        const unsigned char* p = irow + j;
#pragma unroll 2
        for (int y = 0; y < n; ++y) {
            const int c = k[y];
            const unsigned* a = (const unsigned*)((uintptr_t)p & ~(uintptr_t)3);
            const unsigned s = (unsigned)((uintptr_t)p & 3);
            unsigned d[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) d[i] = (i < nd || (i == nd && s)) ? a[i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned v = __builtin_amdgcn_alignbyte(d[i + 1], d[i], s);
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[4 * i + b] += (int)((v >> (8 * b)) & 255u) * c;
            }
            p += row_bytes;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nd) *(unsigned*)(orow + j + 4 * i) = resample_pack4(acc + 4 * i);
    }
}

// fp32 normalised out, generic.  tmp [B,h,ow,3] u8 -> out [B,3,1024,1024] fp32: vertical pass to oh rows fused with ToTensor
// (/255), Normalize (ImageNet) and the zero padding to 1024 x 1024 (utils/misc.py:46-67).  One thread per canvas pixel.
__global__ __launch_bounds__(256) void resize_v_normalize_kernel(const unsigned char* __restrict__ tmp, float* __restrict__ out,
                                                                 const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                                 int B, int h, int ow, int oh) {
    const int64_t total = (int64_t)B * 1024 * 1024;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int xx = (int)(i & 1023), yy = (int)((i >> 10) & 1023);
        const int64_t b = i >> 20;
        float v[3] = {0.f, 0.f, 0.f};
        if (yy < oh && xx < ow) {
            const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
            const unsigned char* src = tmp + ((b * h + y0) * (int64_t)ow + xx) * 3;
            const int* k = kk + (int64_t)yy * ksize;
            int a[3] = {RESAMPLE_ACC0, RESAMPLE_ACC0, RESAMPLE_ACC0};
            for (int y = 0; y < n; ++y) {
                const int c = k[y];
                const unsigned char* p = src + (int64_t)y * ow * 3;
                a[0] += p[0] * c; a[1] += p[1] * c; a[2] += p[2] * c;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = normalize_u8(resample_clip8(a[c]), c);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((b * 3 + c) * 1024 + yy) * (int64_t)1024 + xx] = v[c];
    }
}

// fp32 normalised out, four output pixels per thread: a workgroup is one output row (its taps' coefficients are
// wave-uniform), a thread reads 12 contiguous bytes (3 dwords) per tap row and writes one 16-byte chunk per channel.
// ow % 4 == 0 and tmp 4-byte aligned.  Same arithmetic as resize_v_normalize_kernel: bit-identical.
__global__ __launch_bounds__(256) void resize_v_normalize4_kernel(const unsigned char* __restrict__ tmp, float* __restrict__ out,
                                                                  const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                                  int h, int ow, int oh) {
    const int yy = blockIdx.x & 1023;
    const int64_t b = blockIdx.x >> 10;
    const int xx4 = threadIdx.x * 4;
    f32x4 v[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (yy < oh && xx4 < ow) {
        const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
        const unsigned* src = (const unsigned*)(tmp + ((b * h + y0) * (int64_t)ow + xx4) * 3);
        const int* k = kk + (int64_t)yy * ksize;
        int a[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) a[j] = RESAMPLE_ACC0;
        const int64_t stride_dw = (int64_t)ow * 3 / 4;
        for (int y = 0; y < n; ++y) {
            const int c = k[y];
            const unsigned d0 = src[0], d1 = src[1], d2 = src[2];
            src += stride_dw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] += (int)((d0 >> (8 * j)) & 255u) * c;
                a[4 + j] += (int)((d1 >> (8 * j)) & 255u) * c;
                a[8 + j] += (int)((d2 >> (8 * j)) & 255u) * c;
            }
        }
#pragma unroll
        for (int px = 0; px < 4; ++px)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][px] = normalize_u8(resample_clip8(a[px * 3 + c]), c);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(f32x4*)(out + ((b * 3 + c) * 1024 + yy) * (int64_t)1024 + xx4) = v[c];
}

}  // namespace wm
