// Survey resampling (wm_resample_u8): uint8 HWC frame of any size -> uint8 HWC frame of any size, with the 8-bit
// arithmetic of Pillow's ImagingResample (bilinear filter) that the N1 kernels of misc_kernels.h use: 22-bit fixed-point
// coefficient tables computed on the host (host_frontend.h: resize_coeffs), a horizontal pass into an 8-bit intermediate, then
// the vertical pass, every output clip8((acc + 2^21) >> 22).  Integer work: bit-exact with PIL.Image.resize.
//   * resample_h_cols_kernel: horizontal pass for any output width.  Grid (row block, column block): a workgroup owns up
//     to 256 * OPT output columns and stages in LDS, row by row, only the input span those columns read.
//   * resample_v_u8_kernel: vertical pass writing uint8 HWC.  One output row per workgroup (its taps are wave-uniform);
//     a thread filters 16 contiguous bytes of the row with dword loads.  Rows of any byte length and alignment.
#pragma once

#include "misc_kernels.h"
#include "wm_common.h"

namespace wm {

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

// in [h, w, 3] u8 -> out [h, ow, 3] u8.  bounds [ow][2] = (first input column, taps), kk [ow][ksize]; bounds are
// non-decreasing in both entries (Pillow's triangle filter), so the columns [c0, c1) of a block read the input columns
// [bounds[c0].first, bounds[c1-1].first + bounds[c1-1].taps).  LDS: that span of one row + its alignment shift + KMAX * 3
// bytes of slack for the zero-coefficient taps (a zero coefficient times any staged byte adds nothing).
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
            int a0 = 1 << (RESIZE_PREC_BITS - 1), a1 = a0, a2 = a0;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int c = coef[o][k];
                a0 += src[3 * k] * c; a1 += src[3 * k + 1] * c; a2 += src[3 * k + 2] * c;
            }
            unsigned char* dst = out + ((int64_t)row * ow + c0 + tid + 256 * o) * 3;
            dst[0] = (unsigned char)min(max(a0 >> RESIZE_PREC_BITS, 0), 255);
            dst[1] = (unsigned char)min(max(a1 >> RESIZE_PREC_BITS, 0), 255);
            dst[2] = (unsigned char)min(max(a2 >> RESIZE_PREC_BITS, 0), 255);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned char resample_clip8(int acc) { return (unsigned char)min(max(acc >> RESIZE_PREC_BITS, 0), 255); }

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

// in [h][row_bytes] -> out [oh][row_bytes], row_bytes = ow * 3: the vertical filter treats every byte column (pixel and
// channel) alike.  Output dwords are aligned; the input of a tap row is shifted against them by a wave-uniform 0..3 bytes
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
        int acc = 1 << (RESIZE_PREC_BITS - 1);
        for (int y = 0; y < n; ++y) acc += irow[(int64_t)y * row_bytes + j] * k[y];
        orow[j] = resample_clip8(acc);
    }
    for (int64_t j = head + (int64_t)threadIdx.x * 16; j < body_end; j += 256 * 16) {
        const int nd = (int)min((int64_t)4, (body_end - j) >> 2);           // output dwords of this thread, 1..4
        int acc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = 1 << (RESIZE_PREC_BITS - 1);
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

}  // namespace wm
