// Survey lens (include/wm_hip.h, "Survey lens"): a frame resampled once to the pinhole picture of the same camera, by its
// Brown-Conrady calibration.  No reference behaviour exists; the rule is the header's, and the checker is its sequential
// restatement lens_oracle in tests/lens_cases.py.  All arithmetic is IEEE double with one rounding per operation (no
// contraction), in the header's order and parentheses, so the kernel equals the oracle bit for bit.  The inside test, the
// sampling and the store of a wave's row are the ground kernels' (coverage_kernels.h: cov_inside; mosaic_kernels.h:
// mos_sample, mos_store_row), included, not copied.
//
// lens_undistort_kernel, a gather in the geometry of mosaic_fill_kernel: a workgroup of COV_THREADS owns COV_BLOCK_X x
// MOS_FILL_BLOCK_Y output pixels, lane = column, a thread owns MOS_FILL_ROWS consecutive rows of one column.  A wave's 64
// pixels of a row are 192 contiguous bytes of the picture: 48 dword stores through the wave's LDS row when all 64 lie in the
// picture and the row starts on a dword, byte stores otherwise.  EVERY pixel of the picture is written, with the sample or
// with the fill colour, so all 64 lanes of a full block write and only the last block of a row, or a row that starts off a
// dword, takes the byte path.
//   Shared terms.  x, x * x, 2.0 * (x * x), (2.0 * p1) * x and (2.0 * p2) * x depend on the column alone and are computed once
//   per thread; the same operands give the same rounded result, so sharing them across the thread's rows changes no bit.
//   What the fp64 rate buys: some thirty double operations and two divisions' worth per pixel against 6 (nearest) or 15
//   (bilinear) bytes of traffic; the kernel has no loop over frames, no scratch and no LDS but the row buffers.
// The filled pixels are counted per thread, reduced over the wave by shuffles and over the workgroup through the first dword
// of each wave's row buffer (free by then), and sent with one 64-bit atomic per workgroup that filled any.  No atomics touch
// the picture.  What bounds every read: 0 <= u < width and 0 <= v < height (cov_inside) before mos_sample, whose bilinear taps
// are clamped to the frame; what bounds every write: i < ow and j < oh.
#pragma once

#include "mosaic_kernels.h"

namespace wm {

struct lens_camera {                                       // wm_undistort_u8's camera[9], in its order
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

template <int MODE>
__global__ __launch_bounds__(COV_THREADS) void lens_undistort_kernel(frame_desc in, lens_camera cam, double f_out, int oh, int ow,
                                                                     unsigned int fill, unsigned char* __restrict__ out,
                                                                     unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ unsigned int s_row[COV_THREADS / 64][48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_first = blockIdx.x * COV_BLOCK_X;
    const int i = i_first + lane, j0 = blockIdx.y * MOS_FILL_BLOCK_Y + wave * MOS_FILL_ROWS;
    const int h = in.height, w = in.width;
    const double fw = (double)w, fh = (double)h;
    // the column's terms
    const double x = (((double)i + 0.5) - 0.5 * (double)ow) / f_out;
    const double xx = x * x;
    const double xx2 = 2.0 * xx;
    const double p1x2 = (2.0 * cam.p1) * x, p2x2 = (2.0 * cam.p2) * x;
    const double cu = cam.cx + 0.5, cv = cam.cy + 0.5;
    const double half_oh = 0.5 * (double)oh;
    const bool wr = i < ow;
    int filled = 0;
#pragma unroll
    for (int r = 0; r < MOS_FILL_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= oh) break;                                  // wave-uniform
        const double y = (((double)j + 0.5) - half_oh) / f_out;
        const double yy = y * y;
        const double r2 = xx + yy;
        const double rad = 1.0 + r2 * (cam.k1 + r2 * (cam.k2 + r2 * cam.k3));
        const double xd = x * rad + (p1x2 * y + cam.p2 * (r2 + xx2));
        const double yd = y * rad + (cam.p1 * (r2 + 2.0 * yy) + p2x2 * y);
        const double u = cam.fx * xd + cu;
        const double v = cam.fy * yd + cv;
        unsigned char px[3] = {(unsigned char)fill, (unsigned char)(fill >> 8), (unsigned char)(fill >> 16)};
        if (wr) {
            if (cov_inside(u, v, fw, fh)) mos_sample<MODE>(in, h, w, u, v, px);
            else ++filled;
        }
        unsigned char* row = out + ((size_t)j * ow + i_first) * 3;
        mos_store_row(s_row[wave], row, lane, __ballot(wr) == ~0ull && ((uintptr_t)row & 3) == 0, wr, px);
    }
    if (!stats) return;                                      // uniform over the grid
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) filled += __shfl_xor(filled, d);
    if (lane == 0) s_row[wave][0] = (unsigned int)filled;    // the wave's own row buffer, read back by the wave already
    __syncthreads();
    if (tid == 0) {
        unsigned int n = 0;
#pragma unroll
        for (int k = 0; k < COV_THREADS / 64; ++k) n += s_row[k][0];
        if (n) atomicAdd(stats, (unsigned long long)n);
    }
}

}  // namespace wm
