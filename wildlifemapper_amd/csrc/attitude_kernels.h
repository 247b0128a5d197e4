// Survey attitude (include/wm_hip.h, "Survey attitude"): a frame resampled once to the picture a LEVEL pinhole camera at the
// same place would have taken, by the camera's roll and pitch and its Brown-Conrady calibration, in one gather.  No
// reference behaviour exists; the rule is the header's, and the checker is its sequential restatement attitude_oracle in
// tests/attitude_cases.py.  All arithmetic is IEEE double with one rounding per operation (no contraction), in the header's
// order and parentheses, so the kernel equals the oracle bit for bit; with rot the identity X == x, Y == y and Z == 1
// exactly, and the rule is "Survey lens"'s, so lens_undistort_kernel and lens_oracle check this kernel independently.  The
// inside test, the sampling and the store of a wave's row are the ground kernels' (coverage_kernels.h: cov_inside;
// mosaic_kernels.h: mos_sample, mos_store_row), included, not copied; the camera is lens_kernels.h's lens_camera.
//
// attitude_rectify_kernel, a gather in the geometry of lens_undistort_kernel: a workgroup of COV_THREADS owns COV_BLOCK_X x
// MOS_FILL_BLOCK_Y output pixels, lane = column, a thread owns MOS_FILL_ROWS consecutive rows of one column, and a wave's 64
// pixels of a row leave through mos_store_row.  EVERY pixel of the picture is written, with the sample or with the fill.
//   Shared terms.  x, r0 * x, r3 * x and r6 * x depend on the column alone and are computed once per thread; the header's
//   parentheses, (r0 * x + r1 * y) + r2, are chosen so that this changes no bit.  2.0 * p1 and 2.0 * p2 are uniform.  After
//   the division xn and yn depend on the row as well, so nothing of the lens terms is shared across a thread's rows: per
//   pixel that is three divisions (y, xn, yn) and some forty-five double operations, against the lens kernel's one and thirty.
// A pixel with Z <= 0 (or a NaN) looks away from the camera's front half space: it is filled and counted, whatever u and v
// come to.  The filled count goes as in the lens kernel: per thread, shuffles over the wave, the first dword of each wave's
// row buffer over the workgroup, one 64-bit atomic per workgroup that filled any.  No atomics touch the picture, no scratch,
// no LDS but the row buffers.  What bounds every read: Z > 0, 0 <= u < width and 0 <= v < height (cov_inside) before
// mos_sample, whose bilinear taps are clamped to the frame; what bounds every write: i < ow and j < oh.
#pragma once

#include "lens_kernels.h"

namespace wm {

struct attitude_rot {                                      // wm_rectify_u8's rot[9], row-major: d_cam = rot * d_nadir
    double r0, r1, r2, r3, r4, r5, r6, r7, r8;
};

template <int MODE>
__global__ __launch_bounds__(COV_THREADS) void attitude_rectify_kernel(frame_desc in, lens_camera cam, attitude_rot rot, double f_out, int oh,
                                                                       int ow, unsigned int fill, unsigned char* __restrict__ out,
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
    const double r0x = rot.r0 * x, r3x = rot.r3 * x, r6x = rot.r6 * x;
    const double p1_2 = 2.0 * cam.p1, p2_2 = 2.0 * cam.p2;
    const double cu = cam.cx + 0.5, cv = cam.cy + 0.5;
    const double half_oh = 0.5 * (double)oh;
    const bool wr = i < ow;
    int filled = 0;
#pragma unroll
    for (int r = 0; r < MOS_FILL_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= oh) break;                                  // wave-uniform
        const double y = (((double)j + 0.5) - half_oh) / f_out;
        const double X = (r0x + rot.r1 * y) + rot.r2;
        const double Y = (r3x + rot.r4 * y) + rot.r5;
        const double Z = (r6x + rot.r7 * y) + rot.r8;
        const double xn = X / Z, yn = Y / Z;
        const double xx = xn * xn, yy = yn * yn;
        const double rr = xx + yy;                           // "Survey lens"'s r2
        const double rad = 1.0 + rr * (cam.k1 + rr * (cam.k2 + rr * cam.k3));
        const double xd = xn * rad + ((p1_2 * xn) * yn + cam.p2 * (rr + 2.0 * xx));
        const double yd = yn * rad + (cam.p1 * (rr + 2.0 * yy) + (p2_2 * xn) * yn);
        const double u = cam.fx * xd + cu;
        const double v = cam.fy * yd + cv;
        unsigned char px[3] = {(unsigned char)fill, (unsigned char)(fill >> 8), (unsigned char)(fill >> 16)};
        if (wr) {
            if (Z > 0.0 && cov_inside(u, v, fw, fh)) mos_sample<MODE>(in, h, w, u, v, px);
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
