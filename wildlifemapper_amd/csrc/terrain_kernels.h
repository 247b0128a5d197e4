// Survey terrain (include/wm_hip.h, "Survey terrain"): a frame resampled once onto a ground grid, each output pixel's height
// taken from a digital elevation model (DEM), so that the picture's affine georeference is exact whatever the relief: pose,
// terrain height and the Brown-Conrady calibration in one gather.  No reference behaviour exists; the rule is the header's, and
// the checker is its sequential restatement terrain_oracle in tests/terrain_cases.py.  All arithmetic is IEEE double with one
// rounding per operation (no contraction), in the header's order and parentheses, so the kernel equals the oracle bit for bit.
// The inside test, the sampling and the store of a wave's row are the ground kernels' (coverage_kernels.h: cov_inside;
// mosaic_kernels.h: mos_sample, mos_store_row), included, not copied; the camera is lens_kernels.h's lens_camera and the frame
// survey_kernels.h's frame_desc.
//
// terrain_ortho_kernel, a gather in the geometry of attitude_rectify_kernel: a workgroup of COV_THREADS owns COV_BLOCK_X x
// MOS_FILL_BLOCK_Y output pixels, lane = column, a thread owns MOS_FILL_ROWS consecutive rows of one column, and a wave's 64
// pixels of a row leave through mos_store_row.  EVERY pixel of the picture is written, with the sample or with the fill.
//   Shared terms.  The output grid is a general affine, so of a pixel's ground position only g0 * px and g3 * px depend on the
//   column alone; the header's parentheses, (g0 * px + g1 * py) + g2, are chosen so that computing them once per thread changes
//   no bit.  2.0 * p1 and 2.0 * p2 are uniform.  Everything from the DEM cell on depends on row and column.
//   The DEM.  Four plain float loads per pixel that has a height, from a grid that is tiny next to the picture (a post spans
//   tens to hundreds of output pixels, so a wave's loads fall on a few cache lines); it is not staged in LDS.
// A pixel without a height (its position is off the posts' centres, or a NaN), or with Z <= 0 (or a NaN, which a non-finite
// post brings about), or whose (u, v) is outside the frame, is filled.  Two counts go as in the lens kernel -- per thread,
// shuffles over the wave, the first two dwords of each wave's row buffer over the workgroup, at most one 64-bit atomic each per
// workgroup: stats[0] the filled pixels, stats[1] those of them that had no height or a non-finite one.  No atomics touch the
// picture, no scratch, no LDS but the row buffers.  What bounds every read: the has-a-height test, 0 <= a <= dem_w - 1 and
// 0 <= b <= dem_h - 1, with ia <= dem_w - 2 and ib <= dem_h - 2 before the four DEM loads (dem_w, dem_h >= 2 is the host's
// check); Z > 0, 0 <= u < width and 0 <= v < height (cov_inside) before mos_sample, whose bilinear taps are clamped to the
// frame.  What bounds every write: i < ow and j < oh.
#pragma once

#include "lens_kernels.h"

namespace wm {

struct terrain_pose {                                      // wm_ortho_u8's pose[12]: the camera's position, then M row-major
    double ce, cn, cu, m0, m1, m2, m3, m4, m5, m6, m7, m8;
};

struct terrain_dem {                                       // [h][w] float32 posts at cell centres, north-up, and dem_geo[3]
    const float* z;
    int h, w;
    double e0, n0, dcell;
};

struct terrain_geo {                                       // wm_ortho_u8's out_geo[6]: output pixel -> ground
    double g0, g1, g2, g3, g4, g5;
};

template <int MODE>
__global__ __launch_bounds__(COV_THREADS) void terrain_ortho_kernel(frame_desc in, lens_camera cam, terrain_pose pose, terrain_dem dem,
                                                                    terrain_geo geo, int oh, int ow, unsigned int fill,
                                                                    unsigned char* __restrict__ out, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ unsigned int s_row[COV_THREADS / 64][48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_first = blockIdx.x * COV_BLOCK_X;
    const int i = i_first + lane, j0 = blockIdx.y * MOS_FILL_BLOCK_Y + wave * MOS_FILL_ROWS;
    const int h = in.height, w = in.width;
    const double fw = (double)w, fh = (double)h;
    const double a_max = (double)(dem.w - 1), b_max = (double)(dem.h - 1);
    // the column's terms
    const double px_ = (double)i + 0.5;
    const double g0x = geo.g0 * px_, g3x = geo.g3 * px_;
    const double p1_2 = 2.0 * cam.p1, p2_2 = 2.0 * cam.p2;
    const double cu = cam.cx + 0.5, cv = cam.cy + 0.5;
    const bool wr = i < ow;
    int filled = 0, no_height = 0;
#pragma unroll
    for (int r = 0; r < MOS_FILL_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= oh) break;                                  // wave-uniform
        const double py_ = (double)j + 0.5;
        const double E = (g0x + geo.g1 * py_) + geo.g2;
        const double N = (g3x + geo.g4 * py_) + geo.g5;
        const double a = (E - dem.e0) / dem.dcell - 0.5;
        const double b = (dem.n0 - N) / dem.dcell - 0.5;
        unsigned char px[3] = {(unsigned char)fill, (unsigned char)(fill >> 8), (unsigned char)(fill >> 16)};
        if (wr) {
            bool sees = false, height = false;
            if (0.0 <= a && a <= a_max && 0.0 <= b && b <= b_max) {        // the cell has a height; a NaN has none
                const int ia = min((int)floor(a), dem.w - 2), ib = min((int)floor(b), dem.h - 2);
                const double ta = a - (double)ia, tb = b - (double)ib;
                const float* p = dem.z + (size_t)ib * dem.w + ia;
                const double z00 = (double)p[0], z01 = (double)p[1], z10 = (double)p[dem.w], z11 = (double)p[dem.w + 1];
                const double z = (z00 * (1.0 - ta) + z01 * ta) * (1.0 - tb) + (z10 * (1.0 - ta) + z11 * ta) * tb;
                height = __builtin_isfinite(z);
                const double dE = E - pose.ce, dN = N - pose.cn, dU = z - pose.cu;
                const double X = (pose.m0 * dE + pose.m1 * dN) + pose.m2 * dU;
                const double Y = (pose.m3 * dE + pose.m4 * dN) + pose.m5 * dU;
                const double Z = (pose.m6 * dE + pose.m7 * dN) + pose.m8 * dU;
                if (Z > 0.0) {
                    const double xn = X / Z, yn = Y / Z;
                    const double xx = xn * xn, yy = yn * yn;
                    const double rr = xx + yy;                   // "Survey lens"'s r2
                    const double rad = 1.0 + rr * (cam.k1 + rr * (cam.k2 + rr * cam.k3));
                    const double xd = xn * rad + ((p1_2 * xn) * yn + cam.p2 * (rr + 2.0 * xx));
                    const double yd = yn * rad + (cam.p1 * (rr + 2.0 * yy) + (p2_2 * xn) * yn);
                    const double u = cam.fx * xd + cu;
                    const double v = cam.fy * yd + cv;
                    if (cov_inside(u, v, fw, fh)) {
                        mos_sample<MODE>(in, h, w, u, v, px);
                        sees = true;
                    }
                }
            }
            if (!sees) {
                ++filled;
                if (!height) ++no_height;
            }
        }
        unsigned char* row = out + ((size_t)j * ow + i_first) * 3;
        mos_store_row(s_row[wave], row, lane, __ballot(wr) == ~0ull && ((uintptr_t)row & 3) == 0, wr, px);
    }
    if (!stats) return;                                      // uniform over the grid
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        filled += __shfl_xor(filled, d);
        no_height += __shfl_xor(no_height, d);
    }
    if (lane == 0) {                                         // the wave's own row buffer, read back by the wave already
        s_row[wave][0] = (unsigned int)filled;
        s_row[wave][1] = (unsigned int)no_height;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned int n = 0;
#pragma unroll
        for (int k = 0; k < COV_THREADS / 64; ++k) n += s_row[k][tid];
        if (n) atomicAdd(stats + tid, (unsigned long long)n);
    }
}

}  // namespace wm
