// Survey coverage (include/wm_hip.h, "Survey coverage"): a ground grid laid over a survey; every cell gets the number of
// frames whose footprint holds its centre, and the census' individuals are counted into the same grid per class, each
// with the number of frames that could have seen it.  No reference behaviour exists; the rule is the header's, and the
// checker is its sequential restatement coverage_oracle in tests/ground_oracle.py.  Everything is integer counting behind
// an exact double predicate (one rounding per operation, no contraction), so the result equals the oracle bit for bit.
//
// coverage_raster_kernel, gather: one workgroup of COV_THREADS owns a block of COV_BLOCK_X x COV_BLOCK_Y cells; lane =
// column, so a wave's store of a row is 128 contiguous bytes; a thread owns COV_ROWS cells of one column, which share the
// products b0 * Xc and b3 * Xc (the same operands give the same rounded product, so sharing them changes no bit).
// The frames are walked in chunks of COV_CHUNK: every thread loads one frame and decides whether it can touch the block;
// the survivors are compacted into LDS by a wave ballot, and every cell evaluates the exact predicate on them only.
//   Cull.  The centres of a block lie in the ground rectangle [Xc(i_first), Xc(i_last)] x [Yc(j_first), Yc(j_last)]
//   (the centre formula is monotone in the index).  In exact arithmetic u and v are affine, so their values on the
//   rectangle lie between the extremes of its four corners.  The computed u differs from the exact one by little more
//   than 3 * 2^-53 * S, S = |b0| * max|X| + |b1| * max|Y| + |b2| (four roundings: two products, two sums, the sums
//   bounded by S), at a corner as at a cell; the box of the computed corner values widened by M = S * 2^-50 (8 * 2^-53:
//   twice that bound, and room for the roundings of S itself) plus the smallest normal number (products that fall
//   below it lose their relative accuracy) therefore holds every computed cell value.  A frame is dropped only when that box misses [0, W) x [0, H),
//   or when height < 1 or width < 1; a box that is not finite proves nothing and keeps the frame.  The cull changes no
//   count.
// No atomics touch the raster; the per-workgroup histogram goes to stats with 64-bit integer atomics.
//
// coverage_points_kernel: one thread per point, the frames staged through the same LDS chunks (no cull: the points of a
// workgroup are anywhere); seen_by stays in a register; then the cell arithmetic and an int32 atomicAdd into counts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wm_hip.h"
#include "survey_kernels.h"                      // frame_desc

namespace wm {

constexpr int COV_THREADS = 256;                 // 4 waves, one per SIMD
constexpr int COV_BLOCK_X = 64;                  // cells east per workgroup = lanes of a wave
constexpr int COV_ROWS = 8;                      // cells per thread, consecutive rows of one column
constexpr int COV_BLOCK_Y = (COV_THREADS / 64) * COV_ROWS;     // 32 rows per workgroup
constexpr int COV_CHUNK = 256;                   // frames staged in LDS at a time, one per thread
constexpr int COV_CLASSES = WM_COVERAGE_CLASSES;  // labels 0..6 are binned
constexpr int COV_STATS = WM_COVERAGE_STATS;      // stats[m], m < 15: cells seen by m frames; stats[15]: by 15 or more

static_assert(COV_CHUNK == COV_THREADS, "one staged frame per thread");
static_assert(COV_BLOCK_X == 64, "lane = column");

struct CovFrames {                               // a staged chunk: b0..b5 and (height, width) per frame
    double b[6][COV_CHUNK];
    int h[COV_CHUNK], w[COV_CHUNK];
};

__device__ __forceinline__ bool cov_finite(double d) {
    return ((uint64_t)__double_as_longlong(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// The centre of cell `index` of one axis of the grid.
__device__ __forceinline__ double cov_centre(double origin, int index, double cell) {
#pragma clang fp contract(off)
    return origin + ((double)index + 0.5) * cell;
}

// u, v of the rule with the X products given: bu = b0 * X, bv = b3 * X.
__device__ __forceinline__ void cov_uv(double bu, double bv, double b1, double b2, double b4, double b5, double Y, double& u, double& v) {
#pragma clang fp contract(off)
    u = (bu + b1 * Y) + b2;
    v = (bv + b4 * Y) + b5;
}

__device__ __forceinline__ bool cov_inside(double u, double v, double w, double h) {
#pragma clang fp contract(off)
    return 0.0 <= u && u < w && 0.0 <= v && v < h;
}

// sees(f, X, Y) with the X products given.  Mirrors cov_uv and cov_inside, statement for statement: built from the two
// calls, the frame loop of coverage_points_kernel measured slower (profiles/ground_family/).
__device__ __forceinline__ bool cov_sees(double bu, double bv, double b1, double b2, double b4, double b5, double Y, double w, double h) {
#pragma clang fp contract(off)
    const double u = (bu + b1 * Y) + b2;
    const double v = (bv + b4 * Y) + b5;
    return 0.0 <= u && u < w && 0.0 <= v && v < h;
}

__device__ __forceinline__ double cov_min4(double a, double b, double c, double d) { return fmin(fmin(a, b), fmin(c, d)); }
__device__ __forceinline__ double cov_max4(double a, double b, double c, double d) { return fmax(fmax(a, b), fmax(c, d)); }

// One affine row (c0, c1, c2) over the rectangle [xl, xh] x [yl, yh]: false when the computed value of every point of it
// provably lies outside [0, extent); xm, ym = max |x|, max |y| over the rectangle.
__device__ __forceinline__ bool cov_row_may_touch(double c0, double c1, double c2, double xl, double xh, double yl, double yh,
                                                  double xm, double ym, double extent) {
#pragma clang fp contract(off)
    const double p00 = (c0 * xl + c1 * yl) + c2, p10 = (c0 * xh + c1 * yl) + c2;
    const double p01 = (c0 * xl + c1 * yh) + c2, p11 = (c0 * xh + c1 * yh) + c2;
    const double m = ((fabs(c0) * xm + fabs(c1) * ym) + fabs(c2)) * 0x1p-50 + 0x1p-1022;
    const double lo = cov_min4(p00, p10, p01, p11) - m, hi = cov_max4(p00, p10, p01, p11) + m;
    if (!(cov_finite(p00) && cov_finite(p10) && cov_finite(p01) && cov_finite(p11) && cov_finite(lo) && cov_finite(hi))) return true;
    return !(hi < 0.0 || lo >= extent);
}

// What a thread of a raster / plan workgroup knows of its block of COV_BLOCK_X x COV_BLOCK_Y cells: its own column i, first
// row j0 and their centres, and the block's ground rectangle, the centres of its extreme cells by cov_centre itself.
struct CovBlock {
    int i, j0;
    double xl, xh, yl, yh, xm, ym;
    double Xc, Yc[COV_ROWS];

    __device__ __forceinline__ CovBlock(int lane, int wave, double x0, double y0, double cell, int gx, int gy) {
#pragma clang fp contract(off)
        const int i_first = blockIdx.x * COV_BLOCK_X, j_first = blockIdx.y * COV_BLOCK_Y;
        const int i_last = min(i_first + COV_BLOCK_X, gx) - 1, j_last = min(j_first + COV_BLOCK_Y, gy) - 1;
        i = i_first + lane, j0 = j_first + wave * COV_ROWS;
        xl = cov_centre(x0, i_first, cell), xh = cov_centre(x0, i_last, cell);
        yl = cov_centre(y0, j_first, cell), yh = cov_centre(y0, j_last, cell);
        xm = fmax(fabs(xl), fabs(xh)), ym = fmax(fabs(yl), fabs(yh));
        Xc = cov_centre(x0, i, cell);
#pragma unroll
        for (int r = 0; r < COV_ROWS; ++r) Yc[r] = cov_centre(y0, j0 + r, cell);
    }

    // The cull: false only when frame (b, h, w) provably sees no centre of the block.
    __device__ __forceinline__ bool may_touch(const double (&b)[6], int h, int w) const {
#pragma clang fp contract(off)
        return h >= 1 && w >= 1 && cov_row_may_touch(b[0], b[1], b[2], xl, xh, yl, yh, xm, ym, (double)w) &&
               cov_row_may_touch(b[3], b[4], b[5], xl, xh, yl, yh, xm, ym, (double)h);
    }
};

// Frame f's b[6] and (height, width); zeros and false past n_frames.  size is indexed in int on purpose: with (size_t)f * 2
// the helper's address arithmetic is formed in another order than the kernels' own text gave, and coverage_points_kernel's
// bytes change (profiles/ground_family/); f < n_frames <= WM_COVERAGE_MAX_FRAMES keeps f * 2 + 1 far inside int.
static_assert(WM_COVERAGE_MAX_FRAMES <= (1 << 29), "cov_load_frame indexes size[f * 2 + 1] in int");
__device__ __forceinline__ bool cov_load_frame(const double* __restrict__ g2p, const int* __restrict__ size, int f, int n_frames,
                                               double (&b)[6], int& h, int& w) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = 0.0;
    h = w = 0;
    const bool in_range = f < n_frames;
    if (in_range) {
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = g2p[(size_t)f * 6 + k];
        h = size[f * 2];
        w = size[f * 2 + 1];
    }
    return in_range;
}

// The pixel that holds (u, v), for 0 <= u < w, 0 <= v < height.
__device__ __forceinline__ const unsigned char* cov_nearest_pixel(const frame_desc& fd, int w, double u, double v) {
#pragma clang fp contract(off)
    return fd.data + ((size_t)(int)floor(v) * w + (int)floor(u)) * 3;
}

// Stages the frames of a chunk (one per thread: b, h, w) that pass `keep` into s, compacted by a wave ballot; returns
// their number.  All threads call it; it syncs before its writes' slots are known and after the writes.  slot_out, when given,
// receives the slot of a kept frame (-1 otherwise), for a caller that stages more per frame (mosaic_kernels.h: its index).
__device__ __forceinline__ int cov_stage(CovFrames& s, int* s_wave, bool keep, const double (&b)[6], int h, int w, int* slot_out = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < COV_THREADS / 64; ++k) {
        const int c = s_wave[k];
        off += k < wave ? c : 0;
        total += c;
    }
    if (slot_out) *slot_out = -1;
    if (keep) {
        const int slot = off + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
        for (int k = 0; k < 6; ++k) s.b[k][slot] = b[k];
        s.h[slot] = h;
        s.w[slot] = w;
        if (slot_out) *slot_out = slot;
    }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(COV_THREADS) void coverage_raster_kernel(
        const double* __restrict__ g2p, const int* __restrict__ size, int n_frames, double x0, double y0, double cell, int gx, int gy,
        uint16_t* __restrict__ coverage, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ CovFrames s;
    __shared__ int s_wave[COV_THREADS / 64];
    __shared__ int s_hist[COV_STATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovBlock blk(lane, wave, x0, y0, cell, gx, gy);
    const int i = blk.i, j0 = blk.j0;
    if (tid < COV_STATS) s_hist[tid] = 0;
    int cnt[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) cnt[r] = 0;

    for (int base = 0; base < n_frames; base += COV_CHUNK) {
        double b[6];
        int h, w;
        bool keep = false;
        if (cov_load_frame(g2p, size, base + tid, n_frames, b, h, w)) keep = blk.may_touch(b, h, w);
        const int n_s = cov_stage(s, s_wave, keep, b, h, w);
        for (int q = 0; q < n_s; ++q) {
            const double b1 = s.b[1][q], b2 = s.b[2][q], b4 = s.b[4][q], b5 = s.b[5][q];
            const double fw = (double)s.w[q], fh = (double)s.h[q];
            const double bu = s.b[0][q] * blk.Xc, bv = s.b[3][q] * blk.Xc;
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r) cnt[r] += cov_sees(bu, bv, b1, b2, b4, b5, blk.Yc[r], fw, fh) ? 1 : 0;
        }
        __syncthreads();                                     // the chunk is read before the next one overwrites it
    }
    __syncthreads();                                         // s_hist zeroed (n_frames == 0 passes no other barrier)

    if (i < gx) {
#pragma unroll
        for (int r = 0; r < COV_ROWS; ++r) {
            const int j = j0 + r;
            if (j < gy) {
                coverage[(size_t)j * gx + i] = (uint16_t)cnt[r];
                atomicAdd(&s_hist[min(cnt[r], COV_STATS - 1)], 1);
            }
        }
    }
    __syncthreads();
    if (tid < COV_STATS && s_hist[tid] != 0) atomicAdd(&stats[tid], (unsigned long long)s_hist[tid]);
}

__global__ __launch_bounds__(COV_THREADS) void coverage_points_kernel(
        const double* __restrict__ g2p, const int* __restrict__ size, int n_frames, const double* __restrict__ points,
        const int* __restrict__ labels, int n_points, double x0, double y0, double cell, int gx, int gy, int* __restrict__ seen_by,
        int* __restrict__ cell_out, int* __restrict__ counts, unsigned long long* __restrict__ pstats) {
#pragma clang fp contract(off)
    __shared__ CovFrames s;
    __shared__ int s_wave[COV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = blockIdx.x * COV_THREADS + tid;
    const bool live = p < n_points;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double X = live ? points[(size_t)p * 2] : nan, Y = live ? points[(size_t)p * 2 + 1] : nan;
    const bool finite = cov_finite(X) && cov_finite(Y);
    int seen = 0;
    for (int base = 0; base < n_frames; base += COV_CHUNK) {
        double b[6];
        int h, w;
        const bool in_range = cov_load_frame(g2p, size, base + tid, n_frames, b, h, w);
        const int n_s = cov_stage(s, s_wave, in_range && h >= 1 && w >= 1, b, h, w);
        if (finite)
            for (int q = 0; q < n_s; ++q)
                seen += cov_sees(s.b[0][q] * X, s.b[3][q] * X, s.b[1][q], s.b[2][q], s.b[4][q], s.b[5][q], Y, (double)s.w[q],
                                 (double)s.h[q]) ? 1 : 0;
        __syncthreads();
    }
    bool binned = false;
    int ci = -1, cj = -1;
    if (live) {
        const int label = labels[p];
        const double fi = floor((X - x0) / cell), fj = floor((Y - y0) / cell);
        binned = finite && 0.0 <= fi && fi < (double)gx && 0.0 <= fj && fj < (double)gy && 0 <= label && label < COV_CLASSES;
        if (binned) {
            ci = (int)fi;
            cj = (int)fj;
            if (counts) atomicAdd(&counts[((size_t)label * gy + cj) * gx + ci], 1);
        }
        seen_by[p] = seen;
        cell_out[(size_t)p * 2] = cj;
        cell_out[(size_t)p * 2 + 1] = ci;
    }
    const unsigned long long in = __ballot(live && binned), out = __ballot(live && !binned);
    if (lane == 0) {
        if (in) atomicAdd(&pstats[0], (unsigned long long)__popcll(in));
        if (out) atomicAdd(&pstats[1], (unsigned long long)__popcll(out));
    }
}

}  // namespace wm
