// Survey mosaic (include/wm_hip.h, "Survey mosaic"): the frames of a survey laid onto the ground grid of the coverage.
// Every cell chooses ONE frame among those that see its centre -- the one whose centre pixel is nearest, ties to the lowest
// index -- and fetches that frame's pixel.  No reference behaviour exists; the rule is the header's, and the checker is its
// sequential restatement mosaic_oracle in tests/ground_oracle.py.  All arithmetic is IEEE double with one rounding per
// operation (no contraction), so both kernels equal the oracle bit for bit.  The grid, the centres, the staging and the
// cull are the coverage's (coverage_kernels.h: CovBlock, whose may_touch is the two cov_row_may_touch() calls, cov_load_frame,
// cov_stage, cov_uv, cov_inside), included, not copied.
//
// mosaic_plan_kernel, geometry only: the shape of coverage_raster_kernel.  A workgroup of COV_THREADS owns COV_BLOCK_X x
// COV_BLOCK_Y cells, lane = column, a thread owns COV_ROWS cells of one column; the frames are staged through LDS in
// chunks of COV_CHUNK after the conservative cull (which drops only frames that see no centre of the block, hence no
// candidate), and each cell keeps a running (best e, best f).  cov_stage hands back each kept frame's slot, and the frame's
// survey index goes into a second LDS array at that slot.
//   Tie rule.  The chunks walk the frames in ascending index, a thread stages frame base + tid, and the ballot compaction
//   keeps the order of the lanes and of the waves, so the staged list is ascending in f over the whole walk.  A strict
//   e < best therefore keeps the first, that is the lowest, index among equal e.
// No atomics touch source.  won takes one int32 atomic per (wave, row, distinct winner) -- the lanes of a row that chose
// the same frame are counted by a ballot first, and a row of 64 cells has a handful of winners -- and stats two 64-bit
// atomics per workgroup after a reduction in LDS.
//
// mosaic_fill_kernel, the pixel gather: lane = column, so a wave reads 64 consecutive int32 of source and its stores cover
// 192 contiguous bytes of one row of the picture (as 48 dwords through LDS when the whole row is written).  A cell is written iff its source is resident (slot[f] >= 0); every other
// byte is left alone, so the frames may be split over any number of calls.  u, v are recomputed with the plan's
// expression from the same operands, so they have the plan's bits.  What bounds every read: f < n_frames, slot <
// n_resident, a non-null data pointer, the descriptor's (height, width) equal to size[f], and 0 <= u < width, 0 <= v <
// height re-checked here (a source raster that did not come from the plan of these frames cannot index outside a frame);
// a cell that fails one of them is skipped and a status bit is set.
// The sampling (mos_sample) and the store of a wave's row (mos_store_row) are functions of their own: the blended mosaic
// (mosaic_blend_kernels.h) samples and stores through them too.
#pragma once

#include "coverage_kernels.h"
#include "survey_kernels.h"

namespace wm {

constexpr int MOS_FILL_ROWS = 4;                                  // cells per thread of the fill, consecutive rows of one column
constexpr int MOS_FILL_BLOCK_Y = (COV_THREADS / 64) * MOS_FILL_ROWS;

__global__ __launch_bounds__(COV_THREADS) void mosaic_plan_kernel(
        const double* __restrict__ g2p, const int* __restrict__ size, int n_frames, double x0, double y0, double cell, int gx, int gy,
        int* __restrict__ source, int* __restrict__ won, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ CovFrames s;
    __shared__ int s_idx[COV_CHUNK];                         // the survey index of each staged frame
    __shared__ int s_wave[COV_THREADS / 64];
    __shared__ int s_with[COV_THREADS / 64], s_without[COV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovBlock blk(lane, wave, x0, y0, cell, gx, gy);
    const int i = blk.i, j0 = blk.j0;
    double best[COV_ROWS];
    int src[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        best[r] = __longlong_as_double(0x7ff0000000000000ll);    // +inf: the first frame that sees the cell is smaller
        src[r] = -1;
    }

    for (int base = 0; base < n_frames; base += COV_CHUNK) {
        const int f = base + tid;
        double b[6];
        int h, w;
        bool keep = false;
        if (cov_load_frame(g2p, size, f, n_frames, b, h, w)) keep = blk.may_touch(b, h, w);
        int slot_f = -1;
        const int n_s = cov_stage(s, s_wave, keep, b, h, w, &slot_f);
        if (slot_f >= 0) s_idx[slot_f] = f;                  // the frame's index beside it, in the slot cov_stage gave it
        __syncthreads();
        for (int q = 0; q < n_s; ++q) {                      // ascending f: a strict < keeps the lowest index of a tie
            const double b1 = s.b[1][q], b2 = s.b[2][q], b4 = s.b[4][q], b5 = s.b[5][q];
            const double fw = (double)s.w[q], fh = (double)s.h[q];
            const double cu = 0.5 * fw, cv = 0.5 * fh;
            const double bu = s.b[0][q] * blk.Xc, bv = s.b[3][q] * blk.Xc;
            const int fq = s_idx[q];
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r) {
                double u, v;
                cov_uv(bu, bv, b1, b2, b4, b5, blk.Yc[r], u, v);
                const double du = u - cu, dv = v - cv;
                const double e = du * du + dv * dv;
                if (0.0 <= u && u < fw && 0.0 <= v && v < fh && e < best[r]) {     // mirrors cov_inside (coverage_kernels.h)
                    best[r] = e;
                    src[r] = fq;
                }
            }
        }
        __syncthreads();                                     // the chunk is read before the next one overwrites it
    }

    int with = 0, without = 0;
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        const int j = j0 + r;
        const bool live = i < gx && j < gy;
        if (live) source[(size_t)j * gx + i] = src[r];
        const bool has = live && src[r] >= 0;
        with += has ? 1 : 0;
        without += live && !has ? 1 : 0;
        // the cells of this row each frame won: one atomic per distinct winner (wave-uniform loop)
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int fl = __shfl(src[r], leader);
            const unsigned long long same = __ballot(has && src[r] == fl);
            if (lane == leader) atomicAdd(&won[fl], __popcll(same));
            todo &= ~same;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        with += __shfl_xor(with, d);
        without += __shfl_xor(without, d);
    }
    if (lane == 0) {
        s_with[wave] = with;
        s_without[wave] = without;
    }
    __syncthreads();
    if (tid == 0) {
        int a = 0, c = 0;
#pragma unroll
        for (int k = 0; k < COV_THREADS / 64; ++k) {
            a += s_with[k];
            c += s_without[k];
        }
        if (a) atomicAdd(&stats[0], (unsigned long long)a);
        if (c) atomicAdd(&stats[1], (unsigned long long)c);
    }
}

// One channel of one cell, WM_MOSAIC_BILINEAR: the header's three products-and-sums and the rounding to uint8.
__device__ __forceinline__ unsigned char mos_lerp(double p00, double p10, double p01, double p11, double tx, double ty) {
#pragma clang fp contract(off)
    const double a = (1.0 - tx) * p00 + tx * p10;
    const double b = (1.0 - tx) * p01 + tx * p11;
    const double val = (1.0 - ty) * a + ty * b;
    return (unsigned char)fmin(floor(val + 0.5), 255.0);
}

// The header's sampling rule: the three bytes of frame fd (h x w, checked by the caller) at the pixel position (u, v), 0 <= u
// < w, 0 <= v < h.  The fill and the blend's accumulate (mosaic_blend_kernels.h) both sample through it.
template <int MODE>
__device__ __forceinline__ void mos_sample(const frame_desc& fd, int h, int w, double u, double v, unsigned char (&px)[3]) {
#pragma clang fp contract(off)
    if (MODE == WM_MOSAIC_NEAREST) {
        const unsigned char* p = cov_nearest_pixel(fd, w, u, v);
        px[0] = p[0];
        px[1] = p[1];
        px[2] = p[2];
    } else {
        const double fu = u - 0.5, fv = v - 0.5;
        const double xf = floor(fu), yf = floor(fv);
        const double tx = fu - xf, ty = fv - yf;
        const int xa = min(max((int)xf, 0), w - 1), xb = min(max((int)xf + 1, 0), w - 1);
        const int ya = min(max((int)yf, 0), h - 1), yb = min(max((int)yf + 1, 0), h - 1);
        const unsigned char* p00 = fd.data + ((size_t)ya * w + xa) * 3;
        const unsigned char* p10 = fd.data + ((size_t)ya * w + xb) * 3;
        const unsigned char* p01 = fd.data + ((size_t)yb * w + xa) * 3;
        const unsigned char* p11 = fd.data + ((size_t)yb * w + xb) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = mos_lerp((double)p00[c], (double)p10[c], (double)p01[c], (double)p11[c], tx, ty);
    }
}

// One cell of the fill: false when it is not written (no source, a source that is not resident, or a failed check, which
// sets a bit of `bad`); else its three bytes in px.
template <int MODE>
__device__ __forceinline__ bool mos_cell(const frame_desc* __restrict__ frames, int n_resident, const int* __restrict__ slot,
                                         const double* __restrict__ g2p, const int* __restrict__ size, int n_frames, int f, double Xc,
                                         double Y, int& bad, unsigned char (&px)[3]) {
#pragma clang fp contract(off)
    if (f < 0) return false;                                 // no frame saw the cell
    if (f >= n_frames) { bad |= WM_MOSAIC_BAD_SOURCE; return false; }
    const int sl = slot[f];                                  // the residency chain: register_render_kernel mirrors it, statement for statement
    if (sl < 0) return false;                                // its frame is not resident in this call
    if (sl >= n_resident) { bad |= WM_MOSAIC_BAD_SLOT; return false; }
    const frame_desc fd = frames[sl];
    const int h = size[(size_t)f * 2], w = size[(size_t)f * 2 + 1];
    if (!fd.data) { bad |= WM_MOSAIC_BAD_SLOT; return false; }
    if (fd.height != h || fd.width != w) { bad |= WM_MOSAIC_BAD_SIZE; return false; }
    const double* b = g2p + (size_t)f * 6;
    double u, v;
    cov_uv(b[0] * Xc, b[3] * Xc, b[1], b[2], b[4], b[5], Y, u, v);
    if (!cov_inside(u, v, (double)w, (double)h)) { bad |= WM_MOSAIC_BAD_SOURCE; return false; }   // not the plan's source
    mos_sample<MODE>(fd, h, w, u, v, px);
    return true;
}

// A row of a wave whose 64 cells are all written, and whose 192 bytes start on a dword, goes through LDS and leaves as 48
// dword stores; every other row as three byte stores per cell (a dword that holds a byte of a cell that is not written
// must not be stored: that byte is left as it was).  Measured against byte stores everywhere at F = 1 000 on 8192 x 8192
// cells: -3 % (nearest) and -5 % (bilinear), profiles/mosaic/.  s_wave_row is the wave's own 48 dwords of LDS, row the
// picture's first byte of the wave's 64 cells; wr: this lane's cell is written; packed, wave-uniform: __ballot(wr) == ~0ull &&
// ((uintptr_t)row & 3) == 0, which the CALLER writes out (evaluated in here or in a helper, the fill's code comes out with the
// operands of four scalar ORs swapped: the same work, other bytes).
__device__ __forceinline__ void mos_store_row(unsigned int (&s_wave_row)[48], unsigned char* row, int lane, bool packed, bool wr,
                                              const unsigned char (&px)[3]) {
    if (packed) {
        unsigned char* sb = (unsigned char*)s_wave_row;
        sb[lane * 3] = px[0];
        sb[lane * 3 + 1] = px[1];
        sb[lane * 3 + 2] = px[2];
        __builtin_amdgcn_wave_barrier();                     // the wave's LDS writes are issued before its reads
        if (lane < 48) ((unsigned int*)row)[lane] = s_wave_row[lane];
        __builtin_amdgcn_wave_barrier();                     // and the reads before the next row's writes
    } else if (wr) {
        unsigned char* out = row + lane * 3;
        out[0] = px[0];
        out[1] = px[1];
        out[2] = px[2];
    }
}

template <int MODE>
__global__ __launch_bounds__(COV_THREADS) void mosaic_fill_kernel(
        const frame_desc* __restrict__ frames, int n_resident, const int* __restrict__ slot, const double* __restrict__ g2p,
        const int* __restrict__ size, int n_frames, double x0, double y0, double cell, int gx, int gy, const int* __restrict__ source,
        int north_up, unsigned char* __restrict__ mosaic, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ unsigned int s_row[COV_THREADS / 64][48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_first = blockIdx.x * COV_BLOCK_X;
    const int i = i_first + lane, j0 = blockIdx.y * MOS_FILL_BLOCK_Y + wave * MOS_FILL_ROWS;
    const double Xc = cov_centre(x0, i, cell);
    int bad = 0;
#pragma unroll
    for (int r = 0; r < MOS_FILL_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= gy) break;                                  // wave-uniform
        unsigned char px[3] = {0, 0, 0};
        const bool wr = i < gx && mos_cell<MODE>(frames, n_resident, slot, g2p, size, n_frames, source[(size_t)j * gx + i], Xc,
                                                 cov_centre(y0, j, cell), bad, px);
        unsigned char* row = mosaic + ((size_t)(north_up ? gy - 1 - j : j) * gx + i_first) * 3;
        mos_store_row(s_row[wave], row, lane, __ballot(wr) == ~0ull && ((uintptr_t)row & 3) == 0, wr, px);
    }
    if (bad) atomicOr(status, bad);
}

}  // namespace wm
