// Survey mosaic, blended (include/wm_hip.h, "Survey mosaic, blended"): every ground cell is an integer-weighted mean of the
// exposure-corrected pixels of the frames that see it.  A frame's weight falls to zero at its own border and, over `band`
// source pixels, away from the frame whose border is farthest (the seam).  No reference behaviour exists; the rule is the
// header's, and the checker is its sequential restatement blend_oracle in tests/ground_oracle.py.  The weights are
// integers behind double arithmetic with one rounding per operation (no contraction) and the sums are integers, so every
// kernel equals the oracle bit for bit and the accumulators do not depend on how the frames are split over calls.  The
// grid, the centres, the staging and the cull are the coverage's (coverage_kernels.h: CovBlock, cov_load_frame, cov_stage,
// cov_uv, cov_inside) and the sampling and the row store the mosaic's (mosaic_kernels.h: mos_sample, mos_store_row),
// included, not copied.
//
// mosaic_blend_plan_kernel, geometry only: the shape of mosaic_plan_kernel, with two walks over the frames.  The first
// keeps each cell's largest border distance m*; the second, which needs the finished m*, counts the frames whose weight is
// positive.  Both walks stage the same chunks behind the same cull, and neither depends on the order of the frames: m* is
// a maximum, and a tie (m_f == m*) is decided by the comparison alone, wherever the chunk boundary falls.  cells takes one
// int32 atomic per (wave, staged frame) after eight ballots, stats three 64-bit atomics per workgroup after an LDS
// reduction; no atomics touch best.
//
// mosaic_blend_accum_kernel, the pixel gather: a workgroup owns a block of cells and walks the RESIDENT frames only (thread
// t of a chunk takes resident slot base + t, checks it, and culls it against the block).  The four sums of a cell stay in
// registers across all staged frames; acc is read, added to and stored once per cell, and only where a resident frame
// contributed.  best is loaded when the first frame survives the cull, so a workgroup whose block no resident frame can
// touch reads and writes nothing but the frame tables.  What bounds every read: 0 <= index < n_frames, a non-null data
// pointer, the descriptor's (height, width) equal to size[f], and 0 <= u < width, 0 <= v < height (cov_inside); a slot that
// fails a check is skipped, and the workgroup of block (0, 0), which every launch has, reports it.
//
// mosaic_blend_finish_kernel: one pass, a cell per thread and MOS_FILL_ROWS rows per thread as in the fill; 16 bytes in,
// 3 out, through mos_store_row.
#pragma once

#include "coverage_kernels.h"
#include "mosaic_kernels.h"

namespace wm {

// m_f: the distance of (u, v) to the nearest border of a w x h frame, in its pixels.
__device__ __forceinline__ double blend_border(double u, double v, double fw, double fh) {
#pragma clang fp contract(off)
    return fmin(fmin(u, fw - u), fmin(v, fh - v));
}

// q_f of the header from m_f, the cell's m* and k = 256 / band.  For m >= best the seam term is 256 and edge <= 256 decides.
__device__ __forceinline__ int blend_weight(double m, double best, double band, double k) {
#pragma clang fp contract(off)
    const double edge = fmin(m * k, 256.0);
    if (m >= best) return max((int)floor(edge), 1);
    const double seam = fmin(fmax(((m - best) + band) * k, 0.0), 255.0);
    return (int)floor(fmin(seam, edge));
}

// p' of the header: one channel through the Q12 gain and offset.  >> of a negative int64 is arithmetic, that is floor.
__device__ __forceinline__ unsigned int blend_expose(int gain, int offset, unsigned char p) {
    const long long t = ((long long)gain * (long long)p + (long long)offset + 2048ll) >> 12;
    return (unsigned int)min(max(t, 0ll), 255ll);
}

__global__ __launch_bounds__(COV_THREADS) void mosaic_blend_plan_kernel(
        const double* __restrict__ g2p, const int* __restrict__ size, int n_frames, double x0, double y0, double cell, int gx, int gy,
        double band, double k, double* __restrict__ best_out, int* __restrict__ cells, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ CovFrames s;
    __shared__ int s_idx[COV_CHUNK];                         // the survey index of each staged frame (second walk)
    __shared__ int s_wave[COV_THREADS / 64];
    __shared__ int s_cnt[3][COV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovBlock blk(lane, wave, x0, y0, cell, gx, gy);
    const int i = blk.i, j0 = blk.j0;
    double best[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) best[r] = -1.0;       // m_f >= 0: the first frame that sees the cell is larger

    for (int base = 0; base < n_frames; base += COV_CHUNK) { // first walk: m*
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
            for (int r = 0; r < COV_ROWS; ++r) {
                double u, v;
                cov_uv(bu, bv, b1, b2, b4, b5, blk.Yc[r], u, v);
                if (cov_inside(u, v, fw, fh)) {
                    const double m = blend_border(u, v, fw, fh);
                    if (m > best[r]) best[r] = m;
                }
            }
        }
        __syncthreads();                                     // the chunk is read before the next one overwrites it
    }

    int nq[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) nq[r] = 0;
    for (int base = 0; base < n_frames; base += COV_CHUNK) { // second walk: the frames with q > 0, against the finished m*
        const int f = base + tid;
        double b[6];
        int h, w;
        bool keep = false;
        if (cov_load_frame(g2p, size, f, n_frames, b, h, w)) keep = blk.may_touch(b, h, w);
        int slot_f = -1;
        const int n_s = cov_stage(s, s_wave, keep, b, h, w, &slot_f);
        if (slot_f >= 0) s_idx[slot_f] = f;
        __syncthreads();
        for (int q = 0; q < n_s; ++q) {
            const double b1 = s.b[1][q], b2 = s.b[2][q], b4 = s.b[4][q], b5 = s.b[5][q];
            const double fw = (double)s.w[q], fh = (double)s.h[q];
            const double bu = s.b[0][q] * blk.Xc, bv = s.b[3][q] * blk.Xc;
            int in_wave = 0;
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r) {
                double u, v;
                cov_uv(bu, bv, b1, b2, b4, b5, blk.Yc[r], u, v);
                bool c = i < gx && j0 + r < gy && cov_inside(u, v, fw, fh);
                if (c) c = blend_weight(blend_border(u, v, fw, fh), best[r], band, k) > 0;
                nq[r] += c ? 1 : 0;
                in_wave += __popcll(__ballot(c));
            }
            if (lane == 0 && in_wave) atomicAdd(&cells[s_idx[q]], in_wave);
        }
        __syncthreads();
    }

    int seen = 0, gap = 0, many = 0;
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        const int j = j0 + r;
        const bool live = i < gx && j < gy;
        if (live) best_out[(size_t)j * gx + i] = best[r];
        seen += live && best[r] >= 0.0 ? 1 : 0;
        gap += live && !(best[r] >= 0.0) ? 1 : 0;
        many += nq[r] >= 2 ? 1 : 0;                          // nq counts live cells only
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        seen += __shfl_xor(seen, d);
        gap += __shfl_xor(gap, d);
        many += __shfl_xor(many, d);
    }
    if (lane == 0) {
        s_cnt[0][wave] = seen;
        s_cnt[1][wave] = gap;
        s_cnt[2][wave] = many;
    }
    __syncthreads();
    if (tid < 3) {
        int a = 0;
#pragma unroll
        for (int w = 0; w < COV_THREADS / 64; ++w) a += s_cnt[tid][w];
        if (a) atomicAdd(&stats[tid], (unsigned long long)a);
    }
}

template <int MODE>
__global__ __launch_bounds__(COV_THREADS) void mosaic_blend_accum_kernel(
        const frame_desc* __restrict__ frames, const int* __restrict__ index, int n_resident, const double* __restrict__ g2p,
        const int* __restrict__ size, int n_frames, const int* __restrict__ exposure, double x0, double y0, double cell, int gx, int gy,
        double band, double k, const double* __restrict__ best, unsigned int* __restrict__ acc, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ CovFrames s;
    __shared__ const unsigned char* s_data[COV_CHUNK];       // beside each staged frame: its pixels and its exposure
    __shared__ int s_gain[COV_CHUNK], s_offset[COV_CHUNK];
    __shared__ int s_wave[COV_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovBlock blk(lane, wave, x0, y0, cell, gx, gy);
    const int i = blk.i, j0 = blk.j0;
    unsigned int sum[COV_ROWS][4];
    double bst[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        sum[r][0] = sum[r][1] = sum[r][2] = sum[r][3] = 0u;
        bst[r] = 0.0;
    }
    bool loaded = false;
    int bad = 0;

    for (int base = 0; base < n_resident; base += COV_CHUNK) {
        const int rs = base + tid;
        int f = n_frames;                                    // past the survey: cov_load_frame loads nothing
        if (rs < n_resident) {
            f = index[rs];
            if (f < 0 || f >= n_frames) {
                bad |= WM_MOSAIC_BAD_SLOT;
                f = n_frames;
            }
        }
        double b[6];
        int h, w, gain = 4096, offset = 0;
        const unsigned char* data = nullptr;
        bool keep = false;
        if (cov_load_frame(g2p, size, f, n_frames, b, h, w)) {
            const frame_desc fd = frames[rs];
            if (!fd.data) {
                bad |= WM_MOSAIC_BAD_SLOT;
            } else if (fd.height != h || fd.width != w) {
                bad |= WM_MOSAIC_BAD_SIZE;
            } else {
                keep = blk.may_touch(b, h, w);
                data = fd.data;
                if (exposure) {
                    gain = exposure[f * 2];
                    offset = exposure[f * 2 + 1];
                }
            }
        }
        int slot_f = -1;
        const int n_s = cov_stage(s, s_wave, keep, b, h, w, &slot_f);
        if (slot_f >= 0) {
            s_data[slot_f] = data;
            s_gain[slot_f] = gain;
            s_offset[slot_f] = offset;
        }
        __syncthreads();
        if (n_s > 0 && !loaded) {                            // workgroup-uniform: the first frame that may touch the block
            loaded = true;
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r)
                if (i < gx && j0 + r < gy) bst[r] = best[(size_t)(j0 + r) * gx + i];
        }
        for (int q = 0; q < n_s; ++q) {
            const double b1 = s.b[1][q], b2 = s.b[2][q], b4 = s.b[4][q], b5 = s.b[5][q];
            const int fwi = s.w[q], fhi = s.h[q];
            const double fw = (double)fwi, fh = (double)fhi;
            const double bu = s.b[0][q] * blk.Xc, bv = s.b[3][q] * blk.Xc;
            const frame_desc fd = {s_data[q], fhi, fwi};
            const int ga = s_gain[q], of = s_offset[q];
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r) {
                double u, v;
                cov_uv(bu, bv, b1, b2, b4, b5, blk.Yc[r], u, v);
                if (i < gx && j0 + r < gy && cov_inside(u, v, fw, fh)) {
                    const int qf = blend_weight(blend_border(u, v, fw, fh), bst[r], band, k);
                    if (qf > 0) {
                        unsigned char px[3];
                        mos_sample<MODE>(fd, fhi, fwi, u, v, px);
                        sum[r][0] += (unsigned int)qf * blend_expose(ga, of, px[0]);
                        sum[r][1] += (unsigned int)qf * blend_expose(ga, of, px[1]);
                        sum[r][2] += (unsigned int)qf * blend_expose(ga, of, px[2]);
                        sum[r][3] += (unsigned int)qf;
                    }
                }
            }
        }
        __syncthreads();                                     // the chunk is read before the next one overwrites it
    }

#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        if (sum[r][3] > 0u) {                                // only a live cell with a contribution: read, add, store
            unsigned int* a = acc + ((size_t)(j0 + r) * gx + i) * 4;
            const unsigned int a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
            a[0] = a0 + sum[r][0];
            a[1] = a1 + sum[r][1];
            a[2] = a2 + sum[r][2];
            a[3] = a3 + sum[r][3];
        }
    }
    if (bad && blockIdx.x == 0 && blockIdx.y == 0) atomicOr(status, bad);
}

// (acc_c + (wsum >> 1)) / wsum in uint32: acc_c <= 65535 * 256 * 255 = 4 278 124 800 and wsum >> 1 <= 65535 * 128 =
// 8 388 480, so the sum is at most 4 286 513 280 < 2^32.
__global__ __launch_bounds__(COV_THREADS) void mosaic_blend_finish_kernel(const unsigned int* __restrict__ acc, int gx, int gy, int north_up,
                                                                          unsigned char* __restrict__ mosaic) {
    __shared__ unsigned int s_row[COV_THREADS / 64][48];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_first = blockIdx.x * COV_BLOCK_X;
    const int i = i_first + lane, j0 = blockIdx.y * MOS_FILL_BLOCK_Y + wave * MOS_FILL_ROWS;
#pragma unroll
    for (int r = 0; r < MOS_FILL_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= gy) break;                                  // wave-uniform
        unsigned char px[3] = {0, 0, 0};
        bool wr = false;
        if (i < gx) {
            const unsigned int* a = acc + ((size_t)j * gx + i) * 4;
            const unsigned int a0 = a[0], a1 = a[1], a2 = a[2], ws = a[3];
            wr = ws > 0u;
            if (wr) {
                const unsigned int half = ws >> 1;
                px[0] = (unsigned char)((a0 + half) / ws);
                px[1] = (unsigned char)((a1 + half) / ws);
                px[2] = (unsigned char)((a2 + half) / ws);
            }
        }
        unsigned char* row = mosaic + ((size_t)(north_up ? gy - 1 - j : j) * gx + i_first) * 3;
        mos_store_row(s_row[wave], row, lane, __ballot(wr) == ~0ull && ((uintptr_t)row & 3) == 0, wr, px);
    }
}

}  // namespace wm
