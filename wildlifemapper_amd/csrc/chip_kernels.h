// Survey review chips (wm_crop_chips_u8, wm_chip_window): one fixed-size crop per detection, cut out of the frame the
// detection lies in and resampled to chip x chip pixels with the 8-bit arithmetic of Pillow's ImagingResample (bilinear),
// every chip with a window and a scale of its own, in one launch.  No reference behaviour exists for this step (the
// reference draws boxes into a frame it has down-scaled to 768 px, visualize_prediction.py).
//   * chip_window_of: the chip rule, box -> square window (y0, x0, side) in frame pixels; host and device.
//   * crop_chips_kernel: a workgroup makes a band of CHIP_BAND_ROWS output rows of one chip.  It derives the window from the
//     device-resident box, builds the one coefficient table both axes share (square window, square chip) in LDS with
//     resize_coeff_row, filters the window rows its band reads horizontally into LDS, and filters those vertically into
//     the chip.  The chip is PIL.Image.fromarray(Wimg).resize((chip, chip), BILINEAR) bit for bit, Wimg the window's pixels
//     with zeros where it reaches past the frame: taps are clipped at the window's edge, zeros from outside the frame are
//     ordinary pixels.  Where side == chip Pillow skips both passes; the table is then the identity (coefficients 2^22 and
//     0), so the same code path returns the window's pixels.
#pragma once

#include "resample_kernels.h"
#include "survey_kernels.h"

namespace wm {

constexpr int CHIP_MAX_SIDE = 1024;     // WM_CHIP_MAX_SIDE
constexpr int CHIP_BAND_ROWS = 8;       // output rows per workgroup
constexpr int CHIP_STAGE_DWORDS = 3072; // LDS staging of raw frame rows: four rows of the widest window (770 dwords each)

struct chip_window { int y0, x0, side; };

// The chip rule.  fp32, every operation rounded on its own.  A box with a non-finite coordinate gives (0, 0, 0).
__host__ __device__ inline chip_window chip_window_of(const float* box, float context, int min_side, int max_side) {
#pragma clang fp contract(off)
    const float x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    if (!(__builtin_isfinite(x0) && __builtin_isfinite(y0) && __builtin_isfinite(x1) && __builtin_isfinite(y1))) return chip_window{0, 0, 0};
    const float bw = x1 - x0, bh = y1 - y0;
    const float m = bw > bh ? bw : bh;
    float s = ceilf(m * context);
    s = s > (float)min_side ? s : (float)min_side;
    s = s < (float)max_side ? s : (float)max_side;
    const int side = (int)s;
    const float cx = (x0 + x1) * 0.5f, cy = (y0 + y1) * 0.5f;
    const float lim = 1073741824.f;     // 2^30: the window's far edge stays inside int32
    float wx = floorf(cx - 0.5f * side), wy = floorf(cy - 0.5f * side);
    wx = wx > -lim ? wx : -lim; wx = wx < lim ? wx : lim;
    wy = wy > -lim ? wy : -lim; wy = wy < lim ? wy : lim;
    return chip_window{(int)wy, (int)wx, side};
}

// LDS plan of crop_chips_kernel for chips of `chip` pixels and windows up to max_side (host and device agree through these).
// kk: chip * ksize <= chip * (2 * ceil(side / chip) + 1) <= 2 * side + 3 * chip coefficients.
__host__ __device__ inline int chip_kk_cap(int chip, int max_side) { return 2 * max_side + 3 * chip; }
// window rows a band of R output rows reads: its last output's last tap minus its first output's first tap,
// <= (R - 1) * scale + 2 * support + 1 with scale = side / chip, support = max(scale, 1).
__host__ __device__ inline int chip_rows_cap(int chip, int max_side) {
    const int s = max_side > chip ? max_side : chip;
    return ((CHIP_BAND_ROWS + 1) * s + chip - 1) / chip + 2;
}
__host__ __device__ inline int chip_lds_bytes(int chip, int max_side) {
    return (2 * chip + chip_kk_cap(chip, max_side) + CHIP_STAGE_DWORDS) * 4 + chip_rows_cap(chip, max_side) * chip * 3;
}

// frames [n_frames], boxes [n][4] xyxy fp32, box_frame [n] or NULL (all frame 0) -> chips [n][S][S][3] u8 (4-byte aligned,
// S % 4 == 0: every output row starts on a dword), windows [n][3] = (y0, x0, side) or NULL.  Grid: n * ceil(S / 8)
// workgroups.  LDS (chip_lds_bytes): bounds [S][2] | kk [S][ksize] | the horizontally filtered rows [rows][S * 3] u8 |
// raw frame rows staged as aligned dwords.  Frame rows have any byte length and alignment: a row's clipped span is
// fetched as the aligned dwords that cover it, each holding at least one byte of the frame.  A chip whose box is not
// finite, whose frame index is out of range or whose window does not meet its frame is all zeros, and no address is
// formed from it.
__global__ __launch_bounds__(256) void crop_chips_kernel(const frame_desc* __restrict__ frames, int n_frames, const float* __restrict__ boxes,
                                                         const int* __restrict__ box_frame, int S, float context, int min_side,
                                                         int max_side, unsigned char* __restrict__ chips, int* __restrict__ windows) {
    extern __shared__ __attribute__((aligned(16))) unsigned chip_smem[];
    const int tid = threadIdx.x;
    const int bands = (S + CHIP_BAND_ROWS - 1) / CHIP_BAND_ROWS;
    const int ci = blockIdx.x / bands, band = blockIdx.x - ci * bands;
    const int r0 = band * CHIP_BAND_ROWS, r1 = min(r0 + CHIP_BAND_ROWS, S);
    const int row_dw = S * 3 / 4;
    unsigned* out = (unsigned*)(chips + (int64_t)ci * S * S * 3) + (int64_t)r0 * row_dw;
    const int out_dw = (r1 - r0) * row_dw;

    const int f = box_frame ? box_frame[ci] : 0;
    chip_window w{0, 0, 0};
    frame_desc fd{nullptr, 0, 0};
    if (f >= 0 && f < n_frames) {
        w = chip_window_of(boxes + 4 * (int64_t)ci, context, min_side, max_side);
        fd = frames[f];
    }
    if (band == 0 && tid == 0 && windows) {
        windows[3 * (int64_t)ci] = w.y0; windows[3 * (int64_t)ci + 1] = w.x0; windows[3 * (int64_t)ci + 2] = w.side;
    }
    const bool meets = w.side > 0 && fd.data && fd.width > 0 && fd.height > 0 && w.x0 < fd.width && w.y0 < fd.height &&
                       w.x0 + w.side > 0 && w.y0 + w.side > 0;
    if (!meets) {                                  // workgroup-uniform
        for (int i = tid; i < out_dw; i += 256) out[i] = 0u;
        return;
    }

    const int kk_cap = chip_kk_cap(S, max_side), rows_cap = chip_rows_cap(S, max_side);
    int* s_bounds = (int*)chip_smem;
    int* s_kk = s_bounds + 2 * S;
    unsigned char* s_h = (unsigned char*)(s_kk + kk_cap);
    unsigned* s_stage = (unsigned*)(s_h + rows_cap * S * 3);
    const resize_axis ax = resize_axis_of(w.side, S);
    const int ksize = ax.ksize;
    if (tid < S) resize_coeff_row(ax, w.side, tid, &s_bounds[2 * tid], &s_bounds[2 * tid + 1], s_kk + tid * ksize);
    __syncthreads();

    // window rows [y_first, y_first + nrows) feed this band
    int y_first = w.side, y_end = 0;
    for (int r = r0; r < r1; ++r) {
        y_first = min(y_first, s_bounds[2 * r]);
        y_end = max(y_end, s_bounds[2 * r] + s_bounds[2 * r + 1]);
    }
    const int nrows = min(y_end - y_first, rows_cap);
    const int cx0 = max(w.x0, 0), cx1 = min(w.x0 + w.side, fd.width);        // the window's columns inside the frame
    const int span_bytes = (cx1 - cx0) * 3;
    const int rs_dw = (w.side * 3 + 6) / 4 + 1;                              // staged row stride >= (3 + span_bytes + 3) / 4
    const int G = CHIP_STAGE_DWORDS / rs_dw;                                 // rows staged at a time, >= 3

    for (int g0 = 0; g0 < nrows; g0 += G) {
        const int ng = min(G, nrows - g0);
        for (int i = tid; i < ng * rs_dw; i += 256) {
            const int rl = i / rs_dw, d = i - rl * rs_dw;
            const int fy = w.y0 + y_first + g0 + rl;
            if (fy >= 0 && fy < fd.height) {
                // aligned dwords covering [p, p + span_bytes): each holds at least one byte of the frame
                const unsigned char* p = fd.data + ((int64_t)fy * fd.width + cx0) * 3;
                const unsigned* a = (const unsigned*)((uintptr_t)p & ~(uintptr_t)3);
                const int ndw = ((int)((uintptr_t)p & 3) + span_bytes + 3) >> 2;
                if (d < ndw) s_stage[i] = a[d];
            }
        }
        __syncthreads();
        for (int i = tid; i < ng * S; i += 256) {
            const int rl = i / S, xx = i - rl * S;
            const int fy = w.y0 + y_first + g0 + rl;
            int a0 = RESAMPLE_ACC0, a1 = a0, a2 = a0;
            if (fy >= 0 && fy < fd.height) {       // a row outside the frame is a row of zeros
                const int shift = (int)((uintptr_t)(fd.data + ((int64_t)fy * fd.width + cx0) * 3) & 3);
                const unsigned char* sb = (const unsigned char*)(s_stage + rl * rs_dw) + shift;
                const int fx0 = w.x0 + s_bounds[2 * xx], n = s_bounds[2 * xx + 1];
                const int* k = s_kk + xx * ksize;
                for (int t = 0; t < n; ++t) {
                    const int fx = fx0 + t;
                    if (fx >= cx0 && fx < cx1) {   // a column outside the frame is a zero pixel
                        const unsigned char* src = sb + (fx - cx0) * 3;
                        const int c = k[t];
                        a0 += src[0] * c; a1 += src[1] * c; a2 += src[2] * c;
                    }
                }
            }
            unsigned char* dst = s_h + ((g0 + rl) * S + xx) * 3;
            dst[0] = resample_clip8(a0); dst[1] = resample_clip8(a1); dst[2] = resample_clip8(a2);
        }
        __syncthreads();
    }

    // vertical pass: one aligned output dword (4 byte columns) per thread and step
    const unsigned* hrows = (const unsigned*)s_h;
    for (int i = tid; i < out_dw; i += 256) {
        const int rr = i / row_dw, j = i - rr * row_dw;
        const int r = r0 + rr;
        const int n = s_bounds[2 * r + 1];
        const int* k = s_kk + r * ksize;
        const unsigned* hp = hrows + (s_bounds[2 * r] - y_first) * row_dw + j;
        int acc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = RESAMPLE_ACC0;
        for (int y = 0; y < n; ++y) {
            const unsigned v = hp[y * row_dw];
            const int c = k[y];
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] += (int)((v >> (8 * b)) & 255u) * c;
        }
        out[i] = resample_pack4(acc);
    }
}

}  // namespace wm
