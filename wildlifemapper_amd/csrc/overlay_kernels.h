// Survey overlays (wm_draw_boxes_u8, wm_plot_image_u8, wm_box_outline_rect): the picture a reviewer opens first -- a frame
// or a tile with every detection outlined in its class colour (the reference's plot_points, visualize_prediction.py:118-133).
//   * box_outline_rect_of: the outline rule's first step, box -> inclusive integer rectangle (l, t, r, b) or "skipped"; host
//     and device.
//   * draw_boxes_kernel: outlines of n boxes onto n_frames (H,W,3) uint8 frames, in place, in one launch, with the result
//     of drawing them one after another in index order (painter's order) and exactly one store per written pixel.
//   * plot_minmax_kernel, plot_map_kernel: the reference's tile preparation, (B,3,H,W) fp32 -> (B,H,W,3) uint8 with
//     channels 0 and 2 swapped and each image stretched to 0..255 by its own minimum and range.
//
// The outline rule.  Each coordinate of a box (x0, y0, x1, y1) is clamped to [-2^30, 2^30] and truncated toward zero, as
// the reference's int(box[k]) does: (l, t, r, b), r and b inclusive.  A box is skipped -- it draws nothing -- if a
// coordinate is not finite, if r < l or b < t, if its frame index is outside [0, n_frames) or its label outside [0, P).
// The outline of a box is every pixel (x, y) with l <= x <= r, t <= y <= b inside the frame with
//   x - l < width  or  r - x < width  or  y - t < width  or  b - y < width:
// the border grows inward, clipped to the frame, and nothing outside the box is touched.  An outline pixel gets the three
// bytes of palette[label], no blending.  Where r - l + 1 and b - t + 1 both exceed `width` this is the pixel set of
// PIL.ImageDraw.rectangle([l, t, r, b], outline=c, width=width); on smaller sides Pillow paints outside the box and
// this rule does not.
#pragma once

#include "survey_kernels.h"

namespace wm {

constexpr int DRAW_MAX_WIDTH = 16;      // WM_DRAW_MAX_WIDTH
constexpr int DRAW_MAX_PALETTE = 256;   // WM_DRAW_MAX_PALETTE
constexpr int DRAW_SLICES = 8;          // gridDim.y: workgroups that share one box's outline pixels
constexpr int PLOT_MAX_PARTS = 128;     // partial (min, max) pairs per image: WM_PLOT_SCRATCH_BYTES = PLOT_MAX_PARTS * 8

struct outline_rect { int l, t, r, b; bool drawn; };

// Clamp to [-2^30, 2^30], truncate toward zero.  Not drawn: a non-finite coordinate, r < l or b < t.
__host__ __device__ inline outline_rect box_outline_rect_of(const float* box) {
    const float lim = 1073741824.f;
    int v[4];
    for (int k = 0; k < 4; ++k) {
        float c = box[k];
        if (!__builtin_isfinite(c)) return outline_rect{0, 0, 0, 0, false};
        c = c > -lim ? c : -lim;
        c = c < lim ? c : lim;
        v[k] = (int)c;
    }
    return outline_rect{v[0], v[1], v[2], v[3], v[2] >= v[0] && v[3] >= v[1]};
}

// (x, y) inside the rectangle and within `width` pixels of one of its sides.  The differences are taken unsigned: with
// l <= x the true value of x - l is below 2^32 whatever the clamp allows.
__device__ inline bool on_outline(int x, int y, int l, int t, int r, int b, unsigned width) {
    if (x < l || x > r || y < t || y > b) return false;
    return (unsigned)x - (unsigned)l < width || (unsigned)r - (unsigned)x < width || (unsigned)y - (unsigned)t < width ||
           (unsigned)b - (unsigned)y < width;
}

// frames [n_frames], boxes [n][4] xyxy fp32, labels [n], box_frame [n] or NULL (all frame 0), palette [P][3] u8.
// Grid (n, DRAW_SLICES), 256 threads.  Workgroup (i, s) owns box i.  Its outline is four disjoint strips clipped to the
// frame -- the top `width` rows, the bottom rows below them, and between the two the left and the right `width` columns --
// whose pixels are numbered 0 .. total; slice s takes the pixels p with (p / 256) % DRAW_SLICES == s, one per thread and
// step, so every outline pixel of box i belongs to exactly one thread of the launch.  That thread stores the colour
// unless a LATER box (j > i) of the same frame that is itself drawn has the pixel on its outline: then box j's own thread
// stores there, or a still later one's.  Every written pixel is therefore stored exactly once, by the last box that
// covers it, which is what drawing the boxes in index order leaves.  The later boxes go through LDS 256 at a time; only
// those that are drawn, lie in this frame and meet box i's clipped rectangle are kept (the order in which they are kept
// does not matter: a pixel asks whether ANY of them covers it).
// No address is formed from a skipped box, and none outside its frame from a drawn one.
__global__ __launch_bounds__(256) void draw_boxes_kernel(const frame_desc* __restrict__ frames, int n_frames, const float* __restrict__ boxes,
                                                         const int* __restrict__ labels, const int* __restrict__ box_frame, int n,
                                                         const unsigned char* __restrict__ palette, int P, int width) {
    __shared__ int4 s_rect[256];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const int f = box_frame ? box_frame[i] : 0;
    const int lab = labels[i];
    if (f < 0 || f >= n_frames || lab < 0 || lab >= P) return;                 // workgroup-uniform, as every return below
    const outline_rect me = box_outline_rect_of(boxes + 4 * (int64_t)i);
    if (!me.drawn) return;
    const frame_desc fd = frames[f];
    if (!fd.data || fd.width <= 0 || fd.height <= 0) return;
    const int cl = max(me.l, 0), cr = min(me.r, fd.width - 1), ct = max(me.t, 0), cb = min(me.b, fd.height - 1);
    if (cl > cr || ct > cb) return;                                            // wholly off the frame

    // the four strips, in box coordinates (|l|, |t|, |r|, |b| <= 2^30 and width <= 16: no overflow), then clipped
    const int top1 = min(me.t + width - 1, me.b);                              // top strip: rows t .. top1
    const int bot0 = max(me.b - width + 1, top1 + 1);                          // bottom strip: rows bot0 .. b
    const int lef1 = min(me.l + width - 1, me.r);                              // left strip: columns l .. lef1, rows top1 + 1 .. bot0 - 1
    const int rig0 = max(me.r - width + 1, lef1 + 1);                          // right strip: columns rig0 .. r, the same rows
    const int64_t cw = (int64_t)cr - cl + 1;
    const int ta = ct, tb = min(top1, cb);                                     // clipped rows of each strip (empty where a > b)
    const int ba = max(bot0, ct), bb = cb;
    const int ma = max(top1 + 1, ct), mb = min(bot0 - 1, cb);
    const int la = cl, lb = min(lef1, cr);
    const int ra = max(rig0, cl), rb = cr;
    const int64_t n_top = tb >= ta ? ((int64_t)tb - ta + 1) * cw : 0;
    const int64_t n_bot = bb >= ba ? ((int64_t)bb - ba + 1) * cw : 0;
    const int64_t mrows = mb >= ma ? (int64_t)mb - ma + 1 : 0;
    const int lw = lb >= la ? lb - la + 1 : 0, rw = rb >= ra ? rb - ra + 1 : 0;
    const int64_t n_left = mrows * lw, n_right = mrows * rw;
    const int64_t total = n_top + n_bot + n_left + n_right;

    const unsigned c0 = palette[3 * lab], c1 = palette[3 * lab + 1], c2 = palette[3 * lab + 2];
    for (int64_t base = (int64_t)blockIdx.y * 256; base < total; base += (int64_t)DRAW_SLICES * 256) {
        int64_t p = base + tid;
        bool alive = p < total;
        int x = 0, y = 0;
        if (alive) {
            if (p < n_top) { y = ta + (int)(p / cw); x = cl + (int)(p % cw); }
            else if ((p -= n_top) < n_bot) { y = ba + (int)(p / cw); x = cl + (int)(p % cw); }
            else if ((p -= n_bot) < n_left) { y = ma + (int)(p / lw); x = la + (int)(p % lw); }
            else { p -= n_left; y = ma + (int)(p / rw); x = ra + (int)(p % rw); }
        }
        for (int j0 = i + 1; j0 < n; j0 += 256) {
            __syncthreads();                                                   // the previous chunk has been read
            if (tid == 0) s_count = 0;
            __syncthreads();
            const int j = j0 + tid;
            if (j < n) {
                const int fj = box_frame ? box_frame[j] : 0;
                const int lj = labels[j];
                if (fj == f && lj >= 0 && lj < P) {
                    const outline_rect o = box_outline_rect_of(boxes + 4 * (int64_t)j);
                    if (o.drawn && o.l <= cr && o.r >= cl && o.t <= cb && o.b >= ct)
                        s_rect[atomicAdd(&s_count, 1)] = make_int4(o.l, o.t, o.r, o.b);
                }
            }
            __syncthreads();
            const int cnt = s_count;
            for (int k = 0; alive && k < cnt; ++k) {
                const int4 o = s_rect[k];
                if (on_outline(x, y, o.x, o.y, o.z, o.w, (unsigned)width)) alive = false;
            }
        }
        if (alive) {
            unsigned char* dst = const_cast<unsigned char*>(fd.data) + ((int64_t)y * fd.width + x) * 3;
            dst[0] = (unsigned char)c0; dst[1] = (unsigned char)c1; dst[2] = (unsigned char)c2;
        }
    }
}

// ---- the reference's tile preparation ----
// np.transpose(image, (1, 2, 0)); cv2.cvtColor(BGR2RGB) (channels 0 and 2 swap); image -= image.min(); image /= image.max();
// np.int32(image * 255) -- every operation a correctly rounded fp32 operation of its own.  The subtraction is monotonic, so
// the maximum of the shifted image is fl(max - min): one (min, max) pair per image is all the map needs.

__device__ inline void minmax_block(float& mn, float& mx, float* s_mn, float* s_mx) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if ((tid & 63) == 0) { s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; }
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
}

// Stage 1.  in [B][3 * hw] fp32 -> part [B][parts][2] = (min, max) of the elements workgroup (part, image) strides over.
// Grid (parts, B).  vec: 3 * hw % 4 == 0 and `in` 16-byte aligned -- float4 loads.
__global__ __launch_bounds__(256) void plot_minmax_kernel(const float* __restrict__ in, int64_t elems, float* __restrict__ part, int vec) {
    __shared__ float s_mn[4], s_mx[4];
    const float* src = in + (int64_t)blockIdx.y * elems;
    float mn = INFINITY, mx = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const float4* s4 = (const float4*)src;
        for (int64_t q = first; q < elems / 4; q += stride) {
            const float4 v = s4[q];
            mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
            mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
        }
    } else {
        for (int64_t q = first; q < elems; q += stride) {
            const float v = src[q];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    minmax_block(mn, mx, s_mn, s_mx);
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = mn; o[1] = mx;
    }
}

__device__ inline unsigned plot_value(float v, float mn, float range) {
#pragma clang fp contract(off)
    const float a = v - mn;
    const float q = a / range;                 // correctly rounded: the library is built without fast-math
    const float p = q * 255.0f;
    return (unsigned)(int)p & 255u;            // 0..255 by construction for finite input
}

// Stage 2.  Every workgroup folds its image's `parts` pairs (the same values in the same order: every workgroup of an
// image gets the same pair), then maps.  Grid (blocks, B); a thread takes four consecutive pixels of the flattened H * W
// plane per step: out[(p)*3 + c] = f(in[2 - c][p]).  vec: hw % 4 == 0, `in` 16-byte and `out` 4-byte aligned -- three float4
// loads and three dword stores per step.  A constant image (range 0; the reference divides by zero there) gives zeros.
__global__ __launch_bounds__(256) void plot_map_kernel(const float* __restrict__ in, int64_t hw, const float* __restrict__ part, int parts,
                                                       unsigned char* __restrict__ out, int vec) {
#pragma clang fp contract(off)
    __shared__ float s_mn[4], s_mx[4];
    const int tid = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    const float* pp = part + (int64_t)blockIdx.y * parts * 2;
    if (tid < parts) { mn = pp[2 * tid]; mx = pp[2 * tid + 1]; }           // parts <= PLOT_MAX_PARTS <= 256
    minmax_block(mn, mx, s_mn, s_mx);
    const float range = mx - mn;
    const bool flat = !(range > 0.f);
    const float* src = in + (int64_t)blockIdx.y * 3 * hw;
    unsigned char* dst = out + (int64_t)blockIdx.y * 3 * hw;
    const int64_t groups = (hw + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * 256 + tid; g < groups; g += (int64_t)gridDim.x * 256) {
        if (vec) {
            const float4 c0 = ((const float4*)src)[g], c1 = ((const float4*)(src + hw))[g], c2 = ((const float4*)(src + 2 * hw))[g];
            const float r[4] = {c2.x, c2.y, c2.z, c2.w}, gg[4] = {c1.x, c1.y, c1.z, c1.w}, b[4] = {c0.x, c0.y, c0.z, c0.w};
            unsigned by[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                by[3 * k] = flat ? 0u : plot_value(r[k], mn, range);
                by[3 * k + 1] = flat ? 0u : plot_value(gg[k], mn, range);
                by[3 * k + 2] = flat ? 0u : plot_value(b[k], mn, range);
            }
            unsigned* o = (unsigned*)dst + 3 * g;
#pragma unroll
            for (int d = 0; d < 3; ++d) o[d] = by[4 * d] | (by[4 * d + 1] << 8) | (by[4 * d + 2] << 16) | (by[4 * d + 3] << 24);
        } else {
            const int64_t p1 = 4 * g + 4 < hw ? 4 * g + 4 : hw;
            for (int64_t p = 4 * g; p < p1; ++p)
                for (int c = 0; c < 3; ++c) dst[3 * p + c] = flat ? 0 : (unsigned char)plot_value(src[(2 - c) * hw + p], mn, range);
        }
    }
}

}  // namespace wm
