// Validation losses of `evaluate` (contract row A23): the Hungarian match of the 51 queries to an image's ground truth
// (segment_anything/modeling/matcher.py:33-81) and the forward DETR losses on it (build_sam.py:93-147), no gradients.
// The reference copies the cost matrix to the host and calls scipy's linear_sum_assignment once per image; here three
// launches on the caller's stream (cost and match once per 64 images), nothing synchronous:
//   * criterion_cost_kernel: per image the fp32 cost matrix C[q][t] = w_bbox L1 - w_class softmax(logits_q)[label_t]
//     - w_giou GIoU, in the reference's operation order (matcher.py:57-76, utils/box_ops.py:9-61), into scratch (51 T 4
//     bytes per image: stays in L2).  An image whose matrix holds a non-finite value, or a label outside 0..6, gets bit 0
//     of its status word (scipy raises there).
//   * criterion_match_kernel: ONE WAVE per image.  Rectangular assignment by shortest augmenting paths with row and
//     column duals, the algorithm of scipy's linear_sum_assignment, in double on the fp32 costs as scipy runs it.  Rows
//     are the smaller side (the matrix is read transposed when T < 51), columns are spread over the 64 lanes, the
//     per-step minimum is a wave reduction with ties to the lowest column index.  Every loop bound is structural:
//     min(51, T) augmentations of at most columns + 1 steps; an image that would need more gets status bit 1 and no
//     matches (finite costs cannot).  A flagged image is skipped: all matches -1.  The same wave then forms the image's
//     loss terms (fp32, as the reference's) and adds them in double in a fixed order: run-to-run bit-identical.
//   * criterion_sums_kernel: the images' partial sums added in image order; NaN in every sum if any status is set.
// Workgroups never communicate inside a launch; the only atomic is the integer OR on the status word.
#pragma once

#include "wm_common.h"

namespace wm {

constexpr int CR_NQ = WM_NUM_QUERIES, CR_NL = WM_NUM_LOGITS, CR_NO_OBJECT = WM_NUM_LOGITS - 1;
constexpr int CR_MAX_TARGETS = WM_CRITERION_MAX_TARGETS;      // per image: the column state of the solver lives in LDS
constexpr int CR_MAX_IMAGES = 64;                             // images per launch (offsets travel as a kernel argument)
constexpr int CR_SUMS = WM_CRITERION_SUMS;
constexpr int CR_COST_THREADS = 256, CR_COST_MAX_BLOCKS_Y = 32;
static_assert(CR_NQ <= 64, "one lane per query");

struct cr_offsets {
    int tgt[CR_MAX_IMAGES + 1];        // absolute target offsets of this launch's images
};

__device__ __forceinline__ bool cr_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// utils/box_ops.py:9-13
__device__ __forceinline__ float4 cr_xyxy(float4 b) {
#pragma clang fp contract(off)
    return float4{b.x - 0.5f * b.z, b.y - 0.5f * b.w, b.x + 0.5f * b.z, b.y + 0.5f * b.w};
}

// utils/box_ops.py:24-61 for one pair of xyxy boxes
__device__ __forceinline__ float cr_giou(float4 a, float4 b) {
#pragma clang fp contract(off)
    const float area1 = (a.z - a.x) * (a.w - a.y), area2 = (b.z - b.x) * (b.w - b.y);
    const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f), ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = iw * ih;
    const float uni = area1 + area2 - inter;
    const float iou = inter / uni;
    const float ew = fmaxf(fmaxf(a.z, b.z) - fminf(a.x, b.x), 0.f), eh = fmaxf(fmaxf(a.w, b.w) - fminf(a.y, b.y), 0.f);
    const float area = ew * eh;
    return iou - (area - uni) / area;
}

__device__ __forceinline__ float cr_l1(float4 a, float4 b) {
#pragma clang fp contract(off)
    return fabsf(a.x - b.x) + fabsf(a.y - b.y) + fabsf(a.z - b.z) + fabsf(a.w - b.w);
}

// grid (images of this launch, blocks over the image's 51 T entries); cost holds image b's matrix at 51 * offset(b), [q][t]
__global__ __launch_bounds__(CR_COST_THREADS) void criterion_cost_kernel(
        const float* __restrict__ logits, const float* __restrict__ boxes, const float* __restrict__ tgt_boxes,
        const int* __restrict__ tgt_labels, cr_offsets offs, int image_base, float w_class, float w_bbox, float w_giou,
        float* __restrict__ cost, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ float s_prob[CR_NQ][CR_NL];
    __shared__ float4 s_box[CR_NQ];
    const int tid = threadIdx.x, img = image_base + blockIdx.x;
    const int t0 = offs.tgt[blockIdx.x], T = offs.tgt[blockIdx.x + 1] - t0;
    const int n = CR_NQ * T;
    if ((int)blockIdx.y * CR_COST_THREADS >= n) return;          // block-uniform (also T == 0)
    if (tid < CR_NQ) {
        const float* x = logits + ((size_t)img * CR_NQ + tid) * CR_NL;
        float v[CR_NL], mx = x[0];
#pragma unroll
        for (int c = 0; c < CR_NL; ++c) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CR_NL; ++c) { v[c] = expf(v[c] - mx); sum += v[c]; }
#pragma unroll
        for (int c = 0; c < CR_NL; ++c) s_prob[tid][c] = v[c] / sum;
        s_box[tid] = *(const float4*)(boxes + ((size_t)img * CR_NQ + tid) * 4);
    }
    __syncthreads();
    float* c_img = cost + (size_t)CR_NQ * t0;
    bool bad = false;
    for (int e = blockIdx.y * CR_COST_THREADS + tid; e < n; e += gridDim.y * CR_COST_THREADS) {
        const int q = e / T, t = e - q * T;
        const float4 tb = *(const float4*)(tgt_boxes + (size_t)(t0 + t) * 4);
        const int lab = tgt_labels[t0 + t];
        const bool lab_ok = lab >= 0 && lab < CR_NO_OBJECT;          // 7 is no-object, never a target's class
        const float4 pb = s_box[q];
        const float cost_class = -s_prob[q][lab_ok ? lab : 0];
        const float cost_bbox = cr_l1(pb, tb);
        const float cost_giou = -cr_giou(cr_xyxy(pb), cr_xyxy(tb));
        const float c = w_bbox * cost_bbox + w_class * cost_class + w_giou * cost_giou;          // matcher.py:76
        c_img[e] = c;
        bad |= !lab_ok || !cr_finite(c);
    }
    if (bad) atomicOr(&status[img], WM_CRITERION_NONFINITE);
}

__device__ __forceinline__ double cr_wave_sum(double v) {       // fixed butterfly: the same bits on every lane, every run
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// one wave per image; partial[img][CR_SUMS], dual_u [images][51] / dual_v [targets] may be NULL
__global__ __launch_bounds__(64) void criterion_match_kernel(
        const float* __restrict__ logits, const float* __restrict__ boxes, const float* __restrict__ tgt_boxes,
        const int* __restrict__ tgt_labels, cr_offsets offs, int image_base, float eos_coef, const float* __restrict__ cost,
        int* __restrict__ status, int* __restrict__ match, double* __restrict__ partial, double* __restrict__ dual_u,
        double* __restrict__ dual_v) {
#pragma clang fp contract(off)
    __shared__ double s_sp[CR_MAX_TARGETS], s_v[CR_MAX_TARGETS], s_u[CR_NQ];      // shortest path cost and dual per column, dual per row
    __shared__ int s_path[CR_MAX_TARGETS], s_row4col[CR_MAX_TARGETS], s_col4row[CR_NQ];
    __shared__ unsigned char s_sc[CR_MAX_TARGETS], s_sr[CR_NQ];                   // column / row reached in this augmentation
    const int lane = threadIdx.x, img = image_base + blockIdx.x;
    const int t0 = offs.tgt[blockIdx.x], T = offs.tgt[blockIdx.x + 1] - t0;
    const bool transposed = T < CR_NQ;                       // rows = targets, columns = queries
    const int nr = transposed ? T : CR_NQ, nc = transposed ? CR_NQ : T;
    const int rs = transposed ? 1 : T, cs = transposed ? T : 1;
    const float* c_img = cost + (size_t)CR_NQ * t0;
    const double inf = __builtin_inf();
    const bool skip = T == 0 || status[img] != 0;

    for (int j = lane; j < nc; j += 64) { s_v[j] = 0.0; s_row4col[j] = -1; }
    if (lane < CR_NQ) { s_u[lane] = 0.0; s_col4row[lane] = -1; }
    __syncthreads();

    bool failed = false;                                     // wave-uniform
    for (int cur = 0; cur < nr && !skip && !failed; ++cur) {
        for (int j = lane; j < nc; j += 64) { s_sp[j] = inf; s_sc[j] = 0; }
        if (lane < CR_NQ) s_sr[lane] = 0;
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= nc && sink < 0; ++step) {
            if (lane == 0) s_sr[i] = 1;
            const double ui = s_u[i];
            const float* c_row = c_img + (size_t)i * rs;
            double best = inf;
            int bj = INT32_MAX;
            for (int j = lane; j < nc; j += 64) {
                if (s_sc[j]) continue;
                const double r = min_val + (double)c_row[(size_t)j * cs] - ui - s_v[j];
                double sp = s_sp[j];
                if (r < sp) { sp = r; s_sp[j] = r; s_path[j] = i; }
                if (sp < best) { best = sp; bj = j; }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ob = __shfl_xor(best, m, 64);
                const int oj = __shfl_xor(bj, m, 64);
                if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            if (bj == INT32_MAX) break;                      // no column left with a finite path: not with finite costs
            min_val = best;
            const int r4 = s_row4col[bj];
            if (lane == 0) s_sc[bj] = 1;
            if (r4 < 0) sink = bj; else i = r4;
            __syncthreads();
        }
        if (sink < 0) { failed = true; break; }
        // duals, then the augmentation along the path (lane 0: a chain of at most nr links)
        if (lane < nr && s_sr[lane]) s_u[lane] += lane == cur ? min_val : min_val - s_sp[s_col4row[lane]];
        for (int j = lane; j < nc; j += 64)
            if (s_sc[j]) s_v[j] -= min_val - s_sp[j];
        __syncthreads();
        if (lane == 0) {
            int j = sink;
            for (int k = 0; k < nr; ++k) {
                const int pi = s_path[j];
                s_row4col[j] = pi;
                const int pj = s_col4row[pi];
                s_col4row[pi] = j;
                j = pj;
                if (pi == cur || j < 0) break;
            }
        }
        __syncthreads();
    }
    if (failed && lane == 0) status[img] |= WM_CRITERION_UNSOLVED;
    const bool solved = !skip && !failed;

    int m = -1;                                              // lane q: the target matched to query q
    if (lane < CR_NQ && solved) m = transposed ? s_row4col[lane] : s_col4row[lane];
    if (lane < CR_NQ) {
        match[(size_t)img * CR_NQ + lane] = m;
        if (dual_u) dual_u[(size_t)img * CR_NQ + lane] = solved ? (transposed ? s_v[lane] : s_u[lane]) : 0.0;
    }
    if (dual_v)
        for (int t = lane; t < T; t += 64) dual_v[t0 + t] = solved ? (transposed ? s_u[t] : s_v[t]) : 0.0;

    // loss terms of query `lane` (build_sam.py:93-147)
    double wnll = 0.0, w = 0.0, l1 = 0.0, gl = 0.0, matched = 0.0, correct = 0.0, nonempty = 0.0;
    if (lane < CR_NQ) {
        const float* x = logits + ((size_t)img * CR_NQ + lane) * CR_NL;
        float v[CR_NL], mx = x[0];
#pragma unroll
        for (int c = 0; c < CR_NL; ++c) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
        const int cls = m >= 0 ? tgt_labels[t0 + m] : CR_NO_OBJECT;
        float sum = 0.f, x_cls = 0.f, top7 = v[0];
        int am7 = 0;                                         // first maximum, as torch.argmax / topk
#pragma unroll
        for (int c = 0; c < CR_NL; ++c) {
            sum += expf(v[c] - mx);
            if (c == cls) x_cls = v[c];
            if (c < CR_NO_OBJECT && v[c] > top7) { top7 = v[c]; am7 = c; }
        }
        const int am8 = v[CR_NO_OBJECT] > top7 ? CR_NO_OBJECT : am7;
        const float lse = logf(sum);
        const float wc = cls == CR_NO_OBJECT ? eos_coef : 1.f;
        wnll = (double)(wc * -(x_cls - mx - lse));           // F.cross_entropy(..., empty_weight), :106
        w = (double)wc;
        nonempty = am8 != CR_NO_OBJECT ? 1.0 : 0.0;          // :123
        if (m >= 0) {
            const float4 pb = *(const float4*)(boxes + ((size_t)img * CR_NQ + lane) * 4);
            const float4 tb = *(const float4*)(tgt_boxes + (size_t)(t0 + m) * 4);
            l1 = (double)cr_l1(pb, tb);                                                 // :138
            gl = (double)(1.f - cr_giou(cr_xyxy(pb), cr_xyxy(tb)));                     // :143
            matched = 1.0;
            correct = am7 == cls ? 1.0 : 0.0;                                           // :111
        }
    }
    wnll = cr_wave_sum(wnll); w = cr_wave_sum(w); l1 = cr_wave_sum(l1); gl = cr_wave_sum(gl);
    matched = cr_wave_sum(matched); correct = cr_wave_sum(correct); nonempty = cr_wave_sum(nonempty);
    if (lane == 0) {
        double* p = partial + (size_t)img * CR_SUMS;
        p[0] = wnll; p[1] = w; p[2] = l1; p[3] = gl; p[4] = matched; p[5] = correct;
        p[6] = fabs(nonempty - (double)T);                                              // :124
        p[7] = 0.0;
    }
}

// one wave: lane k adds sum k of the images in image order
__global__ __launch_bounds__(64) void criterion_sums_kernel(const double* __restrict__ partial, const int* __restrict__ status,
                                                            int batch, double* __restrict__ sums) {
    const int k = threadIdx.x;
    if (k >= CR_SUMS) return;
    double acc = 0.0;
    int st = 0;
    for (int b = 0; b < batch; ++b) { acc += partial[(size_t)b * CR_SUMS + k]; st |= status[b]; }
    sums[k] = st ? __builtin_nan("") : acc;
}

}  // namespace wm
