// Launcher of the validation losses (criterion_kernels.h): argument checks that need no GPU, then cost -> match -> sums on
// the caller's stream.  Weightless like wm_postprocess_nms: nothing is allocated, the scratch is the caller's.
#pragma once
#include "criterion_kernels.h"
#include "host_core.h"

namespace {

// scratch: the cost matrices [51 * total_targets] fp32 (padded to 16 bytes), then the per-image partial sums [batch][CR_SUMS] double
int64_t criterion_cost_bytes(int total_targets) { return ((int64_t)CR_NQ * total_targets * 4 + 15) / 16 * 16; }

int64_t criterion_scratch_bytes(int batch, int total_targets) {
    if (batch <= 0 || total_targets < 0 || (int64_t)CR_NQ * total_targets > INT32_MAX)
        return fail("wm_criterion_scratch_bytes: batch %d, total_targets %d", batch, total_targets);
    return criterion_cost_bytes(total_targets) + (int64_t)batch * CR_SUMS * 8;
}

int launch_criterion(const float* logits_dev, const float* boxes_dev, const float* tgt_boxes_dev, const int32_t* tgt_labels_dev,
                     const int32_t* tgt_offsets, int batch, float w_class, float w_bbox, float w_giou, float eos_coef, void* scratch_dev,
                     int64_t scratch_bytes, int32_t* match_dev, double* sums_dev, int32_t* status_dev, float* cost_dev, double* dual_u_dev,
                     double* dual_v_dev, hipStream_t s) {
    if (!logits_dev || !boxes_dev || !tgt_offsets || !scratch_dev || !match_dev || !sums_dev || !status_dev) return fail("wm_criterion: null buffer");
    if (batch <= 0) return fail("wm_criterion: batch %d", batch);
    if (tgt_offsets[0] != 0) return fail("wm_criterion: tgt_offsets[0] = %d, not 0", tgt_offsets[0]);
    for (int b = 0; b < batch; ++b) {
        const int64_t t = (int64_t)tgt_offsets[b + 1] - tgt_offsets[b];
        if (t < 0) return fail("wm_criterion: tgt_offsets decreasing at image %d (%d -> %d)", b, tgt_offsets[b], tgt_offsets[b + 1]);
        if (t > CR_MAX_TARGETS) return fail("wm_criterion: image %d has %lld targets, the limit is %d (WM_CRITERION_MAX_TARGETS)", b, (long long)t, CR_MAX_TARGETS);
    }
    const int total = tgt_offsets[batch];
    if (total > 0 && (!tgt_boxes_dev || !tgt_labels_dev)) return fail("wm_criterion: null buffer");
    for (float v : {w_class, w_bbox, w_giou, eos_coef})
        if (!std::isfinite(v)) return fail("wm_criterion: weights (%g, %g, %g) and eos_coef %g must be finite", (double)w_class, (double)w_bbox, (double)w_giou, (double)eos_coef);
    const int64_t need = criterion_scratch_bytes(batch, total);
    if (need < 0) return -1;
    if (scratch_bytes < need) return fail("wm_criterion: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    if ((uintptr_t)scratch_dev % 16 || (uintptr_t)boxes_dev % 16 || (uintptr_t)tgt_boxes_dev % 16) return fail("wm_criterion: scratch and boxes must be 16-byte aligned");
    float* cost = (float*)scratch_dev;
    double* partial = (double*)((char*)scratch_dev + criterion_cost_bytes(total));
    HIP_TRY(hipMemsetAsync(status_dev, 0, (size_t)batch * 4, s));
    for (int b0 = 0; b0 < batch; b0 += CR_MAX_IMAGES) {
        const int nb = std::min(CR_MAX_IMAGES, batch - b0);
        cr_offsets offs;
        int t_max = 0;
        for (int b = 0; b <= nb; ++b) offs.tgt[b] = tgt_offsets[b0 + b];
        for (int b = 0; b < nb; ++b) t_max = std::max(t_max, offs.tgt[b + 1] - offs.tgt[b]);
        if (t_max > 0) {
            const int by = std::min(CR_COST_MAX_BLOCKS_Y, (CR_NQ * t_max + CR_COST_THREADS - 1) / CR_COST_THREADS);
            hipLaunchKernelGGL(criterion_cost_kernel, dim3(nb, by), dim3(CR_COST_THREADS), 0, s, logits_dev, boxes_dev, tgt_boxes_dev,
                               (const int*)tgt_labels_dev, offs, b0, w_class, w_bbox, w_giou, cost, (int*)status_dev);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(criterion_match_kernel, dim3(nb), dim3(64), 0, s, logits_dev, boxes_dev, tgt_boxes_dev, (const int*)tgt_labels_dev,
                           offs, b0, eos_coef, (const float*)cost, (int*)status_dev, (int*)match_dev, partial, dual_u_dev, dual_v_dev);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(criterion_sums_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, (const int*)status_dev, batch, sums_dev);
    HIP_TRY(hipGetLastError());
    if (cost_dev && total > 0) HIP_TRY(hipMemcpyAsync(cost_dev, cost, (size_t)CR_NQ * total * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // namespace
