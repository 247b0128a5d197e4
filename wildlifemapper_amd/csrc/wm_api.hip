// C ABI of the MI355X WildlifeMapper inference path: the extern "C" entry points, in the order of include/wm_hip.h.
// See include/wm_hip.h for the contract.  No torch types, no CPU fallback.  The host-side engine lives in the host_*.h
// headers of this directory (one translation unit).
#include "host_core.h"         // fail / HIP_TRY, wm_handle, the profiled launch Bracket, the instance pickers
#if WM_DEV_TIMELINE
#include "host_dev_timeline.h" // dev build only (tools/build_dev.sh): in-kernel timeline dumps behind WM_DEV_HOOK
#endif
#include "host_gemm.h"
#include "host_norm.h"
#include "host_attn.h"
#include "host_weights.h"
#include "host_encoder.h"
#include "host_decoder.h"
#include "host_frontend.h"
#include "host_survey.h"
#include "host_criterion.h"

extern "C" const char* wm_last_error(void) { return g_err; }
extern "C" int wm_abi_version(void) { return WM_ABI_VERSION; }

// ---- lifetime ----
extern "C" int wm_create(const wm_config* cfg, int device, wm_handle** out) {
    if (!cfg || !out) return fail("wm_create: null argument");
    if (cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->embed_dim % cfg->num_heads) return fail("wm_create: bad dims");
    if (cfg->depth <= 0 || cfg->depth > 64) return fail("wm_create: depth %d out of range", cfg->depth);
    if (cfg->max_batch <= 0) return fail("wm_create: max_batch must be positive");
    if (cfg->embed_dim % 256 || cfg->embed_dim > 1280) return fail("wm_create: embed_dim %d unsupported (multiple of 256, <= 1280)", cfg->embed_dim);
    const int hd = cfg->embed_dim / cfg->num_heads;
    if (hd != 64 && hd != 80) return fail("wm_create: head_dim %d unsupported (64 or 80)", hd);
    if (cfg->precision != WM_PREC_BF16 && cfg->precision != WM_PREC_FP16 && cfg->precision != WM_PREC_FP8) return fail("wm_create: bad precision");
    if (cfg->num_global < 0 || cfg->num_global > WM_MAX_GLOBAL) return fail("wm_create: bad num_global");
    return create_impl(cfg, device, out);
}

extern "C" int wm_destroy(wm_handle* h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    for (void* p : h->allocs) if (p) hipFree(p);
    if (h->tap_buf) hipFree(h->tap_buf);
    if (h->overflow) hipHostFree(h->overflow);
    for (auto& e : h->prof.used) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto& e : h->prof.pool) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    delete h;
    return 0;
}

extern "C" int wm_load_weight(wm_handle* h, const char* name, const float* host_data, const int64_t* shape, int ndim) {
    if (!h || !name || !host_data || !shape) return fail("wm_load_weight: null argument");
    auto it = h->expected.find(name);
    if (it == h->expected.end()) return fail("wm_load_weight: unknown tensor '%s'", name);
    const auto& es = it->second;
    bool ok = (int)es.size() == ndim;
    size_t n = 1;
    for (int i = 0; ok && i < ndim; ++i) { ok = es[i] == shape[i]; n *= (size_t)shape[i]; }
    if (!ok) return fail("wm_load_weight: shape mismatch for '%s'", name);
    HostW w;
    w.shape.assign(shape, shape + ndim);
    w.data.assign(host_data, host_data + n);
    h->staged[name] = std::move(w);
    h->finalized = false;
    return 0;
}

extern "C" int wm_finalize_weights(wm_handle* h) {
    if (!h) return fail("wm_finalize_weights: null handle");
    return finalize_impl(h);
}

// ---- preprocessing ----
extern "C" int wm_preprocess_u8(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, void* stream) {
    if (!img_dev || !out_dev) return fail("wm_preprocess_u8: null buffer");
    if (batch <= 0 || height <= 0 || width <= 0 || height > 1024 || width > 1024)
        return fail("wm_preprocess_u8: batch %d, %dx%d outside 1..1024 (larger images are cropped by the caller, utils/misc.py:57-60)", batch, height, width);
    return launch_simple(nullptr, (hipStream_t)stream, 0.0, preprocess_u8_kernel, dim3(grid_for((int64_t)batch * 1024 * 256)), dim3(256), img_dev, out_dev,
                         batch, height, width);
}

extern "C" int wm_preprocess_u8_resized(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, int size, int max_size,
                                        void* stream) {
    if (!img_dev || !out_dev) return fail("wm_preprocess_u8_resized: null buffer");
    if (batch <= 0 || height <= 0 || width <= 0 || size <= 0) return fail("wm_preprocess_u8_resized: batch %d, %dx%d, size %d", batch, height, width, size);
    int oh, ow;
    resized_size(width, height, size, max_size, &oh, &ow);
    if (oh > 1024 || ow > 1024 || oh <= 0 || ow <= 0)
        return fail("wm_preprocess_u8_resized: %dx%d resizes to %dx%d, outside the 1024x1024 canvas (utils/misc.py:57-60 crops; not built)", height, width, oh, ow);
    return preprocess_resized_impl(img_dev, out_dev, batch, height, width, oh, ow, (hipStream_t)stream);
}

extern "C" int wm_resized_size(int height, int width, int size, int max_size, int* out_h, int* out_w) {
    if (height <= 0 || width <= 0 || size <= 0 || !out_h || !out_w) return fail("wm_resized_size: bad argument");
    resized_size(width, height, size, max_size, out_h, out_w);
    return 0;
}

// host-only (tests): the coefficient tables the resize kernels use for one axis; ksize_out = taps per output, bounds [out][2], kk [out][ksize]
extern "C" int wm_debug_resize_coeffs(int in_size, int out_size, int* bounds_out, int* kk_out, int kk_capacity, int* ksize_out) {
    if (in_size <= 0 || out_size <= 0 || !bounds_out || !kk_out || !ksize_out) return fail("wm_debug_resize_coeffs: bad argument");
    std::vector<int> b, k;
    int ks = 0;
    resize_coeffs(in_size, out_size, b, k, ks);
    if ((size_t)kk_capacity < k.size()) return fail("wm_debug_resize_coeffs: need room for %zu coefficients", k.size());
    memcpy(bounds_out, b.data(), b.size() * 4);
    memcpy(kk_out, k.data(), k.size() * 4);
    *ksize_out = ks;
    return 0;
}

// ---- the path ----
extern "C" int wm_hfc_fft(wm_handle* h, const float* x_dev, float* hfc_dev, int batch, void* stream) {
    if (!h) return fail("wm_hfc_fft: null handle");
    if (batch <= 0 || batch > h->maxB) return fail("wm_hfc_fft: batch %d outside 1..%d", batch, h->maxB);
    if (!x_dev || !hfc_dev) return fail("wm_hfc_fft: null buffer");
    HIP_TRY(hipSetDevice(h->device));
    return fft_impl(h, x_dev, hfc_dev, batch, (hipStream_t)stream);
}

extern "C" int wm_encoder_forward(wm_handle* h, const float* x_dev, const float* hfc_dev, float* out_dev, int batch, void* stream) {
    WM_TRY(check_ready(h, batch, "wm_encoder_forward", true, false));
    if (!x_dev || !hfc_dev || !out_dev) return fail("wm_encoder_forward: null buffer");
    return encoder_impl(h, x_dev, hfc_dev, out_dev, batch, (hipStream_t)stream);
}

extern "C" int wm_decoder_forward(wm_handle* h, const float* emb_dev, float* logits_dev, float* boxes_dev, int batch, void* stream) {
    WM_TRY(check_ready(h, batch, "wm_decoder_forward", false, true));
    if (!emb_dev || !logits_dev || !boxes_dev) return fail("wm_decoder_forward: null buffer");
    hipStream_t s = (hipStream_t)stream;
    // NCHW (B,256,4096) -> token-major (B,4096,256) (transformer.py:83)
    WM_TRY(launch_simple(h, s, batch * 8.4e6, transpose32_kernel, dim3(T / 64, OUTC / 64, batch), dim3(256), emb_dev, h->emb_nhwc, OUTC, T));
    return decoder_impl(h, h->emb_nhwc, logits_dev, boxes_dev, batch, s);
}

extern "C" int wm_postprocess_nms(wm_handle* h, const float* logits_dev, const float* boxes_dev, const float* target_sizes_dev,
                                  float conf_thr, float score_thr, float iou_thr, wm_box_record* records_dev, int batch, void* stream) {
    if (batch <= 0) return fail("wm_postprocess_nms: batch %d", batch);
    if (!logits_dev || !boxes_dev || !target_sizes_dev || !records_dev) return fail("wm_postprocess_nms: null buffer");
    if (h) HIP_TRY(hipSetDevice(h->device));     // weightless kernel: a NULL handle launches on the current device
    return launch_simple(h, (hipStream_t)stream, 0.0, postprocess_nms_kernel, dim3(batch), dim3(64), logits_dev, boxes_dev,
                         target_sizes_dev, conf_thr, score_thr, iou_thr, records_dev);
}

extern "C" int wm_forward(wm_handle* h, const float* x_dev, const float* target_sizes_dev, float* logits_dev, float* boxes_dev,
                          wm_box_record* records_dev, int batch, void* stream) {
    WM_TRY(check_ready(h, batch, "wm_forward", true, true));
    if (!x_dev) return fail("wm_forward: null input");
    return forward_impl(h, x_dev, target_sizes_dev, logits_dev, boxes_dev, records_dev, batch, (hipStream_t)stream);
}

// ---- validation losses ----
extern "C" int64_t wm_criterion_scratch_bytes(int batch, int total_targets) { return criterion_scratch_bytes(batch, total_targets); }

extern "C" int wm_criterion(wm_handle* h, const float* logits_dev, const float* boxes_dev, const float* tgt_boxes_dev,
                            const int32_t* tgt_labels_dev, const int32_t* tgt_offsets, int batch, float w_class, float w_bbox, float w_giou,
                            float eos_coef, void* scratch_dev, int64_t scratch_bytes, int32_t* match_dev, double* sums_dev,
                            int32_t* status_dev, float* cost_dev, double* dual_u_dev, double* dual_v_dev, void* stream) {
    if (h) HIP_TRY(hipSetDevice(h->device));     // weightless kernels: a NULL handle launches on the current device
    return launch_criterion(logits_dev, boxes_dev, tgt_boxes_dev, tgt_labels_dev, tgt_offsets, batch, w_class, w_bbox, w_giou, eos_coef,
                            scratch_dev, scratch_bytes, match_dev, sums_dev, status_dev, cost_dev, dual_u_dev, dual_v_dev, (hipStream_t)stream);
}

// ---- large-frame and survey front end ----
extern "C" int wm_tile_frames_u8(const wm_frame_desc* frames_dev, int n_frames, const int32_t* tiles_dev, float* out_dev, int n_tiles,
                                 void* stream) {
    if (!frames_dev || !tiles_dev || !out_dev) return fail("wm_tile_frames_u8: null buffer");
    if (n_frames <= 0 || n_tiles <= 0) return fail("wm_tile_frames_u8: n_frames %d, n_tiles %d", n_frames, n_tiles);
    return launch_simple(nullptr, (hipStream_t)stream, 0.0, tile_frames_u8_kernel, dim3(grid_for((int64_t)n_tiles * 1024 * 256)), dim3(256),
                         (const frame_desc*)frames_dev, n_frames, (const int*)tiles_dev, out_dev, n_tiles);
}

extern "C" int64_t wm_merge_frames_scratch_bytes(int n_tiles) {
    if (n_tiles <= 0 || (int64_t)n_tiles * WM_NUM_QUERIES > INT32_MAX) return fail("wm_merge_frames_scratch_bytes: n_tiles %d", n_tiles);
    return (int64_t)n_tiles * WM_NUM_QUERIES * MF_SCRATCH_PER_SLOT;
}

extern "C" int wm_merge_frames_nms(const wm_box_record* records_dev, const int32_t* origins_dev, const int32_t* frame_tile_offsets,
                                   int n_frames, float iou_thr, void* scratch_dev, int64_t scratch_bytes, wm_box_record* merged_dev,
                                   wm_box_record* det_dev, int32_t* det_tile_dev, int32_t* det_count_dev, void* stream) {
    return launch_merge_frames<MF_NMS>("wm_merge_frames_nms", "iou_thr", records_dev, origins_dev, frame_tile_offsets, n_frames,
                                       iou_thr, scratch_dev, scratch_bytes, merged_dev, det_dev, det_tile_dev, det_count_dev, nullptr,
                                       nullptr, stream);
}

extern "C" int wm_merge_frames_fuse(const wm_box_record* records_dev, const int32_t* origins_dev, const int32_t* frame_tile_offsets,
                                    int n_frames, float fuse_thr, void* scratch_dev, int64_t scratch_bytes, wm_box_record* merged_dev,
                                    wm_box_record* det_dev, int32_t* det_tile_dev, int32_t* det_count_dev, int32_t* det_members_dev,
                                    int32_t* slot_det_dev, void* stream) {
    return launch_merge_frames<MF_FUSE>("wm_merge_frames_fuse", "fuse_thr", records_dev, origins_dev, frame_tile_offsets, n_frames,
                                        fuse_thr, scratch_dev, scratch_bytes, merged_dev, det_dev, det_tile_dev, det_count_dev,
                                        det_members_dev, slot_det_dev, stream);
}

extern "C" int wm_resample_u8(const uint8_t* in_dev, int height, int width, uint8_t* out_dev, int out_height, int out_width,
                              void* stream) {
    if (!in_dev || !out_dev) return fail("wm_resample_u8: null buffer");
    for (int v : {height, width, out_height, out_width})
        if (v < 1 || v > RESAMPLE_MAX_SIDE)
            return fail("wm_resample_u8: %dx%d -> %dx%d, sides must be in 1..%d", height, width, out_height, out_width, RESAMPLE_MAX_SIDE);
    return resample_impl(in_dev, height, width, out_dev, out_height, out_width, (hipStream_t)stream);
}

extern "C" int wm_scaled_size(int height, int width, double scale, int* out_h, int* out_w) {
    if (!out_h || !out_w) return fail("wm_scaled_size: null output");
    if (height < 1 || width < 1 || height > RESAMPLE_MAX_SIDE || width > RESAMPLE_MAX_SIDE)
        return fail("wm_scaled_size: frame %dx%d outside 1..%d", height, width, RESAMPLE_MAX_SIDE);
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail("wm_scaled_size: scale %g is not a positive finite number", scale);
    const double oh = std::max(1.0, std::floor(height * scale + 0.5)), ow = std::max(1.0, std::floor(width * scale + 0.5));
    if (oh > RESAMPLE_MAX_SIDE || ow > RESAMPLE_MAX_SIDE)
        return fail("wm_scaled_size: %dx%d at scale %g exceeds %d", height, width, scale, RESAMPLE_MAX_SIDE);
    *out_h = (int)oh;
    *out_w = (int)ow;
    return 0;
}

extern "C" int wm_undistort_u8(const uint8_t* in_dev, int height, int width, const double camera[9], uint8_t* out_dev, int out_height,
                               int out_width, double f_out, int mode, const uint8_t fill_rgb[3], int64_t* stats_dev, void* stream) {
    return launch_undistort(in_dev, height, width, camera, out_dev, out_height, out_width, f_out, mode, fill_rgb, stats_dev,
                            (hipStream_t)stream);
}

extern "C" int wm_rectify_u8(const uint8_t* in_dev, int height, int width, const double camera[9], const double rot[9], uint8_t* out_dev,
                             int out_height, int out_width, double f_out, int mode, const uint8_t fill_rgb[3], int64_t* stats_dev, void* stream) {
    return launch_rectify(in_dev, height, width, camera, rot, out_dev, out_height, out_width, f_out, mode, fill_rgb, stats_dev,
                          (hipStream_t)stream);
}

extern "C" int wm_ortho_u8(const uint8_t* in_dev, int height, int width, const double camera[9], const double pose[12], const float* dem_dev,
                           int dem_height, int dem_width, const double dem_geo[3], uint8_t* out_dev, int out_height, int out_width,
                           const double out_geo[6], int mode, const uint8_t fill_rgb[3], int64_t* stats_dev, void* stream) {
    return launch_ortho(in_dev, height, width, camera, pose, dem_dev, dem_height, dem_width, dem_geo, out_dev, out_height, out_width, out_geo,
                        mode, fill_rgb, stats_dev, (hipStream_t)stream);
}

extern "C" int wm_chip_window(const float box[4], float context, int min_side, int max_side, int32_t out[3]) {
    if (!box || !out) return fail("wm_chip_window: null argument");
    WM_TRY(check_chip_rule("wm_chip_window", context, min_side, max_side));
    const chip_window w = chip_window_of(box, context, min_side, max_side);
    out[0] = w.y0; out[1] = w.x0; out[2] = w.side;
    return 0;
}

extern "C" int64_t wm_census_scratch_bytes(int n) { return census_scratch_bytes(n); }

extern "C" int wm_census(const float* boxes_dev, const float* scores_dev, const int32_t* labels_dev, const int32_t* box_frame_dev, int n,
                         const double* georef_dev, int n_frames, double radius, int flags, void* scratch_dev, int64_t scratch_bytes,
                         double* points_dev, int32_t* individual_dev, int32_t* keeper_dev, int32_t* members_dev, int32_t* count_dev,
                         void* stream) {
    return launch_census(boxes_dev, scores_dev, labels_dev, box_frame_dev, n, georef_dev, n_frames, radius, flags, scratch_dev,
                         scratch_bytes, points_dev, individual_dev, keeper_dev, members_dev, count_dev, (hipStream_t)stream);
}

extern "C" int wm_coverage_raster(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx,
                                  int gy, uint16_t* coverage_dev, int64_t* stats_dev, void* stream) {
    return launch_coverage_raster(g2p_dev, size_dev, n_frames, x0, y0, cell, gx, gy, coverage_dev, stats_dev, (hipStream_t)stream);
}

extern "C" int wm_coverage_points(const double* g2p_dev, const int32_t* size_dev, int n_frames, const double* points_dev,
                                  const int32_t* labels_dev, int n_points, double x0, double y0, double cell, int gx, int gy,
                                  int32_t* seen_by_dev, int32_t* cell_dev, int32_t* counts_dev, int64_t* pstats_dev, void* stream) {
    return launch_coverage_points(g2p_dev, size_dev, n_frames, points_dev, labels_dev, n_points, x0, y0, cell, gx, gy, seen_by_dev,
                                  cell_dev, counts_dev, pstats_dev, (hipStream_t)stream);
}

extern "C" int wm_mosaic_plan(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx, int gy,
                              int32_t* source_dev, int32_t* won_dev, int64_t* stats_dev, void* stream) {
    return launch_mosaic_plan(g2p_dev, size_dev, n_frames, x0, y0, cell, gx, gy, source_dev, won_dev, stats_dev, (hipStream_t)stream);
}

extern "C" int wm_mosaic_fill_u8(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev, const double* g2p_dev,
                                 const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx, int gy,
                                 const int32_t* source_dev, int mode, int flags, uint8_t* mosaic_dev, int32_t* status_dev, void* stream) {
    return launch_mosaic_fill(frames_dev, n_resident, slot_dev, g2p_dev, size_dev, n_frames, x0, y0, cell, gx, gy, source_dev, mode, flags,
                              mosaic_dev, status_dev, (hipStream_t)stream);
}

extern "C" int wm_mosaic_blend_plan(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx,
                                    int gy, double band, double* best_dev, int32_t* cells_dev, int64_t* stats_dev, void* stream) {
    return launch_mosaic_blend_plan(g2p_dev, size_dev, n_frames, x0, y0, cell, gx, gy, band, best_dev, cells_dev, stats_dev, (hipStream_t)stream);
}

extern "C" int wm_mosaic_blend_accum_u8(const wm_frame_desc* frames_dev, const int32_t* index_dev, int n_resident, const double* g2p_dev,
                                        const int32_t* size_dev, int n_frames, const int32_t* exposure_dev, double x0, double y0, double cell,
                                        int gx, int gy, double band, const double* best_dev, int mode, uint32_t* acc_dev, int32_t* status_dev,
                                        void* stream) {
    return launch_mosaic_blend_accum(frames_dev, index_dev, n_resident, g2p_dev, size_dev, n_frames, exposure_dev, x0, y0, cell, gx, gy, band,
                                     best_dev, mode, acc_dev, status_dev, (hipStream_t)stream);
}

extern "C" int wm_mosaic_blend_finish_u8(const uint32_t* acc_dev, int gx, int gy, int flags, uint8_t* mosaic_dev, void* stream) {
    return launch_mosaic_blend_finish(acc_dev, gx, gy, flags, mosaic_dev, (hipStream_t)stream);
}

extern "C" int wm_register_render_u8(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev, const double* g2p_dev,
                                     const int32_t* size_dev, int n_frames, const wm_register_pair* pairs_dev, int n_pairs, double cell,
                                     int search, int side, uint8_t* a_dev, uint8_t* b_dev, int32_t* status_dev, void* stream) {
    return launch_register_render(frames_dev, n_resident, slot_dev, g2p_dev, size_dev, n_frames, pairs_dev, n_pairs, cell, search, side,
                                  a_dev, b_dev, status_dev, (hipStream_t)stream);
}

extern "C" int wm_register_search(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                                  int side, int min_cells, int32_t* score_dev, int32_t* best_dev, void* stream) {
    return launch_register_search(a_dev, b_dev, pairs_dev, n_pairs, search, side, min_cells, score_dev, best_dev, (hipStream_t)stream);
}

extern "C" int wm_register_search_zncc(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs,
                                       int search, int side, int min_cells, int64_t* moments_dev, int32_t* best_dev, double* peak_dev,
                                       void* stream) {
    return launch_register_search_zncc(a_dev, b_dev, pairs_dev, n_pairs, search, side, min_cells, moments_dev, best_dev, peak_dev,
                                       (hipStream_t)stream);
}

extern "C" int wm_register_refine(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                                  int side, int64_t* sums_dev, void* stream) {
    return launch_register_refine(a_dev, b_dev, pairs_dev, n_pairs, search, side, sums_dev, (hipStream_t)stream);
}

extern "C" int wm_register_reduce_u8(const uint8_t* in_dev, int n_planes, int ext, int level, uint8_t* out_dev, void* stream) {
    return launch_register_reduce(in_dev, n_planes, ext, level, out_dev, (hipStream_t)stream);
}

extern "C" int wm_crop_chips_u8(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev, const int32_t* box_frame_dev, int n,
                                int chip, float context, int min_side, int max_side, uint8_t* chips_dev, int32_t* windows_dev,
                                void* stream) {
    return launch_crop_chips(frames_dev, n_frames, boxes_dev, box_frame_dev, n, chip, context, min_side, max_side, chips_dev, windows_dev,
                             (hipStream_t)stream);
}

extern "C" int wm_box_outline_rect(const float box[4], int32_t out[4]) {
    if (!box || !out) return fail("wm_box_outline_rect: null argument");
    const outline_rect r = box_outline_rect_of(box);
    out[0] = r.drawn ? r.l : 0; out[1] = r.drawn ? r.t : 0; out[2] = r.drawn ? r.r : 0; out[3] = r.drawn ? r.b : 0;
    return r.drawn ? 0 : 1;
}

extern "C" int wm_draw_boxes_u8(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev, const int32_t* labels_dev,
                                const int32_t* box_frame_dev, int n, const uint8_t* palette_dev, int palette_size, int width,
                                void* stream) {
    return launch_draw_boxes(frames_dev, n_frames, boxes_dev, labels_dev, box_frame_dev, n, palette_dev, palette_size, width,
                             (hipStream_t)stream);
}

extern "C" int wm_plot_image_u8(const float* in_dev, int batch, int height, int width, uint8_t* out_dev, void* scratch_dev,
                                int64_t scratch_bytes, void* stream) {
    return launch_plot_image(in_dev, batch, height, width, out_dev, scratch_dev, scratch_bytes, (hipStream_t)stream);
}

// ---- taps / profiling / debug counters ----
extern "C" int wm_set_tap(wm_handle* h, int which) {
    if (!h) return fail("wm_set_tap: null handle");
    if (which < -3 || which >= h->depth) return fail("wm_set_tap: %d out of range", which);
    h->tap_which = which;
    return 0;
}

extern "C" int wm_read_tap(wm_handle* h, float* out_dev, int batch, void* stream) {
    if (!h || !out_dev) return fail("wm_read_tap: null argument");
    if (!h->tap_buf) return fail("wm_read_tap: no tap captured");
    if (batch <= 0 || batch > h->maxB) return fail("wm_read_tap: bad batch");
    HIP_TRY(hipMemcpyAsync(out_dev, h->tap_buf, (size_t)batch * T * h->D * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int wm_profile_enable(wm_handle* h, int on) {
    if (!h) return fail("wm_profile_enable: null handle");
    h->prof.on = on != 0;
    return 0;
}

extern "C" int wm_profile_reset(wm_handle* h) {
    if (!h) return fail("wm_profile_reset: null handle");
    WM_TRY(prof_collect(h));
    for (auto& a : h->prof.acc) a = wm_kclass_stat{};
    return 0;
}

extern "C" int wm_profile_read(wm_handle* h, wm_kclass_stat* out) {
    if (!h || !out) return fail("wm_profile_read: null argument");
    WM_TRY(prof_collect(h));
    for (int i = 0; i < WM_KCLASS_COUNT; ++i) out[i] = h->prof.acc[i];
    return 0;
}

extern "C" int wm_debug_gemm_variant_counts(int64_t* out, int n) {
    if (!out || n < WM_GEMM_VARIANT_COUNT) return fail("wm_debug_gemm_variant_counts: need room for %d counters", WM_GEMM_VARIANT_COUNT);
    for (int i = 0; i < WM_GEMM_VARIANT_COUNT; ++i) out[i] = g_variant_count[i].load(std::memory_order_relaxed);
    return 0;
}
extern "C" int wm_debug_reset_gemm_variant_counts(void) {
    for (auto& c : g_variant_count) c.store(0, std::memory_order_relaxed);
    return 0;
}

extern "C" int wm_stream_overflow(wm_handle* h, int reset) {
    if (!h || !h->overflow) return fail("wm_stream_overflow: null handle");
    const int v0 = ((volatile int*)h->overflow)[0], v1 = ((volatile int*)h->overflow)[1];
    if (reset) ((volatile int*)h->overflow)[0] = ((volatile int*)h->overflow)[1] = 0;
    return (v0 != 0 ? WM_OVERFLOW_STREAM : 0) | (v1 != 0 ? WM_OVERFLOW_DECODER : 0);
}

extern "C" int wm_debug_saturation_enable(wm_handle* h, int on) {
    if (!h) return fail("wm_debug_saturation_enable: null handle");
    h->sat_on = on != 0;
    return 0;
}

extern "C" int wm_debug_saturation_read(wm_handle* h, int64_t* out, int n, int reset, void* stream) {
    if (!h || !out || n < WM_SAT_COUNT) return fail("wm_debug_saturation_read: need room for %d counters", WM_SAT_COUNT);
    HIP_TRY(hipSetDevice(h->device));
    unsigned long long host[WM_SAT_COUNT];
    HIP_TRY(hipMemcpyAsync(host, h->sat_counts, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < WM_SAT_COUNT; ++i) out[i] = (int64_t)host[i];
    if (reset) HIP_TRY(hipMemsetAsync(h->sat_counts, 0, sizeof(host), (hipStream_t)stream));
    return 0;
}

// ---- single-op entry points ----
extern "C" int wm_op_cvt_f32_to_16(const float* in_dev, void* out_dev, int64_t n, int precision, void* stream) {
    if (n % 4) return fail("cvt: n must be a multiple of 4");
    return launch_cvt_f32_to_16((hipStream_t)stream, precision, in_dev, out_dev, n / 4);
}

extern "C" int wm_op_cvt_16_to_f32(const void* in_dev, float* out_dev, int64_t n, int precision, void* stream) {
    return by_type16(precision, [&](auto t) {
        return launch_simple(nullptr, (hipStream_t)stream, 0.0, cvt_16_to_f32_kernel<decltype(t)>, dim3(grid_for(n)), dim3(256), (const u16*)in_dev, out_dev, n);
    });
}

extern "C" int wm_op_gemm16(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev, int res_mod,
                            float* out_f32_dev, void* out_16_dev, int M, int N, int K, int act, int precision, void* stream) {
    const int layout = act & (WM_GEMM_W_PACKED | WM_GEMM_A_PACKED | WM_GEMM_OUT_PACKED);
    act &= ~(WM_GEMM_W_PACKED | WM_GEMM_A_PACKED | WM_GEMM_OUT_PACKED);
    if (layout && !gemm16_takes_v5(M, N, K))
        return fail("wm_op_gemm16: M=%d N=%d K=%d runs on a half-width kernel, which takes row-major operands only (wm_op_gemm16_takes_packed)", M, N, K);
    return launch_gemm16(nullptr, (hipStream_t)stream, precision, a_dev, (layout & WM_GEMM_W_PACKED) ? nullptr : w_dev, bias_dev, residual_dev, res_mod,
                         out_f32_dev, out_16_dev, M, N, K, act, GX((layout & WM_GEMM_W_PACKED) ? w_dev : nullptr, (layout & WM_GEMM_A_PACKED) != 0,
                                                                   (layout & WM_GEMM_OUT_PACKED) != 0));
}

extern "C" int wm_op_gemm16_takes_packed(int M, int N, int K) { return gemm16_takes_v5(M, N, K) ? 1 : 0; }

extern "C" int wm_op_ln_stats16(const float* x_dev, float* stats_dev, void* x16_dev, int64_t rows, int C, int precision, void* stream) {
    if (!x_dev || !stats_dev || !x16_dev) return fail("wm_op_ln_stats16: null buffer");
    return launch_ln_stats16(nullptr, (hipStream_t)stream, precision, x_dev, stats_dev, x16_dev, rows, C);
}

extern "C" int wm_op_fold_weight16(const void* w16_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, void* wf_dev,
                                   float* c1_dev, float* c2_dev, int N, int K, int precision, void* stream) {
    if (!w16_dev || !gamma_dev || !beta_dev || !wf_dev || !c1_dev || !c2_dev) return fail("wm_op_fold_weight16: null buffer");
    if (N <= 0 || K <= 0 || N % 16 || K % 32) return fail("wm_op_fold_weight16: N=%d K=%d (N %% 16, K %% 32)", N, K);
    if (precision != WM_PREC_FP16 && precision != WM_PREC_BF16) return fail("wm_op_fold_weight16: precision %d", precision);
    return launch_fold_weight((hipStream_t)stream, precision, w16_dev, nullptr, gamma_dev, beta_dev, bias_dev, wf_dev, c1_dev, c2_dev, N, K);
}

extern "C" int wm_op_gemm16_folded_walk(const void* x16_dev, const void* wf_dev, const float* c1_dev, const float* c2_dev, const float* stats_dev,
                                        float eps, void* out_16_dev, int M, int N, int K, int act, int walk, int precision, void* stream) {
    if (!x16_dev || !wf_dev || !c1_dev || !c2_dev || !stats_dev || !out_16_dev) return fail("wm_op_gemm16_folded: null buffer");
    if (walk < 0 || walk > 8) return fail("wm_op_gemm16_folded_walk: walk = %d (0 = the launcher's choice, 1..8 column tiles per workgroup)", walk);
    const int out_packed = (act & WM_GEMM_OUT_PACKED) != 0;
    act &= ~WM_GEMM_OUT_PACKED;
    if (!(walk > 0 ? gemm16_v5_serves(M, N, K) : gemm16_takes_v5(M, N, K)))
        return fail("wm_op_gemm16_folded: M=%d N=%d K=%d is not served by the 256-row-tile kernel", M, N, K);
    GemmExtra x = GX(wf_dev, 1, out_packed);
    x.fold_stats = stats_dev; x.fold_c1 = c1_dev; x.fold_eps = eps; x.walk = walk;
    return launch_gemm16(nullptr, (hipStream_t)stream, precision, x16_dev, nullptr, c2_dev, nullptr, 0, nullptr, out_16_dev, M, N, K, act, x);
}
extern "C" int wm_op_gemm16_folded(const void* x16_dev, const void* wf_dev, const float* c1_dev, const float* c2_dev, const float* stats_dev,
                                   float eps, void* out_16_dev, int M, int N, int K, int act, int precision, void* stream) {
    return wm_op_gemm16_folded_walk(x16_dev, wf_dev, c1_dev, c2_dev, stats_dev, eps, out_16_dev, M, N, K, act, 0, precision, stream);
}

extern "C" int wm_op_gemm16_stats(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev, float* out_f32_dev,
                                  void* x16_dev, float* stats_dev, int M, int N, int K, int layout, int precision, void* stream) {
    if (!a_dev || !w_dev || !residual_dev || !out_f32_dev || !x16_dev || !stats_dev) return fail("wm_op_gemm16_stats: null buffer");
    if (!gemm16_takes_v5(M, N, K)) return fail("wm_op_gemm16_stats: M=%d N=%d K=%d is not served by the 256-row-tile kernel", M, N, K);
    GemmExtra x = GX((layout & WM_GEMM_W_PACKED) ? w_dev : nullptr, (layout & WM_GEMM_A_PACKED) != 0, 0);
    x.st_stats = stats_dev;
    return launch_gemm16(nullptr, (hipStream_t)stream, precision, a_dev, (layout & WM_GEMM_W_PACKED) ? nullptr : w_dev, bias_dev, residual_dev, 0,
                         out_f32_dev, x16_dev, M, N, K, ACT_NONE, x);
}

extern "C" int wm_op_pack16(const void* in_dev, void* out_dev, int64_t rows, int K, void* stream) {
    if (!in_dev || !out_dev || rows <= 0 || K <= 0 || rows % 16 || K % 32) return fail("wm_op_pack16: rows=%lld K=%d (rows %% 16, K %% 32)", (long long)rows, K);
    return launch_simple(nullptr, (hipStream_t)stream, 0.0, pack16_lds_image_kernel, dim3(grid_for(rows * (K / 8))), dim3(256), (const uint4*)in_dev, (uint4*)out_dev, rows, K);
}

extern "C" int wm_op_unpack16(const void* in_dev, void* out_dev, int64_t rows, int K, void* stream) {
    if (!in_dev || !out_dev || rows <= 0 || K <= 0 || rows % 16 || K % 32) return fail("wm_op_unpack16: rows=%lld K=%d (rows %% 16, K %% 32)", (long long)rows, K);
    return launch_simple(nullptr, (hipStream_t)stream, 0.0, unpack16_lds_image_kernel, dim3(grid_for(rows * (K / 8))), dim3(256), (const uint4*)in_dev, (uint4*)out_dev, rows, K);
}

extern "C" int wm_op_ln_stats16_split(const float* x_dev, float* stats_dev, void* hi_dev, void* lo_dev, float* x_rw_dev, int64_t rows, int C,
                                      int precision, void* stream) {
    if (!x_dev || !stats_dev || !hi_dev || !lo_dev) return fail("wm_op_ln_stats16_split: null buffer");
    return launch_ln_stats16(nullptr, (hipStream_t)stream, precision, x_dev, stats_dev, hi_dev, rows, C, lo_dev, x_rw_dev, nullptr);
}

extern "C" int wm_op_gemm16_split(const void* a_dev, const void* w_dev, const float* bias_dev, void* hi_dev, void* lo_dev, float* stats_dev,
                                  int M, int N, int K, int layout, int precision, void* stream) {
    if (!a_dev || !w_dev || !hi_dev || !lo_dev || !stats_dev) return fail("wm_op_gemm16_split: null buffer");
    if (!gemm16_takes_v5(M, N, K)) return fail("wm_op_gemm16_split: M=%d N=%d K=%d is not served by the 256-row-tile kernel", M, N, K);
    GemmExtra x = GX((layout & WM_GEMM_W_PACKED) ? w_dev : nullptr, (layout & WM_GEMM_A_PACKED) != 0, 0);
    x.st_stats = stats_dev; x.res_hi = hi_dev; x.res_lo = lo_dev; x.out_lo = lo_dev;
    return launch_gemm16(nullptr, (hipStream_t)stream, precision, a_dev, (layout & WM_GEMM_W_PACKED) ? nullptr : w_dev, bias_dev, nullptr, 0,
                         nullptr, hi_dev, M, N, K, ACT_NONE, x);
}

extern "C" int wm_op_stream_merge(const void* hi_dev, const void* lo_dev, float* out_dev, int64_t rows, int C, int precision, void* stream) {
    if (!hi_dev || !lo_dev || !out_dev) return fail("wm_op_stream_merge: null buffer");
    return launch_stream_merge(nullptr, (hipStream_t)stream, precision, hi_dev, lo_dev, out_dev, rows, C);
}

extern "C" int wm_op_gemm8(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev, const float* residual_dev,
                           float* out_f32_dev, void* out_16_dev, void* out_8_dev, int M, int N, int K, int act, int precision, void* stream) {
    return launch_gemm8(nullptr, (hipStream_t)stream, precision, a_dev, w_dev, wscale_dev, bias_dev, residual_dev, out_f32_dev, out_16_dev, out_8_dev,
                        M, N, K, act);
}

extern "C" int wm_op_stream_rows(float* x_f32_dev, void* hi_dev, void* lo_dev, int64_t rows, int C, int precision, int merge, void* stream) {
    if (!x_f32_dev || !hi_dev || !lo_dev) return fail("wm_op_stream_rows: null buffer");
    return launch_stream_rows(nullptr, (hipStream_t)stream, precision, x_f32_dev, hi_dev, lo_dev, rows, C, merge != 0);
}

extern "C" int wm_op_gemm8_planes(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev, void* hi_dev, void* lo_dev,
                                  int M, int N, int K, int precision, void* stream) {
    if (!hi_dev || !lo_dev) return fail("wm_op_gemm8_planes: null plane");
    return launch_gemm8(nullptr, (hipStream_t)stream, precision, a_dev, w_dev, wscale_dev, bias_dev, nullptr, nullptr, nullptr, nullptr, M, N, K, ACT_NONE,
                        hi_dev, lo_dev);
}

extern "C" int wm_op_layernorm_fp8_plane(const void* hi_dev, const float* gamma_dev, const float* beta_dev, float eps, void* out_8_dev, int64_t rows, int C,
                                        int precision, void* stream) {
    if (!hi_dev || !out_8_dev || !gamma_dev || !beta_dev) return fail("wm_op_layernorm_fp8_plane: null buffer");
    return launch_layernorm_plane8(nullptr, (hipStream_t)stream, precision, hi_dev, gamma_dev, beta_dev, eps, out_8_dev, rows, C);
}

extern "C" int wm_op_cvt_f32_to_fp8(const float* in_dev, void* out_dev, int64_t n, void* stream) {
    if (n % 4) return fail("cvt fp8: n must be a multiple of 4");
    return launch_simple(nullptr, (hipStream_t)stream, 0.0, cvt_f32_to_fp8_kernel, dim3(grid_for(n / 4)), dim3(256), in_dev, (unsigned char*)out_dev, n / 4);
}

extern "C" int wm_op_conv3x3_16(const void* a_dev, const void* w_dev, float* out_dev, int batch, int c_out, int c_in, int precision,
                               void* stream) {
    return launch_conv3x3_16(nullptr, (hipStream_t)stream, precision, a_dev, w_dev, out_dev, batch * 4096, c_out, c_in);
}

extern "C" int wm_op_patch_embed16(const void* img16_dev, const void* w_dev, const float* bias_dev, float* out_f32_dev, void* out_16_dev,
                                  int batch, int n_out, int c_in, int precision, void* stream) {
    if (!img16_dev || !w_dev) return fail("wm_op_patch_embed16: null buffer");
    return launch_patch_embed16(nullptr, (hipStream_t)stream, precision, img16_dev, w_dev, bias_dev, nullptr, 0, out_f32_dev, out_16_dev, batch, n_out, c_in);
}

extern "C" int wm_op_gemm32(const float* a_dev, const float* w_dev, const float* bias_dev, const float* residual_dev, float* out_dev,
                            int M, int N, int K, int act, void* stream) {
    // act & WM_GEMM32_SPLIT: the fp16-split form (gemm32x3_kernel, W split per K-step); act & WM_GEMM32_PRESPLIT: the same form with W
    // split once by split_w32_kernel (the engine's); otherwise the fp32-MFMA kernel
    const int split = (act & WM_GEMM32_SPLIT) != 0, presplit = (act & WM_GEMM32_PRESPLIT) != 0;
    if (split && presplit) return fail("wm_op_gemm32: WM_GEMM32_SPLIT and WM_GEMM32_PRESPLIT are exclusive");
    return launch_gemm32(nullptr, (hipStream_t)stream, a_dev, w_dev, bias_dev, residual_dev, out_dev, M, N, K, act & 0xff, 0,
                         presplit ? 3 : split ? 2 : 1);
}

extern "C" int wm_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, float* out_f32_dev,
                               void* out_16_dev, int64_t rows, int C, int precision, void* stream) {
    const int packed = (precision & WM_LAYOUT_PACKED) != 0;
    precision &= ~WM_LAYOUT_PACKED;
    if (!out_f32_dev && out_16_dev)      // the transformer blocks' form: column-tiled statistics (the arithmetic of the folded LayerNorm's statistics)
        return launch_layernorm_block(nullptr, (hipStream_t)stream, precision, x_dev, gamma_dev, beta_dev, eps, out_16_dev, rows, C, packed);
    if (packed) return fail("wm_op_layernorm: the LDS-image-order output exists for the 16-bit-only form");
    return launch_layernorm(nullptr, (hipStream_t)stream, precision, x_dev, gamma_dev, beta_dev, eps, out_f32_dev, out_16_dev, rows, C);
}

extern "C" int wm_op_encoder_attention(const void* qkv_dev, const float* qkv_bias_dev, const float* rel_pos_h_dev,
                                       const float* rel_pos_w_dev, void* out_dev, int batch, int heads, int head_dim, int window,
                                       int precision, void* stream) {
    return launch_encoder_attention(nullptr, (hipStream_t)stream, precision, qkv_dev, qkv_bias_dev, rel_pos_h_dev, rel_pos_w_dev, out_dev,
                                    batch, heads, head_dim, window);
}

extern "C" int wm_op_encoder_attention_qkv(const void* q_dev, const void* k_dev, const void* v_dev, int token_stride, const float* qkv_bias_dev,
                                           const float* rel_pos_h_dev, const float* rel_pos_w_dev, void* out_dev, int batch, int heads,
                                           int head_dim, int window, int precision, void* stream) {
    AttnExtra x;
    x.k_sep = k_dev; x.v_sep = v_dev; x.tok_stride = token_stride;
    return launch_encoder_attention(nullptr, (hipStream_t)stream, precision, q_dev, qkv_bias_dev, rel_pos_h_dev, rel_pos_w_dev, out_dev,
                                    batch, heads, head_dim, window, x);
}

extern "C" int wm_op_mha16(const void* q_dev, int q_stride, const void* k_dev, int k_stride, const void* v_dev, int v_stride,
                           void* out_dev, int out_stride, int batch, int heads, int head_dim, int nq, int nk, int precision, void* stream) {
    return launch_mha16(nullptr, (hipStream_t)stream, precision, q_dev, q_stride, k_dev, k_stride, v_dev, v_stride, out_dev, out_stride,
                        batch, heads, head_dim, nq, nk);
}

extern "C" int wm_op_mha32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int batch, int heads,
                           int head_dim, int nq, int nk, void* stream) {
    return launch_mha32(nullptr, (hipStream_t)stream, q_dev, k_dev, v_dev, out_dev, batch, heads, head_dim, nq, nk);
}
