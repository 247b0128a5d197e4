// Survey launchers: merge, census, coverage, mosaic, registration, review chips and overlays.  Each checks every argument on
// the host before its first HIP call.
#pragma once
#include "survey_kernels.h"
#include "census_kernels.h"
#include "coverage_kernels.h"
#include "mosaic_kernels.h"
#include "mosaic_blend_kernels.h"
#include "register_kernels.h"
#include "register_refine_kernels.h"
#include "register_pyramid_kernels.h"
#include "chip_kernels.h"
#include "overlay_kernels.h"
#include "host_core.h"

namespace {

static_assert(sizeof(wm_frame_desc) == sizeof(frame_desc), "wm_frame_desc layout");

// Argument checks and launches of both merge modes; `thr_name` is the threshold's name in error messages.
template <int MODE>
static int launch_merge_frames(const char* name, const char* thr_name, const wm_box_record* records_dev, const int32_t* origins_dev,
                               const int32_t* frame_tile_offsets, int n_frames, float thr, void* scratch_dev, int64_t scratch_bytes,
                               wm_box_record* merged_dev, wm_box_record* det_dev, int32_t* det_tile_dev, int32_t* det_count_dev,
                               int32_t* det_members_dev, int32_t* slot_det_dev, void* stream) {
    if (!records_dev || !origins_dev || !frame_tile_offsets || !scratch_dev || !merged_dev || !det_dev || !det_tile_dev || !det_count_dev)
        return fail("%s: null buffer", name);
    if (MODE == MF_FUSE && (!det_members_dev || !slot_det_dev)) return fail("%s: null buffer", name);
    if (n_frames <= 0) return fail("%s: n_frames %d", name, n_frames);
    if (!(thr >= 0.f && thr < 1.f)) return fail("%s: %s %g outside [0, 1)", name, thr_name, (double)thr);
    if (frame_tile_offsets[0] != 0) return fail("%s: frame_tile_offsets[0] = %d, not 0", name, frame_tile_offsets[0]);
    for (int f = 0; f < n_frames; ++f)
        if (frame_tile_offsets[f + 1] <= frame_tile_offsets[f])
            return fail("%s: frame_tile_offsets not strictly increasing at frame %d (%d -> %d)", name, f, frame_tile_offsets[f],
                        frame_tile_offsets[f + 1]);
    const int n_tiles = frame_tile_offsets[n_frames];
    const int64_t need = wm_merge_frames_scratch_bytes(n_tiles);
    if (need < 0) return -1;
    if (scratch_bytes < need) return fail("%s: scratch of %lld bytes, %lld needed", name, (long long)scratch_bytes, (long long)need);
    if ((uintptr_t)scratch_dev % 16) return fail("%s: scratch not 16-byte aligned", name);
    for (int f0 = 0; f0 < n_frames; f0 += MF_MAX_FRAMES) {
        const int nf = std::min(MF_MAX_FRAMES, n_frames - f0);
        mf_offsets offs;
        for (int f = 0; f <= nf; ++f) offs.tile[f] = frame_tile_offsets[f0 + f];
        hipLaunchKernelGGL(merge_frames_nms_kernel<MODE>, dim3(nf), dim3(MF_THREADS), 0, (hipStream_t)stream, records_dev,
                           (const int*)origins_dev, offs, thr, (char*)scratch_dev, n_tiles * WM_NUM_QUERIES, merged_dev, det_dev,
                           (int*)det_tile_dev, (int*)det_count_dev, (int*)det_members_dev, (int*)slot_det_dev, f0);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Survey census: every argument is checked on the host before the first HIP call; one launch of one workgroup.
int64_t census_scratch_bytes(int n) {
    if (n < 0 || n > WM_CENSUS_MAX_DETS) return fail("wm_census_scratch_bytes: n %d outside 0..%d", n, WM_CENSUS_MAX_DETS);
    return CENSUS_HEADER + (int64_t)n * CENSUS_SCRATCH_PER_DET;
}

int launch_census(const float* boxes_dev, const float* scores_dev, const int32_t* labels_dev, const int32_t* box_frame_dev, int n,
                  const double* georef_dev, int n_frames, double radius, int flags, void* scratch_dev, int64_t scratch_bytes,
                  double* points_dev, int32_t* individual_dev, int32_t* keeper_dev, int32_t* members_dev, int32_t* count_dev,
                  hipStream_t s) {
    const char* name = "wm_census";
    if (n < 0 || n > WM_CENSUS_MAX_DETS) return fail("%s: n %d outside 0..%d", name, n, WM_CENSUS_MAX_DETS);
    if (n == 0) return 0;
    if (!boxes_dev || !scores_dev || !labels_dev || !box_frame_dev || !georef_dev || !scratch_dev || !points_dev || !individual_dev ||
        !keeper_dev || !members_dev || !count_dev)
        return fail("%s: null buffer", name);
    if (n_frames <= 0) return fail("%s: n_frames %d", name, n_frames);
    if (!(std::isfinite(radius) && radius >= 0.0)) return fail("%s: radius %g: need a finite radius >= 0", name, radius);
    const double r2 = radius * radius;
    if (!std::isfinite(r2)) return fail("%s: radius %g: its square is not finite", name, radius);
    if (flags & ~WM_CENSUS_SAME_CLASS) return fail("%s: flags 0x%x", name, (unsigned)flags);
    const int64_t need = census_scratch_bytes(n);
    if (scratch_bytes < need) return fail("%s: scratch of %lld bytes, %lld needed", name, (long long)scratch_bytes, (long long)need);
    if ((uintptr_t)scratch_dev % 16) return fail("%s: scratch not 16-byte aligned", name);
    if ((uintptr_t)boxes_dev % 16 || (uintptr_t)points_dev % 16 || (uintptr_t)georef_dev % 8)
        return fail("%s: boxes_dev / points_dev not 16-byte aligned, or georef_dev not 8-byte aligned", name);
    hipLaunchKernelGGL(census_kernel, dim3(1), dim3(MF_THREADS), 0, s, (const float4*)boxes_dev, scores_dev, (const int*)labels_dev,
                       (const int*)box_frame_dev, n, georef_dev, n_frames, radius, r2, flags & WM_CENSUS_SAME_CLASS, (char*)scratch_dev,
                       (double2*)points_dev, (int*)individual_dev, (int*)keeper_dev, (int*)members_dev, (int*)count_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Survey coverage: every argument is checked on the host before the first HIP call.  The grid of both entries.
static int check_coverage_grid(const char* name, double x0, double y0, double cell, int gx, int gy) {
    if (!std::isfinite(x0)) return fail("%s: x0 %g is not finite", name, x0);
    if (!std::isfinite(y0)) return fail("%s: y0 %g is not finite", name, y0);
    if (!(std::isfinite(cell) && cell > 0.0)) return fail("%s: cell %g: need a finite cell > 0", name, cell);
    if (gx < 1 || gx > WM_COVERAGE_MAX_SIDE) return fail("%s: gx %d outside 1..%d", name, gx, WM_COVERAGE_MAX_SIDE);
    if (gy < 1 || gy > WM_COVERAGE_MAX_SIDE) return fail("%s: gy %d outside 1..%d", name, gy, WM_COVERAGE_MAX_SIDE);
    if ((int64_t)gx * gy > WM_COVERAGE_MAX_CELLS)
        return fail("%s: gx * gy = %lld cells exceed %d", name, (long long)gx * gy, WM_COVERAGE_MAX_CELLS);
    return 0;
}

static int check_coverage_frames(const char* name, const double* g2p_dev, const int32_t* size_dev, int n_frames) {
    if (n_frames < 0 || n_frames > WM_COVERAGE_MAX_FRAMES) return fail("%s: n_frames %d outside 0..%d", name, n_frames, WM_COVERAGE_MAX_FRAMES);
    if (n_frames > 0 && (!g2p_dev || !size_dev)) return fail("%s: null g2p_dev / size_dev with n_frames %d", name, n_frames);
    if ((uintptr_t)g2p_dev % 8 || (uintptr_t)size_dev % 4) return fail("%s: g2p_dev not 8-byte aligned, or size_dev not 4-byte aligned", name);
    return 0;
}

// The workgroups of the raster and the plan: one per block of COV_BLOCK_X x COV_BLOCK_Y cells.
static dim3 coverage_block_grid(int gx, int gy) { return dim3((gx + COV_BLOCK_X - 1) / COV_BLOCK_X, (gy + COV_BLOCK_Y - 1) / COV_BLOCK_Y); }

// n_resident of the mosaic fill and the registration render.
static int check_n_resident(const char* name, int n_resident) {
    if (n_resident < 0 || n_resident > WM_COVERAGE_MAX_FRAMES)
        return fail("%s: n_resident %d outside 0..%d", name, n_resident, WM_COVERAGE_MAX_FRAMES);
    return 0;
}

int launch_coverage_raster(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx,
                           int gy, uint16_t* coverage_dev, int64_t* stats_dev, hipStream_t s) {
    const char* name = "wm_coverage_raster";
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    if (!coverage_dev || !stats_dev) return fail("%s: null coverage_dev / stats_dev", name);
    if ((uintptr_t)coverage_dev % 2 || (uintptr_t)stats_dev % 8) return fail("%s: coverage_dev not 2-byte aligned, or stats_dev not 8-byte aligned", name);
    HIP_TRY(hipMemsetAsync(stats_dev, 0, COV_STATS * sizeof(int64_t), s));
    hipLaunchKernelGGL(coverage_raster_kernel, coverage_block_grid(gx, gy), dim3(COV_THREADS), 0, s, g2p_dev, (const int*)size_dev, n_frames,
                       x0, y0, cell, gx, gy, coverage_dev, (unsigned long long*)stats_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_coverage_points(const double* g2p_dev, const int32_t* size_dev, int n_frames, const double* points_dev,
                           const int32_t* labels_dev, int n_points, double x0, double y0, double cell, int gx, int gy,
                           int32_t* seen_by_dev, int32_t* cell_dev, int32_t* counts_dev, int64_t* pstats_dev, hipStream_t s) {
    const char* name = "wm_coverage_points";
    if (n_points < 0 || n_points > WM_CENSUS_MAX_DETS) return fail("%s: n_points %d outside 0..%d", name, n_points, WM_CENSUS_MAX_DETS);
    if (n_points == 0) return 0;
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    if (!points_dev || !labels_dev || !seen_by_dev || !cell_dev || !pstats_dev) return fail("%s: null buffer", name);
    if ((uintptr_t)points_dev % 8 || (uintptr_t)pstats_dev % 8 || (uintptr_t)labels_dev % 4 || (uintptr_t)seen_by_dev % 4 ||
        (uintptr_t)cell_dev % 4 || (uintptr_t)counts_dev % 4)
        return fail("%s: points_dev / pstats_dev not 8-byte aligned, or an int32 buffer not 4-byte aligned", name);
    HIP_TRY(hipMemsetAsync(pstats_dev, 0, 2 * sizeof(int64_t), s));
    if (counts_dev) HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)COV_CLASSES * gx * gy * sizeof(int32_t), s));
    hipLaunchKernelGGL(coverage_points_kernel, dim3((n_points + COV_THREADS - 1) / COV_THREADS), dim3(COV_THREADS), 0, s, g2p_dev,
                       (const int*)size_dev, n_frames, points_dev, (const int*)labels_dev, n_points, x0, y0, cell, gx, gy, (int*)seen_by_dev,
                       (int*)cell_dev, (int*)counts_dev, (unsigned long long*)pstats_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Survey mosaic: the coverage's grid and frame checks, every argument checked on the host before the first HIP call.
int launch_mosaic_plan(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx, int gy,
                       int32_t* source_dev, int32_t* won_dev, int64_t* stats_dev, hipStream_t s) {
    const char* name = "wm_mosaic_plan";
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    if (!source_dev) return fail("%s: null source_dev", name);
    if (!stats_dev) return fail("%s: null stats_dev", name);
    if (n_frames > 0 && !won_dev) return fail("%s: null won_dev with n_frames %d", name, n_frames);
    if ((uintptr_t)source_dev % 4 || (uintptr_t)won_dev % 4 || (uintptr_t)stats_dev % 8)
        return fail("%s: source_dev / won_dev not 4-byte aligned, or stats_dev not 8-byte aligned", name);
    HIP_TRY(hipMemsetAsync(stats_dev, 0, 2 * sizeof(int64_t), s));
    if (n_frames > 0) HIP_TRY(hipMemsetAsync(won_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
    hipLaunchKernelGGL(mosaic_plan_kernel, coverage_block_grid(gx, gy), dim3(COV_THREADS), 0, s, g2p_dev, (const int*)size_dev, n_frames, x0,
                       y0, cell, gx, gy, (int*)source_dev, (int*)won_dev, (unsigned long long*)stats_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_mosaic_fill(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev, const double* g2p_dev,
                       const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx, int gy, const int32_t* source_dev,
                       int mode, int flags, uint8_t* mosaic_dev, int32_t* status_dev, hipStream_t s) {
    const char* name = "wm_mosaic_fill_u8";
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_n_resident(name, n_resident));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    if (mode != WM_MOSAIC_NEAREST && mode != WM_MOSAIC_BILINEAR) return fail("%s: mode %d is neither WM_MOSAIC_NEAREST nor WM_MOSAIC_BILINEAR", name, mode);
    if (flags & ~WM_MOSAIC_NORTH_UP) return fail("%s: flags 0x%x", name, (unsigned)flags);
    if (!source_dev) return fail("%s: null source_dev", name);
    if (!mosaic_dev) return fail("%s: null mosaic_dev", name);
    if (!status_dev) return fail("%s: null status_dev", name);
    if (n_frames > 0 && n_resident > 0 && !frames_dev) return fail("%s: null frames_dev with n_resident %d", name, n_resident);
    if (n_frames > 0 && n_resident > 0 && !slot_dev) return fail("%s: null slot_dev with n_frames %d", name, n_frames);
    if ((uintptr_t)frames_dev % 8 || (uintptr_t)slot_dev % 4 || (uintptr_t)source_dev % 4 || (uintptr_t)status_dev % 4)
        return fail("%s: frames_dev not 8-byte aligned, or slot_dev / source_dev / status_dev not 4-byte aligned", name);
    if (n_frames == 0 || n_resident == 0) return 0;                   // no source can be resident: nothing is written
    const dim3 grid((gx + COV_BLOCK_X - 1) / COV_BLOCK_X, (gy + MOS_FILL_BLOCK_Y - 1) / MOS_FILL_BLOCK_Y);
    const int north_up = flags & WM_MOSAIC_NORTH_UP;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(COV_THREADS), 0, s, (const frame_desc*)frames_dev, n_resident, (const int*)slot_dev, g2p_dev,
                           (const int*)size_dev, n_frames, x0, y0, cell, gx, gy, (const int*)source_dev, north_up, mosaic_dev, (int*)status_dev);
    };
    mode == WM_MOSAIC_NEAREST ? launch(mosaic_fill_kernel<WM_MOSAIC_NEAREST>) : launch(mosaic_fill_kernel<WM_MOSAIC_BILINEAR>);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Survey mosaic, blended: the mosaic's checks plus band, every argument checked on the host before the first HIP call.
// k = 256 / band, the rule's one division, is computed here; a band so small that k overflows is refused with the band.
static int check_blend_band(const char* name, double band, double& k) {
    k = 256.0 / band;
    if (!(std::isfinite(band) && band > 0.0 && std::isfinite(k))) return fail("%s: band %g: need a finite band > 0 with a finite 256 / band", name, band);
    return 0;
}

int launch_mosaic_blend_plan(const double* g2p_dev, const int32_t* size_dev, int n_frames, double x0, double y0, double cell, int gx, int gy,
                             double band, double* best_dev, int32_t* cells_dev, int64_t* stats_dev, hipStream_t s) {
    const char* name = "wm_mosaic_blend_plan";
    double k;
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    WM_TRY(check_blend_band(name, band, k));
    if (!best_dev) return fail("%s: null best_dev", name);
    if (!stats_dev) return fail("%s: null stats_dev", name);
    if (n_frames > 0 && !cells_dev) return fail("%s: null cells_dev with n_frames %d", name, n_frames);
    if ((uintptr_t)best_dev % 8 || (uintptr_t)stats_dev % 8 || (uintptr_t)cells_dev % 4)
        return fail("%s: best_dev / stats_dev not 8-byte aligned, or cells_dev not 4-byte aligned", name);
    HIP_TRY(hipMemsetAsync(stats_dev, 0, 3 * sizeof(int64_t), s));
    if (n_frames > 0) HIP_TRY(hipMemsetAsync(cells_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
    hipLaunchKernelGGL(mosaic_blend_plan_kernel, coverage_block_grid(gx, gy), dim3(COV_THREADS), 0, s, g2p_dev, (const int*)size_dev, n_frames,
                       x0, y0, cell, gx, gy, band, k, best_dev, (int*)cells_dev, (unsigned long long*)stats_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_mosaic_blend_accum(const wm_frame_desc* frames_dev, const int32_t* index_dev, int n_resident, const double* g2p_dev,
                              const int32_t* size_dev, int n_frames, const int32_t* exposure_dev, double x0, double y0, double cell, int gx,
                              int gy, double band, const double* best_dev, int mode, uint32_t* acc_dev, int32_t* status_dev, hipStream_t s) {
    const char* name = "wm_mosaic_blend_accum_u8";
    double k;
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_n_resident(name, n_resident));
    WM_TRY(check_coverage_grid(name, x0, y0, cell, gx, gy));
    WM_TRY(check_blend_band(name, band, k));
    if (mode != WM_MOSAIC_NEAREST && mode != WM_MOSAIC_BILINEAR) return fail("%s: mode %d is neither WM_MOSAIC_NEAREST nor WM_MOSAIC_BILINEAR", name, mode);
    if (!best_dev) return fail("%s: null best_dev", name);
    if (!acc_dev) return fail("%s: null acc_dev", name);
    if (!status_dev) return fail("%s: null status_dev", name);
    if (n_resident > 0 && !frames_dev) return fail("%s: null frames_dev with n_resident %d", name, n_resident);
    if (n_resident > 0 && !index_dev) return fail("%s: null index_dev with n_resident %d", name, n_resident);
    if ((uintptr_t)frames_dev % 8 || (uintptr_t)best_dev % 8 || (uintptr_t)index_dev % 4 || (uintptr_t)exposure_dev % 4 ||
        (uintptr_t)acc_dev % 4 || (uintptr_t)status_dev % 4)
        return fail("%s: frames_dev / best_dev not 8-byte aligned, or index_dev / exposure_dev / acc_dev / status_dev not 4-byte aligned", name);
    if (n_resident == 0) return 0;                                    // no frame to walk: nothing is read or written
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, coverage_block_grid(gx, gy), dim3(COV_THREADS), 0, s, (const frame_desc*)frames_dev, (const int*)index_dev,
                           n_resident, g2p_dev, (const int*)size_dev, n_frames, (const int*)exposure_dev, x0, y0, cell, gx, gy, band, k, best_dev,
                           (unsigned int*)acc_dev, (int*)status_dev);
    };
    mode == WM_MOSAIC_NEAREST ? launch(mosaic_blend_accum_kernel<WM_MOSAIC_NEAREST>) : launch(mosaic_blend_accum_kernel<WM_MOSAIC_BILINEAR>);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_mosaic_blend_finish(const uint32_t* acc_dev, int gx, int gy, int flags, uint8_t* mosaic_dev, hipStream_t s) {
    const char* name = "wm_mosaic_blend_finish_u8";
    WM_TRY(check_coverage_grid(name, 0.0, 0.0, 1.0, gx, gy));
    if (flags & ~WM_MOSAIC_NORTH_UP) return fail("%s: flags 0x%x", name, (unsigned)flags);
    if (!acc_dev) return fail("%s: null acc_dev", name);
    if (!mosaic_dev) return fail("%s: null mosaic_dev", name);
    if ((uintptr_t)acc_dev % 4) return fail("%s: acc_dev not 4-byte aligned", name);
    const dim3 grid((gx + COV_BLOCK_X - 1) / COV_BLOCK_X, (gy + MOS_FILL_BLOCK_Y - 1) / MOS_FILL_BLOCK_Y);
    hipLaunchKernelGGL(mosaic_blend_finish_kernel, grid, dim3(COV_THREADS), 0, s, (const unsigned int*)acc_dev, gx, gy, flags & WM_MOSAIC_NORTH_UP,
                       mosaic_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Survey registration: every argument checked on the host before the first HIP call.  What both entries share.
static int check_register_shape(const char* name, const wm_register_pair* pairs_dev, int search, int side) {
    if (search < 0 || search > WM_REGISTER_MAX_SEARCH) return fail("%s: search %d outside 0..%d", name, search, WM_REGISTER_MAX_SEARCH);
    if (side < 1 || side > WM_REGISTER_MAX_SIDE) return fail("%s: side %d outside 1..%d", name, side, WM_REGISTER_MAX_SIDE);
    if (!pairs_dev) return fail("%s: null pairs_dev", name);
    if ((uintptr_t)pairs_dev % 8) return fail("%s: pairs_dev not 8-byte aligned", name);
    return 0;
}

int launch_register_render(const wm_frame_desc* frames_dev, int n_resident, const int32_t* slot_dev, const double* g2p_dev,
                           const int32_t* size_dev, int n_frames, const wm_register_pair* pairs_dev, int n_pairs, double cell, int search,
                           int side, uint8_t* a_dev, uint8_t* b_dev, int32_t* status_dev, hipStream_t s) {
    const char* name = "wm_register_render_u8";
    if (n_pairs < 0 || n_pairs > WM_REGISTER_MAX_PAIRS) return fail("%s: n_pairs %d outside 0..%d", name, n_pairs, WM_REGISTER_MAX_PAIRS);
    if (n_pairs == 0) return 0;
    WM_TRY(check_coverage_frames(name, g2p_dev, size_dev, n_frames));
    WM_TRY(check_n_resident(name, n_resident));
    if (!(std::isfinite(cell) && cell > 0.0)) return fail("%s: cell %g: need a finite cell > 0", name, cell);
    WM_TRY(check_register_shape(name, pairs_dev, search, side));
    if (!a_dev) return fail("%s: null a_dev", name);
    if (!b_dev) return fail("%s: null b_dev", name);
    if (!status_dev) return fail("%s: null status_dev", name);
    if (n_resident > 0 && !frames_dev) return fail("%s: null frames_dev with n_resident %d", name, n_resident);
    if (n_frames > 0 && !slot_dev) return fail("%s: null slot_dev with n_frames %d", name, n_frames);
    if ((uintptr_t)frames_dev % 8 || (uintptr_t)slot_dev % 4 || (uintptr_t)status_dev % 4)
        return fail("%s: frames_dev not 8-byte aligned, or slot_dev / status_dev not 4-byte aligned", name);
    const int ext = side + 2 * search;
    const int row_blocks = (ext + REG_RENDER_BLOCK_Y - 1) / REG_RENDER_BLOCK_Y;
    const dim3 grid((ext + 63) / 64, 2 * row_blocks, n_pairs);                    // y: plane A's blocks of rows, then plane B's
    hipLaunchKernelGGL(register_render_kernel, grid, dim3(REG_THREADS), 0, s, (const frame_desc*)frames_dev, n_resident, (const int*)slot_dev,
                       g2p_dev, (const int*)size_dev, n_frames, pairs_dev, cell, search, side, row_blocks, a_dev, b_dev, (int*)status_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Offsets per thread of either search: the largest K of {4, 2, 1} whose blocks of 256 * K offsets leave at most a tenth of
// their threads without an offset on (2S + 1)^2 offsets (a larger K shares each read of A among more offsets), else 1.
// WM_REGISTER_K = 1 | 2 | 4 overrides it (tools/register_time.py's A/B; the result does not depend on K).
static int register_offsets_per_thread(int n_off) {
    if (const char* e = getenv("WM_REGISTER_K")) {
        const int k = atoi(e);
        if (k == 1 || k == 2 || k == 4) return k;
    }
    for (int k : {4, 2}) {
        const int per = REG_THREADS * k, padded = (n_off + per - 1) / per * per;
        if ((padded - n_off) * 10 <= padded) return k;
    }
    return 1;
}

// Rows of A per tile of either search: 32 where the two tiles fit the LDS, else 16.
static int register_tile_rows(int search) {
    static_assert(reg_search_lds(WM_REGISTER_MAX_SEARCH, REG_TILE_ROWS_MAX / 2) <= REG_LDS_MAX, "16 rows fit at every search <= 64");
    return reg_search_lds(search, REG_TILE_ROWS_MAX) <= REG_LDS_MAX ? REG_TILE_ROWS_MAX : REG_TILE_ROWS_MAX / 2;
}

// Both searches: the shared checks, the metric's own pointer checks, the table's memset, the tiles, the K rule, the search
// launch and the pick launch.  SAD keeps two int32 per offset in score_dev; the correlation six int64 in moments_dev and
// the picks' q in peak_dev.  The K rule was measured for both kernels (profiles/register/README.md,
// profiles/register_zncc/README.md): for the correlation it picks the fastest K at search 16; at search 32 it picks K = 2
// where K = 4 measured 1.7 % faster, too little and too few points for a second rule.
template <bool ZNCC>
static int launch_register_search_as(const char* name, const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev,
                                     int n_pairs, int search, int side, int min_cells, std::conditional_t<ZNCC, int64_t, int32_t>* table_dev,
                                     int32_t* best_dev, double* peak_dev, hipStream_t s) {
    if (n_pairs < 0 || n_pairs > WM_REGISTER_MAX_PAIRS) return fail("%s: n_pairs %d outside 0..%d", name, n_pairs, WM_REGISTER_MAX_PAIRS);
    if (n_pairs == 0) return 0;
    WM_TRY(check_register_shape(name, pairs_dev, search, side));
    if (min_cells < 1) return fail("%s: min_cells %d: need at least 1", name, min_cells);
    if (!a_dev) return fail("%s: null a_dev", name);
    if (!b_dev) return fail("%s: null b_dev", name);
    if constexpr (ZNCC) {
        if (!table_dev) return fail("%s: null moments_dev", name);
        if (!best_dev) return fail("%s: null best_dev", name);
        if (!peak_dev) return fail("%s: null peak_dev", name);
        if ((uintptr_t)table_dev % 8) return fail("%s: moments_dev not 8-byte aligned", name);
        if ((uintptr_t)peak_dev % 8) return fail("%s: peak_dev not 8-byte aligned", name);
        if ((uintptr_t)best_dev % 4) return fail("%s: best_dev not 4-byte aligned", name);
    } else {
        if (!table_dev) return fail("%s: null score_dev", name);
        if (!best_dev) return fail("%s: null best_dev", name);
        if ((uintptr_t)table_dev % 4 || (uintptr_t)best_dev % 4) return fail("%s: score_dev / best_dev not 4-byte aligned", name);
    }
    using table = reg_table<ZNCC>;
    const int w1 = 2 * search + 1, n_off = w1 * w1;
    HIP_TRY(hipMemsetAsync(table_dev, 0, (size_t)n_pairs * n_off * table::entries * sizeof(*table_dev), s));
    const int tile_rows = register_tile_rows(search);
    const int lds = reg_search_lds(search, tile_rows);
    const int tiles_x = (side + REG_TILE_X - 1) / REG_TILE_X, tiles_y = (side + tile_rows - 1) / tile_rows;
    const int k = register_offsets_per_thread(n_off);
    const int off_blocks = (n_off + REG_THREADS * k - 1) / (REG_THREADS * k);
    const dim3 grid(tiles_x * tiles_y * off_blocks, n_pairs);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(REG_THREADS), lds, s, a_dev, b_dev, pairs_dev, search, side, tile_rows, tiles_x, off_blocks,
                           (typename table::elem*)table_dev);
    };
    k == 4 ? launch(register_search_kernel<4, ZNCC>) : k == 2 ? launch(register_search_kernel<2, ZNCC>) : launch(register_search_kernel<1, ZNCC>);
    HIP_TRY(hipGetLastError());
    if constexpr (ZNCC)
        hipLaunchKernelGGL(register_zncc_best_kernel, dim3(n_pairs), dim3(REG_THREADS), 0, s, (const long long*)table_dev, search, min_cells,
                           (int*)best_dev, peak_dev);
    else
        hipLaunchKernelGGL(register_best_kernel, dim3(n_pairs), dim3(REG_THREADS), 0, s, (const int*)table_dev, search, min_cells, (int*)best_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_register_search(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search, int side,
                           int min_cells, int32_t* score_dev, int32_t* best_dev, hipStream_t s) {
    return launch_register_search_as<false>("wm_register_search", a_dev, b_dev, pairs_dev, n_pairs, search, side, min_cells, score_dev, best_dev,
                                            nullptr, s);
}

int launch_register_search_zncc(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search,
                                int side, int min_cells, int64_t* moments_dev, int32_t* best_dev, double* peak_dev, hipStream_t s) {
    return launch_register_search_as<true>("wm_register_search_zncc", a_dev, b_dev, pairs_dev, n_pairs, search, side, min_cells, moments_dev,
                                           best_dev, peak_dev, s);
}

// The refinement's sums: one memset and one launch.  B must carry a ring of one cell, so search 0 is refused here.
int launch_register_refine(const uint8_t* a_dev, const uint8_t* b_dev, const wm_register_pair* pairs_dev, int n_pairs, int search, int side,
                           int64_t* sums_dev, hipStream_t s) {
    const char* name = "wm_register_refine";
    if (n_pairs < 0 || n_pairs > WM_REGISTER_MAX_PAIRS) return fail("%s: n_pairs %d outside 0..%d", name, n_pairs, WM_REGISTER_MAX_PAIRS);
    if (n_pairs == 0) return 0;
    if (search < 1 || search > WM_REGISTER_MAX_SEARCH) return fail("%s: search %d outside 1..%d", name, search, WM_REGISTER_MAX_SEARCH);
    WM_TRY(check_register_shape(name, pairs_dev, search, side));
    if (!a_dev) return fail("%s: null a_dev", name);
    if (!b_dev) return fail("%s: null b_dev", name);
    if (!sums_dev) return fail("%s: null sums_dev", name);
    if ((uintptr_t)sums_dev % 8) return fail("%s: sums_dev not 8-byte aligned", name);
    HIP_TRY(hipMemsetAsync(sums_dev, 0, (size_t)n_pairs * REFINE_SUMS * sizeof(*sums_dev), s));
    const int tiles_x = (side + REFINE_TILE_X - 1) / REFINE_TILE_X, tiles_y = (side + REFINE_TILE_Y - 1) / REFINE_TILE_Y;
    hipLaunchKernelGGL(register_refine_kernel, dim3(tiles_x * tiles_y, n_pairs), dim3(REG_THREADS), 0, s, a_dev, b_dev, pairs_dev, search, side,
                       tiles_x, (unsigned long long*)sums_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The pyramid's reduce: one launch, a wave per 64 x 64 tile, LEVEL a template argument so that every level's steps unroll.
int launch_register_reduce(const uint8_t* in_dev, int n_planes, int ext, int level, uint8_t* out_dev, hipStream_t s) {
    const char* name = "wm_register_reduce_u8";
    constexpr int max_ext = WM_REGISTER_MAX_SIDE + 2 * WM_REGISTER_MAX_SEARCH;
    if (n_planes < 0 || n_planes > WM_REGISTER_MAX_PAIRS) return fail("%s: n_planes %d outside 0..%d", name, n_planes, WM_REGISTER_MAX_PAIRS);
    if (n_planes == 0) return 0;
    if (level < 1 || level > WM_REGISTER_MAX_LEVEL) return fail("%s: level %d outside 1..%d", name, level, WM_REGISTER_MAX_LEVEL);
    if (ext < 1 || ext > max_ext) return fail("%s: ext %d outside 1..%d", name, ext, max_ext);
    if (ext % (1 << level)) return fail("%s: ext %d is not a multiple of 2^level = %d", name, ext, 1 << level);
    if (!in_dev) return fail("%s: null in_dev", name);
    if (!out_dev) return fail("%s: null out_dev", name);
    if ((uintptr_t)in_dev % 4) return fail("%s: in_dev not 4-byte aligned", name);
    if ((uintptr_t)out_dev % 4) return fail("%s: out_dev not 4-byte aligned", name);
    const int oe = ext >> level;
    const uintptr_t in0 = (uintptr_t)in_dev, in1 = in0 + (size_t)n_planes * ext * ext, out0 = (uintptr_t)out_dev,
                    out1 = out0 + (size_t)n_planes * oe * oe;
    if (in0 < out1 && out0 < in1) return fail("%s: in_dev and out_dev overlap", name);
    const int tiles_x = (ext + REDUCE_TILE - 1) / REDUCE_TILE, waves = REG_THREADS / 64;
    const dim3 grid((tiles_x * tiles_x + waves - 1) / waves, n_planes);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(REG_THREADS), 0, s, in_dev, ext, tiles_x, out_dev); };
    switch (level) {
        case 1: launch(register_reduce_kernel<1>); break;
        case 2: launch(register_reduce_kernel<2>); break;
        case 3: launch(register_reduce_kernel<3>); break;
        case 4: launch(register_reduce_kernel<4>); break;
        case 5: launch(register_reduce_kernel<5>); break;
        default: launch(register_reduce_kernel<6>); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- survey review chips: one PIL-exact crop per detection, windows and coefficients derived on the device ----
static_assert(CHIP_MAX_SIDE == WM_CHIP_MAX_SIDE, "WM_CHIP_MAX_SIDE");

// the arguments wm_chip_window and wm_crop_chips_u8 share
int check_chip_rule(const char* name, float context, int min_side, int max_side) {
    if (!(context >= 1.f && context <= 8.f)) return fail("%s: context %g outside [1, 8]", name, (double)context);
    if (min_side < 1 || min_side > max_side || max_side > WM_CHIP_MAX_SIDE)
        return fail("%s: min_side %d, max_side %d: need 1 <= min_side <= max_side <= %d", name, min_side, max_side, WM_CHIP_MAX_SIDE);
    return 0;
}

// Weightless and asynchronous: no handle, no scratch, no allocation, no table upload.
int launch_crop_chips(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev, const int32_t* box_frame_dev, int n, int chip,
                      float context, int min_side, int max_side, uint8_t* chips_dev, int32_t* windows_dev, hipStream_t s) {
    const char* name = "wm_crop_chips_u8";
    if (n < 0) return fail("%s: n %d", name, n);
    if (n == 0) return 0;
    if (!frames_dev || !boxes_dev || !chips_dev) return fail("%s: null buffer", name);
    if (n_frames <= 0) return fail("%s: n_frames %d", name, n_frames);
    if (chip < 16 || chip > 256 || chip % 4) return fail("%s: chip %d: need a multiple of 4 in 16..256", name, chip);
    if ((uintptr_t)chips_dev % 4) return fail("%s: chips_dev not 4-byte aligned", name);
    WM_TRY(check_chip_rule(name, context, min_side, max_side));
    const int64_t grid = (int64_t)n * ((chip + CHIP_BAND_ROWS - 1) / CHIP_BAND_ROWS);
    if (grid > INT32_MAX) return fail("%s: n %d chips of %d rows exceed one launch", name, n, chip);
    const int lds = chip_lds_bytes(chip, max_side);           // <= 54 KiB at chip 256, max_side 1024
    hipLaunchKernelGGL(crop_chips_kernel, dim3((unsigned)grid), dim3(256), lds, s, (const frame_desc*)frames_dev, n_frames, boxes_dev,
                       (const int*)box_frame_dev, chip, context, min_side, max_side, chips_dev, (int*)windows_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- survey overlays: box outlines drawn in place, and the reference's tile preparation ----
static_assert(DRAW_MAX_WIDTH == WM_DRAW_MAX_WIDTH && DRAW_MAX_PALETTE == WM_DRAW_MAX_PALETTE, "WM_DRAW_*");
static_assert(PLOT_MAX_PARTS * 2 * sizeof(float) == WM_PLOT_SCRATCH_BYTES, "WM_PLOT_SCRATCH_BYTES");

// Weightless and asynchronous: no handle, no scratch, no allocation.
int launch_draw_boxes(const wm_frame_desc* frames_dev, int n_frames, const float* boxes_dev, const int32_t* labels_dev,
                      const int32_t* box_frame_dev, int n, const uint8_t* palette_dev, int palette_size, int width, hipStream_t s) {
    const char* name = "wm_draw_boxes_u8";
    if (n < 0) return fail("%s: n %d", name, n);
    if (n == 0) return 0;
    if (!frames_dev || !boxes_dev || !labels_dev || !palette_dev) return fail("%s: null buffer", name);
    if (n_frames <= 0) return fail("%s: n_frames %d", name, n_frames);
    if (width < 1 || width > WM_DRAW_MAX_WIDTH) return fail("%s: width %d outside 1..%d", name, width, WM_DRAW_MAX_WIDTH);
    if (palette_size < 1 || palette_size > WM_DRAW_MAX_PALETTE)
        return fail("%s: palette_size %d outside 1..%d", name, palette_size, WM_DRAW_MAX_PALETTE);
    hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)n, DRAW_SLICES), dim3(256), 0, s, (const frame_desc*)frames_dev, n_frames, boxes_dev,
                       (const int*)labels_dev, (const int*)box_frame_dev, n, palette_dev, palette_size, width);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Two launches on `s`: the partial (min, max) pairs of every image into the caller's scratch, then the map.
int launch_plot_image(const float* in_dev, int batch, int height, int width, uint8_t* out_dev, void* scratch_dev, int64_t scratch_bytes,
                      hipStream_t s) {
    const char* name = "wm_plot_image_u8";
    if (batch < 0) return fail("%s: batch %d", name, batch);
    if (batch == 0) return 0;
    if (!in_dev || !out_dev || !scratch_dev) return fail("%s: null buffer", name);
    if (height <= 0 || width <= 0) return fail("%s: height %d, width %d", name, height, width);
    if (batch > 65535) return fail("%s: batch %d exceeds one launch (65535)", name, batch);
    if ((uintptr_t)in_dev % 4 || (uintptr_t)scratch_dev % 4) return fail("%s: in_dev or scratch_dev not 4-byte aligned", name);
    if (scratch_bytes < (int64_t)batch * WM_PLOT_SCRATCH_BYTES)
        return fail("%s: scratch of %lld bytes, %lld needed", name, (long long)scratch_bytes, (long long)batch * WM_PLOT_SCRATCH_BYTES);
    const int64_t hw = (int64_t)height * width;
    const int vec = hw % 4 == 0 && (uintptr_t)in_dev % 16 == 0 && (uintptr_t)out_dev % 4 == 0;
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(PLOT_MAX_PARTS, (3 * hw + 4095) / 4096));
    hipLaunchKernelGGL(plot_minmax_kernel, dim3(parts, batch), dim3(256), 0, s, in_dev, 3 * hw, (float*)scratch_dev, vec);
    HIP_TRY(hipGetLastError());
    const unsigned blocks = grid_for((hw + 3) / 4, 256 * 4, 1024);
    hipLaunchKernelGGL(plot_map_kernel, dim3(blocks, batch), dim3(256), 0, s, in_dev, hw, (const float*)scratch_dev, parts, out_dev, vec);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
