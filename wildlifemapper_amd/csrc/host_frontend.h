// Image front end: the val-transform resize (N1) and the survey resampler, two clients of one plan cache (slots per
// device and stream) and one horizontal launch; and the survey's lens correction, which shares the resampler's size limits.
// The survey launchers are in host_survey.h.
#pragma once
#include <climits>

#include "resample_kernels.h"
#include "attitude_kernels.h"
#include "terrain_kernels.h"
#include "lens_kernels.h"
#include "host_core.h"

namespace {

// augmentation.py:80-99 (get_size_with_aspect_ratio): (w, h), size, max_size -> (oh, ow)
void resized_size(int w, int h, int size, int max_size, int* oh, int* ow) {
    if (max_size > 0) {
        const double mn = (double)std::min(w, h), mx = (double)std::max(w, h);       // Python floats are doubles
        if (mx / mn * size > max_size) size = (int)std::nearbyint(max_size * mn / mx);               // Python round(): half to even
    }
    if ((w <= h && w == size) || (h <= w && h == size)) { *oh = h; *ow = w; return; }
    if (w < h) { *ow = size; *oh = (int)((double)size * h / w); }
    else { *oh = size; *ow = (int)((double)size * w / h); }
}

// Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc, bilinear filter (support 1), whole axis; double arithmetic
// in the same operation order (resample_kernels.h: resize_coeff_row, which crop_chips_kernel runs on the device too)
void resize_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk, int& ksize) {
    const resize_axis ax = resize_axis_of(in_size, out_size);
    ksize = ax.ksize;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    for (int xx = 0; xx < out_size; ++xx)
        resize_coeff_row(ax, in_size, xx, &bounds[(size_t)xx * 2], &bounds[(size_t)xx * 2 + 1], &kk[(size_t)xx * ksize]);
}

// ---- what both callers share: the plan slots of a stream, its intermediate image, the horizontal launch ----
constexpr int RESAMPLE_MAX_SIDE = 65536;       // the merge's fp32 frame coordinates keep sub-0.01 px resolution up to here
constexpr int TERRAIN_MAX_SIDE = 32768;        // posts a side of wm_ortho_u8's DEM: a post index and a row of posts fit an int
constexpr int RESAMPLE_PLAN_SLOTS = 8;         // coefficient tables cached per (device, stream), least recently used evicted

// how the horizontal pass of one geometry runs (resample_h_geometry)
struct ResampleHGeometry {
    bool fast_h = false;                       // on resample_h_cols_kernel
    int opt = 1, lds_h = 0;                    // 256 * opt columns per workgroup, its LDS bytes
};

// One geometry's tables, both axes in one device buffer (bx, kx, by, ky; an unchanged axis has none), uploaded on the
// caller's stream from a pinned copy, so a new geometry neither allocates nor blocks the host: a slot is refilled only
// after the event of its last upload, RESAMPLE_PLAN_SLOTS geometries ago, and the stream orders the device buffer's
// overwrite after every kernel that read it.
struct ResampleSlot {
    std::array<int, 4> key{0, 0, 0, 0};        // (h, w, oh, ow); h == 0: empty
    int ksx = 0, ksy = 0;
    size_t off_kx = 0, off_by = 0, off_ky = 0; // in ints; bx at 0
    int* dev = nullptr;
    int* host = nullptr;
    size_t cap = 0;                            // ints of dev and host
    hipEvent_t copied = nullptr;               // recorded after the upload out of `host`
    ResampleHGeometry hg;
    uint64_t used = 0;
};
// The intermediate (horizontally resampled) image, one per STREAM: calls on different streams of a device may overlap
// on the GPU (a loader thread's side stream), and a shared buffer would be overwritten under the first call's kernels.
struct ResampleTmp { unsigned char* p = nullptr; size_t bytes = 0; };
struct ResampleStreamState {
    ResampleSlot slot[RESAMPLE_PLAN_SLOTS];
    ResampleTmp tmp;
    uint64_t clock = 0;
};
std::map<std::pair<int, hipStream_t>, ResampleStreamState> g_resample;

int resample_tmp_grow(ResampleTmp& tmp, size_t need) {
    if (need <= tmp.bytes) return 0;
    if (tmp.p) HIP_TRY(hipFree(tmp.p));                // hipFree synchronises the device: no kernel still reads the old buffer
    tmp.p = nullptr; tmp.bytes = 0;
    HIP_TRY(hipMalloc((void**)&tmp.p, need));
    tmp.bytes = need;
    return 0;
}

// the column-blocked horizontal kernel: <= 20 taps, and the input span of the widest block of 256 * opt columns fits LDS
void resample_h_geometry(const std::vector<int>& b, int ow, int ks, ResampleHGeometry& g) {
    g.opt = std::min(4, (ow + 255) / 256);
    g.fast_h = false;
    if (ks > 20) return;
    for (int x = 1; x < ow; ++x)
        if (b[2 * x] < b[2 * x - 2] || b[2 * x] + b[2 * x + 1] < b[2 * x - 2] + b[2 * x - 1]) return;
    int span = 0;
    for (int c0 = 0; c0 < ow; c0 += 256 * g.opt) {
        const int c1 = std::min(c0 + 256 * g.opt, ow) - 1;
        span = std::max(span, b[2 * c1] + b[2 * c1 + 1] - b[2 * c0]);
    }
    g.lds_h = (span * 3 + 3 + 3) / 4 * 4 + 64;      // span + alignment shift, + slack for the zero-coefficient taps (KMAX * 3 bytes)
    g.fast_h = g.lds_h <= 64 * 1024;
}

// rows per workgroup of the column-blocked kernel: its coefficient registers are loaded once per workgroup
int resample_rows_per_block(int rows) { return std::max(4, std::min(16, rows / (256 * 8))); }

// the column-blocked kernel's instance: KMAX taps (4 | 12 | 20, the caller has checked ks <= 20), 256 * (1..4) columns per workgroup
template <class F>
void by_taps_cols(int ks, int opt, F&& f) {
    auto cols = [&](auto km) { opt <= 1 ? f(km, int_c<1>{}) : opt <= 2 ? f(km, int_c<2>{}) : opt <= 3 ? f(km, int_c<3>{}) : f(km, int_c<4>{}); };
    ks <= 4 ? cols(int_c<4>{}) : ks <= 12 ? cols(int_c<12>{}) : cols(int_c<20>{});
}

// The horizontal pass of both callers: in [rows, w, 3] -> out [rows, ow, 3], rows = the rows of one frame or of a batch.
int resample_h_launch(const unsigned char* in, unsigned char* out, int rows, int w, int ow, const int* bx, const int* kx, int ksx,
                      const ResampleHGeometry& g, hipStream_t s) {
    if (g.fast_h) {
        const int rpb = resample_rows_per_block(rows);
        const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)((ow + 256 * g.opt - 1) / (256 * g.opt)));
        by_taps_cols(ksx, g.opt, [&](auto km, auto op) {
            hipLaunchKernelGGL((resample_h_cols_kernel<decltype(km)::value, decltype(op)::value>), grid, dim3(256), g.lds_h, s, in, out, bx, kx, ksx,
                               rows, w, ow, rpb);
        });
    } else {                                                           // > 20 taps (scale below ~0.1): one thread per output pixel
        hipLaunchKernelGGL(resize_h_u8_kernel, dim3(grid_for((int64_t)rows * ow)), dim3(256), 0, s, in, out, bx, kx, ksx, 1, rows, w, ow);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int resample_plan(ResampleStreamState& st, int h, int w, int oh, int ow, hipStream_t s, ResampleSlot** out) {
    const std::array<int, 4> key{h, w, oh, ow};
    ResampleSlot* sl = &st.slot[0];
    for (ResampleSlot& c : st.slot) {
        if (c.key == key) { c.used = ++st.clock; *out = &c; return 0; }
        if (c.used < sl->used) sl = &c;
    }
    if (sl->copied) HIP_TRY(hipEventSynchronize(sl->copied));
    else HIP_TRY(hipEventCreateWithFlags(&sl->copied, hipEventDisableTiming));
    std::vector<int> bx, kx, by, ky;
    sl->ksx = sl->ksy = 0;
    if (ow != w) resize_coeffs(w, ow, bx, kx, sl->ksx);
    if (oh != h) resize_coeffs(h, oh, by, ky, sl->ksy);
    sl->off_kx = bx.size();
    sl->off_by = sl->off_kx + kx.size();
    sl->off_ky = sl->off_by + by.size();
    const size_t total = sl->off_ky + ky.size();
    sl->key = {0, 0, 0, 0};
    if (total > sl->cap) {
        if (sl->dev) HIP_TRY(hipFree(sl->dev));            // hipFree synchronises the device: no kernel still reads the old tables
        if (sl->host) HIP_TRY(hipHostFree(sl->host));
        sl->dev = nullptr; sl->host = nullptr; sl->cap = 0;
        HIP_TRY(hipMalloc((void**)&sl->dev, total * 4));
        HIP_TRY(hipHostMalloc((void**)&sl->host, total * 4, hipHostMallocDefault));
        sl->cap = total;
    }
    if (!bx.empty()) memcpy(sl->host, bx.data(), bx.size() * 4);
    if (!kx.empty()) memcpy(sl->host + sl->off_kx, kx.data(), kx.size() * 4);
    if (!by.empty()) memcpy(sl->host + sl->off_by, by.data(), by.size() * 4);
    if (!ky.empty()) memcpy(sl->host + sl->off_ky, ky.data(), ky.size() * 4);
    if (total) HIP_TRY(hipMemcpyAsync(sl->dev, sl->host, total * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(sl->copied, s));
    if (ow != w) resample_h_geometry(bx, ow, sl->ksx, sl->hg);
    sl->key = key;
    sl->used = ++st.clock;
    *out = sl;
    return 0;
}

// ---- N1: val transform resize (PIL bilinear semantics) + normalise + pad ----
// A client of the resampler's state: its tables live in the plan slots of (device, stream), 8 geometries with the least
// recently used evicted, are uploaded on the caller's stream from pinned memory, and a new geometry no longer blocks the
// host (N1 used to keep every geometry for the life of the process, per device, uploaded by a synchronous copy).
// As Pillow does, an unchanged axis has no table and no pass: without a horizontal pass the vertical kernel reads the
// input; without a vertical pass preprocess_u8_kernel normalises and pads the rows it is given.  The bits are those of
// the identity table (coefficients 2^22, 0): clip8((2^21 + 2^22 v) >> 22) = v.  (The val transform's size rule keeps the
// aspect ratio, so it changes both axes or neither; the one-axis cases follow resample_plan's rule all the same.)
// WM_RESIZE_GENERIC=1 (read per call): the generic horizontal and vertical kernels.
int preprocess_resized_impl(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, int oh, int ow, hipStream_t s) {
    if ((int64_t)batch * height > INT_MAX) return fail("wm_preprocess_u8_resized: batch %d x height %d is more than 2^31 - 1 rows", batch, height);
    const int rows = batch * height;
    const char* env = getenv("WM_RESIZE_GENERIC");
    const bool generic = env && atoi(env);
    const unsigned char* src = img_dev;
    ResampleSlot* pl = nullptr;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (ow != width || oh != height) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        ResampleStreamState& st = g_resample[{dev, s}];
        WM_TRY(resample_plan(st, height, width, oh, ow, s, &pl));
        if (ow != width) {
            WM_TRY(resample_tmp_grow(st.tmp, (size_t)batch * height * ow * 3));
            ResampleHGeometry g = pl->hg;
            g.fast_h = g.fast_h && !generic;
            WM_TRY(resample_h_launch(src, st.tmp.p, rows, width, ow, pl->dev, pl->dev + pl->off_kx, pl->ksx, g, s));
            src = st.tmp.p;
        }
    }
    if (oh == height) {
        hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid_for((int64_t)batch * 1024 * 256)), dim3(256), 0, s, src, out_dev, batch, oh, ow);
    } else {
        const int* by = pl->dev + pl->off_by;
        const int* ky = pl->dev + pl->off_ky;
        // four pixels per thread by dword loads: the intermediate image is an allocation of its own; the caller's input may start anywhere
        if (ow % 4 == 0 && !generic && ((uintptr_t)src & 3) == 0)
            hipLaunchKernelGGL(resize_v_normalize4_kernel, dim3((unsigned)batch * 1024u), dim3(256), 0, s, src, out_dev, by, ky, pl->ksy, height, ow, oh);
        else
            hipLaunchKernelGGL(resize_v_normalize_kernel, dim3(grid_for((int64_t)batch * 1024 * 1024)), dim3(256), 0, s, src, out_dev, by, ky, pl->ksy,
                               batch, height, ow, oh);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- survey resampling: any size -> any size, uint8 HWC (PIL bilinear semantics) ----
int resample_impl(const uint8_t* in_dev, int height, int width, uint8_t* out_dev, int out_height, int out_width, hipStream_t s) {
    if (height == out_height && width == out_width) {                  // both of Pillow's passes skipped
        HIP_TRY(hipMemcpyAsync(out_dev, in_dev, (size_t)height * width * 3, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_dev_mu);
    ResampleStreamState& st = g_resample[{dev, s}];
    ResampleSlot* pl = nullptr;
    WM_TRY(resample_plan(st, height, width, out_height, out_width, s, &pl));
    const unsigned char* src = in_dev;
    if (out_width != width) {
        unsigned char* dst = out_dev;                                  // no vertical pass: straight into the output
        if (out_height != height) {
            WM_TRY(resample_tmp_grow(st.tmp, (size_t)height * out_width * 3));
            dst = st.tmp.p;
        }
        WM_TRY(resample_h_launch(in_dev, dst, height, width, out_width, pl->dev, pl->dev + pl->off_kx, pl->ksx, pl->hg, s));
        src = dst;
    }
    if (out_height != height) {
        hipLaunchKernelGGL(resample_v_u8_kernel, dim3((unsigned)out_height), dim3(256), 0, s, src, out_dev, (const int*)(pl->dev + pl->off_by),
                           (const int*)(pl->dev + pl->off_ky), pl->ksy, (int64_t)out_width * 3);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---- survey lens and attitude: a frame -> the pinhole picture of its camera (include/wm_hip.h "Survey lens"), or of a level
// camera at the same place ("Survey attitude") ----
// Every argument is checked on the host before the first HIP call; one memset of the optional count and one launch.
// rot == nullptr: wm_undistort_u8, which has no rotation.
int check_lens_args(const char* name, const uint8_t* in_dev, int height, int width, const double* camera, const double* rot, bool has_rot,
                    uint8_t* out_dev, int out_height, int out_width, double f_out, int mode, const uint8_t* fill_rgb, int64_t* stats_dev) {
    static const char* const entry[9] = {"fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"};
    if (!in_dev) return fail("%s: null in_dev", name);
    if (!out_dev) return fail("%s: null out_dev", name);
    if (!camera) return fail("%s: null camera", name);
    if (has_rot && !rot) return fail("%s: null rot", name);
    if (!fill_rgb) return fail("%s: null fill_rgb", name);
    for (int v : {height, width, out_height, out_width})
        if (v < 1 || v > RESAMPLE_MAX_SIDE)
            return fail("%s: %dx%d -> %dx%d, sides must be in 1..%d", name, height, width, out_height, out_width, RESAMPLE_MAX_SIDE);
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(camera[k])) return fail("%s: camera %s %g is not finite", name, entry[k], camera[k]);
    if (!(camera[0] > 0.0)) return fail("%s: camera fx %g: need a focal length > 0", name, camera[0]);
    if (!(camera[1] > 0.0)) return fail("%s: camera fy %g: need a focal length > 0", name, camera[1]);
    if (has_rot)
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(rot[k])) return fail("%s: rot[%d] %g is not finite", name, k, rot[k]);
    if (!(std::isfinite(f_out) && f_out > 0.0)) return fail("%s: f_out %g: need a finite focal length > 0", name, f_out);
    if (mode != WM_MOSAIC_NEAREST && mode != WM_MOSAIC_BILINEAR) return fail("%s: mode %d is neither WM_MOSAIC_NEAREST nor WM_MOSAIC_BILINEAR", name, mode);
    if ((uintptr_t)stats_dev % 8) return fail("%s: stats_dev not 8-byte aligned", name);
    const uintptr_t in0 = (uintptr_t)in_dev, in1 = in0 + (size_t)height * width * 3, out0 = (uintptr_t)out_dev,
                    out1 = out0 + (size_t)out_height * out_width * 3;
    if (in0 < out1 && out0 < in1) return fail("%s: in_dev and out_dev overlap", name);
    return 0;
}

int launch_undistort(const uint8_t* in_dev, int height, int width, const double* camera, uint8_t* out_dev, int out_height, int out_width,
                     double f_out, int mode, const uint8_t* fill_rgb, int64_t* stats_dev, hipStream_t s) {
    WM_TRY(check_lens_args("wm_undistort_u8", in_dev, height, width, camera, nullptr, false, out_dev, out_height, out_width, f_out, mode, fill_rgb,
                           stats_dev));
    if (stats_dev) HIP_TRY(hipMemsetAsync(stats_dev, 0, sizeof(int64_t), s));
    const frame_desc in{in_dev, height, width};
    const lens_camera cam{camera[0], camera[1], camera[2], camera[3], camera[4], camera[5], camera[6], camera[7], camera[8]};
    const unsigned int fill = (unsigned int)fill_rgb[0] | (unsigned int)fill_rgb[1] << 8 | (unsigned int)fill_rgb[2] << 16;
    const dim3 grid((out_width + COV_BLOCK_X - 1) / COV_BLOCK_X, (out_height + MOS_FILL_BLOCK_Y - 1) / MOS_FILL_BLOCK_Y);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(COV_THREADS), 0, s, in, cam, f_out, out_height, out_width, fill, out_dev,
                           (unsigned long long*)stats_dev);
    };
    mode == WM_MOSAIC_NEAREST ? launch(lens_undistort_kernel<WM_MOSAIC_NEAREST>) : launch(lens_undistort_kernel<WM_MOSAIC_BILINEAR>);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rectify(const uint8_t* in_dev, int height, int width, const double* camera, const double* rot, uint8_t* out_dev, int out_height,
                   int out_width, double f_out, int mode, const uint8_t* fill_rgb, int64_t* stats_dev, hipStream_t s) {
    WM_TRY(check_lens_args("wm_rectify_u8", in_dev, height, width, camera, rot, true, out_dev, out_height, out_width, f_out, mode, fill_rgb,
                           stats_dev));
    if (stats_dev) HIP_TRY(hipMemsetAsync(stats_dev, 0, sizeof(int64_t), s));
    const frame_desc in{in_dev, height, width};
    const lens_camera cam{camera[0], camera[1], camera[2], camera[3], camera[4], camera[5], camera[6], camera[7], camera[8]};
    const attitude_rot r{rot[0], rot[1], rot[2], rot[3], rot[4], rot[5], rot[6], rot[7], rot[8]};
    const unsigned int fill = (unsigned int)fill_rgb[0] | (unsigned int)fill_rgb[1] << 8 | (unsigned int)fill_rgb[2] << 16;
    const dim3 grid((out_width + COV_BLOCK_X - 1) / COV_BLOCK_X, (out_height + MOS_FILL_BLOCK_Y - 1) / MOS_FILL_BLOCK_Y);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(COV_THREADS), 0, s, in, cam, r, f_out, out_height, out_width, fill, out_dev,
                           (unsigned long long*)stats_dev);
    };
    mode == WM_MOSAIC_NEAREST ? launch(attitude_rectify_kernel<WM_MOSAIC_NEAREST>) : launch(attitude_rectify_kernel<WM_MOSAIC_BILINEAR>);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- survey terrain: a frame -> its orthophoto over a height grid (include/wm_hip.h "Survey terrain") ----
// The frame, camera, picture, mode, fill, alignment and overlap checks are check_lens_args' (an orthophoto has no f_out of its
// own: the output grid is out_geo); then pose, the DEM and out_geo.  One memset of the optional counts and one launch.
int launch_ortho(const uint8_t* in_dev, int height, int width, const double* camera, const double* pose, const float* dem_dev, int dem_height,
                 int dem_width, const double* dem_geo, uint8_t* out_dev, int out_height, int out_width, const double* out_geo, int mode,
                 const uint8_t* fill_rgb, int64_t* stats_dev, hipStream_t s) {
    const char* name = "wm_ortho_u8";
    WM_TRY(check_lens_args(name, in_dev, height, width, camera, nullptr, false, out_dev, out_height, out_width, 1.0, mode, fill_rgb, stats_dev));
    if (!pose) return fail("%s: null pose", name);
    if (!dem_dev) return fail("%s: null dem_dev", name);
    if (!dem_geo) return fail("%s: null dem_geo", name);
    if (!out_geo) return fail("%s: null out_geo", name);
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose[k])) return fail("%s: pose[%d] %g is not finite", name, k, pose[k]);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(dem_geo[k])) return fail("%s: dem_geo[%d] %g is not finite", name, k, dem_geo[k]);
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(out_geo[k])) return fail("%s: out_geo[%d] %g is not finite", name, k, out_geo[k]);
    if (!(dem_geo[2] > 0.0)) return fail("%s: dem_geo[2] (dcell) %g: need a post spacing > 0", name, dem_geo[2]);
    if (dem_height < 2 || dem_height > TERRAIN_MAX_SIDE || dem_width < 2 || dem_width > TERRAIN_MAX_SIDE)
        return fail("%s: dem_height %d, dem_width %d: the DEM's sides must be in 2..%d", name, dem_height, dem_width, TERRAIN_MAX_SIDE);
    if ((uintptr_t)dem_dev % 4) return fail("%s: dem_dev not 4-byte aligned", name);
    const uintptr_t dem0 = (uintptr_t)dem_dev, dem1 = dem0 + (size_t)dem_height * dem_width * sizeof(float), out0 = (uintptr_t)out_dev,
                    out1 = out0 + (size_t)out_height * out_width * 3;
    if (dem0 < out1 && out0 < dem1) return fail("%s: dem_dev and out_dev overlap", name);
    if (stats_dev) HIP_TRY(hipMemsetAsync(stats_dev, 0, 2 * sizeof(int64_t), s));
    const frame_desc in{in_dev, height, width};
    const lens_camera cam{camera[0], camera[1], camera[2], camera[3], camera[4], camera[5], camera[6], camera[7], camera[8]};
    const terrain_pose ps{pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], pose[6], pose[7], pose[8], pose[9], pose[10], pose[11]};
    const terrain_dem dem{dem_dev, dem_height, dem_width, dem_geo[0], dem_geo[1], dem_geo[2]};
    const terrain_geo geo{out_geo[0], out_geo[1], out_geo[2], out_geo[3], out_geo[4], out_geo[5]};
    const unsigned int fill = (unsigned int)fill_rgb[0] | (unsigned int)fill_rgb[1] << 8 | (unsigned int)fill_rgb[2] << 16;
    const dim3 grid((out_width + COV_BLOCK_X - 1) / COV_BLOCK_X, (out_height + MOS_FILL_BLOCK_Y - 1) / MOS_FILL_BLOCK_Y);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(COV_THREADS), 0, s, in, cam, ps, dem, geo, out_height, out_width, fill, out_dev,
                           (unsigned long long*)stats_dev);
    };
    mode == WM_MOSAIC_NEAREST ? launch(terrain_ortho_kernel<WM_MOSAIC_NEAREST>) : launch(terrain_ortho_kernel<WM_MOSAIC_BILINEAR>);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
