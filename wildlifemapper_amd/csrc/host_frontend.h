// Image front end: the val-transform resize (plan cache per device) and the survey resampler (plan slots per stream).
// The survey launchers are in host_survey.h.
#pragma once
#include "misc_kernels.h"
#include "resample_kernels.h"
#include "host_core.h"

namespace {

// ---- N1: val transform resize (PIL bilinear semantics) + normalise + pad ----
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

// the row / column-blocked horizontal kernels' instance: KMAX taps (4 | 12 | 20, the caller has checked ks <= 20), 256 * (1..4) columns per workgroup
template <class F>
void by_taps_cols(int ks, int opt, F&& f) {
    auto cols = [&](auto km) { opt <= 1 ? f(km, int_c<1>{}) : opt <= 2 ? f(km, int_c<2>{}) : opt <= 3 ? f(km, int_c<3>{}) : f(km, int_c<4>{}); };
    ks <= 4 ? cols(int_c<4>{}) : ks <= 12 ? cols(int_c<12>{}) : cols(int_c<20>{});
}

struct ResizePlan {          // device tables of one geometry; owned by the library for the life of the process
    int oh = 0, ow = 0, ksx = 0, ksy = 0;
    int *bx = nullptr, *kx = nullptr, *by = nullptr, *ky = nullptr;
};
struct ResizeTmp { unsigned char* p = nullptr; size_t bytes = 0; };
struct ResizeDevState {
    std::map<std::array<int, 4>, ResizePlan> plans;      // (h, w, size, max_size); read-only once built
    // the intermediate (horizontally resampled) image, one per STREAM: calls on different streams of a device may overlap
    // on the GPU (a loader thread's side stream), and a shared buffer would be overwritten under the first call's kernels
    std::map<hipStream_t, ResizeTmp> tmp;
};
std::map<int, ResizeDevState> g_resize;

int upload_ints(const std::vector<int>& v, int** out) {
    HIP_TRY(hipMalloc((void**)out, v.size() * 4));
    HIP_TRY(hipMemcpy(*out, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

int preprocess_resized_impl(const uint8_t* img_dev, float* out_dev, int batch, int height, int width, int size, int max_size, int oh, int ow,
                            hipStream_t s) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_dev_mu);
    ResizeDevState& st = g_resize[dev];
    const std::array<int, 4> key{height, width, size, max_size};
    auto it = st.plans.find(key);
    if (it == st.plans.end()) {
        ResizePlan pl;
        pl.oh = oh; pl.ow = ow;
        std::vector<int> b, k;
        resize_coeffs(width, ow, b, k, pl.ksx);
        WM_TRY(upload_ints(b, &pl.bx)); WM_TRY(upload_ints(k, &pl.kx));
        resize_coeffs(height, oh, b, k, pl.ksy);
        WM_TRY(upload_ints(b, &pl.by)); WM_TRY(upload_ints(k, &pl.ky));
        it = st.plans.emplace(key, pl).first;
    }
    const ResizePlan& pl = it->second;
    const size_t need = (size_t)batch * height * ow * 3;
    ResizeTmp& tmp = st.tmp[s];
    if (need > tmp.bytes) {
        if (tmp.p) HIP_TRY(hipFree(tmp.p));              // hipFree synchronises the device: no kernel still reads the old buffer
        tmp.p = nullptr; tmp.bytes = 0;
        HIP_TRY(hipMalloc((void**)&tmp.p, need));
        tmp.bytes = need;
    }
    // horizontal pass: the row-staged kernel where its geometry holds (<= 20 taps, <= 1024 output columns, a row fits LDS), else the generic one
    const int64_t rows_total = (int64_t)batch * height;
    const int lds_h = ((width * 3 + 3 + 3) / 4 + 1) * 4 + 64;      // row + alignment shift, + slack for the zero-coefficient taps (KMAX * 3 bytes)
    const bool fast_h = pl.ksx <= 20 && ow <= 1024 && lds_h <= 64 * 1024 && !(getenv("WM_RESIZE_GENERIC") && atoi(getenv("WM_RESIZE_GENERIC")));
    if (fast_h) {
        const int rpb = (int)std::max<int64_t>(4, std::min<int64_t>(16, rows_total / (256 * 8)));     // rows per workgroup: the coefficient registers are loaded once per workgroup
        const dim3 grid((unsigned)((rows_total + rpb - 1) / rpb));
        const int64_t in_bytes = rows_total * width * 3;
        by_taps_cols(pl.ksx, (ow + 255) / 256, [&](auto km, auto op) {
            hipLaunchKernelGGL((resize_h_rows_kernel<decltype(km)::value, decltype(op)::value>), grid, dim3(256), lds_h, s, img_dev, tmp.p, (const int*)pl.bx,
                               (const int*)pl.kx, pl.ksx, rows_total, width, ow, rpb, in_bytes);
        });
    } else {
        hipLaunchKernelGGL(resize_h_u8_kernel, dim3(grid_for((int64_t)batch * height * ow)), dim3(256), 0, s, img_dev, tmp.p, (const int*)pl.bx,
                           (const int*)pl.kx, pl.ksx, batch, height, width, ow);
    }
    if (ow % 4 == 0 && !(getenv("WM_RESIZE_GENERIC") && atoi(getenv("WM_RESIZE_GENERIC"))))
        hipLaunchKernelGGL(resize_v_normalize4_kernel, dim3((unsigned)batch * 1024u), dim3(256), 0, s, (const unsigned char*)tmp.p, out_dev,
                           (const int*)pl.by, (const int*)pl.ky, pl.ksy, height, ow, oh);
    else
        hipLaunchKernelGGL(resize_v_normalize_kernel, dim3(grid_for((int64_t)batch * 1024 * 1024)), dim3(256), 0, s, (const unsigned char*)tmp.p, out_dev,
                           (const int*)pl.by, (const int*)pl.ky, pl.ksy, batch, height, ow, oh);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- survey resampling: any size -> any size, uint8 HWC (PIL bilinear semantics) ----
constexpr int RESAMPLE_MAX_SIDE = 65536;       // the merge's fp32 frame coordinates keep sub-0.01 px resolution up to here
constexpr int RESAMPLE_PLAN_SLOTS = 8;         // coefficient tables cached per (device, stream), least recently used evicted

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
    bool fast_h = false;                       // horizontal pass on resample_h_cols_kernel
    int opt = 1, lds_h = 0;
    uint64_t used = 0;
};
struct ResampleStreamState {
    ResampleSlot slot[RESAMPLE_PLAN_SLOTS];
    ResizeTmp tmp;                             // the horizontally resampled image
    uint64_t clock = 0;
};
std::map<std::pair<int, hipStream_t>, ResampleStreamState> g_resample;

// the column-blocked horizontal kernel: <= 20 taps, and the input span of the widest block of 256 * opt columns fits LDS
void resample_h_geometry(const std::vector<int>& b, int ow, int ks, ResampleSlot& sl) {
    sl.opt = std::min(4, (ow + 255) / 256);
    sl.fast_h = false;
    if (ks > 20) return;
    for (int x = 1; x < ow; ++x)
        if (b[2 * x] < b[2 * x - 2] || b[2 * x] + b[2 * x + 1] < b[2 * x - 2] + b[2 * x - 1]) return;
    int span = 0;
    for (int c0 = 0; c0 < ow; c0 += 256 * sl.opt) {
        const int c1 = std::min(c0 + 256 * sl.opt, ow) - 1;
        span = std::max(span, b[2 * c1] + b[2 * c1 + 1] - b[2 * c0]);
    }
    sl.lds_h = (span * 3 + 3 + 3) / 4 * 4 + 64;     // span + alignment shift, + slack for the zero-coefficient taps (KMAX * 3 bytes)
    sl.fast_h = sl.lds_h <= 64 * 1024;
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
    if (ow != w) resample_h_geometry(bx, ow, sl->ksx, *sl);
    sl->key = key;
    sl->used = ++st.clock;
    *out = sl;
    return 0;
}

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
            const size_t need = (size_t)height * out_width * 3;
            if (need > st.tmp.bytes) {
                if (st.tmp.p) HIP_TRY(hipFree(st.tmp.p));              // hipFree synchronises the device
                st.tmp.p = nullptr; st.tmp.bytes = 0;
                HIP_TRY(hipMalloc((void**)&st.tmp.p, need));
                st.tmp.bytes = need;
            }
            dst = st.tmp.p;
        }
        const int* bx = pl->dev;
        const int* kx = pl->dev + pl->off_kx;
        if (pl->fast_h) {
            const int rpb = std::max(4, std::min(16, height / (256 * 8)));
            const dim3 grid((unsigned)((height + rpb - 1) / rpb), (unsigned)((out_width + 256 * pl->opt - 1) / (256 * pl->opt)));
            by_taps_cols(pl->ksx, pl->opt, [&](auto km, auto op) {
                hipLaunchKernelGGL((resample_h_cols_kernel<decltype(km)::value, decltype(op)::value>), grid, dim3(256), pl->lds_h, s, in_dev, dst, bx, kx, pl->ksx,
                                   height, width, out_width, rpb);
            });
        } else {                                                       // > 20 taps (scale below ~0.1): one thread per output pixel
            hipLaunchKernelGGL(resize_h_u8_kernel, dim3(grid_for((int64_t)height * out_width)), dim3(256), 0, s, in_dev, dst, bx, kx, pl->ksx,
                               1, height, width, out_width);
        }
        HIP_TRY(hipGetLastError());
        src = dst;
    }
    if (out_height != height) {
        hipLaunchKernelGGL(resample_v_u8_kernel, dim3((unsigned)out_height), dim3(256), 0, s, src, out_dev, (const int*)(pl->dev + pl->off_by),
                           (const int*)(pl->dev + pl->off_ky), pl->ksy, (int64_t)out_width * 3);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace
