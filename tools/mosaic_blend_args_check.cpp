// Stand-alone check of the host-side argument validation of wm_mosaic_blend_plan / wm_mosaic_blend_accum_u8 /
// wm_mosaic_blend_finish_u8, for a sanitizer build of the host code (no GPU needed: every call here returns before the first
// HIP call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/mosaic_blend_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o mosaic_blend_args_check && ./mosaic_blend_args_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "wm_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAIL: %s (last error: %s)\n", what, wm_last_error()); ++failures; }
}

static bool says(const char* word) { return std::strstr(wm_last_error(), word) != nullptr; }

// Fake device pointers, never dereferenced on these paths.
struct Args {
    uintptr_t frames = 0x1000, g2p = 0x2000, size = 0x3000, best = 0x4000, cells = 0x5000, stats = 0x6000, index = 0x7000, acc = 0x8000,
              status = 0x9000, exposure = 0xA000, mosaic = 0xB001;
    int n_frames = 2, n_resident = 2, gx = 5, gy = 3, mode = WM_MOSAIC_BILINEAR, flags = WM_MOSAIC_NORTH_UP;
    double x0 = 0.0, y0 = 0.0, cell = 1.0, band = 8.0;
};

static int plan(const Args& a) {
    return wm_mosaic_blend_plan((const double*)a.g2p, (const int32_t*)a.size, a.n_frames, a.x0, a.y0, a.cell, a.gx, a.gy, a.band, (double*)a.best,
                                (int32_t*)a.cells, (int64_t*)a.stats, nullptr);
}

static int accum(const Args& a) {
    return wm_mosaic_blend_accum_u8((const wm_frame_desc*)a.frames, (const int32_t*)a.index, a.n_resident, (const double*)a.g2p,
                                    (const int32_t*)a.size, a.n_frames, (const int32_t*)a.exposure, a.x0, a.y0, a.cell, a.gx, a.gy, a.band,
                                    (const double*)a.best, a.mode, (uint32_t*)a.acc, (int32_t*)a.status, nullptr);
}

static int finish(const Args& a) { return wm_mosaic_blend_finish_u8((const uint32_t*)a.acc, a.gx, a.gy, a.flags, (uint8_t*)a.mosaic, nullptr); }

template <class F>
static void all_three(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(plan(a) < 0 && says(word), what);
    expect(accum(a) < 0 && says(word), what);
    expect(finish(a) < 0 && says(word), what);
}

template <class F>
static void both(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(plan(a) < 0 && says(word), what);
    expect(accum(a) < 0 && says(word), what);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    expect(wm_abi_version() == WM_ABI_VERSION, "ABI version");
    all_three([](Args& a) { a.gx = 0; }, "gx", "gx 0");
    all_three([&](Args& a) { a.gx = imin; }, "gx", "gx INT_MIN");
    all_three([](Args& a) { a.gx = WM_COVERAGE_MAX_SIDE + 1; }, "gx", "gx past the cap");
    all_three([&](Args& a) { a.gx = imax; }, "gx", "gx INT_MAX");
    all_three([](Args& a) { a.gy = 0; }, "gy", "gy 0");
    all_three([](Args& a) { a.gy = -1; }, "gy", "gy -1");
    all_three([&](Args& a) { a.gy = imax; }, "gy", "gy INT_MAX");
    all_three([](Args& a) { a.gx = WM_COVERAGE_MAX_SIDE; a.gy = WM_COVERAGE_MAX_SIDE; }, "gx * gy", "2^28 cells");
    all_three([](Args& a) { a.gx = 8192; a.gy = 8193; }, "gx * gy", "one row past 2^26 cells");
    both([](Args& a) { a.n_frames = -1; }, "n_frames", "n_frames -1");
    both([](Args& a) { a.n_frames = WM_COVERAGE_MAX_FRAMES + 1; }, "n_frames", "n_frames past the cap");
    both([&](Args& a) { a.n_frames = imax; }, "n_frames", "n_frames INT_MAX");
    both([&](Args& a) { a.n_frames = imin; }, "n_frames", "n_frames INT_MIN");
    both([&](Args& a) { a.x0 = nan; }, "x0", "x0 NaN");
    both([&](Args& a) { a.x0 = -inf; }, "x0", "x0 -inf");
    both([&](Args& a) { a.y0 = nan; }, "y0", "y0 NaN");
    both([&](Args& a) { a.y0 = inf; }, "y0", "y0 inf");
    both([](Args& a) { a.cell = 0.0; }, "cell", "cell 0");
    both([](Args& a) { a.cell = -0.5; }, "cell", "cell < 0");
    both([&](Args& a) { a.cell = nan; }, "cell", "cell NaN");
    both([&](Args& a) { a.cell = inf; }, "cell", "cell inf");
    both([](Args& a) { a.band = 0.0; }, "band", "band 0");
    both([](Args& a) { a.band = -0.0; }, "band", "band -0");
    both([](Args& a) { a.band = -8.0; }, "band", "band < 0");
    both([&](Args& a) { a.band = nan; }, "band", "band NaN");
    both([&](Args& a) { a.band = inf; }, "band", "band inf");
    both([&](Args& a) { a.band = -inf; }, "band", "band -inf");
    both([](Args& a) { a.band = std::numeric_limits<double>::denorm_min(); }, "band", "band so small that 256 / band overflows");
    both([](Args& a) { a.g2p = 0; }, "g2p_dev", "null g2p");
    both([](Args& a) { a.size = 0; }, "size_dev", "null size");
    both([](Args& a) { a.g2p = 0x2004; }, "aligned", "misaligned g2p");
    both([](Args& a) { a.size = 0x3002; }, "aligned", "misaligned size");
    both([](Args& a) { a.best = 0; }, "best_dev", "null best");
    both([](Args& a) { a.best = 0x4004; }, "aligned", "misaligned best");
    Args a;
    a = Args(); a.cells = 0; expect(plan(a) < 0 && says("cells_dev"), "null cells");
    a = Args(); a.stats = 0; expect(plan(a) < 0 && says("stats_dev"), "null stats");
    a = Args(); a.cells = 0x5002; expect(plan(a) < 0 && says("aligned"), "misaligned cells");
    a = Args(); a.stats = 0x6004; expect(plan(a) < 0 && says("aligned"), "misaligned stats");
    a = Args(); a.n_resident = -1; expect(accum(a) < 0 && says("n_resident"), "n_resident -1");
    a = Args(); a.n_resident = imin; expect(accum(a) < 0 && says("n_resident"), "n_resident INT_MIN");
    a = Args(); a.n_resident = WM_COVERAGE_MAX_FRAMES + 1; expect(accum(a) < 0 && says("n_resident"), "n_resident past the cap");
    a = Args(); a.n_resident = imax; expect(accum(a) < 0 && says("n_resident"), "n_resident INT_MAX");
    for (int mode : {-1, 2, imax, imin}) { a = Args(); a.mode = mode; expect(accum(a) < 0 && says("mode"), "bad mode"); }
    a = Args(); a.frames = 0; expect(accum(a) < 0 && says("frames_dev"), "null frames");
    a = Args(); a.index = 0; expect(accum(a) < 0 && says("index_dev"), "null index");
    a = Args(); a.acc = 0; expect(accum(a) < 0 && says("acc_dev"), "null acc");
    a = Args(); a.status = 0; expect(accum(a) < 0 && says("status_dev"), "null status");
    a = Args(); a.frames = 0x1004; expect(accum(a) < 0 && says("aligned"), "misaligned frames");
    a = Args(); a.index = 0x7002; expect(accum(a) < 0 && says("aligned"), "misaligned index");
    a = Args(); a.exposure = 0xA002; expect(accum(a) < 0 && says("aligned"), "misaligned exposure");
    a = Args(); a.acc = 0x8002; expect(accum(a) < 0 && says("aligned"), "misaligned acc");
    a = Args(); a.status = 0x9002; expect(accum(a) < 0 && says("aligned"), "misaligned status");
    // no frame to walk: 0 after the checks, before any HIP call; the exposure table may be NULL
    a = Args(); a.n_resident = 0; a.frames = 0; a.index = 0; expect(accum(a) == 0, "n_resident == 0 returns 0");
    a = Args(); a.n_resident = 0; a.frames = 0; a.index = 0; a.exposure = 0; expect(accum(a) == 0, "n_resident == 0 and no table returns 0");
    a = Args(); a.n_resident = 0; a.mode = 9; expect(accum(a) < 0 && says("mode"), "n_resident == 0 still checks mode");
    a = Args(); a.n_resident = 0; a.band = 0.0; expect(accum(a) < 0 && says("band"), "n_resident == 0 still checks band");
    a = Args(); a.n_resident = 0; a.acc = 0; expect(accum(a) < 0 && says("acc_dev"), "n_resident == 0 still checks acc");
    for (int flags : {2, 3, 4, -1, imin, imax}) { a = Args(); a.flags = flags; expect(finish(a) < 0 && says("flags"), "unknown flags bits"); }
    a = Args(); a.acc = 0; expect(finish(a) < 0 && says("acc_dev"), "finish: null acc");
    a = Args(); a.mosaic = 0; expect(finish(a) < 0 && says("mosaic_dev"), "finish: null mosaic");
    a = Args(); a.acc = 0x8002; expect(finish(a) < 0 && says("aligned"), "finish: misaligned acc");
    std::printf(failures ? "mosaic_blend_args_check: %d FAILED\n" : "mosaic_blend_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
