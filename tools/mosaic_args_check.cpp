// Stand-alone check of the host-side argument validation of wm_mosaic_plan / wm_mosaic_fill_u8, for a sanitizer build of the
// host code (no GPU needed: every call here returns before the first HIP call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/mosaic_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o mosaic_args_check && ./mosaic_args_check
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
    uintptr_t frames = 0x1000, g2p = 0x2000, size = 0x3000, source = 0x4000, won = 0x5000, stats = 0x6000, slot = 0x7000, mosaic = 0x8001,
              status = 0x9000;
    int n_frames = 2, n_resident = 2, gx = 5, gy = 3, mode = WM_MOSAIC_BILINEAR, flags = WM_MOSAIC_NORTH_UP;
    double x0 = 0.0, y0 = 0.0, cell = 1.0;
};

static int plan(const Args& a) {
    return wm_mosaic_plan((const double*)a.g2p, (const int32_t*)a.size, a.n_frames, a.x0, a.y0, a.cell, a.gx, a.gy, (int32_t*)a.source,
                          (int32_t*)a.won, (int64_t*)a.stats, nullptr);
}

static int fill(const Args& a) {
    return wm_mosaic_fill_u8((const wm_frame_desc*)a.frames, a.n_resident, (const int32_t*)a.slot, (const double*)a.g2p, (const int32_t*)a.size,
                             a.n_frames, a.x0, a.y0, a.cell, a.gx, a.gy, (const int32_t*)a.source, a.mode, a.flags, (uint8_t*)a.mosaic,
                             (int32_t*)a.status, nullptr);
}

template <class F>
static void both(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(plan(a) < 0 && says(word), what);
    expect(fill(a) < 0 && says(word), what);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    expect(wm_abi_version() == WM_ABI_VERSION, "ABI version");
    both([](Args& a) { a.gx = 0; }, "gx", "gx 0");
    both([&](Args& a) { a.gx = imin; }, "gx", "gx INT_MIN");
    both([](Args& a) { a.gx = WM_COVERAGE_MAX_SIDE + 1; }, "gx", "gx past the cap");
    both([&](Args& a) { a.gx = imax; }, "gx", "gx INT_MAX");
    both([](Args& a) { a.gy = 0; }, "gy", "gy 0");
    both([](Args& a) { a.gy = -1; }, "gy", "gy -1");
    both([&](Args& a) { a.gy = imax; }, "gy", "gy INT_MAX");
    both([](Args& a) { a.gx = WM_COVERAGE_MAX_SIDE; a.gy = WM_COVERAGE_MAX_SIDE; }, "gx * gy", "2^28 cells");
    both([](Args& a) { a.gx = 8192; a.gy = 8193; }, "gx * gy", "one row past 2^26 cells");
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
    both([](Args& a) { a.g2p = 0; }, "g2p_dev", "null g2p");
    both([](Args& a) { a.size = 0; }, "size_dev", "null size");
    both([](Args& a) { a.g2p = 0x2004; }, "aligned", "misaligned g2p");
    both([](Args& a) { a.size = 0x3002; }, "aligned", "misaligned size");
    both([](Args& a) { a.source = 0; }, "source_dev", "null source");
    both([](Args& a) { a.source = 0x4002; }, "aligned", "misaligned source");
    Args a;
    a = Args(); a.won = 0; expect(plan(a) < 0 && says("won_dev"), "null won");
    a = Args(); a.stats = 0; expect(plan(a) < 0 && says("stats_dev"), "null stats");
    a = Args(); a.won = 0x5002; expect(plan(a) < 0 && says("aligned"), "misaligned won");
    a = Args(); a.stats = 0x6004; expect(plan(a) < 0 && says("aligned"), "misaligned stats");
    a = Args(); a.n_resident = -1; expect(fill(a) < 0 && says("n_resident"), "n_resident -1");
    a = Args(); a.n_resident = imin; expect(fill(a) < 0 && says("n_resident"), "n_resident INT_MIN");
    a = Args(); a.n_resident = WM_COVERAGE_MAX_FRAMES + 1; expect(fill(a) < 0 && says("n_resident"), "n_resident past the cap");
    a = Args(); a.n_resident = imax; expect(fill(a) < 0 && says("n_resident"), "n_resident INT_MAX");
    for (int mode : {-1, 2, imax, imin}) { a = Args(); a.mode = mode; expect(fill(a) < 0 && says("mode"), "bad mode"); }
    for (int flags : {2, 3, 4, -1, imin, imax}) { a = Args(); a.flags = flags; expect(fill(a) < 0 && says("flags"), "unknown flags bits"); }
    a = Args(); a.frames = 0; expect(fill(a) < 0 && says("frames_dev"), "null frames");
    a = Args(); a.slot = 0; expect(fill(a) < 0 && says("slot_dev"), "null slot");
    a = Args(); a.mosaic = 0; expect(fill(a) < 0 && says("mosaic_dev"), "null mosaic");
    a = Args(); a.status = 0; expect(fill(a) < 0 && says("status_dev"), "null status");
    a = Args(); a.frames = 0x1004; expect(fill(a) < 0 && says("aligned"), "misaligned frames");
    a = Args(); a.slot = 0x7002; expect(fill(a) < 0 && says("aligned"), "misaligned slot");
    a = Args(); a.status = 0x9002; expect(fill(a) < 0 && says("aligned"), "misaligned status");
    // nothing can be resident: 0 after the checks, before any HIP call
    a = Args(); a.n_resident = 0; a.frames = 0; a.slot = 0; expect(fill(a) == 0, "n_resident == 0 returns 0");
    a = Args(); a.n_frames = 0; a.g2p = 0; a.size = 0; a.frames = 0; a.slot = 0; expect(fill(a) == 0, "n_frames == 0 returns 0");
    a = Args(); a.n_resident = 0; a.mode = 9; expect(fill(a) < 0 && says("mode"), "n_resident == 0 still checks mode");
    std::printf(failures ? "mosaic_args_check: %d FAILED\n" : "mosaic_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
