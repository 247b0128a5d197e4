// Stand-alone check of the host-side argument validation of wm_coverage_raster / wm_coverage_points, for a sanitizer build
// of the host code (no GPU needed: every call here returns before the first HIP call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/coverage_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o coverage_args_check && ./coverage_args_check
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
    uintptr_t g2p = 0x2000, size = 0x3000, cov = 0x4000, stats = 0x5000, pts = 0x6000, labels = 0x7000, seen = 0x8000, cidx = 0x9000,
              counts = 0xa000, pstats = 0xb000;
    int n_frames = 2, n_points = 4, gx = 5, gy = 3;
    double x0 = 0.0, y0 = 0.0, cell = 1.0;
};

static int raster(const Args& a) {
    return wm_coverage_raster((const double*)a.g2p, (const int32_t*)a.size, a.n_frames, a.x0, a.y0, a.cell, a.gx, a.gy, (uint16_t*)a.cov,
                              (int64_t*)a.stats, nullptr);
}

static int points(const Args& a) {
    return wm_coverage_points((const double*)a.g2p, (const int32_t*)a.size, a.n_frames, (const double*)a.pts, (const int32_t*)a.labels,
                              a.n_points, a.x0, a.y0, a.cell, a.gx, a.gy, (int32_t*)a.seen, (int32_t*)a.cidx, (int32_t*)a.counts,
                              (int64_t*)a.pstats, nullptr);
}

template <class F>
static void both(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(raster(a) < 0 && says(word), what);
    expect(points(a) < 0 && says(word), what);
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
    Args a;
    a = Args(); a.cov = 0; expect(raster(a) < 0 && says("coverage_dev"), "null coverage");
    a = Args(); a.stats = 0; expect(raster(a) < 0 && says("stats_dev"), "null stats");
    a = Args(); a.cov = 0x4001; expect(raster(a) < 0 && says("aligned"), "misaligned coverage");
    a = Args(); a.stats = 0x5004; expect(raster(a) < 0 && says("aligned"), "misaligned stats");
    a = Args(); a.pts = 0; expect(points(a) < 0 && says("null"), "null points");
    a = Args(); a.labels = 0; expect(points(a) < 0 && says("null"), "null labels");
    a = Args(); a.seen = 0; expect(points(a) < 0 && says("null"), "null seen_by");
    a = Args(); a.cidx = 0; expect(points(a) < 0 && says("null"), "null cell");
    a = Args(); a.pstats = 0; expect(points(a) < 0 && says("null"), "null pstats");
    a = Args(); a.pts = 0x6004; expect(points(a) < 0 && says("aligned"), "misaligned points");
    a = Args(); a.pstats = 0xb004; expect(points(a) < 0 && says("aligned"), "misaligned pstats");
    a = Args(); a.counts = 0xa002; expect(points(a) < 0 && says("aligned"), "misaligned counts");
    a = Args(); a.n_points = -1; expect(points(a) < 0 && says("n_points"), "n_points -1");
    a = Args(); a.n_points = WM_CENSUS_MAX_DETS + 1; expect(points(a) < 0 && says("n_points"), "n_points past the cap");
    a = Args(); a.n_points = imax; expect(points(a) < 0 && says("n_points"), "n_points INT_MAX");
    expect(wm_coverage_points(nullptr, nullptr, -5, nullptr, nullptr, 0, nan, nan, -1.0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0,
           "n_points == 0 returns 0 before any pointer");
    std::printf(failures ? "coverage_args_check: %d FAILED\n" : "coverage_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
