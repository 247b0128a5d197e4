// Stand-alone check of the host-side argument validation of wm_ortho_u8 (survey terrain), beside rectify_args_check.cpp and
// survey_args_check.cpp: for a sanitizer build of the host code (no GPU needed: every call here returns before the first HIP
// call).  Build and run, from the repository root, as a program of its own:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/ortho_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o ortho_args_check && ./ortho_args_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "wm_hip.h"

static int failures = 0, checks = 0;

static void expect(bool ok, const char* what) {
    ++checks;
    if (!ok) { std::printf("FAIL: %s (last error: %s)\n", what, wm_last_error()); ++failures; }
}

static bool says(const char* word) { return std::strstr(wm_last_error(), word) != nullptr; }

// Fake device pointers, never dereferenced on these paths: a 37 x 53 frame at `in` to a 30 x 40 orthophoto at `out` over an 8 x 8
// DEM at `dem`, the camera 50 m up, rolled 4 and pitched 3 degrees, its picture's up 30 degrees east of north.
struct Args {
    uintptr_t in = 0x100000, out = 0x200000, dem = 0x300000, stats = 0xf000;
    int height = 37, width = 53, dem_height = 8, dem_width = 8, out_height = 30, out_width = 40, mode = WM_MOSAIC_BILINEAR;
    double camera[9] = {50.0, 50.0, 26.0, 18.0, -0.1, 0.01, 0.001, -0.0007, -0.001};
    double pose[12] = {100.0, 200.0, 50.0, 0.86573, -0.49558, -0.06966, -0.52672, -0.84848, -0.05234, -0.03317, 0.08201, -0.99620};
    double dem_geo[3] = {60.0, 240.0, 10.0};
    double out_geo[6] = {0.43301, -0.25, 96.41, -0.25, -0.43301, 211.5};
    uint8_t fill[3] = {9, 8, 7};
    const double *camera_ptr = camera, *pose_ptr = pose, *dem_geo_ptr = dem_geo, *out_geo_ptr = out_geo;
    const uint8_t* fill_ptr = fill;
};

static int ortho(const Args& a) {
    return wm_ortho_u8((const uint8_t*)a.in, a.height, a.width, a.camera_ptr, a.pose_ptr, (const float*)a.dem, a.dem_height, a.dem_width, a.dem_geo_ptr,
                       (uint8_t*)a.out, a.out_height, a.out_width, a.out_geo_ptr, a.mode, a.fill_ptr, (int64_t*)a.stats, nullptr);
}

template <class F>
static void bad(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(ortho(a) < 0 && says("wm_ortho_u8: ") && says(word), what);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    char word[32];
    expect(wm_abi_version() == WM_ABI_VERSION && WM_ABI_VERSION == 13, "ABI version 13");
    bad([](Args& a) { a.in = 0; }, "null in_dev", "null in");
    bad([](Args& a) { a.out = 0; }, "null out_dev", "null out");
    bad([](Args& a) { a.dem = 0; }, "null dem_dev", "null dem");
    bad([](Args& a) { a.camera_ptr = nullptr; }, "null camera", "null camera");
    bad([](Args& a) { a.pose_ptr = nullptr; }, "null pose", "null pose");
    bad([](Args& a) { a.dem_geo_ptr = nullptr; }, "null dem_geo", "null dem_geo");
    bad([](Args& a) { a.out_geo_ptr = nullptr; }, "null out_geo", "null out_geo");
    bad([](Args& a) { a.fill_ptr = nullptr; }, "null fill_rgb", "null fill");
    for (int s : {0, -1, imin, 65537, imax}) {
        bad([&](Args& a) { a.height = s; }, "1..65536", "height outside 1..65536");
        bad([&](Args& a) { a.width = s; }, "1..65536", "width outside 1..65536");
        bad([&](Args& a) { a.out_height = s; }, "1..65536", "out_height outside 1..65536");
        bad([&](Args& a) { a.out_width = s; }, "1..65536", "out_width outside 1..65536");
    }
    for (int s : {1, 0, -1, imin, 32769, imax}) {
        bad([&](Args& a) { a.dem_height = s; }, "2..32768", "dem_height outside 2..32768");
        bad([&](Args& a) { a.dem_width = s; }, "2..32768", "dem_width outside 2..32768");
    }
    const char* const entry[9] = {"camera fx", "camera fy", "camera cx", "camera cy", "camera k1", "camera k2", "camera p1", "camera p2", "camera k3"};
    for (double o : {nan, inf, -inf}) {
        for (int k = 0; k < 9; ++k) bad([&](Args& a) { a.camera[k] = o; }, entry[k], "camera entry not finite");
        for (int k = 0; k < 12; ++k) {
            std::snprintf(word, sizeof word, "pose[%d]", k);
            bad([&](Args& a) { a.pose[k] = o; }, word, "pose entry not finite");
        }
        for (int k = 0; k < 3; ++k) {
            std::snprintf(word, sizeof word, "dem_geo[%d]", k);
            bad([&](Args& a) { a.dem_geo[k] = o; }, word, "dem_geo entry not finite");
        }
        for (int k = 0; k < 6; ++k) {
            std::snprintf(word, sizeof word, "out_geo[%d]", k);
            bad([&](Args& a) { a.out_geo[k] = o; }, word, "out_geo entry not finite");
        }
    }
    for (double o : {0.0, -0.0, -50.0}) {
        bad([&](Args& a) { a.camera[0] = o; }, "camera fx", "fx <= 0");
        bad([&](Args& a) { a.camera[1] = o; }, "camera fy", "fy <= 0");
        bad([&](Args& a) { a.dem_geo[2] = o; }, "dcell", "dcell <= 0");
    }
    for (int m : {-1, 2, imax, imin}) bad([&](Args& a) { a.mode = m; }, "mode", "unknown mode");
    for (uintptr_t off : {1, 4, 7}) bad([&](Args& a) { a.stats = 0xf000 + off; }, "stats_dev not 8-byte aligned", "misaligned stats");
    for (uintptr_t off : {1, 2, 3}) bad([&](Args& a) { a.dem = 0x300000 + off; }, "dem_dev not 4-byte aligned", "misaligned DEM");
    // 37 x 53 x 3 bytes in, 30 x 40 x 3 out, 8 x 8 x 4 of DEM: ranges that meet from either side or nest
    const uintptr_t in_bytes = 37 * 53 * 3, out_bytes = 30 * 40 * 3, dem_bytes = 8 * 8 * 4;
    for (uintptr_t out : {(uintptr_t)0x100000, 0x100000 + in_bytes - 1, 0x100000 - out_bytes + 1, (uintptr_t)0x100100})
        bad([&](Args& a) { a.out = out; }, "in_dev and out_dev overlap", "in and out overlap");
    for (uintptr_t dem : {(uintptr_t)0x200000, 0x200000 + out_bytes - 4, 0x200000 - dem_bytes + 4, (uintptr_t)0x200100})
        bad([&](Args& a) { a.dem = dem; }, "dem_dev and out_dev overlap", "DEM and out overlap");
    // ranges that only touch pass the overlap check: the null frame put in their way is what stops the call
    bad([&](Args& a) { a.dem = 0x200000 - dem_bytes; a.in = 0; }, "null in_dev", "a DEM that ends where the picture begins is not refused");
    // the largest legal shapes pass every size computation before an overlap check stops them: 12.9e9 bytes of picture, 4.3e9 of DEM
    bad([&](Args& a) { a.height = a.width = a.out_height = a.out_width = 65536; a.out = a.in + (uintptr_t)65536 * 65536 * 3 - 1; }, "overlap",
        "largest frames, ranges that touch");
    bad([&](Args& a) { a.dem_height = a.dem_width = 32768; a.dem = 0x40000000; a.out = a.dem + (uintptr_t)32768 * 32768 * 4 - 4; },
        "dem_dev and out_dev overlap", "largest DEM, ranges that touch");
    // an M that is no rotation is the kernel's to take: only finiteness is checked
    bad([&](Args& a) { for (int k = 3; k < 12; ++k) a.pose[k] = 0.0; a.in = 0; }, "null in_dev", "all-zero M is not refused for itself");

    std::printf("ortho_args_check: %d checks, ", checks);
    std::printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
