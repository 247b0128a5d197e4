// Stand-alone check of the host-side argument validation of wm_rectify_u8 (survey attitude), beside survey_args_check.cpp,
// which drives every other survey entry: for a sanitizer build of the host code (no GPU needed: every call here returns
// before the first HIP call).  Build and run, from the repository root, as a program of its own:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/rectify_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o rectify_args_check && ./rectify_args_check
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

// Fake device pointers, never dereferenced on these paths: a 37 x 53 frame at `in` to a 30 x 40 picture at `out`, rolled 4 and
// pitched 3 degrees.
struct Args {
    uintptr_t in = 0x100000, out = 0x200000, stats = 0xf000;
    int height = 37, width = 53, out_height = 30, out_width = 40, mode = WM_MOSAIC_BILINEAR;
    double camera[9] = {50.0, 50.0, 26.0, 18.0, -0.1, 0.01, 0.001, -0.0007, -0.001};
    double rot[9] = {0.99756405, -0.00365077, 0.06966087, 0.0, 0.99862953, 0.05233596, -0.06975647, -0.05220847, 0.99619692};
    double f_out = 50.0;
    uint8_t fill[3] = {9, 8, 7};
    const double *camera_ptr = camera, *rot_ptr = rot;
    const uint8_t* fill_ptr = fill;
};

static int rectify(const Args& a) {
    return wm_rectify_u8((const uint8_t*)a.in, a.height, a.width, a.camera_ptr, a.rot_ptr, (uint8_t*)a.out, a.out_height, a.out_width, a.f_out,
                         a.mode, a.fill_ptr, (int64_t*)a.stats, nullptr);
}

template <class F>
static void bad(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(rectify(a) < 0 && says("wm_rectify_u8: ") && says(word), what);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    expect(wm_abi_version() == WM_ABI_VERSION && WM_ABI_VERSION == 13, "ABI version 13");
    bad([](Args& a) { a.in = 0; }, "null in_dev", "null in");
    bad([](Args& a) { a.out = 0; }, "null out_dev", "null out");
    bad([](Args& a) { a.camera_ptr = nullptr; }, "null camera", "null camera");
    bad([](Args& a) { a.rot_ptr = nullptr; }, "null rot", "null rot");
    bad([](Args& a) { a.fill_ptr = nullptr; }, "null fill_rgb", "null fill");
    for (int s : {0, -1, imin, 65537, imax}) {
        bad([&](Args& a) { a.height = s; }, "1..65536", "height outside 1..65536");
        bad([&](Args& a) { a.width = s; }, "1..65536", "width outside 1..65536");
        bad([&](Args& a) { a.out_height = s; }, "1..65536", "out_height outside 1..65536");
        bad([&](Args& a) { a.out_width = s; }, "1..65536", "out_width outside 1..65536");
    }
    const char* const entry[9] = {"camera fx", "camera fy", "camera cx", "camera cy", "camera k1", "camera k2", "camera p1", "camera p2", "camera k3"};
    const char* const rot_entry[9] = {"rot[0]", "rot[1]", "rot[2]", "rot[3]", "rot[4]", "rot[5]", "rot[6]", "rot[7]", "rot[8]"};
    for (int k = 0; k < 9; ++k)
        for (double o : {nan, inf, -inf}) {
            bad([&](Args& a) { a.camera[k] = o; }, entry[k], "camera entry not finite");
            bad([&](Args& a) { a.rot[k] = o; }, rot_entry[k], "rot entry not finite");
        }
    for (double o : {0.0, -0.0, -50.0}) {
        bad([&](Args& a) { a.camera[0] = o; }, "camera fx", "fx <= 0");
        bad([&](Args& a) { a.camera[1] = o; }, "camera fy", "fy <= 0");
    }
    for (double o : {0.0, -1.0, nan, inf, -inf}) bad([&](Args& a) { a.f_out = o; }, "f_out", "f_out not a finite number > 0");
    for (int m : {-1, 2, imax, imin}) bad([&](Args& a) { a.mode = m; }, "mode", "unknown mode");
    for (uintptr_t off : {1, 4, 7}) bad([&](Args& a) { a.stats = 0xf000 + off; }, "stats_dev not 8-byte aligned", "misaligned stats");
    // 37 x 53 x 3 bytes in, 30 x 40 x 3 out: the two ranges meet from either side or nest
    const uintptr_t in_bytes = 37 * 53 * 3, out_bytes = 30 * 40 * 3;
    for (uintptr_t out : {(uintptr_t)0x100000, 0x100000 + in_bytes - 1, 0x100000 - out_bytes + 1, (uintptr_t)0x100100})
        bad([&](Args& a) { a.out = out; }, "overlap", "in and out overlap");
    // the largest legal shape passes every size computation before the overlap check stops it: 12.9e9 bytes of input reach over out
    bad([&](Args& a) { a.height = a.width = a.out_height = a.out_width = 65536; a.out = a.in + (uintptr_t)65536 * 65536 * 3 - 1; }, "overlap",
        "largest frames, ranges that touch");
    // a rotation that is no rotation is the kernel's to take (the rule is a homography): only finiteness is checked, and a
    // degenerate one with everything else in order gets as far as the null pointer put in its way
    bad([&](Args& a) { for (double& r : a.rot) r = 0.0; a.in = 0; }, "null in_dev", "all-zero rot is not refused for itself");

    std::printf("rectify_args_check: %d checks, ", checks);
    std::printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
