// Stand-alone check of wm_census's host-side argument validation, for a sanitizer build of the host code (no GPU needed:
// every call here returns before the first HIP call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/census_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o census_args_check && ./census_args_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "wm_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAIL: %s (last error: %s)\n", what, wm_last_error()); ++failures; }
}

// Fake device pointers, never dereferenced on these paths.
static int call(int n, double radius, int flags, uintptr_t scratch, int64_t scratch_bytes, int n_frames, uintptr_t buf) {
    void* p = (void*)buf;
    return wm_census((const float*)p, (const float*)p, (const int32_t*)p, (const int32_t*)p, n, (const double*)p, n_frames, radius,
                     flags, (void*)scratch, scratch_bytes, (double*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, nullptr);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    expect(wm_abi_version() == WM_ABI_VERSION, "ABI version");
    expect(wm_census_scratch_bytes(0) >= 0, "scratch bytes of 0");
    expect(wm_census_scratch_bytes(WM_CENSUS_MAX_DETS) > 0, "scratch bytes at the cap");
    expect(wm_census_scratch_bytes(WM_CENSUS_MAX_DETS + 1) < 0, "scratch bytes past the cap");
    expect(wm_census_scratch_bytes(-1) < 0 && wm_census_scratch_bytes(std::numeric_limits<int>::min()) < 0, "scratch bytes of n < 0");
    expect(wm_census_scratch_bytes(std::numeric_limits<int>::max()) < 0, "scratch bytes of INT_MAX");
    const int64_t need = wm_census_scratch_bytes(10);
    expect(wm_census(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nan, -1, nullptr, -1, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr) == 0, "n == 0 returns 0 before any pointer");
    expect(call(-1, 1.0, 0, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "outside"), "n < 0");
    expect(call(WM_CENSUS_MAX_DETS + 1, 1.0, 0, 0x1000, INT64_MAX, 1, 0x2000) < 0, "n past the cap");
    expect(call(std::numeric_limits<int>::max(), 1.0, 0, 0x1000, INT64_MAX, 1, 0x2000) < 0, "n = INT_MAX");
    expect(call(10, 1.0, 0, 0x1000, need, 1, 0) < 0 && std::strstr(wm_last_error(), "null"), "null buffers");
    expect(call(10, 1.0, 0, 0x1000, need, 0, 0x2000) < 0 && std::strstr(wm_last_error(), "n_frames"), "n_frames 0");
    expect(call(10, -1.0, 0, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "radius"), "radius < 0");
    expect(call(10, nan, 0, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "radius"), "radius NaN");
    expect(call(10, inf, 0, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "radius"), "radius inf");
    expect(call(10, 1e200, 0, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "square"), "radius^2 overflows");
    expect(call(10, 1.0, 2, 0x1000, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "flags"), "unknown flag");
    expect(call(10, 1.0, -1, 0x1000, need, 1, 0x2000) < 0, "flags -1");
    expect(call(10, 1.0, 0, 0x1000, need - 1, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "scratch of"), "scratch one byte short");
    expect(call(10, 1.0, 0, 0x1000, -5, 1, 0x2000) < 0, "negative scratch size");
    expect(call(10, 1.0, 0, 0x1008, need, 1, 0x2000) < 0 && std::strstr(wm_last_error(), "aligned"), "misaligned scratch");
    expect(call(10, 1.0, 0, 0x1000, need, 1, 0x2004) < 0 && std::strstr(wm_last_error(), "aligned"), "misaligned boxes / points");
    std::printf(failures ? "census_args_check: %d FAILED\n" : "census_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
