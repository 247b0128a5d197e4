// Stand-alone check of the host-side argument validation of wm_register_search_zncc, for a sanitizer build of the host code
// (no GPU needed: every call here returns before the first HIP call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/register_zncc_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o register_zncc_args_check && ./register_zncc_args_check
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
    uintptr_t pairs = 0x4000, a = 0x5001, b = 0x6003, moments = 0x8000, best = 0xa000, peak = 0xb000;
    int n_pairs = 3, search = 4, side = 64, min_cells = 1;
};

static int search(const Args& a) {
    return wm_register_search_zncc((const uint8_t*)a.a, (const uint8_t*)a.b, (const wm_register_pair*)a.pairs, a.n_pairs, a.search, a.side,
                                   a.min_cells, (int64_t*)a.moments, (int32_t*)a.best, (double*)a.peak, nullptr);
}

template <class F>
static void bad(F change, const char* word, const char* what) {
    Args a;
    change(a);
    expect(search(a) < 0 && says("wm_register_search_zncc") && says(word), what);
}

int main() {
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    expect(wm_abi_version() == WM_ABI_VERSION && WM_ABI_VERSION == 13, "ABI version 13");
    bad([](Args& a) { a.n_pairs = -1; }, "n_pairs", "n_pairs -1");
    bad([&](Args& a) { a.n_pairs = imin; }, "n_pairs", "n_pairs INT_MIN");
    bad([](Args& a) { a.n_pairs = WM_REGISTER_MAX_PAIRS + 1; }, "n_pairs", "n_pairs past the cap");
    bad([&](Args& a) { a.n_pairs = imax; }, "n_pairs", "n_pairs INT_MAX");
    bad([](Args& a) { a.search = -1; }, "search", "search -1");
    bad([&](Args& a) { a.search = imin; }, "search", "search INT_MIN");
    bad([](Args& a) { a.search = WM_REGISTER_MAX_SEARCH + 1; }, "search", "search past the cap");
    bad([&](Args& a) { a.search = imax; }, "search", "search INT_MAX");
    bad([](Args& a) { a.side = 0; }, "side", "side 0");
    bad([](Args& a) { a.side = -7; }, "side", "side -7");
    bad([](Args& a) { a.side = WM_REGISTER_MAX_SIDE + 1; }, "side", "side past the cap");
    bad([&](Args& a) { a.side = imax; }, "side", "side INT_MAX");
    bad([&](Args& a) { a.side = imin; }, "side", "side INT_MIN");
    bad([](Args& a) { a.pairs = 0; }, "pairs_dev", "null pairs");
    bad([](Args& a) { a.pairs = 0x4004; }, "aligned", "misaligned pairs");
    bad([](Args& a) { a.min_cells = 0; }, "min_cells", "min_cells 0");
    bad([](Args& a) { a.min_cells = -1; }, "min_cells", "min_cells -1");
    bad([&](Args& a) { a.min_cells = imin; }, "min_cells", "min_cells INT_MIN");
    bad([](Args& a) { a.a = 0; }, "a_dev", "null a");
    bad([](Args& a) { a.b = 0; }, "b_dev", "null b");
    bad([](Args& a) { a.moments = 0; }, "moments_dev", "null moments");
    bad([](Args& a) { a.best = 0; }, "best_dev", "null best");
    bad([](Args& a) { a.peak = 0; }, "peak_dev", "null peak");
    for (uintptr_t off : {1, 2, 4, 7}) {
        bad([&](Args& a) { a.moments += off; }, "moments_dev not 8-byte aligned", "misaligned moments");
        bad([&](Args& a) { a.peak += off; }, "peak_dev not 8-byte aligned", "misaligned peak");
    }
    for (uintptr_t off : {1, 2, 3}) bad([&](Args& a) { a.best += off; }, "best_dev not 4-byte aligned", "misaligned best");
    Args a;
    // n_pairs == 0: 0 before looking at any pointer or any other argument
    a.n_pairs = 0; a.pairs = 0; a.a = 0; a.b = 0; a.moments = 0; a.best = 0; a.peak = 0; a.search = -3; a.side = 0; a.min_cells = 0;
    expect(search(a) == 0, "n_pairs == 0 returns 0");
    // the largest legal shape passes every size computation before the pointer checks stop it
    a = Args(); a.n_pairs = WM_REGISTER_MAX_PAIRS; a.search = WM_REGISTER_MAX_SEARCH; a.side = WM_REGISTER_MAX_SIDE; a.min_cells = imax; a.peak = 0;
    expect(search(a) < 0 && says("peak_dev"), "largest shape, null peak");
    std::printf(failures ? "register_zncc_args_check: %d FAILED\n" : "register_zncc_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
