// Stand-alone check of the host-side argument validation of wm_register_render_u8, wm_register_search,
// wm_register_search_zncc and wm_register_refine, for a sanitizer build of the host code (no GPU needed: every call here returns before the first HIP
// call).  Build and run, from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include tools/register_args_check.cpp wildlifemapper_amd/csrc/wm_api.hip \
//         -o register_args_check && ./register_args_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "wm_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAIL: %s (last error: %s)\n", what, wm_last_error()); ++failures; }
}

static bool says(const char* word) { return std::strstr(wm_last_error(), word) != nullptr; }

// Fake device pointers, never dereferenced on these paths.
struct Args {
    uintptr_t frames = 0x1000, g2p = 0x2000, size = 0x3000, pairs = 0x4000, a = 0x5001, b = 0x6003, slot = 0x7000, score = 0x8000,
              status = 0x9000, best = 0xa000, peak = 0xb000, moments = 0xc000, sums = 0xd000;
    int n_frames = 2, n_resident = 2, n_pairs = 3, search = 4, side = 64, min_cells = 1;
    double cell = 0.5;
};

static int render(const Args& a) {
    return wm_register_render_u8((const wm_frame_desc*)a.frames, a.n_resident, (const int32_t*)a.slot, (const double*)a.g2p,
                                 (const int32_t*)a.size, a.n_frames, (const wm_register_pair*)a.pairs, a.n_pairs, a.cell, a.search, a.side,
                                 (uint8_t*)a.a, (uint8_t*)a.b, (int32_t*)a.status, nullptr);
}

static int search(const Args& a) {
    return wm_register_search((const uint8_t*)a.a, (const uint8_t*)a.b, (const wm_register_pair*)a.pairs, a.n_pairs, a.search, a.side,
                              a.min_cells, (int32_t*)a.score, (int32_t*)a.best, nullptr);
}

static int zncc(const Args& a) {
    return wm_register_search_zncc((const uint8_t*)a.a, (const uint8_t*)a.b, (const wm_register_pair*)a.pairs, a.n_pairs, a.search, a.side,
                                   a.min_cells, (int64_t*)a.moments, (int32_t*)a.best, (double*)a.peak, nullptr);
}

static int refine(const Args& a) {
    return wm_register_refine((const uint8_t*)a.a, (const uint8_t*)a.b, (const wm_register_pair*)a.pairs, a.n_pairs, a.search, a.side,
                              (int64_t*)a.sums, nullptr);
}

// an entry and the name its messages begin with
struct Entry { int (*call)(const Args&); const char* name; };
static const Entry RENDER = {render, "wm_register_render_u8: "}, SEARCH = {search, "wm_register_search: "}, ZNCC = {zncc, "wm_register_search_zncc: "},
                   REFINE = {refine, "wm_register_refine: "};

// a bad argument: each of the entries refuses it under its own name with `word` in the message
template <class F>
static void bad(std::initializer_list<Entry> entries, F change, const char* word, const char* what) {
    Args a;
    change(a);
    for (const Entry& e : entries) expect(e.call(a) < 0 && says(e.name) && says(word), what);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
    expect(wm_abi_version() == WM_ABI_VERSION && WM_ABI_VERSION == 13, "ABI version 13");
    expect(sizeof(wm_register_pair) == 32, "wm_register_pair is 32 bytes");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.n_pairs = -1; }, "n_pairs", "n_pairs -1");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.n_pairs = imin; }, "n_pairs", "n_pairs INT_MIN");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.n_pairs = WM_REGISTER_MAX_PAIRS + 1; }, "n_pairs", "n_pairs past the cap");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.n_pairs = imax; }, "n_pairs", "n_pairs INT_MAX");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.search = -1; }, "search", "search -1");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.search = imin; }, "search", "search INT_MIN");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.search = WM_REGISTER_MAX_SEARCH + 1; }, "search", "search past the cap");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.search = imax; }, "search", "search INT_MAX");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.side = 0; }, "side", "side 0");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.side = -7; }, "side", "side -7");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.side = WM_REGISTER_MAX_SIDE + 1; }, "side", "side past the cap");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.side = imax; }, "side", "side INT_MAX");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [&](Args& a) { a.side = imin; }, "side", "side INT_MIN");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.pairs = 0; }, "pairs_dev", "null pairs");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.pairs = 0x4004; }, "aligned", "misaligned pairs");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.a = 0; }, "a_dev", "null a");
    bad({RENDER, SEARCH, ZNCC, REFINE}, [](Args& a) { a.b = 0; }, "b_dev", "null b");
    Args a;
    // n_pairs == 0: 0 before looking at any pointer or any other argument
    a.n_pairs = 0; a.pairs = 0; a.a = 0; a.b = 0; a.score = 0; a.moments = 0; a.sums = 0; a.best = 0; a.peak = 0; a.status = 0; a.search = -3; a.side = 0;
    a.min_cells = 0; a.cell = nan; a.n_frames = -1;
    expect(render(a) == 0, "render: n_pairs == 0 returns 0");
    expect(search(a) == 0, "search: n_pairs == 0 returns 0");
    expect(zncc(a) == 0, "zncc: n_pairs == 0 returns 0");
    expect(refine(a) == 0, "refine: n_pairs == 0 returns 0");
    bad({RENDER}, [](Args& a) { a.n_frames = -1; }, "n_frames", "n_frames -1");
    bad({RENDER}, [&](Args& a) { a.n_frames = imin; }, "n_frames", "n_frames INT_MIN");
    bad({RENDER}, [](Args& a) { a.n_frames = WM_COVERAGE_MAX_FRAMES + 1; }, "n_frames", "n_frames past the cap");
    bad({RENDER}, [&](Args& a) { a.n_frames = imax; }, "n_frames", "n_frames INT_MAX");
    bad({RENDER}, [](Args& a) { a.n_resident = -1; }, "n_resident", "n_resident -1");
    bad({RENDER}, [&](Args& a) { a.n_resident = imin; }, "n_resident", "n_resident INT_MIN");
    bad({RENDER}, [](Args& a) { a.n_resident = WM_COVERAGE_MAX_FRAMES + 1; }, "n_resident", "n_resident past the cap");
    bad({RENDER}, [&](Args& a) { a.n_resident = imax; }, "n_resident", "n_resident INT_MAX");
    for (double cell : {0.0, -0.5, nan, inf, -inf}) bad({RENDER}, [&](Args& a) { a.cell = cell; }, "cell", "bad cell");
    bad({RENDER}, [](Args& a) { a.g2p = 0; }, "g2p_dev", "null g2p");
    bad({RENDER}, [](Args& a) { a.size = 0; }, "size_dev", "null size");
    bad({RENDER}, [](Args& a) { a.g2p = 0x2004; }, "aligned", "misaligned g2p");
    bad({RENDER}, [](Args& a) { a.size = 0x3002; }, "aligned", "misaligned size");
    bad({RENDER}, [](Args& a) { a.frames = 0; }, "frames_dev", "null frames");
    bad({RENDER}, [](Args& a) { a.slot = 0; }, "slot_dev", "null slot");
    bad({RENDER}, [](Args& a) { a.status = 0; }, "status_dev", "null status");
    bad({RENDER}, [](Args& a) { a.frames = 0x1004; }, "aligned", "misaligned frames");
    bad({RENDER}, [](Args& a) { a.slot = 0x7002; }, "aligned", "misaligned slot");
    bad({RENDER}, [](Args& a) { a.status = 0x9002; }, "aligned", "misaligned status");
    for (int mc : {0, -1, imin}) bad({SEARCH, ZNCC}, [&](Args& a) { a.min_cells = mc; }, "min_cells", "min_cells below 1");
    bad({SEARCH, ZNCC}, [](Args& a) { a.best = 0; }, "best_dev", "null best");
    bad({SEARCH}, [](Args& a) { a.score = 0; }, "score_dev", "null score");
    bad({SEARCH}, [](Args& a) { a.score = 0x8002; }, "aligned", "misaligned score");
    bad({SEARCH}, [](Args& a) { a.best = 0xa001; }, "aligned", "misaligned best");
    bad({ZNCC}, [](Args& a) { a.moments = 0; }, "moments_dev", "null moments");
    bad({ZNCC}, [](Args& a) { a.peak = 0; }, "peak_dev", "null peak");
    for (uintptr_t off : {1, 2, 4, 7}) {
        bad({ZNCC}, [&](Args& a) { a.moments += off; }, "moments_dev not 8-byte aligned", "misaligned moments");
        bad({ZNCC}, [&](Args& a) { a.peak += off; }, "peak_dev not 8-byte aligned", "misaligned peak");
    }
    for (uintptr_t off : {1, 2, 3}) bad({ZNCC}, [&](Args& a) { a.best += off; }, "best_dev not 4-byte aligned", "misaligned best");
    expect(WM_REGISTER_REFINE_SUMS == 28, "WM_REGISTER_REFINE_SUMS is 28");
    bad({REFINE}, [](Args& a) { a.search = 0; }, "search", "refine: search 0 (B carries no ring)");
    bad({REFINE}, [](Args& a) { a.sums = 0; }, "sums_dev", "null sums");
    for (uintptr_t off : {1, 2, 4, 7}) bad({REFINE}, [&](Args& a) { a.sums += off; }, "sums_dev not 8-byte aligned", "misaligned sums");
    // the largest legal shape passes every size computation before the pointer checks stop it
    a = Args(); a.n_pairs = WM_REGISTER_MAX_PAIRS; a.search = WM_REGISTER_MAX_SEARCH; a.side = WM_REGISTER_MAX_SIDE; a.min_cells = imax; a.best = 0;
    expect(search(a) < 0 && says("best_dev"), "largest shape, null best");
    a.status = 0; expect(render(a) < 0 && says("status_dev"), "largest shape, null status");
    a.best = Args().best; a.peak = 0; expect(zncc(a) < 0 && says("peak_dev"), "largest shape, null peak");
    a.sums = 0; expect(refine(a) < 0 && says("sums_dev"), "largest shape, null sums");
    std::printf(failures ? "register_args_check: %d FAILED\n" : "register_args_check: all passed\n", failures);
    return failures ? 1 : 0;
}
