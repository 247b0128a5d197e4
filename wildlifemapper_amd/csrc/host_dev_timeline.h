// Dev instrumentation: in-kernel timelines of the GEMMs and the attention kernels (tools/gemm_bench.py, tools/g8_timeline.py,
// tools/win_timeline.py with WM_GEMM_DBG / WM_GEMM8_DBG / WM_ATTN_DBG) and the tile-order A/B (WM_GEMM_GROUP_M).  Included only with
// -DWM_DEV_TIMELINE=1 (tools/build_dev.sh); the product library carries neither the instrumented kernel instances nor these
// environment switches.  Each timeline function is called through WM_DEV_HOOK: 0 = not taken (the launcher goes on), 1 = the instrumented
// launch replaced the launcher's own, < 0 = error.
#pragma once
#include "attn_common.h"
#include "gemm16_v5.h"
#include "gemm8.h"
#include "host_core.h"

namespace {

// tile-order A/B (WM_GEMM_GROUP_M = row tiles per group of the grouped order, every 256-row-tile instance)
void dev_group_m(Gemm16Args& a) {
    if (const char* e = getenv("WM_GEMM_GROUP_M")) { if (atoi(e) > 0) a.group_m = atoi(e); }
}

// column tiles per workgroup of the folded-LayerNorm consumer (WM_GEMM_WALK = T; gemm16_v5.h "Column walk"): as if asked for by the caller
void dev_walk(Gemm16Args& a) {
    if (const char* e = getenv("WM_GEMM_WALK")) { if (atoi(e) > 0) a.walk = atoi(e); }
}

static double dev_median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

// WM_GEMM_DBG: interval timing inside the plain or the folded-LayerNorm consumer 256 x 320 instance, on its 1st launch and on every 31st
// (after a run of back-to-back launches).  One record of six stamps per tile, in (workgroup, tile of its walk) order.
template <class T16, int BN, int NSLOT, bool FOLDP, bool FOLDC>
int dev_gemm16v5_timeline(hipStream_t s, const Gemm16Args& a, int grid, int lds) {
    if constexpr (BN == 320 && NSLOT == 3 && !FOLDP) {
        static const bool dbg = getenv("WM_GEMM_DBG") != nullptr;
        static int dbg_count = 0;
        if (dbg) ++dbg_count;
        if (!dbg || (dbg_count != 1 && dbg_count % 31 != 0)) return 0;
        static unsigned* buf = nullptr;
        const int walk = a.walk > 1 ? a.walk : 1, tiles = grid * walk;
        const size_t bytes = 512 + (size_t)tiles * 48;
        if (!buf) HIP_TRY(hipMalloc((void**)&buf, 512 + 8192 * 48));
        if (tiles > 8192) return fail("dbg grid");
        HIP_TRY(hipMemsetAsync(buf, 0, bytes, s));
        Gemm16Args d = a;
        d.zero_page = (const u16*)buf;
        WM_TRY(set_max_lds((const void*)gemm16v5_kernel<T16, BN, NSLOT, true, false, FOLDC>, lds));
        hipLaunchKernelGGL((gemm16v5_kernel<T16, BN, NSLOT, true, false, FOLDC>), dim3(grid), dim3(512), lds, s, d);
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<unsigned char> hbuf(bytes);
        HIP_TRY(hipMemcpy(hbuf.data(), buf, bytes, hipMemcpyDeviceToHost));
        const unsigned* hb = (const unsigned*)hbuf.data();
        fprintf(stderr, "[gemm16v5 dbg] launch %d  M=%d N=%d K=%d act=%d out_packed=%d foldc=%d walk=%d grid=%d  marks relative to group-0 mark 0 of step 8\n",
                dbg_count, a.M, a.N, a.K, a.act, a.out_packed, (int)FOLDC, walk, grid);
        for (int g = 0; g < 2; ++g)
            for (int st = 0; st < 10; st += 3) {
                fprintf(stderr, "  g%d s%2d:", g, st + 8);
                for (int k = 0; k < 6; ++k) fprintf(stderr, " %7u", hb[g * 64 + st * 6 + k] - hb[0]);
                fprintf(stderr, "\n");
            }
        fprintf(stderr, "  workgroup 0 epilogue (10 ns units after loop end): ring free %u, pass0 staged %u, pass0 stores issued %u, pass1 staged %u, pass1 stores issued %u\n",
                hb[104], hb[105], hb[106], hb[107], hb[108]);
        fprintf(stderr, "  workgroup 0 main loop: %u s_memtime counts in %.2f us -> %.0f MHz\n", hb[109], hb[110] * 0.01, hb[109] / (hb[110] * 0.01));
        // per-tile wall-clock stamps (100 MHz): [0] entry (first tile of a workgroup) or hand-over barrier passed (later tiles of a walk),
        // [1] first barrier passed, [2] loop end, [3] stores acknowledged (last tile of a workgroup, else 0), [4] CU, [5] last staging read
        const unsigned long long* r = (const unsigned long long*)(hbuf.data() + 512);
        unsigned long long t_min = ~0ull, t_max = 0;
        for (int i = 0; i < tiles; ++i) { t_min = std::min(t_min, r[i * 6]); t_max = std::max(t_max, std::max(r[i * 6 + 3], r[i * 6 + 5])); }
        auto cu_key = [&](int i) { const unsigned long long v = r[i * 6 + 4]; return (v >> 32 << 16) | ((v >> 8) & 0xff) | (((v >> 13) & 7) << 8); };
        std::vector<int> ids(tiles);
        for (int i = 0; i < tiles; ++i) ids[i] = i;
        std::sort(ids.begin(), ids.end(), [&](int x, int y) { return cu_key(x) != cu_key(y) ? cu_key(x) < cu_key(y) : r[x * 6] < r[y * 6]; });
        // the boundaries between successive tiles of one CU.  Between workgroups: hand-over = the next one's entry - the last one's stores
        // acknowledged, fill = entry -> first barrier.  Inside a walk: hand-over = last staging read -> hand-over barrier passed, fill = from
        // there to the first barrier (it includes the drain of the stores, which nothing waits for separately).
        std::vector<double> ho_wg, fill_wg, fill_later, ho_in, fill_in, loop, epi, drain, period, gap_wg, gap_in;
        for (int k = 0; k < tiles; ++k) {
            const int i = ids[k];
            const bool first = i % walk == 0, last = i % walk == walk - 1;
            (first ? fill_wg : fill_in).push_back((double)(r[i * 6 + 1] - r[i * 6]) * 0.01);
            loop.push_back((double)(r[i * 6 + 2] - r[i * 6 + 1]) * 0.01);
            epi.push_back((double)(r[i * 6 + 5] - r[i * 6 + 2]) * 0.01);
            if (last) drain.push_back((double)(r[i * 6 + 3] - r[i * 6 + 5]) * 0.01);
            if (k == 0 || cu_key(ids[k - 1]) != cu_key(i)) continue;
            const int j = ids[k - 1];
            period.push_back((double)(r[i * 6 + 1] - r[j * 6 + 1]) * 0.01);
            if (first) {
                ho_wg.push_back(((double)r[i * 6] - (double)r[j * 6 + 3]) * 0.01);
                gap_wg.push_back(((double)r[i * 6 + 1] - (double)r[j * 6 + 5]) * 0.01);
                fill_later.push_back((double)(r[i * 6 + 1] - r[i * 6]) * 0.01);
            } else {
                ho_in.push_back(((double)r[i * 6] - (double)r[j * 6 + 5]) * 0.01);
                gap_in.push_back(((double)r[i * 6 + 1] - (double)r[j * 6 + 5]) * 0.01);
            }
        }
        fprintf(stderr, "  span %.2f us, %d tiles on %d workgroups; medians per tile [us]: loop %.2f, loop end -> last staging read %.2f, last staging read -> stores acknowledged %.2f (n=%zu), first barrier -> next tile's first barrier on the CU %.2f\n",
                (t_max - t_min) * 0.01, tiles, grid, dev_median(loop), dev_median(epi), dev_median(drain), drain.size(), dev_median(period));
        fprintf(stderr, "  boundary between workgroups (n=%zu): hand-over (stores acknowledged -> next entry) %.2f, fill (entry -> first barrier) %.2f [all first tiles: %.2f], last staging read -> next first barrier %.2f\n",
                ho_wg.size(), dev_median(ho_wg), dev_median(fill_later), dev_median(fill_wg), dev_median(gap_wg));
        fprintf(stderr, "  boundary inside a walk (n=%zu): hand-over (last staging read -> barrier passed) %.2f, fill and store drain (-> first barrier) %.2f, last staging read -> next first barrier %.2f\n",
                ho_in.size(), dev_median(ho_in), dev_median(fill_in), dev_median(gap_in));
        // timeline of the tiles that ran on the CU of tile 0
        fprintf(stderr, "  tiles on the CU of workgroup 0 (entry, barrier0, loop end, last staging read, stores acknowledged; us from first entry):\n");
        for (int k = 0; k < tiles; ++k) {
            const int i = ids[k];
            if (cu_key(i) != cu_key(0)) continue;
            fprintf(stderr, "    wg %4d tile %d: %7.2f %7.2f %7.2f %7.2f %7.2f\n", i / walk, i % walk, (r[i * 6] - t_min) * 0.01, (r[i * 6 + 1] - t_min) * 0.01,
                    (r[i * 6 + 2] - t_min) * 0.01, (r[i * 6 + 5] - t_min) * 0.01, r[i * 6 + 3] ? (r[i * 6 + 3] - t_min) * 0.01 : 0.0);
        }
        return 1;
    }
    return 0;
}

// WM_GEMM8_DBG: per-workgroup wall-clock stamps of an instance's 5th launch (not the plane form)
template <class T16, bool PLANES>
int dev_gemm8_timeline(hipStream_t s, Gemm8Args a, int grid) {
    using G = G8;
    static const bool dbg = getenv("WM_GEMM8_DBG") != nullptr;
    static int dbg_count = 0;
    if (PLANES || !dbg || ++dbg_count != 5) return 0;
    unsigned long long* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, (size_t)grid * 32 + 16));
    HIP_TRY(hipMemset(buf, 0, (size_t)grid * 32 + 16));
    a.dbg = buf;
    WM_TRY(set_max_lds((const void*)gemm8_kernel<T16, true>, G::LDS));
    hipLaunchKernelGGL((gemm8_kernel<T16, true>), dim3(grid), dim3(512), G::LDS, s, a);
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned long long> r((size_t)grid * 4 + 2);
    HIP_TRY(hipMemcpy(r.data(), buf, r.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(buf));
    unsigned long long t_min = ~0ull, t_max = 0;
    double pro = 0, loop = 0, epi = 0;
    for (int i = 0; i < grid; ++i) {
        t_min = std::min(t_min, r[i * 4]); t_max = std::max(t_max, r[i * 4 + 3]);
        pro += (double)(r[i * 4 + 1] - r[i * 4]); loop += (double)(r[i * 4 + 2] - r[i * 4 + 1]); epi += (double)(r[i * 4 + 3] - r[i * 4 + 2]);
    }
    fprintf(stderr, "[gemm8 dbg] workgroup 0 main loop: %llu shader cycles in %.2f us -> %.0f MHz\n", r[(size_t)grid * 4], r[(size_t)grid * 4 + 1] * 0.01,
            (double)r[(size_t)grid * 4] / (r[(size_t)grid * 4 + 1] * 0.01));
    fprintf(stderr, "[gemm8 dbg] BK=%d M=%d N=%d K=%d out=%s: span %.2f us; per workgroup avg: prologue %.2f us, loop %.2f us (%.0f ns per 128 of K), epilogue %.2f us; %d workgroups\n",
            G::BKB, a.M, a.N, a.K, a.residual ? "f32+res" : (a.out8 ? "fp8" : "16"), (t_max - t_min) * 0.01, pro / grid * 0.01, loop / grid * 0.01,
            loop / grid * 10.0 / (a.K / 128.0), epi / grid * 0.01, grid);
    return 1;
}

// WM_ATTN_DBG: phase stamps of workgroup 0 on the 5th launch of an attention kernel instance KERN (`waves` x `marks` stamps,
// relative to the first); extra = the kernel's arguments after AttnArgs
template <auto KERN, class... Extra>
int dev_attn_timeline(const char* tag, int waves, int marks, dim3 grid, dim3 block, int lds, hipStream_t s, const AttnArgs& a, Extra... extra) {
    static const bool dbg = getenv("WM_ATTN_DBG") != nullptr;
    static int dbg_count = 0;
    if (!dbg || ++dbg_count != 5) return 0;
    unsigned long long* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, 8 * 64 * 8));
    HIP_TRY(hipMemset(buf, 0, 8 * 64 * 8));
    AttnArgs a2 = a; a2.tl = buf;
    hipLaunchKernelGGL(KERN, grid, block, lds, s, a2, extra...);
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long host[8 * 64];
    HIP_TRY(hipMemcpy(host, buf, sizeof(host), hipMemcpyDeviceToHost));
    for (int w = 0; w < waves; ++w) {
        fprintf(stderr, "%s wave %d:", tag, w);
        for (int i = 0; i < marks; ++i) fprintf(stderr, " %lld", (long long)(host[w * 64 + i] - host[0]));
        fprintf(stderr, "\n");
    }
    hipFree(buf);
    return 1;
}

}  // namespace
