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

// WM_GEMM_DBG: interval timing inside the plain 256 x 320 instance, on its 1st and (after a run of back-to-back launches) 31st launch
template <class T16, int BN, int NSLOT, bool FOLDP, bool FOLDC>
int dev_gemm16v5_timeline(hipStream_t s, const Gemm16Args& a, int grid, int lds) {
    if constexpr (BN == 320 && NSLOT == 3 && !FOLDP && !FOLDC) {
        static const bool dbg = getenv("WM_GEMM_DBG") != nullptr;
        static int dbg_count = 0;
        if (dbg) ++dbg_count;
        if (!dbg || (dbg_count != 1 && dbg_count != 31)) return 0;
        static unsigned* buf = nullptr;
        const size_t bytes = 512 + (size_t)grid * 40;
        if (!buf) HIP_TRY(hipMalloc((void**)&buf, 512 + 8192 * 40));
        if (grid > 8192) return fail("dbg grid");
        HIP_TRY(hipMemsetAsync(buf, 0, bytes, s));
        Gemm16Args d = a;
        d.zero_page = (const u16*)buf;
        WM_TRY(set_max_lds((const void*)gemm16v5_kernel<T16, BN, NSLOT, true>, lds));
        hipLaunchKernelGGL((gemm16v5_kernel<T16, BN, NSLOT, true>), dim3(grid), dim3(512), lds, s, d);
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<unsigned char> hbuf(bytes);
        HIP_TRY(hipMemcpy(hbuf.data(), buf, bytes, hipMemcpyDeviceToHost));
        const unsigned* hb = (const unsigned*)hbuf.data();
        fprintf(stderr, "[gemm16v5 dbg] M=%d N=%d K=%d  marks relative to group-0 mark 0 of step 8\n", a.M, a.N, a.K);
        for (int g = 0; g < 2; ++g)
            for (int st = 0; st < 10; st += 3) {
                fprintf(stderr, "  g%d s%2d:", g, st + 8);
                for (int k = 0; k < 6; ++k) fprintf(stderr, " %7u", hb[g * 64 + st * 6 + k] - hb[0]);
                fprintf(stderr, "\n");
            }
        fprintf(stderr, "  workgroup 0 epilogue (10 ns units after loop end): ring free %u, pass0 staged %u, pass0 stores issued %u, pass1 staged %u, pass1 stores issued %u\n",
                hb[104], hb[105], hb[106], hb[107], hb[108]);
        fprintf(stderr, "  workgroup 0 main loop: %u s_memtime counts in %.2f us -> %.0f MHz\n", hb[109], hb[110] * 0.01, hb[109] / (hb[110] * 0.01));
        // per-workgroup wall-clock stamps (100 MHz): entry, first barrier passed, loop end, stores acknowledged
        const unsigned long long* r = (const unsigned long long*)(hbuf.data() + 512);
        unsigned long long t_min = ~0ull, t_max = 0;
        for (int i = 0; i < grid; ++i) { t_min = std::min(t_min, r[i * 5]); t_max = std::max(t_max, r[i * 5 + 3]); }
        double pro = 0, loop = 0, epi = 0;
        for (int i = 0; i < grid; ++i) {
            pro += (double)(r[i * 5 + 1] - r[i * 5]); loop += (double)(r[i * 5 + 2] - r[i * 5 + 1]); epi += (double)(r[i * 5 + 3] - r[i * 5 + 2]);
        }
        fprintf(stderr, "  span %.2f us; per workgroup avg: prologue %.2f us, loop %.2f us, epilogue %.2f us\n", (t_max - t_min) * 0.01,
                pro / grid * 0.01, loop / grid * 0.01, epi / grid * 0.01);
        // timeline of the workgroups that ran on the CU of workgroup 0 (same XCC + HW_ID CU/SE bits)
        auto cu_key = [&](int i) { const unsigned long long v = r[i * 5 + 4]; return (v >> 32 << 16) | ((v >> 8) & 0xff) | (((v >> 13) & 7) << 8); };
        for (int probe : {0, 1}) {
            fprintf(stderr, "  workgroups sharing the CU of workgroup %d (entry, barrier0, loop end, done; us from first entry):\n", probe);
            std::vector<int> ids;
            for (int i = 0; i < grid; ++i) if (cu_key(i) == cu_key(probe)) ids.push_back(i);
            std::sort(ids.begin(), ids.end(), [&](int x, int y) { return r[x * 5] < r[y * 5]; });
            for (int i : ids)
                fprintf(stderr, "    wg %4d: %7.2f %7.2f %7.2f %7.2f\n", i, (r[i * 5] - t_min) * 0.01, (r[i * 5 + 1] - t_min) * 0.01,
                        (r[i * 5 + 2] - t_min) * 0.01, (r[i * 5 + 3] - t_min) * 0.01);
        }
        // distribution of entry times
        std::vector<double> ent(grid), fin(grid);
        for (int i = 0; i < grid; ++i) { ent[i] = (r[i * 5] - t_min) * 0.01; fin[i] = (r[i * 5 + 3] - t_min) * 0.01; }
        std::sort(ent.begin(), ent.end()); std::sort(fin.begin(), fin.end());
        fprintf(stderr, "  entry times: min %.2f p25 %.2f p50 %.2f p75 %.2f max %.2f; done: min %.2f p50 %.2f max %.2f\n", ent[0], ent[grid / 4], ent[grid / 2],
                ent[3 * grid / 4], ent[grid - 1], fin[0], fin[grid / 2], fin[grid - 1]);
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
