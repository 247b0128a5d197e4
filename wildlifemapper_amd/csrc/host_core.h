// Host core of the engine: error plumbing, per-device launcher state, the handle, the profiled launch bracket and the
// helpers that pick a template instance.  Host-only; part of the one translation unit wm_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <tuple>
#include <type_traits>
#include <mutex>
#include <set>
#include <string>
#include <algorithm>
#include <array>
#include <vector>

#include "../../include/wm_hip.h"
#include "wm_common.h"

// Dev instrumentation (host_dev_timeline.h) is compiled only with -DWM_DEV_TIMELINE=1 (tools/build_dev.sh).  A launcher
// reaches it through one WM_DEV_HOOK line, which the product build drops unevaluated: non-zero from the hook ends the
// launcher (1: the instrumented launch took the place of its own; < 0: error).
#ifndef WM_DEV_TIMELINE
#define WM_DEV_TIMELINE 0
#endif
#if WM_DEV_TIMELINE
#define WM_DEV_HOOK(call) do { const int _d = (call); if (_d) return _d < 0 ? _d : 0; } while (0)
#else
#define WM_DEV_HOOK(call) do { } while (0)
#endif

using namespace wm;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define WM_TRY(expr)            \
    do {                        \
        int _r = (expr);        \
        if (_r != 0) return _r; \
    } while (0)

// ---------------------------------------------------------------------------
// per-device launcher state (a process may drive several devices, one handle each)
// ---------------------------------------------------------------------------
static std::mutex g_dev_mu;

// hipFuncAttributeMaxDynamicSharedMemorySize is per (function, device)
static int set_max_lds(const void* fn, int bytes) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::set<std::pair<const void*, int>> done;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (done.count({fn, dev})) return 0;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({fn, dev});
    return 0;
}

// Scratch memory of the handle-less single-op entry points (tests, tools), one buffer per (device, stream, use): a stream's launches
// are ordered, two streams never share a buffer.  Grown by free + malloc (hipFree synchronises the device).  Handles own their own.
static int op_scratch(hipStream_t s, int use, size_t bytes, void** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    struct Buf { void* p = nullptr; size_t cap = 0; };
    static std::map<std::tuple<int, hipStream_t, int>, Buf> bufs;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    Buf& b = bufs[std::make_tuple(dev, s, use)];
    if (b.cap < bytes) {
        if (b.p) hipFree(b.p);
        b.p = nullptr; b.cap = 0;
        HIP_TRY(hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = b.p;
    return 0;
}

static int num_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    static std::map<int, int> cus;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = cus.find(dev);
    if (it != cus.end()) return it->second;
    hipDeviceProp_t prop;
    int n = 256;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = prop.multiProcessorCount;
    cus[dev] = n;
    return n;
}

// 256 B of zeros per device: source of out-of-image taps of the implicit-GEMM conv
static int zero_page_for_device(const uint16_t** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static std::map<int, uint16_t*> pages;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = pages.find(dev);
    if (it == pages.end()) {
        uint16_t* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, 256));
        HIP_TRY(hipMemset(p, 0, 256));
        it = pages.emplace(dev, p).first;
    }
    *out = it->second;
    return 0;
}

// which GEMM kernel instance each launch took (wm_debug_gemm_variant_counts): the tests assert on it, so that a
// change of the dispatch heuristic cannot silently leave an instance without a value check
static std::atomic<int64_t> g_variant_count[WM_GEMM_VARIANT_COUNT];
static inline void count_variant(int v) { g_variant_count[v].fetch_add(1, std::memory_order_relaxed); }

// ---------------------------------------------------------------------------
// picking a template instance: a launcher passes a generic lambda and reads the choice off its argument's type
// (decltype(t) is the operand type, decltype(bn)::value the width)
// ---------------------------------------------------------------------------
template <int V>
using int_c = std::integral_constant<int, V>;

// 16-bit operand type of a precision value: FP16 for WM_PREC_FP16, BF16 for every other value (a launcher that takes
// only the two checks before it asks)
template <class F>
static auto by_type16(int prec, F&& f) { return prec == WM_PREC_FP16 ? f(FP16{}) : f(BF16{}); }

// column-tile width of the 256-row-tile GEMM over N channels, which is also the tile width of the folded LayerNorm's
// partial statistics over C channels (the producer GEMM's at N = C)
static int fold_bn_for(int C) { return C % 320 == 0 ? 320 : 256; }
template <class F>
static auto by_tile_width(int n, F&& f) { return fold_bn_for(n) == 320 ? f(int_c<320>{}) : f(int_c<256>{}); }

// head_dim of an attention kernel instance: f(int_c<HD>{}) for the one of HDS that equals hd, none() where
// no instance is built for it
template <int... HDS, class F, class N>
static int by_head_dim(int hd, F&& f, N&& none) {
    int r = 0;
    return ((hd == HDS && ((r = f(int_c<HDS>{})), true)) || ...) ? r : none();
}

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
namespace {

constexpr int T = 4096;          // tokens per tile (64 x 64)
constexpr int GRID = 64;
constexpr int HFC = 1024;        // HFC adaptor width (image_encoder.py:65-87)
constexpr int HFC_HEADS = 8;
constexpr int OUTC = 256;        // neck / decoder width
constexpr int NQ = WM_NUM_QUERIES;
constexpr int DEC_MLP = 2048;

struct HostW {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

struct EvPair {
    hipEvent_t a, b;
    int kclass;
    double flops, bytes;
};

struct Profiler {
    bool on = false;
    std::vector<EvPair> used;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    wm_kclass_stat acc[WM_KCLASS_COUNT] = {};
};

}  // namespace

struct wm_handle {
    wm_config cfg{};
    int fp8_gemms = WM_FP8_ALL;             // fp8 mode: which of a block's GEMMs run e4m3 (wm_config.fp8_gemms, 0 = all)
    int fp8_bf16_tail = 0, fp8_bf16_head = 0;  // fp8 mode: the first / last blocks that stay bf16 (env WM_FP8_BF16_HEAD / _TAIL, default 0)
    int fp16_tail = 0;      // bf16 mode: the last fp16_tail transformer blocks use fp16 operands (parity margin dial; default 0)
    int device = 0;
    int D = 0, depth = 0, heads = 0, hd = 0, prec = 0, maxB = 0;
    bool is_global[64] = {};
    bool finalized = false, enc_ready = false, dec_ready = false;
    std::map<std::string, std::vector<int64_t>> expected;   // name -> shape
    std::map<std::string, HostW> staged;
    std::map<std::string, uint16_t*> w16;
    // folded LayerNorm (WM_CFG_FOLD_LN): per consumer GEMM weight name: gamma (.) W in LDS-image order, c1, c2; per-row partial
    // statistics of the residual stream [maxB * 4096][<= 4][2]
    std::map<std::string, uint16_t*> wfold;
    std::map<std::string, float*> fold_c1, fold_c2;
    std::map<std::string, float*> wsrc32;   // fp32 device copies of the weights that get folded (qkv, lin1 of every block): gamma (.) W is rounded once
    float* fold_stats = nullptr;
    // split stream (gemm16_v5.h "Split stream"): xn16 = hi plane, lo16 = lo plane, both LDS-image order; `split`: used wherever the
    // residual GEMMs of a folded block run the 256-row-tile kernel (WM_STREAM_SPLIT=0 keeps the fp32 stream: A/B runs).
    // overflow: host-pinned, device-visible word the stream's producers set when an fp16 hi plane clamps (wm_stream_overflow).
    uint16_t* lo16 = nullptr;
    bool split = false;
    // fp8 blocks (round 4): the stream as two planes of rows (x16last = hi bf16, lo16; gemm8.h PLANES) between the e4m3 residual GEMMs, so the
    // LayerNorm-to-e4m3 pass reads 2 bytes per element (gemm8.h PLANES); WM_FP8_ROWS=0 keeps the fp32 stream (A/B runs)
    bool rows8 = true;
    bool fold_from16 = false;               // WM_FOLD_FROM16=1 (A/B runs): gamma (.) W from the 16-bit weight, rounded twice (round 3's form)
    int* overflow = nullptr;
    bool fold = false, fold_bf16 = false;   // WM_CFG_FOLD_LN: fp16-operand blocks; WM_CFG_FOLD_LN_BF16: bf16-operand blocks too
    std::map<std::string, uint16_t*> w16p;  // the same weights in LDS-image order (gemm16_v5.h "Operand layout"), for the 256-row-tile kernels
    std::map<std::string, uint8_t*> w8k;    // qkv / lin1 of the fp8 blocks again with the K columns at wm::plane_pos (operand = layernorm_plane_fp8_kernel's output)
    std::map<std::string, uint8_t*> w8;     // WM_PREC_FP8: e4m3 weights of the blocks' GEMMs; their per-channel scales live in w32[name + ".wscale"]
    uint8_t* ao8 = nullptr;                 // attention output as e4m3 (A operand of proj)
    std::map<std::string, float*> w32;
    std::vector<void*> allocs;
    Profiler prof;
    std::map<const float*, std::pair<uint16_t*, uint16_t*>> w32x3;   // decoder weights as fp16 (hi, lo) planes of W * 2^6 (gemm32.h gemm32x3_kernel), by fp32 copy
    std::map<std::pair<const float*, int>, uint16_t*> bias16;   // qkv biases rounded to a 16-bit operand type (window attention's padded tokens), by (fp32 copy, type)
    float* mha_part = nullptr;              // token -> image attention: per key chunk partial softmaxes (launch_mha32)
    size_t mha_part_cap = 0;
    bool row_major = false;                 // WM_ROW_MAJOR_OPERANDS=1 (A/B runs): no operand in LDS-image order
    bool sat_on = false;                    // wm_debug_saturation_enable
    unsigned long long* sat_counts = nullptr;   // [WM_SAT_COUNT] device counters
    int tap_which = -2;
    float* tap_buf = nullptr;

    // workspace (device)
    float *resid = nullptr, *tokbase = nullptr;
    uint16_t *xn16 = nullptr, *ao16 = nullptr, *qkv16 = nullptr, *hid16 = nullptr;
    uint16_t *p16 = nullptr, *h16 = nullptr, *he16 = nullptr, *hp16 = nullptr, *pt16 = nullptr, *q16 = nullptr,
             *kv16 = nullptr, *aoh16 = nullptr, *y1n16 = nullptr, *h1_16 = nullptr, *y2_16 = nullptr, *y2t16 = nullptr;
    float *pt32 = nullptr, *y1 = nullptr, *y1n32 = nullptr, *z32 = nullptr;
    float *n1 = nullptr, *n2 = nullptr, *emb_nhwc = nullptr, *emb_nchw = nullptr;
    uint16_t *n1n16 = nullptr, *x16last = nullptr;
    float *dkeys = nullptr, *dk_a = nullptr, *dk_b = nullptr, *dk_c = nullptr;      // [B*T,256],[B*T,128] x3
    float *dq = nullptr, *dt_q = nullptr, *dt_k = nullptr, *dt_v = nullptr, *dt_att = nullptr, *dt_hid = nullptr,
          *dt_h1 = nullptr, *dt_h2 = nullptr;
    float *logits = nullptr, *boxes = nullptr, *hfc = nullptr, *tsz_default = nullptr;
    float2 *fftR = nullptr, *fft_tw = nullptr;
    float* kpe = nullptr;           // dense PE, token-major [T,256]
    wm_box_record* records = nullptr;
};

namespace {

template <class P>
int dalloc(wm_handle* h, P** out, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    h->allocs.push_back(p);
    *out = (P*)p;
    return 0;
}

// a buffer of dalloc's that goes before its handle does (hipFree synchronises the device: no kernel still reads it)
void dfree(wm_handle* h, void* p) {
    hipFree(p);
    for (auto& a : h->allocs) if (a == p) a = nullptr;
}

// -------- profiled launch bracket --------
struct Bracket {
    wm_handle* h;
    hipStream_t s;
    int idx = -1;
    Bracket(wm_handle* h_, hipStream_t s_, int kclass, double flops, double bytes) : h(h_), s(s_) {
        if (!h || !h->prof.on) return;
        Profiler& p = h->prof;
        std::pair<hipEvent_t, hipEvent_t> ev;
        if (!p.pool.empty()) { ev = p.pool.back(); p.pool.pop_back(); }
        else { hipEventCreate(&ev.first); hipEventCreate(&ev.second); }
        hipEventRecord(ev.first, s);
        p.used.push_back(EvPair{ev.first, ev.second, kclass, flops, bytes});
        idx = (int)p.used.size() - 1;
    }
    ~Bracket() {
        if (idx >= 0) hipEventRecord(h->prof.used[idx].b, s);
    }
};

int prof_collect(wm_handle* h) {
    Profiler& p = h->prof;
    for (auto& e : p.used) {
        HIP_TRY(hipEventSynchronize(e.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
        p.acc[e.kclass].launches += 1;
        p.acc[e.kclass].ms += ms;
        p.acc[e.kclass].flops += e.flops;
        p.acc[e.kclass].bytes += e.bytes;
        p.pool.push_back({e.a, e.b});
    }
    p.used.clear();
    return 0;
}

template <class K, class... Args>
int launch_simple(wm_handle* h, hipStream_t s, double bytes, K kern, dim3 grid, dim3 block, Args... args) {
    Bracket br(h, s, WM_KCLASS_OTHER, 0.0, bytes);
    hipLaunchKernelGGL(kern, grid, block, 0, s, args...);
    HIP_TRY(hipGetLastError());
    return 0;
}

unsigned grid_for(int64_t n, int per = 256, unsigned cap = 256 * 16) {
    int64_t g = (n + per - 1) / per;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

int check_ready(wm_handle* h, int batch, const char* fn, bool need_enc, bool need_dec) {
    if (!h) return fail("%s: null handle", fn);
    if (!h->finalized) return fail("%s: weights not finalized", fn);
    if (need_enc && !h->enc_ready) return fail("%s: encoder weights not loaded", fn);
    if (need_dec && !h->dec_ready) return fail("%s: decoder weights not loaded", fn);
    if (batch <= 0 || batch > h->maxB) return fail("%s: batch %d outside 1..%d", fn, batch, h->maxB);
    HIP_TRY(hipSetDevice(h->device));
    return 0;
}

}  // namespace
