// Flash-style multi-head attention on MFMA 32x32x16 (bf16 / fp16), gfx950: what the three kernels share.
//
//   attn_global_kernel   (attn_glob4.h)  - 4096 (or any multiple of 64) keys per head, optional decomposed rel-pos bias: 4-wave
//                                          workgroups, any query count that is a multiple of 128
//   attn_global8_kernel  (attn_glob8.h)  - the same arithmetic in 8-wave workgroups whose SIMD partners run in anti-phase: the 4
//                                          global blocks (image_encoder.py:246-262, 347-383) and, without the bias, the HFC
//                                          cross-attention (image_encoder.py:500-503)
//   attn_window_kernel   (attn_window.h) - 14x14 windows with zero-padded tokens that still act as keys/values
//                                          (image_encoder.py:190-199, 265-311)
//
// Per wave: 32 query rows, scores computed TRANSPOSED (S^T = K Q^T) so that a
// lane owns one query column: its 32x32 accumulator registers are that query's
// scores for 16 of the tile's 32 keys, the partner lane (lane^32) holds the other
// 16.  Softmax is therefore lane-local plus one cross-half exchange, and the
// exponentiated tile is already the B operand of the P*V product
// (O^T = V^T P^T, cdna_hip_programming.md §3 "An accumulator tile as the next
// MFMA's operand"), whose A operand V^T comes from the row-major V tile in LDS
// through ds_read_b64_tr_b16 (T10).
//
// The rel-pos bias is never materialised per (query,key) pair in memory:
//   bias[q,(kh,kw)] = q.Rh[qh-kh+S-1] + q.Rw[qw-kw+S-1]   (unscaled q, :376-381)
// For global attention a key tile is one grid row (kh fixed, kw = 0..63), so the
// kw-term is the same 64-vector for every tile (kept in registers, used as the
// MFMA accumulator's initial value) and the kh-term is one scalar per tile.
// Both are produced in the prologue by MFMA products Q x table^T (relpos_stage_tables / relpos_terms below).
#pragma once
#include <type_traits>
#include "wm_common.h"

#ifndef WM_DEV_TIMELINE
#define WM_DEV_TIMELINE 0
#endif

namespace wm {

struct AttnArgs {
    const u16* q; const u16* k; const u16* v;   // 16-bit, row = token
    u16* out;
    int q_stride, k_stride, v_stride, out_stride;   // elements between consecutive tokens
    int nq, nk;                                     // tokens per image (queries / keys)
    float scale;                                    // head_dim^-0.5
    const float* rel_h; const float* rel_w;         // [2*S-1, HD] fp32 or null
    const float* qkv_bias;                          // window kernel: [3*D] fp32 (padded tokens)
    const u16* qkv_bias16;                          // the same, rounded to the operand type: a padded token's K / V row
    int heads;
    // q carries scale * log2(e) ("Scores" below): the engine folds it into the q rows of the qkv weight (one rounding, as before); the
    // single-op entry points scale a copy of q first (scale_q16_kernel, one more rounding)
    unsigned char* out8;                            // WM_PREC_FP8: write the output as e4m3 bytes (row stride out_stride bytes) instead of 16-bit
#if WM_DEV_TIMELINE
    unsigned long long* tl;                         // dev build: s_memtime stamps of workgroup 0 ([wave][64]) or null
#endif
};

template <int HD> struct AttnGeom {
    static constexpr int KS = HD * 2 + 16;                      // K row stride (bytes): odd multiple of 16 B
    static constexpr int VS = (HD == 128) ? 320 : 192;          // V row stride (bytes): odd multiple of 64 B
    static constexpr int NKS = HD / 16;                         // QK^T k-steps
    static constexpr int NDT = (HD + 31) / 32;                  // 32-row O^T tiles
    static constexpr int CH = HD / 8;                           // 16-byte chunks per row
    // HD = 80: the last 32-row O^T tile has 16 spare rows.  The V image's pad column HD is set to 1.0 once, so row HD
    // of O^T = sum_k P[k][q] = the softmax denominator, from the matrix pipe instead of 32 v_add per tile (and it is
    // the sum of exactly the rounded P values the numerator uses).  Lane (c, h = 0) holds it in o[NDT-1][LSUM_R].
    static constexpr bool LSUM_IN_O = (HD % 32) != 0;
    static constexpr int LSUM_R = ((HD % 32) / 8) * 4;
    static_assert(!LSUM_IN_O || (HD % 8) == 0, "pad column must fall on accumulator register LSUM_R of half 0");
};

// ---------------------------------------------------------------------------
// The 32x32 accumulator layout, once: register r of tile t in lane half h is row acc_key(t, r, h) of the product -- a key (or a
// rel-pos table row) for S^T = K Q^T, an output dim for O^T = V^T P^T -- and the lane's column is its query c = lane & 31.
// ---------------------------------------------------------------------------
__device__ __forceinline__ constexpr int acc_key(int t, int r, int h) { return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&a)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[t][r] = 0.f;
}

// The maximum over both halves of a query's keys: the other half sits in lane ^ 32.  v_permlane32_swap (vector pipe) instead of
// ds_bpermute (an LDS round trip).
__device__ __forceinline__ float max_across_halves(float mx) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// ---------------------------------------------------------------------------
// fragment readers
// ---------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ typename T::vec8 lds_read_v8(const char* p) {
    return *(const typename T::vec8*)p;
}

// V^T fragment for one 32x32x16 k-step: two transposed reads of 4 keys x 16 dims.  A lane's address inside the V image
// (rows = keys, stride VS): 16-lane group g, half g >> 1 picks keys + 4, g & 1 picks dims + 16.
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
template <int HD>
__device__ __forceinline__ int v_lane_off(int lane) {
    const int g = lane >> 4, lq = (lane >> 2) & 3, lp = lane & 3;
    return (4 * (g >> 1) + lq) * AttnGeom<HD>::VS + (16 * (g & 1) + 4 * lp) * 2;
}
template <class T>
__device__ __forceinline__ typename T::vec8 lds_read_vT_pair(lds_s16x4_ptr first, lds_s16x4_ptr second) {
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(first);
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(second);
    s16x8 r;
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
    r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
    return __builtin_bit_cast(typename T::vec8, r);
}
template <class T>
__device__ __forceinline__ typename T::vec8 lds_read_vT(const char* p_first, int second_off) {
    return lds_read_vT_pair<T>((lds_s16x4_ptr)(p_first), (lds_s16x4_ptr)(p_first + second_off));
}
// the same at (one opaque base register) + (compile-time offset), see lds_base_opaque in attn_glob8.h
template <class T>
__device__ __forceinline__ typename T::vec8 lds_read_vT_at(unsigned base, int off, int second_off) {
    return lds_read_vT_pair<T>((lds_s16x4_ptr)(size_t)(base + off), (lds_s16x4_ptr)(size_t)(base + off + second_off));
}

// S^T[t] += K[tile rows 32t..32t+31] * Q^T over HD, K rows in LDS with stride KS.
template <class T, int HD, int NT>
__device__ __forceinline__ void qk_tile(f32x16 (&s)[NT], const typename T::vec8 (&qf)[AttnGeom<HD>::NKS],
                                        const char* sK, int lane) {
    using G = AttnGeom<HD>;
    const int r31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            typename T::vec8 kf = lds_read_v8<T>(sK + (32 * t + r31) * G::KS + (16 * ks + 8 * h) * 2);
            s[t] = T::mfma32(kf, qf[ks], s[t]);
        }
}

// Online-softmax state of one wave (32 queries, lane = query column + 32*half).
template <int NDT> struct SoftmaxState {
    float m;          // reference point of the exponentials (log2 domain); scores reach the softmax RELATIVE to it (see "Scores" below)
    float l;          // running sum, this lane's half of the keys only
    f32x16 o[NDT];    // O^T accumulators
    __device__ __forceinline__ void init() {
        m = 0.f; l = 0.f;
        zero_acc(o);
    }
};

// Scores (round 4).  Q reaches the kernels multiplied by c1 = softmax scale * log2 e (folded into the q rows of the qkv weight
// before its one rounding; the host launchers' `q_prescaled`, host_attn.h), so the QK^T accumulators ARE the log2-domain scores, and
// everything that used to be added per score on the vector pipe rides the matrix pipe instead:
//   - the kw rel-pos term: the accumulators' initial value (as before);
//   - the per-(query, key tile) scalar -- minus the reference point m -- through ONE extra 16-deep k-step of the QK^T product:
//     B[k][query] holds the scalar as a (hi, lo) pair of 16-bit values (22 / 16 significant bits), A[key][k] is 1.0 at that pair's two
//     k positions and 0 elsewhere, the same for every key of the tile (bias_a_frag / bias_b_const).  The B fragment is rebuilt when m
//     moves.  (The 8-wave kernel's instances without rel-pos; the others add their scalar in front of the exp2 or carry it in the
//     accumulators' initial value, see each kernel.)
// The softmax is then max (the deferred-rescale check), exp2 of the accumulator itself, convert: the FMA per score is gone
// (32 of ~116 vector instructions per 64-key tile in the global kernel).  m moves only when some query's maximum exceeds it by more
// than RESCALE_THR (log2 units) -- and at the first tile, where it becomes that tile's maximum -- so P <= 2^RESCALE_THR: harmless in
// fp32 accumulators and for 16-bit floating P.  When it moves, the tile's scores are corrected on the vector pipe (rare).
constexpr float RESCALE_THR = 6.0f;

// The deferred-rescale step, once.  `mx` = this tile's maximum relative to the reference point st.m, over both lane halves; `ndone`
// = tiles accumulated so far.  The reference point moves at the first tile (to that tile's maximum) and when some query's maximum
// grew past the threshold (by max(mx, 0): never down); l and o are rescaled unless it is the first tile, where they are still 0 and
// alpha is inf when the tile's maximum is below -128 (0 * inf = nan).  Returns whether it moved, and by how much in `d`: the caller
// then corrects what it holds relative to the old reference point.
// (This form -- the whole rule in one body, the tile count rather than a `first` flag -- is the one that leaves the 8-wave kernel's
// code as it was; the window kernel keeps its own copy, see there.  profiles/attn_family/README.md has the forms tried.)
template <int NDT>
__device__ __forceinline__ bool move_reference(SoftmaxState<NDT>& st, float mx, int ndone, float& d) {
    if (ndone == 0 || !__all(mx <= RESCALE_THR)) {
        d = ndone == 0 ? mx : fmaxf(mx, 0.f);
        if (ndone > 0) {
            const float alpha = __builtin_amdgcn_exp2f(-d);
            st.l *= alpha;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) st.o[dt][r] *= alpha;
        }
        st.m += d;
        return true;
    }
    return false;
}

template <class T> __device__ __forceinline__ unsigned one_pair_bits() {
    return std::is_same<T, FP16>::value ? 0x3C003C00u : 0x3F803F80u;           // (1.0, 1.0) as two 16-bit floats
}
// A fragment of the bias k-step for a lane holding k = 8 h .. 8 h + 7: 1.0 at k = 2 pos, 2 pos + 1 if `mine`, else 0
template <class T>
__device__ __forceinline__ typename T::vec8 bias_a_frag(int pos, bool mine) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 a;
#pragma unroll
    for (int d = 0; d < 4; ++d) a[d] = (mine && d == pos) ? one_pair_bits<T>() : 0u;
    return __builtin_bit_cast(typename T::vec8, a);
}
template <class T>
__device__ __forceinline__ void hi_lo(float v, typename T::elem& hi, typename T::elem& lo) {
    hi = T::from_f32(v);
    lo = T::from_f32(v - T::to_f32(hi));
}
// B fragment, no per-tile term: (hi, lo) of `v` at k = 0, 1 (lanes of half 0; bias_a_frag(0, h == 0) selects them)
template <class T>
__device__ __forceinline__ typename T::vec8 bias_b_const(float v) {
    typename T::vec8 b;
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = T::from_f32(0.f);
    typename T::elem hi, lo;
    hi_lo<T>(v, hi, lo);
    b[0] = hi; b[1] = lo;
    return b;
}
// q -> c1 q for callers that hold the reference's plain q (the single-op entry points): out[row][0..cols) = round16(c1 * in[row][0..cols))
template <class T>
__global__ __launch_bounds__(256) void scale_q16_kernel(const u16* __restrict__ in, int in_stride, u16* __restrict__ out, int64_t rows, int cols, float c1) {
    const int cpr = cols / 8;
    const int64_t n = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / cpr;
        const int ch = (int)(i - row * cpr);
        typename T::vec8 v = *(const typename T::vec8*)(in + row * in_stride + ch * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = T::from_f32(T::to_f32(v[j]) * c1);
        *(typename T::vec8*)(out + row * cols + ch * 8) = v;
    }
}

// Set the pad column HD of `rows` V rows (stride VS) to 1.0 (see AttnGeom::LSUM_IN_O).
template <class T, int HD>
__device__ __forceinline__ void v_pad_ones(char* sV, int rows, int tid, int nthreads) {
    using G = AttnGeom<HD>;
    if constexpr (G::LSUM_IN_O) {
        const typename T::elem one = T::from_f32(1.0f);
        for (int r = tid; r < rows; r += nthreads) *(typename T::elem*)(sV + r * G::VS + HD * 2) = one;
    }
}

// ---------------------------------------------------------------------------
// output
// ---------------------------------------------------------------------------
// head `head` of output row `row` (a token of the whole batch) in `base` = p.out (16-bit) or p.out8 (e4m3): the same element offset
template <int HD, class E>
__device__ __forceinline__ E* out_row(E* base, int out_stride, size_t row, int head) { return base + row * out_stride + head * HD; }

// Normalise and store O^T: lane (c = lane&31, h) holds dims acc_key(dt, r, h) of query c.
template <class T, int HD>
__device__ __forceinline__ void store_out(SoftmaxState<AttnGeom<HD>::NDT>& st, u16* out_row, int lane, bool valid, unsigned char* out8_row = nullptr) {
    using G = AttnGeom<HD>;
    const int h = lane >> 5;
    float l;
    if constexpr (G::LSUM_IN_O) l = __shfl(st.o[G::NDT - 1][G::LSUM_R], lane & 31, 64);
    else l = st.l + __shfl_xor(st.l, 32, 64);
    const float inv = 1.0f / l;
    if (!valid) return;
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int d = 32 * dt + 8 * rg + 4 * h;
            if (d < HD) {
                if (out8_row) {                              // wave-uniform: e4m3 A operand of the fp8 proj GEMM (gemm8.h)
                    const f32x4 v{st.o[dt][4 * rg] * inv, st.o[dt][4 * rg + 1] * inv, st.o[dt][4 * rg + 2] * inv, st.o[dt][4 * rg + 3] * inv};
                    *(unsigned*)(out8_row + d) = pack4_e4m3(v);
                } else {
                    typename T::vec4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = T::from_f32_bounded(st.o[dt][4 * rg + j] * inv);     // a convex combination of V rows
                    *(typename T::vec4*)(out_row + d) = o;
                }
            }
        }
}

// The same through a per-wave LDS image [32 queries][ROW_STRIDE bytes]: normalised 16-bit rows are written as the accumulators hold
// them (8 B per lane, one query per lane) and leave as 16-B chunks of whole rows, `row_ptr(r)` giving query r's output row or null.
// A row-per-lane store instruction touches 32 different 128-B lines (20 such stores per item: ~3.4k cycles of an 18k-cycle window
// item in the timeline); a chunked one touches ~8.
template <class T, int HD, class RowPtr>
__device__ __forceinline__ void store_out_rows(SoftmaxState<AttnGeom<HD>::NDT>& st, char* stage, int lane, RowPtr row_ptr) {
    using G = AttnGeom<HD>;
    constexpr int RS = HD * 2 + 16;
    const int c = lane & 31, h = lane >> 5;
    float l;
    if constexpr (G::LSUM_IN_O) l = __shfl(st.o[G::NDT - 1][G::LSUM_R], c, 64);
    else l = st.l + __shfl_xor(st.l, 32, 64);
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int d = 32 * dt + 8 * rg + 4 * h;
            if (d < HD) {
                typename T::vec4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = T::from_f32_bounded(st.o[dt][4 * rg + j] * inv);     // a convex combination of V rows
                *(typename T::vec4*)(stage + c * RS + d * 2) = o;
            }
        }
    constexpr int CH = HD / 8, NCHUNK = 32 * CH;
#pragma unroll
    for (int i = 0; i < (NCHUNK + 63) / 64; ++i) {
        const int e = lane + 64 * i;
        if (e < NCHUNK) {
            const int r = e / CH, ch = e % CH;
            u16* dst = row_ptr(r);
            if (dst) *(s16x8*)(dst + ch * 8) = *(const s16x8*)(stage + r * RS + ch * 16);
        }
    }
}

// ---------------------------------------------------------------------------
// Rel-pos prologue of global attention (64 x 64 grid: tables of 127 rows), for both global kernels.
// ---------------------------------------------------------------------------
// Both table images side by side in `sTab` (the idle K / V ring): 2 x 128 rows x HD 16-bit, row stride KS; rel_w rows 0..127, rel_h
// rows 128..255, row 127 of each zero.  All NTHR threads of the workgroup; the caller's barriers stand around it.
// All of a thread's table chunks are requested before the first is converted (as a rolled loop each load was waited for in turn:
// ~12k cycles of the prologue in the 8-wave kernel's timeline).
template <class T, int HD, int NTHR>
__device__ __forceinline__ void relpos_stage_tables(const float* rel_w, const float* rel_h, char* sTab, int tid) {
    using G = AttnGeom<HD>;
    constexpr int NTC = 256 * (HD / 4) / NTHR;
    static_assert(256 * (HD / 4) % NTHR == 0, "table chunks per thread");
    f32x4 tv[NTC];
#pragma unroll
    for (int i = 0; i < NTC; ++i) {
        const int e = tid + i * NTHR, row = e / (HD / 4), c4 = e % (HD / 4);
        const float* tab = row < 128 ? rel_w : rel_h;
        const int tr = min(row & 127, 126);              // row 127 of an image is zero (below)
        tv[i] = *(const f32x4*)(tab + (size_t)tr * HD + c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < NTC; ++i) {
        const int e = tid + i * NTHR, row = e / (HD / 4), c4 = e % (HD / 4);
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (row & 127) < 127 ? T::from_f32(tv[i][j]) : T::from_f32(0.f);
        *(typename T::vec4*)(sTab + row * G::KS + c4 * 8) = o;
    }
}

// rel_w (registers: the kw-term of this lane's 32 keys per tile, relw) and rel_h (LDS: the kh-term [kh][query] fp32 in `sT`) for
// the wave's 32 queries q0 .. q0 + 31, from the staged table images.  sT: the wave's 32 x 65 floats, first used as [query][65]
// staging.  `between()` runs between the two halves (the dev build's stamp).
template <class T, int HD, class Between>
__device__ __forceinline__ void relpos_terms(f32x16 (&relw)[2], float* sT, const typename T::vec8 (&qf)[AttnGeom<HD>::NKS],
                                             const char* sTab, int q0, float inv_scale, int lane, Between&& between) {
    using G = AttnGeom<HD>;
    const int c = lane & 31, h = lane >> 5;
    const int qh = q0 >> 6, qw0 = q0 & 63;
    float* sRelH = sT;                                 // [kh][query] fp32, aliased with the [query][65] staging
    {   // rel_w: T[c][i] = q_c . table_w[i] for the 127 rows in two passes of 64; lane (c, h) keeps the entries its keys need
        const int qw = qw0 + c;
        zero_acc(relw);
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            f32x16 acc[2];
            zero_acc(acc);
            qk_tile<T, HD, 2>(acc, qf, sTab + pass * 64 * G::KS, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int il = acc_key(t, r, h);
                    sT[c * 65 + il] = acc[t][r];
                }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            // every lane reads a (valid) entry and keeps it by select: as `if`s these were 32 divergent branches per pass
            // (8.2k of the prologue's 26k cycles in the timeline)
            float tv[2][16];                               // all 32 reads in flight, then the selects
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kw = acc_key(t, r, h);
                    tv[t][r] = sT[c * 65 + ((qw + 63 - kw) & 63)];
                }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kw = acc_key(t, r, h);
                    const int idx = qw + 63 - kw;
                    asm volatile("" : "+v"(tv[t][r]));     // the read stays unconditional (hipcc sinks it under the condition otherwise)
                    relw[t][r] = (idx >> 6) == pass ? tv[t][r] * inv_scale : relw[t][r];
                }
            __builtin_amdgcn_s_waitcnt(0xc07f);
        }
    }
    between();
    {   // rel_h: the 64 table rows qh + 63 - kh of this wave's query row, straight from the table image
        const char* sTabH = sTab + 128 * G::KS;
        f32x16 acc[2];
        zero_acc(acc);
        const int r31 = lane & 31;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int row = qh + 63 - (32 * t + r31);
                typename T::vec8 kf = lds_read_v8<T>(sTabH + row * G::KS + (16 * ks + 8 * h) * 2);
                acc[t] = T::mfma32(kf, qf[ks], acc[t]);
            }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kh = acc_key(t, r, h);
                sRelH[kh * 32 + c] = acc[t][r] * inv_scale;
            }
    }
}

// ---------------------------------------------------------------------------
// dev build: one s_memtime stamp of the wave into slot `slot` of its timeline `tl` (in LDS)
// ---------------------------------------------------------------------------
#if WM_DEV_TIMELINE
__device__ __forceinline__ void dev_stamp(unsigned long long* tl, int slot, int lane) {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    if (lane == 0) tl[slot] = t;
}
#endif

}  // namespace wm
