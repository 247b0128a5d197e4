// Window attention (attn_common.h has the per-wave layout and the online softmax): one workgroup per (tile, window, head); all 196 keys of the
// window (incl. padded tokens, whose k/v are the qkv bias) resident in LDS.
// grid (25, heads, batch), 448 threads = 7 waves, wave w owns query slots 32w..32w+31.
//
// Rel-pos bias per wave: T[c][i] = q_c . table[i] by one MFMA pass over the 64-row
// table image (rel_h rows 0..26, rel_w rows 32..58), staged per wave in LDS; each
// lane then gathers its query's 14 + 14 values U[kh] = T[qh-kh+13], V[kw] = T[32+qw-kw+13]
// into registers.  Key slots are laid out 14 x 16 (two zero pad columns), so that in the
// fully unrolled key loop a score's bias is one add of two registers (see the key loop).
#pragma once
#include "attn_common.h"

namespace wm {

template <int HD> struct WindowLds {
    using G = AttnGeom<HD>;
    static constexpr int NKEY = 224;                                       // 196 padded to 7 x 32
    static constexpr int NWAVE = 7;
    static constexpr int K_BYTES = NKEY * G::KS, V_BYTES = NKEY * G::VS;
    static constexpr int TAB_BYTES = 64 * G::KS;                           // rel_h rows 0..26, rel_w rows 32..58
    static constexpr int T_BYTES = NWAVE * 32 * 65 * 4;                    // per wave [query][65] fp32
    static constexpr int K_OFF = 0, V_OFF = K_BYTES, TAB_OFF = V_OFF + V_BYTES, T_OFF = TAB_OFF + TAB_BYTES;
    static constexpr int TOTAL = T_OFF + T_BYTES;
};

template <class T, int HD>
__global__ __launch_bounds__(448, 2) void attn_window_kernel(AttnArgs p, int nitems) {
    using G = AttnGeom<HD>;
    using L = WindowLds<HD>;
    constexpr int WS = 14, GRID = 64, NWIN = 5, NTOK = WS * WS, NTHR = 448;
    constexpr int NPF = (L::NKEY * G::CH) / NTHR;                // 16-byte K (and V) chunks per thread per item
    static_assert((L::NKEY * G::CH) % NTHR == 0, "staging split");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int D = p.heads * HD;
    const float inv_scale = 1.0f / p.scale;

    char* sK = smem + L::K_OFF;
    char* sV = smem + L::V_OFF;
    char* sTab = smem + L::TAB_OFF;
    float* sT = (float*)(smem + L::T_OFF) + wave * (32 * 65);

    // Persistent: one workgroup per CU walks items (tile, window, head).  All 196 keys of a window live in
    // LDS (one workgroup per CU), so nothing else on the CU could hide the latency of staging them: the next
    // item's K / V chunks and Q fragments are fetched into registers while the current item computes.
    // Item order: heads of one window are neighbours and, through the XCD remap, share an L2.
    auto decode = [&](int item, int& b, int& win, int& head) {
        head = item % p.heads;
        win = (item / p.heads) % (NWIN * NWIN);
        b = item / (p.heads * NWIN * NWIN);
    };

    s16x8 kreg[NPF], vreg[NPF];
    auto prefetch_kv = [&](int item) {
        int b, win, head;
        decode(item, b, win, head);
        const int wy = win / NWIN, wx = win % NWIN;
        const u16* kbase = p.k + ((size_t)b * GRID * GRID) * p.k_stride + head * HD;
        const u16* vbase = p.v + ((size_t)b * GRID * GRID) * p.v_stride + head * HD;
        // the chunk coordinates are re-derived per item from an opaque copy of tid: hoisted out of the item loop they were spilled, and
        // every reload (scratch = vector memory) came with a vmcnt(0) that drained the prefetch loads issued before it
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid_o + i * NTHR;
            const int key = e / G::CH, ch = e % G::CH;                                  // key slot = 16 kh + kw (kw 14, 15: zero rows)
            // A token outside the image is zero after norm1, so its qkv row is the bias (image_encoder.py:190-194, 281); the two pad
            // columns of the 14 x 16 slot layout take the bias row too: their scores carry the -1e30 column bias, so P = 0 exactly
            // whatever finite K / V they hold.  The row pointer is SELECTED bitwise -- as `if`s this was two exec-mask branches per
            // chunk, and converting the fp32 bias here put 4 loads and a vmcnt(0) in the middle of every edge window's prefetch
            // (timeline: 3-9k of an item's 23k cycles went into issuing it).
            const int y = wy * WS + (key >> 4), x = wx * WS + (key & 15);
            const bool in = (key & 15) < WS && y < GRID && x < GRID;
            const size_t tok = (size_t)(min(y, GRID - 1) * GRID + min(x, GRID - 1));
            const size_t msk = (size_t)0 - (size_t)in;
            const u16* krow = (const u16*)(((size_t)(kbase + tok * p.k_stride) & msk) | ((size_t)(p.qkv_bias16 + D + head * HD) & ~msk));
            const u16* vrow = (const u16*)(((size_t)(vbase + tok * p.v_stride) & msk) | ((size_t)(p.qkv_bias16 + 2 * D + head * HD) & ~msk));
            const s16x8 kv8 = *(const s16x8*)(krow + ch * 8);
            const s16x8 vv8 = *(const s16x8*)(vrow + ch * 8);
            kreg[i] = kv8;
            vreg[i] = vv8;
        }
    };
    auto commit_kv = [&]() {
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const int e = tid + i * NTHR;
            const int key = e / G::CH, ch = e % G::CH;
            *(s16x8*)(sK + key * G::KS + ch * 16) = kreg[i];
            *(s16x8*)(sV + key * G::VS + ch * 16) = vreg[i];
        }
    };
    // this wave's 32 query slots of an item: validity, token, Q fragments
    const int qi = wave * 32 + c;                         // slot in the window (0..223)
    const int qh = qi / WS, qw = qi - qh * WS;
    struct QInfo { bool valid; size_t row; };
    auto q_info = [&](int item) {
        int b, win, head;
        decode(item, b, win, head);
        const int y = (win / NWIN) * WS + qh, x = (win % NWIN) * WS + qw;
        const bool valid = (qi < NTOK) && (y < GRID) && (x < GRID);
        const size_t tok = valid ? (size_t)(y * GRID + x) : 0;
        return QInfo{valid, (size_t)b * GRID * GRID + tok};
    };
    // (Fetching Q as 16-B chunks of whole rows -- ~14 lines per load instruction instead of 32 -- and forming the fragments through
    // LDS was tried: the five divisions per lane and the LDS round trip cost more than the lines saved, +4 % per launch.)
    auto load_q = [&](typename T::vec8 (&qf)[G::NKS], int item) {
        int b, win, head;
        decode(item, b, win, head);
        const QInfo qi_ = q_info(item);
        const u16* src = p.q + qi_.row * p.q_stride + head * HD;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks) qf[ks] = *(const typename T::vec8*)(src + 16 * ks + 8 * h);
    };

    // rel-pos tables: the same for every item of this launch
    for (int e = tid; e < 64 * (HD / 4); e += NTHR) {
        const int row = e / (HD / 4), c4 = e % (HD / 4);
        const int tr = row & 31;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (tr < 2 * WS - 1) v = *(const f32x4*)((row < 32 ? p.rel_h : p.rel_w) + (size_t)tr * HD + c4 * 4);
        typename T::vec4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = T::from_f32(v[j]);
        *(typename T::vec4*)(sTab + row * G::KS + c4 * 8) = o;
    }

    const int Gd = gridDim.x;
    int item = xcd_remap(blockIdx.x, Gd);
    if (item >= nitems) return;
    typename T::vec8 qf[G::NKS], qn[G::NKS];
    prefetch_kv(item);
    load_q(qf, item);
    commit_kv();
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) asm volatile("" : "+v"(qf[ks]));      // landed before the loop, as at its back edge (below)

    v_pad_ones<T, HD>(sV, L::NKEY, tid, NTHR);            // the staging never touches the pad columns again
    __syncthreads();

#if WM_DEV_TIMELINE
    // dev: stamps of workgroup 0 (items 1..3 of its walk), 16 per item: 0 top, 1 prefetch issued, 2 rel-pos U / V ready, 3..6 key steps,
    // 7 stored, 8 barrier, 9 K / V committed, 10 barrier
    unsigned long long* tls = (unsigned long long*)(smem + L::TOTAL) + wave * 64;
    const bool tl_on = p.tl && blockIdx.x == 0;
    int tl_it = 0;
    auto stamp = [&](int k) {
        if (tl_on && tl_it >= 1 && tl_it < 4) dev_stamp(tls, (tl_it - 1) * 16 + k, lane);
    };
#define WM_WIN_STAMP(k) stamp(k)
#else
#define WM_WIN_STAMP(k)
#endif
    while (true) {
        const int next = item + Gd;
        const bool has_next = next < nitems;
        WM_WIN_STAMP(0);
        if (has_next) prefetch_kv(next);                  // in flight during this item's compute
        WM_WIN_STAMP(1);
        // T[c][i]: i<32 -> q.rel_h[i], i>=32 -> q.rel_w[i-32], pre-divided by the softmax scale
        float U[WS], V[WS];
        {
            f32x16 acc[2];
            zero_acc(acc);
            qk_tile<T, HD, 2>(acc, qf, sTab, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) sT[c * 65 + acc_key(t, r, h)] = acc[t][r] * inv_scale;
            // table rows 27..31 are zero, so out-of-window slots (qh, qw up to 15) read zeros
#pragma unroll
            for (int k = 0; k < WS; ++k) {
                U[k] = sT[c * 65 + (qh - k + WS - 1)];
                V[k] = sT[c * 65 + 32 + (qw - k + WS - 1)];
            }
        }
        WM_WIN_STAMP(2);
        SoftmaxState<G::NDT> st;
        st.init();
        // Key slots are laid out 14 rows (kh) x 16 columns (kw; 14 and 15 are zero rows, masked through the bias): a 32-key MFMA
        // tile is 2 kh rows, so for accumulator register r of lane half h the key is kh = 2 (tile) + (r >> 3),
        // kw = (r & 3) + 8 ((r >> 2) & 1) + 4 h: kh is a compile-time constant and kw depends on the lane only through h.
        // Each lane therefore pre-selects its 8 kw values once (Vsel, -1e30 for the two pad columns) and a score's rel-pos
        // bias is ONE add of two registers, U[kh] + Vsel[idx]; the 224 slots are 3 steps of 64 keys + 1 of 32.
        float Vsel[8];
#pragma unroll
        for (int i8 = 0; i8 < 8; ++i8) {
            const int kw0 = (i8 & 3) + 8 * (i8 >> 2);                              // half 0; half 1: + 4
            Vsel[i8] = h ? (kw0 + 4 < WS ? V[kw0 + 4 < WS ? kw0 + 4 : 0] : -1e30f) : V[kw0 < WS ? kw0 : 0];
        }
        // Key loop in 7 half-steps of 32 keys (two kh rows), software-pipelined inside the wave: QK^T of half-step i + 1 is ISSUED
        // before the exponentials of half-step i, so the matrix pipe works under this wave's own softmax (the two waves of a SIMD
        // overlap only by chance: timeline, 7k cycles of key loop per wave, 14k of a 17k-cycle item on a two-wave SIMD).  Two score
        // tiles of 16 registers alternate -- the same 32 registers the 64-key step held.
        // Scores are log2-domain and relative to st.m (attn_common.h "Scores"): q carries c1, and -m rides in the kw bias registers (Vsel),
        // i.e. in the accumulators' initial value, so a probability is exp2 of the accumulator itself (no FMA per score).
        {
            f32x16 sp[2][1];
            auto s_init = [&](f32x16& d, int i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r] = U[2 * i + (r >> 3)] + Vsel[(r & 3) + 4 * ((r >> 2) & 1)];
            };
            s_init(sp[0][0], 0);
            qk_tile<T, HD, 1>(sp[0], qf, sK, lane);
            // v_lane_off (attn_common.h), written out: through the helper the head_dim 64 instances change by one instruction
            const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
            const int vlo = (4 * (g >> 1) + lq) * G::VS + (16 * (g & 1) + 4 * lp) * 2;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                f32x16& cur = sp[i & 1][0];
                float mx0 = -1e30f, mx1 = -1e30f;
#pragma unroll
                for (int r = 0; r < 8; ++r) { mx0 = fmaxf(mx0, cur[r]); mx1 = fmaxf(mx1, cur[8 + r]); }
                const float mx = max_across_halves(fmaxf(mx0, mx1));
                // move_reference (attn_common.h), written out: through the helper -- in any of the forms tried -- hipcc orders this loop's
                // vector instructions and LDS reads differently (profiles/attn_family/README.md).  Keep the two in step.
                if (i == 0 || !__all(mx <= RESCALE_THR)) {          // the reference point moves: first half-step, or a maximum grew past the threshold
                    const float d = i == 0 ? mx : fmaxf(mx, 0.f);    // (move_reference)
                    if (i > 0) {
                        const float alpha = __builtin_amdgcn_exp2f(-d);
                        st.l *= alpha;
#pragma unroll
                        for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) st.o[dt][r] *= alpha;
                    }
                    st.m += d;
#pragma unroll
                    for (int r = 0; r < 16; ++r) cur[r] -= d;
#pragma unroll
                    for (int i8 = 0; i8 < 8; ++i8) Vsel[i8] -= d;   // the following half-steps start from the new reference point
                }
                // From here the order is written out and fenced (sched_barrier): left alone, hipcc clusters the 16 exponentials and
                // puts all 11 MFMAs behind them.  QK^T(i + 1): one MFMA, then three or four scores' exponentials, five times; then
                // P V(i): one MFMA per ~4 vector instructions (the converts of the second P fragment, the next tile's bias sums).
                float ls = 0.f;
                const bool more = i + 1 < 7;
                f32x16& nxt = sp[(i + 1) & 1][0];
                const char* kn = sK + (i + 1) * 32 * G::KS + (lane & 31) * G::KS + 16 * h;
                if (more) s_init(nxt, i + 1);
                typename T::vec8 kf[G::NKS];                                // K fragments: two requested ahead of their MFMA
                if (more) { kf[0] = lds_read_v8<T>(kn); kf[1] = lds_read_v8<T>(kn + 32); }
                __builtin_amdgcn_sched_barrier(0);
                constexpr int EPG = (16 + G::NKS - 1) / G::NKS;             // exponentials per MFMA gap
#pragma unroll
                for (int ks = 0; ks < G::NKS; ++ks) {
                    if (more) {
                        nxt = T::mfma32(kf[ks], qf[ks], nxt);
                        if (ks + 2 < G::NKS) kf[ks + 2] = lds_read_v8<T>(kn + 32 * (ks + 2));
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = ks * EPG; r < min(16, (ks + 1) * EPG); ++r) {
                        const float pv = __builtin_amdgcn_exp2f(cur[r]);
                        cur[r] = pv;
                        if constexpr (!G::LSUM_IN_O) ls += pv;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                st.l += ls;
                typename T::vec8 pb0, pb1;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) pb0[jj] = T::from_f32_bounded(cur[jj]);
                const char* vp = sV + (i * 32) * G::VS + vlo;
                typename T::vec8 va[G::NDT], vb[G::NDT];                    // V^T fragments of the two 16-key halves
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) va[dt] = lds_read_vT<T>(vp + dt * 64, 8 * G::VS);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) {
                    st.o[dt] = T::mfma32(va[dt], pb0, st.o[dt]);
                    vb[dt] = lds_read_vT<T>(vp + 16 * G::VS + dt * 64, 8 * G::VS);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int jj = dt * 3; jj < min(8, dt * 3 + 3); ++jj) pb1[jj] = T::from_f32_bounded(cur[8 + jj]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (G::NDT * 3 < 8) {
#pragma unroll
                    for (int jj = G::NDT * 3; jj < 8; ++jj) pb1[jj] = T::from_f32_bounded(cur[8 + jj]);
                }
#pragma unroll
                for (int dt = 0; dt < G::NDT; ++dt) st.o[dt] = T::mfma32(vb[dt], pb1, st.o[dt]);
                if (i == 1 || i == 3 || i == 5) WM_WIN_STAMP(3 + i / 2);
            }
        }
        {
            int b, win, head;
            decode(item, b, win, head);
            WM_WIN_STAMP(6);
            // the next item's Q fragments: requested here, where the score / P / bias registers are dead (beside the K / V staging
            // registers they cost 4 spills, and each spill reload's vmcnt(0) serialised the prefetch: timeline), landed by the commit
            if (has_next) load_q(qn, next);
            if (p.out8) {
                const QInfo qo = q_info(item);
                store_out<T, HD>(st, out_row<HD>(p.out, p.out_stride, qo.row, head), lane, qo.valid, out_row<HD>(p.out8, p.out_stride, qo.row, head));
            } else {
                const int wy = win / NWIN, wx = win % NWIN;
                store_out_rows<T, HD>(st, (char*)sT, lane, [&](int r) -> u16* {
                    const int slot = wave * 32 + r;
                    const int sh = slot / WS, sw = slot - sh * WS;
                    const int y = wy * WS + sh, x = wx * WS + sw;
                    const bool ok = slot < NTOK && y < GRID && x < GRID;
                    return ok ? out_row<HD>(p.out, p.out_stride, (size_t)b * GRID * GRID + (size_t)(y * GRID + x), head) : nullptr;
                });
            }
        }
        WM_WIN_STAMP(7);
        if (!has_next) break;
        __syncthreads();                                  // every wave is done with this item's K / V
        WM_WIN_STAMP(8);
        commit_kv();
        WM_WIN_STAMP(9);
        // the Q fragments must have LANDED here: left to hipcc, their vmcnt wait sits at the first MFMA of the next item, behind that
        // item's K / V prefetch in the in-order counter -- the whole prefetch latency exposed at every item start (timeline: 3-4k cycles)
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks) { qf[ks] = qn[ks]; asm volatile("" : "+v"(qf[ks])); }

        item = next;
        __syncthreads();
        WM_WIN_STAMP(10);
#if WM_DEV_TIMELINE
        ++tl_it;
#endif
    }
#if WM_DEV_TIMELINE
    __syncthreads();
    if (tl_on && lane == 0)
        for (int i = 0; i < 64; ++i) p.tl[wave * 64 + i] = tls[i];
#endif
}

}  // namespace wm
