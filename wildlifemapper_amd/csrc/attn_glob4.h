// Global attention, the 4-wave form (attn_common.h has the per-wave layout): key tile = 64 keys = one grid row when REL.
// Two workgroups per CU; takes every query count that is a multiple of 128.  attn_glob8.h holds the 8-wave form that the
// product shapes run.
// grid (nq/128 * heads * batch), 256 threads.
#pragma once
#include "attn_common.h"

namespace wm {

// One key tile of NT*32 keys: s[t] hold the log2-domain scores without the tile's scalar `tile_bias` (the kh rel-pos
// term, 0 without rel-pos) and without the reference point: both are added per score here (one v_add in front of the exp2).  The
// 8-wave kernel's non-rel-pos instances move that add to the matrix pipe (bias k-step, "Scores"); for this kernel's shapes it measured
// slower (head_dim 128: 1257 vs 1190 us, 34 MFMAs per tile against a vector phase that is already the shorter one).  sV: the tile's V rows;
// ndone: key tiles accumulated before this one.
template <class T, int HD, int NT>
__device__ __forceinline__ void softmax_pv(SoftmaxState<AttnGeom<HD>::NDT>& st, f32x16 (&s)[NT], int ndone, float tile_bias, const char* sV, int lane) {
    using G = AttnGeom<HD>;
    float mx0 = -1e30f, mx1 = -1e30f;                       // two chains: a dependent v_max3 issues every ~8 cycles, not 4
#pragma unroll
    for (int r = 0; r < 16; ++r) { mx0 = fmaxf(mx0, s[0][r]); mx1 = fmaxf(mx1, s[NT - 1][r]); }
    // this tile's maximum relative to the reference point (same association as attn_glob8.h)
    const float mx = max_across_halves(fmaxf(mx0, mx1) + (tile_bias - st.m));
    float d;
    move_reference(st, mx, ndone, d);                       // the scores are absolute here: nothing to correct by d
    const float off = tile_bias - st.m;
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f(s[t][r] + off);
            s[t][r] = pv;
            if constexpr (!G::LSUM_IN_O) ls += pv;      // else: row HD of O^T accumulates the sum (V pad column = 1)
        }
    st.l += ls;

    // P^T fragments -> O^T += V^T P^T.  k-step ks covers keys 16*ks .. 16*ks+15 of the tile.
    const int vlo = v_lane_off<HD>(lane);
#pragma unroll
    for (int ks = 0; ks < 2 * NT; ++ks) {
        typename T::vec8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = T::from_f32_bounded(s[ks >> 1][8 * (ks & 1) + j]);     // P <= 2^RESCALE_THR
#pragma unroll
        for (int dt = 0; dt < G::NDT; ++dt) {
            const char* p = sV + (16 * ks) * G::VS + dt * 64 + vlo;
            typename T::vec8 va = lds_read_vT<T>(p, 8 * G::VS);
            st.o[dt] = T::mfma32(va, pb, st.o[dt]);
        }
    }
}

template <int HD, bool REL> struct GlobalLds {
    using G = AttnGeom<HD>;
    static constexpr int WAVE_F = 32 * 65;                                    // floats per wave (padded staging)
    static constexpr int RELH_BYTES = REL ? 4 * WAVE_F * 4 : 0;              // [wave][kh][query] fp32, aliased with [query][65] staging
    static constexpr int K_BYTES = 64 * G::KS, V_BYTES = 64 * G::VS;
    static constexpr int KV_OFF = RELH_BYTES;
    static constexpr int TOTAL = RELH_BYTES + 2 * (K_BYTES + V_BYTES);
    static_assert(!REL || 2 * (K_BYTES + V_BYTES) >= 256 * G::KS, "both rel-pos table images are staged in the two-tile K/V ring");
};

template <class T, int HD, bool REL>
__global__ __launch_bounds__(256, 2) void attn_global_kernel(AttnArgs p) {
    using G = AttnGeom<HD>;
    using L = GlobalLds<HD, REL>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    // 1-D grid, XCD-aware: the workgroups of one (image, head) share K / V and get one XCD's L2 (attn_glob8.h has the measurement)
    const int nqb = p.nq / 128;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int head = (lid / nqb) % p.heads, b = lid / (nqb * p.heads);
    const int q0 = (lid % nqb) * 128 + wave * 32;

    const u16* qb = p.q + ((size_t)b * p.nq) * p.q_stride + head * HD;
    const u16* kb = p.k + ((size_t)b * p.nk) * p.k_stride + head * HD;
    const u16* vb = p.v + ((size_t)b * p.nk) * p.v_stride + head * HD;

    // Q fragments (B operand): lane holds Q[q0+c][16ks + 8h .. +7], in the log2 domain (see "Scores")
    typename T::vec8 qf[G::NKS];
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks)
        qf[ks] = *(const typename T::vec8*)(qb + (size_t)(q0 + c) * p.q_stride + 16 * ks + 8 * h);

    char* sKV = smem + L::KV_OFF;
    f32x16 relw[2];
    float* sRelH = (float*)smem + wave * L::WAVE_F;

    if constexpr (REL) {
        // ---- prologue: rel_w (registers) and rel_h (LDS) for this wave's 32 queries; the K / V ring is idle and holds the tables ----
        __syncthreads();
        relpos_stage_tables<T, HD, 256>(p.rel_w, p.rel_h, sKV, tid);
        __syncthreads();
        relpos_terms<T, HD>(relw, sRelH, qf, sKV, q0, 1.0f / p.scale, lane, [] {});
        __syncthreads();
    }

    // ---- main loop over key tiles of 64 ----
    const int ntiles = p.nk / 64;
    constexpr int NCH = 64 * G::CH;                 // 16-B chunks per K (or V) tile
    constexpr int PER = (NCH + 255) / 256;
    s16x8 kreg[PER], vreg[PER];

    // per-thread source pointers of the staging chunks, advanced by one tile per issue (no per-tile address math)
    const u16* kp[PER];
    const u16* vp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = min(tid + i * 256, NCH - 1);
        kp[i] = kb + (size_t)(e / G::CH) * p.k_stride + (e % G::CH) * 8;
        vp[i] = vb + (size_t)(e / G::CH) * p.v_stride + (e % G::CH) * 8;
    }
    const size_t k_step = (size_t)64 * p.k_stride, v_step = (size_t)64 * p.v_stride;
    auto issue = [&](int) {                          // tiles are requested in order
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (tid + i * 256 < NCH) {
                kreg[i] = *(const s16x8*)kp[i];
                vreg[i] = *(const s16x8*)vp[i];
            }
            kp[i] += k_step;
            vp[i] += v_step;
        }
    };
    v_pad_ones<T, HD>(sKV + L::K_BYTES, 64, tid, 256);
    v_pad_ones<T, HD>(sKV + (L::K_BYTES + L::V_BYTES) + L::K_BYTES, 64, tid, 256);
    auto commit = [&](int buf) {
        char* sK = sKV + buf * (L::K_BYTES + L::V_BYTES);
        char* sV = sK + L::K_BYTES;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + i * 256;
            if (e < NCH) {
                const int key = e / G::CH, ch = e % G::CH;
                *(s16x8*)(sK + key * G::KS + ch * 16) = kreg[i];
                *(s16x8*)(sV + key * G::VS + ch * 16) = vreg[i];
            }
        }
    };

    SoftmaxState<G::NDT> st;
    st.init();
    issue(0);
    commit(0);
    __syncthreads();

    for (int j = 0; j < ntiles; ++j) {
        const int buf = j & 1;
        if (j + 1 < ntiles) issue(j + 1);
        const char* sK = sKV + buf * (L::K_BYTES + L::V_BYTES);
        const char* sV = sK + L::K_BYTES;
        f32x16 s[2];
        float rh = 0.f;
        if constexpr (REL) {
            rh = sRelH[j * 32 + c];                       // kh-term: one scalar per query and tile, added in front of the exp2
#pragma unroll
            for (int t = 0; t < 2; ++t) s[t] = relw[t];    // kw-term: the accumulators' initial value
        } else {
            zero_acc(s);
        }
        qk_tile<T, HD, 2>(s, qf, sK, lane);
        softmax_pv<T, HD, 2>(st, s, j, rh, sV, lane);
        if (j + 1 < ntiles) commit(buf ^ 1);
        __syncthreads();
    }
    const size_t row = (size_t)b * p.nq + q0 + c;
    store_out<T, HD>(st, out_row<HD>(p.out, p.out_stride, row, head), lane, true, p.out8 ? out_row<HD>(p.out8, p.out_stride, row, head) : nullptr);
}

}  // namespace wm
