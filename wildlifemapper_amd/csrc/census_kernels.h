// Survey census (include/wm_hip.h, "Survey census"): the detections of a whole survey, projected to the ground through
// their frames' georeferences and grouped into individuals, at most one detection of any frame per individual.  No
// reference behaviour exists (the reference evaluates single down-scaled images); the rule is the header's, and the
// checker is its sequential restatement census_oracle in tests/ground_oracle.py.
//
// census_kernel, one workgroup per survey, built from the survey merge's pieces (survey_kernels.h: mf_ord keys, the
// any-n mf_bitonic in LDS or global scratch, mf_row / mf_lower_bound windows, a state word per candidate read with
// workgroup-scope atomics, __syncthreads_or rounds, mf_scan ranks):
//   1. every detection's ground point, in double, one rounding per operation -> points (input order); the valid ones
//      become candidates with the key (score descending, input index ascending); extents of the valid points;
//   2. priority order (bitonic sort); point, frame, label and input index of every candidate in that order;
//   3. spatial order: (row of height w, fp32 of X - Xmin), w = 2 * radius plus a margin that covers the fp32 rounding
//      of the keys and of the window's ends;
//   4. rounds.  The sequential rule gives candidate p (priority position) to the nearest eligible individual founded
//      before it, so p's outcome is a function of the outcomes of the higher-priority candidates within 2 * radius: the
//      keepers within radius, and for each of them whether one of its members (within radius of it) is of p's frame.
//      In a round every undecided p scans its window [x - w, x + w] x [y - w, y + w]; if a higher-priority candidate in
//      it is undecided p waits, else p evaluates the rule exactly, in double.  The highest-priority undecided candidate
//      never waits, so a round decides at least one and the loop ends within n rounds; decisions are read with
//      workgroup-scope atomics and never change, so the fixed point is the sequential result whatever the schedule.
//      The round loop is bounded by n; anything still undecided after it sets WM_CENSUS_UNSOLVED and stays at -1.
//   5. members per keeper (atomic counts), keepers' ranks in priority order (block scan) = the individuals' numbers.
#pragma once

#include "survey_kernels.h"

namespace wm {

constexpr int CENSUS_UNDECIDED = -1;             // state: -1, or the priority position of the candidate's keeper
constexpr int CENSUS_HEADER = 256;               // scratch header: int[0] = rounds taken (diagnostic), rest unused
constexpr int CENSUS_SCRATCH_PER_DET = 16 + 8 + 4 + 4 + 4 + 4 + 4;   // cpt, skey, sval, cidx, cframe, clabel, state
constexpr int CENSUS_BLOCKED = 4;                // same-frame neighbours' individuals kept in registers

__device__ __forceinline__ uint64_t census_ord(double d) {      // order-preserving double -> u64
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double census_unord(uint64_t u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

__device__ __forceinline__ bool census_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool census_finite(double d) {
    return ((uint64_t)__double_as_longlong(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

__device__ __forceinline__ float census_f32(double d) {         // fp32 sort key of a non-negative offset, finite
    return fminf((float)d, 3.4028234663852886e38f);
}

// Calls f(q) for every candidate q of the rows [r0, r1] whose x key lies in [xlo, xhi], until f returns true.
template <class F>
__device__ __forceinline__ void census_window(const uint64_t* key, const int* val, int n, int r0, int r1, float xlo, float xhi, F f) {
    for (int r = r0; r <= r1; ++r) {
        const uint64_t row = (uint64_t)r << 32;
        int m = mf_lower_bound(key, n, row | mf_ord(xlo));
        const int m1 = mf_lower_bound(key, n, (row | mf_ord(xhi)) + 1);
        for (; m < m1; ++m)
            if (f(val[m])) return;
    }
}

__global__ __launch_bounds__(MF_THREADS) void census_kernel(
        const float4* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
        const int* __restrict__ box_frame, int n_in, const double* __restrict__ georef, int n_frames, double radius, double r2,
        int same_class, char* __restrict__ scratch, double2* __restrict__ points, int* __restrict__ individual,
        int* __restrict__ keeper, int* __restrict__ members_out, int* __restrict__ count) {
#pragma clang fp contract(off)
    __shared__ uint64_t l_key[MF_LDS_SORT];
    __shared__ int l_val[MF_LDS_SORT];
    __shared__ int s_n, s_wave[MF_THREADS / 64];
    __shared__ unsigned long long s_xmin, s_xmax, s_ymin, s_ymax;
    const int tid = threadIdx.x;
    char* body = scratch + CENSUS_HEADER;
    double2* cpt = (double2*)body;
    uint64_t* g_key = (uint64_t*)(body + (size_t)n_in * 16);
    int* g_val = (int*)(body + (size_t)n_in * 24);
    int* cidx = (int*)(body + (size_t)n_in * 28);
    int* cframe = (int*)(body + (size_t)n_in * 32);
    int* clabel = (int*)(body + (size_t)n_in * 36);
    int* state = (int*)(body + (size_t)n_in * 40);
    if (tid == 0) { s_n = 0; s_xmin = ~0ull; s_ymin = ~0ull; s_xmax = 0ull; s_ymax = 0ull; }
    __syncthreads();

    // 1. ground points (input order) + candidate keys
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < n_in; i += MF_THREADS) {
        const float4 b = boxes[i];
        const float s = scores[i];
        const int f = box_frame[i];
        bool ok = census_finite(b.x) && census_finite(b.y) && census_finite(b.z) && census_finite(b.w) && census_finite(s) &&
                  f >= 0 && f < n_frames;
        double X = nan, Y = nan;
        if (ok) {
            const double* a = georef + (size_t)f * 6;
            const double cx = ((double)b.x + (double)b.z) * 0.5, cy = ((double)b.y + (double)b.w) * 0.5;
            X = (a[0] * cx + a[1] * cy) + a[2];
            Y = (a[3] * cx + a[4] * cy) + a[5];
            ok = census_finite(X) && census_finite(Y);
            if (!ok) { X = nan; Y = nan; }
        }
        points[i] = double2{X, Y};
        individual[i] = -1;
        if (ok) {
            const float sc = s == 0.f ? 0.f : s;                      // -0 ties with +0, as the comparison does
            const int c = atomicAdd(&s_n, 1);
            g_key[c] = ((uint64_t)(~mf_ord(sc)) << 32) | (unsigned)i;
            atomicMin(&s_xmin, (unsigned long long)census_ord(X)); atomicMax(&s_xmax, (unsigned long long)census_ord(X));
            atomicMin(&s_ymin, (unsigned long long)census_ord(Y)); atomicMax(&s_ymax, (unsigned long long)census_ord(Y));
        }
    }
    __syncthreads();
    const int n = s_n;
    const bool in_lds = n <= MF_LDS_SORT;
    uint64_t* key = in_lds ? l_key : g_key;
    int* val = in_lds ? l_val : g_val;

    // 2. priority order
    if (in_lds)
        for (int c = tid; c < n; c += MF_THREADS) l_key[c] = g_key[c];
    __syncthreads();
    mf_bitonic(key, val, n);

    const double x_min = n > 0 ? census_unord(s_xmin) : 0.0, y_min = n > 0 ? census_unord(s_ymin) : 0.0;
    const double x_ext = n > 0 ? census_unord(s_xmax) - x_min : 0.0, y_ext = n > 0 ? census_unord(s_ymax) - y_min : 0.0;
    // Keys are fp32 of offsets in [0, ext]: each is off by at most ext * 2^-24, and so is each end of a window.  Two
    // points whose double test passes at 2 * radius are closer than 2 * radius * (1 + 2^-50) in both axes.
    const float ext = census_f32(fmax(x_ext, y_ext));
    const float rf = census_f32(radius);
    const float w = fminf(2.f * rf * (1.f + 0x1p-20f) + ext * 0x1p-21f + 1e-30f, 3.4028234663852886e38f);

    // 3. candidates in priority order, then the spatial order (row of Y, X)
    for (int c = tid; c < n; c += MF_THREADS) {
        const int i = (int)(key[c] & 0xffffffffu);
        cidx[c] = i;
        cpt[c] = points[i];
        cframe[c] = box_frame[i];
        clabel[c] = labels[i];
        state[c] = CENSUS_UNDECIDED;
    }
    __syncthreads();
    for (int c = tid; c < n; c += MF_THREADS) {
        const double2 p = cpt[c];
        key[c] = ((uint64_t)mf_row(census_f32(p.y - y_min), 0.f, w) << 32) | mf_ord(census_f32(p.x - x_min));
        val[c] = c;
    }
    __syncthreads();
    mf_bitonic(key, val, n);

    // 4. rounds
    int rounds = 0;
    for (; rounds < n; ++rounds) {
        int pending_any = 0;
        for (int c = tid; c < n; c += MF_THREADS) {
            if (mf_load_state(&state[c]) != CENSUS_UNDECIDED) continue;
            const double2 p = cpt[c];
            const int pframe = cframe[c], plabel = clabel[c];
            const float fx = census_f32(p.x - x_min), fy = census_f32(p.y - y_min);
            const float xlo = fx - w, xhi = fx + w;
            const int r0 = mf_row(fy - w, 0.f, w), r1 = mf_row(fy + w, 0.f, w);
            // every higher-priority candidate of the window decided?  the individuals p's own frame already gave to
            bool pending = false;
            int nblk = 0, blk[CENSUS_BLOCKED];
#pragma unroll
            for (int j = 0; j < CENSUS_BLOCKED; ++j) blk[j] = -1;
            census_window(key, val, n, r0, r1, xlo, xhi, [&](int q) {
                if (q >= c) return false;
                const int st = mf_load_state(&state[q]);
                if (st == CENSUS_UNDECIDED) { pending = true; return true; }
                if (cframe[q] == pframe) {
#pragma unroll
                    for (int j = 0; j < CENSUS_BLOCKED; ++j)
                        if (j == nblk) blk[j] = st;
                    ++nblk;
                }
                return false;
            });
            if (pending) { pending_any = 1; continue; }
            // the rule: nearest eligible keeper, ties to the earlier one
            int best = c;
            double best_d2 = 0.0;
            census_window(key, val, n, r0, r1, xlo, xhi, [&](int q) {
                if (q >= c || mf_load_state(&state[q]) != q) return false;         // keepers founded before p
                if (same_class && clabel[q] != plabel) return false;
                const double2 a = cpt[q];
                const double dx = p.x - a.x, dy = p.y - a.y;
                const double d2 = dx * dx + dy * dy;
                if (!(d2 <= r2)) return false;
                if (best != c && !(d2 < best_d2 || (d2 == best_d2 && q < best))) return false;
                bool blocked = false;
#pragma unroll
                for (int j = 0; j < CENSUS_BLOCKED; ++j) blocked |= blk[j] == q;
                if (!blocked && nblk > CENSUS_BLOCKED)
                    census_window(key, val, n, r0, r1, xlo, xhi, [&](int m) {
                        if (m < c && cframe[m] == pframe && mf_load_state(&state[m]) == q) blocked = true;
                        return blocked;
                    });
                if (!blocked) { best = q; best_d2 = d2; }
                return false;
            });
            __hip_atomic_store(&state[c], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (!__syncthreads_or(pending_any)) { ++rounds; break; }
    }
    __syncthreads();

    // 5. members, ranks, outputs
    int* members = g_val;                               // the spatial order is no longer needed
    int* krank = (int*)g_key;
    int unsolved = 0;
    for (int c = tid; c < n; c += MF_THREADS) members[c] = 0;
    __syncthreads();
    for (int c = tid; c < n; c += MF_THREADS) {
        const int st = state[c];
        if (st == CENSUS_UNDECIDED) unsolved = 1;
        else __hip_atomic_fetch_add(&members[st], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    unsolved = __syncthreads_or(unsolved);
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += MF_THREADS) {
        const int c = c0 + tid;
        const bool kept = c < n && state[c] == c;
        int total;
        const int rank = base + mf_scan(kept ? 1 : 0, s_wave, total);
        if (kept) {
            krank[c] = rank;
            keeper[rank] = cidx[c];
            members_out[rank] = members[c];
        }
        base += total;
    }
    __syncthreads();
    for (int c = tid; c < n; c += MF_THREADS) {
        const int st = state[c];
        if (st != CENSUS_UNDECIDED) individual[cidx[c]] = krank[st];
    }
    if (tid == 0) {
        count[0] = base;
        count[1] = unsolved ? WM_CENSUS_UNSOLVED : 0;
        *(int*)scratch = rounds;
    }
}

}  // namespace wm
