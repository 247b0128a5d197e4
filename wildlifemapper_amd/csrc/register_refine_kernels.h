// Survey registration, refinement (include/wm_hip.h, "Survey registration, refinement"): around the integer peak of a pair,
// the normal equations of one Gauss-Newton step of the brightness-constancy equation -- sub-cell shift, yaw, scale, gain and
// offset -- as 28 integer sums per pair.  No reference behaviour exists; the rule is the header's, and the checker is its
// sequential restatement refine_sums_oracle in tests/register_cases.py.  Every term is an integer, so the kernel equals
// the oracle bit for bit whatever the order of its additions; the 4 x 4 or 6 x 6 solve is the host's (registration.py).
//
// register_refine_kernel: blockIdx.y = pair, blockIdx.x = tile of REFINE_TILE_X x REFINE_TILE_Y cells of A.  The workgroup
// stages its tile of A and the matching tile of B grown by one cell on every side in LDS, one byte per cell; a thread owns
// one column of the tile and REFINE_TILE_Y / 4 consecutive rows, so a wave reads consecutive bytes of a row.  The 28 sums
// are int64 accumulators in registers (every product has two int32 factors: v_mad_i64_i32, or a v_mul_lo / v_mul_hi pair);
// a cell that does not count adds zeros.  They are reduced over the wave by shuffles (28 x 6 steps of two ds_bpermute), over
// the four waves through LDS, and leave as at most 28 64-bit vector atomics per workgroup.  What bounds every read: the pair's check (1 <= gx, gy <= side, uniform over the
// workgroup, before the first store), i < gx and j < gy for A, and row and column < side + 2 * search for B (search >= 1 is
// the launcher's check: B carries the ring).
#pragma once

#include "register_kernels.h"

namespace wm {

constexpr int REFINE_SUMS = 28;                   // 21 products c_k * c_l (k <= l), 6 c_k * r, r * r
constexpr int REFINE_TILE_X = 64;                 // cells east per tile: a lane per column
constexpr int REFINE_TILE_Y = 32;                 // cells north per tile: REFINE_TILE_Y / 4 rows per wave
constexpr int REFINE_ROWS = REFINE_TILE_Y / (REG_THREADS / 64);
constexpr int REFINE_B_X = REFINE_TILE_X + 2, REFINE_B_Y = REFINE_TILE_Y + 2;

static_assert(REFINE_SUMS == WM_REGISTER_REFINE_SUMS, "WM_REGISTER_REFINE_SUMS");
static_assert(REG_THREADS == 4 * REFINE_TILE_X && REFINE_TILE_Y % 4 == 0, "a lane per column, four waves over the rows");
// |x|, |y| <= WM_REGISTER_MAX_SIDE - 1 and |e - w|, |nn - ss| <= 254, so |c2|, |c3| <= 2 * 511 * 254 = 259 588; a square is
// below 6.8e10 and WM_REGISTER_MAX_SIDE^2 of them below 1.8e16
constexpr long long REFINE_C_MAX = 2LL * (WM_REGISTER_MAX_SIDE - 1) * 254;
static_assert(REFINE_C_MAX * REFINE_C_MAX < INT64_MAX / ((long long)WM_REGISTER_MAX_SIDE * WM_REGISTER_MAX_SIDE),
              "the largest sum of a pair fits int64");
static_assert(REFINE_C_MAX < (1LL << 31), "every c_k fits int32");

__global__ __launch_bounds__(REG_THREADS) void register_refine_kernel(
        const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const wm_register_pair* __restrict__ pairs, int search,
        int side, int tiles_x, unsigned long long* __restrict__ sums) {
    __shared__ unsigned char sA[REFINE_TILE_Y][REFINE_TILE_X];
    __shared__ unsigned char sB[REFINE_B_Y][REFINE_B_X];
    __shared__ long long s_wave[REG_THREADS / 64][REFINE_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.y;
    const wm_register_pair pr = pairs[p];
    if (pr.gx < 1 || pr.gx > side || pr.gy < 1 || pr.gy > side) return;      // a bad pair keeps its zeroed sums
    const int i0 = ((int)blockIdx.x % tiles_x) * REFINE_TILE_X, j0 = ((int)blockIdx.x / tiles_x) * REFINE_TILE_Y;
    if (i0 >= pr.gx || j0 >= pr.gy) return;
    const int ext = side + 2 * search;
    const unsigned char* pa = a + (size_t)p * side * side;
    const unsigned char* pb = b + (size_t)p * ext * ext;

    for (int e = tid; e < REFINE_TILE_Y * REFINE_TILE_X; e += REG_THREADS) {
        const int r = e / REFINE_TILE_X, c = e % REFINE_TILE_X, j = j0 + r, i = i0 + c;
        sA[r][c] = j < pr.gy && i < pr.gx ? pa[(size_t)j * side + i] : (unsigned char)0;      // only cells j < gy, i < gx count
    }
    for (int e = tid; e < REFINE_B_Y * REFINE_B_X; e += REG_THREADS) {
        const int r = e / REFINE_B_X, c = e % REFINE_B_X;
        const int J = j0 + search - 1 + r, I = i0 + search - 1 + c;          // >= 0: search >= 1
        sB[r][c] = J < ext && I < ext ? pb[(size_t)J * ext + I] : (unsigned char)0;
    }
    __syncthreads();

    long long acc[REFINE_SUMS];
#pragma unroll
    for (int k = 0; k < REFINE_SUMS; ++k) acc[k] = 0;
    const int x = 2 * (i0 + lane) + 1 - pr.gx;
#pragma unroll
    for (int rr = 0; rr < REFINE_ROWS; ++rr) {
        const int r = wave * REFINE_ROWS + rr;
        const int y = 2 * (j0 + r) + 1 - pr.gy;
        const int av = sA[r][lane], bv = sB[r + 1][lane + 1];
        const int ev = sB[r + 1][lane + 2], wv = sB[r + 1][lane], nv = sB[r + 2][lane + 1], sv = sB[r][lane + 1];
        const int m = (av != 0 && bv != 0 && ev != 0 && wv != 0 && nv != 0 && sv != 0) ? 1 : 0;    // the cell counts
        const int gxv = m * (ev - wv), gyv = m * (nv - sv), res = m * (av - bv);
        const int c[6] = {gxv, gyv, x * gyv - y * gxv, x * gxv + y * gyv, m * bv, m};
        int q = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int l = k; l < 6; ++l) acc[q++] += (long long)c[k] * c[l];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[21 + k] += (long long)c[k] * res;
        acc[27] += (long long)res * res;
    }
#pragma unroll
    for (int k = 0; k < REFINE_SUMS; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
        if (lane == 0) s_wave[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < REFINE_SUMS) {
        long long v = s_wave[0][tid];
#pragma unroll
        for (int k = 1; k < REG_THREADS / 64; ++k) v += s_wave[k][tid];
        if (v) atomicAdd(sums + (size_t)p * REFINE_SUMS + tid, (unsigned long long)v);         // two's complement: signed sums add up
    }
}

}  // namespace wm
