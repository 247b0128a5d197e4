// Survey registration, pyramid (include/wm_hip.h, "Survey registration, pyramid"): a stack of uint8 planes reduced by 2 x 2
// rounded means, `level` times, with 0 -- "not seen" -- absorbing: a coarse cell is seen iff every fine cell under it is.  No
// reference behaviour exists; the rule is the header's recursion with its rounding at every level, and the checker is its
// restatement reduce_oracle in tests/pyramid_cases.py.  Everything is integer, so the kernel equals the oracle bit for bit.
//
// register_reduce_kernel<LEVEL>: one pass from level 0 to LEVEL.  Every input byte is read once, only R_LEVEL is written,
// and no intermediate level leaves the registers: there is no LDS, no barrier and no atomic.  A WAVE owns a 64 x 64 tile of
// one plane (blockIdx.y = plane, the four waves of a workgroup take four consecutive tiles of a row of tiles, so the two
// halves of a 128-byte line are read by neighbouring waves); a lane owns 8 x 8 cells, lane = ty * 8 + tx, loaded as eight
// row pieces of two dwords -- eight lanes read the 64 consecutive bytes of a tile row.
//   level 1      on packed bytes: two rows of a dword are widened to 16-bit fields (bytes 0, 2 and bytes 1, 3), added with the
//                rounding 2 in every field and shifted; the "any zero" test is reg_nonzero_mask of both rows, ANDed with
//                itself a byte down.  A lane then holds 4 x 4 cells as 16-bit fields.
//   levels 2, 3  in the lane's registers, on the unpacked fields (16, then 4 values).
//   levels 4-6   across lanes, two shuffles per level (the x partner lane ^ 1, 2, 4, then the y partner lane ^ 8, 16, 32); a
//                horizontal pair travels as its sum, 0 if either cell is 0 (a seen cell is >= 1, so the sum of two is not 0).
// What goes out: level 1 a dword per lane and output row, level 2 two bytes, from level 3 on one byte from the lanes whose
// (tx, ty) are multiples of 2^(LEVEL - 3).
// Paths: with ext % 4 == 0 every row of every plane is dword aligned (in_dev is) and a row piece inside the plane is two
// dword loads; otherwise (ext % 4 == 2), and for the piece that straddles the plane's east edge, the cells are loaded byte by
// byte, columns >= ext as 0.  The same for the stores: dwords (level 1) or byte pairs (level 2) where the output side is a
// multiple of 4 or 2, else bytes.  What bounds every access: row < ext and column < ext for the input, row and column <
// ext >> LEVEL for the output, tile < tiles_x^2 (uniform over a wave: it leaves whole).  ext % 2^LEVEL == 0 is the
// launcher's check, so a coarse cell lies wholly inside the plane or wholly outside it.
#pragma once

#include "register_kernels.h"

namespace wm {

constexpr int REDUCE_TILE = 64;                   // cells per side of a wave's tile = 2^WM_REGISTER_MAX_LEVEL
constexpr int REDUCE_LANE = 8;                    // cells per side of a lane's block: levels 1..3 stay in its registers

static_assert((1 << WM_REGISTER_MAX_LEVEL) == REDUCE_TILE, "the coarsest level is one cell per tile");
static_assert(REDUCE_LANE * REDUCE_LANE == 64 && REDUCE_LANE * 8 == REDUCE_TILE, "8 x 8 lanes of 8 x 8 cells");

typedef unsigned int reduce_u32_a4 __attribute__((aligned(4), may_alias));
typedef unsigned short reduce_u16_a2 __attribute__((aligned(2), may_alias));

// one step of the rule on four cells
__device__ __forceinline__ unsigned int reduce_four(unsigned int a, unsigned int b, unsigned int c, unsigned int d) {
    return (a != 0u && b != 0u && c != 0u && d != 0u) ? (a + b + c + d + 2u) >> 2 : 0u;
}

// one step on two rows of four cells, packed: the two results in the 16-bit fields of the return value
__device__ __forceinline__ unsigned int reduce_rows_packed(unsigned int top, unsigned int bot) {
    const unsigned int f = 0x00ff00ffu;
    const unsigned int sum = (top & f) + ((top >> 8) & f) + (bot & f) + ((bot >> 8) & f) + 0x00020002u;      // <= 4 * 255 + 2 per field
    const unsigned int m = reg_nonzero_mask(top) & reg_nonzero_mask(bot);
    return (sum >> 2) & f & m & (m >> 8);
}

// eight cells of a plane row from column c on, as two dwords (lowest byte first); columns >= lim read as 0
__device__ __forceinline__ uint2 reduce_load8(const unsigned char* __restrict__ row, int c, int lim, bool dwords) {
    if (dwords && c + 7 < lim) {
        const reduce_u32_a4* q = (const reduce_u32_a4*)(row + c);
        return make_uint2(q[0], q[1]);
    }
    unsigned int lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c + k < lim) lo |= (unsigned int)row[c + k] << (8 * k);
        if (c + 4 + k < lim) hi |= (unsigned int)row[c + 4 + k] << (8 * k);
    }
    return make_uint2(lo, hi);
}

template <int LEVEL>
__global__ __launch_bounds__(REG_THREADS) void register_reduce_kernel(const unsigned char* __restrict__ in, int ext, int tiles_x,
                                                                       unsigned char* __restrict__ out) {
    static_assert(LEVEL >= 1 && LEVEL <= WM_REGISTER_MAX_LEVEL, "1 <= level <= WM_REGISTER_MAX_LEVEL");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = (int)blockIdx.x * (REG_THREADS / 64) + wave;
    if (tile >= tiles_x * tiles_x) return;                       // uniform over the wave, and nothing below waits for another wave
    const int tx = lane & 7, ty = lane >> 3;
    const int i0 = (tile % tiles_x) * REDUCE_TILE + tx * REDUCE_LANE, j0 = (tile / tiles_x) * REDUCE_TILE + ty * REDUCE_LANE;
    const int oe = ext >> LEVEL;
    const unsigned char* pin = in + (size_t)blockIdx.y * ext * ext;
    unsigned char* pout = out + (size_t)blockIdx.y * oe * oe;

    // level 0 -> 1: eight row pieces, two rows at a time; one[r][h] holds cells (r, 2h) and (r, 2h + 1) of the lane's 4 x 4
    const bool dwords = (ext & 3) == 0;
    unsigned int one[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + 2 * r;
        uint2 top = make_uint2(0u, 0u), bot = top;
        if (j < ext && i0 < ext) {                               // ext is even: row j + 1 is inside with row j
            top = reduce_load8(pin + (size_t)j * ext, i0, ext, dwords);
            bot = reduce_load8(pin + (size_t)(j + 1) * ext, i0, ext, dwords);
        }
        one[r][0] = reduce_rows_packed(top.x, bot.x);
        one[r][1] = reduce_rows_packed(top.y, bot.y);
    }
    if constexpr (LEVEL == 1) {
        const int oi = i0 >> 1, oj = j0 >> 1;
        const bool whole = (oe & 3) == 0;                        // then every output row is dword aligned (out_dev is)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (oj + r >= oe || oi >= oe) continue;
            const unsigned int v = (one[r][0] & 0xffu) | ((one[r][0] >> 16) << 8) | ((one[r][1] & 0xffu) << 16) | ((one[r][1] >> 16) << 24);
            unsigned char* q = pout + (size_t)(oj + r) * oe + oi;
            if (whole) {
                *(reduce_u32_a4*)q = v;                          // oi % 4 == 0 and oe % 4 == 0: all four are inside
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (oi + k < oe) q[k] = (unsigned char)(v >> (8 * k));
            }
        }
        return;
    } else {
        // level 1 -> 2: the lane's 2 x 2
        unsigned int two[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const unsigned int t = one[2 * r][h], b = one[2 * r + 1][h];
                two[r][h] = reduce_four(t & 0xffffu, t >> 16, b & 0xffffu, b >> 16);
            }
        if constexpr (LEVEL == 2) {
            const int oi = i0 >> 2, oj = j0 >> 2;
            const bool whole = (oe & 1) == 0;                    // then every byte pair is 2-byte aligned and inside
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (oj + r >= oe || oi >= oe) continue;
                unsigned char* q = pout + (size_t)(oj + r) * oe + oi;
                if (whole) {
                    *(reduce_u16_a2*)q = (unsigned short)(two[r][0] | (two[r][1] << 8));
                } else {
                    q[0] = (unsigned char)two[r][0];
                    if (oi + 1 < oe) q[1] = (unsigned char)two[r][1];
                }
            }
            return;
        } else {
            // level 2 -> 3: the lane's one value; then LEVEL - 3 steps across lanes
            unsigned int v = reduce_four(two[0][0], two[0][1], two[1][0], two[1][1]);
#pragma unroll
            for (int b = 0; b < LEVEL - 3; ++b) {
                const unsigned int h = (unsigned int)__shfl_xor((int)v, 1 << b);
                const unsigned int s = (v != 0u && h != 0u) ? v + h : 0u;
                const unsigned int t = (unsigned int)__shfl_xor((int)s, 8 << b);
                v = (s != 0u && t != 0u) ? (s + t + 2u) >> 2 : 0u;              // the same in all four lanes of the 2 x 2
            }
            constexpr int sh = LEVEL - 3, low = (1 << sh) - 1;
            const int oi = i0 >> LEVEL, oj = j0 >> LEVEL;
            if ((tx & low) == 0 && (ty & low) == 0 && oi < oe && oj < oe) pout[(size_t)oj * oe + oi] = (unsigned char)v;
        }
    }
}

}  // namespace wm
