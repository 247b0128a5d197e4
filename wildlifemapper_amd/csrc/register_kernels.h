// Survey registration (include/wm_hip.h, "Survey registration"): every overlapping pair of frames is rendered onto a common
// ground patch as two uint8 luma planes, and the shift at which they agree is found by an exhaustive integer search.  No
// reference behaviour exists; the rule is the header's, and the checker is its sequential restatement register_oracle in
// tests/register_cases.py.  The render's arithmetic is the coverage's (IEEE double, one rounding per operation, no
// contraction); everything after it is integer, so all three kernels equal the oracle bit for bit.
//
// register_render_kernel: lane = column, a thread owns REG_RENDER_ROWS cells of one column, blockIdx.z = pair, blockIdx.y =
// (plane, block of rows).  A plane is written whole or not at all: the pair's and the frame's checks are uniform over the
// workgroup and come before the first store.  What bounds every read: 0 <= frame < n_frames, 0 <= slot < n_resident, a
// non-null data pointer, the descriptor's (height, width) equal to size[f], and 0 <= u < width, 0 <= v < height from sees.
//
// register_search_kernel<K, ZNCC>, the hot path of both searches: (2S+1)^2 * gx * gy cell pairs per pair of frames.  A
// workgroup owns one tile of REG_TILE_X x tile_rows cells of A, the matching tile of B grown by 2S in both axes, and 256 * K
// consecutive offsets (o = (dy + S) * (2S+1) + (dx + S), lane = consecutive o, so the lanes of a wave read consecutive
// bytes of one or two B rows).  Both tiles sit in LDS as (value dword, mask dword) pairs -- mask byte 0xff where the cell is
// seen -- so one ds_read_b64 fetches four cells with their mask.  A thread walks the tile four cells at a time: the A pair
// is a broadcast read shared by its K offsets; per offset one new B pair (the previous one is kept: a row is walked with a
// sliding dword window), two v_alignbyte_b32 to bring B and its mask to A's byte phase, three ANDs (both operands and the
// mask by (a != 0) & (b != 0), so a cell that either frame does not see adds 0) and one v_bcnt_u32_b32 (8 bits per counted
// cell).  The decomposition, the pair check, the staging, the offset setup, the walk and the flush guard are the same text
// for both metrics; the metric decides three spots under `if constexpr`:
//   SAD (include/wm_hip.h, "Survey registration"; checker: search_oracle in tests/register_cases.py): one v_sad_u8 per 4
//     cells and offset; tile partials go to score by int32 atomics, two per (tile, offset), against tile_rows * 16 steps.
//   correlation (include/wm_hip.h, "Survey registration, correlation search"; checker: zncc_search_oracle in
//     tests/register_cases.py): two v_sad_u8 against 0 (the byte sums) and three v_dot4_u32_u8 (sum a^2, sum b^2, sum
//     ab).  A tile's partials fit 32 bits (the static_assert beside REG_TILE_ROWS_MAX); they go to moments by six 64-bit
//     vector atomics per (tile, offset).
// What keeps every instance at the registers and bytes it had as two kernels: profiles/register_family/README.md.
//
// register_best_kernel, register_zncc_best_kernel: one workgroup per pair scans the table twice -- the best offset, then the
// best outside its 3 x 3 -- in reg_pick, with the metric's candidate, order and output from reg_pick_sad / reg_pick_zncc.
// SAD's order is the header's cross products, the correlation's the score q, three IEEE double operations on exact integers
// (no contraction, no sqrt); both then fall to the unique key (dy^2 + dx^2, dy, dx), so the order is total and the
// reduction's shape is free.
#pragma once

#include "mosaic_kernels.h"
#include "survey_kernels.h"

namespace wm {

constexpr int REG_THREADS = 256;
constexpr int REG_TILE_X = 64;                    // cells east per tile of the search = 16 dwords
constexpr int REG_TILE_DW = REG_TILE_X / 4;
constexpr int REG_RENDER_ROWS = 4;                // cells per thread of the render, consecutive rows of one column
constexpr int REG_RENDER_BLOCK_Y = (REG_THREADS / 64) * REG_RENDER_ROWS;
constexpr int REG_LDS_MAX = 64 * 1024;
constexpr int REG_TILE_ROWS_MAX = 32;             // rows of A per tile of either search: 32, or 16 where 32 do not fit the LDS
// the correlation search keeps a tile's partial sums in 32 bits: at most 64 x 32 cells of 255 * 255 = 133 171 200
static_assert(255LL * 255 * REG_TILE_X * REG_TILE_ROWS_MAX < (1LL << 31), "a tile's sum of products fits 32 bits");

static_assert(sizeof(wm_register_pair) == 32, "wm_register_pair layout");
static_assert(WM_REGISTER_BAD_SLOT == WM_MOSAIC_BAD_SLOT && WM_REGISTER_BAD_SIZE == WM_MOSAIC_BAD_SIZE, "the two residency chains set the same bits");

__host__ __device__ inline bool reg_pair_ok(const wm_register_pair& pr, int n_frames, int side) {
    return pr.frame_a >= 0 && pr.frame_a < n_frames && pr.frame_b >= 0 && pr.frame_b < n_frames && pr.gx >= 1 && pr.gx <= side &&
           pr.gy >= 1 && pr.gy <= side;
}

// dwords of one staged B row: the tile, 2S cells of halo, and one more dword for the window's look-ahead
__host__ __device__ constexpr int reg_b_stride(int search) { return (REG_TILE_X + 2 * search + 3) / 4 + 1; }
__host__ __device__ constexpr int reg_search_lds(int search, int tile_rows) {
    return (tile_rows * REG_TILE_DW + (tile_rows + 2 * search) * reg_b_stride(search)) * (int)sizeof(uint2);
}

__global__ __launch_bounds__(REG_THREADS) void register_render_kernel(
        const frame_desc* __restrict__ frames, int n_resident, const int* __restrict__ slot, const double* __restrict__ g2p,
        const int* __restrict__ size, int n_frames, const wm_register_pair* __restrict__ pairs, double cell, int search, int side,
        int row_blocks, unsigned char* __restrict__ a, unsigned char* __restrict__ b, int* __restrict__ status) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.z;
    const int plane_b = (int)blockIdx.y >= row_blocks ? 1 : 0;
    const int rb = (int)blockIdx.y - plane_b * row_blocks;
    const int s = plane_b ? search : 0;
    const int ext = side + 2 * s;                                // the plane is ext x ext
    const int i = blockIdx.x * 64 + lane, j0 = rb * REG_RENDER_BLOCK_Y + wave * REG_RENDER_ROWS;
    if ((int)blockIdx.x * 64 >= ext || rb * REG_RENDER_BLOCK_Y >= ext) return;
    const bool reporter = blockIdx.x == 0 && rb == 0 && tid == 0;
    const wm_register_pair pr = pairs[p];
    if (!reg_pair_ok(pr, n_frames, side)) { if (reporter) atomicOr(status, WM_REGISTER_BAD_PAIR); return; }
    const int f = plane_b ? pr.frame_b : pr.frame_a;
    const int sl = slot[f];                                      // the residency chain: mirrors mos_cell (mosaic_kernels.h), statement for statement
    if (sl < 0) return;                                          // its frame is not resident in this call
    if (sl >= n_resident) { if (reporter) atomicOr(status, WM_REGISTER_BAD_SLOT); return; }
    const frame_desc fd = frames[sl];
    const int h = size[(size_t)f * 2], w = size[(size_t)f * 2 + 1];
    if (!fd.data) { if (reporter) atomicOr(status, WM_REGISTER_BAD_SLOT); return; }
    if (fd.height != h || fd.width != w) { if (reporter) atomicOr(status, WM_REGISTER_BAD_SIZE); return; }
    if (i >= ext) return;
    const double* bb = g2p + (size_t)f * 6;
    const double b1 = bb[1], b2 = bb[2], b4 = bb[4], b5 = bb[5];
    const double Xc = cov_centre(pr.x0, i - s, cell);
    const double bu = bb[0] * Xc, bv = bb[3] * Xc;
    const double fw = (double)w, fh = (double)h;
    unsigned char* plane = (plane_b ? b : a) + (size_t)p * ext * ext;
    const int lim_x = pr.gx + 2 * s, lim_y = pr.gy + 2 * s;
#pragma unroll
    for (int r = 0; r < REG_RENDER_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= ext) break;
        unsigned char val = 0;
        if (i < lim_x && j < lim_y && h >= 1 && w >= 1) {
            double u, v;
            cov_uv(bu, bv, b1, b2, b4, b5, cov_centre(pr.y0, j - s, cell), u, v);
            if (cov_inside(u, v, fw, fh)) {
                const unsigned char* px = cov_nearest_pixel(fd, w, u, v);
                const int y = (77 * (int)px[0] + 150 * (int)px[1] + 29 * (int)px[2] + 128) >> 8;
                val = (unsigned char)max(1, y);                   // 0 is kept for "not seen"
            }
        }
        plane[(size_t)j * ext + i] = val;
    }
}

// 0xff in every byte of v that is not 0
__device__ __forceinline__ unsigned int reg_nonzero_mask(unsigned int v) {
    unsigned int m = (((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u;
    return (m - (m >> 7)) | m;
}

// four cells of a plane row starting at column c (bytes of a dword, lowest first); columns >= lim read as 0
__device__ __forceinline__ unsigned int reg_load4(const unsigned char* __restrict__ row, int c, int lim) {
    if (c + 3 < lim && (((uintptr_t)(row + c)) & 3) == 0) return *(const unsigned int*)(row + c);
    unsigned int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c + k < lim) v |= (unsigned int)row[c + k] << (8 * k);
    return v;
}

constexpr int REG_MOMENTS = 6;                                   // n, sum a, sum b, sum a^2, sum b^2, sum ab

// what a search keeps per offset: SAD two int32 (sad, n), the correlation REG_MOMENTS 64-bit sums
template <bool ZNCC> struct reg_table { using elem = int; static constexpr int entries = 2; };
template <> struct reg_table<true> { using elem = unsigned long long; static constexpr int entries = REG_MOMENTS; };

template <int K, bool ZNCC>
__global__ __launch_bounds__(REG_THREADS) void register_search_kernel(
        const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, const wm_register_pair* __restrict__ pairs, int search,
        int side, int tile_rows, int tiles_x, int off_blocks, typename reg_table<ZNCC>::elem* __restrict__ table) {
    extern __shared__ uint2 reg_lds[];
    const int tid = threadIdx.x;
    const int p = blockIdx.y;
    const wm_register_pair pr = pairs[p];
    if (pr.gx < 1 || pr.gx > side || pr.gy < 1 || pr.gy > side) return;      // a bad pair keeps its zeroed table
    const int ob = (int)blockIdx.x % off_blocks, tile = (int)blockIdx.x / off_blocks;
    const int i0 = (tile % tiles_x) * REG_TILE_X, j0 = (tile / tiles_x) * tile_rows;
    if (i0 >= pr.gx || j0 >= pr.gy) return;
    const int ext = side + 2 * search, w1 = 2 * search + 1, n_off = w1 * w1;
    const int bs = reg_b_stride(search), b_rows = tile_rows + 2 * search;
    uint2* sA = reg_lds;                                         // [tile_rows][REG_TILE_DW]
    uint2* sB = reg_lds + tile_rows * REG_TILE_DW;               // [b_rows][bs]
    const unsigned char* pa = a + (size_t)p * side * side;
    const unsigned char* pb = b + (size_t)p * ext * ext;

    for (int e = tid; e < tile_rows * REG_TILE_DW; e += REG_THREADS) {
        const int r = e / REG_TILE_DW, c = i0 + (e % REG_TILE_DW) * 4, j = j0 + r;
        const unsigned int v = j < pr.gy ? reg_load4(pa + (size_t)j * side, c, pr.gx) : 0u;       // only cells j < gy, i < gx count
        sA[e] = make_uint2(v, reg_nonzero_mask(v));
    }
    for (int e = tid; e < b_rows * bs; e += REG_THREADS) {
        const int r = e / bs, c = i0 + (e % bs) * 4, j = j0 + r;
        const unsigned int v = j < ext ? reg_load4(pb + (size_t)j * ext, c, ext) : 0u;
        sB[e] = make_uint2(v, reg_nonzero_mask(v));
    }
    __syncthreads();

    // plain local arrays, in this order: accumulators held in a struct or a policy object cost every K > 1 instance an
    // address add per LDS read, and another order renumbers the registers (profiles/register_family/README.md)
    int o[K], sh[K], sad[K], row_b[K];                           // row_b: an index into sB, so every read stays an LDS read
    unsigned int cnt[K], sa[K], sb[K], saa[K], sbb[K], sab[K];   // sad: SAD alone; sa .. sab: the correlation alone
#pragma unroll
    for (int k = 0; k < K; ++k) {
        o[k] = (ob * K + k) * REG_THREADS + tid;
        const int oc = min(o[k], n_off - 1);                     // a thread past the last offset walks the last one and drops it
        const int dyi = oc / w1, dxi = oc - dyi * w1;
        sh[k] = dxi & 3;
        row_b[k] = dyi * bs + (dxi >> 2);
        sad[k] = 0;
        cnt[k] = sa[k] = sb[k] = saa[k] = sbb[k] = sab[k] = 0u;
    }
    for (int r = 0; r < tile_rows; ++r) {
        uint2 lo[K];
#pragma unroll
        for (int k = 0; k < K; ++k) lo[k] = sB[row_b[k]];
#pragma unroll
        for (int c = 0; c < REG_TILE_DW; ++c) {
            const uint2 av = sA[r * REG_TILE_DW + c];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint2 hi = sB[row_b[k] + c + 1];
                const unsigned int bv = __builtin_amdgcn_alignbyte(hi.x, lo[k].x, sh[k]);
                const unsigned int bm = __builtin_amdgcn_alignbyte(hi.y, lo[k].y, sh[k]);
                const unsigned int am = av.x & bm, bmv = bv & av.y;              // a cell that either frame does not see adds 0 to every sum
                if constexpr (ZNCC) {
                    sa[k] = __builtin_amdgcn_sad_u8(am, 0u, sa[k]);
                    sb[k] = __builtin_amdgcn_sad_u8(bmv, 0u, sb[k]);
                    saa[k] = __builtin_amdgcn_udot4(am, am, saa[k], false);
                    sbb[k] = __builtin_amdgcn_udot4(bmv, bmv, sbb[k], false);
                    sab[k] = __builtin_amdgcn_udot4(am, bmv, sab[k], false);
                } else {
                    sad[k] = (int)__builtin_amdgcn_sad_u8(am, bmv, (unsigned int)sad[k]);
                }
                cnt[k] += __popc(av.y & bm);                     // 8 bits per counted cell
                lo[k] = hi;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) row_b[k] += bs;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (o[k] < n_off && cnt[k]) {                            // a counted cell has a, b >= 1: the correlation's six partials are positive
            auto* out = table + ((size_t)p * n_off + o[k]) * reg_table<ZNCC>::entries;
            if constexpr (ZNCC) {
                atomicAdd(out, (unsigned long long)(cnt[k] >> 3));
                atomicAdd(out + 1, (unsigned long long)sa[k]);
                atomicAdd(out + 2, (unsigned long long)sb[k]);
                atomicAdd(out + 3, (unsigned long long)saa[k]);
                atomicAdd(out + 4, (unsigned long long)sbb[k]);
                atomicAdd(out + 5, (unsigned long long)sab[k]);
            } else {
                if (sad[k]) atomicAdd(out, sad[k]);
                atomicAdd(out + 1, (int)cnt[k] >> 3);
            }
        }
}

// the tie key of both searches: the smaller (dy^2 + dx^2, dy, dx)
__device__ __forceinline__ bool reg_key_less(int pdy, int pdx, int qdy, int qdx) {
    const int dp = pdy * pdy + pdx * pdx, dq = qdy * qdy + qdx * qdx;
    if (dp != dq) return dp < dq;
    if (pdy != qdy) return pdy < qdy;
    return pdx < qdx;
}

template <class S> struct reg_cand { S score; int n, dy, dx; };   // an offset and its score; n < 0: no candidate

// What reg_pick asks of a metric: the table's element and entries per offset, the score's type and its value in the empty
// candidate, the header's order (p beats q), offer (the candidate of offset o = (dy, dx), if it has one that `skip` does
// not exclude, replaces `mine` where it beats it) and write (best[2] of the pass, and the correlation's peak).
struct reg_pick_sad {
    using elem = int;
    static constexpr int entries = reg_table<false>::entries;
    using cand = reg_cand<int>;                              // score: the sad
    static constexpr int no_score = -1;
    static __device__ __forceinline__ bool beats(const cand& p, const cand& q) {
        if (p.n < 0) return false;
        if (q.n < 0) return true;
        const long long l = (long long)p.score * q.n, r = (long long)q.score * p.n;
        if (l != r) return l < r;
        return reg_key_less(p.dy, p.dx, q.dy, q.dx);
    }
    template <class Skip>
    static __device__ __forceinline__ void offer(const int* __restrict__ sc, int o, int dy, int dx, int min_cells, Skip skip, cand& mine) {
        const cand c = {sc[o * 2], sc[o * 2 + 1], dy, dx};
        if (c.n < min_cells) return;
        if (skip(dy, dx)) return;
        if (beats(c, mine)) mine = c;
    }
    static __device__ __forceinline__ void write(const cand& top, bool has, int* __restrict__ out, double*) { out[2] = has ? top.score : -1; }
};

struct reg_pick_zncc {
    using elem = long long;
    static constexpr int entries = reg_table<true>::entries;
    using cand = reg_cand<double>;                           // score: q
    static constexpr double no_score = 0.0;
    static __device__ __forceinline__ bool beats(const cand& p, const cand& q) {
        if (p.n < 0) return false;
        if (q.n < 0) return true;
        if (p.score != q.score) return p.score > q.score;
        return reg_key_less(p.dy, p.dx, q.dy, q.dx);
    }
    // the score q of an offset: three IEEE double operations on exact integers, no contraction, no sqrt
    template <class Skip>
    static __device__ __forceinline__ void offer(const long long* __restrict__ mo, int o, int dy, int dx, int min_cells, Skip skip, cand& mine) {
#pragma clang fp contract(off)
        const long long* m = mo + (size_t)o * REG_MOMENTS;
        const long long n = m[0];
        if (n < min_cells) return;
        if (skip(dy, dx)) return;
        const long long sa = m[1], sb = m[2];
        const long long va = n * m[3] - sa * sa, vb = n * m[4] - sb * sb;      // exact: every product is below 2^53
        if (va <= 0 || vb <= 0) return;                                         // a flat plane has no correlation
        const double c = (double)(n * m[5] - sa * sb);
        const cand cd = {(c * fabs(c)) / ((double)va * (double)vb), (int)n, dy, dx};
        if (beats(cd, mine)) mine = cd;
    }
    static __device__ __forceinline__ void write(const cand& top, bool has, int* __restrict__ out, double* __restrict__ peak) {
        out[2] = has ? 1 : 0;
        *peak = has ? top.score : __builtin_nan("");
    }
};

// Both picks: the scan, the 3 x 3 exclusion on the second pass, the wave butterfly, the s_wave combine, the eight ints.
template <class P>
__device__ __forceinline__ void reg_pick(const typename P::elem* __restrict__ table, int search, int min_cells, int* __restrict__ best,
                                         double* __restrict__ peak, typename P::cand* s_wave, typename P::cand& s_first) {
    using cand = typename P::cand;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x, w1 = 2 * search + 1, n_off = w1 * w1;
    const typename P::elem* tab = table + (size_t)p * n_off * P::entries;
    for (int pass = 0; pass < 2; ++pass) {
        cand first = {P::no_score, -1, 0, 0};
        if (pass) first = s_first;
        cand mine = {P::no_score, -1, 0, 0};
        const auto in_first_3x3 = [&](int dy, int dx) { return pass && max(abs(dy - first.dy), abs(dx - first.dx)) < 2; };
        if (!pass || first.n >= 0)
            for (int o = tid; o < n_off; o += REG_THREADS)
                P::offer(tab, o, o / w1 - search, o % w1 - search, min_cells, in_first_3x3, mine);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const cand other = {__shfl_xor(mine.score, d), __shfl_xor(mine.n, d), __shfl_xor(mine.dy, d), __shfl_xor(mine.dx, d)};
            if (P::beats(other, mine)) mine = other;
        }
        if (lane == 0) s_wave[wave] = mine;
        __syncthreads();
        if (tid == 0) {
            cand top = s_wave[0];
#pragma unroll
            for (int k = 1; k < REG_THREADS / 64; ++k)
                if (P::beats(s_wave[k], top)) top = s_wave[k];
            int* out = best + (size_t)p * 8 + pass * 4;
            const bool has = top.n >= 0;
            out[0] = has ? top.dy : 0;
            out[1] = has ? top.dx : 0;
            out[3] = has ? top.n : 0;
            P::write(top, has, out, peak + (size_t)p * 2 + pass);
            s_first = top;
        }
        __syncthreads();
    }
}

// The shared memory is declared in the kernels and not in reg_pick: as a static of a function template it is not internal
// to the code object, and a store that nothing reads (s_first.score) is then kept (profiles/register_family/README.md).
__global__ __launch_bounds__(REG_THREADS) void register_best_kernel(const int* __restrict__ score, int search, int min_cells,
                                                                     int* __restrict__ best) {
    __shared__ reg_pick_sad::cand s_wave[REG_THREADS / 64];
    __shared__ reg_pick_sad::cand s_first;
    reg_pick<reg_pick_sad>(score, search, min_cells, best, nullptr, s_wave, s_first);
}

__global__ __launch_bounds__(REG_THREADS) void register_zncc_best_kernel(const long long* __restrict__ moments, int search, int min_cells,
                                                                          int* __restrict__ best, double* __restrict__ peak) {
    __shared__ reg_pick_zncc::cand s_wave[REG_THREADS / 64];
    __shared__ reg_pick_zncc::cand s_first;
    reg_pick<reg_pick_zncc>(moments, search, min_cells, best, peak, s_wave, s_first);
}

}  // namespace wm
