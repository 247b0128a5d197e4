// Large-frame and survey front end: overlapping 1024 x 1024 tiles cut out of frames of any size, and
// the cross-tile merge of their detections, for one or many frames per launch.  No reference behaviour exists for this
// step (the reference down-scales whole frames, dataloader_coco.py:288); the checker is the numpy restatement in
// oracle/tiling_oracle.py.
//   * tile_frames_u8_kernel: one model batch cut from several frames (per-tile frame index): ToTensor + Normalize
//     (normalize_u8), zeros where a tile reaches past its frame.
//   * merge_frames_nms_kernel<MF_NMS>: per frame (a segment of tiles), the slots that survived their own tile's NMS move to
//     frame coordinates and compete in one more greedy class-agnostic NMS (descending score, ties by ascending slot): an
//     animal seen by two overlapping tiles is reported once.  Survivors carry WM_FLAG_MERGED and nms_rank = their
//     position in the frame's merged list (-1 otherwise).  No limit on tiles per frame.
//   * merge_frames_nms_kernel<MF_FUSE>: the same candidates and order, greedy absorption instead of suppression: a keeper
//     absorbs every later unabsorbed candidate of another tile whose intersection over the smaller box exceeds fuse_thr,
//     and its detection's box is the union of its members' boxes -- an animal cut by a tile seam is reported once, with
//     its whole box.
#pragma once

#include "wm_common.h"

namespace wm {

// Mirrors wm_frame_desc of include/wm_hip.h (16 bytes).
struct frame_desc {
    const unsigned char* data;
    int height, width;
};

// tiles[n][3] = (frame index, y0, x0).  A tile whose frame index is out of range is written as zeros.
__global__ __launch_bounds__(256) void tile_frames_u8_kernel(const frame_desc* __restrict__ frames, int n_frames,
                                                             const int* __restrict__ tiles, float* __restrict__ out, int n) {
    const int64_t total = (int64_t)n * 1024 * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int x4 = (int)(i & 255) * 4;
        const int y = (int)((i >> 8) & 1023);
        // one tile row per 256 threads, so t is wave-uniform: the tile's row and its frame descriptor are scalar loads
        const int64_t t = __builtin_amdgcn_readfirstlane((int)(i >> 18));
        const int f = tiles[3 * t];
        f32x4 v[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        if (f >= 0 && f < n_frames) {
            const frame_desc fd = frames[f];
            const int H = fd.height, W = fd.width;
            const int fy = tiles[3 * t + 1] + y, fx0 = tiles[3 * t + 2] + x4;
            if (fy >= 0 && fy < H) {
                // a global, not generic, pointer: global_load instead of flat_load for the pixels
                const auto* row = (const __attribute__((address_space(1))) unsigned char*)fd.data + (int64_t)fy * W * 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int fx = fx0 + j;
                    if (fx >= 0 && fx < W) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) v[c][j] = normalize_u8(row[(int64_t)fx * 3 + c], c);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)(out + ((t * 3 + c) * 1024 + y) * (int64_t)1024 + x4) = v[c];
    }
}

// ---------------------------------------------------------------------------
// Segmented cross-tile merge.  One workgroup per frame, every step in that workgroup (workgroups meet only at kernel
// boundaries; no inter-workgroup hand-off):
//   1. compact the frame's candidates (WM_FLAG_NMS) as 64-bit priority keys (~score order << 32 | slot), write every
//      slot's output record (frame-coordinate box, WM_FLAG_MERGED clear, nms_rank -1);
//   2. bitonic-sort the keys: candidate c of the frame = its position in (score desc, slot asc) order;
//   3. frame-coordinate boxes per candidate; the largest box width / height of the frame;
//   4. bitonic-sort the candidates by (row, x0) -- rows of the largest box height -- so the boxes a box can intersect
//      lie in <= a few rows, each a contiguous x0 range found by binary search (no storage beyond O(candidates));
//   5. resolve greedy NMS by rounds: a candidate is kept when every higher-priority box that would suppress it is
//      decided and none is kept, suppressed as soon as one of them is kept.  The fixed point is sequential greedy NMS;
//      the rounds number the longest dependency chain;
//   6. survivors' nms_rank = prefix count of kept in priority order; records and the compacted detection list.
// The IoU test is postprocess_nms_kernel's: inter / (area_a + area_p - inter) > iou_thr, un-contracted, the
// higher-priority box as `a`.  Pairs with inter == 0 can never suppress (iou_thr >= 0), so only boxes whose interiors
// meet are compared.  Boxes must be finite.
//
// MF_FUSE (greedy absorption; thr = fuse_thr) changes three steps.  A pair matches when its boxes come from different
// tiles and inter / min(area_a, area_p) > fuse_thr (the same un-contracted inter and areas; 0 / 0 never matches, so the
// search window of step 5 is unchanged).
//   5. p is decided once the matching, not absorbed q < p of the smallest priority index is known: kept -> p is absorbed
//      by q (state MF_SUPPRESSED + q); none -> p is kept; undecided -> p waits.  That q is the first keeper that matches
//      p, so the fixed point is the sequential rule (each keeper absorbs every later unabsorbed candidate that matches
//      its own box);
//   union pass: every absorbed box applies min / max to its keeper's box, held as order-preserving u32 encodings in
//      place of the keeper's cbox, and adds 1 to its member count (the sval scratch): order-independent, deterministic;
//   6. det carries the union box, det_members the member count, slot_det[slot] the list index of the slot's detection
//      (kept or absorbed; -1 for a non-candidate): keepers' ranks go through the skey scratch to their members.
// ---------------------------------------------------------------------------
constexpr int MF_THREADS = 1024, MF_MAX_FRAMES = 64, MF_LDS_SORT = 4096;
constexpr int MF_NMS = 0, MF_FUSE = 1;
constexpr int MF_UNDECIDED = 0, MF_KEPT = 1, MF_SUPPRESSED = 2;   // MF_FUSE: MF_SUPPRESSED + q = absorbed by candidate q
constexpr int MF_SCRATCH_PER_SLOT = 16 + 8 + 4 + 4 + 4;      // cbox, skey, sval, cslot, state

struct mf_offsets {
    int tile[MF_MAX_FRAMES + 1];       // absolute tile offsets of this launch's frames
};

__device__ __forceinline__ unsigned mf_ord(float f) {       // order-preserving float -> u32
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float mf_unord(unsigned u) {     // inverse of mf_ord
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// Ascending bitonic sort of (key, val) pairs, any n: the comparator of the first step of every merge stage pairs
// mirrored positions, so all comparators point the same way and the virtual +inf padding past n never moves.
__device__ void mf_bitonic(uint64_t* key, int* val, int n) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int half = np2 >> 1;
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += blockDim.x) {
                const int blk = t / j, p = t - blk * j;
                int a, b;
                if (j == (k >> 1)) { a = blk * k + p; b = blk * k + k - 1 - p; }
                else { a = blk * 2 * j + p; b = a + j; }
                if (b < n) {
                    const uint64_t ka = key[a], kb = key[b];
                    if (kb < ka) {
                        key[a] = kb; key[b] = ka;
                        const int va = val[a]; val[a] = val[b]; val[b] = va;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int mf_lower_bound(const uint64_t* key, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int mf_row(float y, float y_min, float row_h) {
#pragma clang fp contract(off)
    const float r = floorf((y - y_min) / row_h);
    return r <= 0.f ? 0 : (r >= 1073741824.f ? 1073741824 : (int)r);
}

__device__ __forceinline__ int mf_load_state(const int* s) {
    return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Block-wide exclusive prefix sum of one int per thread (1024 threads = 16 waves of 64); returns the block total too.
__device__ __forceinline__ int mf_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < MF_THREADS / 64; ++w) {
        const int c = s_wave[w];
        if (w < wave) before += c;
        all += c;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// det_members / slot_det: MF_FUSE only (unused by MF_NMS).
template <int MODE>
__global__ __launch_bounds__(MF_THREADS) void merge_frames_nms_kernel(
        const wm_box_record* __restrict__ rec, const int* __restrict__ origins, mf_offsets offs, float thr,
        char* __restrict__ scratch, int n_slots_total, wm_box_record* __restrict__ out, wm_box_record* __restrict__ det,
        int* __restrict__ det_tile, int* __restrict__ det_count, int* __restrict__ det_members, int* __restrict__ slot_det,
        int frame_base) {
#pragma clang fp contract(off)
    constexpr bool FUSE = MODE == MF_FUSE;
    __shared__ uint64_t l_key[MF_LDS_SORT];
    __shared__ int l_val[MF_LDS_SORT];
    __shared__ int s_n, s_wave[MF_THREADS / 64];
    __shared__ unsigned s_wmax, s_hmax, s_ymin;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int t0 = offs.tile[f], t1 = offs.tile[f + 1];
    const int s0 = t0 * WM_NUM_QUERIES, ns = (t1 - t0) * WM_NUM_QUERIES;
    float4* cbox = (float4*)scratch + s0;
    uint64_t* g_key = (uint64_t*)(scratch + (size_t)n_slots_total * 16) + s0;
    int* g_val = (int*)(scratch + (size_t)n_slots_total * 24) + s0;
    int* cslot = (int*)(scratch + (size_t)n_slots_total * 28) + s0;
    int* state = (int*)(scratch + (size_t)n_slots_total * 32) + s0;
    if (tid == 0) { s_n = 0; s_wmax = mf_ord(0.f); s_hmax = mf_ord(0.f); s_ymin = 0xffffffffu; }
    __syncthreads();

    // 1. records out (frame coordinates, not merged) + candidate keys
    for (int i = tid; i < ns; i += MF_THREADS) {
        wm_box_record r = rec[s0 + i];
        const int tile = t0 + i / WM_NUM_QUERIES;
        const float oy = (float)origins[2 * tile], ox = (float)origins[2 * tile + 1];
        r.box[0] += ox; r.box[1] += oy; r.box[2] += ox; r.box[3] += oy;
        const bool cand = (r.flags & WM_FLAG_NMS) != 0;
        r.flags &= ~WM_FLAG_MERGED;
        r.nms_rank = -1;
        out[s0 + i] = r;
        if (cand) {
            const float sc = r.score == 0.f ? 0.f : r.score;          // -0 ties with +0, as the comparison does
            const int c = atomicAdd(&s_n, 1);
            g_key[c] = ((uint64_t)(~mf_ord(sc)) << 32) | (unsigned)i;
        } else if constexpr (FUSE) {
            slot_det[s0 + i] = -1;
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

    // 3. candidate boxes in priority order, frame extents
    for (int c = tid; c < n; c += MF_THREADS) {
        const int slot = (int)(key[c] & 0xffffffffu);
        cslot[c] = slot;
        const float4 b = *(const float4*)&out[s0 + slot].box[0];
        cbox[c] = b;
        state[c] = MF_UNDECIDED;
        atomicMax(&s_wmax, mf_ord(fmaxf(b.z - b.x, 0.f)));
        atomicMax(&s_hmax, mf_ord(fmaxf(b.w - b.y, 0.f)));
        atomicMin(&s_ymin, mf_ord(b.y));
    }
    __syncthreads();
    const float wmax = __uint_as_float(s_wmax & 0x7fffffffu), hmax = __uint_as_float(s_hmax & 0x7fffffffu);
    const float y_min = n > 0 ? mf_unord(s_ymin) : 0.f;
    const float row_h = fmaxf(hmax, 1.f);

    // 4. spatial order: (row of y0, x0)
    for (int c = tid; c < n; c += MF_THREADS) {
        const float4 b = cbox[c];
        key[c] = ((uint64_t)mf_row(b.y, y_min, row_h) << 32) | mf_ord(b.x);
        val[c] = c;
    }
    __syncthreads();
    mf_bitonic(key, val, n);

    // 5. rounds.  A box q meets p only if q.y0 in (p.y0 - h_q, p.y1) and q.x0 in (p.x0 - w_q, p.x1); the search window
    // widens the lower ends by a margin that covers the rounding of the fp32 widths.
    for (;;) {
        int pending_any = 0;
        for (int c = tid; c < n; c += MF_THREADS) {
            if (mf_load_state(&state[c]) != MF_UNDECIDED) continue;
            const float4 p = cbox[c];
            const float parea = (p.z - p.x) * (p.w - p.y);
            const float ylo = p.y - (hmax + (1.f + hmax * 0x1p-20f + fabsf(p.y) * 0x1p-20f));
            const float xlo = p.x - (wmax + (1.f + wmax * 0x1p-20f + fabsf(p.x) * 0x1p-20f));
            const int r0 = mf_row(ylo, y_min, row_h), r1 = mf_row(p.w, y_min, row_h);
            bool dead = false, pending = false;                  // MF_NMS
            int best = c, best_st = MF_UNDECIDED;                // MF_FUSE: smallest matching unabsorbed q seen, its state
            const int ptile = FUSE ? cslot[c] / WM_NUM_QUERIES : 0;
            for (int r = r0; r <= r1 && !dead; ++r) {
                const uint64_t row = (uint64_t)r << 32;
                int m = mf_lower_bound(key, n, row | mf_ord(xlo));
                const int m1 = mf_lower_bound(key, n, (row | mf_ord(p.z)) + 1);
                for (; m < m1 && !dead; ++m) {
                    const int q = val[m];
                    if (q >= best) continue;                     // MF_NMS: best == c throughout
                    const int st = mf_load_state(&state[q]);
                    if (FUSE ? st >= MF_SUPPRESSED : st == MF_SUPPRESSED) continue;
                    const float4 a = cbox[q];
                    const float xx0 = fmaxf(a.x, p.x), yy0 = fmaxf(a.y, p.y);
                    const float xx1 = fminf(a.z, p.z), yy1 = fminf(a.w, p.w);
                    const float iw = fmaxf(0.f, xx1 - xx0), ih = fmaxf(0.f, yy1 - yy0);
                    const float inter = iw * ih;
                    const float aarea = (a.z - a.x) * (a.w - a.y);
                    if constexpr (FUSE) {
                        const float ios = inter / fminf(aarea, parea);
                        if (ios > thr && cslot[q] / WM_NUM_QUERIES != ptile) { best = q; best_st = st; }
                    } else {
                        const float iou = inter / (aarea + parea - inter);
                        if (iou > thr) {
                            if (st == MF_KEPT) dead = true;
                            else pending = true;
                        }
                    }
                }
            }
            if constexpr (FUSE) {
                // every matching q < best was seen absorbed (final), so best is the first keeper or still open
                if (best == c || best_st == MF_KEPT)
                    __hip_atomic_store(&state[c], best == c ? MF_KEPT : MF_SUPPRESSED + best, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    pending_any = 1;
            } else {
                if (dead || !pending)
                    __hip_atomic_store(&state[c], dead ? MF_SUPPRESSED : MF_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    pending_any = 1;
            }
        }
        if (!__syncthreads_or(pending_any)) break;
    }

    // union pass: keepers' cbox -> order-preserving encodings, then every absorbed box widens its keeper's
    uint4* ubox = (uint4*)cbox;
    int* members = g_val;
    int* krank = (int*)g_key;
    if constexpr (FUSE) {
        for (int c = tid; c < n; c += MF_THREADS) {
            if (state[c] != MF_KEPT) continue;
            const float4 b = cbox[c];
            ubox[c] = uint4{mf_ord(b.x), mf_ord(b.y), mf_ord(b.z), mf_ord(b.w)};
            members[c] = 1;
        }
        __syncthreads();
        for (int c = tid; c < n; c += MF_THREADS) {
            const int st = state[c];
            if (st < MF_SUPPRESSED) continue;
            const int q = st - MF_SUPPRESSED;
            const float4 b = cbox[c];
            unsigned* u = (unsigned*)&ubox[q];
            __hip_atomic_fetch_min(&u[0], mf_ord(b.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_min(&u[1], mf_ord(b.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&u[2], mf_ord(b.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&u[3], mf_ord(b.w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&members[q], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
    }

    // 6. ranks, records, detection list
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += MF_THREADS) {
        const int c = c0 + tid;
        const bool kept = c < n && state[c] == MF_KEPT;
        int total;
        const int rank = base + mf_scan(kept ? 1 : 0, s_wave, total);
        if (kept) {
            const int slot = cslot[c];
            wm_box_record r = out[s0 + slot];
            r.flags |= WM_FLAG_MERGED;
            r.nms_rank = rank;
            out[s0 + slot] = r;
            if constexpr (FUSE) {
                const uint4 u = ubox[c];
                r.box[0] = mf_unord(u.x); r.box[1] = mf_unord(u.y); r.box[2] = mf_unord(u.z); r.box[3] = mf_unord(u.w);
                det_members[s0 + rank] = members[c];
                slot_det[s0 + slot] = rank;
                krank[c] = rank;
            }
            det[s0 + rank] = r;
            det_tile[s0 + rank] = slot / WM_NUM_QUERIES;
        }
        base += total;
    }
    if (tid == 0) det_count[frame_base + f] = base;
    if constexpr (FUSE) {
        __syncthreads();
        for (int c = tid; c < n; c += MF_THREADS) {
            const int st = state[c];
            if (st >= MF_SUPPRESSED) slot_det[s0 + cslot[c]] = krank[st - MF_SUPPRESSED];
        }
    }
}

}  // namespace wm
