// The k-nearest selection that the gallery walks share (identify.hip: the exhaustive search; ivf.hip: the probed lists), ONE
// definition: the key, a row's bounded list in LDS, the rank-counting cut and the merge of ascending partial k-lists.
//
// key = bits(d0) << 32 | id, d0 = 2 (1 - sc) >= +0 the metric-0 distance of pair_tiles.h and id the row number a caller reports
// (the gallery row itself, or ids[stored row] of an inverted file).  Keys are unique per query, so the k smallest are the same
// set in the same order whatever order workgroups, waves and lanes meet the candidates in.  All ones is "no candidate".
#pragma once
#include "pair_tiles.h"

namespace fn {

constexpr int IMAXK = 64;
constexpr int IMERGE_CAP = 128;      // merge list: up to 64 kept + 64 new keys
constexpr unsigned long long INONE = ~0ull;

typedef unsigned long long u64;

// list capacity of a row for a given k: the k kept keys and one column tile (16) of survivors, in steps of 16
__host__ __device__ __forceinline__ int id_cap(int k) { return ((k + 15) / 16) * 16 + 16; }

// Cut a list of n <= 128 unique keys (LDS, owned by the calling wave) to its min(n, k) smallest, ascending, by counting ranks;
// when n >= k the k-th smallest becomes the row's threshold.  Returns the new length.  Single wave: LDS operations of one wave
// execute in program order, so the reads of the rank loop precede the writes below for every lane.
__device__ __forceinline__ int id_prune(u64* __restrict__ list, int n, int k, u64* __restrict__ thr, int lane) {
    const u64 a = lane < n ? list[lane] : INONE;
    const u64 b = lane + 64 < n ? list[lane + 64] : INONE;
    int ra = 0, rb = 0;
    for (int j = 0; j < n; ++j) {
        const u64 v = list[j];       // one address for the wave: broadcast
        ra += v < a;
        rb += v < b;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < n && ra < k) {
        list[ra] = a;
        if (ra == k - 1) *thr = a;
    }
    if (lane + 64 < n && rb < k) {
        list[rb] = b;
        if (rb == k - 1) *thr = b;
    }
    __builtin_amdgcn_wave_barrier();
    return n < k ? n : k;
}

// The epilogue of one super-tile of walk_gallery (its on_tile): each lane compares its 16 values with its rows' current k-th
// best key (sThr, all ones until a row has k candidates) and appends the survivors to the row's list (sList [64][cap], sCnt);
// a list that cannot take another column tile is cut to its k smallest by the wave that owns the row.  Rows belong to one wave:
// no workgroup barrier.  split: accumulator 0 holds column tile `wave` of the query rows 0..15 and the lists are wave * 16 + row;
// otherwise qwave == wave.  g1: the walk's end; nq: its query rows.  col_id(col): the id of gallery row col < g1, the key's low
// word and what skip_row[] is compared with.
template <typename ColId>
__device__ __forceinline__ void id_select_tile(int c0, f32x4 (&acc)[4], int g1, int nq, int qwave, int wave, bool split, const int (&skip_row)[4],
                                               DotRange& seen, u64* __restrict__ sList, u64* __restrict__ sThr, int* __restrict__ sCnt, int cap, int k,
                                               ColId col_id) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        if (split && ct > 0) break;                        // split: accumulator 0 holds column tile `wave`
        const int tcol = c0 + (split ? wave : ct) * 16;
        if (tcol >= g1) continue;                          // beyond the slab: zero-padded columns, never candidates
        const int col = tcol + lr;
        const int id = col < g1 ? col_id(col) : -1;
        bool appended = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lg * 4 + r;         // the list; the query row is qwave * 16 + lg * 4 + r
            const float s = acc[ct][r];
            if (qwave * 16 + lg * 4 + r >= nq || col >= g1) continue;          // padding rows and zero-padded columns are never candidates
            seen.add(s);
            if (id == skip_row[r]) continue;
            const u64 key = ((u64)__float_as_uint(pair_distance(s, 0)) << 32) | (unsigned)id;
            if (key < sThr[row]) {
                const int slot = atomicAdd(&sCnt[row], 1);  // < cap: a row holds <= cap - 16 before a column tile adds <= 16
                sList[row * cap + slot] = key;
                appended = true;
            }
        }
        if (__ballot(appended) == 0ull) continue;          // the common case once the thresholds are tight
        __builtin_amdgcn_wave_barrier();
        const int cnt = lane < 16 ? sCnt[wave * 16 + lane] : 0;
        u64 full = __ballot(cnt > cap - 16);
        while (full) {
            const int row = wave * 16 + __builtin_ctzll(full);
            full &= full - 1;
            const int n = id_prune(sList + row * cap, sCnt[row], k, &sThr[row], lane);
            if (lane == 0) sCnt[row] = n;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// What cuts a list in id_emit and id_merge: cut(list, n, k, thr, lane) -> the new length, id_prune's contract.  IdCutSmallest,
// their default, is id_prune itself; candidates.hip passes the cut that keeps one key per label.
struct IdCutSmallest {
    __device__ __forceinline__ int operator()(u64* __restrict__ list, int n, int k, u64* __restrict__ thr, int lane) const {
        return id_prune(list, n, k, thr, lane);
    }
};

// After the walk (and a workgroup barrier): list `row`, cut to its k smallest, goes out ascending as out[0 .. k), all ones
// behind its length.  Called by the whole wave that owns the row.
template <typename Cut = IdCutSmallest>
__device__ __forceinline__ void id_emit(u64* __restrict__ sList, u64* __restrict__ sThr, const int* __restrict__ sCnt, int row, int cap, int k, int lane,
                                        u64* __restrict__ out, Cut cut = Cut()) {
    const int n = cut(sList + row * cap, sCnt[row], k, &sThr[row], lane);
    if (lane < k) out[lane] = lane < n ? sList[row * cap + lane] : INONE;
}

// One wave cuts `total` keys, key_at(0 .. total) (all ones: none), to the k smallest: ascending in sList [IMERGE_CAP] (LDS),
// sThr one LDS word.  Returns their number.
template <typename KeyAt, typename Cut = IdCutSmallest>
__device__ __forceinline__ int id_merge(u64* __restrict__ sList, u64* __restrict__ sThr, long total, int k, int lane, KeyAt key_at, Cut cut = Cut()) {
    if (lane == 0) *sThr = INONE;
    __builtin_amdgcn_wave_barrier();
    int n = 0;
    for (long base = 0; base < total; base += 64) {
        const long idx = base + lane;
        const u64 key = idx < total ? key_at(idx) : INONE;
        const bool keep = key < *sThr;                         // all ones never passes
        const u64 m = __ballot(keep);
        if (m == 0ull) continue;
        if (keep) sList[n + __popcll(m & ((1ull << lane) - 1ull))] = key;
        n += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (n > IMERGE_CAP - 64) n = cut(sList, n, k, sThr, lane);
    }
    return cut(sList, n, k, sThr, lane);
}

}  // namespace fn
