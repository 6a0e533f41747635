// 1:N identification: for each of Q query rows the k nearest of G gallery rows, without the [Q, G] distance matrix ever
// reaching memory.
//
// Arithmetic (exact): s(q, g) = the ascending-e fmaf chain from 0.0f of query[q][e] * gallery[g][e], computed on
// v_mfma_f32_16x16x4_f32, which is that chain bit for bit (validation.hip); sc = min(max(s, -1), 1);
// rank key d0 = 2 (1 - sc), the metric-0 distance of confidence_kernel, for BOTH metrics (arccos is monotone in it).  Order:
// ascending (d0, gallery row).  d0 >= +0, so  key = bits(d0) << 32 | row  is a 64-bit integer whose unsigned order is that
// order; keys are unique per query, so the k smallest are the same set in the same order whatever order workgroups, waves and
// lanes meet the candidates in.  All ones is "no candidate".
//
// gallery_search_kernel: one workgroup per (64 query rows, slab of gallery rows).  The slab is walked in 64-column
// super-tiles by pair_tiles.h's walk_gallery (wave w = query rows 16w..16w+15 against four 16x16 column tiles).  After
// a super-tile each lane compares its 16 values with its rows' current k-th best key (LDS, all ones until a row has k
// candidates) and appends the survivors to the row's list; a list that cannot take another column tile is cut to its k
// smallest by the wave that owns the row.  Rows belong to one wave: selection needs no workgroup barrier.
// gallery_merge_kernel: one wave per query cuts the slabs' k-lists to the final k and writes distances, rows and labels.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

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

__global__ __launch_bounds__(256, 4) void gallery_search_kernel(const float* __restrict__ queries, int Q, const float* __restrict__ gallery, int G,
                                                             int E, int k, const int* __restrict__ skip, int slab_rows, int split, u64* __restrict__ partial,
                                                             int* __restrict__ range) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    __shared__ u64 sThr[F32_TILE];
    __shared__ int sCnt[F32_TILE];
    const int cap = id_cap(k);
    u64* sList = reinterpret_cast<u64*>(dyn);                  // [F32_TILE][cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)G, (long)g0 + slab_rows);     // g0 < G < 2^31; the sum may pass it
    const int nq = Q - q0;                                     // >= 1
    if (tid < F32_TILE) {
        sThr[tid] = INONE;
        sCnt[tid] = 0;
    }
    // split (Q <= 16, one query tile): every wave multiplies the same 16 query rows against ITS column tile and keeps its own
    // lists (list wave * 16 + row), which go out as four partial lists per slab.  Otherwise wave w owns query rows 16w..16w+15.
    const int qwave = split ? 0 : wave;
    const bool wave_live = qwave * 16 < nq;
    int skip_row[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + qwave * 16 + lg * 4 + r;
        skip_row[r] = (skip && q < Q) ? skip[q] : -1;
    }
    DotRange seen;
    // selection after each super-tile: C/D layout column = lane & 15, row = 4 (lane >> 4) + register
    walk_gallery(sA, sB, queries + (long)q0 * E, nq, gallery, g0, g1, E, wave_live, qwave * 16, split ? wave * 16 : -1, [&](int c0, f32x4 (&acc)[4]) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (split && ct > 0) break;                        // split: accumulator 0 holds column tile `wave`
            const int tcol = c0 + (split ? wave : ct) * 16;
            if (tcol >= g1) continue;                          // beyond the slab: zero-padded columns, never candidates
            const int col = tcol + lr;
            bool appended = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wave * 16 + lg * 4 + r;         // the list; the query row is qwave * 16 + lg * 4 + r
                const float s = acc[ct][r];
                if (qwave * 16 + lg * 4 + r >= nq || col >= g1) continue;          // padding rows and zero-padded columns are never candidates
                seen.add(s);
                if (col == skip_row[r]) continue;
                const u64 key = ((u64)__float_as_uint(pair_distance(s, 0)) << 32) | (unsigned)col;
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
    });
    seen.publish(range, lane);
    __syncthreads();                                           // also orders the list initialisation for an empty slab walk
    const long pslab = split ? (long)slab * 4 + wave : slab;
    for (int r = 0; r < 16; ++r) {                             // ascending k-list of every list of this wave -> partial[pslab][q][k]
        const int qrow = qwave * 16 + r, row = wave * 16 + r;
        if (qrow >= nq) break;
        const int n = id_prune(sList + row * cap, sCnt[row], k, &sThr[row], lane);
        if (lane < k) partial[(pslab * Q + q0 + qrow) * k + lane] = lane < n ? sList[row * cap + lane] : INONE;
    }
}

// One wave per query: the slabs' ascending k-lists -> the final k.  dist from the key (metric 0) or arccos of the recomputed
// chain (metric 1: the key holds d0, from which sc cannot be recovered exactly).
__global__ __launch_bounds__(64) void gallery_merge_kernel(const u64* __restrict__ partial, int slabs, int Q, int k, int metric,
                                                           const float* __restrict__ queries, const float* __restrict__ gallery, int E,
                                                           const int* __restrict__ labels, float* __restrict__ dist, int* __restrict__ rows,
                                                           int* __restrict__ row_labels) {
    __shared__ u64 sList[IMERGE_CAP];
    __shared__ u64 sThr;
    const int q = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) sThr = INONE;
    __builtin_amdgcn_wave_barrier();
    int n = 0;
    const long total = (long)slabs * k;
    for (long base = 0; base < total; base += 64) {
        const long idx = base + lane;
        u64 key = INONE;
        if (idx < total) {
            const long sl = idx / k;
            key = partial[(sl * Q + q) * k + (idx - sl * k)];
        }
        const bool keep = key < sThr;                          // all ones never passes
        const u64 m = __ballot(keep);
        if (m == 0ull) continue;
        if (keep) sList[n + __popcll(m & ((1ull << lane) - 1ull))] = key;
        n += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (n > IMERGE_CAP - 64) n = id_prune(sList, n, k, &sThr, lane);
    }
    n = id_prune(sList, n, k, &sThr, lane);
    if (lane >= k) return;
    const long o = (long)q * k + lane;
    if (lane >= n) {                                           // fewer than k admissible rows
        dist[o] = __int_as_float(0x7f800000);
        rows[o] = -1;
        if (row_labels) row_labels[o] = -1;
        return;
    }
    const u64 key = sList[lane];
    const int row = (int)(unsigned)(key & 0xffffffffull);
    float d = __uint_as_float((unsigned)(key >> 32));
    if (metric == 1) d = pair_distance(dot_chain(queries + (long)q * E, gallery + (long)row * E, E), 1);
    dist[o] = d;
    rows[o] = row;
    if (row_labels) row_labels[o] = labels[row];
}

// partial lists per (slab, query): four when the waves split the column tiles (Q <= 16), else one
static int id_lists(int Q) { return Q <= 16 ? 4 : 1; }

}  // namespace fn
using namespace fn;

extern "C" int fn_gallery_search_workspace(int Q, int G, int k, int slab_rows, long long* bytes) {
    FN_REQUIRE(bytes && slab_rows >= 0, "gallery_search_workspace: bad arguments");
    int srows, slabs;
    if (int rc = check_walk_shape("gallery_search", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(k >= 1 && k <= IMAXK, "gallery_search: k must be in [1, 64] (k %d)", k);
    *bytes = (long long)slabs * id_lists(Q) * Q * k * (long long)sizeof(u64);
    return FN_OK;
}

extern "C" int fn_gallery_search(const float* queries, int Q, const float* gallery, int G, int E, int k, int metric, const int32_t* skip,
                                 const int32_t* labels, int slab_rows, void* workspace, float* dist, int32_t* rows, int32_t* row_labels,
                                 float* range, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("gallery_search", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(k >= 1 && k <= IMAXK, "gallery_search: k must be in [1, 64] (k %d)", k);
    if (int rc = check_walk_args("gallery_search", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(dist && rows, "gallery_search: bad arguments");
    FN_REQUIRE(!row_labels || labels, "gallery_search: row_labels needs labels");
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const size_t dyn = (size_t)F32_TILE * id_cap(k) * sizeof(u64);   // <= 40 KiB; with the static tiles below the 64 KiB default
    hipLaunchKernelGGL(gallery_search_kernel, dim3((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs), dim3(256), dyn, st, queries, Q, gallery, G, E, k,
                       (const int*)skip, srows, (int)(id_lists(Q) == 4), (u64*)workspace, (int*)range);
    hipLaunchKernelGGL(gallery_merge_kernel, dim3((unsigned)Q), dim3(64), 0, st, (const u64*)workspace, slabs * id_lists(Q), Q, k, metric, queries, gallery,
                       E, (const int*)labels, dist, (int*)rows, (int*)row_labels);
    return check_launch("gallery_search");
}
