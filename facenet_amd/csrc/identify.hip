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
// The key, the lists and the cuts are topk_select.h's, shared with the probed-list search of ivf.hip.
#include "topk_select.h"
#include "../../include/facenet_hip.h"

namespace fn {

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
    // selection after each super-tile (topk_select.h); the key's low word is the gallery row itself
    walk_gallery(sA, sB, queries + (long)q0 * E, nq, gallery, g0, g1, E, wave_live, qwave * 16, split ? wave * 16 : -1, [&](int c0, f32x4 (&acc)[4]) {
        id_select_tile(c0, acc, g1, nq, qwave, wave, split, skip_row, seen, sList, sThr, sCnt, cap, k, [](int col) { return col; });
    });
    seen.publish(range, lane);
    __syncthreads();                                           // also orders the list initialisation for an empty slab walk
    const long pslab = split ? (long)slab * 4 + wave : slab;
    for (int r = 0; r < 16; ++r) {                             // ascending k-list of every list of this wave -> partial[pslab][q][k]
        const int qrow = qwave * 16 + r, row = wave * 16 + r;
        if (qrow >= nq) break;
        id_emit(sList, sThr, sCnt, row, cap, k, lane, partial + (pslab * Q + q0 + qrow) * k);
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
    const long total = (long)slabs * k;
    const int n = id_merge(sList, &sThr, total, k, lane, [&](long idx) {
        const long sl = idx / k;
        return partial[(sl * Q + q) * k + (idx - sl * k)];
    });
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
