// Candidate lists of identities: for each of Q query rows the k nearest DISTINCT labels of G gallery rows, each with its nearest
// row, without the [Q, G] distance matrix ever reaching memory.
//
// Arithmetic, key and order: identify.hip's, bit for bit (pair_tiles.h's walk_gallery on the exact fp32 MFMA, topk_select.h's
// key = bits(d0) << 32 | row).  best(q, c) is the smallest key over the admissible rows of label c; the answer is the k labels with
// the smallest best, ascending, each reported through the row in that key.
//
// The walk, the LDS lists, the two modes (Q <= 16: the waves split the column tiles) and the per-slab partial lists are those of
// gallery_search_kernel; what changes is the cut.  A key is DOMINATED when its list holds a smaller key of the same label.  The
// cut keeps the min(n, k) smallest undominated keys, and the k-th of them becomes the row's threshold only once k distinct labels
// are present.  That threshold is sound: a candidate whose key is not below the k-th best distinct identity so far is either
// dominated (its label is listed with a smaller key) or has k other identities in front of its own; either way it is not in the
// answer.  Keys are unique per query, so the answer is one set in one order however candidates arrive, and a slab's list holds
// every label of the final answer whose best row lies in that slab (a label in front of it in the slab is in front of it overall).
//
// Labels of list entries are not kept in LDS (the lists already take up to 40 KiB): the cut gathers gallery_labels[row] for the
// two entries a lane holds, the table being small and L2-resident, and the uniform loops over the entries take entry j's label
// from the lane that holds it (v_readlane) next to its key (one LDS address for the wave: a broadcast).
//
// The threshold of the k-th DISTINCT identity is far away when identities have many rows, and a gallery stores them class after
// class: without more, the rows of the nearest identities are appended by the dozen and the lists are cut after nearly every
// column tile.  So a filter in front of the append drops dominated candidates: within a column tile, of the candidates of one
// query row whose labels are equal over a run of adjacent columns only the smallest is appended (a segmented minimum over the 16
// lanes of a lane group, on DPP row shifts; run only when a group holds two candidates).  What it drops is dominated by a key
// that is appended in its place, so the answer cannot change.  It needs the labels of the columns, which a wave loads one
// super-tile ahead, 64 labels in one coalesced load, so that no load is waited for.
#include "topk_select.h"
#include "../../include/facenet_hip.h"

namespace fn {

// id_prune's contract with "smallest" read as "smallest undominated": list of n <= 128 unique keys, owned by the calling wave.
struct IdCutDistinct {
    const int* __restrict__ glabels;
    __device__ __forceinline__ int operator()(u64* __restrict__ list, int n, int k, u64* __restrict__ thr, int lane) const {
        n = __builtin_amdgcn_readfirstlane(n);                 // wave-uniform, and provably so: j below selects a lane
        const bool ha = lane < n, hb = lane + 64 < n;
        const u64 a = ha ? list[lane] : INONE;
        const u64 b = hb ? list[lane + 64] : INONE;
        const int la = ha ? glabels[(unsigned)(a & 0xffffffffull)] : -1;       // labels are >= 0: -1 and -2 match no entry
        const int lb = hb ? glabels[(unsigned)(b & 0xffffffffull)] : -2;
        const int n0 = n < 64 ? n : 64;
        bool da = false, db = false;                           // dominated
        for (int j = 0; j < n0; ++j) {
            const u64 v = list[j];
            const int lj = __builtin_amdgcn_readlane(la, j);
            da |= (lj == la) & (v < a);
            db |= (lj == lb) & (v < b);
        }
        for (int j = 64; j < n; ++j) {
            const u64 v = list[j];
            const int lj = __builtin_amdgcn_readlane(lb, j - 64);
            da |= (lj == la) & (v < a);
            db |= (lj == lb) & (v < b);
        }
        const bool ka = ha && !da, kb = hb && !db;
        const u64 ua = __ballot(ka), ub = __ballot(kb);        // the undominated entries: one per label
        int ra = 0, rb = 0;
        for (u64 m = ua; m; m &= m - 1) {
            const u64 v = list[__builtin_ctzll(m)];
            ra += v < a;
            rb += v < b;
        }
        for (u64 m = ub; m; m &= m - 1) {
            const u64 v = list[64 + __builtin_ctzll(m)];
            ra += v < a;
            rb += v < b;
        }
        const int distinct = __popcll(ua) + __popcll(ub), kept = distinct < k ? distinct : k;
        __builtin_amdgcn_wave_barrier();
        if (ka && ra < k) {
            list[ra] = a;
            if (ra == k - 1) *thr = a;                         // only with k distinct labels present
        }
        if (kb && rb < k) {
            list[rb] = b;
            if (rb == k - 1) *thr = b;
        }
        __builtin_amdgcn_wave_barrier();
        return kept;
    }
};

// Lane l of a row of 16 lanes takes src from lane l - O (UP) or l + O (!UP): v_mov_b32_dpp row_shr / row_shl.  A lane without such
// a lane in its row keeps `none`.
template <bool UP, int O>
__device__ __forceinline__ int row_shift(int none, int src) {
    return __builtin_amdgcn_update_dpp(none, src, (UP ? 0x110 : 0x100) + O, 0xf, 0xf, false);
}
template <bool UP, int O>
__device__ __forceinline__ unsigned run_min_step(int lab, unsigned acc) {
    const bool mate = row_shift<UP, O>(-1, lab) == lab;        // labels are >= 0, or -1 behind the walk's end, where nothing is a candidate
    const unsigned w = (unsigned)row_shift<UP, O>(-1, (int)acc);
    return mate && w < acc ? w : acc;
}
// The minimum of v over the lanes of the calling lane's group of 16 that lie BEFORE it (UP) or AFTER it (!UP) and reach it through
// lanes of its own label at distances 1, 2, 4, 8 (for a run of equal labels: all of the run on that side); all ones without one.
// Only values of the lane's own label are combined, whatever the labels are.
template <bool UP>
__device__ __forceinline__ unsigned run_min_exclusive(int lab, unsigned v) {
    v = run_min_step<UP, 8>(lab, run_min_step<UP, 4>(lab, run_min_step<UP, 2>(lab, run_min_step<UP, 1>(lab, v))));
    return row_shift<UP, 1>(-1, lab) == lab ? (unsigned)row_shift<UP, 1>(-1, (int)v) : 0xffffffffu;
}

// id_select_tile with the filter in front of the append and the distinct cut.  labs: lane i holds gallery_labels[c0 + i] (-1
// from g1 on).
__device__ __forceinline__ void dc_select_tile(int c0, f32x4 (&acc)[4], int g1, int nq, int qwave, int wave, bool split, const int (&skip_row)[4],
                                               DotRange& seen, u64* __restrict__ sList, u64* __restrict__ sThr, int* __restrict__ sCnt,
                                               int cap, int k, int labs, const int* __restrict__ glabels) {
    const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        if (split && ct > 0) break;                        // split: accumulator 0 holds column tile `wave`
        const int tile = split ? wave : ct;
        const int tcol = c0 + tile * 16;
        if (tcol >= g1) continue;                          // beyond the slab: zero-padded columns, never candidates
        const int col = tcol + lr;
        unsigned d[4];                                     // bits(d0) of a candidate, all ones: none.  Within a column tile the key
        bool any = false;                                  // order is (d, lane): the columns ascend with the lanes
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = wave * 16 + lg * 4 + r;         // the list; the query row is qwave * 16 + lg * 4 + r
            const float s = acc[ct][r];
            d[r] = 0xffffffffu;
            if (qwave * 16 + lg * 4 + r >= nq || col >= g1) continue;          // padding rows and zero-padded columns are never candidates
            seen.add(s);
            if (col == skip_row[r]) continue;
            const unsigned bits = __float_as_uint(pair_distance(s, 0));
            if ((((u64)bits << 32) | (unsigned)col) < sThr[row]) d[r] = bits, any = true;
        }
        if (__ballot(any) == 0ull) continue;               // the common case once the thresholds are tight
        const int lab = __shfl(labs, tile * 16 + lr);      // of this lane's column
        u64 two = 0;                                       // some lane group holds two candidates of one query row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const u64 m = __ballot(d[r] != 0xffffffffu);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned x = (unsigned)(m >> (16 * g)) & 0xffffu;
                two |= x & (x - 1);
            }
        }
        if (two) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {                  // one side, then the other: a run's smallest (d, lane) survives both
                if (d[r] >= run_min_exclusive<true>(lab, d[r])) d[r] = 0xffffffffu;          // equal distances: the lower column stays
                if (d[r] > run_min_exclusive<false>(lab, d[r])) d[r] = 0xffffffffu;
            }
        }
        bool appended = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (d[r] == 0xffffffffu) continue;
            const int row = wave * 16 + lg * 4 + r;
            const u64 key = ((u64)d[r] << 32) | (unsigned)col;
            const int slot = atomicAdd(&sCnt[row], 1);      // < cap: a row holds <= cap - 16 before a column tile adds <= 16
            sList[row * cap + slot] = key;
            appended = true;
        }
        if (__ballot(appended) == 0ull) continue;
        __builtin_amdgcn_wave_barrier();
        const int cnt = lane < 16 ? sCnt[wave * 16 + lane] : 0;
        u64 full = __ballot(cnt > cap - 16);
        while (full) {
            const int row = wave * 16 + __builtin_ctzll(full);
            full &= full - 1;
            const int n = IdCutDistinct{glabels}(sList + row * cap, sCnt[row], k, &sThr[row], lane);
            if (lane == 0) sCnt[row] = n;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256, 4) void gallery_candidates_kernel(const float* __restrict__ queries, int Q, const float* __restrict__ gallery,
                                                                 int G, const int* __restrict__ glabels, int E, int k,
                                                                 const int* __restrict__ skip, int slab_rows, int split, u64* __restrict__ partial,
                                                                 int* __restrict__ range) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    __shared__ u64 sThr[F32_TILE];
    __shared__ int sCnt[F32_TILE];
    __shared__ __align__(16) int sSkip[F32_TILE];              // (in LDS, not in four registers through the multiplication)
    const int cap = id_cap(k);
    u64* sList = reinterpret_cast<u64*>(dyn);                  // [F32_TILE][cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)G, (long)g0 + slab_rows);     // g0 < G < 2^31; the sum may pass it
    const int nq = Q - q0;                                     // >= 1
    if (tid < F32_TILE) {
        sThr[tid] = INONE;
        sCnt[tid] = 0;
        sSkip[tid] = (skip && q0 + tid < Q) ? skip[q0 + tid] : -1;
    }
    const int qwave = split ? 0 : wave;                        // the two modes of gallery_search_kernel
    const bool wave_live = qwave * 16 < nq;
    DotRange seen;
    int ahead = g0 + lane < g1 ? glabels[g0 + lane] : -1;      // the labels of the next super-tile's columns, lane i: column c0 + i
    walk_gallery(sA, sB, queries + (long)q0 * E, nq, gallery, g0, g1, E, wave_live, qwave * 16, split ? wave * 16 : -1, [&](int c0, f32x4 (&acc)[4]) {
        const int labs = ahead, col = c0 + F32_TILE + lane;
        ahead = col < g1 ? glabels[col] : -1;                  // (g1 <= G: inside the table)
        int skip_row[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) skip_row[r] = sSkip[qwave * 16 + lg * 4 + r];
        dc_select_tile(c0, acc, g1, nq, qwave, wave, split, skip_row, seen, sList, sThr, sCnt, cap, k, labs, glabels);
    });
    seen.publish(range, lane);
    __syncthreads();                                           // also orders the list initialisation for an empty slab walk
    const long pslab = split ? (long)slab * 4 + wave : slab;
    for (int r = 0; r < 16; ++r) {                             // the ascending list of every list of this wave -> partial[pslab][q][k]
        const int qrow = qwave * 16 + r, row = wave * 16 + r;
        if (qrow >= nq) break;
        id_emit(sList, sThr, sCnt, row, cap, k, lane, partial + (pslab * Q + q0 + qrow) * k, IdCutDistinct{glabels});
    }
}

// One wave per query: the slabs' lists (a label may stand in several) -> the final k.  dist: as gallery_merge_kernel.
__global__ __launch_bounds__(64) void gallery_candidates_merge_kernel(const u64* __restrict__ partial, int slabs, int Q, int k, int metric,
                                                                      const float* __restrict__ queries, const float* __restrict__ gallery, int E,
                                                                      const int* __restrict__ glabels, float* __restrict__ dist,
                                                                      int* __restrict__ rows) {
    __shared__ u64 sList[IMERGE_CAP];
    __shared__ u64 sThr;
    const int q = blockIdx.x, lane = threadIdx.x;
    const long total = (long)slabs * k;
    const int n = id_merge(sList, &sThr, total, k, lane, [&](long idx) {
        const long sl = idx / k;
        return partial[(sl * Q + q) * k + (idx - sl * k)];
    }, IdCutDistinct{glabels});
    if (lane >= k) return;
    const long o = (long)q * k + lane;
    if (lane >= n) {                                           // fewer than k admissible identities
        dist[o] = __int_as_float(0x7f800000);
        rows[o] = -1;
        return;
    }
    const u64 key = sList[lane];
    const int row = (int)(unsigned)(key & 0xffffffffull);
    float d = __uint_as_float((unsigned)(key >> 32));
    if (metric == 1) d = pair_distance(dot_chain(queries + (long)q * E, gallery + (long)row * E, E), 1);
    dist[o] = d;
    rows[o] = row;
}

// partial lists per (slab, query): four when the waves split the column tiles (Q <= 16), else one
static int candidate_lists(int Q) { return Q <= 16 ? 4 : 1; }

}  // namespace fn
using namespace fn;

extern "C" int fn_gallery_candidates_workspace(int Q, int G, int k, int slab_rows, long long* bytes) {
    FN_REQUIRE(bytes && slab_rows >= 0, "gallery_candidates_workspace: bad arguments");
    int srows, slabs;
    if (int rc = check_walk_shape("gallery_candidates", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(k >= 1 && k <= IMAXK, "gallery_candidates: k must be in [1, 64] (k %d)", k);
    *bytes = (long long)slabs * candidate_lists(Q) * Q * k * (long long)sizeof(u64);
    return FN_OK;
}

extern "C" int fn_gallery_candidates(const float* queries, int Q, const float* gallery, int G, const int32_t* gallery_labels, int E, int k,
                                     int metric, const int32_t* skip, int slab_rows, void* workspace, float* dist, int32_t* rows,
                                     int32_t* range, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("gallery_candidates", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(k >= 1 && k <= IMAXK, "gallery_candidates: k must be in [1, 64] (k %d)", k);
    if (int rc = check_walk_args("gallery_candidates", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(gallery_labels, "gallery_candidates: gallery_labels must be given");
    FN_REQUIRE(dist && rows, "gallery_candidates: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const int lists = candidate_lists(Q);
    const size_t dyn = (size_t)F32_TILE * id_cap(k) * sizeof(u64);   // <= 40 KiB; with the static tiles below the 64 KiB default
    hipLaunchKernelGGL(gallery_candidates_kernel, dim3((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs), dim3(256), dyn, st, queries, Q, gallery, G,
                       (const int*)gallery_labels, E, k, (const int*)skip, srows, (int)(lists == 4), (u64*)workspace, (int*)range);
    hipLaunchKernelGGL(gallery_candidates_merge_kernel, dim3((unsigned)Q), dim3(64), 0, st, (const u64*)workspace, slabs * lists, Q, k, metric,
                       queries, gallery, E, (const int*)gallery_labels, dist, (int*)rows);
    return check_launch("gallery_candidates");
}
