// Face clustering: a radius search, "every gallery row nearer than eps" as a CSR, and DBSCAN on that CSR.
// The [Q, G] distance matrix never reaches memory.
//
// Arithmetic (exact): pair_tiles.h's, the dot products and distances of identify.hip / validation.hip.  (q, g) are neighbours
// when pair_distance(s, metric) < eps, the strict fp32 comparison of ConfidenceMatrix, the classifiers' predict and Gallery.who.
//
// radius_kernel<FILL>: one workgroup of 4 waves per (64 query rows, slab of gallery rows), wave w = query rows 16w..16w+15, on
// pair_tiles.h's walk_gallery.  After a super-tile, for each column tile and accumulator register the
// 16 lanes of a lane group hold 16 consecutive columns of ONE query row: a ballot gives the group's hits, a hit's position is the
// row's cursor plus the popcount of the lower hit bits, and the cursor advances by the group's popcount.  Rows belong to one wave
// and column tiles are met in ascending order: no atomics, no workgroup barrier, columns ascending.  The count pass
// leaves the cursors in counts[slab][q]; radius_scan_kernel turns them into offsets[q] and a base per (slab, q); the fill pass
// starts each cursor at its base and writes nothing at or beyond `capacity`.
//
// DBSCAN: a row is core when degree + 1 >= min_samples; clusters are the connected components of the core rows.  parent[] (the
// labels buffer) is a forest with parent[i] <= i.  A round = hook (every core edge (i, j) with different parents lowers the
// larger parent's parent to the smaller parent with an atomic min) + jump (every row follows its parents to a root: all trees
// are stars again).  A round whose hook met no such edge found the fixed point, each core row labelled by the smallest row of its
// component, which is unique: scheduling cannot change the result.  Then border rows take the label of the core neighbour with
// the smallest (bits(d0) << 32 | col) key, and a scan over the roots gives consecutive ids in ascending order of the roots.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

typedef unsigned long long u64;

template <bool FILL>
__global__ __launch_bounds__(256, 4) void radius_kernel(const float* __restrict__ queries, int Q, const float* __restrict__ gallery, int G, int E,
                                                     int metric, float eps, const int* __restrict__ skip, int slab_rows, int* __restrict__ counts,
                                                     const long long* __restrict__ base, int* __restrict__ cols, float* __restrict__ dist,
                                                     long long capacity, int* __restrict__ range) {
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)G, (long)g0 + slab_rows);     // g0 < G < 2^31; the sum may pass it
    const int nq = Q - q0;                                     // >= 1
    const bool wave_live = wave * 16 < nq;
    int skip_row[4];
    long long cursor[4];                                       // per query row of this lane group; equal in its 16 lanes
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + wave * 16 + lg * 4 + r;
        skip_row[r] = (skip && q < Q) ? skip[q] : -1;
        cursor[r] = (FILL && q < Q) ? base[(long)slab * Q + q] : 0;
    }
    DotRange seen;
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register.  Column tiles ascending, so each row's hits come out in
    // ascending column order.
    walk_gallery(sA, sB, queries + (long)q0 * E, nq, gallery, g0, g1, E, wave_live, wave * 16, -1, [&](int c0, f32x4 (&acc)[4]) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int col = c0 + ct * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = acc[ct][r];
                const bool real = wave * 16 + lg * 4 + r < nq && col < g1;     // padding rows and zero-padded columns: never neighbours
                if (!FILL && real) seen.add(s);
                const float d = pair_distance(s, metric);                      // what the CSR reports
                const bool hit = d < eps && real && col != skip_row[r];
                const unsigned group = (unsigned)(__ballot(hit) >> (lg * 16)) & 0xffffu;        // the 16 columns of this row
                if (FILL && hit) {
                    const long long pos = cursor[r] + __popc(group & ((1u << lr) - 1u));
                    if (pos < capacity) {
                        cols[pos] = col;
                        dist[pos] = d;
                    }
                }
                cursor[r] += __popc(group);
            }
        }
    });
    if (FILL) return;
    seen.publish(range, lane);
    if (lr == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + wave * 16 + lg * 4 + r;
            if (q < Q) counts[(long)slab * Q + q] = (int)cursor[r];     // <= slab_rows <= 2^30; 0 from a wave that is not live
        }
    }
}

constexpr int SCAN_T = 1024;

// Exclusive scan of v over the workgroup's SCAN_T threads (Hillis-Steele in LDS); *total receives the sum.
__device__ __forceinline__ long long block_exclusive_scan(long long v, long long* sh, long long* total) {
    const int tid = threadIdx.x;
    __syncthreads();                                           // the previous use of sh is over
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_T; o <<= 1) {
        const long long add = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    *total = sh[SCAN_T - 1];
    return sh[tid] - v;
}

// counts[slab][q] -> offsets[q] (exclusive over q of the row totals; offsets[Q] = nnz) and base[slab][q] = offsets[q] + the
// counts of the slabs before it.  One workgroup walks the rows 1024 at a time; not a hot path.
__global__ __launch_bounds__(SCAN_T) void radius_scan_kernel(const int* __restrict__ counts, int slabs, int Q, long long* __restrict__ base,
                                                            long long* __restrict__ offsets) {
    __shared__ long long sh[SCAN_T];
    long long carry = 0;
    for (long q0 = 0; q0 < Q; q0 += SCAN_T) {
        const long q = q0 + threadIdx.x;
        long long row = 0;
        if (q < Q)
            for (int s = 0; s < slabs; ++s) row += counts[(long)s * Q + q];
        long long total;
        long long at = carry + block_exclusive_scan(row, sh, &total);
        if (q < Q) {
            offsets[q] = at;
            for (int s = 0; s < slabs; ++s) {
                base[(long)s * Q + q] = at;
                at += counts[(long)s * Q + q];
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) offsets[Q] = carry;
}

// ---- DBSCAN ---------------------------------------------------------------------------------------------------------------
enum { DB_CONVERGED = 0, DB_ROUNDS = 1, DB_CLUSTERS = 2, DB_NOISE = 3, DB_CHANGED = 4, DB_INFO_WORDS = 8 };

// parent[] is read and lowered by many workgroups within one launch: relaxed agent-scope accesses, so that no value is served
// from a stale cache line for ever.  A stale value is still a valid one (an earlier, larger ancestor of the same component).
__device__ __forceinline__ int db_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void db_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void dbscan_init_kernel(const long long* __restrict__ offsets, int N, int min_samples, int* __restrict__ parent, int* __restrict__ core,
                                   int* __restrict__ info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < DB_INFO_WORDS) info[i] = 0;
    if (i >= N) return;
    const bool c = offsets[i + 1] - offsets[i] + 1 >= (long long)min_samples;       // the row counts itself
    core[i] = c;
    parent[i] = c ? i : -1;
}

__global__ void dbscan_hook_kernel(const long long* __restrict__ offsets, const int* __restrict__ cols, const int* __restrict__ core, int N,
                                   int* __restrict__ parent, int* __restrict__ info) {
    if (info[DB_CONVERGED]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !core[i]) return;
    bool changed = false;
    for (long long e = offsets[i]; e < offsets[i + 1]; ++e) {
        const int j = cols[e];
        if (j < 0 || j >= N || !core[j]) continue;             // (a column outside [0, N) is not a row of a self-join: ignored)
        const int pi = db_load(parent + i), pj = db_load(parent + j);
        if (pi == pj) continue;
        changed = true;
        atomicMin(parent + max(pi, pj), min(pi, pj));          // parent[x] <= x stays true: no cycles
    }
    if (changed) info[DB_CHANGED] = 1;
}

__global__ void dbscan_jump_kernel(const int* __restrict__ core, int N, int* __restrict__ parent, int* __restrict__ info) {
    if (info[DB_CONVERGED]) return;        // (set below only when the hook changed nothing: the trees are stars already)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        info[DB_ROUNDS] += 1;
        if (!info[DB_CHANGED]) info[DB_CONVERGED] = 1;
        info[DB_CHANGED] = 0;
    }
    if (i >= N || !core[i]) return;
    // Roots do not change during this launch and every other parent only moves to a proper ancestor (< itself): the loop ends,
    // at a root.
    int p = db_load(parent + i);
    for (;;) {
        const int pp = db_load(parent + p);
        if (pp == p) break;
        p = pp;
    }
    db_store(parent + i, p);
}

// A non-core row with a core neighbour joins the cluster of the core neighbour with the smallest (bits(d0) << 32 | col) key.
// d0 is the metric-0 distance: the CSR's own for metric 0; for metric 1 it is recomputed from the fmaf chain, which is the MFMA's
// bit for bit (the arccos does not give sc back).  Also flags the roots for the scan.
__global__ void dbscan_border_kernel(const long long* __restrict__ offsets, const int* __restrict__ cols, const float* __restrict__ dist, int metric,
                                     const float* __restrict__ emb, int E, const int* __restrict__ core, int N, int* __restrict__ labels,
                                     int* __restrict__ ids, const int* __restrict__ info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (core[i]) {
        ids[i] = labels[i] == i;
        return;
    }
    ids[i] = 0;
    u64 best = ~0ull;
    for (long long e = offsets[i]; e < offsets[i + 1]; ++e) {
        const int j = cols[e];
        if (j < 0 || j >= N || !core[j]) continue;
        const float d0 = metric == 1 ? pair_distance(dot_chain(emb + (long)i * E, emb + (long)j * E, E), 0) : dist[e];
        const u64 key = ((u64)__float_as_uint(d0) << 32) | (unsigned)j;
        best = key < best ? key : best;
    }
    labels[i] = best == ~0ull ? -1 : labels[(int)(unsigned)(best & 0xffffffffull)];      // a core row's label: its root
}

// ids[r] (1 at the roots) -> the exclusive scan: the id of the cluster rooted at r; info: clusters.
__global__ __launch_bounds__(SCAN_T) void dbscan_ids_kernel(int* __restrict__ ids, int N, int* __restrict__ info) {
    __shared__ long long sh[SCAN_T];
    long long carry = 0;
    for (long i0 = 0; i0 < N; i0 += SCAN_T) {
        const long i = i0 + threadIdx.x;
        const long long v = i < N ? ids[i] : 0;
        long long total;
        const long long at = carry + block_exclusive_scan(v, sh, &total);
        if (i < N) ids[i] = (int)at;
        carry += total;
    }
    if (threadIdx.x == 0) info[DB_CLUSTERS] = (int)carry;
}

__global__ void dbscan_relabel_kernel(const int* __restrict__ ids, int N, int* __restrict__ labels, int* __restrict__ info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int root = i < N ? labels[i] : 0;
    if (i < N && root >= 0) labels[i] = ids[root];
    const u64 noise = __ballot(i < N && root < 0);
    if ((threadIdx.x & 63) == 0 && noise) atomicAdd(&info[DB_NOISE], __popcll(noise));
}

// workspace: base int64 [slabs][Q], then counts int32 [slabs][Q]
static long long rd_base_bytes(int slabs, int Q) { return (long long)slabs * Q * (long long)sizeof(long long); }

}  // namespace fn
using namespace fn;

extern "C" int fn_radius_workspace(int Q, int G, int slab_rows, long long* bytes) {
    int srows, slabs;
    if (int rc = check_walk_shape("radius_workspace", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(bytes, "radius_workspace: bad arguments");
    *bytes = rd_base_bytes(slabs, Q) + (long long)slabs * Q * (long long)sizeof(int);
    return FN_OK;
}

extern "C" int fn_radius_count(const float* queries, int Q, const float* gallery, int G, int E, int metric, float eps, const int32_t* skip,
                               int slab_rows, void* workspace, int64_t* offsets, int32_t* range, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("radius_count", Q, G, slab_rows, &srows, &slabs)) return rc;
    if (int rc = check_walk_args("radius_count", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(eps == eps, "radius_count: eps is NaN");
    FN_REQUIRE(offsets && (uintptr_t)offsets % 8 == 0, "radius_count: offsets must be an 8-byte aligned int64 [Q + 1]");
    hipStream_t st = (hipStream_t)stream;
    long long* base = (long long*)workspace;
    int* counts = (int*)((char*)workspace + rd_base_bytes(slabs, Q));
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    hipLaunchKernelGGL(radius_kernel<false>, dim3((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs), dim3(256), 0, st, queries, Q, gallery, G, E, metric, eps,
                       (const int*)skip, srows, counts, (const long long*)nullptr, (int*)nullptr, (float*)nullptr, 0LL, (int*)range);
    hipLaunchKernelGGL(radius_scan_kernel, dim3(1), dim3(SCAN_T), 0, st, (const int*)counts, slabs, Q, base, (long long*)offsets);
    return check_launch("radius_count");
}

extern "C" int fn_radius_fill(const float* queries, int Q, const float* gallery, int G, int E, int metric, float eps, const int32_t* skip,
                              int slab_rows, const void* workspace, int32_t* cols, float* dist, long long capacity, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("radius_fill", Q, G, slab_rows, &srows, &slabs)) return rc;
    if (int rc = check_walk_args("radius_fill", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(eps == eps, "radius_fill: eps is NaN");
    FN_REQUIRE(capacity >= 0 && (capacity == 0 || (cols && dist)), "radius_fill: cols and dist must hold `capacity` >= 0 elements");
    if (capacity == 0) return FN_OK;
    hipLaunchKernelGGL(radius_kernel<true>, dim3((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, queries, Q, gallery, G,
                       E, metric, eps, (const int*)skip, srows, (int*)nullptr, (const long long*)workspace, (int*)cols, dist, capacity,
                       (int*)nullptr);
    return check_launch("radius_fill");
}

extern "C" int fn_dbscan_init(int N, const int64_t* offsets, int min_samples, int32_t* labels, int32_t* core, int32_t* info, void* stream) {
    FN_REQUIRE(N >= 1 && min_samples >= 1, "dbscan: N and min_samples must be at least 1 (N %d, min_samples %d)", N, min_samples);
    FN_REQUIRE(offsets && labels && core && info, "dbscan_init: bad arguments");
    hipLaunchKernelGGL(dbscan_init_kernel, dim3((unsigned)cdiv(N > DB_INFO_WORDS ? N : DB_INFO_WORDS, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)offsets, N, min_samples, (int*)labels, (int*)core, (int*)info);
    return check_launch("dbscan_init");
}

extern "C" int fn_dbscan_rounds(int N, const int64_t* offsets, const int32_t* cols, const int32_t* core, int32_t* labels, int32_t* info,
                                int rounds, void* stream) {
    FN_REQUIRE(N >= 1 && rounds >= 1 && rounds <= 1024, "dbscan_rounds: N must be at least 1 and rounds in [1, 1024] (N %d, rounds %d)", N, rounds);
    FN_REQUIRE(offsets && core && labels && info, "dbscan_rounds: bad arguments");     // cols may be NULL when the CSR is empty
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(N, 256));
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(dbscan_hook_kernel, grid, dim3(256), 0, st, (const long long*)offsets, (const int*)cols, (const int*)core, N, (int*)labels,
                           (int*)info);
        hipLaunchKernelGGL(dbscan_jump_kernel, grid, dim3(256), 0, st, (const int*)core, N, (int*)labels, (int*)info);
    }
    return check_launch("dbscan_rounds");
}

extern "C" int fn_dbscan_finish(int N, const int64_t* offsets, const int32_t* cols, const float* dist, int metric, const float* emb, int E,
                                const int32_t* core, int32_t* labels, int32_t* ids, int32_t* info, void* stream) {
    FN_REQUIRE(N >= 1, "dbscan: N and min_samples must be at least 1 (N %d)", N);
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);
    FN_REQUIRE(offsets && core && labels && ids && info, "dbscan_finish: bad arguments");
    FN_REQUIRE(metric == 0 || (emb && E >= 1), "dbscan_finish: metric 1 needs the embeddings, to recompute the metric-0 distance of the border rule");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(N, 256));
    hipLaunchKernelGGL(dbscan_border_kernel, grid, dim3(256), 0, st, (const long long*)offsets, (const int*)cols, dist, metric, emb, E,
                       (const int*)core, N, (int*)labels, (int*)ids, (const int*)info);
    hipLaunchKernelGGL(dbscan_ids_kernel, dim3(1), dim3(SCAN_T), 0, st, (int*)ids, N, (int*)info);
    hipLaunchKernelGGL(dbscan_relabel_kernel, grid, dim3(256), 0, st, (const int*)ids, N, (int*)labels, (int*)info);
    return check_launch("dbscan_finish");
}
