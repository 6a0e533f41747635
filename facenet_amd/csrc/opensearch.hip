// Open-set 1:N evaluation: for each of Q probes its nearest MATE (the nearest gallery row of its own
// identity), its nearest IMPOSTOR (the nearest row of any other identity) and the RANK of that mate (how many impostors lie
// before it), without the [Q, G] distance matrix ever reaching memory and without the k <= 64 limit of the top-k lists.
//
// Arithmetic (exact): pair_tiles.h's.  s, sc, d0 = pair_distance(s, 0) and the key bits(d0) << 32 | row are the very bits of
// identify.hip, cluster.hip, validation.hip and verification.hip; the smallest key wins, so equal distances go to the lower row.
//
// mate_search_kernel<RANK>: one workgroup of 4 waves per (64 query rows, slab of gallery rows), wave w = query rows 16w..16w+15,
// on pair_tiles.h's walk_gallery, as radius_kernel.  A lane holds 4 query rows x 4 column tiles of a super-tile.
//   RANK = false: per query row two running minima, one over its mates and one over its impostors.  A lane meets its columns in
//     ascending order (column tiles and super-tiles ascend), so within a lane "smaller key" is "strictly smaller bits(d0)": the
//     minimum is kept as (bits(d0), column), 2 x 2 x 4 = 16 registers, and becomes the 64-bit key after the walk, when the 16
//     lanes of a lane group reduce theirs with shuffles and lane 0 of the group writes partial[slab][q][2].
//   RANK = true: a second walk, since the count needs the mate's key first.  It reads each row's final mate key and counts the
//     admissible impostor keys below it per lane; the lane group adds the counts as integers into counts[slab][q].
// No LDS beyond sA / sB, no workgroup barrier of its own, no atomics: rows belong to one wave, every (slab, q) word has one writer.
// mate_merge_kernel: one thread per (q, population) takes the minimum over the slabs, writes row and distance (metric 1: arccos
// of the recomputed chain, as gallery_merge_kernel) and keeps the mate key for the second walk.  mate_rank_kernel: one thread per
// q adds the slabs' counts.  Minima of unique keys and integer sums: the result depends neither on slab_rows nor on scheduling.
//
// The Q <= 16 mode of gallery_search_kernel (the four waves split the column tiles of one query tile) is NOT built: this is an
// evaluation over many probes; a handful of probes still runs, with three waves of its one query tile idle.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

typedef unsigned long long u64;
constexpr u64 ONONE = ~0ull;       // "no such row": it decodes to row -1

__device__ __forceinline__ u64 group_min(u64 v) {      // over the 16 lanes of a lane group
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool RANK>
__global__ __launch_bounds__(256, 4) void mate_search_kernel(const float* __restrict__ queries, int Q, const int* __restrict__ qlabels,
                                                          const float* __restrict__ gallery, int G, const int* __restrict__ glabels, int E,
                                                          const int* __restrict__ skip, int slab_rows, u64* __restrict__ partial,
                                                          const u64* __restrict__ mate_key, int* __restrict__ counts, int* __restrict__ range) {
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)G, (long)g0 + slab_rows);     // g0 < G < 2^31; the sum may pass it
    const int nq = Q - q0;                                     // >= 1
    const bool wave_live = wave * 16 < nq;
    int below[4];
    unsigned best_d[2][4];                                     // [mate / impostor][row]: bits(d0) of the nearest so far ...
    int best_c[2][4];                                          // ... and its column; all ones: none
    u64 mkey[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + wave * 16 + lg * 4 + r;
        mkey[r] = (RANK && q < Q) ? mate_key[q] : 0;           // all ones (no mate) counts every impostor: mate_rank_kernel drops it
        below[r] = 0;
        best_d[0][r] = best_d[1][r] = 0xffffffffu;
        best_c[0][r] = best_c[1][r] = -1;
    }
    DotRange seen;
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
    walk_gallery(sA, sB, queries + (long)q0 * E, nq, gallery, g0, g1, E, wave_live, wave * 16, -1, [&](int c0, f32x4 (&acc)[4]) {
        // The rows' labels and skip rows are read again for every super-tile (8 cached loads against 64 x 64 x E multiply-adds)
        // instead of living in 8 registers through the multiplication, which is where the register budget is met.
        int glab[4], qlab[4], skip_row[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int col = c0 + ct * 16 + lr;
            glab[ct] = col < g1 ? glabels[col] : -1;           // all twelve loads are in flight together
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + wave * 16 + lg * 4 + r;
            qlab[r] = q < Q ? qlabels[q] : -1;
            skip_row[r] = (skip && q < Q) ? skip[q] : -1;
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int col = c0 + ct * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = acc[ct][r];
                // padding rows and zero-padded columns (d0 = 2: nearer than a real row beyond that) leave before any comparison
                const bool real = wave * 16 + lg * 4 + r < nq && col < g1;
                if (!RANK && real) seen.add(s);                // skipped pairs included, as fn_gallery_search
                const bool admissible = real && col != skip_row[r];
                const bool mate = glab[ct] == qlab[r] && qlab[r] >= 0;         // label -1: a probe known to be absent
                const unsigned d = __float_as_uint(pair_distance(s, 0));
                if (RANK) {
                    const u64 key = ((u64)d << 32) | (unsigned)col;
                    below[r] += admissible && !mate && key < mkey[r];
                } else {
                    const unsigned dm = (admissible && mate) ? d : 0xffffffffu, di = (admissible && !mate) ? d : 0xffffffffu;
                    if (dm < best_d[0][r]) best_d[0][r] = dm, best_c[0][r] = col;      // strict: an equal distance keeps the lower column
                    if (di < best_d[1][r]) best_d[1][r] = di, best_c[1][r] = col;
                }
            }
        }
    });
    if (!RANK) seen.publish(range, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + wave * 16 + lg * 4 + r;
        if (RANK) {
            const int n = group_sum(below[r]);                 // <= slab_rows <= 2^30; 0 from a wave that is not live
            if (lr == 0 && q < Q) counts[(long)slab * Q + q] = n;
        } else {
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const u64 key = group_min(((u64)best_d[w][r] << 32) | (unsigned)best_c[w][r]);
                if (lr == 0 && q < Q) partial[((long)slab * Q + q) * 2 + w] = key;
            }
        }
    }
}

// One thread per (q, w): w = 0 the mate, 1 the impostor.  dist from the key (metric 0) or arccos of the recomputed chain (metric 1:
// the key holds d0, from which sc cannot be recovered exactly).
__global__ __launch_bounds__(256) void mate_merge_kernel(const u64* __restrict__ partial, int slabs, int Q, int metric,
                                                         const float* __restrict__ queries, const float* __restrict__ gallery, int E,
                                                         float* __restrict__ dist, int* __restrict__ rows, u64* __restrict__ mate_key) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2L * Q) return;
    u64 key = ONONE;
    for (int s = 0; s < slabs; ++s) {
        const u64 v = partial[(long)s * Q * 2 + i];
        key = v < key ? v : key;
    }
    const int q = (int)(i >> 1);
    if (!(i & 1)) mate_key[q] = key;
    if (key == ONONE) {
        dist[i] = __int_as_float(0x7f800000);
        rows[i] = -1;
        return;
    }
    const int row = (int)(unsigned)(key & 0xffffffffull);
    float d = __uint_as_float((unsigned)(key >> 32));
    if (metric == 1) d = pair_distance(dot_chain(queries + (long)q * E, gallery + (long)row * E, E), 1);
    dist[i] = d;
    rows[i] = row;
}

__global__ __launch_bounds__(256) void mate_rank_kernel(const int* __restrict__ counts, const u64* __restrict__ mate_key, int slabs, int Q,
                                                        int* __restrict__ rank) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    int n = 0;                                                 // <= G - 1 < 2^31
    for (int s = 0; s < slabs; ++s) n += counts[(long)s * Q + q];
    rank[q] = mate_key[q] == ONONE ? -1 : n;
}

// workspace: partial u64 [slabs][Q][2], mate_key u64 [Q], counts int32 [slabs][Q]
static long long ms_partial_bytes(int slabs, int Q) { return (long long)slabs * Q * 2 * (long long)sizeof(u64); }
static long long ms_key_bytes(int Q) { return (long long)Q * (long long)sizeof(u64); }

}  // namespace fn
using namespace fn;

extern "C" int fn_mate_search_workspace(int Q, int G, int slab_rows, long long* bytes) {
    int srows, slabs;
    if (int rc = check_walk_shape("mate_search_workspace", Q, G, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(bytes, "mate_search_workspace: bad arguments");
    *bytes = ms_partial_bytes(slabs, Q) + ms_key_bytes(Q) + (long long)slabs * Q * (long long)sizeof(int);
    return FN_OK;
}

extern "C" int fn_mate_search(const float* queries, int Q, const int32_t* query_labels, const float* gallery, int G,
                              const int32_t* gallery_labels, int E, int metric, const int32_t* skip, int slab_rows, void* workspace,
                              float* dist, int32_t* rows, int32_t* rank, int32_t* range, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("mate_search", Q, G, slab_rows, &srows, &slabs)) return rc;
    if (int rc = check_walk_args("mate_search", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(query_labels && gallery_labels, "mate_search: query_labels and gallery_labels must be given");
    FN_REQUIRE(dist && rows, "mate_search: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    u64* partial = (u64*)workspace;
    u64* mate_key = (u64*)((char*)workspace + ms_partial_bytes(slabs, Q));
    int* counts = (int*)((char*)mate_key + ms_key_bytes(Q));
    const dim3 grid((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs);
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    hipLaunchKernelGGL(mate_search_kernel<false>, grid, dim3(256), 0, st, queries, Q, (const int*)query_labels, gallery, G,
                       (const int*)gallery_labels, E, (const int*)skip, srows, partial, (const u64*)nullptr, (int*)nullptr, (int*)range);
    hipLaunchKernelGGL(mate_merge_kernel, dim3((unsigned)cdiv(2L * Q, 256)), dim3(256), 0, st, (const u64*)partial, slabs, Q, metric, queries,
                       gallery, E, dist, (int*)rows, mate_key);
    if (rank) {
        hipLaunchKernelGGL(mate_search_kernel<true>, grid, dim3(256), 0, st, queries, Q, (const int*)query_labels, gallery, G,
                           (const int*)gallery_labels, E, (const int*)skip, srows, (u64*)nullptr, (const u64*)mate_key, counts, (int*)nullptr);
        hipLaunchKernelGGL(mate_rank_kernel, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, st, (const int*)counts, (const u64*)mate_key, slabs, Q,
                           (int*)rank);
    }
    return check_launch("mate_search");
}
