// The minimum spanning tree of a gallery's rows under the mutual-reachability distance: Boruvka's algorithm
// on the device, the structure single linkage at every threshold, DBSCAN* at every eps and HDBSCAN are read from.  The [N, N]
// matrix never reaches memory.
//
// Arithmetic (exact): pair_tiles.h's.  s is the ascending-e fmaf chain, d = pair_distance(s, 0), and the weight of the pair (i, j)
// is w = max(d, core[i], core[j]) in fp32 (core NULL: zeros).  s(i, j) = s(j, i) bit for bit, so w is symmetric.  Edges are
// ordered by (bits(w), lo, hi), lo = min(i, j), hi = max(i, j): a strict total order, so the minimum spanning tree is unique (it
// is what Kruskal returns on the edges sorted that way) and depends neither on slab_rows nor on scheduling.
//
// A round: mst_nearest_kernel (the hot path: one self-join walk on pair_tiles.h's walk_gallery with the workgroup shape of
// mate_search_kernel<false>) gives every row its smallest (bits(w), col) over the columns of OTHER components; the lowest column
// among equal weights is also the lowest (lo, hi) of that row, so the row's key is its minimum edge.  Then, O(N) each:
//   merge: the minimum over the slabs -> rowkey[row]; a 64-bit atomic min of bits(w) << 32 | lo per component;
//   tie:   the rows that attain it lower the component's hi with a 32-bit atomic min: (bits(w), lo, hi) is the true minimum;
//   hook:  every component's root emits its edge and hangs itself under the other end's component.  Under the total order the
//          chosen edges form a forest whose only cycles are the pairs of components that chose the same edge: that edge is emitted
//          from the smaller component id, which stays a root;
//   jump:  every row follows parent[] from its component to the root (parent[] is not written here) and lowers minrow[root];
//   relabel: comp[row] = minrow[root], the smallest row of the merged component;
//   end:   one thread: rounds, components = N - edges, done.
// Every loop is bounded and no kernel waits for another workgroup.  Every kernel of a round returns at once when info[0] (done)
// is set, so the caller can enqueue ceil(log2 N) rounds (Boruvka's bound: a round at least halves the components) and read info
// once.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

typedef unsigned long long u64;
constexpr u64 MST_NONE = ~0ull;        // "no row outside my component"
enum { MST_DONE = 0, MST_ROUNDS = 1, MST_COMPONENTS = 2, MST_EDGES = 3, MST_INFO_WORDS = 8 };

__device__ __forceinline__ u64 mst_group_min(u64 v) {      // over the 16 lanes of a lane group
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// One workgroup of 4 waves per (64 rows, slab of columns), wave w = rows 16w..16w+15.  A lane holds 4 rows x 4 column tiles of a
// super-tile and meets its columns in ascending order, so within a lane "smaller key" is "strictly smaller bits(w)".  No LDS
// beyond sA / sB, no atomics: every (slab, row) word has one writer.
__global__ __launch_bounds__(256, 4) void mst_nearest_kernel(const float* __restrict__ rows, int N, int E, const float* __restrict__ core,
                                                          const int* __restrict__ comp, int slab_rows, u64* __restrict__ partial,
                                                          const int* __restrict__ info) {
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    if (info[MST_DONE]) return;                                // (no kernel of this launch writes it: uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)N, (long)g0 + slab_rows);     // g0 < N < 2^31; the sum may pass it
    const int nq = N - q0;                                     // >= 1
    const bool wave_live = wave * 16 < nq;
    unsigned best_w[4];                                        // bits(w) of the nearest row of another component so far ...
    int best_c[4];                                             // ... and its column; all ones: none
#pragma unroll
    for (int r = 0; r < 4; ++r) best_w[r] = 0xffffffffu, best_c[r] = -1;
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
    walk_gallery(sA, sB, rows + (long)q0 * E, nq, rows, g0, g1, E, wave_live, wave * 16, -1, [&](int c0, f32x4 (&acc)[4]) {
        // comp[] and core[] of the rows and columns are read again for every super-tile, as glabels in mate_search_kernel
        int ccomp[4], rcomp[4];
        float ccore[4], rcore[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int col = c0 + ct * 16 + lr;
            ccomp[ct] = col < g1 ? comp[col] : -1;
            ccore[ct] = (core && col < g1) ? core[col] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + wave * 16 + lg * 4 + r;
            rcomp[r] = q < N ? comp[q] : -1;
            rcore[r] = (core && q < N) ? core[q] : 0.f;
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int col = c0 + ct * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // padding rows and zero-padded columns (d = 2: a plausible weight) leave before any comparison
                const bool real = wave * 16 + lg * 4 + r < nq && col < g1;
                const float w = fmaxf(fmaxf(pair_distance(acc[ct][r], 0), rcore[r]), ccore[ct]);
                const unsigned k = (real && ccomp[ct] != rcomp[r]) ? __float_as_uint(w) : 0xffffffffu;
                if (k < best_w[r]) best_w[r] = k, best_c[r] = col;             // strict: an equal weight keeps the lower column
            }
        }
    });
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + wave * 16 + lg * 4 + r;
        const u64 key = mst_group_min(((u64)best_w[r] << 32) | (unsigned)best_c[r]);
        if (lr == 0 && q < N) partial[(long)slab * N + q] = key;
    }
}

// ---- contraction: plain kernels, one thread per row, O(N) per round -------------------------------------------------------------
struct MstWork {
    u64* partial;          // [slabs][N]
    u64* rowkey;           // [N]  the row's minimum edge: bits(w) << 32 | col
    u64* cbest;            // [N]  per component id: min bits(w) << 32 | lo
    unsigned* chi;         // [N]  per component id: min hi among the edges that attain cbest
    int* parent;           // [N]  per component id: the component it hangs under
    int* minrow;           // [N]  per root: the smallest row of the merged component
    int* root;             // [N]  per row: the root its component reached
};

__device__ __forceinline__ u64 mst_wlo(u64 key, int row) {    // bits(w) << 32 | min(row, col)
    const unsigned col = (unsigned)(key & 0xffffffffull);
    return (key & 0xffffffff00000000ull) | min((unsigned)row, col);
}

__global__ void mst_reset_kernel(MstWork k, int N, const int* __restrict__ info) {
    if (info[MST_DONE]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    k.cbest[i] = MST_NONE;
    k.chi[i] = 0xffffffffu;
    k.parent[i] = i;
    k.minrow[i] = 0x7fffffff;
}

__global__ void mst_merge_kernel(MstWork k, int slabs, int N, const int* __restrict__ comp, const int* __restrict__ info) {
    if (info[MST_DONE]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    u64 key = MST_NONE;
    for (int s = 0; s < slabs; ++s) {
        const u64 v = k.partial[(long)s * N + i];
        key = v < key ? v : key;
    }
    k.rowkey[i] = key;
    if (key != MST_NONE) atomicMin(&k.cbest[comp[i]], mst_wlo(key, i));
}

__global__ void mst_tie_kernel(MstWork k, int N, const int* __restrict__ comp, const int* __restrict__ info) {
    if (info[MST_DONE]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const u64 key = k.rowkey[i];
    if (key == MST_NONE) return;
    const int c = comp[i];
    if (mst_wlo(key, i) == k.cbest[c]) atomicMin(&k.chi[c], max((unsigned)i, (unsigned)(key & 0xffffffffull)));
}

__global__ void mst_hook_kernel(MstWork k, int N, const int* __restrict__ comp, int* __restrict__ edges, float* __restrict__ weights,
                                int* __restrict__ info) {
    if (info[MST_DONE]) return;                                // (set by mst_end_kernel alone)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N || comp[c] != c) return;                        // the component's id is its smallest row
    const u64 best = k.cbest[c];
    if (best == MST_NONE) return;                              // nothing outside: the last component (or no comparable weight)
    const int lo = (int)(unsigned)(best & 0xffffffffull), hi = (int)k.chi[c];
    if (lo < 0 || hi <= lo || hi >= N) return;
    const int other = comp[lo] == c ? comp[hi] : comp[lo];
    const bool mutual = k.cbest[other] == best && k.chi[other] == (unsigned)hi;
    if (mutual && other < c) {                                 // the smaller component emits the edge and stays a root
        k.parent[c] = other;
        return;
    }
    if (!mutual) k.parent[c] = other;
    const int at = atomicAdd(&info[MST_EDGES], 1);
    if (at < N - 1) {
        edges[2 * at] = lo;
        edges[2 * at + 1] = hi;
        weights[at] = __uint_as_float((unsigned)(best >> 32));
    }
}

__global__ void mst_jump_kernel(MstWork k, int N, const int* __restrict__ comp, const int* __restrict__ info) {
    if (info[MST_DONE]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    // parent[] is a forest (see the head of the file) that no thread of this launch writes: at most N - 1 steps reach a root.
    int p = comp[i];
    for (int step = 0; step < N; ++step) {
        const int pp = k.parent[p];
        if (pp == p) break;
        p = pp;
    }
    k.root[i] = p;
    atomicMin(&k.minrow[p], i);
}

__global__ void mst_relabel_kernel(MstWork k, int N, int* __restrict__ comp, const int* __restrict__ info) {
    if (info[MST_DONE]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) comp[i] = k.minrow[k.root[i]];
}

__global__ void mst_end_kernel(int N, int* __restrict__ info) {
    if (info[MST_DONE] || threadIdx.x || blockIdx.x) return;
    info[MST_ROUNDS] += 1;
    info[MST_COMPONENTS] = N - info[MST_EDGES];
    if (info[MST_EDGES] >= N - 1) info[MST_DONE] = 1;
}

__global__ void mst_init_kernel(int N, int* __restrict__ comp, int* __restrict__ info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < MST_INFO_WORDS) info[i] = i == MST_DONE ? N == 1 : i == MST_COMPONENTS ? N : 0;
    if (i < N) comp[i] = i;
}

static long long mst_align(long long b) { return (b + 15) / 16 * 16; }
// workspace: partial, rowkey, cbest (u64), then chi, parent, minrow, root (32-bit), each 16-byte aligned
static long long mst_carve(void* workspace, int slabs, int N, MstWork* k) {
    char* p = (char*)workspace;
    long long at = 0;
    auto take = [&](long long bytes) {
        char* here = p + at;
        at += mst_align(bytes);
        return here;
    };
    k->partial = (u64*)take((long long)slabs * N * 8);
    k->rowkey = (u64*)take((long long)N * 8);
    k->cbest = (u64*)take((long long)N * 8);
    k->chi = (unsigned*)take((long long)N * 4);
    k->parent = (int*)take((long long)N * 4);
    k->minrow = (int*)take((long long)N * 4);
    k->root = (int*)take((long long)N * 4);
    return at;
}

}  // namespace fn
using namespace fn;

extern "C" int fn_mst_workspace(int N, int slab_rows, long long* bytes) {
    int srows, slabs;
    if (int rc = check_walk_shape("mst_workspace", N, N, slab_rows, &srows, &slabs)) return rc;
    FN_REQUIRE(bytes, "mst_workspace: bad arguments");
    MstWork k;
    *bytes = mst_carve(nullptr, slabs, N, &k);
    return FN_OK;
}

extern "C" int fn_mst_init(int N, int32_t* comp, int32_t* info, void* stream) {
    FN_REQUIRE(N >= 1, "mst: N must be at least 1 (N %d)", N);
    FN_REQUIRE(comp && info, "mst_init: bad arguments");
    hipLaunchKernelGGL(mst_init_kernel, dim3((unsigned)cdiv(N > MST_INFO_WORDS ? N : MST_INFO_WORDS, 256)), dim3(256), 0, (hipStream_t)stream, N,
                       (int*)comp, (int*)info);
    return check_launch("mst_init");
}

extern "C" int fn_mst_rounds(const float* rows, int N, int E, const float* core, int slab_rows, void* workspace, int32_t* comp, int32_t* edges,
                             float* weights, int32_t* info, int rounds, void* stream) {
    int srows, slabs;
    if (int rc = check_walk_shape("mst_rounds", N, N, slab_rows, &srows, &slabs)) return rc;
    if (int rc = check_walk_args("mst_rounds", rows, rows, workspace, E, 0)) return rc;
    FN_REQUIRE(rounds >= 1 && rounds <= 64, "mst_rounds: rounds must be in [1, 64] (rounds %d)", rounds);
    FN_REQUIRE(comp && info && (N == 1 || (edges && weights)), "mst_rounds: bad arguments");
    if (N == 1) return FN_OK;                                  // done at init: nothing to write
    hipStream_t st = (hipStream_t)stream;
    MstWork k;
    mst_carve(workspace, slabs, N, &k);
    const dim3 walk((unsigned)cdiv(N, F32_TILE), (unsigned)slabs), grid((unsigned)cdiv(N, 256));
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(mst_reset_kernel, grid, dim3(256), 0, st, k, N, (const int*)info);
        hipLaunchKernelGGL(mst_nearest_kernel, walk, dim3(256), 0, st, rows, N, E, core, (const int*)comp, srows, k.partial, (const int*)info);
        hipLaunchKernelGGL(mst_merge_kernel, grid, dim3(256), 0, st, k, slabs, N, (const int*)comp, (const int*)info);
        hipLaunchKernelGGL(mst_tie_kernel, grid, dim3(256), 0, st, k, N, (const int*)comp, (const int*)info);
        hipLaunchKernelGGL(mst_hook_kernel, grid, dim3(256), 0, st, k, N, (const int*)comp, (int*)edges, weights, (int*)info);
        hipLaunchKernelGGL(mst_jump_kernel, grid, dim3(256), 0, st, k, N, (const int*)comp, (const int*)info);
        hipLaunchKernelGGL(mst_relabel_kernel, grid, dim3(256), 0, st, k, N, (int*)comp, (const int*)info);
        hipLaunchKernelGGL(mst_end_kernel, dim3(1), dim3(64), 0, st, N, (int*)info);
    }
    return check_launch("mst_rounds");
}
