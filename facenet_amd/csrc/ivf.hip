// The inverted-file (IVF) index of a gallery: the centroid step of spherical k-means, and the exact
// k-nearest search over the lists each query probes.
//
// fn_kmeans_update: one workgroup per list, lanes along e, the members' rows read in ascending row order: sum[c][e] is the
// sequential fp64 sum, so a call is reproducible bit for bit; no atomics.
//
// fn_ivf_search: the arithmetic, the key and the selection are fn_gallery_search's (pair_tiles.h, topk_select.h), over the rows of
// the probed lists only; the key's low word is ids[stored row], the ORIGINAL row.  Five launches, no host round trip:
//   ivf_count_kernel     (query, probe) pairs per list (integer atomics)
//   ivf_plan_kernel      one workgroup: the exclusive scan of the counts -> each list's block of the gathered query table, and
//                        the tile descriptors (list, first gathered row, <= 64 rows)
//   ivf_gather_kernel    one wave per pair copies its query row into its list's block; the slot inside the block comes from an
//                        atomic cursor: the result cannot depend on it, keys are unique per query
//   ivf_search_kernel    one workgroup of 4 waves per descriptor walks [list_start[l], list_start[l + 1]) with the gathered block
//                        as query rows; a pair's ascending k-list goes to partial[pair]
//   ivf_merge_kernel     one wave per query cuts its nprobe partial lists to k
// The grid of the search is the bound  sum_l ceil(c_l / 64) <= floor(P / 64) + min(L, P),  P = Q nprobe; surplus workgroups exit.
#include "topk_select.h"
#include "../../include/facenet_hip.h"

namespace fn {

constexpr int IVF_MAX_LISTS = 1 << 20;
constexpr long IVF_MAX_PAIRS = 1L << 28;
constexpr int PLAN_THREADS = 1024;

// ---- spherical k-means: the centroid step -------------------------------------------------------------------------------------
// n2 is the sequential ascending-e fp64 sum from 0.0 of the rounded products sum[e] * sum[e] (no fused multiply-add).
__device__ __forceinline__ double kmeans_n2(const double* __restrict__ sum, int E) {
#pragma clang fp contract(off)
    double n2 = 0.0;
    for (int e = 0; e < E; ++e) {
        const double p = sum[e] * sum[e];
        n2 = n2 + p;
    }
    return n2;
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ rows, int N, int E, const int* __restrict__ order,
                                                            const int* __restrict__ list_start, const float* __restrict__ prev,
                                                            float* __restrict__ centroids, int* __restrict__ kept) {
    __shared__ double sSum[512];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int m0 = min(max(list_start[c], 0), N), m1 = min(max(list_start[c + 1], m0), N);
    const auto row_of = [&](int m) { return (long)min(max(order[m], 0), N - 1) * E; };      // never outside the table
    const int e0 = tid, e1 = tid + 256;                        // E <= 512: at most two columns per thread
    const bool on0 = e0 < E, on1 = e1 < E;
    double s0 = 0.0, s1 = 0.0;
    int m = m0;
    for (; m + 4 <= m1; m += 4) {                              // four rows in flight; added in ascending member order
        long r[4];
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = row_of(m + i);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = on0 ? rows[r[i] + e0] : 0.f;
            b[i] = on1 ? rows[r[i] + e1] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s0 += (double)a[i];
            s1 += (double)b[i];
        }
    }
    for (; m < m1; ++m) {
        const long r = row_of(m);
        if (on0) s0 += (double)rows[r + e0];
        if (on1) s1 += (double)rows[r + e1];
    }
    if (on0) sSum[e0] = s0;
    if (on1) sSum[e1] = s1;
    __syncthreads();
    const double n2 = kmeans_n2(sSum, E);                      // every thread: the same order, the same bits
    const bool keep = m1 <= m0 || n2 == 0.0;
    if (tid == 0) kept[c] = keep ? 1 : 0;
    const double norm = sqrt(n2);
    if (on0) centroids[(long)c * E + e0] = keep ? prev[(long)c * E + e0] : (float)(s0 / norm);
    if (on1) centroids[(long)c * E + e1] = keep ? prev[(long)c * E + e1] : (float)(s1 / norm);
}

// ---- the probed-list search ---------------------------------------------------------------------------------------------------
// The workspace: a block of int32 words (count [L], cursor [L], qstart [L + 1], ntiles [1]), the descriptors
// int4 [D], slot_pair int32 [P], partial u64 [P][k], gathered fp32 [P][E]; every part starts on a multiple of 16 bytes.
struct IvfLayout {
    long count, cursor, qstart, ntiles, desc, slot_pair, partial, gathered, bytes;
    long P;
    int D;
};
static inline long up16(long b) { return (b + 15) / 16 * 16; }
static inline IvfLayout ivf_layout(int Q, int L, int nprobe, int E, int k) {
    IvfLayout w;
    w.P = (long)Q * nprobe;
    w.D = (int)(w.P / F32_TILE + (w.P < L ? w.P : L));
    w.count = 0;
    w.cursor = w.count + 4L * L;
    w.qstart = w.cursor + 4L * L;
    w.ntiles = w.qstart + 4L * (L + 1);
    w.desc = up16(w.ntiles + 4);
    w.slot_pair = w.desc + 16L * w.D;
    w.partial = up16(w.slot_pair + 4L * w.P);
    w.gathered = up16(w.partial + 8L * w.P * k);
    w.bytes = w.gathered + 4L * w.P * E;
    return w;
}

// the list of a pair, or -1: an entry outside [0, L) probes nothing
__device__ __forceinline__ int ivf_probe(const int* __restrict__ probes, long p, int L) {
    const int l = probes[p];
    return (l >= 0 && l < L) ? l : -1;
}

__global__ __launch_bounds__(256) void ivf_count_kernel(const int* __restrict__ probes, long P, int L, int* __restrict__ count) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const int l = ivf_probe(probes, p, L);
        if (l >= 0) atomicAdd(&count[l], 1);
    }
}

// One workgroup.  Thread t owns the lists [t per, (t + 1) per): their sums, an exclusive scan over the threads, then the starts
// and the descriptors of its lists.
__global__ __launch_bounds__(PLAN_THREADS) void ivf_plan_kernel(const int* __restrict__ count, int L, int* __restrict__ qstart,
                                                                int* __restrict__ ntiles, int4* __restrict__ desc) {
    __shared__ int sQ[PLAN_THREADS], sT[PLAN_THREADS];
    const int t = threadIdx.x, per = (L + PLAN_THREADS - 1) / PLAN_THREADS;
    const int l0 = min(L, t * per), l1 = min(L, l0 + per);
    int nq = 0, nt = 0;
    for (int l = l0; l < l1; ++l) {
        nq += count[l];
        nt += (count[l] + F32_TILE - 1) / F32_TILE;
    }
    sQ[t] = nq;
    sT[t] = nt;
    __syncthreads();
    for (int o = 1; o < PLAN_THREADS; o <<= 1) {               // inclusive scan over the threads
        const int aq = t >= o ? sQ[t - o] : 0, at = t >= o ? sT[t - o] : 0;
        __syncthreads();
        sQ[t] += aq;
        sT[t] += at;
        __syncthreads();
    }
    int q = sQ[t] - nq, d = sT[t] - nt;
    for (int l = l0; l < l1; ++l) {
        const int c = count[l];
        qstart[l] = q;
        for (int done = 0; done < c; done += F32_TILE) desc[d++] = make_int4(l, q + done, min(F32_TILE, c - done), 0);
        q += c;
    }
    if (t == PLAN_THREADS - 1) {
        qstart[L] = sQ[t];
        *ntiles = sT[t];
    }
}

// One wave per pair: its slot in its list's block, the pair's number there, and the query row.
__global__ __launch_bounds__(256) void ivf_gather_kernel(const float* __restrict__ queries, const int* __restrict__ probes, long P, int nprobe, int L,
                                                         int E, const int* __restrict__ qstart, int* __restrict__ cursor, int* __restrict__ slot_pair,
                                                         float* __restrict__ gathered) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int l = ivf_probe(probes, p, L);
    if (l < 0) return;
    int slot = 0;
    if (lane == 0) {
        slot = qstart[l] + atomicAdd(&cursor[l], 1);
        slot_pair[slot] = (int)p;
    }
    slot = __shfl(slot, 0);
    const float4* src = reinterpret_cast<const float4*>(queries + (p / nprobe) * E);
    float4* dst = reinterpret_cast<float4*>(gathered + (long)slot * E);
    for (int i = lane; i < E / 4; i += 64) dst[i] = src[i];
}

__global__ __launch_bounds__(256, 4) void ivf_search_kernel(const float* __restrict__ gathered, const int* __restrict__ slot_pair,
                                                         const int4* __restrict__ desc, const int* __restrict__ ntiles, const float* __restrict__ lists,
                                                         const int* __restrict__ ids, const int* __restrict__ list_start, int G, int E, int k,
                                                         int nprobe, const int* __restrict__ skip, u64* __restrict__ partial, int* __restrict__ range) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    __shared__ u64 sThr[F32_TILE];
    __shared__ int sCnt[F32_TILE];
    if ((int)blockIdx.x >= *ntiles) return;                    // the grid is a bound
    const int cap = id_cap(k);
    u64* sList = reinterpret_cast<u64*>(dyn);                  // [F32_TILE][cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lg = lane >> 4;
    const int4 d = desc[blockIdx.x];                           // list, first gathered row, rows
    const int first = d.y, nq = d.z;
    const int g0 = min(max(list_start[d.x], 0), G), g1 = min(max(list_start[d.x + 1], g0), G);
    if (tid < F32_TILE) {
        sThr[tid] = INONE;
        sCnt[tid] = 0;
    }
    const bool wave_live = wave * 16 < nq;
    int skip_row[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + lg * 4 + r;
        skip_row[r] = (skip && row < nq) ? skip[slot_pair[first + row] / nprobe] : -1;
    }
    DotRange seen;
    // the selection of gallery_search_kernel; the key's low word is the original row, and so is what skip names
    walk_gallery(sA, sB, gathered + (long)first * E, nq, lists, g0, g1, E, wave_live, wave * 16, -1, [&](int c0, f32x4 (&acc)[4]) {
        id_select_tile(c0, acc, g1, nq, wave, wave, false, skip_row, seen, sList, sThr, sCnt, cap, k, [&](int col) { return ids[col]; });
    });
    seen.publish(range, lane);
    __syncthreads();                                           // also orders the list initialisation for an empty list
    for (int r = 0; r < 16; ++r) {                             // ascending k-list of every row of this wave -> partial[pair][k]
        const int row = wave * 16 + r;
        if (row >= nq) break;
        id_emit(sList, sThr, sCnt, row, cap, k, lane, partial + (long)slot_pair[first + row] * k);
    }
}

// One wave per query: its nprobe ascending k-lists -> the final k.  dist from the key (metric 0) or arccos of the recomputed
// chain (metric 1); for the latter the stored row is found again: the partial list a key came from names its list, in which
// ids ascend.
__global__ __launch_bounds__(64) void ivf_merge_kernel(const u64* __restrict__ partial, const int* __restrict__ probes, int nprobe, int L, int k,
                                                       int metric, const float* __restrict__ queries, const float* __restrict__ lists,
                                                       const int* __restrict__ ids, const int* __restrict__ list_start, int G, int E,
                                                       float* __restrict__ dist, int* __restrict__ rows) {
    __shared__ u64 sList[IMERGE_CAP];
    __shared__ u64 sThr;
    __shared__ int sSrc[IMAXK];
    const int q = blockIdx.x, lane = threadIdx.x;
    const long total = (long)nprobe * k, p0 = (long)q * nprobe;
    const auto key_at = [&](long idx) {                        // a pair that probes nothing has no partial list
        const long j = idx / k;
        return ivf_probe(probes, p0 + j, L) >= 0 ? partial[p0 * k + idx] : INONE;
    };
    const int n = id_merge(sList, &sThr, total, k, lane, key_at);
    if (metric == 1) {
        sSrc[lane] = 0;
        __builtin_amdgcn_wave_barrier();
        for (long base = 0; base < total; base += 64) {
            const long idx = base + lane;
            const u64 key = idx < total ? key_at(idx) : INONE;
            if (key == INONE) continue;
            for (int i = 0; i < n; ++i)
                if (sList[i] == key) sSrc[i] = (int)(idx / k);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane >= k) return;
    const long o = (long)q * k + lane;
    if (lane >= n) {                                           // fewer than k admissible rows in the probed lists
        dist[o] = __int_as_float(0x7f800000);
        rows[o] = -1;
        return;
    }
    const u64 key = sList[lane];
    const int row = (int)(unsigned)(key & 0xffffffffull);
    float d = __uint_as_float((unsigned)(key >> 32));
    if (metric == 1) {
        const int l = max(ivf_probe(probes, p0 + sSrc[lane], L), 0);
        int lo = min(max(list_start[l], 0), G), hi = min(max(list_start[l + 1], lo), G);
        while (lo < hi) {                                      // first stored row of the list with ids >= row
            const int mid = (lo + hi) >> 1;
            if (ids[mid] < row) lo = mid + 1; else hi = mid;
        }
        lo = min(lo, G - 1);
        d = pair_distance(dot_chain(queries + (long)q * E, lists + (long)lo * E, E), 1);
    }
    dist[o] = d;
    rows[o] = row;
}

static int check_ivf_shape(int Q, int L, int nprobe, int E, int k) {
    FN_REQUIRE(Q >= 1 && L >= 1 && nprobe >= 1, "ivf_search: Q, L and nprobe must be at least 1 (Q %d, L %d, nprobe %d)", Q, L, nprobe);
    FN_REQUIRE(L <= IVF_MAX_LISTS, "ivf_search: %d lists (at most %d)", L, IVF_MAX_LISTS);
    FN_REQUIRE((long)Q * nprobe <= IVF_MAX_PAIRS, "ivf_search: Q * nprobe = %ld pairs (at most %ld)", (long)Q * nprobe, IVF_MAX_PAIRS);
    FN_REQUIRE(k >= 1 && k <= IMAXK, "ivf_search: k must be in [1, 64] (k %d)", k);
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "ivf_search: the embedding length must be a multiple of 4 in [4, 512] (E %d)", E);
    return FN_OK;
}

}  // namespace fn
using namespace fn;

extern "C" int fn_kmeans_update(const float* rows, int N, int E, const int32_t* order, const int32_t* list_start, int L, const float* prev,
                                float* centroids, int32_t* kept, void* stream) {
    FN_REQUIRE(N >= 1 && L >= 1, "kmeans_update: N and L must be at least 1 (N %d, L %d)", N, L);
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "kmeans_update: the embedding length must be a multiple of 4 in [4, 512] (E %d)", E);
    FN_REQUIRE(rows && order && list_start && prev && centroids && kept, "kmeans_update: bad arguments");
    FN_REQUIRE(prev != centroids, "kmeans_update: the new centroids must not overwrite the previous ones");
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)L), dim3(256), 0, (hipStream_t)stream, rows, N, E, (const int*)order, (const int*)list_start, prev,
                       centroids, (int*)kept);
    return check_launch("kmeans_update");
}

extern "C" int fn_ivf_search_workspace(int Q, int L, int nprobe, int E, int k, long long* bytes) {
    FN_REQUIRE(bytes, "ivf_search_workspace: bad arguments");
    if (int rc = check_ivf_shape(Q, L, nprobe, E, k)) return rc;
    *bytes = ivf_layout(Q, L, nprobe, E, k).bytes;
    return FN_OK;
}

extern "C" int fn_ivf_search(const float* queries, int Q, const float* lists, const int32_t* ids, int G, const int32_t* list_start, int L, int E,
                             const int32_t* probes, int nprobe, int k, int metric, const int32_t* skip, void* workspace, float* dist,
                             int32_t* rows, int32_t* range, void* stream) {
    if (int rc = check_ivf_shape(Q, L, nprobe, E, k)) return rc;
    FN_REQUIRE(G >= 1, "ivf_search: G must be at least 1 (G %d)", G);
    if (int rc = check_walk_args("ivf_search", queries, lists, workspace, E, metric)) return rc;
    FN_REQUIRE(ids && list_start && probes && dist && rows, "ivf_search: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const IvfLayout w = ivf_layout(Q, L, nprobe, E, k);
    char* ws = (char*)workspace;
    int *count = (int*)(ws + w.count), *cursor = (int*)(ws + w.cursor), *qstart = (int*)(ws + w.qstart);
    int *ntiles = (int*)(ws + w.ntiles), *slot_pair = (int*)(ws + w.slot_pair);
    int4* desc = (int4*)(ws + w.desc);
    u64* partial = (u64*)(ws + w.partial);
    float* gathered = (float*)(ws + w.gathered);
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    fill_words(count, 0u, 0u, 2 * L, st);                      // count and cursor
    hipLaunchKernelGGL(ivf_count_kernel, dim3((unsigned)(w.P / 256 + 1 < 4096 ? w.P / 256 + 1 : 4096)), dim3(256), 0, st, (const int*)probes, w.P, L, count);
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(PLAN_THREADS), 0, st, (const int*)count, L, qstart, ntiles, desc);
    hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)((w.P + 3) / 4)), dim3(256), 0, st, queries, (const int*)probes, w.P, nprobe, L, E,
                       (const int*)qstart, cursor, slot_pair, gathered);
    const size_t dyn = (size_t)F32_TILE * id_cap(k) * sizeof(u64);   // as gallery_search_kernel
    hipLaunchKernelGGL(ivf_search_kernel, dim3((unsigned)w.D), dim3(256), dyn, st, (const float*)gathered, (const int*)slot_pair, (const int4*)desc,
                       (const int*)ntiles, lists, (const int*)ids, (const int*)list_start, G, E, k, nprobe, (const int*)skip, partial, (int*)range);
    hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)Q), dim3(64), 0, st, (const u64*)partial, (const int*)probes, nprobe, L, k, metric, queries, lists,
                       (const int*)ids, (const int*)list_start, G, E, dist, (int*)rows);
    return check_launch("ivf_search");
}
