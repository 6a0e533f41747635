// The exact-fp32 pair machinery: ONE definition of everything that decides a bit of a pair's distance or of the `range` words, for
// the kernels that compare distances exactly (validation.hip: the confusion counts; identify.hip and ivf.hip: the k nearest rows;
// opensearch.hip: the nearest mate and impostor; cluster.hip: every row within a radius; faceclass.hip takes tri_decode alone).
// DESIGN.md section 16.  loss.hip's fn_pairwise_sqdist takes ord_f32, DotRange and pair_distance from here but NOT the dot
// product: it sums s by wavefront reduction, so its distances agree with the chain's to rounding, not in bits.
// verification.hip histograms the bit patterns of d themselves (the exact TAR at FAR, EER and ROC: DESIGN.md section 23).
//
// What it guarantees: a dot product s is the ascending-e fmaf chain from 0.0f (v_mfma_f32_16x16x4_f32 fed through mfma_chunk is
// that chain bit for bit, and so is dot_chain); sc = min(max(s, -1), 1); d = 2 (1 - sc) (metric 0) or arccos(sc) (metric 1); the
// callers compare d with the strict fp32 <.  `range` receives ord_f32 of the smallest and largest RAW s of the pairs a kernel
// evaluated, and keeps its initial words (which decode to hi < lo) when it evaluated none.
//
// Which pairs are evaluated is defined here too: the gallery walk (identify.hip, ivf.hip, opensearch.hip, cluster.hip) and the class-pair
// walk (validation.hip's confidence_folds_kernel, verification.hip's pair_key_histogram_kernel, false_pairs.hip's
// false_pairs_kernel; confidence_kernel keeps its own scalar walk: it is the independent reference of the exactness tests).
//
// A new consumer of the gallery walk supplies a prologue (its per-row state) and on_tile(c0, acc), the epilogue of one super-tile.
// A new consumer of the class-pair walk supplies what it does with a valid pair's dot product, inside the loops that section shows.
#pragma once
#include "common.h"

namespace fn {

// ---- scalars -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ord_f32(float f) {      // order-preserving float -> int
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

// min / max of the raw dot products one lane has met.  write: one lane of a wave that evaluated a pair.  publish: the whole wave.
struct DotRange {
    float hi = -3e38f, lo = 3e38f;      // (in this order pairwise_kernel compiles to the very code it had)
    __device__ __forceinline__ void add(float s) {
        lo = fminf(lo, s);
        hi = fmaxf(hi, s);
    }
    __device__ __forceinline__ void write(int* __restrict__ range) const {
        atomicMin(&range[0], ord_f32(lo));
        atomicMax(&range[1], ord_f32(hi));
    }
    __device__ __forceinline__ void publish(int* __restrict__ range, int lane) {
        lo = -wave_max(-lo);
        hi = wave_max(hi);
        if (lane == 0 && range && hi >= lo) write(range);
    }
};

// statistics.py:45-53
__device__ __forceinline__ float pair_distance(float s, int metric) {
    const float sc = fminf(fmaxf(s, -1.f), 1.f);
    return (metric == 0) ? 2.f * (1.f - sc) : acosf(sc);
}

// the chain itself, for the kernels that recompute single pairs
__device__ __forceinline__ float dot_chain(const float* __restrict__ x, const float* __restrict__ y, int E) {
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fmaf(x[e], y[e], s);
    return s;
}

// first n with thr[n] > d over T ascending thresholds: d < thr[n] holds from there on
__device__ __forceinline__ int threshold_bin(const float* thr, int T, float d) {
    int l = 0, h = T;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (thr[m] > d) h = m; else l = m + 1;
    }
    return l;
}

// (i, k), k <= i, from the linear index b = i (i + 1) / 2 + k
__device__ __forceinline__ void tri_decode(long b, int& i, int& k) {
    i = (int)((sqrtf(8.f * (float)b + 1.f) - 1.f) * 0.5f);
    while ((long)i * (i + 1) / 2 > b) --i;
    while ((long)(i + 1) * (i + 2) / 2 <= b) ++i;
    k = (int)(b - (long)i * (i + 1) / 2);
}

// ---- staging -----------------------------------------------------------------------------------------------------------------
// 64 x 64 super-tiles, 32-wide embedding chunks, LDS rows of 36 floats (16-byte aligned, conflict-free ds_read_b128 per 16 lanes).
// Column c of a chunk goes to LDS position f32_chunk_pos(c): inside each block of 16 the 4x4 (step, lane group) index is
// transposed, so that the float4 a lane of group g reads holds k = 4s + g for the four MFMA steps s = 0..3 in order.
constexpr int F32_TILE = 64, F32_CHUNK = 32, F32_LD = F32_CHUNK + 4;
__device__ __forceinline__ int f32_chunk_pos(int c) { return (c & 16) | ((c & 3) << 2) | ((c >> 2) & 3); }

// One thread's share (of 256) of a 64-row chunk: rows beyond `rows` and columns beyond E are zeros, which add fma(0, 0, acc) = acc.
__device__ __forceinline__ void rows_load(float4 (&v)[2], const float* __restrict__ src, int rows, int E, int e0, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256, r = t >> 3, col = e0 + (t & 7) * 4;
        v[i] = (r < rows && col < E) ? *reinterpret_cast<const float4*>(src + (long)r * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void rows_store(const float4 (&v)[2], float (*dst)[F32_LD], int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256, r = t >> 3, p = f32_chunk_pos((t & 7) * 4);     // the four elements: lane groups 0..3 of one step
        dst[r][p] = v[i].x; dst[r][p + 4] = v[i].y; dst[r][p + 8] = v[i].z; dst[r][p + 12] = v[i].w;
    }
}

struct IdChunk {      // one thread's share of a staged chunk: 2 float4 of the query tile, 2 of the gallery tile
    float4 a[2], b[2];
};
__device__ __forceinline__ void id_load(IdChunk& c, const float* __restrict__ qrows, int nq, const float* __restrict__ grows, int ng, int E,
                                        int e0, int tid) {
    rows_load(c.a, qrows, nq, E, e0, tid);
    rows_load(c.b, grows, ng, E, e0, tid);
}
__device__ __forceinline__ void id_store(const IdChunk& c, float (*sA)[F32_LD], float (*sB)[F32_LD], int tid) {
    rows_store(c.a, sA, tid);
    rows_store(c.b, sB, tid);
}

// The same chunk without a prefetch; vec: E % 4 == 0 (rows are 16-byte aligned), else element by element.
__device__ __forceinline__ void stage_rows(float (*dst)[F32_LD], const float* __restrict__ src, int rows, int E, int e0, bool vec, int tid) {
    if (vec) {
        float4 v[2];
        rows_load(v, src, rows, E, e0, tid);
        rows_store(v, dst, tid);
    } else {
        for (int t = tid; t < F32_TILE * F32_CHUNK; t += 256) {
            const int r = t >> 5, c = t & 31;
            dst[r][f32_chunk_pos(c)] = (r < rows && e0 + c < E) ? src[(long)r * E + e0 + c] : 0.f;
        }
    }
}

// ---- the MFMA block: the 32 k of a staged chunk in ascending order into 16 x 16 accumulators ------------------------------------
// A rows arow + (lane & 15); C/D layout: column = lane & 15, row = 4 (lane >> 4) + register.
__device__ __forceinline__ f32x4 mfma_operand(const float (*s)[F32_LD], int row, int blk) {
    const int lane = threadIdx.x & 63;
    return *reinterpret_cast<const f32x4*>(&s[row + (lane & 15)][blk * 16 + (lane >> 4) * 4]);
}
__device__ __forceinline__ f32x4 mfma_step(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc[ct]: B rows 16 ct .. 16 ct + 15.  The four accumulators are independent and interleaved.
__device__ __forceinline__ void mfma_chunk(const float (*sA)[F32_LD], const float (*sB)[F32_LD], int arow, f32x4 (&acc)[4]) {
#pragma unroll
    for (int blk = 0; blk < F32_CHUNK / 16; ++blk) {
        const f32x4 av = mfma_operand(sA, arow, blk);
        f32x4 bv[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bv[ct] = mfma_operand(sB, ct * 16, blk);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma_step(av[s], bv[ct][s], acc[ct]);
    }
}
// the same with a wave-uniform mask: a column tile that is not live is not read
__device__ __forceinline__ void mfma_chunk(const float (*sA)[F32_LD], const float (*sB)[F32_LD], int arow, f32x4 (&acc)[4], const bool (&live)[4]) {
#pragma unroll
    for (int blk = 0; blk < F32_CHUNK / 16; ++blk) {
        const f32x4 av = mfma_operand(sA, arow, blk);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (!live[ct]) continue;
            const f32x4 bv = mfma_operand(sB, ct * 16, blk);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[ct] = mfma_step(av[s], bv[s], acc[ct]);
        }
    }
}
// one column tile: B rows brow .. brow + 15
__device__ __forceinline__ void mfma_chunk(const float (*sA)[F32_LD], const float (*sB)[F32_LD], int arow, int brow, f32x4& acc) {
#pragma unroll
    for (int blk = 0; blk < F32_CHUNK / 16; ++blk) {
        const f32x4 av = mfma_operand(sA, arow, blk), bv = mfma_operand(sB, brow, blk);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma_step(av[s], bv[s], acc);
    }
}

// ---- the gallery walk ----------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads multiplies its <= 64 query rows (qrows, nq of them) with the gallery rows [g0, g1) in 64-column
// super-tiles; the next chunk's global loads are in flight while the current one is multiplied.  A live wave's A rows are
// arow .. arow + 15; it fills acc[ct] for columns c0 + 16 ct .. c0 + 16 ct + 15 (brow < 0), or acc[0] alone for the columns
// c0 + brow .. c0 + brow + 15.  After each super-tile a live wave (wave_live is wave-uniform) calls on_tile(c0, acc), c0 the
// super-tile's first gallery row; acc is zero again when the next one starts.  Rows >= nq and columns >= g1 are zero padding:
// on_tile must leave them out.  A workgroup barrier separates the caller's LDS initialisation from the first on_tile.
template <typename OnTile>
__device__ __forceinline__ void walk_gallery(float (*sA)[F32_LD], float (*sB)[F32_LD], const float* __restrict__ qrows, int nq,
                                             const float* __restrict__ gallery, int g0, int g1, int E, bool wave_live, int arow, int brow,
                                             OnTile on_tile) {
    const int tid = threadIdx.x;
    const int nchunk = (E + F32_CHUNK - 1) / F32_CHUNK, ntile = (g1 - g0 + F32_TILE - 1) / F32_TILE;
    f32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    IdChunk next;
    id_load(next, qrows, nq, gallery + (long)g0 * E, g1 - g0, E, 0, tid);
    for (int tile = 0; tile < ntile; ++tile) {
        const int c0 = g0 + tile * F32_TILE;
        for (int ch = 0; ch < nchunk; ++ch) {
            __syncthreads();                                   // the previous chunk has been read
            id_store(next, sA, sB, tid);
            __syncthreads();
            if (ch + 1 < nchunk)
                id_load(next, qrows, nq, gallery + (long)c0 * E, g1 - c0, E, (ch + 1) * F32_CHUNK, tid);
            else if (tile + 1 < ntile)
                id_load(next, qrows, nq, gallery + (long)(c0 + F32_TILE) * E, g1 - c0 - F32_TILE, E, 0, tid);
            if (!wave_live) continue;
            if (brow >= 0) mfma_chunk(sA, sB, arow, brow, acc[0]);
            else mfma_chunk(sA, sB, arow, acc);
        }
        if (!wave_live) continue;
        on_tile(c0, acc);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// ---- the class-pair walk -------------------------------------------------------------------------------------------------------
// Which row pairs of a pool sorted by class are evaluated, and in which population.  The grid is class_pair_groups' (host, below):
// the first diag_groups workgroups of 256 threads walk the diagonal class pairs (i, i) with that stride and evaluate the strict
// upper triangle (genuine pairs); the other off_groups walk the off-diagonal pairs (i, k), i > k, with theirs and evaluate the
// whole rectangle (impostor pairs).  So `diag` is workgroup-uniform.  A class pair is covered with 64 x 64 super-tiles; wave w
// multiplies its rows 16 w .. 16 w + 15 with four 16 x 16 column tiles, and a column tile without a pair is neither read nor live.
//
//     for (ClassPair p(C, diag_groups, off_groups); p.next(cls_start);)       all threads; the caller's per-pair state goes here
//         for (PairTile t; t.next(p);) {                                      all threads
//             t.dots(p, sA, sB, emb, E, vec);                                 all threads: it holds the barriers of the chunk loop
//             for ct: if (t.live[ct]) for r: if (t.ok(p, ct, r)) ... t.acc[ct][r], t.ia(r), t.ib(ct) ...      wave-level
//         }
//
// live[] is wave-uniform; ok() is per lane.  A consumer supplies what it does with a valid pair's dot product and nothing else.
struct ClassPair {
    bool diag;                               // this workgroup's population: genuine (strict upper triangle) or impostor
    long b, npairs, stride;
    int i, k, a0, na, b0, nb;                // classes i >= k: rows a0 .. a0 + na - 1 against rows b0 .. b0 + nb - 1
    __device__ __forceinline__ ClassPair(int C, int diag_groups, int off_groups) {
        diag = (int)blockIdx.x < diag_groups;
        npairs = diag ? (long)C : (long)C * (C - 1) / 2;
        stride = diag ? diag_groups : off_groups;
        b = (diag ? (long)blockIdx.x : (long)blockIdx.x - diag_groups) - stride;
    }
    __device__ __forceinline__ bool next(const int* __restrict__ cls_start) {
        while ((b += stride) < npairs) {
            if (diag) {
                i = k = (int)b;
            } else {                         // b = j (j + 1) / 2 + k with k <= j, i = j + 1 > k
                tri_decode(b, i, k);
                i += 1;
            }
            a0 = cls_start[i], na = cls_start[i + 1] - a0;
            b0 = cls_start[k], nb = cls_start[k + 1] - b0;
            if (!(diag && na < 2)) return true;      // else: no pair at all
        }
        return false;
    }
};

struct PairTile {
    int ta = 0, tb = -F32_TILE, r0;          // the super-tile's first row and column within the classes; this wave's first row
    bool live[4];
    f32x4 acc[4];                            // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
    __device__ __forceinline__ bool next(const ClassPair& p) {     // row-major; a super-tile entirely on/below the diagonal is left out
        do {
            if ((tb += F32_TILE) >= p.nb) ta += F32_TILE, tb = 0;
            if (ta >= p.na || p.nb < 1) return false;
        } while (p.diag && tb + F32_TILE - 1 <= ta);
        return true;
    }
    __device__ __forceinline__ void dots(const ClassPair& p, float (*sA)[F32_LD], float (*sB)[F32_LD], const float* __restrict__ emb, int E, bool vec) {
        const int tid = threadIdx.x, wave = tid >> 6;
        r0 = ta + wave * 16;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int c0 = tb + ct * 16;
            live[ct] = r0 < p.na && c0 < p.nb && !(p.diag && c0 + 15 <= r0);
            acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int e0 = 0; e0 < E; e0 += F32_CHUNK) {
            __syncthreads();
            stage_rows(sA, emb + (long)(p.a0 + ta) * E, p.na - ta, E, e0, vec, tid);
            stage_rows(sB, emb + (long)(p.b0 + tb) * E, p.nb - tb, E, e0, vec, tid);
            __syncthreads();
            mfma_chunk(sA, sB, wave * 16, acc, live);
        }
    }
    __device__ __forceinline__ int ia(int r) const { return r0 + ((threadIdx.x & 63) >> 4) * 4 + r; }
    __device__ __forceinline__ int ib(int ct) const { return tb + ct * 16 + (threadIdx.x & 15); }
    __device__ __forceinline__ bool ok(const ClassPair& p, int ct, int r) const {
        return ia(r) < p.na && ib(ct) < p.nb && !(p.diag && ib(ct) <= ia(r));      // strict upper triangle (statistics.py:32-34)
    }
};

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The grid of the class-pair walk: diag_groups + off_groups workgroups.  false: more classes than the walk takes.
static inline bool class_pair_groups(int C, int* diag_groups, int* off_groups) {
    const long off_pairs = (long)C * (C - 1) / 2;
    *diag_groups = C < 256 ? C : 256;
    *off_groups = (int)(off_pairs < 2048 ? off_pairs : 2048);
    return C < 65536;
}

// Slab height (a multiple of 64) and count.  Chosen by the library: about 8192 workgroups in all (32 per CU: the tail of the
// last round stays small), but never slabs of fewer than 512 rows, whose first super-tiles (the search's thresholds still open,
// every value a survivor) would weigh too much; with many query tiles this is one slab.
static inline int id_slabs(int Q, int G, int slab_rows, int* rows_out) {
    const long qtiles = cdiv(Q, F32_TILE);
    long rows = slab_rows;
    if (rows <= 0) {
        const long want = cdiv(8192, qtiles);
        rows = cdiv(G, want);
        if (rows < 512) rows = 512;
    }
    rows = (rows + F32_TILE - 1) / F32_TILE * F32_TILE;
    if (rows > (1L << 30)) rows = 1L << 30;
    *rows_out = (int)rows;
    return cdiv(G, rows);
}

// The argument rules of every entry point that walks a gallery, in two parts: the shape (-> the slab height and count), which
// the workspace queries check too, and the operands of a launch.
static inline int check_walk_shape(const char* what, int Q, int G, int slab_rows, int* srows, int* slabs) {
    FN_REQUIRE(Q >= 1 && G >= 1, "%s: Q and G must be at least 1 (Q %d, G %d)", what, Q, G);
    FN_REQUIRE(slab_rows >= 0, "%s: bad arguments", what);
    *slabs = id_slabs(Q, G, slab_rows, srows);
    FN_REQUIRE(*slabs <= 65535, "%s: %d slabs of %d rows (at most 65535)", what, *slabs, *srows);
    return FN_OK;
}
static inline int check_walk_args(const char* what, const void* queries, const void* gallery, const void* workspace, int E, int metric) {
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "%s: the embedding length must be a multiple of 4 in [4, 512] (E %d)", what, E);
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);   // statistics.py:55
    FN_REQUIRE(queries && gallery && workspace, "%s: bad arguments", what);
    FN_REQUIRE(((uintptr_t)queries | (uintptr_t)gallery | (uintptr_t)workspace) % 16 == 0,
               "%s: queries, gallery and workspace must be 16-byte aligned", what);
    return FN_OK;
}

}  // namespace fn
