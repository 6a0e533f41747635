// What the kernels that walk a gallery in 64 x 64 exact-fp32 super-tiles share (identify.hip: the k nearest rows; cluster.hip:
// every row within a radius): the tile constants, one thread's share of a staged chunk with its global load and LDS store, the
// ordered-int encoding of the `range` words, and the rule that cuts a gallery into slabs.  ONE definition: the two files must
// stage and multiply in the same order for their distances to agree bit for bit (common.h).
#pragma once
#include "common.h"

namespace fn {

constexpr int IT = F32_TILE;         // query rows per workgroup, gallery rows per super-tile
constexpr int IE = F32_CHUNK;        // embedding chunk
constexpr int ILD = F32_LD;          // LDS row stride in floats (common.h: the staging validation.hip uses)

__device__ __forceinline__ int id_ord(float f) {
    const int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

struct IdChunk {      // one thread's share of a staged chunk: 2 float4 of the query tile, 2 of the gallery tile
    float4 a[2], b[2];
};

__device__ __forceinline__ void id_load(IdChunk& c, const float* __restrict__ qrows, int nq, const float* __restrict__ grows, int ng, int E,
                                        int e0, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256, r = t >> 3, col = e0 + (t & 7) * 4;
        c.a[i] = (r < nq && col < E) ? *reinterpret_cast<const float4*>(qrows + (long)r * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        c.b[i] = (r < ng && col < E) ? *reinterpret_cast<const float4*>(grows + (long)r * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__device__ __forceinline__ void id_store(const IdChunk& c, float (*sA)[ILD], float (*sB)[ILD], int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256, r = t >> 3, p = f32_chunk_pos((t & 7) * 4);
        sA[r][p] = c.a[i].x; sA[r][p + 4] = c.a[i].y; sA[r][p + 8] = c.a[i].z; sA[r][p + 12] = c.a[i].w;
        sB[r][p] = c.b[i].x; sB[r][p + 4] = c.b[i].y; sB[r][p + 8] = c.b[i].z; sB[r][p + 12] = c.b[i].w;
    }
}

// Slab height (a multiple of 64) and count.  Chosen by the library: about 8192 workgroups in all (32 per CU: the tail of the
// last round stays small), but never slabs of fewer than 512 rows, whose first super-tiles (the search's thresholds still open,
// every value a survivor) would weigh too much; with many query tiles this is one slab.
static inline int id_slabs(int Q, int G, int slab_rows, int* rows_out) {
    const long qtiles = cdiv(Q, IT);
    long rows = slab_rows;
    if (rows <= 0) {
        const long want = cdiv(8192, qtiles);
        rows = cdiv(G, want);
        if (rows < 512) rows = 512;
    }
    rows = (rows + IT - 1) / IT * IT;
    if (rows > (1L << 30)) rows = 1L << 30;
    *rows_out = (int)rows;
    return cdiv(G, rows);
}

}  // namespace fn
