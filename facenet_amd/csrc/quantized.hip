// The quantised gallery: an int8 shortlist on v_mfma_i32_16x16x64_i8, the exact fp32 re-rank of the
// shortlist and a certificate that says whether a row outside the shortlist could have entered the top k.
//
// fn_quantize_rows: one wave per fp32 row x: m = max |x_e|, code c_e = rint((double) x_e * 127.0 / (double) m) (fp64, half to
// even) as int8 [N][Ep] (Ep = E rounded up to 64, zero filled), scale = (float)((double) m / 127.0), rho = ||x - scale c|| and
// norm = ||x|| as sequential fp64 sums of rounded squares, IEEE square root, stored as the smallest float not below it.
//
// fn_qgallery_search, two launches (three when a query has more than 64 partial lists), no host round trip:
//   qgallery_shortlist_kernel   one workgroup per (64 query rows, slab): idot = the int32 dot product of two code rows (an exact
//                               integer in any order), s^ = (sq sg) (float) idot, key = bits(pair_distance(s^, 0)) << 32 | row, the
//                               R smallest per (slab, query) by topk_select.h exactly as gallery_search_kernel keeps its k
//   qgallery_rerank_kernel      one wave per query: the slabs' lists -> the R-key shortlist; s = dot_chain on the fp32 tables for
//                               its rows (the bits of every other search), cut to k; the certificate in fp64
// The shortlist is a pure function of the inputs; a certified query's answer is fn_gallery_search's bit for bit.
#include "topk_select.h"
#include "../../include/facenet_hip.h"

namespace fn {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int Q8_PAD = 64;                 // code rows are padded to a multiple of this: no MFMA step straddles a row's end
constexpr int Q8_CHUNK = 128;              // code bytes of a row staged per chunk: two 64-deep MFMA steps
constexpr int Q8_LD = Q8_CHUNK + 16;       // LDS row of 144 bytes: 16-byte aligned, 36 words (the stride of pair_tiles.h)

__host__ __device__ __forceinline__ int q8_padded(int E) { return (E + Q8_PAD - 1) / Q8_PAD * Q8_PAD; }

// List capacity of a row of the shortlist kernel.  id_select_tile cuts a list once it holds more than cap - 16 keys, so with
// id_cap(R) (R + 16 for R = 64) a row that keeps 64 keys is cut after every tile that appends one; here it is cut after 8 to 48
// appended keys.  At most 88: 64 x 88 x 8 bytes of lists and the static tiles stay below the 64 KiB default; id_prune takes <= 128.
__host__ __device__ __forceinline__ int q8_cap(int R) { return R + 48 < 88 ? R + 48 : 88; }

// ---- quantisation -------------------------------------------------------------------------------------------------------------
// the smallest float >= v, v >= 0 finite
__device__ __forceinline__ float float_not_below(double v) {
    const float f = (float)v;
    return (double)f < v ? __uint_as_float(__float_as_uint(f) + 1u) : f;
}

// sequential ascending sum from 0.0 of sq[0 .. E), each already a rounded square
__device__ __forceinline__ double seq_sum(const double* __restrict__ sq, int E) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc = acc + sq[e];
    return acc;
}

// (code, residual squared, square) of one element; every product is rounded before it is used
__device__ __forceinline__ int quantize_element(float x, double m, float scale, double& res2, double& x2) {
#pragma clang fp contract(off)
    const double xd = (double)x;
    int c = 0;
    if (m > 0.0) {
        const double p = xd * 127.0;
        c = (int)rint(p / m);
    }
    const double sc = (double)scale * (double)c;
    const double t = xd - sc;
    res2 = t * t;
    x2 = xd * xd;
    return c;
}

__global__ __launch_bounds__(256) void quantize_rows_kernel(const float* __restrict__ rows, int N, int E, int Ep, signed char* __restrict__ codes,
                                                            float* __restrict__ scale, float* __restrict__ rho, float* __restrict__ norm) {
    __shared__ double sRes[4][512], sSq[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = (long)blockIdx.x * 4 + wave;
    if (n >= N) return;                                        // no workgroup barrier below: a wave works on its own
    const float4* src = reinterpret_cast<const float4*>(rows + n * E);
    float4 v[2];
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {                              // E <= 512: at most two float4 per lane
        const int w = lane + i * 64;
        v[i] = w < E / 4 ? src[w] : make_float4(0.f, 0.f, 0.f, 0.f);
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[i].x), fabsf(v[i].y)), fmaxf(fabsf(v[i].z), fabsf(v[i].w))));
    }
    mx = wave_max(mx);
    const double m = (double)mx;
    const float sc = mx > 0.f ? (float)(m / 127.0) : 0.f;
    unsigned* out = reinterpret_cast<unsigned*>(codes + n * Ep);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int w = lane + i * 64;
        if (w >= Ep / 4) continue;
        unsigned packed = 0u;
        if (w < E / 4) {
            const float x[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = quantize_element(x[j], m, sc, sRes[wave][w * 4 + j], sSq[wave][w * 4 + j]);
                packed |= ((unsigned)c & 0xffu) << (8 * j);
            }
        }
        out[w] = packed;                                       // the padding bytes are zeros
    }
    __builtin_amdgcn_wave_barrier();                           // one wave: its LDS operations execute in program order
    if (lane == 0) {
        scale[n] = sc;
        rho[n] = float_not_below(sqrt(seq_sum(sRes[wave], E)));
    }
    if (lane == 1) norm[n] = float_not_below(sqrt(seq_sum(sSq[wave], E)));
}

// ---- the code walk: walk_gallery of pair_tiles.h over int8 rows ----------------------------------------------------------------
struct CodeChunk {                         // one thread's share (of 256) of a staged chunk: 64 rows x 128 bytes of either table
    i32x4 a[2], b[2];
};
__device__ __forceinline__ void codes_load(i32x4 (&v)[2], const signed char* __restrict__ src, int rows, int Ep, int e0, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256, r = t >> 3, col = e0 + (t & 7) * 16;
        v[i] = (r < rows && col < Ep) ? *reinterpret_cast<const i32x4*>(src + (long)r * Ep + col) : i32x4{0, 0, 0, 0};
    }
}
__device__ __forceinline__ void codes_store(const i32x4 (&v)[2], signed char (*dst)[Q8_LD], int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int t = tid + i * 256;
        *reinterpret_cast<i32x4*>(&dst[t >> 3][(t & 7) * 16]) = v[i];
    }
}
// Lane l holds the 16 bytes (lane >> 4) of a 64-byte step of row (lane & 15), for A and for B alike: whatever k the hardware
// gives a (lane group, byte), both operands give it the same one, and the sum of integers has no order.
__device__ __forceinline__ i32x4 code_operand(const signed char (*s)[Q8_LD], int row, int step) {
    const int lane = threadIdx.x & 63;
    return *reinterpret_cast<const i32x4*>(&s[row + (lane & 15)][step * 64 + (lane >> 4) * 16]);
}

// As walk_gallery: a workgroup of 256 threads multiplies its <= 64 query code rows with the gallery code rows [g0, g1) in
// 64-column super-tiles, the next chunk's loads in flight while the current one is multiplied.  A live wave's A rows are
// arow .. arow + 15; it fills acc[ct] for columns c0 + 16 ct .. (brow < 0) or acc[0] for c0 + brow .. c0 + brow + 15, and calls
// on_tile(c0, acc) after each super-tile.  Rows >= nq and columns >= g1 are zero padding.
template <typename OnTile>
__device__ __forceinline__ void walk_codes(signed char (*sA)[Q8_LD], signed char (*sB)[Q8_LD], const signed char* __restrict__ qcodes, int nq,
                                           const signed char* __restrict__ gcodes, int g0, int g1, int Ep, bool wave_live, int arow, int brow,
                                           OnTile on_tile) {
    const int tid = threadIdx.x;
    const int nchunk = (Ep + Q8_CHUNK - 1) / Q8_CHUNK, ntile = (g1 - g0 + F32_TILE - 1) / F32_TILE;
    i32x4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = i32x4{0, 0, 0, 0};
    CodeChunk next;
    codes_load(next.a, qcodes, nq, Ep, 0, tid);
    codes_load(next.b, gcodes + (long)g0 * Ep, g1 - g0, Ep, 0, tid);
    for (int tile = 0; tile < ntile; ++tile) {
        const int c0 = g0 + tile * F32_TILE;
        for (int ch = 0; ch < nchunk; ++ch) {
            __syncthreads();                                   // the previous chunk has been read
            codes_store(next.a, sA, tid);
            codes_store(next.b, sB, tid);
            __syncthreads();
            if (ch + 1 < nchunk) {
                codes_load(next.a, qcodes, nq, Ep, (ch + 1) * Q8_CHUNK, tid);
                codes_load(next.b, gcodes + (long)c0 * Ep, g1 - c0, Ep, (ch + 1) * Q8_CHUNK, tid);
            } else if (tile + 1 < ntile) {
                codes_load(next.a, qcodes, nq, Ep, 0, tid);
                codes_load(next.b, gcodes + (long)(c0 + F32_TILE) * Ep, g1 - c0 - F32_TILE, Ep, 0, tid);
            }
            if (!wave_live) continue;
#pragma unroll
            for (int step = 0; step < Q8_CHUNK / 64; ++step) {
                if (ch * Q8_CHUNK + step * 64 >= Ep) break;    // wave-uniform: the chunk's second half lies beyond the row
                const i32x4 av = code_operand(sA, arow, step);
                if (brow >= 0) {
                    acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, code_operand(sB, brow, step), acc[0], 0, 0, 0);
                } else {
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, code_operand(sB, ct * 16, step), acc[ct], 0, 0, 0);
                }
            }
        }
        if (!wave_live) continue;
        on_tile(c0, acc);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = i32x4{0, 0, 0, 0};
    }
}

// ---- first stage: the shortlist -----------------------------------------------------------------------------------------------
// gallery_search_kernel with the code walk: partial[pslab][q][R] receives the R smallest keys of (slab, query), ascending.
__global__ __launch_bounds__(256, 4) void qgallery_shortlist_kernel(const signed char* __restrict__ qcodes, const float* __restrict__ qscale, int Q,
                                                                    const signed char* __restrict__ gcodes, const float* __restrict__ gscale, int G,
                                                                    int Ep, int R, const int* __restrict__ skip, int slab_rows, int split,
                                                                    u64* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) signed char sA[F32_TILE][Q8_LD], sB[F32_TILE][Q8_LD];
    __shared__ u64 sThr[F32_TILE];
    __shared__ int sCnt[F32_TILE];
    const int cap = q8_cap(R);
    u64* sList = reinterpret_cast<u64*>(dyn);                  // [F32_TILE][cap]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int q0 = blockIdx.x * F32_TILE, slab = blockIdx.y;
    const int g0 = slab * slab_rows, g1 = (int)min((long)G, (long)g0 + slab_rows);
    const int nq = Q - q0;                                     // >= 1
    if (tid < F32_TILE) {
        sThr[tid] = INONE;
        sCnt[tid] = 0;
    }
    const int qwave = split ? 0 : wave;                        // split (Q <= 16): the four waves take one column tile each
    const bool wave_live = qwave * 16 < nq;
    int skip_row[4];
    float sq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + qwave * 16 + lg * 4 + r;
        skip_row[r] = (skip && q < Q) ? skip[q] : -1;
        sq[r] = q < Q ? qscale[q] : 0.f;
    }
    DotRange unused;                                           // `range` belongs to the re-rank: s^ is not a chain value
    walk_codes(sA, sB, qcodes + (long)q0 * Ep, nq, gcodes, g0, g1, Ep, wave_live, qwave * 16, split ? wave * 16 : -1, [&](int c0, i32x4 (&acc)[4]) {
        f32x4 est[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            if (split && ct > 0) break;
            const int col = c0 + (split ? wave : ct) * 16 + lr;
            const float sg = col < g1 ? gscale[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) est[ct][r] = (sq[r] * sg) * (float)acc[ct][r];      // |idot| < 2^24: the conversion is exact
        }
        id_select_tile(c0, est, g1, nq, qwave, wave, split, skip_row, unused, sList, sThr, sCnt, cap, R, [](int col) { return col; });
    });
    __syncthreads();                                           // also orders the list initialisation for an empty slab walk
    const long pslab = split ? (long)slab * 4 + wave : slab;
    for (int r = 0; r < 16; ++r) {
        const int qrow = qwave * 16 + r, row = wave * 16 + r;
        if (qrow >= nq) break;
        id_emit(sList, sThr, sCnt, row, cap, R, lane, partial + (pslab * Q + q0 + qrow) * R);
    }
}

// ---- between the stages: many partial lists are merged by many waves first ---------------------------------------------------
// With Q <= 16 and a long gallery a query has thousands of partial lists (four per 512-row slab) and one wave per query would
// merge them all.  Beyond 2 Q8_FANIN lists, one wave per (query, group of Q8_FANIN lists) cuts the group to R keys first.
constexpr int Q8_FANIN = 32;
static int q8_groups(int nlists) { return nlists > 2 * Q8_FANIN ? cdiv(nlists, Q8_FANIN) : 0; }

__global__ __launch_bounds__(64) void qgallery_premerge_kernel(const u64* __restrict__ partial, int nlists, int Q, int R, u64* __restrict__ merged) {
    __shared__ u64 sList[IMERGE_CAP];
    __shared__ u64 sThr;
    const int q = blockIdx.x, grp = blockIdx.y, lane = threadIdx.x;
    const long l0 = (long)grp * Q8_FANIN;
    const long nl = min((long)Q8_FANIN, nlists - l0);
    const int n = id_merge(sList, &sThr, nl * R, R, lane, [&](long idx) {
        const long sl = idx / R;
        return partial[((l0 + sl) * Q + q) * R + (idx - sl * R)];
    });
    if (lane < R) merged[((long)grp * Q + q) * R + lane] = lane < n ? sList[lane] : INONE;
}

// ---- second stage: re-rank and certificate ------------------------------------------------------------------------------------
// B of DESIGN.md section 27 and the right-hand side d~_R - 2 B - 8 u, in fp64 in the written order; false: the row norms are
// outside what the slack was derived for.  A NaN makes every comparison with the result false.
__device__ __forceinline__ bool certificate_rhs(double rq, double nq, double rho_max, double norm_max, int E, float d_R, double& rhs) {
#pragma clang fp contract(off)
    const double u = 0x1p-24;
    const double eu = (double)E * u;
    const double gamma = eu / (1.0 - eu);
    const double t1 = rq * norm_max;
    const double xq = nq + rq;
    const double t2 = xq * rho_max;
    const double gn = gamma * nq;
    const double t3 = gn * norm_max;
    double B = t1 + t2;
    B = B + t3;
    B = B + 4.0 * u;
    rhs = (double)d_R - 2.0 * B;
    rhs = rhs - 8.0 * u;
    const double yq = norm_max + rho_max;
    const double w = xq * yq;
    return w <= 1.05;
}

__global__ __launch_bounds__(64) void qgallery_rerank_kernel(const u64* __restrict__ partial, int nlists, int Q, int R, int k, int metric,
                                                             const float* __restrict__ queries, const float* __restrict__ gallery, int E,
                                                             const float* __restrict__ qrho, const float* __restrict__ qnorm, double rho_max,
                                                             double norm_max, float* __restrict__ dist, int* __restrict__ rows,
                                                             int* __restrict__ certified, u64* __restrict__ shortlist_keys, int* __restrict__ range) {
    __shared__ u64 sList[IMERGE_CAP], sKey[IMAXK];
    __shared__ u64 sThr, sThr2;
    __shared__ __align__(16) float sQ[512];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int n = id_merge(sList, &sThr, (long)nlists * R, R, lane, [&](long idx) {
        const long sl = idx / R;
        return partial[(sl * Q + q) * R + (idx - sl * R)];
    });
    if (shortlist_keys && lane < R) shortlist_keys[(long)q * R + lane] = lane < n ? sList[lane] : INONE;
    const bool full = n == R;
    const float d_R = full ? __uint_as_float((unsigned)(sList[R - 1] >> 32)) : 0.f;
    for (int e = lane; e < E; e += 64) sQ[e] = queries[(long)q * E + e];
    __syncthreads();
    DotRange seen;
    if (lane < n) {                                            // dot_chain with the query in LDS and the row read 16 bytes at a time
        const int row = (int)(unsigned)(sList[lane] & 0xffffffffull);
        const float4* g = reinterpret_cast<const float4*>(gallery + (long)row * E);
        float s = 0.f;
        for (int e = 0; e < E; e += 4) {
            const float4 gv = g[e >> 2];
            s = fmaf(sQ[e], gv.x, s);
            s = fmaf(sQ[e + 1], gv.y, s);
            s = fmaf(sQ[e + 2], gv.z, s);
            s = fmaf(sQ[e + 3], gv.w, s);
        }
        seen.add(s);
        sKey[lane] = ((u64)__float_as_uint(pair_distance(s, 0)) << 32) | (unsigned)row;
    }
    seen.publish(range, lane);
    if (lane == 0) sThr2 = INONE;
    __syncthreads();
    const int m = id_prune(sKey, n, k, &sThr2, lane);
    if (lane == 0) {
        bool cert = true;
        if (full) {                                            // then m == k: R >= k
            double rhs;
            const bool in_domain = certificate_rhs((double)qrho[q], (double)qnorm[q], rho_max, norm_max, E, d_R, rhs);
            const float d0_k = __uint_as_float((unsigned)(sKey[k - 1] >> 32));
            cert = in_domain && (double)d0_k < rhs;
        }
        certified[q] = cert ? 1 : 0;
    }
    if (lane >= k) return;
    const long o = (long)q * k + lane;
    if (lane >= m) {                                           // fewer than k admissible rows
        dist[o] = __int_as_float(0x7f800000);
        rows[o] = -1;
        return;
    }
    const u64 key = sKey[lane];
    const int row = (int)(unsigned)(key & 0xffffffffull);
    float d = __uint_as_float((unsigned)(key >> 32));
    if (metric == 1) d = pair_distance(dot_chain(queries + (long)q * E, gallery + (long)row * E, E), 1);
    dist[o] = d;
    rows[o] = row;
}

static int q8_lists(int Q) { return Q <= 16 ? 4 : 1; }

static int check_qshape(int Q, int G, int k, int shortlist, int slab_rows, int* srows, int* slabs) {
    if (int rc = check_walk_shape("qgallery_search", Q, G, slab_rows, srows, slabs)) return rc;
    FN_REQUIRE(k >= 1 && k <= IMAXK, "qgallery_search: k must be in [1, 64] (k %d)", k);
    FN_REQUIRE(shortlist >= k && shortlist <= IMAXK, "qgallery_search: shortlist must be in [k, 64] (k %d, shortlist %d)", k, shortlist);
    return FN_OK;
}

}  // namespace fn
using namespace fn;

extern "C" int fn_quantize_rows(const float* rows, int N, int E, int8_t* codes, float* scale, float* rho, float* norm, void* stream) {
    FN_REQUIRE(N >= 1, "quantize_rows: N must be at least 1 (N %d)", N);
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "quantize_rows: the embedding length must be a multiple of 4 in [4, 512] (E %d)", E);
    FN_REQUIRE(rows && codes && scale && rho && norm, "quantize_rows: bad arguments");
    FN_REQUIRE(((uintptr_t)rows | (uintptr_t)codes) % 16 == 0, "quantize_rows: rows and codes must be 16-byte aligned");
    hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, rows, N, E, q8_padded(E), (signed char*)codes,
                       scale, rho, norm);
    return check_launch("quantize_rows");
}

extern "C" int fn_qgallery_search_workspace(int Q, int G, int k, int shortlist, int slab_rows, long long* bytes) {
    FN_REQUIRE(bytes && slab_rows >= 0, "qgallery_search_workspace: bad arguments");
    int srows, slabs;
    if (int rc = check_qshape(Q, G, k, shortlist, slab_rows, &srows, &slabs)) return rc;
    const int nlists = slabs * q8_lists(Q);                    // <= 4 * 65535; the groups of the pre-merge follow the lists
    *bytes = ((long long)nlists + q8_groups(nlists)) * Q * shortlist * (long long)sizeof(u64);
    return FN_OK;
}

extern "C" int fn_qgallery_search(const float* queries, int Q, const float* gallery, int G, const int8_t* qcodes, const float* qscale,
                                  const int8_t* gcodes, const float* gscale, const float* qrho, const float* qnorm, double rho_max,
                                  double norm_max, int E, int k, int shortlist, int metric, const int32_t* skip, int slab_rows, void* workspace,
                                  float* dist, int32_t* rows, int32_t* certified, unsigned long long* shortlist_keys, int32_t* range,
                                  void* stream) {
    int srows, slabs;
    if (int rc = check_qshape(Q, G, k, shortlist, slab_rows, &srows, &slabs)) return rc;
    if (int rc = check_walk_args("qgallery_search", queries, gallery, workspace, E, metric)) return rc;
    FN_REQUIRE(qcodes && qscale && gcodes && gscale && qrho && qnorm && dist && rows && certified, "qgallery_search: bad arguments");
    FN_REQUIRE(((uintptr_t)qcodes | (uintptr_t)gcodes) % 16 == 0, "qgallery_search: the code tables must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const int lists = q8_lists(Q);
    const size_t dyn = (size_t)F32_TILE * q8_cap(shortlist) * sizeof(u64);     // <= 44 KiB; with the static tiles below the 64 KiB default
    hipLaunchKernelGGL(qgallery_shortlist_kernel, dim3((unsigned)cdiv(Q, F32_TILE), (unsigned)slabs), dim3(256), dyn, st, (const signed char*)qcodes, qscale,
                       Q, (const signed char*)gcodes, gscale, G, q8_padded(E), shortlist, (const int*)skip, srows, (int)(lists == 4), (u64*)workspace);
    const u64* final_lists = (const u64*)workspace;
    int nlists = slabs * lists;
    if (const int groups = q8_groups(nlists)) {
        u64* merged = (u64*)workspace + (long)nlists * Q * shortlist;
        hipLaunchKernelGGL(qgallery_premerge_kernel, dim3((unsigned)Q, (unsigned)groups), dim3(64), 0, st, (const u64*)workspace, nlists, Q, shortlist, merged);
        final_lists = merged;
        nlists = groups;
    }
    hipLaunchKernelGGL(qgallery_rerank_kernel, dim3((unsigned)Q), dim3(64), 0, st, final_lists, nlists, Q, shortlist, k, metric, queries,
                       gallery, E, qrho, qnorm, rho_max, norm_max, dist, (int*)rows, (int*)certified, (u64*)shortlist_keys, (int*)range);
    return check_launch("qgallery_search");
}
