// Face-to-face pair classifiers: facenet/faceclass.py:8-118 (FaceToFaceDistanceClassifier,
// FaceToFaceNormalizedEmbeddingsClassifier), the class-weighted binary cross-entropy over every pair of a batch of
// apps/train_classifier.py:60-84 with its gradient, and the per-class-pair prediction counts behind ConfusionMatrix (:17-57).
//
// Every entry point computes its dot products with the same 64 x 64 tile routine (tile_dots: one fmaf chain per pair over
// e = 0 .. E-1, operands staged in LDS) and turns them into a distance with the same f2f_pair_distance.  The distance of a pair
// therefore has the same bits in fn_f2f_distance, fn_f2f_pair_counts and the training loss, and the counts equal
// (fn_f2f_distance < threshold).sum() exactly.  fp32 throughout: the decision d < threshold is taken on fp32 values.
// DESIGN.md section 12.
#include "pair_tiles.h"      // tri_decode
#include "../../include/facenet_hip.h"

namespace fn {

enum { F2F_DISTANCE = 0, F2F_NORMALIZED = 1 };
constexpr int FT = 64;        // rows per tile side (16 x 16 threads, 4 x 4 pairs each)
constexpr int FK = 16;        // embedding elements per LDS stage
constexpr int ROW_ABSENT = -1, ROW_INVALID = -2;

// d(x, y) of faceclass.py:48-77 / :102-110 from the dot product and the two norms.  r2 receives (2 (nx - ny) / (nx + ny))^2, the
// factor of theta (0 in the normalized mode).  Every rounding is spelled out: the compiler may not contract differently at
// different call sites.  Symmetric in (x, y) bit for bit.
__device__ __forceinline__ float f2f_pair_distance(float dot, float nx, float ny, int mode, float theta, float& r2) {
#pragma clang fp contract(off)
    if (mode == F2F_NORMALIZED) {
        r2 = 0.f;
        return 2.f * (1.f - dot);
    }
    const float nn = nx * ny;
    const float c = dot / nn;
    const float r = 2.f * (nx - ny) / (nx + ny);
    r2 = r * r;
    const float tr = theta * r2;
    return 2.f * (1.f - c) + tr;
}

struct TileLds {
    float a[FK][FT + 4];      // [e][row]: a thread reads its 4 rows as one 16-byte word
    float b[FK][FT + 4];
    int rowA[FT], rowB[FT];   // table row of each tile row, ROW_ABSENT past the end, ROW_INVALID for an out-of-range index
};

__device__ __forceinline__ f32x4 load_row4(const float* __restrict__ tab, int g, int E, int e) {
    if (g >= 0 && e < E) return *reinterpret_cast<const f32x4*>(tab + (long)g * E + e);
    const float v = (g == ROW_INVALID) ? __builtin_nanf("") : 0.f;
    return f32x4{v, v, v, v};
}

// acc[i][j] = dot(A row 4ty+i, B row 4tx+j) as ONE fmaf chain over e = 0 .. E-1 (zero padding after E adds exact zeros).  The
// caller has filled L.rowA / L.rowB and synchronised.
__device__ __forceinline__ void tile_dots(TileLds& L, const float* __restrict__ tabA, const float* __restrict__ tabB, int E,
                                          float (&acc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int lr = tid >> 2, lc = (tid & 3) * 4;                  // loader: row lr, elements lc .. lc+3 of the stage
    const int ga = L.rowA[lr], gb = L.rowB[lr];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int e0 = 0; e0 < E; e0 += FK) {
        const f32x4 va = load_row4(tabA, ga, E, e0 + lc), vb = load_row4(tabB, gb, E, e0 + lc);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L.a[lc + j][lr] = va[j];
            L.b[lc + j][lr] = vb[j];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < FK; ++e) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&L.a[e][ty * 4]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&L.b[e][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
    }
    __syncthreads();                                              // L may be refilled by the caller after this
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- norms -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f2f_row_norms_kernel(const float* __restrict__ x, int n, int E, float* __restrict__ norms) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double s = 0.0;
    for (int e = lane; e < E; e += 64) {
        const double v = (double)x[(long)row * E + e];
        s += v * v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) norms[row] = (float)sqrt(s);
}


// Loads the table rows (and their norms) of tile t of a row-index list (rows != nullptr: rows[l], checked against n_tab) or of a
// contiguous range starting at table row `first` with `count` rows.  Called by threads 0 .. FT-1.
__device__ __forceinline__ void tile_row(int t, int r, const int* __restrict__ rows, int first, int count, int n_tab,
                                         const float* __restrict__ norms, int& g, float& nv) {
    const int l = t * FT + r;
    g = ROW_ABSENT;
    if (l < count) {
        g = rows ? rows[l] : first + l;
        if (g < 0 || g >= n_tab) g = ROW_INVALID;
    }
    nv = (g >= 0 && norms) ? norms[g] : (g == ROW_INVALID ? __builtin_nanf("") : 0.f);
}

// ---- training: loss and parameter gradients over the pairs a < b of one batch ----------------------------------------------
// One workgroup per tile pair (ta <= tb) of the upper triangle.  Its sums, in fp64, go to ws[tile][4] =
// {sum l, sum g (threshold - d), sum g, sum g r2} with g = (1 - z) - (1 + (q - 1) z) sigmoid(-s), not yet divided by #pairs.
__global__ __launch_bounds__(256) void f2f_pair_loss_kernel(const float* __restrict__ tab, const float* __restrict__ norms, int n_tab,
                                                            const int* __restrict__ rows, int B, int K, int E, int mode, float q,
                                                            const float* __restrict__ params, double* __restrict__ ws) {
    __shared__ TileLds L;
    __shared__ float sNA[FT], sNB[FT];
    __shared__ double sRed[4][4];
    int tb, ta;
    tri_decode(blockIdx.x, tb, ta);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < FT) tile_row(ta, tid, rows, 0, B, n_tab, norms, L.rowA[tid], sNA[tid]);
    else if (tid < 2 * FT) tile_row(tb, tid - FT, rows, 0, B, n_tab, norms, L.rowB[tid - FT], sNB[tid - FT]);
    __syncthreads();
    float acc[4][4];
    tile_dots(L, tab, tab, E, acc);
    const float alpha = params[0], thr = params[1], theta = params[2];
    float sl = 0.f, sa = 0.f, st = 0.f, sr = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = ta * FT + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = tb * FT + tx * 4 + j;
            if (a >= b || b >= B) continue;                       // pairs a < b (train_classifier.py:62-63)
            const bool z = (a / K) == (b / K);                    // :66-72
            const float w = z ? q : 1.f;                          // 1 + (q - 1) z
            float r2;
            const float d = f2f_pair_distance(acc[i][j], sNA[ty * 4 + i], sNB[tx * 4 + j], mode, theta, r2);
            const float u = thr - d;
            const float s = alpha * u;                            // faceclass.py:23-27
            // tf.nn.weighted_cross_entropy_with_logits: (1 - z) s + (1 + (q - 1) z) (log1p(exp(-|s|)) + max(-s, 0))
            const float l = (z ? 0.f : s) + w * (log1pf(expf(-fabsf(s))) + fmaxf(-s, 0.f));
            const float g = (z ? 0.f : 1.f) - w / (1.f + expf(s));
            sl += l;
            sa += g * u;
            st += g;
            sr += g * r2;
        }
    }
    double v[4] = {wave_sum_f64((double)sl), wave_sum_f64((double)sa), wave_sum_f64((double)st), wave_sum_f64((double)sr)};
    if ((tid & 63) == 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) sRed[tid >> 6][c] = v[c];
    __syncthreads();
    if (tid < 4) ws[(long)blockIdx.x * 4 + tid] = ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
}

// Sums the tile partials in tile order (256 consecutive runs, then the runs in order), in fp64, and writes
// loss[0] = mean l, grad = {d/dalpha, d/dthreshold, d/dtheta, 0} (train_classifier.py:83-84 differentiated).
__global__ __launch_bounds__(256) void f2f_pair_loss_finish_kernel(const double* __restrict__ ws, int tiles, double inv_pairs, int mode,
                                                                   const float* __restrict__ params, float* __restrict__ loss,
                                                                   float* __restrict__ grad) {
    __shared__ double sRun[256][4];
    const int tid = threadIdx.x;
    const int per = (tiles + 255) / 256, t0 = tid * per, t1 = min(tiles, t0 + per);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = t0; t < t1; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += ws[(long)t * 4 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) sRun[tid][c] = s[c];
    __syncthreads();
    if (tid < 4) {
        double tot = 0.0;
        for (int r = 0; r < 256; ++r) tot += sRun[r][tid];
        sRun[0][tid] = tot;                                       // run 0 is read by thread tid only from here on
    }
    __syncthreads();
    if (tid == 0) {
        const double alpha = (double)params[0];
        loss[0] = (float)(sRun[0][0] * inv_pairs);
        grad[0] = (float)(sRun[0][1] * inv_pairs);                // sum g (threshold - d)
        grad[1] = (float)(alpha * sRun[0][2] * inv_pairs);        // sum g alpha
        grad[2] = mode == F2F_DISTANCE ? (float)(-alpha * sRun[0][3] * inv_pairs) : 0.f;   // -sum g alpha r2
        grad[3] = 0.f;
    }
}

// ---- ConfusionMatrix counts: one workgroup per class pair (i >= k), #(d < threshold) over the whole n_i x n_k rectangle ----
__global__ __launch_bounds__(256) void f2f_pair_counts_kernel(const float* __restrict__ tab, const float* __restrict__ norms,
                                                              const int* __restrict__ cls_start, int E, int mode,
                                                              const float* __restrict__ params, long long* __restrict__ counts) {
    __shared__ TileLds L;
    __shared__ float sNA[FT], sNB[FT];
    __shared__ long long sRed[4];
    int ci, ck;
    tri_decode(blockIdx.x, ci, ck);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = cls_start[ci], na = cls_start[ci + 1] - a0;
    const int b0 = cls_start[ck], nb = cls_start[ck + 1] - b0;
    const int n_tab = max(a0 + na, b0 + nb);
    const float thr = params[1], theta = params[2];
    long long cnt = 0;
    for (int ta = 0; ta * FT < na; ++ta)
        for (int tb = 0; tb * FT < nb; ++tb) {
            if (tid < FT) tile_row(ta, tid, nullptr, a0, na, n_tab, norms, L.rowA[tid], sNA[tid]);
            else if (tid < 2 * FT) tile_row(tb, tid - FT, nullptr, b0, nb, n_tab, norms, L.rowB[tid - FT], sNB[tid - FT]);
            __syncthreads();
            float acc[4][4];
            tile_dots(L, tab, tab, E, acc);
            int c = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int a = ta * FT + ty * 4 + i, b = tb * FT + tx * 4 + j;
                    if (a >= na || b >= nb) continue;
                    float r2;
                    const float d = f2f_pair_distance(acc[i][j], sNA[ty * 4 + i], sNB[tx * 4 + j], mode, theta, r2);
                    c += d < thr ? 1 : 0;                         // faceclass.py:80 / :112, strict
                }
            cnt += c;
            __syncthreads();                                      // sNA / sNB are rewritten by the next tile
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) sRed[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = sRed[0] + sRed[1] + sRed[2] + sRed[3];
}

// ---- distance / logits matrix [N, M] ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f2f_distance_kernel(const float* __restrict__ x, const float* __restrict__ nx, int N,
                                                           const float* __restrict__ y, const float* __restrict__ ny, int M, int E,
                                                           int mode, const float* __restrict__ params, int logits, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ TileLds L;
    __shared__ float sNA[FT], sNB[FT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (tid < FT) tile_row(ta, tid, nullptr, 0, N, N, nx, L.rowA[tid], sNA[tid]);
    else if (tid < 2 * FT) tile_row(tb, tid - FT, nullptr, 0, M, M, ny, L.rowB[tid - FT], sNB[tid - FT]);
    __syncthreads();
    float acc[4][4];
    tile_dots(L, x, y, E, acc);
    const float alpha = params[0], thr = params[1], theta = params[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = ta * FT + ty * 4 + i;
        if (a >= N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = tb * FT + tx * 4 + j;
            if (b >= M) continue;
            float r2;
            const float d = f2f_pair_distance(acc[i][j], sNA[ty * 4 + i], sNB[tx * 4 + j], mode, theta, r2);
            const float u = thr - d;
            out[(long)a * M + b] = logits ? alpha * u : d;        // faceclass.py:23-27
        }
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace fn
using namespace fn;

extern "C" int fn_f2f_row_norms(const float* x, int n, int E, float* norms, void* stream) {
    FN_REQUIRE(x && norms && n > 0 && E > 0, "f2f_row_norms: bad arguments");
    hipLaunchKernelGGL(f2f_row_norms_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, x, n, E, norms);
    return check_launch("f2f_row_norms");
}

extern "C" int fn_f2f_pair_loss_fwd_bwd(const float* table, const float* norms, int n_rows, const int32_t* rows, int P, int K, int E, int mode,
                                        float q, const float* params, float* loss, float* grad, double* ws, long ws_len, void* stream) {
    FN_REQUIRE(mode == F2F_DISTANCE || mode == F2F_NORMALIZED, "f2f_pair_loss: mode %d is neither 0 (distance) nor 1 (normalized)", mode);
    FN_REQUIRE(table && rows && params && loss && grad && ws && n_rows > 0 && (norms || mode == F2F_NORMALIZED),
               "f2f_pair_loss: null argument (norms may be NULL in the normalized mode only)");
    FN_REQUIRE(P >= 1 && K >= 2 && (long)P * K <= (1L << 20), "f2f_pair_loss: P %d, K %d (K >= 2, P K <= 2^20)", P, K);
    FN_REQUIRE(E > 0 && E % 4 == 0 && aligned16(table), "f2f_pair_loss: E %d must be a multiple of 4 with 16-byte aligned rows", E);
    const int B = P * K, nt = cdiv(B, FT);
    const long tiles = (long)nt * (nt + 1) / 2;
    FN_REQUIRE(ws_len >= 4 * tiles, "f2f_pair_loss: workspace of %ld doubles, %ld needed", ws_len, 4 * tiles);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(f2f_pair_loss_kernel, dim3((unsigned)tiles), dim3(256), 0, st, table, norms, n_rows, rows, B, K, E, mode, q, params, ws);
    const double pairs = (double)B * (double)(B - 1) * 0.5;
    hipLaunchKernelGGL(f2f_pair_loss_finish_kernel, dim3(1), dim3(256), 0, st, ws, (int)tiles, 1.0 / pairs, mode, params, loss, grad);
    return check_launch("f2f_pair_loss");
}

extern "C" int fn_f2f_pair_counts(const float* table, const float* norms, const int32_t* cls_start, int C, int E, int mode, const float* params,
                                  int64_t* counts, void* stream) {
    FN_REQUIRE(mode == F2F_DISTANCE || mode == F2F_NORMALIZED, "f2f_pair_counts: mode %d is neither 0 (distance) nor 1 (normalized)", mode);
    FN_REQUIRE(table && cls_start && params && counts && C > 0 && (norms || mode == F2F_NORMALIZED),
               "f2f_pair_counts: null argument or C < 1 (norms may be NULL in the normalized mode only)");
    FN_REQUIRE(E > 0 && E % 4 == 0 && aligned16(table), "f2f_pair_counts: E %d must be a multiple of 4 with 16-byte aligned rows", E);
    const long pairs = (long)C * (C + 1) / 2;
    FN_REQUIRE(pairs < (1L << 31), "f2f_pair_counts: too many classes (%d)", C);
    hipLaunchKernelGGL(f2f_pair_counts_kernel, dim3((unsigned)pairs), dim3(256), 0, (hipStream_t)stream, table, norms, cls_start, E, mode, params,
                       (long long*)counts);
    return check_launch("f2f_pair_counts");
}

extern "C" int fn_f2f_distance(const float* x, const float* nx, int N, const float* y, const float* ny, int M, int E, int mode, const float* params,
                               int logits, float* out, void* stream) {
    FN_REQUIRE(mode == F2F_DISTANCE || mode == F2F_NORMALIZED, "f2f_distance: mode %d is neither 0 (distance) nor 1 (normalized)", mode);
    FN_REQUIRE(x && y && params && out && N > 0 && M > 0 && ((nx && ny) || mode == F2F_NORMALIZED),
               "f2f_distance: null argument or empty input (norms may be NULL in the normalized mode only)");
    FN_REQUIRE(E > 0 && E % 4 == 0 && aligned16(x) && aligned16(y), "f2f_distance: E %d must be a multiple of 4 with 16-byte aligned rows", E);
    FN_REQUIRE(cdiv(N, FT) <= 65535, "f2f_distance: N %d too large", N);
    hipLaunchKernelGGL(f2f_distance_kernel, dim3(cdiv(M, FT), cdiv(N, FT)), dim3(256), 0, (hipStream_t)stream, x, nx, N, y, ny, M, E, mode, params,
                       logits, out);
    return check_launch("f2f_distance");
}
