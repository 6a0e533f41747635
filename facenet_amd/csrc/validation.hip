// Face-to-face validation statistics on device: the class-pair confusion counts of
// facenet/statistics.py:111-138 (ConfidenceMatrix.__init__) with the class-balanced weights of
// SimilarityCalculator.evaluate (:92-103).  The reference walks all C(C+1)/2 class pairs in Python, calls
// pairwise_similarities (:22-57) for each and loops over 100 thresholds with np.count_nonzero: 700-1 550 s per
// validation of 26 489 embeddings in its own logs (models/20200724-231357/logs/report.txt:47,647).
//
// Here: one workgroup per class pair (i >= k).  Distances are computed in 32x32 image tiles from LDS-staged fp32
// embedding chunks (fp32 FMA: thresholds are compared exactly, so no low-precision MFMA here), every distance is
// binned once by upper_bound over the ascending thresholds into an LDS histogram, a prefix sum turns the histogram into
// "count(sims < threshold[n])" for all n at once, and the weighted tp/fn or fp/tn contributions go out as fp64 atomics.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

constexpr int VT = 32;        // images per tile side
constexpr int VE = 64;        // embedding chunk
constexpr int VMAXT = 256;    // thresholds

__global__ __launch_bounds__(256) void confidence_kernel(const float* __restrict__ emb, const int* __restrict__ cls_start, int C, int E,
                                                         const float* __restrict__ thr, int T, int metric, double* __restrict__ out,
                                                         int* __restrict__ range) {
    __shared__ float sA[VT][VE + 1], sB[VT][VE + 1];
    __shared__ float sThr[VMAXT];
    __shared__ int sHist[VMAXT + 1];
    const int tid = threadIdx.x;
    // class pair (i >= k) from the linear block id
    int i, k;
    tri_decode(blockIdx.x, i, k);
    const int a0 = cls_start[i], na = cls_start[i + 1] - a0;
    const int b0 = cls_start[k], nb = cls_start[k + 1] - b0;
    const long P = (i == k) ? (long)na * (na - 1) / 2 : (long)na * nb;
    if (P < 1) return;                                   // statistics.py:126-127
    for (int t = tid; t < T; t += 256) sThr[t] = thr[t];
    for (int t = tid; t <= T; t += 256) sHist[t] = 0;
    __syncthreads();
    const int ar = tid >> 3, bc = (tid & 7) * 4;         // thread -> row ar of the A tile, 4 consecutive rows of the B tile
    DotRange seen;
    for (int ta = 0; ta < na; ta += VT)
        for (int tb = 0; tb < nb; tb += VT) {
            if (i == k && tb + VT - 1 <= ta) continue;   // tile entirely on/below the diagonal: no pair with b > a
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int e0 = 0; e0 < E; e0 += VE) {
                __syncthreads();
                for (int t = tid; t < VT * VE; t += 256) {
                    const int r = t / VE, c = t - r * VE;
                    sA[r][c] = (ta + r < na && e0 + c < E) ? emb[(long)(a0 + ta + r) * E + e0 + c] : 0.f;
                    sB[r][c] = (tb + r < nb && e0 + c < E) ? emb[(long)(b0 + tb + r) * E + e0 + c] : 0.f;
                }
                __syncthreads();
#pragma unroll 8
                for (int c = 0; c < VE; ++c) {
                    const float av = sA[ar][c];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(av, sB[bc + j][c], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ia = ta + ar, ib = tb + bc + j;
                if (ia >= na || ib >= nb || (i == k && ib <= ia)) continue;   // strict upper triangle (:32-34)
                seen.add(acc[j]);
                atomicAdd(&sHist[threshold_bin(sThr, T, pair_distance(acc[j], metric))], 1);     // d < thr[n] counts
            }
        }
    seen.publish(range, tid & 63);
    __syncthreads();
    if (tid == 0) {                                       // prefix: sHist[n] = count(sims < thr[n])
        int run = 0;
        for (int n = 0; n < T; ++n) { run += sHist[n]; sHist[n] = run; }
    }
    __syncthreads();
    const double w = (double)P * ((i == k) ? (double)C : (double)C * (C - 1) * 0.5);   // :93-101
    for (int n = tid; n < T; n += 256) {
        const double c = (double)sHist[n];
        if (i == k) {
            atomicAdd(&out[0 * T + n], c / w);                    // tp
            atomicAdd(&out[3 * T + n], ((double)P - c) / w);      // fn
        } else {
            atomicAdd(&out[2 * T + n], c / w);                    // fp
            atomicAdd(&out[1 * T + n], ((double)P - c) / w);      // tn
        }
    }
}

// ---- the count tables of all F training parts of a k-fold validation in ONE pass over the pairs ------------------------
// A pair of rows held out in folds fa and fb belongs to the training part of every fold except fa and fb, so per class
// pair   hist(training part f) = total - touch_f   with touch_f the histogram of the pairs with fa == f or fb == f.
// Every pair adds 1 to touch[fa] and 1 to touch[fb] (fa != fb) or to touch[fa] and `same` (fa == fb): two LDS atomics
// spread over the folds' rows, and total = (sum_f touch_f + same) / 2 comes out in the epilogue.
//
// Dot products run on v_mfma_f32_16x16x4_f32 (pair_tiles.h's staging and mfma_chunk), which is bit for bit the ascending-k fmaf
// chain of confidence_kernel (a zero-padded k adds fma(0, 0, acc) = acc), so both kernels bin identical distances.
// Which pairs a workgroup evaluates is pair_tiles.h's class-pair walk (ClassPair, PairTile).  The kernel keeps the per-pair
// histograms, and the weighted fp64 tables in LDS until the workgroup has seen all its pairs: the global fp64 atomics happen once
// per workgroup, not once per class pair.
constexpr int OMAXF = 16;       // folds

__global__ __launch_bounds__(256) void confidence_folds_kernel(const float* __restrict__ emb, const int* __restrict__ cls_start,
                                                               const int* __restrict__ fold, const int* __restrict__ train_rows,
                                                               const int* __restrict__ train_classes, int C, int E, int F,
                                                               const float* __restrict__ thr, int T, int metric, double* __restrict__ out,
                                                               int* __restrict__ range, int diag_groups, int off_groups) {
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    __shared__ float sThr[VMAXT];
    __shared__ double sP[OMAXF], sW[OMAXF];
    const int HS = T + 1;
    int* sHist = reinterpret_cast<int*>(dyn);                                          // [F + 1][T + 1]; row F: `same`, then total
    double* sAcc = reinterpret_cast<double*>(dyn + ((((F + 1) * HS * 4) + 15) & ~15));  // [F][2][T]: count / w, (P - count) / w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < T; t += 256) sThr[t] = thr[t];
    for (int t = tid; t < F * 2 * T; t += 256) sAcc[t] = 0.0;
    const bool vec = (E & 3) == 0;
    DotRange seen;
    ClassPair p(C, diag_groups, off_groups);
    const bool diag = p.diag;
    while (p.next(cls_start)) {
        __syncthreads();                                  // the previous pair's epilogue has read the histograms
        for (int t = tid; t < (F + 1) * HS; t += 256) sHist[t] = 0;
        if (tid < F) {                                    // statistics.py:91-101,126-127 for the training part of fold tid
            const long ma = train_rows[(long)p.i * F + tid], mb = train_rows[(long)p.k * F + tid];
            const long P = diag ? ma * (ma - 1) / 2 : ma * mb;
            const int Cf = train_classes[tid];
            sP[tid] = (double)P;
            sW[tid] = (double)P * (diag ? (double)Cf : (double)Cf * (Cf - 1) * 0.5);
        }
        for (PairTile t; t.next(p);) {
            t.dots(p, sA, sB, emb, E, vec);
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (!t.live[ct]) continue;
                const int ib = t.ib(ct);
                const int fb = ib < p.nb ? fold[p.b0 + ib] : 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!t.ok(p, ct, r)) continue;
                    const int fa = fold[p.a0 + t.ia(r)];
                    const float s = t.acc[ct][r];
                    if (F >= 3 || fa == fb) seen.add(s);          // the pair is in at least one training part
                    const int l = threshold_bin(sThr, T, pair_distance(s, metric));
                    atomicAdd(&sHist[fa * HS + l], 1);
                    atomicAdd(&sHist[(fa == fb ? F : fb) * HS + l], 1);
                }
            }
        }
        __syncthreads();
        for (int l = tid; l <= T; l += 256) {             // total = (sum of the touch rows + same) / 2
            int s = sHist[F * HS + l];
            for (int f = 0; f < F; ++f) s += sHist[f * HS + l];
            sHist[F * HS + l] = s >> 1;
        }
        __syncthreads();
        for (int row = wave; row <= F; row += 4) {        // inclusive prefix over the bins: count(sims < thr[n])
            int carry = 0;
            for (int base = 0; base < T; base += 64) {
                const int l = base + lane;
                int v = l < T ? sHist[row * HS + l] : 0;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int u = __shfl_up(v, o);
                    if (lane >= o) v += u;
                }
                v += carry;
                if (l < T) sHist[row * HS + l] = v;
                carry = __shfl(v, 63);
            }
        }
        __syncthreads();
        for (int t = tid; t < F * T; t += 256) {          // entry t belongs to this thread for every pair: no race on sAcc
            const int f = t / T, n = t - f * T;
            const double P = sP[f];
            if (P < 1.0) continue;                        // statistics.py:126-127
            const double c = (double)(sHist[F * HS + n] - sHist[f * HS + n]);
            sAcc[(f * 2 + 0) * T + n] += c / sW[f];
            sAcc[(f * 2 + 1) * T + n] += (P - c) / sW[f];
        }
    }
    seen.publish(range, lane);
    __syncthreads();                                      // a workgroup whose pairs were all empty reads the zeros others wrote
    for (int t = tid; t < F * T; t += 256) {
        const int f = t / T, n = t - f * T;
        const double c = sAcc[(f * 2 + 0) * T + n], r = sAcc[(f * 2 + 1) * T + n];
        double* o = out + (long)f * 4 * T + n;
        if (c != 0.0) atomicAdd(o + (diag ? 0 : 2) * T, c);      // tp | fp
        if (r != 0.0) atomicAdd(o + (diag ? 3 : 1) * T, r);      // fn | tn
    }
}

}  // namespace fn
using namespace fn;

extern "C" int fn_confidence_counts_folds(const float* emb, const int32_t* cls_start, const int32_t* fold, const int32_t* train_rows,
                                          const int32_t* train_classes, int C, int E, int F, const float* thresholds, int T, int metric,
                                          double* out, int32_t* range, void* stream) {
    FN_REQUIRE(emb && cls_start && fold && train_rows && train_classes && thresholds && out && C > 0 && E > 0 && T > 0 && T <= VMAXT &&
                   F >= 2 && F <= OMAXF,
               "confidence_counts_folds: bad arguments (T <= 256, 2 <= folds <= 16)");
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);   // statistics.py:258-260
    int diag_groups, off_groups;
    FN_REQUIRE(class_pair_groups(C, &diag_groups, &off_groups), "confidence_counts_folds: too many classes");
    hipStream_t st = (hipStream_t)stream;
    fill_words(out, 0u, 0u, 2 * F * 4 * T, st);
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const size_t dyn = (size_t)((((F + 1) * (T + 1) * 4) + 15) & ~15) + (size_t)F * 2 * T * sizeof(double);
    if (dyn > 40 * 1024) {   // beyond the default 64 KiB per workgroup together with the static tiles
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(confidence_folds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        FN_REQUIRE(e == hipSuccess, "confidence_counts_folds: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(confidence_folds_kernel, dim3((unsigned)(diag_groups + off_groups)), dim3(256), dyn, st, emb, cls_start, fold, train_rows,
                       train_classes, C, E, F, thresholds, T, metric, out, (int*)range, diag_groups, off_groups);
    return check_launch("confidence_counts_folds");
}

extern "C" int fn_confidence_counts(const float* emb, const int32_t* cls_start, int C, int E, const float* thresholds, int T, int metric,
                                    double* out, int32_t* range, void* stream) {
    FN_REQUIRE(emb && cls_start && thresholds && out && C > 0 && E > 0 && T > 0 && T <= VMAXT, "confidence_counts: bad arguments (T <= 256)");
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);   // statistics.py:258-260
    hipStream_t st = (hipStream_t)stream;
    fill_words(out, 0u, 0u, 2 * 4 * T, st);                              // 4*T doubles; kernel nodes, see fill_words
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const long pairs = (long)C * (C + 1) / 2;
    FN_REQUIRE(pairs < (1L << 31), "confidence_counts: too many classes");
    hipLaunchKernelGGL(confidence_kernel, dim3((unsigned)pairs), dim3(256), 0, st, emb, cls_start, C, E, thresholds, T, metric, out, (int*)range);
    return check_launch("confidence_counts");
}
