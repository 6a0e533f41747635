// The exact verification curve: windowed histograms of the fp32 keys of ALL pairs, genuine and impostor.
//
// A distance can be recomputed to the same bits in every pass (pair_tiles.h), so the k-th smallest impostor distance is found by
// radix selection over recomputed distances: the host narrows a key interval per target from the counts of one pass and asks for
// the next, finer windows.  The [n, n] matrix is never written and nothing is sorted.
//
// The decomposition is confidence_folds_kernel's: a workgroup walks class pairs with a stride, diagonal pairs (genuine: the strict
// upper triangle) and off-diagonal pairs (impostor) in separate workgroups, so a workgroup's population is uniform; each pair is
// covered with 64x64 super-tiles, wave w rows 16w..16w+15 against four 16x16 column tiles.  Counters are uint32 in LDS, R x 1024 of
// them (32 KB at most, one population), kept over all the workgroup's pairs and flushed with 64-bit integer atomics, non-zero bins
// only; "below the window" and the total are counted in registers.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

constexpr int KB = 1024;          // bins per window
constexpr int KMAXR = 8;          // windows
constexpr int KSLOT = KB + 2;     // out words per (window, population): bins, below, total

struct KeyWindows {
    unsigned lo[KMAXR];
    int shift[KMAXR];
};

__device__ __forceinline__ unsigned wave_count(unsigned v) {      // the wave's sum; it fits: no counter exceeds the flush bound
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

// Everything a workgroup has counted goes out; the LDS counters and the register counters are zero afterwards.
__device__ __forceinline__ void key_flush(unsigned* sCnt, unsigned (&below)[KMAXR], unsigned& total, int R, int pop,
                                          unsigned long long* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();
    for (int t = tid; t < R * KB; t += 256) {
        const unsigned v = sCnt[t];
        if (v) {
            atomicAdd(&out[(long)((t >> 10) * 2 + pop) * KSLOT + (t & (KB - 1))], (unsigned long long)v);
            sCnt[t] = 0;
        }
    }
    const unsigned all = wave_count(total);
    total = 0;
#pragma unroll
    for (int r = 0; r < KMAXR; ++r) {
        if (r >= R) break;
        const unsigned under = wave_count(below[r]);
        below[r] = 0;
        if (lane != 0) continue;
        unsigned long long* slot = out + (long)(r * 2 + pop) * KSLOT + KB;
        if (under) atomicAdd(slot, (unsigned long long)under);
        if (all) atomicAdd(slot + 1, (unsigned long long)all);
    }
    __syncthreads();
}

// One LDS atomic per pair and window that holds it.  Merging a lane's four values of one accumulator when they share a bin was
// measured and is not worth its compares.
__global__ __launch_bounds__(256) void pair_key_histogram_kernel(const float* __restrict__ emb, const int* __restrict__ cls_start, int C,
                                                                 int E, int metric, KeyWindows w, int R,
                                                                 unsigned long long* __restrict__ out, int* __restrict__ range,
                                                                 int diag_groups, int off_groups) {
    extern __shared__ __align__(16) unsigned sCnt[];                                   // [R][KB]
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < R * KB; t += 256) sCnt[t] = 0;
    const bool diag = (int)blockIdx.x < diag_groups;
    const int pop = diag ? 0 : 1;
    const long npairs = diag ? (long)C : (long)C * (C - 1) / 2;
    const long stride = diag ? diag_groups : off_groups;
    const int lr = lane & 15, lg = lane >> 4;
    unsigned below[KMAXR], total = 0;
#pragma unroll
    for (int r = 0; r < KMAXR; ++r) below[r] = 0;
    unsigned long pending = 0;                            // an upper bound of what any counter holds: workgroup-uniform
    DotRange seen;
    for (long b = diag ? (long)blockIdx.x : (long)blockIdx.x - diag_groups; b < npairs; b += stride) {
        int i, k;
        if (diag) {
            i = k = (int)b;
        } else {                                          // b = j (j + 1) / 2 + k with k <= j, i = j + 1 > k
            tri_decode(b, i, k);
            i += 1;
        }
        const int a0 = cls_start[i], na = cls_start[i + 1] - a0;
        const int b0 = cls_start[k], nb = cls_start[k + 1] - b0;
        if (diag && na < 2) continue;                     // no pair at all
        for (int ta = 0; ta < na; ta += F32_TILE)
            for (int tb = 0; tb < nb; tb += F32_TILE) {
                if (diag && tb + F32_TILE - 1 <= ta) continue;  // super-tile entirely on/below the diagonal
                // A uint32 counter could wrap.  No test reaches this (it takes 2^32 pairs in one workgroup); it is safe by reading:
                // `pending` is workgroup-uniform and key_flush has a barrier on both sides.
                if (pending + F32_TILE * F32_TILE > 0xffffffffUL) {
                    key_flush(sCnt, below, total, R, pop, out);
                    pending = 0;
                }
                pending += F32_TILE * F32_TILE;
                const int r0 = ta + wave * 16;            // this wave's 16 rows
                bool live[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int c0 = tb + ct * 16;
                    live[ct] = r0 < na && c0 < nb && !(diag && c0 + 15 <= r0);
                }
                f32x4 acc[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int e0 = 0; e0 < E; e0 += F32_CHUNK) {
                    __syncthreads();
                    stage_rows(sA, emb + (long)(a0 + ta) * E, na - ta, E, e0, true, tid);
                    stage_rows(sB, emb + (long)(b0 + tb) * E, nb - tb, E, e0, true, tid);
                    __syncthreads();
                    mfma_chunk(sA, sB, wave * 16, acc, live);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (!live[ct]) continue;
                    const int ib = tb + ct * 16 + lr;     // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
                    unsigned key[4];
                    bool ok[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ia = r0 + lg * 4 + r;
                        ok[r] = ia < na && ib < nb && !(diag && ib <= ia);      // strict upper triangle
                        const float s = acc[ct][r];
                        if (ok[r]) {
                            seen.add(s);
                            ++total;
                        }
                        key[r] = __float_as_uint(pair_distance(s, metric));
                    }
#pragma unroll
                    for (int q = 0; q < KMAXR; ++q) {
                        if (q >= R) break;
                        unsigned bin[4];                  // >= KB: no bin of this window
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool under = key[r] < w.lo[q];
                            bin[r] = (ok[r] && !under) ? (key[r] - w.lo[q]) >> w.shift[q] : 0xffffffffu;
                            if (ok[r] && under) ++below[q];
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (bin[r] < KB) atomicAdd(&sCnt[q * KB + bin[r]], 1u);
                    }
                }
            }
    }
    key_flush(sCnt, below, total, R, pop, out);
    seen.publish(range, lane);
}

}  // namespace fn
using namespace fn;

extern "C" int fn_pair_key_histogram(const float* emb, const int32_t* cls_start, int C, int E, int metric, const uint32_t* lo,
                                     const int32_t* shift, int R, unsigned long long* out, int32_t* range, void* stream) {
    const char* what = "pair_key_histogram";
    FN_REQUIRE(R >= 1 && R <= KMAXR, "%s: the number of windows must be in [1, %d] (R %d)", what, KMAXR, R);
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "%s: the embedding length must be a multiple of 4 in [4, 512] (E %d)", what, E);
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);   // statistics.py:55
    FN_REQUIRE(emb && cls_start && lo && shift && out && C >= 1, "%s: bad arguments", what);
    FN_REQUIRE(C < 65536, "%s: too many classes (C %d, at most 65535)", what, C);
    FN_REQUIRE(((uintptr_t)emb | (uintptr_t)out) % 16 == 0, "%s: emb and out must be 16-byte aligned", what);
    KeyWindows w = {};
    for (int r = 0; r < R; ++r) {
        FN_REQUIRE(shift[r] >= 0 && shift[r] <= 22, "%s: a window's shift must be in [0, 22] (window %d: shift %d)", what, r, shift[r]);
        w.lo[r] = lo[r];
        w.shift[r] = shift[r];
    }
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const long off_pairs = (long)C * (C - 1) / 2;
    const int diag_groups = C < 256 ? C : 256;
    const int off_groups = (int)(off_pairs < 2048 ? off_pairs : 2048);
    const size_t dyn = (size_t)R * KB * sizeof(unsigned);
    hipLaunchKernelGGL(pair_key_histogram_kernel, dim3((unsigned)(diag_groups + off_groups)), dim3(256), dyn, st, emb, cls_start, C, E, metric, w,
                       R, out, (int*)range, diag_groups, off_groups);
    return check_launch(what);
}
