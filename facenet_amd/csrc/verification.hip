// The exact verification curve: windowed histograms of the fp32 keys of ALL pairs, genuine and impostor.
//
// A distance can be recomputed to the same bits in every pass (pair_tiles.h), so the k-th smallest impostor distance is found by
// radix selection over recomputed distances: the host narrows a key interval per target from the counts of one pass and asks for
// the next, finer windows.  The [n, n] matrix is never written and nothing is sorted.
//
// Which pairs a workgroup evaluates is pair_tiles.h's class-pair walk (ClassPair, PairTile), as in confidence_folds_kernel: a
// workgroup's population is uniform, genuine or impostor.  Counters are uint32 in LDS, R x 1024 of them (32 KB at most, one
// population), kept over all the workgroup's pairs and flushed with 64-bit integer atomics, non-zero bins only; "below the window"
// and the total are counted in registers.
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
    const int tid = threadIdx.x, lane = tid & 63;
    for (int t = tid; t < R * KB; t += 256) sCnt[t] = 0;
    ClassPair p(C, diag_groups, off_groups);
    const int pop = p.diag ? 0 : 1;
    unsigned below[KMAXR], total = 0;
#pragma unroll
    for (int r = 0; r < KMAXR; ++r) below[r] = 0;
    unsigned long pending = 0;                            // an upper bound of what any counter holds: workgroup-uniform
    DotRange seen;
    while (p.next(cls_start))
        for (PairTile t; t.next(p);) {
            // A uint32 counter could wrap.  No test reaches this (it takes 2^32 pairs in one workgroup); it is safe by reading:
            // `pending` is workgroup-uniform and key_flush has a barrier on both sides.
            if (pending + F32_TILE * F32_TILE > 0xffffffffUL) {
                key_flush(sCnt, below, total, R, pop, out);
                pending = 0;
            }
            pending += F32_TILE * F32_TILE;
            t.dots(p, sA, sB, emb, E, true);              // fn_pair_key_histogram requires E % 4 == 0
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (!t.live[ct]) continue;
                unsigned key[4];
                bool ok[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ok[r] = t.ok(p, ct, r);
                    const float s = t.acc[ct][r];
                    if (ok[r]) {
                        seen.add(s);
                        ++total;
                    }
                    key[r] = __float_as_uint(pair_distance(s, metric));
                }
#pragma unroll
                for (int q = 0; q < KMAXR; ++q) {
                    if (q >= R) break;
                    unsigned bin[4];                      // >= KB: no bin of this window
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
    int diag_groups, off_groups;
    FN_REQUIRE(class_pair_groups(C, &diag_groups, &off_groups), "%s: too many classes (C %d, at most 65535)", what, C);
    FN_REQUIRE(((uintptr_t)emb | (uintptr_t)out) % 16 == 0, "%s: emb and out must be 16-byte aligned", what);
    KeyWindows w = {};
    for (int r = 0; r < R; ++r) {
        FN_REQUIRE(shift[r] >= 0 && shift[r] <= 22, "%s: a window's shift must be in [0, 22] (window %d: shift %d)", what, r, shift[r]);
        w.lo[r] = lo[r];
        w.shift[r] = shift[r];
    }
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    const size_t dyn = (size_t)R * KB * sizeof(unsigned);
    hipLaunchKernelGGL(pair_key_histogram_kernel, dim3((unsigned)(diag_groups + off_groups)), dim3(256), dyn, st, emb, cls_start, C, E, metric, w,
                       R, out, (int*)range, diag_groups, off_groups);
    return check_launch(what);
}
