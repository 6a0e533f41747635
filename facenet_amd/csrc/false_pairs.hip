// False examples: WHICH pairs a threshold gets wrong, where validation.hip and verification.hip count them.
// The third consumer of pair_tiles.h's class-pair walk: per class the farthest pairs with d > threshold (false negatives), per pair
// of classes the nearest pairs with d < threshold (false positives), picked greedily as the reference's FalseExamples does
// (facenet/statistics.py:334-421): a picked false negative takes both its rows out of its class's further picks, a picked false
// positive its row and its column.  d is pair_distance of the chain dot product: the bits every other consumer compares.
//
// A class pair is walked in rounds.  A round is one walk of the pair's super-tiles; every lane keeps the best 64-bit key over the
// pairs that pass the threshold and whose row and column are not excluded, and counts them.  The key is one that a single `max`
// orders: the distance bits above (complemented for the minimum; d >= +0, so bit patterns order as values do), the complemented
// row-major position of the reference's matrix below (ties go to the smaller position).  The workgroup's best pair is the round's
// pick; it joins the excluded lists (LDS, workgroup-uniform) and the next round walks again.  A round that met at most one passing
// pair ends the class pair: nothing would be left.  So a class pair costs 1 + picks walks at most, and one walk when it has at most
// one offender.  Every pair is evaluated in round 0, which feeds `range`.
#include "pair_tiles.h"
#include "../../include/facenet_hip.h"

namespace fn {

constexpr int FP_PICKS = 64;      // most picks per class (max_fneg) or per pair of classes (max_fpos)

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), o), lo = (unsigned)__shfl_xor((int)(v & 0xffffffffu), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_add_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(256) void false_pairs_kernel(const float* __restrict__ emb, const int* __restrict__ cls_start, int C, int E,
                                                          int metric, float threshold, int max_fneg, int max_fpos,
                                                          int4* __restrict__ records, long long capacity,
                                                          unsigned long long* __restrict__ count, int* __restrict__ range, int diag_groups,
                                                          int off_groups) {
    __shared__ __align__(16) float sA[F32_TILE][F32_LD], sB[F32_TILE][F32_LD];
    __shared__ int sEx[2 * FP_PICKS];                  // excluded rows within the class(es): see exA / exB
    __shared__ unsigned long long sKey[4];
    __shared__ unsigned sMet[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ClassPair p(C, diag_groups, off_groups);
    const int limit = p.diag ? max_fneg : max_fpos;
    // The walk's a rows (ia) are the HIGHER class, its b rows (ib) the lower one.  Off the diagonal the reference's row is ib and
    // its column ia: one entry per pick in each list.  On the diagonal both rows of a pick leave both lists: one list of 2 picks.
    const int* exA = sEx;
    const int* exB = p.diag ? sEx : sEx + FP_PICKS;
    DotRange seen;
    while (p.next(cls_start)) {
        int picks = 0;
        for (;;) {                                     // a round; everything that decides its end is workgroup-uniform
            const int nex = p.diag ? 2 * picks : picks;
            unsigned long long best = 0;               // no key is 0: a position is below 2^32 - 1 and a distance is no NaN
            unsigned met = 0;                          // passing pairs that are not excluded, saturated at 2
            for (PairTile t; t.next(p);) {
                t.dots(p, sA, sB, emb, E, true);       // fn_false_pairs requires E % 4 == 0
                unsigned rowex = 0, colex = 0;         // per tile, not per element: this lane's 4 rows and its column of each tile
                for (int j = 0; j < nex; ++j) {
                    const int ea = exA[j], eb = exB[j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) rowex |= (unsigned)(t.ia(r) == ea) << r;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) colex |= (unsigned)(t.ib(ct) == eb) << ct;
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (!t.live[ct]) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!t.ok(p, ct, r)) continue;
                        const float s = t.acc[ct][r];
                        if (picks == 0) seen.add(s);
                        const float d = pair_distance(s, metric);
                        const bool wrong = p.diag ? d > threshold : d < threshold;      // strict fp32, as every consumer decides
                        if (!wrong || (((rowex >> r) | (colex >> ct)) & 1u)) continue;
                        const unsigned bits = __float_as_uint(d);
                        const unsigned pos = p.diag ? ((unsigned)t.ia(r) << 16) | (unsigned)t.ib(ct)
                                                    : ((unsigned)t.ib(ct) << 16) | (unsigned)t.ia(r);
                        const unsigned long long key = ((unsigned long long)(p.diag ? bits : ~bits) << 32) | (unsigned)~pos;
                        best = key > best ? key : best;
                        met = met < 2 ? met + 1 : 2;
                    }
                }
            }
            best = wave_max_u64(best);
            met = wave_add_u32(met);
            __syncthreads();                           // the previous round's sKey / sMet have been read
            if (lane == 0) sKey[wave] = best, sMet[wave] = met;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 4; ++w) best = sKey[w] > best ? sKey[w] : best;
            met = sMet[0] + sMet[1] + sMet[2] + sMet[3];
            if (met == 0 || limit == 0) break;
            const unsigned hi = (unsigned)(best >> 32), pos = ~(unsigned)(best & 0xffffffffu);
            const int first = (int)(pos >> 16), second = (int)(pos & 0xffffu);          // the reference's (row, column)
            if (tid == 0) {
                const unsigned long long slot = atomicAdd(&count[p.diag ? 0 : 1], 1ull);
                // false negatives fill `records` from the front, false positives from the back; beyond capacity nothing is written
                if (slot < (unsigned long long)capacity)
                    records[p.diag ? (long long)slot : capacity - 1 - (long long)slot] =
                        make_int4(p.b0 + first, p.a0 + second, (int)(p.diag ? hi : ~hi), picks);
                if (p.diag) sEx[2 * picks] = first, sEx[2 * picks + 1] = second;
                else sEx[picks] = second, sEx[FP_PICKS + picks] = first;
            }
            ++picks;
            if (met <= 1 || picks >= limit) break;     // else: the next round's first barrier (in dots) publishes sEx
        }
    }
    seen.publish(range, lane);
}

}  // namespace fn
using namespace fn;

extern "C" int fn_false_pairs(const float* emb, const int32_t* cls_start, int C, int E, int metric, float threshold, int max_fneg,
                              int max_fpos, int32_t* records, long long capacity, unsigned long long* count, int32_t* range,
                              void* stream) {
    const char* what = "false_pairs";
    FN_REQUIRE(E >= 4 && E % 4 == 0 && E <= 512, "%s: the embedding length must be a multiple of 4 in [4, 512] (E %d)", what, E);
    FN_REQUIRE(metric == 0 || metric == 1, "Undefined similarity metric %d", metric);   // statistics.py:55
    FN_REQUIRE(max_fneg >= 0 && max_fneg <= FP_PICKS, "%s: max_fneg must be in [0, %d] (max_fneg %d)", what, FP_PICKS, max_fneg);
    FN_REQUIRE(max_fpos >= 0 && max_fpos <= FP_PICKS, "%s: max_fpos must be in [0, %d] (max_fpos %d)", what, FP_PICKS, max_fpos);
    FN_REQUIRE(capacity >= 0, "%s: capacity must not be negative (capacity %lld)", what, capacity);
    FN_REQUIRE(records || capacity == 0, "%s: records may be null only with capacity 0 (capacity %lld)", what, capacity);
    FN_REQUIRE(emb && cls_start && count && C >= 1, "%s: bad arguments", what);
    int diag_groups, off_groups;
    FN_REQUIRE(class_pair_groups(C, &diag_groups, &off_groups), "%s: too many classes (C %d, at most 65535)", what, C);
    FN_REQUIRE(((uintptr_t)emb | (uintptr_t)records) % 16 == 0 && (uintptr_t)count % 8 == 0,
               "%s: emb and records must be 16-byte aligned, count 8-byte aligned", what);
    hipStream_t st = (hipStream_t)stream;
    if (range) fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);
    hipLaunchKernelGGL(false_pairs_kernel, dim3((unsigned)(diag_groups + off_groups)), dim3(256), 0, st, emb, cls_start, C, E, metric, threshold,
                       max_fneg, max_fpos, (int4*)records, capacity, count, (int*)range, diag_groups, off_groups);
    return check_launch(what);
}
