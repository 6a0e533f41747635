// Batch-mined triplet losses on a whole P x K batch (Hermans, Beyer, Leibe: arXiv 1703.07737 sec. 2):
// batch hard (per anchor the farthest positive and the nearest negative) and batch all (every valid triplet, averaged over the
// active ones), each with the hinge max(d_ap - d_an + alpha, 0) or the soft margin softplus(d_ap - d_an).
//
// Three kernels behind fn_batch_triplet_fwd_bwd, separate launches on the stream (the kernel boundary is what makes one phase's
// coef visible to the next: the eight XCDs' L2s are not coherent with each other):
//   mine    one workgroup per anchor a: row a of dist in LDS, the anchor's positives and negatives compacted in ascending order,
//           its terms, row a of coef, its counts (integer atomics into info) and its partial loss;
//   finish  one workgroup: the fixed-order fp64 sum of the anchors' partial losses, the normaliser Z, loss[0];
//   gather  one workgroup per row r: demb[r] = (2/Z) sum_j (coef[r][j] + coef[j][r]) (emb[r] - emb[j]), j ascending.
// No float atomics anywhere: the result has the same bits run to run, whatever the scheduling.  Rows p and n collect gradient from
// many anchors, which is why the gradient is a per-row gather over coef + coef^T and not a scatter from the anchors.
//
// Every term is formed in fp64 from the fp32 distances, l = ((double)d_ap - (double)d_an) + (double)alpha: the same IEEE operations
// a host reference performs, so `l > 0` is decided identically on both sides.  An anchor's terms are summed in fp64 in a fixed order
// (per thread: positives ascending, its negatives ascending; lanes by butterfly; waves 0..3).  That partial crosses the kernel
// boundary on coef's own diagonal -- coef[a][a] belongs to no term -- rounded once to fp32; the finish kernel sums the diagonal in
// fp64 in a fixed tree and leaves it zero.  The sum never enters the ACC_GRAD fixed-point accumulator (40 fractional bits:
// |sum| < 8.4e6), which 3.1 M terms of up to 4 + alpha each (batch all, N = 1024, K = 4) would overflow.
//
// Further down: fn_xbm_triplet_fwd_bwd and fn_xbm_enqueue, batch hard mined over the batch and a cross-batch memory (section 32).
#include "common.h"
#include "../../include/facenet_hip.h"

namespace fn {

enum { BT_THREADS = 256, BT_WAVES = 4, BT_MAX_N = 1024 };
enum { BT_ANCHORS = 0, BT_TERMS = 1, BT_ACTIVE = 2, BT_NONFINITE = 3 };

struct BtBest {
    float v;
    int i;      // -1: no candidate yet
};
// farthest / nearest candidate, the lowest index on equal distances.  (A NaN never wins and is never beaten: such an anchor sets
// BT_NONFINITE and the loss is NaN whatever is picked; the picked index stays inside the row.)
__device__ __forceinline__ BtBest bt_pick_max(BtBest a, BtBest b) {
    const bool take_b = a.i < 0 || (b.i >= 0 && (b.v > a.v || (b.v == a.v && b.i < a.i)));
    return take_b ? b : a;
}
__device__ __forceinline__ BtBest bt_pick_min(BtBest a, BtBest b) {
    const bool take_b = a.i < 0 || (b.i >= 0 && (b.v < a.v || (b.v == a.v && b.i < a.i)));
    return take_b ? b : a;
}
__device__ __forceinline__ BtBest bt_shfl_xor(BtBest b, int o) {
    BtBest r;
    r.v = __shfl_xor(b.v, o);
    r.i = __shfl_xor(b.i, o);
    return r;
}

__device__ __forceinline__ double bt_wave_sum(double v) {      // v_i + v_j on one lane, v_j + v_i on the other: the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int bt_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// softplus(l) = max(l, 0) + log1p(exp(-|l|)) and sigma(l) = d softplus / dl, neither of which can overflow
__device__ __forceinline__ void bt_soft(double l, double& value, double& sigma) {
    const double e = exp(-fabs(l));
    value = fmax(l, 0.0) + log1p(e);
    sigma = (l >= 0.0 ? 1.0 : e) / (1.0 + e);
}

__global__ __launch_bounds__(BT_THREADS) void batch_triplet_mine_kernel(const float* __restrict__ dist, const int* __restrict__ labels,
                                                                        float* __restrict__ coef, int* __restrict__ info, int N,
                                                                        float alpha, int strategy, int soft) {
    __shared__ float s_d[BT_MAX_N];                    // row a of dist
    __shared__ float s_c[BT_MAX_N];                    // row a of coef; [a] carries the anchor's partial loss to the finish kernel
    __shared__ unsigned short s_pos[BT_MAX_N];         // the anchor's positives, ascending
    __shared__ unsigned short s_neg[BT_MAX_N];         // its negatives, ascending
    __shared__ double s_part[BT_WAVES * BT_MAX_N];     // batch all: each wave's share of every positive's sum over the negatives
    __shared__ int s_cnt[2][BT_WAVES];
    __shared__ double s_red[BT_WAVES];
    __shared__ int s_redi[BT_WAVES];
    __shared__ BtBest s_best[2][BT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x;
    const int la = labels[a];
    for (int j = tid; j < N; j += BT_THREADS) {
        s_d[j] = dist[(long)a * N + j];
        s_c[j] = 0.f;
    }
    __syncthreads();
    // positives and negatives in ascending order: ballot ranks inside a wave, the waves' counts through LDS
    int npos = 0, nneg = 0, bad = 0;
    for (int j0 = 0; j0 < N; j0 += BT_THREADS) {
        const int j = j0 + tid;
        const bool other = j < N && labels[j] != la;
        const bool same = j < N && j != a && !other;
        if ((other || same) && !isfinite(s_d[j])) bad = 1;
        const unsigned long long bp = __ballot(same), bn = __ballot(other), below = (1ull << lane) - 1ull;
        if (lane == 0) {
            s_cnt[0][wave] = __popcll(bp);
            s_cnt[1][wave] = __popcll(bn);
        }
        __syncthreads();
        int base_p = npos, base_n = nneg;
        for (int w = 0; w < BT_WAVES; ++w) {
            if (w < wave) {
                base_p += s_cnt[0][w];
                base_n += s_cnt[1][w];
            }
            npos += s_cnt[0][w];
            nneg += s_cnt[1][w];
        }
        if (same) s_pos[base_p + __popcll(bp & below)] = (unsigned short)j;
        if (other) s_neg[base_n + __popcll(bn & below)] = (unsigned short)j;
        __syncthreads();
    }
    const bool valid = npos > 0 && nneg > 0;            // uniform over the workgroup
    if (!valid) {                                       // nobody's anchor: a row of zeros
        for (int j = tid; j < N; j += BT_THREADS) coef[(long)a * N + j] = 0.f;
        return;
    }
    const int any_bad = __syncthreads_or(bad);
    const double alpha_d = (double)alpha;

    if (strategy == 0) {
        BtBest bp = {0.f, -1}, bn = {0.f, -1};
        for (int k = tid; k < npos; k += BT_THREADS) {
            const int j = s_pos[k];
            bp = bt_pick_max(bp, BtBest{s_d[j], j});
        }
        for (int k = tid; k < nneg; k += BT_THREADS) {
            const int j = s_neg[k];
            bn = bt_pick_min(bn, BtBest{s_d[j], j});
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            bp = bt_pick_max(bp, bt_shfl_xor(bp, o));
            bn = bt_pick_min(bn, bt_shfl_xor(bn, o));
        }
        if (lane == 0) {
            s_best[0][wave] = bp;
            s_best[1][wave] = bn;
        }
        __syncthreads();
        if (tid == 0) {
            bp = s_best[0][0];
            bn = s_best[1][0];
            for (int w = 1; w < BT_WAVES; ++w) {
                bp = bt_pick_max(bp, s_best[0][w]);
                bn = bt_pick_min(bn, s_best[1][w]);
            }
            double value = 0.0;
            float c = 0.f;
            int active = soft ? 1 : 0;
            if (bp.i >= 0 && bn.i >= 0) {
                double l = (double)bp.v - (double)bn.v;
                if (soft) {
                    double sg;
                    bt_soft(l, value, sg);
                    c = (float)sg;
                } else {
                    l += alpha_d;
                    if (l > 0.0) {
                        value = l;
                        c = 1.f;
                        active = 1;
                    }
                }
                if (c != 0.f) {
                    s_c[bp.i] = c;
                    s_c[bn.i] = -c;
                }
            }
            s_c[a] = (float)value;
            atomicAdd(&info[BT_ANCHORS], 1);
            atomicAdd(&info[BT_TERMS], 1);
            if (active) atomicAdd(&info[BT_ACTIVE], active);
            if (any_bad) atomicOr(&info[BT_NONFINITE], 1);
        }
    } else {
        double lsum = 0.0, accn[BT_MAX_N / BT_THREADS] = {0.0, 0.0, 0.0, 0.0};
        int act = 0;
        float dn[BT_MAX_N / BT_THREADS];
#pragma unroll
        for (int q = 0; q < BT_MAX_N / BT_THREADS; ++q) {
            const int k = tid + q * BT_THREADS;
            dn[q] = k < nneg ? s_d[s_neg[k]] : 0.f;
        }
        for (int pi = 0; pi < npos; ++pi) {
            const double dap = (double)s_d[s_pos[pi]];
            double psum = 0.0;
#pragma unroll
            for (int q = 0; q < BT_MAX_N / BT_THREADS; ++q) {
                if (tid + q * BT_THREADS < nneg) {
                    double l = dap - (double)dn[q];
                    if (soft) {
                        double value, sg;
                        bt_soft(l, value, sg);
                        lsum += value;
                        psum += sg;
                        accn[q] += sg;
                    } else {
                        l += alpha_d;
                        if (l > 0.0) {
                            lsum += l;
                            psum += 1.0;
                            accn[q] += 1.0;
                            ++act;
                        }
                    }
                }
            }
            psum = bt_wave_sum(psum);
            if (lane == 0) s_part[wave * BT_MAX_N + pi] = psum;
        }
        lsum = bt_wave_sum(lsum);
        act = bt_wave_sum(act);
        if (lane == 0) {
            s_red[wave] = lsum;
            s_redi[wave] = act;
        }
        __syncthreads();
        for (int k = tid; k < npos; k += BT_THREADS) {
            const double c = ((s_part[k] + s_part[BT_MAX_N + k]) + s_part[2 * BT_MAX_N + k]) + s_part[3 * BT_MAX_N + k];
            s_c[s_pos[k]] = (float)c;
        }
#pragma unroll
        for (int q = 0; q < BT_MAX_N / BT_THREADS; ++q) {
            const int k = tid + q * BT_THREADS;
            if (k < nneg) s_c[s_neg[k]] = -(float)accn[q];
        }
        if (tid == 0) {
            const double total = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
            const int terms = npos * nneg;
            s_c[a] = (float)total;
            atomicAdd(&info[BT_ANCHORS], 1);
            atomicAdd(&info[BT_TERMS], terms);
            atomicAdd(&info[BT_ACTIVE], soft ? terms : ((s_redi[0] + s_redi[1]) + s_redi[2]) + s_redi[3]);
            if (any_bad) atomicOr(&info[BT_NONFINITE], 1);
        }
    }
    __syncthreads();
    for (int j = tid; j < N; j += BT_THREADS) coef[(long)a * N + j] = s_c[j];
}

__device__ __forceinline__ int bt_normaliser(const int* info, int strategy, int soft) {
    return strategy == 0 ? info[BT_ANCHORS] : (soft ? info[BT_TERMS] : info[BT_ACTIVE]);
}

// the anchors' partial losses wait on coef's diagonal: one fixed tree in fp64, then the diagonal is the zero it is specified to be
__global__ __launch_bounds__(BT_MAX_N) void batch_triplet_finish_kernel(float* __restrict__ coef, const int* __restrict__ info,
                                                                        float* __restrict__ loss, int N, int strategy, int soft) {
    __shared__ double s[BT_MAX_N];
    const int tid = threadIdx.x;
    s[tid] = tid < N ? (double)coef[(long)tid * N + tid] : 0.0;
    __syncthreads();
    for (int o = BT_MAX_N / 2; o > 0; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    if (tid < N) coef[(long)tid * N + tid] = 0.f;
    if (tid == 0) {
        const int Z = bt_normaliser(info, strategy, soft);
        loss[0] = info[BT_NONFINITE] ? __builtin_nanf("") : (Z > 0 ? (float)(s[0] / (double)Z) : 0.f);
    }
}

// one workgroup per row r.  The difference form x_r - x_j, not W X: near-duplicate rows do not cancel.  Every rounding of the chain
// is spelled out (one per difference, per product, per add), so the oracle's operation count is the kernel's.
__global__ __launch_bounds__(BT_THREADS) void batch_triplet_gather_kernel(const float* __restrict__ emb, const float* __restrict__ coef,
                                                                          const int* __restrict__ info, float* __restrict__ demb,
                                                                          int N, int E, int strategy, int soft) {
#pragma clang fp contract(off)
    __shared__ float s_w[BT_MAX_N];
    const int tid = threadIdx.x, r = blockIdx.x;
    for (int j = tid; j < N; j += BT_THREADS) s_w[j] = j == r ? 0.f : coef[(long)r * N + j] + coef[(long)j * N + r];
    __syncthreads();
    const int Z = bt_normaliser(info, strategy, soft);
    for (int e = tid; e < E; e += BT_THREADS) {
        float acc = 0.f;
        if (Z > 0) {
            const float xr = emb[(long)r * E + e];
            for (int j = 0; j < N; ++j) {
                const float w = s_w[j];
                if (w != 0.f) {
                    const float diff = xr - emb[(long)j * E + e];
                    const float prod = w * diff;
                    acc = acc + prod;
                }
            }
            acc = (float)((double)acc * 2.0 / (double)Z);
        }
        demb[(long)r * E + e] = acc;
    }
}

// ---- batch hard over the batch and a cross-batch memory (Wang et al., CVPR 2020) ---------------------------
// fn_xbm_triplet_fwd_bwd: the anchor's candidates are the batch columns j != a (union index j) and the slots s < valid of a ring of
// earlier steps' rows (union index N + s), valid = mem_state[1] read here, on the device.  Launches: mine (below), the finish kernel
// above (batch hard: Z = the anchors), gather.  The memory half of the mining never stages the row: M = 65 536 floats do not fit the
// LDS, and every element is looked at once, so each thread streams its stride of row a of mem_dist and of mem_labels with a running
// best.  A thread meets its candidates in ascending union index and the bt_pick_* merges prefer the lower index on equal distances,
// so the pick is the lowest union index whatever the order of the merges.
enum { XBM_MAX_M = 65536, XBM_UNROLL = 4 };
enum { XBM_CURSOR = 0, XBM_VALID = 1, XBM_CALLS = 2 };
enum { XBM_MEM_POS = 4, XBM_MEM_NEG = 5, XBM_VALID_SEEN = 6 };

__device__ __forceinline__ int xbm_valid_rows(const int* state, int M) {
    const int v = state[XBM_VALID];
    return v < 0 ? 0 : (v > M ? M : v);
}

__global__ __launch_bounds__(BT_THREADS) void xbm_triplet_mine_kernel(const float* __restrict__ dist, const int* __restrict__ labels,
                                                                      const float* __restrict__ mem_dist, const int* __restrict__ mem_labels,
                                                                      const int* __restrict__ mem_state, float* __restrict__ coef,
                                                                      int* __restrict__ mpick, float* __restrict__ mcoef,
                                                                      int* __restrict__ info, int N, int M, float alpha, int soft) {
    __shared__ float s_c[BT_MAX_N];                    // row a of coef; [a] carries the anchor's loss term to the finish kernel
    __shared__ BtBest s_best[2][BT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x;
    const int la = labels[a];
    const int valid = xbm_valid_rows(mem_state, M);
    BtBest bp = {0.f, -1}, bn = {0.f, -1};
    int bad = 0;
    for (int j = tid; j < N; j += BT_THREADS) {
        s_c[j] = 0.f;
        if (j != a) {
            const float d = dist[(long)a * N + j];
            if (!isfinite(d)) bad = 1;
            if (labels[j] == la) bp = bt_pick_max(bp, BtBest{d, j});
            else bn = bt_pick_min(bn, BtBest{d, j});
        }
    }
    const float* __restrict__ row = mem_dist + (long)a * M;
    for (int s0 = tid; s0 < valid; s0 += XBM_UNROLL * BT_THREADS) {
        float d[XBM_UNROLL];
        int l[XBM_UNROLL];
#pragma unroll
        for (int q = 0; q < XBM_UNROLL; ++q) {         // the loads of a trip are issued together
            const int s = s0 + q * BT_THREADS;
            const bool in = s < valid;
            d[q] = in ? row[s] : 0.f;
            l[q] = in ? mem_labels[s] : 0;
        }
#pragma unroll
        for (int q = 0; q < XBM_UNROLL; ++q) {
            const int s = s0 + q * BT_THREADS;
            if (s < valid) {
                if (!isfinite(d[q])) bad = 1;
                if (l[q] == la) bp = bt_pick_max(bp, BtBest{d[q], N + s});
                else bn = bt_pick_min(bn, BtBest{d[q], N + s});
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bp = bt_pick_max(bp, bt_shfl_xor(bp, o));
        bn = bt_pick_min(bn, bt_shfl_xor(bn, o));
    }
    if (lane == 0) {
        s_best[0][wave] = bp;
        s_best[1][wave] = bn;
    }
    const int any_bad = __syncthreads_or(bad);
    if (tid == 0) {
        bp = s_best[0][0];
        bn = s_best[1][0];
        for (int w = 1; w < BT_WAVES; ++w) {
            bp = bt_pick_max(bp, s_best[0][w]);
            bn = bt_pick_min(bn, s_best[1][w]);
        }
        int pick_p = -1, pick_n = -1;
        float cp = 0.f, cn = 0.f;
        if (bp.i >= 0 && bn.i >= 0) {                  // an anchor: a positive and a negative somewhere in the union
            double value = 0.0;
            float c = 0.f;
            int active = soft ? 1 : 0;
            double l = (double)bp.v - (double)bn.v;
            if (soft) {
                double sg;
                bt_soft(l, value, sg);
                c = (float)sg;
            } else {
                l += (double)alpha;
                if (l > 0.0) {
                    value = l;
                    c = 1.f;
                    active = 1;
                }
            }
            if (bp.i < N) {
                if (c != 0.f) s_c[bp.i] = c;
            } else {
                pick_p = bp.i - N;
                cp = c;
            }
            if (bn.i < N) {
                if (c != 0.f) s_c[bn.i] = -c;
            } else {
                pick_n = bn.i - N;
                cn = -c;
            }
            s_c[a] = (float)value;
            atomicAdd(&info[BT_ANCHORS], 1);
            atomicAdd(&info[BT_TERMS], 1);
            if (active) atomicAdd(&info[BT_ACTIVE], 1);
            if (any_bad) atomicOr(&info[BT_NONFINITE], 1);
            if (pick_p >= 0) atomicAdd(&info[XBM_MEM_POS], 1);
            if (pick_n >= 0) atomicAdd(&info[XBM_MEM_NEG], 1);
        }
        mpick[2 * a] = pick_p;
        mpick[2 * a + 1] = pick_n;
        mcoef[2 * a] = cp;
        mcoef[2 * a + 1] = cn;
        if (a == 0) info[XBM_VALID_SEEN] = valid;      // this word has one writer
    }
    __syncthreads();
    for (int j = tid; j < N; j += BT_THREADS) coef[(long)a * N + j] = s_c[j];
}

// batch_triplet_gather_kernel's chain, lengthened by the row's own memory picks: batch columns j ascending, then the memory
// positive, then the memory negative.  Memory rows are constants: nothing is written to them.
__global__ __launch_bounds__(BT_THREADS) void xbm_triplet_gather_kernel(const float* __restrict__ emb, const float* __restrict__ coef,
                                                                        const float* __restrict__ mem_emb, const int* __restrict__ mpick,
                                                                        const float* __restrict__ mcoef, const int* __restrict__ info,
                                                                        float* __restrict__ demb, int N, int M, int E) {
#pragma clang fp contract(off)
    __shared__ float s_w[BT_MAX_N];
    const int tid = threadIdx.x, r = blockIdx.x;
    for (int j = tid; j < N; j += BT_THREADS) s_w[j] = j == r ? 0.f : coef[(long)r * N + j] + coef[(long)j * N + r];
    __syncthreads();
    const int Z = info[BT_ANCHORS];
    int slot[2];
    float wm[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        slot[k] = mpick[2 * r + k];
        wm[k] = slot[k] >= 0 && slot[k] < M ? mcoef[2 * r + k] : 0.f;
    }
    for (int e = tid; e < E; e += BT_THREADS) {
        float acc = 0.f;
        if (Z > 0) {
            const float xr = emb[(long)r * E + e];
            for (int j = 0; j < N; ++j) {
                const float w = s_w[j];
                if (w != 0.f) {
                    const float diff = xr - emb[(long)j * E + e];
                    const float prod = w * diff;
                    acc = acc + prod;
                }
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (wm[k] != 0.f) {
                    const float diff = xr - mem_emb[(long)slot[k] * E + e];
                    const float prod = wm[k] * diff;
                    acc = acc + prod;
                }
            }
            acc = (float)((double)acc * 2.0 / (double)Z);
        }
        demb[(long)r * E + e] = acc;
    }
}

// fn_xbm_enqueue, two launches: the copy reads the state words, the advance rewrites them.  One launch doing both would let a
// workgroup move the cursor while another still reads it.  A cursor outside [0, M) -- nothing here writes one -- is folded into it.
__device__ __forceinline__ int xbm_cursor(const int* state, int M) {
    const int c = state[XBM_CURSOR] % M;
    return c < 0 ? c + M : c;
}

__global__ __launch_bounds__(BT_THREADS) void xbm_enqueue_copy_kernel(const float* __restrict__ emb, const int* __restrict__ labels,
                                                                      float* __restrict__ mem_emb, int* __restrict__ mem_labels,
                                                                      const int* __restrict__ mem_state, int N, int M, int E, int start) {
    if (mem_state[XBM_CALLS] < start) return;
    const int cursor = xbm_cursor(mem_state, M);
    const long total = (long)N * E;
    for (long t = (long)blockIdx.x * BT_THREADS + threadIdx.x; t < total; t += (long)gridDim.x * BT_THREADS) {
        const int i = (int)(t / E), e = (int)(t - (long)i * E);
        const int slot = (cursor + i) % M;
        mem_emb[(long)slot * E + e] = emb[t];
        if (e == 0) mem_labels[slot] = labels[i];
    }
}

__global__ void xbm_enqueue_advance_kernel(int* __restrict__ mem_state, int N, int M, int start) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int calls = mem_state[XBM_CALLS];
    if (calls >= start) {
        const int cursor = xbm_cursor(mem_state, M), valid = xbm_valid_rows(mem_state, M);
        mem_state[XBM_CURSOR] = (cursor + N) % M;
        mem_state[XBM_VALID] = valid + N > M ? M : valid + N;
    }
    mem_state[XBM_CALLS] = calls < 0x7fffffff ? calls + 1 : calls;
    mem_state[3] = 0;
}

}  // namespace fn
using namespace fn;

extern "C" int fn_xbm_triplet_fwd_bwd(const float* emb, const float* dist, const int32_t* labels, const float* mem_emb, const float* mem_dist,
                                      const int32_t* mem_labels, const int32_t* mem_state, float* demb, float* loss, float* coef,
                                      int32_t* mpick, float* mcoef, int32_t* info, int N, int M, int E, float alpha, int soft, void* stream) {
    FN_REQUIRE(emb && dist && labels && mem_emb && mem_dist && mem_labels && mem_state && loss && coef && mpick && mcoef && info,
               "xbm_triplet: only demb may be NULL");
    FN_REQUIRE(N >= 2 && N <= BT_MAX_N, "xbm_triplet: N must be in [2, 1024], got %d", N);
    FN_REQUIRE(M >= N && M <= XBM_MAX_M, "xbm_triplet: M must be in [N, 65536], got %d (N = %d)", M, N);
    FN_REQUIRE(E >= 1 && E <= 512, "xbm_triplet: E must be in [1, 512], got %d", E);
    FN_REQUIRE(soft == 0 || soft == 1, "xbm_triplet: soft must be 0 or 1, got %d", soft);
    FN_REQUIRE(soft || (alpha >= 0.f && alpha <= 3.402823466e38f), "xbm_triplet: alpha must be finite and >= 0, got %g", (double)alpha);
    FN_REQUIRE(((uintptr_t)loss & 7) == 0, "xbm_triplet: loss must be an 8-byte aligned fp32[4]");
    hipStream_t st = (hipStream_t)stream;
    fill_words(info, 0u, 0u, 8, st);
    hipLaunchKernelGGL(xbm_triplet_mine_kernel, dim3(N), dim3(BT_THREADS), 0, st, dist, labels, mem_dist, mem_labels, mem_state, coef, mpick,
                       mcoef, info, N, M, alpha, soft);
    hipLaunchKernelGGL(batch_triplet_finish_kernel, dim3(1), dim3(BT_MAX_N), 0, st, coef, info, loss, N, 0, soft);
    if (demb)
        hipLaunchKernelGGL(xbm_triplet_gather_kernel, dim3(N), dim3(BT_THREADS), 0, st, emb, coef, mem_emb, mpick, mcoef, info, demb, N, M, E);
    return check_launch("xbm_triplet");
}

extern "C" int fn_xbm_enqueue(const float* emb, const int32_t* labels, float* mem_emb, int32_t* mem_labels, int32_t* mem_state, int N, int M,
                              int E, int start, void* stream) {
    FN_REQUIRE(emb && labels && mem_emb && mem_labels && mem_state, "xbm_enqueue: no pointer may be NULL");
    FN_REQUIRE(N >= 1 && N <= BT_MAX_N, "xbm_enqueue: N must be in [1, 1024], got %d", N);
    FN_REQUIRE(M >= N && M <= XBM_MAX_M, "xbm_enqueue: M must be in [N, 65536], got %d (N = %d)", M, N);
    FN_REQUIRE(E >= 1 && E <= 512, "xbm_enqueue: E must be in [1, 512], got %d", E);
    FN_REQUIRE(start >= 0, "xbm_enqueue: start must be >= 0, got %d", start);
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)N * E;
    hipLaunchKernelGGL(xbm_enqueue_copy_kernel, dim3((unsigned)((total + BT_THREADS - 1) / BT_THREADS)), dim3(BT_THREADS), 0, st, emb, labels,
                       mem_emb, mem_labels, mem_state, N, M, E, start);
    hipLaunchKernelGGL(xbm_enqueue_advance_kernel, dim3(1), dim3(64), 0, st, mem_state, N, M, start);
    return check_launch("xbm_enqueue");
}

extern "C" int fn_batch_triplet_fwd_bwd(const float* emb, const float* dist, const int32_t* labels, float* demb, float* loss, float* coef,
                                        int32_t* info, int N, int E, float alpha, int strategy, int soft, void* stream) {
    FN_REQUIRE(emb && dist && labels && loss && coef && info, "batch_triplet: emb, dist, labels, loss, coef and info must not be NULL");
    FN_REQUIRE(N >= 2 && N <= BT_MAX_N, "batch_triplet: N must be in [2, 1024], got %d", N);
    FN_REQUIRE(E >= 1 && E <= 512, "batch_triplet: E must be in [1, 512], got %d", E);
    FN_REQUIRE((strategy == 0 || strategy == 1) && (soft == 0 || soft == 1), "batch_triplet: strategy and soft must be 0 or 1, got %d, %d",
               strategy, soft);
    FN_REQUIRE(soft || (alpha >= 0.f && alpha <= 3.402823466e38f), "batch_triplet: alpha must be finite and >= 0, got %g", (double)alpha);
    FN_REQUIRE(((uintptr_t)loss & 7) == 0, "batch_triplet: loss must be an 8-byte aligned fp32[4]");
    hipStream_t st = (hipStream_t)stream;
    fill_words(info, 0u, 0u, 8, st);
    hipLaunchKernelGGL(batch_triplet_mine_kernel, dim3(N), dim3(BT_THREADS), 0, st, dist, labels, coef, info, N, alpha, strategy, soft);
    hipLaunchKernelGGL(batch_triplet_finish_kernel, dim3(1), dim3(BT_MAX_N), 0, st, coef, info, loss, N, strategy, soft);
    if (demb)
        hipLaunchKernelGGL(batch_triplet_gather_kernel, dim3(N), dim3(BT_THREADS), 0, st, emb, coef, info, demb, N, E, strategy, soft);
    return check_launch("batch_triplet");
}
