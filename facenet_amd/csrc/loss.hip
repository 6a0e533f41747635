// Distance matrix, online triplet selection, triplet loss, softmax cross-entropy.
//  * fn_pairwise_sqdist restates facenet/statistics.py:22-57 (pairwise_similarities) on device:
//    one wave per (row i, block of columns), dot products by wavefront reduction.
//  * triplet selection / loss are build-defined (arXiv 1503.03832 sec. 3); the
//    counter-based hash below is shared bit-for-bit with oracle/facenet_oracle.py:hash_u32 so the
//    selected indices can be compared exactly.
//  * softmax cross-entropy = SparseCategoricalCrossentropy(from_logits=True), apps/train_softmax.py:91.
//  * center loss + its center update = facenet/facenet.py:204-217 (center_loss); prelogits norm = the
//    loss.prelogits_norm_* keys of apps/configs/train_softmax.yaml:73-78 (formula: DESIGN.md section 11).
//  * large-margin cosine softmax (NormFace / CosFace / ArcFace) on the normalised embedding and class rows: DESIGN.md section 21.
#include "pair_tiles.h"      // ord_f32, DotRange, pair_distance: shared with the validation, identification and clustering kernels
#include "../../include/facenet_hip.h"

namespace fn {

// out[i][j] for i<n, j<m ; range[0]=ord(min dot) via atomicMin, range[1]=ord(max dot) via atomicMax
__global__ __launch_bounds__(256) void pairwise_kernel(const float* __restrict__ xa, const float* __restrict__ xb, float* __restrict__ out,
                                                       int* __restrict__ range, int n, int m, int E, int metric) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.y;
    const int jb = (blockIdx.x * 4 + wave) * 16;
    if (jb >= m) return;
    // this lane's slice of row i stays in registers (E <= 64*8).  Every sum below is an explicit fma chain in ONE fixed order,
    // and a row's squared norm is computed by the same code whether the row is an `a` or a `b`: out[i][j] and out[j][i] are
    // then the same bits (|a|^2 + |b|^2 commutes, the dot product's terms commute), which the triplet selection relies on
    // when it reads columns instead of rows.  Left to the compiler's contraction choices the two norms differed in the last bit.
    float a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = (lane + 64 * t < E) ? xa[(long)i * E + lane + 64 * t] : 0.f;
    float asq = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) asq = __fmaf_rn(a[t], a[t], asq);
    asq = wave_sum(asq);
    DotRange seen;
    for (int j = jb; j < min(m, jb + 16); ++j) {
        float d = 0.f, bsq = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float b = (lane + 64 * t < E) ? xb[(long)j * E + lane + 64 * t] : 0.f;
            d = __fmaf_rn(a[t], b, d);
            bsq = __fmaf_rn(b, b, bsq);
        }
        d = wave_sum(d);
        float r;
        if (metric == 2) {
            bsq = wave_sum(bsq);
            r = fmaxf(__fmaf_rn(-2.f, d, asq + bsq), 0.f);
        } else {
            seen.add(d);
            r = pair_distance(d, metric);
        }
        if (lane == 0) out[(long)i * m + j] = r;
    }
    if (range && lane == 0 && metric != 2) seen.write(range);    // d is wave-uniform, and this wave has evaluated a pair
}

__device__ __forceinline__ unsigned hash_mix(unsigned h, unsigned v) {
    h ^= v;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned hash_u32(unsigned a, unsigned b, unsigned c) {
    return hash_mix(hash_mix(hash_mix(0x9E3779B9u, a), b), c);
}

// The distance matrix is bitwise symmetric (same products, same order), so thread a reads COLUMN a
// (dist[j*n + a]: consecutive threads -> consecutive addresses) instead of its own row.
// n <= 1024.  scratch (int32, global): per pair q: [a, p, neg, key(u32), cls] at scratch[8 + 5*q].
// info[0] = #pairs, info[1] = #valid (candidate found), info[2] = 1 if fewer pairs than requested triplets,
// info[3] = call counter: the effective seed is seed + info[3], so a HIP-graph replay (frozen kernel arguments)
// still draws fresh negatives every step.  The caller zeroes info once.
// Three launches: (A) one workgroup enumerates the anchor-positive pairs, (B) one WAVE per pair -- spread over the chip -- picks
// the negative, (C) one workgroup ranks the pairs and writes the triplets.  As a single workgroup phase B ran 17 rounds of
// dependent loads (~70 us of the 85 us kernel).
__global__ __launch_bounds__(1024) void select_pairs_kernel(const int* __restrict__ labels, int n, int* __restrict__ info) {
    __shared__ int s_lab[1024];
    __shared__ int s_off[1025];
    const int tid = threadIdx.x;
    int* rec = info + 8;
    for (int i = tid; i < n; i += 1024) s_lab[i] = labels[i];
    __syncthreads();
    // pairs per anchor (a < p, same label), exclusive prefix -> pair ids in row-major order
    int cnt = 0;
    if (tid < n)
        for (int p = tid + 1; p < n; ++p) cnt += (s_lab[p] == s_lab[tid]);
    // inclusive prefix of the per-anchor counts: wave scan + carry of the wave totals (a serial loop of thread 0 over the n entries
    // was ~7 us of dependent LDS round trips)
    {
        __shared__ int s_wtot[16];
        const int lane = tid & 63, wv = tid >> 6;
        int v = tid < n ? cnt : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d);
            if (lane >= d) v += u;
        }
        if (lane == 63) s_wtot[wv] = v;
        __syncthreads();
        int carry = 0;
        for (int w = 0; w < wv; ++w) carry += s_wtot[w];
        if (tid < n) s_off[tid + 1] = v + carry;
        if (tid == 0) s_off[0] = 0;
    }
    __syncthreads();
    if (tid < n) {
        int q = s_off[tid];
        for (int p = tid + 1; p < n; ++p)
            if (s_lab[p] == s_lab[tid]) { rec[5 * q + 0] = tid; rec[5 * q + 1] = p; ++q; }
    }
    if (tid == 0) {
        info[0] = s_off[n];
        info[1] = 0;
    }
}

__global__ __launch_bounds__(256) void select_negatives_kernel(const float* __restrict__ dist, const int* __restrict__ labels, int n,
                                                               float alpha, unsigned seed0, int semi_hard, int* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= info[0]) return;
    const unsigned seed = seed0 + (unsigned)info[3];
    int* rec = info + 8;
    const int a = rec[5 * q + 0], p = rec[5 * q + 1];
    const int la = labels[a];
    const float dap = dist[(long)p * n + a];
    int c = 0, others = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool oth = (j < n) && (labels[j] != la);
        const float daj = oth ? dist[(long)j * n + a] : 0.f;
        const bool cand = oth && (daj - dap < alpha) && (!semi_hard || daj > dap);
        c += __popcll(__ballot(cand));
        others += __popcll(__ballot(oth));
    }
    const bool use_cand = c > 0;
    int want = use_cand ? (int)(hash_u32(seed, (unsigned)q, 0u) % (unsigned)c)
                        : (others > 0 ? (int)(hash_u32(seed, (unsigned)q, 2u) % (unsigned)others) : -1);
    int neg = -1;
    for (int j0 = 0; j0 < n && want >= 0; j0 += 64) {
        const int j = j0 + lane;
        const bool oth = (j < n) && (labels[j] != la);
        const float daj = oth ? dist[(long)j * n + a] : 0.f;
        const bool hit = use_cand ? (oth && (daj - dap < alpha) && (!semi_hard || daj > dap)) : oth;
        const unsigned long long m = __ballot(hit);
        const int cnt = __popcll(m);
        if (want < cnt) {
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            const unsigned long long sel = __ballot(hit && rank == want);
            neg = j0 + (int)__ffsll((long long)sel) - 1;
            want = -1;
        } else {
            want -= cnt;
        }
    }
    if (lane == 0) {
        rec[5 * q + 2] = neg;
        rec[5 * q + 3] = (int)hash_u32(seed, (unsigned)q, 1u);
        rec[5 * q + 4] = use_cand ? 0 : 1;
        if (use_cand) atomicAdd(&info[1], 1);
    }
}

__global__ __launch_bounds__(1024) void select_rank_kernel(int T, int* __restrict__ triplets, int* __restrict__ info) {
    const int tid = threadIdx.x;
    const int* rec = info + 8;
    const int Q = info[0];
    // (cls, key) of the first 4096 pairs staged in LDS as one 64-bit sort key: the O(Q^2) comparison loop then reads LDS, not global
    __shared__ unsigned long long s_key[4096];
    for (int q = tid; q < min(Q, 4096); q += 1024)
        s_key[q] = ((unsigned long long)(unsigned)rec[5 * q + 4] << 32) | (unsigned)rec[5 * q + 3];
    __syncthreads();
    // rank by (cls, key, q); rank < T wins slot `rank`
    for (int q = tid; q < Q; q += 1024) {
        const int cls = rec[5 * q + 4];
        const unsigned key = (unsigned)rec[5 * q + 3];
        const unsigned long long mine = ((unsigned long long)(unsigned)cls << 32) | key;
        int rank = 0;
        const int QL = min(Q, 4096);
        for (int r = 0; r < QL; ++r) {
            const unsigned long long k2 = s_key[r];
            rank += (k2 < mine || (k2 == mine && r < q)) ? 1 : 0;
        }
        for (int r = QL; r < Q; ++r) {
            const int c2 = rec[5 * r + 4];
            const unsigned k2 = (unsigned)rec[5 * r + 3];
            const bool before = (c2 < cls) || (c2 == cls && (k2 < key || (k2 == key && r < q)));
            rank += before ? 1 : 0;
        }
        if (rank < T && rec[5 * q + 2] >= 0) {
            triplets[3 * rank + 0] = rec[5 * q + 0];
            triplets[3 * rank + 1] = rec[5 * q + 1];
            triplets[3 * rank + 2] = rec[5 * q + 2];
        }
    }
    if (tid == 0) {
        info[2] = (Q < T) ? 1 : 0;
        info[3] = info[3] + 1;
    }
}

// emb rows (a0,p0,n0,a1,...), fp32 [3T,E].  One wave per triplet.
__global__ __launch_bounds__(256) void triplet_loss_kernel(const float* __restrict__ emb, float* __restrict__ demb, acc_t* __restrict__ loss,
                                                           int T, int E, float alpha) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    const float* a = emb + (long)(3 * t) * E;
    const float* p = a + E;
    const float* ng = p + E;
    float pos = 0.f, neg = 0.f;
    for (int k = lane; k < E; k += 64) {
        const float dp = a[k] - p[k], dn = a[k] - ng[k];
        pos += dp * dp;
        neg += dn * dn;
    }
    pos = wave_sum(pos);
    neg = wave_sum(neg);
    const float l = pos - neg + alpha;
    const float on = l > 0.f ? 1.f : 0.f;
    if (lane == 0) acc_add<ACC_GRAD>(loss, fmaxf(l, 0.f) / (float)T);
    if (demb) {
        const float s = 2.f * on / (float)T;
        float* da = demb + (long)(3 * t) * E;
        for (int k = lane; k < E; k += 64) {
            da[k] = s * (ng[k] - p[k]);
            da[E + k] = s * (p[k] - a[k]);
            da[2 * E + k] = s * (a[k] - ng[k]);
        }
    }
}

// one workgroup per row: loss += (lse - logit[label])/N ; dlogits = (softmax - onehot) * grad_scale (low precision, padded cols = 0)
template <typename T>
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits, int ld, const int* __restrict__ labels,
                                                           acc_t* __restrict__ loss, unsigned short* __restrict__ dlogits, int ld_d,
                                                           acc_t* __restrict__ dbias, int N, int C, float grad_scale) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (long)row * ld;
    float mx = -3e38f;
    for (int c = tid; c < C; c += 256) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int c = tid; c < C; c += 256) s += __expf(x[c] - mx);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = red[0] + red[1] + red[2] + red[3];
    // an out-of-range class index never indexes the logits: the loss becomes NaN (what TF's GPU kernel returns; its CPU kernel
    // raises, which Trainer.set_images does on the host) and the row contributes no one-hot term
    const int lab = labels[row];
    const bool lab_ok = lab >= 0 && lab < C;
    // (a NaN cannot live in the fixed-point sum: an invalid label sets the flag word, loss_finish_kernel then reports NaN)
    if (tid == 0) {
        if (lab_ok) acc_add<ACC_GRAD>(loss, (logf(s) + mx - x[lab]) / (float)N);
        else reinterpret_cast<volatile unsigned*>(loss)[-1] = 1u;
    }
    if (dlogits) {
        const float inv = 1.f / s;
        unsigned short* d = dlogits + (long)row * ld_d;
        for (int c = tid; c < ld_d; c += 256) {
            float g = 0.f;
            if (c < C) {
                g = (__expf(x[c] - mx) * inv - (c == lab ? 1.f : 0.f)) * grad_scale;
                if (dbias) acc_add<ACC_GRAD>(&dbias[c], g);
            }
            d[c] = LP<T>::from_f32(g);
        }
    }
}

// loss words: [0] = the loss (fp32), [1] = invalid-input flag, [2..3] = fixed-point accumulator (ACC_GRAD) the rows add into
__global__ void loss_finish_kernel(float* loss) {
    const float v = acc_get<ACC_GRAD>(*reinterpret_cast<const acc_t*>(loss + 2));
    loss[0] = reinterpret_cast<const unsigned*>(loss)[1] ? __builtin_nanf("") : v;
}


// ---- embedding regularisers of softmax training ------------------------------------------------------
// terms words: [0] center loss, [1] prelogits norm (fp32 results), [2] flags (bit 0: center term invalid, bit 1: norm term
// invalid), [3] spare, [4..5] and [6..7] the fixed-point accumulators (ACC_GRAD) of the two terms.  The finish kernel reads and
// re-zeroes words 2..7, so one launch per step is enough and the caller zeroes the buffer only once, at allocation.
enum { REG_FLAG = 2, REG_ACC_CENTER = 4, REG_ACC_NORM = 6 };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a row term goes into the fixed-point sum only when the conversion is defined (|v| < 2^(62-40)); otherwise the term's flag is set
__device__ __forceinline__ void reg_acc_add(float* terms, int word, unsigned flag_bit, double v) {
    if (isfinite(v) && fabs(v) < 4194304.0) acc_add<ACC_GRAD>(reinterpret_cast<acc_t*>(terms + word), (float)v);
    else atomicOr(reinterpret_cast<unsigned*>(terms + REG_FLAG), flag_bit);
}

// One wave per row i (4 rows per 256-thread workgroup), 16-byte loads (E % 4 == 0).  a = |x| + 1e-4 is formed in fp32 (x is
// fp32); every other quantity -- sums, the norm, both gradient terms and the update of demb -- is computed in double and demb is
// rounded once, so demb + g is within half an ulp of the exact sum.  p == 1 and p == 2 avoid pow().
__global__ __launch_bounds__(256) void center_loss_kernel(const float* __restrict__ x, const int* __restrict__ labels,
                                                          const float* __restrict__ centers, float* __restrict__ demb,
                                                          float* __restrict__ terms, float* __restrict__ xy, int ld_xy, int N, int E,
                                                          int C, float center_factor, float norm_factor, float p) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int lab = labels[i];
    const bool use_c = centers != nullptr && lab >= 0 && lab < C;
    const float* xr = x + (long)i * E;
    const float* cr = use_c ? centers + (long)lab * E : nullptr;
    const double pd = (double)p;
    const int mode = p == 1.f ? 1 : (p == 2.f ? 2 : 0);
    double sd = 0.0, sa = 0.0;
    for (int e = 4 * lane; e < E; e += 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + e);
        f32x4 cv = {0.f, 0.f, 0.f, 0.f};
        if (use_c) cv = *reinterpret_cast<const f32x4*>(cr + e);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double d = (double)xv[t] - (double)cv[t];
            sd += d * d;
            const double a = (double)(fabsf(xv[t]) + 1e-4f);
            sa += mode == 1 ? a : (mode == 2 ? a * a : pow(a, pd));
        }
        if (xy) {
            float* o = xy + (long)i * ld_xy + e;
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = xv[t];
        }
    }
    sd = wave_sum_d(sd);
    sa = wave_sum_d(sa);
    const double n = mode == 1 ? sa : (mode == 2 ? sqrt(sa) : pow(sa, 1.0 / pd));
    if (lane == 0) {
        if (centers) {
            if (use_c) reg_acc_add(terms, REG_ACC_CENTER, 1u, sd / ((double)N * (double)E));
            else atomicOr(reinterpret_cast<unsigned*>(terms + REG_FLAG), 1u);    // a class index outside [0, C): no center to read
        }
        reg_acc_add(terms, REG_ACC_NORM, 2u, n / (double)N);
        if (xy) xy[(long)i * ld_xy + E] = (float)lab;      // exact for |label| < 2^24
    }
    const bool g_c = use_c && center_factor != 0.f, g_n = norm_factor != 0.f;
    if (!demb || !(g_c || g_n)) return;
    // d/dx of factor_c * mean (x - c)^2 and of factor_n * mean_i n_i: 2 (x - c) / (N E) and sign(x) a^(p-1) n^(1-p) / N
    const double kc = 2.0 * (double)center_factor / ((double)N * (double)E);
    const double kn = (double)norm_factor / (double)N * (mode == 1 ? 1.0 : (mode == 2 ? 1.0 / n : pow(n, 1.0 - pd)));
    float* dr = demb + (long)i * E;
    for (int e = 4 * lane; e < E; e += 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + e);
        f32x4 cv = {0.f, 0.f, 0.f, 0.f};
        if (g_c) cv = *reinterpret_cast<const f32x4*>(cr + e);
        f32x4 dv = *reinterpret_cast<const f32x4*>(dr + e);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            double g = 0.0;
            if (g_c) g += kc * ((double)xv[t] - (double)cv[t]);
            if (g_n && xv[t] != 0.f) {         // sign(0) = 0: TF's gradient of abs
                const double a = (double)(fabsf(xv[t]) + 1e-4f);
                const double w = mode == 1 ? 1.0 : (mode == 2 ? a : pow(a, pd - 1.0));
                g += (xv[t] > 0.f ? kn : -kn) * w;
            }
            dv[t] = (float)((double)dv[t] + g);
        }
        *reinterpret_cast<f32x4*>(dr + e) = dv;
    }
}

__global__ void center_loss_finish_kernel(float* terms) {
    unsigned* flags = reinterpret_cast<unsigned*>(terms + REG_FLAG);
    acc_t* acc = reinterpret_cast<acc_t*>(terms + REG_ACC_CENTER);
    const unsigned f = *flags;
    terms[0] = (f & 1u) ? __builtin_nanf("") : acc_get<ACC_GRAD>(acc[0]);
    terms[1] = (f & 2u) ? __builtin_nanf("") : acc_get<ACC_GRAD>(acc[1]);
    *flags = 0u;
    acc[0] = 0;
    acc[1] = 0;
}

// facenet.py:212-213 with a fixed order for repeated labels: the workgroup of the FIRST row carrying a class owns that class and
// walks the rows that carry it in ascending order, c <- c - k (c_old - x_j); every other workgroup leaves at once.  No atomics:
// every center row has exactly one writer.  rows: [M][ld] fp32 = x_j (E values) followed by float(label_j).  Every rounding is
// spelled out (no fused multiply-add) so a float32 NumPy restatement gives the same bits.
__global__ __launch_bounds__(256) void center_update_kernel(const float* __restrict__ rows, int ld, int M, int E,
                                                            float* __restrict__ centers, int C, float k) {
#pragma clang fp contract(off)
    __shared__ int s_lab[4096];
    __shared__ int s_rows[4096];        // the rows carrying this workgroup's class, ascending
    __shared__ int s_wcnt[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < M; j += 256) {
        const float v = rows[(long)j * ld + E];
        s_lab[j] = (v >= 0.f && v < (float)C && v == floorf(v)) ? (int)v : -1;    // NaN / out of range: no class
    }
    __syncthreads();
    const int y = s_lab[i];
    int dup = 0;
    for (int j = tid; j < i; j += 256) dup |= (s_lab[j] == y);
    if (__syncthreads_or(dup) || y < 0) return;
    // ordered compaction of the rows j >= i with label y (wave ballots + the counts of the waves before): the walk below then
    // visits only them, instead of testing all M labels per element
    int n = 0;
    for (int base = i; base < M; base += 256) {
        const int j = base + tid;
        const bool hit = j < M && s_lab[j] == y;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = n;
        for (int w = 0; w < wave; ++w) off += s_wcnt[w];
        if (hit) s_rows[off + __popcll(m & ((1ull << lane) - 1ull))] = j;
        n += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    float* cr = centers + (long)y * E;
    for (int e = tid; e < E; e += 256) {
        const float c_old = cr[e];
        float c = c_old;
        for (int r = 0; r < n; ++r) {
            const float t = c_old - rows[(long)s_rows[r] * ld + e];
            const float u = k * t;
            c = c - u;
        }
        cr[e] = c;
    }
}
// ---- large-margin cosine softmax: NormFace / CosFace / ArcFace ----------------------------------------
// r[j] = 1 / sqrt(max(sum_e w[j][e]^2, eps)): one wave per class row (4 rows per workgroup), 16-byte loads, per-lane chain in
// ascending e, then the butterfly.  sqrtf and the division are correctly rounded, so a one-hot row gives exactly 1.
__global__ __launch_bounds__(256) void margin_rnorm_kernel(const float* __restrict__ w, int C, int E, float eps, float* __restrict__ rnorm) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= C) return;
    const float* wr = w + (long)j * E;
    float s = 0.f;
    for (int e = 4 * lane; e < E; e += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wr + e);
#pragma unroll
        for (int t = 0; t < 4; ++t) s += v[t] * v[t];
    }
    s = wave_sum(s);
    if (lane == 0) rnorm[j] = 1.f / sqrtf(fmaxf(s, eps));
}

// cos m2, sin m2, th = cos(pi - m2), mm = sin(pi - m2) m2: computed once on the host in double from the fp32 m2, rounded to fp32
struct MarginConsts {
    float scale, cos_m, sin_m, th, mm, m_cos;
};
#define FN_MARGIN_T 0.99999904632568359375f      // 1 - 2^-20: keeps (1 - ct)(1 + ct) >= 2^-20, so dphi/dc < cos m2 + 725 sin m2

// c = clamp(z r, -1, 1); the target column's phi and D = dphi/dc at ct = clamp(c, -T, T).  Every rounding is spelled out.
__device__ __forceinline__ float margin_cosine(float z, float r) {
#pragma clang fp contract(off)
    return fminf(fmaxf(z * r, -1.f), 1.f);
}
__device__ __forceinline__ float margin_phi(float c, const MarginConsts& k, float& D) {
#pragma clang fp contract(off)
    const float ct = fminf(fmaxf(c, -FN_MARGIN_T), FN_MARGIN_T);
    if (ct > k.th) {
        const float a = 1.f - ct, b = 1.f + ct;
        const float q = a * b;                  // a product, not 1 - ct^2: 1 - ct is exact near 1
        const float sq = sqrtf(q);
        const float u = ct * k.cos_m, v = sq * k.sin_m;
        const float n = ct * k.sin_m;
        D = k.cos_m + n / sq;
        return (u - v) - k.m_cos;
    }
    D = 1.f;                                    // theta + m2 > pi: the linear continuation
    return (ct - k.mm) - k.m_cos;
}
__device__ __forceinline__ float margin_logit(float z, float r, bool target, const MarginConsts& k) {
#pragma clang fp contract(off)
    const float c = margin_cosine(z, r);
    float D;
    return k.scale * (target ? margin_phi(c, k, D) : c);
}

// one workgroup per row, shaped like softmax_xent_kernel: l = s c (s phi in the label's column); loss += (lse - l[label]) / N;
// g = (softmax - onehot) grad_scale s D; dz = g r (low precision, padded columns = 0); t[c] += g c (fixed point)
template <typename T>
__global__ __launch_bounds__(256) void margin_softmax_kernel(const float* __restrict__ z, int ld, const float* __restrict__ rnorm,
                                                             const int* __restrict__ labels, acc_t* __restrict__ loss,
                                                             unsigned short* __restrict__ dz, int ld_d, acc_t* __restrict__ tacc, int N, int C,
                                                             MarginConsts k, float grad_scale) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = z + (long)row * ld;
    const int lab = labels[row];
    const bool lab_ok = lab >= 0 && lab < C;
    float mx = -3e38f;
    for (int c = tid; c < C; c += 256) mx = fmaxf(mx, margin_logit(x[c], rnorm[c], c == lab, k));
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int c = tid; c < C; c += 256) s += __expf(margin_logit(x[c], rnorm[c], c == lab, k) - mx);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    s = red[0] + red[1] + red[2] + red[3];
    // an out-of-range class index never indexes the logits: the flag word makes the loss NaN, the row has no one-hot term
    if (tid == 0) {
        if (lab_ok) acc_add<ACC_GRAD>(loss, (logf(s) + mx - margin_logit(x[lab], rnorm[lab], true, k)) / (float)N);
        else reinterpret_cast<volatile unsigned*>(loss)[-1] = 1u;
    }
    if (!dz && !tacc) return;
    const float inv = 1.f / s;
    unsigned short* d = dz ? dz + (long)row * ld_d : nullptr;
    const int cols = dz ? ld_d : C;
    for (int c = tid; c < cols; c += 256) {
        float gz = 0.f;
        if (c < C) {
            const float r = rnorm[c], cv = margin_cosine(x[c], r);
            float D = 1.f, l = cv;
            if (c == lab) l = margin_phi(cv, k, D);
            l = k.scale * l;
            float g = (__expf(l - mx) * inv - (c == lab ? 1.f : 0.f)) * grad_scale;
            g = g * k.scale;
            g = g * D;
            if (tacc) acc_add<ACC_GRAD>(&tacc[c], g * cv);
            gz = g * r;
        }
        if (d) d[c] = LP<T>::from_f32(gz);
    }
}

// dw[j][e] -= (r_j^2 t_j) w[j][e] for j < C: one wave per class row, 16-byte accesses; lane 0 reads t[j] and leaves it zeroed
__global__ __launch_bounds__(256) void margin_wgrad_fix_kernel(float* __restrict__ dw, const float* __restrict__ w, const float* __restrict__ rnorm,
                                                               acc_t* __restrict__ tacc, int C, int E) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= C) return;
    float tf = 0.f;
    if (lane == 0) {
        tf = acc_get<ACC_GRAD>(tacc[j]);
        tacc[j] = 0;
    }
    tf = __shfl(tf, 0);
    const float r = rnorm[j];
    const float kf = (r * r) * tf;
    const float* wr = w + (long)j * E;
    float* dr = dw + (long)j * E;
    for (int e = 4 * lane; e < E; e += 256) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + e);
        f32x4 dv = *reinterpret_cast<const f32x4*>(dr + e);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float p = kf * wv[t];
            dv[t] = dv[t] - p;
        }
        *reinterpret_cast<f32x4*>(dr + e) = dv;
    }
}
}  // namespace fn
using namespace fn;

extern "C" int fn_pairwise_sqdist(const float* xa, const float* xb, float* out, float* range, int n, int m, int E, int metric, void* stream) {
    FN_REQUIRE(xa && xb && out && n > 0 && m > 0 && E > 0 && E <= 512, "pairwise_sqdist: bad arguments (E must be <= 512)");
    FN_REQUIRE(metric >= 0 && metric <= 2, "Undefined similarity metric %d", metric);  // statistics.py:55
    hipStream_t st = (hipStream_t)stream;
    if (range) {
        fill_words(range, 0x7f7fffffu, 0x80800000u, 2, st);   // ord(+FLT_MAX), ord(-FLT_MAX); a kernel node, see fill_words
    }
    hipLaunchKernelGGL(pairwise_kernel, dim3(cdiv(m, 64), n), dim3(256), 0, st, xa, xb, out, (int*)range, n, m, E, metric);
    return check_launch("pairwise_sqdist");
}

extern "C" int fn_select_triplets(const float* dist, const int32_t* labels, int n, float alpha, int nrof_triplets, uint32_t seed,
                                  int semi_hard, int32_t* triplets, int32_t* info, void* stream) {
    FN_REQUIRE(dist && labels && triplets && info && n > 1 && n <= 1024 && nrof_triplets > 0, "select_triplets: bad arguments (n <= 1024)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(select_pairs_kernel, dim3(1), dim3(1024), 0, st, labels, n, info);
    const int max_pairs = n * (n - 1) / 2;      // upper bound; waves beyond info[0] leave at once
    hipLaunchKernelGGL(select_negatives_kernel, dim3(cdiv(max_pairs, 4)), dim3(256), 0, st, dist, labels, n, alpha, seed, semi_hard, info);
    hipLaunchKernelGGL(select_rank_kernel, dim3(1), dim3(1024), 0, st, nrof_triplets, triplets, info);
    return check_launch("select_triplets");
}

extern "C" int fn_triplet_loss_fwd_bwd(const float* emb, float* demb, float* loss, int T, int E, float alpha, void* stream) {
    FN_REQUIRE(emb && loss && T > 0 && E > 0, "triplet_loss: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    FN_REQUIRE(((uintptr_t)loss & 7) == 0, "triplet_loss: loss must be an 8-byte aligned fp32[4]");
    fill_words(loss, 0u, 0u, 4, st);
    hipLaunchKernelGGL(triplet_loss_kernel, dim3(cdiv(T, 4)), dim3(256), 0, st, emb, demb, reinterpret_cast<acc_t*>(loss + 2), T, E, alpha);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, st, loss);
    return check_launch("triplet_loss");
}

extern "C" int fn_softmax_xent_fwd_bwd(const float* logits, int ld, const int32_t* labels, float* loss, void* dlogits_lp, int ld_d, fn_acc_t* dbias_,
                                       int N, int C, float grad_scale, int dtype, void* stream) {
    acc_t* dbias = reinterpret_cast<acc_t*>(dbias_);
    FN_REQUIRE(((uintptr_t)loss & 7) == 0, "softmax_xent: loss must be an 8-byte aligned fp32[4]");
    FN_REQUIRE(dtype == FN_BF16 || dtype == FN_F16, "dtype %d unsupported", dtype);
    FN_REQUIRE(logits && labels && loss && N > 0 && C > 0 && ld >= C && (!dlogits_lp || ld_d >= C), "softmax_xent: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    fill_words(loss, 0u, 0u, 4, st);
    acc_t* lacc = reinterpret_cast<acc_t*>(loss + 2);
    if (dtype == FN_BF16)
        hipLaunchKernelGGL(softmax_xent_kernel<__bf16>, dim3(N), dim3(256), 0, st, logits, ld, labels, lacc, (unsigned short*)dlogits_lp, ld_d, dbias, N, C, grad_scale);
    else
        hipLaunchKernelGGL(softmax_xent_kernel<_Float16>, dim3(N), dim3(256), 0, st, logits, ld, labels, lacc, (unsigned short*)dlogits_lp, ld_d, dbias, N, C, grad_scale);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, st, loss);
    return check_launch("softmax_xent");
}

extern "C" int fn_center_loss_fwd_bwd(const float* x, const int32_t* labels, const float* centers, float* demb, float* terms, float* xy,
                                      int ld_xy, int N, int E, int C, float center_factor, float norm_factor, float p, void* stream) {
    FN_REQUIRE(x && labels && terms && N > 0 && E > 0 && E % 4 == 0, "center_loss: bad arguments (E must be a multiple of 4)");
    FN_REQUIRE(((uintptr_t)x & 15) == 0 && (!demb || ((uintptr_t)demb & 15) == 0) && (!centers || ((uintptr_t)centers & 15) == 0),
               "center_loss: x, demb and centers must be 16-byte aligned");
    FN_REQUIRE(((uintptr_t)terms & 7) == 0, "center_loss: terms must be an 8-byte aligned fp32[8]");
    FN_REQUIRE(!centers || C > 0, "center_loss: centers need C > 0");
    FN_REQUIRE(!xy || ld_xy > E, "center_loss: ld_xy must be > E");
    FN_REQUIRE(center_factor >= 0.f && norm_factor >= 0.f && p > 0.f, "center_loss: factors must be >= 0 and p > 0");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(center_loss_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, x, labels, centers, demb, terms, xy, ld_xy, N, E, C,
                       center_factor, norm_factor, p);
    hipLaunchKernelGGL(center_loss_finish_kernel, dim3(1), dim3(1), 0, st, terms);
    return check_launch("center_loss");
}

extern "C" int fn_center_update(const float* rows, int ld, int M, int E, float* centers, int C, double alfa, void* stream) {
    FN_REQUIRE(rows && centers && M > 0 && M <= 4096 && E > 0 && ld > E && C > 0, "center_update: bad arguments (M <= 4096, ld > E)");
    FN_REQUIRE(alfa >= 0.0 && alfa <= 1.0, "center_update: alfa must be in [0, 1]");
    const float k = (float)(1.0 - alfa);      // (1 - alfa) of facenet.py:213: a Python float, rounded to fp32 once
    hipLaunchKernelGGL(center_update_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, rows, ld, M, E, centers, C, k);
    return check_launch("center_update");
}

extern "C" int fn_margin_weight_rnorm(const float* w, int C, int E, float eps, float* rnorm, void* stream) {
    FN_REQUIRE(w && rnorm && C > 0 && E > 0 && E % 4 == 0 && eps > 0.f, "margin_weight_rnorm: bad arguments (E must be a multiple of 4, eps > 0)");
    FN_REQUIRE(((uintptr_t)w & 15) == 0, "margin_weight_rnorm: w must be 16-byte aligned");
    hipLaunchKernelGGL(margin_rnorm_kernel, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, w, C, E, eps, rnorm);
    return check_launch("margin_weight_rnorm");
}

extern "C" int fn_margin_softmax_fwd_bwd(const float* z, int ld, const float* rnorm, const int32_t* labels, float* loss, void* dz_lp, int ld_d,
                                         fn_acc_t* t, int N, int C, float scale, float m_arc, float m_cos, float grad_scale, int dtype,
                                         void* stream) {
    FN_REQUIRE(((uintptr_t)loss & 7) == 0, "margin_softmax: loss must be an 8-byte aligned fp32[4]");
    FN_REQUIRE(dtype == FN_BF16 || dtype == FN_F16, "dtype %d unsupported", dtype);
    FN_REQUIRE(z && rnorm && labels && loss && N > 0 && C > 0 && ld >= C && (!dz_lp || ld_d >= C), "margin_softmax: bad arguments");
    const double pi = 3.14159265358979323846, m = (double)m_arc;
    // (written so that a NaN setting is refused too)
    FN_REQUIRE(scale > 0.f && m_arc >= 0.f && m < 0.5 * pi && m_cos >= 0.f,
               "margin_softmax: need scale > 0, 0 <= m_arc < pi/2, m_cos >= 0 (got %g, %g, %g)", (double)scale, m, (double)m_cos);
    const MarginConsts k = {scale, (float)cos(m), (float)sin(m), (float)cos(pi - m), (float)(sin(pi - m) * m), m_cos};
    hipStream_t st = (hipStream_t)stream;
    fill_words(loss, 0u, 0u, 4, st);
    acc_t* lacc = reinterpret_cast<acc_t*>(loss + 2);
    acc_t* tacc = reinterpret_cast<acc_t*>(t);
    if (dtype == FN_BF16)
        hipLaunchKernelGGL(margin_softmax_kernel<__bf16>, dim3(N), dim3(256), 0, st, z, ld, rnorm, labels, lacc, (unsigned short*)dz_lp, ld_d, tacc, N, C, k, grad_scale);
    else
        hipLaunchKernelGGL(margin_softmax_kernel<_Float16>, dim3(N), dim3(256), 0, st, z, ld, rnorm, labels, lacc, (unsigned short*)dz_lp, ld_d, tacc, N, C, k, grad_scale);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, st, loss);
    return check_launch("margin_softmax");
}

extern "C" int fn_margin_wgrad_fix(float* dw, const float* w, const float* rnorm, fn_acc_t* t, int C, int E, void* stream) {
    FN_REQUIRE(dw && w && rnorm && t && C > 0 && E > 0 && E % 4 == 0, "margin_wgrad_fix: bad arguments (E must be a multiple of 4)");
    FN_REQUIRE(((uintptr_t)dw & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)t & 7) == 0, "margin_wgrad_fix: dw and w must be 16-byte aligned, t 8-byte");
    hipLaunchKernelGGL(margin_wgrad_fix_kernel, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, dw, w, rnorm, reinterpret_cast<acc_t*>(t), C, E);
    return check_launch("margin_wgrad_fix");
}
